// rt_context.cpp — the context of the C ABI (include/rt_abi.h): create and
// destroy, scene and camera setters, controls, shard state, errors.
//
// Host-side replacement of the reference's render driver (Main.cu:38-109
// allocateScene, :317-366 render, :401-496 main's state handling): the
// context owns the device copy of the (compiled) scene, the per-pixel RNG
// state and frameSum accumulator of one pixel-row shard, a HIP stream and the
// events of its passes (rt_context.h).
//
// Compiled with -ffp-contract=off, as rt_scene.cpp and rt_render.cpp: the
// host-side scene compilation and the camera prelude (Main.cu:336-338) use
// the reference's float operations in the reference's order, so the kernel
// sees bit-identical inputs.
#include <sched.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <thread>

#include "rt_context.h"

static_assert(sizeof(rt_vec3) == 12, "vec3d layout (Math.cuh:35-39)");
static_assert(sizeof(rt_material) == 24, "material layout (WorldTypes.cuh:15-20)");
static_assert(sizeof(rt_sphere) == 40 && offsetof(rt_sphere, mat) == 16, "sphere layout");
static_assert(sizeof(rt_plane) == 60 && offsetof(rt_plane, mat) == 36, "plane layout");
static_assert(sizeof(rt_triangle) == 60 && offsetof(rt_triangle, mat) == 36, "triangle layout");
static_assert(sizeof(rt_quad) == 72 && offsetof(rt_quad, mat) == 48, "quad layout");
static_assert(sizeof(rt_camera) == 24, "camera layout (WorldTypes.cuh:9-13)");
static_assert(sizeof(rt_scene) == 88 && offsetof(rt_scene, spheres) == 24 &&
                  offsetof(rt_scene, sphere_count) == 32 && offsetof(rt_scene, planes) == 40 &&
                  offsetof(rt_scene, triangles) == 56 && offsetof(rt_scene, quads) == 72 &&
                  offsetof(rt_scene, quad_count) == 80,
              "scene layout (WorldTypes.cuh:44-53)");

const char* tuning_env(const char* name) {
    const char* t = std::getenv("BWRT_TUNING");
    return t && std::strcmp(t, "1") == 0 ? std::getenv(name) : nullptr;
}

int fail(rt_context* c, int code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

int hip_fail(rt_context* c, hipError_t e, const char* what) {
    return fail(c, e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP, "%s: %s", what,
                hipGetErrorString(e));
}

// Host-side writes of context state (scene, RNG seeds, frameSum, checkpoint
// restore) and buffer reallocation must not overlap a render still running
// on a caller's stream (rt_render_device), nor a denoise or a reprojection
// pass still reading frameSum: wait for the last of each (its event,
// recorded on whatever stream it ran on).  Work on c->stream is already
// ordered by the stream itself.
int quiesce(rt_context* c) {
    if (c->cpu) return RT_OK;
    HIP_TRY(c, c->render.flush());
    for (Pass* p : {&c->denoise, &c->temporal, &c->denoise_var, &c->temporal_var, &c->xport, &c->assemble, &c->render})
        HIP_TRY(c, p->sync());
    return RT_OK;
}

// The last render (and the passes behind it), on whatever stream it ran,
// then blocking copies
int read_settled(rt_context* c, std::initializer_list<HostCopy> copies) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (const int rc = quiesce(c)) return rc;
    for (const HostCopy& h : copies)
        if (h.dst) HIP_TRY(c, hipMemcpy(h.dst, h.src, h.bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Renders continue each other's RNG / frameSum state, the denoiser and the
// reprojection read frameSum and share the guides and colour buffers, an
// export reads frameSum and the moments, an assembly writes the frame the
// full-frame passes read: work of any of them on stream s waits for the last
// of each that ran on another stream (no host sync)
int order_after_all(rt_context* c, hipStream_t s) {
    for (Pass* p : {&c->render, &c->denoise, &c->temporal, &c->denoise_var, &c->temporal_var, &c->xport, &c->assemble})
        HIP_TRY(c, p->wait_on(s));
    return RT_OK;
}

int ensure_buf(rt_context* c, Buf& b, size_t bytes, const char* host_oom, size_t n) {
    if (b.bytes >= bytes && b.p) return RT_OK;
    if (b.p && !c->cpu) {  // the old buffer may still be in use by queued work
        int rc = quiesce(c);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    b.release();
    if (bytes == 0) return RT_OK;
    if (c->cpu) {
        if (!(b.p = std::calloc(bytes, 1))) return fail(c, RT_ERR_OUT_OF_MEMORY, host_oom, n);
        b.host = true;
    } else {
        HIP_TRY(c, hipMalloc(&b.p, bytes));
    }
    b.bytes = bytes;
    return RT_OK;
}

int shard_rows(int height, int row_offset, int row_stride) {
    if (height <= 0 || row_offset < 0 || row_stride <= 0 || row_offset >= height) return 0;
    return (height - row_offset + row_stride - 1) / row_stride;
}

int shard_check(rt_context* c, int width, int height, int row_offset, int row_stride) {
    if (width <= 0 || height <= 0 || row_offset < 0 || row_stride < 0 || row_offset >= height)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "bad shard %dx%d offset %d stride %d", width, height,
                    row_offset, row_stride);
    if ((long long)width * height > (1ll << 31))
        return fail(c, RT_ERR_UNSUPPORTED, "image larger than 2^31 pixels");
    return RT_OK;
}

extern "C" {

const char* rt_version(void) { return "0.3.0"; }

rt_material rt_material_default(void) {
    rt_material m;
    m.albedo = {0.0f, 0.0f, 0.0f};
    m.emittance = 0.0f;
    m.roughness = 1.0f;
    m.refractive_index = 1.05f;  // WorldTypes.cuh:19 (double 1.05 -> float)
    return m;
}

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_create(int device, rt_context** out) {
    if (!out) return RT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RT_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return RT_ERR_INVALID_ARGUMENT;
    rt_context* c = new rt_context();
    c->device = device;
    // the context's stream at the device's highest priority: its render
    // workgroups dispatch ahead of other streams' work, e.g. the multi-GPU
    // gather and de-interleave of the previous frame that overlap the next
    // render (world size 1, ms per step: 0.761-0.765 vs 0.780-0.785 at
    // normal priority, single-GPU renders unchanged; profiles/r06e/);
    // BWRT_STREAM_PRIO=0: normal priority
    int prio_lo = 0, prio_hi = 0;
    const char* sp = tuning_env("BWRT_STREAM_PRIO");
    const bool high = !(sp && std::atoi(sp) == 0) && hipSetDevice(device) == hipSuccess &&
                      hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess;
    if (hipSetDevice(device) != hipSuccess ||
        (high ? hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi)
              : hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        c->render.create(true) != hipSuccess || c->aux.create(false) != hipSuccess ||
        c->denoise.create(true) != hipSuccess) {
        rt_destroy(c);
        return RT_ERR_HIP;
    }
    c->render.home = c->stream;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->num_cus = prop.multiProcessorCount;
    if (const char* gm = tuning_env("BWRT_GRID_MULT")) c->grid_mult = std::atoi(gm);
    if (const char* db = tuning_env("BWRT_DEINT_BLOCKS")) c->deint_blocks = std::max(std::atoi(db), 0);
    if (const char* kk = tuning_env("BWRT_KERNEL")) c->simple = std::strcmp(kk, "simple") == 0;
    if (const char* bk = tuning_env("BWRT_BLOCK")) c->block = std::atoi(bk);
    if (const char* tw = tuning_env("BWRT_TILE")) {
        const int t = std::atoi(tw);
        if (t >= 0 && t <= 64 && (t & (t - 1)) == 0) c->tile_w = t;
    }
    if (const char* g = tuning_env("BWRT_TILE_SQ")) c->tile_sq = std::atoi(g) != 0;
    if (const char* g = tuning_env("BWRT_GREC")) c->grec = std::atoi(g) ? 1 : 0;
    if (const char* g = tuning_env("BWRT_LEAF_BATCH")) c->leaf_batch = std::min(std::max(std::atoi(g), 1), 64);
    if (const char* g = tuning_env("BWRT_REFILL")) c->refill = std::min(std::max(std::atoi(g), 1), 64);
    if (const char* g = tuning_env("BWRT_SPREAD")) c->spread = std::atoi(g) ? 1 : 0;
    if (const char* g = tuning_env("BWRT_ORDER")) c->order_feedback = std::atoi(g) != 0;
    if (const char* g = tuning_env("BWRT_SKY")) {
        c->sky_on = std::atoi(g) != 0;
        c->sky_eager = std::atoi(g) == 2;
    }
    if (const char* g = tuning_env("BWRT_ORDER_PERIOD")) c->order_period = std::max(std::atoi(g), 1);
    if (const char* g = tuning_env("BWRT_DENOISE_KERNEL"))
        c->dn_kernel = std::strcmp(g, "tiled") == 0 ? 1 : std::strcmp(g, "direct") == 0 ? 0 : -1;
    if (const char* g = tuning_env("BWRT_ADAPTIVE_KERNEL"))
        c->ad_kernel = std::strcmp(g, "simple") == 0 ? 1 : std::strcmp(g, "queued") == 0 ? 2 : 0;
    if (const char* g = tuning_env("BWRT_PRECISION"))
        c->precision = std::strcmp(g, "fast") == 0 ? RT_PRECISION_REFERENCE_FAST : RT_PRECISION_EXACT;
    *out = c;
    return RT_OK;
}

int rt_create_cpu(int threads, rt_context** out) {
    if (!out) return RT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (threads < 0) return RT_ERR_INVALID_ARGUMENT;
    // rt_cpu.cpp is built for x86-64-v3 (hardware fma for the exactly
    // specified fma steps of rt_path.h)
    if (!rt_cpu_supported()) return RT_ERR_UNSUPPORTED;
    rt_context* c = new rt_context();
    c->cpu = true;
    c->render.host = c->denoise.host = c->temporal.host = c->denoise_var.host = c->temporal_var.host = true;
    c->xport.host = c->assemble.host = true;
    c->device = -1;
    c->threads = threads > 0 ? threads : rt_cpu_threads();
    *out = c;
    return RT_OK;
}

int rt_cpu_threads(void) {
    // the CPUs this process may run on (sched affinity), not the machine's,
    // capped by a cgroup v2 CPU quota (cpu.max "quota period", rounded up):
    // a container may see every CPU of the host but be granted a share
    int n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    if (n <= 0) n = 1;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[32] = {0};
        long period = 0;
        if (std::fscanf(f, "%31s %ld", quota, &period) == 2 && std::strcmp(quota, "max") != 0 && period > 0) {
            const long q = std::atol(quota);
            const int share = (int)((q + period - 1) / period);
            if (share > 0 && share < n) n = share;
        }
        std::fclose(f);
    }
    return n;
}

void rt_destroy(rt_context* c) {
    if (!c) return;
    if (!c->cpu) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        c->render.pending = false;  // its launch is done: the stream is synchronised
        for (Pass* p : {&c->render, &c->aux, &c->denoise, &c->temporal, &c->denoise_var, &c->temporal_var, &c->xport, &c->assemble}) {
            (void)p->sync();
            p->destroy();
        }
        if (c->host_rgba) (void)hipHostFree(c->host_rgba);
        for (hipEvent_t e : c->ad_ev)
            if (e) (void)hipEventDestroy(e);
        if (c->sky_ev) {
            (void)hipEventSynchronize(c->sky_ev);
            (void)hipEventDestroy(c->sky_ev);
        }
        if (c->stream) (void)hipStreamDestroy(c->stream);
    }
    delete c;  // every Buf frees itself
}

int rt_set_scene(rt_context* c, const rt_scene* s) {
    const HostFpEnv fp;
    if (!c || !s) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (s->sphere_count < 0 || s->plane_count < 0 || s->triangle_count < 0 || s->quad_count < 0)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "negative primitive count");
    if ((s->sphere_count && !s->spheres) || (s->plane_count && !s->planes) ||
        (s->triangle_count && !s->triangles) || (s->quad_count && !s->quads))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "null primitive array with non-zero count");
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
    rt_scene_options opt;
    for (const char* name : rt_scene_option_names)
        if (const char* v = tuning_env(name)) rt_scene_option_set(opt, name, v);
    rt_compiled_scene cs;
    std::string err;
    if (const int rc = rt_compile_scene(*s, opt, cs, err)) return fail(c, rc, "%s", err.c_str());
    // nothing of the context has changed so far, and the compiled scene
    // replaces the old one only once the buffer holds it
    const size_t bytes = cs.data.size() * sizeof(float);
    int rc = quiesce(c);  // a render on a caller's stream may still read the scene
    if (!rc) rc = ensure_buf(c, c->scene_buf, bytes, "host scene of %zu bytes", bytes);
    // the light table: every record, then the polygon lights' sampling blocks
    std::vector<float> ltab(cs.lights);
    ltab.insert(ltab.end(), cs.light_polys.begin(), cs.light_polys.end());
    // and the two light trees (rt_set_light_hierarchy; rt_context::table_args has the offsets)
    ltab.insert(ltab.end(), cs.light_tree_spheres.begin(), cs.light_tree_spheres.end());
    ltab.insert(ltab.end(), cs.light_tree_all.begin(), cs.light_tree_all.end());
    const size_t lbytes = ltab.size() * sizeof(float);
    if (!rc && lbytes) rc = ensure_buf(c, c->light_buf, lbytes, "host light table of %zu bytes", lbytes);
    if (rc) {
        if (!c->scene_buf.p) c->has_scene = false;  // the old buffer went in the attempt to grow it
        return rc;
    }
    if (c->cpu) {
        std::memcpy(c->scene_buf.p, cs.data.data(), bytes);
        if (lbytes) std::memcpy(c->light_buf.p, ltab.data(), lbytes);
    } else {
        HIP_TRY(c, hipMemcpyAsync(c->scene_buf.p, cs.data.data(), bytes, hipMemcpyHostToDevice, c->stream));
        if (lbytes) HIP_TRY(c, hipMemcpyAsync(c->light_buf.p, ltab.data(), lbytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    rt_sky_collect(*s, cs, c->sky_prims);
    std::vector<float>().swap(cs.data);
    c->scene = std::move(cs);
    c->camera = s->camera;
    c->has_scene = true;
    c->view_changed();
    c->st.end_nonuniform();  // a non-uniform accumulation ends with its scene
    c->vs.drop_history();  // primitive ids change meaning
    return RT_OK;
}

int rt_set_camera(rt_context* c, const rt_camera* cam) {
    if (!c || !cam) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    c->camera = *cam;
    c->view_changed();
    return RT_OK;
}

int rt_set_background(rt_context* c, float r, float g, float b) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    c->background[0] = r;
    c->background[1] = g;
    c->background[2] = b;
    return RT_OK;
}

// Only the choice of kernels at the next launch: the shard state (RNG
// streams, frameSum, frame counter) is shared by both modes and stays
int rt_set_precision(rt_context* c, int precision) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (precision != RT_PRECISION_EXACT && precision != RT_PRECISION_REFERENCE_FAST)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_set_precision: unknown precision %d", precision);
    if (c->cpu && precision != RT_PRECISION_EXACT)
        return fail(c, RT_ERR_UNSUPPORTED,
                    "rt_set_precision: RT_PRECISION_REFERENCE_FAST is not supported on a CPU context "
                    "(the CPU fallback is bit-identical to the exact kernels)");
    c->precision = precision;
    return RT_OK;
}

int rt_get_precision(const rt_context* c) { return c ? c->precision : RT_PRECISION_EXACT; }

// Only the choice of estimator at the next render: accumulation, frame counter
// and RNG streams stay, as with rt_set_background
int rt_set_light_sampling(rt_context* c, int on) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (on != 0 && on != 1) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_set_light_sampling: %d is neither 0 nor 1", on);
    c->light_sampling = on != 0;
    return RT_OK;
}

int rt_get_light_sampling(const rt_context* c) { return c && c->light_sampling ? 1 : 0; }

// Likewise only a choice at the next render, and only where light sampling acts
// (rt_context::nee_args)
int rt_set_light_picking(rt_context* c, int mode) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_LIGHT_PICK_UNIFORM && mode != RT_LIGHT_PICK_WEIGHTED)
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_set_light_picking: %d is neither RT_LIGHT_PICK_UNIFORM nor RT_LIGHT_PICK_WEIGHTED", mode);
    c->light_picking = mode;
    return RT_OK;
}

int rt_get_light_picking(const rt_context* c) { return c ? c->light_picking : RT_LIGHT_PICK_UNIFORM; }

// Likewise: how many records of the scene's table a render sees
int rt_set_light_shapes(rt_context* c, int mode) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_LIGHT_SHAPES_SPHERES && mode != RT_LIGHT_SHAPES_ALL)
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_set_light_shapes: %d is neither RT_LIGHT_SHAPES_SPHERES nor RT_LIGHT_SHAPES_ALL", mode);
    c->light_shapes = mode;
    return RT_OK;
}

int rt_get_light_shapes(const rt_context* c) { return c ? c->light_shapes : RT_LIGHT_SHAPES_SPHERES; }

int rt_get_lights(rt_context* c, float* out, int capacity) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (capacity < 0 || (capacity > 0 && !out)) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_get_lights: bad capacity / null out");
    const int n = c->n_lights();
    const int k = n < capacity ? n : capacity;
    if (k > 0) std::memcpy(out, c->scene.lights.data(), (size_t)k * RT_LIGHT_FLOATS * sizeof(float));
    return n;
}

// Likewise: whether the weighted pick descends the light tree (rt_context::table_args)
int rt_set_light_hierarchy(rt_context* c, int on) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (on != 0 && on != 1) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_set_light_hierarchy: %d is neither 0 nor 1", on);
    c->light_hierarchy = on != 0;
    return RT_OK;
}

int rt_get_light_hierarchy(const rt_context* c) { return c && c->light_hierarchy ? 1 : 0; }

int rt_get_light_tree(rt_context* c, float* out, int capacity) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (capacity < 0 || (capacity > 0 && !out)) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_get_light_tree: bad capacity / null out");
    const std::vector<float>& t = c->light_tree();
    const int n = (int)(t.size() / RT_LIGHT_NODE_FLOATS);
    const int k = n < capacity ? n : capacity;
    if (k > 0) std::memcpy(out, t.data(), (size_t)k * RT_LIGHT_NODE_FLOATS * sizeof(float));
    return n;
}

// An introspection call: its device buffers live for the call (a local Buf
// frees itself), the light table is only read
int rt_light_pick_probabilities(rt_context* c, const float* points, const int* prims, int count, float* out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (count < 0 || (count > 0 && (!points || !prims || !out)))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_light_pick_probabilities: bad count / null array");
    const int n = c->n_lights();
    if (n == 0 || count == 0) return n;
    const rt_nee_args N = c->table_args(n);
    if (c->cpu) {
        rt_cpu_pick_probabilities(N, c->scene.n_sph, points, prims, count, out, c->threads);
        return n;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t pb = (size_t)count * 6 * sizeof(float), ib = (size_t)count * sizeof(int), ob = (size_t)count * n * sizeof(float);
    Buf dp, di, dout;
    HIP_TRY(c, hipMalloc(&dp.p, pb));
    HIP_TRY(c, hipMalloc(&di.p, ib));
    HIP_TRY(c, hipMalloc(&dout.p, ob));
    HIP_TRY(c, hipMemcpyAsync(dp.p, points, pb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(di.p, prims, ib, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, rt_launch_pick_probabilities(N, c->scene.n_sph, dp.as<const float>(), di.as<const int>(), count, dout.as<float>(), c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, dout.p, ob, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return n;
}

int rt_get_camera(const rt_context* c, rt_camera* cam) {
    if (!c || !cam) return RT_ERR_INVALID_ARGUMENT;
    *cam = c->camera;
    return RT_OK;
}

// Controls.cuh:5-75 in the reference's float operation order: the direction
// vectors are rotY * rotX (matrix product, Math.cuh:191-199) times a basis
// vector (mat * vec = row dots, Math.cuh:144-150); position +/-= k * dir.
int rt_apply_controls(rt_camera* cam, unsigned keys, float dt) {
    if (!cam) return RT_ERR_INVALID_ARGUMENT;
    const HostFpEnv fp;
    struct V3 {
        float x, y, z;
    };
    const float move = 5 * dt;
    const float rot = 2 * dt;
    const float cy = cosf(cam->angle[0]), sy = sinf(cam->angle[0]);  // rotationMatrix3DY
    const float cx = cosf(cam->angle[1]), sx = sinf(cam->angle[1]);  // rotationMatrix3DX
    const float L[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}};
    const float U[3][3] = {{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}};
    float M[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i][j] = L[i][0] * U[0][j] + L[i][1] * U[1][j] + L[i][2] * U[2][j];
    auto mul = [&](float x, float y, float z) {
        return V3{M[0][0] * x + M[0][1] * y + M[0][2] * z, M[1][0] * x + M[1][1] * y + M[1][2] * z,
                  M[2][0] * x + M[2][1] * y + M[2][2] * z};
    };
    const V3 front = mul(0, 0, -1), right = mul(1, 0, 0);
    rt_vec3& p = cam->position;
    int flags = 0;
    auto add = [&](float k, V3 v, float sign) {  // position (+|-)= k * v
        const V3 kv{k * v.x, k * v.y, k * v.z};
        if (sign > 0) {
            p.x = p.x + kv.x;
            p.y = p.y + kv.y;
            p.z = p.z + kv.z;
        } else {
            p.x = p.x - kv.x;
            p.y = p.y - kv.y;
            p.z = p.z - kv.z;
        }
        flags |= RT_CONTROLS_MOVED;
    };
    if (keys & RT_KEY_W) add(move, front, +1);
    if (keys & RT_KEY_A) add(move, right, -1);
    if (keys & RT_KEY_S) add(move, front, -1);
    if (keys & RT_KEY_D) add(move, right, +1);
    if (keys & RT_KEY_SPACE) {
        p.y += move;
        flags |= RT_CONTROLS_MOVED;
    }
    if (keys & RT_KEY_LEFT_SHIFT) {
        p.y -= move;
        flags |= RT_CONTROLS_MOVED;
    }
    if (keys & RT_KEY_LEFT) {
        cam->angle[0] += rot;
        flags |= RT_CONTROLS_MOVED;
    }
    if (keys & RT_KEY_RIGHT) {
        cam->angle[0] -= rot;
        flags |= RT_CONTROLS_MOVED;
    }
    if (keys & RT_KEY_UP) {
        cam->angle[1] += rot;
        flags |= RT_CONTROLS_MOVED;
    }
    if (keys & RT_KEY_DOWN) {
        cam->angle[1] -= rot;
        flags |= RT_CONTROLS_MOVED;
    }
    if (keys & RT_KEY_ESCAPE) flags |= RT_CONTROLS_QUIT;
    return flags;
}

int rt_controls(rt_context* c, unsigned keys, float dt) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const int flags = rt_apply_controls(&c->camera, keys, dt);
    if (flags > 0 && (flags & RT_CONTROLS_MOVED)) c->view_changed();
    return flags;
}

int rt_reset_accumulation(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    c->st.restart();
    return RT_OK;
}

unsigned rt_frame_counter(const rt_context* c) { return c ? c->st.frame() : 0u; }

int rt_set_max_bounces(rt_context* c, int mb) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (mb < 0) return fail(c, RT_ERR_INVALID_ARGUMENT, "max_bounces < 0");
    if (mb > RT_MAX_BOUNCES) return fail(c, RT_ERR_UNSUPPORTED, "max_bounces > %d", RT_MAX_BOUNCES);
    c->max_bounces = mb;
    return RT_OK;
}

int rt_set_samples_per_pixel(rt_context* c, int n) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (n < 1) return fail(c, RT_ERR_INVALID_ARGUMENT, "samples per pixel < 1");
    if (n > RT_MAX_SAMPLES_PER_PIXEL)
        return fail(c, RT_ERR_UNSUPPORTED, "samples per pixel > %d", RT_MAX_SAMPLES_PER_PIXEL);
    c->spp_inner = n;
    return RT_OK;
}

int rt_set_kernel_timing(rt_context* c, int enable) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    c->ktiming = enable != 0;
    if (!c->ktiming) c->render.timed = false;  // no stale duration from an earlier launch
    return RT_OK;
}

// Opt-in: the post-render passes on a non-uniform accumulation (rt_post.cpp
// full_frame_check reads it; it has no other effect)
int rt_set_adaptive_filters(rt_context* c, int enable) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    c->st.set_filters(enable != 0);
    return RT_OK;
}

int rt_get_adaptive_filters(const rt_context* c) { return c && c->st.filters() ? 1 : 0; }

int rt_shard_rows(int height, int row_offset, int row_stride) {
    return shard_rows(height, row_offset, row_stride == 0 ? 1 : row_stride);
}

int rt_init_rand(rt_context* c, int width, int height, int row_offset, int row_stride) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (row_stride == 0) row_stride = 1;
    if (const int rc = shard_check(c, width, height, row_offset, row_stride)) return rc;
    const int rows = shard_rows(height, row_offset, row_stride);
    const size_t npix = (size_t)rows * width;
    c->new_view();  // the guides are those of one frame shape
    c->st.end_tracking();  // the moments are those of one shard
    c->vs.set_shape(width, height);  // the history sets are those of one frame shape
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
    int rc = quiesce(c);  // a render on a caller's stream may still use the state
    const char* oom = "host state for %zu pixels";
    if (!rc) rc = ensure_buf(c, c->rng, npix * 6 * sizeof(unsigned), oom, npix);
    if (!rc) rc = ensure_buf(c, c->accum, npix * 3 * sizeof(float), oom, npix);
    if (!rc && c->cpu) rc = ensure_buf(c, c->rgba, npix * 4, oom, npix);  // (a GPU context's: at the first render)
    if (rc) return rc;
    if (c->cpu) {
        std::memset(c->rng.p, 0, npix * 6 * sizeof(unsigned));
        std::memset(c->accum.p, 0, npix * 3 * sizeof(float));
        std::memset(c->rgba.p, 0, npix * 4);
        rt_cpu_init_rand(c->rng.as<unsigned>(), width, rows, row_offset, row_stride);
    } else {
        HIP_TRY(c, hipMemsetAsync(c->accum.p, 0, npix * 3 * sizeof(float), c->stream));
        HIP_TRY(c, rt_launch_init_rand(c->rng.as<unsigned>(), width, rows, row_offset, row_stride, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->width = width;
    c->height = height;
    c->row_offset = row_offset;
    c->row_stride = row_stride;
    c->rows = rows;
    c->st.restart();
    c->order_stale = true;
    return RT_OK;
}

int rt_synchronize(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (c->cpu) return RT_OK;  // CPU renders are synchronous
    HIP_TRY(c, hipSetDevice(c->device));
    // record a deferred end event first, so the render pass's event always
    // marks the last render (later renders on a caller's stream wait on it)
    HIP_TRY(c, c->render.flush());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (Pass* p : {&c->render, &c->aux, &c->denoise, &c->temporal, &c->denoise_var, &c->temporal_var, &c->xport, &c->assemble})
        HIP_TRY(c, p->sync());
    return RT_OK;
}

void* rt_get_stream(rt_context* c) { return c && !c->cpu ? (void*)c->stream : nullptr; }

float rt_last_kernel_ms(rt_context* c) { return c ? c->render.elapsed_ms() : -1.0f; }

int rt_get_state(rt_context* c, uint32_t* rng, float* accum) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const size_t npix = (size_t)c->rows * c->width;
    if (!c->rng.p) return fail(c, RT_ERR_INVALID_ARGUMENT, "no shard state (render or rt_init_rand first)");
    if (c->cpu) {  // (no HIP call on a CPU context: the machine may have no GPU)
        if (rng) std::memcpy(rng, c->rng.p, npix * 6 * sizeof(unsigned));
        if (accum) planes_to_rgb(c->accum.as<float>(), npix, accum);
        return RT_OK;
    }
    std::vector<float> planes;
    if (accum && !try_resize(planes, npix * 3)) return fail(c, RT_ERR_OUT_OF_MEMORY, "host state for %zu pixels", npix);
    const int rc = read_settled(c, {{rng, c->rng.p, npix * 6 * sizeof(unsigned)},
                                    {accum ? planes.data() : nullptr, c->accum.p, npix * 3 * sizeof(float)}});
    if (rc) return rc;
    if (accum) planes_to_rgb(planes.data(), npix, accum);
    return RT_OK;
}

int rt_set_state(rt_context* c, const uint32_t* rng, const float* accum, unsigned frame_counter) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->rng.p) return fail(c, RT_ERR_INVALID_ARGUMENT, "no shard state (rt_init_rand first)");
    if (frame_counter == 0) return fail(c, RT_ERR_INVALID_ARGUMENT, "frame_counter must be >= 1");
    const size_t npix = (size_t)c->rows * c->width;
    if (c->cpu) {
        if (rng) std::memcpy(c->rng.p, rng, npix * 6 * sizeof(unsigned));
        if (accum) rgb_to_planes(accum, npix, c->accum.as<float>());
        c->st.set_frame(frame_counter);
        return RT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = quiesce(c);  // a render on a caller's stream may still use the state
    if (rc) return rc;
    std::vector<float> planes;
    if (rng)
        HIP_TRY(c, hipMemcpyAsync(c->rng.p, rng, npix * 6 * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    if (accum) {
        planes.resize(npix * 3);
        rgb_to_planes(accum, npix, planes.data());
        HIP_TRY(c, hipMemcpyAsync(c->accum.p, planes.data(), npix * 3 * sizeof(float), hipMemcpyHostToDevice,
                                  c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->st.set_frame(frame_counter);  // frameSum is no longer the sum the moments followed
    return RT_OK;
}

const char* rt_error_string(int status) {
    switch (status) {
        case RT_OK: return "ok";
        case RT_ERR_INVALID_ARGUMENT: return "invalid argument";
        case RT_ERR_NO_DEVICE: return "no HIP device";
        case RT_ERR_HIP: return "HIP runtime error";
        case RT_ERR_OUT_OF_MEMORY: return "out of device memory";
        case RT_ERR_NO_SCENE: return "no scene";
        case RT_ERR_UNSUPPORTED: return "unsupported";
        default: return "unknown status";
    }
}

const char* rt_last_error(const rt_context* c) { return c ? c->err.c_str() : ""; }

const char* rt_last_kernel_name(const rt_context* c) { return c ? c->kernel_name.c_str() : ""; }

int rt_context_threads(const rt_context* c) { return c && c->cpu ? c->threads : 0; }

}  // extern "C"
