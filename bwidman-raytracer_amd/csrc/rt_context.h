// rt_context.h — what the host units of the C ABI (include/rt_abi.h) share:
// struct rt_context with its buffer and pass types, the error helpers, and
// the kernel launchers.  Private to csrc/.
//
//   rt_context.cpp  create / destroy, setters, controls, state, errors
//   rt_render.cpp   prepare, fill_view, launch, rt_render*, multi-GPU, de-interleave
//   rt_render_adaptive.cpp  rt_render_adaptive*, rt_get_counts (rt_adaptive.h)
//   rt_post.cpp     first-hit features, denoiser, temporal reprojection, moment readout
//   rt_gather.cpp   rt_export_shard*, rt_assemble*, the assembled frame (rt_assemble.h)
//   rt_group.h      over this header: lists of shard contexts, block geometry, the _device preamble
//   rt_scene.cpp    the scene compiler (rt_scene.h; no HIP, no context)
//   rt_accum.h      the accumulation's host state and its transition table (no HIP)
//   rt_view.h       the view-bound host state (view, guides, history roles, assembled record) likewise
// The render kernels: rt_launch.h declares the launchers of their units
// (rt_kernels{,_bvh,_fast,_bvh_fast,_shared}.hip); one header per kernel
// (rt_kernel_simple.h, rt_kernel_sorted.h, rt_kernel_pair.h, rt_kernel_refill.h)
// over rt_pixel.h and rt_hit.h, the launch policy in rt_launch_brute.h.
// The post-render passes' kernels and arithmetic: rt_atrous.h (what the filters
// and the reprojection share, host and device), rt_atrous_tile.h (the pixel and
// the LDS-tiled kernel with their launchers, device only), then one header and
// one unit each: rt_denoise, rt_denoise_var, rt_temporal, rt_temporal_var, rt_moments; rt_assemble
// (the two copies behind rt_export_shard* and rt_assemble*, counted or not).
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>
#include <xmmintrin.h>

#include "../../include/rt_abi.h"
#include "rt_accum.h"
#include "rt_launch.h"
#include "rt_layout.h"
#include "rt_scene.h"
#include "rt_sky.h"
#include "rt_view.h"

// ---- kernel launchers (the render units': rt_launch.h) ------------------------
// scalar C++ CPU fallback (rt_cpu.cpp)
// (N.n_lights > 0: the next-event estimator of rt_light.h, here and in rt_cpu_adaptive_render)
int rt_cpu_render(const rt_kparams& K, const rt_nee_args& N, int threads);
// rt_light_pick_probabilities on the host: rt_launch_pick_probabilities' twin (host pointers)
void rt_cpu_pick_probabilities(const rt_nee_args& N, int n_sph, const float* points, const int* prims, int count, float* out,
                               int threads);
// adaptive sampling on the host (rt_adaptive.h): selection into A.list /
// *A.list_n, the listed pixels' frames, their update, the resolve pass
void rt_cpu_adaptive_select(const rt_ad_args& A, int threads);
// the selection of rt_render_adaptive_reprojected, from the pending planes
void rt_cpu_adaptive_select_reproj(const rt_ad_reproj_args& R, int threads);
// on row shards: the row sums of the shard's rows into its block, and the
// selection from the gathered blocks
void rt_cpu_adaptive_rows_block(const rt_ad_args& A, long plane, int threads);
void rt_cpu_adaptive_select_shard(const rt_ad_shard_args& S, int threads);
void rt_cpu_adaptive_render(const rt_kparams& K, const rt_nee_args& N, const rt_ad_args& A, int threads);
void rt_cpu_adaptive_finish(const rt_ad_args& A, int threads);
void rt_cpu_init_rand(unsigned* rng, int width, int rows, int row_offset, int row_stride);
bool rt_cpu_supported();
void rt_cpu_aov(const rt_kparams& K, int threads, float4* ga, float4* gb, float4* alb);
void rt_cpu_denoise_level(const rt_dn_level& L, int threads);
void rt_cpu_temporal(const rt_tp_args& T, int threads);
void rt_cpu_temporal_var(const rt_tv_cnt_args& V, int threads);  // V.cnt non-null: the count-aware pass
void rt_cpu_temporal_var_input(const rt_tv_input& A, int threads);
void rt_cpu_moments(const rt_mom_args& A, int threads);
void rt_cpu_denoise_var(const rt_dv_args& A, int stage, int threads);
void rt_cpu_export_shard(const rt_asm_args& A, int threads);
void rt_cpu_assemble(const rt_asm_args& A, int threads);
// a-trous filter (rt_denoise.hip)
hipError_t rt_launch_denoise_level(const rt_dn_level& L, bool tiled, hipStream_t stream);
// temporal reprojection (rt_temporal.hip)
hipError_t rt_launch_temporal(const rt_tp_args& T, hipStream_t stream);
// moment-carrying reprojection and the input stage of the levels behind it (rt_temporal_var.hip)
// (V.cnt non-null: the count-aware kernel of rt_temporal_var_counted)
hipError_t rt_launch_temporal_var(const rt_tv_cnt_args& V, hipStream_t stream);
hipError_t rt_launch_temporal_var_input(const rt_tv_input& A, hipStream_t stream);
// luminance moment update (rt_moments.hip)
hipError_t rt_launch_moments(const rt_mom_args& A, hipStream_t stream);
// variance-guided filter (rt_denoise_var.hip): stage 0 input, 1 sigma pass, 2 level
hipError_t rt_launch_denoise_var(const rt_dv_args& A, int stage, bool tiled, hipStream_t stream);
// a shard's block and the assembled frame, counted or not (rt_assemble.hip); max_blocks > 0 caps the grid
hipError_t rt_launch_export_shard(const rt_asm_args& A, int max_blocks, hipStream_t stream);
hipError_t rt_launch_assemble(const rt_asm_args& A, int max_blocks, hipStream_t stream);
// adaptive sampling (rt_adaptive.hip): the count fill; stage 0 row sums, 1 column
// sums + test + scan + scatter, 2 the listed pixels' moment update, 3 resolve
hipError_t rt_launch_adaptive_fill(uint2* cnt, unsigned long long* total, long npix, unsigned n, unsigned J,
                                   hipStream_t stream);
hipError_t rt_launch_adaptive(const rt_ad_args& A, int stage, hipStream_t stream);
// stages 0 and 1 of rt_render_adaptive_reprojected: row sums over the pending
// planes, column sums + test with the `fresh` term, then scan and scatter as ever
hipError_t rt_launch_adaptive_reproj(const rt_ad_reproj_args& R, hipStream_t stream);
// adaptive sampling on row shards: the row sums of a shard's rows into its block
// (planes of `plane` words, padding rows zeroed), and stage 1 with the column
// taps from the gathered blocks
hipError_t rt_launch_adaptive_rows_block(const rt_ad_args& A, long plane, hipStream_t stream);
hipError_t rt_launch_adaptive_shard(const rt_ad_shard_args& S, hipStream_t stream);

// ---- buffers -------------------------------------------------------------------
// Device memory on a GPU context, host memory on a CPU context (ensure_buf);
// frees itself with the context.
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    bool host = false;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    void release() {
        if (p) host ? std::free(p) : (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// ---- passes --------------------------------------------------------------------
// One kind of work the context puts on a stream (render, de-interleave,
// denoise, reprojection): where the last one ran, the event that marks its
// end — later work on another stream and host-side state writes are ordered
// after it; events, not stream handles, so a caller may destroy its streams —
// and its duration.  A CPU context (`host`) has no events: a pass is over
// when it returns, and is timed by the wall clock.
struct Pass {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // start marker (timed passes) and end
    hipStream_t stream = nullptr;             // of the last one
    // the context's own stream, for the render pass alone: a pass there
    // without a start marker leaves its end event `pending` (see end)
    hipStream_t home = nullptr;
    bool host = false;
    bool recorded = false;  // ev1 was recorded at least once
    bool pending = false;   // the last one ran on `home` and ev1 is not recorded for it yet
    bool timed = false;     // ev0 .. ev1 bracket the last one
    bool marked = false;    // begin() recorded the start marker
    float cpu_ms = -1.0f;
    std::chrono::steady_clock::time_point t0;

    // the events; `timing`: a start marker too and default flags, else an
    // end event without timing.  Idempotent (the temporal pass creates its
    // events on first use: nothing is allocated before the first call).
    hipError_t create(bool timing) {
        hipError_t e = hipSuccess;
        if (timing && !ev0) e = hipEventCreate(&ev0);
        if (e == hipSuccess && !ev1) e = timing ? hipEventCreate(&ev1) : hipEventCreateWithFlags(&ev1, hipEventDisableTiming);
        return e;
    }
    hipError_t begin(hipStream_t s, bool with_marker) {
        marked = with_marker;
        if (host) t0 = std::chrono::steady_clock::now();
        return !host && with_marker ? hipEventRecord(ev0, s) : hipSuccess;
    }
    // Every recorded event is a marker packet the GPU drains between two
    // kernels (~5 us each on MI355X, tools/ev_ab.sh).  On `home`, which lives
    // as long as the context, an unmarked pass therefore records nothing:
    // flush() records the end event when a later call needs it, and
    // back-to-back renders carry no packet between them.
    hipError_t end(hipStream_t s) {
        stream = s;
        if (host) {
            cpu_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        } else if (home && s == home && !marked) {
            pending = true;
        } else {
            pending = false;
            const hipError_t e = hipEventRecord(ev1, s);
            if (e != hipSuccess) return e;
            recorded = true;
        }
        timed = marked;
        return hipSuccess;
    }
    hipError_t flush() {
        if (!pending) return hipSuccess;
        pending = false;
        const hipError_t e = hipEventRecord(ev1, home);
        if (e == hipSuccess) recorded = true;
        return e;
    }
    // order stream s after the last pass (nothing to do on its own stream)
    hipError_t wait_on(hipStream_t s) {
        if (!(recorded || pending) || stream == s) return hipSuccess;
        const hipError_t e = flush();
        return e != hipSuccess ? e : hipStreamWaitEvent(s, ev1, 0);
    }
    hipError_t sync() { return recorded ? hipEventSynchronize(ev1) : hipSuccess; }  // host-side wait (flush first)
    float elapsed_ms() {
        if (host) return cpu_ms;
        float ms = -1.0f;
        if (!timed || hipEventSynchronize(ev1) != hipSuccess || hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess)
            return -1.0f;
        return ms;
    }
    void destroy() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    }
};

struct rt_context {
    int device = 0;
    int num_cus = 256;
    bool simple = false;  // BWRT_KERNEL=simple: one-path-per-lane kernel (A/B reference)
    int grid_mult = 0;  // persistent grid = grid_mult x resident workgroups per CU x CUs
    hipStream_t stream = nullptr;
    // render: the kernels read and write the shard state, so a launch on
    // another stream and host-side state writes wait for the last one.
    // aux: the last de-interleave (rt_synchronize waits for it; it touches no
    // state).  denoise: its levels read frameSum and share the guides and
    // colour buffers.  temporal: the reprojection pass, likewise; its events
    // are created by the first temporal call.  denoise_var: the
    // variance-guided filter, which shares the guides and colour buffers with
    // the denoiser; its events are created by its first call.
    // temporal_var: the moment-carrying reprojection pass (rt_temporal_var),
    // which shares the history sets with `temporal`; likewise.  xport: the
    // last rt_export_shard, which reads frameSum and the moments (the next
    // render waits for it).  assemble: the last rt_assemble, which writes the
    // assembled frame the three full-frame passes read.  Both create their
    // events on first use.
    Pass render, aux, denoise, temporal, denoise_var, temporal_var, xport, assemble;
    // CPU backend (rt_create_cpu): host buffers, and the scalar fallback of
    // rt_cpu.cpp instead of the kernels
    bool cpu = false;
    int threads = 1;
    bool ktiming = true;  // start marker before each render launch (rt_set_kernel_timing)
    std::string err;

    bool has_scene = false;
    rt_camera camera{};
    float background[3] = {0.0f, 0.0f, 0.0f};  // backgroundColor, Main.cu:27
    rt_compiled_scene scene;  // of scene_buf (its `data` is dropped once scene_buf holds it)
    Buf scene_buf;

    // shard state
    int width = 0, height = 0, row_offset = 0, row_stride = 1, rows = 0;
    Buf rng, accum, rgba;
    Buf rec;  // sorted kernel's record stack in global memory (deep paths)
    // launch-order feedback (rt_layout.h): tile-group costs of the last
    // launch and the order sorted from them, valid for a grid of order_n groups
    Buf gcost, gorder;
    long order_n = 0;
    // re-sort the launch order every order_period-th launch (BWRT_ORDER_PERIOD;
    // a grid without an order is always sorted): the per-group costs follow
    // the image, so a kept order is as good as a fresh one, and the sort
    // kernel plus its launch gap cost ~8 us per launch.  Config 3 bench kernel
    // average, three alternating runs: every launch 0.7567 / 0.7543 / 0.7535,
    // every 4th 0.7479 / 0.7461 / 0.7476, every 16th 0.7462 / 0.7430 / 0.7469,
    // never again 0.7451 / 0.7458 / 0.7484 ms (profiles/r03f/order_period_ab.txt);
    // config 2 0.1503 / 0.1515 vs 0.1555 / 0.1565, config 4 5.50 vs 5.52 ms
    int order_period = 16;
    // the kept order was measured on another image (new scene, camera or
    // shard): the next launch re-sorts its costs whatever the period
    bool order_stale = true;
    unsigned long long launches = 0;
    bool order_feedback = true;  // BWRT_ORDER=0: blockIdx order
    int grec = -1;  // BWRT_GREC: 1 / 0 force global / LDS records; -1 = launch policy
    void* host_rgba = nullptr;  // pinned staging for rt_render_multi
    size_t host_rgba_bytes = 0;
    int block = 0;               // BWRT_BLOCK: sorted-kernel workgroup lanes (0 = launch policy)
    int tile_w = -1;             // BWRT_TILE: wave tile width (0 = linear order; -1 = launch policy)
    int tile_sq = 0;             // BWRT_TILE_SQ: a 4-wave group's tiles as 2 x 2 (experiment)
    int leaf_batch = -1;         // BWRT_LEAF_BATCH: BVH refill kernel leaf-batch threshold (-1 = launch policy)
    int refill = -1;             // BWRT_REFILL: BVH refill kernel refill threshold (-1 = launch policy)
    int spread = -1;             // BWRT_SPREAD: 1 / 0 force the pair kernel on / off (-1 = launch policy)
    int deint_blocks = 0;        // BWRT_DEINT_BLOCKS: cap on the de-interleave grid (0 = one thread per 16 bytes)
    std::string kernel_name;     // the render kernel of the last launch (rt_last_kernel_name)
    int precision = RT_PRECISION_EXACT;  // rt_set_precision (BWRT_PRECISION): which kernels the next render launches
    // rt_set_light_sampling: the next render takes the next-event estimation kernel (rt_kernel_nee.h) or its
    // CPU twin; light_buf holds the scene's light table (scene.lights; rt_set_scene uploads it)
    bool light_sampling = false;
    Buf light_buf;
    // rt_set_light_picking: how an NEE level picks its light (rt_light.h); acts only where nee_args
    // returns a table
    int light_picking = RT_LIGHT_PICK_UNIFORM;
    static_assert(RT_PICK_UNIFORM == RT_LIGHT_PICK_UNIFORM && RT_PICK_WEIGHTED == RT_LIGHT_PICK_WEIGHTED, "rt_layout.h / rt_abi.h");
    // rt_set_light_shapes: which records of the scene's table a render sees, the sphere lights alone or
    // the polygon lights behind them as well
    int light_shapes = RT_LIGHT_SHAPES_SPHERES;
    static_assert(RT_SHAPES_SPHERES == RT_LIGHT_SHAPES_SPHERES && RT_SHAPES_ALL == RT_LIGHT_SHAPES_ALL, "rt_layout.h / rt_abi.h");
    int n_lights() const {
        return light_shapes == RT_LIGHT_SHAPES_ALL ? (int)(scene.lights.size() / RT_LIGHT_FLOATS) : scene.n_sphere_lights;
    }
    // The light table a render at max_bounces takes, or none ({null, 0}: the default estimator, its
    // kernels and launch policy): the switch, and a scene and a depth where the estimators differ (an
    // empty table and max_bounces 0 are bit-identical to the default, rt_light.h)
    rt_nee_args nee_args(int max_bounces) const {
        const int n = n_lights();
        if (!light_sampling || n == 0 || max_bounces <= 0) return {nullptr, 0, 0, nullptr, 0, nullptr};
        return table_args(n);
    }
    // rt_set_light_hierarchy: weighted picking descends the light tree of the table form the render sees
    // (rt_light.h RT_PICK_TREE) instead of walking the table; acts only where picking is weighted and
    // that table holds at least 2 records (light_buf: records, sampling blocks, then the two trees)
    bool light_hierarchy = false;
    // the table of n = n_lights() > 0 records with the pick mode that acts on it (nee_args, and
    // rt_light_pick_probabilities, which asks whatever the switch and the depth)
    rt_nee_args table_args(int n) const {
        const float* tab = light_buf.as<const float>();
        const float* polys = tab + scene.lights.size();
        if (light_hierarchy && light_picking == RT_LIGHT_PICK_WEIGHTED && n >= 2) {
            const float* trees = polys + scene.light_polys.size();
            const float* tree = n > scene.n_sphere_lights ? trees + scene.light_tree_spheres.size() : trees;
            return {tab, n, RT_PICK_TREE, polys, scene.n_sphere_lights, tree};
        }
        return {tab, n, light_picking, polys, scene.n_sphere_lights, nullptr};
    }
    // the tree of the current shapes mode's table (empty: fewer than 2 records)
    const std::vector<float>& light_tree() const {
        return n_lights() > scene.n_sphere_lights ? scene.light_tree_all : scene.light_tree_spheres;
    }
    // the frame counter, the moment tracking and the non-uniform state: what
    // frameSum currently holds (rt_accum.h has the rules)
    rt_accum_state st;
    int max_bounces = RT_DEFAULT_MAX_BOUNCES;
    int spp_inner = 1;  // samplesPerPixel, Main.cu:27

    // the view counter, the guides' validity, the roles of the temporal history
    // sets and the record of the assembled frame (rt_view.h has the rules)
    rt_view_state vs;

    // denoiser (rt_denoise): the first-hit guides of the current full frame
    // {n.xyz, prim} / {P.xyz, depth}, valid for one view (`vs`), and two
    // ping-pong colour buffers
    Buf guide_a, guide_b, dn_col[2], dn_rgba;
    Buf dn_rs;  // rt_denoise_var: the reciprocal luminance sigma, one float per pixel
    Buf aov_a, aov_b, aov_alb;  // rt_render_aov scratch (any shard; GPU contexts)
    int dn_kernel = -1;  // BWRT_DENOISE_KERNEL: 0 direct, 1 tiled, -1 = the measured per-level policy

    // temporal reprojection (rt_temporal, rt_temporal_var): two buffer sets
    // {colour + length, guide copy, {s2, dof}, camera}; which one is the history
    // and which holds the pending result is `vs`'s to say.  Nothing is allocated
    // (events included) before the first call, `mom` by the first
    // rt_temporal_var call only.
    struct TpSet {
        Buf col, ga, gb, mom;
        float cam_pos[3] = {}, rot[9] = {}, screen_z = 0.0f;
    };
    TpSet tp[2];

    // luminance moment tracking (rt_set_moments): a copy of frameSum before
    // the last tracked batch (3 planes) and {M, M2} per shard pixel, updated
    // by one pass behind every tracked render call (`st`, rt_accum.h).
    // Nothing is allocated before tracking is on and a render runs.
    Buf mom_prev, mom_m;

    // assembled frame (rt_assemble*, DESIGN.md sections 17 and 19): a full-frame
    // snapshot {frameSum, optionally {M, M2}, optionally {n_p, J_p}}
    // de-interleaved from the ranks' gathered blocks, which the full-frame
    // passes read when the context's own pixel state is a row shard; its record
    // and whether it is current are `vs`'s to say.  as_block: this context's
    // exported block, as_gather: the gathered blocks (staging of the host forms
    // and of rt_assemble_multi).  Nothing is allocated before the first call.
    struct Assembled {
        Buf sum, mom, cnt;
    };
    Assembled as;
    Buf as_block, as_gather;
    bool assembled_current() const { return vs.assembled_current(width, height); }
    rt_block_shape assembled_shape() const { return rt_block_shape_of(vs.assembled().planes); }  // moments, counts
    bool holds_shard() const { return row_offset != 0 || row_stride > 1; }

    // adaptive sampling (rt_render_adaptive, rt_adaptive.h).  While `st` is
    // non-uniform, ad_cnt holds {n_p, J_p} per pixel (filled with the context's
    // counts by the first adaptive call of an accumulation; nothing is
    // allocated before).  The selection's scratch: row sums, mask words with
    // their popcounts, the list and {list_n, frame total}.  ad_ev: select /
    // render / update + resolve brackets of the last call, recorded only with
    // kernel timing on.
    int ad_kernel = 0;  // BWRT_ADAPTIVE_KERNEL: 1 simple, 2 queued, 0 = launch policy
    Buf ad_cnt, ad_rows, ad_mask, ad_pop, ad_list, ad_stat, ad_color;
    // on row shards (rt_adaptive_export_rows, rt_render_adaptive_shard): this
    // context's row-sum block and the gathered blocks, staging of the host
    // forms and of rt_render_adaptive_multi.  Whether the last export is still
    // current is `st`'s to say.
    Buf ad_block, ad_gather;
    hipEvent_t ad_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ad_timed = false;
    float ad_cpu_ms[3] = {-1.0f, -1.0f, -1.0f};
    long long ad_cpu_selected = 0, ad_cpu_total = 0;

    // sky table (rt_sky.h): the table of the view `sky_key`, on the host and
    // (GPU contexts) in sky_buf; rebuilt and uploaded only when the key
    // changes.  sky_gen counts scene and camera changes (rt_set_scene,
    // rt_set_camera, rt_controls); sky_builds counts the tables built.
    struct SkyKey {
        unsigned long long gen = 0;
        int width = 0, height = 0, rows = 0, row_offset = 0, row_stride = 0, tile_w = 0, tile_sq = 0, spp_inner = 0;
        float jitter = 0.0f;
        bool operator==(const SkyKey& o) const {
            return gen == o.gen && width == o.width && height == o.height && rows == o.rows &&
                   row_offset == o.row_offset && row_stride == o.row_stride && tile_w == o.tile_w &&
                   tile_sq == o.tile_sq && spp_inner == o.spp_inner && jitter == o.jitter;
        }
    };
    // A render builds the table of a view at the view's SECOND launch: a
    // build costs about as much host time as the sky path saves in fifty
    // config-3 launches (DESIGN.md "sky groups"), so a moving camera, whose
    // views are launched once, never pays for one; an accumulating view pays
    // once.  BWRT_SKY=0: no sky path; 2: build at the first launch (tests, A/B)
    bool sky_on = true, sky_eager = false;
    unsigned long long sky_gen = 1, sky_builds = 0;
    SkyKey sky_key;   // gen 0: no table yet
    SkyKey sky_seen;  // the view of the last launch that went without a table
    bool sky_any = false;  // the table has a set bit
    bool sky_uploaded = false;  // sky_buf holds sky_bits
    rt_sky_prims sky_prims;  // of the context's scene (rt_set_scene)
    std::vector<uint32_t> sky_bits;
    Buf sky_buf;
    hipEvent_t sky_ev = nullptr;  // behind the last upload (created by the first one)

    // a new view (scene, camera, frame shape): the guides are stale
    void new_view() { vs.new_view(); }
    // the scene or the camera changed: the next render restarts the
    // accumulation (Controls.cuh: any movement sets accumulatedFrames = 1), on
    // another image than the launch order and the sky table were made for
    void view_changed() {
        st.restart();
        order_stale = true;
        sky_gen++;
        new_view();
    }
};

// ---- helpers shared by the units (rt_context.cpp) -----------------------------
// IEEE float state for the library's host-side float work (scene compile,
// camera set-up, controls): round to nearest, no FTZ / DAZ, whatever the
// calling thread holds (a -ffast-math library or torch.set_flush_denormal
// may have set them), restored on return — the GPU keeps f32 denormals and
// the compiled scene must not depend on the caller
struct HostFpEnv {
    unsigned saved;
    HostFpEnv() : saved(_mm_getcsr()) {
        _mm_setcsr((saved & ~(_MM_ROUND_MASK | _MM_FLUSH_ZERO_MASK | 0x0040u)) | _MM_ROUND_NEAREST);  // 0x40 = DAZ
    }
    ~HostFpEnv() { _mm_setcsr(saved); }
};

// Tuning and diagnostic knobs (BWRT_BLOCK, BWRT_TILE, BWRT_GREC, BWRT_SPREAD,
// BWRT_ORDER*, BWRT_BVH_*, BWRT_STAMPS, ...; listed in rt_abi.h) are read
// only when the process sets BWRT_TUNING=1: a default context always takes
// the measured launch policy, whatever else the environment holds.
const char* tuning_env(const char* name);

int fail(rt_context* c, int code, const char* fmt, ...);
int hip_fail(rt_context* c, hipError_t e, const char* what);

#define HIP_TRY(ctx, expr)                                  \
    do {                                                    \
        hipError_t _e = (expr);                             \
        if (_e != hipSuccess) return hip_fail(ctx, _e, #expr); \
    } while (0)

// Host-side wait for every pass that uses the shard state or the assembled
// frame (render, denoise, temporal, variance-guided denoise, export, assembly),
// on whatever streams they ran; no-op on a CPU context
int quiesce(rt_context* c);
// Order stream s after the same passes (no host sync)
int order_after_all(rt_context* c, hipStream_t s);
// At least `bytes` in b (never shrinks).  A CPU context allocates host
// memory; its failure is RT_ERR_OUT_OF_MEMORY with the message host_oom
// (a format taking n).  A buffer that may be in use is freed only after
// quiesce() and a sync of the context's stream.
int ensure_buf(rt_context* c, Buf& b, size_t bytes, const char* host_oom = "host buffer (%zu)", size_t n = 0);
int shard_rows(int height, int row_offset, int row_stride);
int shard_check(rt_context* c, int width, int height, int row_offset, int row_stride);  // RT_OK or the failure
// Host copies of device buffers of a GPU context once no queued work writes
// them: the context's stream synchronised, quiesce(), then one hipMemcpy per
// entry with a destination.  Staging memory is the caller's (try_resize).
struct HostCopy {
    void* dst;
    const void* src;
    size_t bytes;
};
int read_settled(rt_context* c, std::initializer_list<HostCopy> copies);
template <class T>
bool try_resize(std::vector<T>& v, size_t n) {  // false: out of host memory
    try {
        v.resize(n);
    } catch (...) {
        return false;
    }
    return true;
}
// Camera prelude and compiled scene of a width x height view (shard
// row_offset, stride, rows) into K; every other field 0 (rt_render.cpp)
void fill_view(rt_context* c, int width, int height, int row_offset, int stride, int rows, rt_kparams& K);
// The launch policy's wave tiles of a brute-force view (K.rows, K.width set)
void policy_tiles(const rt_context* c, rt_kparams& K);
// The sky table of view K (tile shape set) in c->sky_bits, rebuilt only when
// its key changed (rt_render.cpp)
void sky_table(rt_context* c, const rt_kparams& K);

// ---- layouts of the ABI's host arrays -----------------------------------------
// frameSum: 3 planes of npix on the device, interleaved RGB at the ABI
inline void planes_to_rgb(const float* planes, size_t npix, float* out) {
    for (size_t i = 0; i < npix; i++)
        for (int ch = 0; ch < 3; ch++) out[3 * i + ch] = planes[ch * npix + i];
}
inline void rgb_to_planes(const float* rgb, size_t npix, float* planes) {
    for (size_t i = 0; i < npix; i++)
        for (int ch = 0; ch < 3; ch++) planes[ch * npix + i] = rgb[3 * i + ch];
}
// float4 images: .xyz as RGB triplets, .w as one plane
inline void xyz_of(const float4* v, size_t npix, float* out) {
    for (size_t i = 0; i < npix; i++) {
        out[3 * i + 0] = v[i].x;
        out[3 * i + 1] = v[i].y;
        out[3 * i + 2] = v[i].z;
    }
}
inline void w_of(const float4* v, size_t npix, void* out) {  // float or int32 bits
    for (size_t i = 0; i < npix; i++) std::memcpy(static_cast<char*>(out) + 4 * i, &v[i].w, 4);
}
