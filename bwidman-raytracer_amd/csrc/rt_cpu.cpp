// rt_cpu.cpp — scalar C++ CPU fallback of the render kernel (host only).
//
// The same path as the HIP kernels (reference /root/reference/bwidman-raytracer/src:
// launchRaytracer Main.cu:274-315, tracePath Main.cu:208-272, Intersection.cuh:
// 15-173), one pixel per loop iteration, all `samples` progressive frames of a
// pixel in a row with its RNG state and frameSum in registers, built from the
// per-ray functions of rt_path.h that the kernels use (compiled here for the
// host: -ffp-contract=off, IEEE sqrtss/divss, hardware fma for the exactly
// specified fma steps), so every pixel is bit-identical to the GPU result and
// to the oracle (tests/test_cpu_fallback.py).
//
// Threads take 256-pixel chunks of the shard from an atomic counter
// (std::thread; the calling thread works too).  Scenes with a BVH walk the
// same threaded fp32 node arrays as the kernels, scalar: a leaf is tested as
// soon as the walk reaches it, with the same (t, RT_KEY) acceptance, so the
// result does not depend on the visiting order (rt_path.h key_accept).
//
// This is an explicit backend: only contexts made by rt_create_cpu() render
// here (include/rt_abi.h).  A GPU context never falls back to it.
#include <atomic>
#include <thread>

#include <xmmintrin.h>  // MXCSR
#include <vector>

#include "rt_light.h"
#include "rt_path.h"

namespace {

// scalar threaded-BVH walk: the kernels' closest_hit_bvh without the wave
// scheduling (no leaf parking)
void closest_hit_bvh_cpu(const rt_kparams& K, f3 o, f3 d, float& best_t, int& best_id) {
    if (!bvh_safe(K, o, d)) {  // NaN/inf rays, overflowing tests: the reference's interleaved loop
        closest_hit_brute(K, o, d, best_t, best_id);
        return;
    }
    const float a = dot(d, d);
    const float a4 = 4.0f * a;
    const float a2 = 2.0f * a;
    best_t = INFINITY;
    best_id = -1;
    int best_key = -1;
    planes_first(K, o, d, best_t, best_id, best_key);
    const SlabRay sr = slab_ray(o, d);
    const float* nodes = K.bvh_nodes + (size_t)ray_octant(K, d) * K.bvh_order_stride;
    int node = 0;
    while (node >= 0) {
        const float* nd = nodes + 8 * (size_t)node;  // {bmin, miss, bmax, leaf}
        const int miss = rt_f2i(nd[3]);
        if (!slab_enter(nd[0], nd[1], nd[2], nd[4], nd[5], nd[6], sr, best_t)) {
            node = miss;
            continue;
        }
        const int lf = rt_f2i(nd[7]);
        if (lf < 0) {  // internal: first child next
            node = node + 1;
            continue;
        }
        const int first = lf & 0xffffff, count = lf >> 24;
        for (int k = 0; k < count; k++)
            leaf_test(K, K.bvh_leafrec + (size_t)RT_LEAF_FLOATS * (first + k), o, d, a2, a4, best_t, best_id, best_key);
        node = miss;
    }
}

// One path from (o, d) (tracePath, Main.cu:208-272, iteratively): the
// per-level records, folded innermost-first into the returned radiance; the
// twin of rt_kernel_lane.h's lane_loop, statement for statement.
// NEE: next-event estimation (rt_light.h) — at a diffuse hit whose scattered
// ray will be traced, the three draws, the direct term of the picked light
// through a shadow ray, and the suppression of the emission the scattered ray
// finds on a reachable table light.  The caller takes NEE iff N.n_lights > 0,
// PICK (how nee_sample picks its light, rt_light.h) from N.pick and SHAPES
// (RT_SHAPES_ALL: the table holds polygon lights) from its record counts.
template <bool NEE, int PICK, int SHAPES>
f3 trace_path(const rt_kparams& K, const rt_nee_args& N, Xorwow& rs, f3 o, f3 d) {
    // recursion records (code, k, cosAngle; NEE: aux): at most max_bounces + 1 hits
    int rec_code[RT_MAX_LEVELS];
    float rec_k[RT_MAX_LEVELS], rec_c[RT_MAX_LEVELS];
    [[maybe_unused]] int rec_aux[NEE ? RT_MAX_LEVELS : 1];
    int depth = 0;
    [[maybe_unused]] int nee_prim = -1;  // >= 0: (o, d) is the scattered ray of an NEE level on that primitive
    auto hit = [&](f3 ro, f3 rd, float& t, int& id) {
        if (K.bvh_nodes)
            closest_hit_bvh_cpu(K, ro, rd, t, id);
        else
            closest_hit_brute(K, ro, rd, t, id);
    };
    while (true) {
        float t;
        int id;
        hit(o, d, t, id);
        if (id < 0) break;  // miss: backgroundColor (Main.cu:269-271)
        // shade (Main.cu:237-264)
        const float* h = K.hit + RT_HIT_FLOATS * id;
        const f3 P = add(o, scale(t, d));
        f3 n = mk(h[0], h[1], h[2]);
        if (h[3] != 0.0f) n = normalize3(sub(P, n));  // sphere: centre -> normal
        [[maybe_unused]] int aux = 0;
        if constexpr (NEE) {
            if (nee_prim >= 0 && light_suppressed<SHAPES>(K, N, o, nee_prim, id)) aux = RT_NEE_DROP;
            nee_prim = -1;
        }
        f3 scatter;
        int code = id;
        float k = 0.0f;  // specular brdf scalar, or an NEE level's weight
        if (rand_range(rs, 1.0f) < RT_SPECULAR_CHANCE) {  // brdfChoice (Main.cu:243)
            scatter = specular_scatter(rs, d, n, h[8], h[10], h[9], k);
            code = ~id;
        } else {
            scatter = random_direction(rs, n);  // brdf = 4 * albedo
            if constexpr (NEE) {
                const int kind = nee_normal_kind(h[3] != 0.0f, n);
                if (depth + 1 <= K.max_bounces && N.n_lights > 0 && kind) {
                    const NeeSample s = nee_sample<PICK, SHAPES>(rs, N, P, n, id, kind);
                    aux |= RT_NEE_LEVEL | (s.j << RT_NEE_JSHIFT);
                    k = s.k;
                    nee_prim = id;
                    if (s.trace) {
                        float ts;
                        int ids;
                        hit(P, s.wi, ts, ids);
                        if (ids == s.prim) aux |= RT_NEE_VISIBLE;
                    }
                }
            }
        }
        rec_code[depth] = code;
        rec_k[depth] = k;
        rec_c[depth] = dot(scatter, n);  // cosAngle, Main.cu:264
        if constexpr (NEE) rec_aux[depth] = aux;
        depth++;
        o = P;
        d = scatter;
        if (depth > K.max_bounces) break;  // the next call returns background (Main.cu:210)
    }
    // fold the recursion innermost-first (Main.cu:262-268)
    float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];
    for (int l = depth - 1; l >= 0; --l) {
        if constexpr (NEE)
            fold_level_nee(rec_code[l], rec_k[l], rec_c[l], rec_aux[l], K.hit, N, lx, ly, lz);
        else
            fold_level(rec_code[l], rec_k[l], rec_c[l], K.hit, lx, ly, lz);
    }
    return mk(lx, ly, lz);
}

// Every frame of shard pixel p (Main.cu:285-312 per frame, frames in order),
// the first one `first`: K.first_frame, or n_p + 1 of a listed pixel of an
// adaptive call (rt_adaptive.h), whose image the resolve pass writes
template <bool NEE, int PICK, int SHAPES>
void render_pixel_as(const rt_kparams& K, const rt_nee_args& N, long npix, long p, unsigned first) {
    const int j = (int)(p / K.width);
    const int x = (int)(p - (long)j * K.width);
    const int y = K.row_offset + j * K.row_stride;
    Xorwow rs;
    rs.d = K.rng[0 * npix + p];
    rs.v0 = K.rng[1 * npix + p];
    rs.v1 = K.rng[2 * npix + p];
    rs.v2 = K.rng[3 * npix + p];
    rs.v3 = K.rng[4 * npix + p];
    rs.v4 = K.rng[5 * npix + p];
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (first != 1u) {
        ax = K.accum[0 * npix + p];
        ay = K.accum[1 * npix + p];
        az = K.accum[2 * npix + p];
    }
    const f3 d0 = primary_dir(K, x, y);
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
    unsigned frame = first;
    for (int s = 0; s < K.samples; s++) {
        // jittered camera ray (Main.cu:290-292)
        const f3 jit = random_direction(rs, d0);
        const f3 dcam = normalize3(add(d0, scale(K.jitter, jit)));
        // samplesPerPixel paths from it; the last one is kept (Main.cu:296-298)
        f3 L = trace_path<NEE, PICK, SHAPES>(K, N, rs, cam, dcam);
        for (int i = 1; i < K.spp_inner; i++) L = trace_path<NEE, PICK, SHAPES>(K, N, rs, cam, dcam);
        float lx = L.x, ly = L.y, lz = L.z;
        if (K.spp_inner != 1) {  // pixel /= samplesPerPixel: (1.0f / k) * pixel (Math.cuh:91-97)
            const float k = 1.0f / (float)K.spp_inner;
            lx = k * lx;
            ly = k * ly;
            lz = k * lz;
        }
        // progressive accumulation (Main.cu:299-304)
        if (frame == 1u) {
            ax = 0.0f;
            ay = 0.0f;
            az = 0.0f;
        }
        ax = ax + lx;
        ay = ay + ly;
        az = az + lz;
        frame++;
    }
    K.rng[0 * npix + p] = rs.d;
    K.rng[1 * npix + p] = rs.v0;
    K.rng[2 * npix + p] = rs.v1;
    K.rng[3 * npix + p] = rs.v2;
    K.rng[4 * npix + p] = rs.v3;
    K.rng[5 * npix + p] = rs.v4;
    K.accum[0 * npix + p] = ax;
    K.accum[1 * npix + p] = ay;
    K.accum[2 * npix + p] = az;
    if (K.rgba) K.rgba[p] = tone_map(ax, ay, az, frame - 1u);
}

// (the estimator is picked once per pixel: rt_set_light_sampling, rt_set_light_picking, rt_set_light_hierarchy,
// rt_set_light_shapes)
template <int SHAPES>
void render_pixel_nee(const rt_kparams& K, const rt_nee_args& N, long npix, long p, unsigned first) {
    if (N.pick == RT_PICK_TREE)
        render_pixel_as<true, RT_PICK_TREE, SHAPES>(K, N, npix, p, first);
    else if (N.pick == RT_PICK_WEIGHTED)
        render_pixel_as<true, RT_PICK_WEIGHTED, SHAPES>(K, N, npix, p, first);
    else
        render_pixel_as<true, RT_PICK_UNIFORM, SHAPES>(K, N, npix, p, first);
}

void render_pixel(const rt_kparams& K, const rt_nee_args& N, long npix, long p, unsigned first) {
    if (N.n_lights > N.n_sphere_lights)
        render_pixel_nee<RT_SHAPES_ALL>(K, N, npix, p, first);
    else if (N.n_lights > 0)
        render_pixel_nee<RT_SHAPES_SPHERES>(K, N, npix, p, first);
    else
        render_pixel_as<false, RT_PICK_UNIFORM, RT_SHAPES_SPHERES>(K, N, npix, p, first);
}

// fn(p) for p = 0 .. n-1 in 256-item chunks, which `threads` threads (>= 1; the
// calling thread works too) take from an atomic counter; returns the threads
// used when all are done (the barrier between two filter levels).  Every item
// writes only its own outputs, so the result does not depend on the thread count.
template <class Fn>
int parallel_items(long n, int threads, const Fn& fn) {
    constexpr long kChunk = 256;
    const long chunks = (n + kChunk - 1) / kChunk;
    if (threads < 1) threads = 1;
    if ((long)threads > chunks) threads = (int)(chunks > 0 ? chunks : 1);
    std::atomic<long> next(0);
    auto work = [&]() {
        // IEEE float state for the whole pass, whatever the calling thread
        // holds (a -ffast-math library or torch.set_flush_denormal may have
        // set FTZ / DAZ, and new threads inherit it): round to nearest, no
        // denormal flushing — the GPU keeps f32 denormals — restored after
        const unsigned saved = _mm_getcsr();
        _mm_setcsr((saved & ~(_MM_ROUND_MASK | _MM_FLUSH_ZERO_MASK | 0x0040u)) | _MM_ROUND_NEAREST);  // 0x40 = DAZ
        for (long c = next.fetch_add(1); c < chunks; c = next.fetch_add(1)) {
            const long end = (c + 1) * kChunk < n ? (c + 1) * kChunk : n;
            for (long p = c * kChunk; p < end; p++) fn(p);
        }
        _mm_setcsr(saved);
    };
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads - 1);
    for (int t = 1; t < threads; t++) {
        try {
            pool.emplace_back(work);
        } catch (...) {  // no more threads: the ones running (and this one) finish the work
            break;
        }
    }
    work();
    for (std::thread& t : pool) t.join();
    return (int)pool.size() + 1;
}

}  // namespace

// The host can run this translation unit (built for x86-64-v3); checked with
// baseline instructions only
__attribute__((target("arch=x86-64"))) bool rt_cpu_supported() {
    __builtin_cpu_init();
    return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
}

// curand_init(y*W + x, 0, 0) for every shard pixel (Main.cu:369-380), planes
void rt_cpu_init_rand(unsigned* rng, int width, int rows, int row_offset, int row_stride) {
    const long npix = (long)rows * width;
    for (long p = 0; p < npix; p++) {
        const int j = (int)(p / width);
        const int x = (int)(p - (long)j * width);
        const Xorwow s = xorwow_seed(pixel_seed(x, row_offset + j * row_stride, width));
        rng[0 * npix + p] = s.d;
        rng[1 * npix + p] = s.v0;
        rng[2 * npix + p] = s.v1;
        rng[3 * npix + p] = s.v2;
        rng[4 * npix + p] = s.v3;
        rng[5 * npix + p] = s.v4;
    }
}

// Render K.samples frames of the shard in K (host pointers) on `threads`
// threads (>= 1).  Returns the threads actually used.
int rt_cpu_render(const rt_kparams& K, const rt_nee_args& N, int threads) {
    const long npix = (long)K.rows * K.width;
    return parallel_items(npix, threads, [&](long p) { render_pixel(K, N, npix, p, K.first_frame); });
}

void rt_cpu_pick_probabilities(const rt_nee_args& N, int n_sph, const float* points, const int* prims, int count, float* out,
                               int threads) {
    parallel_items(count, threads, [&](long i) {
        const float* q = points + 6 * i;
        const int prim = prims[i];
        const f3 P = mk(q[0], q[1], q[2]), n = mk(q[3], q[4], q[5]);
        float* row = out + (size_t)i * N.n_lights;
        if (N.n_lights > N.n_sphere_lights)
            nee_pick_probabilities<RT_SHAPES_ALL>(N, P, n, prim, prim >= 0 && prim < n_sph, row);
        else
            nee_pick_probabilities<RT_SHAPES_SPHERES>(N, P, n, prim, prim >= 0 && prim < n_sph, row);
    });
}

// ---- first-hit features and the a-trous filter on the host -------------------
#include "rt_denoise.h"
#include "rt_denoise_var.h"
#include "rt_moments.h"
#include "rt_temporal.h"
#include "rt_temporal_var.h"

namespace {

// fn(x, y, p) for every pixel p = y * width + x of a width x height image, as
// parallel_items
template <class Fn>
void parallel_pixels(int width, int height, int threads, const Fn& fn) {
    parallel_items((long)width * height, threads, [&](long p) {
        const int y = (int)(p / width);
        fn((int)(p - (long)y * width), y, p);
    });
}

}  // namespace

// The feature buffers of the shard in K (rt_hit.h rt_aov_kernel): ga, gb
// and alb as the kernel packs them (alb may be null)
void rt_cpu_aov(const rt_kparams& K, int threads, float4* ga, float4* gb, float4* alb) {
    parallel_pixels(K.width, K.rows, threads, [&](int x, int j, long p) {
        const int y = K.row_offset + j * K.row_stride;
        const f3 o = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
        const f3 d = primary_dir(K, x, y);
        float t;
        int id;
        if (K.bvh_nodes)
            closest_hit_bvh_cpu(K, o, d, t, id);
        else
            closest_hit_brute(K, o, d, t, id);
        const AovHit a = aov_shade(K, o, d, t, id);
        ga[p] = make_float4(a.n.x, a.n.y, a.n.z, rt_i2f(a.prim));
        gb[p] = make_float4(a.P.x, a.P.y, a.P.z, a.depth);
        if (alb) alb[p] = make_float4(a.albedo.x, a.albedo.y, a.albedo.z, 0.0f);
    });
}

// One filter level (L.f.step >= 1) or, with L.f.step == 0, the conversion pass
void rt_cpu_denoise_level(const rt_dn_level& L, int threads) {
    parallel_pixels(L.f.width, L.f.height, threads, [&](int x, int y, long p) {
        const bool cnt = L.cnt != nullptr;  // the non-uniform state: every pixel's own count
        if (L.f.step == 0)
            at_store(L.f, p, cnt ? DnFilterCnt::texel(L, p) : DnFilter<true>::texel(L, p));
        else if (L.first && cnt)
            at_run_direct<DnFilterCnt>(L, x, y);
        else if (L.first)
            at_run_direct<DnFilter<true>>(L, x, y);
        else
            at_run_direct<DnFilter<false>>(L, x, y);
    });
}

// The temporal reprojection pass (rt_temporal.h), on the same pool
void rt_cpu_temporal(const rt_tp_args& T, int threads) {
    parallel_pixels(T.width, T.height, threads, [&](int x, int y, long) {
        if (T.cnt)
            tp_run_pixel_cnt(T, x, y);
        else
            tp_run_pixel(T, x, y);
    });
}

// The moment-carrying reprojection pass and the input stage of the levels
// behind it (rt_temporal_var.h), on the same pool
void rt_cpu_temporal_var(const rt_tv_cnt_args& V, int threads) {
    parallel_pixels(V.t.width, V.t.height, threads, [&](int x, int y, long) {
        if (V.cnt)
            tv_run_pixel_cnt(V, x, y);
        else
            tv_run_pixel(V, x, y);
    });
}
void rt_cpu_temporal_var_input(const rt_tv_input& A, int threads) {
    parallel_pixels(A.f.width, A.f.height, threads, [&](int x, int y, long p) { at_store(A.f, p, tv_input(A, x, y)); });
}

// The luminance moment update of one render call (rt_moments.h), on the same pool
void rt_cpu_moments(const rt_mom_args& A, int threads) {
    parallel_items(A.npix, threads, [&](long p) { mom_update(A, p); });
}

// One pass of the variance-guided filter (rt_denoise_var.h): stage 0 the input
// stage, 1 a sigma pass, 2 a level
void rt_cpu_denoise_var(const rt_dv_args& A, int stage, int threads) {
    parallel_pixels(A.f.width, A.f.height, threads, [&](int x, int y, long p) {
        if (stage == 0)
            at_store(A.f, p, A.cnt ? dv_input_cnt(A, x, y) : dv_input(A, x, y));
        else if (stage == 1)
            A.rs[p] = dv_sigma(A, x, y);
        else
            at_run_direct<DvFilter>(A, x, y);
    });
}

// ---- a shard's block and the assembled frame on the host (rt_assemble.h) --------
#include "rt_assemble.h"

// The 4-byte items of the kernels, on the same pool: every item writes only its
// own words, so the result does not depend on the thread count
void rt_cpu_export_shard(const rt_asm_args& A, int threads) {
    const bool counted = rt_block_shape_of(A.planes).counted;
    parallel_items(asm_items(A, A.rows_per_shard, 1), threads,
                   [&](long q) { counted ? asm_export_item<1, true>(A, q) : asm_export_item<1, false>(A, q); });
}

void rt_cpu_assemble(const rt_asm_args& A, int threads) {
    const bool counted = rt_block_shape_of(A.planes).counted;
    parallel_items(asm_items(A, A.rows, 1), threads,
                   [&](long q) { counted ? asm_assemble_item<1, true>(A, q) : asm_assemble_item<1, false>(A, q); });
}

// ---- adaptive sampling on the host (rt_adaptive.h) -----------------------------
#include "rt_adaptive.h"

namespace {
// The tail of every selection: selected(x, y, p) of every pixel, then the list
// in ascending pixel order (one thread: the order is the specification), its
// length, and the frames it adds to the total
template <class Sel>
void build_list(const rt_ad_args& A, int threads, const Sel& selected) {
    std::vector<unsigned char> flags((size_t)A.npix);  // (no ballot on the host: one byte per pixel)
    parallel_pixels(A.width, A.height, threads, [&](int x, int y, long p) { flags[(size_t)p] = selected(x, y, p) ? 1 : 0; });
    unsigned n = 0;
    for (long p = 0; p < A.npix; p++)
        if (flags[(size_t)p]) A.list[n++] = (int)p;
    *A.list_n = n;
    *A.total = *A.total + (unsigned long long)n * (unsigned)A.k;
}
}  // namespace

// The selection: row sums, then column sums and the test, then the list
void rt_cpu_adaptive_select(const rt_ad_args& A, int threads) {
    parallel_pixels(A.width, A.height, threads, [&](int x, int y, long p) { ad_row_sums(A, x, y, p); });
    build_list(A, threads, [&](int x, int y, long p) { return ad_selected(A, x, y, p); });
}

// The selection of rt_render_adaptive_reprojected: the same three steps over the
// pending planes, the test with the `fresh` term
void rt_cpu_adaptive_select_reproj(const rt_ad_reproj_args& R, int threads) {
    const rt_ad_args& A = R.A;
    parallel_pixels(A.width, A.height, threads, [&](int x, int y, long p) { ad_row_sums_reproj(R, x, y, p); });
    build_list(A, threads, [&](int x, int y, long p) { return ad_selected_reproj(R, x, y, p); });
}

// A shard's row sums into its block, padding rows zeroed
void rt_cpu_adaptive_rows_block(const rt_ad_args& A, long plane, int threads) {
    parallel_pixels(A.width, A.height, threads, [&](int x, int y, long p) { ad_row_sums(A, x, y, p); });
    for (int k = 0; k < 3; k++)
        for (long i = A.npix; i < plane; i++) A.rowv[k * plane + i] = 0.0f;  // (+0.0f: all bits zero, plane 2's int 0 too)
}

// The selection of a shard from the gathered blocks: every pixel's flag depends
// on that pixel alone, the list is made by one thread in ascending order
void rt_cpu_adaptive_select_shard(const rt_ad_shard_args& S, int threads) {
    build_list(S.A, threads, [&](int x, int j, long p) { return ad_selected_shard(S, x, j, p); });
}

// A.k more frames of every listed pixel, each from its own frame count
void rt_cpu_adaptive_render(const rt_kparams& K, const rt_nee_args& N, const rt_ad_args& A, int threads) {
    parallel_items((long)*A.list_n, threads, [&](long i) {
        const long p = A.list[i];
        render_pixel(K, N, A.npix, p, A.cnt[p].x + 1u);
    });
}

// The listed pixels' moment update, then the resolve pass over every pixel
void rt_cpu_adaptive_finish(const rt_ad_args& A, int threads) {
    parallel_items((long)*A.list_n, threads, [&](long i) { ad_update(A, (long)A.list[i]); });
    parallel_items(A.npix, threads, [&](long p) { ad_resolve(A, p); });
}
