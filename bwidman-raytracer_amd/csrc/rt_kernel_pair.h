// rt_kernel_pair.h — the pair kernel (small frames and shards).
#pragma once
#include "rt_hit.h"

// A 128-lane group of two waves for 64 pixels: wave 0 owns them (lane j
// pixel j of the group's tile), wave 1 is their helper (lane 64 + j works
// for owner j only), so no queue, no counters and no compaction — a wave
// holds at most 64 tasks anyway.  A round (3 barriers):
//   X  execute: the owner runs its pixel's diffuse bounce or camera ray in
//      place (genRandomDirection, Main.cu:193-206, 290-292) and posts the
//      next ray; the helper runs the owner's SPEC task (Main.cu:245-255) from
//      its slot and posts that ray;
//   H  closest hit (Main.cu:214-235): the owner takes its SPEC result back
//      and records the bounce; owner and helper each test every other index
//      i of the reference's interleaved loop on the posted ray, the helper
//      the even ones (index 0 carries the planes), the owner the odd ones
//      (rays that fail bvh_safe: the whole loop on the owner);
//   S  owner and helper merge the halves the same way (the smaller
//      distance, ties to the larger RT_KEY); the helper computes the hit
//      point and normal (Main.cu:237-241) for both, the owner draws
//      brdfChoice (:243), parks a finished path for its fold in the next X
//      phase (Main.cu:262-268, 299-304) and posts a SPEC task.
// Every pixel consumes its RNG stream in the reference's order, so results
// equal the sorted kernel's and the oracle's bit for bit.
// LDS: [hit table][records 3 x max_bounces x 64][exchange PF x 64][live flag]
#define RT_PAIR_FIELDS 25
// occupancy target of the pair kernel
#ifndef RT_PAIR_WAVES
#define RT_PAIR_WAVES 7
#endif
RT_MODE_BEGIN
template <bool HIT_LDS, bool ORDER, bool QUADS>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(RT_PAIR_WAVES)))
rt_render_pair_kernel(rt_kparams K) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const int j = tid & 63;           // the pixel this lane works for
    const bool owner = tid < 64;      // (wave-uniform)
    const int n_prim = K.n_sph + K.n_pln + K.n_tri + K.n_quad;
    const float* hit_tab = K.hit;
    float* rec_base = smem;
    if (HIT_LDS) {
        for (int i = tid; i < n_prim * RT_HIT_FLOATS; i += 128) smem[i] = K.hit[i];
        hit_tab = smem;
        rec_base = smem + ((n_prim * RT_HIT_FLOATS + 3) & ~3);
    }
    const int levels = K.max_bounces;
    // record stack [level][field][pixel] (the owner's only)
    lds_float* rec = (lds_float*)(rec_base + j);
    // exchange [field][pixel]: 0-2 ray origin (in S the helper overwrites it
    // with the hit point), 3-5 ray direction, 6 ray flag (0 none, 1 split
    // closest hit, 2 whole loop on the owner), 7-8 the helper's half (t, id),
    // 9-11 the hit's normal (written by the helper in S), 12-14 SPEC
    // scattered direction out, 15 SPEC kspec out, 16-21 RNG state (SPEC in /
    // out), 22 SPEC flag (1 posted, 3 posted and its ray traced), 23-24 the
    // owner's (t, id)
    lds_float* xb = (lds_float*)(rec_base + 3 * levels * 64) + j;
#define XF(f) xb[(f) * 64]
    int* live_flag = reinterpret_cast<int*>(rec_base + 3 * levels * 64 + RT_PAIR_FIELDS * 64);
    const long npix = (long)K.rows * K.width;
    const long nitems = items_of(K, npix);
    diag_group_start(K);
    const long group = ORDER && K.group_order ? (long)K.group_order[blockIdx.x] : (long)blockIdx.x;
    if (ORDER && tid == 0) K.group_cost[group] = (unsigned)__builtin_amdgcn_s_memrealtime();
    PixelState px;
    load_item(K, npix, nitems, owner ? group * 64 + j : nitems, px);  // (helpers: no pixel)
    int mode = px.passes_left > 0 ? T_REGEN : T_NONE;  // the owner's task this round
    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f), hn = o;
    int hid = 0, depth = 0;
    bool hit = false;   // (owner) last S found a hit: its point and normal come from the helper
    int hflag = 0;      // (helper) the ray flag of this round
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
    if (owner) XF(22) = __int_as_float(0);
    __syncthreads();

    bool fold = false;  // a finished path waits for its fold (run in the owner's X phase)
    while (true) {
        // ---- X: execute
        bool has_ray = false, ended = false;
        int dcode = 0;              // deepest level (a bounce at depth max_bounces)
        float dk = 0.0f, dc = 0.0f;
        if (owner) {
            if (fold) {  // fold innermost-first (Main.cu:262-268), accumulate (:299-304)
                fold = false;
                float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];  // backgroundColor (Main.cu:209-211)
                if (depth > K.max_bounces)  // (the deepest level, parked in XF(6..8))
                    fold_level(__float_as_int(XF(6)), XF(7), XF(8), hit_tab, lx, ly, lz);
                const int nrec = depth > K.max_bounces ? K.max_bounces : depth;
                for (int l = nrec - 1; l >= 0; --l) {
                    const lds_float* q = rec + 3 * l * 64;
                    fold_level(__float_as_int(q[0]), q[64], q[128], hit_tab, lx, ly, lz);
                }
                accumulate_frame(px, lx, ly, lz);
            }
            if (hit) {  // the hit point and normal the helper computed in S
                hit = false;
                o = mk(XF(0), XF(1), XF(2));
                hn = mk(XF(9), XF(10), XF(11));
            }
            if (mode == T_REGEN || mode == T_DIFF) {
                f3 r = random_direction(px.rs, mode == T_REGEN ? px.d0 : hn);
                if (mode == T_REGEN) {  // jittered camera ray, Main.cu:290-292
                    d = normalize3(add(px.d0, scale(K.jitter, r)));
                    o = cam;
                    depth = 0;
                    has_ray = true;
                } else {  // diffuse bounce, Main.cu:257-264: brdf = 4 * albedo (fold)
                    const float cosang = dot(r, hn);
                    if (depth < K.max_bounces) {
                        lds_float* q = rec + 3 * depth * 64;
                        q[0] = __int_as_float(hid);
                        q[64] = 0.0f;
                        q[128] = cosang;
                        d = r;
                        has_ray = true;
                    } else {
                        dcode = hid;
                        dc = cosang;
                        ended = true;
                    }
                    depth++;
                }
            }
            if (mode != T_SPEC) {  // (a SPEC lane's ray flag is the helper's)
                const int flag = has_ray ? (bvh_safe(K, o, d) ? 1 : 2) : 0;
                XF(0) = o.x;
                XF(1) = o.y;
                XF(2) = o.z;
                XF(3) = d.x;
                XF(4) = d.y;
                XF(5) = d.z;
                XF(6) = __int_as_float(flag);
            }
        } else {
            const int sf = __float_as_int(XF(22));
            if (sf & 1) {  // the owner's SPEC task, Main.cu:245-255
                Xorwow rs;
                RS_GET(rs, XF, 16);
                const f3 nrm = mk(XF(9), XF(10), XF(11));
                const f3 dd = mk(XF(3), XF(4), XF(5));  // the incoming ray
                const float4 h2 = *reinterpret_cast<const float4*>(hit_tab + RT_HIT_FLOATS * hid + 8);
                float kspec;
                const f3 r = specular_scatter(rs, dd, nrm, h2.x, h2.z, h2.y, kspec);
                XF(12) = r.x;
                XF(13) = r.y;
                XF(14) = r.z;
                XF(15) = kspec;
                RS_PUT(rs, XF, 16);
                int flag = 0;
                if (sf & 2) {  // traced: the ray from the hit point (posted in XF(0..2))
                    XF(3) = r.x;
                    XF(4) = r.y;
                    XF(5) = r.z;
                    flag = bvh_safe(K, mk(XF(0), XF(1), XF(2)), r) ? 1 : 2;
                }
                XF(6) = __int_as_float(flag);
            }
        }
        __syncthreads();

        // ---- H: SPEC take-back, closest hit halves
        float t = INFINITY;
        int id = -1;
        int rflag = 0;
        if (owner) {
            if (mode == T_SPEC) {
                const f3 r = mk(XF(12), XF(13), XF(14));
                const float kspec = XF(15);
                RS_GET(px.rs, XF, 16);
                const float cosang = dot(r, hn);  // cosAngle, Main.cu:264
                if (depth < K.max_bounces) {
                    lds_float* q = rec + 3 * depth * 64;
                    q[0] = __int_as_float(~hid);
                    q[64] = kspec;
                    q[128] = cosang;
                    d = r;
                    has_ray = true;
                } else {
                    dcode = ~hid;
                    dk = kspec;
                    dc = cosang;
                    ended = true;
                }
                depth++;
            }
            if (has_ray) {
                rflag = __float_as_int(XF(6));
                if (rflag == 1)  // (the odd indices: the owner also took its SPEC result back)
                    closest_hit_brute<QUADS, 2>(K, o, d, t, id, 1);
                else
                    closest_hit_brute<QUADS>(K, o, d, t, id);
                XF(23) = t;
                XF(24) = __int_as_float(id);
            }
        } else {
            hflag = __float_as_int(XF(6));
            if (hflag == 1) {
                closest_hit_brute<QUADS, 2>(K, mk(XF(0), XF(1), XF(2)), mk(XF(3), XF(4), XF(5)), t, id, 0);
                XF(7) = t;
                XF(8) = __int_as_float(id);
            }
        }
        __syncthreads();

        // ---- S: merge, shade, fold, post
        int live = 0;
        if (owner) {
            if (rflag == 1) {  // the helper's half: smaller distance, ties to the larger key
                const float t2 = XF(7);
                const int id2 = __float_as_int(XF(8));
                if (id2 >= 0 && (t2 < t || (t2 == t && prim_key(K, id2) > prim_key(K, id)))) {
                    t = t2;
                    id = id2;
                }
            }
            mode = T_NONE;
            if (has_ray) {
                if (id >= 0) {  // Main.cu:237-245 (the helper computes the point and normal)
                    hid = id;
                    hit = true;
                    mode = rand_range(px.rs, 1.0f) < RT_SPECULAR_CHANCE ? T_SPEC : T_DIFF;  // brdfChoice
                } else {
                    ended = true;
                }
            }
            if (ended) {
                // the fold runs in the next X phase, beside the helper's SPEC
                // tasks (the longer half of X); the deepest level waits in
                // XF(6..8), free until the owner posts its next ray there
                fold = true;
                XF(6) = __int_as_float(dcode);
                XF(7) = dk;
                XF(8) = dc;
                mode = px.passes_left > 1 ? T_REGEN : T_NONE;
            }
            int sf = 0;
            if (mode == T_SPEC) {  // the helper's task next round (its hit, normal and ray it has)
                RS_PUT(px.rs, XF, 16);
                sf = depth < K.max_bounces ? 3 : 1;  // 3: its scattered ray is traced from the hit point
            }
            XF(22) = __int_as_float(sf);
            live = __ballot(mode != T_NONE || fold) != 0ull;
            if (j == 0) *live_flag = live;
        } else if (hflag != 0) {
            // the same merge as the owner's, then the hit point and normal
            // (Main.cu:237-241; the same float operations), for the owner's
            // next X phase and the SPEC task
            float tt = XF(23);
            int ii = __float_as_int(XF(24));
            if (hflag == 1 && id >= 0 && (t < tt || (t == tt && prim_key(K, id) > prim_key(K, ii)))) {
                tt = t;
                ii = id;
            }
            if (ii >= 0) {
                const float4 h0 = *reinterpret_cast<const float4*>(hit_tab + RT_HIT_FLOATS * ii);
                const f3 hp = add(mk(XF(0), XF(1), XF(2)), scale(tt, mk(XF(3), XF(4), XF(5))));
                f3 nn = mk(h0.x, h0.y, h0.z);
                if (h0.w != 0.0f) nn = normalize3(sub(hp, nn));  // sphere normal
                XF(0) = hp.x;
                XF(1) = hp.y;
                XF(2) = hp.z;
                XF(9) = nn.x;
                XF(10) = nn.y;
                XF(11) = nn.z;
                hid = ii;
            }
        }
        __syncthreads();
        if (!owner) live = *live_flag;
        if (!live) break;  // (group-uniform)
    }
#undef XF
    if (px.valid && px.passes_left == 0 && px.frame != K.first_frame) store_pixel(K, npix, px);
    if (ORDER && tid == 0) {
        const volatile __attribute__((address_space(4))) rt_kparams* kp =
            (const volatile __attribute__((address_space(4))) rt_kparams*)__builtin_amdgcn_kernarg_segment_ptr();
        int* const ord = kp->group_order;
        unsigned* const cost = kp->group_cost;
        const long g = ord ? (long)__builtin_nontemporal_load(&ord[blockIdx.x]) : (long)blockIdx.x;
        cost[g] = (unsigned)__builtin_amdgcn_s_memrealtime() - cost[g];
    }
    diag_group_end<true>(K);
}
RT_MODE_END
