// rt_light.h — next-event estimation (rt_set_light_sampling; DESIGN.md section
// 23): the arithmetic of sampling the scene's emissive spheres at a diffuse
// bounce, shared by the HIP kernel (rt_kernel_nee.h, device pass) and the CPU
// twin (rt_cpu.cpp, host pass).  Not from the reference, which finds its lights
// by chance alone.
//
// Exact arithmetic only, written once: one rounding per operation in the
// written order (every includer is built with -ffp-contract=off), divisions
// through rt_div, roots through rt_sqrt, the angle through rt_sincos, so a GPU
// and a CPU context agree bit for bit.
//
// The estimator.  A diffuse bounce of the default estimator evaluates
// 4 albedo cos L under the uniform-hemisphere pdf 1 / 2pi (rt_path.h).  At an
// NEE LEVEL — a hit whose diffuse branch was taken, whose scattered ray will be
// traced (depth + 1 <= max_bounces) and with a non-empty light table — the part
// of that integral over one table light's cone, the light picked uniformly, is
// estimated directly:
//   direct = (n_lights * omega * cs) * (diffuse_brdf * emitted_j)
// with omega = 1 - cos(theta_max) = Omega / 2pi, wi uniform in the cone and
// cs = dot(wi, n), if the light is REACHABLE (the hit is not on it and lies
// outside it), cs > 0 and the shadow ray's closest hit is the light; else 0.
// In exchange the scattered ray of that level, when it hits a table light that
// is reachable from the level's point, drops that hit's emitted light (the
// direct term has counted it).  Emission is kept everywhere else.  Both
// estimators have the same expectation.
//
// Non-unit normals.  The reference shades planes and polygons with their
// un-normalised normal n (rt_path.h): random_direction's flip r - 2 (r.n) n of
// the lower half of its ball points is then no mirror image but stretches the
// normal component by g = 2 |n|^2 - 1, and the default estimator's expectation
// over the upper hemisphere of unit directions u becomes
//   (1 / 4pi) 4 albedo (u.n) [1 + 1 / (g q^2)] L(u),  q = 1 - un^2 + un^2 / g^2,
// un = u.n / |n| (the kept half, and the stretched half through the Jacobian of
// u = A r / |A r|, A = diag(1, 1, g)); |n| = 1 gives the 1 / 2pi above.  The
// direct term therefore takes (cs / 2) [1 + 1 / (g q^2)] in place of cs on such
// a surface; sphere normals are normalised and |n|^2 == 1 keeps cs itself.
// With |n|^2 <= 1/2 (g <= 0: the flip leaves directions below the surface) or
// NaN a hit is no NEE level.
//
// Draws at an NEE level, behind random_direction's: the light pick, u1, u2 —
// always all three, so the draws do not depend on geometry.
//
// Record of a level (four dwords): code, k, cosAngle as the default kernels',
// and aux; a diffuse level does not use k for a specular scalar, so an NEE
// level keeps n_lights * omega * cs there.
//
// Weighted picking (rt_set_light_picking, RT_LIGHT_PICK_WEIGHTED; DESIGN.md
// section 24).  The same three draws in the same order, but light j is picked
// with probability w_j / W, W the float sum of the weights in table order, and
// the direct term takes W / w_j where the uniform pick takes n_lights.  The
// weight of table light j at the level's point P (normal n):
//   w_j = 0                       if !light_reachable(P, prim, l_j, w, d2), else
//   s2 = r2 / d2,  omega_j = s2 / (1 + sqrt(1 - s2))
//   cc = (w . n) / (sqrt(d2) nl)  nl = 1 (kind 1), sqrt(n . n) (kind 2)
//   cb = max(0, cc) + sqrt(s2)    >= cos(theta_c - theta_max), the largest
//                                 cosine inside the cone; > 0 where one is
//   pw = |e.x| + |e.y| + |e.z|
//   w_j = (pw omega_j) cb         and 0 unless that is > 0 (zero, NaN, underflow)
// !(W > 0): the direct term is 0 without a shadow ray; the level stays an NEE
// level (the suppression stays on) and j is the uniform formula's.  Else j is
// the first positive-weight light whose running sum (the additions of W, in
// their order) exceeds u W, or the last positive-weight light.  The path does
// not depend on the pick: same draws, same rays, same RNG state.
//
// Polygon lights (rt_set_light_shapes, RT_LIGHT_SHAPES_ALL; DESIGN.md section
// 25; SHAPES = RT_SHAPES_ALL below).  Records [n_sphere_lights, n_lights) of the
// table are emissive triangles and quads (rt_layout.h has the record and the
// sampling block, rt_scene.cpp which polygons are admitted).  A level draws the
// same three numbers whatever the kind of the picked light.  For a polygon:
//   A = A0 + A1, t = u1 A; a quad's second half (v0, v2, v3') is taken when
//   t >= A0, with u1' = min(1, (t - A0) / A1); else the half (v0, v1, v2) with
//   u1' = min(1, t / A0)                       (a triangle: A1 = 0, always this)
//   su = sqrt(u1'), b1 = u2 su, b2 = 1 - su
//   Q = a + b1 (b - a) + b2 (c - a)            the half (a, b, c); area-uniform
//   w = Q - P, d2 = w . w, wi = normalize3(w)
//   cos_l = |n_l . w| / (|n_l| sqrt(d2))       polygons are hit from both sides
//   omega = A cos_l / (2pi d2)                 the sample's measure in the unit
//                                              of the sphere's Omega / 2pi
//   k = (inv_pick omega) wc                    wc as for a sphere
// and no shadow ray (trace = false, k = 0) unless d2 > 0, cos_l > 0, cs > 0 and
// k is finite.  The sample is visible iff the shadow ray's closest hit is the
// polygon.  A polygon light is REACHABLE from a level on primitive `prim` iff
// prim is not the polygon itself; the suppression asks the same rule, so the
// direct term integrates exactly the directions on which the scattered ray
// drops the emission.  Weighted picking weighs a polygon by the sphere formula
// on the record's bounding sphere with s2 = min(1, R^2 / d2): positive wherever
// the polygon can contribute (a point inside that sphere included).
//
// The light hierarchy (rt_set_light_hierarchy; PICK =
// RT_PICK_TREE below).  Weighted picking through a stochastic descent of the
// binary tree that rt_scene.cpp builds over the table (rt_layout.h has the
// node: bounding sphere {c, R2}, power phi, children a and b), O(depth) per
// level where the table walk is O(n).  The same three draws in the same order.
// The importance of a child reference k at the level's point P (normal n, nl as
// above, on primitive `prim`), n_lights = N:
//   k >= N - 1, the leaf of record j = k - (N - 1):
//     I = w_j, the weight above (nee_pick_weight, or nee_pick_weight_poly for a
//     polygon record): an unreachable light has I = 0
//   else, internal node k with sphere {c, R2} and power phi:
//     w = c - P, d2 = w . w
//     s2 = min(1, R2 / d2)
//     cc = (w . n) / (sqrt(d2) nl)
//     cb = max(0, cc) + sqrt(s2)            the bound of w_j, on the node's sphere
//     I = (phi / max(d2, R2)) cb            and 0 unless that is > 0
// The descent starts with the root's children (a, b), inv = 1 and the pick draw
// u, and at every level:
//   S = I_a + I_b;  !(S > 0): no pick (below)
//   t = u S;  the left child a is taken iff I_a > 0 and (t < I_a or !(I_b > 0)),
//   else the right child b; I_c the importance of the child taken
//   u = min(1, t / I_a) (left), min(1, (t - I_a) / I_b) (right): the one draw,
//       rescaled into the branch taken
//   inv = inv (S / I_c)
//   a leaf: j is its record and inv_pick = inv, where the table walk has W / w_j;
//   else (a, b) = the children of the node taken, and the next level.
// No pick (!(S > 0) at some level): the direct term is 0 without a shadow ray,
// the level stays an NEE level (the suppression stays on) and j is the uniform
// formula's, as with !(W > 0) of the table walk.  Below the root this happens
// without any underflow: a node has importance wherever its sphere is seen, its
// leaves only where they are reachable and have power (P on one leaf and inside
// its sibling; a zero-power sibling).  Every light below such a level has
// w_j = 0, so the picks that end there are lost to no light that could
// contribute; the p_j of a point then sum to less than 1.
// Unbiased: light j is picked with probability p_j = prod (I_c / S) over its
// levels, 1 / inv up to rounding, and the estimator divides by it; what has to
// hold is p_j > 0 wherever w_j > 0.  The last factor is w_j itself.  Above it,
// every ancestor's sphere contains the light's bounding sphere (rt_layout.h: in
// exact arithmetic on the stored floats), so the cone of its sphere from P
// contains the light's cone (all directions where P is inside it: s2 = 1): its
// cb bounds the largest cosine in that cone from above, so it is >= the
// light's own and > 0 (cb >= sqrt(s2) > 0 for every finite P in any case); its
// phi is a sum that holds the light's own > 0 (w_j > 0 needs pw > 0), and
// max(d2, R2) is finite.  So I > 0 on
// the whole way down, except by underflow of phi / max(d2, R2) or of the
// product with cb (and a sibling's I overflowing S, which takes phi near
// FLT_MAX).  Underflow: a child whose I rounds to 0 is not taken while its
// sibling has I > 0, and both at 0 is the no-pick rule; the lights below lose
// their direct term there and the suppression still drops their emission, a
// bias bounded by their share of the light at P, which is below 2^-126 of the
// sibling's by the definition of underflow.
// Resolution: u is a multiple of 2^-24, and a branch of probability p keeps
// 24 + log2(p) bits of it, so after the whole descent u S of the last level
// still resolves 2^-24 / p_j of the leaf: a light is reached by
// about p_j 2^24 values of u, as in the table walk's u W, whatever the depth
// (at most ceil(log2 N) + 1); lights with p_j < 2^-24 are reached by u = 0 at
// most.  Each rescaling division adds half an ulp to u, d ulps over d levels.
// Everything behind the pick is the table walk's: the cone or area sample, wc,
// the overflow guard, the record and the fold.
#pragma once
#include "rt_path.h"

// aux of a level's record
#define RT_NEE_DROP 1     // this hit's emitted light is suppressed
#define RT_NEE_LEVEL 2    // an NEE level: the fold adds the direct term (possibly 0)
#define RT_NEE_VISIBLE 4  // the direct term is not 0: the shadow ray reached light j
#define RT_NEE_JSHIFT 3   // light j from bit 3 up

namespace {

struct LightRec {
    f3 c;
    float r2;
    f3 e;
    int prim;
};

RT_HD LightRec light_load(const float* lights, int j) {
    const float4 a = *reinterpret_cast<const float4*>(lights + RT_LIGHT_FLOATS * (size_t)j);
    const float4 b = *reinterpret_cast<const float4*>(lights + RT_LIGHT_FLOATS * (size_t)j + 4);
    LightRec l;
    l.c = mk(a.x, a.y, a.z);
    l.r2 = a.w;
    l.e = mk(b.x, b.y, b.z);
    l.prim = rt_f2i(b.w);
    return l;
}

// The same record for the weight passes of weighted picking, whose index m is
// uniform across a wave: the device pass reads it through the constant address
// space, which makes the loads scalar ones (one per wave through the scalar
// data cache, no vector memory instruction).  The table is never written while
// a render kernel runs.
RT_HD LightRec light_load_uniform(const float* lights, int m) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const float cfloat;
    cfloat* p = (cfloat*)(lights + RT_LIGHT_FLOATS * (size_t)m);
    LightRec l;
    l.c = mk(p[0], p[1], p[2]);
    l.r2 = p[3];
    l.e = mk(p[4], p[5], p[6]);
    l.prim = rt_f2i(p[7]);
    return l;
#else
    return light_load(lights, m);
#endif
}

// A point P on primitive `prim` can be lit by the light through its cone: P is
// not on the light and lies outside it.  w = C - P, d2 = |w|^2.  The sampling
// and the suppression both ask this one function.
RT_HD bool light_reachable(f3 P, int prim, const LightRec& l, f3& w, float& d2) {
    w = sub(l.c, P);
    d2 = dot(w, w);
    return prim != l.prim && d2 > l.r2;
}

// The same question for a polygon light (record index >= n_sphere_lights)
RT_HD bool poly_light_reachable(f3 P, int prim, const LightRec& l, f3& w, float& d2) {
    w = sub(l.c, P);
    d2 = dot(w, w);
    return prim != l.prim;
}

// The table index of primitive `prim`, -1 if it is no table light (records are in
// primitive order: the ids ascend)
RT_HD int light_of_prim(const rt_nee_args& N, int prim) {
    int lo = 0, hi = N.n_lights - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int id = rt_f2i(N.lights[RT_LIGHT_FLOATS * (size_t)mid + 7]);
        if (id == prim) return mid;
        if (id < prim)
            lo = mid + 1;
        else
            hi = mid - 1;
    }
    return -1;
}

// Suppression: the scattered ray of an NEE level at P on `prim` hit primitive
// `id`; true when that hit's emitted light is to be dropped
template <int SHAPES = RT_SHAPES_SPHERES>
RT_HD bool light_suppressed(const rt_kparams& K, const rt_nee_args& N, f3 P, int prim, int id) {
    if constexpr (SHAPES == RT_SHAPES_SPHERES)
        if (id >= K.n_sph) return false;
    const int m = light_of_prim(N, id);
    if (m < 0) return false;
    f3 w;
    float d2;
    if constexpr (SHAPES == RT_SHAPES_ALL)
        if (m >= N.n_sphere_lights) return prim != id;
    return light_reachable(P, prim, light_load(N.lights, m), w, d2);
}

// Whether a hit with normal n can be an NEE level, and how its direct term
// weighs the cosine: 0 not at all, 1 by cs (unit normal), 2 by the stretched form
RT_HD int nee_normal_kind(bool sphere, f3 n) {
    if (sphere) return 1;
    const float s = dot(n, n);
    if (s == 1.0f) return 1;
    return s > 0.5f && s < INFINITY ? 2 : 0;
}

// The three draws of an NEE level and the sample they give at P (normal n as
// the path has it, on primitive `prim`): light j, and, when `trace`, the shadow
// ray's direction wi, the weight k = n_lights * omega * cs (kind 2: the stretched form of cs; PICK weighted:
// W / w_j in place of n_lights, see the head of this file) and the id the shadow
// ray must return.  !trace: the direct term is 0 without a shadow ray.
struct NeeSample {
    int j, prim;
    bool trace;
    float k;
    f3 wi;
};

// The weight of table light l at P (normal n of length nl, on primitive `prim`)
// under weighted picking (see the head of this file); > 0 or exactly 0
RT_HD float nee_pick_weight(const LightRec& l, f3 P, f3 n, float nl, int prim) {
    f3 w;
    float d2;
    if (!light_reachable(P, prim, l, w, d2)) return 0.0f;
    const float s2 = rt_div(l.r2, d2);
    const float omega = rt_div(s2, 1.0f + rt_sqrt(1.0f - s2));
    const float cc = rt_div(dot(w, n), rt_sqrt(d2) * nl);
    const float cb = fmaxf(0.0f, cc) + rt_sqrt(s2);
    const float pw = fabsf(l.e.x) + fabsf(l.e.y) + fabsf(l.e.z);
    const float wt = (pw * omega) * cb;
    return wt > 0.0f ? wt : 0.0f;
}

// The same weight for a polygon light, on the record's bounding sphere with
// s2 = min(1, R^2 / d2): P may lie inside that sphere and still be lit
RT_HD float nee_pick_weight_poly(const LightRec& l, f3 P, f3 n, float nl, int prim) {
    f3 w;
    float d2;
    if (!poly_light_reachable(P, prim, l, w, d2)) return 0.0f;
    const float s2 = fminf(1.0f, rt_div(l.r2, d2));
    const float omega = rt_div(s2, 1.0f + rt_sqrt(1.0f - s2));
    const float cc = rt_div(dot(w, n), rt_sqrt(d2) * nl);
    const float cb = fmaxf(0.0f, cc) + rt_sqrt(s2);
    const float pw = fabsf(l.e.x) + fabsf(l.e.y) + fabsf(l.e.z);
    const float wt = (pw * omega) * cb;
    return wt > 0.0f ? wt : 0.0f;
}

// The weight of table light m, whatever its kind (m uniform across a wave)
template <int SHAPES>
RT_HD float nee_weight_of(const rt_nee_args& N, int m, f3 P, f3 n, float nl, int prim) {
    const LightRec l = light_load_uniform(N.lights, m);
    if constexpr (SHAPES == RT_SHAPES_ALL)
        if (m >= N.n_sphere_lights) return nee_pick_weight_poly(l, P, n, nl, prim);
    return nee_pick_weight(l, P, n, nl, prim);
}

// A child of the light tree as the descent sees it (see the head of this file):
// its importance at the level's point, > 0 or exactly 0, and an internal node's
// own children (a leaf: a = its record, b = -1)
struct TreeChild {
    float imp;
    int a, b;
};

// Child reference k differs from lane to lane: vector loads of a small table
template <int SHAPES>
RT_HD TreeChild tree_child(const rt_nee_args& N, int k, f3 P, f3 n, float nl, int prim) {
    TreeChild c;
    const int j = k - (N.n_lights - 1);
    if (j >= 0) {
        const LightRec l = light_load(N.lights, j);
        [[maybe_unused]] bool poly = false;
        if constexpr (SHAPES == RT_SHAPES_ALL) poly = j >= N.n_sphere_lights;
        c.imp = poly ? nee_pick_weight_poly(l, P, n, nl, prim) : nee_pick_weight(l, P, n, nl, prim);
        c.a = j;
        c.b = -1;
        return c;
    }
    const float4 s = *reinterpret_cast<const float4*>(N.tree + RT_LIGHT_NODE_FLOATS * (size_t)k);
    const float4 q = *reinterpret_cast<const float4*>(N.tree + RT_LIGHT_NODE_FLOATS * (size_t)k + 4);
    const f3 w = sub(mk(s.x, s.y, s.z), P);
    const float d2 = dot(w, w);
    const float s2 = fminf(1.0f, rt_div(s.w, d2));
    const float cc = rt_div(dot(w, n), rt_sqrt(d2) * nl);
    const float cb = fmaxf(0.0f, cc) + rt_sqrt(s2);
    const float imp = rt_div(q.x, fmaxf(d2, s.w)) * cb;
    c.imp = imp > 0.0f ? imp : 0.0f;
    c.a = rt_f2i(q.y);
    c.b = rt_f2i(q.z);
    return c;
}

// The descent (see the head of this file): true with the leaf's record j and
// inv = 1 / (the probability of ending there), false where some level has no
// importance (j and inv are then not to be used).  FORCED, for
// nee_pick_probabilities: no draw; bit i of `path` takes the right child at
// level i, and a child of importance 0 on the way is no pick either.  One loop
// with one live node; the children of the node taken come with its importance.
template <int SHAPES, bool FORCED = false>
RT_HD bool tree_descend(const rt_nee_args& N, f3 P, f3 n, float nl, int prim, float u, unsigned long long path, int& j,
                        float& inv) {
    const float4 root = *reinterpret_cast<const float4*>(N.tree + 4);
    int a = rt_f2i(root.y), b = rt_f2i(root.z);
    inv = 1.0f;
    while (true) {
        const TreeChild l = tree_child<SHAPES>(N, a, P, n, nl, prim);
        const TreeChild r = tree_child<SHAPES>(N, b, P, n, nl, prim);
        const float S = l.imp + r.imp;
        if (!(S > 0.0f)) return false;
        const float t = u * S;
        bool left = l.imp > 0.0f && (t < l.imp || !(r.imp > 0.0f));
        if constexpr (FORCED) {
            left = !(path & 1ull);
            path >>= 1;
        }
        const float ic = left ? l.imp : r.imp;
        if constexpr (FORCED)
            if (!(ic > 0.0f)) return false;
        u = fminf(1.0f, rt_div(left ? t : t - l.imp, ic));
        inv = inv * rt_div(S, ic);
        const int k = left ? a : b;
        if (k >= N.n_lights - 1) {
            j = k - (N.n_lights - 1);
            return true;
        }
        a = left ? l.a : r.a;
        b = left ? l.b : r.b;
    }
}

// rt_light_pick_probabilities: the probability with which an NEE level at P
// (normal n, on primitive `prim`, a sphere's or not) picks each table light
// under N.pick, out[0 .. n_lights), from the functions nee_sample picks with:
// 1 / n (uniform), w_j / W (weighted), 1 / inv of the descent forced to light
// j's leaf (tree).  All 0 where the pick rule gives no direct term (!(W > 0),
// no pick), and where a hit with this normal is no NEE level.
template <int SHAPES>
RT_HD void nee_pick_probabilities(const rt_nee_args& N, f3 P, f3 n, int prim, bool sphere, float* out) {
    const int kind = nee_normal_kind(sphere, n);
    const float nl = kind == 2 ? rt_sqrt(dot(n, n)) : 1.0f;
    float W = 0.0f;
    if (kind && N.pick == RT_PICK_WEIGHTED)
        for (int m = 0; m < N.n_lights; m++) W = W + nee_weight_of<SHAPES>(N, m, P, n, nl, prim);
    for (int m = 0; m < N.n_lights; m++) {
        float p = 0.0f;
        if (!kind) {
        } else if (N.pick == RT_PICK_TREE) {
            // the way to leaf m, read upwards: bit 0 ends as the root's branch
            unsigned long long path = 0ull;
            int k = N.n_lights - 1 + m;
            for (int up = rt_f2i(N.tree[RT_LIGHT_NODE_FLOATS * (size_t)k + 7]); up >= 0;
                 up = rt_f2i(N.tree[RT_LIGHT_NODE_FLOATS * (size_t)k + 7])) {
                path = (path << 1) | (rt_f2i(N.tree[RT_LIGHT_NODE_FLOATS * (size_t)up + 6]) == k ? 1ull : 0ull);
                k = up;
            }
            int j;
            float inv;
            if (tree_descend<SHAPES, true>(N, P, n, nl, prim, 0.0f, path, j, inv)) p = rt_div(1.0f, inv);
        } else if (N.pick == RT_PICK_WEIGHTED) {
            if (W > 0.0f) p = rt_div(nee_weight_of<SHAPES>(N, m, P, n, nl, prim), W);
        } else {
            p = rt_div(1.0f, (float)N.n_lights);
        }
        out[m] = p;
    }
}

// The direction towards a polygon light's area sample (see the head of this
// file; q: the light's sampling block): wi and the sample's measure omega;
// false: not reachable, or the sample cannot contribute (d2 or cos_l not > 0)
RT_HD bool nee_poly_dir(const float* q, int lprim, f3 P, int prim, float u1, float u2, f3& wi, float& omega) {
    if (prim == lprim) return false;
    const float4 q0 = *reinterpret_cast<const float4*>(q);
    const float4 q1 = *reinterpret_cast<const float4*>(q + 4);
    const float4 q2 = *reinterpret_cast<const float4*>(q + 8);
    const float4 q3 = *reinterpret_cast<const float4*>(q + 12);
    const float4 q4 = *reinterpret_cast<const float4*>(q + 16);
    const f3 a = mk(q0.x, q0.y, q0.z);
    f3 b = mk(q1.x, q1.y, q1.z), c = mk(q2.x, q2.y, q2.z);
    const float a0 = q0.w, a1 = q1.w, nl = q2.w;
    const float area = a0 + a1;
    const float t = u1 * area;
    float uh;
    if (a1 > 0.0f && t >= a0) {
        b = c;
        c = mk(q3.x, q3.y, q3.z);
        uh = rt_div(t - a0, a1);
    } else {
        uh = rt_div(t, a0);
    }
    const float su = rt_sqrt(fminf(1.0f, uh));
    const float b1 = u2 * su, b2 = 1.0f - su;
    const f3 Q = add(add(a, scale(b1, sub(b, a))), scale(b2, sub(c, a)));
    const f3 w = sub(Q, P);
    const float d2 = dot(w, w);
    if (!(d2 > 0.0f)) return false;
    const float cl = rt_div(fabsf(dot(mk(q4.x, q4.y, q4.z), w)), nl * rt_sqrt(d2));
    if (!(cl > 0.0f)) return false;
    omega = rt_div(area * cl, (2.0f * RT_PI) * d2);
    wi = normalize3(w);
    return true;
}

template <int PICK, int SHAPES = RT_SHAPES_SPHERES>
RT_HD NeeSample nee_sample(Xorwow& rs, const rt_nee_args& N, f3 P, f3 n, int prim, int kind) {
    const float u = rand_range(rs, 1.0f);
    const float u1 = rand_range(rs, 1.0f);
    const float u2 = rand_range(rs, 1.0f);
    const float nf = (float)N.n_lights;
    NeeSample s;
    s.j = (int)(u * nf);
    if (s.j > N.n_lights - 1) s.j = N.n_lights - 1;
    s.trace = false;
    s.k = 0.0f;
    s.wi = mk(0.0f, 0.0f, 0.0f);
    // what multiplies omega * cs: 1 / (the probability of picking light j)
    float inv_pick = nf;
    if constexpr (PICK == RT_PICK_WEIGHTED) {
        // two passes over the table, the index uniform across a wave; the
        // second one computes the same weights again (the same expressions
        // give the same bits), so none is kept anywhere
        const float nl = kind == 2 ? rt_sqrt(dot(n, n)) : 1.0f;
        float W = 0.0f;
        for (int m = 0; m < N.n_lights; m++) W = W + nee_weight_of<SHAPES>(N, m, P, n, nl, prim);
        if (!(W > 0.0f)) {
            s.prim = -1;
            return s;
        }
        const float target = u * W;
        float run = 0.0f, wj = 0.0f;
        for (int m = 0; m < N.n_lights; m++) {
            const float wt = nee_weight_of<SHAPES>(N, m, P, n, nl, prim);
            if (wt > 0.0f) {
                run = run + wt;
                s.j = m;
                wj = wt;
                if (run > target) break;
            }
        }
        inv_pick = rt_div(W, wj);
    }
    if constexpr (PICK == RT_PICK_TREE) {
        const float nl = kind == 2 ? rt_sqrt(dot(n, n)) : 1.0f;
        int jt;
        if (!tree_descend<SHAPES>(N, P, n, nl, prim, u, 0ull, jt, inv_pick)) {
            s.prim = -1;
            return s;
        }
        s.j = jt;
    }
    const LightRec l = light_load(N.lights, s.j);
    s.prim = l.prim;
    float omega;
    f3 wi;  // the sample's direction: s.wi only once the sample stands (no sample: k and wi stay 0)
    [[maybe_unused]] bool poly = false;
    if constexpr (SHAPES == RT_SHAPES_ALL) poly = s.j >= N.n_sphere_lights;
    // (the two kinds meet in one wave: what follows the direction is written once)
    if (poly) {
        if (!nee_poly_dir(N.poly + RT_POLY_LIGHT_FLOATS * (size_t)(s.j - N.n_sphere_lights), l.prim, P, prim, u1, u2, wi, omega))
            return s;
    } else {
        f3 w;
        float d2;
        if (!light_reachable(P, prim, l, w, d2)) return s;
        const float s2 = rt_div(l.r2, d2);
        const float cm = rt_sqrt(1.0f - s2);
        omega = rt_div(s2, 1.0f + cm);  // 1 - cos(theta_max) without the cancellation
        // cos and sin of the polar angle from t = 1 - cos: 1 - ct * ct would cancel for a small light
        // (at s2 = 1e-6 it leaves nine distinct sines), t (2 - t) keeps every bit of t; t <= omega <= 1
        const float t = u1 * omega;
        const float ct = 1.0f - t;
        const float st = rt_sqrt(t * (2.0f - t));
        const float phi = 2.0f * RT_PI * u2;
        float sp, cp;
        rt_sincos(phi, sp, cp);
        const f3 loc = mk(st * cp, st * sp, ct);
        // frame around the axis, combined as specular_scatter combines its own; the
        // tangents here are orthonormal (a cone-uniform wi of unit length needs
        // them so: specular_scatter's cross products are not normalised, and its
        // helper axis is parallel to a y-aligned normal)
        const f3 a = normalize3(w);
        f3 some = mk(1.0f, 0.0f, 0.0f);
        if (fabsf(a.x) > 0.9f) some = mk(0.0f, 1.0f, 0.0f);
        const f3 t1 = normalize3(cross(a, some));
        const f3 t2 = cross(a, t1);
        wi = mk(dot(mk(t1.x, t2.x, a.x), loc), dot(mk(t1.y, t2.y, a.y), loc), dot(mk(t1.z, t2.z, a.z), loc));
    }
    const float cs = dot(wi, n);
    if (!(cs > 0.0f)) return s;
    float wc = cs;
    if (kind == 2) {
        const float nn = dot(n, n);
        const float g = 2.0f * nn - 1.0f;
        const float un2 = rt_div(cs * cs, nn);
        const float q = (1.0f - un2) + rt_div(un2, g * g);
        wc = (0.5f * cs) * (1.0f + rt_div(1.0f, g * (q * q)));
    }
    s.k = (inv_pick * omega) * wc;
    if constexpr (SHAPES == RT_SHAPES_ALL) {
        // a polygon's omega has no bound (d2 -> 0): an overflown k is no sample
        if (poly && !(s.k < INFINITY)) {
            s.k = 0.0f;
            return s;
        }
    }
    s.wi = wi;
    s.trace = true;
    return s;
}

// fold_level (rt_path.h) with the level's aux: innermost-first
//   L = (keep ? emitted : 0) [+ direct] + (brdf * L) * cosAngle
// aux = 0 is fold_level's own expression.
RT_HD void fold_level_nee(int c0, float k, float c, int aux, const float* hit_tab, const rt_nee_args& N, float& lx,
                          float& ly, float& lz) {
    const bool spec = c0 < 0;
    const float* h = hit_tab + RT_HIT_FLOATS * (spec ? ~c0 : c0);
    const float4 e = *reinterpret_cast<const float4*>(h + 4);
    const float4 da = *reinterpret_cast<const float4*>(h + 12);
    const float bx = spec ? k : da.x, by = spec ? k : da.y, bz = spec ? k : da.z;
    float ex = e.x, ey = e.y, ez = e.z;
    if (aux & RT_NEE_DROP) ex = ey = ez = 0.0f;
    if (aux & RT_NEE_LEVEL) {
        float dx = 0.0f, dy = 0.0f, dz = 0.0f;
        if (aux & RT_NEE_VISIBLE) {
            const float4 le = *reinterpret_cast<const float4*>(N.lights + RT_LIGHT_FLOATS * (size_t)(aux >> RT_NEE_JSHIFT) + 4);
            dx = k * (da.x * le.x);
            dy = k * (da.y * le.y);
            dz = k * (da.z * le.z);
        }
        ex = ex + dx;
        ey = ey + dy;
        ez = ez + dz;
    }
    lx = ex + (bx * lx) * c;
    ly = ey + (by * ly) * c;
    lz = ez + (bz * lz) * c;
}

}  // namespace
