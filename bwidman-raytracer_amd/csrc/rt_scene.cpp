// rt_scene.cpp — the host scene compiler (rt_scene.h).
//
// Host-side replacement of the reference's allocateScene (Main.cu:38-109): every quantity the
// reference recomputes per ray but that depends only on the primitive is
// computed here once, and large scenes get a BVH.
//
// Compiled with -ffp-contract=off: the compilation uses the reference's float
// operations in the reference's order, so the kernel sees bit-identical
// inputs.  The caller holds the IEEE float state (rt_set_scene: HostFpEnv).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_scene.h"

struct float4;  // rt_layout.h names them in pointer members only; no HIP header here
struct float2;
struct uint2;
#include "rt_layout.h"

namespace {

struct V3 {
    float x, y, z;
};
V3 v3(const rt_vec3& a) { return {a.x, a.y, a.z}; }
V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross(V3 a, V3 b) {  // Math.cuh:103-108
    float i = a.y * b.z - a.z * b.y;
    float j = -(a.x * b.z - a.z * b.x);
    float k = a.x * b.y - a.y * b.x;
    return {i, j, k};
}

void put_material(float* h, const rt_material& m) {
    // emittedLight = emittance * albedo (Main.cu:238)
    h[4] = m.emittance * m.albedo.x;
    h[5] = m.emittance * m.albedo.y;
    h[6] = m.emittance * m.albedo.z;
    h[7] = m.albedo.x;  // slots 7, 11, 15: the raw albedo (aov_shade; no render kernel reads these lanes)
    h[8] = m.roughness;
    // fresnel(): square(ior)/square(1.0f) - 1.0f (Main.cu:125)
    h[9] = (m.refractive_index * m.refractive_index) / (1.0f * 1.0f) - 1.0f;
    h[10] = m.roughness * m.roughness;  // Main.cu:119 evaluates roughness*roughness first
    h[11] = m.albedo.y;
    // diffuse brdf = 2 / (1 - specularChance) * albedo (Main.cu:259): the
    // double constant narrows to 4.0f; scaling by 4 is exact
    const float dk = (float)(2.0 / (1 - 0.5f));
    h[12] = dk * m.albedo.x;
    h[13] = dk * m.albedo.y;
    h[14] = dk * m.albedo.z;
    h[15] = m.albedo.z;
}

// Triangle / quad record: {n, d, v0, in0, v1, in1, ...}; Intersection.cuh:109-127
// Cull sphere of a triangle, used by polygon_test to skip the exact test for
// rays whose LINE passes farther than Rc from the centre.  Such a ray's
// plane hit P (as the reference computes it, with float rounding) is at
// least Rc - R from the triangle; outside a triangle with smallest angle
// alpha some edge function dot(in_k, P - v_k) is then below
// -|in_k| * (Rc - R) * sin(alpha / 2), and the inflation
//   Rc = R (1 + 2^-20) + 2^-14 * scale / (0.25 sin alpha)
// (scale >= every coordinate of the scene and of any culled ray origin)
// keeps that margin > 2^-14 * scale, several hundred times the rounding of
// the reference's P = o + t d and of its edge dots (~2^-21 * scale).  So the
// reference rejects every culled triangle.  Degenerate/skinny triangles
// (sin alpha < 2^-10) and quads (possibly non-convex / non-planar) are never
// culled (Rc^2 = inf).
void cull_sphere(float* cs, const rt_vec3* verts, int nv, double scale) {
    cs[0] = cs[1] = cs[2] = 0.0f;
    cs[3] = INFINITY;
    if (nv != 3) return;
    double v[3][3];
    for (int k = 0; k < 3; k++) {
        v[k][0] = verts[k].x;
        v[k][1] = verts[k].y;
        v[k][2] = verts[k].z;
    }
    double c[3], r = 0.0, min_sin = 1.0;
    for (int a = 0; a < 3; a++) c[a] = (v[0][a] + v[1][a] + v[2][a]) / 3.0;
    for (int k = 0; k < 3; k++) {
        double d2 = 0.0, e1[3], e2[3], l1 = 0.0, l2 = 0.0, dp = 0.0;
        for (int a = 0; a < 3; a++) {
            d2 += (v[k][a] - c[a]) * (v[k][a] - c[a]);
            e1[a] = v[(k + 1) % 3][a] - v[k][a];
            e2[a] = v[(k + 2) % 3][a] - v[k][a];
            l1 += e1[a] * e1[a];
            l2 += e2[a] * e2[a];
            dp += e1[a] * e2[a];
        }
        r = std::max(r, std::sqrt(d2));
        const double cosang = (l1 > 0.0 && l2 > 0.0) ? dp / std::sqrt(l1 * l2) : 1.0;
        min_sin = std::min(min_sin, std::sqrt(std::max(0.0, 1.0 - cosang * cosang)));
    }
    if (!(min_sin >= 1.0 / 1024.0) || !std::isfinite(r) || !std::isfinite(scale)) return;
    const double rc = r * (1.0 + std::ldexp(1.0, -20)) + std::ldexp(1.0, -14) * scale / (0.25 * min_sin);
    const double rc2 = rc * rc * (1.0 + std::ldexp(1.0, -20));
    if (!(rc2 < 1e30)) return;
    cs[0] = (float)c[0];
    cs[1] = (float)c[1];
    cs[2] = (float)c[2];
    cs[3] = (float)rc2;
}

void compile_polygon(float* q, float* h, const rt_vec3* verts, int nv, const rt_material& m, double scale) {
    V3 v[4], e[4];
    for (int k = 0; k < nv; k++) v[k] = v3(verts[k]);
    for (int k = 0; k < nv; k++) e[k] = sub(v[(k + 1) % nv], v[k]);
    V3 n = cross(e[0], e[1]);   // plane {v0, {e0, e1}}: normal = cross(d0, d1)
    float d = -dot(n, v[0]);    // Intersection.cuh:83
    q[0] = n.x;
    q[1] = n.y;
    q[2] = n.z;
    q[3] = d;
    for (int k = 0; k < nv; k++) {
        V3 in = cross(n, e[k]);  // Intersection.cuh:125-127
        float* r = q + RT_POLY_EDGES + 6 * k;
        r[0] = v[k].x;
        r[1] = v[k].y;
        r[2] = v[k].z;
        r[3] = in.x;
        r[4] = in.y;
        r[5] = in.z;
    }
    h[0] = n.x;
    h[1] = n.y;
    h[2] = n.z;
    h[3] = 0.0f;
    put_material(h, m);
    // cull sphere (centre, Rc^2), appended after the edge data
    float* cs = q + (nv == 3 ? RT_TRI_CULL : RT_QUAD_CULL);
    cull_sphere(cs, verts, nv, scale);
}

// The light-table record and the sampling block (rt_layout.h rt_nee_args) of
// polygon `id`, whose hit-table row is h; false: the polygon is not admissible
// and stays an emitter that paths find by chance (always unbiased).
// Admissible: emittance finite and > 0, every vertex finite, the compiled
// normal n = cross(e0, e1) with finite |n|^2 > 0, both halves of positive area,
// and for a quad convexity of what polygon_test accepts.  That test intersects
// the plane through v0 with normal n and asks dot(cross(n, e_k), P - v_k) >= 0
// of every edge: the accepted region is the quad projected along n into that
// plane, and it is the projected quad itself exactly when every projected
// vertex passes every edge's test.  Checked here in double on v0, v1, v2 and
// v3' (v3 projected); vertex j against edge k for j = k and j = k + 1 is on the
// edge's line identically (0 up to rounding) and is not asked.
bool polygon_light(const float* h, const rt_vec3* verts, int nv, const rt_material& m, int id, float* rec, float* blk) {
    if (!(std::isfinite(m.emittance) && m.emittance > 0.0f)) return false;
    double v[4][3];
    for (int k = 0; k < nv; k++) {
        if (!(std::isfinite(verts[k].x) && std::isfinite(verts[k].y) && std::isfinite(verts[k].z))) return false;
        v[k][0] = verts[k].x;
        v[k][1] = verts[k].y;
        v[k][2] = verts[k].z;
    }
    const float nn = h[0] * h[0] + h[1] * h[1] + h[2] * h[2];
    if (!(std::isfinite(nn) && nn > 0.0f)) return false;
    const double n[3] = {h[0], h[1], h[2]};
    auto dot3 = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    auto cross3 = [](const double* a, const double* b, double* c) {
        c[0] = a[1] * b[2] - a[2] * b[1];
        c[1] = a[2] * b[0] - a[0] * b[2];
        c[2] = a[0] * b[1] - a[1] * b[0];
    };
    auto diff = [](const double* a, const double* b, double* c) {
        for (int i = 0; i < 3; i++) c[i] = a[i] - b[i];
    };
    auto half_area = [&](const double* a, const double* b, const double* c) {
        double p[3], q[3], x[3];
        diff(b, a, p);
        diff(c, a, q);
        cross3(p, q, x);
        return 0.5 * std::sqrt(dot3(x, x));
    };
    double v3p[3] = {v[2][0], v[2][1], v[2][2]};  // a triangle: v2 again
    if (nv == 4) {
        double w[3];
        diff(v[3], v[0], w);
        const double s = dot3(n, w) / dot3(n, n);
        for (int i = 0; i < 3; i++) v3p[i] = v[3][i] - s * n[i];
        const double* pv[4] = {v[0], v[1], v[2], v3p};
        for (int k = 0; k < 4; k++) {
            double e[3], in[3];
            diff(pv[(k + 1) % 4], pv[k], e);
            cross3(n, e, in);
            for (int j = 0; j < 4; j++) {
                if (j == k || j == (k + 1) % 4) continue;
                double w2[3];
                diff(pv[j], pv[k], w2);
                if (!(dot3(in, w2) >= 0.0)) return false;
            }
        }
    }
    const float a0 = (float)half_area(v[0], v[1], v[2]);
    const float a1 = nv == 4 ? (float)half_area(v[0], v[2], v3p) : 0.0f;
    if (!(std::isfinite(a0) && a0 > 0.0f) || (nv == 4 && !(std::isfinite(a1) && a1 > 0.0f))) return false;
    if (!std::isfinite(a0 + a1)) return false;
    if (!(std::isfinite((float)v3p[0]) && std::isfinite((float)v3p[1]) && std::isfinite((float)v3p[2]))) return false;
    const float nl = std::sqrt(nn);
    // bounding sphere: the vertices' mean and the largest distance from it (as
    // rounded to float), to the original and the projected vertices
    double c[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < nv; k++)
        for (int i = 0; i < 3; i++) c[i] += v[k][i] / nv;
    const float cf[3] = {(float)c[0], (float)c[1], (float)c[2]};
    double r2 = 0.0;
    auto reach = [&](const double* p) {
        double d2 = 0.0;
        for (int i = 0; i < 3; i++) d2 += (p[i] - (double)cf[i]) * (p[i] - (double)cf[i]);
        r2 = std::max(r2, d2);
    };
    for (int k = 0; k < nv; k++) reach(v[k]);
    reach(v3p);
    float r2f = (float)(r2 * (1.0 + std::ldexp(1.0, -20)));
    if (!((double)r2f >= r2)) r2f = std::nextafter(r2f, INFINITY);
    if (!(std::isfinite(cf[0]) && std::isfinite(cf[1]) && std::isfinite(cf[2]) && std::isfinite(r2f) && r2f > 0.0f)) return false;
    rec[0] = cf[0];
    rec[1] = cf[1];
    rec[2] = cf[2];
    rec[3] = r2f;
    rec[4] = h[4];
    rec[5] = h[5];
    rec[6] = h[6];
    std::memcpy(&rec[7], &id, 4);
    const float b[RT_POLY_LIGHT_FLOATS] = {verts[0].x, verts[0].y, verts[0].z, a0,  verts[1].x, verts[1].y, verts[1].z, a1,
                                           verts[2].x, verts[2].y, verts[2].z, nl,  (float)v3p[0], (float)v3p[1], (float)v3p[2], 0.0f,
                                           h[0], h[1], h[2], 0.0f};
    std::memcpy(blk, b, sizeof b);
    return true;
}

// ---- the light tree (rt_layout.h RT_LIGHT_NODE_FLOATS; rt_set_light_hierarchy) ----
// A binary tree over records [0, n) of the light table, n >= 2.  A node's
// records are sorted along each axis by their centres (ties and non-finite
// centres by table index, so the build is deterministic) and split where
//   phi_left area_left + phi_right area_right
// is smallest over the three axes and the admissible positions: phi the summed
// leaf power of a side, area the surface of the box around its spheres — what
// Conty Estevez and Kulla's heuristic keeps of the surface-area heuristic when
// emitters have no orientation.  Admissible: both sides fit the depth that is
// left, 2^(budget - 1) records each, the root's budget being
// ceil(log2 n) + 1 levels; so no leaf lies deeper than that.  Internal nodes
// are numbered in preorder, the root 0; the bounds are merged on the way back
// up, in double on the children's stored floats, and rounded outwards.
struct LightTreeBuild {
    const float* lights;
    int n;
    float* out;  // (2n - 1) * RT_LIGHT_NODE_FLOATS, the leaves filled in
    int next = 0;
    std::vector<char> ok;  // the node's sphere is finite
};

void light_tree_put_int(float* slot, int v) { std::memcpy(slot, &v, 4); }

struct LightBox {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, phi = 0.0;
    void add(const float* node) {  // a leaf node with a finite sphere
        const double r = std::sqrt((double)node[3]);
        for (int a = 0; a < 3; a++) {
            lo[a] = std::min(lo[a], node[a] - r);
            hi[a] = std::max(hi[a], node[a] + r);
        }
        phi += node[4];
    }
    double cost() const {
        if (!(hi[0] >= lo[0])) return 0.0;  // empty
        const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
        return phi * (2.0 * (x * y + y * z + z * x));
    }
};

int light_tree_node(LightTreeBuild& B, int* idx, int count, int parent, int budget) {
    if (count == 1) {
        const int k = B.n - 1 + idx[0];
        light_tree_put_int(B.out + (size_t)RT_LIGHT_NODE_FLOATS * k + 7, parent);
        return k;
    }
    const int k = B.next++;
    auto leaf = [&](int j) { return B.out + (size_t)RT_LIGHT_NODE_FLOATS * ((size_t)B.n - 1 + j); };
    const long cap = 1L << (budget - 1);  // records a side may hold
    const int first = (int)std::max(1L, (long)count - cap), last = (int)std::min((long)count - 1, cap);
    std::vector<int> order(idx, idx + count);
    std::vector<double> right((size_t)count + 1);
    // (key, table index) is a total order: sorting again along an axis gives the same sequence
    auto sort_along = [&](int axis) {
        auto key = [&](int j) { return B.ok[(size_t)B.n - 1 + j] ? leaf(j)[axis] : INFINITY; };
        std::sort(order.begin(), order.end(), [&](int p, int q) {
            const float kp = key(p), kq = key(q);
            return kp < kq || (kp == kq && p < q);
        });
    };
    int half = (count + 1) / 2, best_axis = -1;  // (no finite cost anywhere: the median in table order)
    double best = INFINITY;
    for (int axis = 0; axis < 3; axis++) {
        sort_along(axis);
        LightBox r;
        right[(size_t)count] = 0.0;
        for (int i = count - 1; i >= 1; i--) {
            if (B.ok[(size_t)B.n - 1 + order[i]]) r.add(leaf(order[i]));
            right[(size_t)i] = r.cost();
        }
        LightBox l;
        for (int i = 1; i <= last; i++) {  // i records on the left
            if (B.ok[(size_t)B.n - 1 + order[i - 1]]) l.add(leaf(order[i - 1]));
            const double c = l.cost() + right[(size_t)i];
            if (i >= first && c < best) {
                best = c;
                half = i;
                best_axis = axis;
            }
        }
    }
    if (best_axis >= 0) {
        sort_along(best_axis);
        std::copy(order.begin(), order.end(), idx);
    }
    const int a = light_tree_node(B, idx, half, k, budget - 1);
    const int b = light_tree_node(B, idx + half, count - half, k, budget - 1);
    float* nd = B.out + (size_t)RT_LIGHT_NODE_FLOATS * k;
    const float* na = B.out + (size_t)RT_LIGHT_NODE_FLOATS * a;
    const float* nb = B.out + (size_t)RT_LIGHT_NODE_FLOATS * b;
    float sph[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool ok = B.ok[a] || B.ok[b];
    if (B.ok[a] && B.ok[b]) {
        // the smallest sphere around both, its centre rounded to float; then the
        // radius that reaches both children from that centre
        double ca[3], cb[3], d2 = 0.0;
        for (int i = 0; i < 3; i++) {
            ca[i] = na[i];
            cb[i] = nb[i];
            d2 += (cb[i] - ca[i]) * (cb[i] - ca[i]);
        }
        const double d = std::sqrt(d2), ra = std::sqrt((double)na[3]), rb = std::sqrt((double)nb[3]);
        double t = 0.0;  // the centre at ca + t (cb - ca)
        if (d + rb <= ra)
            t = 0.0;
        else if (d + ra <= rb)
            t = 1.0;
        else
            t = (0.5 * (d + ra + rb) - ra) / d;
        double da2 = 0.0, db2 = 0.0;
        for (int i = 0; i < 3; i++) {
            sph[i] = (float)(ca[i] + t * (cb[i] - ca[i]));
            da2 += ((double)sph[i] - ca[i]) * ((double)sph[i] - ca[i]);
            db2 += ((double)sph[i] - cb[i]) * ((double)sph[i] - cb[i]);
        }
        const double R = std::max(std::sqrt(da2) + ra, std::sqrt(db2) + rb);
        const double R2 = R * R * (1.0 + std::ldexp(1.0, -20));
        float r2f = (float)R2;
        if (!((double)r2f >= R2)) r2f = std::nextafter(r2f, INFINITY);
        sph[3] = std::isfinite(r2f) ? r2f : 3.4028234663852886e38f;  // (coordinates beyond float's square root)
    } else if (ok) {
        std::memcpy(sph, B.ok[a] ? na : nb, sizeof sph);
    }
    B.ok[k] = ok;
    std::memcpy(nd, sph, sizeof sph);
    nd[4] = na[4] + nb[4];
    light_tree_put_int(nd + 5, a);
    light_tree_put_int(nd + 6, b);
    light_tree_put_int(nd + 7, parent);
    return k;
}

// polys: the sampling blocks of records [n_sphere_lights, ...)
void build_light_tree(const float* lights, const float* polys, int n_sphere_lights, int n, std::vector<float>& out) {
    out.clear();
    if (n < 2) return;
    out.assign((size_t)(2 * n - 1) * RT_LIGHT_NODE_FLOATS, 0.0f);
    LightTreeBuild B{lights, n, out.data()};
    B.ok.assign((size_t)2 * n - 1, 0);
    std::vector<int> idx((size_t)n);
    for (int j = 0; j < n; j++) {
        idx[j] = j;
        const float* l = lights + (size_t)RT_LIGHT_FLOATS * j;
        float* nd = out.data() + (size_t)RT_LIGHT_NODE_FLOATS * (n - 1 + j);
        std::memcpy(nd, l, 4 * sizeof(float));
        const float pw = std::fabs(l[4]) + std::fabs(l[5]) + std::fabs(l[6]);
        float phi;
        if (j < n_sphere_lights) {
            phi = pw * l[3];
        } else {
            const float* q = polys + (size_t)RT_POLY_LIGHT_FLOATS * (j - n_sphere_lights);
            phi = (pw * (q[3] + q[7])) / RT_PI;
        }
        const bool ok = std::isfinite(l[0]) && std::isfinite(l[1]) && std::isfinite(l[2]) && std::isfinite(l[3]) && std::isfinite(phi);
        B.ok[(size_t)n - 1 + j] = ok;
        nd[4] = ok ? phi : 0.0f;
        light_tree_put_int(nd + 5, j);
        light_tree_put_int(nd + 6, -1);
    }
    int budget = 1;  // ceil(log2 n) + 1
    while ((1L << (budget - 1)) < n) budget++;
    light_tree_node(B, idx.data(), n, -1, budget);
}

// ---- BVH over spheres / triangles / quads (large scenes) -------------------
// Binned-SAH binary tree, emitted as EIGHT threaded (stackless) node arrays,
// one per ray-direction octant: in array k the children of every node are
// laid out near side of the node's split axis first for that octant, each
// node holding its "miss" link (next node once the subtree is skipped).  A
// lane walks the array of its ray's octant, so boxes come front to back
// along every split and the running closest hit prunes the rest
// (multiple-threaded BVH).  Boxes are inflated by 1e-3 + 1e-4 * |coordinate|
// — orders of magnitude beyond the rounding of the reference's hit tests —
// so every hit the reference can accept lies inside its leaf's box.
struct BvhItem {
    float lo[3], hi[3], c[3];
    int id;
};

struct BvhNode {
    float lo[3], hi[3];
    int left = -1, right = -1;  // children (internal)
    int axis = 0;               // split axis (internal): left child holds the smaller centroids
    int first = 0, count = 0;   // prims range (leaf)
};

struct BvhBuilder {
    static constexpr int kBins = 16;
    int max_leaf = 8;         // BWRT_BVH_LEAF
    float trav_cost = 0.0f;   // BWRT_BVH_CT: SAH cost of one node step relative to one primitive test
    int order_mask = 7;       // octant bits that get their own node array (set from the scene extents; BWRT_BVH_ORDER_MASK)
    std::vector<BvhItem> items;
    std::vector<BvhNode> tree;
    std::vector<int> prims;
    std::vector<float> nodes;  // 8 orders x n_nodes x 8 floats
    // the same threaded arrays as 16-byte nodes (rt_layout.h bvh_nodes16):
    // boxes in fp16 rounded outward; n16 = every box fits the fp16 range
    std::vector<uint32_t> nodes16;  // 8 orders x n_nodes x 4 words
    bool n16 = false;
    int n_nodes = 0;

    // fp16 bits of the largest half <= v (down) or the smallest half >= v
    // (up); false if |v| exceeds the finite fp16 range
    static bool half_bound(float v, bool up, uint16_t& out) {
        if (!(std::fabs(v) <= 65504.0f)) return false;
        if (std::fabs(v) < 6.103515625e-05f) {  // below the smallest normal: +-2^-14
            out = up ? 0x0400 : 0x8400;
            return true;
        }
        uint32_t f;
        std::memcpy(&f, &v, 4);
        const uint32_t sign = (f >> 16) & 0x8000u;
        const int e = (int)((f >> 23) & 0xff) - 127 + 15;  // 1..30 here
        uint32_t m = (f >> 13) & 0x3ffu;                   // truncated toward zero
        uint16_t h = (uint16_t)(sign | ((uint32_t)e << 10) | m);
        const bool inexact = (f & 0x1fffu) != 0;
        // truncation moved |v| down: step one ulp outward when that is the wrong way
        if (inexact && (up != (sign != 0))) h = (uint16_t)(h + 1);  // away from zero
        if (((h >> 10) & 0x1f) == 0x1f) return false;             // stepped to infinity
        out = h;
        return true;
    }

    static float inflate(float v) { return 1e-3f + 1e-4f * std::fabs(v); }
    static float area(const float* lo, const float* hi) {
        const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return (dx < 0 || dy < 0 || dz < 0) ? 0.0f : 2.0f * (dx * dy + dy * dz + dz * dx);
    }

    int make_leaf(int node, int b, int e) {
        tree[node].first = (int)prims.size();
        tree[node].count = e - b;
        for (int i = b; i < e; i++) prims.push_back(items[i].id);
        return node;
    }

    int build(int b, int e) {
        const int node = (int)tree.size();
        tree.emplace_back();
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = b; i < e; i++)
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], items[i].lo[a]);
                hi[a] = std::max(hi[a], items[i].hi[a]);
                clo[a] = std::min(clo[a], items[i].c[a]);
                chi[a] = std::max(chi[a], items[i].c[a]);
            }
        for (int a = 0; a < 3; a++) {
            tree[node].lo[a] = lo[a];
            tree[node].hi[a] = hi[a];
        }
        const int n = e - b;
        if (n <= 2) return make_leaf(node, b, e);
        // binned SAH over the three axes
        float best_cost = INFINITY;
        int best_axis = -1, best_bin = -1;
        for (int a = 0; a < 3; a++) {
            const float ext = chi[a] - clo[a];
            if (!(ext > 0.0f)) continue;
            int cnt[kBins] = {0};
            float blo[kBins][3], bhi[kBins][3];
            for (int k = 0; k < kBins; k++)
                for (int q = 0; q < 3; q++) {
                    blo[k][q] = INFINITY;
                    bhi[k][q] = -INFINITY;
                }
            for (int i = b; i < e; i++) {
                int k = (int)((items[i].c[a] - clo[a]) / ext * kBins);
                k = std::min(std::max(k, 0), kBins - 1);
                cnt[k]++;
                for (int q = 0; q < 3; q++) {
                    blo[k][q] = std::min(blo[k][q], items[i].lo[q]);
                    bhi[k][q] = std::max(bhi[k][q], items[i].hi[q]);
                }
            }
            float rarea[kBins];
            int rcnt[kBins];
            float rl[3] = {INFINITY, INFINITY, INFINITY}, rh[3] = {-INFINITY, -INFINITY, -INFINITY};
            int rc = 0;
            for (int k = kBins - 1; k > 0; k--) {
                rc += cnt[k];
                for (int q = 0; q < 3; q++) {
                    rl[q] = std::min(rl[q], blo[k][q]);
                    rh[q] = std::max(rh[q], bhi[k][q]);
                }
                rarea[k] = area(rl, rh);
                rcnt[k] = rc;
            }
            float ll[3] = {INFINITY, INFINITY, INFINITY}, lh[3] = {-INFINITY, -INFINITY, -INFINITY};
            int lc = 0;
            for (int k = 0; k < kBins - 1; k++) {
                lc += cnt[k];
                for (int q = 0; q < 3; q++) {
                    ll[q] = std::min(ll[q], blo[k][q]);
                    lh[q] = std::max(lh[q], bhi[k][q]);
                }
                if (lc == 0 || rcnt[k + 1] == 0) continue;
                const float cost = area(ll, lh) * lc + rarea[k + 1] * rcnt[k + 1];
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = a;
                    best_bin = k;
                }
            }
        }
        const float leaf_cost = area(lo, hi) * n;
        best_cost += trav_cost * area(lo, hi);
        int mid;
        if (best_axis >= 0 && (best_cost < leaf_cost || n > max_leaf)) {
            const int a = best_axis;
            const float ext = chi[a] - clo[a];
            auto it = std::partition(items.begin() + b, items.begin() + e, [&](const BvhItem& x) {
                int k = (int)((x.c[a] - clo[a]) / ext * kBins);
                k = std::min(std::max(k, 0), kBins - 1);
                return k <= best_bin;
            });
            mid = (int)(it - items.begin());
        } else if (n <= max_leaf) {
            return make_leaf(node, b, e);
        } else {  // all centroids equal: split in the middle
            mid = (b + e) / 2;
        }
        if (mid <= b || mid >= e) mid = (b + e) / 2;
        const int l = build(b, mid);
        const int r = build(mid, e);
        tree[node].axis = best_axis >= 0 ? best_axis : 0;
        tree[node].left = l;
        tree[node].right = r;
        return node;
    }

    // threaded array for the ray-direction octant `order` (bit a set: d[a] < 0):
    // at every node the child on the near side of its split axis comes first
    void emit(int order, int node, std::vector<int>& pos, std::vector<int>& seq) {
        pos[node] = (int)seq.size();
        seq.push_back(node);
        const BvhNode& t = tree[node];
        if (t.left < 0) return;
        const bool left_first = !((order >> t.axis) & 1);
        emit(order, left_first ? t.left : t.right, pos, seq);
        emit(order, left_first ? t.right : t.left, pos, seq);
    }

    void finish() {
        n_nodes = (int)tree.size();
        nodes.assign((size_t)8 * n_nodes * 8, 0.0f);
        nodes16.assign((size_t)8 * n_nodes * 4, 0u);
        n16 = true;
        std::vector<int> pos(n_nodes), seq, end(n_nodes);
        for (int order = 0; order < 8; order++) {
            if (order & ~order_mask) continue;  // never selected by the kernel
            seq.clear();
            emit(order, 0, pos, seq);
            // subtree end in this order: position after the last descendant
            for (int i = n_nodes - 1; i >= 0; i--) {
                const BvhNode& t = tree[seq[i]];
                end[i] = t.left < 0 ? i + 1 : std::max(end[pos[t.left]], end[pos[t.right]]);
            }
            float* base = nodes.data() + (size_t)order * n_nodes * 8;
            for (int i = 0; i < n_nodes; i++) {
                const BvhNode& t = tree[seq[i]];
                float* nd = base + (size_t)i * 8;
                for (int a = 0; a < 3; a++) {
                    nd[a] = t.lo[a];
                    nd[4 + a] = t.hi[a];
                }
                const int miss = end[i] < n_nodes ? end[i] : -1;
                const int leaf = t.left < 0 ? ((t.count << 24) | t.first) : -1;
                std::memcpy(&nd[3], &miss, 4);
                std::memcpy(&nd[7], &leaf, 4);
                // 16-byte node: {lo.x | lo.y, lo.z | hi.x, hi.y | hi.z} in fp16
                // (lo rounded down, hi up) + w: the miss link of an internal node
                // (-1 = done) or ~leaf of a leaf (count >= 1, so w < -2^24; a
                // leaf's miss link is always the next node, i + 1)
                uint16_t hb[6];
                for (int a = 0; a < 3; a++)
                    n16 = n16 && half_bound(t.lo[a], false, hb[a]) && half_bound(t.hi[a], true, hb[3 + a]);
                uint32_t* q = nodes16.data() + ((size_t)order * n_nodes + i) * 4;
                q[0] = hb[0] | (uint32_t)hb[1] << 16;
                q[1] = hb[2] | (uint32_t)hb[3] << 16;
                q[2] = hb[4] | (uint32_t)hb[5] << 16;
                const int w = t.left < 0 ? ~leaf : miss;
                std::memcpy(&q[3], &w, 4);
            }
        }
    }

    // ---- spatial splits (SBVH, Stich, Friedrich & Dietrich 2009) ----------
    // A reference is a primitive cut down to a region of space: its box
    // bounds the part of the primitive inside every split plane it was cut
    // by (polygons clipped in double precision, spheres by their box).  A
    // primitive may sit in several leaves; testing it more than once changes
    // nothing ((t, key) acceptance), and the union of its references' boxes
    // covers the whole primitive.  Boxes are inflated as above when stored.
    struct Ref {
        double lo[3], hi[3];
        int id;
    };
    std::vector<double> geo;  // per primitive id: up to 4 vertices, 12 doubles
    std::vector<int> geo_nv;  // 3 / 4: polygon vertices; 0: clipped by its box
    double root_area = 0.0;
    size_t ref_budget = 0, n_refs = 0;
    double split_alpha = 1e-5;  // try spatial splits when the object split's children overlap > alpha * root area
    static constexpr int kSpatialBins = 32;

    static double dinflate(double v) { return 1e-3 + 1e-4 * std::fabs(v); }
    static float fdown(double v) {
        float f = (float)v;
        if ((double)f > v) f = std::nextafter(f, -INFINITY);
        return f;
    }
    static float fup(double v) {
        float f = (float)v;
        if ((double)f < v) f = std::nextafter(f, INFINITY);
        return f;
    }
    static double darea(const double* lo, const double* hi) {
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return (dx < 0 || dy < 0 || dz < 0) ? 0.0 : 2.0 * (dx * dy + dy * dz + dz * dx);
    }

    // the part of r with s0 <= x_a <= s1; false if there is none
    bool clip(const Ref& r, int a, double s0, double s1, Ref& out) const {
        out = r;
        out.lo[a] = std::max(r.lo[a], s0);
        out.hi[a] = std::min(r.hi[a], s1);
        if (out.lo[a] > out.hi[a]) return false;
        const int nv = geo_nv[r.id];
        if (nv < 3) return true;
        double poly[8][3], tmp[8][3];
        int n = nv;
        for (int k = 0; k < nv; k++)
            for (int q = 0; q < 3; q++) poly[k][q] = geo[(size_t)12 * r.id + 3 * k + q];
        for (int side = 0; side < 2 && n > 0; side++) {
            int m = 0;
            for (int k = 0; k < n; k++) {
                const double* p = poly[k];
                const double* q = poly[(k + 1) % n];
                const double dp = side == 0 ? p[a] - s0 : s1 - p[a];
                const double dq = side == 0 ? q[a] - s0 : s1 - q[a];
                if (dp >= 0.0)
                    for (int c = 0; c < 3; c++) tmp[m][c] = p[c];
                if (dp >= 0.0) m++;
                if ((dp >= 0.0) != (dq >= 0.0)) {
                    const double t = dp / (dp - dq);
                    for (int c = 0; c < 3; c++) tmp[m][c] = p[c] + t * (q[c] - p[c]);
                    m++;
                }
            }
            n = m;
            for (int k = 0; k < n; k++)
                for (int c = 0; c < 3; c++) poly[k][c] = tmp[k][c];
        }
        // no part of the polygon in the slab (a sliver on its boundary is
        // covered by the neighbouring reference's inflated box)
        if (n == 0) return false;
        double plo[3] = {INFINITY, INFINITY, INFINITY}, phi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < n; k++)
            for (int c = 0; c < 3; c++) {
                plo[c] = std::min(plo[c], poly[k][c]);
                phi[c] = std::max(phi[c], poly[k][c]);
            }
        for (int c = 0; c < 3; c++) {
            out.lo[c] = std::max(out.lo[c], plo[c]);
            out.hi[c] = std::min(out.hi[c], phi[c]);
            if (out.lo[c] > out.hi[c]) {  // rounding: keep a degenerate box at the slab
                out.lo[c] = out.hi[c] = std::min(std::max(0.5 * (plo[c] + phi[c]), out.lo[c]), out.hi[c]);
            }
        }
        return true;
    }

    int build_s(std::vector<Ref>& refs) {
        const int node = (int)tree.size();
        tree.emplace_back();
        const int n = (int)refs.size();
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (const Ref& r : refs)
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], r.lo[a]);
                hi[a] = std::max(hi[a], r.hi[a]);
                const double c = 0.5 * (r.lo[a] + r.hi[a]);
                clo[a] = std::min(clo[a], c);
                chi[a] = std::max(chi[a], c);
            }
        for (int a = 0; a < 3; a++) {
            tree[node].lo[a] = fdown(lo[a] - dinflate(lo[a]));
            tree[node].hi[a] = fup(hi[a] + dinflate(hi[a]));
        }
        auto leaf = [&]() {
            tree[node].first = (int)prims.size();
            tree[node].count = n;
            for (const Ref& r : refs) prims.push_back(r.id);
            return node;
        };
        if (n <= 2) return leaf();
        // object split: binned SAH over the reference centroids
        double best_cost = INFINITY, ov_area = 0.0;
        int best_axis = -1, best_bin = -1;
        for (int a = 0; a < 3; a++) {
            const double ext = chi[a] - clo[a];
            if (!(ext > 0.0)) continue;
            int cnt[kBins] = {0};
            double blo[kBins][3], bhi[kBins][3];
            for (int k = 0; k < kBins; k++)
                for (int q = 0; q < 3; q++) blo[k][q] = INFINITY, bhi[k][q] = -INFINITY;
            for (const Ref& r : refs) {
                int k = (int)((0.5 * (r.lo[a] + r.hi[a]) - clo[a]) / ext * kBins);
                k = std::min(std::max(k, 0), kBins - 1);
                cnt[k]++;
                for (int q = 0; q < 3; q++) blo[k][q] = std::min(blo[k][q], r.lo[q]), bhi[k][q] = std::max(bhi[k][q], r.hi[q]);
            }
            double rl[kBins][3], rh[kBins][3];
            int rc[kBins];
            double al[3] = {INFINITY, INFINITY, INFINITY}, ah[3] = {-INFINITY, -INFINITY, -INFINITY};
            int c = 0;
            for (int k = kBins - 1; k > 0; k--) {
                c += cnt[k];
                for (int q = 0; q < 3; q++) al[q] = std::min(al[q], blo[k][q]), ah[q] = std::max(ah[q], bhi[k][q]);
                for (int q = 0; q < 3; q++) rl[k][q] = al[q], rh[k][q] = ah[q];
                rc[k] = c;
            }
            double ll[3] = {INFINITY, INFINITY, INFINITY}, lh[3] = {-INFINITY, -INFINITY, -INFINITY};
            int lc = 0;
            for (int k = 0; k < kBins - 1; k++) {
                lc += cnt[k];
                for (int q = 0; q < 3; q++) ll[q] = std::min(ll[q], blo[k][q]), lh[q] = std::max(lh[q], bhi[k][q]);
                if (lc == 0 || rc[k + 1] == 0) continue;
                const double cost = darea(ll, lh) * lc + darea(rl[k + 1], rh[k + 1]) * rc[k + 1];
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = a;
                    best_bin = k;
                    double ol[3], oh[3];
                    for (int q = 0; q < 3; q++) ol[q] = std::max(ll[q], rl[k + 1][q]), oh[q] = std::min(lh[q], rh[k + 1][q]);
                    ov_area = darea(ol, oh);
                }
            }
        }
        // spatial split: chop the references into spatial bins
        bool spatial = false;
        double split_pos = 0.0;
        if (n_refs < ref_budget && ov_area > split_alpha * root_area) {
            for (int a = 0; a < 3; a++) {
                const double ext = hi[a] - lo[a];
                if (!(ext > 0.0)) continue;
                const double w = ext / kSpatialBins;
                int ent[kSpatialBins] = {0}, ext_[kSpatialBins] = {0};
                double blo[kSpatialBins][3], bhi[kSpatialBins][3];
                for (int k = 0; k < kSpatialBins; k++)
                    for (int q = 0; q < 3; q++) blo[k][q] = INFINITY, bhi[k][q] = -INFINITY;
                for (const Ref& r : refs) {
                    int k0 = (int)((r.lo[a] - lo[a]) / w), k1 = (int)((r.hi[a] - lo[a]) / w);
                    k0 = std::min(std::max(k0, 0), kSpatialBins - 1);
                    k1 = std::min(std::max(k1, k0), kSpatialBins - 1);
                    bool any = false;
                    int first = -1, last = -1;
                    for (int k = k0; k <= k1; k++) {
                        const double s0 = k == 0 ? -INFINITY : lo[a] + k * w;
                        const double s1 = k == kSpatialBins - 1 ? INFINITY : lo[a] + (k + 1) * w;
                        Ref part;
                        if (!clip(r, a, s0, s1, part)) continue;
                        any = true;
                        if (first < 0) first = k;
                        last = k;
                        for (int q = 0; q < 3; q++) blo[k][q] = std::min(blo[k][q], part.lo[q]), bhi[k][q] = std::max(bhi[k][q], part.hi[q]);
                    }
                    if (!any) {  // (rounding) count it in its box's first bin
                        first = last = k0;
                        for (int q = 0; q < 3; q++) blo[k0][q] = std::min(blo[k0][q], r.lo[q]), bhi[k0][q] = std::max(bhi[k0][q], r.hi[q]);
                    }
                    ent[first]++;
                    ext_[last]++;
                }
                double rl[kSpatialBins][3], rh[kSpatialBins][3];
                int rc[kSpatialBins];
                double al[3] = {INFINITY, INFINITY, INFINITY}, ah[3] = {-INFINITY, -INFINITY, -INFINITY};
                int c = 0;
                for (int k = kSpatialBins - 1; k > 0; k--) {
                    c += ext_[k];
                    for (int q = 0; q < 3; q++) al[q] = std::min(al[q], blo[k][q]), ah[q] = std::max(ah[q], bhi[k][q]);
                    for (int q = 0; q < 3; q++) rl[k][q] = al[q], rh[k][q] = ah[q];
                    rc[k] = c;
                }
                double ll[3] = {INFINITY, INFINITY, INFINITY}, lh[3] = {-INFINITY, -INFINITY, -INFINITY};
                int lc = 0;
                for (int k = 0; k < kSpatialBins - 1; k++) {
                    lc += ent[k];
                    for (int q = 0; q < 3; q++) ll[q] = std::min(ll[q], blo[k][q]), lh[q] = std::max(lh[q], bhi[k][q]);
                    if (lc == 0 || rc[k + 1] == 0) continue;
                    const double cost = darea(ll, lh) * lc + darea(rl[k + 1], rh[k + 1]) * rc[k + 1];
                    if (cost < best_cost) {
                        best_cost = cost;
                        best_axis = a;
                        spatial = true;
                        split_pos = lo[a] + (k + 1) * w;
                    }
                }
            }
        }
        const double leaf_cost = darea(lo, hi) * n;
        best_cost += trav_cost * darea(lo, hi);
        if (best_axis < 0 || (best_cost >= leaf_cost && n <= max_leaf)) {
            if (n <= max_leaf) return leaf();
        }
        std::vector<Ref> L, R;
        if (best_axis >= 0 && spatial) {
            const int a = best_axis;
            for (const Ref& r : refs) {
                if (r.hi[a] <= split_pos) {
                    L.push_back(r);
                } else if (r.lo[a] >= split_pos) {
                    R.push_back(r);
                } else {
                    Ref pl, pr;
                    const bool hl = clip(r, a, -INFINITY, split_pos, pl), hr = clip(r, a, split_pos, INFINITY, pr);
                    if (hl) L.push_back(pl);
                    if (hr) R.push_back(pr);
                    if (!hl && !hr) L.push_back(r);
                }
            }
        } else if (best_axis >= 0) {
            const int a = best_axis;
            const double ext = chi[a] - clo[a];
            for (const Ref& r : refs) {
                int k = (int)((0.5 * (r.lo[a] + r.hi[a]) - clo[a]) / ext * kBins);
                k = std::min(std::max(k, 0), kBins - 1);
                (k <= best_bin ? L : R).push_back(r);
            }
        }
        if (L.empty() || R.empty()) {  // no usable split: halve the list along the widest centroid axis
            L.clear();
            R.clear();
            int a = 0;
            for (int q = 1; q < 3; q++)
                if (chi[q] - clo[q] > chi[a] - clo[a]) a = q;
            std::sort(refs.begin(), refs.end(),
                      [a](const Ref& x, const Ref& y) { return x.lo[a] + x.hi[a] < y.lo[a] + y.hi[a]; });
            L.assign(refs.begin(), refs.begin() + n / 2);
            R.assign(refs.begin() + n / 2, refs.end());
            best_axis = a;
        }
        n_refs += L.size() + R.size() - (size_t)n;
        std::vector<Ref>().swap(refs);
        const int l = build_s(L);
        const int r = build_s(R);
        tree[node].axis = best_axis;
        tree[node].left = l;
        tree[node].right = r;
        return node;
    }

    void add(int id, const float* lo, const float* hi) {
        BvhItem it;
        for (int a = 0; a < 3; a++) {
            it.lo[a] = lo[a] - inflate(lo[a]);
            it.hi[a] = hi[a] + inflate(hi[a]);
            it.c[a] = 0.5f * (lo[a] + hi[a]);
        }
        it.id = id;
        items.push_back(it);
    }
};

int unsupported(std::string& err, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return RT_ERR_UNSUPPORTED;
}

}  // namespace

const char* const rt_scene_option_names[10] = {"BWRT_NO_CULL",  "BWRT_BVH_MIN",   "BWRT_BVH_LEAF",       "BWRT_BVH_CT",
                                               "BWRT_BVH_SBVH", "BWRT_BVH_REFS",  "BWRT_BVH_ALPHA",      "BWRT_BVH_ORDER_MASK",
                                               "BWRT_BVH_N16",  "BWRT_BVH_STATS"};

bool rt_scene_option_set(rt_scene_options& o, const char* name, const char* v) {
    const auto is = [name](const char* n) { return std::strcmp(name, n) == 0; };
    if (is("BWRT_NO_CULL")) o.no_cull = true;  // set at all
    else if (is("BWRT_BVH_MIN")) o.bvh_min = std::atoi(v);
    // leaf = (count << 24) | first in an int: count <= 127 keeps the sign
    // bit clear (a negative value means "internal node" to the kernels)
    else if (is("BWRT_BVH_LEAF")) o.bvh_leaf = std::min(std::max(std::atoi(v), 1), 127);
    else if (is("BWRT_BVH_CT")) o.bvh_ct = (float)std::atof(v);
    else if (is("BWRT_BVH_SBVH")) o.bvh_sbvh = std::atoi(v) != 0;
    else if (is("BWRT_BVH_REFS")) o.bvh_refs = std::atof(v);
    else if (is("BWRT_BVH_ALPHA")) o.bvh_alpha = std::atof(v);
    else if (is("BWRT_BVH_ORDER_MASK")) o.bvh_order_mask = std::atoi(v) & 7;
    else if (is("BWRT_BVH_N16")) o.bvh_n16 = std::atoi(v) != 0;
    else if (is("BWRT_BVH_STATS")) o.bvh_stats = true;  // set at all
    else return false;
    return true;
}

int rt_compile_scene(const rt_scene& scene, const rt_scene_options& opt, rt_compiled_scene& out, std::string& err) {
    const rt_scene* s = &scene;
    rt_compiled_scene r;  // moved into `out` at the end: a failure leaves `out` as it was
    const int ns = r.n_sph = s->sphere_count, np = r.n_pln = s->plane_count;
    const int nt = r.n_tri = s->triangle_count, nq = r.n_quad = s->quad_count;
    const size_t off_pln = r.off_pln = (size_t)ns * RT_SPH_FLOATS;
    const size_t off_tri = r.off_tri = off_pln + (size_t)np * RT_PLN_FLOATS;
    const size_t off_quad = r.off_quad = off_tri + (size_t)nt * RT_TRI_FLOATS;
    const size_t off_hit = r.off_hit = off_quad + (size_t)nq * RT_QUAD_FLOATS;
    const size_t total = off_hit + (size_t)(ns + np + nt + nq) * RT_HIT_FLOATS + 4;
    std::vector<float>& h = r.data;
    h.assign(total, 0.0f);
    float* hit = h.data() + off_hit;
    int id = 0;
    for (int i = 0; i < ns; i++, id++) {  // Intersection.cuh:32-38
        const rt_sphere& sp = s->spheres[i];
        float* q = h.data() + (size_t)i * RT_SPH_FLOATS;
        q[0] = sp.position.x;
        q[1] = sp.position.y;
        q[2] = sp.position.z;
        q[3] = sp.radius * sp.radius;
        float* hh = hit + (size_t)id * RT_HIT_FLOATS;
        hh[0] = sp.position.x;
        hh[1] = sp.position.y;
        hh[2] = sp.position.z;
        hh[3] = 1.0f;  // sphere: normal = normalize(P - centre)
        put_material(hh, sp.mat);
        // light table (rt_layout.h rt_nee_args): emitted as the hit table has it
        if (std::isfinite(sp.mat.emittance) && sp.mat.emittance > 0.0f && std::isfinite(sp.radius) && sp.radius > 0.0f) {
            float rec[RT_LIGHT_FLOATS] = {q[0], q[1], q[2], q[3], hh[4], hh[5], hh[6], 0.0f};
            std::memcpy(&rec[7], &id, 4);
            r.lights.insert(r.lights.end(), rec, rec + RT_LIGHT_FLOATS);
        }
    }
    for (int i = 0; i < np; i++, id++) {  // Intersection.cuh:69,83
        const rt_plane& pl = s->planes[i];
        V3 n = cross(v3(pl.directions[0]), v3(pl.directions[1]));
        float d = -dot(n, v3(pl.origin));
        float* q = h.data() + off_pln + (size_t)i * RT_PLN_FLOATS;
        q[0] = n.x;
        q[1] = n.y;
        q[2] = n.z;
        q[3] = d;
        float* hh = hit + (size_t)id * RT_HIT_FLOATS;
        hh[0] = n.x;
        hh[1] = n.y;
        hh[2] = n.z;
        hh[3] = 0.0f;
        put_material(hh, pl.mat);
    }
    // scene scale for polygon culling: >= every primitive coordinate and the
    // camera position; rays whose origin lies beyond it are never culled
    double scale = 1.0;
    auto grow = [&](const rt_vec3& v, double extra) {
        scale = std::max(scale, std::max(std::fabs((double)v.x), std::max(std::fabs((double)v.y), std::fabs((double)v.z))) + extra);
    };
    grow(s->camera.position, 0.0);
    for (int i = 0; i < ns; i++) grow(s->spheres[i].position, std::fabs((double)s->spheres[i].radius));
    for (int i = 0; i < nt; i++)
        for (int k = 0; k < 3; k++) grow(s->triangles[i].vertices[k], 0.0);
    for (int i = 0; i < nq; i++)
        for (int k = 0; k < 4; k++) grow(s->quads[i].vertices[k], 0.0);
    scale *= 2.0;
    if (!std::isfinite(scale) || scale > 1e30 || opt.no_cull) scale = INFINITY;
    r.cull_omax = std::isfinite(scale) ? (float)scale : -1.0f;  // -1: no ray is culled
    for (int i = 0; i < nt; i++, id++)
        compile_polygon(h.data() + off_tri + (size_t)i * RT_TRI_FLOATS, hit + (size_t)id * RT_HIT_FLOATS,
                        s->triangles[i].vertices, 3, s->triangles[i].mat, scale);
    for (int i = 0; i < nq; i++, id++)
        compile_polygon(h.data() + off_quad + (size_t)i * RT_QUAD_FLOATS, hit + (size_t)id * RT_HIT_FLOATS,
                        s->quads[i].vertices, 4, s->quads[i].mat, scale);
    // polygon lights behind the sphere lights (rt_set_light_shapes): always built, the mode chooses at a render
    r.n_sphere_lights = (int)(r.lights.size() / RT_LIGHT_FLOATS);
    {
        float rec[RT_LIGHT_FLOATS], blk[RT_POLY_LIGHT_FLOATS];
        auto light = [&](int pid, const rt_vec3* verts, int nv, const rt_material& m) {
            if (!polygon_light(hit + (size_t)pid * RT_HIT_FLOATS, verts, nv, m, pid, rec, blk)) return;
            r.lights.insert(r.lights.end(), rec, rec + RT_LIGHT_FLOATS);
            r.light_polys.insert(r.light_polys.end(), blk, blk + RT_POLY_LIGHT_FLOATS);
        };
        for (int i = 0; i < nt; i++) light(ns + np + i, s->triangles[i].vertices, 3, s->triangles[i].mat);
        for (int i = 0; i < nq; i++) light(ns + np + nt + i, s->quads[i].vertices, 4, s->quads[i].mat);
    }
    // the light trees of the two table forms (rt_set_light_hierarchy): likewise always built
    {
        const int n_all = (int)(r.lights.size() / RT_LIGHT_FLOATS);
        build_light_tree(r.lights.data(), r.light_polys.data(), r.n_sphere_lights, r.n_sphere_lights, r.light_tree_spheres);
        if (n_all > r.n_sphere_lights)
            build_light_tree(r.lights.data(), r.light_polys.data(), r.n_sphere_lights, n_all, r.light_tree_all);
    }
    // overflow bounds of the bounded primitives' tests (rt_layout.h ovf_*;
    // a NaN or inf input makes its bound infinite, so no ray is culled and
    // every BVH ray takes the brute-force loop)
    {
        double sc = 0.0, rmax = 0.0, nm = 0.0, im = 0.0;
        auto upd = [](double& b, float x) {
            const double a = std::fabs((double)x);
            if (!(a <= b)) b = std::isnan(a) ? INFINITY : a;
        };
        for (int i = 0; i < ns; i++) {
            const rt_sphere& sp = s->spheres[i];
            upd(sc, sp.position.x);
            upd(sc, sp.position.y);
            upd(sc, sp.position.z);
            upd(rmax, sp.radius);
        }
        auto polyb = [&](const rt_vec3* v, int nv, const float* rec) {
            for (int k = 0; k < nv; k++) {
                upd(sc, v[k].x);
                upd(sc, v[k].y);
                upd(sc, v[k].z);
            }
            for (int a = 0; a < 3; a++) upd(nm, rec[a]);
            for (int k = 0; k < nv; k++)  // {v_k[3], in_k[3]} from float 4 on
                for (int a = 0; a < 3; a++) upd(im, rec[RT_POLY_EDGES + 6 * k + 3 + a]);
        };
        for (int i = 0; i < nt; i++) polyb(s->triangles[i].vertices, 3, h.data() + off_tri + (size_t)i * RT_TRI_FLOATS);
        for (int i = 0; i < nq; i++) polyb(s->quads[i].vertices, 4, h.data() + off_quad + (size_t)i * RT_QUAD_FLOATS);
        const double S = (sc + rmax) * (1.0 + 1e-6), N = nm * (1.0 + 1e-6), I = im * (1.0 + 1e-6);
        r.ovf_sc = (float)std::min(S, 3e38);
        r.ovf_nm = (float)std::min(N, 3e38);
        r.ovf_im = (float)std::min(I, 3e38);
        // culling (polygon_test) skips only polygons whose exact test rejects
        // the ray; a NaN in the inside test would instead accept it, so rays
        // are culled only when, for every origin within cull_omax, no polygon
        // test can overflow: max|d_i| <= cull_dmax (the bounds of the
        // kernel's bvh_safe with om = cull_omax, halved)
        double dmax = INFINITY;
        if (r.cull_omax > 0.0f) {
            const double om = r.cull_omax;
            dmax = std::min(dmax, 1e18 / (om + S));
            if (N > 0.0) {
                dmax = std::min(dmax, 1e36 / N);
                dmax = std::min(dmax, (1e37 - om - S) / (6e4 * N * (om + 3.0 * S)));  // P finite
                if (I > 0.0) dmax = std::min(dmax, (3e36 / I - om - S) / (6e4 * N * (om + 3.0 * S)));
                if (!(N * (om + 3.0 * S) < 1e33)) dmax = -1.0;  // t = num / nd may overflow
            }
            dmax *= 0.5;
        }
        r.cull_dmax = std::isfinite(dmax) ? (float)std::min(dmax, 3e38) : (dmax > 0.0 ? INFINITY : -1.0f);
        if (!(r.cull_dmax > 0.0f)) r.cull_dmax = -1.0f;
    }
    // BVH for large scenes (BWRT_BVH_MIN primitives, default 64)
    size_t &off_bvh = r.off_bvh, &off_bvh_prims = r.off_bvh_prims, &off_bvh_vtx = r.off_bvh_vtx, &off_bvh16 = r.off_bvh16;
    {
        const int bvh_min = opt.bvh_min;
        const int nb = ns + nt + nq;
        if (nb > 0 && nb >= bvh_min) {
            // leaf encoding: 24-bit index of a leaf's first primitive record
            if (nb >= (1 << 24))
                return unsupported(err, "%d bounded primitives: the BVH holds at most 2^24 - 1", nb);
            BvhBuilder B;
            B.items.reserve(nb);
            for (int i = 0; i < ns; i++) {
                const rt_sphere& sp = s->spheres[i];
                const float r = std::fabs(sp.radius);
                const float lo[3] = {sp.position.x - r, sp.position.y - r, sp.position.z - r};
                const float hi[3] = {sp.position.x + r, sp.position.y + r, sp.position.z + r};
                B.add(i, lo, hi);
            }
            auto poly = [&](int id, const rt_vec3* v, int nv) {
                float lo[3] = {v[0].x, v[0].y, v[0].z}, hi[3] = {v[0].x, v[0].y, v[0].z};
                for (int k = 1; k < nv; k++) {
                    const float p[3] = {v[k].x, v[k].y, v[k].z};
                    for (int a = 0; a < 3; a++) {
                        lo[a] = std::min(lo[a], p[a]);
                        hi[a] = std::max(hi[a], p[a]);
                    }
                }
                B.add(id, lo, hi);
            };
            for (int i = 0; i < nt; i++) poly(ns + np + i, s->triangles[i].vertices, 3);
            for (int i = 0; i < nq; i++) poly(ns + np + nt + i, s->quads[i].vertices, 4);
            B.tree.reserve(2 * (size_t)nb);
            B.max_leaf = opt.bvh_leaf;
            B.trav_cost = opt.bvh_ct;
            // spatial splits (BWRT_BVH_SBVH=0: object splits only), references
            // up to BWRT_BVH_REFS x the primitives (default 2)
            if (opt.bvh_sbvh) {
                B.geo.assign((size_t)12 * (ns + np + nt + nq), 0.0);
                B.geo_nv.assign((size_t)(ns + np + nt + nq), 0);
                auto geo = [&](int id, const rt_vec3* v, int nv) {
                    B.geo_nv[id] = nv;
                    for (int k = 0; k < nv; k++) {
                        B.geo[(size_t)12 * id + 3 * k + 0] = v[k].x;
                        B.geo[(size_t)12 * id + 3 * k + 1] = v[k].y;
                        B.geo[(size_t)12 * id + 3 * k + 2] = v[k].z;
                    }
                };
                for (int i = 0; i < nt; i++) geo(ns + np + i, s->triangles[i].vertices, 3);
                for (int i = 0; i < nq; i++) geo(ns + np + nt + i, s->quads[i].vertices, 4);
                std::vector<BvhBuilder::Ref> refs;
                refs.reserve(nb);
                double rlo[3] = {INFINITY, INFINITY, INFINITY}, rhi[3] = {-INFINITY, -INFINITY, -INFINITY};
                auto addref = [&](int id, const double* lo, const double* hi) {
                    BvhBuilder::Ref r;
                    for (int a = 0; a < 3; a++) {
                        r.lo[a] = lo[a];
                        r.hi[a] = hi[a];
                        rlo[a] = std::min(rlo[a], lo[a]);
                        rhi[a] = std::max(rhi[a], hi[a]);
                    }
                    r.id = id;
                    refs.push_back(r);
                };
                for (int i = 0; i < ns; i++) {
                    const rt_sphere& sp = s->spheres[i];
                    const double r = std::fabs((double)sp.radius);
                    const double lo[3] = {sp.position.x - r, sp.position.y - r, sp.position.z - r};
                    const double hi[3] = {sp.position.x + r, sp.position.y + r, sp.position.z + r};
                    addref(i, lo, hi);
                }
                auto polyref = [&](int id, const rt_vec3* v, int nv) {
                    double lo[3] = {v[0].x, v[0].y, v[0].z}, hi[3] = {v[0].x, v[0].y, v[0].z};
                    for (int k = 1; k < nv; k++) {
                        const double p[3] = {v[k].x, v[k].y, v[k].z};
                        for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], p[a]), hi[a] = std::max(hi[a], p[a]);
                    }
                    addref(id, lo, hi);
                };
                for (int i = 0; i < nt; i++) polyref(ns + np + i, s->triangles[i].vertices, 3);
                for (int i = 0; i < nq; i++) polyref(ns + np + nt + i, s->quads[i].vertices, 4);
                const double refs_x = opt.bvh_refs;
                B.split_alpha = opt.bvh_alpha;
                B.root_area = BvhBuilder::darea(rlo, rhi);
                B.ref_budget = (size_t)(refs_x * nb);
                B.n_refs = (size_t)nb;
                B.build_s(refs);
                if (B.prims.size() >= (1u << 24))
                    return unsupported(err, "%zu BVH references: at most 2^24 - 1", B.prims.size());
            } else {
                B.build(0, nb);
            }
            // octant arrays only along the scene's long axes (extent >= half
            // the longest): each bit doubles the node data the walks spread
            // over the caches, and a short axis buys little front-to-back
            // order.  Config 5 (extents ~25 / 9 / 31): x and z, 157 -> 147 ms
            // with 16-byte nodes (all three axes; z alone 187, x alone 272)
            {
                const BvhNode& root = B.tree[0];
                float ext[3], mx = 0.0f;
                for (int a = 0; a < 3; a++) mx = std::max(mx, ext[a] = root.hi[a] - root.lo[a]);
                B.order_mask = 0;
                for (int a = 0; a < 3; a++)
                    if (!(ext[a] < 0.5f * mx)) B.order_mask |= 1 << a;
            }
            if (opt.bvh_order_mask >= 0) B.order_mask = opt.bvh_order_mask;
            B.finish();
            if (opt.bvh_stats) {  // diagnostics (tests, tuning)
                long ax[3] = {0, 0, 0}, inner = 0;
                for (const BvhNode& t : B.tree)
                    if (t.left >= 0) ax[t.axis]++, inner++;
                std::fprintf(stderr, "bvh: %d nodes, %ld internal, %zu references of %d primitives, split axes x %ld y %ld z %ld, octant mask %d, n16 %d\n",
                             (int)B.tree.size(), inner, B.prims.size(), nb, ax[0], ax[1], ax[2], B.order_mask, B.n16 ? 1 : 0);
            }
            r.bvh_nodes_per_order = B.n_nodes;
            r.bvh_order_mask = B.order_mask;
            off_bvh = (total + 3) & ~(size_t)3;
            // leaf records, RT_LEAF_FLOATS (128 B) each, start on a 128-byte
            // boundary: a record spans one cache line
            off_bvh_prims = (off_bvh + B.nodes.size() + 31) & ~(size_t)31;
            // vertex-form leaf records after them (64 B each, 64-byte aligned;
            // the GPU's ray-refill kernel reads these, the CPU walk the full
            // form), then the 16-byte nodes, again from a 128-byte boundary
            // (eight nodes per line, the same lines for every scene)
            off_bvh_vtx = off_bvh_prims + B.prims.size() * RT_LEAF_FLOATS;
            off_bvh16 = B.n16 ? (off_bvh_vtx + B.prims.size() * RT_LEAF_VFLOATS + 31) & ~(size_t)31 : 0;
            h.resize((B.n16 ? off_bvh16 + B.nodes16.size() : off_bvh_vtx + B.prims.size() * RT_LEAF_VFLOATS) + 4, 0.0f);
            std::memcpy(h.data() + off_bvh, B.nodes.data(), B.nodes.size() * sizeof(float));
            if (B.n16) std::memcpy(h.data() + off_bvh16, B.nodes16.data(), B.nodes16.size() * sizeof(uint32_t));
            for (size_t j = 0; j < B.prims.size(); j++) {
                const int id = B.prims[j];
                float* r = h.data() + off_bvh_prims + j * RT_LEAF_FLOATS;
                int kind, idx, nf;
                const float* src;
                if (id < ns) {
                    kind = 0, idx = id, nf = RT_SPH_FLOATS, src = h.data() + (size_t)idx * RT_SPH_FLOATS;
                } else if (id < ns + np + nt) {  // (the BVH does not cull: no cull sphere)
                    kind = 2, idx = id - ns - np, nf = RT_TRI_CULL, src = h.data() + off_tri + (size_t)idx * RT_TRI_FLOATS;
                } else {
                    kind = 3, idx = id - ns - np - nt, nf = RT_QUAD_CULL,
                    src = h.data() + off_quad + (size_t)idx * RT_QUAD_FLOATS;
                }
                // {key, record...} (rt_layout.h): kind = key & 3, the id
                // follows from the index; polygons as {n, d, edges} without
                // the cull sphere wherever the compiled record keeps it
                const int key = RT_KEY(kind, idx);
                std::memcpy(&r[0], &key, 4);
                float* rv = h.data() + off_bvh_vtx + j * RT_LEAF_VFLOATS;  // vertex form
                std::memcpy(&rv[0], &key, 4);
                if (kind == 0) {
                    std::memcpy(&r[1], src, (size_t)nf * sizeof(float));
                    std::memcpy(&rv[1], src, (size_t)nf * sizeof(float));
                } else {
                    std::memcpy(&r[1], src, 4 * sizeof(float));
                    std::memcpy(&r[5], src + RT_POLY_EDGES, (size_t)(kind == 2 ? 18 : 24) * sizeof(float));
                    for (int k = 0; k < (kind == 2 ? 3 : 4); k++)
                        std::memcpy(&rv[1 + 3 * k], src + RT_POLY_EDGES + 6 * k, 3 * sizeof(float));
                }
            }
        }
    }
    if (!opt.bvh_n16) r.off_bvh16 = 0;  // the data keeps the nodes either way
    out = std::move(r);
    return RT_OK;
}
