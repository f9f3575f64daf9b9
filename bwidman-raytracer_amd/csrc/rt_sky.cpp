// rt_sky.cpp — the sky table (rt_sky.h): which wave tiles of a view see
// nothing but the background, proven on the host once per view.
//
// For a pixel of such a tile every frame's camera ray misses, and the
// reference (Main.cu:287-304) then does two things per frame: the rejection
// loop of genRandomDirection for the jitter, which advances the pixel's
// XORWOW stream, and frameSum += backgroundColor.  Everything else (the
// normalisations, the hemisphere flip, the closest hit) draws no random
// number and its result is discarded, so the sorted kernel leaves it out for
// tile groups whose bits are all set.
//
// The proof, per tile (all in double precision; the float inputs are the
// kernel's own):
//
// Ray set.  The kernel's camera ray of pixel (x, y) is
//     d = normalize(d0 + jitter * r),  d0 = normalize(rot * (x - W/2, y - H/2, screen_z))
// with |r| <= 1 + 1e-6 (a normalised ball point, reflected about d0).  The
// tile's pixels lie in the rectangle of the screen plane between its corner
// pixels, `rot *` is linear, and a circular cone of half-angle below 90
// degrees is convex, so every exact d0 lies in the cone round the normalised
// sum A of the four corner directions through the farthest corner
// (half-angle theta_t).  The jitter turns a direction by at most
// asin(jitter * 1.00001); the float rounding of d0 (three products and a
// normalisation: below 1e-6 rad) and of the jittered sum is covered by
// kSlackAngle.  theta = theta_t + both; tiles with theta >= 1 rad are not sky.
// (The corners are taken on the tile grid's lines, x = min(i * tile_w, W - 1):
// a slightly wider rectangle, shared between neighbours.)
//
// Spheres (Intersection.cuh:15-62).  With w = c - o the reference's
// discriminant is 4 ((w.d)^2 - a (|w|^2 - R^2)): negative, and the sphere
// rejected, when the ray's LINE passes farther than R from c.  In float the
// difference o - c is off by at most 2^-23 S per component (S = the scene
// scale, rt_sky_prims::scale, at least twice every coordinate) and the two
// terms carry a few 2^-24 relative roundings of a |w|^2 each, FMA-contracted
// or not.  A sphere is cleared when
//     (|w| s - 2^-20 S)^2 > R^2 + 2^-14 |w|^2,   |w| s > 2^-20 S,
// s = the smallest sine of the angle between w and any line of the cone
// (both its directions: phi - theta > 0 and phi + theta < pi are required,
// phi = angle(A, w)).  The first term moves the centre by more than the
// rounding of o - c, the second is the criterion the kernel's cull spheres
// use (rt_path.h `culled`), 64 times the rounding of the discriminant; the
// absolute term also keeps |w|^2 far from underflow.
//
// Triangles are cleared through their cull spheres by the same test: a ray
// whose line passes a cull sphere is rejected by the reference
// (rt_scene.cpp cull_sphere has the argument, for origins within S and
// directions within cull_dmax).  Quads have no cull sphere in the
// compiled scene (the kernel never culls them: it cannot assume they are
// convex); here a quad whose vertices, projected on its plane {v0, cross(e0,
// e1)}, form a convex polygon with every corner's sine at least 2^-10, and
// lie within 2^-10 of their extent of that plane, gets the bounding sphere
// of the projected vertices inflated exactly as cull_sphere does.  The
// reference's inside test dot(cross(n, e_k), P - v_k) >= 0 ignores the
// components of e_k and v_k along n, so it accepts exactly that projected
// polygon, and cull_sphere's argument (a point farther than Rc - R from a
// convex polygon fails the edge function of its nearest edge or of one of
// the two edges at its nearest corner by |in_k| (Rc - R) sin(alpha / 2))
// carries over.  A polygon is also cleared by the plane criterion below on
// its own compiled plane (the reference intersects that plane first and
// rejects t <= nearZero before any inside test, Intersection.cuh:118-122):
// whichever of the two applies.  That is what clears a wall whose bounding
// sphere holds the camera, for rays that point away from it.  A polygon with
// neither (a skinny triangle or a non-convex quad, too close to its plane's
// zero set) makes the table empty.
//
// Planes (Intersection.cuh:64-106).  t = -(n.o + d) / (n.dir) is rejected
// when t <= nearZero.  With s0 = n.o + d and m = sign(s0) n, a plane is
// cleared when m.dir / |m| > 2^-18 over the whole cone and |s0| > 2^-18
// (|n| |o| sqrt(3) + |d|): both float sums then have the exact sums' signs
// (their rounding is below 2^-21 of those magnitudes), numerator and
// denominator are finite and non-zero, and the quotient is negative (or the
// reference already rejected |n.dir| < nearZero).
//
// Nothing is proven, and the table is empty, when the scene is outside the
// bounds under which those margins hold: a non-finite value anywhere, S
// above 1e9 (every square of the tests stays below 1e20 |d|^2, far from
// overflow: the reference accepts NaN distances, rt_path.h bvh_safe),
// cull_dmax below 2 (a unit direction may not be culled), a BVH scene (it
// never takes the sorted kernel), the camera inside a bounding sphere, the
// linear launch order, samplesPerPixel > 1 (its frames trace several paths
// per camera ray), a jitter of 0.25 or more.
#include <algorithm>
#include <cmath>

#include "rt_scene.h"
#include "rt_sky.h"

struct float4;  // rt_layout.h names them in pointer members only; no HIP header here
struct float2;
struct uint2;
#include "rt_layout.h"

namespace {

const double kAbs = 9.5367431640625e-07;   // 2^-20, x scale: absolute slack of a line distance
const double kRel = 6.103515625e-05;       // 2^-14, x |w|^2: the cull spheres' relative term
const double kSign = 3.814697265625e-06;   // 2^-18: sign margin of the plane sums
const double kSlackAngle = 1e-5;           // rad: float rounding of the camera ray
const double kScaleMax = 1e9;

struct D3 {
    double x, y, z;
};
D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double len(D3 a) { return std::sqrt(dot(a, a)); }
D3 mul(double k, D3 a) { return {k * a.x, k * a.y, k * a.z}; }
D3 d3(const rt_vec3& v) { return {v.x, v.y, v.z}; }

// Bounding sphere {c, Rc^2} of a convex, nearly planar quad, inflated as
// rt_scene.cpp cull_sphere inflates a triangle's; false: no clearing test
bool quad_sphere(const rt_vec3* verts, double scale, double* out) {
    const int nv = 4;
    D3 v[nv], p[nv];
    for (int k = 0; k < nv; k++) v[k] = d3(verts[k]);
    const D3 n = cross(sub(v[1], v[0]), sub(v[2], v[1]));  // cross(e0, e1), compile_polygon
    const double nl = len(n);
    if (!(nl > 0.0) || !std::isfinite(nl)) return false;
    const D3 nh = mul(1.0 / nl, n);
    double extent = 0.0;
    for (int k = 1; k < nv; k++) extent = std::max(extent, len(sub(v[k], v[0])));
    if (!(extent > 0.0) || !std::isfinite(extent)) return false;
    const double tol = std::ldexp(extent, -10);
    D3 c = {0.0, 0.0, 0.0};
    for (int k = 0; k < nv; k++) {
        const double off = dot(nh, sub(v[k], v[0]));
        if (!(std::fabs(off) <= tol)) return false;
        p[k] = sub(v[k], mul(off, nh));
        c = {c.x + 0.25 * p[k].x, c.y + 0.25 * p[k].y, c.z + 0.25 * p[k].z};
    }
    double r = 0.0, min_sin = 1.0;
    for (int k = 0; k < nv; k++) {
        const D3 e = sub(p[(k + 1) % nv], p[k]), in = cross(nh, e);
        const double el = len(e);
        if (!(el > 0.0)) return false;
        for (int j = 0; j < nv; j++)  // the other vertices strictly inside edge k
            if (j != k && j != (k + 1) % nv && !(dot(in, sub(p[j], p[k])) > tol * el)) return false;
        const D3 b = sub(p[(k + nv - 1) % nv], p[k]);
        const double bl = len(b);
        if (!(bl > 0.0)) return false;
        const double cosang = dot(e, b) / (el * bl);
        min_sin = std::min(min_sin, std::sqrt(std::max(0.0, 1.0 - cosang * cosang)));
        r = std::max(r, len(sub(p[k], c)));
    }
    if (!(min_sin >= 1.0 / 1024.0) || !std::isfinite(r) || !std::isfinite(scale)) return false;
    const double rc = r * (1.0 + std::ldexp(1.0, -20)) + std::ldexp(1.0, -14) * scale / (0.25 * min_sin);
    const double rc2 = rc * rc * (1.0 + std::ldexp(1.0, -20));
    if (!(rc2 < 1e30)) return false;
    out[0] = c.x, out[1] = c.y, out[2] = c.z, out[3] = rc2;
    return true;
}

// the tile grid of rt_pixel.h launch_items / item_to_pixel
struct TileGrid {
    int tw = 0, th = 0;
    long tiles_x = 0, tiles_y = 0;  // tiles that hold pixels
    long px = 0, py = 0;            // padded to even sizes (tile_sq)
};
TileGrid tile_grid(const rt_kparams& K) {
    TileGrid g;
    if (K.tile_w <= 0 || K.tile_w > 64 || (K.tile_w & (K.tile_w - 1)) || K.width <= 0 || K.rows <= 0) return g;
    g.tw = K.tile_w;
    g.th = 64 / K.tile_w;
    g.tiles_x = g.px = ((long)K.width + g.tw - 1) / g.tw;
    g.tiles_y = g.py = ((long)K.rows + g.th - 1) / g.th;
    if (K.tile_sq) {
        g.px += g.px & 1;
        g.py += g.py & 1;
    }
    return g;
}

}  // namespace

void rt_sky_collect(const rt_scene& s, const rt_compiled_scene& r, rt_sky_prims& out) {
    rt_sky_prims P;
    P.scale = r.cull_omax;
    P.cull_dmax = r.cull_dmax;
    bool ok = r.off_bvh == 0 && r.cull_omax > 0.0f && std::isfinite(r.cull_omax);
    const float* h = r.data.data();
    auto put = [&](std::vector<double>& to, const float* q) {
        for (int a = 0; a < 4; a++) {
            if (!std::isfinite(q[a])) ok = false;
            to.push_back(q[a]);
        }
    };
    for (int i = 0; ok && i < r.n_sph; i++) {
        put(P.sph, h + (size_t)i * RT_SPH_FLOATS);
        if (!(P.sph.back() >= 0.0)) ok = false;
    }
    for (int i = 0; ok && i < r.n_pln; i++) put(P.pln, h + r.off_pln + (size_t)i * RT_PLN_FLOATS);
    for (int i = 0; ok && i < r.n_tri; i++) {
        // (Rc^2 = inf: no cull sphere; the triangle can still be cleared by its plane)
        const float* q = h + r.off_tri + (size_t)i * RT_TRI_FLOATS;
        for (int a = 0; a < 4; a++) P.poly.push_back(q[RT_TRI_CULL + a]);
        put(P.poly, q);
    }
    for (int i = 0; ok && i < r.n_quad; i++) {
        double q[4] = {0.0, 0.0, 0.0, INFINITY};  // (likewise for a quad that gets no sphere)
        (void)quad_sphere(s.quads[i].vertices, P.scale, q);
        P.poly.insert(P.poly.end(), q, q + 4);
        put(P.poly, h + r.off_quad + (size_t)i * RT_QUAD_FLOATS);
    }
    P.ok = ok;
    if (!ok) {
        P.sph.clear();
        P.pln.clear();
        P.poly.clear();
    }
    out = std::move(P);
}

long rt_sky_tiles(const rt_kparams& K) {
    const TileGrid g = tile_grid(K);
    return g.px * g.py;
}

void rt_sky_build(const rt_kparams& K, const rt_sky_prims& P, std::vector<uint32_t>& bits) {
    const TileGrid g = tile_grid(K);
    const long tiles = g.px * g.py;
    bits.assign(rt_sky_words(tiles), 0u);
    if (tiles == 0 || !P.ok || K.spp_inner > 1) return;
    const double S = P.scale;
    if (!(S > 0.0 && S <= kScaleMax) || !(P.cull_dmax >= 2.0)) return;
    const double jit = K.jitter;
    if (!(jit >= 0.0 && jit < 0.25)) return;
    const D3 cam = {K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]};
    double R[9];
    for (int a = 0; a < 9; a++) R[a] = K.rot[a];
    const double sz = K.screen_z;
    bool finite = std::isfinite(cam.x) && std::isfinite(cam.y) && std::isfinite(cam.z) && std::isfinite(sz);
    for (int a = 0; a < 9; a++) finite = finite && std::isfinite(R[a]);
    if (!finite || !(std::fabs(cam.x) <= S && std::fabs(cam.y) <= S && std::fabs(cam.z) <= S)) return;

    // per primitive: what does not depend on the tile
    struct Sph {
        D3 w;
        double wl, lim2;  // |w|, R^2 + 2^-14 |w|^2
    };
    struct Pln {
        D3 m;  // sign(s0) n / |n|
    };
    struct Poly {  // cleared by its sphere or by its plane, whichever is usable
        Sph s;
        Pln p;
        bool s_ok, p_ok;
    };
    std::vector<Sph> sph(P.sph.size() / 4);
    std::vector<Pln> pln(P.pln.size() / 4);
    std::vector<Poly> poly(P.poly.size() / 8);
    const double abs_slack = kAbs * S;
    // false: the camera inside (or within the slack of) the sphere, no line clears it
    auto sphere_of = [&](const double* q, Sph& s) {
        s.w = sub({q[0], q[1], q[2]}, cam);
        const double l2 = dot(s.w, s.w);
        s.wl = std::sqrt(l2);
        s.lim2 = q[3] + kRel * l2;
        return std::isfinite(s.lim2) && s.wl > abs_slack && (s.wl - abs_slack) * (s.wl - abs_slack) > s.lim2;
    };
    // false: the camera too close to the plane (or the plane too large) for the signs to be certain
    auto plane_of = [&](const double* q, Pln& p) {
        const D3 n = {q[0], q[1], q[2]};
        const double nl = len(n), s0 = dot(n, cam) + q[3];
        if (!(nl > 0.0) || !(nl < 1e18) || !(std::fabs(q[3]) < 1e18)) return false;
        if (!(std::fabs(s0) > kSign * (nl * len(cam) * 1.7320508075688772 + std::fabs(q[3])))) return false;
        p.m = mul((s0 > 0.0 ? 1.0 : -1.0) / nl, n);
        return true;
    };
    for (size_t i = 0; i < sph.size(); i++)
        if (!sphere_of(&P.sph[4 * i], sph[i])) return;
    for (size_t i = 0; i < pln.size(); i++)
        if (!plane_of(&P.pln[4 * i], pln[i])) return;
    for (size_t i = 0; i < poly.size(); i++) {
        poly[i].s_ok = sphere_of(&P.poly[8 * i], poly[i].s);
        poly[i].p_ok = plane_of(&P.poly[8 * i + 4], poly[i].p);
        if (!poly[i].s_ok && !poly[i].p_ok) return;
    }

    // unit directions on the tile grid's lines
    const long gx = g.tiles_x + 1, gy = g.tiles_y + 1;
    std::vector<D3> dir((size_t)(gx * gy));
    for (long iy = 0; iy < gy; iy++) {
        const long j = std::min(iy * g.th, (long)K.rows - 1);
        const double py = (double)((long)K.row_offset + j * K.row_stride - K.height / 2);
        for (long ix = 0; ix < gx; ix++) {
            const double px = (double)(std::min(ix * g.tw, (long)K.width - 1) - K.width / 2);
            const D3 pr = {R[0] * px + R[1] * py + R[2] * sz, R[3] * px + R[4] * py + R[5] * sz,
                           R[6] * px + R[7] * py + R[8] * sz};
            const double l = len(pr);
            // (a zero or non-finite direction poisons its tiles: NaN fails every test below)
            dir[(size_t)(iy * gx + ix)] = mul(1.0 / l, pr);
        }
    }
    const double delta = std::asin(jit * 1.00001) + kSlackAngle;
    const double cd = std::cos(delta), sd = std::sin(delta), cos1 = std::cos(1.0);

    // the tiles [tx0, tx1) x [ty0, ty1): 1 every ray provably misses, 0 not
    // proven, -1 not proven and no tile inside can be (the whole cone on the
    // far side of a plane; only a shortcut: "not sky" needs no proof)
    auto rect_is_sky = [&](long tx0, long ty0, long tx1, long ty1) -> int {
        const D3 c00 = dir[(size_t)(ty0 * gx + tx0)], c10 = dir[(size_t)(ty0 * gx + tx1)];
        const D3 c01 = dir[(size_t)(ty1 * gx + tx0)], c11 = dir[(size_t)(ty1 * gx + tx1)];
        const D3 sum = {c00.x + c10.x + c01.x + c11.x, c00.y + c10.y + c01.y + c11.y, c00.z + c10.z + c01.z + c11.z};
        const double sl = len(sum);
        if (!(sl > 1.0)) return 0;  // (also NaN) corners more than 90 degrees apart
        const D3 A = mul(1.0 / sl, sum);
        const double ct = std::min(std::min(dot(A, c00), dot(A, c10)), std::min(dot(A, c01), dot(A, c11)));
        if (!(ct > 0.0)) return 0;
        const double st = std::sqrt(std::max(0.0, 1.0 - ct * ct));
        const double cth = ct * cd - st * sd, sth = st * cd + ct * sd;  // cos, sin of theta = theta_t + delta
        if (!(cth > cos1)) return 0;
        auto plane_clears = [&](const Pln& p, double& far_side) {
            const double cp = dot(p.m, A), sp = std::sqrt(std::max(0.0, 1.0 - cp * cp));
            far_side = cp * cth + sp * sth;             // cos(psi - theta)
            return cp * cth - sp * sth > kSign;         // cos(psi + theta)
        };
        auto sphere_clears = [&](const Sph& s) {
            const double cphi = dot(A, s.w), sphi = len(cross(A, s.w));  // x |w|
            const double lo = sphi * cth - cphi * sth, hi = sphi * cth + cphi * sth;  // |w| sin(phi -+ theta)
            const double dist = std::min(lo, hi) - abs_slack;
            return dist > 0.0 && dist * dist > s.lim2;
        };
        double far_side;
        for (const Pln& p : pln)
            if (!plane_clears(p, far_side)) return far_side < 0.0 ? -1 : 0;  // every direction beyond it
        for (const Sph& s : sph)
            if (!sphere_clears(s)) return 0;
        for (const Poly& q : poly)
            if (!(q.p_ok && plane_clears(q.p, far_side)) && !(q.s_ok && sphere_clears(q.s))) return 0;
        return 1;
    };
    // tile (tx, ty) -> its place in the launch order (item_to_pixel's inverse)
    auto set_bit = [&](long tx, long ty) {
        const long t = K.tile_sq ? ((ty >> 1) * (g.px >> 1) + (tx >> 1)) * 4 + (ty & 1) * 2 + (tx & 1) : ty * g.px + tx;
        bits[(size_t)(t >> 5)] |= 1u << (t & 31);
    };
    // blocks of kB x kB tiles first (a block's cone holds its tiles' cones),
    // single tiles only where a block is neither proven nor hopeless; the
    // padding tiles hold no pixel: nothing to prove or skip, their bits stay 0
    const long kB = 8;
    for (long by = 0; by < g.tiles_y; by += kB)
        for (long bx = 0; bx < g.tiles_x; bx += kB) {
            const long ex = std::min(bx + kB, g.tiles_x), ey = std::min(by + kB, g.tiles_y);
            const int whole = rect_is_sky(bx, by, ex, ey);
            if (whole < 0) continue;
            for (long ty = by; ty < ey; ty++)
                for (long tx = bx; tx < ex; tx++)
                    if (whole > 0 || rect_is_sky(tx, ty, tx + 1, ty + 1) > 0) set_bit(tx, ty);
        }
}
