"""Float64 reference of next-event estimation, written from the specification
comment at the head of csrc/rt_light.h and the layout comment of
csrc/rt_layout.h (rt_nee_args) — numpy only, no product code.  Inputs arrive
as float32 and are widened once; everything after that is float64 (except
fold(), which the header specifies exactly and which is therefore float32 with
one rounding per operation).

Besides the values every discrete choice reports its DECISION MARGIN (how far
the deciding quantity is from its threshold, in that quantity's own relative
unit), so a test can tell the cases a float evaluation may legitimately decide
the other way, and k reports its SENSITIVITY INTERVAL (k with the sampled
point or direction displaced by the float rounding of its construction).

tests/test_nee_reference.py validates this file against closed forms and then
holds tools/nee_probe.hip's host pass to it; tests/test_gpu_nee_probe.py the
device pass.
"""
import ctypes as C

import numpy as np

RT_PI = float(np.float32(3.1415926535))  # rt_layout.h: the float the product calls pi
TWO_PI = 2.0 * RT_PI
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)  # the smallest normal float
EPS = 2.0 ** -24
DECIDED = 2.0 ** -20  # decision threshold, in the margin's own relative unit
WI_TOL = 2.0 ** -20
K_REL = 32 * EPS
WEIGHT_REL = 64 * EPS

UNIFORM, WEIGHTED = 0, 1
SPHERES, ALL = 0, 1


def f32(x):
    return np.asarray(x, np.float32)


def _dot(a, b):
    return (a * b).sum(-1)


def _exact32(x):
    """x (float64) is a float32 value"""
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(x).astype(np.float64) == x


# ---- the light table ------------------------------------------------------------------

def _v(p):
    return np.array([p.x, p.y, p.z], np.float32)


def _cross32(a, b):
    """the reference's cross product, each operation rounded to float (the hit table's normal floats)"""
    with np.errstate(all="ignore"):
        return np.array([a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]], np.float32)


def _half_area(a, b, c):
    x = np.cross(b - a, c - a)
    return 0.5 * np.sqrt(_dot(x, x))


def _polygon(verts, mat, pid):
    """The record and block of one polygon as rt_layout.h defines them, None if
    the polygon is not admitted (rt_light.h / rt_layout.h: emittance finite
    and > 0, finite vertices, a finite normal of positive length, both halves
    of positive area, a quad's projection convex)."""
    with np.errstate(all="ignore"):
        e = np.float32(mat.emittance)
        if not (np.isfinite(e) and e > 0):
            return None
        v32 = [_v(p) for p in verts]
        if not all(np.isfinite(p).all() for p in v32):
            return None
        n32 = _cross32(v32[1] - v32[0], v32[2] - v32[1])
        nn32 = np.float32(np.float32(n32[0] * n32[0] + n32[1] * n32[1]) + n32[2] * n32[2])
        if not (np.isfinite(nn32) and nn32 > 0):
            return None
        v = [p.astype(np.float64) for p in v32]
        n = n32.astype(np.float64)
        v3p = v[2].copy()
        if len(v) == 4:
            v3p = v[3] - (_dot(n, v[3] - v[0]) / _dot(n, n)) * n
            p = [v[0], v[1], v[2], v3p]
            for k in range(4):  # convex: every vertex inside every edge (inner normal n x e_k)
                inner = np.cross(n, p[(k + 1) % 4] - p[k])
                for j in range(4):
                    if j in (k, (k + 1) % 4):
                        continue
                    if not (_dot(inner, p[j] - p[k]) >= 0):
                        return None
        a0 = _half_area(v[0], v[1], v[2])
        a1 = _half_area(v[0], v[2], v3p) if len(v) == 4 else 0.0
        if not (np.isfinite(f32(a0)) and f32(a0) > 0) or (len(v) == 4 and not (np.isfinite(f32(a1)) and f32(a1) > 0)):
            return None
        if not np.isfinite(f32(a0 + a1)) or not np.isfinite(f32(v3p)).all():
            return None
        centre = f32(np.mean(v, axis=0)).astype(np.float64)  # the record holds it as a float
        r2 = max(_dot(q - centre, q - centre) for q in v + [v3p])
        if not (np.isfinite(f32(centre)).all() and np.isfinite(f32(r2))):
            return None
        emitted = e * _v(mat.albedo)
        block = np.concatenate([v[0], [a0], v[1], [a1], v[2], [np.sqrt(_dot(n, n))], v3p, [0.0], n, [0.0]])
        return dict(centre=centre, r2=r2, emitted=emitted.astype(np.float64), prim=pid, block=block)


def light_table(scene):
    """The table of rt_layout.h's comment for a bwrt Scene, in float64 (values
    that the layout defines as floats — vertices, n, emitted, a sphere's r*r —
    are float32 values): dict(n_sph, n_sphere_lights, centre (L, 3), r2 (L,),
    emitted (L, 3), prim (L,), blocks (L - n_sphere_lights, 20))."""
    ns, npl, nt, nq = scene.counts
    recs = []
    with np.errstate(all="ignore"):
        for i in range(ns):
            s = scene.spheres[i]
            e, r = np.float32(s.mat.emittance), np.float32(s.radius)
            if np.isfinite(e) and e > 0 and np.isfinite(r) and r > 0:
                recs.append(dict(centre=_v(s.position).astype(np.float64), r2=float(r * r),
                                 emitted=(e * _v(s.mat.albedo)).astype(np.float64), prim=i, block=None))
    nsl = len(recs)
    for i in range(nt):
        recs.append(_polygon(list(scene.triangles[i].vertices), scene.triangles[i].mat, ns + npl + i))
    for i in range(nq):
        recs.append(_polygon(list(scene.quads[i].vertices), scene.quads[i].mat, ns + npl + nt + i))
    recs = [r for r in recs if r is not None]
    return make_table([r["centre"] for r in recs], [r["r2"] for r in recs], [r["emitted"] for r in recs],
                      [r["prim"] for r in recs], [r["block"] for r in recs[nsl:]], nsl, ns)


def make_table(centre, r2, emitted, prim, blocks, n_sphere_lights, n_sph):
    n = len(prim)
    return dict(n_sph=int(n_sph), n_sphere_lights=int(n_sphere_lights),
                centre=np.asarray(centre, np.float64).reshape(n, 3), r2=np.asarray(r2, np.float64).reshape(n),
                emitted=np.asarray(emitted, np.float64).reshape(n, 3), prim=np.asarray(prim, np.int64).reshape(n),
                blocks=np.asarray(blocks, np.float64).reshape(n - n_sphere_lights, 20))


def table_from_words(words):
    """The table of a table.bin (tools/nee_probe.hip), widened: (table, hit rows as float32)"""
    words = np.asarray(words, np.uint32)
    nl, nsl, ns, nh = (int(x) for x in words[:4].view(np.int32))
    f = words[4:].view(np.float32)
    rec = f[:8 * nl].reshape(nl, 8)
    blk = f[8 * nl:8 * nl + 20 * (nl - nsl)].reshape(nl - nsl, 20)
    hit = f[8 * nl + 20 * (nl - nsl):].reshape(nh, 16)
    t = make_table(rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7].copy().view(np.int32), blk, nsl, ns)
    return t, hit


def table_words(t, hit=None):
    """table.bin of a table (an r2 that is no float is rounded up) with an optional hit table behind it"""
    nl, nsl = len(t["prim"]), t["n_sphere_lights"]
    rec = np.zeros((nl, 8), np.float32)
    rec[:, 0:3] = t["centre"]
    r2 = f32(t["r2"]).copy()
    low = r2.astype(np.float64) < t["r2"]
    r2[low] = np.nextafter(r2[low], np.float32(np.inf))
    rec[:, 3] = r2
    rec[:, 4:7] = t["emitted"]
    rec[:, 7] = t["prim"].astype(np.int32).view(np.float32)
    hit = np.zeros((0, 16), np.float32) if hit is None else f32(hit)
    head = np.array([nl, nsl, t["n_sph"], len(hit)], np.int32)
    return np.concatenate([head.view(np.uint32), rec.reshape(-1).view(np.uint32), f32(t["blocks"]).reshape(-1).view(np.uint32),
                           hit.reshape(-1).view(np.uint32)])


def seen(t, shapes):
    """the number of table lights a render in shape mode `shapes` sees"""
    return t["n_sphere_lights"] if shapes == SPHERES else len(t["prim"])


# ---- the draws -------------------------------------------------------------------------

def draws(state):
    """The three uniforms of an NEE level from RNG states (N, 6) {d, v0 .. v4}
    by the oracle's orc_curand (independent of rt_path.h's Xorwow):
    u = float32(float32(word) * float32(2^-32)).  Returns (u (N, 3) float64,
    words (N, 3), the states after)."""
    import oracle
    lib = oracle.lib()
    st = np.ascontiguousarray(state, np.uint32).copy()
    n = len(st)
    words = np.empty((n, 3), np.uint32)
    base = st.ctypes.data
    P32 = C.POINTER(C.c_uint32)
    step = lib.orc_curand
    for i in range(n):
        p = C.cast(base + 24 * i, P32)
        words[i, 0] = step(p)
        words[i, 1] = step(p)
        words[i, 2] = step(p)
    u = (words.astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float32)
    return u.astype(np.float64), words, st


# ---- conditioning ------------------------------------------------------------------------
# A value check presumes that the roundings of a case's intermediates stay roundings in its
# result.  Where they do not, the case is ILL-CONDITIONED: left out of the value checks and
# counted, like an undecided case, on the reference alone.  The rule uses no constant of its
# own: an intermediate is displaced by 4 ulp (2^-22 relative: the displacement the sensitivity
# interval of k gives a polygon's Q), and the case is ill-conditioned when that alone moves the
# checked value by more than the value's whole tolerance.

DISPLACED = 2.0 ** -22


def cone_ill(r2, d2, tol, clamp=False):
    """omega = 1 - sqrt(1 - s2), s2 = r2 / d2 [min(1, .) with clamp], moves by more than tol
    relative when d2 is displaced by 4 ulp: a point just outside a light (for a polygon's
    weight: next to the rim of its bounding sphere, on either side)."""
    def om(d):
        s2 = r2 / d
        if clamp:
            s2 = np.minimum(1.0, s2)
        return s2 / (1.0 + np.sqrt(np.maximum(0.0, 1.0 - s2)))
    with np.errstate(all="ignore"):
        o = om(d2)
        move = np.maximum(np.abs(om(d2 * (1 + DISPLACED)) - o), np.abs(om(d2 * (1 - DISPLACED)) - o))
        return (move > tol * o) & (clamp | (d2 > r2))


# ---- weights ---------------------------------------------------------------------------

def pick_weight(t, m, P, n, nl, prim, poly, tol=WEIGHT_REL):
    """w_m at P (normal n of length nl, on primitive prim) under weighted
    picking; poly: by the polygon rule (bounding sphere, s2 = min(1, R^2/d2)).
    Returns (w, decided, ill): decided False where a float evaluation may put
    the weight on the other side of 0 (reachability within the threshold, a
    weight in the underflow range, a NaN cosine); ill: cone_ill at the
    weight's tolerance (tol: of the value the weight goes into)."""
    c, r2, e, lp = t["centre"][m], t["r2"][m], t["emitted"][m], t["prim"][m]
    with np.errstate(all="ignore"):
        w = c - P
        d2 = _dot(w, w)
        if poly:
            reach = prim != lp
            decided = np.ones(np.shape(d2), bool)
            s2 = np.minimum(1.0, r2 / d2)
        else:
            reach = (prim != lp) & (d2 > r2)
            decided = (prim == lp) | (np.abs(d2 - r2) > DECIDED * r2) | _d2_exact(w, d2)
            s2 = r2 / d2
        omega = s2 / (1.0 + np.sqrt(1.0 - s2))
        cc = _dot(w, n) / (np.sqrt(d2) * nl)
        cb = np.fmax(0.0, cc) + np.sqrt(s2)
        pw = np.abs(e).sum(-1)
        wt = (pw * omega) * cb
        # a float evaluation rounds s2, pw omega and the weight: each is surely 0 below 2^-152 (half the
        # smallest subnormal, with room for the roundings before) and surely normal above 2^-120
        lo, hi = 2.0 ** -152, 2.0 ** -120
        zero = (pw == 0) | (s2 < lo) | (pw * omega < lo) | (wt < lo)
        normal = (s2 > hi) & (pw * omega > hi) & (wt > hi)
        wt = np.where(reach & (wt > 0) & ~zero, wt, 0.0)
        decided = decided & ~(reach & ~zero & ~normal) & ~(reach & np.isnan(cc)) & ~(reach & ~np.isfinite(wt))
        ill = reach & cone_ill(r2, d2, tol, poly)
    return wt, decided, ill


def _d2_exact(w, d2):
    """every operation of the float evaluation of d2 = w . w is exact"""
    sq = w * w
    return (_exact32(w).all(-1) & _exact32(sq).all(-1) & _exact32(sq[..., 0] + sq[..., 1]) & _exact32(d2))


# ---- the sample ------------------------------------------------------------------------

def stretched_cos(cs, nn, shift=0.0):
    """kind 2: (cs / 2) [1 + 1 / (g q^2)]; shift: the relative displacement of un^2"""
    g = 2.0 * nn - 1.0
    un2 = cs * cs / nn * (1.0 + shift)
    q = 1.0 - un2 + un2 / (g * g)
    return 0.5 * cs * (1.0 + 1.0 / (g * q * q))


def stretched_ill(cs, nn, kind):
    """q = 1 - un^2 + un^2 / g^2 cancels for a direction along a long normal (un -> 1, g > 1):
    un^2 displaced by 4 ulp moves the weight by more than k's tolerance"""
    with np.errstate(all="ignore"):
        w0 = stretched_cos(cs, nn)
        move = np.maximum(np.abs(stretched_cos(cs, nn, DISPLACED) - w0), np.abs(stretched_cos(cs, nn, -DISPLACED) - w0))
        return (kind == 2) & (move > K_REL * np.abs(w0))


def _wc(cs, n, kind):
    nn = _dot(n, n)
    with np.errstate(all="ignore"):
        return np.where(kind == 2, stretched_cos(cs, nn), cs)


def nee_sample(t, pick, shapes, u, P, n, prim, kind):
    """The sample of an NEE level for N cases: u (N, 3) the three draws, P, n
    (N, 3), prim, kind (N,).  Returns a dict of arrays: j, prim (-1 where no
    light is picked), trace, k, wi; margin (the smallest decision margin of
    the case, inf where every choice is exact) with the single margins
    m_pick, m_half, m_reach, m_cos, m_cosl, m_frame, m_k; k_lo, k_hi (the
    sensitivity interval, before the relative widening), k_rel (the relative
    widening that the pick mode adds to 32 * 2^-24) and ill (the case is
    ill-conditioned, see above: a sphere's cone just outside the light, a
    weight of the table likewise, a polygon sample whose direction a 4 ulp
    displacement of Q or of t = u1 A moves by more than 2^-20)."""
    P, n, u = (np.asarray(x, np.float64) for x in (P, n, u))
    prim, kind = np.asarray(prim, np.int64), np.asarray(kind, np.int64)
    N = len(P)
    L, nsl = seen(t, shapes), t["n_sphere_lights"]
    inf = np.full(N, np.inf)
    with np.errstate(all="ignore"):
        x = u[:, 0] * L
        j = np.minimum(np.floor(x), L - 1).astype(np.int64)
        m_pick = np.where(x == np.round(x), np.inf, np.abs(x - np.round(x)) / L)
        inv_pick = np.full(N, float(L))
        picked = np.ones(N, bool)
        k_rel = np.zeros(N)
        ill_w = np.zeros(N, bool)
        if pick == WEIGHTED:
            nl = np.where(kind == 2, np.sqrt(_dot(n, n)), 1.0)
            w = np.zeros((N, L))
            dec = np.ones(N, bool)
            ill_w = np.zeros(N, bool)
            for m in range(L):
                w[:, m], d, iw = pick_weight(t, m, P, n, nl, prim, shapes == ALL and m >= nsl, K_REL)
                dec &= d
                ill_w |= iw
            W = w.sum(1)
            picked = W > 0
            pos = w > 0
            run = np.cumsum(w, 1)
            target = u[:, 0] * W
            over = pos & (run > target[:, None])
            last = L - 1 - np.argmax(pos[:, ::-1], 1)
            first = np.argmax(over, 1)
            jw = np.where(over.any(1), first, last)
            # every positive light but the last decides run > target
            gap = np.where(pos & (np.arange(L)[None, :] != last[:, None]), np.abs(run - target[:, None]) / W[:, None], np.inf)
            # an exact tie is no close call: two positive lights of one and the same weight make W = 2 w and,
            # at u == 1/2, target = w = run without a rounding, in float as in double; the tie goes on (>)
            two = (pos.sum(1) == 2) & (w.max(1) == np.where(pos, w, np.inf).min(1)) & (u[:, 0] == 0.5)
            gap = np.where(two[:, None] & (gap == 0), np.inf, gap)
            m_w = np.where(dec, gap.min(1), 0.0)
            m_pick = np.where(picked, m_w, np.where(dec, m_pick, 0.0))
            j = np.where(picked, jw, j)
            wj = np.take_along_axis(w, j[:, None], 1)[:, 0]
            inv_pick = np.where(picked, W / wj, 0.0)
            k_rel = np.full(N, (L + 32) * EPS)
        lp = t["prim"][j]
        c, r2 = t["centre"][j], t["r2"][j]
        is_poly = (j >= nsl) if shapes == ALL else np.zeros(N, bool)
        # sphere: uniform in the cone
        w = c - P
        d2 = _dot(w, w)
        reach_s = (prim != lp) & (d2 > r2)
        m_reach = np.where((prim == lp) | _d2_exact(w, d2), np.inf, np.abs(d2 - r2) / r2)
        s2 = r2 / d2
        omega_s = s2 / (1.0 + np.sqrt(1.0 - s2))
        # cos = 1 - t, sin = sqrt(t (2 - t)): 1 - cos^2 would cancel for a small cone even in double
        tt = u[:, 1] * omega_s
        ct = 1.0 - tt
        st = np.sqrt(np.maximum(0.0, tt * (2.0 - tt)))
        phi = TWO_PI * u[:, 2]
        a = w / np.sqrt(d2)[:, None]
        use_y = np.abs(a[:, 0]) > 0.9
        m_frame = np.abs(np.abs(a[:, 0]) - 0.9)
        helper = np.where(use_y[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
        t1 = np.cross(a, helper)
        t1 = t1 / np.sqrt(_dot(t1, t1))[:, None]
        t2 = np.cross(a, t1)
        wi_s = (st * np.cos(phi))[:, None] * t1 + (st * np.sin(phi))[:, None] * t2 + ct[:, None] * a
        # polygon: area-uniform
        wi_p, omega_p, ok_p = np.zeros((N, 3)), np.zeros(N), np.zeros(N, bool)
        m_half, m_cosl, Q, scale_q = inf.copy(), inf.copy(), np.zeros((N, 3)), np.zeros(N)
        ill_p = np.zeros(N, bool)
        nlv = np.zeros((N, 3))
        if is_poly.any():
            b = t["blocks"][np.where(is_poly, j - nsl, 0)] if len(t["blocks"]) else np.zeros((N, 20))
            v0, a0, v1, a1, v2, nlen, v3, nlv = b[:, 0:3], b[:, 3], b[:, 4:7], b[:, 7], b[:, 8:11], b[:, 11], b[:, 12:15], b[:, 16:19]
            A = a0 + a1
            tq = u[:, 1] * A
            second = (a1 > 0) & (tq >= a0)
            m_half = np.where(a1 > 0, np.abs(tq - a0) / A, np.inf)
            uh = np.minimum(1.0, np.where(second, (tq - a0) / a1, tq / a0))
            su = np.sqrt(uh)
            b1, b2 = u[:, 2] * su, 1.0 - su
            pb = np.where(second[:, None], v2, v1)
            pc = np.where(second[:, None], v3, v2)
            Q = v0 + b1[:, None] * (pb - v0) + b2[:, None] * (pc - v0)
            scale_q = np.max(np.abs(np.concatenate([v0, pb, pc, P], 1)), 1)  # of the half's vertices and P
            wp = Q - P
            d2p = _dot(wp, wp)
            wi_p = wp / np.sqrt(d2p)[:, None]
            nw = _dot(nlv, wp)
            cos_l = np.abs(nw) / (nlen * np.sqrt(d2p))
            m_cosl = np.where(d2p > 0, cos_l, 0.0)  # relative to |n_l| |w|
            omega_p = A * cos_l / (TWO_PI * d2p)
            ok_p = (prim != lp) & (d2p > 0) & (cos_l > 0)
            # ill-conditioned: t = u1 A displaced by 4 ulp moves the direction by more than its tolerance (the
            # second half's u1' = (t - A0) / A1 cancels next to the half boundary, and su = sqrt(u1') divides
            # what is left by 2 su: the corner v3'); Q's own displacement is tried with k's interval below
            for sgn in (-1.0, 1.0):
                td = tq * (1.0 + sgn * DISPLACED)
                uhd = np.clip(np.where(second, (td - a0) / a1, td / a0), 0.0, 1.0)
                sud = np.sqrt(uhd)
                Qt = v0 + (u[:, 2] * sud)[:, None] * (pb - v0) + (1.0 - sud)[:, None] * (pc - v0)
                wt_ = Qt - P
                ill_p |= np.abs(wt_ / np.sqrt(_dot(wt_, wt_))[:, None] - wi_p).max(1) > WI_TOL
            m_reach = np.where(is_poly, np.inf, m_reach)
            m_frame = np.where(is_poly, np.inf, m_frame)
        ok = picked & np.where(is_poly, ok_p, reach_s)
        wi = np.where(is_poly[:, None], wi_p, wi_s)
        omega = np.where(is_poly, omega_p, omega_s)
        nlen_n = np.sqrt(_dot(n, n))
        cs = _dot(wi, n)
        m_cos = np.where(np.isnan(cs), np.inf, np.abs(cs) / nlen_n)  # a NaN normal gives NaN in any order
        m_cos = np.where(ok, m_cos, np.inf)
        m_cosl = np.where(is_poly & picked & (prim != lp), m_cosl, np.inf)
        m_half = np.where(is_poly & picked & (prim != lp), m_half, np.inf)
        m_frame = np.where(ok, m_frame, np.inf)
        m_reach = np.where(picked, m_reach, np.inf)
        lit = ok & (cs > 0)

        def k_of(csv, om):
            return (inv_pick * om) * _wc(csv, n, kind)

        k = k_of(cs, omega)
        # k must be a finite float for a polygon: decided off the edge of the range
        m_k = np.where(lit & is_poly, np.abs(k - FLT_MAX) / FLT_MAX, np.inf)
        trace = lit & ~(is_poly & ~(k <= FLT_MAX))
        # sensitivity: the direction (sphere) or the sampled point (polygon) displaced
        ks = [k]
        for sgn in (-1.0, 1.0):
            ks.append(np.where(is_poly, k, k_of(cs + sgn * WI_TOL * nlen_n, omega)))
        if is_poly.any():
            dq = 4.0 * scale_q * 2.0 ** -23  # 4 ulp of the largest coordinate magnitude
            for axis in range(3):
                for sgn in (-1.0, 1.0):
                    Qd = Q.copy()
                    Qd[:, axis] += sgn * dq
                    wd = Qd - P
                    d2d = _dot(wd, wd)
                    cl = np.abs(_dot(nlv, wd)) / (nlen * np.sqrt(d2d))
                    wid = wd / np.sqrt(d2d)[:, None]
                    kd = k_of(_dot(wid, n), A * cl / (TWO_PI * d2d))
                    ks.append(np.where(is_poly, kd, k))
                    ill_p |= is_poly & (np.abs(wid - wi).max(1) > WI_TOL)
        ks = np.where(np.isnan(ks), k, np.array(ks))
        k_lo, k_hi = ks.min(0), ks.max(0)
        ill = ill_w | np.where(is_poly, ill_p, cone_ill(r2, d2, K_REL)) | stretched_ill(cs, _dot(n, n), kind)
        k = np.where(trace, k, 0.0)
        wi = np.where(trace[:, None], wi, 0.0)
        out_prim = np.where(picked, lp, -1)
        margin = np.minimum.reduce([m_pick, m_half, m_reach, m_cos, m_cosl, m_frame, m_k])
    return dict(j=j, prim=out_prim, trace=trace, k=k, wi=wi, margin=margin, m_pick=m_pick, m_half=m_half, m_reach=m_reach,
                m_cos=m_cos, m_cosl=m_cosl, m_frame=m_frame, m_k=m_k, k_lo=np.where(trace, k_lo, 0.0),
                k_hi=np.where(trace, k_hi, 0.0), k_rel=k_rel, ill=ill, is_poly=is_poly, picked=picked, s2=np.where(is_poly, np.nan, s2))


# ---- suppression -----------------------------------------------------------------------

def suppressed(t, shapes, P, prim, ident):
    """Whether the scattered ray of a level at P on `prim`, having hit primitive
    `ident`, drops that hit's emission: ident is a table light (spheres mode:
    an emissive sphere) reachable from the level.  Returns (flag, decided)."""
    P = np.asarray(P, np.float64)
    prim, ident = np.asarray(prim, np.int64), np.asarray(ident, np.int64)
    L, nsl = seen(t, shapes), t["n_sphere_lights"]
    ids = t["prim"][:L]
    out = np.zeros(len(P), bool)
    decided = np.ones(len(P), bool)
    for i in range(len(P)):
        hit = np.nonzero(ids == ident[i])[0]
        if len(hit) == 0 or (shapes == SPHERES and ident[i] >= t["n_sph"]):
            continue
        m = int(hit[0])
        if m >= nsl:
            out[i] = prim[i] != ident[i]
            continue
        w = t["centre"][m] - P[i]
        d2, r2 = _dot(w, w), t["r2"][m]
        out[i] = prim[i] != ident[i] and d2 > r2
        decided[i] = prim[i] == ident[i] or abs(d2 - r2) > DECIDED * r2 or bool(_d2_exact(w, d2))
    return out, decided


# ---- the kind of a normal ---------------------------------------------------------------

def normal_kind(sphere, n):
    """Whether a hit with normal n can be an NEE level and how its direct term
    weighs the cosine (rt_light.h "Non-unit normals"): 1 for a sphere's normal
    (normalised where it is formed) and for |n|^2 == 1 (cs itself), 2 for any
    other |n|^2 in (1/2, FLT_MAX] (the stretched form), 0 for |n|^2 <= 1/2, a
    |n|^2 no float holds, or NaN.  Returns (kind, decided): decided False where
    a float evaluation of |n|^2 may fall on the other side of 1/2, of 1 or of
    the largest float — closer than DECIDED to it and not exact."""
    n = np.asarray(n, np.float64)
    sphere = np.asarray(sphere, bool)
    with np.errstate(all="ignore"):
        nn = _dot(n, n)
        exact = _d2_exact(n, nn)
        kind = np.where(nn == 1.0, 1, np.where((nn > 0.5) & (nn <= FLT_MAX), 2, 0))
        near = np.zeros(nn.shape, bool)
        for edge in (0.5, 1.0, FLT_MAX):
            near |= np.abs(nn - edge) <= DECIDED * edge
        decided = sphere | np.isnan(nn) | exact | ~near
    return np.where(sphere, 1, kind), decided


# ---- the fold (exact: float32, one rounding per operation) ------------------------------

RT_NEE_DROP, RT_NEE_LEVEL, RT_NEE_VISIBLE, RT_NEE_JSHIFT = 1, 2, 4, 3


def fold(c0, k, c, aux, hit, emitted, L):
    """L' = (keep ? emitted : 0) [+ direct] + (brdf * L) * cosAngle for N
    levels; hit: the hit table rows as float32 (emitted at [4:7], the diffuse
    brdf at [12:15]), emitted: the table lights' emitted floats (n, 3),
    c0 < 0: a specular level of row ~c0 whose brdf is the scalar k.
    direct = k * (diffuse_brdf * emitted_j) on a visible NEE level."""
    c0, aux = np.asarray(c0, np.int64), np.asarray(aux, np.int64)
    k, c, L = f32(k), f32(c), f32(L)
    spec = c0 < 0
    row = np.where(spec, ~c0, c0)
    hit = f32(hit)
    with np.errstate(all="ignore"):
        da = hit[row, 12:15]
        brdf = np.where(spec[:, None], k[:, None], da)
        e = np.where((aux & RT_NEE_DROP)[:, None] != 0, np.float32(0), hit[row, 4:7])
        level = (aux & RT_NEE_LEVEL) != 0
        vis = level & ((aux & RT_NEE_VISIBLE) != 0)
        le = f32(emitted)[np.where(vis, aux >> RT_NEE_JSHIFT, 0)] if len(emitted) else np.zeros((len(c0), 3), np.float32)
        direct = np.where(vis[:, None], k[:, None] * (da * le), np.float32(0))
        e = np.where(level[:, None], e + direct, e)
        return f32(e + (brdf * L) * c[:, None])


# ---- closed forms ----------------------------------------------------------------------

def sphere_mean_k(s2, cos_c):
    """E[k] of one sphere light (uniform pick, unit normal) whose cone lies
    above the horizon: the cone's irradiance over pi, halved by the 1 / 2pi
    unit of omega: s2 cos(theta_c) / 2."""
    return 0.5 * s2 * cos_c


def polygon_mean_k(verts, P, n):
    """E[k] of one polygon light fully above the horizon of the unit normal n at
    P, by Lambert's edge sum: I / (2 pi), I = 1/2 sum_i gamma_i (n . g_i)."""
    verts = [np.asarray(v, np.float64) - np.asarray(P, np.float64) for v in verts]
    total = 0.0
    for i in range(len(verts)):
        a, b = verts[i], verts[(i + 1) % len(verts)]
        g = np.cross(a, b)
        lg = np.sqrt(_dot(g, g))
        if lg == 0:
            continue
        gamma = np.arctan2(lg, _dot(a, b))
        total += gamma * _dot(np.asarray(n, np.float64), g / lg)
    return abs(0.5 * total) / (2.0 * np.pi)
