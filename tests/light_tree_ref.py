"""The light hierarchy's pick probabilities in float64, restated from the
specification at the head of csrc/rt_light.h (the paragraphs "Weighted picking",
"Polygon lights" and "The light hierarchy") and from the node layout in
csrc/rt_layout.h — not from the code.  Inputs are the float32 values the library
stores (the light table of rt_get_lights, the nodes of rt_get_light_tree) and
the float32 points; everything behind them is float64, vectorised over points.

Beside every value stands a first-order bound of the RELATIVE error a float32
evaluation in the specified order may have against it, u = 2^-24 per rounding:

  w = c - P                 one rounding per component (the inputs are exact)
  d2 = w . w                sum of positive terms                      5 u
  s2 = R2 / d2                                                         6 u
  cm = sqrt(1 - s2)         |delta cm| <= min(sqrt(7 u), 7 u / cm) + u: the
                            error of s2 meets the root's singularity at s2 = 1
  omega = s2 / (1 + cm)     8 u + |delta cm|
  cc                        numerator: absolute 4 u |w| |n| (it may cancel);
                            denominator 8 u; |cc| <= 1: absolute 13 u
  cb = max(0, cc) + sqrt(s2)    absolute 19 u, so relative 19 u / cb
  pw                        2 u
  a leaf, (pw omega) cb:    E = u (14 + 19 / cb) + min(sqrt(7 u), 7 u / cm)
  a node, (phi / max(d2, R2)) cb:   E = u (7 + 19 / cb)
  a level, inv (S / I_c):   max(E_a, E_b) + E_c + 3 u
  p = 1 / inv:              the levels' sum + u

tests/test_light_tree.py doubles the bound: the second-order terms, and the
rounding of this float64 evaluation itself (2^-53 per operation).
"""
import numpy as np

U = 2.0 ** -24


def _kind(pts, sphere):
    n = pts[:, 3:6].astype(np.float64)
    s = (n * n).sum(1)
    with np.errstate(invalid="ignore"):
        kind = np.where(sphere | (s == 1.0), 1, np.where((s > 0.5) & np.isfinite(s), 2, 0))
    nl = np.where(kind == 2, np.sqrt(np.where(s > 0, s, 1.0)), 1.0)
    return kind, nl


def _cone(c, r2, pts, nl, clamp):
    """d2, s2, omega-free pieces of the weight formulas for one sphere {c, r2} at
    every point: d2, s2 (clamped to 1 if asked), cb and cm"""
    P = pts[:, :3].astype(np.float64)
    n = pts[:, 3:6].astype(np.float64)
    w = c[None].astype(np.float64) - P
    d2 = (w * w).sum(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s2 = np.float64(r2) / d2
        if clamp:
            s2 = np.minimum(1.0, s2)
        cc = (w * n).sum(1) / (np.sqrt(d2) * nl)
        cb = np.maximum(0.0, np.nan_to_num(cc, nan=0.0)) + np.sqrt(np.maximum(s2, 0.0))
        cm = np.sqrt(np.maximum(1.0 - s2, 0.0))
    return d2, s2, cb, cm


def leaf_weights(lights, n_sphere_lights, pts, prims, nl):
    """w_j (n, K) and its error bound, the weight of weighted picking"""
    n, K = len(lights), len(pts)
    W, E = np.zeros((n, K)), np.zeros((n, K))
    for j in range(n):
        l = lights[j]
        poly = j >= n_sphere_lights
        d2, s2, cb, cm = _cone(l["centre"], l["r2"], pts, nl, poly)
        reach = prims != l["prim"]
        if not poly:
            reach &= d2 > np.float64(l["r2"])
        pw = np.abs(l["emitted"].astype(np.float64)).sum()
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            wt = (pw * (s2 / (1.0 + cm))) * cb
            e = U * (14.0 + 19.0 / cb) + np.minimum(np.sqrt(7 * U), 7 * U / cm)
        ok = reach & (wt > 0)
        W[j] = np.where(ok, wt, 0.0)
        E[j] = np.where(ok, e, 0.0)
    return W, E


def node_importances(tree, n, pts, nl):
    """I (n - 1, K) of the internal nodes and its error bound"""
    K = len(pts)
    I, E = np.zeros((n - 1, K)), np.zeros((n - 1, K))
    for k in range(n - 1):
        nd = tree[k]
        d2, s2, cb, _ = _cone(nd["centre"], nd["r2"], pts, nl, True)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            imp = (np.float64(nd["phi"]) / np.maximum(d2, np.float64(nd["r2"]))) * cb
            e = U * (7.0 + 19.0 / cb)
        ok = imp > 0
        I[k] = np.where(ok, imp, 0.0)
        E[k] = np.where(ok, e, 0.0)
    return I, E


def probabilities(tree, lights, n_sphere_lights, pts, prims, n_scene_spheres):
    """What rt_light_pick_probabilities returns with the hierarchy on, by the
    specification: p (K, n), its relative error bound (K, n), the linear weights
    w (K, n) with their bound, and the smallest importance on each light's way
    down (K, n; inf where the way is empty).  Rows of points that are no NEE
    level (kind 0) are 0."""
    n, K = len(lights), len(pts)
    sphere = (prims >= 0) & (prims < n_scene_spheres)
    kind, nl = _kind(pts, sphere)
    W, EW = leaf_weights(lights, n_sphere_lights, pts, prims, nl)
    NI, NE = node_importances(tree, n, pts, nl)
    I = np.concatenate([NI, W])   # by node index: internal nodes, then the leaves
    E = np.concatenate([NE, EW])
    p = np.ones((K, n))
    bound = np.full((K, n), U)
    least = np.full((K, n), np.inf)
    for j in range(n):
        k = n - 1 + j
        while tree[k]["parent"] >= 0:
            up = int(tree[k]["parent"])
            a, b = int(tree[up]["a"]), int(tree[up]["b"])
            S = I[a] + I[b]
            with np.errstate(divide="ignore", invalid="ignore"):
                p[:, j] *= np.where(S > 0, I[k] / S, 0.0)
            bound[:, j] += np.maximum(E[a], E[b]) + E[k] + 3 * U
            least[:, j] = np.minimum(least[:, j], I[k])
            k = up
    dead = kind == 0
    p[dead] = 0.0
    return p, bound, W.T * ~dead[:, None], EW.T, least


def no_pick_mass(tree, lights, n_sphere_lights, pts, prims, n_scene_spheres):
    """The probability (K,) with which the descent ends at a level whose two
    children both have importance 0 (the no-pick rule), found on its own way:
    the probability of reaching each internal node, root first.  1 where the
    root itself has no importance; > 0 below the root where a node's sphere is
    seen from P but none of its leaves is reachable (or has power)."""
    n, K = len(lights), len(pts)
    sphere = (prims >= 0) & (prims < n_scene_spheres)
    kind, nl = _kind(pts, sphere)
    W, _ = leaf_weights(lights, n_sphere_lights, pts, prims, nl)
    NI, _ = node_importances(tree, n, pts, nl)
    I = np.concatenate([NI, W])
    reach = np.zeros((2 * n - 1, K))
    reach[0] = 1.0
    mass = np.zeros(K)
    for k in range(n - 1):  # parents stand in front of their children
        a, b = int(tree[k]["a"]), int(tree[k]["b"])
        S = I[a] + I[b]
        with np.errstate(divide="ignore", invalid="ignore"):
            reach[a] = np.where(S > 0, reach[k] * I[a] / S, 0.0)
            reach[b] = np.where(S > 0, reach[k] * I[b] / S, 0.0)
        mass += np.where(S > 0, 0.0, reach[k])
    mass[kind == 0] = 1.0
    return mass
