"""Float64 numpy restatement of the denoiser's specification (DESIGN.md
"Denoiser", bwidman-raytracer_amd/csrc/rt_denoise.h) and of the first-hit
feature buffers, for the tests: np.exp, shifted-array taps, no library.

Inputs are what the public interface gives: frameSum (H, W, 3) float32 and the
frame count n, and the feature buffers of Renderer.render_aov.  The hit point
P (kept by the library next to the normal) is restated from the camera:
P = o + depth * primary_dir, 0 on a miss.
"""
import numpy as np

K = np.array([3 / 8, 1 / 4, 1 / 16])


def rotation(camera):
    """rotationMatrix3DY(angle[0]) * rotationMatrix3DX(angle[1])."""
    a0, a1 = float(camera.angle[0]), float(camera.angle[1])
    cy, sy, cx, sx = np.cos(a0), np.sin(a0), np.cos(a1), np.sin(a1)
    L = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    U = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return L @ U


def primary_dirs(camera, width, height, ys=None, dx=0.0, dy=0.0):
    """Unit directions (rows, W, 3) of the un-jittered primary rays of rows
    `ys` (default all): pixelPosition (x - W/2, y - H/2, -(W/2) / tan(fov/2))
    with integer halves, rotated, normalised; (dx, dy) a sub-pixel offset."""
    ys = np.arange(height) if ys is None else np.asarray(ys)
    x = np.arange(width, dtype=np.float64) - width // 2 + dx
    y = ys.astype(np.float64) - height // 2 + dy
    with np.errstate(all="ignore"):
        z = -float(width // 2) / np.tan(float(camera.fov) / 2.0)
        pix = np.stack(np.broadcast_arrays(x[None, :], y[:, None], z), -1)
        d = pix @ rotation(camera).T
        return d / np.linalg.norm(d, axis=-1, keepdims=True)


def hit_points(camera, width, height, depth, prim):
    o = np.array([camera.position.x, camera.position.y, camera.position.z], np.float64)
    with np.errstate(all="ignore"):
        P = o + depth.astype(np.float64)[..., None] * primary_dirs(camera, width, height)
    return np.where((prim < 0)[..., None], 0.0, P)


def first_hit(scene, width, height, ys=None, dx=0.0, dy=0.0):
    """Float64 closest hit of spheres and planes (the scenes the feature tests
    make): prim, depth, normal per pixel, the reference's acceptance
    t > nearZero and its sphere root (-b - sqrt(disc)) / 2a."""
    cam = scene.camera
    o = np.array([cam.position.x, cam.position.y, cam.position.z], np.float64)
    d = primary_dirs(cam, width, height, ys, dx, dy)
    shape = d.shape[:-1]
    best_t = np.full(shape, np.inf)
    best_id = np.full(shape, -1, np.int64)
    normal = np.zeros(shape + (3,))
    ns, npl = scene.counts[0], scene.counts[1]
    with np.errstate(all="ignore"):
        for i in range(ns):
            s = scene.spheres[i]
            c = np.array([s.position.x, s.position.y, s.position.z], np.float64)
            xp = o - c
            a = (d * d).sum(-1)
            b = 2.0 * (d @ xp)
            cc = xp @ xp - float(s.radius) ** 2
            disc = b * b - 4 * a * cc
            t = (-b - np.sqrt(disc)) / (2 * a)
            ok = (disc >= 0) & (t > 1e-4) & (t <= best_t)
            best_t = np.where(ok, t, best_t)
            best_id = np.where(ok, i, best_id)
            n = o + t[..., None] * d - c
            normal = np.where(ok[..., None], n / np.linalg.norm(n, axis=-1, keepdims=True), normal)
        for i in range(npl):
            p = scene.planes[i]
            d0 = np.array([p.directions[0].x, p.directions[0].y, p.directions[0].z], np.float64)
            d1 = np.array([p.directions[1].x, p.directions[1].y, p.directions[1].z], np.float64)
            n = np.cross(d0, d1)
            dd = -(n @ np.array([p.origin.x, p.origin.y, p.origin.z], np.float64))
            nd = d @ n
            t = -((n @ o) + dd) / nd
            ok = (np.abs(nd) >= 1e-4) & (t > 1e-4) & (t <= best_t)
            best_t = np.where(ok, t, best_t)
            best_id = np.where(ok, ns + i, best_id)
            normal = np.where(ok[..., None], n / np.linalg.norm(n), normal)
    return best_id, best_t, normal


def tone_map(c):
    """frameSum / n -> ACES -> gamma -> * 255 -> round -> u8 (rt_path.h tone_map
    with n = 1), float64; fminf / to_u8 treat NaN as the C code does."""
    with np.errstate(all="ignore"):
        cc = 0.6 * c
        num = cc * (2.51 * cc + 0.03)
        den = cc * (2.43 * cc + 0.59) + 0.14
        tm = np.fmin(num / den, 1.0)  # fminf: a NaN quotient gives 1
        g = np.sqrt(tm) * 255.0
        r = np.floor(g + 0.5)
        r = np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0))
    out = np.empty(c.shape[:-1] + (4,), np.uint8)
    out[..., :3] = r.astype(np.uint8)
    out[..., 3] = 255
    return out


def denoise_ref(accum, n, normal, P, prim, iterations, sigma_color, sigma_normal, sigma_plane):
    """The filtered linear colour (H, W, 3) float64.  c0 and the three
    per-level constants are formed in float32 as the specification says (they
    are inputs of the filter); everything else is float64."""
    f32 = np.float32
    H, W = prim.shape
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(n)
        c = (inv * accum.astype(f32)).astype(np.float64)
        nrm = normal.astype(np.float64)
        P = P.astype(np.float64)
        miss = prim < 0
        i_n = np.float64(f32(1.0) / (f32(sigma_normal) * f32(sigma_normal)))
        i_p = np.float64(f32(1.0) / (f32(sigma_plane) * f32(sigma_plane)))
        for level in range(iterations):
            s = 1 << level
            sc = f32(sigma_color) * f32(2.0 ** -level)
            i_c = np.float64(f32(1.0) / (sc * sc))
            sum_w = np.zeros((H, W))
            sum_c = np.zeros((H, W, 3))
            for dy in range(-2, 3):
                oy = dy * s
                if abs(oy) >= H:
                    continue
                yp = slice(max(0, -oy), H - max(0, oy))
                yq = slice(max(0, oy), H - max(0, -oy))
                for dx in range(-2, 3):
                    ox = dx * s
                    if abs(ox) >= W:
                        continue
                    xp = slice(max(0, -ox), W - max(0, ox))
                    xq = slice(max(0, ox), W - max(0, -ox))
                    h = K[abs(dy)] * K[abs(dx)]
                    cq = c[yq, xq]
                    dc = cq - c[yp, xp]
                    ec = (dc * dc).sum(-1) * i_c
                    dn = nrm[yq, xq] - nrm[yp, xp]
                    en = (dn * dn).sum(-1) * i_n
                    pd = (nrm[yp, xp] * (P[yq, xq] - P[yp, xp])).sum(-1)
                    ex = (pd * pd) * i_p
                    e = (ec + en) + ex
                    ok = (miss[yq, xq] == miss[yp, xp]) & (e >= 0)
                    w = h * np.exp(-e)
                    ok &= w > 0
                    sum_w[yp, xp] += np.where(ok, w, 0.0)
                    sum_c[yp, xp] += np.where(ok[..., None], w[..., None] * cq, 0.0)
            c = np.where((sum_w > 0)[..., None], sum_c / sum_w[..., None], c)
    return c


def rel_err(got, ref):
    """max |got - ref| / (1 + |ref|) over the entries finite in the reference;
    the others must be the same non-finite values."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), "non-finite entries differ"
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / (1.0 + np.abs(ref[fin]))))
