"""Light tables and shading points shared by tests/test_light_tree.py (CPU) and
tests/test_gpu_light_tree.py: the scenes whose tables have 2, 3, 5, 8, 40 and
256 sphere lights, a mixed table and a 40-quad panel, and for each of them a
seeded set of points {P, n, prim} for rt_light_pick_probabilities.

Nothing here looks at what the library computes: the point sets depend on the
scene's geometry and the tree's stored spheres alone.
"""
import numpy as np

from bwrt import Renderer, scenes
from test_light_picking import eight_lights, small_normal_scene
from test_light_shapes import forty_quads, mixed, stress_with_emissive_triangles


def five_lights():
    s = eight_lights()
    sph = list(s.spheres)[:5] + [list(s.spheres)[8]]
    return scenes.Scene(s.camera, sph, [scenes._floor()], [], [], name="five_lights")


def forty_spheres():
    """tests/test_gpu_light_picking.py's long table: over 16 KB of hit table"""
    return scenes.stress_scene(n_triangles=400, n_spheres=48, n_emissive=40)


def sixty_four_lights():
    return scenes.stress_scene(n_triangles=200, n_spheres=96, n_emissive=64)


def many_spheres():
    return scenes.stress_scene(n_triangles=200, n_spheres=260, n_emissive=256)


# name -> (scene maker, shapes mode, number of table lights)
TABLES = {
    "2": (small_normal_scene, "spheres", 2),
    "3": (scenes.scene_07, "spheres", 3),
    "5": (five_lights, "spheres", 5),
    "8": (eight_lights, "spheres", 8),
    "40": (forty_spheres, "spheres", 40),
    "256": (many_spheres, "spheres", 256),
    "mixed": (mixed, "all", 7),
    "quads": (forty_quads, "all", 40),
}


def long_mixed():
    """forty_spheres with four of its triangles made emissive: 44 records of both
    kinds over more than 16 KB of hit table"""
    s = forty_spheres()
    for i in (3, 17, 142, 399):
        s.triangles[i].mat.emittance = 15.0
    return s


# what only the GPU comparison renders: polygon records with the hit table in global memory and behind the BVH walk
RENDER_TABLES = {**TABLES, "long_mixed": (long_mixed, "all", 44), "stress_tris": (stress_with_emissive_triangles, "all", 12)}


def renderer(lib, name, pick="weighted", hierarchy=True, gpu=False, on=True):
    make, shapes, _ = RENDER_TABLES[name]
    r = Renderer(0, lib=lib) if gpu else Renderer.cpu(0, lib=lib)
    r.set_scene(make())
    r.set_light_sampling(on)
    r.set_light_picking(pick)
    r.set_light_shapes(shapes)
    r.set_light_hierarchy(hierarchy)
    return r


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
# |n|^2 in (1/2, inf) and not 1: kind 2 (csrc/rt_light.h nee_normal_kind)
KIND2 = np.array([[0, 0.8, 0], [0.3, 1.1, -0.2], [-0.5, 0.5, 0.5], [0.1, -0.2, 3.0]], np.float32)

MARGIN = 1e-4  # every point keeps |d2 - r2| > MARGIN r2 to every sphere light: no reachability toss-up


def points_of(name, lights, tree, scene, seed=7, per_kind=120):
    """(points (K, 6) float32, prims (K,) int32, kinds (K,) of str).  The kinds:
    floor (on the floor plane), light (on a table light, prim its own), inside
    (inside an internal node's sphere, free normals), kind2 (the same with
    non-unit normals), beside (on the floor next to the lowest light)."""
    rng = np.random.default_rng(seed)
    n_sph_scene = scene.counts[0]
    floor_prim = n_sph_scene  # the first plane
    n = len(lights)
    pts, prims, kinds = [], [], []

    def put(P, nrm, prim, kind):
        pts.append(np.concatenate([np.asarray(P, np.float32), np.asarray(nrm, np.float32)]))
        prims.append(prim)
        kinds.append(kind)

    c = lights["centre"].astype(np.float64)
    lo, hi = c.min(0) - 3.0, c.max(0) + 3.0
    for _ in range(per_kind):
        put([rng.uniform(lo[0], hi[0]), 0.0, rng.uniform(lo[2], hi[2])], [0, 1, 0], floor_prim, "floor")
    for k in range(per_kind):
        j = k % n
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if lights["prim"][j] < n_sph_scene:
            r = np.sqrt(np.float64(lights["r2"][j]))
            P = (c[j] + r * u).astype(np.float32)
            nrm = (P.astype(np.float64) - c[j])
            put(P, (nrm / np.linalg.norm(nrm)).astype(np.float32), int(lights["prim"][j]), "light")
        else:  # a polygon: its bounding sphere's centre lies on it (the vertices' mean)
            put(c[j].astype(np.float32), AXES[3], int(lights["prim"][j]), "light")
    internal = tree[: n - 1]
    for k in range(2 * per_kind):
        nd = internal[k % len(internal)]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        P = nd["centre"].astype(np.float64) + rng.uniform(0.0, 0.95) * np.sqrt(np.float64(nd["r2"])) * u
        if k < per_kind:
            put(P, AXES[rng.integers(len(AXES))], -1, "inside")
        else:
            put(P, KIND2[rng.integers(len(KIND2))], -1, "kind2")
    low = int(np.argmin(c[:, 1]))
    r_low = np.sqrt(np.float64(lights["r2"][low]))
    for _ in range(per_kind):
        a = rng.uniform(0, 2 * np.pi)
        d = r_low * 10.0 ** rng.uniform(-2.0, 0.5)  # from a hundredth of the radius beside the foot point
        put([c[low][0] + d * np.cos(a), 0.0, c[low][2] + d * np.sin(a)], [0, 1, 0], floor_prim, "beside")
    pts, prims, kinds = np.array(pts, np.float32), np.array(prims, np.int32), np.array(kinds)
    # the margin rule, in float64 on the float32 points
    sph = lights["prim"] < n_sph_scene
    d2 = ((c[None, sph] - pts[:, None, :3].astype(np.float64)) ** 2).sum(-1)
    r2 = lights["r2"][sph].astype(np.float64)[None]
    own = prims[:, None] == lights["prim"][sph][None]
    keep = (own | (np.abs(d2 - r2) > MARGIN * r2)).all(1)
    return pts[keep], prims[keep], kinds[keep]


def far_points(lights, scene, seed=11, count=64):
    """Floor-normal points 1e12 .. 1e19.5 away: phi / d2 goes through the float32
    denormals to 0, and d2 itself overflows at the far end."""
    rng = np.random.default_rng(seed)
    pts = []
    for _ in range(count):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        pts.append(np.concatenate([10.0 ** rng.uniform(12.0, 19.5) * u, [0, 1, 0]]))
    return np.array(pts, np.float32), np.full(count, -1, np.int32)
