"""The scenes of tools/light_tree_sweep.py and tools/time_light_tree.py (DESIGN.md
section 29), by the size of their light table: scene 07 (3 lights), the
eight-light row of tests/test_light_picking.py, stress scenes with 64 and 256
emissive spheres (BVH scenes), and an emissive mesh — a wavy sheet of 22 x 23
cells, 1,012 triangles, over scene 07's geometry (a BVH scene as well).
Each entry: name -> (maker, shapes mode)."""
import math
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
from bwrt import scenes  # noqa: E402
from bwrt.abi import Sphere, Triangle, Vec3  # noqa: E402
from bwrt.scenes import material, vec  # noqa: E402


def eight_lights():
    ys = [0.25, 0.4, 0.7, 1.0, 1.5, 2.2, 3.2, 4.5]
    cols = [(1, 0.6, 0.2), (1, 0.2, 0.6), (0.2, 0.8, 0.2), (1, 1, 1), (0.3, 0.5, 1), (1, 1, 0.3), (0.6, 0.3, 1), (1, 0.4, 0.4)]
    sph = [Sphere(vec(-3.5 + i, y, -4.0), 0.2, material(c, 10)) for i, (y, c) in enumerate(zip(ys, cols))]
    sph.append(Sphere(vec(0.5, 0.6, -2.8), 0.6, material((0.8, 0.8, 0.8))))
    return scenes.Scene(scenes.camera_07(), sph, [scenes._floor()], [], [], name="eight_lights")


def emissive_mesh(nx=22, nz=23):
    """Scene 07's geometry, its spheres dark, under a sheet y = 4 + 0.4 sin x cos z
    over [-5.5, 5.5] x [-9.75, 1.75] in cells of 0.5 x 0.5, two triangles each;
    the emittance varies across the sheet by 8x.  (The triangles' un-normalised
    normals have length 1/4: hits on the sheet itself take no light sample.)"""
    s = scenes.scene_07()
    for i in range(s.counts[0]):
        s.spheres[i].mat.emittance = 0.0
    k = 0.5
    y = lambda x, z: 4.0 + 0.4 * math.sin(x) * math.cos(z)
    tris = []
    for i in range(nx):
        for j in range(nz):
            x0, z0 = (i - nx / 2) * k, -4.0 + (j - nz / 2) * k
            a = vec(x0, y(x0, z0), z0)
            b = vec(x0 + k, y(x0 + k, z0), z0)
            c = vec(x0 + k, y(x0 + k, z0 + k), z0 + k)
            d = vec(x0, y(x0, z0 + k), z0 + k)
            m = material((1, 0.9, 0.8), 0.25 * (1.0 + ((i * 7 + j * 3) % 8)))
            tris += [Triangle((Vec3 * 3)(a, b, d), m), Triangle((Vec3 * 3)(c, d, b), m)]
    n = s.counts
    return scenes.Scene(s.camera, list(s.spheres)[:n[0]], list(s.planes)[:n[1]], list(s.triangles)[:n[2]] + tris, [],
                        name="emissive_mesh")


TABLES = {
    "3": (scenes.scene_07, "spheres"),
    "8": (eight_lights, "spheres"),
    "64": (lambda: scenes.stress_scene(2000, 96, 64), "spheres"),
    "256": (lambda: scenes.stress_scene(2000, 288, 256), "spheres"),
    "1012": (emissive_mesh, "all"),
}
