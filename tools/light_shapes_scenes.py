"""The scenes of tools/time_light_shapes.py and tools/light_shapes_sweep.py
(tests/test_light_shapes.py builds the same ones): scene
07's geometry under a ceiling panel of four unit quads (unit normals: the
reference shades polygons with their un-normalised normal), the same panel as
eight triangles, scene 07 with its three sphere lights and the panel, and the
stress scene with four of its triangles made emissive."""
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
from bwrt import scenes  # noqa: E402
from bwrt.abi import Quad, Triangle, Vec3  # noqa: E402
from bwrt.scenes import material, vec  # noqa: E402


def _panel(kind):
    m = material((1, 0.9, 0.7), 12)
    out = []
    for x in (-1, 0):
        for z in (-5, -4):
            a, b, c, d = vec(x, 4, z), vec(x + 1, 4, z), vec(x + 1, 4, z + 1), vec(x, 4, z + 1)
            if kind == "quads":
                out.append(Quad((Vec3 * 4)(a, b, c, d), m))
            else:
                out += [Triangle((Vec3 * 3)(a, b, d), m), Triangle((Vec3 * 3)(c, d, b), m)]
    return out


def _with(s, triangles=(), quads=(), name=""):
    n = s.counts
    return scenes.Scene(s.camera, list(s.spheres)[:n[0]], list(s.planes)[:n[1]], list(s.triangles)[:n[2]] + list(triangles),
                        list(s.quads)[:n[3]] + list(quads), name=name)


def _dark_07():
    s = scenes.scene_07()
    for i in range(s.counts[0]):
        s.spheres[i].mat.emittance = 0.0
    return s


def quad_panel():
    return _with(_dark_07(), quads=_panel("quads"), name="quad_panel")


def triangle_panel():
    return _with(_dark_07(), triangles=_panel("triangles"), name="triangle_panel")


def mixed():
    return _with(scenes.scene_07(), quads=_panel("quads"), name="mixed")


def stress_with_emissive_triangles(lit=(3, 17, 4242, 9999)):
    s = scenes.stress_scene()
    for i in lit:
        s.triangles[i].mat.emittance = 15.0
    return s
