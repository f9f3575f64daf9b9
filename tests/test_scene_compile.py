"""The scene compiler (csrc/rt_scene.cpp) on its own: a stand-alone program,
compiled here with g++ against rt_scene.cpp alone (no HIP, no context), reads
scene files as the host CLI does and prints an FNV-1a-64 digest of the
compiled float buffer with every offset, count and bound.  The digests in
tests/golden/compiled_scene_digests.json were taken from the library before
the compiler became its own unit: they pin the compiled bytes and with them
the shape of the BVH.  CPU only."""
import json
import os
import subprocess

import pytest

from bwrt import scenefile, scenes
from scenegen import _random_scene, _scaled

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "bwidman-raytracer_amd")
GOLDEN = os.path.join(REPO, "tests", "golden", "compiled_scene_digests.json")

PROGRAM = r'''
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "scene_file.hpp"
#include "rt_scene.h"

static rt_scene view(const bwrt::SceneData& sd) {
    rt_scene s;
    s.camera = sd.camera;
    s.spheres = sd.spheres.data(), s.sphere_count = (int)sd.spheres.size();
    s.planes = sd.planes.data(), s.plane_count = (int)sd.planes.size();
    s.triangles = sd.triangles.data(), s.triangle_count = (int)sd.triangles.size();
    s.quads = sd.quads.data(), s.quad_count = (int)sd.quads.size();
    return s;
}

static void print(const rt_compiled_scene& c) {
    uint64_t h = 1469598103934665603ull;  // FNV-1a-64 over the bytes of the float buffer
    const unsigned char* b = (const unsigned char*)c.data.data();
    for (size_t i = 0; i < c.data.size() * 4; i++) h = (h ^ b[i]) * 1099511628211ull;
    auto bits = [](float f) { unsigned u; std::memcpy(&u, &f, 4); return u; };
    std::printf("fnv=%016llx floats=%zu n=%d,%d,%d,%d off=%zu,%zu,%zu,%zu bvh=%zu,%zu,%zu,%zu nodes=%d mask=%d "
                "cull=%08x,%08x ovf=%08x,%08x,%08x\n",
                (unsigned long long)h, c.data.size(), c.n_sph, c.n_pln, c.n_tri, c.n_quad, c.off_pln, c.off_tri,
                c.off_quad, c.off_hit, c.off_bvh, c.off_bvh_prims, c.off_bvh_vtx, c.off_bvh16, c.bvh_nodes_per_order,
                c.bvh_order_mask, bits(c.cull_omax), bits(c.cull_dmax), bits(c.ovf_sc), bits(c.ovf_nm),
                bits(c.ovf_im));
}

// --lights: the light table of next-event estimation as tools/nee_probe.hip
// reads it: {n_lights, n_sphere_lights, n_sph, 0}, the records, the polygon blocks
static bool dump_lights(const rt_compiled_scene& c, const char* path) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const int32_t head[4] = {(int32_t)(c.lights.size() / RT_LIGHT_RECORD_FLOATS), c.n_sphere_lights, c.n_sph, 0};
    bool ok = std::fwrite(head, 4, 4, f) == 4;
    ok = ok && std::fwrite(c.lights.data(), 4, c.lights.size(), f) == c.lights.size();
    ok = ok && std::fwrite(c.light_polys.data(), 4, c.light_polys.size(), f) == c.light_polys.size();
    return std::fclose(f) == 0 && ok;
}

// usage: prog scene.txt [BWRT_KNOB=value ...] [--then-fail] [--lights out.bin]
int main(int argc, char** argv) {
    bwrt::SceneData sd;
    const std::string e = bwrt::load_scene(argv[1], sd);
    if (!e.empty()) return std::fprintf(stderr, "%s\n", e.c_str()), 2;
    rt_scene_options opt;
    bool then_fail = false;
    const char* lights = nullptr;
    for (int i = 2; i < argc; i++) {
        if (!std::strcmp(argv[i], "--then-fail")) { then_fail = true; continue; }
        if (!std::strcmp(argv[i], "--lights") && i + 1 < argc) { lights = argv[++i]; continue; }
        char* eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        *eq = 0;
        if (!rt_scene_option_set(opt, argv[i], eq + 1)) return std::fprintf(stderr, "no knob %s\n", argv[i]), 2;
    }
    rt_compiled_scene out;
    std::string err;
    int rc = rt_compile_scene(view(sd), opt, out, err);
    if (rc) return std::fprintf(stderr, "%d %s\n", rc, err.c_str()), 1;
    print(out);
    if (lights && !dump_lights(out, lights)) return std::fprintf(stderr, "cannot write %s\n", lights), 2;
    if (then_fail) {
        // 2^24 spheres, the smallest scene the compiler refuses (it does so
        // after it has compiled every primitive record): `out` must stay
        std::vector<rt_sphere> many((size_t)1 << 24, rt_sphere{{0, 0, 0}, 1.0f, bwrt::mat(rt_vec3{1, 1, 1})});
        bwrt::SceneData big;
        big.camera = sd.camera;
        big.spheres.swap(many);
        rc = rt_compile_scene(view(big), opt, out, err);
        std::printf("rc=%d err=%s\n", rc, err.c_str());
        print(out);
    }
    return 0;
}
'''


def cases():
    """(name, scene factory, knobs): every built-in scene, the stress scene at
    two extreme scales of test_stress_bvh_scaled (3e4: boxes beyond fp16, so
    no 16-byte nodes; 1e10: every test overflows) and four random scenes,
    each with the default options and with a BVH forced (BWRT_BVH_MIN=1), and
    the stress scene once without spatial splits."""
    named = [(k, f) for k, f in scenes.SCENES.items()]
    named += [(f"stress_x{k:g}", lambda k=k: _scaled(scenes.stress_scene(), k)) for k in (3e4, 1e10)]
    named += [(f"random{seed}", lambda seed=seed: _random_scene(seed)) for seed in range(4)]
    out = []
    for name, make in named:
        out.append((name, make, {}))
        out.append((name + "+bvh_min1", make, {"BWRT_BVH_MIN": "1"}))
    out.append(("stress+sbvh0", scenes.stress_scene, {"BWRT_BVH_SBVH": "0"}))
    return out


def compile_program(d):
    """The stand-alone program built in directory d (tests/test_nee_reference.py
    builds it too, for its --lights dump)."""
    src = d / "main.cpp"
    src.write_text(PROGRAM)
    exe = d / "scene_compile"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "host"),
                    "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src),
                    os.path.join(PKG, "csrc", "rt_scene.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_compile")
    exe = compile_program(d)
    files = {}

    def run(name, make, knobs, *extra):
        key = name.split("+")[0]
        if key not in files:  # one file per scene, shared by its cases
            files[key] = d / (key + ".txt")
            scenefile.save(str(files[key]), make())
        args = [f"{k}={v}" for k, v in knobs.items()]
        r = subprocess.run([str(exe), str(files[key]), *args, *extra], check=True, capture_output=True, text=True)
        return r.stdout.splitlines()
    return run


def test_compiled_scenes_match_the_recorded_digests(prog):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {name: prog(name, make, knobs)[0] for name, make, knobs in cases()}
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}
    # the brute-force scenes stay brute force, and the forced ones get a tree
    assert " bvh=0,0,0,0 " in got["04"] and " bvh=0,0,0,0 " in got["07"]
    assert " bvh=0,0,0,0 " not in got["04+bvh_min1"] and " bvh=0,0,0,0 " not in got["07+bvh_min1"]


def test_failed_compile_leaves_its_output_untouched(prog):
    """No scene below the BVH's 2^24-primitive limit fails after compilation
    has begun, so this runs at the limit, at the rt_compile_scene level: the
    result of an earlier compile survives the refused one bit for bit."""
    before, status, after = prog("07+bvh_min1", scenes.scene_07, {"BWRT_BVH_MIN": "1"}, "--then-fail")
    assert status == "rc=-6 err=16777216 bounded primitives: the BVH holds at most 2^24 - 1"  # RT_ERR_UNSUPPORTED
    assert after == before
