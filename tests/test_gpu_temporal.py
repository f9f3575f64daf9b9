"""Temporal reprojection on the MI355X: the HIP kernel against the CPU backend,
bit for bit (both run the arithmetic of csrc/rt_temporal.h).  Each test runs
the same sequence of views on a GPU and on a CPU context, both seeded by
init_rand: the renders are bit-identical (tests/test_gpu_parity.py), so every
temporal output must be too.
"""
import numpy as np
import pytest

from bwrt import Renderer, scenes
from test_temporal import BOUNCES, FRAMES, MOVES, SECOND, moved, special_sequence, view, view_a

pytestmark = pytest.mark.gpu

KEYS = ("rgba", "color", "length")


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def assert_same_views(got, want):
    assert len(got) == len(want)
    for i, (g, c) in enumerate(zip(got, want)):
        for k in KEYS:
            assert same(g[k], c[k]), (i, k)


def walk(r, name, w, h, move, denoise_last=None):
    """Views A, B = A + move, C = B + SECOND on a freshly seeded context; the
    last call again with the spatial filter when asked."""
    scene = scenes.SCENES[name]()
    r.set_scene(scene)
    r.init_rand(w, h)
    cams = [view_a(scene)]
    cams.append(moved(cams[0], **MOVES[move]))
    cams.append(moved(cams[1], **SECOND))
    out = [view(r, c, w, h) for c in cams]
    if denoise_last is not None:
        rgba, col, ln = r.temporal(w, h, denoise=denoise_last, want_color=True, want_length=True)
        out.append({"rgba": rgba, "color": col, "length": ln})
    return out


@pytest.mark.parametrize("name,w,h,move", [
    ("07", 67, 45, "yaw"), ("07", 67, 45, "sideways"), ("07", 67, 45, "dolly"),
    ("07", 333, 187, "yaw"), ("07", 333, 187, "sideways"),
    ("04_box", 64, 36, "sideways"),  # quads
    ("stress", 96, 54, "dolly"),     # the guides of the BVH walk
])
def test_equals_cpu(gpu, cpu, name, w, h, move):
    g = walk(gpu, name, w, h, move, denoise_last={})
    c = walk(cpu, name, w, h, move, denoise_last={})
    assert_same_views(g, c)
    assert (c[1]["length"] > FRAMES).any() and c[2]["length"].max() > 2 * FRAMES  # chained histories
    assert not same(c[3]["color"], c[2]["color"])  # the filter kernels read the temporal buffer
    assert same(c[3]["length"], c[2]["length"])
    assert gpu.last_temporal_ms() > 0


@pytest.mark.parametrize("variant", ["direct", "tiled"])
def test_filtered_walk_equals_cpu_forced_variant(monkeypatch, bwrt_lib, cpu, variant):
    """The filter behind the reprojection with a forced level variant, six
    levels (step 32 included): the one path on which the plain filter's level-0
    source carries a non-zero .w, the history length, through the tile."""
    monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)  # read at rt_create (BWRT_TUNING=1)
    with Renderer(0, lib=bwrt_lib) as r:
        g = walk(r, "07", 67, 45, "yaw", denoise_last={"iterations": 6})
    c = walk(cpu, "07", 67, 45, "yaw", denoise_last={"iterations": 6})
    assert_same_views(g, c)
    assert (c[3]["length"] > 0).all() and not same(c[3]["color"], c[2]["color"])


def test_equals_cpu_zero_iterations_and_parameters(gpu, cpu):
    out = []
    for r in (gpu, cpu):
        walk(r, "07", 67, 45, "yaw")
        out.append([r.temporal(67, 45, denoise={"iterations": 0}, want_color=True, want_length=True),
                    r.temporal(67, 45, max_history=2.0, normal_cos_min=0.999, plane_tol=1e-3, want_color=True,
                               want_length=True),
                    r.temporal(67, 45, denoise={"iterations": 6}, want_color=True, want_length=True)])
    for g, c in zip(*out):
        assert all(same(x, y) for x, y in zip(g, c))


def test_special_values_equal_cpu(gpu, cpu):
    w, h = 67, 45
    vals = ((np.nan, np.inf, -np.inf), (np.inf, -np.inf, np.nan))
    gh, gv, gpx, gcur = special_sequence(gpu, w, h, *vals)
    ch, cv, cpx, ccur = special_sequence(cpu, w, h, *vals)
    assert gpx == cpx and gcur == ccur
    assert same(gh["color"], ch["color"]) and same(gh["length"], ch["length"])
    for k in KEYS:
        assert same(gv[k], cv[k]), k
    others = np.ones((h, w), bool)
    for p in gcur:
        others[p] = False
    assert np.isfinite(gv["color"][others]).all()


def test_state_is_untouched(gpu):
    scene = scenes.scene_07()
    w, h = 64, 36
    out = []
    for with_temporal in (True, False):
        gpu.set_scene(scene)
        gpu.init_rand(w, h)
        gpu.temporal_reset()
        t = (lambda: gpu.temporal(w, h, denoise={})) if with_temporal else (lambda: None)
        gpu.render(w, h, 2, BOUNCES, first_frame=1)
        before = gpu.get_state(h, w)
        t()
        after = gpu.get_state(h, w)
        assert np.array_equal(before[0], after[0]) and same(before[1], after[1])
        gpu.render(w, h, 1, BOUNCES)
        gpu.set_camera(moved(scene.camera, **MOVES["yaw"]))
        gpu.render(w, h, 2, BOUNCES)
        t()
        img = gpu.render(w, h, 1, BOUNCES)
        out.append((img, gpu.frame_counter) + gpu.get_state(h, w))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] == 4
    assert np.array_equal(out[0][2], out[1][2]) and same(out[0][3], out[1][3])


def test_repeated_calls_are_identical(gpu):
    """The same call five times in a row: no race between the taps of the
    history and the stores of the pending result (they are different sets)."""
    w, h = 333, 187
    walk(gpu, "07", w, h, "yaw")
    for dn in (None, {}):
        first = gpu.temporal(w, h, denoise=dn, want_color=True, want_length=True)
        for _ in range(4):
            again = gpu.temporal(w, h, denoise=dn, want_color=True, want_length=True)
            assert all(same(x, y) for x, y in zip(first, again))


def test_device_output_and_stream_ordering(gpu, cpu):
    import torch
    scene = scenes.scene_07()
    w, h = 160, 90
    ca = view_a(scene)
    cb = moved(ca, **MOVES["yaw"])
    # the CPU context computes what every device buffer must hold
    cpu.set_scene(scene)
    cpu.init_rand(w, h)
    want_a = view(cpu, ca, w, h)
    want_b = view(cpu, cb, w, h)
    want_dn = cpu.denoise(w, h)
    want_b_filtered = cpu.temporal(w, h, denoise={})
    cpu.render(w, h, 1, BOUNCES)
    want_b4 = cpu.temporal(w, h)

    def image(t):
        return t.cpu().numpy().view(np.uint8).reshape(h, w, 4)

    gpu.set_scene(scene)
    gpu.init_rand(w, h)
    gpu.temporal_reset()
    bufs = [torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(6)]
    raw, t_a, t_b, dn, t_f, t_4 = bufs
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `stream`)
    s = stream.cuda_stream
    # view A: render and temporal call on the caller's stream, then view B's render (it resets
    # frameSum, which the temporal call reads) right behind them
    gpu.set_camera(ca)
    gpu.render_device(gpu.params(w, h, FRAMES, BOUNCES), raw.data_ptr(), s)
    gpu.temporal_device(t_a.data_ptr(), s)
    gpu.set_camera(cb)
    gpu.render_device(gpu.params(w, h, FRAMES, BOUNCES), raw.data_ptr(), s)
    # view B's temporal call on the context's stream (after the render on the caller's), a denoise of
    # the frame on the caller's stream behind it (shared guides), a filtered temporal call there too
    gpu.temporal_device(t_b.data_ptr(), None)
    gpu.denoise_device(dn.data_ptr(), s)
    gpu.temporal_device(t_f.data_ptr(), s, denoise={})
    # a render on the context's stream right behind the filtered call on the caller's, and a temporal
    # call of the longer frame behind that
    gpu.render_device(gpu.params(w, h, 1, BOUNCES), raw.data_ptr(), None)
    gpu.temporal_device(t_4.data_ptr(), s)
    stream.synchronize()
    gpu.synchronize()
    assert np.array_equal(image(t_a), want_a["rgba"])
    assert np.array_equal(image(t_b), want_b["rgba"])
    assert np.array_equal(image(dn), want_dn)
    assert np.array_equal(image(t_f), want_b_filtered)
    assert np.array_equal(image(t_4), want_b4)
    assert not np.array_equal(image(t_b), image(t_f))
    assert gpu.last_temporal_ms() > 0
    # the synchronous call in the same view: the same bits as the device variant
    assert np.array_equal(gpu.temporal(w, h), want_b4)


def test_precision_mode_does_not_reach_the_pass(bwrt_lib, cpu):
    """The unit is built once with the exact flags: a context that renders in
    the reference-fast mode reprojects the same state to the same bits."""
    scene = scenes.scene_07()
    w, h = 67, 45
    cams = [view_a(scene)]
    cams.append(moved(cams[0], **MOVES["sideways"]))
    cpu.set_scene(scene)
    cpu.init_rand(w, h)
    want, states = [], []
    for c in cams:
        want.append(view(cpu, c, w, h))
        states.append(cpu.get_state(h, w))
    with Renderer(0, lib=bwrt_lib) as r:
        r.set_precision("fast")
        r.set_scene(scene)
        r.init_rand(w, h)
        for c, (rng, acc), v in zip(cams, states, want):
            r.set_camera(c)
            r.set_state(rng, acc, FRAMES + 1)
            got = r.temporal(w, h, want_color=True, want_length=True)
            assert all(same(x, v[k]) for x, k in zip(got, KEYS))
