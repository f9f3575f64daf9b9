"""rt_temporal_var on the MI355X: the HIP kernels of csrc/rt_temporal_var.hip
against the CPU backend, bit for bit (both run the arithmetic of
csrc/rt_temporal_var.h).  Each test runs the same sequence of views on a GPU and
on a CPU context, both seeded by init_rand: the renders are bit-identical
(tests/test_gpu_parity.py), so every output must be too.
"""
import numpy as np
import pytest

import assemble_case as A
from bwrt import Renderer, scenes
from test_temporal import BOUNCES, MOVES, SECOND, moved, view_a
from test_temporal_var import SKY, path, render_view, special_sequence, tv

pytestmark = pytest.mark.gpu

CHAIN = [MOVES["yaw"], MOVES["sideways"], MOVES["dolly"], SECOND]
FILTER = {"iterations": 3, "sigma_lum": 4.0, "min_batches": 3}


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


@pytest.fixture(scope="module")
def dev(bwrt_lib):
    """A GPU context of this module's own: the tests switch tracking and the background."""
    if bwrt_lib.rt_device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X")
    r = Renderer(0, lib=bwrt_lib)
    yield r
    r.close()


def same(a, b):
    """Equal values, NaN equal to NaN (the 1x1 frame's camera ray is NaN, of either sign)."""
    return A.same_values(a, b)


def walk(r, name, w, h, moves, mode, dv_last=FILTER, sky=True):
    """The views of `moves` on a freshly seeded context, 3 frames each, one
    unfiltered call per view, then the filtered call in the last view.  mode:
    "untracked", "tracked" (every view as calls of 2 + 1 frames: J = 2) or
    "plain" (view A's call is rt_temporal's: a history without a moment plane)."""
    scene = scenes.SCENES[name]()
    r.set_scene(scene)
    r.set_background(*(SKY if sky else (0, 0, 0)))
    r.set_moments(mode == "tracked")
    r.init_rand(w, h)
    r.temporal_reset()
    out = []
    for i, cam in enumerate(path(scene, moves)):
        render_view(r, cam, w, h, (2, 1) if mode == "tracked" else (3,))
        if i == 0 and mode == "plain":
            out.append(r.temporal(w, h, want_color=True, want_length=True))
        else:
            out.append(tv(r, w, h))
    if dv_last is not None:
        out.append(tv(r, w, h, dv_last))
    r.set_moments(False)
    r.set_background(0, 0, 0)
    return out


SHAPES = [
    ("07", 67, 45, [MOVES["yaw"], SECOND]), ("07", 67, 45, [MOVES["sideways"], SECOND]),
    ("07", 67, 45, [MOVES["dolly"], SECOND]), ("07", 67, 45, CHAIN),
    ("07", 333, 187, [MOVES["yaw"], SECOND]),  # partial 32 x 8 groups on both edges
    ("07", 5, 3, [MOVES["yaw"], SECOND]), ("07", 1, 1, [MOVES["yaw"]]),
    ("stress", 96, 54, [MOVES["dolly"], SECOND]),  # the guides of the BVH walk
]


@pytest.mark.parametrize("mode", ["untracked", "tracked", "plain"])
@pytest.mark.parametrize("name,w,h,moves", SHAPES,
                         ids=["yaw", "sideways", "dolly", "chained", "333x187", "5x3", "1x1", "stress"])
def test_equals_cpu(dev, cpu, name, w, h, moves, mode):
    g = walk(dev, name, w, h, moves, mode)
    c = walk(cpu, name, w, h, moves, mode)
    assert len(g) == len(c) == len(moves) + 2
    for i, (x, y) in enumerate(zip(g, c)):
        assert same(x, y), i
    assert dev.last_temporal_var_ms() > 0
    if w >= 64:  # the sequence did what it is for
        dof = c[-2][3][..., 1]
        assert dof.max() >= (len(moves) if mode != "tracked" else 2 * len(moves) + 1) - 1e-3
        assert (dof >= 1.5).any() and (dof < 1.5).any()  # both sources of the input stage
        assert not same(c[-1][1], c[-2][1]) and same(c[-1][2], c[-2][2])


@pytest.mark.parametrize("variant", ["direct", "tiled", None])
def test_levels_equal_cpu(monkeypatch, bwrt_lib, cpu, variant):
    """Levels 0..6 (step 32 included) behind the reprojection, with a forced level variant and with the policy."""
    if variant:
        monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)  # read at rt_create (BWRT_TUNING=1)
    w, h = 67, 45
    res = []
    with Renderer(0, lib=bwrt_lib) as r:
        for x in (r, cpu):
            walk(x, "07", w, h, CHAIN, "untracked", dv_last=None)
            res.append([tv(x, w, h, dict(FILTER, iterations=it)) for it in range(7)])
    for it, (g, c) in enumerate(zip(*res)):
        assert same(g, c), it
    assert not same(res[1][6][1], res[1][5][1])


def test_five_levels_on_partial_groups(dev, cpu):
    w, h = 333, 187
    dv = dict(FILTER, iterations=5)
    g = walk(dev, "07", w, h, [MOVES["sideways"], SECOND], "tracked", dv_last=dv)
    c = walk(cpu, "07", w, h, [MOVES["sideways"], SECOND], "tracked", dv_last=dv)
    assert same(g, c)


def test_parameters_reach_the_kernel(dev, cpu):
    out = []
    for r in (dev, cpu):
        walk(r, "07", 67, 45, [MOVES["yaw"], SECOND], "untracked", dv_last=None)
        out.append([tv(r, 67, 45, max_history=2.0, normal_cos_min=0.999, plane_tol=1e-3),
                    tv(r, 67, 45, dict(FILTER, min_batches=2)), tv(r, 67, 45, dict(FILTER, min_batches=8))])
    for g, c in zip(*out):
        assert same(g, c)
    assert not same(out[1][1], out[1][2])


def test_special_values_equal_cpu(dev, cpu):
    w, h = 67, 45
    vals = ((np.nan, np.inf, np.inf), (np.inf, np.nan, np.inf))
    dv = dict(iterations=3, sigma_lum=4.0, min_batches=2)
    g = special_sequence(dev, w, h, *vals, dv)
    c = special_sequence(cpu, w, h, *vals, dv)
    dev.set_background(0, 0, 0)
    cpu.set_background(0, 0, 0)
    assert g[6] == c[6] and g[7] == c[7]
    assert same(g[4], c[4]) and same(g[5], c[5])
    others = np.ones((h, w), bool)
    for p in g[7]:
        others[p] = False
    for res in (g[4], g[5]):
        assert np.isfinite(res[1][others]).all() and np.isfinite(res[3][others]).all()


def test_repeated_sequences_are_identical(dev):
    """The same sequence five times: no race between the taps of the history
    and the stores of the pending result (they are different sets), none in the
    input stage's window over the pending colours."""
    first = walk(dev, "07", 333, 187, [MOVES["yaw"], SECOND], "tracked")
    for _ in range(4):
        assert A.same(walk(dev, "07", 333, 187, [MOVES["yaw"], SECOND], "tracked"), first)


def test_precision_mode_does_not_reach_the_pass(bwrt_lib, cpu):
    """The unit is built once with the exact flags: a context that renders in
    the reference-fast mode reprojects the same state to the same bits."""
    scene = scenes.scene_07()
    w, h = 67, 45
    cams = path(scene, [MOVES["sideways"]])
    cpu.set_scene(scene)
    cpu.init_rand(w, h)
    cpu.temporal_reset()
    want, states = [], []
    for c in cams:
        render_view(cpu, c, w, h, (3,))
        want.append((tv(cpu, w, h), tv(cpu, w, h, FILTER)))
        states.append(cpu.get_state(h, w))
    with Renderer(0, lib=bwrt_lib) as r:
        r.set_precision("fast")
        r.set_scene(scene)
        r.init_rand(w, h)
        for c, (rng, acc), v in zip(cams, states, want):
            r.set_camera(c)
            r.set_state(rng, acc, 3 + 1)
            assert same((tv(r, w, h), tv(r, w, h, FILTER)), v)


def test_state_is_untouched(dev):
    scene = scenes.scene_07()
    w, h = 64, 36
    out = []
    for with_calls in (True, False):
        dev.set_scene(scene)
        dev.set_moments(True)
        dev.init_rand(w, h)
        dev.temporal_reset()
        t = (lambda dv=None: tv(dev, w, h, dv)) if with_calls else (lambda dv=None: None)
        dev.render(w, h, 2, BOUNCES, first_frame=1)
        before = dev.get_state(h, w)
        t({})
        assert A.same(dev.get_state(h, w), before)
        dev.render(w, h, 1, BOUNCES)
        t()
        mid = (dev.moments_batches, dev.variance(h, w))
        dev.set_camera(moved(scene.camera, **MOVES["yaw"]))
        dev.render(w, h, 2, BOUNCES)
        t()
        t(FILTER)
        img = dev.render(w, h, 1, BOUNCES)
        out.append((mid, img, dev.frame_counter, dev.moments_batches, dev.variance(h, w)) + tuple(dev.get_state(h, w)))
    dev.set_moments(False)
    assert A.same(out[0], out[1]) and out[0][2] == 4 and out[0][3] == 2


def test_device_output_and_stream_ordering(dev, cpu):
    import torch
    scene = scenes.scene_07()
    w, h = 160, 90
    ca = view_a(scene)
    cb = moved(ca, **MOVES["yaw"])
    dvp = {"iterations": 2}
    # the CPU context computes what every device buffer must hold
    cpu.set_scene(scene)
    cpu.init_rand(w, h)
    cpu.temporal_reset()
    render_view(cpu, ca, w, h, (3,))
    want_a = tv(cpu, w, h)[0]
    render_view(cpu, cb, w, h, (3,))
    want_b = tv(cpu, w, h)[0]
    want_b_filtered = tv(cpu, w, h, FILTER)[0]
    cpu.render(w, h, 1, BOUNCES)
    want_dv = cpu.denoise_var(w, h, **dvp)
    want_b4 = tv(cpu, w, h)[0]

    def image(t):
        return t.cpu().numpy().view(np.uint8).reshape(h, w, 4)

    dev.set_scene(scene)
    dev.init_rand(w, h)
    dev.temporal_reset()
    raw, t_a, t_b, t_f, dv, t_4 = [torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(6)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `stream`)
    s = stream.cuda_stream
    # view A: render and call on the caller's stream, then view B's render (it resets frameSum, which
    # the call reads) right behind them
    dev.set_camera(ca)
    dev.render_device(dev.params(w, h, 3, BOUNCES), raw.data_ptr(), s)
    dev.temporal_var_device(t_a.data_ptr(), s)
    dev.set_camera(cb)
    dev.render_device(dev.params(w, h, 3, BOUNCES), raw.data_ptr(), s)
    # view B's call on the context's own stream (after the render on the caller's), the filtered call
    # on the caller's behind it, then directly behind: a render on the context's stream (it writes the
    # frameSum the call read), a variance-guided denoise of the longer frame on the caller's (it shares
    # the colour buffers with the levels) and a call on the context's stream behind that
    dev.temporal_var_device(t_b.data_ptr(), None)
    dev.temporal_var_device(t_f.data_ptr(), s, denoise_var=FILTER)
    dev.render_device(dev.params(w, h, 1, BOUNCES), raw.data_ptr(), None)
    dev.denoise_var_device(dv.data_ptr(), s, **dvp)
    dev.temporal_var_device(t_4.data_ptr(), None)
    stream.synchronize()
    dev.synchronize()
    assert np.array_equal(image(t_a), want_a)
    assert np.array_equal(image(t_b), want_b)
    assert np.array_equal(image(t_f), want_b_filtered)
    assert np.array_equal(image(dv), want_dv)
    assert np.array_equal(image(t_4), want_b4)
    assert not np.array_equal(image(t_b), image(t_f))
    assert dev.last_temporal_var_ms() > 0
    # the synchronous call in the same view: the same bits as the device variant
    assert np.array_equal(tv(dev, w, h)[0], want_b4)
