"""Adaptive sampling for a moving camera on the MI355X:
the selection kernels of csrc/rt_adaptive.hip over the pending planes and the
count-aware kernel of csrc/rt_temporal_var.hip against the CPU backend, bit for
bit (both run the arithmetic of csrc/rt_adaptive.h and csrc/rt_temporal_var.h).
Each test runs the same loop on a GPU and on a CPU context, both seeded by
init_rand: the renders are bit-identical (tests/test_gpu_parity.py), so the
selected sets, counts, frameSum, RNG state and every output must be too.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_temporal_case as AT
import assemble_case as A
from adaptive_temporal_case import tv, tvc
from bwrt import Renderer, abi, scenes
from test_temporal import BOUNCES, MOVES, SECOND

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
    if bwrt_lib.rt_device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on an MI355X")
    r = Renderer(0, lib=bwrt_lib)
    yield r
    r.close()


def same(a, b):
    """Equal values, NaN equal to NaN (the 1x1 frame's camera ray is NaN, of either sign)."""
    return A.same_values(a, b)


def walk(r, scene, w, h, moves, rounds=2, dv_last=FILTER, k0=AT.K0, **params):
    """The loop over the views of `moves` on a freshly seeded context: per view
    the pending results and, per round, the selected set, the counts, the
    frameSum and RNG state and the counted call's results; then the counted call
    with levels in the last view."""
    r.set_scene(scene)
    r.set_moments(True)
    r.set_adaptive_filters(True)
    r.init_rand(w, h)
    r.temporal_reset()
    out = []
    for cam in AT.path(scene, moves):
        out.append(AT.begin_view(r, cam, w, h, k0))
        for _ in range(rounds):
            img, col, st, took = AT.adaptive_round(r, w, h, **params)
            s = AT.frame_state(r, w, h)
            out.append((img, col, st["selected"], st["frames_total"], took, s["n"], s["j"], s["rng"], s["accum"]))
            out.append(tvc(r, w, h))
    if dv_last is not None:
        out.append(tvc(r, w, h, dv_last))
    r.set_moments(False)
    r.set_adaptive_filters(False)
    return out


def forced(w, h):
    """The tiny frames take the largest window (it is clipped at every border)
    and a first round forced by min_frames: the second round's taps then have
    degrees of freedom, and its window decides."""
    return dict(radius=4, min_frames=AT.K0 + 1) if w * h < 100 else dict(radius=2)


SHAPES = [
    ("07", 67, 45, [MOVES["yaw"], SECOND]), ("07", 67, 45, [MOVES["sideways"], SECOND]),
    ("07", 67, 45, [MOVES["dolly"], SECOND]), ("07", 67, 45, CHAIN),
    ("07", 333, 187, [MOVES["yaw"], SECOND]),  # a partial mask word in every row, partial 32 x 8 groups
    ("07", 5, 3, [MOVES["yaw"], SECOND]), ("07", 1, 1, [MOVES["yaw"]]),  # windows larger than the frame
    ("stress", 96, 54, [MOVES["dolly"], SECOND]),  # the BVH scene: its list kernel and guides
]


@pytest.mark.parametrize("name,w,h,moves", SHAPES,
                         ids=["yaw", "sideways", "dolly", "chained", "333x187", "5x3", "1x1", "stress"])
def test_equals_cpu(dev, cpu, name, w, h, moves):
    scene = scenes.SCENES[name]()
    g = walk(dev, scene, w, h, moves, **forced(w, h))
    c = walk(cpu, scene, w, h, moves, **forced(w, h))
    assert len(g) == len(c) == 5 * (len(moves) + 1) + 1
    for i, (x, y) in enumerate(zip(g, c)):
        assert same(x, y), i
    assert dev.last_temporal_var_ms() > 0
    if w >= 64:  # the sequence did what it is for
        took, n, j = c[-3][4], c[-3][5], c[-3][6]
        assert 0 < took.sum() and len(np.unique(n)) > 1
        if name == "07":  # (it has sky: pixels that no round selects)
            assert took.sum() < w * h and len(np.unique(n)) == 3 and (j == 1).any() and (j == 3).any()
        dof = c[-2][3][..., 1]
        assert dof.max() > 2 * len(moves)
        assert not same(c[-1][1], c[-2][1]) and same(c[-1][2], c[-2][2])  # the levels ran; the history is unfiltered


@pytest.mark.parametrize("variant", ["direct", "tiled", None])
def test_levels_equal_cpu(monkeypatch, bwrt_lib, cpu, variant):
    """Levels 0..6 behind the counted call, with a forced level variant and with the policy."""
    if variant:
        monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)  # read at rt_create (BWRT_TUNING=1)
    w, h = 67, 45
    scene = scenes.scene_07()
    res = []
    with Renderer(0, lib=bwrt_lib) as r:
        for x in (r, cpu):
            walk(x, scene, w, h, [MOVES["yaw"], SECOND], rounds=1, dv_last=None)
            x.set_adaptive_filters(True)  # (the frame is still the non-uniform one)
            res.append([tvc(x, w, h, dict(FILTER, iterations=it)) for it in range(7)])
            x.set_adaptive_filters(False)
    for it, (g, c) in enumerate(zip(*res)):
        assert same(g, c), it
    assert not same(res[1][6][1], res[1][5][1])


@pytest.mark.parametrize("which,kernel", [("simple", "rt_render_kernel<256,list>"),
                                          ("queued", "rt_render_list_kernel<256>")])
def test_both_list_kernels(monkeypatch, bwrt_lib, cpu, which, kernel):
    monkeypatch.setenv("BWRT_ADAPTIVE_KERNEL", which)
    w, h = 67, 45
    scene = scenes.scene_07()
    with Renderer(0, lib=bwrt_lib) as r:
        g = walk(r, scene, w, h, [MOVES["sideways"]], dv_last=None)
        assert r.last_kernel_name() == kernel
    c = walk(cpu, scene, w, h, [MOVES["sideways"]], dv_last=None)
    assert same(g, c)


def test_special_values_equal_cpu(dev, cpu):
    """The infinite-emittance light: non-finite colours and, after a second
    batch, NaN moments in the pending planes and the frame."""
    w, h = 67, 45
    scene = scenes.scene_07()
    scene.spheres[2].mat.emittance = float("inf")
    g = walk(dev, scene, w, h, [MOVES["yaw"]], k0=4)
    c = walk(cpu, scene, w, h, [MOVES["yaw"]], k0=4)
    assert same(g, c)
    col, mom = c[-2][1], c[-2][3]
    bad = ~np.isfinite(col).all(-1)
    assert 0.01 < bad.mean() < 0.95 and np.isnan(mom[..., 0][bad]).any() and np.isfinite(col[~bad]).all()


def test_repeated_sequences_are_identical(dev):
    scene = scenes.scene_07()
    first = walk(dev, scene, 333, 187, [MOVES["yaw"]])
    for _ in range(4):
        assert A.same(walk(dev, scene, 333, 187, [MOVES["yaw"]]), first)


def test_device_entry_points_and_stream_ordering(dev, cpu):
    import torch
    scene = scenes.scene_07()
    w, h = 160, 90
    cams = AT.path(scene, [MOVES["yaw"]])
    # the CPU context computes what every device buffer must hold
    cpu.set_scene(scene)
    cpu.set_moments(True)
    cpu.set_adaptive_filters(True)
    cpu.init_rand(w, h)
    cpu.temporal_reset()
    want = []
    for cam in cams:
        want.append(AT.begin_view(cpu, cam, w, h)[0])
        want.append(AT.adaptive_round(cpu, w, h)[0])
        want.append(tvc(cpu, w, h)[0])
        want.append(AT.adaptive_round(cpu, w, h)[0])
        want.append(tvc(cpu, w, h, FILTER)[0])
    want_state = AT.frame_state(cpu, w, h)
    cpu.set_moments(False)
    cpu.set_adaptive_filters(False)

    def image(t):
        return t.cpu().numpy().view(np.uint8).reshape(h, w, 4)

    dev.set_scene(scene)
    dev.set_moments(True)
    dev.set_adaptive_filters(True)
    dev.init_rand(w, h)
    dev.temporal_reset()
    bufs = [torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(len(want) + 1)]
    raw, outs = bufs[0], bufs[1:]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `stream`)
    s = stream.cuda_stream
    # view A on the caller's stream, view B alternating between the context's stream and the caller's:
    # render, rt_temporal_var_device, adaptive, counted, adaptive, counted, back to back, no host synchronisation
    for v, cam in enumerate(cams):
        o = outs[5 * v:5 * v + 5]
        alt = (lambda i: s) if v == 0 else (lambda i: None if i % 2 else s)
        dev.set_camera(cam)
        dev.render_device(dev.params(w, h, AT.K0, BOUNCES), raw.data_ptr(), alt(0))
        dev.temporal_var_device(o[0].data_ptr(), alt(1))
        dev.render_adaptive_reprojected_device(o[1].data_ptr(), alt(2), BOUNCES, samples=AT.K, **AT.BASE)
        dev.temporal_var_counted_device(o[2].data_ptr(), alt(3))
        dev.render_adaptive_reprojected_device(o[3].data_ptr(), alt(4), BOUNCES, samples=AT.K, **AT.BASE)
        dev.temporal_var_counted_device(o[4].data_ptr(), alt(5), denoise_var=FILTER)
    stream.synchronize()
    dev.synchronize()
    for i, (t, wnt) in enumerate(zip(outs, want)):
        assert np.array_equal(image(t), wnt), i
    assert same(AT.frame_state(dev, w, h), want_state)
    assert len(np.unique(want_state["n"])) == 3
    # the synchronous call in the same view: the same bits as the device variant
    assert np.array_equal(tvc(dev, w, h, FILTER)[0], want[-1])
    dev.set_moments(False)
    dev.set_adaptive_filters(False)


def test_error_contract(bwrt_lib):
    lib = bwrt_lib
    inv, uns = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED
    scene = scenes.scene_07()
    w, h = 33, 17
    cam = AT.path(scene, [])[0]
    with Renderer(0, lib=lib) as r:
        d = r.adaptive_reprojected_params(samples=1)
        t = lib.rt_temporal_params_default()
        call = lambda: lib.rt_render_adaptive_reprojected(r.ctx, C.byref(d), BOUNCES, None, None, None)  # noqa: E731
        dcall = lambda p=None: lib.rt_render_adaptive_reprojected_device(r.ctx, C.byref(d), BOUNCES, p, None)  # noqa: E731
        assert call() == abi.RT_ERR_NO_SCENE
        r.set_scene(scene)
        r.set_moments(True)
        r.set_camera(cam)
        r.render(w, h, 2, BOUNCES)
        assert call() == inv and dcall() == inv and b"no pending" in lib.rt_last_error(r.ctx)
        r.temporal(w, h)
        assert call() == inv and b"no moments" in lib.rt_last_error(r.ctx)
        r.temporal_var(w, h)
        assert dcall(C.c_void_p(2)) == inv and b"aligned" in lib.rt_last_error(r.ctx)
        r.set_precision("fast")
        assert call() == uns and dcall() == uns and b"REFERENCE_FAST" in lib.rt_last_error(r.ctx)
        r.set_precision("exact")
        assert (r.counts(h, w)[0] == 2).all() and (r.counts(h, w)[1] == 1).all()  # every refusal touched nothing
        assert dcall() == abi.RT_OK
        r.synchronize()
        assert set(np.unique(r.counts(h, w)[0])) == {2, 3}
        assert lib.rt_temporal_var_counted_device(r.ctx, C.byref(t), None, None, None) == uns  # the switch is off
        assert b"non-uniform" in lib.rt_last_error(r.ctx)
        assert lib.rt_temporal_var_device(r.ctx, C.byref(t), None, None, None) == uns
        r.set_adaptive_filters(True)
        assert lib.rt_temporal_var_device(r.ctx, C.byref(t), None, None, None) == uns
        assert lib.rt_temporal_var_counted_device(r.ctx, C.byref(t), None, C.c_void_p(2), None) == inv
        assert lib.rt_temporal_var_counted_device(r.ctx, C.byref(t), None, None, None) == abi.RT_OK
        r.synchronize()
        r.render(w, h, 2, BOUNCES, first_frame=1, row_offset=1, row_stride=2)
        assert call() == uns and b"row shard" in lib.rt_last_error(r.ctx)
