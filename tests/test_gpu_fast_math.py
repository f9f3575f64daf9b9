"""Per-site accuracy of the reference-fast precision mode (DESIGN.md section 8,
"What FAST replaces, per site"): every primitive of csrc/rt_path.h that the
mode changes, evaluated on the GPU by tools/fast_math_probe.hip and compared
in float64.

build/mathprobe is the header built as the exact units are (its device bits
must equal the bits of the header's own host pass, the CPU fallback's
arithmetic); build/mathprobe_fast is the header built as the reference-fast
units are.  Each (binary, function) pair runs once and is shared, read-only.

"ulp" below is the spacing of the correctly rounded float32 result, and an
error is |got - float64 reference| in that unit.  Any NaN equals any NaN
(IEEE 754 fixes neither sign nor payload of a generated NaN).
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.path.join(REPO, "build", "mathprobe")
FAST = os.path.join(REPO, "build", "mathprobe_fast")

SQRT, RCP, INV_LEN, DIV, DIV_SPEC, SINCOS, ATAN, TONE_MAP, RAW_SIN, RAW_COS = range(10)
ARITY = {SQRT: 1, RCP: 1, INV_LEN: 1, DIV: 2, DIV_SPEC: 1, SINCOS: 1, ATAN: 1, TONE_MAP: 4, RAW_SIN: 1, RAW_COS: 1}
OUTS = {SINCOS: 2}
NAMES = {SQRT: "rt_sqrt", RCP: "rt_rcp", INV_LEN: "rt_inv_len", DIV: "rt_div", DIV_SPEC: "rt_div_spec_chance",
         SINCOS: "rt_sincos", ATAN: "atan_nn", TONE_MAP: "tone_map", RAW_SIN: "v_sin_f32", RAW_COS: "v_cos_f32"}

STRIDE = 4099
INF_BITS = 0x7F800000
SIGN = 0x80000000
MIN_NORMAL = 0x00800000


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits_of(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def strided(lo_bits, hi_bits):
    """Every 4099th bit pattern of [lo_bits, hi_bits], both ends included."""
    b = np.arange(lo_bits, hi_bits + 1, STRIDE, dtype=np.int64)
    return np.unique(np.append(b, hi_bits)).astype(np.uint32)


def edge_bits():
    """The 64 patterns on either side of every class boundary of rt_sqrt.h and
    of the number format (0, the smallest normal, 2^+-60, 2^-96, 2^118, 2^126,
    FLT_MAX), in both signs; +-0, +-inf, NaNs; a block of denormals."""
    bounds = [0.0, np.ldexp(1.0, -126), np.ldexp(1.0, -60), np.ldexp(1.0, 60), np.ldexp(1.0, -96),
              np.ldexp(1.0, 118), np.ldexp(1.0, 126), float(np.finfo(np.float32).max)]
    out = []
    for v in bounds:
        b = int(bits_of(v))
        around = np.arange(b - 64, b + 65, dtype=np.int64)
        around = around[(around >= 0) & (around <= 0x7FFFFFFF)]  # below +0: the negative side is the sign copy
        out.append(around)
        out.append(around | SIGN)
    out.append(np.array([0, SIGN, INF_BITS, INF_BITS | SIGN, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF],
                        dtype=np.int64))
    den = np.unique(np.append(np.arange(1, MIN_NORMAL, 8191, dtype=np.int64), MIN_NORMAL - 1))
    out += [den, den | SIGN]
    return np.unique(np.concatenate(out)).astype(np.uint32)


def both_signs(b):
    return np.unique(np.concatenate([b, b | np.uint32(SIGN)]))


TWO_PI_BITS = int(bits_of(2 * np.pi))  # float32(2 pi) > 2 pi: the last pattern inside [0, 2 pi) is one below
LAST_BELOW_2PI = TWO_PI_BITS - 1
assert float(f32(LAST_BELOW_2PI)) < 2 * np.pi <= float(f32(TWO_PI_BITS))


def sincos_inputs():
    parts = [strided(0, LAST_BELOW_2PI)]
    for k in range(5):  # the 4,096 floats on either side of every multiple of pi / 2
        c = int(bits_of(k * np.pi / 2))
        a = np.arange(c - 4096, c + 4097, dtype=np.int64)
        parts.append(a[(a >= 0) & (a <= LAST_BELOW_2PI)].astype(np.uint32))
    parts.append(np.array([LAST_BELOW_2PI], dtype=np.uint32))
    return f32(np.unique(np.concatenate(parts)))


def div_inputs():
    """(x, y): strided finite patterns of both signs, y in a fixed shuffle; a
    mantissa sweep of [1, 2) / [1, 2); the edge patterns against each other
    and against ordinary values."""
    x = both_signs(strided(0, INF_BITS))
    y = np.random.default_rng(4099).permutation(both_signs(strided(1733, INF_BITS)))[:len(x)]
    x = x[:len(y)]
    mx = np.arange(0x3F800000, 0x40000000, 17, dtype=np.uint32)
    my = np.random.default_rng(17).permutation(np.arange(0x3F800000 + 5, 0x40000000, 17, dtype=np.uint32))[:len(mx)]
    e = edge_bits()
    ex, ey = np.meshgrid(e[::7], e[::5])
    ordinary = bits_of([1.0, -3.0, 0.1, 1e-4, 2e-30, 7e19])
    ox, oy = np.meshgrid(e, ordinary)
    xs = np.concatenate([x, mx, ex.ravel(), ox.ravel(), oy.ravel()])
    ys = np.concatenate([y, my[:len(mx)], ey.ravel(), oy.ravel(), ox.ravel()])
    return np.stack([f32(xs), f32(ys)], axis=1)


TONE_N = (1, 2, 3, 7, 8, 1000)


def tone_inputs():
    """frameSum = v * n, v log-spaced over [0, 1e4] (0 itself included), the
    three channels on different values; NaN, +-inf and negative sums mixed in."""
    v = np.concatenate([[0.0], np.logspace(-8, 4, 6000)]).astype(np.float32)
    rows = []
    for n in TONE_N:
        s = (v * np.float32(n)).astype(np.float32)
        t = np.stack([s, np.roll(s, 1777), s[::-1]], axis=1)
        rows.append(np.concatenate([t, f32(np.full((len(t), 1), n, dtype=np.uint32))], axis=1))
        odd = np.array([np.nan, np.inf, -np.inf, -1.0, -0.02, -0.0119, -1e-3, -1e-30, -7.5, 0.5], dtype=np.float32)
        a, b, c = np.meshgrid(odd, odd, odd, indexing="ij")
        o = np.stack([a.ravel() * np.float32(n), b.ravel(), c.ravel()], axis=1).astype(np.float32)
        rows.append(np.concatenate([o, f32(np.full((len(o), 1), n, dtype=np.uint32))], axis=1))
    return np.concatenate(rows).astype(np.float32)


def _inputs(fid):
    e = f32(edge_bits())
    if fid in (SQRT, INV_LEN):  # every non-negative float; negatives come with the edges
        return np.concatenate([f32(strided(0, INF_BITS)), e])
    if fid in (RCP, DIV_SPEC):
        return np.concatenate([f32(both_signs(strided(0, INF_BITS))), e])
    if fid == DIV:
        return div_inputs()
    if fid == SINCOS:
        return sincos_inputs()
    if fid == ATAN:
        return np.concatenate([f32(strided(0, int(bits_of(50.0)))), np.array([np.inf], dtype=np.float32)])
    if fid == TONE_MAP:
        return tone_inputs()
    return (np.arange(1 << 20, dtype=np.float64) / (1 << 20)).astype(np.float32)  # exact turns k / 2^20


_CACHE = {}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """probe(fid) -> (inputs, exact device words, exact host words or None,
    fast device words): one run of each binary per function, shared."""
    d = tmp_path_factory.mktemp("mathprobe")
    for exe in (EXACT, FAST):
        assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"

    def run(fid):
        if fid not in _CACHE:
            x = np.ascontiguousarray(_inputs(fid), dtype=np.float32)
            assert x.size % ARITY[fid] == 0
            inp = str(d / f"in{fid}.bin")
            x.tofile(inp)
            res = []
            for tag, exe, host in (("exact", EXACT, fid not in (RAW_SIN, RAW_COS)), ("fast", FAST, False)):
                out = str(d / f"{tag}{fid}.bin")
                cmd = [exe, str(fid), inp, out] + ([out + ".host"] if host else [])
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
                assert r.returncode == 0, (cmd, r.stdout, r.stderr)
                n = x.size // ARITY[fid]
                for p in [out] + ([out + ".host"] if host else []):
                    w = np.fromfile(p, dtype=np.uint32)
                    assert w.size == n * OUTS.get(fid, 1), (p, w.size, n)
                    w = w.reshape(n, OUTS.get(fid, 1)) if fid in OUTS else w
                    w.setflags(write=False)
                    res.append(w)
            x = x.reshape(-1, ARITY[fid]) if ARITY[fid] > 1 else x
            x.setflags(write=False)
            _CACHE[fid] = (x, res[0], res[1] if len(res) == 3 else None, res[-1])
        return _CACHE[fid]

    return run


def same_bits(a, b):
    """Word for word, a NaN equal to any NaN."""
    fa, fb = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


def ulp_err(got, want64):
    """|got - want64| in spacings of the correctly rounded float32 result."""
    with np.errstate(over="ignore", invalid="ignore"):
        cr = want64.astype(np.float32)
        sp = np.abs(np.spacing(cr)).astype(np.float64)
        return np.abs(got.astype(np.float64) - want64) / sp


def is_normal(x):
    a = np.abs(np.asarray(x, dtype=np.float64))
    return (a >= 2.0 ** -126) & (a <= float(np.finfo(np.float32).max))


def is_denormal32(x):
    b = bits_of(x) & np.uint32(0x7FFFFFFF)
    return (b > 0) & (b < MIN_NORMAL)


@pytest.mark.parametrize("fid", [SQRT, RCP, INV_LEN, DIV, DIV_SPEC, SINCOS, ATAN, TONE_MAP], ids=lambda f: NAMES[f])
def test_exact_device_equals_host_pass(probe, fid):
    """EXACT: the device pass of rt_path.h and its host pass (the CPU
    fallback's arithmetic) give the same bits for every input, edges
    included."""
    x, dev, host, _ = probe(fid)
    ok = same_bits(dev, host) if fid != TONE_MAP else dev == host
    bad = np.argwhere(~ok)[:8, 0]
    payload = int(((dev != host) & ok).sum())
    print(f"\nFASTMATH exact {NAMES[fid]}: {len(dev)} inputs, {int((~ok).sum())} mismatches, "
          f"{payload} NaNs of another payload")
    assert ok.all(), [(x[i].tolist(), dev[i].tolist(), host[i].tolist()) for i in bad]


def _want(fid, x64):
    with np.errstate(all="ignore"):
        if fid == SQRT:
            return np.sqrt(x64)
        if fid == RCP:
            return 1.0 / x64
        return 1.0 / np.sqrt(x64)


def _ieee_special(fid, x):
    """IEEE results at +-0, +-inf and negative arguments (NaN: NaN)."""
    z = np.float32(0.0)
    with np.errstate(all="ignore"):
        if fid == SQRT:
            return np.sqrt(x)
        if fid == RCP:
            return np.float32(1.0) / x
        r = np.float32(1.0) / np.sqrt(x)
        return np.where((x == z) & np.signbit(x), np.float32(-np.inf), r).astype(np.float32)  # rSqrt(-0) = -inf


def _classes(v):
    v = np.asarray(v, dtype=np.float32)
    names = ("nan", "inf", "zero", "denormal", "normal")
    masks = (np.isnan(v), np.isinf(v), v == 0, is_denormal32(v), is_normal(v))
    return {n: int(m.sum()) for n, m in zip(names, masks) if m.any()}


@pytest.mark.parametrize("fid", [SQRT, RCP, INV_LEN], ids=lambda f: NAMES[f])
def test_fast_sqrt_rcp_inv_len(probe, fid):
    """One v_sqrt_f32 / v_rcp_f32 / v_rsq_f32: within 1 ulp wherever input and
    result are normal (rt_sqrt.h's stated figure); IEEE at +-0, +-inf, NaN and
    negative arguments; a denormal input gives the result of the flushed input
    or a 1-ulp result, never NaN."""
    x, _, _, fast = probe(fid)
    got = fast.view(np.float32)
    x64 = x.astype(np.float64)
    want = _want(fid, x64)
    den = is_denormal32(x)
    neg_domain = (fid != RCP) & (x < 0)

    ordinary = is_normal(x64) & ~neg_domain & is_normal(want)
    err = ulp_err(got[ordinary], want[ordinary])
    print(f"\nFASTMATH fast {NAMES[fid]}: {int(ordinary.sum())} normal inputs, max error {err.max():.4f} ulp")
    assert int(ordinary.sum()) > 500000
    assert not np.isnan(got[ordinary]).any()
    assert err.max() <= 1.0, (x[ordinary][err.argmax()], got[ordinary][err.argmax()])

    special = ~den & ((x == 0) | np.isinf(x) | np.isnan(x) | (neg_domain & is_normal(x64)))
    ieee = _ieee_special(fid, x[special])
    assert special.sum() >= 8
    assert same_bits(bits_of(got[special]), bits_of(ieee)).all(), \
        list(zip(x[special].tolist(), got[special].tolist(), ieee.tolist()))[:16]

    # denormal inputs: what the instruction does with them is the hardware's choice of two
    xd, gd = x[den], got[den]
    flushed = _ieee_special(fid, np.copysign(np.float32(0.0), xd))
    is_flushed = same_bits(bits_of(gd), bits_of(flushed))
    with np.errstate(all="ignore"):
        wd = _want(fid, xd.astype(np.float64))
        cr = wd.astype(np.float32)
        close = np.where(np.isfinite(cr) & (cr != 0), ulp_err(gd, wd) <= 1.0, same_bits(bits_of(gd), bits_of(cr)))
    print(f"FASTMATH fast {NAMES[fid]}: {int(den.sum())} denormal inputs -> {_classes(gd)}; "
          f"{int(is_flushed.sum())} as the flushed input, {int((close & ~is_flushed).sum())} as a 1-ulp result")
    assert den.sum() > 100
    assert (is_flushed | close).all(), list(zip(xd[~(is_flushed | close)].tolist(), gd[~(is_flushed | close)].tolist()))[:8]
    positive = xd > 0 if fid != RCP else np.ones(len(xd), dtype=bool)  # (sqrt of a negative denormal may be NaN)
    assert not np.isnan(gd[positive]).any()


def test_fast_div(probe):
    """x * v_rcp_f32(y): within 2 ulp where x, y, 1 / y and x / y are normal
    (1 ulp of the reciprocal plus one rounding)."""
    xy, _, _, fast = probe(DIV)
    got = fast.view(np.float32)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        q = x / y
        ok = is_normal(x) & is_normal(y) & is_normal(1.0 / y) & is_normal(q)
    err = ulp_err(got[ok], q[ok])
    print(f"\nFASTMATH fast rt_div: {int(ok.sum())} all-normal pairs of {len(got)}, max error {err.max():.4f} ulp")
    assert int(ok.sum()) > 500000
    assert err.max() <= 2.0, (xy[ok][err.argmax()], got[ok][err.argmax()])


def test_fast_div_spec_chance_is_exact(probe):
    """A multiply by 2 is a division by 0.5: FAST bits equal EXACT bits."""
    x, exact, _, fast = probe(DIV_SPEC)
    ok = same_bits(exact, fast)
    assert ok.all(), list(zip(x[~ok].tolist(), exact[~ok].tolist(), fast[~ok].tolist()))[:8]
    finite = np.isfinite(x)
    assert np.array_equal(exact.view(np.float32)[finite], (x[finite] / np.float32(0.5)).astype(np.float32))


def _hardware_h(probe):
    """Maximum absolute error of v_sin_f32 / v_cos_f32 themselves, on exactly
    representable turns k / 2^20 against float64 sin / cos of 2 pi t."""
    t, dev, _, _ = probe(RAW_SIN)
    t2, dev2, _, _ = probe(RAW_COS)
    assert np.array_equal(t, t2) and len(t) == 1 << 20
    ang = 2.0 * np.pi * t.astype(np.float64)
    return (float(np.abs(dev.view(np.float32).astype(np.float64) - np.sin(ang)).max()),
            float(np.abs(dev2.view(np.float32).astype(np.float64) - np.cos(ang)).max()))


def test_fast_sincos(probe):
    """v_sin_f32 / v_cos_f32 of x * (1 / 2 pi) on [0, 2 pi): absolute error
    against float64 of at most H + 6.0e-7 + 6e-8.  6.0e-7 = 2 pi (2^-24 +
    2^-25): the rounding of the product angle * 1/(2 pi) to a turn below 1 and
    the rounded constant, through a slope of 2 pi per turn; 6e-8: one ulp of
    the result; H: the instruction's own maximum absolute error, measured in
    the same run from the raw builtins (hardware, not project code)."""
    h_sin, h_cos = _hardware_h(probe)
    x, _, _, fast = probe(SINCOS)
    assert (x >= 0).all() and (x.astype(np.float64) < 2 * np.pi).all() and len(x) > 250000
    got = fast.view(np.float32).astype(np.float64)
    e_sin = np.abs(got[:, 0] - np.sin(x.astype(np.float64)))
    e_cos = np.abs(got[:, 1] - np.cos(x.astype(np.float64)))
    print(f"\nFASTMATH hardware H: v_sin_f32 {h_sin:.4e}, v_cos_f32 {h_cos:.4e} (turns k / 2^20)")
    print(f"FASTMATH fast rt_sincos: {len(x)} angles, max |error| sin {e_sin.max():.4e} (at {x[e_sin.argmax()]!r}), "
          f"cos {e_cos.max():.4e} (at {x[e_cos.argmax()]!r})")
    assert e_sin.max() <= h_sin + 6.0e-7 + 6e-8
    assert e_cos.max() <= h_cos + 6.0e-7 + 6e-8


def test_fast_atan(probe):
    """atan_nn keeps its polynomial under FAST; its two divisions become
    x * rcp(y) and -rcp(x).  On [0, 50] and +inf: at most 4e-7 (the EXACT bar
    of test_numerics.py) + 1.8e-7 (3 * 2^-24: the 2-ulp quotient through a
    slope of at most 1); atan_nn(inf) within 1e-7 of pi / 2."""
    x, _, _, fast = probe(ATAN)
    got = fast.view(np.float32).astype(np.float64)
    assert np.isinf(x[-1]) and (x[:-1] >= 0).all() and (x[:-1] <= 50).all() and len(x) > 200000
    err = np.abs(got - np.arctan(x.astype(np.float64)))
    print(f"\nFASTMATH fast atan_nn: {len(x)} arguments, max |error| {err.max():.4e} (at {x[err.argmax()]!r})")
    assert err.max() <= 4e-7 + 1.8e-7
    assert abs(got[-1] - np.pi / 2) < 1e-7


def test_fast_tone_map(probe):
    """Every channel byte of FAST within 1 of EXACT's (a relative error of a
    few ulp crosses one rounding boundary and no more); NaN sums give 0 in
    both modes; alpha is 255."""
    x, exact, _, fast = probe(TONE_MAP)
    assert sorted(set(x[:, 3].view(np.uint32).tolist())) == sorted(TONE_N)
    ch = lambda w: np.stack([(w >> (8 * k)) & 0xFF for k in range(4)], axis=1).astype(np.int32)  # noqa: E731
    e, f = ch(exact), ch(fast)
    assert (e[:, 3] == 255).all() and (f[:, 3] == 255).all()
    nan = np.isnan(x[:, :3])
    print(f"\nFASTMATH tone_map: {int(nan.sum())} NaN sums -> bytes EXACT {np.unique(e[:, :3][nan]).tolist()}, "
          f"FAST {np.unique(f[:, :3][nan]).tolist()}")
    # a NaN sum stays NaN up to clamp(color, 1.0f) = fminf(NaN, 1) = 1 (Math.cuh:253-262, the reference's
    # own behaviour, which EXACT restates and the oracle shares): byte 255, the same in both modes.  The
    # NaN -> 0 of to_u8 is met by a negative tone-mapped value (sqrt of a negative), below.
    assert nan.any() and (e[:, :3][nan] == 255).all() and (f[:, :3][nan] == 255).all()
    # (the numerator 0.6 v (2.51 * 0.6 v + 0.03) is negative for v in (-0.01992, 0))
    v = x[:, :3].astype(np.float64) / x[:, 3:].view(np.uint32).astype(np.float64)
    neg = (v < 0) & (v > -0.019)
    assert neg.sum() > 100 and (e[:, :3][neg] == 0).all() and (f[:, :3][neg] == 0).all()
    d = np.abs(e[:, :3] - f[:, :3])
    print(f"\nFASTMATH fast tone_map: {len(x)} pixels, {int((d > 0).sum())} channel bytes differ from EXACT, "
          f"max {int(d.max())}")
    assert d.max() <= 1, x[np.argwhere(d > 1)[:8, 0]]
    assert {0, 255} <= set(np.unique(e[:, :3]).tolist()) and len(np.unique(e[:, :3])) > 128  # the whole byte range
