"""Next-event estimation against a float64 reference, sample by sample — CPU only.

(a) tests/nee_ref.py, written from the specification comments of
    csrc/rt_light.h and csrc/rt_layout.h, against closed forms: no product code.
(b) the scene compiler's light table (records and polygon sampling blocks,
    through the --lights dump of tests/test_scene_compile.py's program) against
    nee_ref.light_table.
(c) the host pass of tools/nee_probe.hip (build/neeprobe_cpu --host: the
    functions of csrc/rt_light.h with the CPU twin's flags) against the
    reference on random cases and on edge families, under tolerances derived
    in DESIGN.md section 26 (tests/nee_cases.py states the conditions).
tests/test_gpu_nee_probe.py holds the device pass to the same conditions.
"""
import os

import numpy as np
import pytest

import nee_cases as K
import nee_ref as R

PROBE_CPU = os.path.join(K.BUILD, "neeprobe_cpu")


# ---- (a) the reference against closed forms ------------------------------------------------

G = 512


def _grid(g):
    u = (np.arange(g) + 0.5) / g
    return np.stack(np.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2)  # stratified (u1, u2), cell midpoints


def _grid_mean_k(t, shapes, P, n, kind=1, g=G):
    grid = _grid(g)
    m = len(grid)
    u = np.concatenate([np.full((m, 1), 0.5), grid], 1)
    r = R.nee_sample(t, R.UNIFORM, shapes, u, np.tile(P, (m, 1)), np.tile(n, (m, 1)), np.full(m, 99), np.full(m, kind))
    return r["k"].mean(), r


@pytest.mark.parametrize("s2", [0.25, 1e-2, 1e-4])
def test_sphere_cone_mean_is_the_irradiance_integral(s2):
    """One light at distance 1, its centre at polar angle theta_c from the unit
    normal, the cone above the horizon: E[k] = s2 cos(theta_c) / 2.
    Discretisation: cs = ct cos(theta_c) + st sin(theta_c) cos(phi - phi0); the
    mean of the cosine over G equally spaced phi vanishes identically and ct is
    linear in u1, which the midpoint rule integrates exactly, so what is left
    is float64 rounding, G^2 * 2^-53 < 1e-10 relative — and the float the
    product calls pi (rt_layout.h RT_PI), whose phi = 2 RT_PI u2 overshoots the
    period by delta = 2 RT_PI - 2 pi: the grid mean of the cosine is then at
    most delta / 2 pi, on an amplitude of at most sin(theta_max) sin(theta_c)."""
    delta = abs(R.TWO_PI - 2 * np.pi)
    theta_max = np.arcsin(np.sqrt(s2))
    for frac in (0.0, 0.3, 0.7, 0.98):
        theta_c = frac * (np.pi / 2 - theta_max)
        c = R.f32([np.sin(theta_c) * 0.6, np.sin(theta_c) * 0.8, np.cos(theta_c)]).astype(np.float64)
        t = R.make_table([c], [float(np.float32(s2))], [[1, 1, 1]], [0], np.zeros((0, 20)), 1, 1)
        d2 = (c * c).sum()
        want = R.sphere_mean_k(t["r2"][0] / d2, c[2] / np.sqrt(d2))
        got, r = _grid_mean_k(t, R.SPHERES, [0.0, 0.0, 0.0], [0.0, 0.0, 1.0])
        assert r["trace"].all()
        omega = 1.0 - np.sqrt(1.0 - t["r2"][0] / d2)
        bound = 1e-10 * want + omega * np.sqrt(s2) * np.sin(theta_c) * delta / (2 * np.pi) * 1.01
        assert abs(got - want) <= bound, (s2, frac, got, want, bound)
        assert bound < 1e-7 * want


POLYGONS = {
    "right triangle": [(0, 0, 0), (1, 0, 0), (0, 0, 1)],
    "unit square": [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)],
    "1:3 quad": [(0, 0, 0), (1, 0, 0), (1, 0, 1), (-2, 0, 1)],
}


def _polygon_table(verts):
    import types
    v = [types.SimpleNamespace(x=p[0], y=p[1], z=p[2]) for p in verts]
    mat = types.SimpleNamespace(emittance=1.0, albedo=types.SimpleNamespace(x=1.0, y=1.0, z=1.0))
    rec = R._polygon(v, mat, 5)
    return R.make_table([rec["centre"]], [rec["r2"]], [rec["emitted"]], [5], [rec["block"]], 0, 1), rec


@pytest.mark.parametrize("name", list(POLYGONS))
@pytest.mark.parametrize("view", ["above", "oblique", "inside"])
def test_polygon_mean_is_lamberts_edge_sum(name, view):
    """One polygon light (its normal along -y, seen from below) over a point
    whose unit normal is +y: E[k] = I / (2 pi), Lambert's edge sum over the
    sampled shape.  `inside`: the point lies inside the bounding sphere.
    Discretisation, from two grid sizes.  The map (u1', u2) -> Q preserves
    area, a grid cell is a piece of the half of equal area with its sample
    inside, the integrand is smooth on the polygon (P is off its plane), and a
    half boundary (u1 = 1/2 or 1/4) is a cell boundary of both grids: the grid
    mean converges to the integral with an error e(h) = C h^p (1 + o(1)), of
    order p >= 1 at the least (p = 2 where the midpoint rule is undisturbed,
    3/2 from the square root at u1' -> 0).  Then e(h) - e(h/2) =
    e(h/2) (2^p - 1) >= e(h/2): the mean at 512 x 512 is no farther from the
    integral than it is from the mean at 256 x 256.  That distance is demanded
    as the bound — and is itself below 1e-4 of the value in all nine cases, so
    a wrong half area, a swapped half or a wrong constant fails in every view."""
    verts = np.array(POLYGONS[name], np.float64)
    t, rec = _polygon_table(POLYGONS[name])
    centre, rad = rec["centre"], np.sqrt(rec["r2"])
    P = {"above": centre + [0.0, -4.0, 0.0], "oblique": centre + [3.0, -2.0, 1.0], "inside": centre + [0.1, -0.3 * rad, 0.05]}[view]
    P = R.f32(P).astype(np.float64)
    n = np.array([0.0, 1.0, 0.0])
    got, r = _grid_mean_k(t, R.ALL, P, n)
    coarse, _ = _grid_mean_k(t, R.ALL, P, n, g=G // 2)
    assert r["trace"].all()
    want = R.polygon_mean_k(verts, P, n)
    bound = abs(got - coarse)
    print(f"{name} {view}: mean k {got:.9g}, closed form {want:.9g}, |diff| {abs(got - want):.3g} <= bound {bound:.3g} "
          f"({bound / want:.2g} of the value)")
    assert abs(got - want) <= bound, (got, want, bound)
    assert bound < 1e-4 * want


@pytest.mark.parametrize("nn", [0.64, 2.0, 4.0])
def test_stretched_weight_against_the_flip_of_random_direction(nn):
    """Kind 2: the default estimator's diffuse bounce on a normal of length^2 nn,
    simulated in float64 — a uniform direction r (ball point, normalised), the
    lower half flipped by r - 2 (r.n) n, weighted by (s.n) — against
    (cs / 2) [1 + 1 / (g q^2)]: E[(s.n) 1{un in bin}] = int_bin wc d(un), per bin
    of the unit direction's normal component, within 5 standard errors."""
    rng = np.random.default_rng(K.SEED)
    m = 1 << 22
    r = rng.normal(size=(m, 3))
    r /= np.sqrt((r * r).sum(1))[:, None]
    n = np.array([0.0, 0.0, np.sqrt(nn)])
    rn = r @ n
    s = np.where((rn < 0)[:, None], r - 2.0 * rn[:, None] * n, r)
    weight = s @ n
    un = s[:, 2] / np.sqrt((s * s).sum(1))
    assert (un >= 0).all()
    edges = np.linspace(0.0, 1.0, 9)
    x = (np.arange(1 << 16) + 0.5) / (1 << 16)
    for lo, hi in zip(edges[:-1], edges[1:]):
        f = weight * ((un >= lo) & (un < hi))
        sim, se = f.mean(), f.std() / np.sqrt(m)
        xs = lo + (hi - lo) * x
        want = R.stretched_cos(xs * np.sqrt(nn), nn).mean() * (hi - lo)
        assert abs(sim - want) <= 5 * se, (nn, lo, hi, sim, want, se)


@pytest.mark.parametrize("n_lights", [1, 2, 3, 8, 41])
def test_weighted_pick_probabilities(n_lights):
    """2^12 random points and normals over a table of n lights, all on
    nee_sample's own answers: light j is picked at both ends of the u-interval
    [run_{j-1}, run_j) / W, whose width is p_j, and where it gives a sample the
    factor in its k (against the uniform pick's k of the same light and
    direction, which carries n_lights) is 1 / p_j — so every term of
    sum_j p_j (W / w_j) [w_j > 0] is 1 and the sum the number of positive lights.
    And every light that gives a sample with k > 0 under the uniform pick has
    w_j > 0 (cb bounds the cone's cosines): over a grid of (u1, u2) that holds
    the cone's rim, u1 = 1 - 2^-24 and u1 = 1, at eight azimuths."""
    words = R.table_words(K._grid(n_lights))
    t, _ = R.table_from_words(words)
    rng = np.random.default_rng([K.SEED, n_lights])
    m = 1 << 12
    P = rng.uniform([-8, 0, -8], [6, 6, 0], (m, 3))
    n = K._unit(rng, m)
    prim = np.full(m, 1 << 20)
    one = np.ones(m, int)
    w = np.stack([R.pick_weight(t, j, P, n, 1.0, prim, False)[0] for j in range(n_lights)], 1)
    W = w.sum(1)
    run = np.cumsum(w, 1)
    pos = w > 0
    cfg, j = np.nonzero(pos)
    lo = (run - w)[cfg, j] / W[cfg]
    hi = run[cfg, j] / W[cfg]
    half = np.full(len(cfg), 0.5)
    for uu in (lo + (hi - lo) * 1e-6, hi - (hi - lo) * 1e-6):
        r = R.nee_sample(t, R.WEIGHTED, R.SPHERES, np.stack([uu, half, half], 1), P[cfg], n[cfg], prim[cfg], one[cfg])
        assert (r["j"] == j).all()
    rw = R.nee_sample(t, R.WEIGHTED, R.SPHERES, np.stack([(lo + hi) / 2, half, half], 1), P[cfg], n[cfg], prim[cfg], one[cfg])
    ru = R.nee_sample(t, R.UNIFORM, R.SPHERES, np.stack([(j + 0.5) / n_lights, half, half], 1), P[cfg], n[cfg], prim[cfg], one[cfg])
    assert (rw["j"] == j).all() and (ru["j"] == j).all() and (rw["trace"] == ru["trace"]).all() and ru["trace"].any()
    lit = ru["trace"]
    term = (hi - lo)[lit] * (n_lights * rw["k"][lit] / ru["k"][lit])
    assert np.allclose(term, 1.0, rtol=1e-9, atol=0), np.abs(term - 1).max()
    # a light that can contribute has a positive weight
    for jj in range(n_lights):
        lit = np.zeros(m, bool)
        for u1 in (0.125, 0.5, 0.875, 1.0 - 2.0 ** -24, 1.0):
            for u2 in (np.arange(8) + 0.5) / 8:
                u = np.tile([(jj + 0.5) / n_lights, u1, u2], (m, 1))
                r = R.nee_sample(t, R.UNIFORM, R.SPHERES, u, P, n, prim, one)
                assert (r["j"] == jj).all()
                lit |= r["k"] > 0
        assert lit.any() and (w[lit, jj] > 0).all()


# ---- (b) the light table -------------------------------------------------------------------

@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    t = K.dump_tables(tmp_path_factory.mktemp("nee_tables"))
    t.update(K.crafted_tables())
    for v in t.values():
        v.setflags(write=False)
    return t


def _ulps(a, b):
    a, b = R.f32(a), R.f32(b)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", list(K.scene_tables()))
def test_light_table_matches_the_reference(tables, name):
    got, _ = R.table_from_words(tables[name])
    scene = K.scene_tables()[name]()
    want = R.light_table(scene)
    if name == "exclusions":
        import test_light_shapes as S
        assert [int(p) for p in want["prim"]] == S.exclusion_scene()[1]
    assert got["n_sph"] == want["n_sph"] == scene.counts[0]
    assert got["n_sphere_lights"] == want["n_sphere_lights"]
    assert np.array_equal(got["prim"], want["prim"]) and (np.diff(got["prim"]) > 0).all()
    assert np.array_equal(got["emitted"], want["emitted"])
    nsl = got["n_sphere_lights"]
    assert np.array_equal(got["centre"][:nsl], want["centre"][:nsl]) and np.array_equal(got["r2"][:nsl], want["r2"][:nsl])
    gb, wb = got["blocks"], want["blocks"]
    assert gb.shape == wb.shape and len(gb) == len(got["prim"]) - nsl
    exact = [0, 1, 2, 4, 5, 6, 8, 9, 10, 15, 16, 17, 18, 19]  # v0, v1, v2, the zero words, n
    assert np.array_equal(gb[:, exact], wb[:, exact])
    for col in (3, 7, 11, 12, 13, 14):  # A0, A1, |n|, v3'
        assert (_ulps(gb[:, col], wb[:, col]) <= 1).all(), (col, gb[:, col], wb[:, col])
    assert (_ulps(got["centre"][nsl:], want["centre"][nsl:]) <= 1).all()
    # the bounding sphere, around the record's own centre: contains every original and projected vertex, tightly
    quads = {int(p): scene.quads[int(p) - sum(scene.counts[:3])].vertices[3] for p in got["prim"][nsl:]
             if int(p) >= sum(scene.counts[:3])}
    for i in range(len(gb)):
        pts = [wb[i, 0:3], wb[i, 4:7], wb[i, 8:11], wb[i, 12:15]]
        pid = int(got["prim"][nsl + i])
        if pid in quads:
            pts.append(R._v(quads[pid]).astype(np.float64))
        far = max(((p - got["centre"][nsl + i]) ** 2).sum() for p in pts)
        assert far <= got["r2"][nsl + i] <= far * (1 + 2.0 ** -19), (i, far, got["r2"][nsl + i])
    # what the cases below rely on
    if name == "quad_1_3":
        assert np.allclose(gb[0, [3, 7]], [0.5, 1.5])
    if name == "lifted_quad":
        assert abs(gb[0, 13] - 4.0) < 1e-6 and gb[0, 13] != 4.4
    if name in ("box", "box_front"):  # the top quad of the box is 20 x 1, its front 20 x 10
        assert gb[0, 11] == (20.0 if name == "box" else 200.0)


# ---- (c) the host pass against the reference ------------------------------------------------

_RUNS = {}


@pytest.fixture(scope="module")
def host(tables, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("nee_host")

    def run(table, fid):
        if (table, fid) not in _RUNS:
            words, cases, random = K.run_inputs(tables, table, fid)
            r, _, out = K.run_probe([PROBE_CPU, "--host"], fid, words, cases, tmp)
            assert r.returncode == 0, (r.args, r.stdout, r.stderr)
            for a in (cases, out):
                a.setflags(write=False)
            _RUNS[table, fid] = (words, cases, random, out)
        return _RUNS[table, fid]
    return run


def test_crafted_states_hit_their_draws():
    st = K.crafted_states(4, np.random.default_rng(1))
    u, words, _ = R.draws(st)
    i = 0
    for draw in range(3):
        for name, target in K.CRAFT_WORDS.items():
            assert (words[i:i + 4, draw] == target).all()
            want = {"zero": 0.0, "one": 1.0, "one_max": 1.0, "below_one": 1.0 - 2.0 ** -24}[name]
            assert (u[i:i + 4, draw] == want).all()
            i += 4


@pytest.mark.parametrize("table,fid", K.SAMPLE_RUNS, ids=[f"{t}-{f}" for t, f in K.SAMPLE_RUNS])
def test_host_pass_sample(tables, host, table, fid):
    # the reference first: the random part of the set is decided to 99 % on its margins alone
    words, cases, random, out = host(table, fid)
    ref = K.sample_reference(words, fid, cases)
    und = K.check_undecided_share(ref, random)
    if table == "underflow":
        assert not ref["picked"][random].any()
    if table == "zero_first":
        assert (ref["j"][ref["picked"]] == 2).all() and ref["picked"].any()
    if table == "twins":  # the exact tie at u == 1/2 is decided, and for the second light
        assert (ref["margin"][-256:] > R.DECIDED).all() and (ref["j"][-256:] == 1).all() and ref["trace"][-256:].any()
    if table == "origin_quad":
        assert (~ref["trace"][-128:] & (ref["margin"][-128:] > R.DECIDED)).all()  # k overflows: no sample
    if table == "exact_r2":
        tail = slice(-512, -256)  # P = (2, 0, 0): d2 == 4 exactly, only the light with r2 below 4 is reachable
        assert (ref["margin"][tail] > R.DECIDED).all() and (ref["trace"][tail] == (ref["j"][tail] == 0)).all()
    dec, lit = K.check_sample(ref, cases, out)
    line = f"{table}/{fid}: undecided {und[0]} random + {und[1]} edge of {len(cases)}; decided {dec}, traced and checked {lit}, {und[2]} ill-conditioned"
    print(line)
    assert lit > 1000 or table in ("underflow", "origin_quad")


@pytest.mark.parametrize("table,fid", K.OTHER_RUNS, ids=[f"{t}-{f}" for t, f in K.OTHER_RUNS])
def test_host_pass_weights_suppression_fold(tables, host, table, fid):
    words, cases, random, out = host(table, fid)
    print(K.check_run({table: tables[table]}, table, fid, cases, random, out))


@pytest.mark.parametrize("decade", range(len(K.DECADES)))
def test_direction_stays_on_the_light(tables, host, decade):
    """Per decade of s2 (one sphere light seen from 8 to 12 away, 2^16 cases):
    the share of traced samples whose float wi misses the sphere in float64
    geometry is at most twice the share that the reference's own direction,
    rounded once to float, misses, plus 2 cases per 2^16.  Measured, of about
    52700 traced random cases each (before: the cone's sine from 1 - ct * ct, all
    samples at the centre from 1e-8 down; now: from t (2 - t); ref: the rounded
    reference):
      s2 <=   0.9  0.1  1e-2  1e-3  1e-4  1e-5  1e-6  1e-7  1e-8  1e-9
      before    0    0     0     2     7   122  1386  6529     0     0
      now       0    0     0     0     0     1     0     2     5    23
      ref       0    0     0     0     0     0     0     1     2    16"""
    words, cases, random, out = host(f"decade{decade}", 0)
    ref = K.sample_reference(words, 0, cases)
    (n, got, ideal), = K.miss_shares(ref, cases, random, out)
    line = f"s2 <= {K.DECADES[decade]:g}: {n} traced, wi misses {got} ({got / n:.4%}), the rounded reference {ideal} ({ideal / n:.4%})"
    print(line)
    assert n > 20000
    assert got <= 2 * ideal + 2.0 * n / 65536, line
