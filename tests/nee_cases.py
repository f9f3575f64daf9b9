"""Tables, case sets and the reference conditions shared by
tests/test_nee_reference.py (host pass of tools/nee_probe.hip, CPU) and
tests/test_gpu_nee_probe.py (device pass): everything is generated from fixed
numpy seeds, and every condition is stated against tests/nee_ref.py alone."""
import os
import subprocess

import numpy as np

import nee_ref as R
from bwrt import scenefile, scenes
from bwrt.abi import Sphere
from bwrt.scenes import material, vec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "build")
SEED = 20261021
N = 1 << 16


# ---- scenes and tables -------------------------------------------------------------------

def quad_1_3():
    """A convex quad (unit normal) whose halves (v0, v1, v2) and (v0, v2, v3) have areas 0.5 and 1.5"""
    import test_light_shapes as S
    q = S.quad([(0, 4, -5), (1, 4, -5), (1, 4, -4), (-2, 4, -4)], S.PANEL)
    return S.with_polygons(S.dark_07(), quads=[q], name="quad_1_3")


def lifted_quad():
    """A unit quad whose fourth vertex is lifted 0.4 off the plane of the first three"""
    import test_light_shapes as S
    q = S.quad([(0, 4, -5), (1, 4, -5), (1, 4, -4), (0, 4.4, -4)], S.PANEL)
    return S.with_polygons(S.dark_07(), quads=[q], name="lifted_quad")


def far_triangle():
    """A triangle at coordinates near 1e4"""
    import test_light_shapes as S
    t = S.tri([(10000, 4, -5), (10001, 4, -5), (10000, 4, -4)], S.PANEL)
    return S.with_polygons(S.dark_07(), triangles=[t], name="far_triangle")


def box_front():
    """04_box with its front mirror quad emissive: a light whose normal has length 200"""
    s = scenes.scene_04_box()
    s.quads[0].mat.emittance = 0.5
    return s


def small_light_scene(below=0):
    """A floor under one sphere light that subtends s2 = r^2 / d^2 of about 1e-4
    from the lit points below it (radius 0.05, 5 above the floor); below: that
    many small dark spheres under the floor, which make the scene a BVH one."""
    sph = [Sphere(vec(0, 5, -4), 0.05, material((1, 0.9, 0.8), 4000))]
    for i in range(below):
        sph.append(Sphere(vec(-4 + (i % 8), -1.0 - 0.5 * (i // 8), -8 + 0.7 * (i % 5)), 0.1, material((0.5, 0.5, 0.5))))
    return scenes.Scene(scenes.camera_07(), sph, [scenes._floor()], [], [], name=f"small_light{below}")


def scene_tables():
    """name -> scene factory of every compiled table; the exclusion scene carries its admitted ids"""
    import test_light_picking as K
    import test_light_shapes as S
    return {
        "07": scenes.scene_07, "eight_lights": K.eight_lights, "quad_panel": S.quad_panel, "triangle_panel": S.triangle_panel,
        "mixed": S.mixed, "box": S.box_with_emissive_quad, "box_front": box_front, "stress_tri": S.stress_with_emissive_triangles,
        "quad_1_3": quad_1_3, "lifted_quad": lifted_quad, "far_triangle": far_triangle,
        "exclusions": lambda: S.exclusion_scene()[0],
    }


# where the random points of a table lie when not around its lights
BOXES = {"far_triangle": ((-10.0, 0.0, -10.0), (10.0, 6.0, 0.0)), "underflow": ((-10.0, 0.0, -10.0), (10.0, 6.0, 0.0))}


def dump_tables(tmp):
    """The scene compiler's tables through the --lights dump of tests/test_scene_compile.py's program"""
    from test_scene_compile import compile_program
    exe = compile_program(tmp)
    out = {}
    for name, make in scene_tables().items():
        path, dump = tmp / (name + ".txt"), tmp / (name + ".lights")
        scenefile.save(str(path), make())
        subprocess.run([str(exe), str(path), "--lights", str(dump)], check=True, capture_output=True)
        out[name] = np.fromfile(dump, np.uint32)
    return out


def _sphere_table(centres, radii, emitted, n_sph=None):
    n = len(centres)
    r2 = R.f32(np.asarray(radii, np.float32) ** 2)
    return R.make_table(R.f32(centres), r2, R.f32(emitted), np.arange(n), np.zeros((0, 20)), n, n if n_sph is None else n_sph)


def _grid(n, emitted=None):
    c = [(-6.0 + 1.5 * (i % 8), 2.0 + 0.75 * (i // 8), -4.0 - 0.5 * (i % 3)) for i in range(n)]
    e = np.tile([[3.0, 2.0, 1.0]], (n, 1)) if emitted is None else emitted
    return _sphere_table(c, [0.1 + 0.02 * (i % 7) for i in range(n)], e)


DECADES = [0.9, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9]
DECADE_CENTRE, DECADE_D = (0.0, 5.0, -4.0), 8.0


def crafted_tables():
    """name -> table.bin words of the tables no scene compiles"""
    t = {}
    # concentric sphere lights: seen from distance d >= DECADE_D, light i subtends s2 <= DECADES[i]
    t["decades"] = _sphere_table([DECADE_CENTRE] * len(DECADES), [DECADE_D * np.sqrt(s) for s in DECADES],
                                 [[1.0, 1.0, 1.0]] * len(DECADES))
    for i, s2 in enumerate(DECADES):  # and each of them alone: 2^16 samples of one decade
        t[f"decade{i}"] = _sphere_table([DECADE_CENTRE], [DECADE_D * np.sqrt(s2)], [[1.0, 1.0, 1.0]])
    for n in (1, 2, 40, 41):
        t[f"grid{n}"] = _grid(n)
    z = np.tile([[3.0, 2.0, 1.0]], (3, 1))
    z[:2] = 0.0
    t["zero_first"] = _grid(3, z)  # the last light is the only positive one
    z = np.tile([[3.0, 2.0, 1.0]], (3, 1))
    z[1] = 0.0
    t["zero_mid"] = _grid(3, z)  # a zero-emission light between two others
    # every weight underflows: emission at the smallest normal float, the lights small and far
    t["underflow"] = _sphere_table([(1000.0 + i, 5.0, -4.0) for i in range(3)], [1e-3] * 3, [[2e-38, 0.0, 0.0]] * 3)
    # two lights that mirror each other in the plane x == 0
    t["twins"] = _sphere_table([(-1.0, 3.0, -4.0), (1.0, 3.0, -4.0)], [0.25, 0.25], [[3.0, 2.0, 1.0]] * 2)
    # three lights around the origin whose r2 is 4 - ulp, 4, 4 + ulp: P = (2, 0, 0) has d2 == 4 exactly
    e = _sphere_table([(0.0, 0.0, 0.0)] * 3, [2.0] * 3, [[1.0, 1.0, 1.0]] * 3)
    four = np.float32(4.0)
    e["r2"] = np.array([np.nextafter(four, np.float32(0)), four, np.nextafter(four, np.float32(8))], np.float64)
    t["exact_r2"] = e
    # a 1000 x 1000 quad with v0 at the origin: a point 1e-17 off its edge overflows k
    v = np.array([[0, 0, 0], [1000, 0, 0], [1000, 0, 1000], [0, 0, 1000]], np.float64)
    blk = np.concatenate([v[0], [5e5], v[1], [5e5], v[2], [1e6], v[3], [0.0], [0.0, -1e6, 0.0], [0.0]])
    t["origin_quad"] = R.make_table([[500.0, 0.0, 500.0]], [500000.0 * (1 + 2.0 ** -20)], [[1.0, 1.0, 1.0]], [7], [blk], 0, 3)
    return {k: R.table_words(v) for k, v in t.items()}


# ---- cases -------------------------------------------------------------------------------

_STATES = {}


def states(n=N):
    """n random RNG states and their reference draws (u, words, states after), computed once"""
    if n not in _STATES:
        st = np.random.default_rng(SEED).integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
        _STATES[n] = (st,) + R.draws(st)
    return _STATES[n]


CRAFT_WORDS = {"zero": 0x00000000, "one": 0xFFFFFF80, "one_max": 0xFFFFFFFF, "below_one": 0xFFFFFF00}


def crafted_states(n_each, rng):
    """States whose first, second or third draw is exactly 0, exactly 1.0 (word
    >= 0xFFFFFF80 rounds up to 2^32) or the float just below 1: XORWOW's counter
    d enters only the output sum, so d = target - output with d == 0."""
    st = rng.integers(0, 1 << 32, (n_each * 12, 6), dtype=np.uint64).astype(np.uint32)
    st[:, 0] = 0
    _, words, _ = R.draws(st)
    i = 0
    for draw in range(3):
        for target in CRAFT_WORDS.values():
            sl = slice(i, i + n_each)
            st[sl, 0] = (np.uint64(target) - words[sl, draw].astype(np.uint64)).astype(np.uint32)
            i += n_each
    return st


def state_with_draw(draw, word, n, rng):
    """n states whose draw number `draw` (0 .. 2) is the word `word`"""
    st = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    st[:, 0] = 0
    _, words, _ = R.draws(st)
    st[:, 0] = (np.uint64(word) - words[:, draw].astype(np.uint64)).astype(np.uint32)
    return st


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(1))[:, None]


def light_geometry(t):
    """per table light: a point of it, its unit normal there (spheres: towards +y) and its extent"""
    nsl = t["n_sphere_lights"]
    pts, nrm = t["centre"].copy(), np.tile([[0.0, 1.0, 0.0]], (len(t["prim"]), 1))
    pts[:nsl, 1] += np.sqrt(t["r2"][:nsl])
    for i, b in enumerate(t["blocks"]):
        pts[nsl + i] = b[0:3] + 0.3 * (b[4:7] - b[0:3]) + 0.3 * (b[8:11] - b[0:3])
        nrm[nsl + i] = b[16:19] / b[11]
    return pts, nrm


def sample_cases(name, words, shapes, n=N, edges=True):
    """The cases of a nee_sample run on table `name`: dict(words (n, 14) uint32,
    random (n,) bool: the random part, the edge families behind it), drawn with
    a fixed seed.  Consecutive random cases come from different families: floor
    points, free points with unit, stretched and short normals, points facing
    or lying on a light."""
    t, _ = R.table_from_words(words)
    L, nsl = R.seen(t, shapes), t["n_sphere_lights"]
    rng = np.random.default_rng([SEED, sum(map(ord, name)), shapes])
    c, rad = t["centre"][:L], np.sqrt(t["r2"][:L])
    lo, hi = BOXES.get(name, ((c - rad[:, None]).min(0) - 3.0, (c + rad[:, None]).max(0) + 3.0))
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    foreign = t["n_sph"]  # the floor of every scene here: a plane is never a table light
    P = rng.uniform(lo, hi, (n, 3))
    if name.startswith("decade"):  # on a shell 8 .. 12 around the common centre: light i subtends at most DECADES[i]
        P = np.asarray(DECADE_CENTRE) + _unit(rng, n) * rng.uniform(DECADE_D, 1.5 * DECADE_D, (n, 1))
    nrm = _unit(rng, n)
    prim = np.full(n, foreign, np.int64)
    kind = np.ones(n, np.int64)
    fam = np.arange(n) % 8
    floor = fam < 3
    if name.startswith("decade"):  # (no floor: these normals lean towards the light, so most cases are traced)
        to = np.asarray(DECADE_CENTRE) - P
        nrm[fam < 5] = (to / np.sqrt((to * to).sum(1))[:, None] + 0.5 * nrm)[fam < 5]
        nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    else:
        P[floor, 1] = lo[1] if name not in BOXES else 0.0
        nrm[floor] = [0.0, 1.0, 0.0]
    k2 = fam == 5
    nrm[k2] *= np.sqrt(rng.choice([0.64, 2.0, 4.0, 40000.0], k2.sum()))[:, None]
    kind[k2] = 2
    k0 = fam == 6
    nrm[k0] *= np.sqrt(0.3)
    kind[k0] = 0
    face = fam == 7
    pick = rng.integers(0, L, n)
    to = c[pick] - P
    nrm[face] = (to / np.sqrt((to * to).sum(1))[:, None])[face]
    on = face & (rng.random(n) < 0.5)
    prim[on] = t["prim"][pick][on]
    if L > nsl and name not in BOXES:
        # (after the floor was laid:) the random points stay where the reference calls a polygon sample well-conditioned: 4 ulp of the
        # coordinates' magnitude M (the displacement of Q in k's sensitivity interval) is 2^-21 M, which moves
        # a direction by 2^-20 at a ray length of M / 2.  Nearer points are ill-conditioned cases (counted,
        # capped at 1 % of a random set); the edge families below go there on purpose.
        B = t["blocks"]
        M = np.abs(np.concatenate([B[:, 0:3], B[:, 4:7], B[:, 8:11], B[:, 12:15]])).max()
        for _ in range(16):  # (a point moved away from one light may land next to another)
            for m in range(nsl, L):
                off = P - c[m]
                d = np.sqrt((off * off).sum(1))
                keep = np.maximum(M, np.abs(P).max(1)) / 2.0
                near = d < rad[m] + keep
                grow = (rad[m] + keep * (1.0 + rng.random(n))) / np.maximum(d, 1e-9)
                P[near] = c[m] + off[near] * grow[near, None]
    st = states(N)[0][:n].copy()
    random = np.ones(n, bool)
    if edges:
        e = _edge_cases(name, t, L, foreign, rng, lo, hi)
        m = len(e["P"])
        P[n - m:], nrm[n - m:], prim[n - m:], kind[n - m:] = e["P"], e["n"], e["prim"], e["kind"]
        st[n - m:] = e["state"]
        random[n - m:] = False
    out = np.zeros((n, 14), np.uint32)
    out[:, 0:6] = st
    out[:, 6:9] = R.f32(P).view(np.uint32)
    out[:, 9:12] = R.f32(nrm).view(np.uint32)
    out[:, 12] = prim.astype(np.int32).view(np.uint32)
    out[:, 13] = kind.astype(np.int32).view(np.uint32)
    return dict(words=out, random=random)


def _edge_cases(name, t, L, foreign, rng, lo, hi):
    """The edge families of a sample run (a few hundred cases each): crafted
    draws; NaN normals; and, where the shadow ray is not short against the
    coordinates' float spacing, points on, inside, at the rim of and next to
    the lights."""
    parts = []

    def add(P, n, prim, kind=1, state=None):
        P = np.atleast_2d(np.asarray(P, np.float64))
        m = len(P)
        parts.append(dict(P=P, n=np.broadcast_to(np.asarray(n, np.float64), (m, 3)).copy(),
                          prim=np.broadcast_to(np.asarray(prim, np.int64), (m,)).copy(),
                          kind=np.broadcast_to(np.asarray(kind, np.int64), (m,)).copy(),
                          state=rng.integers(0, 1 << 32, (m, 6), dtype=np.uint64).astype(np.uint32) if state is None else state))

    cs = crafted_states(24, rng)
    Pf = rng.uniform(lo, hi, (len(cs), 3))
    Pf[:, 1] = lo[1] if name not in BOXES else 0.0
    add(Pf, [0.0, 1.0, 0.0], foreign, 1, cs)
    add(rng.uniform(lo, hi, (256, 3)), [np.nan, 0.0, 1.0], foreign, 0)
    if name not in BOXES:
        pts, nrm = light_geometry(t)
        c, rad, nsl = t["centre"], np.sqrt(t["r2"]), t["n_sphere_lights"]
        reps = 32
        for m in range(min(L, 8)):
            ids = t["prim"][m]
            if m < nsl:
                d = _unit(rng, reps)
                add(c[m] + rad[m] * d, d, ids)            # on the light itself
                add(c[m] + rad[m] * d, d, foreign)        # at d2 == r2 within rounding
                add(c[m] + 0.5 * rad[m] * d, d, foreign)  # inside it
                add(c[m] + rad[m] * (1 + 2.0 ** -8) * d, -d, foreign)  # just outside, facing away
            else:
                nl = nrm[m]
                side = np.where(rng.random(reps) < 0.5, 1.0, -1.0)[:, None]
                add(np.tile(pts[m], (reps, 1)), nl, ids, 1)                           # on the light itself
                add(np.tile(pts[m], (reps, 1)) + 2.0 * _unit(rng, reps) * [1, 0, 1], nl, foreign, 1)  # in its plane (about)
                add(c[m] + 0.3 * rad[m] * side * nl, -side * nl, foreign)            # inside the bounding sphere
                b = t["blocks"][m - nsl]
                add(b[0:3] + 1e-6 * side * nl, -side * nl, foreign)                   # next to a vertex
                add(c[m] + 0.3 * rad[m] * side * nl, -side * nl * np.sqrt(2.0), foreign, 2)
    if name == "twins":
        # u == 1/2 exactly on two lights of equal weight (P in their plane of symmetry): run == target, not beyond
        Pt = R.f32(np.stack([np.zeros(256), rng.uniform(-1, 2, 256), rng.uniform(-7, -1, 256)], 1)).astype(np.float64)
        add(Pt, [0.0, 1.0, 0.0], foreign, 1, state_with_draw(0, 0x80000000, 256, rng))
    if name == "exact_r2":
        add(np.tile([[2.0, 0.0, 0.0]], (256, 1)), [-1.0, 0.0, 0.0], foreign)
        add(np.tile([[0.0, -2.0, 0.0]], (256, 1)), [0.0, 1.0, 0.0], foreign)
    if name == "origin_quad":
        # u1 == 0 exactly puts the sample on v2, in float as in double: P lies 1e-17 beside it
        st = crafted_states(64, rng)[64 * 4:64 * 5]  # second draw, word 0
        u, _, _ = R.draws(st)
        assert (u[:, 1] == 0.0).all()
        add(np.tile([[1000.0, 1e-17, 1000.0]], (64, 1)), [0.0, -1.0, 0.0], foreign, 1, st)
        add(np.tile([[1000.0, -1e-17, 1000.0]], (64, 1)), [0.0, 1.0, 0.0], foreign, 1, st)
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def weight_cases(words, n=N):
    """cases of nee_pick_weight / nee_pick_weight_poly: {m, P, n, nl, prim} over the whole table"""
    s = sample_cases("weights", words, R.ALL, n)["words"]
    t, _ = R.table_from_words(words)
    rng = np.random.default_rng([SEED, 4])
    nrm = s[:, 9:12].view(np.float32).astype(np.float64)
    kind = s[:, 13].view(np.int32)
    with np.errstate(invalid="ignore"):
        nl = np.where(kind == 2, np.sqrt((nrm * nrm).sum(1)), 1.0)
    out = np.zeros((n, 9), np.uint32)
    out[:, 0] = rng.integers(0, len(t["prim"]), n).astype(np.uint32)
    out[:, 1:7] = s[:, 6:12]
    out[:, 7] = R.f32(nl).view(np.uint32)
    out[:, 8] = s[:, 12]
    return out


def suppressed_cases(words, n=N):
    """cases of light_suppressed: {P, prim, id}; id runs over every table id, the
    ids between them, -1 and ids beyond the last; P also on the sphere lights"""
    t, _ = R.table_from_words(words)
    s = sample_cases("suppressed", words, R.ALL, n)["words"]
    rng = np.random.default_rng([SEED, 6])
    last = int(t["prim"].max())
    ids = np.arange(-1, last + 4)
    out = np.zeros((n, 5), np.uint32)
    out[:, 0:3] = s[:, 6:9]
    ident = ids[np.arange(n) % len(ids)]
    prim = np.where(rng.random(n) < 0.3, ident, rng.choice(np.concatenate([ids, [t["n_sph"]]]), n))
    out[:, 3] = prim.astype(np.int32).view(np.uint32)
    out[:, 4] = ident.astype(np.int32).view(np.uint32)
    return out


def fold_table(words, rows=6):
    """the table with a small hit table behind it, and that hit table"""
    t, _ = R.table_from_words(words)
    rng = np.random.default_rng([SEED, 8])
    hit = rng.uniform(0.0, 4.0, (rows, 16)).astype(np.float32)
    hit[1, 4:7] = 0.0
    return R.table_words(t, hit), hit


def fold_cases(words, rows=6, n=N):
    """cases of fold_level_nee: {c0, k, c, aux, L}: diffuse and specular levels, every aux flag, every light"""
    t, _ = R.table_from_words(words)
    rng = np.random.default_rng([SEED, 9])
    row = rng.integers(0, rows, n)
    c0 = np.where(rng.random(n) < 0.3, ~row, row)
    aux = rng.integers(0, 8, n) | (rng.integers(0, len(t["prim"]), n) << R.RT_NEE_JSHIFT)
    aux[rng.random(n) < 0.2] = 0
    f = rng.uniform(0.0, 3.0, (n, 5)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, np.nan, 1e-40, 3e38, -1.5], np.float32)
    sel = rng.random((n, 5)) < 0.05
    f[sel] = rng.choice(special, sel.sum())
    out = np.zeros((n, 7), np.uint32)
    out[:, 0] = c0.astype(np.int32).view(np.uint32)
    out[:, 1:3] = f[:, 0:2].view(np.uint32)
    out[:, 3] = aux.astype(np.int32).view(np.uint32)
    out[:, 4:7] = f[:, 2:5].view(np.uint32)
    return out


def kind_edge_cases():
    """The exact cases of nee_normal_kind: (sphere flag, n, the kind demanded;
    None: the reference leaves it undecided, any of 0, 1, 2 passes)"""
    inf, nan, h = np.inf, np.nan, 0.5
    e = []
    for n in ((0, 1, 0), (0, 0, -1), (-1, 0, 0), (0.5, 0.5, np.sqrt(0.5))):  # |n|^2 exactly 1 (the last: within rounding, not exact)
        e.append((0, n, 1 if n[0] != 0.5 else None))
    e += [(0, (h, h, 0), 0), (0, (0, -h, h), 0),                      # exactly 1/2: no level
          (0, (h, h, 2.0 ** -12), 2), (0, (h, 2.0 ** -12, -h), 2),     # 1/2 + 2^-24, the float above 1/2
          (0, (h, h, 2.0 ** -14), None),                               # 1/2 + 2^-28 is no float (it rounds to 1/2): undecided
          (0, (1, 2.0 ** -12, 0), None),                               # 1 + 2^-24 is no float (it rounds to 1): undecided
          (0, (1, 2.0 ** -11, 0), 2),                                  # 1 + 2^-22: a float, exact, kind 2
          (0, (2, 0, 0), 2), (0, (0, 0.8, 0), 2), (0, (0, 0.7, 0), 0), (0, (0, 0, 0), 0), (0, (1e-30, 0, 0), 0),
          (0, (inf, 0, 0), 0), (0, (0, -inf, 1), 0), (0, (3e19, 3e19, 0), 0), (0, (1e19, 1e19, 1e19), 2),  # +inf, overflow, 3e38
          (0, (nan, 0, 1), 0), (0, (0, 1, nan), 0), (0, (nan, nan, nan), 0), (0, (inf, nan, 0), 0)]
    for n in ((0, 1, 0), (0, 0, 0), (h, h, 0), (7, 0, 0), (inf, 0, 0), (nan, 0, 1), (nan, nan, nan), (0.1, 0.1, 0.1)):
        e.append((1, n, 1))                                            # the sphere flag, whatever n
    return e


def kind_cases(n=N):
    """cases of nee_normal_kind: {sphere, n}: directions scaled to |n|^2 around
    1/2, 1 and far from both, the sphere flag on an eighth, the exact cases last"""
    rng = np.random.default_rng([SEED, 9, 9])
    nn = rng.choice([0.25, 0.49, 0.5, 0.51, 0.64, 1.0, 1.25, 2.0, 4.0, 40000.0, 1e-12, 1e30], n) * \
        np.where(rng.random(n) < 0.5, 1.0, 1.0 + rng.normal(size=n) * 2.0 ** -18)
    nrm = _unit(rng, n) * np.sqrt(nn)[:, None]
    axis = rng.random(n) < 0.25  # axis-aligned: |n|^2 is one exact square
    nrm[axis] = np.eye(3)[rng.integers(0, 3, axis.sum())] * np.sqrt(nn[axis])[:, None]
    sphere = rng.random(n) < 0.125
    edge = kind_edge_cases()
    m = len(edge)
    sphere[n - m:] = [s for s, _, _ in edge]
    nrm[n - m:] = [v for _, v, _ in edge]
    out = np.zeros((n, 4), np.uint32)
    out[:, 0] = sphere
    with np.errstate(over="ignore"):
        out[:, 1:4] = R.f32(nrm).view(np.uint32)
    return out


def check_kind(cases, out):
    """nee_normal_kind against float64 on |n|^2, wherever that decides; the exact cases by name"""
    want, dec = R.normal_kind(cases[:, 0] != 0, _f(cases[:, 1:4]))
    got = out.view(np.int32)
    assert len(got) == len(cases)
    edge = kind_edge_cases()
    m = len(edge)
    demanded = [k for _, _, k in edge]
    for i, k in enumerate(demanded):  # stated by hand, and the reference agrees with the hand
        if k is not None:
            assert dec[len(cases) - m + i] and want[len(cases) - m + i] == k, (edge[i], want[len(cases) - m + i])
    # (about 8 % of the random cases sit on 1/2 or 1 within 2^-20 on purpose; each kind is a twentieth at the least)
    assert dec[:len(cases) - m].mean() > 0.8 and all((want[:len(cases) - m] == k).mean() > 0.05 for k in (0, 1, 2))
    bad = np.nonzero(dec & (got != want))[0]
    assert len(bad) == 0, ("kind", bad[:8], got[bad[:8]], want[bad[:8]], _f(cases[bad[:8], 1:4]))
    assert np.isin(got, (0, 1, 2)).all()
    return int(dec.sum())


# ---- the runs ----------------------------------------------------------------------------

# (table, function id): the nee_sample runs; 0 / 1 uniform / weighted over the spheres, 2 / 3 over all shapes
DECADE_RUNS = [(f"decade{i}", 0) for i in range(len(DECADES))]
SAMPLE_RUNS = [(t, f) for t in ("07", "eight_lights") for f in (0, 1)] + DECADE_RUNS + \
              [(t, f) for t in ("quad_panel", "triangle_panel", "mixed", "box_front", "stress_tri", "quad_1_3", "lifted_quad",
                                "far_triangle", "exclusions") for f in (2, 3)] + \
              [("decades", 0), ("grid1", 1), ("grid2", 1), ("grid40", 0), ("grid40", 1), ("grid41", 0), ("grid41", 1),
               ("zero_first", 1), ("zero_mid", 1), ("twins", 1), ("underflow", 1), ("exact_r2", 0), ("origin_quad", 2)]
DIVERGENT_RUN = ("mixed", 3)  # spheres and polygons, all kinds, 7 lights: the weighted break leaves at every m
OTHER_RUNS = [("eight_lights", 4), ("exact_r2", 4), ("quad_panel", 5), ("mixed", 6), ("mixed", 7), ("07", 8), ("07", 9)]


def run_inputs(tables, table, fid):
    """(table.bin words, cases words, random mask or None) of one run"""
    w = tables[table]
    if fid <= 3:
        s = sample_cases(table, w, R.SPHERES if fid < 2 else R.ALL)
        return w, s["words"], s["random"]
    if fid in (4, 5):
        return w, weight_cases(w), None
    if fid in (6, 7):
        return w, suppressed_cases(w), None
    if fid == 9:
        return w, kind_cases(), None
    return fold_table(w)[0], fold_cases(w), None


def run_probe(args, fid, table_words, case_words, tmp, timeout=60):
    """One probe run: args = [binary] for both passes, [binary, "--host"] for the
    host pass alone.  Returns the subprocess result and (device words or None,
    host words) if it ended well."""
    tp, cp, out = tmp / "table.bin", tmp / "cases.bin", tmp / "out.bin"
    table_words.tofile(tp)
    case_words.tofile(cp)
    host_only = len(args) > 1
    outs = [str(out) + ".host"] if host_only else [str(out), str(out) + ".host"]
    r = subprocess.run([*args, str(fid), str(tp), str(cp), *outs], capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        return r, None, None
    return r, None if host_only else np.fromfile(outs[0], np.uint32), np.fromfile(outs[-1], np.uint32)


# ---- the conditions ----------------------------------------------------------------------

def _f(words):
    return np.ascontiguousarray(words).view(np.float32).astype(np.float64)


def sample_reference(words, fid, cases):
    """The reference's answer to a sample run (before the product is consulted)"""
    t, _ = R.table_from_words(words)
    u, _, after = R.draws(cases[:, 0:6])
    ref = R.nee_sample(t, fid & 1, fid >> 1, u, _f(cases[:, 6:9]), _f(cases[:, 9:12]), cases[:, 12].view(np.int32),
                       cases[:, 13].view(np.int32))
    ref["after"] = after
    ref["u"] = u
    ref["table"] = t
    return ref


def check_undecided_share(ref, random):
    """At most 1 % of the random cases are undecided, and at most 1 % of the
    random traced ones are ill-conditioned (nee_ref: left out of the value
    checks) — on the reference alone.  Returns the counts (undecided random,
    undecided edge, ill-conditioned traced)."""
    und = ~(ref["margin"] > R.DECIDED)
    share = und[random].mean()
    assert share <= 0.01, share
    lit = ref["trace"] & ~und
    if (lit & random).any():
        assert ref["ill"][lit & random].mean() <= 0.01, ref["ill"][lit & random].mean()
    return int(und[random].sum()), int(und[~random].sum()), int((lit & ref["ill"]).sum())


def check_sample(ref, cases, out):
    """The conditions of a sample run on the probe's output words (n, 13).
    Returns the number of decided cases and of traced ones among them."""
    out = out.reshape(-1, 13)
    assert len(out) == len(cases)
    # the RNG state: three steps, in every case
    bad = np.nonzero((out[:, 7:13] != ref["after"]).any(1))[0]
    assert len(bad) == 0, ("RNG state", bad[:8])
    dec = ref["margin"] > R.DECIDED
    j, prim, trace = out[:, 0].view(np.int32), out[:, 1].view(np.int32), out[:, 2] != 0
    for name, got in (("j", j), ("prim", prim), ("trace", trace)):
        bad = np.nonzero(dec & (got != ref[name]))[0]
        assert len(bad) == 0, (name, bad[:8], got[bad[:8]], ref[name][bad[:8]], ref["margin"][bad[:8]])
    k, wi = _f(out[:, 3]), _f(out[:, 4:7])
    none = dec & ~ref["trace"]
    bad = np.nonzero(none & ((k != 0) | (wi != 0).any(1)))[0]
    assert len(bad) == 0, ("k and wi are 0 without a sample", bad[:8], k[bad[:8]], wi[bad[:8]])
    lit = dec & ref["trace"] & ~ref["ill"]
    err = np.abs(wi - ref["wi"]).max(1)
    bad = np.nonzero(lit & ~(err <= R.WI_TOL))[0]
    assert len(bad) == 0, ("wi", len(bad), bad[:8], err[bad[:8]], ref["s2"][bad[:8]])
    rel = R.K_REL + ref["k_rel"]
    bad = np.nonzero(lit & ~((k >= ref["k_lo"] * (1 - rel)) & (k <= ref["k_hi"] * (1 + rel))))[0]
    assert len(bad) == 0, ("k", len(bad), bad[:8], k[bad[:8]], ref["k_lo"][bad[:8]], ref["k_hi"][bad[:8]])
    return int(dec.sum()), int(lit.sum())


def miss_shares(ref, cases, random, out):
    """Over the random cases of a run on a `decade` table, per table light:
    (traced samples, those whose float wi misses the light in float64 geometry,
    those whose reference wi rounded once to float misses it)."""
    out = out.reshape(-1, 13)
    t = ref["table"]
    P = _f(cases[:, 6:9])
    lit = random & ref["trace"] & (ref["margin"] > R.DECIDED) & (out[:, 2] != 0)

    def misses(wi):
        j = ref["j"]
        w = t["centre"][j] - P
        wi = wi / np.sqrt((wi * wi).sum(1))[:, None]
        along = (w * wi).sum(1)
        return (w * w).sum(1) - along * along > t["r2"][j]

    with np.errstate(invalid="ignore"):
        got, ideal = misses(_f(out[:, 4:7])), misses(R.f32(ref["wi"]).astype(np.float64))
    rows = []
    for d in range(len(t["prim"])):
        sel = lit & (ref["j"] == d)
        rows.append((int(sel.sum()), int((sel & got).sum()), int((sel & ideal).sum())))
    return rows


def _weight_inputs(words, cases):
    t, _ = R.table_from_words(words)
    nsl = t["n_sphere_lights"]
    m = cases[:, 0].astype(np.int64)
    P, n, nl, prim = _f(cases[:, 1:4]), _f(cases[:, 4:7]), _f(cases[:, 7]), cases[:, 8].view(np.int32).astype(np.int64)
    return t, m, P, n, nl, prim, nsl


def weights_reference(words, fid, cases):
    t, m, P, n, nl, prim, nsl = _weight_inputs(words, cases)
    w, dec, extra = np.zeros(len(m)), np.zeros(len(m), bool), np.zeros(len(m), bool)
    for light in range(len(t["prim"])):
        sel = m == light
        if sel.any():
            w[sel], dec[sel], extra[sel] = R.pick_weight(t, light, P[sel], n[sel], nl[sel], prim[sel], fid == 5)
    return w, dec, extra


def check_weight_values(w, dec, extra, out):
    got = _f(out)
    assert dec.mean() > 0.9 and extra[dec & (w > 0)].mean() <= 0.01
    dec = dec & ~extra
    bad = np.nonzero(dec & (w == 0) & (out != 0))[0]
    assert len(bad) == 0, ("weight exactly 0", bad[:8], got[bad[:8]])
    ok = (np.abs(got - w) <= R.WEIGHT_REL * w) | (np.abs(got - w) <= R.FLT_MIN)
    bad = np.nonzero(dec & ~ok)[0]
    assert len(bad) == 0, ("weight", bad[:8], got[bad[:8]], w[bad[:8]])
    return int(dec.sum())


def check_suppressed(words, fid, cases, out):
    t, _ = R.table_from_words(words)
    ref, dec = R.suppressed(t, fid - 6, _f(cases[:, 0:3]), cases[:, 3].view(np.int32), cases[:, 4].view(np.int32))
    assert dec.mean() > 0.9 and ref.any() and not ref.all()
    bad = np.nonzero(dec & ((out != 0) != ref))[0]
    assert len(bad) == 0, ("suppressed", bad[:8])
    return int(dec.sum())


def check_fold(words, cases, out):
    t, _ = R.table_from_words(words)
    _, hit = fold_table(words)
    want = R.fold(cases[:, 0].view(np.int32), cases[:, 1].view(np.float32), cases[:, 2].view(np.float32),
                  cases[:, 3].view(np.int32), hit, t["emitted"], cases[:, 4:7].view(np.float32))
    got = out.reshape(-1, 3).view(np.float32)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.nonzero(~same.all(1))[0]
    assert len(bad) == 0, ("fold", bad[:8], got[bad[:8]], want[bad[:8]])


def check_run(tables, table, fid, cases, random, out, ref=None):
    """Every reference condition of one run on one pass's output words; returns a line of figures"""
    w = tables[table]
    if fid <= 3:
        ref = sample_reference(w, fid, cases) if ref is None else ref
        und = check_undecided_share(ref, random)
        dec, lit = check_sample(ref, cases, out)
        return f"{table}/{fid}: undecided {und[0]} random + {und[1]} edge of {len(cases)}, traced and checked {lit}, {und[2]} ill-conditioned"
    if fid in (4, 5):
        wt, dec, extra = weights_reference(w, fid, cases)
        return f"{table}/{fid}: {check_weight_values(wt, dec, extra, out)} decided weights, {int((dec & extra).sum())} more ill-conditioned"
    if fid in (6, 7):
        return f"{table}/{fid}: {check_suppressed(w, fid, cases, out)} decided"
    if fid == 9:
        return f"{table}/{fid}: {check_kind(cases, out)} decided kinds of {len(cases)}"
    check_fold(w, cases, out)
    return f"{table}/{fid}: equal bits"
