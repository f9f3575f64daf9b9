"""The replay driver of the next-event-estimation path loop: a fourth,
independent text of the loop that csrc/rt_kernel_lane.h (twice: the shadow ray
inline and deferred) and csrc/rt_cpu.cpp state, written from the comment at
the head of csrc/rt_light.h and DESIGN.md sections 23 to 25 — not from those
files.  tests/test_nee_path.py holds the CPU twin to it bit for bit,
tests/test_gpu_nee_path.py the kernels.

It holds the state of every pixel of a small frame and advances all live paths
one level at a time.  Every building block is pinned elsewhere and used as it
is:

* the camera ray, the closest hit and the scattering are the oracle's own
  functions (oracle.camera_rays / closest_hits / scatter);
* nee_normal_kind, nee_sample in its four modes and light_suppressed are the
  host pass of build/neeprobe_cpu, one run per level over all live paths
  (tests/test_nee_reference.py holds that pass to the float64 reference);
* the light table is the scene compiler's --lights dump, its ids those of
  nee_ref.light_table;
* the fold is float32 numpy, one rounding per operation, and is cross-checked
  against nee_ref.fold level by level.

What the driver alone decides — the loop:

* a hit is an NEE LEVEL iff light sampling is on, the diffuse branch was taken,
  depth + 1 <= max_bounces, the table of the current shapes mode is not empty,
  and nee_normal_kind of the hit's normal is not 0;
* an NEE level draws three numbers, always, behind random_direction's draws;
* its sample is VISIBLE iff it is traced and the oracle's closest hit from the
  level's point along wi is the sampled light's primitive;
* the SUPPRESSION is asked at the next hit of the path, with the level's point
  and primitive and the new hit's primitive; a miss, the path's end and the next
  inner path of samples_per_pixel all start without one;
* per level, innermost first:  L = (dropped ? 0 : emitted) [+ direct] +
  (brdf * L) * cosAngle,  direct = k * (diffuse_brdf * emitted_j) if visible,
  else 0, and the `+ direct` at NEE levels only;
* of the samples_per_pixel inner paths of a frame the last one is kept, scaled
  by 1 / samples_per_pixel; frame 1 resets the accumulation.
"""
import numpy as np

import nee_cases as K
import nee_ref as R
import oracle as O

PROBE_CPU = [K.BUILD + "/neeprobe_cpu", "--host"]
UNIFORM, WEIGHTED = R.UNIFORM, R.WEIGHTED
SPHERES, ALL = R.SPHERES, R.ALL
DROP, LEVEL, VISIBLE, JSHIFT = R.RT_NEE_DROP, R.RT_NEE_LEVEL, R.RT_NEE_VISIBLE, R.RT_NEE_JSHIFT

# one record per hit of every path ("level"); the first five fields are the
# level's tuple, the rest is what the coverage counts of tests/test_nee_path.py read
LEVEL_DTYPE = np.dtype([("pixel", np.int32), ("frame", np.int32), ("depth", np.int32), ("prim", np.int32), ("aux", np.int32),
                        ("inner", np.int32),     # which of the frame's samples_per_pixel paths
                        ("specular", bool),      # the specular branch was taken
                        ("kind", np.int32),      # nee_normal_kind where it was asked, else -1
                        ("traced", bool),        # an NEE level whose sample has a shadow ray
                        ("asked", bool),         # the previous level of the path was an NEE level
                        ("on_light", bool),      # the hit primitive is a light of the current table
                        ("inherit", bool)])      # depth 0 of an inner path whose predecessor ended behind an NEE level


def _f32(x):
    return np.asarray(x, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """float arrays equal bit for bit; a NaN equals any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def light_words(scene, tmp, name="scene"):
    """The scene compiler's light table of `scene` as table.bin words (the --lights
    dump of tests/test_scene_compile.py's program, built once per directory)."""
    import subprocess

    from bwrt import scenefile
    from test_scene_compile import compile_program
    exe = tmp / "scene_compile"
    if not exe.exists():
        compile_program(tmp)
    path, dump = tmp / (name + ".txt"), tmp / (name + ".lights")
    scenefile.save(str(path), scene)
    subprocess.run([str(exe), str(path), "--lights", str(dump)], check=True, capture_output=True)
    return np.fromfile(dump, np.uint32)


def tonemap(frame_sum, frames):
    """RGBA8 of a frameSum after `frames` frames, by the oracle's own text: one
    more pass of orc_render_rows over the empty scene (every ray misses and
    adds the background, 0) on a copy of the sum.  frames >= 2."""
    from bwrt import scenes
    assert frames >= 2, "frame 1 resets the sum"
    rows, width = frame_sum.shape[:2]
    st = O.OracleState(width, rows)
    st.accum[...] = frame_sum
    return O.render(scenes.empty_scene(), st, 1, 0, first_frame=frames).copy()


class Driver:
    """driver = Driver(scene, width, height, table, tmp, ...); driver.render(frames,
    max_bounces); then driver.frame_sum() (rows, width, 3), driver.rng_state()
    (6, rows, width) and driver.levels (LEVEL_DTYPE)."""

    def __init__(self, scene, width, height, table, tmp, light_sampling=True, pick=UNIFORM, shapes=SPHERES,
                 samples_per_pixel=1, row_offset=0, row_stride=1, background=(0.0, 0.0, 0.0)):
        self.scene, self.width, self.height, self.tmp = scene, width, height, tmp
        self.nee, self.pick, self.shapes, self.spp = bool(light_sampling), pick, shapes, int(samples_per_pixel)
        self.background = _f32(background)
        ys = np.arange(row_offset, height, row_stride, dtype=np.int32)
        self.rows = len(ys)
        self.y = np.repeat(ys, width)
        self.x = np.tile(np.arange(width, dtype=np.int32), self.rows)
        self.n = len(self.x)
        self.rng = np.stack([O.curand_init(int(y) * width + int(x)) for x, y in zip(self.x, self.y)]).astype(np.uint32)
        self.accum = np.zeros((self.n, 3), np.float32)
        self.frame = 1
        self.levels = np.zeros(0, LEVEL_DTYPE)
        self.probe_runs = 0
        # the table, and what the current shapes mode sees of it
        if table is None:  # (without light sampling no table is looked at)
            assert not self.nee
            table = R.table_words(R.make_table([], [], [], [], [], 0, scene.counts[0]))
        self.table_words = np.asarray(table, np.uint32)
        t, _ = R.table_from_words(self.table_words)
        if self.nee:
            want = R.light_table(scene)
            assert np.array_equal(t["prim"], want["prim"]) and t["n_sphere_lights"] == want["n_sphere_lights"]
        self.n_lights = R.seen(t, shapes)
        self.light_prims = t["prim"][:self.n_lights].astype(np.int32)
        self.light_emitted = _f32(t["emitted"])

    # -- the pinned building blocks --------------------------------------------------------
    def _probe(self, fid, cases):
        r, _, out = K.run_probe(PROBE_CPU, fid, self.table_words, np.ascontiguousarray(cases, np.uint32), self.tmp)
        assert r.returncode == 0, (r.args, r.stdout, r.stderr)
        self.probe_runs += 1
        return out

    def _kind(self, sphere, normal):
        cases = np.zeros((len(normal), 4), np.uint32)
        cases[:, 0] = sphere
        cases[:, 1:4] = _bits(normal)
        return self._probe(9, cases).view(np.int32)

    def _sample(self, state, P, normal, prim, kind):
        cases = np.zeros((len(P), 14), np.uint32)
        cases[:, 0:6] = state
        cases[:, 6:9], cases[:, 9:12] = _bits(P), _bits(normal)
        cases[:, 12], cases[:, 13] = prim.astype(np.int32).view(np.uint32), kind.astype(np.int32).view(np.uint32)
        out = self._probe(self.pick + 2 * self.shapes, cases).reshape(-1, 13)
        return dict(j=out[:, 0].view(np.int32), prim=out[:, 1].view(np.int32), trace=out[:, 2] != 0,
                    k=out[:, 3].copy().view(np.float32), wi=out[:, 4:7].copy().view(np.float32), state=out[:, 7:13])

    def _suppressed(self, P, prim, ident):
        cases = np.zeros((len(P), 5), np.uint32)
        cases[:, 0:3] = _bits(P)
        cases[:, 3], cases[:, 4] = prim.astype(np.int32).view(np.uint32), ident.astype(np.int32).view(np.uint32)
        return self._probe(6 + self.shapes, cases) != 0

    # -- the loop ----------------------------------------------------------------------------
    def render(self, frames, max_bounces, first_frame=None):
        if first_frame is not None:
            self.frame = first_frame
        for _ in range(frames):
            origin, direction, self.rng = O.camera_rays(self.scene, self.width, self.height, self.x, self.y, self.rng)
            ended_behind_level = np.zeros(self.n, bool)
            for inner in range(self.spp):  # the last one is kept
                val, ended_behind_level = self._paths(origin, direction, max_bounces, inner, ended_behind_level)
            val = np.float32(1.0) / np.float32(self.spp) * val
            if self.frame == 1:
                self.accum[...] = 0.0
            self.accum = self.accum + val
            self.frame += 1

    def _paths(self, origin, direction, max_bounces, inner, inherit):
        n = self.n
        ray_o, ray_d = origin.copy(), direction.copy()
        alive = np.arange(n)
        pend = np.zeros(n, bool)  # the path's previous level was an NEE level, at pend_P on pend_prim
        pend_P, pend_prim = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        ended = np.zeros(n, bool)  # the path ended by a miss behind an NEE level
        folds, records = [], []
        with np.errstate(all="ignore"):
            for depth in range(max_bounces + 1):
                if len(alive) == 0:
                    break
                hit = O.closest_hits(self.scene, ray_o[alive], ray_d[alive])
                on = hit["kind"] >= 0
                ended[alive[~on]] = pend[alive[~on]]  # a miss ends the path, here behind an NEE level
                pend[alive[~on]] = False
                idx = alive[on]
                if len(idx) == 0:
                    alive = idx
                    break
                prim, P, normal, mat = hit["prim"][on], hit["point"][on], hit["normal"][on], hit["material"][on]
                m = len(idx)
                # the suppression of the level before, asked here
                asked = pend[idx].copy()
                drop = np.zeros(m, bool)
                if asked.any():
                    drop[asked] = self._suppressed(pend_P[idx][asked], pend_prim[idx][asked], prim[asked])
                pend[idx] = False
                specular, scat, brdf, self.rng[idx] = O.scatter(self.rng[idx], ray_d[idx], normal, mat)
                emitted = mat[:, 3:4] * mat[:, 0:3]
                cos = (scat[:, 0] * normal[:, 0] + scat[:, 1] * normal[:, 1]) + scat[:, 2] * normal[:, 2]
                # an NEE level?
                kind = np.full(m, -1, np.int32)
                level = np.zeros(m, bool)
                if self.nee and self.n_lights > 0 and depth + 1 <= max_bounces:
                    cand = ~specular
                    if cand.any():
                        kind[cand] = self._kind(hit["kind"][on][cand] == O.KIND_SPHERE, normal[cand])
                    level = cand & (kind != 0)
                aux = np.where(drop, DROP, 0).astype(np.int32)
                k = np.zeros(m, np.float32)
                traced = np.zeros(m, bool)
                if level.any():
                    s = self._sample(self.rng[idx[level]], P[level], normal[level], prim[level], kind[level])
                    self.rng[idx[level]] = s["state"]
                    visible = np.zeros(level.sum(), bool)
                    if s["trace"].any():
                        tr = s["trace"]
                        shadow = O.closest_hits(self.scene, P[level][tr], s["wi"][tr])
                        visible[tr] = shadow["prim"] == s["prim"][tr]
                    aux[level] |= LEVEL | np.where(visible, VISIBLE, 0) | (s["j"] << JSHIFT)
                    k[level] = s["k"]
                    traced[level] = s["trace"]
                    pend[idx[level]] = True
                    pend_P[idx[level]], pend_prim[idx[level]] = P[level], prim[level]
                folds.append((idx, emitted, brdf, cos, k, aux, specular))
                rec = np.zeros(m, LEVEL_DTYPE)
                rec["pixel"], rec["frame"], rec["depth"], rec["prim"], rec["aux"] = idx, self.frame, depth, prim, aux
                rec["inner"], rec["specular"], rec["kind"], rec["traced"], rec["asked"] = inner, specular, kind, traced, asked
                rec["on_light"] = np.isin(prim, self.light_prims)
                rec["inherit"] = inherit[idx] if depth == 0 else False
                records.append(rec)
                ray_o[idx], ray_d[idx] = P, scat
                alive = idx
            # what is still alive stands for the background
            L =np.tile(self.background, (n, 1))
            for idx, emitted, brdf, cos, k, aux, specular in reversed(folds):
                L[idx] = self._fold(emitted, brdf, cos, k, aux, specular, L[idx])
        if records:
            self.levels = np.concatenate([self.levels] + records)
        return L, ended

    def _fold(self, emitted, brdf, cos, k, aux, specular, L):
        e = np.where(((aux & DROP) != 0)[:, None], np.float32(0), emitted)
        level = (aux & LEVEL) != 0
        visible = level & ((aux & VISIBLE) != 0)
        le = self.light_emitted[np.where(visible, aux >> JSHIFT, 0)] if len(self.light_emitted) else np.zeros_like(e)
        direct = np.where(visible[:, None], k[:, None] * (brdf * le), np.float32(0))
        e = np.where(level[:, None], e + direct, e)
        out = _f32(e + (brdf * L) * cos[:, None])
        # the same level through nee_ref.fold: row i of a hit table made of these levels
        m = len(out)
        hit = np.zeros((m, 16), np.float32)
        hit[:, 4:7], hit[:, 12:15] = emitted, brdf
        c0 = np.where(specular, ~np.arange(m), np.arange(m))
        want = R.fold(c0, np.where(specular, brdf[:, 0], k), cos, aux, hit, self.light_emitted, L)
        assert same_bits(out, want)
        return out

    # -- results ---------------------------------------------------------------------------
    def frame_sum(self):
        return self.accum.reshape(self.rows, self.width, 3).copy()

    def rng_state(self):
        return np.ascontiguousarray(self.rng.T).reshape(6, self.rows, self.width)

    def level_tuples(self):
        """per level (pixel, frame, depth, prim, aux)"""
        return self.levels[["pixel", "frame", "depth", "prim", "aux"]]
