"""pg_scatter_f_mode_at / pg_scatter_sample_mode_at: the scattering queries under a TransportMode (k_scatter_importance, csrc/pg_cameraimportance.h).

Mode 0 (Radiance) must be the existing plain and _diff_ calls byte for byte.  Mode 1 (Importance) may differ from mode 0 in `f` alone, and only through a
transmissive BxDF: FresnelSpecular's transmission branch is pinned to a float32 NumPy restatement of reflection.cpp:487-521 under both modes, bit for bit, and
for every transmissive fixture f(Radiance) = f(Importance) x the mode's factor within a bound derived from the roundings in which the two expressions differ.
Batches of 1, 64, 65 and 600 rays run in host and in device memory with guard bytes around every output.  tests/test_emulated_scatter_importance.py runs this
file without a GPU."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24  # the relative error of one correctly rounded float32 operation
R, T, DIFFUSE, GLOSSY, SPECULAR, ALL = 1, 2, 4, 8, 16, 31
SPEC_T, FRESNEL_SPEC, MICRO_T = 5, 6, 8  # PgBxDFType
SIZES = (1, 64, 65, 600)
N = max(SIZES)
ONE_MINUS_EPS = np.nextafter(F32(1), F32(0))


def _load(filename):
    spec = importlib.util.spec_from_file_location(filename[:-3] + "_helpers", os.path.join(os.path.dirname(__file__), filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GS, _CI = _load("test_gpu_scatter.py"), _load("test_gpu_camera_importance.py")
records_equal, ray_set, Bsdfs, bits, same_bits, first_difference = _GS.records_equal, _GS.ray_set, _GS.Bsdfs, _GS.bits, _GS.same_bits, _GS.first_difference
guarded_call = _CI.guarded_call


class Case:
    """One scene on the device with N rays -- the aimed end of tests/test_gpu_scatter.py's ray set, so that most hit and every material is met from both sides --
    an unnormalised wi and a Point2f per ray, and the rays' interactions."""

    def __init__(self, gpu, name, seed):
        self.gpu, self.name = gpu, name
        self.host = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
        self.gs = gpu.GpuScene(self.host.desc)
        o, d, tmax, wi, u = ray_set(self.host, seed)
        self.o, self.d, self.tmax, self.wi, self.u = (np.ascontiguousarray(a[-N:]) for a in (o, d, tmax, wi, u))
        self.isect = self.gs.intersect_at(self.o, self.d, self.tmax)
        assert len(self.tmax) == N and (self.isect["prim"] >= 0).sum() > N // 2

    def query(self, sample, flags, mode, diff=None, n=N, mem=None, rays=None):
        o, d, tmax = rays if rays is not None else (self.o, self.d, self.tmax)
        extra = self.u if sample else self.wi
        if mem is None:
            call = self.gs.scatter_sample_at if sample else self.gs.scatter_f_at
            return call(o[:n], d[:n], tmax[:n], extra[:n], flags=flags, diff=None if diff is None else diff[:n], mode=mode)
        name = "pg_scatter_sample_mode_at" if sample else "pg_scatter_f_mode_at"
        args = [self.gs._h, n, o[:n], d[:n], tmax[:n], None, extra[:n], None if diff is None else diff[:n], int(flags), int(mode), None, (self.gpu.SCATTER_DTYPE, n)]
        return guarded_call(self.gpu, name, args, mem)[0]

    def close(self):
        self.gs.close()
        self.host.close()


ALL_SCENES = ["cornell_32", "cornell_plastic", "mat_metal", "cornell_glass_eta", "cornell_mirror_glass", "mat_uber", "mat_roughglass", "mat_translucent",
              "vol_path_none_glass", "bump_maps"]


@pytest.fixture(scope="module")
def cases(gpu):
    made = {}

    def case(name):
        if name not in made: made[name] = Case(gpu, name, 1200 + ALL_SCENES.index(name))
        return made[name]
    yield case
    for sc in made.values(): sc.close()


# ---- 1. mode 0 = the existing plain and _diff_ calls, byte for byte ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def camera_case(gpu, cases):
    """Per scene: N camera rays with the differentials pg_camera_rays_at reports, and the existing calls' records for them (with and without differentials)."""
    made = {}

    def case(name):
        if name not in made:
            sc = cases(name)
            rd = sc.host.render_desc()
            w, h = sc.host.film_size
            rng = np.random.default_rng(5)
            cam = sc.gs.camera_rays(rd, (rng.random((N, 2)) * [w, h]).astype(F32), rng.random((N, 2)).astype(F32), rng.random(N).astype(F32))
            rays = tuple(np.ascontiguousarray(cam[f]) for f in ("o", "d", "t_max"))
            diff = np.ascontiguousarray(cam["differentials"])
            assert diff.any()
            base = {(s, with_diff): sc.query(s, ALL, None, diff if with_diff else None, rays=rays) for s in (False, True) for with_diff in (False, True)}
            made[name] = (sc, rays, diff, base)
        return made[name]
    return case


@pytest.mark.parametrize("device_memory", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["cornell_32", "cornell_glass_eta", "mat_uber", "bump_maps"])  # the constant and the textured scenes of the issue
def test_mode_zero_is_the_existing_calls(gpu, camera_case, name, n, device_memory):
    sc, rays, diff, base = camera_case(name)
    mem = gpu.PG_MEM_DEVICE if device_memory else gpu.PG_MEM_HOST
    for sample in (False, True):
        for with_diff in (False, True):
            got = sc.query(sample, ALL, 0, diff if with_diff else None, n=n, mem=mem, rays=rays)
            assert records_equal(got, base[(sample, with_diff)][:n]), (name, n, sample, with_diff, first_difference(got, base[(sample, with_diff)][:n]))
    if name == "bump_maps" and n == N:  # (the differentials are read there: the case cannot pass by ignoring them)
        assert not records_equal(base[(False, True)], base[(False, False)])


# ---- 2. mode 1 = mode 0 wherever no transmissive BxDF contributes; everywhere in every field but f -------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SCENES)
def test_importance_changes_f_alone_and_only_through_transmission(cases, name):
    sc = cases(name)
    no_transmission = name in ("cornell_32", "cornell_plastic", "mat_metal", "bump_maps")
    for flags in (ALL, ALL & ~SPECULAR, ALL & ~T, R | SPECULAR, SPECULAR | T, GLOSSY | T, R | T | SPECULAR):
        for sample in (False, True):
            rad, imp = sc.query(sample, flags, 0), sc.query(sample, flags, 1)
            same_f = (bits(rad["f"]) == bits(imp["f"])).all(1)
            imp_f = imp.copy()
            imp_f["f"] = rad["f"]
            assert records_equal(imp_f, rad), (name, flags, sample, first_difference(imp_f, rad))  # all fields except f
            if no_transmission or not flags & T: assert same_f.all(), (name, flags, sample)
            if sample: assert same_f[(rad["sampled_type"] & T) == 0].all(), (name, flags)
            else: assert (rad["sampled_type"] == 0).all()


@pytest.mark.parametrize("device_memory", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["cornell_glass_eta", "mat_roughglass", "bump_maps"])  # k_scatter_importance<false, .> and, for bump_maps, <true, .>
def test_importance_batches_in_both_memories(gpu, cases, name, n, device_memory):
    sc = cases(name)
    mem = gpu.PG_MEM_DEVICE if device_memory else gpu.PG_MEM_HOST
    for sample in (False, True):
        whole = sc.query(sample, ALL, 1)
        got = sc.query(sample, ALL, 1, n=n, mem=mem)
        assert records_equal(got, whole[:n]), (name, n, sample, first_difference(got, whole[:n]))


@pytest.mark.parametrize("name", ["bump_maps", "mat_uber"])
def test_importance_with_differentials_is_the_diff_call_but_for_f(gpu, camera_case, name):
    """Mode 1 with the camera rays' differentials (k_scatter_importance<true, .> reading them by ray, for bump_maps) against pg_scatter_*_diff_at: every field
    but f, and on bump_maps -- nothing transmits there -- f too.  A mixed batch (every other ray's differentials zeroed) is per ray the one or the other."""
    sc, rays, diff, base = camera_case(name)
    mixed = diff.copy()
    mixed[1::2] = 0
    odd = np.arange(N) % 2 == 1
    for sample in (False, True):
        want, plain = base[(sample, True)], base[(sample, False)]
        for n, mem in ((N, None), (65, gpu.PG_MEM_HOST), (65, gpu.PG_MEM_DEVICE)):
            got = sc.query(sample, ALL, 1, diff, n=n, mem=mem, rays=rays)
            if name != "bump_maps": got["f"] = want["f"][:n]
            assert records_equal(got, want[:n]), (name, sample, n, first_difference(got, want[:n]))
        got = sc.query(sample, ALL, 1, mixed, rays=rays)
        want_mixed = np.where(odd, plain, want)
        if name != "bump_maps": got["f"] = want_mixed["f"]
        assert records_equal(got, want_mixed), (name, sample, "mixed", first_difference(got, want_mixed))
    if name == "bump_maps":  # (the differentials are read: with them the records are not the plain ones)
        assert not records_equal(base[(False, True)], base[(False, False)]) and not records_equal(base[(True, True)], base[(True, False)])


# ---- 3. FresnelSpecular, both sides of the surface, against the restatement ---------------------------------------------------------------------------------------
def fr_dielectric(cos_i, eta_i, eta_t):  # reflection.cpp:47-68
    cos_i = np.clip(cos_i, F32(-1), F32(1))
    entering = cos_i > 0
    eta_i, eta_t = np.where(entering, eta_i, eta_t), np.where(entering, eta_t, eta_i)
    cos_i = np.abs(cos_i)
    sin_i = np.sqrt(np.maximum(F32(0), F32(1) - cos_i * cos_i))
    sin_t = eta_i / eta_t * sin_i
    cos_t = np.sqrt(np.maximum(F32(0), F32(1) - sin_t * sin_t))
    with np.errstate(all="ignore"):
        parl = ((eta_t * cos_i) - (eta_i * cos_t)) / ((eta_t * cos_i) + (eta_i * cos_t))
        perp = ((eta_i * cos_i) - (eta_t * cos_t)) / ((eta_i * cos_i) + (eta_t * cos_t))
    return np.where(sin_t >= 1, F32(1), (parl * parl + perp * perp) / F32(2)).astype(F32)


def restate_fresnel_specular(B, bx, u0, mode):
    """BSDF::Sample_f over one FresnelSpecular BxDF that matches the flags (reflection.cpp:714-779 around :487-521): f, pdf, wi (world) and the sampled type, for
    the rows of B (all of them on that BxDF).  The BSDF's world-to-local dot products are B.local's."""
    n = len(B.rows)
    eta_a, eta_b, Rr, Tt = bx["eta_a"], bx["eta_b"], bx["R"], bx["T"]
    wo = B.wo_l
    u = np.minimum(u0 * F32(1) - F32(0), ONE_MINUS_EPS)
    F = fr_dielectric(wo[:, 2], eta_a, eta_b)
    reflect = u < F
    entering = wo[:, 2] > 0
    eta_i, eta_t = np.where(entering, eta_a, eta_b), np.where(entering, eta_b, eta_a)
    nz = np.where(wo[:, 2] < 0, F32(-1), F32(1))  # Faceforward(Normal3f(0, 0, 1), wo)
    eta = eta_i / eta_t
    cos_i = (F32(0) * wo[:, 0] + F32(0) * wo[:, 1]) + nz * wo[:, 2]  # Refract, reflection.h:97-109
    sin2_i = np.maximum(F32(0), F32(1) - cos_i * cos_i)
    sin2_t = eta * eta * sin2_i
    tir = sin2_t >= 1
    with np.errstate(all="ignore"):
        cos_t = np.sqrt(F32(1) - sin2_t)
        k = eta * cos_i - cos_t
        wt = np.stack([eta * -wo[:, 0] + k * F32(0), eta * -wo[:, 1] + k * F32(0), eta * -wo[:, 2] + k * nz], 1)
        ft = Tt * (F32(1) - F)[:, None]
        if mode == 0: ft = ft * ((eta_i * eta_i) / (eta_t * eta_t))[:, None]
        f_t = ft / np.abs(wt[:, 2])[:, None]
        wr = np.stack([-wo[:, 0], -wo[:, 1], wo[:, 2]], 1)
        f_r = (Rr * F[:, None]) / np.abs(wr[:, 2])[:, None]
    pdf = np.where(reflect, F, np.where(tir, F32(0), F32(1) - F))
    none = (wo[:, 2] == 0) | (pdf == 0)
    wi_l = np.where(reflect[:, None], wr, wt).astype(F32)
    f = np.where(none[:, None], 0, np.where(reflect[:, None], f_r, f_t)).astype(F32)
    typ = np.where(none, 0, np.where(reflect, SPECULAR | R, SPECULAR | T))
    assert f.dtype == F32 and wi_l.dtype == F32
    return f, np.where(none, 0, pdf).astype(F32), np.where(none[:, None], 0, B.world(wi_l)).astype(F32), typ


def test_fresnel_specular_transmission_equals_the_restatement(gpu, oracle, cases):
    sc = cases("cornell_glass_eta")
    # N rays at the glass: from the scene's own ray set the points on it, met again from random points of the scene (even lanes) and from one unit inside it
    B = Bsdfs(gpu, oracle, sc.host.desc, sc.isect)
    on_glass = sc.isect[B.rows[(B.nb == 1) & (B.kind[:, 0] == FRESNEL_SPEC)]]
    assert len(on_glass) >= 20
    rng = np.random.default_rng(31)
    at = on_glass[rng.integers(0, len(on_glass), N)]
    lo, hi = sc.host.nodes()["bmin"][0], sc.host.nodes()["bmax"][0]
    outside = (lo + (hi - lo) * rng.random((N, 3))).astype(F32)
    inside = (at["p"] - at["n"] * np.sign((at["n"] * at["wo"]).sum(1))[:, None]).astype(F32)  # behind the face the ray set's ray met
    even = (np.arange(N) % 2 == 0)[:, None]
    o = np.ascontiguousarray(np.where(even, outside, inside))
    d = np.ascontiguousarray(np.where(even, at["p"] - outside, rng.normal(size=(N, 3))).astype(F32))
    rays = (o, d, np.full(N, np.inf, F32))
    isect = sc.gs.intersect_at(*rays)
    B = Bsdfs(gpu, oracle, sc.host.desc, isect)
    glass = np.flatnonzero((B.nb == 1) & (B.kind[:, 0] == FRESNEL_SPEC))
    assert len(glass) >= N // 3
    rows = B.rows[glass]
    # restrict the restatement to the glass rows
    for attr in ("ns", "ng", "wo", "ss", "ts", "wo_l"): setattr(B, attr, getattr(B, attr)[glass])
    bx = B.bx[B.index[glass, 0]]
    B.rows = rows
    assert (B.wo_l[:, 2] > 0).sum() >= 40 and (B.wo_l[:, 2] < 0).sum() >= 40  # both sides of the surface
    # SPECULAR | TRANSMISSION alone does not match a FresnelSpecular (its type has REFLECTION too, reflection.h:225): no component, a black record
    for mode in (0, 1):
        none = sc.query(True, SPECULAR | T, mode, rays=rays)[rows]
        assert (none["n_matching"] == 0).all() and not none["f"].any() and not none["pdf"].any() and (none["sampled_type"] == 0).all()
    differs = 0
    for flags in (SPECULAR | T | R, ALL):
        got = {mode: sc.query(True, flags, mode, rays=rays)[rows] for mode in (0, 1)}
        for mode in (0, 1):
            f, pdf, wi, typ = restate_fresnel_specular(B, bx, sc.u[rows, 0], mode)
            g = got[mode]
            assert (g["n_matching"] == 1).all() and np.array_equal(g["sampled_type"], typ)
            assert same_bits(g["f"], f) and same_bits(g["pdf"], pdf) and same_bits(g["wi"], wi), (flags, mode)
        transmitted = got[0]["sampled_type"] == (SPECULAR | T)
        assert transmitted.sum() >= 20 and (transmitted & (B.wo_l[:, 2] > 0)).any() and (transmitted & (B.wo_l[:, 2] < 0)).any()
        differs += int(((bits(got[0]["f"]) != bits(got[1]["f"])).any(1) & transmitted & got[0]["f"].any(1)).sum())
        assert same_bits(got[0]["f"][~transmitted], got[1]["f"][~transmitted])
    assert differs >= 20


# ---- 4. the remaining transmissive materials: f(Radiance) = f(Importance) x the mode's factor ------------------------------------------------------------------
FIXTURES = {"cornell_mirror_glass": (SPECULAR | T | R, FRESNEL_SPEC), "mat_uber": (SPECULAR | T, SPEC_T), "mat_roughglass": (GLOSSY | T, MICRO_T),
            "mat_translucent": (GLOSSY | T, MICRO_T), "vol_path_none_glass": (SPECULAR | T | R, FRESNEL_SPEC)}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_radiance_is_importance_times_the_modes_factor(gpu, oracle, cases, name):
    sc = cases(name)
    flags, kind = FIXTURES[name]
    B = Bsdfs(gpu, oracle, sc.host.desc, sc.isect)
    match, count = B.matching(flags)
    differing = 0
    for sample in (False, True) if kind == MICRO_T else (True,):  # (a specular BxDF's f() is black: only Sample_f shows it)
        rad, imp = sc.query(sample, flags, 0)[B.rows], sc.query(sample, flags, 1)[B.rows]
        # the BxDF whose f the record holds: the chosen one of Sample_f (reflection.cpp:721-733), the one matching BxDF of the f query
        if sample:
            comp = np.minimum(np.floor(sc.u[B.rows, 0] * count.astype(F32)).astype(np.int64), count - 1)
            chosen = np.array([np.flatnonzero(match[i])[comp[i]] if count[i] else 0 for i in range(len(B.rows))])
        else:
            assert (count <= 1).all()
            chosen = match.argmax(1)
        bx = B.bx[B.index[np.arange(len(B.rows)), chosen]]
        on = (count > 0) & (B.kind[np.arange(len(B.rows)), chosen] == kind) & ((rad["sampled_type"] & T) != 0 if sample else True)
        entering = B.wo_l[:, 2] > 0
        if kind == MICRO_T:
            # reflection.cpp:257-273: eta = CosTheta(wo) > 0 ? etaB / etaA : etaA / etaB; factor = 1 / eta, squared inside the value.
            # Radiance rounds (x factor), (x factor), (/ denominator) and (x (1 - F) T): four operations; Importance multiplies by 1 exactly and rounds the
            # last two; the product f(Importance) x factor x factor below is formed in double, exactly.  Six roundings differ: 6 u, with the second-order terms.
            eta = np.where(entering, bx["eta_b"] / bx["eta_a"], bx["eta_a"] / bx["eta_b"]).astype(F32)
            fac = (F32(1) / eta).astype(np.float64) ** 2
            bound = 6 * U * (1 + 6 * U)
        else:
            # reflection.cpp:163-164, :514-516: ft *= (etaI etaI) / (etaT etaT), then ft / AbsCosTheta(wi).  Radiance rounds the product and the quotient,
            # Importance the quotient; formed in float32 the comparison product would round once more: two on each side, 4 u (the product below is exact).
            eta_i, eta_t = np.where(entering, bx["eta_a"], bx["eta_b"]), np.where(entering, bx["eta_b"], bx["eta_a"])
            fac = ((eta_i * eta_i) / (eta_t * eta_t)).astype(np.float64)
            bound = 4 * U * (1 + 4 * U)
        assert fac.dtype == np.float64
        fr, fi = rad["f"].astype(np.float64), imp["f"].astype(np.float64) * fac[:, None]
        usable = on[:, None] & np.isfinite(fr) & np.isfinite(fi) & (np.abs(fr) > 1e-30) & (np.abs(fi) > 1e-30)  # (float32 normals: u holds)
        err = np.abs(fr - fi)[usable] / np.abs(fr)[usable]
        print(name, "sample" if sample else "f", "records", int(usable.any(1).sum()), "largest deviation", err.max() / U if len(err) else 0, "u; bound", bound / U, "u")
        assert usable.any(1).sum() >= 10 and err.max() <= bound, (name, sample, err.max() / U)
        assert same_bits(rad["f"][~on], imp["f"][~on])  # every other record: no transmissive BxDF of this kind behind f
        zero = on[:, None] & ~usable
        assert (((rad["f"] == 0) | ~np.isfinite(rad["f"])) == ((imp["f"] == 0) | ~np.isfinite(imp["f"])))[zero].all()
        differing += int((on & rad["f"].any(1) & (bits(rad["f"]) != bits(imp["f"])).any(1)).sum())
    assert differing >= 1, name  # the property no test on the parent can satisfy
