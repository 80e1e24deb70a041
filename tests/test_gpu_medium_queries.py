"""pg_transmittance_at / pg_intersect_tr_at / pg_medium_sample_at: VisibilityTester::Tr (light.cpp:63-81), Scene::IntersectTr (scene.cpp:57-70) and
Medium::Sample (homogeneous.cpp:49-74, grid.cpp:61-86) for batches of rays (PgTransmittance, PgMediumSample, csrc/pg_mediumquery.h).

The reference is a Python restatement of the two loops over the oracle's entry points: oracle_intersect gives each pass's primitive, oracle_intersect_interaction
its t, p, pError and n, oracle_spawn_ray_origin the re-spawned origin, oracle_grid_tr / oracle_grid_sample the tracking loops on the same stream of draws (they
report how many they used), and a homogeneous segment's exponentials come from glibc in float32.  The media, the primitives' interfaces and materials are read
from HostScene.desc.  Every field of every record is compared bit for bit.  Under motion the same loop takes each pass's hit from GpuScene.intersect_at, which
pins the re-spawned rays and their times.  tests/test_emulated_medium_queries.py runs this file without a GPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
F32 = np.float32


def _load(filename):
    spec = importlib.util.spec_from_file_location(filename[:-3] + "_helpers", os.path.join(os.path.dirname(__file__), filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GS = _load("test_gpu_scatter.py")
_GI = _GS._GI
_MH = _load("test_medium_headers_on_host.py")
records_equal, first_difference, struct_array, ray_set = _GS.records_equal, _GS.first_difference, _GS.struct_array, _GS.ray_set
DeviceArrays, same_bits, bits = _GS.DeviceArrays, _GS.same_bits, _GS.bits
restate_distance, restate_weight, expf = _MH.restate_distance, _MH.restate_weight, _MH.expf

PG_MAT_NONE = 0
MAX_FLOAT = np.finfo(F32).max
SHADOW_TMAX = F32(1) - F32(0.0001)  # 1 - ShadowEpsilon
N_U = 48  # draws per ray handed to the grid scenes: the restatement's `used` stays below it for every ray (asserted)


def spawn(oracle, p, perr, n, w):
    """OffsetRayOrigin (geometry.h:1440-1454): the oracle's entry."""
    a = [np.ascontiguousarray(x, F32) for x in (p, perr, n, w)]
    out = np.zeros(3, F32)
    oracle.lib().oracle_spawn_ray_origin(*[x.ctypes.data for x in a], out.ctypes.data)
    return out


class Scene:
    """One scene on the device, the tables of its description the walks read, and its rays with a start medium each."""

    def __init__(self, gpu, name, seed):
        self.gpu, self.name = gpu, name
        self.host = gpu.HostScene(os.path.join(ROOT, "scenes", "cornell.pbrt") if name == "cornell" else os.path.join(GOLD, name + ".pbrt"))
        d = self.desc = self.host.desc
        self.gs = gpu.GpuScene(d)
        self.nm = d.n_media
        self.media = struct_array(d.media, self.nm, gpu.abi.PgMedium)
        self.media_grid = np.ctypeslib.as_array(d.media_grid, (self.nm,)) if d.n_grids > 0 else np.full(self.nm, -1, np.int32)
        self.grids = (gpu.abi.PgDensityGrid * d.n_grids).from_address(C.addressof(d.grids.contents)) if d.n_grids > 0 else []
        self.density = np.ctypeslib.as_array(d.grid_density, (d.n_density_floats,)) if d.n_grids > 0 else None
        self.mat_type = struct_array(d.materials, d.n_materials, gpu.abi.PgMaterial)["type"]
        self.tri_material = np.ctypeslib.as_array(d.tri_material, (d.n_prims_all,))
        self.m_in = np.ctypeslib.as_array(d.tri_medium_inside, (d.n_prims_all,)) if d.tri_medium_inside else None
        self.m_out = np.ctypeslib.as_array(d.tri_medium_outside, (d.n_prims_all,)) if d.tri_medium_outside else None
        o, dd, tmax, _, _ = ray_set(self.host, seed)
        eo, ed = self.boundary_rays(seed)
        k = len(eo) - (1 if (len(tmax) + len(eo)) % 256 == 0 else 0)
        self.o, self.d = np.ascontiguousarray(np.concatenate([o, eo[:k]]), F32), np.ascontiguousarray(np.concatenate([dd, ed[:k]]), F32)
        self.tmax = np.concatenate([tmax, np.full(k, np.inf, F32)])
        n = self.n = len(self.tmax)
        assert n % 256 != 0 and 1500 < n < 2600
        rng = np.random.default_rng(seed + 31)
        self.medium = (np.arange(n) % (self.nm + 2) - 1).astype(np.int32)  # -1, every medium, n_media (invalid), and again
        self.time = np.zeros(n, F32)
        self.u = np.minimum(rng.random((n, N_U)).astype(F32), _GS.ONE_MINUS_EPS)
        # the rays of the Tr query: SpawnRayTo's form -- d = p1 - o, tMax = 1 - ShadowEpsilon; lengths from a tenth of the scene to beyond it, the aimed
        # rays three times as far as the boundary triangle they were aimed at
        lo, hi = self.host.nodes()["bmin"][0], self.host.nodes()["bmax"][0]
        diag = np.sqrt(((hi - lo) ** 2).sum(), dtype=F32)
        length = np.sqrt((self.d.astype(np.float64) ** 2).sum(1))
        scale = np.where(np.arange(n) < len(tmax), diag * rng.uniform(0.1, 1.2, n) / np.maximum(length, 1e-30), 1.0)
        self.d_tr = np.ascontiguousarray(self.d * scale[:, None].astype(F32), F32)
        self.p1 = (self.o + self.d_tr).astype(F32)
        self.tmax_tr = np.full(n, SHADOW_TMAX, F32)

    def boundary_rays(self, seed, n_aimed=400):
        """Rays from inside the bounds through the centroids of top-level triangles without a material (medium boundaries), three times as long as the way there."""
        rng = np.random.default_rng(seed + 17)
        d = self.desc
        flags = np.ctypeslib.as_array(d.tri_flags, (d.n_prims_all,))[: d.n_tris]
        none = np.flatnonzero(((flags & (32 | 64)) == 0) & (self.mat_type[np.maximum(self.tri_material[: d.n_tris], 0)] == PG_MAT_NONE) & (self.tri_material[: d.n_tris] >= 0))
        if len(none) == 0: return np.zeros((0, 3), F32), np.zeros((0, 3), F32)
        tris = none[rng.integers(0, len(none), n_aimed)]
        idx = np.ctypeslib.as_array(d.indices, (d.n_prims_all, 3))[tris]
        P = np.ctypeslib.as_array(d.P, (d.n_verts, 3))
        b = rng.dirichlet((1, 1, 1), n_aimed).astype(F32)
        c = P[idx[:, 0]] * b[:, 0:1] + P[idx[:, 1]] * b[:, 1:2] + P[idx[:, 2]] * b[:, 2:3]
        lo, hi = self.host.nodes()["bmin"][0], self.host.nodes()["bmax"][0]
        o = (lo + (hi - lo) * (0.05 + 0.9 * rng.random((n_aimed, 3)))).astype(F32)
        return o, ((c - o) * F32(3)).astype(F32)

    def close(self):
        self.gs.close()
        self.host.close()

    # ---- each pass's closest hits: prim, t, p, pError, n
    def trace_oracle(self, oracle):
        def trace(o, d, tmax, time):
            o, d, tmax = (np.ascontiguousarray(a, F32) for a in (o, d, tmax))
            prim, t, _, _ = oracle.intersect(self.desc, o, d, tmax)
            hit, t2, out = _GI.oracle_interactions(oracle, self.desc, o, d, tmax)
            assert np.array_equal(hit, prim >= 0) and same_bits(t[hit], t2[hit])
            return prim, t, out[:, 0:3], out[:, 3:6], out[:, 6:9]
        return trace

    def trace_device(self):
        def trace(o, d, tmax, time):
            r = self.gs.intersect_at(o, d, tmax, time)
            return r["prim"], r["t"], r["p"], r["p_error"], r["n"]
        return trace


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------
def segment_tr(sc, oracle, med, o, d, t_seg, stream):
    """ray.medium->Tr(ray, sampler) over [0, t_seg] as three factors, and the draws it made (stream: the ray's numbers not yet consumed)."""
    if sc.media_grid[med] >= 0:  # GridDensityMedium::Tr, grid.cpp:88-120: the oracle's loop on the same numbers
        g = sc.grids[sc.media_grid[med]]
        den = sc.density[int(g.density_offset):]
        used = C.c_int(0)
        o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
        tr = oracle.lib().oracle_grid_tr(C.addressof(g), den.ctypes.data, o.ctypes.data, d.ctypes.data, float(t_seg), stream.ctypes.data if len(stream) else None, len(stream),
                                         C.byref(used))
        return np.full(3, F32(tr), F32), used.value
    with np.errstate(all="ignore"):  # HomogeneousMedium::Tr, homogeneous.cpp:44-47
        d_len = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        x = min(F32(t_seg * d_len), MAX_FLOAT)
        return np.array([expf(F32(-sc.media["sigma_t"][med][c]) * x) for c in range(3)], F32), 0


def walk(sc, oracle, trace, o, d, tmax, time, medium, u, p1=None):
    """VisibilityTester::Tr (p1 given) or Scene::IntersectTr for every ray: (records, the final segment's ray per ray as (o, d, tmax), passes, segments)."""
    n = len(tmax)
    n_u = 0 if u is None else u.shape[1]
    rec = np.zeros(n, sc.gpu.TRANSMITTANCE_DTYPE)
    valid = (medium >= -1) & (medium < sc.nm)
    rec["status"][~valid] = -1
    Tr = np.ones((n, 3), F32)
    med, cross, used = medium.copy(), np.zeros(n, np.int32), np.zeros(n, np.int32)
    co, cd, ct = o.copy(), d.copy(), tmax.copy()
    active = np.flatnonzero(valid)
    passes = segments = 0
    while len(active):
        passes += 1; segments += len(active)
        assert passes < 64
        prim, t, p, perr, nrm = trace(co[active], cd[active], ct[active], time[active])
        go_on = []
        for k, i in enumerate(active):
            surface = prim[k] >= 0
            opaque = surface and sc.mat_type[sc.tri_material[prim[k]]] != PG_MAT_NONE
            if p1 is not None and opaque: Tr[i] = 0  # light.cpp:70-72: blocked, and this segment draws nothing
            elif med[i] >= 0:
                stream = u[i, min(used[i], n_u):] if n_u else np.zeros(0, F32)
                f, k_used = segment_tr(sc, oracle, med[i], co[i], cd[i], t[k] if surface else ct[i], stream)
                Tr[i] = Tr[i] * f
                used[i] += k_used
            if surface and not opaque:  # step over a surface without a material
                m_in = sc.m_in[prim[k]] if sc.m_in is not None else -1
                m_out = sc.m_out[prim[k]] if sc.m_out is not None else -1
                if m_in == m_out: m_in = m_out = med[i]  # primitive.cpp:121-125: no transition, the ray's medium on both sides
                if p1 is not None:  # isect.SpawnRayTo(p1), interaction.h:69-72
                    origin = spawn(oracle, p[k], perr[k], nrm[k], p1[i] - p[k])
                    nd, nt = (p1[i] - origin).astype(F32), SHADOW_TMAX
                else:  # isect.SpawnRay(ray.d), interaction.h:64-67
                    origin = spawn(oracle, p[k], perr[k], nrm[k], cd[i])
                    nd, nt = cd[i].copy(), F32(np.inf)
                with np.errstate(all="ignore"):
                    outside = (nd[0] * nrm[k][0] + nd[1] * nrm[k][1]) + nd[2] * nrm[k][2] > 0
                med[i] = m_out if outside else m_in
                co[i], cd[i], ct[i] = origin, nd, nt
                cross[i] += 1
                go_on.append(i)
            else:
                rec["status"][i] = 1 if opaque else 0
        active = np.array(go_on, np.int64)
    v = valid
    rec["Tr"][v], rec["medium"][v], rec["crossings"][v], rec["draws_used"][v] = Tr[v], med[v], cross[v], used[v]
    return rec, (co, cd, ct), passes, segments


def expected_isect(sc, final, time, valid):
    """The interaction IntersectTr leaves: pg_intersect_at's record of the walk's last segment; prim -1 and zeros for a ray that was not walked."""
    co, cd, ct = final
    want = sc.gs.intersect_at(co, cd, ct, time)
    blank = np.zeros(1, sc.gpu.INTERACTION_DTYPE)
    blank["prim"] = -1
    want[~valid] = blank[0]
    return want


def restate_medium_sample(sc, oracle, o, d, tmax, medium, u):
    n, n_u = len(tmax), u.shape[1]
    rec = np.zeros(n, sc.gpu.MEDIUM_SAMPLE_DTYPE)
    rec["sampled"] = -1
    draw = lambda i, k: u[i, k] if k < n_u else F32(0.5)
    for i in np.flatnonzero((medium >= 0) & (medium < sc.nm)):
        m = sc.media[medium[i]]
        r = rec[i:i + 1]
        with np.errstate(all="ignore"):
            if sc.media_grid[medium[i]] >= 0:  # GridDensityMedium::Sample: the oracle's delta tracking on the same numbers
                g = sc.grids[sc.media_grid[medium[i]]]
                den = sc.density[int(g.density_offset):]
                used, tt = C.c_int(0), C.c_float(0)
                oi, di = np.ascontiguousarray(o[i]), np.ascontiguousarray(d[i])
                sampled = oracle.lib().oracle_grid_sample(C.addressof(g), den.ctypes.data, oi.ctypes.data, di.ctypes.data, float(tmax[i]), u[i].ctypes.data, n_u,
                                                          C.byref(used), C.byref(tt)) != 0
                t = F32(tt.value) if sampled else tmax[i]
                beta = m["sigma_s"] / F32(g.sigma_t) if sampled else np.ones(3, F32)
                r["draws_used"] = used.value
            else:  # HomogeneousMedium::Sample: always two draws
                _, dist = restate_distance(m["sigma_t"], draw(i, 0), draw(i, 1))
                d_len = np.sqrt((d[i, 0] * d[i, 0] + d[i, 1] * d[i, 1]) + d[i, 2] * d[i, 2])
                beta, t, sampled = restate_weight(m["sigma_s"], m["sigma_t"], dist, d_len, tmax[i])
                r["draws_used"] = 2
            r["sampled"], r["beta"], r["t"], r["wo"], r["g"], r["medium"] = int(sampled), beta, t, -d[i], m["g"], medium[i]
            if sampled: r["p"] = o[i] + d[i] * t
    return rec


# ---- the cases: computed once per scene, shared by the tests ---------------------------------------------------------------------------------------------
HOMOGENEOUS = ["vol_path_none", "vol_smoke", "vol_fog_halfspace", "vol_instances", "directlighting/j_null_boundaries"]
GRIDS = ["grid_puff", "grid_fog_camera", "grid_transformed"]
MOTION = ["motion_vol", "nest_motion_vol", "grid_puff_motion"]
SEEDS = {name: 901 + k for k, name in enumerate(HOMOGENEOUS + GRIDS + MOTION + ["cornell"])}


@pytest.fixture(scope="module")
def case(gpu, oracle):
    """name -> the scene, the device's records of both walks and the restatement's."""
    cache = {}

    def get(name):
        if name in cache: return cache[name]
        sc = Scene(gpu, name, SEEDS[name])
        moving = name in MOTION
        if moving: sc.time = np.random.default_rng(SEEDS[name] + 5).random(sc.n).astype(F32)
        u = sc.u if sc.desc.n_grids > 0 else None
        trace = sc.trace_device() if moving else sc.trace_oracle(oracle)
        c = dict(sc=sc, u=u)
        c["tr"] = sc.gs.transmittance_at(sc.o, sc.d_tr, sc.tmax_tr, sc.p1, sc.medium, u, sc.time)
        c["itr"], c["isect"] = sc.gs.intersect_tr_at(sc.o, sc.d, sc.tmax, sc.medium, u, sc.time, with_interaction=True)
        c["want_tr"], _, c["tr_passes"], c["tr_segments"] = walk(sc, oracle, trace, sc.o, sc.d_tr, sc.tmax_tr, sc.time, sc.medium, u, sc.p1)
        c["want_itr"], c["final"], c["itr_passes"], c["itr_segments"] = walk(sc, oracle, trace, sc.o, sc.d, sc.tmax, sc.time, sc.medium, u)
        cache[name] = c
        return c
    yield get
    for c in cache.values(): c["sc"].close()


def check_walks(c, name):
    sc = c["sc"]
    valid = (sc.medium >= -1) & (sc.medium < sc.nm)
    assert c["tr"].dtype == c["itr"].dtype == sc.gpu.TRANSMITTANCE_DTYPE and c["isect"].dtype == sc.gpu.INTERACTION_DTYPE
    assert records_equal(c["tr"], c["want_tr"]), (name, "Tr", first_difference(c["tr"], c["want_tr"]))
    assert records_equal(c["itr"], c["want_itr"]), (name, "IntersectTr", first_difference(c["itr"], c["want_itr"]))
    want = expected_isect(sc, c["final"], sc.time, valid)
    assert records_equal(c["isect"], want), (name, "isect", first_difference(c["isect"], want))
    first = valid & (c["want_itr"]["crossings"] == 0)  # a ray that ends at its first hit: pg_intersect_at's bytes for the ray as given
    assert first.sum() >= 200 and records_equal(c["isect"][first], sc.gs.intersect_at(sc.o, sc.d, sc.tmax, sc.time)[first])
    for rec in (c["tr"], c["itr"]):
        rest = rec[~valid].copy()
        assert (rest["status"] == -1).all() and len(rest) >= 100
        rest["status"] = 0
        assert not rest.view(np.uint8).any() and not rec["reserved"].any()  # not walked: every other field 0
    blocked = c["tr"]["status"] == 1
    assert not c["tr"]["Tr"][blocked].any() and (c["itr"]["status"] == 1).sum() == (valid & (c["isect"]["prim"] >= 0)).sum()


# ---- 1. homogeneous media and surfaces without a material --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOMOGENEOUS)
def test_homogeneous_walks_equal_the_restatement(case, name):
    c = case(name)
    check_walks(c, name)
    assert not c["tr"]["draws_used"].any() and not c["itr"]["draws_used"].any()
    sc = c["sc"]
    alone = sc.gs.intersect_tr_at(sc.o, sc.d, sc.tmax, sc.medium, None, sc.time)  # isect = NULL changes no record
    assert records_equal(alone, c["itr"])


def test_the_homogeneous_ray_sets_reach_every_case(case):
    """What the rays must reach over the scenes of case 1, decided by the restatement alone."""
    tr = np.concatenate([case(name)["want_tr"] for name in HOMOGENEOUS])
    itr = np.concatenate([case(name)["want_itr"] for name in HOMOGENEOUS])
    counts = dict(tr_two=(tr["crossings"] >= 2).sum(), itr_two=(itr["crossings"] >= 2).sum(), blocked=(tr["status"] == 1).sum(),
                  reached=(tr["status"] == 0).sum(), escaped=(itr["status"] == 0).sum(), hit=(itr["status"] == 1).sum(),
                  attenuated=((tr["status"] == 0) & (tr["Tr"] < 1).all(1) & (tr["Tr"] > 0).all(1)).sum())
    assert all(v >= 32 for v in counts.values()), counts
    assert max(case(name)["tr_passes"] for name in HOMOGENEOUS) >= 3 and max(case(name)["itr_passes"] for name in HOMOGENEOUS) >= 3  # both queues reused


# ---- 2. grid media -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_grid_walks_equal_the_restatement(case, oracle, name):
    c = case(name)
    sc = c["sc"]
    assert sc.desc.n_grids > 0
    assert c["want_tr"]["draws_used"].max() <= N_U and c["want_itr"]["draws_used"].max() <= N_U  # the stream was long enough for every ray
    check_walks(c, name)
    # the same rays with one draw each: both sides draw 0.5 beyond the stream, and the records say that it ran out
    u1 = np.ascontiguousarray(sc.u[:, :1])
    trace = sc.trace_oracle(oracle)
    for got, want in ((sc.gs.transmittance_at(sc.o, sc.d_tr, sc.tmax_tr, sc.p1, sc.medium, u1, sc.time), walk(sc, oracle, trace, sc.o, sc.d_tr, sc.tmax_tr, sc.time, sc.medium, u1, sc.p1)[0]),
                      (sc.gs.intersect_tr_at(sc.o, sc.d, sc.tmax, sc.medium, u1, sc.time), walk(sc, oracle, trace, sc.o, sc.d, sc.tmax, sc.time, sc.medium, u1)[0])):
        assert records_equal(got, want), (name, first_difference(got, want))
        assert (want["draws_used"] > 1).sum() >= 32 and np.array_equal(got["draws_used"] > 1, want["draws_used"] > 1)


def test_the_grid_ray_sets_consume_draws(case):
    tr = np.concatenate([case(name)["want_tr"] for name in GRIDS])
    itr = np.concatenate([case(name)["want_itr"] for name in GRIDS])
    counts = dict(tr_three=(tr["draws_used"] >= 3).sum(), itr_three=(itr["draws_used"] >= 3).sum(),
                  drew_and_crossed=((itr["draws_used"] >= 1) & (itr["crossings"] >= 1)).sum(), partial=((itr["Tr"] > 0) & (itr["Tr"] < 1)).all(1).sum())
    assert all(v >= 32 for v in counts.values()), counts


# ---- 3. Medium::Sample -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOMOGENEOUS + GRIDS)
def test_medium_sample_equals_the_restatement(case, oracle, name):
    sc = case(name)["sc"]
    first = sc.gs.intersect_at(sc.o, sc.d, sc.tmax)
    before = sc.gs.counters()
    sampled = left = 0
    for tmax in (first["t"], np.full(sc.n, np.inf, F32)):  # the ray as Scene::Intersect left it, and an unbounded one
        got = sc.gs.medium_sample_at(sc.o, sc.d, tmax, sc.medium, sc.u)
        want = restate_medium_sample(sc, oracle, sc.o, sc.d, tmax, sc.medium, sc.u)
        assert got.dtype == sc.gpu.MEDIUM_SAMPLE_DTYPE and records_equal(got, want), (name, first_difference(got, want))
        assert want["draws_used"].max() <= N_U
        none = (sc.medium < 0) | (sc.medium >= sc.nm)
        assert np.array_equal(got["sampled"] == -1, none) and none.sum() >= 100
        rest = got[none].copy()
        rest["sampled"] = 0
        assert not rest.view(np.uint8).any()
        sampled += int((want["sampled"] == 1).sum()); left += int((want["sampled"] == 0).sum())
    two = restate_medium_sample(sc, oracle, sc.o, sc.d, first["t"], sc.medium, sc.u[:, :1])  # a stream of one draw: 0.5 beyond it
    assert records_equal(sc.gs.medium_sample_at(sc.o, sc.d, first["t"], sc.medium, np.ascontiguousarray(sc.u[:, :1])), two)
    assert sc.gs.counters() == before  # the call moves no counter
    assert sampled >= 32 and left >= 32, (name, sampled, left)


# ---- 4. motion, instances under motion, nesting: by composition with pg_intersect_at ------------------------------------------------------------------------
@pytest.mark.parametrize("name", MOTION)
def test_walks_under_motion_compose_with_intersect_at(case, name):
    c = case(name)
    check_walks(c, name)
    sc = c["sc"]
    if (sc.mat_type == PG_MAT_NONE).any():  # (the two fog scenes have no surface without a material: their walks are one segment at the ray's time)
        assert (c["want_tr"]["crossings"] >= 1).sum() >= 32 and (c["want_itr"]["crossings"] >= 1).sum() >= 32, name
    else: assert name != "grid_puff_motion" and ((c["want_itr"]["Tr"] < 1).all(1) & (c["want_itr"]["Tr"] > 0).all(1)).sum() >= 100
    at0 = sc.gs.intersect_tr_at(sc.o, sc.d, sc.tmax, sc.medium, c["u"], np.zeros(sc.n, F32))
    assert not records_equal(at0, c["itr"]), name  # the case cannot pass with the times ignored


# ---- 5. no media ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_scene_without_media_is_intersect_p(case):
    c = case("cornell")
    sc = c["sc"]
    assert sc.nm == 0 and (sc.mat_type != PG_MAT_NONE).all()
    valid = sc.medium == -1
    occ = sc.gs.intersect_p_at(sc.o, sc.d_tr, sc.tmax_tr, sc.time)
    tr = c["tr"]
    assert np.array_equal(tr["status"][valid], occ[valid].astype(np.int32)) and (tr["status"][~valid] == -1).all()
    assert (occ[valid] == 1).sum() >= 100 and (occ[valid] == 0).sum() >= 100
    clear = valid & (occ == 0)
    assert (tr["Tr"][clear] == 1).all() and not tr["Tr"][~clear].any() and not tr["crossings"].any() and not tr["draws_used"].any()
    check_walks(c, "cornell")


# ---- 6. device memory ----------------------------------------------------------------------------------------------------------------------------------------
PAD = 256  # bytes the device arrays are longer than the results: guard bytes, to catch a write past them


@pytest.mark.parametrize("name", ["vol_instances", "grid_puff_motion"])
def test_device_memory_equals_host_memory(case, name):
    c = case(name)
    sc = c["sc"]
    n, n_u = sc.n, N_U
    first_t = sc.gs.intersect_at(sc.o, sc.d, sc.tmax, sc.time)["t"]
    host_sample = sc.gs.medium_sample_at(sc.o, sc.d, first_t, sc.medium, sc.u, sc.time)
    u = sc.u  # (a scene without grids reads none of it)
    host_tr = sc.gs.transmittance_at(sc.o, sc.d_tr, sc.tmax_tr, sc.p1, sc.medium, u, sc.time)
    host_itr, host_isect = sc.gs.intersect_tr_at(sc.o, sc.d, sc.tmax, sc.medium, u, sc.time, with_interaction=True)
    assert records_equal(host_tr, c["tr"]) and records_equal(host_itr, c["itr"]) and records_equal(host_isect, c["isect"])  # (draws nobody reads change nothing)
    guard = lambda nbytes: np.full(nbytes + PAD, 0xAB, np.uint8)

    def check(dev, i, want):
        got = dev.get(i, np.uint8)
        w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert len(got) == len(w) + PAD and np.array_equal(got[:len(w)], w) and (got[len(w):] == 0xAB).all(), (name, i)
    dev = DeviceArrays()
    inputs = (sc.o, sc.d, sc.tmax, sc.time, sc.d_tr, sc.tmax_tr, sc.p1, sc.medium, u, first_t)
    po, pd, pt, ptime, pdtr, pttr, pp1, pmed, pu, pft = (dev.put(a) for a in inputs)  # 0 .. 9
    for rnd in range(2):  # the second, identical call finds the scene's scratch as the first left it
        ptr_out, pitr_out, pisect, psample = dev.put(guard(32 * n)), dev.put(guard(32 * n)), dev.put(guard(128 * n)), dev.put(guard(64 * n))
        base = 10 + 4 * rnd
        sc.gs.transmittance_at_device(n, po, pdtr, pttr, ptime, pp1, pmed, pu, n_u, ptr_out)
        check(dev, base, host_tr)
        sc.gs.intersect_tr_at_device(n, po, pd, pt, ptime, pmed, pu, n_u, pitr_out, pisect)
        check(dev, base + 1, host_itr); check(dev, base + 2, host_isect); check(dev, base, host_tr)
        sc.gs.medium_sample_at_device(n, po, pd, pft, ptime, pmed, pu, n_u, psample)
        check(dev, base + 3, host_sample)
    alone = dev.put(guard(32 * n))  # 18
    sc.gs.intersect_tr_at_device(n, po, pd, pt, ptime, pmed, pu, n_u, alone, None)  # isect = NULL
    check(dev, 18, host_itr)
    for i, a in enumerate(inputs):  # the inputs were only read
        assert np.array_equal(dev.get(i, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1))


# ---- 7. counters ---------------------------------------------------------------------------------------------------------------------------------------------
SHADING = ("camera_rays", "mis_rays", "shade_launches", "resolve_launches", "shade_items", "shadow_rays", "shadow_launches", "light_tri_tests")


@pytest.mark.parametrize("name", ["vol_path_none", "grid_puff"])
def test_counters_count_segments_and_passes(case, gpu, name):
    c = case(name)
    sc, gs = c["sc"], c["sc"].gs
    valid = (sc.medium >= -1) & (sc.medium < sc.nm)
    for want, passes, segments, call in ((c["want_tr"], c["tr_passes"], c["tr_segments"], lambda: gs.transmittance_at(sc.o, sc.d_tr, sc.tmax_tr, sc.p1, sc.medium, c["u"], sc.time)),
                                         (c["want_itr"], c["itr_passes"], c["itr_segments"], lambda: gs.intersect_tr_at(sc.o, sc.d, sc.tmax, sc.medium, c["u"], sc.time))):
        gs.counters_reset()
        call()
        cn = gs.counters()
        assert cn["closest_rays"] == valid.sum() + want["crossings"][valid].sum() == segments
        assert cn["closest_launches"] == 1 + want["crossings"][valid].max() == passes >= 3
        assert cn["closest_node_visits"] > 0 and all(cn[k] == 0 for k in SHADING)
    # a batch without a valid medium index: nothing is traced
    gs.counters_reset()
    bad = np.full(sc.n, sc.nm, np.int32)
    rec, isect = gs.intersect_tr_at(sc.o, sc.d, sc.tmax, bad, c["u"], sc.time, with_interaction=True)
    assert (rec["status"] == -1).all() and (isect["prim"] == -1).all()
    cn = gs.counters()
    assert cn["closest_rays"] == 0 and cn["closest_launches"] == 0 and cn["closest_node_visits"] == 0
    # empty batches and mismatched lengths
    assert len(gs.transmittance_at(sc.o[:0], sc.d[:0], sc.tmax[:0], sc.p1[:0], sc.medium[:0])) == 0 and len(gs.intersect_tr_at(sc.o[:0], sc.d[:0], sc.tmax[:0], sc.medium[:0])) == 0
    assert gs.medium_sample_at(sc.o[:0], sc.d[:0], sc.tmax[:0], sc.medium[:0], sc.u[:0]).dtype == gpu.MEDIUM_SAMPLE_DTYPE and gs.counters() == cn
    for call, args in ((gs.transmittance_at, (sc.o, sc.d, sc.tmax, sc.p1[:-1], sc.medium)), (gs.transmittance_at, (sc.o, sc.d, sc.tmax, sc.p1, sc.medium[:-1])),
                       (gs.intersect_tr_at, (sc.o, sc.d[:-1], sc.tmax, sc.medium)), (gs.medium_sample_at, (sc.o, sc.d, sc.tmax, sc.medium, sc.u.reshape(-1)[:-1]))):
        with pytest.raises(ValueError):
            call(*args)
    # prefixes of one batch: a record does not depend on its neighbours
    for k in (1, 63, 257):
        assert records_equal(gs.intersect_tr_at(sc.o[:k], sc.d[:k], sc.tmax[:k], sc.medium[:k], None if c["u"] is None else c["u"][:k], sc.time[:k]), c["itr"][:k]), k
