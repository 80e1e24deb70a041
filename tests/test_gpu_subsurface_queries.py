"""pg_subsurface_sample_at / pg_subsurface_f_at / pg_subsurface_sample_f_at: BSSRDF::Sample_S (bssrdf.cpp:238-251, Sample_Sp :253-328) at the closest hits of a
batch of rays and the BSDF it installs at the exit point (PgSubsurfaceSample, csrc/pg_subsurfacequery.h).

The reference is a Python restatement of Sample_S / Sample_Sp around the oracle's entries: oracle_intersect + oracle_intersect_interaction give each probe step's
hit, oracle_spawn_ray_origin the origin of SpawnRayTo, oracle_bssrdf_probe_segment the segment, oracle_bssrdf_pdf_sp and oracle_bssrdf_radial the pdf and Sr.  The
frame (ss, ts, ns) at po is formed from the PgInteraction of the ray as tests/test_gpu_scatter.py forms it; the full record of pi is pg_intersect_at's of the probe
ray that found it (composition), with wo = shading_n and t = 0.  Every field of every record is compared bit for bit.  Under motion the chain's hits come from
GpuScene.intersect_at at the rays' times, and the two ends of the motion are tied to the oracle-based restatement (test_the_shutters_ends_reach_the_oracle).

Textured coefficients (bssrdf_coefficients_at<true> of the new header, a copy of k_shade's block that no golden image reaches): sss_textured_sigma_kt has
two-colour textures and no bump map, so every record and pi equals the restatement under one of two PgBSSRDF copies whose sigma_t / rho are recomputed in
float32 from the texture's two values; sss_textured_kd_bump has a bumped frame at po, which this file does not restate, so of it S alone is pinned bit for
bit (Sr needs no frame) under the two coefficient sets SubsurfaceFromDiffuse derives, status against pg_scatter_f_at's n_bxdfs, and the rest by the records'
invariants.  tests/test_emulated_subsurface_queries.py runs this file without a GPU."""
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
records_equal, first_difference, struct_array, ray_set = _GS.records_equal, _GS.first_difference, _GS.struct_array, _GS.ray_set
DeviceArrays, same_bits, bits, dot32, normalize32, cross64 = _GS.DeviceArrays, _GS.same_bits, _GS.bits, _GS.dot32, _GS.normalize32, _GS.cross64
ONE_MINUS_EPS, INV_PI = _GS.ONE_MINUS_EPS, _GS.INV_PI
SHADOW_TMAX = F32(1) - F32(0.0001)  # 1 - ShadowEpsilon
PI, PI_OVER_2, PI_OVER_4 = F32(3.14159265358979323846), F32(1.57079632679489661923), F32(0.78539816339744830961)
LIBM = C.CDLL("libm.so.6")
for _f in ("sinf", "cosf"):
    getattr(LIBM, _f).restype = C.c_float
    getattr(LIBM, _f).argtypes = [C.c_float]


def spawn(oracle, p, perr, n, w):
    a = [np.ascontiguousarray(x, F32) for x in (p, perr, n, w)]
    out = np.zeros(3, F32)
    oracle.lib().oracle_spawn_ray_origin(*[x.ctypes.data for x in a], out.ctypes.data)
    return out


class Scene:
    """One scene on the device, the tables of its description Sample_S reads, and its rays with (u1, u2.x, u2.y) each."""

    def __init__(self, gpu, name, seed, text=None):
        self.gpu, self.name = gpu, name
        if text is not None: self.host = gpu.HostScene(text=text)
        elif name.endswith("+transition"):  # the golden scene with the object's MediumInterface turned into a transition: fog inside, none outside
            text = open(os.path.join(GOLD, name[:-len("+transition")] + ".pbrt")).read()
            assert text.count('MediumInterface "fog" "fog"') == 1
            self.host = gpu.HostScene(text=text.replace('MediumInterface "fog" "fog"', 'MediumInterface "fog" ""'))
        else: self.host = gpu.HostScene(os.path.join(ROOT, "scenes", "cornell.pbrt") if name == "cornell" else os.path.join(GOLD, name + ".pbrt"))
        d = self.desc = self.host.desc
        self.gs = gpu.GpuScene(d)
        self.nb = d.n_bssrdfs
        self.bssrdfs = (gpu.abi.PgBSSRDF * self.nb).from_address(C.addressof(d.bssrdfs.contents)) if self.nb else []
        self.tables = C.addressof(d.bssrdf_tables.contents) if self.nb else 0
        self.material_bssrdf = np.ctypeslib.as_array(d.material_bssrdf, (d.n_materials,)) if self.nb else np.full(d.n_materials, -1, np.int32)
        self.tri_material = np.ctypeslib.as_array(d.tri_material, (d.n_prims_all,))
        self.m_in = np.ctypeslib.as_array(d.tri_medium_inside, (d.n_prims_all,)) if d.tri_medium_inside else None
        self.m_out = np.ctypeslib.as_array(d.tri_medium_outside, (d.n_prims_all,)) if d.tri_medium_outside else None
        o, dd, tmax, _, _ = ray_set(self.host, seed, n_random=1100, aimed=300)
        eo, ed = self.aimed_rays(seed)
        k = len(eo) - (1 if (len(tmax) + len(eo)) % 256 == 0 else 0)
        self.o, self.d = np.ascontiguousarray(np.concatenate([o, eo[:k]]), F32), np.ascontiguousarray(np.concatenate([dd, ed[:k]]), F32)
        self.tmax = np.concatenate([tmax, np.full(k, np.inf, F32)])
        n = self.n = len(self.tmax)
        assert n % 256 != 0 and 1500 <= n <= 2600, n
        rng = np.random.default_rng(seed + 31)
        self.u = np.minimum(rng.random((n, 3)).astype(F32), ONE_MINUS_EPS)
        self.time = np.zeros(n, F32)

    def aimed_rays(self, seed, n_aimed=900):
        """Rays aimed at the objects whose material carries a BSSRDF, whatever their shape: the points where ray_set's rays met such a material are the
        targets (found with intersect_at: this only chooses rays, every expectation is the restatement's); two thirds start inside the scene's bounds (outside
        the object, mostly), one third between two targets (inside a convex object)."""
        rng = np.random.default_rng(seed + 17)
        o0, d0, t0, _, _ = ray_set(self.host, seed, n_random=1100, aimed=300)
        r = self.gs.intersect_at(o0, d0, t0)
        hit = r["prim"] >= 0
        targets = r["p"][hit & (self.material_bssrdf[np.where(hit, r["material"], 0)] >= 0)]
        lo, hi = self.host.nodes()["bmin"][0], self.host.nodes()["bmax"][0]
        o = (lo + (hi - lo) * (0.05 + 0.9 * rng.random((n_aimed, 3)))).astype(F32)
        if len(targets) < 8:  # (no BSSRDF in reach: aim at the middle of the scene)
            c = (lo + (hi - lo) * (0.3 + 0.4 * rng.random((n_aimed, 3)))).astype(F32)
            return o, (c - o).astype(F32)
        c = targets[rng.integers(0, len(targets), n_aimed)]
        a, b = targets[rng.integers(0, len(targets), n_aimed)], targets[rng.integers(0, len(targets), n_aimed)]
        o[::3] = (F32(0.5) * (a + b))[::3]
        return o, ((c - o) * F32(1.5)).astype(F32)

    def close(self):
        self.gs.close()
        self.host.close()

    def trace_oracle(self, oracle):
        def trace(o, d, tmax, time):
            o, d, tmax = (np.ascontiguousarray(a, F32) for a in (o, d, tmax))
            prim, t, _, _ = oracle.intersect(self.desc, o, d, tmax)
            hit, t2, out = _GI.oracle_interactions(oracle, self.desc, o, d, tmax)
            assert np.array_equal(hit, prim >= 0) and same_bits(t[hit], t2[hit])
            return prim, out[:, 0:3], out[:, 3:6], out[:, 6:9]
        return trace

    def trace_device(self):
        def trace(o, d, tmax, time):
            r = self.gs.intersect_at(o, d, tmax, time)
            return r["prim"], r["p"], r["p_error"], r["n"]
        return trace


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------
def sample_s(sc, oracle, trace, o, d, tmax, time, u, coef=None, has=None):
    """Sample_S for every ray: (records, pi, po, steps of the longest chain).  coef: a PgBSSRDF that stands for every bssrdfs[] entry (a textured material's
    table with one of its coefficient sets, `textured` cleared); has: per ray, whether ComputeScatteringFunctions got as far as setting the bssrdf."""
    L = oracle.lib()
    n = len(tmax)
    po = sc.gs.intersect_at(o, d, tmax, time)
    rec = np.zeros(n, sc.gpu.SUBSURFACE_SAMPLE_DTYPE)
    pi = np.zeros(n, sc.gpu.INTERACTION_DTYPE)
    pi["prim"] = -1
    rec["prim"] = po["prim"]
    rec["status"] = np.where(po["prim"] >= 0, 0, -1)
    rec["bssrdf"] = rec["medium_inside"] = rec["medium_outside"] = -1
    hit = po["prim"] >= 0
    idx = np.where(hit, sc.material_bssrdf[np.where(hit, po["material"], 0)], -1)
    if has is not None: idx = np.where(has, idx, -1)
    B = (lambda k: coef) if coef is not None else (lambda k: sc.bssrdfs[k])
    ss = normalize32(po["shading_dpdu"].copy()) if n else np.zeros((0, 3), F32)
    ts = cross64(po["shading_n"], ss)
    frame = np.ascontiguousarray(np.concatenate([ss, ts, po["shading_n"]], 1), F32)
    u1 = np.zeros(n, F32); target = np.zeros((n, 3), F32)
    co, cd = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    active = []
    for i in np.flatnonzero(idx >= 0):
        assert not B(idx[i]).textured
        rec["status"][i], rec["bssrdf"][i], rec["eta"][i] = 1, idx[i], B(idx[i]).eta
        out = np.zeros(7, F32)
        p = np.ascontiguousarray(po["p"][i])
        if not L.oracle_bssrdf_probe_segment(C.addressof(B(idx[i])), sc.tables, frame[i].ctypes.data, p.ctypes.data, float(u[i, 0]), float(u[i, 1]), float(u[i, 2]),
                                             out.ctypes.data): continue
        pd = out[4:7] - out[1:4]
        if not pd.any(): continue
        u1[i], target[i], co[i], cd[i] = out[0], out[4:7], out[1:4], pd
        active.append(i)
    active = np.array(active, np.int64)
    med = np.zeros(n, np.int32)  # medium of the probe ray under way, index + 1 (Sample_Sp's `base` carries none)
    found = [[] for _ in range(n)]  # per ray: (probe ray o, d, p, n, prim, its medium) of every hit on the material
    steps = 0
    while len(active):
        steps += 1
        assert steps < 4000
        rec["chain_rays"][active] += 1
        prim, p, perr, nrm = trace(co[active], cd[active], np.full(len(active), SHADOW_TMAX, F32), time[active])
        go_on = []
        for k, i in enumerate(active):
            if prim[k] < 0: continue
            if sc.tri_material[prim[k]] == B(idx[i]).match_material:
                found[i].append((co[i].copy(), cd[i].copy(), p[k].copy(), nrm[k].copy(), int(prim[k]), int(med[i])))
            nd = (target[i] - p[k]).astype(F32)
            if not nd.any(): continue
            m_in = sc.m_in[prim[k]] + 1 if sc.m_in is not None else 0
            m_out = sc.m_out[prim[k]] + 1 if sc.m_out is not None else 0
            if m_in == m_out: m_in = m_out = med[i]
            with np.errstate(all="ignore"):
                outside = (nd[0] * nrm[k][0] + nd[1] * nrm[k][1]) + nd[2] * nrm[k][2] > 0
            med[i] = m_out if outside else m_in
            co[i], cd[i] = spawn(oracle, p[k], perr[k], nrm[k], nd), nd
            go_on.append(i)
        active = np.array(go_on, np.int64)
    chosen = []
    for i in np.flatnonzero(idx >= 0):
        nf = len(found[i])
        rec["n_found"][i] = nf
        if nf == 0: continue
        sel = min(max(int(F32(u1[i] * F32(nf))), 0), nf - 1)
        ro, rd, p, nrm, prim, rmed = found[i][sel]
        b = C.addressof(B(idx[i]))
        pop = np.ascontiguousarray(po["p"][i])
        with np.errstate(all="ignore"):
            pdf = F32(L.oracle_bssrdf_pdf_sp(b, sc.tables, frame[i].ctypes.data, pop.ctypes.data, p.ctypes.data, nrm.ctypes.data)) / F32(nf)
            dv = pop - p
            r = np.sqrt(F32(F32(dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]))
        out = np.zeros(9, F32)
        L.oracle_bssrdf_radial(b, sc.tables, float(r), 0.5, out.ctypes.data)
        if not out[:3].any() or pdf == 0: continue
        m_in = sc.m_in[prim] + 1 if sc.m_in is not None else 0
        m_out = sc.m_out[prim] + 1 if sc.m_out is not None else 0
        if m_in == m_out: m_in = m_out = rmed
        rec["status"][i], rec["S"][i], rec["pdf"][i], rec["medium_inside"][i], rec["medium_outside"][i] = 2, out[:3], pdf, m_in - 1, m_out - 1
        chosen.append((i, ro, rd, p, nrm, prim))
    if chosen:  # pi: pg_intersect_at's record of the probe ray that found the chosen hit, with wo = shading.n (bssrdf.cpp:243-248), t = 0
        rows = np.array([c[0] for c in chosen])
        full = sc.gs.intersect_at(np.array([c[1] for c in chosen], F32), np.array([c[2] for c in chosen], F32), np.full(len(rows), SHADOW_TMAX, F32), time[rows])
        assert np.array_equal(full["prim"], [c[5] for c in chosen]) and same_bits(full["p"], np.array([c[3] for c in chosen], F32)) and same_bits(full["n"], np.array([c[4] for c in chosen], F32))
        full["wo"] = full["shading_n"]
        full["t"] = 0
        pi[rows] = full
    return rec, pi, po, steps


# ---- the adapter BSDF: float32, every operation in the order csrc/pg_bxdf.h and csrc/pg_bssrdf.h write it -------------------------------------------------
def fr_dielectric(cos_i, eta_t):  # reflection.cpp:47-68 with etaI = 1
    with np.errstate(all="ignore"):
        cos_i = np.clip(cos_i, F32(-1), F32(1))
        enter = cos_i > 0
        ei, et = np.where(enter, F32(1), eta_t).astype(F32), np.where(enter, eta_t, F32(1)).astype(F32)
        cos_i = np.abs(cos_i)
        sin_i = np.sqrt(np.maximum(F32(0), F32(1) - cos_i * cos_i))
        sin_t = ei / et * sin_i
        cos_t = np.sqrt(np.maximum(F32(0), F32(1) - sin_t * sin_t))
        rparl = ((et * cos_i) - (ei * cos_t)) / ((et * cos_i) + (ei * cos_t))
        rperp = ((ei * cos_i) - (et * cos_t)) / ((ei * cos_i) + (et * cos_t))
        return np.where(sin_t >= 1, F32(1), (rparl * rparl + rperp * rperp) / F32(2)).astype(F32)


def adapter_lobe_f(oracle, eta, cos_i):  # SeparableBSSRDFAdapter::f = Sw(wi) * eta^2, bssrdf.h:97-100, :214-219
    m1 = np.array([oracle.lib().oracle_fresnel_moment1(float(F32(1) / e)) for e in eta], F32)
    c = F32(1) - F32(2) * m1
    with np.errstate(all="ignore"):
        return ((F32(1) - fr_dielectric(cos_i, eta)) / (c * PI)) * (eta * eta)


def cosine_sample_hemisphere(u0, u1):  # sampling.cpp:91-109, sampling.h:159-163; sinf / cosf are glibc's
    n = len(u0)
    out = np.zeros((n, 3), F32)
    ox, oy = F32(2) * u0 - F32(1), F32(2) * u1 - F32(1)
    for i in range(n):
        if ox[i] == 0 and oy[i] == 0: dx = dy = F32(0)
        else:
            if abs(ox[i]) > abs(oy[i]): r, theta = ox[i], PI_OVER_4 * (oy[i] / ox[i])
            else: r, theta = oy[i], PI_OVER_2 - PI_OVER_4 * (ox[i] / oy[i])
            dx, dy = r * F32(LIBM.cosf(float(theta))), r * F32(LIBM.sinf(float(theta)))
        out[i] = dx, dy, np.sqrt(max(F32(0), F32(F32(1) - dx * dx) - dy * dy))
    return out


class Adapter:
    def __init__(self, gpu, oracle, pi, eta):
        self.gpu, self.oracle, self.pi, self.eta = gpu, oracle, pi, np.ascontiguousarray(eta, F32)
        self.rows = np.flatnonzero(pi["prim"] >= 0)
        r = pi[self.rows]
        self.ns, self.ng, self.wo = r["shading_n"], r["n"], r["wo"]
        self.ss = normalize32(r["shading_dpdu"].copy())
        self.ts = cross64(self.ns, self.ss)
        self.wo_l = self.local(self.wo)

    local = _GS.Bsdfs.local
    world = _GS.Bsdfs.world

    def records(self, flags):
        want = np.zeros(len(self.pi), self.gpu.SCATTER_DTYPE)
        want["prim"] = -1
        r = self.rows
        want["prim"][r], want["n_bxdfs"][r], want["n_matching"][r], want["eta"][r], want["shading_n"][r] = self.pi["prim"][r], 1, int((flags & 5) == 5), 1, self.ns
        return want

    def f_pdf(self, wi, flags):
        wi = wi[self.rows]
        wi_l = self.local(wi)
        want = self.records(flags)
        match = (flags & 5) == 5
        ok = self.wo_l[:, 2] != 0
        reflect = dot32(wi, self.ng) * dot32(self.wo, self.ng) > 0
        f = np.where(ok & reflect & match, adapter_lobe_f(self.oracle, self.eta[self.rows], wi_l[:, 2]), F32(0)).astype(F32)
        pdf = np.where(ok & match & (self.wo_l[:, 2] * wi_l[:, 2] > 0), np.abs(wi_l[:, 2]) * INV_PI, F32(0)).astype(F32)
        want["f"][self.rows], want["pdf"][self.rows], want["wi"][self.rows] = f[:, None], pdf, wi
        return want

    def sample_f(self, u, flags):
        u = u[self.rows]
        want = self.records(flags)
        if (flags & 5) != 5: return want
        wi_l = cosine_sample_hemisphere(np.minimum(u[:, 0], ONE_MINUS_EPS), u[:, 1])
        wi_l[:, 2] = np.where(self.wo_l[:, 2] < 0, -wi_l[:, 2], wi_l[:, 2])
        pdf = np.where(self.wo_l[:, 2] * wi_l[:, 2] > 0, np.abs(wi_l[:, 2]) * INV_PI, F32(0)).astype(F32)
        ok = (self.wo_l[:, 2] != 0) & (pdf != 0)
        wi = self.world(np.ascontiguousarray(wi_l))
        reflect = dot32(wi, self.ng) * dot32(self.wo, self.ng) > 0
        f = np.where(reflect, adapter_lobe_f(self.oracle, self.eta[self.rows], wi_l[:, 2]), F32(0)).astype(F32)
        r = self.rows[ok]
        want["f"][r], want["pdf"][r], want["wi"][r], want["sampled_type"][r] = f[ok][:, None], pdf[ok], wi[ok], 5
        return want


# ---- the cases: computed once per scene, shared by the tests ---------------------------------------------------------------------------------------------
CONSTANT = ["sss_subsurface", "sss_kd_rough", "sss_two_materials", "sss_named_spheres", "sss_instances", "sss_mix_component"]
MEDIA = ["sss_preset_volpath", "sss_preset_volpath+transition"]
MOTION = ["sss_motion", "sss_nest_motion"]
TEXTURED = ["sss_textured_sigma_kt", "sss_textured_kd_bump"]
SEEDS = {name: 1201 + k for k, name in enumerate(CONSTANT + MEDIA + MOTION + TEXTURED + ["cornell"])}


@pytest.fixture(scope="module")
def case(gpu, oracle):
    """name -> the scene, the device's records and the restatement's."""
    cache = {}

    def get(name):
        if name in cache: return cache[name]
        sc = Scene(gpu, name, SEEDS[name])
        moving = name in MOTION
        if moving: sc.time = np.random.default_rng(SEEDS[name] + 5).random(sc.n).astype(F32)
        c = dict(sc=sc)
        c["rec"], c["pi"], c["po"] = sc.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u, sc.time, with_po=True)
        if name not in TEXTURED:
            c["want"], c["want_pi"], c["want_po"], c["steps"] = sample_s(sc, oracle, sc.trace_device() if moving else sc.trace_oracle(oracle), sc.o, sc.d, sc.tmax, sc.time, sc.u)
        cache[name] = c
        return c
    yield get
    for c in cache.values(): c["sc"].close()


def check(c, name):
    sc = c["sc"]
    assert c["rec"].dtype == sc.gpu.SUBSURFACE_SAMPLE_DTYPE and c["pi"].dtype == c["po"].dtype == sc.gpu.INTERACTION_DTYPE
    assert records_equal(c["po"], c["want_po"]), (name, "po", first_difference(c["po"], c["want_po"]))  # pg_intersect_at's bytes
    assert records_equal(c["rec"], c["want"]), (name, "record", first_difference(c["rec"], c["want"]))
    assert records_equal(c["pi"], c["want_pi"]), (name, "pi", first_difference(c["pi"], c["want_pi"]))
    assert not c["rec"]["reserved"].any()


# ---- 1. constant coefficients ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONSTANT)
def test_constant_coefficients_equal_the_restatement(case, name):
    c = case(name)
    w = c["want"]
    counts = dict(sampled=(w["status"] == 2).sum(), two=(w["n_found"] >= 2).sum(), black=(w["status"] == 1).sum(), missed=(w["status"] == -1).sum())
    print(name, counts, "longest chain", c["steps"])
    assert counts["sampled"] >= 200 and counts["two"] >= 20 and counts["black"] >= 10 and counts["missed"] >= 10, (name, counts)  # by the restatement alone
    check(c, name)
    alone, pi = c["sc"].gs.subsurface_sample_at(c["sc"].o, c["sc"].d, c["sc"].tmax, c["sc"].u, c["sc"].time)  # po = NULL changes no record
    assert records_equal(alone, c["rec"]) and records_equal(pi, c["pi"])


# ---- 2. media ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MEDIA)
def test_the_exit_points_medium_interface(case, name):
    c = case(name)
    assert c["sc"].desc.n_media > 0
    check(c, name)
    ok = c["want"]["status"] == 2
    inside, outside = c["want"]["medium_inside"][ok], c["want"]["medium_outside"][ok]
    assert ok.sum() >= 200
    if name.endswith("+transition"): assert ((inside == 0) & (outside == -1)).sum() >= 100  # the primitive's own transition
    else: assert (inside == -1).all() and (outside == -1).all()  # fog on both sides is no transition: the probe ray's medium, and Sample_Sp's rays start without one


# ---- 3. motion and nesting: by composition with pg_intersect_at ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MOTION)
def test_chains_under_motion_compose_with_intersect_at(case, name):
    c = case(name)
    check(c, name)
    sc = c["sc"]
    assert (c["want"]["status"] == 2).sum() >= 100, name
    n = sc.n
    even = np.arange(n) % 2 == 0
    ends = [sc.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u, np.full(n, t, F32)) for t in (0, 1)]
    assert not records_equal(ends[0][0], ends[1][0]), name  # the case cannot pass with the times ignored
    mixed = sc.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u, np.where(even, F32(0), F32(1)).astype(F32))  # times per lane
    assert records_equal(mixed[0], np.where(even, ends[0][0], ends[1][0])) and records_equal(mixed[1], np.where(even, ends[0][1], ends[1][1]))
    assert records_equal(sc.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u)[0], ends[0][0])  # time = NULL equals zeros


def denoted_sample(rec, pi, po, sc, end):
    """One call's results in a form two scenes can share (test_gpu_interactions.denoted: a prim or instance number through what it denotes; time dropped)."""
    as_isect = np.zeros(len(rec), sc.gpu.INTERACTION_DTYPE)
    as_isect["prim"], as_isect["instance"] = rec["prim"], -1
    rest = rec.copy()
    rest["prim"] = 0
    return _GI.denoted(as_isect, sc.host, end)[0], rest.tobytes(), _GI.denoted(pi, sc.host, end), _GI.denoted(po, sc.host, end)


@pytest.mark.parametrize("name", MOTION)
def test_the_shutters_ends_reach_the_oracle(case, gpu, oracle, name):
    """The two ends of the motion tied to the CPU restatement, not to the device's own pg_intersect_at.  The oracle's entries trace at Ray's default time 0, where
    AnimatedTransform::Interpolate returns the start transform itself: the scene at rest under its start transforms.  So at time 0 every record, pi and po of the
    moving scene must equal the oracle-based restatement of that very scene.  For the close end the scene is written once more with its `ActiveTransform StartTime`
    and `EndTime` blocks exchanged: its time 0 is the original's time 1 (Interpolate returns the end transform itself there), it equals the oracle-based restatement
    too, and the original's results at time 1 must denote the same records.  (A static twin in the usual sense does not exist for sss_nest_motion: a shape that
    moves INSIDE an object definition is a TransformedPrimitive there, which a scene without motion cannot state -- its transform would be baked into the
    vertices, other roundings -- so both scenes take this route.)"""
    c = case(name)
    sc, n = c["sc"], c["sc"].n
    zero, one = np.zeros(n, F32), np.ones(n, F32)
    got = sc.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u, zero, with_po=True)
    want = sample_s(sc, oracle, sc.trace_oracle(oracle), sc.o, sc.d, sc.tmax, zero, sc.u)
    for g, w, what in zip(got, want, ("record", "pi", "po")):
        assert records_equal(g, w), (name, "open", what, first_difference(g, w))
    text = open(os.path.join(GOLD, name + ".pbrt")).read()
    assert text.count("ActiveTransform EndTime") >= 2
    text = text.replace("ActiveTransform StartTime", "ActiveTransform @").replace("ActiveTransform EndTime", "ActiveTransform StartTime").replace("ActiveTransform @", "ActiveTransform EndTime")
    rev = Scene(gpu, name + " reversed", SEEDS[name], text=text)
    try:
        got_r = rev.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u, zero, with_po=True)
        want_r = sample_s(rev, oracle, rev.trace_oracle(oracle), sc.o, sc.d, sc.tmax, zero, sc.u)
        for g, w, what in zip(got_r, want_r, ("record", "pi", "po")):
            assert records_equal(g, w), (name, "close, reversed scene", what, first_difference(g, w))
        got1 = sc.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u, one, with_po=True)
        assert (got1[1]["time"][got1[0]["status"] == 2] == 1).all()
        assert denoted_sample(*got1, sc, True) == denoted_sample(*got_r, rev, False), (name, "the records at the shutter's close differ from the reversed scene's at its open")
        assert not records_equal(got[0], got1[0]) and (got1[0]["status"] == 2).sum() >= 100 and (got[0]["status"] == 2).sum() >= 100
    finally: rev.close()


# ---- 4. textured coefficients: the invariants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TEXTURED)
def test_textured_coefficients_keep_the_invariants(case, name):
    c = case(name)
    sc, rec, pi = c["sc"], c["rec"], c["pi"]
    assert any(b.textured for b in sc.bssrdfs)
    want_po = sc.gs.intersect_at(sc.o, sc.d, sc.tmax, sc.time)
    assert records_equal(c["po"], want_po) and np.array_equal(rec["prim"], want_po["prim"])
    hit = want_po["prim"] >= 0
    idx = np.where(hit, sc.material_bssrdf[np.where(hit, want_po["material"], 0)], -1)
    assert np.array_equal(rec["status"] == -1, ~hit) and (rec["status"][hit & (idx < 0)] == 0).all()
    has = rec["status"] >= 1  # (a textured BSSRDF exists only where the BSDF has a BxDF)
    assert has.sum() >= 300 and (idx[has] >= 0).all() and np.array_equal(rec["bssrdf"][has], idx[has]) and (rec["bssrdf"][~has] == -1).all()
    ok = rec["status"] == 2
    assert ok.sum() >= 200 and np.array_equal(pi["prim"] >= 0, ok)
    match = np.array([sc.bssrdfs[k].match_material for k in rec["bssrdf"][ok]])
    assert np.array_equal(pi["material"][ok], match) and same_bits(pi["wo"][ok], pi["shading_n"][ok])
    assert (rec["n_found"][ok] >= 1).all() and (rec["chain_rays"][ok] >= rec["n_found"][ok]).all() and (rec["pdf"][ok] > 0).all() and (rec["S"][ok] > 0).any(1).all()
    rest = rec[~ok]
    assert not rest["S"].any() and not rest["pdf"].any() and (rest["medium_inside"] == -1).all() and not rec["reserved"].any()
    blank = pi[~ok].copy()
    blank["prim"] = 0
    assert not blank.view(np.uint8).any()


def coefficient_sets(sc, oracle, k, a_values, b_value):
    """bssrdfs[k] once per value the two-colour texture `a` takes, as ComputeScatteringFunctions hands the coefficients to TabulatedBSSRDF's constructor
    (bssrdf.h:146-150), in float32: textured == 1 sigma_a = scale * a, sigma_s = scale * b (subsurface.cpp:87-88); textured == 2
    SubsurfaceFromDiffuse(table, Kd = a, scale * mfp = scale * b) (kdsubsurface.cpp:88-91, bssrdf.cpp:182-191) around the oracle's InvertCatmullRom."""
    bd = sc.bssrdfs[k]
    assert bd.textured in (1, 2)
    rho_samples = sc.tables + 4 * bd.table
    rho_eff = rho_samples + 4 * (bd.n_rho + bd.n_radius + bd.n_rho * bd.n_radius)
    scale, b = F32(bd.scale), np.array(b_value, F32)
    out = []
    for a in a_values:
        a = np.array(a, F32)
        if bd.textured == 1: sa, ssc = a * scale, b * scale
        else:
            mfree = b * scale
            r = np.array([oracle.lib().oracle_invert_catmull_rom(bd.n_rho, rho_samples, rho_eff, float(x)) for x in a], F32)
            ssc, sa = r / mfree, (F32(1) - r) / mfree
        sig_t = (sa + ssc).astype(F32)
        rho = (ssc / sig_t).astype(F32)
        cp = type(bd).from_buffer_copy(bd)
        cp.textured = 0
        for ch in range(3): cp.sigma_t[ch], cp.rho[ch] = sig_t[ch], rho[ch]
        out.append(cp)
    return out


def textured_index(sc):
    k = [i for i in range(sc.nb) if sc.bssrdfs[i].textured]
    assert len(k) == 1
    return k[0]


def test_a_two_colour_sigma_a_gives_one_of_two_restatements(case, oracle):
    """sss_textured_sigma_kt has no bump map: po's frame is Scene::Intersect's, sigma_a is a 3D checkerboard of two colours (point-sampled: a ray query has no
    differentials) and Kt a 2D one of white and black with Kr black -- where it is black the BSDF is empty and ComputeScatteringFunctions returns before it sets
    the BSSRDF (subsurface.cpp:79-80).  So every record, with its pi, equals bit for bit the restatement under one of the two coefficient sets, where `has`
    (n_bxdfs > 0 of pg_scatter_f_at for the same rays) says which hits carry a BSSRDF at all.  This pins bssrdf_coefficients_at<true>'s textured == 1 branch."""
    name = "sss_textured_sigma_kt"
    c = case(name)
    sc, n = c["sc"], c["sc"].n
    k = textured_index(sc)
    assert sc.bssrdfs[k].textured == 1 and sc.bssrdfs[k].scale == 2
    sets = coefficient_sets(sc, oracle, k, ([0.002, 0.004, 0.02], [0.02, 0.004, 0.002]), [0.05, 0.06, 0.08])
    has = sc.gs.scatter_f_at(sc.o, sc.d, sc.tmax, sc.d, sc.time)["n_bxdfs"] > 0
    wants = [sample_s(sc, oracle, sc.trace_oracle(oracle), sc.o, sc.d, sc.tmax, sc.time, sc.u, coef=cp, has=has) for cp in sets]
    assert records_equal(c["po"], wants[0][2])
    rows = lambda a, size: np.ascontiguousarray(a).view(np.uint8).reshape(n, size)
    same = [(rows(c["rec"], 64) == rows(w[0], 64)).all(1) & (rows(c["pi"], 128) == rows(w[1], 128)).all(1) for w in wants]
    bad = np.flatnonzero(~(same[0] | same[1]))
    assert len(bad) == 0, (len(bad), bad[:5], first_difference(c["rec"][bad[:1]], wants[0][0][bad[:1]]), first_difference(c["rec"][bad[:1]], wants[1][0][bad[:1]]))
    on = c["rec"]["status"] >= 1
    hit = c["po"]["prim"] >= 0
    textured = hit & (sc.material_bssrdf[np.where(hit, c["po"]["material"], 0)] == k)
    counts = dict(first=(on & same[0] & ~same[1]).sum(), second=(on & same[1] & ~same[0]).sum(), sampled=(c["rec"]["status"] == 2).sum(),
                  empty_bsdf=(textured & ~has).sum(), black=(c["rec"]["status"] == 1).sum())
    print(name, counts)
    assert counts["first"] >= 50 and counts["second"] >= 50 and counts["sampled"] >= 200 and counts["empty_bsdf"] >= 20 and counts["black"] >= 10, counts
    assert (c["rec"]["status"][textured & ~has] == 0).all() and (c["rec"]["status"][textured & has] >= 1).all()  # "textured BSSRDF and an empty BxDF list: none"


def test_a_two_colour_kd_gives_one_of_two_profiles(case, oracle):
    """sss_textured_kd_bump: the frame at po is bumped, which this file does not restate, so the chain is not; but S = Sr(|po.p - pi.p|) needs no frame.  Kd is
    a 2D checkerboard of two colours (point-sampled), so S of every sampled record equals oracle_bssrdf_radial under one of the two coefficient sets
    SubsurfaceFromDiffuse derives, bit for bit: this pins bssrdf_coefficients_at<true>'s textured == 2 branch.  status follows pg_scatter_f_at's n_bxdfs."""
    name = "sss_textured_kd_bump"
    c = case(name)
    sc, rec, pi, po = c["sc"], c["rec"], c["pi"], c["po"]
    k = textured_index(sc)
    assert sc.bssrdfs[k].textured == 2 and sc.bssrdfs[k].scale == 1
    sets = coefficient_sets(sc, oracle, k, ([0.7, 0.3, 0.2], [0.2, 0.5, 0.8]), [10, 14, 20])
    has = sc.gs.scatter_f_at(sc.o, sc.d, sc.tmax, sc.d, sc.time)["n_bxdfs"] > 0
    hit = po["prim"] >= 0
    textured = hit & (sc.material_bssrdf[np.where(hit, po["material"], 0)] == k)
    assert np.array_equal(rec["status"] >= 1, textured & has) and (textured & has).sum() >= 300
    ok = np.flatnonzero(rec["status"] == 2)
    dv = po["p"][ok] - pi["p"][ok]
    r = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    assert r.dtype == F32
    S = np.zeros((2, len(ok), 3), F32)
    out = np.zeros(9, F32)
    for s, cp in enumerate(sets):
        for j in range(len(ok)):
            oracle.lib().oracle_bssrdf_radial(C.addressof(cp), sc.tables, float(r[j]), 0.5, out.ctypes.data)
            S[s, j] = out[:3]
    same = [(bits(rec["S"][ok]) == bits(S[s])).all(1) for s in (0, 1)]
    assert (same[0] | same[1]).all(), (int((~(same[0] | same[1])).sum()), "of", len(ok))
    counts = dict(first=(same[0] & ~same[1]).sum(), second=(same[1] & ~same[0]).sum())
    print(name, counts)
    assert counts["first"] >= 50 and counts["second"] >= 50, counts


# ---- 5. no BSSRDF ------------------------------------------------------------------------------------------------------------------------------------------
def test_a_scene_without_bssrdf_is_served(case):
    c = case("cornell")
    assert c["sc"].nb == 0
    check(c, "cornell")
    st = c["rec"]["status"]
    assert ((st == 0) | (st == -1)).all() and (st == 0).sum() >= 500 and (st == -1).sum() >= 10 and (c["pi"]["prim"] == -1).all()


# ---- 6. the adapter BSDF at pi -------------------------------------------------------------------------------------------------------------------------------
ADAPTER_MASKS = (31, 1 | 4, 16 | 1)


@pytest.mark.parametrize("name", ["sss_subsurface", "sss_two_materials"])
def test_the_exit_bsdf_equals_the_restatement(case, gpu, oracle, name):
    c = case(name)
    sc, pi, eta = c["sc"], c["pi"], c["rec"]["eta"]
    rng = np.random.default_rng(77)
    wi = (rng.normal(size=(sc.n, 3)) * rng.uniform(0.5, 2, (sc.n, 1))).astype(F32)
    u = np.minimum(rng.random((sc.n, 2)).astype(F32), ONE_MINUS_EPS)
    u[::17, 0] = 0
    ad = Adapter(gpu, oracle, pi, eta)
    assert len(ad.rows) >= 200
    before = sc.gs.counters()
    for flags in ADAPTER_MASKS:
        got, want = sc.gs.subsurface_f_at(pi, eta, wi, flags), ad.f_pdf(wi, flags)
        assert got.dtype == gpu.SCATTER_DTYPE and records_equal(got, want), (name, "f / Pdf", flags, first_difference(got, want))
        got, want = sc.gs.subsurface_sample_f_at(pi, eta, u, flags), ad.sample_f(u, flags)
        assert records_equal(got, want), (name, "Sample_f", flags, first_difference(got, want))
        if flags == 16 | 1: assert not got["pdf"].any() and not got["n_matching"].any()
        else: assert (got["pdf"] > 0).sum() >= 200 and (got["f"] > 0).all(1).sum() >= 200
    assert sc.gs.counters() == before  # nothing is traced, no counter moves


# ---- 7. launch shapes, device memory, counters --------------------------------------------------------------------------------------------------------------
def test_batch_sizes_are_prefixes_of_one_batch(case):
    c = case("sss_instances")
    sc = c["sc"]
    for k in (0, 1, 63, 64, 65, 257):
        rec, pi, po = sc.gs.subsurface_sample_at(sc.o[:k], sc.d[:k], sc.tmax[:k], sc.u[:k], sc.time[:k], with_po=True)
        assert records_equal(rec, c["rec"][:k]) and records_equal(pi, c["pi"][:k]) and records_equal(po, c["po"][:k]), k
    with pytest.raises(ValueError):
        sc.gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u[:-1])


PAD = 256  # bytes the device arrays are longer than the results: guard bytes, to catch a write past them


@pytest.mark.parametrize("name", ["sss_two_materials", "sss_nest_motion"])
def test_device_memory_equals_host_memory(case, name):
    c = case(name)
    sc = c["sc"]
    n = sc.n
    rng = np.random.default_rng(5)
    wi, u2 = rng.normal(size=(n, 3)).astype(F32), np.minimum(rng.random((n, 2)).astype(F32), ONE_MINUS_EPS)
    eta = np.ascontiguousarray(c["rec"]["eta"])
    host_f, host_s = sc.gs.subsurface_f_at(c["pi"], eta, wi, 31), sc.gs.subsurface_sample_f_at(c["pi"], eta, u2, 31)
    guard = lambda nbytes: np.full(nbytes + PAD, 0xAB, np.uint8)

    def check_bytes(dev, i, want):
        got = dev.get(i, np.uint8)
        w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert len(got) == len(w) + PAD and np.array_equal(got[:len(w)], w) and (got[len(w):] == 0xAB).all(), (name, i)
    dev = DeviceArrays()
    inputs = (sc.o, sc.d, sc.tmax, sc.time, sc.u, eta, wi, u2)
    po_, pd_, pt_, ptime, pu, peta, pwi, pu2 = (dev.put(a) for a in inputs)  # 0 .. 7
    for rnd in range(2):  # the second, identical call finds the scene's scratch as the first left it
        out, ppi, ppo, pf, ps = dev.put(guard(64 * n)), dev.put(guard(128 * n)), dev.put(guard(128 * n)), dev.put(guard(64 * n)), dev.put(guard(64 * n))
        base = 8 + 5 * rnd
        sc.gs.subsurface_sample_at_device(n, po_, pd_, pt_, ptime, pu, ppo, ppi, out)
        check_bytes(dev, base, c["rec"]); check_bytes(dev, base + 1, c["pi"]); check_bytes(dev, base + 2, c["po"])
        sc.gs.subsurface_f_at_device(n, ppi, peta, pwi, 31, pf)
        sc.gs.subsurface_sample_f_at_device(n, ppi, peta, pu2, 31, ps)
        check_bytes(dev, base + 3, host_f); check_bytes(dev, base + 4, host_s); check_bytes(dev, base + 1, c["pi"])
    alone, pi2 = dev.put(guard(64 * n)), dev.put(guard(128 * n))  # 18, 19
    sc.gs.subsurface_sample_at_device(n, po_, pd_, pt_, ptime, pu, None, pi2, alone)  # po = NULL
    check_bytes(dev, 18, c["rec"]); check_bytes(dev, 19, c["pi"])
    for i, a in enumerate(inputs):  # the inputs were only read
        assert np.array_equal(dev.get(i, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1))


SHADING = ("camera_rays", "mis_rays", "shade_launches", "resolve_launches", "shade_items", "shadow_rays", "shadow_launches", "light_tri_tests")


@pytest.mark.parametrize("name", ["sss_subsurface", "cornell"])
def test_counters_count_the_first_walk(case, name):
    c = case(name)
    sc, gs = c["sc"], c["sc"].gs
    gs.counters_reset()
    gs.subsurface_sample_at(sc.o, sc.d, sc.tmax, sc.u, sc.time)
    cn = gs.counters()
    assert cn["closest_rays"] == sc.n + c["want"]["chain_rays"].sum() and cn["closest_launches"] == 1 + c["steps"]
    assert cn["closest_node_visits"] > 0 and all(cn[k] == 0 for k in SHADING)
    if name == "sss_subsurface":
        assert c["steps"] >= 3 and c["steps"] == c["want"]["chain_rays"].max()
        gs.counters_reset()
        gs.intersect_at(sc.o, sc.d, sc.tmax, sc.time)
        first = gs.counters()
        assert cn["closest_node_visits"] > first["closest_node_visits"]  # the chains' launches moved the visit totals beyond the first launch's
