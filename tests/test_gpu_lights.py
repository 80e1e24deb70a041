"""pg_light_sample_at / pg_light_pdf_at / pg_light_le_at: Light::Sample_Li with VisibilityTester::Unoccluded, Light::Pdf_Li and the emitted radiance a ray
meets (PgLightSample, csrc/pg_lightquery.h), at reference points that are pg_intersect_at records.

The reference for point, spot, distant, triangle area and constant infinite lights is a float32 NumPy restatement written in the order the reference writes
the arithmetic (point.cpp:43-52, spot.cpp:51-72, distant.cpp:50-60, diffuse.cpp:68-81 with shape.cpp:56-70 and triangle.cpp:582-607, infinite.cpp:93-135
with sampling.h:72-89, 127-141 and mipmap.h's triangle()), fed from desc.lights, desc.P / indices and the PgInteraction records; OffsetRayOrigin,
IntersectP and Triangle::Intersect are the oracle's entries; sinf / cosf / acosf / atan2f are glibc's, the reference's own.  Every field of every record is
compared bit for bit.  The other light kinds are pinned by composition.  tests/test_emulated_lights.py runs this file without a GPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
F32 = np.float32


def _load(filename):
    spec = importlib.util.spec_from_file_location(filename[:-3] + "_helpers", os.path.join(os.path.dirname(__file__), filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GS = _load("test_gpu_scatter.py")
records_equal, first_difference, struct_array, ray_set = _GS.records_equal, _GS.first_difference, _GS.struct_array, _GS.ray_set
dot32, normalize32, cross64, DeviceArrays, same_bits, bits = _GS.dot32, _GS.normalize32, _GS.cross64, _GS.DeviceArrays, _GS.same_bits, _GS.bits

AREA, POINT, SPOT, DISTANT, INFINITE, PROJECTION, GONIO = range(7)  # PgLightType
TRI_FLIP_NORMAL, TRI_HAS_N, PRIM_SPHERE = 1, 4, 32
PI, INV_PI, INV_2PI = F32(3.14159265358979323846), F32(0.31830988618379067154), F32(0.15915494309189533577)
MACH_EPS = F32(5.9604644775390625e-08)
SHADOW_TMAX = F32(1) - F32(0.0001)  # 1 - ShadowEpsilon

LIBM = C.CDLL("libm.so.6")
for _f in ("sinf", "cosf", "acosf"):
    getattr(LIBM, _f).restype, getattr(LIBM, _f).argtypes = C.c_float, [C.c_float]
LIBM.atan2f.restype, LIBM.atan2f.argtypes = C.c_float, [C.c_float, C.c_float]


def libm1(name, x):
    fn = getattr(LIBM, name)
    return np.array([fn(float(v)) for v in x], F32)


def lensq32(a):
    return (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]


def mat3(m, w):  # Transform::operator()(Vector3), transform.h:233-239, over the light's nine floats
    return np.stack([(m[:, 3 * r] * w[:, 0] + m[:, 3 * r + 1] * w[:, 1]) + m[:, 3 * r + 2] * w[:, 2] for r in range(3)], 1)


def gamma32(n):  # pbrt.h:289-291
    return (F32(n) * MACH_EPS) / (F32(1) - F32(n) * MACH_EPS)


def spawn_origin(oracle, p, perr, n, w):
    """OffsetRayOrigin (geometry.h:1440-1454) row by row: the oracle's entry."""
    p, perr, n, w = (np.ascontiguousarray(a, F32) for a in (p, perr, n, w))
    out = np.zeros_like(p)
    fn = oracle.lib().oracle_spawn_ray_origin
    for i in range(len(p)):
        fn(p[i].ctypes.data, perr[i].ctypes.data, n[i].ctypes.data, w[i].ctypes.data, out[i].ctypes.data)
    return out


class Scene:
    """One scene on the device, its description's tables as NumPy views, and the reference points of its ray set."""

    def __init__(self, gpu, name=None, text=None, seed=0, extra_rays=None):
        self.gpu = gpu
        self.host = gpu.HostScene(os.path.join(GOLD, name + ".pbrt")) if text is None else gpu.HostScene(text=text)
        d = self.desc = self.host.desc
        self.gs = gpu.GpuScene(d)
        self.lights = struct_array(d.lights, d.n_lights, gpu.abi.PgLight)
        self.nl = d.n_lights
        self.indices = np.ctypeslib.as_array(d.indices, (d.n_prims_all, 3))
        self.flags = np.ctypeslib.as_array(d.tri_flags, (d.n_prims_all,))
        self.P = np.ctypeslib.as_array(d.P, (d.n_verts, 3))
        self.N = np.ctypeslib.as_array(d.N, (d.n_verts, 3)) if d.N else None
        self.spheres = struct_array(d.spheres, d.n_spheres, gpu.abi.PgSphere)
        o, dd, tmax, wi, u = ray_set(self.host, seed)
        if extra_rays is not None:
            eo, ed = extra_rays(self)
            k = len(eo) - (1 if (len(tmax) + len(eo)) % 256 == 0 else 0)
            o, dd = np.ascontiguousarray(np.concatenate([o, eo[:k]]), F32), np.ascontiguousarray(np.concatenate([dd, ed[:k]]), F32)
            tmax = np.concatenate([tmax, np.full(k, np.inf, F32)])
            rng = np.random.default_rng(seed + 7)
            wi, u = np.concatenate([wi, rng.normal(size=(k, 3)).astype(F32)]), np.concatenate([u, rng.random((k, 2)).astype(F32)])
        self.o, self.d, self.tmax, self.wi_random, self.u = o, dd, tmax, np.ascontiguousarray(wi, F32), np.ascontiguousarray(u, F32)
        self.n = len(tmax)
        assert self.n % 256 != 0 and self.n > 1500
        self.ref = self.gs.intersect_at(o, dd, tmax)
        self.light = (np.arange(self.n) % (self.nl + 2) - 1).astype(np.int32)  # -1, every light, n_lights, and again

    def close(self):
        self.gs.close()
        self.host.close()

    def emitter(self, li):
        """The shape of area light li: 'triangle', or the quadric's PgQuadricShape number."""
        prim = self.lights["prim"][li]
        return "triangle" if not self.flags[prim] & PRIM_SPHERE else int(self.spheres["shape"][self.indices[prim, 0]])

    def image_texel(self, image):  # the one texel of a 1 x 1 MIPMap, and its wrap mode
        im = struct_array(self.desc.images, self.desc.n_images, self.gpu.abi.PgImage)[image]
        assert im["width"] == 1 and im["height"] == 1 and im["n_levels"] == 1 and not im["is_float"]
        off = int(im["level_offset"][0])
        return np.ctypeslib.as_array(self.desc.texels, (self.desc.n_texel_floats,))[off:off + 3].astype(F32), int(im["wrap"])

    def env_table(self, l):
        nu, nv = int(l["env_nu"]), int(l["env_nv"])
        size = (2 * nu + 2) * nv + 2 * nv + 2
        t = np.ctypeslib.as_array(self.desc.env_tables, (self.desc.n_env_floats,))[int(l["env_table"]):int(l["env_table"]) + size]
        return t, nu, nv


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------
def sample_1d(func, cdf, func_int, n, u):  # Distribution1D::SampleContinuous, sampling.h:72-89
    first = int(np.searchsorted(cdf[:n + 1], u, side="right"))  # FindInterval: the first entry beyond u
    offset = min(max(first - 1, 0), n - 1)
    du = F32(u) - cdf[offset]
    if cdf[offset + 1] - cdf[offset] > 0: du = du / (cdf[offset + 1] - cdf[offset])
    pdf = func[offset] / func_int if func_int > 0 else F32(0)
    return (F32(offset) + du) / F32(n), F32(pdf), offset


def lookup_1x1(texel, wrap, s, t):  # MIPMap::Lookup(st) = triangle(0, st) over one texel, mipmap.h:189-243
    s, t = s * F32(1) - F32(0.5), t * F32(1) - F32(0.5)
    s0, t0 = np.floor(s), np.floor(t)
    ds, dt = s - s0, t - t0

    def tex(ss, tt):
        inside = (ss == 0) & (tt == 0) if wrap == 1 else np.ones(len(ss), bool)  # (black outside; repeat and clamp find the texel)
        return np.where(inside[:, None], texel[None, :], F32(0))
    return ((tex(s0, t0) * ((F32(1) - ds) * (F32(1) - dt))[:, None] + tex(s0, t0 + 1) * ((F32(1) - ds) * dt)[:, None])
            + tex(s0 + 1, t0) * (ds * (F32(1) - dt))[:, None]) + tex(s0 + 1, t0 + 1) * (ds * dt)[:, None]


def spherical(w):  # SphericalTheta / SphericalPhi, geometry.h:1468-1475
    theta = libm1("acosf", np.clip(w[:, 2], F32(-1), F32(1)))
    phi = np.array([LIBM.atan2f(float(y), float(x)) for x, y in zip(w[:, 0], w[:, 1])], F32)
    return theta, np.where(phi < 0, phi + F32(2) * PI, phi)


def triangle_of(sc, li):
    idx = sc.indices[sc.lights["prim"][li]]
    return sc.P[idx[:, 0]], sc.P[idx[:, 1]], sc.P[idx[:, 2]], sc.flags[sc.lights["prim"][li]], idx


def restate_samples(sc, oracle, ref, light, u):
    """(records, shadow rays, kind per sample) of Light::Sample_Li + the tester's ray for the closed-form lights; kind: the PgLightType, -1 = invalid index,
    -2 = invalid ref.  `visibility` is 1 for every tested sample: the caller sets it from IntersectP."""
    n = len(ref)
    L = sc.lights
    valid = (ref["prim"] >= 0) & (light >= 0) & (light < sc.nl)
    kind = np.where(ref["prim"] < 0, -2, np.where((light < 0) | (light >= sc.nl), -1, L["type"][np.clip(light, 0, sc.nl - 1)] if sc.nl else -1))
    li = np.where(valid, light, 0)
    l = L[li]
    p, perr, nrm = ref["p"], ref["p_error"], ref["n"]
    pdf = np.zeros(n, F32)
    Li, wi, pl, ln, lerr = (np.zeros((n, 3), F32) for _ in range(5))
    with np.errstate(all="ignore"):
        # ---- point, spot (point.cpp:43-52, spot.cpp:51-72)
        to = l["pos"] - p
        wi_pt = normalize32(to)
        d2 = lensq32(to)
        wl = normalize32(mat3(l["w2l"], -wi_pt))
        cos = wl[:, 2]
        delta = (cos - l["cos_total_width"]) / (l["cos_falloff_start"] - l["cos_total_width"])
        falloff = np.where(cos < l["cos_total_width"], F32(0), np.where(cos >= l["cos_falloff_start"], F32(1), (delta * delta) * (delta * delta))).astype(F32)
        for k, radiance in ((POINT, l["L"] / d2[:, None]), (SPOT, (l["L"] * falloff[:, None]) / d2[:, None])):
            m = valid & (kind == k)
            pdf[m], Li[m], wi[m], pl[m] = 1, radiance[m], wi_pt[m], l["pos"][m]
        # ---- distant (distant.cpp:50-60)
        m = valid & (kind == DISTANT)
        pdf[m], Li[m], wi[m] = 1, l["L"][m], l["pos"][m]
        pl[m] = (p + l["pos"] * (F32(2) * l["world_radius"])[:, None])[m]
        # ---- diffuse area light on a triangle (diffuse.cpp:68-81, shape.cpp:56-70, triangle.cpp:582-607)
        m = valid & (kind == AREA)
        if m.any():
            p0, p1, p2, flags, idx = triangle_of(sc, li)
            assert not (flags[m] & PRIM_SPHERE).any()
            su0 = np.sqrt(u[:, 0])
            b0, b1 = F32(1) - su0, u[:, 1] * su0
            b2 = (F32(1) - b0) - b1
            sp = (p0 * b0[:, None] + p1 * b1[:, None]) + p2 * b2[:, None]
            sn = normalize32(cross64(p1 - p0, p2 - p0))
            has_n = (flags & TRI_HAS_N) != 0
            if sc.N is not None:
                ns = (sc.N[idx[:, 0]] * b0[:, None] + sc.N[idx[:, 1]] * b1[:, None]) + sc.N[idx[:, 2]] * b2[:, None]
                flip = np.where(has_n, dot32(sn, ns) < 0, (flags & TRI_FLIP_NORMAL) != 0)
            else: flip = (flags & TRI_FLIP_NORMAL) != 0
            sn = np.where(flip[:, None], -sn, sn)
            serr = ((np.abs(p0 * b0[:, None]) + np.abs(p1 * b1[:, None])) + np.abs(p2 * b2[:, None])) * gamma32(6)
            apdf = F32(1) / l["area"]
            w = sp - p
            wn = normalize32(w)
            apdf = np.where(lensq32(w) == 0, F32(0), apdf * (lensq32(p - sp) / np.abs(dot32(sn, -wn)))).astype(F32)
            apdf = np.where(np.isinf(apdf), F32(0), apdf)
            apdf = np.where((apdf == 0) | (lensq32(sp - p) == 0), F32(0), apdf)  # diffuse.cpp:74-77
            awi = normalize32(sp - p)
            lit = (l["two_sided"] != 0) | (dot32(sn, -awi) > 0)
            pdf[m], wi[m], pl[m], ln[m], lerr[m] = apdf[m], awi[m], sp[m], sn[m], serr[m]
            Li[m] = np.where(lit[:, None], l["L"], F32(0))[m]
        # ---- infinite light over a 1 x 1 map (infinite.cpp:99-125, sampling.h:127-134)
        for i in np.flatnonzero(valid & (kind == INFINITE)):
            tab, nu, nv = sc.env_table(l[i])
            marg = tab[(2 * nu + 2) * nv:]
            d1, pdf1, v = sample_1d(marg, marg[nv:], marg[2 * nv + 1], nv, u[i, 1])
            row = tab[(2 * nu + 2) * v:]
            d0, pdf0, _ = sample_1d(row, row[nu:], row[2 * nu + 1], nu, u[i, 0])
            map_pdf = F32(pdf0 * pdf1)
            if map_pdf == 0: continue
            theta, phi = F32(d1 * PI), F32(F32(d0 * F32(2)) * PI)
            sin_t, cos_t, sin_p, cos_p = (F32(LIBM.sinf(float(theta))), F32(LIBM.cosf(float(theta))), F32(LIBM.sinf(float(phi))), F32(LIBM.cosf(float(phi))))
            wi[i] = mat3(l["l2w"][i:i + 1], np.array([[sin_t * cos_p, sin_t * sin_p, cos_t]], F32))[0]
            pdf[i] = F32(0) if sin_t == 0 else map_pdf / (F32(F32(2) * PI) * PI * sin_t)
            pl[i] = p[i] + wi[i] * (F32(2) * l["world_radius"][i])
            texel, wrap = sc.image_texel(int(l["env_image"][i]))
            Li[i] = lookup_1x1(texel, wrap, np.array([d0], F32), np.array([d1], F32))[0]
    assert not (valid & (kind > INFINITE)).any(), "the restatement has no projection or goniometric light"
    none = pdf == 0  # no sample: Li, wi and the tester's end point are reported as 0
    for a in (Li, wi, pl, ln, lerr): a[none] = 0
    tested = valid & (pdf > 0) & (Li != 0).any(1)
    rec = np.zeros(n, sc.gpu.LIGHT_SAMPLE_DTYPE)
    rec["light"] = np.where(valid, light, -1)
    rec["visibility"] = np.where(tested, 1, np.where(valid, -1, 0))
    rec["pdf"], rec["Li"], rec["wi"], rec["p_light"], rec["n_light"] = pdf, Li, wi, pl, ln
    shadow = np.zeros((n, 8), F32)
    t = np.flatnonzero(tested)
    origin = spawn_origin(oracle, p[t], perr[t], nrm[t], pl[t] - p[t])  # p0.SpawnRayTo(p1), interaction.h:73-78
    target = spawn_origin(oracle, pl[t], lerr[t], ln[t], origin - pl[t])
    shadow[t, 0:3], shadow[t, 3], shadow[t, 4:7], shadow[t, 7] = origin, SHADOW_TMAX, target - origin, ref["time"][t]
    return rec, shadow, kind


def restate_triangle_pdf(sc, oracle, ref, li, wi):
    """Shape::Pdf(ref, wi) against the emitter's own triangle (shape.cpp:72-87) for the rows given: the ray is ref.SpawnRay(wi)."""
    p0, p1, p2, flags, _ = triangle_of(sc, li)
    p0, p1, p2 = (np.ascontiguousarray(a, F32) for a in (p0, p1, p2))
    ro = spawn_origin(oracle, ref["p"], ref["p_error"], ref["n"], wi)
    wi = np.ascontiguousarray(wi, F32)
    lib = oracle.lib()
    hit = np.zeros(len(ref), bool)
    b = np.zeros((len(ref), 3), F32)
    t = C.c_float(0)
    for i in range(len(ref)):
        hit[i] = lib.oracle_triangle_intersect(p0[i].ctypes.data, p1[i].ctypes.data, p2[i].ctypes.data, ro[i].ctypes.data, wi[i].ctypes.data, C.c_float(np.inf), C.byref(t),
                                               b[i].ctypes.data) != 0
    with np.errstate(all="ignore"):
        lp = (p0 * b[:, 0:1] + p1 * b[:, 1:2]) + p2 * b[:, 2:3]
        ln = normalize32(cross64(p0 - p2, p1 - p2))
        pdf = lensq32(ref["p"] - lp) / (np.abs(dot32(ln, -wi)) * sc.lights["area"][li])
        pdf = np.where(np.isinf(pdf), F32(0), pdf)
    return np.where(hit, pdf, F32(0)).astype(F32)


def restate_infinite_pdf(sc, li, wi):
    """InfiniteAreaLight::Pdf_Li (infinite.cpp:127-135) with Distribution2D::Pdf (sampling.h:135-141), row by row."""
    out = np.zeros(len(wi), F32)
    l = sc.lights[li]
    w = mat3(l["w2l"], wi)
    theta, phi = spherical(w)
    sin_t = libm1("sinf", theta)
    for i in range(len(wi)):
        if sin_t[i] == 0: continue
        tab, nu, nv = sc.env_table(l[i])
        iu = min(max(int(F32(phi[i] * INV_2PI) * F32(nu)), 0), nu - 1)
        iv = min(max(int(F32(theta[i] * INV_PI) * F32(nv)), 0), nv - 1)
        marg = tab[(2 * nu + 2) * nv:]
        out[i] = (tab[(2 * nu + 2) * iv + iu] / marg[2 * nv + 1]) / (F32(F32(2) * PI) * PI * sin_t[i])
    return out


def restate_infinite_le(sc, li, d):
    """InfiniteAreaLight::Le(ray) (infinite.cpp:93-97) of light li for every direction."""
    l = sc.lights[np.full(len(d), li)]
    theta, phi = spherical(normalize32(mat3(l["w2l"], d)))
    texel, wrap = sc.image_texel(int(sc.lights["env_image"][li]))
    return lookup_1x1(texel, wrap, phi * INV_2PI, theta * INV_PI)


def light_rays(both_sides):
    """Rays aimed at the area lights' triangles: from inside the bounds and -- both_sides -- from just behind the emitter, along its normal."""
    def make(sc):
        rng = np.random.default_rng(5)
        lo, hi = sc.host.nodes()["bmin"][0], sc.host.nodes()["bmax"][0]
        os_, ds = [], []
        for li in np.flatnonzero(sc.lights["type"] == AREA):
            if sc.emitter(li) != "triangle": continue
            p0, p1, p2 = (sc.P[k].astype(np.float64) for k in sc.indices[sc.lights["prim"][li]])
            nrm = np.cross(p1 - p0, p2 - p0)
            nrm /= np.linalg.norm(nrm)
            for _ in range(40):
                a, b = rng.random(2)
                if a + b > 1: a, b = 1 - a, 1 - b
                q = p0 + a * (p1 - p0) + b * (p2 - p0)
                o = lo + (hi - lo) * (0.1 + 0.8 * rng.random(3))
                os_.append(o); ds.append(q - o)
                if both_sides:
                    for side in (-1.0, 1.0):  # 0.05 away from the emitter on either side (nearer than the ceiling behind a Cornell light), straight at it
                        os_.append(q + side * 0.05 * nrm); ds.append(-side * nrm)
        return np.array(os_, F32).reshape(-1, 3), np.array(ds, F32).reshape(-1, 3)
    return make


# ---- 1. and 2.: the closed-form lights and the constant infinite light against the restatement ------------------------------------------------------------
CLOSED_FORM = ["cornell_32", "cornell_point", "cornell_delta_only", "cornell_spot_power", "directlighting/e_five_kinds_of_light", "cornell_twosided",
               "cornell_lightnormals", "env_uniform_open"]
SEEDS = {name: 501 + k for k, name in enumerate(CLOSED_FORM)}


@pytest.fixture(scope="module")
def closed_case(gpu, oracle):
    """name -> the device's records and the restatement's for one scene's reference points (computed once, kept for the test of the whole set)."""
    cache = {}

    def case(name):
        if name in cache: return cache[name]
        sc = Scene(gpu, name, seed=SEEDS[name], extra_rays=light_rays(False))
        got, got_shadow = sc.gs.light_sample_at(sc.ref, sc.light, sc.u, with_shadow_rays=True)
        alone = sc.gs.light_sample_at(sc.ref, sc.light, sc.u)
        want, want_shadow, kind = restate_samples(sc, oracle, sc.ref, sc.light, sc.u)
        t = np.flatnonzero(want["visibility"] == 1)
        occ, _ = oracle.intersect_p(sc.desc, want_shadow[t, 0:3], want_shadow[t, 4:7], want_shadow[t, 3])  # Scene::IntersectP over the tester's rays
        want["visibility"][t] = 1 - occ.astype(np.int32)
        cache[name] = dict(sc=sc, got=got, got_shadow=got_shadow, alone=alone, want=want, want_shadow=want_shadow, kind=kind)
        return cache[name]
    yield case
    for c in cache.values(): c["sc"].close()


@pytest.mark.parametrize("name", CLOSED_FORM)
def test_samples_of_closed_form_lights_equal_the_restatement(closed_case, name):
    c = closed_case(name)
    assert c["got"].dtype == c["sc"].gpu.LIGHT_SAMPLE_DTYPE
    assert records_equal(c["got"], c["want"]), (name, first_difference(c["got"], c["want"]))
    assert c["got_shadow"].shape == (c["sc"].n, 8) and same_bits(c["got_shadow"], c["want_shadow"]), name
    assert records_equal(c["alone"], c["got"])  # shadow = NULL changes no record
    if name == "env_uniform_open":  # the EXT instantiation's arithmetic pin: Distribution2D, libm's sinf / cosf, the 1 x 1 MIPMap
        inf = c["kind"] == INFINITE
        assert inf.sum() >= 100 and (c["want"]["visibility"][inf] >= 0).sum() >= 100 and (c["want"]["visibility"][inf] == 1).sum() >= 50


def test_the_closed_form_reference_points_reach_every_case(closed_case):
    """What the inputs must reach over the whole set, decided by the restatement alone."""
    cases = [closed_case(name) for name in CLOSED_FORM]
    kind = np.concatenate([c["kind"] for c in cases])
    vis = np.concatenate([c["want"]["visibility"] for c in cases])
    for k in (POINT, SPOT, DISTANT, AREA):
        assert (kind == k).sum() >= 100, (k, (kind == k).sum())
    assert ((vis == 1) & (kind >= 0)).sum() >= 50 and ((vis == 0) & (kind >= 0)).sum() >= 50
    assert ((vis == -1) & (kind >= 0)).sum() >= 20  # a one-sided emitter from behind, a spot outside its cone, pdf == 0
    assert ((vis == -1) & (kind == AREA)).sum() >= 5 and ((vis == -1) & (kind == SPOT)).sum() >= 5
    assert (kind == -1).sum() >= 20 and (kind == -2).sum() >= 20
    u0 = np.concatenate([c["sc"].u[:, 0] for c in cases])
    assert ((u0 == 0) & (kind >= 0)).sum() >= 20 and ((u0 == _GS.ONE_MINUS_EPS) & (kind >= 0)).sum() >= 20


# ---- 3. every other light kind, by composition ---------------------------------------------------------------------------------------------------------------
OTHER_SCENES = ["light_projection", "light_gonio_power", "quadric_lights", "sphere_partial", "sphere_enclosing", "env_map"]


@pytest.fixture(scope="module")
def tested_by_kind():
    return {}


@pytest.mark.parametrize("name", OTHER_SCENES)
def test_other_light_kinds_compose_with_intersect_p_at(gpu, tested_by_kind, name):
    """Projection and goniometric lights, sphere / cylinder / disk emitters and a mapped environment have no restatement here: the bits of their Sample_Li stay
    pinned by the golden images, which are rendered through the same device functions (light_sample_li, shadow_ray_to).  Checked here: visibility is the
    any-hit answer of the very ray reported, untested samples report no ray, Li is black exactly where nothing is tested or pdf == 0, and a projection /
    goniometric light's tester ends at lights[].pos."""
    sc = Scene(gpu, name, seed=601 + OTHER_SCENES.index(name))
    rec, shadow = sc.gs.light_sample_at(sc.ref, sc.light, sc.u, with_shadow_rays=True)
    valid = rec["light"] >= 0
    assert np.array_equal(valid, (sc.ref["prim"] >= 0) & (sc.light >= 0) & (sc.light < sc.nl)) and np.array_equal(rec["light"][valid], sc.light[valid])
    tested = valid & (rec["visibility"] >= 0)
    rest = rec[~valid].copy()
    rest["light"] = 0
    assert not rest.view(np.uint8).any()  # no sample drawn: light = -1, every other field 0
    t = np.flatnonzero(tested)
    occ = sc.gs.intersect_p_at(shadow[t, 0:3], shadow[t, 4:7], shadow[t, 3], shadow[t, 7])
    assert np.array_equal(rec["visibility"][t], 1 - occ.astype(np.int32)), name
    assert (shadow[t, 3] == SHADOW_TMAX).all() and not shadow[~tested].any()
    black = (rec["Li"] == 0).all(1)
    assert np.array_equal(black[valid], ((rec["visibility"] == -1) | (rec["pdf"] == 0))[valid]), name
    assert not rec["reserved"].any() and (rec["pdf"][tested] > 0).all()
    kinds = sc.lights["type"][np.where(valid, sc.light, 0)]
    for kk in (PROJECTION, GONIO):
        m = valid & (kinds == kk)
        assert same_bits(rec["p_light"][m], sc.lights["pos"][sc.light[m]]) and not rec["n_light"][m].any() and (rec["pdf"][m] == 1).all()
    for li in range(sc.nl):
        key = {AREA: ("emitter", sc.emitter(li)), INFINITE: "infinite map"}.get(sc.lights["type"][li], int(sc.lights["type"][li]))
        tested_by_kind[key] = tested_by_kind.get(key, 0) + int((tested & (sc.light == li)).sum())
    sc.close()


def test_the_other_light_kinds_are_all_tested(tested_by_kind):
    """Over test_other_light_kinds_compose_with_intersect_p_at's scenes (which run before this one): every kind has at least 50 tested samples."""
    for key in (PROJECTION, GONIO, ("emitter", 0), ("emitter", 1), ("emitter", 2), "infinite map"):  # sphere, cylinder, disk
        assert tested_by_kind.get(key, 0) >= 50, (key, tested_by_kind)


# ---- 4. Pdf_Li ----------------------------------------------------------------------------------------------------------------------------------------------
PDF_SCENES = ["cornell_32", "cornell_spot_power", "directlighting/e_five_kinds_of_light", "cornell_twosided", "env_uniform_open"]


def test_pdf_li_equals_the_restatement(closed_case, oracle):
    nonzero = zero = infinite = delta = 0
    for name in PDF_SCENES:
        c = closed_case(name)
        sc, rec = c["sc"], c["got"]
        own = (np.arange(sc.n) % 2 == 0) & (rec["pdf"] > 0)  # the sample query's own wi for half the points, random directions for the rest
        wi = np.ascontiguousarray(np.where(own[:, None], rec["wi"], sc.wi_random), F32)
        before = sc.gs.counters()
        got = sc.gs.light_pdf_at(sc.ref, sc.light, wi)
        assert sc.gs.counters() == before  # this call moves no counter
        assert got.dtype == F32 and got.shape == (sc.n,)
        want = np.zeros(sc.n, F32)
        m = np.flatnonzero(c["kind"] == AREA)
        want[m] = restate_triangle_pdf(sc, oracle, sc.ref[m], sc.light[m], wi[m])
        nonzero += int((want[m] != 0).sum()); zero += int((want[m] == 0).sum())
        m = np.flatnonzero(c["kind"] == INFINITE)
        want[m] = restate_infinite_pdf(sc, sc.light[m], wi[m])
        infinite += int((want[m] > 0).sum())
        delta += int(np.isin(c["kind"], (POINT, SPOT, DISTANT)).sum())
        bad = np.flatnonzero(bits(got) != bits(want))
        assert len(bad) == 0, (name, len(bad), bad[:5], got[bad[:5]], want[bad[:5]], c["kind"][bad[:5]])
        assert not got[c["kind"] < 0].any() and not got[np.isin(c["kind"], (POINT, SPOT, DISTANT))].any()  # invalid inputs and delta lights: 0
    assert nonzero >= 100 and zero >= 100 and infinite >= 100 and delta >= 100, (nonzero, zero, infinite, delta)


def test_pdf_li_of_other_delta_lights_is_zero(gpu):
    sc = Scene(gpu, "light_gonio_power", seed=611)
    pdf = sc.gs.light_pdf_at(sc.ref, sc.light, sc.wi_random)
    assert np.isin(sc.lights["type"], (PROJECTION, GONIO)).sum() >= 2 and not pdf.any()
    sc.close()


# ---- 5. Le ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_32", "cornell_twosided", "cornell_point"])
def test_le_at_hits_is_the_area_lights_rule(gpu, name):
    sc = Scene(gpu, name, seed=701, extra_rays=light_rays(True))
    le, isect = sc.gs.light_le_at(sc.o, sc.d, sc.tmax, with_interaction=True)
    assert le.dtype == F32 and le.shape == (sc.n, 3)
    assert records_equal(isect, sc.ref)  # isect, when asked for, is pg_intersect_at's bytes
    assert same_bits(sc.gs.light_le_at(sc.o, sc.d, sc.tmax), le)
    emissive = (isect["prim"] >= 0) & (isect["light"] >= 0)
    l = sc.lights[np.where(emissive, isect["light"], 0)]
    lit = emissive & ((l["two_sided"] != 0) | (dot32(isect["n"], isect["wo"]) > 0))
    want = np.where(lit[:, None], l["L"], F32(0)).astype(F32)
    assert same_bits(le, want), name
    assert emissive.sum() >= 50 and (isect["prim"] < 0).sum() >= 20  # (no infinite light: a miss gives zeros, as `want` has them)
    one_sided = emissive & (l["two_sided"] == 0)
    if name != "cornell_twosided": assert (one_sided & lit).sum() >= 20 and (one_sided & ~lit).sum() >= 20  # seen from both sides
    else: assert not one_sided.any() and lit.sum() == emissive.sum()
    sc.close()


TWO_SKIES = """
LookAt 0 0 5  0 0 0  0 1 0
Camera "perspective" "float fov" [ 45 ]
Film "image" "integer xresolution" [ 8 ] "integer yresolution" [ 8 ] "string filename" "two_skies.pfm"
Sampler "halton" "integer pixelsamples" [ 1 ]
Integrator "path" "integer maxdepth" [ 2 ]
WorldBegin
AttributeBegin
  Rotate 40 1 0.2 0
  LightSource "infinite" "rgb L" [ 0.3 0.5 0.9 ]
AttributeEnd
AttributeBegin
  Rotate -75 0.1 1 0.4
  LightSource "infinite" "rgb L" [ 1.25 0.75 0.1 ] "rgb scale" [ 2 1 0.5 ]
AttributeEnd
LightSource "point" "point from" [ 0 3 0 ] "rgb I" [ 5 5 5 ]
Material "matte" "rgb Kd" [ 0.5 0.5 0.5 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ -1 -1 0  1 -1 0  1 1 0  -1 1 0 ]
WorldEnd
"""


def rays_at_the_quad(sc):
    rng = np.random.default_rng(6)
    o = np.stack([rng.uniform(-2, 2, 200), rng.uniform(-2, 2, 200), rng.uniform(1, 3, 200) * np.where(np.arange(200) % 2 == 0, 1, -1)], 1)
    q = np.stack([rng.uniform(-0.9, 0.9, 200), rng.uniform(-0.9, 0.9, 200), np.zeros(200)], 1)
    return o.astype(F32), (q - o).astype(F32)


def test_le_of_escaped_rays_sums_the_infinite_lights_in_order(gpu):
    sc = Scene(gpu, text=TWO_SKIES, seed=711, extra_rays=rays_at_the_quad)
    assert list(sc.lights["type"]) == [INFINITE, INFINITE, POINT]
    le, isect = sc.gs.light_le_at(sc.o, sc.d, sc.tmax, with_interaction=True)
    miss = isect["prim"] < 0
    assert miss.sum() >= 500 and (~miss).sum() >= 100
    want = np.zeros((sc.n, 3), F32)
    for li in (0, 1):  # path.cpp:81-85: L starts at 0, the lights add in lights[] order
        want[miss] = want[miss] + restate_infinite_le(sc, li, sc.d[miss])
    assert same_bits(le, want), np.flatnonzero((bits(le) != bits(want)).any(1))[:5]
    assert (le[miss] > 0).all() and not le[~miss].any()
    sc.close()


# ---- 6. time --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nest_motion(gpu):
    sc = Scene(gpu, "nest_motion", seed=801)
    yield sc
    sc.close()


def at_time(ref, time):
    r = ref.copy()
    r["time"] = time
    return r


def test_time_is_per_reference_point(nest_motion):
    sc = nest_motion
    even = np.arange(sc.n) % 2 == 0
    at0, sh0 = sc.gs.light_sample_at(at_time(sc.ref, F32(0)), sc.light, sc.u, with_shadow_rays=True)
    at1, sh1 = sc.gs.light_sample_at(at_time(sc.ref, F32(1)), sc.light, sc.u, with_shadow_rays=True)
    assert (at0["visibility"] != at1["visibility"]).sum() >= 16  # the case cannot pass with the time ignored
    mixed, shm = sc.gs.light_sample_at(at_time(sc.ref, np.where(even, F32(0), F32(1)).astype(F32)), sc.light, sc.u, with_shadow_rays=True)
    assert records_equal(mixed, np.where(even, at0, at1)) and same_bits(shm, np.where(even[:, None], sh0, sh1))
    tested = (at1["light"] >= 0) & (at1["visibility"] >= 0)
    assert tested.sum() >= 100 and (sh1[tested, 7] == 1).all() and not sh1[~tested].any()


# ---- 7. shapes and memory -----------------------------------------------------------------------------------------------------------------------------------
def test_batch_sizes_are_prefixes_of_one_batch(nest_motion):
    sc = nest_motion
    ref = at_time(sc.ref, np.random.default_rng(3).random(sc.n).astype(F32))
    wi = sc.wi_random
    whole, whole_sh = sc.gs.light_sample_at(ref, sc.light, sc.u, with_shadow_rays=True)
    whole_pdf = sc.gs.light_pdf_at(ref, sc.light, wi)
    whole_le = sc.gs.light_le_at(sc.o, sc.d, sc.tmax, ref["time"])
    for n in (1, 63, 257):
        part, part_sh = sc.gs.light_sample_at(ref[:n], sc.light[:n], sc.u[:n], with_shadow_rays=True)
        assert records_equal(part, whole[:n]) and same_bits(part_sh, whole_sh[:n]), n
        assert same_bits(sc.gs.light_pdf_at(ref[:n], sc.light[:n], wi[:n]), whole_pdf[:n]), n
        assert same_bits(sc.gs.light_le_at(sc.o[:n], sc.d[:n], sc.tmax[:n], ref["time"][:n]), whole_le[:n]), n


PAD = 256  # bytes the device arrays are longer than the results: guard bytes, to catch a write past them


def test_device_memory_equals_host_memory(nest_motion):
    sc = nest_motion
    n = 1000
    ref = at_time(sc.ref[:n], np.where(np.arange(n) % 2 == 0, F32(0), F32(1)).astype(F32))
    light, u, wi = (np.ascontiguousarray(a[:n]) for a in (sc.light, sc.u, sc.wi_random))
    o, d, tmax, time = (np.ascontiguousarray(a[:n]) for a in (sc.o, sc.d, sc.tmax, ref["time"]))
    host, host_sh = sc.gs.light_sample_at(ref, light, u, with_shadow_rays=True)
    host_pdf = sc.gs.light_pdf_at(ref, light, wi)
    host_le, host_isect = sc.gs.light_le_at(o, d, tmax, time, with_interaction=True)
    guard = lambda nbytes: np.full(nbytes + PAD, 0xAB, np.uint8)

    def check(dev, i, want):
        got = dev.get(i, np.uint8)
        w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert len(got) == len(w) + PAD and np.array_equal(got[:len(w)], w) and (got[len(w):] == 0xAB).all(), i
    dev = DeviceArrays()
    pref, plight, pu, pwi = (dev.put(a) for a in (ref, light, u, wi))  # 0 .. 3
    pout, psh = dev.put(guard(64 * n)), dev.put(guard(32 * n))  # 4, 5
    sc.gs.light_sample_at_device(n, pref, plight, pu, pout, psh)
    check(dev, 4, host); check(dev, 5, host_sh)
    pout2 = dev.put(guard(64 * n))  # 6
    sc.gs.light_sample_at_device(n, pref, plight, pu, pout2, None)  # shadow = NULL
    check(dev, 6, host); check(dev, 5, host_sh)
    ppdf = dev.put(guard(4 * n))  # 7
    sc.gs.light_pdf_at_device(n, pref, plight, pwi, ppdf)
    check(dev, 7, host_pdf)
    po, pd, pt, ptime = (dev.put(a) for a in (o, d, tmax, time))  # 8 .. 11
    ple, pisect = dev.put(guard(12 * n)), dev.put(guard(128 * n))  # 12, 13
    sc.gs.light_le_at_device(n, po, pd, pt, ptime, pisect, ple)
    check(dev, 12, host_le); check(dev, 13, host_isect)
    ple2 = dev.put(guard(12 * n))  # 14
    sc.gs.light_le_at_device(n, po, pd, pt, ptime, None, ple2)
    check(dev, 14, host_le); check(dev, 13, host_isect)
    for i, a in enumerate((ref, light, u, wi)):  # the inputs were only read
        assert np.array_equal(dev.get(i, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1))


SHADING = ("camera_rays", "mis_rays", "shade_launches", "resolve_launches", "shade_items")


def test_counters_misses_and_mismatched_lengths(nest_motion, gpu):
    sc = nest_motion
    gs = sc.gs
    # a batch of valid samples only (an invalid one reports visibility 0, like its other fields): shadow_rays grows by (visibility >= 0).sum()
    hits = np.flatnonzero(sc.ref["prim"] >= 0)
    gs.counters_reset()
    rec = gs.light_sample_at(sc.ref[hits], np.zeros(len(hits), np.int32), sc.u[hits])
    cn = gs.counters()
    assert (rec["light"] == 0).all() and (rec["visibility"] == -1).sum() >= 20
    assert cn["shadow_rays"] == (rec["visibility"] >= 0).sum() >= 500 and cn["shadow_launches"] == 1 and cn["shadow_node_visits"] > 0
    assert all(cn[k] == 0 for k in SHADING + ("closest_rays", "closest_launches", "closest_node_visits", "light_tri_tests"))
    # the mixed batch: invalid references and indices add nothing
    gs.counters_reset()
    rec = gs.light_sample_at(sc.ref, sc.light, sc.u)
    cn = gs.counters()
    assert cn["shadow_rays"] == ((rec["light"] >= 0) & (rec["visibility"] >= 0)).sum() >= 100 and cn["shadow_launches"] == 1 and cn["shadow_node_visits"] > 0
    assert all(cn[k] == 0 for k in SHADING + ("closest_rays", "closest_launches", "closest_node_visits", "light_tri_tests"))
    gs.light_pdf_at(sc.ref, sc.light, sc.wi_random)
    assert gs.counters() == cn  # Pdf_Li moves nothing
    gs.counters_reset()
    gs.light_le_at(sc.o, sc.d, sc.tmax)
    cn = gs.counters()
    assert cn["closest_rays"] == sc.n and cn["closest_launches"] == 1 and all(cn[k] == 0 for k in SHADING + ("shadow_rays", "shadow_launches"))
    # a batch whose every reference point is a miss: no ray is traced, every record is light = -1 and zeros
    miss = sc.ref[sc.ref["prim"] < 0]
    assert len(miss) >= 20
    gs.counters_reset()
    rec, shadow = gs.light_sample_at(miss, np.zeros(len(miss), np.int32), sc.u[:len(miss)], with_shadow_rays=True)
    assert (rec["light"] == -1).all() and not shadow.any()
    rest = rec.copy()
    rest["light"] = 0
    assert not rest.view(np.uint8).any()
    cn = gs.counters()
    assert cn["shadow_rays"] == 0 and cn["shadow_launches"] == 1 and cn["shadow_node_visits"] == 0 and cn["closest_rays"] == 0
    assert not gs.light_pdf_at(miss, np.zeros(len(miss), np.int32), sc.wi_random[:len(miss)]).any()
    # empty batches
    empty = gs.light_sample_at(sc.ref[:0], sc.light[:0], sc.u[:0])
    assert empty.dtype == gpu.LIGHT_SAMPLE_DTYPE and len(empty) == 0 and len(gs.light_pdf_at(sc.ref[:0], sc.light[:0], sc.wi_random[:0])) == 0
    assert gs.light_le_at(sc.o[:0], sc.d[:0], sc.tmax[:0]).shape == (0, 3) and gs.counters() == cn
    for call, args in ((gs.light_sample_at, (sc.ref, sc.light[:-1], sc.u)), (gs.light_sample_at, (sc.ref, sc.light, sc.u[:-1])),
                       (gs.light_pdf_at, (sc.ref, sc.light, sc.wi_random[:-1])), (gs.light_pdf_at, (sc.ref[:-1], sc.light, sc.wi_random)),
                       (gs.light_le_at, (sc.o, sc.d[:-1], sc.tmax))):
        with pytest.raises(ValueError):
            call(*args)
    assert gs.counters() == cn
