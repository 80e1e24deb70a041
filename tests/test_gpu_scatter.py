"""pg_scatter_f_at / pg_scatter_sample_at: BSDF::f, BSDF::Pdf and BSDF::Sample_f at the closest hits of a batch of rays (PgScatter, csrc/pg_scatter.h),
as PathIntegrator::Li sees the BSDF after ComputeScatteringFunctions(ray, arena, true) for a ray without differentials.

The reference for constant-parameter materials is a float32 NumPy restatement of BSDF::f / Pdf / Sample_f (reflection.cpp:680-796) around the oracle's
per-BxDF entries oracle_lobe_f_pdf / oracle_lobe_sample_f, fed from the scene description (materials[], bxdfs[]) and from the PgInteraction of the same
rays (wo, n, shading_n, shading_dpdu); every record of every ray is compared bit for bit.  Textured materials are pinned against constant twins and a
closed-form checkerboard; a bumped frame against its invariants.  tests/test_emulated_scatter.py runs this file without a GPU."""
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


_GI = _load("test_gpu_interactions.py")
scene_rays, DeviceArrays, same_bits, bits = _GI.scene_rays, _GI.DeviceArrays, _GI.same_bits, _GI.bits

BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_SPECULAR, BSDF_ALL = 1, 2, 16, 31
NON_SPECULAR = BSDF_ALL & ~BSDF_SPECULAR  # the mask EstimateDirect uses
MASKS = (BSDF_ALL, NON_SPECULAR, BSDF_REFLECTION | BSDF_SPECULAR)
# the BxDFType each constructor passes to BxDF() (reflection.h), by PgBxDFType 0 .. 9
TYPE_OF = np.array([0, 1 | 4, 2 | 4, 1 | 4, 1 | 16, 2 | 16, 1 | 2 | 16, 1 | 8, 2 | 8, 1 | 8], np.int32)
ONE_MINUS_EPS = np.nextafter(F32(1), F32(0))
PG_MAT_NONE, PG_MAT_TEXTURED = 0, 6
MAXB = 8  # PG_MAX_BXDFS
INV_PI = F32(0.31830988618379067154)


def records_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def struct_array(ptr, n, ctype):
    """n structures behind a ctypes pointer as a structured NumPy array (a view)."""
    if n == 0: return np.zeros(0, np.dtype(ctype))
    return np.frombuffer((ctype * n).from_address(C.addressof(ptr.contents)), dtype=np.dtype(ctype))


def ray_set(scene, seed, n_random=1500, aimed=512):
    """scene_rays' rays (n_random random + up to `aimed` aimed ones; one dropped where the sum is a multiple of 256: the batch never fills its blocks), an
    unnormalised wi and a Point2f per ray -- u[0] = 0 and 1 - eps among them."""
    o, d, tmax = scene_rays(scene, n_random, seed, aimed=aimed)
    if len(tmax) % 256 == 0: o, d, tmax = np.ascontiguousarray(o[:-1]), np.ascontiguousarray(d[:-1]), np.ascontiguousarray(tmax[:-1])
    n = len(tmax)
    assert n % 256 != 0
    rng = np.random.default_rng(seed + 1000)
    wi = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 2, (n, 1))).astype(F32)
    u = rng.random((n, 2)).astype(F32)
    u[::17, 0] = 0
    u[5::17, 0] = ONE_MINUS_EPS
    return o, d, tmax, wi, np.minimum(u, ONE_MINUS_EPS)


# ---- the restatement: float32, every operation in the order csrc/pg_device.h and csrc/pg_bxdf.h write it (the kernels are built without contraction) ----
def dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize32(a):  # geometry.h:984-986, :243-248: v * (1 / sqrt((x x + y y) + z z))
    inv = F32(1) / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a * inv[:, None]


def cross64(a, b):  # geometry.h:957-963: evaluated in double, rounded once
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F32)


class Bsdfs:
    """The BSDFs at the hits of one batch, as the restatement holds them: the frame (ns, ng = n, ss = Normalize(shading.dpdu), ts = Cross(ns, ss)) and wo from
    the PgInteraction records, the BxDF list from materials[] / bxdfs[].  Rows are the rays that hit a primitive with a material (`rows`)."""

    def __init__(self, pkg, oracle, desc, isect):
        self.L = oracle.lib()
        self.mats = struct_array(desc.materials, desc.n_materials, pkg.abi.PgMaterial)
        self.bx = struct_array(desc.bxdfs, desc.n_bxdfs, pkg.abi.PgBxDF)
        self.bx_addr = C.addressof(desc.bxdfs.contents) if desc.n_bxdfs else 0
        assert self.bx.dtype.itemsize == 120
        hit = isect["prim"] >= 0
        self.mat_type = np.where(hit, self.mats["type"][np.where(hit, isect["material"], 0)], -1)
        self.rows = np.flatnonzero(hit & (self.mat_type != PG_MAT_NONE))
        r = isect[self.rows]
        m = self.mats[r["material"]]
        self.first, self.nb, self.eta = m["first_bxdf"].astype(np.int64), m["n_bxdfs"].astype(np.int64), m["bsdf_eta"]
        self.ns, self.ng, self.wo = r["shading_n"], r["n"], r["wo"]
        self.ss = normalize32(r["shading_dpdu"])
        self.ts = cross64(self.ns, self.ss)
        self.wo_l = self.local(self.wo)
        N = len(self.rows)
        lobe = np.arange(MAXB)[None, :]
        self.present = lobe < self.nb[:, None]
        self.index = np.where(self.present, self.first[:, None] + lobe, 0)  # bxdfs[] index of lobe l of row i
        self.kind = np.where(self.present, self.bx["type"][self.index] if desc.n_bxdfs else 0, 0)  # PgBxDFType
        self.type = np.where(self.present, TYPE_OF[self.kind], 0)  # BxDFType bits
        self.types_word = (self.kind.astype(np.uint64) << (4 * np.arange(MAXB, dtype=np.uint64))[None, :]).sum(1).astype(np.uint32)
        assert N == 0 or self.kind[self.present].min() >= 1

    def local(self, v):  # BSDF::WorldToLocal: three dots
        return np.ascontiguousarray(np.stack([dot32(v, self.ss), dot32(v, self.ts), dot32(v, self.ns)], 1))

    def world(self, v):  # BSDF::LocalToWorld: (ss.x v.x + ts.x v.y) + ns.x v.z
        return (self.ss * v[:, 0:1] + self.ts * v[:, 1:2]) + self.ns * v[:, 2:3]

    def reflect(self, wi):  # the geometric-hemisphere rule: with n, not with ns
        return dot32(wi, self.ng) * dot32(self.wo, self.ng) > 0

    def lobes_f_pdf(self, wi_l, rows=None):
        """BxDF::f (ScaledBxDF factors applied, innermost first) and BxDF::Pdf of every BxDF of every row for (wo, wi) in the local frame."""
        N = len(self.rows)
        out = np.zeros((N, MAXB, 4), F32)
        fn, base, wo_a, wi_a, out_a = self.L.oracle_lobe_f_pdf, self.bx_addr, self.wo_l.ctypes.data, wi_l.ctypes.data, out.ctypes.data
        first, nb = self.first.tolist(), self.nb.tolist()
        for i in (range(N) if rows is None else rows.tolist()):
            for l in range(nb[i]):
                fn(base + 120 * (first[i] + l), wo_a + 12 * i, wi_a + 12 * i, out_a + 16 * (i * MAXB + l))
        f, pdf = out[:, :, 0:3].copy(), out[:, :, 3].copy()
        for l in range(MAXB):
            f[:, l] = self.scaled(f[:, l], self.index[:, l], self.present[:, l])
        return f, pdf

    def scaled(self, f, index, on):
        b = self.bx[index] if len(self.bx) else np.zeros(len(index), self.bx.dtype)
        for k in range(3):  # ScaledBxDF, reflection.cpp:98-107: scale * f, innermost wrapper first
            m = on & (b["n_scales"] > k)
            f = np.where(m[:, None], b["scale"][:, 3 * k:3 * k + 3] * f, f)
        return f

    def matching(self, flags):
        match = self.present & ((self.type & flags) == self.type)
        return match, match.sum(1)

    def records(self, pkg, isect, flags):
        """The fields of PgScatter that do not depend on the query."""
        want = np.zeros(len(isect), pkg.SCATTER_DTYPE)
        want["prim"] = isect["prim"]
        r = self.rows
        want["n_bxdfs"][r] = self.nb
        want["n_matching"][r] = self.matching(flags)[1]
        want["eta"][r] = self.eta
        want["shading_n"][r] = self.ns
        want["types"][r] = self.types_word
        return want

    def f_pdf(self, pkg, isect, wi, masks):
        """BSDF::f and BSDF::Pdf (reflection.cpp:680-693, :781-796) for every mask: {flags: records}."""
        wi = wi[self.rows]
        wi_l = self.local(wi)
        F, P = self.lobes_f_pdf(wi_l)
        reflect = self.reflect(wi)
        hemi = np.where(reflect[:, None], self.type & BSDF_REFLECTION, self.type & BSDF_TRANSMISSION) != 0
        nothing = self.wo_l[:, 2] == 0
        out = {}
        for flags in masks:
            match, m = self.matching(flags)
            f, pdf = np.zeros((len(wi), 3), F32), np.zeros(len(wi), F32)
            for l in range(MAXB):
                sel = match[:, l] & hemi[:, l]
                f = np.where(sel[:, None], f + F[:, l], f)
                pdf = np.where(match[:, l], pdf + P[:, l], pdf)
            with np.errstate(all="ignore"):
                pdf = np.where(m > 0, pdf / m.astype(F32), F32(0))
            f[nothing] = 0
            pdf[nothing] = 0
            want = self.records(pkg, isect, flags)
            want["f"][self.rows], want["pdf"][self.rows], want["wi"][self.rows] = f, pdf, wi
            out[flags] = want
        self.other_hemisphere = int((~reflect & ~nothing).sum())
        return out

    def sample_f(self, pkg, isect, u, flags):
        """BSDF::Sample_f (reflection.cpp:714-779); also returns the PgBxDFType of the sampled BxDF per row (0 = no sample)."""
        N = len(self.rows)
        u = u[self.rows]
        match, m = self.matching(flags)
        um = u[:, 0] * m.astype(F32)
        comp = np.minimum(np.floor(um).astype(np.int64), m - 1)  # min((int)floor(u0 * m), m - 1)
        chosen = np.argmax(match & (np.cumsum(match, 1) == (comp + 1)[:, None]), axis=1)
        u_remapped = np.minimum(um - comp.astype(F32), ONE_MINUS_EPS)
        active = (m > 0) & (self.wo_l[:, 2] != 0)
        s = np.zeros((N, 7), F32)
        s_type = np.zeros(N, np.int32)
        fn, base, wo_a, s_a = self.L.oracle_lobe_sample_f, self.bx_addr, self.wo_l.ctypes.data, s.ctypes.data
        idx = self.index[np.arange(N), chosen].tolist()
        u0, u1 = u_remapped.tolist(), u[:, 1].tolist()
        for i in np.flatnonzero(active).tolist():
            s_type[i] = fn(base + 120 * idx[i], wo_a + 12 * i, u0[i], u1[i], s_a + 28 * i)
        ok = active & (s[:, 3] != 0)
        f = self.scaled(s[:, 0:3], self.index[np.arange(N), chosen], ok)
        pdf = s[:, 3].copy()
        wi_l = np.ascontiguousarray(s[:, 4:7])
        wi = self.world(wi_l)
        specular = (self.type[np.arange(N), chosen] & BSDF_SPECULAR) != 0
        rest = ok & ~specular  # :760-775: the other matching BxDFs' pdfs, and f over the matching BxDFs of the hemisphere the pair is in
        F, P = self.lobes_f_pdf(wi_l, np.flatnonzero(rest))
        hemi = np.where(self.reflect(wi)[:, None], self.type & BSDF_REFLECTION, self.type & BSDF_TRANSMISSION) != 0
        f2 = np.zeros((N, 3), F32)
        for l in range(MAXB):
            f2 = np.where((match[:, l] & hemi[:, l])[:, None], f2 + F[:, l], f2)
            pdf = np.where(rest & match[:, l] & (chosen != l) & (m > 1), pdf + P[:, l], pdf)
        f = np.where(rest[:, None], f2, f)
        with np.errstate(all="ignore"):
            pdf = np.where(m > 1, pdf / m.astype(F32), pdf)
        want = self.records(pkg, isect, flags)
        r = self.rows[ok]
        want["f"][r], want["pdf"][r], want["wi"][r], want["sampled_type"][r] = f[ok], pdf[ok], wi[ok], s_type[ok]
        return want, np.where(ok, self.kind[np.arange(N), chosen], 0), int((active & ~ok).sum())


def first_difference(got, want):
    for name in got.dtype.names:
        bad = np.flatnonzero((bits(got[name]).reshape(len(got), -1) != bits(want[name]).reshape(len(want), -1)).any(1))
        if len(bad): return f"{name}: {len(bad)} rays differ, first ray {bad[0]}: got {got[name][bad[0]]}, want {want[name][bad[0]]}"
    return "equal"


# ---- 1. constant materials = the restatement over the oracle's lobes -------------------------------------------------------------------------------------
# (cornell_orennayar beside the scenes of the issue: no other of them has an OrenNayar BxDF to sample)
CONSTANT_SCENES = ["cornell_plastic", "cornell_mirror_glass", "mat_uber", "mat_metal", "mat_substrate", "mat_translucent", "mat_roughglass", "mat_mix", "quadrics",
                   "instance_boxes", "cornell_orennayar"]
SEEDS = {name: 301 + k for k, name in enumerate(CONSTANT_SCENES)}


@pytest.fixture(scope="module")
def constant_case(gpu, oracle):
    """name -> what one scene's ray set gave on the device and in the restatement (computed once per scene, kept for the test of the whole set)."""
    cache = {}

    def case(name):
        if name in cache: return cache[name]
        scene = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
        desc = scene.desc
        gs = gpu.GpuScene(desc)
        o, d, tmax, wi, u = ray_set(scene, SEEDS[name])
        isect = gs.intersect_at(o, d, tmax)
        got_f = {fl: gs.scatter_f_at(o, d, tmax, wi, flags=fl) for fl in MASKS}
        got_s = {fl: gs.scatter_sample_at(o, d, tmax, u, flags=fl) for fl in MASKS}
        gs.close()
        b = Bsdfs(gpu, oracle, desc, isect)
        assert (b.mat_type != PG_MAT_TEXTURED).all()
        want_f = b.f_pdf(gpu, isect, wi, MASKS)
        out = {"n": len(tmax), "hits": int((isect["prim"] >= 0).sum()), "other_hemisphere": b.other_hemisphere, "sampled": np.zeros(10, np.int64), "no_sample": 0,
               "got_f": got_f, "got_s": got_s, "want_f": want_f, "want_s": {}, "scales": np.bincount(b.bx["n_scales"][b.index[b.present]], minlength=4) if len(b.bx) else np.zeros(4, int)}
        for fl in MASKS:
            want, kinds, failed = b.sample_f(gpu, isect, u, fl)
            out["want_s"][fl] = want
            out["sampled"] += np.bincount(kinds, minlength=10)
            out["no_sample"] += failed
        cache[name] = out
        scene.close()
        return out
    return case


@pytest.mark.parametrize("name", CONSTANT_SCENES)
def test_constant_materials_equal_the_restatement(constant_case, name):
    c = constant_case(name)
    assert c["hits"] > c["n"] // 2 and c["hits"] < c["n"]
    for fl in MASKS:  # every record of every ray: hits, misses, rays whose wo lies in the tangent plane
        assert records_equal(c["got_f"][fl], c["want_f"][fl]), (name, "f / Pdf", fl, first_difference(c["got_f"][fl], c["want_f"][fl]))
        assert records_equal(c["got_s"][fl], c["want_s"][fl]), (name, "Sample_f", fl, first_difference(c["got_s"][fl], c["want_s"][fl]))
        assert not c["got_f"][fl]["sampled_type"].any()
    if name == "mat_mix":  # mixA and mixSpec wrap their BxDFs once, mixNested wraps mixA's twice: the scene has both
        assert c["scales"][1] > 0 and c["scales"][2] > 0 and c["scales"][3] == 0, c["scales"]
    else: assert c["scales"][1:].sum() == 0


def test_the_constant_ray_sets_cover_the_library(constant_case):
    """What the ray sets must reach, over the whole set (decided by the restatement alone): every BxDF of the ABI sampled, pairs in the other geometric
    hemisphere -- wi beyond the surface as n sees it, where BSDF::f sums the transmissive BxDFs --, and samples the BxDF refused (pdf == 0)."""
    cases = [constant_case(name) for name in CONSTANT_SCENES]
    assert sum(c["hits"] for c in cases) > sum(c["n"] for c in cases) // 2
    sampled = sum(c["sampled"] for c in cases)
    assert (sampled[1:10] >= 20).all(), sampled
    assert sum(c["other_hemisphere"] for c in cases) >= 50
    assert sum(c["no_sample"] for c in cases) >= 20, [c["no_sample"] for c in cases]


# ---- 2. the interaction output ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_32", "quadrics", "nest_motion"])
def test_interactions_beside_the_records_are_intersect_ats(gpu, name):
    scene = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
    gs = gpu.GpuScene(scene.desc)
    o, d, tmax, wi, u = ray_set(scene, 41)
    time = np.random.default_rng(42).random(len(tmax)).astype(F32)
    isect = gs.intersect_at(o, d, tmax, time)
    assert (isect["prim"] >= 0).mean() > 0.5
    if name == "nest_motion": assert (isect["instance_inner"] >= 0).sum() > 20
    for call, arg in ((gs.scatter_f_at, wi), (gs.scatter_sample_at, u)):
        rec, with_isect = call(o, d, tmax, arg, time=time, flags=BSDF_ALL, with_interaction=True)
        assert with_isect.dtype == gpu.INTERACTION_DTYPE and records_equal(with_isect, isect)
        alone = call(o, d, tmax, arg, time=time, flags=BSDF_ALL)
        assert alone.dtype == gpu.SCATTER_DTYPE and records_equal(alone, rec)
        assert np.array_equal(rec["prim"], isect["prim"]) and (rec["n_bxdfs"][rec["prim"] >= 0] >= 1).all()
    gs.close()


# ---- 3. textured = constant where the texture is constant ---------------------------------------------------------------------------------------------------
QUADS_HEAD = """
LookAt 0 0 -6  0 0 0  0 1 0
Camera "perspective" "float fov" [ 45 ]
Film "image" "integer xresolution" [ 8 ] "integer yresolution" [ 8 ] "string filename" "quads.pfm"
WorldBegin
LightSource "point" "point from" [ 0 0 -5 ]
"""
QUAD = 'Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ %s ] "float uv" [ 0 0  1 0  1 1  0 1 ]\n'
QUAD_P = ["-2.2 -2.2 0  -0.1 -2.2 0.3  -0.1 -0.1 0  -2.2 -0.1 -0.2", "0.1 -2.2 0  2.2 -2.2 0  2.2 -0.1 0.4  0.1 -0.1 0", "-2.2 0.1 0.2  -0.1 0.1 0  -0.1 2.2 0  -2.2 2.2 0",
          "0.1 0.1 0  2.2 0.1 -0.3  2.2 2.2 0  0.1 2.2 0.1"]
# every spectrum ("rgb") and float parameter of the four materials
QUAD_MATERIALS = [
    ("plastic", [("rgb", "Kd", "0.3 0.5 0.2"), ("rgb", "Ks", "0.4 0.3 0.2"), ("float", "roughness", "0.15")]),
    ("uber", [("rgb", "Kd", "0.3 0.5 0.2"), ("rgb", "Ks", "0.35 0.3 0.25"), ("rgb", "Kr", "0.2 0.2 0.3"), ("rgb", "Kt", "0.4 0.4 0.5"), ("rgb", "opacity", "0.6 0.7 0.9"),
              ("float", "uroughness", "0.05"), ("float", "vroughness", "0.3"), ("float", "eta", "1.3")]),
    ("glass", [("rgb", "Kr", "0.9 0.8 0.7"), ("rgb", "Kt", "0.7 0.9 0.8"), ("float", "uroughness", "0.1"), ("float", "vroughness", "0.35"), ("float", "eta", "1.4")]),
    ("metal", [("rgb", "eta", "1.5 0.4 0.3"), ("rgb", "k", "1.8 2.5 3"), ("float", "uroughness", "0.02"), ("float", "vroughness", "0.2")])]


def quads_scene(textured):
    """Four quads with plastic, uber, rough glass and metal: every parameter a 2D checkerboard ("aamode" "none") whose two values are equal, or -- the twin --
    the same values as literals."""
    text = QUADS_HEAD
    for q, (mat, params) in enumerate(QUAD_MATERIALS):
        words = []
        for k, (kind, name, value) in enumerate(params):
            if textured:
                tex = f"t{q}_{k}"
                text += (f'Texture "{tex}" "{"spectrum" if kind == "rgb" else "float"}" "checkerboard" "string aamode" "none" "float uscale" [ {3 + k} ] "float vscale" [ {2 + q} ] '
                         f'"{kind} tex1" [ {value} ] "{kind} tex2" [ {value} ]\n')
                words.append(f'"texture {name}" "{tex}"')
            else: words.append(f'"{kind} {name}" [ {value} ]')
        text += f'AttributeBegin\n  Material "{mat}" ' + " ".join(words) + "\n  " + QUAD % QUAD_P[q] + "AttributeEnd\n"
    return text + "WorldEnd\n"


def aimed_rays(scene, n, seed, box=((-3, -3, -6), (3, 3, -2)), both_sides=True):
    """n rays from a box in front of (and, every third, mirrored behind) the z = 0 plane towards random points of the scene's triangles; then wi and u."""
    desc = scene.desc
    rng = np.random.default_rng(seed)
    P = np.ctypeslib.as_array(desc.P, (desc.n_verts, 3))
    idx = np.ctypeslib.as_array(desc.indices, (desc.n_tris, 3))
    k = rng.integers(0, desc.n_tris, n)
    w = rng.dirichlet([1, 1, 1], n)
    target = w[:, 0:1] * P[idx[k, 0]] + w[:, 1:2] * P[idx[k, 1]] + w[:, 2:3] * P[idx[k, 2]]
    o = rng.uniform(box[0], box[1], (n, 3))
    if both_sides: o[::3, 2] = -o[::3, 2]
    o = o.astype(F32)
    d = (target - o).astype(F32)
    wi = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 2, (n, 1))).astype(F32)
    u = np.minimum(rng.random((n, 2)).astype(F32), ONE_MINUS_EPS)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.full(n, np.inf, F32), wi, u


def test_textured_materials_with_constant_textures_equal_their_constant_twins(gpu):
    """MatEval on the device (csrc/pg_material.h: the textures evaluated at the hit, roughness_to_alpha, the BxDFs in Add() order) builds the list the host
    builds for the same values: the records of both queries are the same bytes, under every mask."""
    out = {}
    for textured in (True, False):
        scene = gpu.HostScene(text=quads_scene(textured))
        desc = scene.desc
        assert desc.n_tris == 8 and desc.n_instances == 0
        types = struct_array(desc.materials, desc.n_materials, gpu.abi.PgMaterial)["type"]
        tri_mat = np.ctypeslib.as_array(desc.tri_material, (desc.n_tris,))
        assert (types[tri_mat] == PG_MAT_TEXTURED).all() if textured else not (types == PG_MAT_TEXTURED).any()
        assert (desc.n_textured == 4) if textured else (desc.n_textured == 0)
        gs = gpu.GpuScene(desc)
        o, d, tmax, wi, u = aimed_rays(scene, 1999, 77)
        isect = gs.intersect_at(o, d, tmax)
        out[textured] = (isect, [gs.scatter_f_at(o, d, tmax, wi, flags=fl) for fl in MASKS], [gs.scatter_sample_at(o, d, tmax, u, flags=fl) for fl in MASKS],
                         tri_mat[np.maximum(isect["prim"], 0)].copy())
        gs.close()
    (ia, fa, sa, ma), (ib, fb, sb, mb) = out[True], out[False]
    hit = ia["prim"] >= 0
    assert hit.sum() > 1900 and np.array_equal(ia["prim"], ib["prim"])  # the same geometry: the same primitives
    assert np.array_equal(ma, mb) and len(np.unique(ma[hit])) == 4
    for mat in np.unique(ma[hit]):  # every quad is hit often, from both sides
        on = hit & (ma == mat)
        assert on.sum() > 300 and (ia["wo"][on, 2] > 0).sum() > 50 and (ia["wo"][on, 2] < 0).sum() > 50
    assert len(set(fa[0]["n_bxdfs"][hit])) >= 3 and fa[0]["n_bxdfs"][hit].max() >= 4
    for a, b in zip(fa + sa, fb + sb):
        assert records_equal(a, b), first_difference(a, b)
    assert sum(int((s["pdf"] != 0).sum()) for s in sa) > 3000 and (fa[0]["pdf"] != 0).sum() > 1000


# ---- 4. textured with two values ----------------------------------------------------------------------------------------------------------------------------
CHECKER_KD = (F32([0.8, 0.7, 0.6]), F32([0.1, 0.2, 0.5]))
CHECKER_SCENE = QUADS_HEAD + """
Texture "chk" "spectrum" "checkerboard" "string aamode" "none" "float uscale" [ 5 ] "float vscale" [ 3 ] "float udelta" [ 0.25 ]
  "rgb tex1" [ 0.8 0.7 0.6 ] "rgb tex2" [ 0.1 0.2 0.5 ]
Material "matte" "texture Kd" "chk"
""" + QUAD % "-2 -2 0  2 -2 0.5  2 2 0  -2 2 -0.5" + "WorldEnd\n"


def test_a_checkerboard_of_two_colours_selects_kd_by_the_closed_form(gpu):
    """One matte quad under a two-colour checkerboard without antialiasing: with wi on wo's side, f = Kd_k * InvPi (LambertianReflection::f) for the k that
    UVMapping2D::Map and Checkerboard2DTexture::Evaluate (textures/checkerboard.h:58-64) select at the record's uv: s = su u + du, t = sv v + dv,
    k = (floor(s) + floor(t)) % 2 -- in float32, as written."""
    scene = gpu.HostScene(text=CHECKER_SCENE)
    desc = scene.desc
    assert struct_array(desc.materials, desc.n_materials, gpu.abi.PgMaterial)["type"][desc.tri_material[0]] == PG_MAT_TEXTURED
    gs = gpu.GpuScene(desc)
    o, d, tmax, _, _ = aimed_rays(scene, 1001, 5)
    rec, isect = gs.scatter_f_at(o, d, tmax, -d, flags=BSDF_ALL, with_interaction=True)  # wi = -ray.d: wo's own direction, not normalised
    gs.close()
    hit = rec["prim"] >= 0
    assert hit.sum() > 950
    r, uv = rec[hit], isect["uv"][hit]
    s, t = F32(5) * uv[:, 0] + F32(0.25), F32(3) * uv[:, 1] + F32(0)
    assert s.dtype == F32 and t.dtype == F32
    k = (np.floor(s).astype(np.int64) + np.floor(t).astype(np.int64)) % 2
    want = np.where((k == 0)[:, None], CHECKER_KD[0] * INV_PI, CHECKER_KD[1] * INV_PI)
    assert want.dtype == F32 and same_bits(r["f"], want)
    assert (k == 0).sum() >= 100 and (k == 1).sum() >= 100
    assert (r["n_bxdfs"] == 1).all() and (r["types"] == 1).all() and (r["eta"] == 1).all() and (r["n_matching"] == 1).all()


# ---- 5. bump mapping ----------------------------------------------------------------------------------------------------------------------------------------
def test_bumped_frames_are_consistent(gpu):
    """Scene bump_maps: shading_n is the BSDF's ns after Material::Bump.  No reference value exists for a bumped frame short of a render -- the oracle has no
    entry for Material::Bump alone --, so this test pins the frame's invariants only: a unit normal on n's side that differs from Scene::Intersect's, and a
    BSDF that is evaluated in it.  The bit-level pin of material_bump remains the golden images (tests/test_gpu_parity.py: bump_maps)."""
    scene = gpu.HostScene(os.path.join(GOLD, "bump_maps.pbrt"))
    gs = gpu.GpuScene(scene.desc)
    o, d, tmax, wi, u = ray_set(scene, 61)
    rec, isect = gs.scatter_f_at(o, d, tmax, wi, flags=BSDF_ALL, with_interaction=True)
    smp = gs.scatter_sample_at(o, d, tmax, u, flags=BSDF_ALL)
    gs.close()
    hit = (rec["prim"] >= 0) & (rec["n_bxdfs"] > 0)
    assert hit.sum() > len(tmax) // 2
    r, it = rec[hit], isect[hit]
    ns = r["shading_n"].astype(np.float64)
    length = np.sqrt((ns * ns).sum(1))
    print("bump_maps: max | |shading_n| - 1 | =", np.abs(length - 1).max() / 2.0 ** -23, "ulp of 1")
    assert np.abs(length - 1).max() <= 2 * 2.0 ** -23  # unit to 2 ulp
    assert ((ns * it["n"].astype(np.float64)).sum(1) >= 0).all()  # Faceforward(ns, n)
    bumped = (bits(r["shading_n"]) != bits(it["shading_n"])).any(1)
    print("bump_maps:", int(bumped.sum()), "of", int(hit.sum()), "hits have a bumped shading normal")
    assert bumped.sum() >= 100
    assert same_bits(smp["shading_n"], rec["shading_n"]) and np.array_equal(smp["types"], rec["types"])
    lambert = (r["n_bxdfs"] == 1) & (r["types"] == 1)
    assert (lambert & bumped).sum() >= 50
    same_side = dot32(wi[hit], it["n"]) * dot32(it["wo"], it["n"]) > 0
    in_plane = dot32(it["wo"], r["shading_n"]) == 0  # BSDF::f: wo.z == 0 gives nothing
    nonzero = (r["f"] != 0).any(1)
    assert np.array_equal(nonzero[lambert], (same_side & ~in_plane)[lambert])


# ---- 6. time ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nest_motion(gpu):
    scene = gpu.HostScene(os.path.join(GOLD, "nest_motion.pbrt"))
    gs = gpu.GpuScene(scene.desc)
    yield gs, ray_set(scene, 71)
    gs.close()


def test_time_is_per_ray(nest_motion):
    gs, (o, d, tmax, wi, u) = nest_motion
    n = len(tmax)
    even = np.arange(n) % 2 == 0
    time = np.where(even, F32(0), F32(1)).astype(F32)
    for call, arg in ((gs.scatter_f_at, wi), (gs.scatter_sample_at, u)):
        at0, at1 = (call(o, d, tmax, arg, time=np.full(n, t, F32), flags=BSDF_ALL) for t in (0, 1))
        assert (at0["prim"] != at1["prim"]).sum() >= 64  # the case cannot pass with the time ignored
        mixed = call(o, d, tmax, arg, time=time, flags=BSDF_ALL)
        assert records_equal(mixed, np.where(even, at0, at1))
        assert records_equal(call(o, d, tmax, arg, flags=BSDF_ALL), at0)  # time=None equals zeros


# ---- 7. shapes and memory -------------------------------------------------------------------------------------------------------------------------------------
def test_batch_sizes_are_prefixes_of_one_batch(nest_motion):
    gs, (o, d, tmax, wi, u) = nest_motion
    time = np.random.default_rng(3).random(len(tmax)).astype(F32)
    for call, arg in ((gs.scatter_f_at, wi), (gs.scatter_sample_at, u)):
        whole, whole_isect = call(o, d, tmax, arg, time=time, flags=NON_SPECULAR, with_interaction=True)
        for n in (1, 63, 257):
            part, part_isect = call(o[:n], d[:n], tmax[:n], arg[:n], time=time[:n], flags=NON_SPECULAR, with_interaction=True)
            assert records_equal(part, whole[:n]) and records_equal(part_isect, whole_isect[:n]), n


PAD = 256  # bytes the device arrays are longer than the results: guard words, to catch a write past them


def test_device_memory_equals_host_memory(nest_motion, gpu):
    gs, rays = nest_motion
    n = 1000
    o, d, tmax, wi, u = (np.ascontiguousarray(x[:n]) for x in rays)
    time = np.where(np.arange(n) % 2 == 0, F32(0), F32(1)).astype(F32)
    for host_call, device_call, arg in ((gs.scatter_f_at, gs.scatter_f_at_device, wi), (gs.scatter_sample_at, gs.scatter_sample_at_device, u)):
        host, host_isect = host_call(o, d, tmax, arg, time=time, flags=BSDF_ALL, with_interaction=True)
        dev = DeviceArrays()
        po, pd, pt, ptime, parg = (dev.put(a) for a in (o, d, tmax, time, arg))
        pout = dev.put(np.full(64 * n + PAD, 0xAB, np.uint8))
        pisect = dev.put(np.full(128 * n + PAD, 0xAB, np.uint8))
        device_call(n, po, pd, pt, ptime, parg, BSDF_ALL, pisect, pout)
        out, isect = dev.get(5, np.uint8), dev.get(6, np.uint8)
        assert np.array_equal(out[:64 * n], host.view(np.uint8)) and (out[64 * n:] == 0xAB).all() and len(out) == 64 * n + PAD
        assert np.array_equal(isect[:128 * n], host_isect.view(np.uint8)) and (isect[128 * n:] == 0xAB).all()
        pout2 = dev.put(np.full(64 * n + PAD, 0xAB, np.uint8))
        device_call(n, po, pd, pt, None, parg, BSDF_ALL, None, pout2)  # no times, no interactions
        out2 = dev.get(7, np.uint8)
        assert np.array_equal(out2[:64 * n], host_call(o, d, tmax, arg, flags=BSDF_ALL).view(np.uint8)) and (out2[64 * n:] == 0xAB).all()
        assert (dev.get(6, np.uint8)[128 * n:] == 0xAB).all()


def test_a_batch_of_misses_an_empty_batch_and_the_counters(nest_motion, gpu):
    gs, _ = nest_motion
    rng = np.random.default_rng(4)
    n = 300
    o = np.stack([rng.uniform(-500, 1000, n), rng.uniform(2000, 3000, n), rng.uniform(-500, 1000, n)], 1).astype(F32)
    d = np.stack([rng.normal(size=n), rng.uniform(0.1, 1, n), rng.normal(size=n)], 1).astype(F32)  # above the room, going up
    tmax = np.where(np.arange(n) % 2 == 0, F32(np.inf), rng.uniform(1, 5000, n)).astype(F32)
    wi, u = rng.normal(size=(n, 3)).astype(F32), rng.random((n, 2)).astype(F32)
    lib = gpu.gpu_lib()
    for call, arg, fn in ((gs.scatter_f_at, wi, lib.pg_scatter_f_at), (gs.scatter_sample_at, u, lib.pg_scatter_sample_at)):
        gs.counters_reset()
        rec = call(o, d, tmax, arg, flags=BSDF_ALL)
        assert (rec["prim"] == -1).all()
        rest = rec.copy()
        rest["prim"] = 0
        assert not rest.view(np.uint8).any()  # a miss: every other field is 0
        cn = gs.counters()
        assert cn["closest_rays"] == n and cn["closest_launches"] == 1 and cn["closest_node_visits"] > 0
        assert all(cn[k] == 0 for k in ("shadow_rays", "shadow_launches", "camera_rays", "mis_rays", "shade_launches", "resolve_launches", "shade_items"))
        before = gs.counters()
        empty = call(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros((0, len(arg[0])), F32), flags=BSDF_ALL)
        assert empty.dtype == gpu.SCATTER_DTYPE and len(empty) == 0
        assert fn(gs._h, 0, None, None, None, None, None, 31, None, None, 0, None) == 0  # n == 0 touches nothing, not even its arguments
        out = np.zeros(4, gpu.SCATTER_DTYPE)
        P = lambda a: a.ctypes.data
        assert fn(gs._h, 4, P(o), P(d), P(tmax), None, P(arg), 32, None, P(out), gpu.PG_MEM_HOST, None) == -1 and b"flags" in lib.pg_last_error()
        assert fn(gs._h, 4, P(o), P(d), P(tmax), None, None, 31, None, P(out), gpu.PG_MEM_HOST, None) == -1
        assert gs.counters() == before and not out.view(np.uint8).any()  # no device work followed
        with pytest.raises(ValueError):
            call(o, d, tmax, arg[:-1], flags=BSDF_ALL)


def test_a_boundary_without_material_has_no_bsdf(gpu):
    """vol_path_none: the smoke's sphere and the thin medium's box are medium boundaries (Material "none" / ""): the hit is reported, a BSDF is not."""
    scene = gpu.HostScene(os.path.join(GOLD, "vol_path_none.pbrt"))
    desc = scene.desc
    gs = gpu.GpuScene(desc)
    o, d, tmax, wi, u = ray_set(scene, 81)
    types = struct_array(desc.materials, desc.n_materials, gpu.abi.PgMaterial)["type"]
    for rec, isect in (gs.scatter_f_at(o, d, tmax, wi, with_interaction=True), gs.scatter_sample_at(o, d, tmax, u, with_interaction=True)):
        hit = rec["prim"] >= 0
        boundary = hit & (types[np.maximum(isect["material"], 0)] == PG_MAT_NONE)
        assert boundary.sum() >= 50 and (hit & ~boundary).sum() >= 500
        rest = rec[boundary].copy()
        assert (rest["prim"] >= 0).all() and np.array_equal(rest["prim"], isect["prim"][boundary])
        rest["prim"] = 0
        assert not rest.view(np.uint8).any()  # n_bxdfs = 0 and the rest 0
        assert (rec["n_bxdfs"][hit & ~boundary] >= 1).all() and (rec["eta"][hit & ~boundary] == 1).all()
    gs.close()
