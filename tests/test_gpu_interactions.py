"""pg_intersect_at / pg_intersect_p_at: batched Scene::Intersect / IntersectP with Ray::time, returning the SurfaceInteraction (PgInteraction,
csrc/pg_interaction.h).  Against the oracle at time 0, against closed forms in float32 NumPy for the fields the oracle has no entry for, and --
what an implementation that forwards to the time-0 launches of pg_intersect would fail -- against static scenes at the two ends of a motion.
Section 5b: pg_intersect / pg_intersect_p, which go through the same device path, with host and with device memory.
tests/test_emulated_interactions.py runs a subset of this file without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("PBRT_EMULATED_DEVICE") == "1"
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def scene_rays(scene, n_random, seed, aimed=512):
    """n_random rays from around the scene's bounds in random directions (some axis-parallel), then up to `aimed` rays from inside the bounds towards the
    centroids of top-level triangles, so that most rays hit; a fifth of the rays end at a finite tMax."""
    rng = np.random.default_rng(seed)
    desc = scene.desc
    nodes = scene.nodes()
    lo, hi = nodes["bmin"][0], nodes["bmax"][0]
    ext = hi - lo
    o = (lo - 0.1 * ext + 1.2 * ext * rng.random((n_random, 3))).astype(F32)
    d = rng.normal(size=(n_random, 3)).astype(F32)
    d[: n_random // 20, 0] = 0
    d[n_random // 20: n_random // 10, 1:] = 0
    flags = np.ctypeslib.as_array(desc.tri_flags, (desc.n_prims_all,))[: desc.n_tris]
    tris = np.flatnonzero((flags & (32 | 64)) == 0)
    if len(tris):
        tris = tris[rng.permutation(len(tris))[:aimed]]
        idx = np.ctypeslib.as_array(desc.indices, (desc.n_prims_all, 3))[tris]
        P = np.ctypeslib.as_array(desc.P, (desc.n_verts, 3))
        c = (P[idx[:, 0]] + P[idx[:, 1]] + P[idx[:, 2]]) / F32(3)
        o2 = (lo + ext * (0.1 + 0.8 * rng.random((len(tris), 3)))).astype(F32)
        o, d = np.concatenate([o, o2]), np.concatenate([d, (c - o2).astype(F32)])
    tmax = np.full(len(o), np.inf, F32)
    tmax[::5] = F32(0.8) * np.sqrt((ext * ext).sum(), dtype=F32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), tmax


def oracle_interactions(oracle, desc, o, d, tmax):
    """oracle_intersect_interaction ray by ray (time 0): hit mask, t and {p, pError, n}."""
    lib = oracle.lib()
    n = len(tmax)
    hit = np.zeros(n, bool); t = np.zeros(n, F32); out = np.zeros((n, 9), F32)
    tt = C.c_float(0)
    for i in range(n):
        hit[i] = lib.oracle_intersect_interaction(desc, o[i].ctypes.data, d[i].ctypes.data, float(tmax[i]), C.byref(tt), out[i].ctypes.data) != 0
        t[i] = tt.value
    return hit, t, out


def check_against_oracle(oracle, desc, o, d, tmax, rec):
    """prim and t are oracle.intersect's; p, p_error and n are oracle_intersect_interaction's, in every bit."""
    oprim, ot, _, _ = oracle.intersect(desc, o, d, tmax)
    assert np.array_equal(rec["prim"], oprim) and same_bits(rec["t"], ot)
    hit, t, out = oracle_interactions(oracle, desc, o, d, tmax)
    assert np.array_equal(hit, rec["prim"] >= 0) and same_bits(rec["t"][hit], t[hit])
    assert same_bits(rec["p"][hit], out[hit, 0:3]) and same_bits(rec["p_error"][hit], out[hit, 3:6]) and same_bits(rec["n"][hit], out[hit, 6:9])


# ---- 1. time 0 against the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_32", "quadrics", "instance_boxes", "nest_motion"])
def test_time_zero_equals_the_oracle(gpu, oracle, name):
    scene = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
    desc = scene.desc
    gs = gpu.GpuScene(desc)
    o, d, tmax = scene_rays(scene, 2048, 11)
    rec = gs.intersect_at(o, d, tmax)
    assert rec.dtype == gpu.INTERACTION_DTYPE and len(rec) == len(tmax)
    hit = rec["prim"] >= 0
    assert hit.mean() > 0.5 and (~hit).any()
    flags = np.ctypeslib.as_array(desc.tri_flags, (desc.n_prims_all,))
    if name == "quadrics": assert ((flags[rec["prim"][hit]] & 32) != 0).sum() > 50
    if name in ("instance_boxes", "nest_motion"): assert (rec["instance"][hit] >= 0).sum() > 100 and (rec["instance"][hit] < 0).any()
    if name == "nest_motion": assert (rec["instance_inner"][hit] >= 0).sum() > 20
    else: assert (rec["instance_inner"][hit] == -1).all()
    if name == "cornell_32": assert (rec["instance"][hit] == -1).all()
    check_against_oracle(oracle, desc, o, d, tmax, rec)
    occ = gs.intersect_p_at(o, d, tmax)
    oocc, _ = oracle.intersect_p(desc, o, d, tmax)
    assert occ.dtype == np.uint8 and np.array_equal(occ, oocc) and np.array_equal(occ != 0, hit)
    prim, t, _ = gs.intersect(o, d, tmax)  # the unchanged unit entry point
    assert np.array_equal(rec["prim"], prim) and same_bits(rec["t"], t)
    gs.close()


# ---- 2. the fields the oracle has no entry for, against closed forms ---------------------------------------------------------------------------------
CLOSED_FORM_SCENE = """
LookAt 0 0 -6  0 0 0  0 1 0
Camera "perspective" "float fov" [ 45 ]
Film "image" "integer xresolution" [ 8 ] "integer yresolution" [ 8 ] "string filename" "closed.pfm"
WorldBegin
AttributeBegin
  Material "matte" "rgb Kd" [ 0.7 0.6 0.5 ]
  Translate 0.3 -0.2 2
  Rotate 20 1 0.3 0
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ -2.5 -2.5 0  2.5 -2.5 0.3  2.5 2.5 0  -2.5 2.5 -0.2 ]
    "float uv" [ 0.125 0.25  0.875 0.0625  1.5 0.75  -0.25 1.125 ]
AttributeEnd
AttributeBegin
  Material "plastic" "rgb Kd" [ 0.2 0.3 0.8 ]
  Translate -0.4 0.1 0.5
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 1 4 2 ] "point P" [ -1 -1 0.2  1 -1 -0.1  1 1 0.1  -1 1 0  2.2 0 0.6 ]
    "float uv" [ 0 0  1 0.1  0.9 1  0.05 0.95  1.7 0.4 ]
    "normal N" [ -0.3 -0.2 -1  0.25 -0.3 -1  0.3 0.2 -1  -0.2 0.35 -1  0.6 0 -0.8 ]
AttributeEnd
AttributeBegin
  Material "mirror"
  Shape "trianglemesh" "integer indices" [ 0 1 2 ] "point P" [ -3 -3 -1  -1 -3 -1.5  -2 -1 -0.5 ]
AttributeEnd
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 5 5 5 ]
  Material "matte" "rgb Kd" [ 0.8 0.8 0.8 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 1.5 1.5 -1  3 1.5 -1  3 3 -0.5  1.5 3 -0.5 ]
AttributeEnd
WorldEnd
"""


def test_fields_beyond_the_oracle_match_closed_forms(gpu):
    """Meshes in world space without instances.  make_isect (csrc/pg_triangle.h) forms p as t.p0 * b0 + t.p1 * b1 + t.p2 * b2 and tex_hit_setup's uvHit as
    b0 uv0 + b1 uv1 + b2 uv2, both left to right -- the order written in the assertions below -- and the kernels are built without contraction, so float32
    NumPy in that order reproduces them bit for bit."""
    scene = gpu.HostScene(text=CLOSED_FORM_SCENE)
    desc = scene.desc
    assert desc.n_instances == 0 and desc.n_spheres == 0 and desc.n_prims_all == desc.n_tris == 8
    gs = gpu.GpuScene(desc)
    o, d, tmax = scene_rays(scene, 1024, 5, aimed=8)
    rng = np.random.default_rng(6)
    P = np.ctypeslib.as_array(desc.P, (desc.n_verts, 3))
    idx = np.ctypeslib.as_array(desc.indices, (desc.n_tris, 3))
    k = rng.integers(0, desc.n_tris, 1024)  # rays at random points of random triangles: every mesh is hit often
    w = rng.dirichlet([1, 1, 1], 1024)
    target = (w[:, 0:1] * P[idx[k, 0]] + w[:, 1:2] * P[idx[k, 1]] + w[:, 2:3] * P[idx[k, 2]])
    o2 = np.stack([rng.uniform(-3, 3, 1024), rng.uniform(-3, 3, 1024), rng.uniform(-6, -2, 1024)], 1).astype(F32)
    o, d, tmax = np.concatenate([o, o2]), np.concatenate([d, (target - o2).astype(F32)]), np.concatenate([tmax, np.full(1024, np.inf, F32)])
    rec = gs.intersect_at(o, d, tmax)
    prim, t, bary = gs.intersect(o, d, tmax)
    gs.close()
    assert np.array_equal(rec["prim"], prim) and same_bits(rec["t"], t)
    hit = prim >= 0
    assert hit.sum() > 1000
    r, pr, b = rec[hit], prim[hit], bary[hit]
    flags = np.ctypeslib.as_array(desc.tri_flags, (desc.n_tris,))[pr]
    b0, b1, b2 = b[:, 0:1], b[:, 1:2], b[:, 2:3]
    p0, p1, p2 = P[idx[pr, 0]], P[idx[pr, 1]], P[idx[pr, 2]]
    assert p0.dtype == F32 and b.dtype == F32
    assert same_bits(r["p"], (b0 * p0 + b1 * p1) + b2 * p2)
    UV = np.ctypeslib.as_array(desc.UV, (desc.n_verts, 2))
    has_uv = (flags & 8) != 0
    uv0 = np.where(has_uv[:, None], UV[idx[pr, 0]], F32([0, 0]))  # triangle.h:104-106: the default parameterisation
    uv1 = np.where(has_uv[:, None], UV[idx[pr, 1]], F32([1, 0]))
    uv2 = np.where(has_uv[:, None], UV[idx[pr, 2]], F32([1, 1]))
    assert has_uv.sum() > 300 and (~has_uv).sum() > 50 and uv0.dtype == F32
    assert same_bits(r["uv"], (b0 * uv0 + b1 * uv1) + b2 * uv2)
    md = -d[hit]  # wo = Normalize(-ray.d): v * (1 / sqrt((x x + y y) + z z)), geometry.h:243-248, :984-986
    inv = F32(1) / np.sqrt((md[:, 0] * md[:, 0] + md[:, 1] * md[:, 1]) + md[:, 2] * md[:, 2])
    assert inv.dtype == F32 and same_bits(r["wo"], md * inv[:, None])
    has_n = (flags & 4) != 0
    assert has_n.sum() > 200 and (~has_n).sum() > 300 and not (flags & 16).any()
    assert same_bits(r["shading_n"][~has_n], r["n"][~has_n])
    # Normalize of a float vector: five roundings in the squared length (3 u relative, all terms positive; u = 2^-24), halved by the root, plus the
    # root's, the reciprocal's and the product's own: 4.5 u per component, so | |ns| - 1 | <= 4.5 u, asserted as 5 u
    sn = r["shading_n"][has_n].astype(np.float64)
    assert np.abs(np.sqrt((sn * sn).sum(1)) - 1).max() <= 5 * 2.0 ** -24
    assert ((r["n"][has_n].astype(np.float64) * sn).sum(1) >= 0).all()
    assert not same_bits(r["shading_n"][has_n], r["n"][has_n])
    mat = np.ctypeslib.as_array(desc.tri_material, (desc.n_tris,))
    light = np.ctypeslib.as_array(desc.tri_light, (desc.n_tris,))
    assert np.array_equal(r["material"], mat[pr]) and np.array_equal(r["light"], light[pr])
    assert len(set(r["material"])) == 4 and (r["light"] >= 0).sum() > 50 and (r["light"] < 0).sum() > 500
    assert (r["instance"] == -1).all() and (r["instance_inner"] == -1).all() and (r["reserved"] == 0).all() and (r["time"] == 0).all()


# ---- 3. and 4. the shutter's ends are exact; the time is per ray --------------------------------------------------------------------------------------
OPEN, CLOSE = 0.3, 0.8
MOTION_SCENE = """
LookAt 278 273 -800  278 273 0  0 1 0
Camera "perspective" "float shutteropen" [ 0.3 ] "float shutterclose" [ 0.8 ] "float fov" [ 39.3 ]
Film "image" "integer xresolution" [ 8 ] "integer yresolution" [ 8 ] "string filename" "motion.pfm"
TransformTimes 0.3 0.8
WorldBegin
Material "matte" "rgb Kd" [ 0.73 0.73 0.73 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 552.8 0 0   0 0 0   0 0 559.2   549.6 0 559.2 ]
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 549.6 0 559.2   0 0 559.2   0 548.8 559.2   556 548.8 559.2 ]
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 17 12 4 ]
  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ 343 548.7 227   343 548.7 332   213 548.7 332   213 548.7 227 ]
AttributeEnd
ObjectBegin "boxes"
Material "matte" "rgb Kd" [ 0.7 0.7 0.2 ]
Shape "trianglemesh"
  "integer indices" [ 0 1 2 0 2 3  4 5 6 4 6 7  8 9 10 8 10 11  12 13 14 12 14 15  16 17 18 16 18 19  20 21 22 20 22 23 ]
  "point P" [ 130 165 65   82 165 225   240 165 272   290 165 114
              290 0 114   290 165 114   240 165 272   240 0 272
              130 0 65   130 165 65   290 165 114   290 0 114
              82 0 225   82 165 225   130 165 65   130 0 65
              240 0 272   240 165 272   82 165 225   82 0 225
              130 0 65   290 0 114   240 0 272   82 0 225 ]
Material "glass" "float index" [ 1.4 ]
Shape "trianglemesh"
  "integer indices" [ 0 1 2 0 2 3  4 5 6 4 6 7  8 9 10 8 10 11  12 13 14 12 14 15  16 17 18 16 18 19  20 21 22 20 22 23 ]
  "point P" [ 423 330 247   265 330 296   314 330 456   472 330 406
              423 0 247   423 330 247   472 330 406   472 0 406
              472 0 406   472 330 406   314 330 456   314 0 456
              314 0 456   314 330 456   265 330 296   265 0 296
              265 0 296   265 330 296   423 330 247   423 0 247
              423 0 247   472 0 406   314 0 456   265 0 296 ]
ObjectEnd
ObjectBegin "ball"
  Material "mirror"
  Translate 0 40 0
  Shape "sphere" "float radius" [ 40 ]
ObjectEnd
%s
WorldEnd
"""
# the instances' transform A, and what the END transform has on top of it (B = A extra): rotations and translations, nothing mirrored
BOXES_A, BOXES_EXTRA = "  Translate 20 10 30\n  Rotate 15 0 1 0.2\n  Scale 0.6 0.6 0.6\n", "  Translate 380 260 40\n  Rotate 70 0.3 1 0\n"
BALL_A, BALL_EXTRA = "  Translate 120 60 320\n  Scale 1.5 1.5 1.5\n", "  Translate 180 120 -90\n  Rotate 50 1 0 0.5\n"
SLIDE_A, SLIDE_EXTRA, SLIDE_HALF = "  Translate 20 10 30\n  Scale 0.6 0.6 0.6\n", "  Translate 300 200 60\n", "  Translate 150 100 30\n"


def moving(a, extra, name):
    return "AttributeBegin\n" + a + "  ActiveTransform EndTime\n" + extra + "  ActiveTransform All\n  ObjectInstance \"" + name + "\"\nAttributeEnd\n"


def still(a, name):
    return "AttributeBegin\n" + a + "  ObjectInstance \"" + name + "\"\nAttributeEnd\n"


def motion_rays(n, seed, centre=None):
    """From in front of the room towards the places the two instances occupy at either end of their motion (and a few elsewhere) -- or towards `centre`."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(100, 450, n), rng.uniform(100, 450, n), rng.uniform(-800, -300, n)], 1).astype(F32)
    target = np.stack([rng.uniform(0, 556, n), rng.uniform(0, 500, n), rng.uniform(50, 400, n)], 1)
    if centre is not None: target = np.asarray(centre) + rng.normal(size=(n, 3)) * 70
    d = (target - o).astype(F32)
    tmax = np.full(n, np.inf, F32)
    tmax[::9] = 900
    return o, d, tmax


def denoted(rec, scene, end=False):
    """A batch's records in a form two scenes can share.  `prim` and `instance` are numbers of ONE scene's arrays: primitives are numbered in the order its
    BVH leaves them in, and the BVH of a scene with motion is built over the motion's bounds, so the same triangle carries another number in the static
    scene (the geometry fields of the two came out equal in every bit while 1315 of 2048 `prim` differed).  They are compared through what they denote:
    a triangle's vertices, flags, material and light, a quadric's PgSphere, an instance's object and its transform at this end of the motion.  Every other
    field but `time` is compared as it is: returns (what prim denotes, what instance denotes, the rest as bytes)."""
    desc = scene.desc
    flags = np.ctypeslib.as_array(desc.tri_flags, (desc.n_prims_all,))
    idx = np.ctypeslib.as_array(desc.indices, (desc.n_prims_all, 3))
    mat = np.ctypeslib.as_array(desc.tri_material, (desc.n_prims_all,))
    light = np.ctypeslib.as_array(desc.tri_light, (desc.n_prims_all,))
    P = np.ctypeslib.as_array(desc.P, (desc.n_verts, 3))

    def prim_key(k):
        if k < 0: return None
        shape = bytes(desc.spheres[idx[k, 0]]) if flags[k] & 32 else P[idx[k]].tobytes()
        return (int(flags[k]), int(mat[k]), int(light[k]), shape)

    def instance_key(i):
        if i < 0: return None
        inst = desc.instances[i]
        obj = desc.objects[inst.object]
        return (obj.n_prims, obj.n_nodes, bytes(inst.i2w_end if end and inst.animated else inst.i2w), bytes(inst.w2i_end if end and inst.animated else inst.w2i))

    rest = rec.copy()
    rest["time"] = 0; rest["prim"] = 0; rest["instance"] = 0
    return [prim_key(k) for k in rec["prim"]], [instance_key(i if k >= 0 else -1) for k, i in zip(rec["prim"], rec["instance"])], rest.tobytes()


@pytest.fixture(scope="module")
def shutter(gpu):
    """The scene whose two instances move (rotation and translation) over the shutter, queried with all rays at its open and at its close, and the two
    static scenes with the same objects instanced under the start and under the end transform -- TransformedPrimitives too: the same arithmetic."""
    o, d, tmax = motion_rays(2048, 21)
    out = {"rays": (o, d, tmax)}
    texts = {"moving": moving(BOXES_A, BOXES_EXTRA, "boxes") + moving(BALL_A, BALL_EXTRA, "ball"),
             "A": still(BOXES_A, "boxes") + still(BALL_A, "ball"), "B": still(BOXES_A + BOXES_EXTRA, "boxes") + still(BALL_A + BALL_EXTRA, "ball")}
    for key, text in texts.items():
        scene = gpu.HostScene(text=MOTION_SCENE % text)
        assert scene.desc.n_instances == 2 and sum(scene.desc.instances[i].animated for i in range(2)) == (2 if key == "moving" else 0)
        gs = gpu.GpuScene(scene.desc)
        if key == "moving":
            assert tuple(scene.desc.instances[0].time) == (F32(OPEN), F32(CLOSE))
            out["open"] = gs.intersect_at(o, d, tmax, np.full(len(tmax), OPEN, F32))
            out["close"] = gs.intersect_at(o, d, tmax, np.full(len(tmax), CLOSE, F32))
            out["occ_open"] = gs.intersect_p_at(o, d, tmax, np.full(len(tmax), OPEN, F32))
            out["occ_close"] = gs.intersect_p_at(o, d, tmax, np.full(len(tmax), CLOSE, F32))
            out["gs"], out["scene"] = gs, scene
        else:
            out[key] = gs.intersect_at(o, d, tmax)
            out["occ_" + key] = gs.intersect_p_at(o, d, tmax)
            out["scene_" + key] = scene
            gs.close()
    yield out
    out["gs"].close()


def test_shutter_ends_equal_the_static_scenes(shutter, oracle):
    o, d, tmax = shutter["rays"]
    a, b = shutter["open"], shutter["close"]
    assert (a["time"] == F32(OPEN)).all() and (b["time"] == F32(CLOSE)).all()
    # the case cannot pass with the time ignored: the ends are far apart
    assert (a["prim"] != b["prim"]).mean() >= 0.25
    assert ((a["instance"] >= 0) & (a["prim"] >= 0)).sum() > 300 and ((b["instance"] >= 0) & (b["prim"] >= 0)).sum() > 300
    assert (a["instance_inner"][a["prim"] >= 0] == -1).all() and (b["instance_inner"][b["prim"] >= 0] == -1).all()
    assert denoted(a, shutter["scene"]) == denoted(shutter["A"], shutter["scene_A"]), "records at the shutter's open differ from the static scene under the start transform"
    assert denoted(b, shutter["scene"], end=True) == denoted(shutter["B"], shutter["scene_B"]), "records at the shutter's close differ from the static scene under the end transform"
    assert np.array_equal(shutter["occ_open"], shutter["occ_A"]) and np.array_equal(shutter["occ_close"], shutter["occ_B"])
    assert np.array_equal(shutter["occ_open"] != 0, a["prim"] >= 0) and np.array_equal(shutter["occ_close"] != 0, b["prim"] >= 0)
    # ... and the static scenes' records are the oracle's: the chain reaches the reference
    check_against_oracle(oracle, shutter["scene_A"].desc, o, d, tmax, shutter["A"])
    check_against_oracle(oracle, shutter["scene_B"].desc, o, d, tmax, shutter["B"])


def test_time_is_per_ray(shutter):
    o, d, tmax = (x[:256] for x in shutter["rays"])
    time = np.where(np.arange(256) % 2 == 0, F32(OPEN), F32(CLOSE)).astype(F32)
    rec = shutter["gs"].intersect_at(o, d, tmax, time)
    want = np.where(np.arange(256) % 2 == 0, shutter["open"][:256], shutter["close"][:256])
    assert np.array_equal(rec.view(np.uint8), want.view(np.uint8))
    assert (shutter["open"][:256]["prim"] != shutter["close"][:256]["prim"]).sum() >= 64
    occ = shutter["gs"].intersect_p_at(o, d, tmax, time)
    assert np.array_equal(occ, np.where(np.arange(256) % 2 == 0, shutter["occ_open"][:256], shutter["occ_close"][:256]))


def test_shutter_middle_under_a_pure_translation(gpu):
    """Half way through a pure translation the interpolated transform is the static one up to rounding (AnimatedTransform::Interpolate recomposes it from
    the decomposed T, R and S): the same primitives, and points that agree within the two interactions' own error bounds -- no other tolerance."""
    o, d, tmax = motion_rays(256, 33, centre=(276, 169, 204))  # (where the object is half way)
    mid = F32(0.5 * (OPEN + CLOSE))
    scene = gpu.HostScene(text=MOTION_SCENE % moving(SLIDE_A, SLIDE_EXTRA, "boxes"))
    gs = gpu.GpuScene(scene.desc)
    m, a, b = (gs.intersect_at(o, d, tmax, np.full(256, t, F32)) for t in (mid, OPEN, CLOSE))
    gs.close()
    still_scene = gpu.HostScene(text=MOTION_SCENE % still(SLIDE_A + SLIDE_HALF, "boxes"))
    gs = gpu.GpuScene(still_scene.desc)
    s = gs.intersect_at(o, d, tmax)
    gs.close()
    assert (m["time"] == mid).all() and denoted(m, scene)[0] == denoted(s, still_scene)[0]  # (prim: through what it denotes, see denoted())
    assert np.array_equal(m["instance"] >= 0, s["instance"] >= 0) and np.array_equal(m["material"], s["material"])
    assert (np.abs(m["p"] - s["p"]) <= m["p_error"] + s["p_error"]).all()
    on = (m["prim"] >= 0) & (m["instance"] >= 0)
    assert on.sum() > 30
    assert (m["p"][on] != a["p"][on]).any(axis=1).all() and (m["p"][on] != b["p"][on]).any(axis=1).all()


# ---- 5. shapes of the launch ----------------------------------------------------------------------------------------------------------------------
def test_batch_sizes_are_prefixes_of_one_batch(shutter):
    o, d, tmax = shutter["rays"]
    time = np.where(np.arange(len(tmax)) % 3 == 0, F32(OPEN), np.where(np.arange(len(tmax)) % 3 == 1, F32(CLOSE), F32(0.45))).astype(F32)
    gs = shutter["gs"]
    whole = gs.intersect_at(o, d, tmax, time)
    occ = gs.intersect_p_at(o, d, tmax, time)
    assert len(set(whole["prim"])) >= 16 and len(set(whole["instance"])) == 3
    for n in (1, 63, 64, 65, 1000):
        part = gs.intersect_at(o[:n], d[:n], tmax[:n], time[:n])
        assert np.array_equal(part.view(np.uint8), whole[:n].view(np.uint8)), n
        assert np.array_equal(gs.intersect_p_at(o[:n], d[:n], tmax[:n], time[:n]), occ[:n]), n


def test_a_batch_of_misses_and_an_empty_batch(shutter, gpu):
    gs = shutter["gs"]
    rng = np.random.default_rng(4)
    n = 300
    o = np.stack([rng.uniform(-500, 1000, n), rng.uniform(2000, 3000, n), rng.uniform(-500, 1000, n)], 1).astype(F32)
    d = np.stack([rng.normal(size=n), rng.uniform(0.1, 1, n), rng.normal(size=n)], 1).astype(F32)  # above the room, going up
    tmax = np.where(np.arange(n) % 2 == 0, F32(np.inf), rng.uniform(1, 5000, n)).astype(F32)
    time = rng.uniform(OPEN, CLOSE, n).astype(F32)
    rec = gs.intersect_at(o, d, tmax, time)
    assert (rec["prim"] == -1).all() and same_bits(rec["t"], tmax) and same_bits(rec["time"], time)
    rest = rec.copy()
    rest["prim"] = 0; rest["t"] = 0; rest["time"] = 0
    assert not rest.view(np.uint8).any()
    assert not gs.intersect_p_at(o, d, tmax, time).any()
    before = gs.counters()
    empty = gs.intersect_at(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, F32))
    assert empty.dtype == gpu.INTERACTION_DTYPE and len(empty) == 0 and len(gs.intersect_p_at(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, F32))) == 0
    lib = gpu.gpu_lib()
    assert lib.pg_intersect_at(gs._h, 0, None, None, None, None, None, 0, None) == 0  # n == 0 touches nothing, not even its arguments
    assert lib.pg_intersect_p_at(gs._h, 0, None, None, None, None, None, 0, None) == 0
    assert gs.counters() == before


def test_no_times_means_time_zero(shutter):
    o, d, tmax = (x[:500] for x in shutter["rays"])
    gs = shutter["gs"]
    a, b = gs.intersect_at(o, d, tmax), gs.intersect_at(o, d, tmax, np.zeros(500, F32))
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and (a["time"] == 0).all()
    assert np.array_equal(gs.intersect_p_at(o, d, tmax), gs.intersect_p_at(o, d, tmax, np.zeros(500, F32)))
    # time 0 lies before the motion's start: the start transform
    assert denoted(a, shutter["scene"]) == denoted(shutter["open"][:500], shutter["scene"])


class DeviceArrays:
    """Device memory for the PG_MEM_DEVICE calls: torch tensors on the GPU -- on the emulated device, whose device memory is the host's, NumPy arrays."""

    def __init__(self):
        self.keep = []

    def put(self, a):
        if EMULATED:
            t = np.ascontiguousarray(a).copy()
            self.keep.append(t)
            return t.ctypes.data
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        self.keep.append(t)
        return t.data_ptr()

    def get(self, i, dtype):
        t = self.keep[i]
        if EMULATED: return t.view(np.uint8).reshape(-1).view(dtype)
        import torch
        torch.cuda.synchronize()
        return t.cpu().numpy().view(dtype)


def test_device_memory_output_equals_host_output(shutter, gpu):
    o, d, tmax = (x[:1000] for x in shutter["rays"])
    n = 1000
    time = np.where(np.arange(n) % 2 == 0, F32(OPEN), F32(CLOSE)).astype(F32)
    gs = shutter["gs"]
    host = gs.intersect_at(o, d, tmax, time)
    host_occ = gs.intersect_p_at(o, d, tmax, time)
    dev = DeviceArrays()
    po, pd, pt, ptime = dev.put(o), dev.put(d), dev.put(tmax), dev.put(time)
    pout = dev.put(np.full(n * gpu.INTERACTION_DTYPE.itemsize, 0xAB, np.uint8))
    pocc = dev.put(np.full(n, 0xAB, np.uint8))
    gs.intersect_at_device(n, po, pd, pt, ptime, pout)
    gs.intersect_p_at_device(n, po, pd, pt, ptime, pocc)
    assert np.array_equal(dev.get(4, np.uint8), host.view(np.uint8))
    assert np.array_equal(dev.get(5, np.uint8), host_occ)
    gs.intersect_at_device(n, po, pd, pt, None, pout)  # no times
    assert np.array_equal(dev.get(4, np.uint8), gs.intersect_at(o, d, tmax).view(np.uint8))


# ---- 5b. pg_intersect / pg_intersect_p, the unit pair, go through the same device path ------------------------------------------------------------------
@pytest.fixture(scope="module", params=["cornell_32", "shutter"])
def unit_case(request, gpu, shutter):
    """(scene on the device, 2049 rays that hit and miss) for the golden Cornell box and for the moving, instanced scene of `shutter`."""
    if request.param == "shutter":
        yield (shutter["gs"],) + motion_rays(2049, 23)
        return
    scene = gpu.HostScene(os.path.join(GOLD, "cornell_32.pbrt"))
    gs = gpu.GpuScene(scene.desc)
    o, d, tmax = scene_rays(scene, 2049, 17)
    mix = np.random.default_rng(18).permutation(len(tmax))[:2049]  # the aimed rays among the random ones
    yield gs, np.ascontiguousarray(o[mix]), np.ascontiguousarray(d[mix]), np.ascontiguousarray(tmax[mix])
    gs.close()


PAD = 64  # elements the device arrays are longer than the results, to catch a write past them


def unit_pair_on_device(gpu, gs, o, d, tmax):
    """pg_intersect and pg_intersect_p with PG_MEM_DEVICE: the four result arrays as bytes, each PAD elements longer than its result and pre-filled 0xAB."""
    n = len(tmax)
    dev = DeviceArrays()
    po, pd, pt = dev.put(o), dev.put(d), dev.put(tmax)
    out = [dev.put(np.full(size, 0xAB, np.uint8)) for size in (4 * (n + PAD), 4 * (n + PAD), 4 * (3 * n + PAD), n + PAD)]
    lib = gpu.gpu_lib()
    assert lib.pg_intersect(gs._h, n, po, pd, pt, out[0], out[1], out[2], gpu.PG_MEM_DEVICE, None) == 0, lib.pg_last_error()
    assert lib.pg_intersect_p(gs._h, n, po, pd, pt, out[3], gpu.PG_MEM_DEVICE, None) == 0, lib.pg_last_error()
    return [dev.get(3 + k, np.uint8) for k in range(4)]


def test_unit_pair_device_memory_equals_host_memory(unit_case, gpu):
    gs, o, d, tmax = unit_case
    n = 1000  # three regions of 256 entries and part of a fourth
    o, d, tmax = o[:n], d[:n], tmax[:n]
    prim, t, bary = gs.intersect(o, d, tmax)
    occ = gs.intersect_p(o, d, tmax)
    hit = prim >= 0
    assert hit.sum() > 100 and (~hit).sum() > 20
    assert not bits(bary[~hit]).any() and same_bits(t[~hit], tmax[~hit])  # a miss: three zeros, the ray's own tmax
    assert np.array_equal(occ != 0, hit)
    dprim, dt, dbary, docc = unit_pair_on_device(gpu, gs, o, d, tmax)
    for got, want in ((dprim, prim), (dt, t), (dbary, bary), (docc, occ)):
        assert np.array_equal(got[:want.nbytes], want.view(np.uint8).reshape(-1))
        assert len(got) - want.nbytes == PAD * want.itemsize and (got[want.nbytes:] == 0xAB).all()


def test_unit_pair_counters_do_not_depend_on_the_memory_kind(unit_case, gpu):
    gs, o, d, tmax = unit_case
    o, d, tmax = o[:1000], d[:1000], tmax[:1000]
    keys = [kind + what for kind in ("closest_", "shadow_") for what in ("rays", "node_visits", "tri_tests", "launches")]
    gs.counters_reset()
    unit_pair_on_device(gpu, gs, o, d, tmax)
    device = gs.counters()
    gs.counters_reset()
    gs.intersect(o, d, tmax)
    gs.intersect_p(o, d, tmax)
    host = gs.counters()
    assert [device[k] for k in keys] == [host[k] for k in keys]
    assert host["closest_rays"] == host["shadow_rays"] == 1000 and host["closest_launches"] == host["shadow_launches"] == 1
    assert host["closest_node_visits"] > 1000 and host["shadow_node_visits"] > 1000 and host["closest_tri_tests"] > 0 and host["shadow_tri_tests"] > 0


def test_unit_pair_batch_sizes_are_prefixes_of_one_batch(unit_case):
    """The buffers grow up to the largest batch and are then reused by a smaller one."""
    gs, o, d, tmax = unit_case
    sizes = (1, 63, 64, 65, 257, 1000, 2049, 1)
    got = [gs.intersect(o[:n], d[:n], tmax[:n]) + (gs.intersect_p(o[:n], d[:n], tmax[:n]),) for n in sizes]
    whole = got[sizes.index(2049)]
    assert len(set(whole[0])) >= 8 and (whole[0] < 0).any()
    for n, part in zip(sizes, got):
        for a, b in zip(part, whole):
            assert len(a) == n and a.tobytes() == b[:n].tobytes(), n


def test_unit_pair_is_the_at_pair_without_times(shutter):
    """On the moving scene: rays without a time are rays at time 0, whichever entry point takes them."""
    o, d, tmax = shutter["rays"]
    gs = shutter["gs"]
    prim, t, _ = gs.intersect(o, d, tmax)
    rec = gs.intersect_at(o, d, tmax, time=None)
    assert np.array_equal(prim, rec["prim"]) and same_bits(t, rec["t"])
    assert ((rec["instance"] >= 0) & (prim >= 0)).sum() > 300 and (prim < 0).any()
    assert np.array_equal(gs.intersect_p(o, d, tmax), gs.intersect_p_at(o, d, tmax, time=None))


def test_unit_pair_refused_arguments(shutter, gpu):
    gs = shutter["gs"]
    lib = gpu.gpu_lib()
    o, d, tmax = (np.ascontiguousarray(x[:4]) for x in shutter["rays"])
    prim, t, bary, occ = np.zeros(4, np.int32), np.zeros(4, F32), np.zeros((4, 3), F32), np.zeros(4, np.uint8)
    before = gs.counters()
    assert lib.pg_intersect(gs._h, 0, None, None, None, None, None, None, gpu.PG_MEM_HOST, None) == 0  # n == 0 touches nothing, not even its arguments
    assert lib.pg_intersect_p(gs._h, 0, None, None, None, None, gpu.PG_MEM_HOST, None) == 0
    assert gs.counters() == before
    closest, anyhit = [a.ctypes.data for a in (o, d, tmax, prim, t, bary)], [a.ctypes.data for a in (o, d, tmax, occ)]
    for mem in (gpu.PG_MEM_HOST, gpu.PG_MEM_DEVICE):
        for k in range(len(closest)):
            assert lib.pg_intersect(gs._h, 4, *closest[:k], None, *closest[k + 1:], mem, None) == -1  # PG_ERR_INVALID
            assert b"pg_intersect:" in lib.pg_last_error()
        for k in range(len(anyhit)):
            assert lib.pg_intersect_p(gs._h, 4, *anyhit[:k], None, *anyhit[k + 1:], mem, None) == -1
            assert b"pg_intersect_p:" in lib.pg_last_error()
    assert gs.counters() == before and not prim.any() and not bits(t).any() and not bits(bary).any() and not occ.any()  # no device work followed
    with pytest.raises(ValueError):
        gs.intersect(o, d[:3], tmax)
    with pytest.raises(ValueError):
        gs.intersect_p(o[:3], d, tmax)


# ---- 6. arguments --------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(shutter, gpu):
    gs = shutter["gs"]
    lib = gpu.gpu_lib()
    o, d, tmax = (np.ascontiguousarray(x[:4]) for x in shutter["rays"])
    time = np.zeros(4, F32)
    out = np.zeros(4, gpu.INTERACTION_DTYPE)
    occ = np.zeros(4, np.uint8)
    before = gs.counters()
    P = lambda a: a.ctypes.data
    for args in ((4, P(o), P(d), P(tmax), P(time), None), (4, None, P(d), P(tmax), P(time), P(out)), (-1, P(o), P(d), P(tmax), P(time), P(out)),
                 (4, P(o), None, P(tmax), None, P(out)), (4, P(o), P(d), None, None, P(out))):
        assert lib.pg_intersect_at(gs._h, *args, gpu.PG_MEM_HOST, None) == -1  # PG_ERR_INVALID
        assert b"pg_intersect_at" in lib.pg_last_error()
    assert lib.pg_intersect_at(None, 4, P(o), P(d), P(tmax), None, P(out), gpu.PG_MEM_HOST, None) == -1
    for args in ((4, P(o), P(d), P(tmax), P(time), None), (4, None, P(d), P(tmax), P(time), P(occ)), (-1, P(o), P(d), P(tmax), P(time), P(occ))):
        assert lib.pg_intersect_p_at(gs._h, *args, gpu.PG_MEM_HOST, None) == -1
        assert b"pg_intersect_p_at" in lib.pg_last_error()
    assert gs.counters() == before and not out.view(np.uint8).any() and not occ.any()  # no device work followed
    with pytest.raises(ValueError):
        gs.intersect_at(o, d[:3], tmax)
