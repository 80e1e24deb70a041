"""Camera importance (csrc/pg_cameraimportance.h): pg_camera_we_at -- PerspectiveCamera::We and ::Pdf_We per ray -- and pg_camera_sample_wi_at -- ::Sample_Wi per
reference point with VisibilityTester::Unoccluded.

Every field is pinned bit for bit to a float32 NumPy restatement of perspective.cpp:146-225 (Transform::operator() as transform.h spells it, the oracle's
OffsetRayOrigin around SpawnRay / SpawnRayTo) on a pinhole, a thin-lens and three moving cameras at and beyond both ends of their motion, where
AnimatedTransform::Interpolate hands out the stored matrices.  Between the ends, where the interpolated inverse has no restatement here, the rays
pg_camera_rays_at generates must come back to their film points.  Visibility is pg_intersect_p_at's (and the oracle's IntersectP) for the reported shadow ray.
Batches of 1, 64, 65 and 600 items run in host memory and in device memory, with guard bytes on both sides of every output.
tests/test_emulated_camera_importance.py runs this file without a GPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = 256  # guard bytes on either side of every output
SCENES = ["cornell_32", "cornell_lens", "camanim_translate", "camanim_rotate", "camanim_times_scale"]
MOVING = SCENES[2:]
SIZES = (1, 64, 65, 600)  # one lane; a full wave; one past it; several blocks with a ragged tail
N = max(SIZES)
PI = F32(3.14159265358979323846)
SHADOW_TMAX = F32(1) - F32(0.0001)


def _load(filename):
    spec = importlib.util.spec_from_file_location(filename[:-3] + "_helpers", os.path.join(os.path.dirname(__file__), filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_CQ, _GL = _load("test_gpu_camera_queries.py"), _load("test_gpu_lights.py")
xform_point, xform_vec, v3, concentric_sample_disk = _CQ.xform_point, _CQ.xform_vec, _CQ.v3, _CQ.concentric_sample_disk
DeviceArrays, same_bits, bits, records_equal, dot32, spawn_origin = _CQ.DeviceArrays, _CQ.same_bits, _CQ.bits, _CQ.records_equal, _GL.dot32, _GL.spawn_origin


# ---- calls with guarded outputs, in host or in device memory -------------------------------------------------------------------------------------------------
def guarded_call(gpu, name, args, mem):
    """The raw entry point `name` with `args` (an array = an input; (dtype, count) = an output of that many records; anything else as given) followed by mem
    and a NULL stream.  Every output lies between PAD guard bytes, which must come back intact; returns the outputs."""
    dev = DeviceArrays() if mem == gpu.PG_MEM_DEVICE else None
    keep, outs, call = [], [], []
    for a in args:
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            keep.append(a)
            call.append(dev.put(a) if dev else a.ctypes.data)
        elif isinstance(a, tuple):
            dtype, count = a
            guard = np.full(2 * PAD + np.dtype(dtype).itemsize * count, 0xAB, np.uint8)
            if dev: base, slot = dev.put(guard), len(dev.keep)
            else: base, slot = guard.ctypes.data, guard
            assert base % 16 == 0
            outs.append((slot, np.dtype(dtype), count))
            call.append(base + PAD)
        else: call.append(a)
    st = getattr(gpu.gpu_lib(), name)(*call, mem, None)
    assert st == 0, (name, st, gpu.gpu_lib().pg_last_error())
    got = []
    for slot, dtype, count in outs:
        raw = dev.get(slot - 1, np.uint8) if dev else slot
        nbytes = dtype.itemsize * count
        assert (raw[:PAD] == 0xAB).all() and (raw[PAD + nbytes:] == 0xAB).all(), (name, "guard bytes")
        got.append(raw[PAD:PAD + nbytes].copy().view(dtype))
    return got


def we_at(gpu, sc, o, d, time, mem):
    n = len(o)
    return guarded_call(gpu, "pg_camera_we_at", [sc.gs._h, C.byref(sc.rd), C.byref(sc.we), n, o, d, time, (gpu.CAMERA_IMPORTANCE_DTYPE, n)], mem)[0]


def sample_wi_at(gpu, sc, ref, u, mem, shadow=True):
    n = len(ref)
    got = guarded_call(gpu, "pg_camera_sample_wi_at", [sc.gs._h, C.byref(sc.rd), C.byref(sc.we), n, ref, u, (gpu.CAMERA_SAMPLE_DTYPE, n),
                                                      (F32, 8 * n) if shadow else None], mem)
    return (got[0], got[1].reshape(n, 8)) if shadow else got[0]


# ---- the restatement: float32, every operation in the order the reference writes it --------------------------------------------------------------------------
def matrices_at(sc, time):
    """AnimatedTransform::Interpolate at times at or beyond the ends (transform.cpp:1144-1152): the stored start / end transform and its stored inverse, as
    (16, n) arrays -- m[k] is entry k of every ray's matrix."""
    rd, we = sc.rd, sc.we
    t0, t1 = (F32(rd.camera_time[0]), F32(rd.camera_time[1])) if rd.camera_animated else (F32(np.inf), F32(np.inf))
    start, end = time <= t0, time >= t1
    assert (start | end).all()  # (nothing in between is restated)
    pick = lambda a, b: np.where(start[None, :], np.array(a[:], F32)[:, None], np.array(b[:], F32)[:, None]).astype(F32)
    return pick(rd.camera_to_world, rd.camera_to_world_end), pick(we.world_to_camera, we.world_to_camera_end)


def restate_we(sc, c2w, w2c, o, d):
    """We(ray, &pRaster) and Pdf_We(ray, &pdfPos, &pdfDir), perspective.cpp:146-201, as CAMERA_IMPORTANCE_DTYPE records."""
    rd, n = sc.rd, len(o)
    radius, focal, A = F32(rd.lens_radius), F32(rd.focal_distance), F32(sc.we.image_area)
    rec = np.zeros(n, sc.gpu.CAMERA_IMPORTANCE_DTYPE)
    with np.errstate(all="ignore"):
        cos = dot32(d, xform_vec(c2w, v3(0, 0, 1, n)))
        p_focus = o + d * ((focal if radius > 0 else F32(1)) / cos)[:, None]
        pr = xform_point(np.array(sc.we.camera_to_raster[:], F32), xform_point(w2c, p_focus))
        sb = [F32(b) for b in rd.sample_bounds]
        outside = (pr[:, 0] < sb[0]) | (pr[:, 0] >= sb[2]) | (pr[:, 1] < sb[1]) | (pr[:, 1] >= sb[3])
        lens_area = (PI * radius) * radius if radius != 0 else F32(1)
        cos2 = cos * cos
        We, pdf_dir = F32(1) / (((A * lens_area) * cos2) * cos2), F32(1) / (((A * cos) * cos) * cos)
    front = ~(cos <= 0)
    inside = front & ~outside
    rec["status"] = np.where(front, np.where(outside, 1, 2), 0)
    rec["We"], rec["pdf_pos"], rec["pdf_dir"] = np.where(inside, We, 0), np.where(inside, F32(1) / lens_area, 0), np.where(inside, pdf_dir, 0)
    rec["p_raster"], rec["cos_theta"] = np.where(front[:, None], pr[:, :2], 0), np.where(front, cos, 0)
    assert We.dtype == F32 and pr.dtype == F32 and pdf_dir.dtype == F32
    return rec


def restate_sample_wi(sc, oracle, ref, u):
    """Sample_Wi, perspective.cpp:203-225, as CAMERA_SAMPLE_DTYPE records (visibility left -1) and the rays of ref.SpawnRayTo(lensIntr) of the samples bdpt tests."""
    rd, n = sc.rd, len(ref)
    radius = F32(rd.lens_radius)
    c2w, w2c = matrices_at(sc, ref["time"])
    valid = ref["prim"] >= 0
    rec = np.zeros(n, sc.gpu.CAMERA_SAMPLE_DTYPE)
    p_lens_cam = np.concatenate([radius * concentric_sample_disk(u), np.zeros((n, 1), F32)], 1)
    p_lens, n_lens = xform_point(c2w, p_lens_cam), xform_vec(c2w, v3(0, 0, 1, n))
    with np.errstate(all="ignore"):
        wi = p_lens - ref["p"]
        dist = np.sqrt((wi[:, 0] * wi[:, 0] + wi[:, 1] * wi[:, 1]) + wi[:, 2] * wi[:, 2])
        wi = wi * (F32(1) / dist)[:, None]
        lens_area = (PI * radius) * radius if radius != 0 else F32(1)
        pdf = (dist * dist) / (np.abs(dot32(n_lens, wi)) * lens_area)
        zero = np.zeros((n, 3), F32)
        we = restate_we(sc, c2w, w2c, spawn_origin(oracle, p_lens, zero, n_lens, -wi), -wi)  # We(lensIntr.SpawnRay(-wi), pRaster)
    rec["status"], rec["visibility"] = np.where(valid, we["status"], -1), -1
    for f, v in (("pdf", pdf), ("We", we["We"]), ("wi", wi), ("p_lens", p_lens), ("n_lens", n_lens), ("p_raster", we["p_raster"])):
        rec[f] = np.where(valid if v.ndim == 1 else valid[:, None], v, 0)
    tested = valid & (pdf > 0) & (we["We"] != 0)
    origin = spawn_origin(oracle, ref["p"], ref["p_error"], ref["n"], p_lens - ref["p"])  # interaction.h:73-78
    target = spawn_origin(oracle, p_lens, zero, n_lens, origin - p_lens)
    shadow = np.concatenate([origin, np.full((n, 1), SHADOW_TMAX, F32), target - origin, ref["time"][:, None]], 1).astype(F32)
    return rec, np.where(tested[:, None], shadow, 0).astype(F32), tested


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One scene on the device with N rays for We and N reference points for Sample_Wi, all at times at or beyond the ends of the camera's motion."""

    def __init__(self, gpu, name):
        self.gpu, self.name = gpu, name
        self.host = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
        self.rd, self.we = self.host.render_desc(), self.host.camera_we_desc()
        self.gs = gpu.GpuScene(self.host.desc)
        rd = self.rd
        rng = np.random.default_rng(900 + SCENES.index(name))
        sb = [float(b) for b in rd.sample_bounds]
        # film points inside the sample bounds, exactly on pMin and pMax, and outside
        film = (rng.random((N, 2)) * [sb[2] - sb[0], sb[3] - sb[1]] + [sb[0], sb[1]]).astype(F32)
        film[:8] = [(sb[0], sb[1]), (sb[2], sb[3]), (sb[0], sb[3]), (sb[2], sb[1]), (sb[0] - 0.5, 3), (sb[2] + 2.25, 5), (7, sb[1] - 1.5), (9.5, sb[3] + 0.125)]
        film[8:40] += rng.choice([-1, 1], (32, 2)) * [sb[2] - sb[0], sb[3] - sb[1]]
        lens = np.minimum(rng.random((N, 2)).astype(F32), np.nextafter(F32(1), F32(0)))
        self.film, self.lens = np.ascontiguousarray(film), np.ascontiguousarray(lens)
        # the rays of the camera at the start of its motion and (odd lanes) at its end, at times at and beyond those ends
        even = np.arange(N) % 2 == 0
        rays = self.gs.camera_rays(self.still(0), film, lens)
        if rd.camera_animated:
            rays = np.where(even, rays, self.gs.camera_rays(self.still(1), film, lens))
            t0, t1 = F32(rd.camera_time[0]), F32(rd.camera_time[1])
            time = np.where(even, np.where(np.arange(N) % 4 == 0, t0, t0 - F32(0.5)), np.where(np.arange(N) % 4 == 1, t1, t1 + F32(0.75))).astype(F32)
        else: time = rng.random(N).astype(F32)
        o, d = rays["o"].copy(), rays["d"].copy()
        # backwards, perpendicular to the camera's axis, and with an unnormalised d
        axis_x = xform_vec(np.array(rd.camera_to_world[:], F32), v3(1, 0, 0, 1))[0]
        d[40:48] = -d[40:48]
        d[48:52] = axis_x
        d[52:56] = -axis_x
        d[56:80] *= rng.uniform(0.25, 4, (24, 1)).astype(F32)
        self.o, self.d, self.time = np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(time)
        # reference points: the hits of camera rays, the hits of rays spawned from those hits, and hand-filled medium vertices (n = 0)
        inside = (rng.random((N, 2)) * [sb[2] - sb[0], sb[3] - sb[1]] + [sb[0], sb[1]]).astype(F32)
        cam = self.gs.camera_rays(self.still(0), inside, lens)
        first = self.gs.intersect_at(cam["o"], cam["d"], cam["t_max"], time)
        hit = first["prim"] >= 0
        bounce = rng.normal(size=(N, 3)).astype(F32)
        second = self.gs.intersect_at(first["p"] + bounce * F32(0.01), bounce, np.full(N, np.inf, F32), time)
        ref = np.where(np.arange(N) % 3 == 1, second, first)
        lo, hi = self.host.nodes()["bmin"][0], self.host.nodes()["bmax"][0]
        medium = np.zeros(N, gpu.INTERACTION_DTYPE)
        medium["p"] = (lo - 0.6 * (hi - lo) + 2.2 * (hi - lo) * rng.random((N, 3))).astype(F32)  # in and around the scene, behind the camera too
        medium["p"][8::9, 2] = lo[2] - F32(2.5) * (hi[2] - lo[2])  # ... and some well behind it (the cameras look along +z from z = -800)
        ref = np.where(np.arange(N) % 3 == 2, medium, ref)
        ref["time"] = time
        self.ref, self.u = np.ascontiguousarray(ref), np.ascontiguousarray(np.minimum(rng.random((N, 2)).astype(F32), np.nextafter(F32(1), F32(0))))
        assert hit.sum() > N // 2 and (ref["prim"] < 0).sum() >= 1  # (rays that escaped: invalid reference points)

    def still(self, end):
        """The camera frozen at one end of its motion (as tests/test_gpu_camera_queries.py freezes it): what Interpolate hands out there."""
        rd = self.gpu.abi.PgRenderDesc.from_buffer_copy(self.rd)
        if end: rd.camera_to_world = self.rd.camera_to_world_end
        rd.camera_animated = 0
        return rd

    def close(self):
        self.gs.close()
        self.host.close()


@pytest.fixture(scope="module")
def cases(gpu, oracle):
    made = {}

    def case(name):
        if name not in made:
            sc = made[name] = Case(gpu, name)
            sc.want_we = restate_we(sc, *matrices_at(sc, sc.time), sc.o, sc.d)
            sc.want_wi, sc.want_shadow, sc.tested = restate_sample_wi(sc, oracle, sc.ref, sc.u)
        return made[name]
    yield case
    for sc in made.values(): sc.close()


def first_bad(got, want):
    for f in got.dtype.names:
        bad = np.flatnonzero((bits(got[f]) != bits(want[f])).reshape(len(got), -1).any(1))
        if len(bad): return f, len(bad), int(bad[0]), got[f][bad[0]], want[f][bad[0]]
    return None


# ---- 1. We / Pdf_We = the restatement, every field bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_memory", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_we_equals_the_restatement(gpu, cases, name, n, device_memory):
    sc = cases(name)
    got = we_at(gpu, sc, sc.o[:n], sc.d[:n], sc.time[:n], gpu.PG_MEM_DEVICE if device_memory else gpu.PG_MEM_HOST)
    assert records_equal(got, sc.want_we[:n]), (name, n, first_bad(got, sc.want_we[:n]))


def test_the_rays_reach_every_case(cases):
    for name in SCENES:
        want = cases(name).want_we
        assert all((want["status"] == s).sum() >= 8 for s in (0, 1, 2)), (name, np.bincount(want["status"]))
        assert (want["status"][40:48] == 0).all() and (want["status"][:4] > 0).all()  # backwards; the film's corners face the camera
        assert (want["status"][48:56] < 2).all() and (want["status"][48:56] == 0).any()  # along the camera's x axis: cosTheta is 0 or rounding's, never on the film
        on_max = want[1]  # exactly on pMax: outside (>=), whatever rounding makes of the way back
        assert on_max["status"] == 1 or on_max["p_raster"][0] < cases(name).rd.sample_bounds[2]
        scaled = want[56:80]
        assert (scaled["status"] == 2).any() and not same_bits(scaled["cos_theta"], np.minimum(scaled["cos_theta"], 1))  # an unnormalised d: cosTheta > 1 occurs
    for name in MOVING:  # both ends and both sides of each are there, lane by lane
        sc = cases(name)
        t0, t1 = sc.rd.camera_time[0], sc.rd.camera_time[1]
        assert all(m.sum() >= N // 8 for m in (sc.time == F32(t0), sc.time < F32(t0), sc.time == F32(t1), sc.time > F32(t1)))
        # ... and the ends differ: the end's rays under the start's matrices are not the records
        wrong = restate_we(sc, *matrices_at(sc, np.full(N, F32(t0))), sc.o, sc.d)
        assert not records_equal(wrong, sc.want_we)


def test_we_without_time_is_time_zero(gpu, cases):
    sc = cases("camanim_translate")
    host = sc.gs.camera_we_at(sc.rd, sc.we, sc.o, sc.d)
    assert records_equal(host, sc.gs.camera_we_at(sc.rd, sc.we, sc.o, sc.d, np.zeros(N, F32))) and not records_equal(host, sc.want_we)
    assert records_equal(sc.gs.camera_we_at(sc.rd, sc.we, sc.o, sc.d, sc.time), sc.want_we)
    empty = sc.gs.camera_we_at(sc.rd, sc.we, np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    assert empty.dtype == gpu.CAMERA_IMPORTANCE_DTYPE and len(empty) == 0
    with pytest.raises(ValueError):
        sc.gs.camera_we_at(sc.rd, sc.we, sc.o, sc.d[:-1])


# ---- 2. round trip: the rays pg_camera_rays_at generates come back to their film points, between the ends too -------------------------------------------------
# The largest deviation of the RESTATEMENT (not of the device) over the end-time samples of the five scenes, measured when this test was written:
#   |p_raster - p_film| 5.995e-3 pixels (camanim_rotate's end; 1.7e-3 for the still pinhole -- the way back goes through a point ONE unit in front of a camera
#   800 units from the origin, and loses the digits of that sum; 5.7e-6 for the thin lens, whose plane of focus lies 1000 units out),
#   |We cos / (pdf_pos pdf_dir) - 1| 2.587e-7.
# Four times that is allowed.  A wrong matrix or a wrong branch is off by pixels, not by rounding.
RESTATED_RASTER, RESTATED_RATIO = 6.0e-3, 2.6e-7


def round_trip_deviation(rec, film):
    assert (rec["status"] == 2).all(), np.bincount(rec["status"])
    ratio = rec["We"].astype(np.float64) * rec["cos_theta"] / (rec["pdf_pos"].astype(np.float64) * rec["pdf_dir"])
    return np.abs(rec["p_raster"].astype(np.float64) - film).max(), np.abs(ratio - 1).max()


@pytest.mark.parametrize("name", SCENES)
def test_generated_rays_come_back_to_their_film_points(gpu, cases, name):
    sc = cases(name)
    rd = sc.rd
    rng = np.random.default_rng(77)
    sb = [float(b) for b in rd.sample_bounds]
    film = (rng.random((N, 2)) * [sb[2] - sb[0] - 0.5, sb[3] - sb[1] - 0.5] + [sb[0] + 0.25, sb[1] + 0.25]).astype(F32)  # a quarter pixel inside the bounds
    # the restatement's own deviation, at the ends of the motion
    for end in (0, 1) if rd.camera_animated else (0,):
        rays = sc.gs.camera_rays(sc.still(end), film, sc.lens)
        t = np.full(N, F32(rd.camera_time[end]) if rd.camera_animated else F32(0))
        own = round_trip_deviation(restate_we(sc, *matrices_at(sc, t), rays["o"], rays["d"]), film)
        print(name, "restatement at end", end, own)
        assert own[0] <= RESTATED_RASTER and own[1] <= RESTATED_RATIO, (name, own)
    # the device, over the whole shutter: for a moving camera most of these times lie strictly between the ends
    u_time = np.minimum(rng.random(N).astype(F32), np.nextafter(F32(1), F32(0)))
    rays = sc.gs.camera_rays(rd, film, sc.lens, u_time)
    if rd.camera_animated:
        assert ((rays["time"] > rd.camera_time[0]) & (rays["time"] < rd.camera_time[1])).sum() >= N // 3
    got = round_trip_deviation(sc.gs.camera_we_at(rd, sc.we, rays["o"], rays["d"], rays["time"]), film)
    print(name, "device over the shutter", got)
    assert got[0] <= 4 * RESTATED_RASTER and got[1] <= 4 * RESTATED_RATIO, (name, got)


# ---- 3. Sample_Wi = the restatement; 4. visibility = pg_intersect_p_at of the reported ray ----------------------------------------------------------------------
@pytest.mark.parametrize("device_memory", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_sample_wi_equals_the_restatement(gpu, cases, name, n, device_memory):
    sc = cases(name)
    mem = gpu.PG_MEM_DEVICE if device_memory else gpu.PG_MEM_HOST
    got, shadow = sample_wi_at(gpu, sc, sc.ref[:n], sc.u[:n], mem)
    want = sc.want_wi[:n].copy()
    want["visibility"] = got["visibility"]  # (test 4's)
    assert records_equal(got, want), (name, n, first_bad(got, want))
    assert same_bits(shadow, sc.want_shadow[:n]), (name, n, np.flatnonzero((bits(shadow) != bits(sc.want_shadow[:n])).any(1))[:4])
    tested = sc.tested[:n]
    assert ((got["visibility"] >= 0) == tested).all() and (got["visibility"][~tested] == -1).all() and not shadow[~tested].any()
    if tested.any():
        occ = sc.gs.intersect_p_at(shadow[tested, 0:3], shadow[tested, 4:7], shadow[tested, 3], shadow[tested, 7])
        assert np.array_equal(got["visibility"][tested], 1 - occ.astype(np.int32)), name
    assert records_equal(sample_wi_at(gpu, sc, sc.ref[:n], sc.u[:n], mem, shadow=False), got)  # shadow = NULL


def test_the_reference_points_reach_every_case(gpu, oracle, cases):
    for name in SCENES:
        sc = cases(name)
        got, shadow = sc.gs.camera_sample_wi_at(sc.rd, sc.we, sc.ref, sc.u, with_shadow_rays=True)
        assert got.dtype == gpu.CAMERA_SAMPLE_DTYPE
        vis = got["visibility"]
        assert all((vis == v).sum() >= 8 for v in (-1, 0, 1)), (name, np.bincount(vis + 1))  # not tested, occluded, visible
        assert all((got["status"] == s).sum() >= 1 for s in (-1, 0, 2)), (name, np.bincount(got["status"] + 1))
        medium = ~sc.ref["n"].any(1) & (sc.ref["prim"] >= 0)
        assert (vis[medium] >= 0).sum() >= 8 and (vis[~medium] >= 0).sum() >= 8  # medium vertices and surface points are both tested
        assert (sc.ref["p_error"][sc.tested].any(1)).sum() >= 8  # ... through a SpawnRayTo that has an error bound to step over
        if not sc.rd.camera_animated:  # the oracle's IntersectP (which knows no time) agrees: visible and occluded points both occur
            t = sc.tested
            occ = oracle.intersect_p(sc.host.desc, shadow[t, 0:3], shadow[t, 4:7], shadow[t, 3])[0]
            assert occ.any() and not occ.all() and np.array_equal(vis[t], 1 - np.asarray(occ, np.int32)), name
    with pytest.raises(ValueError):
        sc.gs.camera_sample_wi_at(sc.rd, sc.we, sc.ref, sc.u[:-1])


# ---- 5. counters --------------------------------------------------------------------------------------------------------------------------------------------------
def test_counters(gpu, cases):
    sc = cases("camanim_rotate")
    gs = sc.gs
    gs.counters_reset()
    gs.camera_we_at(sc.rd, sc.we, sc.o, sc.d, sc.time)
    cn = gs.counters()
    assert all(v == 0 for k, v in cn.items() if not k.endswith("_ms")), cn  # We traces nothing and moves nothing
    got = gs.camera_sample_wi_at(sc.rd, sc.we, sc.ref, sc.u)
    cn = gs.counters()
    tested = int((got["visibility"] >= 0).sum())
    assert tested == sc.tested.sum() >= 100
    assert cn["shadow_rays"] == tested and cn["shadow_launches"] == 1 and cn["shadow_node_visits"] > 0 and cn["shadow_tri_tests"] > 0
    moved = {"shadow_rays", "shadow_launches", "shadow_node_visits", "shadow_tri_tests", "node_visits", "tri_tests"}
    assert all(v == 0 for k, v in cn.items() if k not in moved and not k.endswith("_ms")), cn
    # the any-hit statistics are pg_intersect_p_at's for the same rays
    _, shadow = gs.camera_sample_wi_at(sc.rd, sc.we, sc.ref, sc.u, with_shadow_rays=True)
    t = sc.tested
    gs.counters_reset()
    gs.intersect_p_at(shadow[t, 0:3], shadow[t, 4:7], shadow[t, 3], shadow[t, 7])
    again = gs.counters()
    assert all(again[k] == cn[k] for k in moved), (again, cn)
    # a batch without a valid reference point: one launch, nothing traced
    gs.counters_reset()
    miss = np.zeros(65, gpu.INTERACTION_DTYPE)
    miss["prim"] = -1
    got, shadow = gs.camera_sample_wi_at(sc.rd, sc.we, miss, sc.u[:65], with_shadow_rays=True)
    want = np.zeros(65, gpu.CAMERA_SAMPLE_DTYPE)
    want["status"] = want["visibility"] = -1
    assert records_equal(got, want) and not shadow.any()
    cn = gs.counters()
    assert cn["shadow_rays"] == 0 and cn["shadow_launches"] == 1 and cn["shadow_node_visits"] == 0


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["camanim_ortho", "camanim_env", os.path.join("realistic", "a_singlet")])
def test_other_cameras_are_refused(gpu, cases, name):
    host = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
    rd = host.render_desc()
    assert rd.camera_type != 0 and host.camera_we_desc() is None
    gs = gpu.GpuScene(host.desc)
    gs.counters_reset()
    sc = cases("cornell_32")
    for call in (lambda: gs.camera_we_at(rd, sc.we, sc.o, sc.d), lambda: gs.camera_sample_wi_at(rd, sc.we, sc.ref, sc.u)):
        with pytest.raises(gpu.PbrtGpuError, match=r"\(-2\).*perspective camera"):
            call()
    cn = gs.counters()
    assert all(v == 0 for k, v in cn.items() if not k.endswith("_ms")), cn
    gs.close()
    host.close()
