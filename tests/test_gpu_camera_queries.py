"""The camera queries (csrc/pg_cameraquery.h): pg_camera_rays_at -- Camera::GenerateRayDifferential for a batch of CameraSamples, as PgCameraRay records --
and pg_scatter_f_diff_at / pg_scatter_sample_diff_at -- the scattering queries for rays that carry differentials.

Main rays are pinned to oracle_generate_ray bit for bit, the differentials of the perspective and orthographic cameras to a float32 NumPy restatement of
perspective.cpp:117-140 / orthographic.cpp:95-113 with Transform::operator() and ScaleDifferentials, the environment camera's to the finite difference
of camera.cpp:52-93 formed from oracle_generate_ray.  A moving camera's shutter ends equal the still cameras under its two transforms; the realistic
camera's records keep their invariants and move the lens statistics as a frame does.  The last test assembles two directlighting frames of textured,
bump-mapped scenes from query calls alone and requires the device's own film -- and the reference binary's image -- in every bit: it fails without the
differentials.  tests/test_emulated_camera_queries.py runs this file without a GPU."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
F32 = np.float32
CQ = os.path.join(GOLD, "camera_queries")
REAL = os.path.join(GOLD, "realistic")
ONE_MINUS_EPS = np.nextafter(F32(1), F32(0))
NON_SPECULAR = 31 & ~16
PAD = 256  # guard bytes on either side of a device output


def _load(filename):
    spec = importlib.util.spec_from_file_location(filename[:-3] + "_helpers", os.path.join(os.path.dirname(__file__), filename))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GS = _load("test_gpu_scatter.py")
records_equal, first_difference, ray_set, DeviceArrays, bits, same_bits = _GS.records_equal, _GS.first_difference, _GS.ray_set, _GS.DeviceArrays, _GS.bits, _GS.same_bits

# ---- 1. the three simple cameras: main rays = the oracle's, differentials = the restatement ---------------------------------------------------------------
CAM_SCENE = """
LookAt 1 2 -6  0.2 0.1 0  0.1 1 0.05
Camera %s
Film "image" "integer xresolution" [ 20 ] "integer yresolution" [ 12 ] "string filename" "cam.pfm"
Sampler "halton" "integer pixelsamples" [ 3 ]
WorldBegin
LightSource "point" "point from" [ 0 0 -5 ]
Material "matte"
Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point P" [ -2 -2 0  2 -2 0  2 2 0  -2 2 0 ]
WorldEnd
"""
SHUTTER = ' "float shutteropen" [ 0.25 ] "float shutterclose" [ 0.75 ]'
CAMERAS = {"pinhole": '"perspective" "float fov" [ 45 ]',
           "thinlens": '"perspective" "float fov" [ 45 ] "float lensradius" [ 0.3 ] "float focaldistance" [ 5 ]' + SHUTTER,
           "ortho": '"orthographic" "float screenwindow" [ -3 3 -2 2 ]' + SHUTTER,
           "ortho_lens": '"orthographic" "float screenwindow" [ -3 3 -2 2 ] "float lensradius" [ 0.2 ] "float focaldistance" [ 4 ]',
           "environment": '"environment"'}
N_SAMPLES = 333  # not a multiple of the block size; more than one block


def camera_samples(w, h, seed, n=N_SAMPLES):
    """n CameraSamples over (and around) a w x h film: pixel corners, points outside the image, pLens at 0 and next to 1, u_time at 0 and next to 1."""
    rng = np.random.default_rng(seed)
    film = (rng.random((n, 2)) * [w, h]).astype(F32)
    lens = np.minimum(rng.random((n, 2)).astype(F32), ONE_MINUS_EPS)
    time = np.minimum(rng.random(n).astype(F32), ONE_MINUS_EPS)
    special = [(0, 0), (w, 0), (0, h), (w, h), (7, 5), (w / 2, h / 2), (-3.5, 2.25), (w + 7.25, h + 1.5), (5.5, -4), (-0.125, h + 0.5)]
    film[:len(special)] = special
    lens[1], lens[3], lens[11], lens[12], lens[13] = (0, 0), (ONE_MINUS_EPS, ONE_MINUS_EPS), (0, 0), (ONE_MINUS_EPS, 0), (0.5, 0.5)
    time[0], time[2], time[14] = 0, ONE_MINUS_EPS, 0
    assert n % 256 != 0 and n > 256
    return np.ascontiguousarray(film), np.ascontiguousarray(lens), np.ascontiguousarray(time)


def oracle_rays(oracle, rd, film, lens):
    """oracle_generate_ray per sample: (n, 7) float32 -- o, d, tMax."""
    L = oracle.lib()
    out = np.zeros((len(film), 7), F32)
    a = np.zeros(7, F32)
    for i in range(len(film)):
        L.oracle_generate_ray(C.byref(rd), float(film[i, 0]), float(film[i, 1]), float(lens[i, 0]), float(lens[i, 1]), a.ctypes.data)
        out[i] = a
    return out


# float32, every operation in the order csrc/pg_camera.h and csrc/pg_device.h write it (the kernels are built without contraction)
def v3(x, y, z, n):
    return np.stack([np.broadcast_to(F32(x), (n,)), np.broadcast_to(F32(y), (n,)), np.broadcast_to(F32(z), (n,))], 1).astype(F32)


def xform_point(m, p):  # transform.h:219-231
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    xp = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
    yp = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
    zp = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
    wp = ((m[12] * x + m[13] * y) + m[14] * z) + m[15]
    inv = F32(1) / wp
    return np.where((wp == 1)[:, None], np.stack([xp, yp, zp], 1), np.stack([inv * xp, inv * yp, inv * zp], 1))


def xform_vec(m, v):  # transform.h:233-239
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([(m[0] * x + m[1] * y) + m[2] * z, (m[4] * x + m[5] * y) + m[6] * z, (m[8] * x + m[9] * y) + m[10] * z], 1)


def normalize32(a):  # geometry.h:984-986, :243-248
    inv = F32(1) / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a * inv[:, None]


def concentric_sample_disk(u):
    """sampling.cpp:113-130 with the host libm's sinf / cosf -- the `oracle` fixture has checked that they are the ones the device restates."""
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = libm.cosf.restype = C.c_float
    libm.sinf.argtypes = libm.cosf.argtypes = [C.c_float]
    out = np.zeros((len(u), 2), F32)
    pi4, pi2 = F32(0.78539816339744830961), F32(1.57079632679489661923)
    for i in range(len(u)):
        ox, oy = F32(2) * u[i, 0] - F32(1), F32(2) * u[i, 1] - F32(1)
        if ox == 0 and oy == 0: continue
        if abs(ox) > abs(oy): r, theta = ox, pi4 * (oy / ox)
        else: r, theta = oy, pi2 - pi4 * (ox / oy)
        out[i] = (r * F32(libm.cosf(theta)), r * F32(libm.sinf(theta)))
    return out


def restated_differentials(rd, film, lens, o, d):
    """GenerateRayDifferential's rxOrigin, rxDirection, ryOrigin, ryDirection of the perspective / orthographic camera (perspective.cpp:117-140,
    orthographic.cpp:95-113), carried to world space (transform.h:264-273) and scaled by 1 / sqrt(spp) about the main ray (o, d) (geometry.h:908-913)."""
    n = len(film)
    r2c, c2w = np.array(rd.raster_to_camera[:], F32), np.array(rd.camera_to_world[:], F32)
    dxc, dyc = np.array(rd.dx_camera[:], F32)[None, :], np.array(rd.dy_camera[:], F32)[None, :]
    radius, focal = F32(rd.lens_radius), F32(rd.focal_distance)
    p_camera = xform_point(r2c, np.stack([film[:, 0], film[:, 1], np.zeros(n, F32)], 1))
    zero = v3(0, 0, 0, n)
    p_lens = np.concatenate([radius * concentric_sample_disk(lens), np.zeros((n, 1), F32)], 1) if radius > 0 else zero
    if rd.camera_type == 0:
        if radius > 0:
            out = []
            for shift in (dxc, dyc):
                dirn = normalize32(p_camera + shift)
                ft = focal / dirn[:, 2]
                p_focus = zero + dirn * ft[:, None]
                out += [p_lens, normalize32(p_focus - p_lens)]
            rxo, rxd, ryo, ryd = out
        else: rxo, rxd, ryo, ryd = zero, normalize32(p_camera + dxc), zero, normalize32(p_camera + dyc)
    else:
        assert rd.camera_type == 1
        co, cd = p_camera, v3(0, 0, 1, n)
        if radius > 0:  # the main ray's direction after the lens (orthographic.cpp:80-93): ft below is computed from IT
            ft = focal / cd[:, 2]
            cd = normalize32((co + cd * ft[:, None]) - p_lens)
            ft = focal / cd[:, 2]
            along = v3(0, 0, 1, n) * ft[:, None]
            rxo, rxd = p_lens, normalize32(((p_camera + dxc) + along) - p_lens)
            ryo, ryd = p_lens, normalize32(((p_camera + dyc) + along) - p_lens)
        else: rxo, rxd, ryo, ryd = co + dxc, cd, co + dyc, cd
    rxo, ryo, rxd, ryd = xform_point(c2w, rxo), xform_point(c2w, ryo), xform_vec(c2w, rxd), xform_vec(c2w, ryd)
    s = F32(1) / np.sqrt(F32(rd.spp))
    got = np.concatenate([o + (rxo - o) * s, d + (rxd - d) * s, o + (ryo - o) * s, d + (ryd - d) * s], 1)
    assert got.dtype == F32
    return got


def finite_difference_differentials(oracle, rd, film, lens, o, d):
    """Camera::GenerateRayDifferential, camera.cpp:52-93 (the environment camera inherits it): rays at pFilm + (.05, 0) and + (0, .05), then ScaleDifferentials."""
    eps = F32(0.05)
    inv = F32(1) / eps
    sx = oracle_rays(oracle, rd, film + np.array([eps, 0], F32), lens)
    sy = oracle_rays(oracle, rd, film + np.array([0, eps], F32), lens)
    parts = [o + (sx[:, 0:3] - o) * inv, d + (sx[:, 3:6] - d) * inv, o + (sy[:, 0:3] - o) * inv, d + (sy[:, 3:6] - d) * inv]
    s = F32(1) / np.sqrt(F32(rd.spp))
    return np.concatenate([o + (parts[0] - o) * s, d + (parts[1] - d) * s, o + (parts[2] - o) * s, d + (parts[3] - d) * s], 1)


def lerp_time(rd, u):  # Lerp(sample.time, shutterOpen, shutterClose), pbrt.h:417
    return (F32(1) - u) * F32(rd.shutter_open) + u * F32(rd.shutter_close)


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_simple_cameras_equal_the_oracle_and_the_restatement(gpu, oracle, name):
    scene = gpu.HostScene(text=CAM_SCENE % CAMERAS[name])
    rd = scene.render_desc()
    assert rd.camera_type == {"pinhole": 0, "thinlens": 0, "ortho": 1, "ortho_lens": 1, "environment": 2}[name] and rd.spp == 3 and not rd.camera_animated
    assert (rd.lens_radius > 0) == (name in ("thinlens", "ortho_lens"))
    film, lens, time = camera_samples(20, 12, 11)
    gs = gpu.GpuScene(scene.desc)
    gs.counters_reset()
    rec = gs.camera_rays(rd, film, lens, time)
    assert rec.dtype == gpu.CAMERA_RAY_DTYPE and len(rec) == N_SAMPLES
    want = oracle_rays(oracle, rd, film, lens)
    assert same_bits(rec["o"], want[:, 0:3]) and same_bits(rec["d"], want[:, 3:6]) and same_bits(rec["t_max"], want[:, 6])
    assert (rec["weight"] == 1).all() and (rec["has_differentials"] == 1).all() and (rec["medium"] == rd.camera_medium).all() and not rec["reserved"].any()
    assert same_bits(rec["time"], lerp_time(rd, time))
    if name == "environment": diff = finite_difference_differentials(oracle, rd, film, lens, rec["o"], rec["d"])
    else: diff = restated_differentials(rd, film, lens, rec["o"], rec["d"])
    bad = np.flatnonzero((bits(rec["differentials"]) != bits(diff)).any(1))
    assert len(bad) == 0, (name, len(bad), bad[:5], rec["differentials"][bad[:1]], diff[bad[:1]])
    assert (bits(rec["differentials"][:, 0:3]) != bits(rec["o"])).any() or (bits(rec["differentials"][:, 3:6]) != bits(rec["d"])).any()
    # batches: a prefix of one sample, NULL pLens / u_time = zeros, and the empty batch; no counter moves
    one = gs.camera_rays(rd, film[:1], lens[:1], time[:1])
    assert records_equal(one, rec[:1])
    zeros = gs.camera_rays(rd, film, np.zeros_like(lens), np.zeros_like(time))
    assert records_equal(gs.camera_rays(rd, film), zeros)
    if rd.lens_radius == 0:  # a pinhole ignores pLens
        assert same_bits(zeros["o"], rec["o"]) and same_bits(zeros["differentials"], rec["differentials"])
    else: assert not same_bits(zeros["o"], rec["o"])
    empty = gs.camera_rays(rd, np.zeros((0, 2), F32))
    assert empty.dtype == gpu.CAMERA_RAY_DTYPE and len(empty) == 0
    cn = gs.counters()
    assert all(v == 0 for k, v in cn.items() if not k.endswith("_ms")), cn
    with pytest.raises(ValueError):
        gs.camera_rays(rd, film, lens[:-1])
    bad_rd = gpu.abi.PgRenderDesc.from_buffer_copy(rd)
    bad_rd.camera_medium = 3  # the scene has no media: refused against the SCENE's facts, with pg_render's text
    with pytest.raises(gpu.PbrtGpuError, match="camera_medium 3 out of range"):
        gs.camera_rays(bad_rd, film)
    gs.close()
    scene.close()


# ---- 2. a moving camera -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["camanim_rotate", "camanim_ortho", "camanim_env"])
def test_a_moving_cameras_shutter_ends_are_the_still_cameras(gpu, name):
    scene = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
    rd = scene.render_desc()
    assert rd.camera_animated and rd.shutter_open == rd.camera_time[0] and rd.shutter_close == rd.camera_time[1]
    w, h = scene.film_size
    film, lens, _ = camera_samples(w, h, 23)
    n = len(film)
    gs = gpu.GpuScene(scene.desc)
    still = []
    for end in (0, 1):
        srd = gpu.abi.PgRenderDesc.from_buffer_copy(rd)
        srd.camera_animated = 0
        if end:
            for k in range(16): srd.camera_to_world[k] = rd.camera_to_world_end[k]
        still.append(gs.camera_rays(srd, film, lens, np.full(n, end, F32)))
    at = [gs.camera_rays(rd, film, lens, np.full(n, t, F32)) for t in (0, 1)]
    assert records_equal(at[0], still[0]), first_difference(at[0], still[0])
    assert records_equal(at[1], still[1]), first_difference(at[1], still[1])
    ray = lambda r: np.concatenate([bits(r["o"]), bits(r["d"])], 1)
    assert (ray(at[0]) != ray(at[1])).any(1).sum() > n // 2  # the camera does move
    mid = gs.camera_rays(rd, film, lens, np.full(n, 0.375, F32))
    assert (ray(mid) != ray(at[0])).any(1).sum() > n // 2 and (ray(mid) != ray(at[1])).any(1).sum() > n // 2  # ... and is interpolated in between
    u = np.array([0, 1, 0.375], F32)[np.arange(n) % 3]
    mixed = gs.camera_rays(rd, film, lens, u)
    want = np.where(np.arange(n) % 3 == 0, at[0], np.where(np.arange(n) % 3 == 1, at[1], mid))
    assert records_equal(mixed, want), first_difference(mixed, want)
    assert same_bits(mixed["time"], lerp_time(rd, u))
    gs.close()
    scene.close()


# ---- 3. the realistic camera --------------------------------------------------------------------------------------------------------------------------------
def frame_samples(oracle, scene, rd, dims=5):
    """The camera samples of one frame under a GlobalSampler: pixel, sample number and dimensions 0 .. dims-1 of every sample of every pixel (GetCameraSample,
    sampler.cpp:46-52: pFilm = pixel + Get2D(), time = Get1D(), pLens = Get2D()); further dimensions are what Li draws next."""
    L = oracle.lib()
    sb, pb = rd.sample_bounds, rd.pixel_bounds
    px, py, u = [], [], []
    for y in range(max(sb[1], pb[1]), min(sb[3], pb[3])):
        for x in range(max(sb[0], pb[0]), min(sb[2], pb[2])):
            for k in range(rd.spp):
                px.append(x); py.append(y)
                u.append([L.oracle_sampler_dimension(scene.desc, rd, x, y, k, dim) for dim in range(dims)])
    u = np.array(u, F32)
    film = np.stack([np.array(px, F32) + u[:, 0], np.array(py, F32) + u[:, 1]], 1)
    return np.array(px), np.array(py), np.ascontiguousarray(film), np.ascontiguousarray(u[:, 3:5]), np.ascontiguousarray(u[:, 2]), u


@pytest.mark.parametrize("name", ["d_clamped_aperture", "j_moving"])
def test_realistic_records_and_lens_statistics(gpu, oracle, name):
    scene = gpu.HostScene(os.path.join(REAL, name + ".pbrt"))
    rd = scene.render_desc()
    assert rd.camera_type == 3 and bool(rd.camera_animated) == (name == "j_moving") and rd.sampler == 0
    _, _, film, lens, time, _ = frame_samples(oracle, scene, rd)
    n = len(film)
    assert n % 256 == 0  # (whole tiles; the sample sets above are the ones that end inside a block)
    fresh = gpu.GpuScene(scene.desc)
    fresh.render(rd)
    frame = fresh.counters()
    fresh.close()
    gs = gpu.GpuScene(scene.desc)
    gs.counters_reset()
    rec = gs.camera_rays(rd, film, lens, time)
    cn = gs.counters()
    print(name, "lens rays", cn["lens_rays_total"], "vignetted", cn["lens_rays_vignetted"], "frame", frame["lens_rays_total"], frame["lens_rays_vignetted"],
          "samples of weight 0:", int((rec["weight"] == 0).sum()), "of", n)
    assert (cn["lens_rays_total"], cn["lens_rays_vignetted"]) == (frame["lens_rays_total"], frame["lens_rays_vignetted"])
    assert cn["lens_rays_total"] >= 3 * (rec["weight"] != 0).sum() and all(v == 0 for k, v in cn.items() if not k.startswith("lens_") and not k.endswith("_ms")), cn
    assert (rec["weight"] >= 0).all()
    dead = rec["weight"] == 0
    assert dead.sum() >= 8 and (~dead).sum() >= n // 2
    assert not rec[dead].view(np.uint8).any()  # a vignetted sample: a record of zeros
    live = rec[~dead]
    assert (live["has_differentials"] == 1).all() and (live["medium"] == rd.camera_medium).all() and np.isinf(live["t_max"]).all()
    length = np.sqrt((live["d"].astype(np.float64) ** 2).sum(1))
    print(name, "max | |d| - 1 | =", np.abs(length - 1).max() / 2.0 ** -23, "ulp of 1")
    assert np.abs(length - 1).max() <= 2 * 2.0 ** -23
    assert same_bits(live["time"], lerp_time(rd, time[~dead]))
    assert np.isfinite(live["differentials"]).all() and (bits(live["differentials"][:, 3:6]) != bits(live["d"])).any()
    # device memory: the same bytes, and guard bytes on both sides of `out` intact; NULL pLens / u_time are zeros
    dev = DeviceArrays()
    pf, pl, pt = dev.put(film), dev.put(lens), dev.put(time)
    buf = dev.put(np.full(PAD + 96 * n + PAD, 0xAB, np.uint8))
    gs.camera_rays_device(rd, n, pf, pl, pt, buf + PAD)
    got = dev.get(3, np.uint8)
    assert (got[:PAD] == 0xAB).all() and (got[PAD + 96 * n:] == 0xAB).all() and len(got) == 2 * PAD + 96 * n
    assert np.array_equal(got[PAD:PAD + 96 * n], rec.view(np.uint8))
    gs.camera_rays_device(rd, 77, pf, None, None, buf + PAD)
    got = dev.get(3, np.uint8)
    assert np.array_equal(got[PAD:PAD + 96 * 77], gs.camera_rays(rd, film[:77]).view(np.uint8)) and np.array_equal(got[PAD + 96 * 77:PAD + 96 * n], rec.view(np.uint8)[96 * 77:])
    assert (got[:PAD] == 0xAB).all() and (got[PAD + 96 * n:] == 0xAB).all()
    lib = gpu.gpu_lib()
    assert lib.pg_camera_rays_at(gs._h, C.byref(rd), 4, pf, None, None, buf + PAD + 4, gpu.PG_MEM_DEVICE, None) == -1 and b"16-byte aligned" in lib.pg_last_error()
    gs.close()


# ---- 4. scattering with differentials -----------------------------------------------------------------------------------------------------------------------
def diff_call(gpu, gs, name, o, d, tmax, extra, diff, flags=31, time=None):
    """The _diff_ entry point itself on host arrays (diff may be None: the binding's methods then take the plain entry point)."""
    n = len(tmax)
    o, d, tmax, extra = (np.ascontiguousarray(a, F32) for a in (o, d, tmax, extra))
    diff = None if diff is None else np.ascontiguousarray(diff, F32)
    out, isect = np.empty(n, gpu.SCATTER_DTYPE), np.empty(n, gpu.INTERACTION_DTYPE)
    st = getattr(gpu.gpu_lib(), name)(gs._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data, extra.ctypes.data,
                                      None if diff is None else diff.ctypes.data, flags, isect.ctypes.data, out.ctypes.data, gpu.PG_MEM_HOST, None)
    assert st == 0, gpu.gpu_lib().pg_last_error()
    return out, isect


@pytest.mark.parametrize("name", ["cornell_plastic", "quadrics", "instance_boxes"])
def test_constant_materials_ignore_differentials(gpu, name):
    scene = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
    gs = gpu.GpuScene(scene.desc)
    o, d, tmax, wi, u = ray_set(scene, 91, n_random=300, aimed=100)
    n = len(tmax)
    rng = np.random.default_rng(92)
    diff = rng.normal(size=(n, 12)).astype(F32)
    diff[::5] = 0
    for plain, entry, arg in ((gs.scatter_f_at, "pg_scatter_f_diff_at", wi), (gs.scatter_sample_at, "pg_scatter_sample_diff_at", u)):
        want, want_isect = plain(o, d, tmax, arg, flags=NON_SPECULAR, with_interaction=True)
        assert (want["prim"] >= 0).sum() > n // 2
        for dd in (diff, None):
            got, got_isect = diff_call(gpu, gs, entry, o, d, tmax, arg, dd, NON_SPECULAR)
            assert records_equal(got, want) and records_equal(got_isect, want_isect), first_difference(got, want)
        assert records_equal(plain(o, d, tmax, arg, flags=NON_SPECULAR, diff=diff), want)
    gs.close()
    scene.close()


@pytest.fixture(scope="module")
def thinlens(gpu, oracle):
    """The thin-lens fixture: scene, handle, description and its frame's camera rays from the query."""
    scene = gpu.HostScene(os.path.join(CQ, "thinlens.pbrt"))
    rd = scene.render_desc()
    gs = gpu.GpuScene(scene.desc)
    px, py, film, lens, time, u = frame_samples(oracle, scene, rd, dims=7)
    cam = gs.camera_rays(rd, film, lens, time)
    yield {"scene": scene, "rd": rd, "gs": gs, "cam": cam, "px": px, "py": py, "u": u}
    gs.close()
    scene.close()


def test_textured_materials_read_the_differentials(gpu, thinlens):
    """On the fixture with an image map, a closed-form checkerboard and a bump map: NULL diff and twelve zeros are the plain call; the camera's differentials
    change f (the image map's level, the checkerboard's filter) and the bumped normal; device memory equals host memory."""
    gs, cam = thinlens["gs"], thinlens["cam"]
    assert gs is not None and (cam["weight"] == 1).all()
    n = len(cam)
    o, d, tmax, diff = (np.ascontiguousarray(cam[k]) for k in ("o", "d", "t_max", "differentials"))
    wi = np.ascontiguousarray(-d)
    u = np.random.default_rng(7).random((n, 2)).astype(F32)
    for plain, entry, arg, device in ((gs.scatter_f_at, "pg_scatter_f_diff_at", wi, gs.scatter_f_diff_at_device),
                                      (gs.scatter_sample_at, "pg_scatter_sample_diff_at", u, gs.scatter_sample_diff_at_device)):
        want, want_isect = plain(o, d, tmax, arg, flags=NON_SPECULAR, with_interaction=True)
        hit = want["n_bxdfs"] > 0
        assert hit.sum() > n * 3 // 4
        for dd in (None, np.zeros((n, 12), F32), -np.zeros((n, 12), F32)):
            got, got_isect = diff_call(gpu, gs, entry, o, d, tmax, arg, dd, NON_SPECULAR)
            assert records_equal(got, want) and records_equal(got_isect, want_isect), first_difference(got, want)
        full, full_isect = diff_call(gpu, gs, entry, o, d, tmax, arg, diff, NON_SPECULAR)
        assert records_equal(full_isect, want_isect) and records_equal(plain(o, d, tmax, arg, flags=NON_SPECULAR, diff=diff), full)
        changed_f = (bits(full["f"]) != bits(want["f"])).any(1)
        changed_n = (bits(full["shading_n"]) != bits(want["shading_n"])).any(1)
        print(entry, "hits", int(hit.sum()), "f changed at", int(changed_f.sum()), "bumped normal changed at", int(changed_n.sum()))
        assert changed_f.sum() >= 20 and changed_n.sum() >= 5 and not changed_f[~hit].any()
        assert np.array_equal(full["prim"], want["prim"]) and np.array_equal(full["types"], want["types"])
        # per ray: the rays whose twelve floats are zero take the plain path, their neighbours do not
        some = diff.copy()
        some[::2] = 0
        mixed, _ = diff_call(gpu, gs, entry, o, d, tmax, arg, some, NON_SPECULAR)
        assert records_equal(mixed, np.where(np.arange(n) % 2 == 0, want, full))
        dev = DeviceArrays()
        po, pd, pt, parg, pdiff = (dev.put(a) for a in (o, d, tmax, arg, diff))
        pout = dev.put(np.full(PAD + 64 * n + PAD, 0xAB, np.uint8))
        device(n, po, pd, pt, None, parg, pdiff, NON_SPECULAR, None, pout + PAD)
        out = dev.get(5, np.uint8)
        assert np.array_equal(out[PAD:PAD + 64 * n], full.view(np.uint8)) and (out[:PAD] == 0xAB).all() and (out[PAD + 64 * n:] == 0xAB).all()
        device(n, po, pd, pt, None, parg, None, NON_SPECULAR, None, pout + PAD)
        assert np.array_equal(dev.get(5, np.uint8)[PAD:PAD + 64 * n], want.view(np.uint8))


def test_a_checkerboard_without_antialiasing_ignores_differentials(gpu):
    """tests/test_gpu_scatter.py's two-colour checkerboard, "aamode" "none", on a matte quad: the footprint is computed and nothing reads it."""
    scene = gpu.HostScene(text=_GS.CHECKER_SCENE)
    rd = scene.render_desc()
    gs = gpu.GpuScene(scene.desc)
    film, lens, time = camera_samples(8, 8, 31)
    cam = gs.camera_rays(rd, film, lens, time)
    o, d, tmax, diff = (np.ascontiguousarray(cam[k]) for k in ("o", "d", "t_max", "differentials"))
    want = gs.scatter_f_at(o, d, tmax, -d, flags=31)
    got = gs.scatter_f_at(o, d, tmax, -d, flags=31, diff=diff)
    assert (want["n_bxdfs"] == 1).sum() > 100 and len(np.unique(want["f"][want["n_bxdfs"] == 1], axis=0)) == 2
    assert diff.any(1).all() and records_equal(got, want), first_difference(got, want)
    gs.close()
    scene.close()


# ---- 5. a frame assembled from queries = the device's own frame = the reference's image --------------------------------------------------------------------
def dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def assemble(gpu, gs, rd, cam, u, with_differentials):
    """DirectLightingIntegrator::Li with "maxdepth" 1, strategy "all" and ONE delta light, per camera sample, out of query calls:
    L = Le + f * |wi . ns| * Li / pdf where the shadow ray arrives (integrator.cpp:153-157; Ld / nSamples with nSamples = 1), then L * the camera ray's
    weight (integrator.cpp:329).  float32 NumPy, the operations in EstimateDirect's order."""
    n = len(cam)
    L = np.zeros((n, 3), F32)
    live = cam["weight"] != 0  # (Li is not called for a sample of weight 0, integrator.cpp:294-296)
    c = cam[live]
    o, d, tmax, time = (np.ascontiguousarray(c[k]) for k in ("o", "d", "t_max", "time"))
    le, isect = gs.light_le_at(o, d, tmax, time, with_interaction=True)
    ls = gs.light_sample_at(isect, np.zeros(len(c), np.int32), np.ascontiguousarray(u[live][:, 5:7]))  # uLight: dimensions 5 and 6 (a point light ignores it)
    wi = np.ascontiguousarray(ls["wi"])
    sc = gs.scatter_f_at(o, d, tmax, wi, time=time, flags=NON_SPECULAR, diff=np.ascontiguousarray(c["differentials"]) if with_differentials else None)
    assert np.array_equal(sc["prim"], isect["prim"])
    f = sc["f"] * np.abs(dot32(wi, sc["shading_n"]))[:, None]
    with np.errstate(all="ignore"):
        ld = (f * ls["Li"]) / ls["pdf"][:, None]
    ld = np.where((ls["visibility"] == 1)[:, None], ld, F32(0))
    L[live] = (le + ld) * c["weight"][:, None]
    assert L.dtype == F32
    return L, int((ls["visibility"] == 1).sum()), int(live.sum())


@pytest.mark.parametrize("name", ["thinlens", "realistic"])
def test_a_frame_assembled_from_queries_is_the_devices_frame_and_the_references_image(gpu, oracle, name):
    scene = gpu.HostScene(os.path.join(CQ, name + ".pbrt"))
    rd, dl = scene.render_desc(), scene.direct_desc()
    assert dl is not None and dl.strategy == 0 and dl.n_lights == 1 and rd.max_depth == 1 and rd.spp == 1 and rd.sampler == 0 and not rd.filter_general
    assert rd.camera_type == (3 if name == "realistic" else 0) and (name == "realistic" or rd.lens_radius > 0) and scene.film_size == (16, 16)
    ref = gpu.read_pfm(os.path.join(CQ, name + ".pfm"))
    stats = json.load(open(os.path.join(CQ, name + ".json")))
    gs = gpu.GpuScene(scene.desc)
    gs.counters_reset()
    film, strays = gs.render_direct(rd, dl)
    cn = gs.counters()
    scene.film_clear()
    scene.film_merge(rd, film, strays)
    img = scene.film_image().copy()
    print(name, {k: (cn[k], stats[k]) for k in ("camera_rays", "closest_rays", "shadow_rays")}, "strays", len(strays))
    assert img.shape == ref.shape and np.array_equal(img.view(np.uint32), ref.view(np.uint32))  # the device's frame is the reference's
    for k in ("camera_rays", "closest_rays", "shadow_rays"):
        assert cn[k] == stats[k], (k, cn[k], stats[k])
    px, py, pfilm, plens, ptime, u = frame_samples(oracle, scene, rd, dims=7)
    assert len(px) == 256 and list(rd.sample_bounds) == [0, 0, 16, 16]
    cam = gs.camera_rays(rd, pfilm, plens, ptime)
    pixel = py * 16 + px  # one 16 x 16 tile: the film's entries are its pixels, row by row
    assert len(film) == 256 and np.array_equal(np.sort(pixel), np.arange(256))
    out = {}
    for with_differentials in (True, False):
        L, n_visible, n_live = assemble(gpu, gs, rd, cam, u, with_differentials)
        rgb = np.zeros((256, 3), F32)
        rgb[pixel] = L
        out[with_differentials] = rgb
    assert n_live == stats["closest_rays"] and n_visible <= stats["shadow_rays"]
    differing = (bits(out[True]) != bits(film["rgb"])).any(1)
    print(name, "pixels differing from the device's film: with differentials", int(differing.sum()), "without", int((bits(out[False]) != bits(film["rgb"])).any(1).sum()),
          "lit pixels", n_visible, "samples of weight 0", 256 - n_live)
    assert not differing.any(), (name, np.flatnonzero(differing)[:8], out[True][differing][:2], film["rgb"][differing][:2])
    assert (bits(out[False]) != bits(film["rgb"])).any(1).sum() >= 1  # the differentials are what closes the gap
    assert (film["rgb"] != 0).any(1).sum() >= 100
    # ... and merged by the host's Film it is the reference binary's image
    mine = film.copy()
    mine["rgb"] = out[True]
    scene.film_clear()
    scene.film_merge(rd, mine, strays)
    assert np.array_equal(scene.film_image().view(np.uint32), ref.view(np.uint32))
    gs.close()
    scene.close()
