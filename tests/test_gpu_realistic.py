"""Camera "realistic" on the device (camera_type 3, ABI 30): every fixture of tests/golden/realistic -- scenes the UNMODIFIED reference binary rendered
(tools/make_realistic_goldens.py) -- must come out as the reference's image in every bit, with its ray counters, its integrator statistics and its
"Rays vignetted by lens system" numbers, in both shadow-ray orders and in the launch mode the benchmark times.  Then: tile shards merge to the
one-shard film, and frames of different cameras on ONE scene handle equal frames on fresh handles (the per-frame weights and lens table)."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLD, check_integrator_stats

pytestmark = pytest.mark.gpu
REAL = os.path.join(GOLD, "realistic")
NAMES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(REAL, "*.json")))
MODES = (("reference", 0), ("free", 0), ("free", 1))  # (shadow-ray order, PG_OPT_OVERLAP_SHADOW): the last is what bench.py times
_scenes = {}


def host_scene(gpu, name, folder=REAL):
    """Parsed once per session: focusing a lens and bounding its 64 exit pupils takes the host seconds."""
    if name not in _scenes:
        _scenes[name] = gpu.HostScene(os.path.join(folder, name + ".pbrt"))
    return _scenes[name]


def image_of(scene, rd, film, strays):
    scene.film_clear()
    scene.film_merge(rd, film, strays)
    return scene.film_image()


def test_fixtures_exist():
    assert len(NAMES) >= 11 and all(os.path.exists(os.path.join(REAL, n + ".pfm")) for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_the_reference_image_bit_for_bit(gpu, monkeypatch, name):
    scene = host_scene(gpu, name)
    ref = gpu.read_pfm(os.path.join(REAL, name + ".pfm"))
    stats = json.load(open(os.path.join(REAL, name + ".json")))
    rd = scene.render_desc()
    assert rd.camera_type == 3
    for order, overlap in MODES:
        monkeypatch.setenv("PG_ANYHIT_ORDER", order)
        gs = gpu.GpuScene(scene.desc)
        try:
            gs.set_option(gpu.abi.PG_OPT_OVERLAP_SHADOW, overlap)
            film, strays = gs.render(rd)
            cn = gs.counters()
        finally:
            gs.close()
        img = image_of(scene, rd, film, strays)
        differing = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
        assert img.shape == ref.shape and differing == 0, (name, order, overlap, differing, float(np.abs(img - ref).max()))
        for k in ("camera_rays", "closest_rays", "shadow_rays", "lens_rays_total", "lens_rays_vignetted"):
            assert cn[k] == stats[k], (name, order, overlap, k, cn[k], stats[k])
        check_integrator_stats(cn, stats)


def test_three_tile_shards_merge_to_the_one_shard_film(gpu):
    """Scene (b): the gathering film with weights; 2 x 2 tiles over 3 shards."""
    scene = host_scene(gpu, "b_weighted_gaussian")
    gs = gpu.GpuScene(scene.desc)
    try:
        full = scene.render_desc()
        film, strays = gs.render(full)
        one = image_of(scene, full, film, strays).copy()
        shards = []
        for r in range(3):
            srd = scene.render_desc(tile_first=r, tile_step=3)
            shards.append(gs.render(srd))
    finally:
        gs.close()
    scene.film_clear()
    scene.film_merge_shards(full, shards)
    merged = scene.film_image()
    assert np.array_equal(one.view(np.uint32), merged.view(np.uint32))
    assert np.array_equal(one.view(np.uint32), gpu.read_pfm(os.path.join(REAL, "b_weighted_gaussian.pfm")).view(np.uint32))


def test_cameras_take_turns_on_one_scene_handle(gpu):
    """A realistic frame, a perspective frame and a realistic frame with another lens on the SAME handle, each against a fresh handle: the weight array
    and the lens table belong to a frame, not to the scene.  (The three scenes are one Cornell box: one geometry, one Halton table.)"""
    a, e = host_scene(gpu, "a_singlet"), host_scene(gpu, "e_dgauss")
    p = host_scene(gpu, "cornell_32", GOLD)
    frames = [(a, a.render_desc()), (p, p.render_desc()), (e, e.render_desc())]
    assert [rd.camera_type for _, rd in frames] == [3, 0, 3]
    shared = gpu.GpuScene(a.desc)
    try:
        for scene, rd in frames:
            film, strays = shared.render(rd)
            fresh = gpu.GpuScene(a.desc)
            try:
                film2, strays2 = fresh.render(rd)
            finally:
                fresh.close()
            assert np.array_equal(film["rgb"].view(np.uint32), film2["rgb"].view(np.uint32)) and np.array_equal(film["weight"], film2["weight"])
            assert len(strays) == len(strays2)
            if scene is not p:  # (and the realistic frames are the reference's images)
                ref = gpu.read_pfm(os.path.join(REAL, ("a_singlet" if scene is a else "e_dgauss") + ".pfm"))
                assert np.array_equal(image_of(scene, rd, film, strays).view(np.uint32), ref.view(np.uint32))
    finally:
        shared.close()


def test_a_caller_compiled_against_abi_29_still_renders(gpu):
    """ABI 30 only appended to PgRenderDesc and PgCounters: a caller built against ABI 29 (a host application, the reference-side binding) that meets the
    new library owns shorter structs.  Its frame equals the ABI 30 caller's, nothing behind its description is needed and nothing behind its counters written."""
    import ctypes as C
    abi, lib = gpu.abi, gpu.gpu_lib()
    scene = host_scene(gpu, "cornell_32", GOLD)
    rd = scene.render_desc()
    gs = gpu.GpuScene(scene.desc)
    try:
        film, strays = gs.render(rd)
        want = gs.counters()
    finally:
        gs.close()
    head = abi.PgRenderDesc.n_lens_interfaces.offset
    old_rd = (C.c_ubyte * head).from_buffer_copy(bytes(rd)[:head])  # exactly what such a caller owns
    C.cast(old_rd, C.POINTER(C.c_int32))[0] = 29
    old_scene = abi.PgSceneDesc.from_buffer_copy(scene.desc)
    old_scene.abi_version = 29
    h = C.c_void_p()
    assert lib.pg_scene_create(C.byref(old_scene), C.byref(h)) == abi.PG_OK, lib.pg_last_error()
    try:
        n = lib.pg_render_tile_count(C.cast(old_rd, C.POINTER(abi.PgRenderDesc)))
        film2 = np.zeros(n * rd.tile_pixels, gpu.FILM_PIXEL_DTYPE)
        strays2 = np.zeros(4096, gpu.STRAY_DTYPE)
        ns = C.c_int32(0)
        assert lib.pg_render(h, C.cast(old_rd, C.POINTER(abi.PgRenderDesc)), film2.ctypes.data, strays2.ctypes.data, 4096, C.byref(ns), abi.PG_MEM_HOST, None) == abi.PG_OK, lib.pg_last_error()
        room = abi.PgCounters.lens_rays_total.offset
        cn = (C.c_ubyte * (room + 16))(*([0xA5] * (room + 16)))
        assert lib.pg_counters(h, C.cast(cn, C.POINTER(abi.PgCounters))) == abi.PG_OK
    finally:
        lib.pg_scene_destroy(h)
    assert np.array_equal(film["rgb"].view(np.uint32), film2["rgb"].view(np.uint32)) and np.array_equal(film["weight"], film2["weight"]) and ns.value == len(strays)
    assert bytes(cn)[room:] == b"\xa5" * 16
    got = abi.PgCounters.from_buffer_copy(bytes(cn)[:room] + bytes(16))
    for k in ("camera_rays", "closest_rays", "shadow_rays", "paths_total", "path_length_sum"):
        assert getattr(got, k) == want[k], k
    bad = abi.PgSceneDesc.from_buffer_copy(scene.desc)
    bad.abi_version = 28
    assert lib.pg_scene_create(C.byref(bad), C.byref(h)) != abi.PG_OK and b"ABI version 28, expected 30" in lib.pg_last_error()
