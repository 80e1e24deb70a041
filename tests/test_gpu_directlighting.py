"""Integrator "directlighting" on the device (pg_render_direct): every fixture of tests/golden/directlighting -- scenes the UNMODIFIED reference binary
rendered (tools/make_directlighting_goldens.py) -- must come out as the reference's image in every bit, with its ray counters and none of the path
integrators' statistics, in both shadow-ray orders and with PG_OPT_OVERLAP_SHADOW set (which these frames accept and ignore: their launches run on one stream).  Then: tile shards merge to the one-shard film, frames of
the two integrator families take turns on ONE scene handle, and descriptions outside what is built are refused with their text and no frame."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
DIRECT = os.path.join(GOLD, "directlighting")
NAMES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(DIRECT, "*.json")))
MODES = (("reference", 0), ("free", 0), ("free", 1))  # (shadow-ray order, PG_OPT_OVERLAP_SHADOW): the option must change nothing here
_scenes = {}


def host_scene(gpu, name, folder=DIRECT):
    if (folder, name) not in _scenes:
        _scenes[folder, name] = gpu.HostScene(os.path.join(folder, name + ".pbrt"))
    return _scenes[folder, name]


def image_of(scene, rd, film, strays):
    scene.film_clear()
    scene.film_merge(rd, film, strays)
    return scene.film_image()


def test_fixtures_exist():
    assert len(NAMES) == 20 and all(os.path.exists(os.path.join(DIRECT, n + ".pfm")) for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_the_reference_image_bit_for_bit(gpu, monkeypatch, name):
    scene = host_scene(gpu, name)
    ref = gpu.read_pfm(os.path.join(DIRECT, name + ".pfm"))
    stats = json.load(open(os.path.join(DIRECT, name + ".json")))
    rd, dl = scene.render_desc(), scene.direct_desc()
    assert rd.integrator == 0 and dl is not None
    for order, overlap in MODES:
        monkeypatch.setenv("PG_ANYHIT_ORDER", order)
        gs = gpu.GpuScene(scene.desc)
        try:
            gs.set_option(gpu.abi.PG_OPT_OVERLAP_SHADOW, overlap)
            film, strays = gs.render_direct(rd, dl)
            cn = gs.counters()
        finally:
            gs.close()
        img = image_of(scene, rd, film, strays)
        differing = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
        print(name, order, overlap, "differing pixels", differing, {k: (cn[k], stats[k]) for k in ("camera_rays", "closest_rays", "shadow_rays")})
        assert img.shape == ref.shape and differing == 0, (name, order, overlap, differing, float(np.abs(img - ref).max()))
        for k in ("camera_rays", "closest_rays", "shadow_rays"):
            assert cn[k] == stats[k], (name, order, overlap, k, cn[k], stats[k])
        if name == "h_specular_depth_1":  # no specular bounce was traced: every closest-hit query is a camera ray or a BSDF-sampled ray of EstimateDirect
            assert cn["closest_rays"] == stats["closest_rays"] == cn["camera_rays"] + cn["mis_rays"], (cn["closest_rays"], cn["camera_rays"], cn["mis_rays"])
        assert cn["paths_total"] == 0 and cn["path_length_count"] == 0 and cn["surface_interactions"] == 0  # directlighting.cpp has no statistics of its own


def test_three_tile_shards_merge_to_the_one_shard_film(gpu):
    """Scene (b): four samples per light; 2 x 2 tiles over 3 shards."""
    scene = host_scene(gpu, "b_four_samples")
    dl = scene.direct_desc()
    gs = gpu.GpuScene(scene.desc)
    try:
        full = scene.render_desc()
        film, strays = gs.render_direct(full, dl)
        one = image_of(scene, full, film, strays).copy()
        shards = [gs.render_direct(scene.render_desc(tile_first=r, tile_step=3), dl) for r in range(3)]
    finally:
        gs.close()
    scene.film_clear()
    scene.film_merge_shards(full, shards)
    merged = scene.film_image()
    assert np.array_equal(one.view(np.uint32), merged.view(np.uint32))
    assert np.array_equal(one.view(np.uint32), gpu.read_pfm(os.path.join(DIRECT, "b_four_samples.pfm")).view(np.uint32))


def test_integrators_take_turns_on_one_scene_handle(gpu):
    """A path frame, a directlighting frame and a path frame again on the SAME handle, each against the same frame on a fresh handle: the accumulators,
    the pending terms and the queues belong to a frame, not to the scene.  (cornell_32 and fixture (b) are one Cornell box: one geometry; the handle is
    created from (b)'s description, whose Halton table serves both.)"""
    p, b = host_scene(gpu, "cornell_32", GOLD), host_scene(gpu, "b_four_samples")
    assert p.desc.n_tris == b.desc.n_tris and b.desc.n_perm_dims >= p.desc.n_perm_dims
    frames = [(p, None), (b, b.direct_desc()), (p, None)]

    def render(gs, scene, dl):
        rd = scene.render_desc()
        return gs.render(rd) if dl is None else gs.render_direct(rd, dl)
    shared = gpu.GpuScene(b.desc)
    try:
        for scene, dl in frames:
            film, strays = render(shared, scene, dl)
            fresh = gpu.GpuScene(b.desc)
            try:
                film2, strays2 = render(fresh, scene, dl)
            finally:
                fresh.close()
            assert np.array_equal(film["rgb"].view(np.uint32), film2["rgb"].view(np.uint32)) and np.array_equal(film["weight"], film2["weight"])
            assert len(strays) == len(strays2)
            if dl is not None:  # (and the directlighting frame is the reference's image; the path frames run on (b)'s description, whose light distribution is not cornell_32's)
                ref = gpu.read_pfm(os.path.join(DIRECT, "b_four_samples.pfm"))
                assert np.array_equal(image_of(scene, scene.render_desc(), film, strays).view(np.uint32), ref.view(np.uint32))
    finally:
        shared.close()


def test_descriptions_outside_what_is_built_are_refused_and_render_nothing(gpu):
    a, l2 = host_scene(gpu, "a_defaults"), host_scene(gpu, "l2_one_stratified")
    cases = []
    rd = a.render_desc()
    rd.integrator = 1
    cases.append((a, rd, a.direct_desc(), "pg_render_direct: integrator 1 (the frame's description carries 0 here"))
    dl = gpu.abi.PgDirectLightingDesc.from_buffer_copy(l2.direct_desc())
    dl.strategy = 0
    cases.append((l2, l2.render_desc(), dl, "pg_render_direct: strategy 0 (all) under sampler 3: the PixelSamplers' sample arrays are not built"))
    for scene, rd, dl, text in cases:
        gs = gpu.GpuScene(scene.desc)
        try:
            gs.counters_reset()
            n = gs.tile_count(rd)
            film = np.full(n * rd.tile_pixels, 7.0, gpu.FILM_PIXEL_DTYPE)
            strays = np.zeros(64, gpu.STRAY_DTYPE)
            ns = C.c_int32(-5)
            st = gpu.gpu_lib().pg_render_direct(gs._h, C.byref(rd), C.byref(dl), film.ctypes.data, strays.ctypes.data, 64, C.byref(ns), gpu.abi.PG_MEM_HOST, None)
            assert st == -1 and text in gpu.gpu_lib().pg_last_error().decode(), gpu.gpu_lib().pg_last_error()
            assert (film["weight"] == 7.0).all() and ns.value == -5 and gs.counters()["camera_rays"] == 0
            with pytest.raises(gpu.PbrtGpuError):
                gs.render_direct(rd, dl)
        finally:
            gs.close()
