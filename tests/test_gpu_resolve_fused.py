"""PathIntegrator frames add a vertex's direct lighting in the shading launch of the path's NEXT vertex (QueueState::pend: the value is known when the
vertex is shaded up to one bit, whether its shadow ray is occluded) and run k_resolve's arithmetic over a short list only -- the vertices with a MIS ray and
the paths that end with something to add or count (k_resolve_list).  PG_RESOLVE=pass, read when the scene is created, keeps the full-queue k_resolve launch
per bounce.  Every scene here is rendered both ways in one process: the films must be equal bit for bit and pg_counters field for field (total and
zero-radiance paths, path length, ray counts, ...).  The scenes are a few hundred pixels at a few samples, chosen for where the join can go wrong; the
comparisons against the reference are the golden suites', which run the default."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LIGHT = re.compile(r"AttributeBegin\n  AreaLightSource.*?AttributeEnd\n", re.S)


def cornell(xres=33, yres=17, spp=3, maxdepth=5, kd=None, specular=False, light="area", integrator=""):
    """scenes/cornell.pbrt at a size whose queues are no multiple of a block or a wave (33 x 17 x 3 = 1683 paths)."""
    t = open(os.path.join(ROOT, "scenes", "cornell.pbrt")).read()
    for old, new in (('"integer xresolution" [ 512 ]', f'"integer xresolution" [ {xres} ]'), ('"integer yresolution" [ 512 ]', f'"integer yresolution" [ {yres} ]'),
                     ('"integer pixelsamples" [ 256 ]', f'"integer pixelsamples" [ {spp} ]'), ('"integer maxdepth" [ 5 ]', f'"integer maxdepth" [ {maxdepth} ] {integrator}')):
        assert t.count(old) == 1, old
        t = t.replace(old, new)
    if kd is not None:
        t = re.sub(r'"rgb Kd" \[[^\]]*\]', f'"rgb Kd" [ {kd} {kd} {kd} ]', t)
    if specular:  # the short box a mirror, the tall box glass
        old = '# short box\nMaterial "matte" "rgb Kd" [ 0.73 0.73 0.73 ]\n'
        assert t.count(old) == 1 and t.count("# tall box\n") == 1
        t = t.replace(old, 'Material "mirror"\n').replace("# tall box\n", 'Material "glass" "float index" [ 1.5 ]\n')
    assert len(LIGHT.findall(t)) == 1
    if light == "point":
        t = LIGHT.sub('LightSource "point" "point from" [ 278 500 279 ] "rgb I" [ 400000 300000 100000 ]\n', t)
    elif light == "none":
        t = LIGHT.sub("", t)
    elif light == "many":  # the area light and a handful of point lights under it, for the spatial light distribution
        pts = "".join(f'LightSource "point" "point from" [ {x} {y} {z} ] "rgb I" [ 30000 40000 50000 ]\n' for x, y, z in
                      ((100, 500, 100), (450, 500, 100), (100, 500, 450), (450, 500, 450), (278, 300, 50), (278, 100, 279), (60, 250, 279), (500, 250, 279)))
        t = t.replace("# light\n", pts)
    else:
        assert light == "area"
    return t


def both_ways(gpu, monkeypatch, text, overlap=0, frames=1):
    """The scene by default and with PG_RESOLVE=pass (a scene reads it when it is created): equal films, equal stray samples, equal counters.  frames: renders
    per scene -- the sparse light tables defer vertices in a scene's first frame only."""
    scene = gpu.HostScene(text=text)
    rd = scene.render_desc()
    out = []
    for mode in (None, "pass"):
        if mode: monkeypatch.setenv("PG_RESOLVE", mode)
        else: monkeypatch.delenv("PG_RESOLVE", raising=False)
        gs = gpu.GpuScene(scene.desc)
        gs.set_option(gpu.abi.PG_OPT_OVERLAP_SHADOW, overlap)
        res = []
        for _ in range(frames):
            gs.counters_reset()
            film, strays = gs.render(rd)
            res.append((film, strays, gs.counters()))
        gs.close()
        out.append(res)
    key = lambda s: np.lexsort((s["src_px"], s["src_py"], s["px"], s["py"]))  # (stray samples are appended in whatever order the blocks finish)
    for frame, ((fa, sa, ca), (fb, sb, cb)) in enumerate(zip(*out)):
        assert fa.tobytes() == fb.tobytes(), frame
        sa, sb = sa[key(sa)], sb[key(sb)]
        assert len(sa) == len(sb) and sa.tobytes() == sb.tobytes(), frame
        assert ca["camera_rays"] > 0 and set(ca) == set(cb)
        differing = {k: (ca[k], cb[k]) for k in ca if ca[k] != cb[k] and not k.endswith("_ms")}  # (every field but the measured times)
        assert not differing, (frame, differing)
    return out[0][-1][2]


def test_matte_cornell_box(gpu, monkeypatch):
    """Occluded and unoccluded shadow rays, BSDF-sampled rays that hit the light's two triangles (the list), queue sizes that fill no block."""
    cn = both_ways(gpu, monkeypatch, cornell())
    assert cn["shadow_rays"] > 0 and cn["mis_rays"] > 0 and 0 < cn["paths_zero_radiance"] < cn["paths_total"]


def test_dark_walls_roulette_ends_paths_with_pending_light(gpu, monkeypatch):
    cn = both_ways(gpu, monkeypatch, cornell(kd=0.05, maxdepth=8))
    assert cn["path_length_min"] < cn["path_length_max"] <= 8


@pytest.mark.parametrize("maxdepth", [0, 1])
def test_no_resolve_launch_and_exactly_one(gpu, monkeypatch, maxdepth):
    both_ways(gpu, monkeypatch, cornell(maxdepth=maxdepth))


def test_specular_bounce_after_a_diffuse_one(gpu, monkeypatch):
    """A mirror and a glass box under the area light: the vertex behind a specular bounce adds its own Le, after the pending light of the bounce before."""
    both_ways(gpu, monkeypatch, cornell(specular=True))


@pytest.mark.parametrize("light", ["point", "none"])
def test_delta_light_only_and_no_light(gpu, monkeypatch, light):
    cn = both_ways(gpu, monkeypatch, cornell(light=light))
    assert cn["mis_rays"] == 0 and (cn["shadow_rays"] > 0) == (light == "point")


def test_several_batches_the_last_one_partial(gpu, monkeypatch):
    monkeypatch.setenv("PG_BATCH_PATHS", "256")
    both_ways(gpu, monkeypatch, cornell())


def test_vertices_deferred_by_the_sparse_light_tables(gpu, monkeypatch):
    """"lightsamplestrategy" "spatial" over nine lights with the tables filled on first touch (PG_SPARSE_LIGHTS=1 switches on what large light counts
    switch on): the first frame's launches defer vertices, the retry launch shades them again -- their pend is added and counted once.  The second
    frame finds every voxel."""
    monkeypatch.setenv("PG_SPARSE_LIGHTS", "1")
    both_ways(gpu, monkeypatch, cornell(light="many", integrator='"string lightsamplestrategy" "spatial"'), frames=2)


def test_any_hit_launch_on_its_own_stream(gpu, monkeypatch):
    """The mode the benchmark times: the shading launch reads the any-hit answers behind the event the full-queue resolve waited for."""
    both_ways(gpu, monkeypatch, cornell(), overlap=1)
