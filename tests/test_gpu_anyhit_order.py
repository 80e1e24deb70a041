"""Shadow rays (BVHAccel::IntersectP, accelerators/bvh.cpp:702-738) answer "is anything hit", and ray.tMax does not change while they are
traced: which nodes pass their box test -- and so which primitives can be met at all -- does not depend on the order of the visits.  The
product therefore visits the child the ray enters first (k_trace<2, .>), and only the reference-statistics tests ask for the reference's
order (PG_ANYHIT_ORDER=reference, tests/conftest.py).  Here: every golden scene and 40 random scenes rendered in BOTH orders -- films,
stray samples and ray counts must be bit-identical; the free order must not test more triangles in total.  And in the launch mode the benchmark
times: the free order with each bounce's any-hit launch on a second stream beside the next closest-hit launch (goldens: reference / free / free
overlapped; random scenes: both orders, serial and overlapped)."""
import os

import numpy as np
import pytest

from conftest import GOLD, golden_names
from test_gpu_fuzz import random_scene, random_scene_ext, random_scene_vol

pytestmark = pytest.mark.gpu
FAST = [n for n in golden_names() if not n.startswith(("sampler_", "filter_02sequence"))]  # (tile-serial samplers: minutes each; one below)


COUNTERS = ("camera_rays", "closest_rays", "shadow_rays", "mis_rays", "shade_items", "closest_node_visits", "closest_tri_tests", "light_tri_tests")
ALL_MODES = (("reference", 0), ("free", 0), ("reference", 1), ("free", 1))


def render_modes(gpu, monkeypatch, scene, modes=ALL_MODES):
    """The scene in every (shadow-ray order, overlap) mode of `modes`, the first being the reference order with one stream.  overlap 1: each bounce's any-hit
    launch on a second stream beside the next closest-hit launch (PG_OPT_OVERLAP_SHADOW, set after the scene exists, as bench.py sets it) -- the mode
    the benchmark's frames are timed in.  Film, sorted strays and the eight counters of every mode equal the first mode's; two renders in the same
    order also read the same nodes and triangles for their shadow rays, since overlap changes no traversal.  Returns the counters per mode."""
    assert modes[0] == ("reference", 0)
    out = {}
    for order, overlap in modes:
        monkeypatch.setenv("PG_ANYHIT_ORDER", order)
        gs = gpu.GpuScene(scene.desc)  # the order is read when the scene is created
        gs.set_option(gpu.abi.PG_OPT_OVERLAP_SHADOW, overlap)
        film, strays = gs.render(scene.render_desc())
        out[order, overlap] = (film, strays, gs.counters())
        gs.close()
    key = lambda s: np.lexsort((s["src_px"], s["src_py"], s["px"], s["py"]))  # (stray samples are appended in whatever order the blocks finish)
    fa, sa, ca = out[modes[0]]
    sa = sa[key(sa)]
    for mode in modes[1:]:
        fb, sb, cb = out[mode]
        assert np.array_equal(fa["rgb"], fb["rgb"]) and np.array_equal(fa["weight"], fb["weight"]), mode
        sb = sb[key(sb)]
        assert len(sa) == len(sb) and all(np.array_equal(sa[f], sb[f]) for f in ("px", "py", "src_px", "src_py", "weight", "rgb")), mode
        for k in COUNTERS:
            assert ca[k] == cb[k], (mode, k, ca[k], cb[k])
        if (mode[0], 0) in out and mode[1] == 1:
            serial = out[mode[0], 0][2]
            for k in ("shadow_tri_tests", "shadow_node_visits"):
                assert serial[k] == cb[k], (mode, k, serial[k], cb[k])
    return {mode: c for mode, (_, _, c) in out.items()}


@pytest.mark.parametrize("name", FAST + ["sampler_stratified"])
def test_golden_scene_same_film_in_both_orders(gpu, monkeypatch, name):
    cn = render_modes(gpu, monkeypatch, gpu.HostScene(os.path.join(GOLD, name + ".pbrt")), (("reference", 0), ("free", 0), ("free", 1)))
    for overlap in (0, 1):  # (a different order may test a few more before the first hit)
        assert cn["free", overlap]["shadow_tri_tests"] <= cn["reference", 0]["shadow_tri_tests"] * 1.5 + 64


@pytest.mark.parametrize("seed", range(40))
def test_random_scene_same_film_in_both_orders(gpu, monkeypatch, seed):
    text = (random_scene, random_scene_ext, random_scene_vol)[seed % 3](seed // 3)
    render_modes(gpu, monkeypatch, gpu.HostScene(text=text))
