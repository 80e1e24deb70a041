"""The query families share one pair of staging arenas and the test-path work buffers of a scene (csrc/pg_abi.hip: Staging, queryScene, queueOver): no call may
see what another family's call, or a larger batch, left behind.

On ONE GpuScene a fixed sequence of host-memory calls runs, one family after the other, the batch size cycling through 65, 1, 600 and 64 (regions of 256
entries: 600 is two regions and part of a third; 65 and 64 sit on both sides of a wave), once in order and once reversed, so that every call follows a
different family's call of a different size, larger and smaller.  Every array a call returns must equal, byte for byte, what the same call with the same
inputs returns on a GpuScene created for it alone.  The inputs that come out of other calls (reference points, shadow rays, exit points) are made once per
batch size on a scene of their own, so both orders and the lone calls see the same bytes.  tests/test_emulated_query_scratch.py runs this file without a
GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = (65, 1, 600, 64)
N = max(SIZES)
ONE_MINUS_EPS = np.nextafter(F32(1), F32(0))


def same_bytes(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def as_tuple(r):
    return r if isinstance(r, tuple) else (r,)


def film_samples(rd_w, rd_h, n, seed, margin):
    """n CameraSamples over a w x h film and `margin` of its size around it; u_time spread over the shutter."""
    rng = np.random.default_rng(seed)
    film = ((rng.random((n, 2)) * (1 + 2 * margin) - margin) * [rd_w, rd_h]).astype(F32)
    lens = np.minimum(rng.random((n, 2)).astype(F32), ONE_MINUS_EPS)
    time = np.minimum(np.linspace(0, 1, n).astype(F32), ONE_MINUS_EPS)
    return np.ascontiguousarray(film), np.ascontiguousarray(lens), np.ascontiguousarray(time)


def interleaved_equals_alone(gpu, desc, calls, inputs):
    """The sequence in order, then reversed, on one scene; every call's arrays against the same call on a scene of its own."""
    steps = list(range(len(calls))) + list(reversed(range(len(calls))))
    gs = gpu.GpuScene(desc)
    got = [as_tuple(calls[c][1](gs, inputs[SIZES[j % len(SIZES)]])) for j, c in enumerate(steps)]
    gs.close()
    alone = {}
    for j, c in enumerate(steps):
        k = SIZES[j % len(SIZES)]
        if (c, k) not in alone:
            fresh = gpu.GpuScene(desc)
            alone[c, k] = as_tuple(calls[c][1](fresh, inputs[k]))
            fresh.close()
        assert same_bytes(got[j], alone[c, k]), (j, calls[c][0], k)
    assert len(alone) == len(steps)  # (every step is a pair of its own: each family ran at two sizes)


QUERY_CALLS = [
    ("intersect_at", lambda gs, x: gs.intersect_at(x.o, x.d, x.tmax, x.time)),
    ("scatter_sample_at", lambda gs, x: gs.scatter_sample_at(x.o, x.d, x.tmax, x.u2, x.time, with_interaction=True)),
    ("light_sample_at", lambda gs, x: gs.light_sample_at(x.ref, x.light, x.u2, with_shadow_rays=True)),
    ("transmittance_at", lambda gs, x: gs.transmittance_at(x.sh_o, x.sh_d, x.sh_tmax, x.sh_p1, x.sh_medium, x.u8, x.sh_time)),
    ("intersect_tr_at", lambda gs, x: gs.intersect_tr_at(x.o, x.d, x.tmax, x.medium, x.u8, x.time, with_interaction=True)),
    ("medium_sample_at", lambda gs, x: gs.medium_sample_at(x.o, x.d, x.t_hit, x.medium, x.u8[:, :2], x.time)),
    ("subsurface_sample_at", lambda gs, x: gs.subsurface_sample_at(x.o, x.d, x.tmax, x.u3, x.time, with_po=True)),
    ("subsurface_sample_f_at", lambda gs, x: gs.subsurface_sample_f_at(x.pi, x.eta, x.u2)),
    ("light_pdf_at", lambda gs, x: gs.light_pdf_at(x.ref, x.light, x.wi)),
    ("light_le_at", lambda gs, x: gs.light_le_at(x.o, x.d, x.tmax, x.time)),
]


def query_inputs(gs, cam, n_lights, k, seed):
    """The first k camera rays with their draws, and what the sequence's later calls take from its earlier ones."""
    rng = np.random.default_rng(seed)
    c = cam[:k]
    x = SimpleNamespace(o=np.ascontiguousarray(c["o"]), d=np.ascontiguousarray(c["d"]), tmax=np.ascontiguousarray(c["t_max"]), time=np.ascontiguousarray(c["time"]),
                        medium=np.ascontiguousarray(c["medium"]))
    draws = np.minimum(rng.random((N, 16)).astype(F32), ONE_MINUS_EPS)[:k]
    x.u2, x.u3, x.u8 = np.ascontiguousarray(draws[:, 0:2]), np.ascontiguousarray(draws[:, 2:5]), np.ascontiguousarray(draws[:, 5:13])
    x.wi = np.ascontiguousarray(draws[:, 13:16] - F32(0.5))
    x.light = rng.integers(0, n_lights, N).astype(np.int32)[:k]
    x.ref = gs.intersect_at(x.o, x.d, x.tmax, x.time)
    x.t_hit = np.where(x.ref["prim"] >= 0, x.ref["t"], x.tmax).astype(F32)
    x.samples, shadow = gs.light_sample_at(x.ref, x.light, x.u2, with_shadow_rays=True)
    tested = x.samples["visibility"] >= 0
    x.sh_o, x.sh_tmax, x.sh_d, x.sh_time = (np.ascontiguousarray(a) for a in (shadow[:, 0:3], shadow[:, 3], shadow[:, 4:7], shadow[:, 7]))
    x.sh_p1 = np.ascontiguousarray(x.samples["p_light"])
    x.sh_medium = np.where(tested, x.medium, -2).astype(np.int32)  # (an untested sample has no shadow ray: an invalid medium, no walk)
    x.sss, x.pi = gs.subsurface_sample_at(x.o, x.d, x.tmax, x.u3, x.time)
    x.eta = np.ascontiguousarray(x.sss["eta"])
    return x


# sss_nest_motion_volpath: moving nested instances (both halves of the hits' matrices), a homogeneous medium, a subsurface material, an area light -- and no surface
# without a material, so no walk there has a second segment; grid_sss_motion has one around its grid medium (whose walks read the staged draws) and gives all four
@pytest.mark.parametrize("name,null_surfaces", [("sss_nest_motion_volpath", False), ("grid_sss_motion", True)])
def test_every_family_after_every_other_equals_the_call_alone(gpu, name, null_surfaces):
    scene = gpu.HostScene(os.path.join(GOLD, name + ".pbrt"))
    rd = scene.render_desc()
    assert scene.desc.n_lights > 0 and scene.desc.n_media > 0 and scene.desc.n_bssrdfs > 0
    prep = gpu.GpuScene(scene.desc)
    cam = prep.camera_rays(rd, *film_samples(rd.full_res[0], rd.full_res[1], N, 7, margin=0.35))
    assert (cam["weight"] > 0).all() and len(np.unique(cam["time"])) > N // 2
    inputs = {k: query_inputs(prep, cam, scene.desc.n_lights, k, 11) for k in SIZES}
    # the largest batch exercises what the calls stage and walk: hits and misses, an exit point found, a walk of more than one segment, a tested shadow ray
    x = inputs[N]
    tr = prep.intersect_tr_at(x.o, x.d, x.tmax, x.medium, x.u8, x.time)
    shadow_tr = prep.transmittance_at(x.sh_o, x.sh_d, x.sh_tmax, x.sh_p1, x.sh_medium, x.u8, x.sh_time)
    prep.close()
    found = dict(hits=int((x.ref["prim"] >= 0).sum()), misses=int((x.ref["prim"] < 0).sum()), exits=int((x.sss["status"] == 2).sum()),
                 walks=int((tr["crossings"] >= 1).sum()), shadow_walks=int((shadow_tr["crossings"] >= 1).sum()), tested=int((x.samples["visibility"] >= 0).sum()))
    print(name, found)
    assert all(v > 0 for k, v in found.items() if null_surfaces or "walks" not in k), found
    interleaved_equals_alone(gpu, scene.desc, QUERY_CALLS, inputs)
    scene.close()


CAMERA_CALLS = [
    ("camera_rays", lambda gs, x: gs.camera_rays(x.rd, x.film, x.lens, x.u_time)),
    ("scatter_f_at(diff)", lambda gs, x: gs.scatter_f_at(x.o, x.d, x.tmax, x.wi, x.time, with_interaction=True, diff=x.diff)),
    ("intersect", lambda gs, x: gs.intersect(x.o, x.d, x.tmax)),
    ("intersect_p", lambda gs, x: gs.intersect_p(x.o, x.d, x.tmax)),
]


def test_camera_rays_and_staged_differentials_between_ray_queries(gpu):
    scene = gpu.HostScene(os.path.join(GOLD, "camera_queries", "realistic.pbrt"))
    rd = scene.render_desc()
    assert rd.camera_type == 3
    film, lens, u_time = film_samples(rd.full_res[0], rd.full_res[1], 3 * N, 23, margin=0.1)
    prep = gpu.GpuScene(scene.desc)
    cam = prep.camera_rays(rd, film, lens, u_time)
    live = cam[cam["weight"] > 0][:N]  # (a vignetted sample is a record of zeros: no ray)
    assert len(live) == N and (cam["weight"][:N] == 0).any()
    rng = np.random.default_rng(29)
    wi = (rng.random((N, 3)) - 0.5).astype(F32)
    d = np.ascontiguousarray(live["d"])
    d[3::7] = -d[3::7]  # (the camera sees nothing but the box: every seventh ray is turned away from it)
    inputs = {k: SimpleNamespace(rd=rd, film=film[:k], lens=lens[:k], u_time=u_time[:k], o=np.ascontiguousarray(live["o"][:k]), d=d[:k],
                                 tmax=np.ascontiguousarray(live["t_max"][:k]), time=np.ascontiguousarray(live["time"][:k]), wi=np.ascontiguousarray(wi[:k]),
                                 diff=np.ascontiguousarray(live["differentials"][:k])) for k in SIZES}
    x = inputs[N]
    with_diff, isect = prep.scatter_f_at(x.o, x.d, x.tmax, x.wi, x.time, with_interaction=True, diff=x.diff)
    without = prep.scatter_f_at(x.o, x.d, x.tmax, x.wi, x.time)
    prep.close()
    # hits and misses, and the staged differentials are read: they change f at textured hits
    found = dict(hits=int((isect["prim"] >= 0).sum()), misses=int((isect["prim"] < 0).sum()), filtered=int((with_diff["f"] != without["f"]).any(1).sum()))
    print(found)
    assert all(v > 0 for v in found.values()), found
    interleaved_equals_alone(gpu, scene.desc, CAMERA_CALLS, inputs)
    scene.close()
