"""pbrt-v3 path-tracing hot path, MI355X-native: Python plumbing.

The product is two native libraries built in-tree by ``make -C pbrt-v3_amd``:

* ``libpbrt_host.so`` -- C++ mirror of pbrt-v3's scene-file front end and API
  state machine (parser, graphics state, BVHAccel build, Film); flattens a
  ``.pbrt`` file into ``PgSceneDesc`` / ``PgRenderDesc``.
* ``libpbrt_gpu.so``  -- hand-written HIP kernels for gfx950 behind the C ABI
  of ``include/pbrt_gpu.h`` (wavefront PathIntegrator, BVH traversal).

This module only binds them with ctypes so tests, ``bench.py`` and
``torch.distributed`` sharding can drive the same entry points the
``pbrt_amd`` CLI uses.  There is no Python or CPU fallback for the device
path: if ``libpbrt_gpu.so`` is missing or no GPU is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .abi import (PgCounters, PgDirectLightingDesc, PgFilmPixel, PgRenderDesc, PgSceneDesc, PgStraySample, PG_MEM_DEVICE, PG_MEM_HOST,
                  PG_OK)

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libpbrt_host.so")
GPU_LIB_PATH = os.environ.get("PBRT_GPU_LIB") or os.path.join(_HERE, "libpbrt_gpu.so")  # override: kernel A/B builds only

FILM_PIXEL_DTYPE = np.dtype([("rgb", np.float32, 3), ("weight", np.float32)])
STRAY_DTYPE = np.dtype([("px", np.int32), ("py", np.int32), ("src_px", np.int32), ("src_py", np.int32),
                        ("rgb", np.float32, 3), ("weight", np.float32)])

# one record of pg_intersect_at: abi.PgInteraction field for field (128 bytes)
INTERACTION_DTYPE = np.dtype([("prim", np.int32), ("instance", np.int32), ("instance_inner", np.int32), ("material", np.int32), ("light", np.int32),
                              ("t", np.float32), ("time", np.float32), ("uv", np.float32, 2),
                              ("p", np.float32, 3), ("p_error", np.float32, 3), ("n", np.float32, 3), ("wo", np.float32, 3),
                              ("shading_n", np.float32, 3), ("shading_dpdu", np.float32, 3), ("shading_dpdv", np.float32, 3), ("reserved", np.float32, 2)])

# one record of pg_scatter_f_at / pg_scatter_sample_at: abi.PgScatter field for field (64 bytes)
SCATTER_DTYPE = np.dtype([("prim", np.int32), ("n_bxdfs", np.int32), ("n_matching", np.int32), ("sampled_type", np.int32),
                          ("f", np.float32, 3), ("pdf", np.float32), ("wi", np.float32, 3), ("eta", np.float32),
                          ("shading_n", np.float32, 3), ("types", np.uint32)])

# one record of pg_light_sample_at: abi.PgLightSample field for field (64 bytes)
LIGHT_SAMPLE_DTYPE = np.dtype([("light", np.int32), ("visibility", np.int32), ("pdf", np.float32), ("Li", np.float32, 3), ("wi", np.float32, 3),
                               ("p_light", np.float32, 3), ("n_light", np.float32, 3), ("reserved", np.float32)])

# one record of pg_transmittance_at / pg_intersect_tr_at: abi.PgTransmittance field for field (32 bytes)
TRANSMITTANCE_DTYPE = np.dtype([("Tr", np.float32, 3), ("status", np.int32), ("medium", np.int32), ("crossings", np.int32), ("draws_used", np.int32),
                                ("reserved", np.int32)])

# one record of pg_medium_sample_at: abi.PgMediumSample field for field (64 bytes)
MEDIUM_SAMPLE_DTYPE = np.dtype([("sampled", np.int32), ("draws_used", np.int32), ("beta", np.float32, 3), ("t", np.float32), ("p", np.float32, 3),
                                ("wo", np.float32, 3), ("g", np.float32), ("medium", np.int32), ("reserved", np.float32, 2)])

# one record of pg_subsurface_sample_at: abi.PgSubsurfaceSample field for field (64 bytes)
SUBSURFACE_SAMPLE_DTYPE = np.dtype([("status", np.int32), ("prim", np.int32), ("bssrdf", np.int32), ("n_found", np.int32), ("S", np.float32, 3),
                                    ("pdf", np.float32), ("eta", np.float32), ("medium_inside", np.int32), ("medium_outside", np.int32),
                                    ("chain_rays", np.int32), ("reserved", np.float32, 4)])

# one record of pg_camera_rays_at: abi.PgCameraRay field for field (96 bytes); `differentials` is what scatter_f_at / scatter_sample_at take as diff
CAMERA_RAY_DTYPE = np.dtype([("o", np.float32, 3), ("t_max", np.float32), ("d", np.float32, 3), ("time", np.float32), ("weight", np.float32), ("medium", np.int32),
                             ("has_differentials", np.int32), ("reserved", np.float32), ("differentials", np.float32, 12)])

# one record of pg_camera_we_at: abi.PgCameraImportance field for field (32 bytes)
CAMERA_IMPORTANCE_DTYPE = np.dtype([("status", np.int32), ("We", np.float32), ("pdf_pos", np.float32), ("pdf_dir", np.float32), ("p_raster", np.float32, 2),
                                    ("cos_theta", np.float32), ("reserved", np.float32)])

# one record of pg_camera_sample_wi_at: abi.PgCameraSample field for field (64 bytes; visibility where LIGHT_SAMPLE_DTYPE has it)
CAMERA_SAMPLE_DTYPE = np.dtype([("status", np.int32), ("visibility", np.int32), ("pdf", np.float32), ("We", np.float32), ("wi", np.float32, 3),
                                ("p_lens", np.float32, 3), ("n_lens", np.float32, 3), ("p_raster", np.float32, 2), ("reserved", np.float32)])

_host = None
_gpu = None


class PbrtGpuError(RuntimeError):
    pass


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise PbrtGpuError(f"{HOST_LIB_PATH} not built; run __graft_entry__.build() or make -C pbrt-v3_amd")
        _host = abi.bind(C.CDLL(HOST_LIB_PATH), abi.HOST_SYMBOLS)
    return _host


def gpu_lib():
    """The HIP back end.  Fails loudly when the extension is missing."""
    global _gpu
    if _gpu is None:
        if not os.path.exists(GPU_LIB_PATH):
            raise PbrtGpuError(f"{GPU_LIB_PATH} not built; run __graft_entry__.build() (there is no CPU fallback)")
        _gpu = abi.bind(C.CDLL(GPU_LIB_PATH), abi.GPU_SYMBOLS)
    return _gpu


def _path_family_only(rd, what):
    """pg_render and pg_render_sharded trace paths whatever scene a description came from, and a directlighting scene's PgRenderDesc cannot
    be told from a path frame's (integrator = 0): the binding remembers where the description came from and refuses instead."""
    if getattr(rd, "direct_lighting", False):
        raise PbrtGpuError(f"{what}: the description belongs to an Integrator \"directlighting\" scene; render it with render_direct / "
                           "render_device_direct and HostScene.direct_desc() (render_scene dispatches); no path-traced frame is given in its place")


def _check(status, what):
    if status != PG_OK:
        msg = gpu_lib().pg_last_error()
        raise PbrtGpuError(f"{what} failed ({status}): {msg.decode() if msg else ''}")


class HostScene:
    """A parsed .pbrt scene: pbrtInit/pbrtParseFile/pbrtCleanup up to (not including) Render."""

    def __init__(self, filename=None, text=None, quick=False, crop=None):
        lib = host_lib()
        cropv = (C.c_float * 4)(*crop) if crop is not None else None
        if filename is not None:
            self._h = lib.pbrt_host_load_file(os.fsencode(filename), int(quick), cropv)
        else:
            self._h = lib.pbrt_host_load_string(text.encode(), int(quick), cropv)
        if not self._h:
            raise PbrtGpuError(f"scene {filename or '<string>'} produced no renderable scene")
        self.desc = lib.pbrt_host_scene_desc(self._h).contents

    def close(self):
        if getattr(self, "_h", None):
            host_lib().pbrt_host_free(self._h)
            self._h = None

    __del__ = close

    def render_desc(self, tile_first=0, tile_step=1):
        rd = PgRenderDesc()
        host_lib().pbrt_host_render_desc(self._h, C.byref(rd))
        rd.tile_first, rd.tile_step = tile_first, tile_step
        rd.direct_lighting = bool(host_lib().pbrt_host_direct_desc(self._h))
        return rd

    def direct_desc(self):
        """Integrator "directlighting": the PgDirectLightingDesc that goes with render_desc() (its light_samples array belongs to this
        scene: keep the scene alive while the description is in use); None for the path integrators."""
        p = host_lib().pbrt_host_direct_desc(self._h)
        return p.contents if p else None

    def camera_we_desc(self):
        """The PgCameraWeDesc that goes with render_desc() into GpuScene.camera_we_at / camera_sample_wi_at: the stored inverses of RasterToCamera and of the
        two ends of CameraToWorld, and the image-plane area; None for a camera that is not the perspective one (the reference implements We for no other)."""
        we = abi.PgCameraWeDesc()
        return we if host_lib().pbrt_host_camera_we_desc(self._h, C.byref(we)) else None

    @property
    def film_size(self):
        w, h = C.c_int(), C.c_int()
        host_lib().pbrt_host_film_size(self._h, C.byref(w), C.byref(h))
        return w.value, h.value

    def film_clear(self):
        host_lib().pbrt_host_film_clear(self._h)

    def film_merge(self, rd, film, strays):
        """Film::MergeFilmTile for one shard (numpy arrays of FILM_PIXEL_DTYPE / STRAY_DTYPE)."""
        film = np.ascontiguousarray(film)
        strays = np.ascontiguousarray(strays)
        host_lib().pbrt_host_film_merge(self._h, C.byref(rd), film.ctypes.data, strays.ctypes.data, len(strays))

    def film_merge_shards(self, full_rd, shards):
        """The n shards [(film, strays), ...] of ONE frame (shard r = the tiles t = r (mod n)), merged in the frame's own tile order:
        Film::MergeShards.  `full_rd` describes the whole frame (tile_first 0, tile_step 1)."""
        n = len(shards)
        films = [np.ascontiguousarray(f) for f, _ in shards]
        strays = [np.ascontiguousarray(s) for _, s in shards]
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in films])
        sp = (C.c_void_p * n)(*[s.ctypes.data for s in strays])
        ns = (C.c_int * n)(*[len(s) for s in strays])
        host_lib().pbrt_host_film_merge_shards(self._h, C.byref(full_rd), n, fp, sp, ns)

    def film_image(self):
        """Final RGB image as Film::WriteImage computes it: (h, w, 3) float32, top row first."""
        w, h = self.film_size
        img = np.empty((h, w, 3), np.float32)
        host_lib().pbrt_host_film_image(self._h, img.ctypes.data)
        return img

    # numpy views of the flattened scene (for tests / diagnostics)
    def nodes(self):
        return np.ctypeslib.as_array(C.cast(self.desc.nodes, C.POINTER(C.c_uint8)), (self.desc.n_nodes * 32,)).view(
            np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("offset", np.int32), ("nprims", np.uint16),
                      ("axis", np.uint8), ("pad", np.uint8)]))

    def indices(self):
        return np.ctypeslib.as_array(self.desc.indices, (self.desc.n_tris, 3))

    def positions(self):
        return np.ctypeslib.as_array(self.desc.P, (self.desc.n_verts, 3))


NODE_DTYPE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("offset", np.int32), ("nprims", np.uint16),
                       ("axis", np.uint8), ("pad", np.uint8)])


def hlbvh_build(bounds, max_prims_in_node=4, device=True):
    """BVHAccel::HLBVHBuild + flattenBVHTree over bare primitive bounds (n x 6 float32: pMin, pMax): on the device through
    pg_hlbvh_build, or with the host front end's builder (device=False).  Returns (nodes, ordered primitive indices)."""
    bounds = np.ascontiguousarray(bounds, np.float32).reshape(-1, 6)
    n = len(bounds)
    nodes = np.zeros(max(1, 2 * n), NODE_DTYPE)
    order = np.zeros(max(1, n), np.int32)
    if device:
        nn = C.c_int32(0)
        _check(gpu_lib().pg_hlbvh_build(n, bounds.ctypes.data, max_prims_in_node, nodes.ctypes.data, C.byref(nn), order.ctypes.data), "pg_hlbvh_build")
    else:
        nn = C.c_int(0)
        host_lib().pbrt_host_hlbvh_build(n, bounds.ctypes.data, max_prims_in_node, nodes.ctypes.data, C.byref(nn), order.ctypes.data)
    return nodes[:nn.value], order[:n]


def set_device_bvh(on):
    """Scenes loaded afterwards build their "hlbvh" accelerators on the device (pbrt_amd --devicebvh)."""
    host_lib().pbrt_host_set_device_bvh(1 if on else 0)


def write_pfm(filename, img):
    img = np.ascontiguousarray(img, np.float32)
    h, w, _ = img.shape
    if host_lib().pbrt_host_write_pfm(os.fsencode(filename), img.ctypes.data, w, h) != 0:
        raise PbrtGpuError(f"cannot write {filename}")


def read_pfm(filename):
    """PFM reader (core/imageio.cpp ReadImagePFM semantics): returns (h, w, 3) float32, top row first."""
    with open(filename, "rb") as f:
        if f.readline().strip() != b"PF":
            raise ValueError("not a colour PFM")
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(w * h * 12), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return np.ascontiguousarray(data[::-1]).astype(np.float32)


def default_max_strays(rd, n_tiles):
    """Room for the box filter's stray samples (a sample whose offset inside its pixel is exactly 0 also lands in the previous
    pixel, film.h:127-132): rare, except under the MaxMinDistSampler, whose first sample of every pixel is (0, 0) by construction
    and lands in up to three neighbours."""
    per_tile = 256 * 4 if rd.sampler == abi.PG_SAMPLER_MAXMINDIST else 256 // 8
    return n_tiles * per_tile + 1024


class GpuScene:
    """Device-resident scene (pg_scene_create) and the render / intersect entry points."""

    def __init__(self, desc, device=0):
        lib = gpu_lib()
        _check(lib.pg_set_device(device), "pg_set_device")
        self.device = device
        h = C.c_void_p()
        _check(lib.pg_scene_create(C.byref(desc), C.byref(h)), "pg_scene_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            gpu_lib().pg_scene_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def tile_count(rd):
        return gpu_lib().pg_render_tile_count(C.byref(rd))

    def render(self, rd, max_strays=None, stream=None):
        """Integrator::Render for the shard in rd into host numpy buffers (film, strays)."""
        _path_family_only(rd, "GpuScene.render")
        n = self.tile_count(rd)
        if max_strays is None:
            max_strays = default_max_strays(rd, n)
        film = np.zeros(n * rd.tile_pixels, FILM_PIXEL_DTYPE)
        strays = np.zeros(max_strays, STRAY_DTYPE)
        ns = C.c_int32(0)
        _check(gpu_lib().pg_render(self._h, C.byref(rd), film.ctypes.data, strays.ctypes.data, max_strays, C.byref(ns),
                                   PG_MEM_HOST, stream), "pg_render")
        return film, strays[:ns.value]

    def render_device(self, rd, film_ptr, strays_ptr, max_strays, nstrays_ptr, stream=None):
        """Same, into caller-owned device buffers (raw pointers; e.g. torch tensors' data_ptr())."""
        _path_family_only(rd, "GpuScene.render_device")
        _check(gpu_lib().pg_render(self._h, C.byref(rd), film_ptr, strays_ptr, max_strays, nstrays_ptr, PG_MEM_DEVICE,
                                   stream), "pg_render")

    def render_direct(self, rd, dl, max_strays=None, stream=None):
        """Integrator::Render under the DirectLightingIntegrator (pg_render_direct): rd as for render(), dl from HostScene.direct_desc()."""
        n = self.tile_count(rd)
        if max_strays is None:
            max_strays = default_max_strays(rd, n)
        film = np.zeros(n * rd.tile_pixels, FILM_PIXEL_DTYPE)
        strays = np.zeros(max_strays, STRAY_DTYPE)
        ns = C.c_int32(0)
        _check(gpu_lib().pg_render_direct(self._h, C.byref(rd), C.byref(dl), film.ctypes.data, strays.ctypes.data, max_strays, C.byref(ns),
                                          PG_MEM_HOST, stream), "pg_render_direct")
        return film, strays[:ns.value]

    def render_device_direct(self, rd, dl, film_ptr, strays_ptr, max_strays, nstrays_ptr, stream=None):
        """Same, into caller-owned device buffers (raw pointers), as render_device()."""
        _check(gpu_lib().pg_render_direct(self._h, C.byref(rd), C.byref(dl), film_ptr, strays_ptr, max_strays, nstrays_ptr, PG_MEM_DEVICE,
                                          stream), "pg_render_direct")

    def intersect(self, o, d, tmax):
        """Batched Scene::Intersect on host arrays: returns prim (int32), t, bary (n,3)."""
        o, d, tmax, _, n = self._rays(o, d, tmax, None)
        prim = np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        bary = np.empty((n, 3), np.float32)
        _check(gpu_lib().pg_intersect(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, prim.ctypes.data,
                                      t.ctypes.data, bary.ctypes.data, PG_MEM_HOST, None), "pg_intersect")
        return prim, t, bary

    def intersect_p(self, o, d, tmax):
        o, d, tmax, _, n = self._rays(o, d, tmax, None)
        occ = np.empty(n, np.uint8)
        _check(gpu_lib().pg_intersect_p(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, occ.ctypes.data,
                                        PG_MEM_HOST, None), "pg_intersect_p")
        return occ

    @staticmethod
    def _rays(o, d, tmax, time):
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        n = len(tmax)
        if time is not None:
            time = np.ascontiguousarray(time, np.float32)
            if o.size != 3 * n or d.size != 3 * n or time.size != n:
                raise ValueError("o and d hold three floats, tmax and time one float per ray")
        elif o.size != 3 * n or d.size != 3 * n:
            raise ValueError("o and d hold three floats, tmax one float per ray")
        return o, d, tmax, time, n

    def intersect_at(self, o, d, tmax, time=None):
        """Batched Scene::Intersect with Ray::time on host arrays (time=None: every ray at time 0): the rays' SurfaceInteractions as a
        structured array of INTERACTION_DTYPE -- moving shapes and instances at the ray's time; prim = -1 on a miss."""
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        out = np.empty(n, INTERACTION_DTYPE)
        _check(gpu_lib().pg_intersect_at(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                         out.ctypes.data, PG_MEM_HOST, None), "pg_intersect_at")
        return out

    def intersect_p_at(self, o, d, tmax, time=None):
        """Batched Scene::IntersectP with Ray::time on host arrays: uint8, 1 = occluded."""
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        occ = np.empty(n, np.uint8)
        _check(gpu_lib().pg_intersect_p_at(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                           occ.ctypes.data, PG_MEM_HOST, None), "pg_intersect_p_at")
        return occ

    def intersect_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, out_ptr, stream=None):
        """pg_intersect_at on caller-owned device buffers (raw pointers; e.g. torch tensors' data_ptr()): n rays, 3 n floats at o_ptr and d_ptr, n at
        tmax_ptr and time_ptr (None: time 0), n records of INTERACTION_DTYPE written at out_ptr.  Nothing visits the host."""
        _check(gpu_lib().pg_intersect_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, out_ptr, PG_MEM_DEVICE, stream), "pg_intersect_at")

    def intersect_p_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, occluded_ptr, stream=None):
        """pg_intersect_p_at on caller-owned device buffers: n bytes written at occluded_ptr."""
        _check(gpu_lib().pg_intersect_p_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, occluded_ptr, PG_MEM_DEVICE, stream), "pg_intersect_p_at")

    def _scatter(self, name, o, d, tmax, extra, per, time, flags, with_interaction, diff=None, mode=None):
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        extra = np.ascontiguousarray(extra, np.float32)
        if extra.size != per * n:
            raise ValueError(("wi holds three floats" if per == 3 else "u holds two floats") + " per ray")
        out = np.empty(n, SCATTER_DTYPE)
        isect = np.empty(n, INTERACTION_DTYPE) if with_interaction else None
        args = [extra.ctypes.data]
        if diff is not None:  # the _diff_ entry points: the differentials follow wi / u
            diff = np.ascontiguousarray(diff, np.float32)
            if diff.size != 12 * n:
                raise ValueError("diff holds twelve floats per ray (PgCameraRay.differentials)")
            name = name.replace("_at", "_diff_at")
            args.append(diff.ctypes.data)
        tail = [int(flags)]
        if mode is not None:  # the _mode_ entry points: diff (may be NULL) behind wi / u, the TransportMode behind flags
            name = name.replace("_diff_at", "_at").replace("_at", "_mode_at")
            if diff is None:
                args.append(None)
            tail.append(int(mode))
        _check(getattr(gpu_lib(), name)(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                        *args, *tail, None if isect is None else isect.ctypes.data, out.ctypes.data, PG_MEM_HOST, None), name)
        return (out, isect) if with_interaction else out

    def scatter_f_at(self, o, d, tmax, wi, time=None, flags=31, with_interaction=False, diff=None, mode=None):
        """Batched BSDF::f and BSDF::Pdf at the rays' closest hits (pg_scatter_f_at) on host arrays: the rays as intersect_at takes them, wi three floats per
        ray (world space, used as given), flags one BxDFType mask (0 .. 31) for all rays.  Returns the records as a structured array of SCATTER_DTYPE, or
        -- with_interaction -- (records, what intersect_at returns for the same rays) from the one trace.  diff: the rays' differentials, twelve floats
        per ray as camera_rays reports them (pg_scatter_f_diff_at: textures are filtered over the footprint ComputeDifferentials finds; twelve zeros =
        a ray without); None: rays without differentials, the plain call.  mode: None = the calls above; abi.PG_MODE_RADIANCE (0) or
        abi.PG_MODE_IMPORTANCE (1) = pg_scatter_f_mode_at, the BSDF under that TransportMode (1: at a vertex of a light subpath)."""
        return self._scatter("pg_scatter_f_at", o, d, tmax, wi, 3, time, flags, with_interaction, diff, mode)

    def scatter_sample_at(self, o, d, tmax, u, time=None, flags=31, with_interaction=False, diff=None, mode=None):
        """Batched BSDF::Sample_f at the rays' closest hits (pg_scatter_sample_at, or -- diff -- pg_scatter_sample_diff_at): as scatter_f_at, with u two
        floats per ray (Sample_f's Point2f)."""
        return self._scatter("pg_scatter_sample_at", o, d, tmax, u, 2, time, flags, with_interaction, diff, mode)

    def scatter_f_mode_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, wi_ptr, diff_ptr, flags, mode, isect_ptr, out_ptr, stream=None):
        """pg_scatter_f_mode_at on caller-owned device buffers: as scatter_f_diff_at_device, with the TransportMode (0 Radiance, 1 Importance) behind flags."""
        _check(gpu_lib().pg_scatter_f_mode_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, wi_ptr, diff_ptr, int(flags), int(mode), isect_ptr, out_ptr, PG_MEM_DEVICE,
                                              stream), "pg_scatter_f_mode_at")

    def scatter_sample_mode_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, diff_ptr, flags, mode, isect_ptr, out_ptr, stream=None):
        """pg_scatter_sample_mode_at on caller-owned device buffers: as scatter_sample_diff_at_device, with the TransportMode behind flags."""
        _check(gpu_lib().pg_scatter_sample_mode_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, diff_ptr, int(flags), int(mode), isect_ptr, out_ptr, PG_MEM_DEVICE,
                                                   stream), "pg_scatter_sample_mode_at")

    def camera_we_at(self, rd, we, o, d, time=None):
        """Batched Camera::We and Camera::Pdf_We (pg_camera_we_at) on host arrays, for the perspective camera rd and we describe (HostScene.render_desc() and
        camera_we_desc()): o and d three floats per ray (d used as given), time one (None: 0).  Returns a structured array of CAMERA_IMPORTANCE_DTYPE; traces
        nothing and moves no counter.  Any other camera is refused (PG_ERR_UNSUPPORTED)."""
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        n = o.size // 3
        if o.size != 3 * n or d.size != 3 * n:
            raise ValueError("o and d hold three floats per ray")
        if time is not None:
            time = np.ascontiguousarray(time, np.float32)
            if time.size != n:
                raise ValueError("time holds one float per ray")
        out = np.empty(n, CAMERA_IMPORTANCE_DTYPE)
        _check(gpu_lib().pg_camera_we_at(self._h, C.byref(rd), C.byref(we), n, o.ctypes.data, d.ctypes.data, None if time is None else time.ctypes.data,
                                         out.ctypes.data, PG_MEM_HOST, None), "pg_camera_we_at")
        return out

    def camera_sample_wi_at(self, rd, we, ref, u, with_shadow_rays=False):
        """Batched Camera::Sample_Wi + VisibilityTester::Unoccluded (pg_camera_sample_wi_at) on host arrays: ref as light_sample_at takes it, u two floats per
        reference point (the lens sample).  Returns a structured array of CAMERA_SAMPLE_DTYPE or -- with_shadow_rays -- (records, (n, 8) float32: origin,
        tMax, direction, time of the tested samples' shadow rays, zeros elsewhere)."""
        ref = np.ascontiguousarray(ref, INTERACTION_DTYPE)
        u = np.ascontiguousarray(u, np.float32)
        n = ref.size
        if u.size != 2 * n:
            raise ValueError("u holds two floats per reference point")
        out = np.empty(n, CAMERA_SAMPLE_DTYPE)
        shadow = np.empty((n, 8), np.float32) if with_shadow_rays else None
        _check(gpu_lib().pg_camera_sample_wi_at(self._h, C.byref(rd), C.byref(we), n, ref.ctypes.data, u.ctypes.data, out.ctypes.data,
                                                None if shadow is None else shadow.ctypes.data, PG_MEM_HOST, None), "pg_camera_sample_wi_at")
        return (out, shadow) if with_shadow_rays else out

    def camera_we_at_device(self, rd, we, n, o_ptr, d_ptr, time_ptr, out_ptr, stream=None):
        """pg_camera_we_at on caller-owned device buffers (raw pointers): 3 n floats at o_ptr and d_ptr, n at time_ptr (None: 0); n records of
        CAMERA_IMPORTANCE_DTYPE written at out_ptr (16-byte aligned).  Nothing visits the host."""
        _check(gpu_lib().pg_camera_we_at(self._h, C.byref(rd), C.byref(we), n, o_ptr, d_ptr, time_ptr, out_ptr, PG_MEM_DEVICE, stream), "pg_camera_we_at")

    def camera_sample_wi_at_device(self, rd, we, n, ref_ptr, u_ptr, out_ptr, shadow_ptr=None, stream=None):
        """pg_camera_sample_wi_at on caller-owned device buffers: n records of INTERACTION_DTYPE at ref_ptr, 2 n floats at u_ptr; n records of
        CAMERA_SAMPLE_DTYPE written at out_ptr (16-byte aligned) and, unless shadow_ptr is None, 8 n floats at shadow_ptr."""
        _check(gpu_lib().pg_camera_sample_wi_at(self._h, C.byref(rd), C.byref(we), n, ref_ptr, u_ptr, out_ptr, shadow_ptr, PG_MEM_DEVICE, stream),
               "pg_camera_sample_wi_at")

    def scatter_f_diff_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, wi_ptr, diff_ptr, flags, isect_ptr, out_ptr, stream=None):
        """pg_scatter_f_diff_at on caller-owned device buffers: as scatter_f_at_device, with 12 n floats at diff_ptr (16-byte aligned; None: no differentials)."""
        _check(gpu_lib().pg_scatter_f_diff_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, wi_ptr, diff_ptr, int(flags), isect_ptr, out_ptr, PG_MEM_DEVICE, stream),
               "pg_scatter_f_diff_at")

    def scatter_sample_diff_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, diff_ptr, flags, isect_ptr, out_ptr, stream=None):
        """pg_scatter_sample_diff_at on caller-owned device buffers: as scatter_sample_at_device, with 12 n floats at diff_ptr."""
        _check(gpu_lib().pg_scatter_sample_diff_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, diff_ptr, int(flags), isect_ptr, out_ptr, PG_MEM_DEVICE, stream),
               "pg_scatter_sample_diff_at")

    def camera_rays(self, rd, p_film, p_lens=None, u_time=None):
        """Batched Camera::GenerateRayDifferential (pg_camera_rays_at) on host arrays, for the camera rd describes: p_film two floats per sample
        (CameraSample::pFilm), p_lens two (pLens; None: 0), u_time one (CameraSample::time before the shutter's Lerp; None: 0).  Returns a structured array
        of CAMERA_RAY_DTYPE: the world-space ray, its time and medium, the sample's weight (0: vignetted, a record of zeros) and the differentials Li
        receives, scaled by 1 / sqrt(rd.spp)."""
        p_film = np.ascontiguousarray(p_film, np.float32)
        n = p_film.size // 2
        if p_film.size != 2 * n:
            raise ValueError("p_film holds two floats per sample")
        if p_lens is not None:
            p_lens = np.ascontiguousarray(p_lens, np.float32)
            if p_lens.size != 2 * n:
                raise ValueError("p_lens holds two floats per sample")
        if u_time is not None:
            u_time = np.ascontiguousarray(u_time, np.float32)
            if u_time.size != n:
                raise ValueError("u_time holds one float per sample")
        out = np.empty(n, CAMERA_RAY_DTYPE)
        _check(gpu_lib().pg_camera_rays_at(self._h, C.byref(rd), n, p_film.ctypes.data, None if p_lens is None else p_lens.ctypes.data,
                                           None if u_time is None else u_time.ctypes.data, out.ctypes.data, PG_MEM_HOST, None), "pg_camera_rays_at")
        return out

    def camera_rays_device(self, rd, n, p_film_ptr, p_lens_ptr, u_time_ptr, out_ptr, stream=None):
        """pg_camera_rays_at on caller-owned device buffers (raw pointers): 2 n floats at p_film_ptr and p_lens_ptr (None: 0), n at u_time_ptr (None: 0); n
        records of CAMERA_RAY_DTYPE written at out_ptr (16-byte aligned).  Nothing visits the host."""
        _check(gpu_lib().pg_camera_rays_at(self._h, C.byref(rd), n, p_film_ptr, p_lens_ptr, u_time_ptr, out_ptr, PG_MEM_DEVICE, stream), "pg_camera_rays_at")

    def scatter_f_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, wi_ptr, flags, isect_ptr, out_ptr, stream=None):
        """pg_scatter_f_at on caller-owned device buffers (raw pointers, as intersect_at_device takes them): 3 n floats at wi_ptr, n records of
        SCATTER_DTYPE written at out_ptr and, unless isect_ptr is None, n of INTERACTION_DTYPE at isect_ptr.  Nothing visits the host."""
        _check(gpu_lib().pg_scatter_f_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, wi_ptr, int(flags), isect_ptr, out_ptr, PG_MEM_DEVICE, stream), "pg_scatter_f_at")

    def scatter_sample_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, flags, isect_ptr, out_ptr, stream=None):
        """pg_scatter_sample_at on caller-owned device buffers: 2 n floats at u_ptr, the outputs as scatter_f_at_device's."""
        _check(gpu_lib().pg_scatter_sample_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, int(flags), isect_ptr, out_ptr, PG_MEM_DEVICE, stream),
               "pg_scatter_sample_at")

    @staticmethod
    def _light_inputs(ref, light, extra, per):
        ref = np.ascontiguousarray(ref, INTERACTION_DTYPE)
        light = np.ascontiguousarray(light, np.int32)
        extra = np.ascontiguousarray(extra, np.float32)
        n = ref.size
        if light.size != n or extra.size != per * n:
            raise ValueError("light holds one index and " + ("wi three floats" if per == 3 else "u two floats") + " per reference point")
        return ref, light, extra, n

    def light_sample_at(self, ref, light, u, with_shadow_rays=False):
        """Batched Light::Sample_Li + VisibilityTester::Unoccluded (pg_light_sample_at) on host arrays: ref the records intersect_at returns (only prim, p,
        p_error, n and time are read; prim >= 0 marks a valid point), light one lights[] index and u two floats per reference point.  Returns the
        records as a structured array of LIGHT_SAMPLE_DTYPE, or -- with_shadow_rays -- (records, (n, 8) float32: origin, tMax, direction, time of
        the tested samples' shadow rays, zeros elsewhere)."""
        ref, light, u, n = self._light_inputs(ref, light, u, 2)
        out = np.empty(n, LIGHT_SAMPLE_DTYPE)
        shadow = np.empty((n, 8), np.float32) if with_shadow_rays else None
        _check(gpu_lib().pg_light_sample_at(self._h, n, ref.ctypes.data, light.ctypes.data, u.ctypes.data, out.ctypes.data,
                                            None if shadow is None else shadow.ctypes.data, PG_MEM_HOST, None), "pg_light_sample_at")
        return (out, shadow) if with_shadow_rays else out

    def light_pdf_at(self, ref, light, wi):
        """Batched Light::Pdf_Li(ref, wi) (pg_light_pdf_at) on host arrays: ref and light as light_sample_at takes them, wi three floats per reference
        point (world space, used as given).  Returns float32 (n,); moves no counter."""
        ref, light, wi, n = self._light_inputs(ref, light, wi, 3)
        pdf = np.empty(n, np.float32)
        _check(gpu_lib().pg_light_pdf_at(self._h, n, ref.ctypes.data, light.ctypes.data, wi.ctypes.data, pdf.ctypes.data, PG_MEM_HOST, None), "pg_light_pdf_at")
        return pdf

    def light_le_at(self, o, d, tmax, time=None, with_interaction=False):
        """The emitted radiance each ray meets (pg_light_le_at) on host arrays: the rays as intersect_at takes them; float32 (n, 3) -- isect.Le(-ray.d) at
        the closest hit, the infinite lights' Le(ray) summed in light order for an escaped ray -- or, with_interaction, (Le, what intersect_at
        returns for the same rays) from the one trace."""
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        le = np.empty((n, 3), np.float32)
        isect = np.empty(n, INTERACTION_DTYPE) if with_interaction else None
        _check(gpu_lib().pg_light_le_at(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                        None if isect is None else isect.ctypes.data, le.ctypes.data, PG_MEM_HOST, None), "pg_light_le_at")
        return (le, isect) if with_interaction else le

    def light_sample_at_device(self, n, ref_ptr, light_ptr, u_ptr, out_ptr, shadow_ptr=None, stream=None):
        """pg_light_sample_at on caller-owned device buffers (raw pointers, as intersect_at_device takes them): n records of INTERACTION_DTYPE at ref_ptr,
        n int32 at light_ptr, 2 n floats at u_ptr; n records of LIGHT_SAMPLE_DTYPE written at out_ptr and, unless shadow_ptr is None, 8 n floats at
        shadow_ptr.  Nothing visits the host."""
        _check(gpu_lib().pg_light_sample_at(self._h, n, ref_ptr, light_ptr, u_ptr, out_ptr, shadow_ptr, PG_MEM_DEVICE, stream), "pg_light_sample_at")

    def light_pdf_at_device(self, n, ref_ptr, light_ptr, wi_ptr, pdf_ptr, stream=None):
        """pg_light_pdf_at on caller-owned device buffers: 3 n floats at wi_ptr, n floats written at pdf_ptr."""
        _check(gpu_lib().pg_light_pdf_at(self._h, n, ref_ptr, light_ptr, wi_ptr, pdf_ptr, PG_MEM_DEVICE, stream), "pg_light_pdf_at")

    def light_le_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, isect_ptr, le_ptr, stream=None):
        """pg_light_le_at on caller-owned device buffers: the rays as intersect_at_device takes them, 3 n floats written at le_ptr and, unless isect_ptr is
        None, n records of INTERACTION_DTYPE at isect_ptr."""
        _check(gpu_lib().pg_light_le_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, isect_ptr, le_ptr, PG_MEM_DEVICE, stream), "pg_light_le_at")

    @staticmethod
    def _medium_inputs(n, medium, u):
        medium = np.ascontiguousarray(medium, np.int32)
        if medium.size != n:
            raise ValueError("medium holds one index per ray")
        if u is None:
            return medium, None, 0
        u = np.ascontiguousarray(u, np.float32)
        if u.size % max(n, 1) != 0 or (n == 0 and u.size):
            raise ValueError("u holds the same number of draws for every ray")
        n_u = u.size // n if n else 0
        return medium, (u if n_u else None), n_u

    def transmittance_at(self, o, d, tmax, p1, medium, u=None, time=None):
        """Batched VisibilityTester::Tr (pg_transmittance_at) on host arrays: the rays of p0.SpawnRayTo(p1) as light_sample_at reports them (origin, direction,
        tmax = 1 - ShadowEpsilon, time), p1 three floats per ray (the point the walk re-aims at), medium one media[] index per ray (-1 = none: the
        ray's medium), u an (n, n_u) array of sampler draws per ray or None (a scene without grid media draws nothing).  Returns a structured array of
        TRANSMITTANCE_DTYPE; a record with draws_used > n_u ran out of draws and must be discarded."""
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        p1 = np.ascontiguousarray(p1, np.float32)
        if p1.size != 3 * n:
            raise ValueError("p1 holds three floats per ray")
        medium, u, n_u = self._medium_inputs(n, medium, u)
        out = np.empty(n, TRANSMITTANCE_DTYPE)
        _check(gpu_lib().pg_transmittance_at(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                             p1.ctypes.data, medium.ctypes.data, None if u is None else u.ctypes.data, n_u, out.ctypes.data, PG_MEM_HOST, None),
               "pg_transmittance_at")
        return out

    def intersect_tr_at(self, o, d, tmax, medium, u=None, time=None, with_interaction=False):
        """Batched Scene::IntersectTr (pg_intersect_tr_at) on host arrays: the rays as intersect_at takes them, medium and u as transmittance_at takes them.
        Returns a structured array of TRANSMITTANCE_DTYPE or -- with_interaction -- (records, the final hits as INTERACTION_DTYPE, prim = -1 on escape)."""
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        medium, u, n_u = self._medium_inputs(n, medium, u)
        out = np.empty(n, TRANSMITTANCE_DTYPE)
        isect = np.empty(n, INTERACTION_DTYPE) if with_interaction else None
        _check(gpu_lib().pg_intersect_tr_at(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                            medium.ctypes.data, None if u is None else u.ctypes.data, n_u, out.ctypes.data,
                                            None if isect is None else isect.ctypes.data, PG_MEM_HOST, None), "pg_intersect_tr_at")
        return (out, isect) if with_interaction else out

    def medium_sample_at(self, o, d, tmax, medium, u, time=None):
        """Batched Medium::Sample (pg_medium_sample_at) on host arrays: the rays with the tmax Scene::Intersect left (intersect_at's t), medium one media[]
        index per ray, u an (n, n_u) array of draws (a homogeneous medium takes two).  Returns a structured array of MEDIUM_SAMPLE_DTYPE; traces nothing
        and moves no counter."""
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        medium, u, n_u = self._medium_inputs(n, medium, u)
        out = np.empty(n, MEDIUM_SAMPLE_DTYPE)
        _check(gpu_lib().pg_medium_sample_at(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                             medium.ctypes.data, None if u is None else u.ctypes.data, n_u, out.ctypes.data, PG_MEM_HOST, None),
               "pg_medium_sample_at")
        return out

    def transmittance_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, p1_ptr, medium_ptr, u_ptr, n_u, out_ptr, stream=None):
        """pg_transmittance_at on caller-owned device buffers (raw pointers, as intersect_at_device takes them): 3 n floats at p1_ptr, n int32 at medium_ptr,
        n * n_u floats at u_ptr (None with n_u = 0); n records of TRANSMITTANCE_DTYPE written at out_ptr.  Nothing visits the host."""
        _check(gpu_lib().pg_transmittance_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, p1_ptr, medium_ptr, u_ptr, int(n_u), out_ptr, PG_MEM_DEVICE, stream),
               "pg_transmittance_at")

    def intersect_tr_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, medium_ptr, u_ptr, n_u, out_ptr, isect_ptr=None, stream=None):
        """pg_intersect_tr_at on caller-owned device buffers: the outputs as transmittance_at_device's and, unless isect_ptr is None, n records of
        INTERACTION_DTYPE at isect_ptr."""
        _check(gpu_lib().pg_intersect_tr_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, medium_ptr, u_ptr, int(n_u), out_ptr, isect_ptr, PG_MEM_DEVICE, stream),
               "pg_intersect_tr_at")

    def medium_sample_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, medium_ptr, u_ptr, n_u, out_ptr, stream=None):
        """pg_medium_sample_at on caller-owned device buffers: n records of MEDIUM_SAMPLE_DTYPE written at out_ptr."""
        _check(gpu_lib().pg_medium_sample_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, medium_ptr, u_ptr, int(n_u), out_ptr, PG_MEM_DEVICE, stream),
               "pg_medium_sample_at")

    def subsurface_sample_at(self, o, d, tmax, u, time=None, with_po=False):
        """Batched BSSRDF::Sample_S at the rays' closest hits (pg_subsurface_sample_at) on host arrays: the rays as intersect_at takes them, u three floats
        per ray (u1, u2.x, u2.y).  Returns (records of SUBSURFACE_SAMPLE_DTYPE, the exit points pi as INTERACTION_DTYPE: prim = -1 unless status == 2) or --
        with_po -- (records, pi, what intersect_at returns for the same rays) from the one trace."""
        o, d, tmax, time, n = self._rays(o, d, tmax, time)
        u = np.ascontiguousarray(u, np.float32)
        if u.size != 3 * n:
            raise ValueError("u holds three floats per ray")
        out, pi = np.empty(n, SUBSURFACE_SAMPLE_DTYPE), np.empty(n, INTERACTION_DTYPE)
        po = np.empty(n, INTERACTION_DTYPE) if with_po else None
        _check(gpu_lib().pg_subsurface_sample_at(self._h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data, None if time is None else time.ctypes.data,
                                                 u.ctypes.data, None if po is None else po.ctypes.data, pi.ctypes.data, out.ctypes.data, PG_MEM_HOST, None),
               "pg_subsurface_sample_at")
        return (out, pi, po) if with_po else (out, pi)

    def _adapter(self, name, pi, eta, extra, per, flags):
        pi = np.ascontiguousarray(pi, INTERACTION_DTYPE)
        eta = np.ascontiguousarray(eta, np.float32)
        extra = np.ascontiguousarray(extra, np.float32)
        n = pi.size
        if eta.size != n or extra.size != per * n:
            raise ValueError("eta holds one float and " + ("wi three floats" if per == 3 else "u two floats") + " per exit point")
        out = np.empty(n, SCATTER_DTYPE)
        _check(getattr(gpu_lib(), name)(self._h, n, pi.ctypes.data, eta.ctypes.data, extra.ctypes.data, int(flags), out.ctypes.data, PG_MEM_HOST, None), name)
        return out

    def subsurface_f_at(self, pi, eta, wi, flags=31):
        """Batched BSDF::f and BSDF::Pdf of the BSDF Sample_S installs at the exit points (pg_subsurface_f_at) on host arrays: pi the records
        subsurface_sample_at returns (prim >= 0 marks a valid one), eta one float per record (the sample's eta), wi three floats per record (world space,
        used as given), flags one BxDFType mask.  Returns SCATTER_DTYPE records; traces nothing and moves no counter."""
        return self._adapter("pg_subsurface_f_at", pi, eta, wi, 3, flags)

    def subsurface_sample_f_at(self, pi, eta, u, flags=31):
        """Batched BSDF::Sample_f of the same BSDF (pg_subsurface_sample_f_at): as subsurface_f_at, with u two floats per record."""
        return self._adapter("pg_subsurface_sample_f_at", pi, eta, u, 2, flags)

    def subsurface_sample_at_device(self, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, po_ptr, pi_ptr, out_ptr, stream=None):
        """pg_subsurface_sample_at on caller-owned device buffers (raw pointers, as intersect_at_device takes them): 3 n floats at u_ptr; n records of
        SUBSURFACE_SAMPLE_DTYPE written at out_ptr, n of INTERACTION_DTYPE at pi_ptr and, unless po_ptr is None, at po_ptr.  Nothing visits the host."""
        _check(gpu_lib().pg_subsurface_sample_at(self._h, n, o_ptr, d_ptr, tmax_ptr, time_ptr, u_ptr, po_ptr, pi_ptr, out_ptr, PG_MEM_DEVICE, stream),
               "pg_subsurface_sample_at")

    def subsurface_f_at_device(self, n, pi_ptr, eta_ptr, wi_ptr, flags, out_ptr, stream=None):
        """pg_subsurface_f_at on caller-owned device buffers: n records of INTERACTION_DTYPE at pi_ptr, n floats at eta_ptr, 3 n at wi_ptr; n records of
        SCATTER_DTYPE written at out_ptr."""
        _check(gpu_lib().pg_subsurface_f_at(self._h, n, pi_ptr, eta_ptr, wi_ptr, int(flags), out_ptr, PG_MEM_DEVICE, stream), "pg_subsurface_f_at")

    def subsurface_sample_f_at_device(self, n, pi_ptr, eta_ptr, u_ptr, flags, out_ptr, stream=None):
        """pg_subsurface_sample_f_at on caller-owned device buffers: 2 n floats at u_ptr, the rest as subsurface_f_at_device's."""
        _check(gpu_lib().pg_subsurface_sample_f_at(self._h, n, pi_ptr, eta_ptr, u_ptr, int(flags), out_ptr, PG_MEM_DEVICE, stream), "pg_subsurface_sample_f_at")

    def counters(self):
        c = PgCounters()
        _check(gpu_lib().pg_counters(self._h, C.byref(c)), "pg_counters")
        return c.as_dict()

    def counters_reset(self):
        _check(gpu_lib().pg_counters_reset(self._h), "pg_counters_reset")

    def set_option(self, option, value):
        """pg_scene_set_option (abi.PG_OPT_*): per-scene switches that never change an image."""
        _check(gpu_lib().pg_scene_set_option(self._h, int(option), int(value)), "pg_scene_set_option")


def render_sharded(gpu_scenes, rd, max_strays=None):
    """pg_render_sharded: the frame of rd (tile_first 0, tile_step 1) over the devices of gpu_scenes -- one host thread per
    device, the packed shards gathered on the first device by one ncclGather (RCCL) or, where RCCL cannot run, peer copies
    (shard_transport() tells which).  Returns [(shard rd, film, strays)] per rank."""
    _path_family_only(rd, "render_sharded")
    n = len(gpu_scenes)
    shards = []
    for r in range(n):
        srd = PgRenderDesc.from_buffer_copy(rd)
        srd.tile_first, srd.tile_step = r, n
        shards.append(srd)
    counts = [GpuScene.tile_count(s) for s in shards]
    if max_strays is None:
        max_strays = default_max_strays(rd, max(counts))
    films = [np.zeros(c * rd.tile_pixels, FILM_PIXEL_DTYPE) for c in counts]
    strays = [np.zeros(max_strays, STRAY_DTYPE) for _ in range(n)]
    handles = (C.c_void_p * n)(*[g._h for g in gpu_scenes])
    fptr = (C.c_void_p * n)(*[f.ctypes.data for f in films])
    sptr = (C.c_void_p * n)(*[s.ctypes.data for s in strays])
    ns = (C.c_int32 * n)()
    _check(gpu_lib().pg_render_sharded(handles, n, C.byref(rd), fptr, sptr, max_strays, ns), "pg_render_sharded")
    return [(shards[r], films[r], strays[r][:ns[r]]) for r in range(n)]


def shard_transport():
    """How the last render_sharded gathered: "rccl" or "peer (<reason>)"."""
    return gpu_lib().pg_shard_transport().decode()


def render_scene(scene, device=0):
    """Whole-frame render of a HostScene on one GPU; returns the final (h, w, 3) image."""
    gs = GpuScene(scene.desc, device)
    try:
        rd = scene.render_desc()
        dl = scene.direct_desc()
        film, strays = gs.render(rd) if dl is None else gs.render_direct(rd, dl)
        scene.film_clear()
        scene.film_merge(rd, film, strays)
        return scene.film_image(), gs.counters()
    finally:
        gs.close()
