"""PgCameraRay, the record of pg_camera_rays_at, and the three entry points of the camera queries (pg_camera_rays_at / pg_scatter_f_diff_at /
pg_scatter_sample_diff_at): the C header, the ctypes mirror and the NumPy dtype agree field for field, the ABI version did not move, no earlier record
changed its size, the symbols are exported and bound, and refused arguments answer before a device is touched.  No compute is launched here (runs
without a GPU)."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

from conftest import GOLD, ROOT

FIELDS = ["o", "t_max", "d", "time", "weight", "medium", "has_differentials", "reserved", "differentials"]
SIZES = [12, 4, 12, 4, 4, 4, 4, 4, 48]
# the records of the earlier queries: header name -> (size, the binding's dtype)
EARLIER = {"PgInteraction": (128, "INTERACTION_DTYPE"), "PgScatter": (64, "SCATTER_DTYPE"), "PgLightSample": (64, "LIGHT_SAMPLE_DTYPE"),
           "PgTransmittance": (32, "TRANSMITTANCE_DTYPE"), "PgMediumSample": (64, "MEDIUM_SAMPLE_DTYPE"), "PgSubsurfaceSample": (64, "SUBSURFACE_SAMPLE_DTYPE"),
           "PgFilmPixel": (16, "FILM_PIXEL_DTYPE"), "PgStraySample": (32, "STRAY_DTYPE")}


def parent_sizes():
    """PARENT_SIZES of tests/test_directlighting_frontend.py: the sizes of the description structures (not retyped here)."""
    spec = importlib.util.spec_from_file_location("directlighting_frontend", os.path.join(os.path.dirname(__file__), "test_directlighting_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PARENT_SIZES


def test_camera_ray_layout_matches_header_and_nothing_else_moved(pkg, tmp_path):
    parent = parent_sizes()
    names = ["PgCameraRay"] + sorted(EARLIER) + sorted(parent)
    body = "\n".join(f"size_t size_{n}(void) {{ return sizeof({n}); }}" for n in names) + "\nint abi_version(void) { return PG_ABI_VERSION; }\n"
    body += "\n".join(f"size_t off_{f}(void) {{ return offsetof(PgCameraRay, {f}); }}\nsize_t len_{f}(void) {{ return sizeof(((PgCameraRay *)0)->{f}); }}" for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}\n')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    for n in names:
        getattr(lib, "size_" + n).restype = C.c_size_t
    dt = pkg.CAMERA_RAY_DTYPE
    assert lib.size_PgCameraRay() == 96 == dt.itemsize == C.sizeof(pkg.abi.PgCameraRay) and 96 % 16 == 0  # six float4
    assert lib.abi_version() == 30 == pkg.abi.PG_ABI_VERSION
    for n, (size, dtype) in EARLIER.items():
        assert getattr(lib, "size_" + n)() == size == C.sizeof(getattr(pkg.abi, n)) == getattr(pkg, dtype).itemsize, n
    for n, size in parent.items():
        assert getattr(lib, "size_" + n)() == size == C.sizeof(getattr(pkg.abi, n)), n
    assert list(dt.names) == FIELDS == [n for n, _ in pkg.abi.PgCameraRay._fields_]  # every field of the header's structure, in its order
    at = 0
    for f, want in zip(FIELDS, SIZES):
        off, size = getattr(lib, "off_" + f), getattr(lib, "len_" + f)
        off.restype = size.restype = C.c_size_t
        assert off() == dt.fields[f][1] == getattr(pkg.abi.PgCameraRay, f).offset == at, f  # (no padding)
        assert size() == dt.fields[f][0].itemsize == getattr(pkg.abi.PgCameraRay, f).size == want, f
        at += want
    assert dt.fields["differentials"][1] == 48  # the last three float4: what lens_camera_sample writes and tex_hit_setup reads
    ints = ("medium", "has_differentials")
    assert all(dt.fields[f][0].base == ("int32" if f in ints else "float32") for f in FIELDS)


def test_the_three_entry_points_exist(pkg):
    lib = pkg.gpu_lib()
    sym = pkg.abi.GPU_SYMBOLS
    res, args = sym["pg_camera_rays_at"]
    assert res is C.c_int and len(args) == 9 and args[1] == C.POINTER(pkg.abi.PgRenderDesc) and args[-2:] == [C.c_int, C.c_void_p]
    for name, plain in (("pg_scatter_f_diff_at", "pg_scatter_f_at"), ("pg_scatter_sample_diff_at", "pg_scatter_sample_at")):
        res, args = sym[name]
        assert res is C.c_int and args == sym[plain][1][:7] + [C.c_void_p] + sym[plain][1][7:]  # the plain call's arguments with diff behind wi / u
    for name in ("pg_camera_rays_at", "pg_scatter_f_diff_at", "pg_scatter_sample_diff_at"):
        assert getattr(lib, name) is not None
    for method in ("camera_rays", "camera_rays_device", "scatter_f_at", "scatter_sample_at", "scatter_f_diff_at_device", "scatter_sample_diff_at_device"):
        assert callable(getattr(pkg.GpuScene, method))


def test_refused_arguments_answer_without_a_device(pkg):
    """The argument checks and the description's own checks come before anything touches a device -- or the scene: they answer on a machine without one."""
    lib = pkg.gpu_lib()
    a = np.zeros(64, np.float32)
    p = a.ctypes.data
    scene = C.c_void_p(8)  # (never dereferenced: every call below is refused first)
    host = pkg.HostScene(os.path.join(GOLD, "cornell_32.pbrt"))
    rd = host.render_desc()
    H, D = pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE
    fn = lib.pg_camera_rays_at
    for mem in (H, D):
        for args in ((None, C.byref(rd), 1, p, p, p, p), (scene, None, 1, p, p, p, p), (scene, C.byref(rd), 1, p, p, p, None), (scene, C.byref(rd), 1, None, p, p, p),
                     (scene, C.byref(rd), -1, p, p, p, p)):
            assert fn(*args, mem, None) == -1 and b"pg_camera_rays_at: null argument" in lib.pg_last_error(), args
    assert fn(scene, C.byref(rd), 0, None, None, None, None, H, None) == 0  # an empty batch touches nothing
    bad = pkg.abi.PgRenderDesc.from_buffer_copy(rd)
    bad.camera_type = 4
    assert fn(scene, C.byref(bad), 1, p, None, None, p, H, None) == -1 and b"pg_render: camera_type 4 (0 = perspective" in lib.pg_last_error()
    bad = pkg.abi.PgRenderDesc.from_buffer_copy(rd)
    bad.camera_type, bad.n_lens_interfaces = 3, 0
    assert fn(scene, C.byref(bad), 1, p, None, None, p, H, None) == -1 and b"realistic camera with 0 lens interfaces" in lib.pg_last_error()
    bad = pkg.abi.PgRenderDesc.from_buffer_copy(rd)
    bad.spp = 0
    assert fn(scene, C.byref(bad), 1, p, None, None, p, H, None) == -1 and b"bad spp" in lib.pg_last_error()
    for name in ("pg_scatter_f_diff_at", "pg_scatter_sample_diff_at"):
        fn = getattr(lib, name)
        tag = name.encode() + b":"
        assert fn(None, 1, p, p, p, p, p, p, 31, None, p, H, None) == -1 and tag in lib.pg_last_error()  # no scene
        for k in (0, 1, 2, 4, 8):  # o, d, tmax, wi / u, out (time, diff and isect may be NULL)
            args = [p, p, p, p, p, p, 31, p, p]
            args[k] = None
            for mem in (H, D):
                assert fn(scene, 1, *args, mem, None) == -1 and tag in lib.pg_last_error() and b"null argument" in lib.pg_last_error(), (name, k)
        assert fn(scene, -1, p, p, p, p, p, p, 31, p, p, H, None) == -1 and tag in lib.pg_last_error()
        assert fn(scene, 1, p, p, p, p, p, p, 32, p, p, H, None) == -1 and b"flags" in lib.pg_last_error()
        assert fn(scene, 1, p, p, p, p, p, p + (-p) % 16 + 4, 31, p, p, D, None) == -1 and b"16-byte aligned" in lib.pg_last_error()  # device differentials are read as float4
        assert fn(scene, 0, None, None, None, None, None, None, 31, None, None, H, None) == 0
    assert not a.any()
    host.close()
