"""PgCameraWeDesc, PgCameraImportance and PgCameraSample -- the description and the records of pg_camera_we_at / pg_camera_sample_wi_at -- and the entry points of
camera importance and TransportMode::Importance (those two, pg_scatter_f_mode_at / pg_scatter_sample_mode_at and pbrt_host_camera_we_desc): the C header, the
ctypes mirror and the NumPy dtype agree field for field and offset for offset, the ABI version did not move, no earlier record changed its size, the symbols
are exported and bound, and refused arguments answer before a device is touched.  No compute is launched here (runs without a GPU)."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

from conftest import GOLD, ROOT

# structure -> [(field, bytes)], in the header's order; None: no NumPy dtype (a description, not a record)
LAYOUT = {
    "PgCameraWeDesc": ([("camera_to_raster", 64), ("world_to_camera", 64), ("world_to_camera_end", 64), ("image_area", 4)], None, 196),
    "PgCameraImportance": ([("status", 4), ("We", 4), ("pdf_pos", 4), ("pdf_dir", 4), ("p_raster", 8), ("cos_theta", 4), ("reserved", 4)], "CAMERA_IMPORTANCE_DTYPE", 32),
    "PgCameraSample": ([("status", 4), ("visibility", 4), ("pdf", 4), ("We", 4), ("wi", 12), ("p_lens", 12), ("n_lens", 12), ("p_raster", 8), ("reserved", 4)],
                       "CAMERA_SAMPLE_DTYPE", 64),
}
EARLIER = {"PgInteraction": (128, "INTERACTION_DTYPE"), "PgScatter": (64, "SCATTER_DTYPE"), "PgLightSample": (64, "LIGHT_SAMPLE_DTYPE"),
           "PgTransmittance": (32, "TRANSMITTANCE_DTYPE"), "PgMediumSample": (64, "MEDIUM_SAMPLE_DTYPE"), "PgSubsurfaceSample": (64, "SUBSURFACE_SAMPLE_DTYPE"),
           "PgCameraRay": (96, "CAMERA_RAY_DTYPE"), "PgFilmPixel": (16, "FILM_PIXEL_DTYPE"), "PgStraySample": (32, "STRAY_DTYPE")}
NEW_GPU = ("pg_camera_we_at", "pg_camera_sample_wi_at", "pg_scatter_f_mode_at", "pg_scatter_sample_mode_at")


def parent_sizes():
    """PARENT_SIZES of tests/test_directlighting_frontend.py: the sizes of the description structures (not retyped here)."""
    spec = importlib.util.spec_from_file_location("directlighting_frontend", os.path.join(os.path.dirname(__file__), "test_directlighting_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PARENT_SIZES


def test_layouts_match_the_header_and_nothing_else_moved(pkg, tmp_path):
    parent = parent_sizes()
    names = sorted(LAYOUT) + sorted(EARLIER) + sorted(parent)
    body = "\n".join(f"size_t size_{n}(void) {{ return sizeof({n}); }}" for n in names) + "\nint abi_version(void) { return PG_ABI_VERSION; }\n"
    for s, (fields, _, _) in LAYOUT.items():
        body += "\n".join(f"size_t off_{s}_{f}(void) {{ return offsetof({s}, {f}); }}\nsize_t len_{s}_{f}(void) {{ return sizeof((({s} *)0)->{f}); }}" for f, _ in fields) + "\n"
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}\n')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    for n in names:
        getattr(lib, "size_" + n).restype = C.c_size_t
    assert lib.abi_version() == 30 == pkg.abi.PG_ABI_VERSION
    for n, (size, dtype) in EARLIER.items():
        assert getattr(lib, "size_" + n)() == size == C.sizeof(getattr(pkg.abi, n)) == getattr(pkg, dtype).itemsize, n
    for n, size in parent.items():
        assert getattr(lib, "size_" + n)() == size == C.sizeof(getattr(pkg.abi, n)), n
    for s, (fields, dtype, size) in LAYOUT.items():
        mirror = getattr(pkg.abi, s)
        dt = getattr(pkg, dtype) if dtype else None
        assert getattr(lib, "size_" + s)() == size == C.sizeof(mirror), s
        assert [f for f, _ in fields] == [n for n, _ in mirror._fields_], s  # every field of the header's structure, in its order
        if dt is not None:
            assert dt.itemsize == size and size % 16 == 0 and list(dt.names) == [f for f, _ in fields], s  # whole float4s
        at = 0
        for f, want in fields:
            off, length = getattr(lib, f"off_{s}_{f}"), getattr(lib, f"len_{s}_{f}")
            off.restype = length.restype = C.c_size_t
            assert off() == getattr(mirror, f).offset == at and length() == getattr(mirror, f).size == want, (s, f)  # (no padding)
            if dt is not None:
                assert dt.fields[f][1] == at and dt.fields[f][0].itemsize == want, (s, f)
                assert dt.fields[f][0].base == ("int32" if f in ("status", "visibility") else "float32"), (s, f)
            at += want
        assert at == size
    # k_light_visibility writes PgCameraSample::visibility where PgLightSample has it
    assert pkg.CAMERA_SAMPLE_DTYPE.fields["visibility"][1] == 4 == pkg.LIGHT_SAMPLE_DTYPE.fields["visibility"][1] == pkg.abi.PgCameraSample.visibility.offset


def test_the_five_entry_points_exist(pkg):
    lib, host = pkg.gpu_lib(), pkg.host_lib()
    sym = pkg.abi.GPU_SYMBOLS
    desc = [C.c_void_p, C.POINTER(pkg.abi.PgRenderDesc), C.POINTER(pkg.abi.PgCameraWeDesc), C.c_int32]
    assert sym["pg_camera_we_at"] == (C.c_int, desc + [C.c_void_p] * 4 + [C.c_int, C.c_void_p])
    assert sym["pg_camera_sample_wi_at"] == (C.c_int, desc + [C.c_void_p] * 4 + [C.c_int, C.c_void_p])
    for name, diff in (("pg_scatter_f_mode_at", "pg_scatter_f_diff_at"), ("pg_scatter_sample_mode_at", "pg_scatter_sample_diff_at")):
        res, args = sym[name]
        assert res is C.c_int and args == sym[diff][1][:9] + [C.c_int32] + sym[diff][1][9:]  # the _diff_ call's arguments with mode behind flags
    for name in NEW_GPU:
        assert getattr(lib, name) is not None
    assert pkg.abi.HOST_SYMBOLS["pbrt_host_camera_we_desc"] == (C.c_int, [C.c_void_p, C.POINTER(pkg.abi.PgCameraWeDesc)]) and host.pbrt_host_camera_we_desc is not None
    for method in ("camera_we_at", "camera_sample_wi_at", "camera_we_at_device", "camera_sample_wi_at_device", "scatter_f_mode_at_device", "scatter_sample_mode_at_device"):
        assert callable(getattr(pkg.GpuScene, method))
    assert callable(pkg.HostScene.camera_we_desc)


def test_refused_arguments_answer_without_a_device(pkg):
    """Every refusal comes before anything touches a device -- or the scene: the calls answer on a machine without one, for a scene pointer that is never read."""
    lib = pkg.gpu_lib()
    a = np.zeros(256, np.float32)
    p = a.ctypes.data
    scene = C.c_void_p(8)
    host = pkg.HostScene(os.path.join(GOLD, "cornell_32.pbrt"))
    rd, we = host.render_desc(), host.camera_we_desc()
    assert we is not None and we.image_area > 0
    H, D = pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE
    INVALID, UNSUPPORTED = -1, -2
    for name in ("pg_camera_we_at", "pg_camera_sample_wi_at"):
        fn = getattr(lib, name)
        tag = name.encode() + b":"
        good = [scene, C.byref(rd), C.byref(we), 1, p, p, p, p]  # scene, desc, we, n, o / ref, d / u, time / out, out / shadow
        required = (0, 1, 2, 4, 5, 7) if name == "pg_camera_we_at" else (0, 1, 2, 4, 5, 6)  # (time and shadow may be NULL)
        for mem in (H, D):
            for k in required:
                args = list(good)
                args[k] = None
                assert fn(*args, mem, None) == INVALID and tag + b" null argument" in lib.pg_last_error(), (name, k)
            args = list(good)
            args[3] = -1
            assert fn(*args, mem, None) == INVALID and tag + b" null argument" in lib.pg_last_error()
        assert fn(scene, C.byref(rd), C.byref(we), 0, None, None, None, None, H, None) == 0  # an empty batch touches nothing
        # a camera without We: refused as unsupported, whatever `we` holds
        for other, kind in (("camanim_ortho", 1), ("camanim_env", 2), (os.path.join("realistic", "a_singlet"), 3)):
            hs = pkg.HostScene(os.path.join(GOLD, other + ".pbrt"))
            other_rd = hs.render_desc()
            assert other_rd.camera_type == kind and hs.camera_we_desc() is None
            assert fn(scene, C.byref(other_rd), C.byref(we), 1, p, p, p, p, H, None) == UNSUPPORTED and tag in lib.pg_last_error() and b"perspective" in lib.pg_last_error()
            hs.close()
        for area in (0.0, -1.0, float("nan"), float("inf")):
            bad = pkg.abi.PgCameraWeDesc.from_buffer_copy(we)
            bad.image_area = area
            assert fn(scene, C.byref(rd), C.byref(bad), 1, p, p, p, p, H, None) == INVALID and b"image_area > 0" in lib.pg_last_error(), area
        bad = pkg.abi.PgCameraWeDesc.from_buffer_copy(we)
        bad.world_to_camera_end[5] = float("nan")
        assert fn(scene, C.byref(rd), C.byref(bad), 1, p, p, p, p, H, None) == INVALID and b"finite" in lib.pg_last_error()
        bad_rd = pkg.abi.PgRenderDesc.from_buffer_copy(rd)
        bad_rd.spp = 0  # the description is checked as pg_camera_rays_at checks it
        assert fn(scene, C.byref(bad_rd), C.byref(we), 1, p, p, p, p, H, None) == INVALID and b"bad spp" in lib.pg_last_error()
    for name in ("pg_scatter_f_mode_at", "pg_scatter_sample_mode_at"):
        fn = getattr(lib, name)
        tag = name.encode() + b":"
        for mode in (-1, 2, 7):
            assert fn(scene, 1, p, p, p, p, p, p, 31, mode, p, p, H, None) == INVALID and tag in lib.pg_last_error() and b"mode" in lib.pg_last_error(), mode
        assert fn(None, 1, p, p, p, p, p, p, 31, 1, None, p, H, None) == INVALID and tag in lib.pg_last_error()  # no scene
        for k in (0, 1, 2, 4, 9):  # o, d, tmax, wi / u, out (time, diff and isect may be NULL)
            args = [p, p, p, p, p, p, 31, 1, p, p]
            args[k] = None
            for mem in (H, D):
                assert fn(scene, 1, *args, mem, None) == INVALID and tag + b" null argument" in lib.pg_last_error(), (name, k)
        for mode in (0, 1):
            assert fn(scene, -1, p, p, p, p, p, p, 31, mode, p, p, H, None) == INVALID and tag in lib.pg_last_error()
            assert fn(scene, 1, p, p, p, p, p, p, 32, mode, p, p, H, None) == INVALID and b"flags" in lib.pg_last_error()
            assert fn(scene, 0, None, None, None, None, None, None, 31, mode, None, None, H, None) == 0
    assert not a.any()
    host.close()
