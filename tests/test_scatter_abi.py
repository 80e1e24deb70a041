"""PgScatter, the record of pg_scatter_f_at / pg_scatter_sample_at: the C header, the ctypes mirror and the NumPy dtype agree field for field, the ABI
version did not move and no existing structure changed its size.  No compute is launched here (runs without a GPU)."""
import ctypes as C
import importlib.util
import os
import subprocess

from conftest import ROOT

FIELDS = ["prim", "n_bxdfs", "n_matching", "sampled_type", "f", "pdf", "wi", "eta", "shading_n", "types"]
SIZES = [4, 4, 4, 4, 12, 4, 12, 4, 12, 4]


def parent_sizes():
    """PARENT_SIZES of tests/test_directlighting_frontend.py: the sizes the structures had before this record was added (not retyped here)."""
    spec = importlib.util.spec_from_file_location("directlighting_frontend", os.path.join(os.path.dirname(__file__), "test_directlighting_frontend.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PARENT_SIZES


def test_scatter_layout_matches_header_and_nothing_else_moved(pkg, tmp_path):
    parent = parent_sizes()
    assert sorted(parent) == ["PgCounters", "PgRenderDesc", "PgSceneDesc"]
    names = ["PgScatter", "PgInteraction"] + sorted(parent)
    src = tmp_path / "probe.c"
    body = "\n".join(f"size_t size_{n}(void) {{ return sizeof({n}); }}" for n in names) + "\nint abi_version(void) { return PG_ABI_VERSION; }\n"
    body += "\n".join(f"size_t off_{f}(void) {{ return offsetof(PgScatter, {f}); }}\nsize_t len_{f}(void) {{ return sizeof(((PgScatter *)0)->{f}); }}" for f in FIELDS)
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}\n')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    for n in names:
        getattr(lib, "size_" + n).restype = C.c_size_t
    dt = pkg.SCATTER_DTYPE
    assert lib.size_PgScatter() == 64 == dt.itemsize == C.sizeof(pkg.abi.PgScatter)
    assert lib.abi_version() == 30 == pkg.abi.PG_ABI_VERSION
    assert lib.size_PgInteraction() == 128 == C.sizeof(pkg.abi.PgInteraction) == pkg.INTERACTION_DTYPE.itemsize
    for n, size in parent.items():
        assert getattr(lib, "size_" + n)() == size == C.sizeof(getattr(pkg.abi, n)), n
    assert list(dt.names) == FIELDS == [n for n, _ in pkg.abi.PgScatter._fields_]  # every field of the header's structure, in its order
    at = 0
    for f, want in zip(FIELDS, SIZES):
        off, size = getattr(lib, "off_" + f), getattr(lib, "len_" + f)
        off.restype = size.restype = C.c_size_t
        assert off() == dt.fields[f][1] == getattr(pkg.abi.PgScatter, f).offset == at, f  # (no padding: four float4)
        assert size() == dt.fields[f][0].itemsize == getattr(pkg.abi.PgScatter, f).size == want, f
        at += want
    assert all(dt.fields[f][0].base == "int32" for f in FIELDS[:4]) and all(dt.fields[f][0].base == "float32" for f in FIELDS[4:9]) and dt.fields["types"][0] == "uint32"


def test_both_entry_points_are_bound(pkg):
    for name in ("pg_scatter_f_at", "pg_scatter_sample_at"):
        assert name in pkg.abi.GPU_SYMBOLS, name
        res, args = pkg.abi.GPU_SYMBOLS[name]
        assert res is C.c_int and len(args) == 12  # scene, n, o, d, tmax, time, wi / u, flags, isect, out, mem, stream
        assert args == pkg.abi.GPU_SYMBOLS["pg_intersect_at"][1][:6] + [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    for method in ("scatter_f_at", "scatter_sample_at", "scatter_f_at_device", "scatter_sample_at_device"):
        assert callable(getattr(pkg.GpuScene, method))


def test_refused_arguments_answer_without_a_device(pkg):
    """The argument checks come before anything touches a device: they answer on a machine without one, with the entry point's name."""
    import numpy as np
    lib = pkg.gpu_lib()
    a = np.zeros(16, np.float32)
    p = a.ctypes.data
    scene = C.c_void_p(8)  # (never dereferenced: every call below is refused first)
    for name in ("pg_scatter_f_at", "pg_scatter_sample_at"):
        fn = getattr(lib, name)
        tag = name.encode() + b":"
        assert fn(None, 1, None, None, None, None, None, 31, None, None, pkg.PG_MEM_HOST, None) == -1 and tag in lib.pg_last_error()
        assert fn(None, 1, p, p, p, p, p, 31, None, p, pkg.PG_MEM_HOST, None) == -1 and tag in lib.pg_last_error()  # no scene
        for k in (0, 1, 2, 4, 7):  # o, d, tmax, wi / u, out (time and isect may be NULL)
            args = [p, p, p, p, p, 31, p, p]
            args[k] = None
            for mem in (pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE):
                assert fn(scene, 1, *args, mem, None) == -1 and tag in lib.pg_last_error() and b"null argument" in lib.pg_last_error(), (name, k)
        assert fn(scene, -1, p, p, p, p, p, 31, p, p, pkg.PG_MEM_HOST, None) == -1 and tag in lib.pg_last_error()
        for flags in (32, -1, 1 << 20):
            assert fn(scene, 1, p, p, p, p, p, flags, p, p, pkg.PG_MEM_HOST, None) == -1
            assert tag in lib.pg_last_error() and b"flags" in lib.pg_last_error(), (name, flags)
    assert not a.any()
