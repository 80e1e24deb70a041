"""PgInteraction, the record of pg_intersect_at: the C header, the ctypes mirror and the NumPy dtype agree field for field, and the ABI version did not
move.  No compute is launched here (runs without a GPU)."""
import ctypes as C
import subprocess

from conftest import ROOT

FIELDS = ["prim", "instance", "instance_inner", "material", "light", "t", "time", "uv", "p", "p_error", "n", "wo", "shading_n", "shading_dpdu", "shading_dpdv",
          "reserved"]


def test_interaction_layout_matches_header(pkg, tmp_path):
    src = tmp_path / "probe.c"
    body = "size_t size_PgInteraction(void) { return sizeof(PgInteraction); }\nint abi_version(void) { return PG_ABI_VERSION; }\n"
    body += "\n".join(f"size_t off_{f}(void) {{ return offsetof(PgInteraction, {f}); }}\nsize_t len_{f}(void) {{ return sizeof(((PgInteraction *)0)->{f}); }}" for f in FIELDS)
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}\n')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.size_PgInteraction.restype = C.c_size_t
    dt = pkg.INTERACTION_DTYPE
    assert lib.size_PgInteraction() == 128 == dt.itemsize == C.sizeof(pkg.abi.PgInteraction)
    assert lib.abi_version() == 30 == pkg.abi.PG_ABI_VERSION
    assert list(dt.names) == FIELDS == [n for n, _ in pkg.abi.PgInteraction._fields_]  # every field of the header's structure, in its order
    for f in FIELDS:
        off, size = getattr(lib, "off_" + f), getattr(lib, "len_" + f)
        off.restype = size.restype = C.c_size_t
        assert off() == dt.fields[f][1] == getattr(pkg.abi.PgInteraction, f).offset, f
        assert size() == dt.fields[f][0].itemsize == getattr(pkg.abi.PgInteraction, f).size, f
    assert all(dt.fields[f][0].base == "int32" for f in FIELDS[:5]) and all(dt.fields[f][0].base == "float32" for f in FIELDS[5:])


def test_both_entry_points_are_bound(pkg):
    for name in ("pg_intersect_at", "pg_intersect_p_at"):
        assert name in pkg.abi.GPU_SYMBOLS, name
        res, args = pkg.abi.GPU_SYMBOLS[name]
        assert res is C.c_int and len(args) == 9  # scene, n, o, d, tmax, time, out / occluded, mem, stream
    for method in ("intersect_at", "intersect_p_at", "intersect_at_device"):
        assert callable(getattr(pkg.GpuScene, method))


def test_null_arguments_are_refused_without_a_device(pkg):
    """The argument checks come before anything touches a device: they answer on a machine without one."""
    lib = pkg.gpu_lib()
    assert lib.pg_intersect_at(None, 1, None, None, None, None, None, pkg.PG_MEM_HOST, None) == -1 and b"pg_intersect_at" in lib.pg_last_error()
    assert lib.pg_intersect_p_at(None, 1, None, None, None, None, None, pkg.PG_MEM_HOST, None) == -1 and b"pg_intersect_p_at" in lib.pg_last_error()
