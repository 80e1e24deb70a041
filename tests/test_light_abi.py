"""PgLightSample, the record of pg_light_sample_at, and the three light queries' entry points (pg_light_sample_at / pg_light_pdf_at / pg_light_le_at): the C
header, the ctypes mirror and the NumPy dtype agree field for field, the ABI version did not move, the symbols are exported and bound, and refused
arguments answer before a device is touched.  No compute is launched here (runs without a GPU)."""
import ctypes as C
import subprocess

import numpy as np

from conftest import ROOT

FIELDS = ["light", "visibility", "pdf", "Li", "wi", "p_light", "n_light", "reserved"]
SIZES = [4, 4, 4, 12, 12, 12, 12, 4]
ENTRY_POINTS = ("pg_light_sample_at", "pg_light_pdf_at", "pg_light_le_at")


def test_light_sample_layout_matches_header(pkg, tmp_path):
    src = tmp_path / "probe.c"
    body = "size_t size_rec(void) { return sizeof(PgLightSample); }\nsize_t size_isect(void) { return sizeof(PgInteraction); }\nint abi_version(void) { return PG_ABI_VERSION; }\n"
    body += "\n".join(f"size_t off_{f}(void) {{ return offsetof(PgLightSample, {f}); }}\nsize_t len_{f}(void) {{ return sizeof(((PgLightSample *)0)->{f}); }}" for f in FIELDS)
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}\n')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.size_rec.restype = lib.size_isect.restype = C.c_size_t
    dt = pkg.LIGHT_SAMPLE_DTYPE
    assert lib.size_rec() == 64 == dt.itemsize == C.sizeof(pkg.abi.PgLightSample)
    assert lib.size_isect() == 128 == pkg.INTERACTION_DTYPE.itemsize  # the reference points' record did not move
    assert list(dt.names) == FIELDS == [n for n, _ in pkg.abi.PgLightSample._fields_]  # every field of the header's structure, in its order
    at = 0
    for f, want in zip(FIELDS, SIZES):
        off, size = getattr(lib, "off_" + f), getattr(lib, "len_" + f)
        off.restype = size.restype = C.c_size_t
        assert off() == dt.fields[f][1] == getattr(pkg.abi.PgLightSample, f).offset == at, f  # (no padding: four float4)
        assert size() == dt.fields[f][0].itemsize == getattr(pkg.abi.PgLightSample, f).size == want, f
        at += want
    assert all(dt.fields[f][0].base == "int32" for f in FIELDS[:2]) and all(dt.fields[f][0].base == "float32" for f in FIELDS[2:])


def test_abi_version_is_still_30(pkg, tmp_path):
    src = tmp_path / "v.c"
    src.write_text(f'#include "{ROOT}/include/pbrt_gpu.h"\nint abi_version(void) {{ return PG_ABI_VERSION; }}\n')
    so = tmp_path / "v.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    assert C.CDLL(str(so)).abi_version() == 30 == pkg.abi.PG_ABI_VERSION


def test_the_three_entry_points_exist(pkg):
    lib = pkg.gpu_lib()
    want = {"pg_light_sample_at": 9, "pg_light_pdf_at": 8, "pg_light_le_at": 10}
    for name in ENTRY_POINTS:
        assert name in pkg.abi.GPU_SYMBOLS, name
        res, args = pkg.abi.GPU_SYMBOLS[name]
        assert res is C.c_int and len(args) == want[name] and args[-2:] == [C.c_int, C.c_void_p]  # ..., mem, stream
        assert getattr(lib, name) is not None
    for method in ("light_sample_at", "light_pdf_at", "light_le_at", "light_sample_at_device", "light_pdf_at_device", "light_le_at_device"):
        assert callable(getattr(pkg.GpuScene, method))


def test_refused_arguments_answer_without_a_device(pkg):
    """The argument checks come before anything touches a device: they answer on a machine without one, with the entry point's name."""
    lib = pkg.gpu_lib()
    a = np.zeros(64, np.float32)
    p = a.ctypes.data
    scene = C.c_void_p(8)  # (never dereferenced: every call below is refused first)
    H, D = pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE
    # the pointer arguments after (scene, n), and which of them may be NULL
    cases = {"pg_light_sample_at": ([p, p, p, p, p], (4,)),  # ref, light, u, out, shadow
             "pg_light_pdf_at": ([p, p, p, p], ()),          # ref, light, wi, pdf
             "pg_light_le_at": ([p, p, p, p, p, p], (3, 4))}  # o, d, tmax, time, isect, Le
    for name, (args, optional) in cases.items():
        fn = getattr(lib, name)
        tag = name.encode() + b":"
        assert fn(None, 1, *([None] * len(args)), H, None) == -1 and tag in lib.pg_last_error()
        assert fn(None, 1, *args, H, None) == -1 and tag in lib.pg_last_error()  # no scene
        for k in range(len(args)):
            if k in optional: continue
            bad = list(args)
            bad[k] = None
            for mem in (H, D):
                assert fn(scene, 1, *bad, mem, None) == -1 and tag in lib.pg_last_error() and b"null argument" in lib.pg_last_error(), (name, k)
        assert fn(scene, -1, *args, H, None) == -1 and tag in lib.pg_last_error()
    assert not a.any()


def test_an_empty_batch_returns_ok_and_touches_nothing(pkg):
    lib = pkg.gpu_lib()
    scene = C.c_void_p(8)  # (never dereferenced: n == 0 returns before anything is read)
    assert lib.pg_light_sample_at(scene, 0, None, None, None, None, None, pkg.PG_MEM_HOST, None) == 0
    assert lib.pg_light_pdf_at(scene, 0, None, None, None, None, pkg.PG_MEM_DEVICE, None) == 0
    assert lib.pg_light_le_at(scene, 0, None, None, None, None, None, None, pkg.PG_MEM_HOST, None) == 0
