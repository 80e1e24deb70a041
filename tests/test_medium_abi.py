"""PgTransmittance and PgMediumSample, the records of the medium queries (pg_transmittance_at / pg_intersect_tr_at / pg_medium_sample_at): the C header, the
ctypes mirrors and the NumPy dtypes agree field for field, the ABI version and the earlier records did not move, the symbols are exported and bound, and
refused arguments answer before a device is touched.  No compute is launched here (runs without a GPU)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT

RECORDS = {
    "PgTransmittance": ("TRANSMITTANCE_DTYPE", 32, ["Tr", "status", "medium", "crossings", "draws_used", "reserved"], [12, 4, 4, 4, 4, 4],
                        {"Tr": "float32"}),
    "PgMediumSample": ("MEDIUM_SAMPLE_DTYPE", 64, ["sampled", "draws_used", "beta", "t", "p", "wo", "g", "medium", "reserved"], [4, 4, 12, 4, 12, 12, 4, 4, 8],
                       {"sampled": "int32", "draws_used": "int32", "medium": "int32"}),
}
ENTRY_POINTS = {"pg_transmittance_at": 13, "pg_intersect_tr_at": 13, "pg_medium_sample_at": 12}


@pytest.mark.parametrize("record", sorted(RECORDS))
def test_record_layout_matches_header(pkg, tmp_path, record):
    dtype_name, total, fields, sizes, kinds = RECORDS[record]
    src = tmp_path / "probe.c"
    body = f"size_t size_rec(void) {{ return sizeof({record}); }}\nsize_t size_isect(void) {{ return sizeof(PgInteraction); }}\n"
    body += "size_t size_light(void) { return sizeof(PgLightSample); }\n"
    body += "\n".join(f"size_t off_{f}(void) {{ return offsetof({record}, {f}); }}\nsize_t len_{f}(void) {{ return sizeof((({record} *)0)->{f}); }}" for f in fields)
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}\n')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.size_rec.restype = lib.size_isect.restype = lib.size_light.restype = C.c_size_t
    dt, ct = getattr(pkg, dtype_name), getattr(pkg.abi, record)
    assert lib.size_rec() == total == dt.itemsize == C.sizeof(ct)
    assert lib.size_isect() == 128 == pkg.INTERACTION_DTYPE.itemsize and lib.size_light() == 64 == pkg.LIGHT_SAMPLE_DTYPE.itemsize  # the earlier records did not move
    assert list(dt.names) == fields == [n for n, _ in ct._fields_]  # every field of the header's structure, in its order
    at = 0
    for f, want in zip(fields, sizes):
        off, size = getattr(lib, "off_" + f), getattr(lib, "len_" + f)
        off.restype = size.restype = C.c_size_t
        assert off() == dt.fields[f][1] == getattr(ct, f).offset == at, f  # (no padding: whole float4s)
        assert size() == dt.fields[f][0].itemsize == getattr(ct, f).size == want, f
        at += want
    assert at == total
    default = "int32" if record == "PgTransmittance" else "float32"
    for f in fields:
        assert dt.fields[f][0].base == kinds.get(f, default), f


def test_abi_version_is_still_30(pkg, tmp_path):
    src = tmp_path / "v.c"
    src.write_text(f'#include "{ROOT}/include/pbrt_gpu.h"\nint abi_version(void) {{ return PG_ABI_VERSION; }}\n')
    so = tmp_path / "v.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    assert C.CDLL(str(so)).abi_version() == 30 == pkg.abi.PG_ABI_VERSION


def test_the_three_entry_points_exist(pkg):
    lib = pkg.gpu_lib()
    for name, nargs in ENTRY_POINTS.items():
        assert name in pkg.abi.GPU_SYMBOLS, name
        res, args = pkg.abi.GPU_SYMBOLS[name]
        assert res is C.c_int and len(args) == nargs and args[-2:] == [C.c_int, C.c_void_p]  # ..., mem, stream
        assert getattr(lib, name) is not None
    for method in ("transmittance_at", "intersect_tr_at", "medium_sample_at"):
        assert callable(getattr(pkg.GpuScene, method)) and callable(getattr(pkg.GpuScene, method + "_device"))


# the arguments after (scene, n) and before (mem, stream); `optional`: the pointers that may be NULL; n_u's position
def _cases(p):
    return {"pg_transmittance_at": ([p, p, p, p, p, p, p, 4, p], (3,), 7),   # o, d, tmax, time, p1, medium, u, n_u, out
            "pg_intersect_tr_at": ([p, p, p, p, p, p, 4, p, p], (3, 8), 6),  # o, d, tmax, time, medium, u, n_u, out, isect
            "pg_medium_sample_at": ([p, p, p, p, p, p, 4, p], (3,), 6)}      # o, d, tmax, time, medium, u, n_u, out


def test_refused_arguments_answer_without_a_device(pkg):
    """The argument checks come before anything touches a device: they answer on a machine without one, with the entry point's name."""
    lib = pkg.gpu_lib()
    a = np.zeros(64, np.float32)
    p = a.ctypes.data
    scene = C.c_void_p(8)  # (never dereferenced: every call below is refused first)
    H, D = pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE
    for name, (args, optional, nu_at) in _cases(p).items():
        fn = getattr(lib, name)
        tag = name.encode() + b":"
        nothing = [None] * len(args)
        nothing[nu_at] = 0
        assert fn(None, 1, *nothing, H, None) == -1 and tag in lib.pg_last_error()
        assert fn(None, 1, *args, H, None) == -1 and tag in lib.pg_last_error()  # no scene
        for k in range(len(args)):
            if k in optional or k == nu_at: continue
            bad = list(args)
            bad[k] = None  # (u among them: n_u = 4 without a stream)
            for mem in (H, D):
                assert fn(scene, 1, *bad, mem, None) == -1 and tag in lib.pg_last_error() and b"null argument" in lib.pg_last_error(), (name, k)
        assert fn(scene, -1, *args, H, None) == -1 and tag in lib.pg_last_error()
        bad = list(args)
        bad[nu_at] = -1
        assert fn(scene, 1, *bad, H, None) == -1 and tag in lib.pg_last_error() and b"n_u" in lib.pg_last_error()
    assert not a.any()


def test_an_empty_batch_returns_ok_and_touches_nothing(pkg):
    lib = pkg.gpu_lib()
    scene = C.c_void_p(8)  # (never dereferenced: n == 0 returns before anything is read)
    for name, (args, _, nu_at) in _cases(None).items():
        nothing = [None] * len(args)
        nothing[nu_at] = 0
        for mem in (pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE):
            assert getattr(lib, name)(scene, 0, *nothing, mem, None) == 0, name
