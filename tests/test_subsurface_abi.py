"""PgSubsurfaceSample, the record of pg_subsurface_sample_at, and the three subsurface entry points (pg_subsurface_sample_at / pg_subsurface_f_at /
pg_subsurface_sample_f_at): the C header, the ctypes mirror and the NumPy dtype agree field for field, the ABI version and the earlier records did not move, the
symbols are exported and bound, and refused arguments answer before a device is touched.  No compute is launched here (runs without a GPU)."""
import ctypes as C
import subprocess

import numpy as np

from conftest import ROOT

FIELDS = ["status", "prim", "bssrdf", "n_found", "S", "pdf", "eta", "medium_inside", "medium_outside", "chain_rays", "reserved"]
SIZES = [4, 4, 4, 4, 12, 4, 4, 4, 4, 4, 16]
FLOATS = {"S", "pdf", "eta", "reserved"}
EARLIER = {"PgInteraction": ("INTERACTION_DTYPE", 128), "PgScatter": ("SCATTER_DTYPE", 64), "PgLightSample": ("LIGHT_SAMPLE_DTYPE", 64),
           "PgTransmittance": ("TRANSMITTANCE_DTYPE", 32), "PgMediumSample": ("MEDIUM_SAMPLE_DTYPE", 64)}
ENTRY_POINTS = {"pg_subsurface_sample_at": 12, "pg_subsurface_f_at": 9, "pg_subsurface_sample_f_at": 9}


def test_record_layout_matches_header(pkg, tmp_path):
    rec = "PgSubsurfaceSample"
    body = f"size_t size_rec(void) {{ return sizeof({rec}); }}\nint abi_version(void) {{ return PG_ABI_VERSION; }}\n"
    body += "\n".join(f"size_t size_{name}(void) {{ return sizeof({name}); }}" for name in EARLIER) + "\n"
    body += "\n".join(f"size_t off_{f}(void) {{ return offsetof({rec}, {f}); }}\nsize_t len_{f}(void) {{ return sizeof((({rec} *)0)->{f}); }}" for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}\n')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.size_rec.restype = C.c_size_t
    dt, ct = pkg.SUBSURFACE_SAMPLE_DTYPE, pkg.abi.PgSubsurfaceSample
    assert lib.size_rec() == 64 == dt.itemsize == C.sizeof(ct)
    assert lib.abi_version() == 30 == pkg.abi.PG_ABI_VERSION  # the version is still 30
    for name, (dtype_name, size) in EARLIER.items():  # every earlier record's size is unchanged
        fn = getattr(lib, "size_" + name)
        fn.restype = C.c_size_t
        assert fn() == size == getattr(pkg, dtype_name).itemsize == C.sizeof(getattr(pkg.abi, name)), name
    assert list(dt.names) == FIELDS == [n for n, _ in ct._fields_]
    at = 0
    for f, want in zip(FIELDS, SIZES):
        off, size = getattr(lib, "off_" + f), getattr(lib, "len_" + f)
        off.restype = size.restype = C.c_size_t
        assert off() == dt.fields[f][1] == getattr(ct, f).offset == at, f  # (no padding: whole float4s)
        assert size() == dt.fields[f][0].itemsize == getattr(ct, f).size == want, f
        assert dt.fields[f][0].base == ("float32" if f in FLOATS else "int32"), f
        at += want
    assert at == 64


def test_the_three_entry_points_exist(pkg):
    lib = pkg.gpu_lib()
    for name, nargs in ENTRY_POINTS.items():
        assert name in pkg.abi.GPU_SYMBOLS, name
        res, args = pkg.abi.GPU_SYMBOLS[name]
        assert res is C.c_int and len(args) == nargs and args[-2:] == [C.c_int, C.c_void_p]  # ..., mem, stream
        assert getattr(lib, name) is not None
    for method in ("subsurface_sample_at", "subsurface_f_at", "subsurface_sample_f_at"):
        assert callable(getattr(pkg.GpuScene, method)) and callable(getattr(pkg.GpuScene, method + "_device"))


# the arguments after (scene, n) and before (mem, stream); `optional`: the pointers that may be NULL; flags' position or None
def _cases(p):
    return {"pg_subsurface_sample_at": ([p, p, p, p, p, p, p, p], (3, 5), None),  # o, d, tmax, time, u, po, pi, out
            "pg_subsurface_f_at": ([p, p, p, 31, p], (), 3),                      # pi, eta, wi, flags, out
            "pg_subsurface_sample_f_at": ([p, p, p, 31, p], (), 3)}               # pi, eta, u, flags, out


def test_refused_arguments_answer_without_a_device(pkg):
    """The argument checks come before anything touches a device: they answer on a machine without one, with the entry point's name."""
    lib = pkg.gpu_lib()
    a = np.zeros(64, np.float32)
    p = a.ctypes.data
    scene = C.c_void_p(8)  # (never dereferenced: every call below is refused first)
    H, D = pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE
    for name, (args, optional, flags_at) in _cases(p).items():
        fn = getattr(lib, name)
        tag = name.encode() + b":"
        assert fn(None, 1, *args, H, None) == -1 and tag in lib.pg_last_error()  # no scene
        for k in range(len(args)):
            if k in optional or k == flags_at: continue
            bad = list(args)
            bad[k] = None  # (NULL pi among them)
            for mem in (H, D):
                assert fn(scene, 1, *bad, mem, None) == -1 and tag in lib.pg_last_error() and b"null argument" in lib.pg_last_error(), (name, k)
        assert fn(scene, -1, *args, H, None) == -1 and tag in lib.pg_last_error()  # negative n
        if flags_at is not None:
            for flags in (-1, 32):
                bad = list(args)
                bad[flags_at] = flags
                assert fn(scene, 1, *bad, H, None) == -1 and tag in lib.pg_last_error() and b"flags" in lib.pg_last_error()
    assert not a.any()


def test_an_empty_batch_returns_ok_and_touches_nothing(pkg):
    lib = pkg.gpu_lib()
    scene = C.c_void_p(8)  # (never dereferenced: n == 0 returns before anything is read)
    for name, (args, _, flags_at) in _cases(None).items():
        for mem in (pkg.PG_MEM_HOST, pkg.PG_MEM_DEVICE):
            assert getattr(lib, name)(scene, 0, *args, mem, None) == 0, name
