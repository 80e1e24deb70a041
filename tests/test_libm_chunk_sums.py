"""tests/golden/libm_chunk_sums.npz -- the 2^32-argument sweeps of csrc/pg_libm.h (tests/test_libm_restated.py) folded into 1024 sums per
function, the form in which tests/test_gpu_device_arithmetic.py compares the DEVICE build of the header with its host build without
needing the GPU box's host libm or its CPU time.  A chunk is 2^22 consecutive argument bit patterns (atan2f: indices of the pairs
pin_atan2f(seed = 1) draws), numbered by the top 10 bits -- a sign, an exponent, a mantissa half; its sum is the sum modulo 2^64 of a
64-bit hash of (argument, result), any NaN counted as 0x7fc00000, signed zeros kept (tests/libm_chunk.h).

This file recomputes a fixed subset of the chunks from the host build of the header and compares it with the fixture: what notices a
stale fixture after an edit to pg_libm.h.  It is also the fixture's generator:

    python tests/test_libm_chunk_sums.py --write    every chunk from pg_libm.h AND from the system's libm; writes only if the two agree
    python tests/test_libm_chunk_sums.py --check    every chunk of both against the committed file
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from test_libm_restated import NAMES as UNARY, has_fma

NAMES = UNARY + ["atan2f"]
NUM_CHUNKS = 1024
FIXTURE = os.path.join(ROOT, "tests", "golden", "libm_chunk_sums.npz")


def build_pin(directory):
    so = os.path.join(str(directory), "libm_pin.so")
    # as tests/test_libm_restated.py: nothing but the header's explicit fma calls is fused, and those compile to the instruction
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fopenmp", "-fPIC", "-shared", os.path.join(ROOT, "tests", "libm_pin.cpp"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.pin_chunk_sums.restype = None
    lib.pin_chunk_sums.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.pin_raw.restype = None
    lib.pin_raw.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def chunk_sums(lib, fn, chunks, system=False):
    chunks = np.ascontiguousarray(chunks, np.uint32)
    out = np.zeros(len(chunks), np.uint64)
    lib.pin_chunk_sums(fn, int(system), chunks.ctypes.data, len(chunks), out.ctypes.data)
    return out


def raw_results(lib, fn, first, count, special=False, system=False):
    """The result bits at the indices first .. first + count - 1: (count,) uint32, for sincosf (count, 2)."""
    a, b = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
    lib.pin_raw(fn, int(system), int(special), first, count, a.ctypes.data, b.ctypes.data)
    return np.stack([a, b], axis=1) if NAMES[fn] == "sincosf" else a


def chunks_to_recompute():
    """Every 16th chunk and the chunks around the values at which the functions change path: +-0 and the subnormals, 1, pi / 4, 120, 88, 2^25,
    inf, the NaNs -- of each the chunk that holds it and the one that holds its predecessor (the value may open its chunk)."""
    chunks = set(range(0, NUM_CHUNKS, 16))
    marks = [0.0, 1.1754942e-38, 1.17549435e-38, 1.0, np.pi / 4, 120.0, 88.0, 2.0 ** 25, np.inf]
    for v in marks:
        u = int(np.float32(v).view(np.uint32))
        for bits in (u, max(u - 1, 0)):
            chunks.add(bits >> 22)
            chunks.add((bits | 0x80000000) >> 22)
    for nan in (0x7f800001, 0x7fbfffff, 0x7fc00000, 0x7fffffff):
        chunks.add(nan >> 22)
        chunks.add((nan | 0x80000000) >> 22)
    return sorted(chunks)


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return build_pin(tmp_path_factory.mktemp("libm_chunks"))


def test_fixture_is_complete():
    z = np.load(FIXTURE)
    assert sorted(z.files) == sorted(NAMES)
    for name in NAMES:
        assert z[name].dtype == np.uint64 and z[name].shape == (NUM_CHUNKS,)
        assert len(np.unique(z[name])) == NUM_CHUNKS, name  # the argument is hashed with the result: no two chunks can share a sum
    assert os.path.getsize(FIXTURE) < 80 * 1024


@pytest.mark.skipif(not has_fma(), reason="the -mfma host build of pg_libm.h needs a CPU with FMA3, as in tests/test_libm_restated.py")
@pytest.mark.parametrize("fn", range(len(NAMES)), ids=NAMES)
def test_fixture_equals_the_host_build_of_the_header(pin, fn):
    want = np.load(FIXTURE)[NAMES[fn]]
    chunks = chunks_to_recompute()
    assert len(chunks) >= 64 + 20
    got = chunk_sums(pin, fn, chunks)
    bad = [c for c, g in zip(chunks, got) if g != want[c]]
    assert not bad, f"{NAMES[fn]}: chunks {bad[:8]} (arguments {bad[0] << 22:#010x} ...) of pg_libm.h no longer hash to tests/golden/libm_chunk_sums.npz: regenerate it (--write)"


def main(argv):
    if len(argv) != 2 or argv[1] not in ("--write", "--check"):
        sys.exit(__doc__)
    if not has_fma():
        sys.exit("this CPU has no FMA3: glibc selects its non-FMA variants here, which pg_libm.h does not restate -- nothing written or checked")
    import time
    every = np.arange(NUM_CHUNKS, dtype=np.uint32)
    sums = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_pin(tmp)
        for fn, name in enumerate(NAMES):
            t0 = time.time()
            sums[name] = chunk_sums(lib, fn, every)
            system = chunk_sums(lib, fn, every, system=True)
            differing = np.nonzero(sums[name] != system)[0]
            print(f"{name}: 1024 chunks of pg_libm.h and of the system's libm in {time.time() - t0:.1f} s, {len(differing)} differ")
            if len(differing):
                sys.exit(f"{name}: the system's libm differs from pg_libm.h in chunks {differing[:8].tolist()}: not the libm the header restates (tests/test_libm_restated.py)")
    if argv[1] == "--write":
        np.savez(FIXTURE, **sums)
        print("wrote", os.path.relpath(FIXTURE, ROOT))
    else:
        z = np.load(FIXTURE)
        stale = {name: int((z[name] != sums[name]).sum()) for name in NAMES}
        if any(stale.values()):
            sys.exit(f"stale chunks per function: {stale}")
        print(f"all {len(NAMES)} x {NUM_CHUNKS} sums equal {os.path.relpath(FIXTURE, ROOT)}, from pg_libm.h and from the system's libm")


if __name__ == "__main__":
    main(sys.argv)
