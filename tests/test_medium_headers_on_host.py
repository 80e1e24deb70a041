"""homogeneous_sample_weight (pbrt-v3_amd/csrc/pg_medium.h), the rest of HomogeneousMedium::Sample behind homogeneous_sample_distance, run WITHOUT a
GPU: tests/medium_headers_host.hip compiles pg_medium.h for the host (hipcc --cuda-host-only, -ffp-contract=off like the device build, as
tests/test_device_headers_on_host.py compiles the device library) and this file compares it bit for bit with a float32 NumPy restatement of
homogeneous.cpp:51-73 whose expf / logf are glibc's, the reference's own."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F32 = np.float32
MAX_FLOAT = np.finfo(F32).max
LIBM = C.CDLL("libm.so.6")
for _f in ("expf", "logf"):
    getattr(LIBM, _f).restype, getattr(LIBM, _f).argtypes = C.c_float, [C.c_float]


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    so = os.path.join(str(tmp_path_factory.mktemp("mediumhost")), "libmedium_headers_host.so")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "medium_headers_host.hip"), "-o", so])
    lib = C.CDLL(so)
    lib.hostdev_homogeneous_sample.restype = lib.hostdev_homogeneous_weight.restype = None
    lib.hostdev_homogeneous_sample.argtypes = [C.c_void_p, C.c_void_p]
    lib.hostdev_homogeneous_weight.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    return lib


def expf(x):
    return F32(LIBM.expf(float(x)))


def restate_distance(sigma_t, u_channel, u_dist):
    """homogeneous.cpp:51-54: the channel and the distance from the two numbers."""
    channel = min(int(F32(u_channel) * F32(3)), 2)
    return channel, F32(-F32(LIBM.logf(float(F32(1) - F32(u_dist)))) / sigma_t[channel])


def restate_weight(sigma_s, sigma_t, dist, d_len, t_max):
    """homogeneous.cpp:55-73 in float32, every operation in the reference's order: (beta, t, sampled)."""
    with np.errstate(all="ignore"):
        t = min(F32(dist / d_len), t_max)
        sampled = bool(t < t_max)
        tr = np.array([expf(F32(F32(-sigma_t[c]) * min(t, MAX_FLOAT)) * d_len) for c in range(3)], F32)  # Exp(-sigma_t * min(t, MaxFloat) * |d|)
        density = sigma_t * tr if sampled else tr
        pdf = F32(0)
        for c in range(3): pdf = F32(pdf + density[c])
        pdf = F32(pdf * (F32(1) / F32(3)))
        if pdf == 0: pdf = F32(1)
        beta = (tr * sigma_s) / pdf if sampled else tr / pdf
    return beta.astype(F32), F32(t), sampled


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def medium_input(sigma_a, sigma_s, g, u_channel, u_dist, d_len, t_max):
    return np.concatenate([sigma_a, sigma_s, (sigma_a + sigma_s).astype(F32), [g, u_channel, u_dist, d_len, t_max]]).astype(F32)


def test_homogeneous_sample_equals_the_restatement(dev):
    rng = np.random.default_rng(20241)
    sampled_n = left_n = inf_n = 0
    out = np.zeros(7, F32)
    for k in range(4000):
        scale = F32(10.0 ** rng.uniform(-3, 2))
        sigma_a, sigma_s = (rng.random(3) * scale).astype(F32), (rng.random(3) * scale).astype(F32)
        d_len = F32(10.0 ** rng.uniform(-2, 2))
        t_max = F32(np.inf) if k % 4 == 0 else F32(10.0 ** rng.uniform(-3, 3))
        uc, ud = F32(rng.random()), F32(rng.random())
        if k % 50 == 0: uc = np.nextafter(F32(1), F32(0))  # the channel clamp
        if k % 50 == 1: ud = F32(0)                        # dist = 0: t = 0
        inp = medium_input(sigma_a, sigma_s, F32(rng.uniform(-0.9, 0.9)), uc, ud, d_len, t_max)
        sigma_t = inp[6:9]
        dev.hostdev_homogeneous_sample(inp.ctypes.data, out.ctypes.data)
        channel, dist = restate_distance(sigma_t, uc, ud)
        beta, t, sampled = restate_weight(inp[3:6], sigma_t, dist, d_len, t_max)
        assert int(out[5]) == channel and same(out[6], dist), k
        assert same(out[0:3], beta) and same(out[3], t) and bool(out[4]) == sampled, (k, out, beta, t, sampled)
        sampled_n += sampled; left_n += not sampled; inf_n += sampled and np.isinf(t_max)
    assert sampled_n >= 500 and left_n >= 500 and inf_n >= 200, (sampled_n, left_n, inf_n)


def test_the_edges_pdf_zero_and_t_equal_tmax(dev):
    out = np.zeros(5, F32)
    rng = np.random.default_rng(7)
    zero_pdf = at_tmax = 0
    for k in range(400):
        sigma_a, sigma_s = (rng.random(3) + 0.5).astype(F32), (rng.random(3) + 0.5).astype(F32)
        d_len = F32(rng.uniform(0.5, 2))
        t_max = F32(rng.uniform(0.5, 4))
        if k % 2 == 0:  # every channel's Tr underflows to 0: pdf == 0 is replaced by 1 and beta is 0 (homogeneous.cpp:68-71)
            sigma_a = (sigma_a * F32(4000)).astype(F32)
            dist = F32(t_max * d_len * F32(rng.uniform(0.9, 3)))
        else:  # dist / |d| lands on tMax exactly, or an ulp to either side: `t < ray.tMax` decides
            dist = F32(t_max * d_len)
            if k % 3 == 1: dist = np.nextafter(dist, F32(np.inf))
        inp = medium_input(sigma_a, sigma_s, F32(0), F32(0), F32(0), d_len, t_max)
        dev.hostdev_homogeneous_weight(inp.ctypes.data, C.c_float(float(dist)), out.ctypes.data)
        beta, t, sampled = restate_weight(inp[3:6], inp[6:9], dist, d_len, t_max)
        assert same(out[0:3], beta) and same(out[3], t) and bool(out[4]) == sampled, (k, out, beta, t, sampled)
        if k % 2 == 0:
            zero_pdf += int(not beta.any())
        else:
            at_tmax += int(t == t_max and not sampled)
    assert zero_pdf >= 150 and at_tmax >= 50, (zero_pdf, at_tmax)
