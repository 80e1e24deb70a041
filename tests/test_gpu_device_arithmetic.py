"""The arithmetic of pbrt-v3_amd/csrc/*.h as the MI355X computes it against the host build of the same source, bit for bit.

Every other per-function test runs a HOST compile of these headers (tests/test_libm_restated.py: pg_libm.h against glibc over all 2^32
arguments; tests/test_device_headers_on_host.py: the geometry, sampling, medium, BSSRDF functions against the oracle).  What makes the
images bit-identical to the reference's is that hipcc's gfx950 code returns the same bits as those host builds -- correctly rounded / and
sqrt (a flag, not the hardware), subnormal operands and results, double -> int conversions, 64-bit products, double division, fma.  Here
tests/device_probe.hip (pbrt-v3_amd/libpg_devprobe.so, compiled with the product's GPUFLAGS) runs the functions one lane per input:

  * pg_libm.h over every float argument (atan2f: the 2^32 pairs of tests/test_libm_restated.py), compared through 1024 chunk sums per
    function with tests/golden/libm_chunk_sums.npz, which tests/test_libm_chunk_sums.py ties to the host build and to glibc;
  * the header functions on the inputs of tests/test_device_headers_on_host.py, and pg_motion.h's interpolate_trs, compared word for word
    with tests/device_headers_host.hip's build, at batch sizes around the wave width and at the full count -- the device library of the
    shading kernels among them: every BxDF (pg_bxdf.h), Henyey-Greenstein (pg_medium.h), the Halton sample index (pg_sampler.h) and the
    camera ray (pg_camera.h) -- and the film kernels' AddSample (pg_film.h) and the light-table kernels' ComputeDistribution (pg_lightdistrib.h).

PG_DEVPROBE_LIB names another build of the probe (to see these tests fail on one compiled with other flags)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from conftest import ROOT
import test_device_headers_on_host as H
import test_libm_chunk_sums as S

pytestmark = pytest.mark.gpu
PROBE_LIB = os.environ.get("PG_DEVPROBE_LIB") or os.path.join(ROOT, "pbrt-v3_amd", "libpg_devprobe.so")
F32 = np.float32
P = C.c_void_p


@pytest.fixture(scope="module")
def probe(gpu):
    if not os.path.exists(PROBE_LIB):
        pytest.fail(PROBE_LIB + " is missing: build() makes it (make -C pbrt-v3_amd libpg_devprobe.so)")
    lib = C.CDLL(PROBE_LIB)
    lib.devprobe_error_string.restype = C.c_char_p
    lib.devprobe_error_string.argtypes = [C.c_int]
    sig = {"libm_chunk_sums": [C.c_int, C.c_uint32, C.c_uint32, P], "libm_raw": [C.c_int, C.c_int, C.c_uint32, C.c_uint32, P, P],
           "tri_test": [C.c_int] + [P] * 8, "quadric_test": [C.c_int] + [P] * 6, "offset_ray_origin": [C.c_int] + [P] * 5, "radical_inverse": [C.c_int] + [P] * 3,
           "scrambled_radical_inverse": [C.c_int, P, P, C.c_int, P, P, P], "concentric_sample_disk": [C.c_int] + [P] * 3, "grid_density": [C.c_int] + [P] * 4,
           "grid_tr": [C.c_int] + [P] * 6 + [C.c_int, P, P], "grid_sample": [C.c_int] + [P] * 6 + [C.c_int, P, P, P], "bssrdf_radial": [C.c_int, P, P, C.c_longlong, P, P, P],
           "fresnel_moment1": [C.c_int, P, P], "invert_catmull_rom": [C.c_int, C.c_int] + [P] * 4, "bssrdf_pdf_sp": [C.c_int, P, P, C.c_longlong] + [P] * 5,
           "bssrdf_probe_segment": [C.c_int, P, P, C.c_longlong] + [P] * 7, "interpolate_trs": [C.c_int, C.c_int] + [P] * 6,
           "lobe_f_pdf": [C.c_int] + [P] * 4, "lobe_sample_f": [C.c_int] + [P] * 6, "henyey_greenstein": [C.c_int] + [P] * 7, "halton_index": [C.c_int] + [P] * 5,
           "camera_ray": [C.c_int] + [P] * 6, "adapter_bsdf": [C.c_int] + [P] * 3, "hg_phase": [C.c_int] + [P] * 2, "russian_roulette": [C.c_int] + [P] * 3,
           "film_tile": [C.c_int, P, C.c_int, P, P, P], "film_radiance": [C.c_int, P, C.c_int, P, P, P], "film_filter_weight": [C.c_int] + [P] * 4,
           "voxel": [C.c_int] + [P] * 6, "distribution_finish": [C.c_int, P, C.c_int, P, P, C.c_int, P],
           "resolve_path": [C.c_int] + [P] * 4, "resolve_vol": [C.c_int] + [P] * 3, "direct_fold": [C.c_int] + [P] * 2, "resolve_roundtrip": [C.c_int] + [P] * 4}
    for name, argtypes in sig.items():
        fn = getattr(lib, "devprobe_" + name)
        fn.restype, fn.argtypes = C.c_int, argtypes
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/device_headers_host.hip: the same headers compiled for the host."""
    if not os.path.exists(H.HIPCC):
        pytest.fail("hipcc is needed to build the host side of the comparison")
    return H.build_host_headers(tmp_path_factory.mktemp("hostdev"))


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    """tests/libm_pin.cpp: pg_libm.h compiled for the host."""
    return S.build_pin(tmp_path_factory.mktemp("libm"))


def ptr(a):
    return a.ctypes.data


def run(probe, name, *args):
    """One entry point of the probe; a HIP error ends the session (nothing more is started on a device that reported one)."""
    status = getattr(probe, "devprobe_" + name)(*[ptr(a) if isinstance(a, np.ndarray) else a for a in args])
    if status != 0:
        pytest.exit(f"devprobe_{name}: HIP error {status}: {probe.devprobe_error_string(status).decode()}", returncode=3)


# ---- pg_libm.h ------------------------------------------------------------------------------------------------------------------------

def canonical(bits):
    bits = np.asarray(bits, np.uint32)
    return np.where((bits & 0x7fffffff) > 0x7f800000, np.uint32(0x7fc00000), bits)


def device_raw(probe, fn, first, count, special=False):
    a, b = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
    run(probe, "libm_raw", fn, int(special), first, count, a, b)
    return np.stack([a, b], axis=1) if S.NAMES[fn] == "sincosf" else a


@pytest.mark.parametrize("fn", range(len(S.NAMES)), ids=S.NAMES)
def test_libm_on_the_device_over_every_argument(probe, pin, fn):
    """The gfx950 build of pg_libm.h returns, for every one of the 2^32 arguments (atan2f: pairs), the bits its host build returns -- any NaN
    for any NaN.  On a difference: the first differing argument of the first differing chunk, from the raw results of both builds."""
    name = S.NAMES[fn]
    want = np.load(S.FIXTURE)[name]
    got = np.zeros(S.NUM_CHUNKS, np.uint64)
    t0 = time.time()
    run(probe, "libm_chunk_sums", fn, 0, S.NUM_CHUNKS, got)
    print(f"{name}: 2^32 evaluations on the device in {time.time() - t0:.2f} s")
    bad = np.nonzero(got != want)[0]
    if len(bad):
        first = int(bad[0]) << 22
        dev, ref = canonical(device_raw(probe, fn, first, 1 << 22)), canonical(S.raw_results(pin, fn, first, 1 << 22))
        lanes = np.nonzero((dev != ref).reshape(1 << 22, -1).any(axis=1))[0]
        where = (f"first at index {first + int(lanes[0]):#010x}: device {np.atleast_1d(dev[lanes[0]]).tolist()} host build {np.atleast_1d(ref[lanes[0]]).tolist()} (result bits), "
                 f"{len(lanes)} of the chunk's 2^22" if len(lanes) else "but the raw results of that chunk agree: the sums are formed differently")
        pytest.fail(f"{name}: {len(bad)} of {S.NUM_CHUNKS} chunks differ from the host build, the first chunk {int(bad[0])} (indices from {first:#010x}); {where}")
    if name == "atan2f":
        n = 22 * 22
        dev, ref = canonical(device_raw(probe, fn, 0, n, special=True)), canonical(S.raw_results(pin, fn, 0, n, special=True))
        diff = np.nonzero(dev != ref)[0]
        assert not len(diff), f"atan2f: edge pair {int(diff[0])} (y = edge[{int(diff[0]) // 22}], x = edge[{int(diff[0]) % 22}]): device {int(dev[diff[0]]):#010x} host build {int(ref[diff[0]]):#010x}"


# ---- the header functions: each case returns (N, host outputs with N rows, device(n) -> outputs of the first n inputs) ---------------------------

class HostHeadersAsOracle:
    """The two oracle entry points tests/test_reference_kats.py's reintersect_cases builds its rays with, served by the host build of the
    device headers (which tests/test_device_headers_on_host.py requires to equal the oracle bit for bit): the same rays, no oracle needed."""
    def __init__(self, host): self.host = host
    def lib(self): return self

    def oracle_triangle_intersect(self, p0, p1, p2, o, d, tmax, t, b):
        out = np.zeros(4, F32)
        hit = self.host.hostdev_tri_test(p0, p1, p2, o, d, tmax, out.ctypes.data)
        t._obj.value = out[0]
        b[:] = [float(x) for x in out[1:]]
        return hit

    def oracle_spawn_ray_origin(self, p, perr, n, w, out):
        self.host.hostdev_offset_ray_origin(p, perr, n, w, out)


def rows(a, n):
    return np.ascontiguousarray(a[:n])


def case_tri_test(probe, host, pkg):
    p0, p1, p2, o, d, tm, n_re = H.triangle_inputs(HostHeadersAsOracle(host))
    N = len(tm)
    out, hit = np.zeros((N, 4), F32), np.zeros(N, np.int32)
    for i in range(N):
        hit[i] = host.hostdev_tri_test(ptr(p0[i]), ptr(p1[i]), ptr(p2[i]), ptr(o[i]), ptr(d[i]), tm[i], ptr(out[i]))
    assert n_re == 1440 and not hit[:n_re].any() and N - n_re == 1200 and hit[n_re:].sum() > 1000

    def device(n):
        dout, dhit = np.zeros((n, 4), F32), np.zeros(n, np.int32)
        run(probe, "tri_test", n, *[rows(a, n) for a in (p0, p1, p2, o, d, tm)], dout, dhit)
        return dhit, np.where(dhit[:, None] != 0, dout, 0)  # t and the barycentrics mean something on a hit
    return N, (hit, np.where(hit[:, None] != 0, out, 0)), device


def case_quadric_test(kind):
    def case(probe, host, pkg):
        cases = (H.quadric_inputs(pkg, "full_sphere") + H.quadric_inputs(pkg, "partial_sphere")) if kind == "sphere" else H.quadric_inputs(pkg, kind)
        assert len(cases) >= 16
        N = sum(len(o) for _, o, _ in cases)
        sp = (pkg.abi.PgSphere * N)()
        o, d = np.concatenate([c[1] for c in cases]), np.concatenate([c[2] for c in cases])
        tm = np.full(N, np.inf, F32)
        k = 0
        for scene, os_, _ in cases:
            for _ in range(len(os_)):
                sp[k] = scene.desc.spheres[0]
                k += 1
        want_shape = {"sphere": 0, "cylinder": 1, "disk": 2, "cone": 3, "paraboloid": 4, "hyperboloid": 5}[kind]  # PgQuadricShape
        assert all(sp[i].shape == want_shape for i in range(0, N, 120))
        t, hit = np.zeros(N, F32), np.zeros(N, np.int32)
        for i in range(N):
            hit[i] = host.hostdev_quadric_test(C.addressof(sp[i]), ptr(o[i]), ptr(d[i]), tm[i], ptr(t[i:i + 1]))
        assert hit.sum() >= 50 and (hit == 0).sum() >= 50, (kind, int(hit.sum()), N)

        def device(n):
            dt, dhit = np.zeros(n, F32), np.zeros(n, np.int32)
            run(probe, "quadric_test", n, C.addressof(sp), rows(o, n), rows(d, n), rows(tm, n), dt, dhit)
            return dhit, np.where(dhit != 0, dt, 0)
        return N, (hit, np.where(hit != 0, t, 0)), device
    return case


def case_offset_ray_origin(probe, host, pkg):
    p, perr, nrm, w = H.offset_ray_origin_inputs()
    N = len(p)
    out = np.zeros((N, 3), F32)
    for i in range(N):
        host.hostdev_offset_ray_origin(ptr(p[i]), ptr(perr[i]), ptr(nrm[i]), ptr(w[i]), ptr(out[i]))

    def device(n):
        dout = np.zeros((n, 3), F32)
        run(probe, "offset_ray_origin", n, rows(p, n), rows(perr, n), rows(nrm, n), rows(w, n), dout)
        return (dout,)
    return N, (out,), device


def radical_lanes():
    bases, values = H.radical_inverse_inputs()
    base = np.array([b for b, _ in bases for _ in values], np.uint32)
    a = np.array([v for _ in bases for v in values], np.uint64)
    perms = np.concatenate([p for _, p in bases]).astype(np.uint16)
    starts = np.cumsum([0] + [len(p) for _, p in bases[:-1]])
    offset = np.array([s for s in starts for _ in values], np.uint32)
    return base, a, perms, offset


def case_radical_inverse(probe, host, pkg):
    base, a, _, _ = radical_lanes()
    out = np.array([host.hostdev_radical_inverse(int(b), int(v)) for b, v in zip(base, a)], F32)

    def device(n):
        dout = np.zeros(n, F32)
        run(probe, "radical_inverse", n, rows(base, n), rows(a, n), dout)
        return (dout,)
    return len(a), (out,), device


def case_scrambled_radical_inverse(probe, host, pkg):
    base, a, perms, offset = radical_lanes()
    out = np.array([host.hostdev_scrambled_radical_inverse(int(b), perms.ctypes.data + 2 * int(o), int(v)) for b, o, v in zip(base, offset, a)], F32)

    def device(n):
        dout = np.zeros(n, F32)
        run(probe, "scrambled_radical_inverse", n, rows(base, n), perms, len(perms), rows(offset, n), rows(a, n), dout)
        return (dout,)
    return len(a), (out,), device


def case_concentric_sample_disk(probe, host, pkg):
    """No host test draws inputs for it: 2 000 random squares' points, and the centre, the corners, the axes and the diagonals (where the two
    branches and the division of one offset by the other meet)."""
    rng = np.random.default_rng(71)
    edge = [0.0, 0.25, 0.5, 0.75, float(F32(1) - F32(2.0 ** -24)), 1e-30, 0.5 + 2.0 ** -24, 0.5 - 2.0 ** -25]
    u = np.concatenate([rng.random((2000, 2)), [(x, y) for x in edge for y in edge]]).astype(F32)
    u0, u1 = np.ascontiguousarray(u[:, 0]), np.ascontiguousarray(u[:, 1])
    out = np.zeros((len(u), 2), F32)
    for i in range(len(u)):
        host.hostdev_concentric_sample_disk(u0[i], u1[i], ptr(out[i]))

    def device(n):
        dout = np.zeros((n, 2), F32)
        run(probe, "concentric_sample_disk", n, rows(u0, n), rows(u1, n), dout)
        return (dout,)
    return len(u), (out,), device


def case_grid(which):
    def case(probe, host, pkg):
        per_scene = []
        for name in H.GRID_SCENES:
            scene, g, den, (o, d, tm, draws, p) = H.grid_inputs(pkg, name)
            N, nd = len(o), draws.shape[1]
            used, val, hit = np.zeros(N, np.int32), np.zeros(N, F32), np.zeros(N, np.int32)
            for i in range(N):
                u, t = C.c_int(), C.c_float()
                if which == "grid_density": val[i] = host.hostdev_grid_density(C.addressof(g), ptr(den), ptr(p[i]))
                elif which == "grid_tr": val[i] = host.hostdev_grid_tr(C.addressof(g), ptr(den), ptr(o[i]), ptr(d[i]), tm[i], ptr(draws[i]), nd, C.byref(u))
                else:
                    hit[i] = host.hostdev_grid_sample(C.addressof(g), ptr(den), ptr(o[i]), ptr(d[i]), tm[i], ptr(draws[i]), nd, C.byref(u), C.byref(t))
                    val[i] = t.value
                used[i] = u.value
            if which == "grid_tr": assert (used > 0).sum() > 100 and used.max() < nd
            if which == "grid_sample": assert hit.sum() > 20 and used.max() < nd

            def device(n, g=g, den=den, o=o, d=d, tm=tm, draws=draws, p=p, nd=nd, keep=scene):
                dused, dval, dhit = np.zeros(n, np.int32), np.zeros(n, F32), np.zeros(n, np.int32)
                if which == "grid_density": run(probe, "grid_density", n, C.addressof(g), den, rows(p, n), dval)
                elif which == "grid_tr": run(probe, "grid_tr", n, C.addressof(g), den, rows(o, n), rows(d, n), rows(tm, n), rows(draws, n), nd, dused, dval)
                else: run(probe, "grid_sample", n, C.addressof(g), den, rows(o, n), rows(d, n), rows(tm, n), rows(draws, n), nd, dused, dval, dhit)
                return dused, dval, dhit
            per_scene.append((N, (used, val, hit), device))
        return per_scene
    return case


def case_bssrdf_radial(probe, host, pkg):
    per_material = []
    for material in H.BSSRDF_MATERIALS:
        scene, r, u = H.bssrdf_radial_inputs(pkg, material)
        dsc = scene.desc
        b = dsc.bssrdfs[0]
        out = np.zeros((len(r), 9), F32)
        for i in range(len(r)):
            host.hostdev_bssrdf_radial(C.addressof(b), dsc.bssrdf_tables, r[i], u[i], ptr(out[i]))
        assert not np.isnan(out).all(axis=1).any()

        def device(n, dsc=dsc, b=b, r=r, u=u, keep=scene):
            dout = np.zeros((n, 9), F32)
            run(probe, "bssrdf_radial", n, C.addressof(b), dsc.bssrdf_tables, dsc.n_bssrdf_floats, rows(r, n), rows(u, n), dout)
            return (dout,)
        per_material.append((len(r), (out,), device))
    return per_material


def case_fresnel_moment1(probe, host, pkg):
    eta = np.concatenate([np.array(H.FRESNEL_MOMENT_ETAS, F32), np.random.default_rng(72).uniform(0.3, 3.0, 2000).astype(F32)])
    out = np.array([host.hostdev_fresnel_moment1(e) for e in eta], F32)

    def device(n):
        dout = np.zeros(n, F32)
        run(probe, "fresnel_moment1", n, rows(eta, n), dout)
        return (dout,)
    return len(eta), (out,), device


def case_invert_catmull_rom(probe, host, pkg):
    _, _, (rho, rho_eff, xs) = H.bssrdf_spatial_inputs(pkg)
    out = np.array([host.hostdev_invert_catmull_rom(len(rho), ptr(rho), ptr(rho_eff), x) for x in xs], F32)

    def device(n):
        dout = np.zeros(n, F32)
        run(probe, "invert_catmull_rom", n, len(rho), rho, rho_eff, rows(xs, n), dout)
        return (dout,)
    return len(xs), (out,), device


def case_bssrdf_spatial(which):
    def case(probe, host, pkg):
        scene, (frame, po, pi, nrm, u1, u2x, u2y), _ = H.bssrdf_spatial_inputs(pkg)
        dsc = scene.desc
        b = dsc.bssrdfs[0]
        N = len(po)
        if which == "bssrdf_pdf_sp":
            out = np.array([host.hostdev_bssrdf_pdf_sp(C.addressof(b), dsc.bssrdf_tables, ptr(frame[i]), ptr(po[i]), ptr(pi[i]), ptr(nrm[i])) for i in range(N)], F32)
            assert (out > 0).sum() > 1000

            def device(n, keep=scene):
                dout = np.zeros(n, F32)
                run(probe, "bssrdf_pdf_sp", n, C.addressof(b), dsc.bssrdf_tables, dsc.n_bssrdf_floats, rows(frame, n), rows(po, n), rows(pi, n), rows(nrm, n), dout)
                return (dout,)
            return N, (out,), device
        out, ok = np.zeros((N, 7), F32), np.zeros(N, np.int32)
        for i in range(N):
            ok[i] = host.hostdev_bssrdf_probe_segment(C.addressof(b), dsc.bssrdf_tables, ptr(frame[i]), ptr(po[i]), u1[i], u2x[i], u2y[i], ptr(out[i]))
        assert ok.sum() > 1000
        mask = lambda o, k: np.concatenate([o[:, :1], np.where(k[:, None] != 0, o[:, 1:], 0)], axis=1)  # the remapped u1 always, the segment when there is one

        def device(n, keep=scene):
            dout, dok = np.zeros((n, 7), F32), np.zeros(n, np.int32)
            run(probe, "bssrdf_probe_segment", n, C.addressof(b), dsc.bssrdf_tables, dsc.n_bssrdf_floats, rows(frame, n), rows(po, n), rows(u1, n), rows(u2x, n), rows(u2y, n), dout, dok)
            return dok, mask(dout, dok)
        return N, (ok, mask(out, ok)), device
    return case


def interpolate_trs_inputs(n=2400):
    """Decompositions as PgInstance carries them: T from 1e-4 to 1e4 either sign; R[0] a random rotation and R[1] = R[0] turned by 0.01 .. 179.9
    degrees (alternately log-uniform and uniform) about a random axis (the quaternions' dot product from ~1, the normalized-lerp branch above 0.9995, down to ~1e-3), every 16th pair
    equal; S = a rotation-free stretch with entries from 1e-4 to 1e4 and a shear of a few per cent, every 8th with one tiny pivot (1e-20, now and then the
    subnormal 1e-40 or 0: the Gauss-Jordan inverse then overflows or divides by zero); dt cycling through 0, 1, 0.5 and a random value."""
    rng = np.random.default_rng(73)
    T, R, S, dt = np.zeros((n, 2, 3), F32), np.zeros((n, 2, 4), F32), np.zeros((n, 2, 9), F32), np.zeros(n, F32)
    def quat_mul(a, b):  # (x, y, z, w)
        av, bv = a[:3], b[:3]
        return np.append(a[3] * bv + b[3] * av + np.cross(av, bv), a[3] * b[3] - av @ bv)
    for i in range(n):
        T[i] = rng.choice([-1.0, 1.0], (2, 3)) * 10.0 ** rng.uniform(-4, 4, (2, 3))
        q0 = rng.normal(size=4); q0 /= np.linalg.norm(q0)
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        angle = np.radians((10.0 ** rng.uniform(-2, np.log10(179.9)) if i % 2 else rng.uniform(0, 179.9)) if i % 16 else 0.0)
        q1 = quat_mul(np.append(np.sin(angle / 2) * axis, np.cos(angle / 2)), q0)
        R[i, 0], R[i, 1] = q0, q1
        for e in range(2):
            m = np.diag(10.0 ** rng.uniform(-4, 4, 3)) @ (np.eye(3) + rng.uniform(-0.05, 0.05, (3, 3)))
            if i % 8 == 3:
                k = int(rng.integers(0, 3))
                m[k, :] = 0; m[:, k] = 0
                m[k, k] = {5: 1e-40, 21: 0.0}.get((i // 8) % 32, 1e-20)
            S[i, e] = m.ravel()
        if i % 8 == 3: S[i, 1] = S[i, 0]  # the lerp keeps the pivot tiny
        dt[i] = [0.0, 1.0, 0.5, rng.random()][i % 4]
    return T, R, S, dt


def case_interpolate_trs(inv):
    def case(probe, host, pkg):
        T, R, S, dt = interpolate_trs_inputs()
        N = len(dt)
        assert N >= 2000
        m, mi = np.zeros((N, 16), F32), np.zeros((N, 16), F32)
        for i in range(N):
            host.hostdev_interpolate_trs(inv, ptr(T[i]), ptr(R[i]), ptr(S[i]), dt[i], ptr(m[i]), ptr(mi[i]))
        all_nan = np.isnan(m).all(axis=1) | (np.isnan(mi).all(axis=1) if inv else False)
        assert all_nan.mean() <= 0.01, all_nan.mean()
        dots = np.abs((R[:, 0] * R[:, 1]).sum(axis=1))
        assert (dots > 0.9995).sum() > 100 and (dots < 0.1).sum() > 20 and (dots < 0.9995).sum() > 1000  # both Slerp branches, nearly half a turn

        def device(n):
            dm, dmi = np.zeros((n, 16), F32), np.zeros((n, 16), F32)
            run(probe, "interpolate_trs", n, inv, rows(T, n), rows(R, n), rows(S, n), rows(dt, n), dm, dmi)
            return dm, dmi
        return N, (m, mi), device
    return case


BXDF_KINDS = range(1, 10)  # every PgBxDFType


def lobe_array(pkg, lobes):
    arr = (pkg.abi.PgBxDF * len(lobes))()
    for i, b in enumerate(lobes):
        arr[i] = b
    return arr


def case_lobe_f_pdf(probe, host, pkg):
    per_kind = []
    for kind in BXDF_KINDS:
        lobes, wo, wi, _, _ = H.bxdf_inputs(pkg, kind)
        N = len(lobes)
        assert N == 400
        arr = lobe_array(pkg, lobes)
        out = np.zeros((N, 4), F32)
        for i in range(N):
            host.hostdev_lobe_f_pdf(C.addressof(arr[i]), ptr(wo[i]), ptr(wi[i]), ptr(out[i]))

        def device(n, arr=arr, wo=wo, wi=wi):
            dout = np.zeros((n, 4), F32)
            run(probe, "lobe_f_pdf", n, C.addressof(arr), rows(wo, n), rows(wi, n), dout)
            return (dout,)
        per_kind.append((N, (out,), device))
    return per_kind


def case_lobe_sample_f(probe, host, pkg):
    """f, pdf, wi and the sampled type, with and without wantF (the wrapper's NaN pdf says the two disagree).  A trial whose pdf is 0 in BOTH builds compares
    pdf and type only, as the host test does against the oracle (BSDF::Sample_f does not look at f and wi then): the host rows are reduced where the host's
    pdf is 0, the device rows where both are 0 -- so a pdf that is 0 in one build only still differs in its own word."""
    per_kind = []
    for kind in BXDF_KINDS:
        lobes, wo, _, u0, u1 = H.bxdf_inputs(pkg, kind)
        N = len(lobes)
        assert N == 400
        arr = lobe_array(pkg, lobes)
        out, typ = np.zeros((N, 7), F32), np.zeros(N, np.int32)
        for i in range(N):
            typ[i] = host.hostdev_lobe_sample_f(C.addressof(arr[i]), ptr(wo[i]), u0[i], u1[i], ptr(out[i]))
        host_zero = out[:, 3] == 0
        assert (~host_zero).sum() > 100, (kind, int((~host_zero).sum()))  # compared in full
        pdf_only = lambda o, zero: np.where(zero[:, None] & (np.arange(7) != 3)[None, :], F32(0), o)

        def device(n, arr=arr, wo=wo, u0=u0, u1=u1, host_zero=host_zero):
            dout, dtyp = np.zeros((n, 7), F32), np.zeros(n, np.int32)
            run(probe, "lobe_sample_f", n, C.addressof(arr), rows(wo, n), rows(u0, n), rows(u1, n), dout, dtyp)
            return dtyp, pdf_only(dout, host_zero[:n] & (dout[:, 3] == 0))
        per_kind.append((N, (typ, pdf_only(out, host_zero)), device))
    return per_kind


def case_henyey_greenstein(probe, host, pkg):
    g, wo, u, ct = H.henyey_greenstein_inputs()
    N = len(g)
    assert N == 3000
    p, wi, phase = np.zeros(N, F32), np.zeros((N, 3), F32), np.zeros(N, F32)
    for i in range(N):
        p[i] = host.hostdev_hg_sample_p(g[i], ptr(wo[i]), u[i, 0], u[i, 1], ptr(wi[i]))
        phase[i] = host.hostdev_phase_hg(ct[i], g[i])

    def device(n):
        dp, dwi, dphase = np.zeros(n, F32), np.zeros((n, 3), F32), np.zeros(n, F32)
        run(probe, "henyey_greenstein", n, rows(g, n), rows(wo, n), rows(u, n), rows(ct, n), dp, dwi, dphase)
        return dp, dwi, dphase
    return N, (p, wi, phase), device


def case_adapter_bsdf(probe, host, pkg):
    rows_in, flags = H.adapter_bsdf_inputs()
    N = len(flags)
    assert N == 840
    out = np.zeros((N, 23), F32)
    for i in range(N):
        host.hostdev_adapter_bsdf(ptr(rows_in[i]), int(flags[i]), ptr(out[i]))

    def device(n):
        dout = np.zeros((n, 23), F32)
        run(probe, "adapter_bsdf", n, rows(rows_in, n), rows(flags, n), dout)
        return (dout,)
    return N, (out,), device


def case_hg_phase(probe, host, pkg):
    rows_in = H.hg_phase_inputs()
    N = len(rows_in)
    assert N == 3000
    out = np.zeros((N, 11), F32)
    for i in range(N):
        host.hostdev_hg_phase(ptr(rows_in[i]), ptr(out[i]))

    def device(n):
        dout = np.zeros((n, 11), F32)
        run(probe, "hg_phase", n, rows(rows_in, n), dout)
        return (dout,)
    return N, (out,), device


def case_russian_roulette(probe, host, pkg):
    rows_in, bounces = H.russian_roulette_inputs()
    N = len(bounces)
    assert N == 318
    out = np.zeros((N, 5), F32)
    for i in range(N):
        host.hostdev_russian_roulette(ptr(rows_in[i]), int(bounces[i]), ptr(out[i]))

    def device(n):
        dout = np.zeros((n, 5), F32)
        run(probe, "russian_roulette", n, rows(rows_in, n), rows(bounces, n), dout)
        return (dout,)
    return N, (out,), device


def case_film_tile(probe, host, pkg):
    per_frame = []
    for rd, ntx, local, pfilm in H.film_tile_inputs(pkg):
        N = len(local)
        assert N == 360
        out = np.zeros((N, 19), np.int32)
        for i in range(N):
            host.hostdev_film_tile(C.addressof(rd), ntx, int(local[i]), ptr(pfilm[i]), ptr(out[i]))

        def device(n, rd=rd, ntx=ntx, local=local, pfilm=pfilm):
            dout = np.zeros((n, 19), np.int32)
            run(probe, "film_tile", n, C.addressof(rd), ntx, rows(local, n), rows(pfilm, n), dout)
            return (dout,)
        per_frame.append((N, (out,), device))
    assert len(per_frame) == 8
    return per_frame


def case_film_radiance(probe, host, pkg):
    rds, rows_in, which = H.film_radiance_inputs(pkg)
    N = len(which)
    arr = (pkg.abi.PgRenderDesc * len(rds))(*rds)
    out = np.zeros((N, 6), F32)
    for i in range(N):
        host.hostdev_film_radiance(C.addressof(arr[which[i]]), ptr(rows_in[i]), ptr(out[i]))

    def device(n):
        dout = np.zeros((n, 6), F32)
        run(probe, "film_radiance", n, C.addressof(arr), len(rds), rows(which, n), rows(rows_in, n), dout)
        return (dout,)
    return N, (out,), device


def case_film_filter_weight(probe, host, pkg):
    rd, xy, rows_in = H.film_filter_weight_inputs(pkg)
    N = len(xy)
    out = np.array([host.hostdev_film_filter_weight(C.addressof(rd), int(xy[i, 0]), int(xy[i, 1]), ptr(rows_in[i])) for i in range(N)], F32)

    def device(n):
        dout = np.zeros(n, F32)
        run(probe, "film_filter_weight", n, C.addressof(rd), rows(xy, n), rows(rows_in, n), dout)
        return (dout,)
    return N, (out,), device


def case_voxel(probe, host, pkg):
    per_grid = []
    for nv, lo, hi, v, idx in H.voxel_inputs():
        N = len(v)
        out = np.zeros((N, 11), F32)
        for i in range(N):
            host.hostdev_voxel(ptr(nv), ptr(lo), ptr(hi), int(v[i]), int(idx[i]), ptr(out[i]))

        def device(n, nv=nv, lo=lo, hi=hi, v=v, idx=idx):
            dout = np.zeros((n, 11), F32)
            run(probe, "voxel", n, nv, lo, hi, rows(v, n), rows(idx, n), dout)
            return (dout,)
        per_grid.append((N, (out,), device))
    return per_grid


def case_distribution_finish(probe, host, pkg):
    """Every distribution of the host test in one buffer, a lane each: the output is the buffer, so a batch of n compares the first n tables."""
    contribs = H.distribution_finish_inputs()
    N = len(contribs)
    nl = np.array([len(c) for c in contribs], np.int32)
    size = 2 * nl + 2
    offset = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int32)
    tables = np.zeros(int(size.sum()), F32)
    for c, o in zip(contribs, offset):
        tables[o:o + len(c)] = c
    out = tables.copy()
    for o, k in zip(offset, nl):
        host.hostdev_distribution_finish(ptr(out[o:]), int(k), 128)
    end = np.concatenate([offset[1:], [len(tables)]])
    per_lane = [out[o:e] for o, e in zip(offset, end)]
    want = np.zeros((N, int(size.max())), F32)
    for i, t in enumerate(per_lane):
        want[i, :len(t)] = t

    def device(n):
        dout = np.zeros(len(tables), F32)
        run(probe, "distribution_finish", n, tables, len(tables), rows(offset, n), rows(nl, n), 128, dout)
        got = np.zeros((n, want.shape[1]), F32)
        for i in range(n):
            got[i, :size[i]] = dout[offset[i]:end[i]]
        assert not dout[end[n - 1] if n else 0:].any()  # the lanes beyond n wrote nothing
        return (got,)
    return N, (want,), device


def case_resolve(name, inputs, n_out, n_iout):
    """One of tests/resolve_probe.h's functions over H's rows for it: float rows, int rows when the function takes them, int outputs when it has them."""
    def make(probe, host, pkg):
        made = inputs()
        frows, irows = made if isinstance(made, tuple) else (made, None)
        N = len(frows)
        out, iout = np.zeros((N, n_out), F32), np.zeros((N, n_iout), np.int32)
        for i in range(N):
            args = [ptr(frows[i])] + ([ptr(irows[i])] if irows is not None else []) + [ptr(out[i])] + ([ptr(iout[i])] if n_iout else [])
            getattr(host, "hostdev_" + name)(*args)

        def device(n):
            dout, diout = np.zeros((n, n_out), F32), np.zeros((n, n_iout), np.int32)
            run(probe, name, n, *([rows(frows, n)] + ([rows(irows, n)] if irows is not None else []) + [dout] + ([diout] if n_iout else [])))
            return (dout, diout) if n_iout else (dout,)
        return N, ((out, iout) if n_iout else (out,)), device
    return make


def case_halton_index(probe, host, pkg):
    per_golden = []
    for golden, scene, rd, pixels in H.halton_index_inputs(pkg):
        N = len(pixels)
        assert N == 400
        px, py = np.array([p[0] for p in pixels], np.int32), np.array([p[1] for p in pixels], np.int32)
        k = np.array([p[2] for p in pixels], np.int64)
        out = np.array([host.hostdev_halton_index(C.addressof(rd), int(px[i]), int(py[i]), int(k[i])) for i in range(N)], np.int64)

        def device(n, rd=rd, px=px, py=py, k=k, keep=scene):
            dout = np.zeros(n, np.int64)
            run(probe, "halton_index", n, C.addressof(rd), rows(px, n), rows(py, n), rows(k, n), dout)
            return (dout,)
        per_golden.append((N, (out,), device))
    assert len(per_golden) == 3
    return per_golden


def case_camera_ray(probe, host, pkg):
    per_camera = []
    for golden in H.CAMERA_GOLDENS:
        scene, rd, (fx, fy, lx, ly) = H.camera_ray_inputs(pkg, golden)
        N = len(fx)
        assert N == 2000
        out = np.zeros((N, 7), F32)
        for i in range(N):
            host.hostdev_camera_ray(C.addressof(rd), fx[i], fy[i], lx[i], ly[i], ptr(out[i]))

        def device(n, rd=rd, fx=fx, fy=fy, lx=lx, ly=ly, keep=scene):
            dout = np.zeros((n, 7), F32)
            run(probe, "camera_ray", n, C.addressof(rd), rows(fx, n), rows(fy, n), rows(lx, n), rows(ly, n), dout)
            return (dout,)
        per_camera.append((N, (out,), device))
    assert len(per_camera) == 6
    return per_camera


CASES = {"tri_test": case_tri_test, "offset_ray_origin": case_offset_ray_origin, "radical_inverse": case_radical_inverse,
         "scrambled_radical_inverse": case_scrambled_radical_inverse, "concentric_sample_disk": case_concentric_sample_disk,
         "grid_density": case_grid("grid_density"), "grid_tr": case_grid("grid_tr"), "grid_sample": case_grid("grid_sample"), "bssrdf_radial": case_bssrdf_radial,
         "fresnel_moment1": case_fresnel_moment1, "invert_catmull_rom": case_invert_catmull_rom, "bssrdf_pdf_sp": case_bssrdf_spatial("bssrdf_pdf_sp"),
         "bssrdf_probe_segment": case_bssrdf_spatial("bssrdf_probe_segment"), "interpolate_trs": case_interpolate_trs(0), "interpolate_trs_inverse": case_interpolate_trs(1)}
CASES.update({"lobe_f_pdf": case_lobe_f_pdf, "lobe_sample_f": case_lobe_sample_f, "henyey_greenstein": case_henyey_greenstein, "halton_index": case_halton_index,
              "camera_ray": case_camera_ray, "adapter_bsdf": case_adapter_bsdf, "hg_phase": case_hg_phase, "russian_roulette": case_russian_roulette})
CASES.update({"film_tile": case_film_tile, "film_radiance": case_film_radiance, "film_filter_weight": case_film_filter_weight, "voxel": case_voxel,
              "distribution_finish": case_distribution_finish})
CASES.update({"resolve_path": case_resolve("resolve_path", H.resolve_path_inputs, 22, 1), "resolve_vol": case_resolve("resolve_vol", H.resolve_vol_inputs, 16, 0),
              "direct_fold": case_resolve("direct_fold", H.direct_fold_inputs, 4, 0),
              "resolve_roundtrip": case_resolve("resolve_roundtrip", H.resolve_roundtrip_inputs, 28, 8)})
CASES.update({"quadric_test_" + kind: case_quadric_test(kind) for kind in ("sphere", "cylinder", "disk", "cone", "paraboloid", "hyperboloid")})


def words(a):
    a = np.ascontiguousarray(a)
    return canonical(a.view(np.uint32)) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_functions_on_the_device_equal_their_host_build(probe, host, pkg, name):
    """Every output word of the gfx950 build equals the host build's on the same inputs (NaN equals NaN), for the first 0, 1, 63, 64, 65 inputs and
    for all of them."""
    made = CASES[name](probe, host, pkg)
    for N, want, device in (made if isinstance(made, list) else [made]):
        assert N > 65
        for n in (0, 1, 63, 64, 65, N):
            t0 = time.time()
            got = device(n)
            if n == N: print(f"{name}: {N} lanes on the device in {time.time() - t0:.3f} s")
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                g, w = words(g), words(w[:n])
                assert g.shape == w.shape
                differs = g != w
                diff = np.nonzero(differs.any(axis=tuple(range(1, differs.ndim))) if differs.ndim > 1 else differs)[0]  # (n = 0: nothing to reshape)
                assert not len(diff), f"{name}: output {k} differs in {len(diff)} of {n} lanes, first lane {int(diff[0])}: device {g[diff[0]].tolist()} host build {w[diff[0]].tolist()}"
