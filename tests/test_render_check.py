"""pg_check_render_desc and the pure decisions of a frame (pbrt-v3_amd/csrc/pg_render_check.h) -- what pg_render does with the caller's
PgRenderDesc before it touches the device -- WITHOUT a GPU: tests/render_check_host.hip is compiled for the host, linked with
libpbrt_host.so and run over golden scenes of every sampler and filter kind.  Each render description must be accepted; one hostile
edit per check (among them the eight that test_gpu_parity.py's test_unsupported_inputs_fail_loudly and
test_invalid_media_and_sampler_descriptions_fail_loudly make on the device) must be refused with the same status and message; the batch
shape and the bounce limits must be what pg_render has always computed.  The second test runs the same program under ASan / UBSan."""
import os
import shutil
import subprocess

import pytest

from conftest import GOLD, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SCENES = ["cornell_32", "vol_smoke", "sobol_cornell", "sampler_stratified_dims", "sampler_maxmindist", "filter_gaussian"]
HOSTILE = 17    # descriptions render_check_host.hip edits and expects to be refused (7 on cornell_32, 3 on vol_smoke, 4 on sobol_cornell, 1 on each other scene)
DECISIONS = 22  # 16 batch shapes (2 frames x 4 budgets x 2 filter kinds), 6 bounce limits


def run_program(pkg, tmp_path, extra):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    pkg.host_lib()  # (libpbrt_host.so is built)
    libdir = os.path.join(ROOT, "pbrt-v3_amd")
    exe = str(tmp_path / "render_check_host")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O1", "-g", "-ffp-contract=off", *extra, "-I" + os.path.join(libdir, "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "render_check_host.hip"), "-o", exe, "-L" + libdir, "-lpbrt_host", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe] + [os.path.join(GOLD, s + ".pbrt") for s in SCENES], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "render_check_host: %d scenes, %d hostile descriptions, %d decisions, 0 failures" % (len(SCENES), HOSTILE, DECISIONS) in r.stdout
    return r


def test_render_descriptions_are_checked_and_frames_shaped_on_the_host(pkg, tmp_path):
    run_program(pkg, tmp_path, [])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU only")
def test_render_checks_are_clean_under_asan_and_ubsan(pkg, tmp_path):
    r = run_program(pkg, tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
