"""The realistic camera's checks of a render description and the lens header WITHOUT a GPU: tests/realistic_check_host.hip is compiled for
the host, linked with libpbrt_host.so and run directly over the fixtures of tests/golden/realistic -- plain, and under ASan / UBSan.  Every
fixture's description must be accepted, one hostile edit per new check refused with its message, a few thousand lens traces per lens stay
inside their tables, and the two trace directions agree with each other through the multi-element lens."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import GOLD, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SCENES = sorted(glob.glob(os.path.join(GOLD, "realistic", "*.pbrt")))
HOSTILE = 12 * len(SCENES)  # eleven edits on every fixture's description, and the description as an ABI 29 caller would own it


def run_program(pkg, tmp_path, extra):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    pkg.host_lib()
    libdir = os.path.join(ROOT, "pbrt-v3_amd")
    exe = str(tmp_path / "realistic_check_host")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O1", "-g", "-ffp-contract=off", *extra, "-I" + os.path.join(libdir, "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "realistic_check_host.hip"), "-o", exe, "-L" + libdir, "-lpbrt_host", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe] + SCENES, capture_output=True, text=True, timeout=1200)
    print(r.stdout[-3000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert len(SCENES) >= 11
    assert "realistic_check_host: %d scenes, %d hostile descriptions, %d rays traced" % (len(SCENES), HOSTILE, 4096 * len(SCENES)) in r.stdout
    assert ", 0 failures" in r.stdout and " 0 round trips" not in r.stdout and " 0 through" not in r.stdout
    return r


def test_lens_descriptions_are_checked_and_lenses_traced_on_the_host(pkg, tmp_path):
    run_program(pkg, tmp_path, [])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU only")
def test_lens_checks_and_traces_are_clean_under_asan_and_ubsan(pkg, tmp_path):
    r = run_program(pkg, tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
