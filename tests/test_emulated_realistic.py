"""tests/test_gpu_realistic.py without a GPU: the device translation units compiled for the host under the SIMT emulator of tests/emu (as
tests/test_emulated_device.py builds them) and the realistic camera's device tests run unchanged in a child pytest -- the lens traced per
camera sample in k_generate, weighted film samples, samples of weight 0 that start no path, the lens statistics.  The tile-serial
samplers' fixtures are left to the GPU, as there: hundreds of thousands of tiny launches take the emulator minutes."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("emulated"))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "emu", "build_emulated.py"), out], stdout=subprocess.DEVNULL)
    return os.path.join(out, "libpbrt_gpu_emulated.so")


def run_gpu_tests(lib, files, select, timeout):
    env = dict(os.environ, PBRT_GPU_LIB=lib, PBRT_EMULATED_DEVICE="1")
    p = subprocess.run([sys.executable, "-m", "pytest", *files, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    tail = p.stdout[-3000:] + p.stderr[-1500:]
    assert p.returncode == 0, tail
    return tail


def test_realistic_camera_on_the_emulated_device(emulated):
    """Scenes (a) singlet, (b) weighted + gaussian film, (e) the multi-element lens, (f) sobol + textures (stored differentials), (j) moving
    camera and shapes: the reference's image in every bit, its ray counters, integrator statistics and lens statistics."""
    out = run_gpu_tests(emulated, ["tests/test_gpu_realistic.py"], "bit_for_bit and (a_singlet or b_weighted or e_dgauss or f_sobol or j_moving)", 1800)
    assert "5 passed" in out and "failed" not in out
