"""tests/test_gpu_directlighting.py without a GPU: the device translation units compiled for the host under the SIMT emulator of tests/emu (as
tests/test_emulated_device.py builds them) and the DirectLightingIntegrator's device tests run unchanged in a child pytest -- the (light, sample)
steps, the closed-form sample arrays of both GlobalSamplers, the summation order, the re-spawn through surfaces without a material, the
refusals.  The tile-serial samplers' fixtures are left to the GPU, as in the other emulated suites."""
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


def test_direct_lighting_on_the_emulated_device(emulated):
    """Scenes a, b, c, d, f, h, i, j, o, p and q: the reference's image in every bit and its ray counters; then the refusals through the entry point."""
    env = dict(os.environ, PBRT_GPU_LIB=emulated, PBRT_EMULATED_DEVICE="1")
    select = "(bit_for_bit and (a_defaults or b_four or c_three or d_one or f_textures or h_specular or i_depth or j_null or o_sphere or p_sphere or q_instances)) or refused"
    p = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_directlighting.py", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=1800)
    tail = p.stdout[-3000:] + p.stderr[-1500:]
    assert p.returncode == 0, tail
    assert "12 passed" in tail and "failed" not in tail, tail
