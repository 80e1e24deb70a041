"""tests/test_gpu_scatter_importance.py without a GPU: the device translation units compiled for the host under the SIMT emulator of tests/emu (as
tests/test_emulated_camera_queries.py builds them) and the TransportMode tests run unchanged in a child pytest -- k_scatter_importance in its four
instantiations beside k_scatter and k_scatter_diff, on the emulated device, whose "device memory" is the host's.  Nothing is deselected."""
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


def test_scatter_importance_on_the_emulated_device(emulated):
    env = dict(os.environ, PBRT_GPU_LIB=emulated, PBRT_EMULATED_DEVICE="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_scatter_importance.py", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=1800)
    tail = p.stdout[-3000:] + p.stderr[-1500:]
    assert p.returncode == 0, tail
    assert "74 passed" in tail and "failed" not in tail and "skipped" not in tail, tail
