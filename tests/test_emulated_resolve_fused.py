"""tests/test_gpu_resolve_fused.py's first scene without a GPU: the device translation units compiled for the host under the SIMT emulator of tests/emu (as
tests/test_emulated_device.py builds them) and the matte Cornell box rendered both ways in a child pytest -- the direct lighting joined in the next
vertex's shading launch with k_resolve_list over the listed vertices, and the full-queue k_resolve launch of PG_RESOLVE=pass: equal films, equal counters."""
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


def test_matte_cornell_box_both_ways_on_the_emulated_device(emulated):
    env = dict(os.environ, PBRT_GPU_LIB=emulated, PBRT_EMULATED_DEVICE="1")
    env.pop("PG_RESOLVE", None)
    p = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_resolve_fused.py", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", "test_matte_cornell_box"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1800)
    tail = p.stdout[-3000:] + p.stderr[-1500:]
    assert p.returncode == 0, tail
    assert "1 passed" in tail and "failed" not in tail, tail
