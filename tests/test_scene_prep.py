"""pg_prepare_scene (pbrt-v3_amd/csrc/pg_scene_prep.h) -- the checks and the host-side layout pg_scene_create runs before it touches the
device -- WITHOUT a GPU: tests/scene_prep_host.hip is compiled for the host, linked with libpbrt_host.so and run over golden scenes of every
feature the description has tables for.  Each must be accepted and laid out consistently, and the hostile edits the GPU tests make
(test_gpu_parity.py: test_unsupported_inputs_fail_loudly, test_malformed_or_too_deep_bvh_is_refused,
test_transformed_primitives_inside_object_definitions_are_validated, test_invalid_media_and_sampler_descriptions_fail_loudly), plus one for
every other stage, must be refused with the same status and message.  The second test runs the same program under ASan / UBSan: this is
the code that indexes memory owned by the caller."""
import os
import shutil
import subprocess

import pytest

from conftest import GOLD, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SCENES = ["cornell_32", "nest_motion", "instance_boxes", "quadrics", "alpha_masks", "tex_image", "tex_materials", "divergent_small", "vol_smoke",
          "grid_puff_sobol", "grid_sss_sobol", "sobol_cornell", "sampler_maxmindist", "many_lights", "cornell_spot_power", "env_map", "light_projection"]
HOSTILE = 18  # descriptions scene_prep_host.hip edits and expects to be refused (9 on cornell_32, 3 on nest_motion, 6 on one scene each)


def run_program(pkg, tmp_path, extra):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    pkg.host_lib()  # (libpbrt_host.so is built)
    libdir = os.path.join(ROOT, "pbrt-v3_amd")
    exe = str(tmp_path / "scene_prep_host")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O1", "-g", "-ffp-contract=off", *extra, "-I" + os.path.join(libdir, "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "scene_prep_host.hip"), "-o", exe, "-L" + libdir, "-lpbrt_host", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe] + [os.path.join(GOLD, s + ".pbrt") for s in SCENES], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "scene_prep_host: %d scenes, %d hostile descriptions, 0 failures" % (len(SCENES), HOSTILE) in r.stdout
    return r


def test_scenes_are_prepared_and_hostile_descriptions_refused_on_the_host(pkg, tmp_path):
    run_program(pkg, tmp_path, [])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="sanitizer builds run on machines without a GPU only")
def test_scene_preparation_is_clean_under_asan_and_ubsan(pkg, tmp_path):
    r = run_program(pkg, tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
