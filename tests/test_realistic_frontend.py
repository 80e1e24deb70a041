"""Camera "realistic" in the host front end (host/realistic.cpp), without a GPU: every fixture of tests/golden/realistic becomes a camera_type 3
render description with the file's interfaces, a focused film distance and 64 non-empty exit pupil boxes; Film::GetPhysicalExtent; the
constructor's Warning; the errors that leave no camera, hence no frame; and the ABI 30 layouts."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT

REAL = os.path.join(GOLD, "realistic")
NAMES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(REAL, "*.json")))
_loaded = {}


def lens_file_rows(path):
    """floatfile.cpp: '#' starts a comment, numbers are separated by white space."""
    vals = [float(t) for line in open(path) for t in line.split("#")[0].split()]
    assert len(vals) % 4 == 0
    return np.array(vals, np.float64).reshape(-1, 4)


def loaded(pkg, name):
    if name not in _loaded:
        before = pkg.host_lib().pbrt_host_error_count()
        scene = pkg.HostScene(os.path.join(REAL, name + ".pbrt"))
        _loaded[name] = (scene, pkg.host_lib().pbrt_host_error_count() - before)
    return _loaded[name]


def test_there_are_fixtures():
    assert len(NAMES) >= 11


@pytest.mark.parametrize("name", NAMES)
def test_fixture_loads_as_a_realistic_camera(pkg, name):
    scene, errors = loaded(pkg, name)
    assert errors == 0
    rd = scene.render_desc()
    assert rd.camera_type == 3 and rd.abi_version == 30
    text = open(os.path.join(REAL, name + ".pbrt")).read()
    lens = "lens_dgauss.dat" if "lens_dgauss.dat" in text else "lens_singlet.dat"
    rows = lens_file_rows(os.path.join(REAL, lens))
    assert rd.n_lens_interfaces == len(rows)
    got = np.array([list(r) for r in rd.lens_interfaces[:rd.n_lens_interfaces]], np.float32)
    # mm -> m in float products (realistic.cpp:69-71); the stop's diameter may have been replaced; the last thickness is the focused one
    assert np.array_equal(got[:, 0], np.float32(rows[:, 0]) * np.float32(.001))
    assert np.array_equal(got[:-1, 1], (np.float32(rows[:, 1]) * np.float32(.001))[:-1])
    assert got[-1, 1] != np.float32(rows[-1, 1]) * np.float32(.001) and 0 < got[-1, 1] < 0.2
    assert np.array_equal(got[:, 2], np.float32(rows[:, 2]))
    boxes = np.array([list(b) for b in rd.exit_pupil_bounds], np.float32)
    assert boxes.shape == (64, 4) and (boxes[:, 0] < boxes[:, 2]).all() and (boxes[:, 1] < boxes[:, 3]).all() and np.isfinite(boxes).all()
    assert rd.lens_simple_weighting == (0 if '"bool simpleweighting" "false"' in text else 1)
    assert np.float32(rd.film_diagonal) == np.float32(np.float64(np.float32(35)) * .001)  # film.cpp:49: one double product


@pytest.mark.parametrize("name, res", [("k_crop", (24, 16)), ("d_clamped_aperture", (16, 16))])
def test_film_physical_extent(pkg, name, res):
    """Film::GetPhysicalExtent, film.cpp:88-93, in float32."""
    rd = loaded(pkg, name)[0].render_desc()
    assert (rd.full_res[0], rd.full_res[1]) == res
    f = np.float32
    diagonal = f(np.float64(f(35)) * .001)
    aspect = f(res[1]) / f(res[0])
    x = np.sqrt(diagonal * diagonal / (f(1) + aspect * aspect), dtype=np.float32)
    y = aspect * x
    want = np.array([-x / f(2), -y / f(2), x / f(2), y / f(2)], np.float32)
    assert np.array_equal(np.array(list(rd.film_physical_extent), np.float32).view(np.uint32), want.view(np.uint32))


def scene_text(camera_params):
    text = open(os.path.join(REAL, "d_clamped_aperture.pbrt")).read()
    start = text.index('Camera "realistic"')
    return text[:start] + 'Camera "realistic" ' + camera_params + text[text.index("\n", start):]


def test_an_aperture_above_the_files_is_clamped_with_a_warning(pkg, capfd):
    lens = os.path.join(REAL, "lens_singlet.dat")
    scene = pkg.HostScene(text=scene_text(f'"string lensfile" "{lens}" "float focusdistance" [ 800 ] "float aperturediameter" [ 27.625 ]'))
    err = capfd.readouterr().err
    assert "Specified aperture diameter 27.625000 is greater than maximum possible 10.000000.  Clamping it." in err
    rd = scene.render_desc()
    assert np.float32(rd.lens_interfaces[2][3]) == np.float32(10) * np.float32(.001) / np.float32(2)  # the file's diameter stands


def test_errors_leave_no_frame_and_the_process_goes_on(pkg, tmp_path):
    lens = os.path.join(REAL, "lens_dgauss.dat")
    five = tmp_path / "five.dat"
    five.write_text("50 5 1.5 20\n-50\n")
    cases = [('"float focusdistance" [ 800 ]', "no lens file"),
             (f'"string lensfile" "{tmp_path}/missing.dat"', "unreadable file"),
             (f'"string lensfile" "{five}"', "not a multiple of four"),
             (f'"string lensfile" "{lens}" "float focusdistance" [ 0.1 ]', "focus distance too short for the lens (realistic.cpp:468)")]
    for params, what in cases:
        before = pkg.host_lib().pbrt_host_error_count()
        with pytest.raises(pkg.PbrtGpuError):
            pkg.HostScene(text=scene_text(params))
        assert pkg.host_lib().pbrt_host_error_count() > before, what
    before = pkg.host_lib().pbrt_host_error_count()
    good = pkg.HostScene(os.path.join(GOLD, "cornell_32.pbrt"))
    assert good.render_desc().camera_type == 0 and pkg.host_lib().pbrt_host_error_count() == before


def test_abi_30_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "probe.c"
    fields = ["n_lens_interfaces", "lens_interfaces", "exit_pupil_bounds", "film_physical_extent", "film_diagonal", "lens_simple_weighting"]
    body = "size_t size_rd(void) { return sizeof(PgRenderDesc); }\nsize_t size_cn(void) { return sizeof(PgCounters); }\nint version(void) { return PG_ABI_VERSION; }\n"
    body += "\n".join(f"size_t off_{f}(void) {{ return offsetof(PgRenderDesc, {f}); }}" for f in fields)
    body += "\nsize_t off_lens_rays_total(void) { return offsetof(PgCounters, lens_rays_total); }\nsize_t off_lens_rays_vignetted(void) { return offsetof(PgCounters, lens_rays_vignetted); }\n"
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    for n in ["size_rd", "size_cn"] + ["off_" + f for f in fields] + ["off_lens_rays_total", "off_lens_rays_vignetted"]:
        getattr(lib, n).restype = C.c_size_t
    assert lib.version() == pkg.abi.PG_ABI_VERSION == 30
    assert lib.size_rd() == C.sizeof(pkg.abi.PgRenderDesc) and lib.size_cn() == C.sizeof(pkg.abi.PgCounters)
    for f in fields:
        assert getattr(lib, "off_" + f)() == getattr(pkg.abi.PgRenderDesc, f).offset, f
    assert lib.off_n_lens_interfaces() == pkg.abi.PgRenderDesc.tile_step.offset + 4  # appended: everything before keeps its place
    for f in ("lens_rays_total", "lens_rays_vignetted"):
        assert getattr(lib, "off_" + f)() == getattr(pkg.abi.PgCounters, f).offset, f
