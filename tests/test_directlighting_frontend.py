"""Integrator "directlighting" in the host front end, without a GPU: the strategy, the lights' sample counts, the refusals raised at
WorldEnd (an Error and no scene, as for everything outside the closed set), and the ABI, to which the integrator added one entry
point and one small description and in which nothing else moved."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import GOLD, ROOT

DIRECT = os.path.join(GOLD, "directlighting")
# sizeof() of the three structures every ABI 30 caller shares with the library, as include/pbrt_gpu.h had them before this integrator
PARENT_SIZES = {"PgRenderDesc": 3152, "PgSceneDesc": 488, "PgCounters": 272}


def text_of(name):
    return open(os.path.join(DIRECT, name + ".pbrt")).read()


def load(pkg, name):
    return pkg.HostScene(os.path.join(DIRECT, name + ".pbrt"))


@pytest.mark.parametrize("name,strategy,samples", [("a_defaults", 0, [1, 1]), ("b_four_samples", 0, [4, 4]), ("d_one_of_18", 1, [1] * 18)])
def test_strategy_and_light_samples_reach_the_description(pkg, name, strategy, samples):
    scene = load(pkg, name)
    dl = scene.direct_desc()
    assert dl is not None and dl.strategy == strategy and dl.n_lights == len(samples) == scene.desc.n_lights
    assert [dl.light_samples[j] for j in range(dl.n_lights)] == samples
    rd = scene.render_desc()
    assert rd.integrator == 0 and rd.max_depth == 5 and rd.abi_version == 30


def test_the_path_integrators_have_no_direct_description(pkg):
    assert pkg.HostScene(os.path.join(GOLD, "cornell_32.pbrt")).direct_desc() is None


def test_maxdepth_pixelbounds_and_quick_render_division(pkg):
    k = load(pkg, "k_gaussian_crop_bounds")
    # "pixelbounds" [ x0 x1 y0 y1 ] = [ 3 20 2 17 ] is Bounds2i{{3, 2}, {20, 17}} (directlighting.cpp:122-123), which lies inside the sample bounds of
    # this film (crop window 0.1 .. 0.9 x 0.05 .. 0.8 of 24 x 20 pixels, widened by the gaussian's radius): the intersection leaves it as it is
    assert list(k.render_desc().pixel_bounds) == [3, 2, 20, 17]
    assert load(pkg, "i_depth_0").render_desc().max_depth == 0
    # lights/diffuse.cpp:143, infinite.cpp:183: --quick divides a light's sample count by four (at least one)
    # (a description's light_samples belong to its scene: the scene is kept while they are read)
    scene = pkg.HostScene(text=text_of("b_four_samples").replace('"integer samples" [ 4 ]', '"integer samples" [ 9 ]'), quick=True)
    quick = scene.direct_desc()
    assert [quick.light_samples[j] for j in range(quick.n_lights)] == [2, 2]
    scene = load(pkg, "e_five_kinds_of_light")  # point, spot, distant: 1; infinite "samples" 2; the area light's two triangles 2
    e = scene.direct_desc()
    assert [e.light_samples[j] for j in range(e.n_lights)] == [1, 1, 1, 2, 2, 2]


def test_an_unknown_strategy_warns_and_means_all(pkg, capfd):
    scene = pkg.HostScene(text=text_of("a_defaults").replace('Integrator "directlighting"', 'Integrator "directlighting" "string strategy" "some"'))
    err = capfd.readouterr().err
    assert 'Strategy "some" for direct lighting unknown. Using "all".' in err
    assert scene.direct_desc().strategy == 0


def refused(pkg, text, capfd, needle):
    before = pkg.host_lib().pbrt_host_error_count()
    with pytest.raises(pkg.PbrtGpuError):
        pkg.HostScene(text=text)
    err = capfd.readouterr().err
    assert pkg.host_lib().pbrt_host_error_count() > before
    assert needle in err and "the scene will not be rendered" in err, err[-2000:]  # (the closing "Scene not rendered" line is printed once per process)


def test_specular_lobes_at_maxdepth_5_are_refused_and_load_at_maxdepth_1(pkg, capfd):
    h = text_of("h_specular_depth_1")
    assert '"integer maxdepth" [ 1 ]' in h
    scene = pkg.HostScene(text=h)
    assert scene.direct_desc().strategy == 0 and scene.render_desc().max_depth == 1
    refused(pkg, h.replace('"integer maxdepth" [ 1 ]', '"integer maxdepth" [ 5 ]'), capfd, "its specular bounces (SpecularReflect / SpecularTransmit) are outside this build's closed set")
    only_mirror = text_of("a_defaults").replace('# short box\nMaterial "matte" "rgb Kd" [ 0.73 0.73 0.73 ]', '# short box\nMaterial "mirror"')
    assert 'Material "mirror"' in only_mirror
    refused(pkg, only_mirror, capfd, 'Integrator "directlighting" with "maxdepth" 5 on a scene whose materials can add specular lobes')
    scene = pkg.HostScene(text=only_mirror.replace('Integrator "directlighting"', 'Integrator "directlighting" "integer maxdepth" [ 1 ]'))
    assert scene.direct_desc() is not None and scene.render_desc().max_depth == 1


def test_strategy_all_under_a_pixel_sampler_is_refused(pkg, capfd):
    l2 = text_of("l2_one_stratified")
    assert 'Sampler "stratified"' in l2 and '"string strategy" "one"' in l2
    scene = load(pkg, "l2_one_stratified")
    assert scene.direct_desc().strategy == 1
    refused(pkg, l2.replace('"string strategy" "one"', '"string strategy" "all"'), capfd, 'Integrator "directlighting" with strategy "all" under sampler "stratified"')


def test_dimensions_beyond_the_samplers_tables_are_refused(pkg, capfd):
    """The ceiling light as a 6 x 6 grid is 72 emissive triangles = 72 lights: at maxdepth 5 their sample arrays occupy
    5 + 4 * 72 * 5 = 1445 dimensions under strategy "all": beyond halton's 1000 and sobol's 1024, where the reference ends its process.  maxdepth 3
    (869) loads under both; strategy "one" draws ten dimensions whatever the light count."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "make_golden.py"))  # (sys.path stays as it is: spawned test processes inherit it)
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    many = mg.with_many_lights(text_of("a_defaults"), n=6)
    refused(pkg, many, capfd, 'Integrator "directlighting": 72 lights at "maxdepth" 5 reach sample dimension 1445, beyond the 1000 of the halton sampler')
    refused(pkg, many.replace('Sampler "halton"', 'Sampler "sobol"'), capfd, "reach sample dimension 1445, beyond the 1024 of the sobol sampler")
    scene = pkg.HostScene(text=many.replace('Integrator "directlighting"', 'Integrator "directlighting" "integer maxdepth" [ 3 ]'))
    assert scene.direct_desc().n_lights == 72 and scene.desc.n_perm_dims >= 5 + 4 * 72
    scene = pkg.HostScene(text=many.replace('Integrator "directlighting"', 'Integrator "directlighting" "string strategy" "one"'))
    assert scene.direct_desc().strategy == 1


def test_the_path_entry_points_refuse_a_directlighting_scene(pkg):
    """render_desc() of such a scene carries integrator 0 (pg_render's texts are pinned), so the binding keeps the scene's integrator with it:
    render(), render_device() and render_sharded() raise instead of path-tracing the frame."""
    scene = load(pkg, "a_defaults")
    rd = scene.render_desc()
    assert rd.direct_lighting and not pkg.HostScene(os.path.join(GOLD, "cornell_32.pbrt")).render_desc().direct_lighting
    for call in (lambda: pkg.GpuScene.render(None, rd), lambda: pkg.GpuScene.render_device(None, rd, 0, 0, 0, 0), lambda: pkg.render_sharded([], rd)):
        with pytest.raises(pkg.PbrtGpuError, match="directlighting"):
            call()


def test_the_closed_set_message_names_the_new_member(pkg, capfd):
    with pytest.raises(pkg.PbrtGpuError):
        pkg.HostScene(text=text_of("a_defaults").replace('Integrator "directlighting"', 'Integrator "whitted"'))
    assert 'Integrator "whitted" is outside this build\'s closed set (path, volpath, directlighting).' in capfd.readouterr().err


def test_abi_grew_by_one_entry_point_and_nothing_moved(pkg, tmp_path):
    names = list(PARENT_SIZES) + ["PgDirectLightingDesc"]
    src = tmp_path / "probe.c"
    body = "\n".join(f"size_t size_{n}(void) {{ return sizeof({n}); }}" for n in names) + "\nint abi_version(void) { return PG_ABI_VERSION; }\n"
    src.write_text(f'#include <stddef.h>\n#include "{ROOT}/include/pbrt_gpu.h"\n{body}')
    so = tmp_path / "probe.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    assert lib.abi_version() == 30 == pkg.abi.PG_ABI_VERSION
    for n in names:
        f = getattr(lib, "size_" + n)
        f.restype = C.c_size_t
        assert f() == C.sizeof(getattr(pkg.abi, n)), n
        if n in PARENT_SIZES:
            assert f() == PARENT_SIZES[n], n
    assert C.sizeof(pkg.abi.PgDirectLightingDesc) == 16
    assert "pg_render_direct" in pkg.abi.GPU_SYMBOLS and "pbrt_host_direct_desc" in pkg.abi.HOST_SYMBOLS


def test_the_cli_refuses_several_gpus(pkg, tmp_path):
    """`pbrt_amd --gpus 2` with this integrator: an Error and no frame, before any device is touched (pg_render_sharded renders the path family only)."""
    exe = os.path.join(ROOT, "pbrt-v3_amd", "pbrt_amd")
    pkg.gpu_lib()  # (libpbrt_gpu.so is built: it raises otherwise)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbrt-v3_amd"), "pbrt_amd"])
    out = tmp_path / "never.pfm"
    r = subprocess.run([exe, "--quiet", "--gpus", "2", "--outfile", str(out), os.path.join(DIRECT, "a_defaults.pbrt")], capture_output=True, text=True)
    assert r.returncode != 0 and not out.exists() and 'Integrator "directlighting" on 2 GPUs is outside this build\'s closed set' in r.stderr, r.stderr[-2000:]
