#!/usr/bin/env python3
"""Generates tests/golden/directlighting/: Integrator "directlighting" scenes rendered by the UNMODIFIED reference binary
(oracle/_ref/pbrt_oracle), each with the statistics it printed.  The scenes are tests/golden/cornell_32.pbrt through the helpers of
oracle/make_golden.py; the ceiling light is two triangles, hence two lights.  Every scene is one the device renders: no specular
bounce is traced in any of them (an all-matte scene, non-specular lobe lists, or "maxdepth" 1), and strategy "all" meets the
GlobalSamplers only.

The conditions at the end are on the REFERENCE's own outputs: they say what the fixtures cover, not what a device must reach.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "directlighting")
BASE = open(os.path.join(ROOT, "tests", "golden", "cornell_32.pbrt")).read()
AREA = 'AreaLightSource "diffuse" "rgb L" [ 17 12 4 ]'


def direct(s, integrator="", xres=32, yres=32, spp=4, area=""):
    """The base scene under the directlighting integrator: its parameters, the film's size, the sample count, the area light's."""
    s = s.replace('Integrator "path" "integer maxdepth" [ 5 ]', ('Integrator "directlighting" ' + integrator).rstrip())
    s = s.replace('"integer xresolution" [ 32 ] "integer yresolution" [ 32 ] ', f'"integer xresolution" [ {xres} ] "integer yresolution" [ {yres} ] ')
    s = s.replace('"integer pixelsamples" [ 8 ]', f'"integer pixelsamples" [ {spp} ]')
    s = s.replace("matte surfaces, PathIntegrator, halton, box filter.", "DirectLightingIntegrator; edited per fixture by tools/make_directlighting_goldens.py.")
    assert "PathIntegrator" not in s
    if area:
        s = s.replace(AREA, AREA + " " + area)
    assert 'Integrator "directlighting"' in s and f"[ {xres} ]" in s and (not area or area in s)
    return s


def material(s, old, new, count=0):
    assert old in s, old
    return s.replace(old, new, count) if count else s.replace(old, new)


def scenes():
    white, green, red = 'Material "matte" "rgb Kd" [ 0.73 0.73 0.73 ]', 'Material "matte" "rgb Kd" [ 0.12 0.45 0.15 ]', 'Material "matte" "rgb Kd" [ 0.65 0.05 0.05 ]'
    out = {}
    out["a_defaults"] = direct(BASE)
    out["b_four_samples"] = direct(BASE, area='"integer samples" [ 4 ]')
    out["c_three_samples_sobol"] = direct(BASE, area='"integer samples" [ 3 ]').replace('Sampler "halton"', 'Sampler "sobol"')
    out["d_one_of_18"] = mg.with_many_lights(direct(BASE, '"string strategy" "one"'), n=3)
    # delta lights (no BSDF-sampled term), a constant infinite light (escaped camera rays take its Le: the wide camera sees past the box) and the area light
    e = direct(BASE, '"string strategy" "all"', area='"integer samples" [ 2 ]').replace('"float fov" [ 39.3 ]', '"float fov" [ 60 ]')
    out["e_five_kinds_of_light"] = e.replace("WorldBegin\n", 'WorldBegin\nLightSource "point" "point from" [ 278 400 100 ] "rgb I" [ 40000 30000 20000 ]\n'
                                             'LightSource "spot" "point from" [ 100 500 100 ] "point to" [ 300 0 300 ] "rgb I" [ 60000 60000 90000 ] "float coneangle" [ 35 ]\n'
                                             'LightSource "distant" "point from" [ 0 1 -1 ] "point to" [ 0 0 0 ] "rgb L" [ 0.5 0.4 0.3 ]\n'
                                             'LightSource "infinite" "rgb L" [ 0.3 0.4 0.6 ] "integer samples" [ 2 ]\n', 1)
    out["f_textures"] = mg.with_textures(direct(BASE, '"string strategy" "all"'))
    g = direct(BASE, '"integer maxdepth" [ 5 ]')
    g = material(g, white, 'Material "plastic" "rgb Kd" [ 0.6 0.6 0.6 ] "rgb Ks" [ 0.3 0.3 0.3 ] "float roughness" [ 0.15 ]', 1)
    g = material(g, green, 'Material "substrate" "rgb Kd" [ 0.12 0.45 0.15 ] "rgb Ks" [ 0.3 0.3 0.3 ] "float uroughness" [ 0.1 ] "float vroughness" [ 0.2 ]')
    g = material(g, red, 'Material "translucent" "rgb Kd" [ 0.65 0.05 0.05 ] "rgb Ks" [ 0.2 0.2 0.2 ] "float roughness" [ 0.2 ]')
    g = material(g, "# short box\n" + white, '# short box\nMaterial "metal" "float roughness" [ 0.1 ]')
    g = material(g, "# tall box", 'Material "glass" "float uroughness" [ 0.2 ] "float vroughness" [ 0.3 ] "float index" [ 1.5 ]\n# tall box')
    out["g_nonspecular_lobes"] = g
    h = direct(BASE, '"integer maxdepth" [ 1 ]')
    h = material(h, green, 'Material "uber" "rgb Kd" [ 0.12 0.45 0.15 ] "rgb Ks" [ 0.2 0.2 0.2 ] "rgb Kr" [ 0.4 0.4 0.4 ] "float roughness" [ 0.1 ]')
    h = material(h, "# short box\n" + white, '# short box\nMaterial "mirror" "rgb Kr" [ 0.9 0.9 0.9 ]')
    h = material(h, "# tall box", 'Material "glass" "float index" [ 1.5 ]\n# tall box')
    out["h_specular_depth_1"] = h
    # maxdepth 0: no sample array was requested (directlighting.cpp:53), so the four samples the light asks for become ONE Get2D pair and no division
    out["i_depth_0"] = direct(BASE, '"integer maxdepth" [ 0 ] "string strategy" "all"', area='"integer samples" [ 4 ]')
    out["j_null_boundaries"] = mg.with_smoke(direct(BASE, '"integer maxdepth" [ 1 ]'))
    out["k_gaussian_crop_bounds"] = direct(BASE, '"integer pixelbounds" [ 3 20 2 17 ]', 24, 20).replace('PixelFilter "box"', 'PixelFilter "gaussian" "float xwidth" [ 1.5 ] "float ywidth" [ 1.5 ]') \
        .replace('"string filename"', '"float cropwindow" [ 0.1 0.9 0.05 0.8 ] "string filename"')
    one16 = direct(BASE, '"string strategy" "one"', 16, 16, 4)
    out["l1_one_random"] = mg.with_sampler(one16, '"random" "integer pixelsamples" [ 2 ]')
    out["l2_one_stratified"] = mg.with_sampler(one16, '"stratified" "integer xsamples" [ 2 ] "integer ysamples" [ 2 ]')
    out["l3_one_02sequence"] = mg.with_sampler(one16, '"02sequence" "integer pixelsamples" [ 4 ]')
    out["l4_one_maxmindist"] = mg.with_sampler(one16, '"maxmindist" "integer pixelsamples" [ 2 ]')
    out["m_moving"] = mg.with_moving_boxes(mg.cam_anim(direct(BASE, '"string strategy" "all"', 24, 24), "Rotate 4 0 1 0\nTranslate 25 10 -30"))
    n = direct(BASE, '"string strategy" "one"', 24, 24)
    n = n.replace('Camera "perspective" "float fov" [ 39.3 ]', 'Camera "realistic" "string lensfile" "../realistic/lens_singlet.dat" "float focusdistance" [ 800 ] "float aperturediameter" [ 8 ]')
    out["n_realistic_one"] = n.replace('"string filename"', '"float diagonal" [ 35 ] "string filename"')
    # a sphere as the area light and hits under an object instance: the interaction, Sphere::Sample / Sphere::Pdf and InterpolatedPrimToWorld at k_direct's vertices
    quad = ('  Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ]\n'
            '    "point P" [ 343 548.7 227   343 548.7 332   213 548.7 332   213 548.7 227 ]\n')
    # (o) every shaded point lies outside the sphere: the cone of Sphere::Sample (sphere.cpp:243-290) and of Sphere::Pdf (sphere.cpp:292-305)
    o = material(direct(BASE, '"string strategy" "all"', area='"integer samples" [ 2 ]'), quad, '  Translate 278 440 280\n  Shape "sphere" "float radius" [ 45 ]\n')
    out["o_sphere_light_outside"] = o
    # (p) every shaded point lies inside the sphere (tests/golden/sphere_enclosing.pbrt): Sphere::Pdf falls back to Shape::Pdf, which intersects the sphere (shape.cpp:72-87)
    out["p_sphere_light_enclosing"] = material(direct(BASE, '"string strategy" "one"'), "# light\n", 'AttributeBegin\n  Translate 278 273 100\n  ReverseOrientation\n'
                                               '  AreaLightSource "diffuse" "rgb L" [ 0.5 0.6 0.8 ]\n  Shape "sphere" "float radius" [ 1500 ]\nAttributeEnd\n# light\n')
    # (q) the boxes and a sphere as one object, placed twice under a rotation and a non-uniform scale: the instance-space ray and InterpolatedPrimToWorld (transform.cpp:262-297)
    q = material(direct(BASE), "# short box\n", 'ObjectBegin "boxes"\n# short box\n')
    q = material(q, "WorldEnd\n", 'AttributeBegin\n  Translate 186 225 168\n  Shape "sphere" "float radius" [ 60 ]\nAttributeEnd\nObjectEnd\n'
                 'AttributeBegin\n  Translate 30 0 40\n  Rotate 12 0 1 0\n  Scale 0.5 0.8 0.45\n  ObjectInstance "boxes"\nAttributeEnd\n'
                 'AttributeBegin\n  Translate 290 0 240\n  Rotate -25 0 1 0\n  Scale 0.45 0.6 0.5\n  ObjectInstance "boxes"\nAttributeEnd\nWorldEnd\n')
    out["q_instances"] = q
    for name, text in out.items():
        assert 'Integrator "directlighting"' in text, name
    assert "trianglemesh" not in o.split("# light")[1].split("AttributeEnd")[0] and out["p_sphere_light_enclosing"].count("AreaLightSource") == 2 and q.count("ObjectInstance") == 2
    assert "cropwindow" in out["k_gaussian_crop_bounds"] and 'Camera "realistic"' in out["n_realistic_one"] and "fov\" [ 60 ]" in out["e_five_kinds_of_light"]
    return out


def run(name, scene_path):
    ref = os.path.join(ROOT, "oracle", "_ref", "pbrt_oracle")
    out = os.path.join(OUT, name + ".pfm")
    # one thread where film tiles overlap: the gaussian filter, and maxmindist (its first film sample of a pixel lies on the pixel's edge)
    nthreads = "1" if "gaussian" in name or "maxmindist" in name else "4"
    p = subprocess.run([ref, "--nthreads", nthreads, "--outfile", out, scene_path], capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"{name}: the reference failed\n{p.stdout}\n{p.stderr}")
    stats = mg.parse_stats(p.stdout)
    json.dump(stats, open(os.path.join(OUT, name + ".json"), "w"))
    print(name, stats, flush=True)
    return stats


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        return np.frombuffer(f.read(w * h * 12), "<f4" if scale < 0 else ">f4")


def main():
    os.makedirs(OUT, exist_ok=True)
    all_scenes = scenes()
    if any("imagemap" in t for t in all_scenes.values()):
        mg.write_test_images(OUT)
    only = sys.argv[1:]
    for name, text in all_scenes.items():
        if only and name not in only:
            continue
        path = os.path.join(OUT, name + ".pbrt")
        open(path, "w").write(text)
        run(name, path)
        assert read_pfm(path[:-5] + ".pfm").any(), f"{name}: the image is all zero"
    if not only:
        img = {n: read_pfm(os.path.join(OUT, n + ".pfm")) for n in ("a_defaults", "b_four_samples", "i_depth_0")}
        assert (img["a_defaults"] != img["b_four_samples"]).any(), "four light samples give the image of one"
        # i (four samples asked for, maxdepth 0) must not be b (the four array elements, divided by four).  It IS a, bit for bit: element 0 of a
        # one-element array of pixel sample s is (GetIndexForSample(s), dimensions 5 + 4 j ...), the very numbers the sequential draws return
        assert (img["b_four_samples"] != img["i_depth_0"]).any(), "maxdepth 0 (no sample arrays) gives the image of the four array samples"
        assert (img["a_defaults"] == img["i_depth_0"]).all(), "maxdepth 0 with one sequential sample per light is not the one-element arrays' image"
        # h: Scene::Intersect calls are the camera rays and EstimateDirect's BSDF-sampled rays, which the reference does not print apart.  The
        # all-matte scene (a) -- the same box, lights, camera and sample numbers -- traces no specular bounce whatever the depth, so its excess over the
        # camera rays is BSDF-sampled rays alone; h's mirror, glass and uber surfaces sample no more of them (their specular lobes are not sampled by
        # EstimateDirect), while one specular bounce per mirror / glass hit would add hundreds.  h's excess must not exceed a's
        st = {n: json.load(open(os.path.join(OUT, n + ".json"))) for n in ("a_defaults", "h_specular_depth_1")}
        excess = {n: v["closest_rays"] - v["camera_rays"] for n, v in st.items()}
        assert 0 <= excess["h_specular_depth_1"] <= excess["a_defaults"], excess


if __name__ == "__main__":
    main()
