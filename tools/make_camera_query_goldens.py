#!/usr/bin/env python3
"""Generates tests/golden/camera_queries/: two Integrator "directlighting" frames rendered by the UNMODIFIED reference binary
(oracle/_ref/pbrt_oracle), by the method of tools/make_directlighting_goldens.py, each with the statistics it printed.  They are the frames
tests/test_gpu_camera_queries.py assembles from query calls: 16 x 16 pixels, one sample per pixel, "maxdepth" 1, strategy "all", ONE point
light (a delta light: EstimateDirect is its first term alone), halton, the box filter -- and surfaces whose BSDF depends on the camera
ray's differentials: a trilinear image map, a closed-form checkerboard and a bump map.  One frame through a perspective thin-lens camera,
one through Camera "realistic" (the singlet of tests/golden/realistic, read from where it lies).

The texture is a small image written here (cq_texture.pfm, 24 x 24: not a power of two, so the MIPMap resamples it).
The conditions at the end are on the REFERENCE's own outputs: they say what the fixtures cover, not what a device must reach.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as mg  # noqa: E402
from make_directlighting_goldens import BASE, direct, material, read_pfm  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "camera_queries")
TEXTURES = ('Texture "cq_img" "spectrum" "imagemap" "string filename" "cq_texture.pfm" "bool trilinear" "true" "float uscale" [ 4 ] "float vscale" [ 3 ]\n'
            'Texture "cq_chk" "spectrum" "checkerboard" "float uscale" [ 9 ] "float vscale" [ 7 ] "rgb tex1" [ 0.8 0.8 0.7 ] "rgb tex2" [ 0.1 0.2 0.5 ]\n'
            'Texture "cq_bump" "float" "imagemap" "string filename" "cq_texture.pfm" "bool trilinear" "true" "float scale" [ 14 ] "float uscale" [ 5 ] "float vscale" [ 5 ]\n')


def write_texture(path):
    y, x = np.mgrid[0:24, 0:24]
    r = 0.5 + 0.45 * np.sin(x * 1.3) * np.cos(y * 0.9)
    g = ((x // 2 + y // 3) % 2) * 0.7 + 0.15
    b = (x * 5 + y * 11) % 24 / 24.0
    img = np.stack([r, g, b], axis=2).astype("<f4")
    open(path, "wb").write(b"PF\n24 24\n-1.0\n" + img[::-1].tobytes())


def scenes():
    white, green, red = 'Material "matte" "rgb Kd" [ 0.73 0.73 0.73 ]', 'Material "matte" "rgb Kd" [ 0.12 0.45 0.15 ]', 'Material "matte" "rgb Kd" [ 0.65 0.05 0.05 ]'
    s = direct(BASE, '"integer maxdepth" [ 1 ] "string strategy" "all"', 16, 16, 1)
    s = material(s, 'AreaLightSource "diffuse" "rgb L" [ 17 12 4 ]', "# (the former emitter: a matte quad)")
    s = material(s, "WorldBegin\n", 'WorldBegin\nLightSource "point" "point from" [ 278 400 100 ] "rgb I" [ 60000 50000 40000 ]\n' + TEXTURES, 1)
    s = material(s, white, 'Material "matte" "texture Kd" "cq_img"', 1)  # floor, ceiling, back wall
    s = material(s, green, 'Material "matte" "texture Kd" "cq_chk"')
    s = material(s, red, 'Material "plastic" "rgb Kd" [ 0.65 0.05 0.05 ] "rgb Ks" [ 0.2 0.2 0.2 ] "float roughness" [ 0.2 ] "texture bumpmap" "cq_bump"')
    assert "AreaLightSource" not in s and s.count("LightSource") == 1
    out = {"thinlens": s.replace('Camera "perspective" "float fov" [ 39.3 ]', 'Camera "perspective" "float fov" [ 39.3 ] "float lensradius" [ 6 ] "float focaldistance" [ 1000 ]')}
    r = s.replace('Camera "perspective" "float fov" [ 39.3 ]', 'Camera "realistic" "string lensfile" "../realistic/lens_singlet.dat" "float focusdistance" [ 800 ] "float aperturediameter" [ 8 ]')
    out["realistic"] = material(r, '"string filename" "cornell.pfm"', '"float diagonal" [ 35 ] "string filename" "cornell.pfm"')  # (the Film's, not the textures')
    assert "lensradius" in out["thinlens"] and 'Camera "realistic"' in out["realistic"] and out["realistic"].count('"float diagonal"') == 1
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    write_texture(os.path.join(OUT, "cq_texture.pfm"))
    ref = os.path.join(ROOT, "oracle", "_ref", "pbrt_oracle")
    for name, text in scenes().items():
        path = os.path.join(OUT, name + ".pbrt")
        open(path, "w").write(text)
        p = subprocess.run([ref, "--nthreads", "4", "--outfile", path[:-5] + ".pfm", path], capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(f"{name}: the reference failed\n{p.stdout}\n{p.stderr}")
        stats = mg.parse_stats(p.stdout)
        json.dump(stats, open(path[:-5] + ".json", "w"))
        print(name, stats, flush=True)
        assert read_pfm(path[:-5] + ".pfm").any(), f"{name}: the image is all zero"
    a, b = (read_pfm(os.path.join(OUT, n + ".pfm")) for n in ("thinlens", "realistic"))
    assert (a != b).any(), "both cameras give one image"


if __name__ == "__main__":
    main()
