#!/usr/bin/env python3
"""Generates tests/golden/realistic/: Camera "realistic" scenes rendered by the UNMODIFIED reference binary (oracle/_ref/pbrt_oracle), with
the statistics it printed -- the keys of the other goldens plus "Camera/Rays vignetted by lens system" (lens_rays_vignetted /
lens_rays_total).  The scenes are tests/golden/cornell_32.pbrt seen through a lens; the lens files are written here (four numbers per
interface, front to rear: curvature radius mm, thickness mm, index of refraction, aperture diameter mm; radius 0 = the aperture stop).

The conditions at the end are on the REFERENCE's own statistics: they say what the fixtures cover, not what a device must reach.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "realistic")
BASE = open(os.path.join(ROOT, "tests", "golden", "cornell_32.pbrt")).read()

# a biconvex singlet of 50 mm focal length (1 / f = (n - 1) (1 / R1 - 1 / R2)) with the aperture stop behind it
LENS_SINGLET = """# singlet, f = 50 mm, stop behind the element
# radius  thickness  index  aperture diameter   (mm)
50     5    1.5   20
-50    2    1     20
0      45   0     10
"""
# a double Gauss of 50 mm focal length: eleven interfaces, the stop in the middle, radii of both signs, cemented pairs and air gaps
LENS_DGAUSS = """# double Gauss, f = 50 mm
29.475   3.76   1.67   25.2
84.83    0.12   1      25.2
19.275   4.025  1.67   23
40.77    3.275  1.699  23
12.75    5.705  1      18
0        4.5    0      17.1
-14.495  1.18   1.603  17
40.77    6.065  1.658  20
-20.385  0.19   1      20
437.065  3.22   1.717  20
-39.73   5.0    1      20
"""


def realistic(s, lens, xres=32, yres=32, spp=4, camera="", film=""):
    s = s.replace('Camera "perspective" "float fov" [ 39.3 ]', f'Camera "realistic" "string lensfile" "{lens}" "float focusdistance" [ 800 ] {camera}'.rstrip())
    s = s.replace('"integer xresolution" [ 32 ] "integer yresolution" [ 32 ] ', f'"integer xresolution" [ {xres} ] "integer yresolution" [ {yres} ] "float diagonal" [ 35 ] {film}')
    s = s.replace('"integer pixelsamples" [ 8 ]', f'"integer pixelsamples" [ {spp} ]')
    assert 'Camera "realistic"' in s and '"float diagonal"' in s
    return s


def scenes():
    S, D = "lens_singlet.dat", "lens_dgauss.dat"
    out = {}
    out["a_singlet"] = realistic(BASE, S, 32, 32, 4)
    out["b_weighted_gaussian"] = realistic(BASE, S, 32, 32, 4, camera='"bool simpleweighting" "false" "float shutteropen" [ 0 ] "float shutterclose" [ 0.5 ] "float aperturediameter" [ 8 ]') \
        .replace('PixelFilter "box"', 'PixelFilter "gaussian" "float xwidth" [ 1.5 ] "float ywidth" [ 1.5 ]')
    out["c_small_aperture"] = realistic(BASE, D, 24, 24, 4, camera='"float aperturediameter" [ 0.5 ]')
    out["d_clamped_aperture"] = realistic(BASE, S, 16, 16, 4, camera='"float aperturediameter" [ 25 ]')
    out["e_dgauss"] = realistic(BASE, D, 32, 32, 4, camera='"float aperturediameter" [ 12 ]')
    out["f_sobol_textured"] = mg.with_textures(realistic(BASE, D, 24, 24, 4, camera='"float aperturediameter" [ 10 ]')) \
        .replace('Sampler "halton" "integer pixelsamples" [ 4 ]', 'Sampler "sobol" "integer pixelsamples" [ 4 ]')
    out["g_random"] = mg.with_sampler(realistic(BASE, S, 16, 16, 2, camera='"float aperturediameter" [ 8 ]'), '"random" "integer pixelsamples" [ 2 ]')
    out["h_stratified"] = mg.with_sampler(realistic(BASE, D, 24, 24, 4, camera='"float aperturediameter" [ 10 ]'),
                                          '"stratified" "integer xsamples" [ 2 ] "integer ysamples" [ 2 ] "integer dimensions" [ 17 ]')
    out["i_volpath_fog"] = mg.with_fog(realistic(BASE, S, 24, 24, 4, camera='"float aperturediameter" [ 8 ]')
                                       .replace('Integrator "path" "integer maxdepth" [ 5 ]', 'Integrator "volpath" "integer maxdepth" [ 5 ]'))
    out["j_moving"] = mg.with_moving_boxes(mg.cam_anim(realistic(BASE, D, 24, 24, 4, camera='"float aperturediameter" [ 10 ]'), "Rotate 4 0 1 0\nTranslate 25 10 -30"))
    out["k_crop"] = realistic(BASE, S, 24, 16, 4, camera='"float aperturediameter" [ 6 ]', film='"float cropwindow" [ 0.25 0.8 0.125 0.9 ] ')
    for name, text in out.items():
        assert "volpath" in text or name != "i_volpath_fog"
        assert 'Sampler "halton"' in text or name[0] in "fgh", name
    return out


def run(name, scene_path):
    ref = os.path.join(ROOT, "oracle", "_ref", "pbrt_oracle")
    out = os.path.join(OUT, name + ".pfm")
    # one thread where FilmTiles overlap (the gaussian filter): they are then merged in tile order (film.cpp:117-130)
    nthreads = "1" if "gaussian" in name else "4"
    p = subprocess.run([ref, "--nthreads", nthreads, "--outfile", out, scene_path], capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"{name}: the reference failed\n{p.stdout}\n{p.stderr}")
    stats = mg.parse_stats(p.stdout)
    m = re.search(r"Rays vignetted by lens system\s+(\d+) /\s+(\d+)", p.stdout)
    if not m:
        sys.exit(f"{name}: the reference printed no lens statistic\n{p.stdout}")
    stats["lens_rays_vignetted"], stats["lens_rays_total"] = int(m.group(1)), int(m.group(2))
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
    open(os.path.join(OUT, "lens_singlet.dat"), "w").write(LENS_SINGLET)
    open(os.path.join(OUT, "lens_dgauss.dat"), "w").write(LENS_DGAUSS)
    if any("i_rgb" in t or "imagemap" in t for t in scenes().values()):
        mg.write_test_images(OUT)
    only = sys.argv[1:]
    fractions = {}
    for name, text in scenes().items():
        path = os.path.join(OUT, name + ".pbrt")
        if only and name not in only:
            if os.path.exists(path[:-5] + ".json"):
                st = json.load(open(path[:-5] + ".json"))
                fractions[name] = st["lens_rays_vignetted"] / st["lens_rays_total"]
            continue
        open(path, "w").write(text)
        st = run(name, path)
        assert 0 < st["lens_rays_vignetted"] < st["lens_rays_total"], (name, st)
        assert read_pfm(path[:-5] + ".pfm").any(), f"{name}: the image is all zero"
        fractions[name] = st["lens_rays_vignetted"] / st["lens_rays_total"]
    print({k: round(v, 3) for k, v in fractions.items()})
    if not only:
        assert max(fractions.values()) > 0.25, "no scene with more than a quarter of its lens rays vignetted"
        assert min(fractions.values()) < 0.10, "no scene with less than a tenth of its lens rays vignetted"


if __name__ == "__main__":
    main()
