"""pbrt_host_camera_we_desc (HostScene.camera_we_desc): the PgCameraWeDesc of a perspective camera against a float32 NumPy restatement, bit for bit.

camera_to_raster is the inverse Transform::operator* stores for RasterToCamera = Inverse(CameraToScreen) * RasterToScreen (camera.h:92-105): the product
ScreenToRaster.m * CameraToScreen.m with Matrix4x4::Mul's association, never a numeric inversion of raster_to_camera.  image_area is A of
perspective.cpp:60-66.  world_to_camera[_end] are the CTMs themselves: the start one is what LookAt leaves (transform.cpp:203-238, restated with its
Gauss-Jordan inverse), the end one is the start one times the matrices of the scene file's end-time
transforms (api.cpp's pbrtTranslate / pbrtRotate / pbrtScale post-multiply the CTM), again products, not inversions.  Runs without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLD

F32 = np.float32
PI = F32(3.14159265358979323846)
LIBM = C.CDLL("libm.so.6")
for _f in ("sinf", "cosf", "tanf"):
    getattr(LIBM, _f).restype, getattr(LIBM, _f).argtypes = C.c_float, [C.c_float]
EYE = F32([278, 273, -800])  # every fixture below starts from LookAt 278 273 -800  278 273 0  0 1 0
STILL = ["cornell_32", "cornell_lens", "cornell_40x24", "cornell_crop"]  # (40 x 24: a film that is not square; crop: a crop window)
MOVING = ["camanim_translate", "camanim_rotate", "camanim_times_scale"]


def mul(a, b):  # Matrix4x4::Mul, transform.h:86-93: ((a0 b0 + a1 b1) + a2 b2) + a3 b3
    r = np.zeros((4, 4), F32)
    for i in range(4):
        for j in range(4):
            r[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return r


def scale(x, y, z):
    return np.diag(F32([x, y, z, 1]))


def translate(x, y, z):
    m = np.eye(4, dtype=F32)
    m[:3, 3] = F32([x, y, z])
    return m


def radians(deg):  # pbrt.h:324
    return (PI / F32(180)) * F32(deg)


def rotate(theta, axis):  # transform.cpp:179-201
    a = F32(axis)
    a = a * (F32(1) / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))
    s, c = F32(LIBM.sinf(radians(theta))), F32(LIBM.cosf(radians(theta)))
    x, y, z, one = a[0], a[1], a[2], F32(1)
    m = np.eye(4, dtype=F32)
    m[0, :3] = [x * x + (one - x * x) * c, x * y * (one - c) - z * s, x * z * (one - c) + y * s]
    m[1, :3] = [x * y * (one - c) + z * s, y * y + (one - y * y) * c, y * z * (one - c) - x * s]
    m[2, :3] = [x * z * (one - c) - y * s, y * z * (one - c) + x * s, z * z + (one - z * z) * c]
    return m


def inverse(m):  # Inverse(const Matrix4x4 &), transform.cpp:111-168: Gauss-Jordan with full pivoting, the pivot's reciprocal formed in double
    a = np.array(m, F32)
    indxc, indxr, ipiv = [0] * 4, [0] * 4, [0] * 4
    for i in range(4):
        irow = icol = 0
        big = F32(0)
        for j in range(4):
            if ipiv[j] != 1:
                for k in range(4):
                    if ipiv[k] == 0 and np.abs(a[j, k]) >= big: big, irow, icol = np.abs(a[j, k]), j, k
        ipiv[icol] += 1
        if irow != icol: a[[irow, icol]] = a[[icol, irow]]
        indxr[i], indxc[i] = irow, icol
        pivinv = F32(1.0 / np.float64(a[icol, icol]))
        a[icol, icol] = 1
        a[icol] = a[icol] * pivinv
        for j in range(4):
            if j != icol:
                save = a[j, icol]
                a[j, icol] = 0
                a[j] = a[j] - a[icol] * save
    for j in (3, 2, 1, 0):
        if indxr[j] != indxc[j]: a[:, [indxr[j], indxc[j]]] = a[:, [indxc[j], indxr[j]]]
    assert a.dtype == F32
    return a


def normalize(v):  # geometry.h:984-986
    return v * (F32(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def cross(a, b):  # geometry.h:957-963: in double, rounded once
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]).astype(F32)


def look_at_ctm(pos, look, up):
    """The CTM after `LookAt` on an identity CTM (api.cpp: curTransform * LookAt(...)): LookAt (transform.cpp:203-238) builds cameraToWorld and returns
    Transform(Inverse(cameraToWorld), cameraToWorld) -- the world-to-camera matrix is that numeric inverse, made once, and everything later multiplies it."""
    pos, look, up = F32(pos), F32(look), F32(up)
    c2w = np.eye(4, dtype=F32)
    c2w[:3, 3] = pos
    direction = normalize(look - pos)
    right = normalize(cross(normalize(up), direction))
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2] = right, cross(direction, right), direction
    return mul(np.eye(4, dtype=F32), inverse(c2w))


def perspective(fov, n, f):  # transform.cpp:303-311: (Scale(invTanAng, invTanAng, 1) * Transform(persp)).m
    n, f = F32(n), F32(f)
    persp = np.zeros((4, 4), F32)
    persp[0, 0] = persp[1, 1] = persp[3, 2] = 1
    persp[2, 2], persp[2, 3] = f / (f - n), -f * n / (f - n)
    inv_tan = F32(1) / F32(LIBM.tanf(radians(fov) / F32(2)))
    return mul(scale(inv_tan, inv_tan, 1), persp)


def camera_line(name):
    text = open(os.path.join(GOLD, name + ".pbrt")).read()
    fov = float(re.search(r'^Camera "perspective" "float fov" \[ ([0-9.]+) \]', text, re.M).group(1))
    assert "screenwindow" not in text and "frameaspectratio" not in text
    return text, fov


def restated_camera_to_raster(fov, res):
    frame = F32(res[0]) / F32(res[1])  # perspective.cpp:240-256: the default screen window
    if frame > 1: x0, x1, y0, y1 = -frame, frame, F32(-1), F32(1)
    else: x0, x1, y0, y1 = F32(-1), F32(1), F32(-1) / frame, F32(1) / frame
    screen_to_raster = mul(mul(scale(res[0], res[1], 1), scale(F32(1) / (x1 - x0), F32(1) / (y0 - y1), 1)), translate(-x0, -y1, 0))
    return mul(screen_to_raster, perspective(fov, 1e-2, 1000.0))


def point(m, p):  # Transform::operator()(Point3f), transform.h:219-231
    m = m.reshape(4, 4)
    v = [((m[r, 0] * p[0] + m[r, 1] * p[1]) + m[r, 2] * p[2]) + m[r, 3] for r in range(4)]
    return F32(v[:3]) if v[3] == 1 else F32(v[:3]) * (F32(1) / v[3])


def restated_area(rd):  # perspective.cpp:60-66
    r2c = np.array(rd.raster_to_camera[:], F32)
    lo, hi = point(r2c, F32([0, 0, 0])), point(r2c, F32([rd.full_res[0], rd.full_res[1], 0]))
    lo, hi = lo * (F32(1) / lo[2]), hi * (F32(1) / hi[2])
    return np.abs((hi[0] - lo[0]) * (hi[1] - lo[1]))


def same(a, b):
    return np.array_equal(np.asarray(a, F32).reshape(-1).view(np.uint32), np.asarray(b, F32).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("name", STILL + MOVING)
def test_the_description_equals_the_restatement(pkg, name):
    text, fov = camera_line(name)
    host = pkg.HostScene(os.path.join(GOLD, name + ".pbrt"))
    rd, we = host.render_desc(), host.camera_we_desc()
    assert rd.camera_type == 0 and we is not None
    res = (rd.full_res[0], rd.full_res[1])
    assert same(we.camera_to_raster[:], restated_camera_to_raster(fov, res)), name
    area = restated_area(rd)
    assert area.dtype == F32 and area > 0 and same([we.image_area], [area]), name
    # the start of the motion: the CTM the scene file's LookAt leaves, restated; it carries the eye to the origin
    start = np.array(we.world_to_camera[:], F32).reshape(4, 4)
    look = [float(t) for t in re.search(r"^LookAt (.*)$", text, re.M).group(1).split()]
    assert look[:3] == [float(e) for e in EYE] and "Transform" not in text.split("LookAt")[0]  # (nothing before the LookAt touches the CTM)
    assert same(start, look_at_ctm(look[0:3], look[3:6], look[6:9])), (name, start)
    assert np.abs(point(start, EYE)).max() < 1e-2 and same(start[3], [0, 0, 0, 1])
    # the end of the motion: the CTM after the scene file's end-time transforms, each post-multiplied as api.cpp does -- both ends are covered here
    end = start
    if name in MOVING:
        block = text.split("ActiveTransform EndTime")[1].split("ActiveTransform All")[0]
        for line in block.strip().splitlines():
            op, *v = line.split()
            v = [float(t) for t in v]
            end = mul(end, {"Translate": lambda: translate(*v), "Scale": lambda: scale(*v), "Rotate": lambda: rotate(v[0], v[1:])}[op]())
        assert rd.camera_animated and not same(end, start)
    else: assert not rd.camera_animated
    assert same(we.world_to_camera_end[:], end), name
    host.close()


@pytest.mark.parametrize("name", ["camanim_ortho", "camanim_env"])
def test_other_cameras_have_none(pkg, name):
    host = pkg.HostScene(os.path.join(GOLD, name + ".pbrt"))
    assert host.render_desc().camera_type in (1, 2) and host.camera_we_desc() is None
    we = pkg.abi.PgCameraWeDesc()
    we.image_area = 5
    assert pkg.host_lib().pbrt_host_camera_we_desc(host._h, C.byref(we)) == 0 and not bytes(we).strip(b"\0")  # "none" leaves zeros
    host.close()
