// pg_camera.h -- Camera::GenerateRay[Differential] as device functions: point / ray transforms, a sample slot's pixel, the camera
// matrix at a time, camera_ray / camera_differentials for perspective, orthographic and environment cameras, and the realistic
// camera's sample through pg_lens.h with its statistics.
//
// Used by k_generate / k_ts_generate (pg_kernels.hip) and by tex_hit_setup (pg_hit.h), which re-derives the camera ray's differentials.
// camera_ray is pinned on the host (tests/test_device_headers_on_host.py) and on the device (tests/test_gpu_device_arithmetic.py).
#ifndef PG_CAMERA_H
#define PG_CAMERA_H
#include "pg_device.h"
#include "pg_sphere.h"
#include "pg_kernels.h"
#include "pg_motion.h"
#include "pg_lens.h"
#include "pg_queue.h"

// ===========================================================================
// Camera ray generation: one lane per (pixel, sample) slot
// ===========================================================================
PG_DEV V3 xform_point(const float *m, V3 p) {  // transform.h:219-231
    float x = p.x, y = p.y, z = p.z;
    float xp = m[0] * x + m[1] * y + m[2] * z + m[3];
    float yp = m[4] * x + m[5] * y + m[6] * z + m[7];
    float zp = m[8] * x + m[9] * y + m[10] * z + m[11];
    float wp = m[12] * x + m[13] * y + m[14] * z + m[15];
    if (wp == 1) return mk(xp, yp, zp);
    float inv = 1.f / wp;
    return mk(inv * xp, inv * yp, inv * zp);
}
PG_DEV void xform_ray(const float *m, V3 &o, V3 &d, float &tMax) {  // transform.h:249-262,277-300
    float x = o.x, y = o.y, z = o.z;
    float xp = (m[0] * x + m[1] * y) + (m[2] * z + m[3]);
    float yp = (m[4] * x + m[5] * y) + (m[6] * z + m[7]);
    float zp = (m[8] * x + m[9] * y) + (m[10] * z + m[11]);
    float wp = (m[12] * x + m[13] * y) + (m[14] * z + m[15]);
    float xAbsSum = (fabsf(m[0] * x) + fabsf(m[1] * y) + fabsf(m[2] * z) + fabsf(m[3]));
    float yAbsSum = (fabsf(m[4] * x) + fabsf(m[5] * y) + fabsf(m[6] * z) + fabsf(m[7]));
    float zAbsSum = (fabsf(m[8] * x) + fabsf(m[9] * y) + fabsf(m[10] * z) + fabsf(m[11]));
    V3 oError = mk(xAbsSum, yAbsSum, zAbsSum) * pgamma(3);
    V3 on;
    if (wp == 1) on = mk(xp, yp, zp);
    else { float inv = 1.f / wp; on = mk(inv * xp, inv * yp, inv * zp); }
    float dx = d.x, dy = d.y, dz = d.z;
    V3 dn = mk(m[0] * dx + m[1] * dy + m[2] * dz, m[4] * dx + m[5] * dy + m[6] * dz, m[8] * dx + m[9] * dy + m[10] * dz);
    float lengthSquared = lensq(dn);
    if (lengthSquared > 0) {
        float dt = dot(vabs(dn), oError) / lengthSquared;
        on = on + dn * dt;
        tMax -= dt;
    }
    o = on; d = dn;
}

// slot -> (local tile, sample-in-batch, pixel-in-tile); a wave is 64 pixels of one tile for one sample
PG_DEV bool slot_to_pixel(const RenderParams &rp, int slot, int &px, int &py, int &sn) {
    int pix = slot & 255;
    int rest = slot >> 8;
    int sIdx = rest % rp.sCount;
    int tileInBatch = rest / rp.sCount;
    int local = rp.tileLocal0 + tileInBatch;
    int t = rp.rd->tile_first + local * rp.rd->tile_step;
    int tx = t % rp.nTilesX, ty = t / rp.nTilesX;
    px = rp.rd->sample_bounds[0] + tx * 16 + (pix & 15);
    py = rp.rd->sample_bounds[1] + ty * 16 + (pix >> 4);
    sn = rp.s0 + sIdx;
    if (px >= rp.rd->sample_bounds[2] || py >= rp.rd->sample_bounds[3]) return false;
    // InsideExclusive(pixel, pixelBounds), integrator.cpp:273
    return px >= rp.rd->pixel_bounds[0] && px < rp.rd->pixel_bounds[2] && py >= rp.rd->pixel_bounds[1] && py < rp.rd->pixel_bounds[3];
}

// The matrix AnimatedTransform CameraToWorld carries a ray of time `time` to world space with (AnimatedTransform::operator()(Ray),
// transform.cpp:1171-1181): the start transform up to startTime, the end transform from endTime on, in between Interpolate (pg_motion.h)
// -- only .m is formed: a ray is transformed by m alone (transform.h:249-262), so Transform(scale)'s inverse is never looked at.
PG_DEV void camera_matrix_at(const PgRenderDesc &rd, float time, float *m) {
    if (!rd.camera_animated || time <= rd.camera_time[0]) { for (int k = 0; k < 16; ++k) m[k] = rd.camera_to_world[k]; return; }
    if (time >= rd.camera_time[1]) { for (int k = 0; k < 16; ++k) m[k] = rd.camera_to_world_end[k]; return; }
    const float dt = (time - rd.camera_time[0]) / (rd.camera_time[1] - rd.camera_time[0]);
    interpolate_trs<false>(rd.camera_T, rd.camera_R, rd.camera_S, dt, m, nullptr);
}
// CameraSample::time -> the ray's time, perspective.cpp:90 / :121: Lerp(sample.time, shutterOpen, shutterClose)
PG_DEV float camera_time(const PgRenderDesc &rd, float u) { return (1 - u) * rd.shutter_open + u * rd.shutter_close; }
// Camera::GenerateRay: PerspectiveCamera (perspective.cpp:95-115,141), OrthographicCamera (orthographic.cpp:68-93,115) and
// EnvironmentCamera (environment.cpp:43-56), ending in CameraToWorld(ray) -- c2w: the matrix of the ray's time (camera_matrix_at).
// (l0, l1) = CameraSample::pLens.
PG_DEV void camera_ray(const PgRenderDesc &rd, const float *c2w, float pFilmX, float pFilmY, float l0, float l1, V3 &o, V3 &d, float &tMax) {
    V3 pCamera = xform_point(rd.raster_to_camera, mk(pFilmX, pFilmY, 0));
    o = mk(0, 0, 0);
    d = normalize(mk(pCamera.x, pCamera.y, pCamera.z));
    tMax = PG_INF;
    if (rd.camera_type == 1) { o = pCamera; d = mk(0, 0, 1); }  // OrthographicCamera, orthographic.cpp:76-78
    if (rd.camera_type == 2) {  // EnvironmentCamera::GenerateRay, environment.cpp:43-56
        const float theta = PG_PI * pFilmY / rd.full_res[1];
        const float phi = 2 * PG_PI * pFilmX / rd.full_res[0];
        float sT, cT, sP, cP;
        pg_sincosf(theta, &sT, &cT);
        pg_sincosf(phi, &sP, &cP);
        o = mk(0, 0, 0);
        d = mk((float)sT * (float)cP, (float)cT, (float)sT * (float)sP);
    }
    if (rd.lens_radius > 0) {
        float lx, ly;
        concentric_sample_disk(l0, l1, lx, ly);
        lx = rd.lens_radius * lx; ly = rd.lens_radius * ly;
        float ft = rd.focal_distance / d.z;
        V3 pFocus = o + d * ft;
        o = mk(lx, ly, 0);
        d = normalize(pFocus - o);
    }
    xform_ray(c2w, o, d, tMax);
}
// The camera ray's differentials (GenerateRayDifferential: perspective.cpp:117-140, orthographic.cpp:95-113, the finite
// difference of camera.cpp:52-93 for the environment camera), carried to world space (transform.h:264-273) and scaled by
// 1 / sqrt(spp) (integrator.cpp:282-283, geometry.h:908-913).  (o, d) = the world-space camera ray.
PG_DEV void camera_differentials(const PgRenderDesc &rd, const float *c2w, float pFilmX, float pFilmY, float l0, float l1, V3 o, V3 d, V3 &rxO, V3 &rxD, V3 &ryO, V3 &ryD) {
    if (rd.camera_type == 2) {
        const float eps = .05f;
        V3 xo, xd, yo, yd;
        float tm;
        camera_ray(rd, c2w, pFilmX + eps, pFilmY, l0, l1, xo, xd, tm);
        camera_ray(rd, c2w, pFilmX, pFilmY + eps, l0, l1, yo, yd, tm);
        rxO = o + vdiv(xo - o, eps); rxD = d + vdiv(xd - d, eps);
        ryO = o + vdiv(yo - o, eps); ryD = d + vdiv(yd - d, eps);
    } else {
        const V3 dxCamera = mk(rd.dx_camera[0], rd.dx_camera[1], rd.dx_camera[2]), dyCamera = mk(rd.dy_camera[0], rd.dy_camera[1], rd.dy_camera[2]);
        const V3 pCamera = xform_point(rd.raster_to_camera, mk(pFilmX, pFilmY, 0));
        V3 co = mk(0, 0, 0), cd = normalize(mk(pCamera.x, pCamera.y, pCamera.z));  // the camera-space main ray again
        if (rd.camera_type == 1) { co = pCamera; cd = mk(0, 0, 1); }
        float lx = 0, ly = 0;
        if (rd.lens_radius > 0) {
            concentric_sample_disk(l0, l1, lx, ly);
            lx = rd.lens_radius * lx; ly = rd.lens_radius * ly;
            const float ft = rd.focal_distance / cd.z;
            const V3 pFocus = co + cd * ft;
            co = mk(lx, ly, 0);
            cd = normalize(pFocus - co);
        }
        if (rd.camera_type == 0) {
            if (rd.lens_radius > 0) {
                const V3 dx = normalize(pCamera + dxCamera);
                float ft = rd.focal_distance / dx.z;
                V3 pFocus = mk(0, 0, 0) + dx * ft;
                rxO = mk(lx, ly, 0);
                rxD = normalize(pFocus - rxO);
                const V3 dy = normalize(pCamera + dyCamera);
                ft = rd.focal_distance / dy.z;
                pFocus = mk(0, 0, 0) + dy * ft;
                ryO = mk(lx, ly, 0);
                ryD = normalize(pFocus - ryO);
            } else {
                rxO = ryO = co;
                rxD = normalize(pCamera + dxCamera);
                ryD = normalize(pCamera + dyCamera);
            }
        } else {
            if (rd.lens_radius > 0) {
                const float ft = rd.focal_distance / cd.z;
                V3 pFocus = (pCamera + dxCamera) + mk(0, 0, 1) * ft;
                rxO = mk(lx, ly, 0);
                rxD = normalize(pFocus - rxO);
                pFocus = (pCamera + dyCamera) + mk(0, 0, 1) * ft;
                ryO = mk(lx, ly, 0);
                ryD = normalize(pFocus - ryO);
            } else {
                rxO = co + dxCamera;
                ryO = co + dyCamera;
                rxD = ryD = cd;
            }
        }
        rxO = xform_point(c2w, rxO); ryO = xform_point(c2w, ryO);
        rxD = m4_vec(c2w, rxD); ryD = m4_vec(c2w, ryD);
    }
    const float sc = 1 / sqrtf((float)rd.spp);
    rxO = o + (rxO - o) * sc; ryO = o + (ryO - o) * sc;
    rxD = d + (rxD - d) * sc; ryD = d + (ryD - d) * sc;
}
// ANIM: the camera moves (PgRenderDesc::camera_animated) -- every sample's camera-to-world matrix is interpolated at its time; the still
// camera's kernel does not carry that code (64 instead of 39 registers, 113 spilled scalars)
// The realistic camera's sample (camera_type 3): Camera::GenerateRayDifferential over the lens system `L` (pg_lens.h) -- the main ray and the
// shifted rays, each carried to world space by c2w and normalized (realistic.cpp:700-701) -- giving the world-space ray, the sample's weight
// (0: vignetted), the calls' statistics, and where `diff` is not null the differentials scaled by 1 / sqrt(spp) (integrator.cpp:282-283) as 12 floats.
PG_DEV float lens_camera_sample(const PgLensSystem &L, const PgRenderDesc &rd, const float *c2w, float pFilmX, float pFilmY, float l0, float l1, V3 &o, V3 &d, float &tMax,
                                int &nCalls, int &nVignetted, float4 *diff) {
    LensRay rays[3];
    float eps[2] = {.05f, .05f};
    auto toWorld = [&](LensRay &r) {
        V3 ro = mk(r.o.x, r.o.y, r.o.z), rdir = mk(r.d.x, r.d.y, r.d.z);
        float tm = PG_INF;
        xform_ray(c2w, ro, rdir, tm);
        rdir = normalize(rdir);
        r.o = lens_v(ro.x, ro.y, ro.z); r.d = lens_v(rdir.x, rdir.y, rdir.z);
    };
    const float wt = lens_generate_ray_differential(L, pFilmX, pFilmY, rd.full_res[0], rd.full_res[1], l0, l1, rd.shutter_close - rd.shutter_open, toWorld, rays, eps,
                                                    &nCalls, &nVignetted);
    if (wt == 0) return 0;
    o = mk(rays[0].o.x, rays[0].o.y, rays[0].o.z); d = mk(rays[0].d.x, rays[0].d.y, rays[0].d.z);
    tMax = PG_INF;
    if (diff) {
        const V3 xo = mk(rays[1].o.x, rays[1].o.y, rays[1].o.z), xd = mk(rays[1].d.x, rays[1].d.y, rays[1].d.z);
        const V3 yo = mk(rays[2].o.x, rays[2].o.y, rays[2].o.z), yd = mk(rays[2].d.x, rays[2].d.y, rays[2].d.z);
        V3 rxO = o + vdiv(xo - o, eps[0]), rxD = d + vdiv(xd - d, eps[0]);  // camera.cpp:72-73, :87-88
        V3 ryO = o + vdiv(yo - o, eps[1]), ryD = d + vdiv(yd - d, eps[1]);
        const float sc = 1 / sqrtf((float)rd.spp);
        rxO = o + (rxO - o) * sc; ryO = o + (ryO - o) * sc;
        rxD = d + (rxD - d) * sc; ryD = d + (ryD - d) * sc;
        diff[0] = make_float4(rxO.x, rxO.y, rxO.z, rxD.x); diff[1] = make_float4(rxD.y, rxD.z, ryO.x, ryO.y); diff[2] = make_float4(ryO.z, ryD.x, ryD.y, ryD.z);
    }
    return wt;
}
// The lens statistics of the lanes of a wave in one set of atomics (as the integrator statistics are counted): calls, vignetted, samples of weight 0
PG_DEV void lens_stats_add(LensFrame *lens, int nCalls, int nVignetted, bool zeroWeight) {
    const unsigned long long calls = wave_sum((unsigned long long)nCalls), vig = wave_sum((unsigned long long)nVignetted), zero = wave_sum(zeroWeight ? 1ull : 0ull);
    if (lane_id() == 0 && calls) {
        unsigned long long *st = lens->stats;
        atomicAdd(st, calls);
        if (vig) atomicAdd(st + 1, vig);
        if (zero) atomicAdd(st + 2, zero);
    }
}

#endif  // PG_CAMERA_H
