// pg_lens.h -- RealisticCamera's lens arithmetic (cameras/realistic.cpp), written once for the host front end (host/realistic.cpp: focusing, exit
// pupil bounds) and for the device (k_generate's realistic instantiation), so that both compute the same bits.  No HIP call and no libm beyond
// sqrt: the header compiles with a plain C++ compiler and for gfx950.  Float operations keep the reference's order and association; the
// translation units that include it are built with -ffp-contract=off and IEEE divide / sqrt.  Citations are to the reference's src/.
#ifndef PG_LENS_H
#define PG_LENS_H
#include <stdint.h>
#include <math.h>
#if defined(__HIPCC__) || defined(HIP_EMU_H)
#define PG_LENS_FN __host__ __device__ inline
#else
#define PG_LENS_FN inline
#endif
#ifndef PG_MAX_LENS_INTERFACES
#define PG_MAX_LENS_INTERFACES 32
#endif
#define PG_LENS_PUPIL_SEGMENTS 64

// The lens block of PgRenderDesc (ABI 30, include/pbrt_gpu.h), field for field: n_lens_interfaces .. lens_simple_weighting
struct PgLensSystem {
    int32_t n;
    float iface[PG_MAX_LENS_INTERFACES][4];  // curvatureRadius, thickness, eta, apertureRadius (realistic.h:62-67), metres, front to rear
    float pupil[PG_LENS_PUPIL_SEGMENTS][4];  // exitPupilBounds: pMin.x, pMin.y, pMax.x, pMax.y
    float extent[4];                         // Film::GetPhysicalExtent(): pMin.x, pMin.y, pMax.x, pMax.y
    float diagonal;                          // Film::diagonal, metres
    int32_t simple;                          // simpleWeighting
};
struct LensV3 { float x, y, z; };
struct LensRay { LensV3 o, d; };  // (tMax = Infinity stays Infinity through every step; time and medium ride along outside)

PG_LENS_FN LensV3 lens_v(float x, float y, float z) { LensV3 r; r.x = x; r.y = y; r.z = z; return r; }
PG_LENS_FN LensV3 lens_sub(LensV3 a, LensV3 b) { return lens_v(a.x - b.x, a.y - b.y, a.z - b.z); }
PG_LENS_FN LensV3 lens_add(LensV3 a, LensV3 b) { return lens_v(a.x + b.x, a.y + b.y, a.z + b.z); }
PG_LENS_FN LensV3 lens_scale(LensV3 a, float s) { return lens_v(a.x * s, a.y * s, a.z * s); }  // geometry.h:232-234
PG_LENS_FN LensV3 lens_div(LensV3 a, float f) { const float inv = 1.f / f; return lens_v(a.x * inv, a.y * inv, a.z * inv); }  // geometry.h:243-248
PG_LENS_FN float lens_dot(LensV3 a, LensV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PG_LENS_FN LensV3 lens_normalize(LensV3 a) { return lens_div(a, sqrtf(a.x * a.x + a.y * a.y + a.z * a.z)); }  // geometry.h:984-986
PG_LENS_FN float lens_lerp(float t, float a, float b) { return (1 - t) * a + t * b; }  // pbrt.h:417
PG_LENS_FN float lens_rear_z(const PgLensSystem &L) { return L.iface[L.n - 1][1]; }  // LensRearZ, realistic.h:69
PG_LENS_FN float lens_front_z(const PgLensSystem &L) {  // LensFrontZ, realistic.h:70-74
    float zSum = 0;
    for (int i = 0; i < L.n; ++i) zSum += L.iface[i][1];
    return zSum;
}

// Scale(1, 1, -1) applied to a ray: Transform::operator()(const Ray &), transform.h:251-264 -- the point with its error bound (:277-300), the
// vector (:235-241), then the origin moved along d to the edge of the error bound.  The matrix is diag(1, 1, -1, 1): w = 1, no division.
PG_LENS_FN LensRay lens_flip_z(const LensRay &r) {
    const float x = r.o.x, y = r.o.y, z = r.o.z;
    const float xp = (1.f * x + 0.f * y) + (0.f * z + 0.f);
    const float yp = (0.f * x + 1.f * y) + (0.f * z + 0.f);
    const float zp = (0.f * x + 0.f * y) + (-1.f * z + 0.f);
    const float g3 = (3 * 5.9604644775390625e-08f) / (1 - 3 * 5.9604644775390625e-08f);  // gamma(3), pbrt.h:289-291
    const float xAbs = (fabsf(1.f * x) + fabsf(0.f * y) + fabsf(0.f * z) + fabsf(0.f));
    const float yAbs = (fabsf(0.f * x) + fabsf(1.f * y) + fabsf(0.f * z) + fabsf(0.f));
    const float zAbs = (fabsf(0.f * x) + fabsf(0.f * y) + fabsf(-1.f * z) + fabsf(0.f));
    const LensV3 oError = lens_v(xAbs * g3, yAbs * g3, zAbs * g3);
    LensRay out;
    out.o = lens_v(xp, yp, zp);
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    out.d = lens_v(1.f * dx + 0.f * dy + 0.f * dz, 0.f * dx + 1.f * dy + 0.f * dz, 0.f * dx + 0.f * dy + -1.f * dz);
    const float lengthSquared = out.d.x * out.d.x + out.d.y * out.d.y + out.d.z * out.d.z;
    if (lengthSquared > 0) {
        const float dt = lens_dot(lens_v(fabsf(out.d.x), fabsf(out.d.y), fabsf(out.d.z)), oError) / lengthSquared;
        out.o = lens_add(out.o, lens_scale(out.d, dt));
    }
    return out;
}

// Quadratic, pbrt.h:419-435: the discriminant, its root, q and both quotients in double, each result rounded to float once
PG_LENS_FN bool lens_quadratic(float a, float b, float c, float *t0, float *t1) {
    const double discrim = (double)b * (double)b - 4 * (double)a * (double)c;
    if (discrim < 0) return false;
    const double rootDiscrim = sqrt(discrim);
    double q;
    if (b < 0) q = -.5 * ((double)b - rootDiscrim);
    else q = -.5 * ((double)b + rootDiscrim);
    *t0 = (float)(q / (double)a);
    *t1 = (float)((double)c / q);
    if (*t0 > *t1) { const float s = *t0; *t0 = *t1; *t1 = s; }
    return true;
}
// RealisticCamera::IntersectSphericalElement, realistic.cpp:153-173
PG_LENS_FN bool lens_intersect_spherical(float radius, float zCenter, const LensRay &ray, float *t, LensV3 *n) {
    const LensV3 o = lens_sub(ray.o, lens_v(0, 0, zCenter));
    const float A = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    const float B = 2 * (ray.d.x * o.x + ray.d.y * o.y + ray.d.z * o.z);
    const float C = o.x * o.x + o.y * o.y + o.z * o.z - radius * radius;
    float t0, t1;
    if (!lens_quadratic(A, B, C, &t0, &t1)) return false;
    const bool useCloserT = (ray.d.z > 0) ^ (radius < 0);
    *t = useCloserT ? (t1 < t0 ? t1 : t0) : (t0 < t1 ? t1 : t0);  // std::min(t0, t1) : std::max(t0, t1)
    if (*t < 0) return false;
    LensV3 nn = lens_normalize(lens_add(o, lens_scale(ray.d, *t)));
    // Faceforward(n, -ray.d), geometry.h:1005-1008
    if (lens_dot(nn, lens_v(-ray.d.x, -ray.d.y, -ray.d.z)) < 0.f) nn = lens_v(-nn.x, -nn.y, -nn.z);
    *n = nn;
    return true;
}
// Refract, reflection.h:97-109
PG_LENS_FN bool lens_refract(LensV3 wi, LensV3 n, float eta, LensV3 *wt) {
    const float cosThetaI = lens_dot(n, wi);
    const float s = 1 - cosThetaI * cosThetaI;
    const float sin2ThetaI = (0.f < s) ? s : 0.f;  // std::max(Float(0), .)
    const float sin2ThetaT = eta * eta * sin2ThetaI;
    if (sin2ThetaT >= 1) return false;
    const float cosThetaT = sqrtf(1 - sin2ThetaT);
    const float k = eta * cosThetaI - cosThetaT;
    *wt = lens_add(lens_v(eta * -wi.x, eta * -wi.y, eta * -wi.z), lens_v(k * n.x, k * n.y, k * n.z));
    return true;
}

// RealisticCamera::TraceLensesFromFilm, realistic.cpp:100-151.  rOut may be null.  (CHECK_GE(t, 0) cannot fire: the spherical branch has
// returned for t < 0, the stop branch divides a negative by a negative or returns.)
PG_LENS_FN bool lens_trace_from_film(const PgLensSystem &L, const LensRay &rCamera, LensRay *rOut) {
    float elementZ = 0;
    LensRay rLens = lens_flip_z(rCamera);
    for (int i = L.n - 1; i >= 0; --i) {
        const float curvatureRadius = L.iface[i][0], thickness = L.iface[i][1], eta = L.iface[i][2], apertureRadius = L.iface[i][3];
        elementZ -= thickness;
        float t;
        LensV3 n = lens_v(0, 0, 0);
        const bool isStop = (curvatureRadius == 0);
        if (isStop) {
            if (rLens.d.z >= 0.0) return false;
            t = (elementZ - rLens.o.z) / rLens.d.z;
        } else {
            const float zCenter = elementZ + curvatureRadius;
            if (!lens_intersect_spherical(curvatureRadius, zCenter, rLens, &t, &n)) return false;
        }
        const LensV3 pHit = lens_add(rLens.o, lens_scale(rLens.d, t));
        const float r2 = pHit.x * pHit.x + pHit.y * pHit.y;
        if (r2 > apertureRadius * apertureRadius) return false;
        rLens.o = pHit;
        if (!isStop) {
            LensV3 w;
            const float etaI = eta;
            const float etaT = (i > 0 && L.iface[i - 1][2] != 0) ? L.iface[i - 1][2] : 1;
            if (!lens_refract(lens_normalize(lens_v(-rLens.d.x, -rLens.d.y, -rLens.d.z)), n, etaI / etaT, &w)) return false;
            rLens.d = w;
        }
    }
    if (rOut) *rOut = lens_flip_z(rLens);
    return true;
}
// RealisticCamera::TraceLensesFromScene, realistic.cpp:175-223 (the host's focusing only).  *negativeT: the reference's CHECK_GE(t, 0) would
// have aborted (a stop met by a ray that runs away from it); the caller reports it.
PG_LENS_FN bool lens_trace_from_scene(const PgLensSystem &L, const LensRay &rCamera, LensRay *rOut, bool *negativeT) {
    float elementZ = -lens_front_z(L);
    LensRay rLens = lens_flip_z(rCamera);
    for (int i = 0; i < L.n; ++i) {
        const float curvatureRadius = L.iface[i][0], thickness = L.iface[i][1], apertureRadius = L.iface[i][3];
        float t;
        LensV3 n = lens_v(0, 0, 0);
        const bool isStop = (curvatureRadius == 0);
        if (isStop) t = (elementZ - rLens.o.z) / rLens.d.z;
        else {
            const float zCenter = elementZ + curvatureRadius;
            if (!lens_intersect_spherical(curvatureRadius, zCenter, rLens, &t, &n)) return false;
        }
        if (!(t >= 0)) { if (negativeT) *negativeT = true; return false; }
        const LensV3 pHit = lens_add(rLens.o, lens_scale(rLens.d, t));
        const float r2 = pHit.x * pHit.x + pHit.y * pHit.y;
        if (r2 > apertureRadius * apertureRadius) return false;
        rLens.o = pHit;
        if (!isStop) {
            LensV3 wt;
            const float etaI = (i == 0 || L.iface[i - 1][2] == 0) ? 1 : L.iface[i - 1][2];
            const float etaT = (L.iface[i][2] != 0) ? L.iface[i][2] : 1;
            if (!lens_refract(lens_normalize(lens_v(-rLens.d.x, -rLens.d.y, -rLens.d.z)), n, etaI / etaT, &wt)) return false;
            rLens.d = wt;
        }
        elementZ += thickness;
    }
    if (rOut) *rOut = lens_flip_z(rLens);
    return true;
}

// RealisticCamera::SampleExitPupil, realistic.cpp:613-631: the point on the rear element's plane; *area = the sampled box's Area()
// (geometry.h:603-606: (pMax.x - pMin.x) * (pMax.y - pMin.y))
PG_LENS_FN float lens_pupil_area(const float *b) { return (b[2] - b[0]) * (b[3] - b[1]); }
PG_LENS_FN LensV3 lens_sample_exit_pupil(const PgLensSystem &L, float pFilmX, float pFilmY, float lens0, float lens1, float *area) {
    const float rFilm = sqrtf(pFilmX * pFilmX + pFilmY * pFilmY);
    int rIndex = (int)(rFilm / (L.diagonal / 2) * PG_LENS_PUPIL_SEGMENTS);
    rIndex = rIndex < PG_LENS_PUPIL_SEGMENTS - 1 ? rIndex : PG_LENS_PUPIL_SEGMENTS - 1;  // std::min(size - 1, rIndex)
    if (rIndex < 0) rIndex = 0;  // (a NaN or negative quotient cannot occur for a finite film point; the table is not read outside itself)
    const float *b = L.pupil[rIndex];
    *area = lens_pupil_area(b);
    const float lx = lens_lerp(lens0, b[0], b[2]), ly = lens_lerp(lens1, b[1], b[3]);  // Bounds2::Lerp, geometry.h:610-613
    const float sinTheta = (rFilm != 0) ? pFilmY / rFilm : 0;
    const float cosTheta = (rFilm != 0) ? pFilmX / rFilm : 1;
    return lens_v(cosTheta * lx - sinTheta * ly, sinTheta * lx + cosTheta * ly, lens_rear_z(L));
}

// RealisticCamera::GenerateRay, realistic.cpp:679-712, up to the camera-space ray that leaves the lens: the weight (0 = vignetted), the ray in
// *out.  fullRes: Film::fullResolution; dShutter = shutterClose - shutterOpen.  The caller carries the ray through CameraToWorld at its
// time and normalizes its direction (:700-701), and counts the call (totalRays, and vignettedRays where 0 comes back).
PG_LENS_FN float lens_generate_ray(const PgLensSystem &L, float sFilmX, float sFilmY, int fullResX, int fullResY, float lens0, float lens1, float dShutter, LensRay *out) {
    const float sx = sFilmX / fullResX, sy = sFilmY / fullResY;
    const float p2x = lens_lerp(sx, L.extent[0], L.extent[2]), p2y = lens_lerp(sy, L.extent[1], L.extent[3]);
    const LensV3 pFilm = lens_v(-p2x, p2y, 0);
    float area;
    const LensV3 pRear = lens_sample_exit_pupil(L, pFilm.x, pFilm.y, lens0, lens1, &area);
    LensRay rFilm;
    rFilm.o = pFilm;
    rFilm.d = lens_sub(pRear, pFilm);
    if (!lens_trace_from_film(L, rFilm, out)) return 0;
    const float cosTheta = lens_normalize(rFilm.d).z;
    const float cos4Theta = (cosTheta * cosTheta) * (cosTheta * cosTheta);
    if (L.simple) return cos4Theta * area / lens_pupil_area(L.pupil[0]);
    return dShutter * (cos4Theta * area) / (lens_rear_z(L) * lens_rear_z(L));
}

// Camera::GenerateRayDifferential, camera.cpp:60-97 (RealisticCamera inherits it): the main ray, then a ray shifted by +.05 in x (by -.05 if
// that one is vignetted), then the same in y; 0 when the main ray or both shifts of an axis are vignetted.  XF carries a camera-space ray
// to world space and normalizes its direction (GenerateRay's tail): void operator()(LensRay &).  rays[0 .. 2] = main, x, y; eps[0 .. 1] = the
// shift that succeeded per axis; nCalls / nVignetted: the GenerateRay calls made and those that returned 0 (the statistic
// "Camera/Rays vignetted by lens system", realistic.cpp:47).
template <class XF>
PG_LENS_FN float lens_generate_ray_differential(const PgLensSystem &L, float sFilmX, float sFilmY, int fullResX, int fullResY, float lens0, float lens1, float dShutter,
                                                XF &&toWorld, LensRay rays[3], float eps[2], int *nCalls, int *nVignetted) {
    *nCalls = 1; *nVignetted = 0;
    const float wt = lens_generate_ray(L, sFilmX, sFilmY, fullResX, fullResY, lens0, lens1, dShutter, &rays[0]);
    if (wt == 0) { *nVignetted = 1; return 0; }
    toWorld(rays[0]);
    for (int axis = 0; axis < 2; ++axis) {
        float w = 0;
        for (int k = 0; k < 2 && w == 0; ++k) {
            const float e = k == 0 ? .05f : -.05f;
            ++*nCalls;
            w = lens_generate_ray(L, axis == 0 ? sFilmX + e : sFilmX, axis == 1 ? sFilmY + e : sFilmY, fullResX, fullResY, lens0, lens1, dShutter, &rays[1 + axis]);
            if (w == 0) ++*nVignetted;
            else { toWorld(rays[1 + axis]); eps[axis] = e; }
        }
        if (w == 0) return 0;
    }
    return wt;
}
// rxOrigin = o + (rx.o - o) / eps and so on (camera.cpp:72-73, :87-88)
PG_LENS_FN LensV3 lens_differential(LensV3 main, LensV3 shifted, float eps) { return lens_add(main, lens_div(lens_sub(shifted, main), eps)); }
#endif
