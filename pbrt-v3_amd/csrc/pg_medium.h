// pg_medium.h -- participating media as device functions: HomogeneousMedium's transmittance and distance sample, the
// Henyey-Greenstein phase function, and a primitive's medium interface.  (GridDensityMedium: pg_grid.h.)
//
// Used by the VOL instantiations of k_shade, k_through, k_resolve_vol and k_sss_exit (pg_kernels.hip) and by k_tr_step / k_medium_sample
// (pg_mediumquery.h).  phase_hg / hg_sample_p are
// pinned on the host (tests/test_device_headers_on_host.py) and on the device (tests/test_gpu_device_arithmetic.py).
#ifndef PG_MEDIUM_H
#define PG_MEDIUM_H
#include "pg_device.h"
#include "pg_kernels.h"

// ===========================================================================
// Participating media (VolPathIntegrator): HomogeneousMedium and the Henyey-Greenstein phase function.  expf / logf /
// sinf / cosf are evaluated in double and rounded once, like every libm call of this file (DESIGN.md "libm").
// ===========================================================================
#define PG_MAX_FLOAT 3.40282346638528859811704183484516925e+38f
PG_DEV Spec sp_exp(Spec a) { return sp3(pg_expf(a.r), pg_expf(a.g), pg_expf(a.b)); }  // Exp(), spectrum.h:414-419
// HomogeneousMedium::Tr, homogeneous.cpp:44-47, for a ray with the given tMax and |d|
PG_DEV Spec medium_tr(const PgMedium &m, float tMax, float dLen) {
    const Spec negSt = sp3(-m.sigma_t[0], -m.sigma_t[1], -m.sigma_t[2]);
    return sp_exp(negSt * pmin(tMax * dLen, PG_MAX_FLOAT));
}
PG_DEV float phase_hg(float cosTheta, float g) {  // medium.h:69-72
    const float denom = 1 + g * g + 2 * g * cosTheta;
    return 0.07957747154594766788f * (1 - g * g) / (denom * sqrtf(denom));
}
PG_DEV float hg_sample_p(float g, V3 wo, V3 &wi, float u0, float u1) {  // HenyeyGreenstein::Sample_p, medium.cpp:194-213
    float cosTheta;
    if ((double)fabsf(g) < 1e-3) cosTheta = 1 - 2 * u0;
    else {
        const float sqrTerm = (1 - g * g) / (1 + g - 2 * g * u0);
        cosTheta = -(1 + g * g - sqrTerm * sqrTerm) / (2 * g);
    }
    const float sinTheta = sqrtf(pmax(0.f, 1 - cosTheta * cosTheta));
    const float phi = 2 * PG_PI * u1;
    V3 v1, v2;
    coordinate_system(wo, v1, v2);
    float sP, cP;
    pg_sincosf(phi, &sP, &cP);
    wi = (v1 * (sinTheta * (float)cP) + v2 * (sinTheta * (float)sP)) + wo * cosTheta;  // SphericalDirection, geometry.h:1461-1466
    return phase_hg(cosTheta, g);
}
// The phase function as EstimateDirect's scattering model at a medium vertex (pg_estimate.h; integrator.cpp:135-141, :181-186): f = pdf = p(wo, wi),
// without a cosine; a sampled direction's value and pdf are Sample_p's one number.  (k_shade's medium vertex spells the same out in place, for its
// registers' sake; these are pinned by tests/test_device_headers_on_host.py and tests/test_gpu_device_arithmetic.py for the kernel that can call them)
struct HgPhase { float g; };
PG_DEV Spec scatter_f_cos(const HgPhase &m, V3 wo, V3 wi) { return sp(phase_hg(dot(wo, wi), m.g)); }
PG_DEV float scatter_pdf(const HgPhase &m, V3 wo, V3 wi) { return phase_hg(dot(wo, wi), m.g); }
PG_DEV Spec scatter_sample(const HgPhase &m, V3 wo, V3 &wi, float u0, float u1, float &pdf) {
    pdf = hg_sample_p(m.g, wo, wi, u0, u1);
    return sp(pdf);
}
// GeometricPrimitive::Intersect's mediumInterface (primitive.cpp:121-125): the primitive's own when it marks a transition,
// else the ray's medium on both sides.  Media are index + 1, 0 = none.
PG_DEV void prim_interface(const DScene &sc, int prim, int rayMedium, int &mIn, int &mOut) {
    const int in1 = sc.triMediumIn ? sc.triMediumIn[prim] + 1 : 0, out1 = sc.triMediumOut ? sc.triMediumOut[prim] + 1 : 0;
    if (in1 != out1) { mIn = in1; mOut = out1; }
    else mIn = mOut = rayMedium;
}
// HomogeneousMedium::Sample's channel and distance from its two numbers, homogeneous.cpp:51-54
PG_DEV void homogeneous_sample_distance(const PgMedium &mm, float uChannel, float uDist, int &channel, float &dist) {
    channel = (int)(uChannel * 3);
    if (channel > 2) channel = 2;
    dist = -pg_logf((1 - uDist)) / mm.sigma_t[channel];
}
// ... and the rest of it, homogeneous.cpp:55-73, for a ray of length dLen = |d| whose tMax is tMaxRay: the interaction's ray parameter t (tMaxRay where
// the ray leaves the medium), whether the medium was sampled, and the weight Sample returns -- k_shade's medium vertex (pg_kernels.hip) spells the same
// out in place, in this operation order; k_medium_sample (pg_mediumquery.h) calls this.  Pinned by tests/test_medium_headers_on_host.py.
PG_DEV Spec homogeneous_sample_weight(const PgMedium &mm, float dist, float dLen, float tMaxRay, float &t, bool &inMedium) {
    t = pmin(dist / dLen, tMaxRay);
    inMedium = t < tMaxRay;
    const Spec sigT = sp3(mm.sigma_t[0], mm.sigma_t[1], mm.sigma_t[2]), sigS = sp3(mm.sigma_s[0], mm.sigma_s[1], mm.sigma_s[2]);
    const Spec Tr = sp_exp((sp3(-sigT.r, -sigT.g, -sigT.b) * pmin(t, PG_MAX_FLOAT)) * dLen);
    const Spec density = inMedium ? sigT * Tr : Tr;
    float pdf = 0;
    pdf += density.r; pdf += density.g; pdf += density.b;
    pdf *= 1 / (float)3;
    if (pdf == 0) pdf = 1;
    return inMedium ? (Tr * sigS) / pdf : Tr / pdf;
}

#endif  // PG_MEDIUM_H
