// pg_bxdf.h -- the BSDFs as device functions: the specialised Bsdf of matte / plastic / mirror / glass with its microfacet
// trigonometry, and the BxDF-list LobeBsdfT over PgBxDF or PkLobe records (lobe_f / lobe_pdf / lobe_f_pdf / lobe_sample_f per BxDF,
// lbsdf_f / lbsdf_pdf / lbsdf_sample_f over a list), the one-lobe AdapterBsdf at a BSSRDF's exit point, and what EstimateDirect asks of any of
// them (scatter_f_cos / scatter_pdf / scatter_sample; pg_medium.h has the phase function's).
//
// Used by k_shade, k_sss_exit (pg_kernels.hip), k_direct (pg_direct.h) and k_scatter (pg_scatter.h).  lobe_f_pdf and lobe_sample_f are pinned on the host
// (tests/test_device_headers_on_host.py) and on the device (tests/test_gpu_device_arithmetic.py), and so are AdapterBsdf's three functions.
#ifndef PG_BXDF_H
#define PG_BXDF_H
#include "pg_device.h"
#include "pg_kernels.h"
#include "pg_texture.h"
#include "pg_bssrdf.h"

// BSDF: LambertianReflection and/or MicrofacetReflection(TrowbridgeReitz, FresnelDielectric(1.5, 1)) lobes in the order
// the materials add them (matte.cpp:45-62, plastic.cpp:45-70); reflection.h:164-213, reflection.cpp:680-796.
struct Bsdf {
    V3 ns, ng, ss, ts; Spec R, Ks; float alpha; int nBxDFs; bool hasDiff, hasSpec;
    bool orenNayar; float onA, onB;  // the diffuse lobe is OrenNayar(R, sigma) (reflection.h:425-431) instead of LambertianReflection
    int specular;  // 0; 1 = SpecularReflection(Kr, FresnelNoOp) (mirror.cpp:44-56); 2 = FresnelSpecular(Kr, Kt, 1, eta) (glass.cpp:45-65)
    Spec Kr, Kt; float eta;
};
#define PG_BSDF_REFLECTION 1
#define PG_BSDF_TRANSMISSION 2
#define PG_BSDF_SPECULAR 16
PG_DEV V3 world_to_local(const Bsdf &b, V3 v) { return mk(dot(v, b.ss), dot(v, b.ts), dot(v, b.ns)); }
PG_DEV V3 local_to_world(const Bsdf &b, V3 v) {
    return mk(b.ss.x * v.x + b.ts.x * v.y + b.ns.x * v.z, b.ss.y * v.x + b.ts.y * v.y + b.ns.y * v.z,
              b.ss.z * v.x + b.ts.z * v.y + b.ns.z * v.z);
}
// reflection.h:52-83
PG_DEV float cos2_theta(V3 w) { return w.z * w.z; }
PG_DEV float sin2_theta(V3 w) { return pmax(0.f, 1.f - cos2_theta(w)); }
PG_DEV float sin_theta(V3 w) { return sqrtf(sin2_theta(w)); }
PG_DEV float tan_theta(V3 w) { return sin_theta(w) / w.z; }
PG_DEV float tan2_theta(V3 w) { return sin2_theta(w) / cos2_theta(w); }
PG_DEV float cos_phi(V3 w) { float st = sin_theta(w); return (st == 0) ? 1 : clampf(w.x / st, -1, 1); }
PG_DEV float sin_phi(V3 w) { float st = sin_theta(w); return (st == 0) ? 0 : clampf(w.y / st, -1, 1); }
PG_DEV float cos2_phi(V3 w) { return cos_phi(w) * cos_phi(w); }
PG_DEV float sin2_phi(V3 w) { return sin_phi(w) * sin_phi(w); }
PG_DEV float fr_dielectric(float cosThetaI, float etaI, float etaT) {  // reflection.cpp:47-68
    cosThetaI = clampf(cosThetaI, -1, 1);
    if (!(cosThetaI > 0.f)) { float t = etaI; etaI = etaT; etaT = t; cosThetaI = fabsf(cosThetaI); }
    float sinThetaI = sqrtf(pmax(0.f, 1 - cosThetaI * cosThetaI));
    float sinThetaT = etaI / etaT * sinThetaI;
    if (sinThetaT >= 1) return 1;
    float cosThetaT = sqrtf(pmax(0.f, 1 - sinThetaT * sinThetaT));
    float Rparl = ((etaT * cosThetaI) - (etaI * cosThetaT)) / ((etaT * cosThetaI) + (etaI * cosThetaT));
    float Rperp = ((etaI * cosThetaI) - (etaT * cosThetaT)) / ((etaI * cosThetaI) + (etaT * cosThetaT));
    return (Rparl * Rparl + Rperp * Rperp) / 2;
}
// TrowbridgeReitzDistribution with alphax == alphay == a, microfacet.cpp:155-184, microfacet.h:57-63
PG_DEV float tr_D(float a, V3 wh) {
    float tan2Theta = tan2_theta(wh);
    if (isinf(tan2Theta)) return 0.f;
    const float cos4Theta = cos2_theta(wh) * cos2_theta(wh);
    float e = (cos2_phi(wh) / (a * a) + sin2_phi(wh) / (a * a)) * tan2Theta;
    return 1 / (PG_PI * a * a * cos4Theta * (1 + e) * (1 + e));
}
PG_DEV float tr_lambda(float a, V3 w) {
    float absTanTheta = fabsf(tan_theta(w));
    if (isinf(absTanTheta)) return 0.f;
    float alpha = sqrtf(cos2_phi(w) * a * a + sin2_phi(w) * a * a);
    float alpha2Tan2Theta = (alpha * absTanTheta) * (alpha * absTanTheta);
    return (-1 + sqrtf(1.f + alpha2Tan2Theta)) / 2;
}
PG_DEV float tr_G1(float a, V3 w) { return 1 / (1 + tr_lambda(a, w)); }
PG_DEV float tr_G(float a, V3 wo, V3 wi) { return 1 / (1 + tr_lambda(a, wo) + tr_lambda(a, wi)); }
PG_DEV float tr_pdf(float a, V3 wo, V3 wh) { return tr_D(a, wh) * tr_G1(a, wo) * absdot(wo, wh) / fabsf(wo.z); }  // microfacet.cpp:339-345
// TrowbridgeReitzSample11 / TrowbridgeReitzSample / Sample_wh (visible area), microfacet.cpp:238-336.  The
// normal-incidence branch evaluates sqrt/cos/sin in double on float arguments, as the reference's source does.
PG_DEV void tr_sample11(float cosTheta, float U1, float U2, float &slope_x, float &slope_y) {
    if ((double)cosTheta > .9999) {
        float r = (float)sqrt((double)(U1 / (1 - U1)));
        float phi = (float)(6.28318530718 * (double)U2);
        double s, c;
        sincos((double)phi, &s, &c);
        slope_x = (float)((double)r * c);
        slope_y = (float)((double)r * s);
        return;
    }
    float sinTheta = sqrtf(pmax(0.f, 1.f - cosTheta * cosTheta));
    float tanTheta = sinTheta / cosTheta;
    float a = 1 / tanTheta;
    float G1 = 2 / (1 + sqrtf(1.f + 1.f / (a * a)));
    float A = 2 * U1 / G1 - 1;
    float tmp = 1.f / (A * A - 1.f);
    if (tmp > 1e10f) tmp = 1e10f;
    float B = tanTheta;
    float D = sqrtf(pmax(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.f));
    float slope_x_1 = B * tmp - D;
    float slope_x_2 = B * tmp + D;
    slope_x = (A < 0 || slope_x_2 > 1.f / tanTheta) ? slope_x_1 : slope_x_2;
    float S;
    if (U2 > 0.5f) { S = 1.f; U2 = 2.f * (U2 - .5f); }
    else { S = -1.f; U2 = 2.f * (.5f - U2); }
    float z = (U2 * (U2 * (U2 * 0.27385f - 0.73369f) + 0.46341f)) /
              (U2 * (U2 * (U2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
    slope_y = S * z * sqrtf(1.f + slope_x * slope_x);
}
PG_DEV V3 tr_sample_wh(float a, V3 wo, float u0, float u1) {
    const bool flip = wo.z < 0;
    V3 wi = flip ? -wo : wo;
    V3 wiStretched = normalize(mk(a * wi.x, a * wi.y, wi.z));
    float slope_x, slope_y;
    tr_sample11(wiStretched.z, u0, u1, slope_x, slope_y);
    float tmp = cos_phi(wiStretched) * slope_x - sin_phi(wiStretched) * slope_y;
    slope_y = sin_phi(wiStretched) * slope_x + cos_phi(wiStretched) * slope_y;
    slope_x = tmp;
    slope_x = a * slope_x;
    slope_y = a * slope_y;
    V3 wh = normalize(mk(-slope_x, -slope_y, 1.f));
    return flip ? -wh : wh;
}
// MicrofacetReflection::f / Pdf / Sample_f, reflection.cpp:226-238, :410-429 (local coordinates)
PG_DEV Spec mf_f(const Bsdf &b, V3 wo, V3 wi) {
    float cosThetaO = fabsf(wo.z), cosThetaI = fabsf(wi.z);
    V3 wh = wi + wo;
    if (cosThetaI == 0 || cosThetaO == 0) return sp(0);
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return sp(0);
    wh = normalize(wh);
    V3 whf = (dot(wh, mk(0, 0, 1)) < 0.f) ? -wh : wh;  // Faceforward
    Spec F = sp(fr_dielectric(dot(wi, whf), 1.5f, 1.f));  // FresnelDielectric(1.5f, 1.f)
    return (((b.Ks * tr_D(b.alpha, wh)) * tr_G(b.alpha, wo, wi)) * F) / (4 * cosThetaI * cosThetaO);
}
PG_DEV float mf_pdf(const Bsdf &b, V3 wo, V3 wi) {
    if (!(wo.z * wi.z > 0)) return 0;
    V3 wh = normalize(wo + wi);
    return tr_pdf(b.alpha, wo, wh) / (4 * dot(wo, wh));
}
PG_DEV void mf_sample(const Bsdf &b, V3 wo, V3 &wi, float u0, float u1, float &pdf) {  // leaves pdf = 0 when no sample
    if (wo.z == 0) return;
    V3 wh = tr_sample_wh(b.alpha, wo, u0, u1);
    if (dot(wo, wh) < 0) return;
    wi = -wo + wh * (2 * dot(wo, wh));  // Reflect, reflection.h:93-95
    if (!(wo.z * wi.z > 0)) return;
    pdf = tr_pdf(b.alpha, wo, wh) / (4 * dot(wo, wh));
}
PG_DEV float lambert_pdf(V3 wo, V3 wi) { return (wo.z * wi.z > 0) ? fabsf(wi.z) * PG_INVPI : 0; }  // reflection.cpp:392-394
// the diffuse lobe: LambertianReflection::f (reflection.cpp:178-180) or OrenNayar::f (:197-219)
PG_DEV Spec diffuse_f(const Bsdf &b, V3 wo, V3 wi) {
    if (!b.orenNayar) return b.R * PG_INVPI;
    float sinThetaI = sin_theta(wi), sinThetaO = sin_theta(wo);
    float maxCos = 0;
    if ((double)sinThetaI > 1e-4 && (double)sinThetaO > 1e-4) {
        float sinPhiI = sin_phi(wi), cosPhiI = cos_phi(wi);
        float sinPhiO = sin_phi(wo), cosPhiO = cos_phi(wo);
        float dCos = cosPhiI * cosPhiO + sinPhiI * sinPhiO;
        maxCos = pmax(0.f, dCos);
    }
    float sinAlpha, tanBeta;
    if (fabsf(wi.z) > fabsf(wo.z)) { sinAlpha = sinThetaO; tanBeta = sinThetaI / fabsf(wi.z); }
    else { sinAlpha = sinThetaI; tanBeta = sinThetaO / fabsf(wo.z); }
    return (b.R * PG_INVPI) * (b.onA + b.onB * maxCos * sinAlpha * tanBeta);
}
PG_DEV Spec bsdf_f_local(const Bsdf &b, V3 wo, V3 wi, bool reflect) {
    Spec f = sp(0);
    if (b.hasDiff && reflect) f = f + diffuse_f(b, wo, wi);
    if (b.hasSpec && reflect) f = f + mf_f(b, wo, wi);
    return f;
}
PG_DEV Spec bsdf_f(const Bsdf &b, V3 woW, V3 wiW) {  // reflection.cpp:680-693
    V3 wi = world_to_local(b, wiW), wo = world_to_local(b, woW);
    if (wo.z == 0) return sp(0);
    bool reflect = dot(wiW, b.ng) * dot(woW, b.ng) > 0;
    return bsdf_f_local(b, wo, wi, reflect);
}
PG_DEV float bsdf_pdf(const Bsdf &b, V3 woW, V3 wiW) {  // reflection.cpp:781-796
    if (b.nBxDFs == 0) return 0.f;
    V3 wo = world_to_local(b, woW), wi = world_to_local(b, wiW);
    if (wo.z == 0) return 0.f;
    float pdf = 0.f;
    if (b.hasDiff) pdf += lambert_pdf(wo, wi);
    if (b.hasSpec) pdf += mf_pdf(b, wo, wi);
    return pdf / b.nBxDFs;
}
// A BSDF whose only lobe is specular: SpecularReflection::Sample_f (reflection.cpp:136-143) or FresnelSpecular::Sample_f
// (:487-521) inside BSDF::Sample_f (:714-779).
PG_DEV Spec bsdf_sample_specular(const Bsdf &b, V3 woWorld, V3 &wiWorld, float u0, float &pdf, int &sampledType) {
    V3 wo = world_to_local(b, woWorld), wi;
    Spec f;
    pdf = 0; sampledType = 0;
    if (wo.z == 0) return sp(0);
    if (b.specular == 1) {
        wi = mk(-wo.x, -wo.y, wo.z);
        pdf = 1;
        f = (sp(1.f) * b.Kr) / fabsf(wi.z);
        sampledType = PG_BSDF_SPECULAR | PG_BSDF_REFLECTION;
    } else {
        const float ur = pmin(u0 * 1 - 0, PG_ONE_MINUS_EPS);
        const float F = fr_dielectric(wo.z, 1.f, b.eta);
        if (ur < F) {
            wi = mk(-wo.x, -wo.y, wo.z);
            sampledType = PG_BSDF_SPECULAR | PG_BSDF_REFLECTION;
            pdf = F;
            f = (b.Kr * F) / fabsf(wi.z);
        } else {
            const bool entering = wo.z > 0;
            const float etaI = entering ? 1.f : b.eta, etaT = entering ? b.eta : 1.f;
            const V3 n = (wo.z < 0.f) ? mk(0, 0, -1) : mk(0, 0, 1);  // Faceforward(Normal3f(0, 0, 1), wo)
            const float eta = etaI / etaT;
            // Refract, reflection.h:97-109
            const float cosThetaI = dot(n, wo);
            const float sin2ThetaI = pmax(0.f, 1 - cosThetaI * cosThetaI);
            const float sin2ThetaT = eta * eta * sin2ThetaI;
            if (sin2ThetaT >= 1) return sp(0);
            const float cosThetaT = sqrtf(1 - sin2ThetaT);
            wi = (-wo) * eta + n * (eta * cosThetaI - cosThetaT);
            Spec ft = b.Kt * (1 - F);
            ft = ft * ((etaI * etaI) / (etaT * etaT));  // TransportMode::Radiance
            sampledType = PG_BSDF_SPECULAR | PG_BSDF_TRANSMISSION;
            pdf = 1 - F;
            f = ft / fabsf(wi.z);
        }
    }
    if (pdf == 0) { sampledType = 0; return sp(0); }
    wiWorld = local_to_world(b, wi);
    return f;
}
PG_DEV Spec bsdf_sample_f(const Bsdf &b, V3 woWorld, V3 &wiWorld, float u0, float u1, float &pdf) {  // reflection.cpp:714-779
    int matchingComps = b.nBxDFs;
    pdf = 0;
    if (matchingComps == 0) return sp(0);
    int comp = (int)floorf(u0 * matchingComps);
    if (comp > matchingComps - 1) comp = matchingComps - 1;
    const bool useSpec = b.hasSpec && (comp == 1 || !b.hasDiff);  // lobe order: Lambertian, then microfacet
    float ur0 = pmin(u0 * matchingComps - comp, PG_ONE_MINUS_EPS);
    V3 wo = world_to_local(b, woWorld), wi = mk(0, 0, 0);
    if (wo.z == 0) return sp(0);
    if (useSpec) mf_sample(b, wo, wi, ur0, u1, pdf);
    else {  // BxDF::Sample_f, :383-390
        wi = cosine_sample_hemisphere(ur0, u1);
        if (wo.z < 0) wi.z *= -1;
        pdf = lambert_pdf(wo, wi);
    }
    if (pdf == 0) return sp(0);
    wiWorld = local_to_world(b, wi);
    if (matchingComps > 1) {
        pdf += useSpec ? lambert_pdf(wo, wi) : mf_pdf(b, wo, wi);
        pdf /= matchingComps;
    }
    bool reflect = dot(wiWorld, b.ng) * dot(woWorld, b.ng) > 0;
    return bsdf_f_local(b, wo, wi, reflect);
}

// Triangle::Sample(u, pdf) + Shape::Sample(ref, u, pdf) + DiffuseAreaLight::Sample_Li
// (triangle.cpp:582-607, shape.cpp:56-70, diffuse.cpp:68-81).
// ===========================================================================
// BSDF over a material's BxDF list (PgBxDF, include/pbrt_gpu.h): every BxDF of core/reflection.cpp the closed set of
// materials can add, and BSDF::f / Pdf / Sample_f over the list (reflection.cpp:680-796).  Used by the EXT kernels for
// every material; the specialised Bsdf above is the same arithmetic with the list shape of matte/plastic/mirror/glass
// baked in.
// ===========================================================================
#define PG_BSDF_DIFFUSE 4
#define PG_BSDF_GLOSSY 8
#define PG_BSDF_ALL 31
// `types`: the PgBxDFType of lobes[i] in bits 4i .. 4i+3, `scaled`: bit i = lobes[i] has ScaledBxDF wrappers -- read once when the
// list is bound (lbsdf_bind), so that BSDF::NumComponents / the component choice of Sample_f / the matching tests of f and Pdf are
// register arithmetic instead of a chain of dependent loads through the lane's list pointer
// LB: what a list is made of.  PgBxDF (120 B, the ABI's record: the scene's constant lists, the shading kernel's own copies) or PkLobe,
// the 48-B record k_material writes and k_shade<3> reads (pg_kernels.h) -- the same member NAMES over a type-dependent layout, so that
// lobe_f / lobe_pdf / lobe_sample_f / lobe_fresnel below are ONE text for both and read each field where it is used.  A MixMaterial's
// ScaledBxDF factors take a record of their own behind a PkLobe; all lobes of a hit have them or none has (the hit's material is a mix or
// it is not): recStride = 2 or 1 records per lobe.  (Round 5: the lists were up to 5 x 120 B + 32 B per textured hit, written by k_material
// and read back line by line -- 4.9 x the slot's algorithmic bytes at the L2s' memory side.)
template <class LB> struct LobeBsdfT { V3 ns, ng, ss, ts; const LB *lobes; int recStride; int n; float eta; unsigned types, scaled; };
typedef LobeBsdfT<PgBxDF> LobeBsdf;
PG_DEV int lobe_fresnel_kind(const PgBxDF &b) { return b.fresnel; }
PG_DEV int lobe_fresnel_kind(const PkLobe &b) { return (int)((b.hdr >> 4) & 3u); }
PG_DEV void lbsdf_bind(LobeBsdfT<PgBxDF> &b, const PgBxDF *lobes, int n, float eta) {
    b.lobes = lobes; b.recStride = 1; b.n = n; b.eta = eta; b.types = 0; b.scaled = 0;
    for (int i = 0; i < n; ++i) {
        b.types |= (unsigned)lobes[i].type << (4 * i);
        b.scaled |= (lobes[i].n_scales > 0 ? 1u : 0u) << i;
    }
}
PG_DEV void lbsdf_bind(LobeBsdfT<PkLobe> &b, const PkLobe *rec, int n, float eta, int recStride) {
    b.lobes = rec; b.recStride = recStride; b.n = n; b.eta = eta; b.types = 0; b.scaled = 0;
    for (int i = 0; i < n; ++i) {
        const unsigned hdr = rec[i * recStride].hdr;
        b.types |= (hdr & 15u) << (4 * i);
        b.scaled |= (((hdr >> 6) & 3u) > 0 ? 1u : 0u) << i;
    }
}
template <class LB> PG_DEV const LB &lobe_at(const LobeBsdfT<LB> &b, int i) { return b.lobes[i * b.recStride]; }
template <class LB> PG_DEV int lbsdf_lobe(const LobeBsdfT<LB> &b, int i) { return (int)((b.types >> (4 * i)) & 15u); }
template <class LB> PG_DEV V3 world_to_local(const LobeBsdfT<LB> &b, V3 v) { return mk(dot(v, b.ss), dot(v, b.ts), dot(v, b.ns)); }
template <class LB> PG_DEV V3 local_to_world(const LobeBsdfT<LB> &b, V3 v) {
    return mk(b.ss.x * v.x + b.ts.x * v.y + b.ns.x * v.z, b.ss.y * v.x + b.ts.y * v.y + b.ns.y * v.z,
              b.ss.z * v.x + b.ts.z * v.y + b.ns.z * v.z);
}
PG_DEV Spec operator-(Spec a, Spec b) { return sp3(a.r - b.r, a.g - b.g, a.b - b.b); }
PG_DEV Spec operator/(Spec a, Spec b) { return sp3(a.r / b.r, a.g / b.g, a.b / b.b); }
PG_DEV Spec sp_sqrt(Spec a) { return sp3(sqrtf(a.r), sqrtf(a.g), sqrtf(a.b)); }
PG_DEV Spec fr_conductor(float cosThetaI, Spec etai, Spec etat, Spec k) {  // reflection.cpp:71-96
    cosThetaI = clampf(cosThetaI, -1, 1);
    const Spec eta = etat / etai;
    const Spec etak = k / etai;
    const float cosThetaI2 = cosThetaI * cosThetaI;
    const float sinThetaI2 = 1.f - cosThetaI2;
    const Spec eta2 = eta * eta;
    const Spec etak2 = etak * etak;
    const Spec t0 = (eta2 - etak2) - sp(sinThetaI2);
    const Spec a2plusb2 = sp_sqrt(t0 * t0 + (eta2 * 4.f) * etak2);
    const Spec t1 = a2plusb2 + sp(cosThetaI2);
    const Spec a = sp_sqrt((a2plusb2 + t0) * 0.5f);
    const Spec t2 = a * (2.f * cosThetaI);
    const Spec Rs = (t1 - t2) / (t1 + t2);
    const Spec t3 = a2plusb2 * cosThetaI2 + sp(sinThetaI2 * sinThetaI2);
    const Spec t4 = t2 * sinThetaI2;
    const Spec Rp = (Rs * (t3 - t4)) / (t3 + t4);
    return (Rp + Rs) * 0.5f;
}
// TrowbridgeReitzDistribution(alphax, alphay), microfacet.cpp:155-184, :310-345
PG_DEV float tr2_D(float ax, float ay, V3 wh) {
    float tan2Theta = tan2_theta(wh);
    if (isinf(tan2Theta)) return 0.f;
    const float cos4Theta = cos2_theta(wh) * cos2_theta(wh);
    float e = (cos2_phi(wh) / (ax * ax) + sin2_phi(wh) / (ay * ay)) * tan2Theta;
    return 1 / (PG_PI * ax * ay * cos4Theta * (1 + e) * (1 + e));
}
PG_DEV float tr2_lambda(float ax, float ay, V3 w) {
    float absTanTheta = fabsf(tan_theta(w));
    if (isinf(absTanTheta)) return 0.f;
    float alpha = sqrtf(cos2_phi(w) * ax * ax + sin2_phi(w) * ay * ay);
    float alpha2Tan2Theta = (alpha * absTanTheta) * (alpha * absTanTheta);
    return (-1 + sqrtf(1.f + alpha2Tan2Theta)) / 2;
}
PG_DEV float tr2_G1(float ax, float ay, V3 w) { return 1 / (1 + tr2_lambda(ax, ay, w)); }
PG_DEV float tr2_G(float ax, float ay, V3 wo, V3 wi) { return 1 / (1 + tr2_lambda(ax, ay, wo) + tr2_lambda(ax, ay, wi)); }
PG_DEV float tr2_pdf(float ax, float ay, V3 wo, V3 wh) { return tr2_D(ax, ay, wh) * tr2_G1(ax, ay, wo) * absdot(wo, wh) / fabsf(wo.z); }
PG_DEV V3 tr2_sample_wh(float ax, float ay, V3 wo, float u0, float u1) {
    const bool flip = wo.z < 0;
    V3 wi = flip ? -wo : wo;
    V3 wiStretched = normalize(mk(ax * wi.x, ay * wi.y, wi.z));
    float slope_x, slope_y;
    tr_sample11(wiStretched.z, u0, u1, slope_x, slope_y);
    float tmp = cos_phi(wiStretched) * slope_x - sin_phi(wiStretched) * slope_y;
    slope_y = sin_phi(wiStretched) * slope_x + cos_phi(wiStretched) * slope_y;
    slope_x = tmp;
    slope_x = ax * slope_x;
    slope_y = ay * slope_y;
    V3 wh = normalize(mk(-slope_x, -slope_y, 1.f));
    return flip ? -wh : wh;
}
PG_DEV bool same_hemisphere(V3 w, V3 wp) { return w.z * wp.z > 0; }  // reflection.h:111-113
PG_DEV V3 reflect_about(V3 wo, V3 n) { return -wo + n * (2 * dot(wo, n)); }  // reflection.h:93-95
PG_DEV bool refract_dir(V3 wi, V3 n, float eta, V3 &wt) {  // reflection.h:97-109
    float cosThetaI = dot(n, wi);
    float sin2ThetaI = pmax(0.f, 1 - cosThetaI * cosThetaI);
    float sin2ThetaT = eta * eta * sin2ThetaI;
    if (sin2ThetaT >= 1) return false;
    float cosThetaT = sqrtf(1 - sin2ThetaT);
    wt = (-wi) * eta + n * (eta * cosThetaI - cosThetaT);
    return true;
}
PG_DEV int lobe_type(int type) {  // the BxDFType each constructor passes to BxDF()
    switch (type) {
    case PG_BXDF_LAMBERT_R: case PG_BXDF_OREN_NAYAR: return PG_BSDF_REFLECTION | PG_BSDF_DIFFUSE;
    case PG_BXDF_LAMBERT_T: return PG_BSDF_TRANSMISSION | PG_BSDF_DIFFUSE;
    case PG_BXDF_SPECULAR_R: return PG_BSDF_REFLECTION | PG_BSDF_SPECULAR;
    case PG_BXDF_SPECULAR_T: return PG_BSDF_TRANSMISSION | PG_BSDF_SPECULAR;
    case PG_BXDF_FRESNEL_SPECULAR: return PG_BSDF_REFLECTION | PG_BSDF_TRANSMISSION | PG_BSDF_SPECULAR;
    case PG_BXDF_MICROFACET_R: case PG_BXDF_FRESNEL_BLEND: return PG_BSDF_REFLECTION | PG_BSDF_GLOSSY;
    case PG_BXDF_MICROFACET_T: return PG_BSDF_TRANSMISSION | PG_BSDF_GLOSSY;
    }
    return 0;
}
PG_DEV bool lobe_matches(int lobe, int t) { const int type = lobe_type(lobe); return (type & t) == type; }  // reflection.h:225
template <class LB> PG_DEV Spec lobe_fresnel(const LB &b, float cosI) {  // Fresnel::Evaluate, reflection.cpp:120-135
    const int kind = lobe_fresnel_kind(b);
    if (kind == PG_FRESNEL_DIELECTRIC) return sp(fr_dielectric(cosI, b.eta_a, b.eta_b));
    if (kind == PG_FRESNEL_CONDUCTOR) return fr_conductor(fabsf(cosI), sp(1.f), sp_of(b.cond_eta), sp_of(b.cond_k));
    return sp(1.f);
}
PG_DEV float pow5f(float v) { return (v * v) * (v * v) * v; }
// IMP (here and in the functions below that hand it down): TransportMode::Importance, for the BSDF at a vertex of a light subpath -- pg_scatter_*_mode_at's
// kernel (pg_cameraimportance.h) alone instantiates it; every other caller leaves the default, TransportMode::Radiance.  The mode is read where
// reflection.cpp reads it: SpecularTransmission::Sample_f (:164), MicrofacetTransmission::f (:265) and FresnelSpecular::Sample_f (:514).  (bsdf_sample_specular
// above, the frames' specialised glass, is not reached by a query and stays Radiance.)
template <bool IMP = false, class LB> PG_DEV Spec lobe_f(const LB &b, int lobe, V3 wo, V3 wi) {  // BxDF::f of the wrapped BxDF (lobe = b.type), local frame
    const float ax = b.alpha_x, ay = b.alpha_y;
    switch (lobe) {
    case PG_BXDF_LAMBERT_R: return sp_of(b.R) * PG_INVPI;  // reflection.cpp:178-180
    case PG_BXDF_LAMBERT_T: return sp_of(b.T) * PG_INVPI;  // :188-190
    case PG_BXDF_OREN_NAYAR: {  // :197-219
        float sinThetaI = sin_theta(wi), sinThetaO = sin_theta(wo);
        float maxCos = 0;
        if (sinThetaI > 1e-4f && sinThetaO > 1e-4f) {
            float sinPhiI = sin_phi(wi), cosPhiI = cos_phi(wi);
            float sinPhiO = sin_phi(wo), cosPhiO = cos_phi(wo);
            float dCos = cosPhiI * cosPhiO + sinPhiI * sinPhiO;
            maxCos = pmax(0.f, dCos);
        }
        float sinAlpha, tanBeta;
        if (fabsf(wi.z) > fabsf(wo.z)) { sinAlpha = sinThetaO; tanBeta = sinThetaI / fabsf(wi.z); }
        else { sinAlpha = sinThetaI; tanBeta = sinThetaO / fabsf(wo.z); }
        return (sp_of(b.R) * PG_INVPI) * (b.on_a + b.on_b * maxCos * sinAlpha * tanBeta);
    }
    case PG_BXDF_MICROFACET_R: {  // :226-238
        float cosThetaO = fabsf(wo.z), cosThetaI = fabsf(wi.z);
        V3 wh = wi + wo;
        if (cosThetaI == 0 || cosThetaO == 0) return sp(0);
        if (wh.x == 0 && wh.y == 0 && wh.z == 0) return sp(0);
        wh = normalize(wh);
        V3 whf = (wh.z < 0.f) ? -wh : wh;  // Faceforward(wh, (0,0,1))
        Spec F = lobe_fresnel(b, dot(wi, whf));
        return (((sp_of(b.R) * tr2_D(ax, ay, wh)) * tr2_G(ax, ay, wo, wi)) * F) / (4 * cosThetaI * cosThetaO);
    }
    case PG_BXDF_MICROFACET_T: {  // :247-274
        if (same_hemisphere(wo, wi)) return sp(0);
        float cosThetaO = wo.z, cosThetaI = wi.z;
        if (cosThetaI == 0 || cosThetaO == 0) return sp(0);
        float eta = wo.z > 0 ? (b.eta_b / b.eta_a) : (b.eta_a / b.eta_b);
        V3 wh = normalize(wo + wi * eta);
        if (wh.z < 0) wh = -wh;
        if (dot(wo, wh) * dot(wi, wh) > 0) return sp(0);
        Spec F = sp(fr_dielectric(dot(wo, wh), b.eta_a, b.eta_b));
        float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
        float factor = IMP ? 1 : 1 / eta;  // (mode == TransportMode::Radiance) ? (1 / eta) : 1
        return ((sp(1.f) - F) * sp_of(b.T)) *
               fabsf(tr2_D(ax, ay, wh) * tr2_G(ax, ay, wo, wi) * eta * eta * absdot(wi, wh) * absdot(wo, wh) * factor * factor /
                     (cosThetaI * cosThetaO * sqrtDenom * sqrtDenom));
    }
    case PG_BXDF_FRESNEL_BLEND: {  // :295-310; Rd = R, Rs = T
        const Spec Rd = sp_of(b.R), Rs = sp_of(b.T);
        Spec diffuse = (((Rd * (28.f / (23.f * PG_PI))) * (sp(1.f) - Rs)) * (1 - pow5f(1 - .5f * fabsf(wi.z)))) * (1 - pow5f(1 - .5f * fabsf(wo.z)));
        V3 wh = wi + wo;
        if (wh.x == 0 && wh.y == 0 && wh.z == 0) return sp(0);
        wh = normalize(wh);
        Spec schlick = Rs + (sp(1.f) - Rs) * pow5f(1 - dot(wi, wh));  // SchlickFresnel, reflection.h:496-499
        Spec specular = schlick * (tr2_D(ax, ay, wh) / (4 * absdot(wi, wh) * pmax(fabsf(wi.z), fabsf(wo.z))));
        return diffuse + specular;
    }
    }
    return sp(0);  // specular BxDFs: f() = 0
}
template <class LB> PG_DEV float lobe_pdf(const LB &b, int lobe, V3 wo, V3 wi) {
    const float ax = b.alpha_x, ay = b.alpha_y;
    switch (lobe) {
    case PG_BXDF_LAMBERT_R: case PG_BXDF_OREN_NAYAR: return same_hemisphere(wo, wi) ? fabsf(wi.z) * PG_INVPI : 0;  // :392-394
    case PG_BXDF_LAMBERT_T: return !same_hemisphere(wo, wi) ? fabsf(wi.z) * PG_INVPI : 0;  // :405-408
    case PG_BXDF_MICROFACET_R: {  // :425-429
        if (!same_hemisphere(wo, wi)) return 0;
        V3 wh = normalize(wo + wi);
        return tr2_pdf(ax, ay, wo, wh) / (4 * dot(wo, wh));
    }
    case PG_BXDF_MICROFACET_T: {  // :444-458
        if (same_hemisphere(wo, wi)) return 0;
        float eta = wo.z > 0 ? (b.eta_b / b.eta_a) : (b.eta_a / b.eta_b);
        V3 wh = normalize(wo + wi * eta);
        if (dot(wo, wh) * dot(wi, wh) > 0) return 0;
        float sqrtDenom = dot(wo, wh) + eta * dot(wi, wh);
        float dwh_dwi = fabsf((eta * eta * dot(wi, wh)) / (sqrtDenom * sqrtDenom));
        return tr2_pdf(ax, ay, wo, wh) * dwh_dwi;
    }
    case PG_BXDF_FRESNEL_BLEND: {  // :480-485
        if (!same_hemisphere(wo, wi)) return 0;
        V3 wh = normalize(wo + wi);
        float pdf_wh = tr2_pdf(ax, ay, wo, wh);
        return .5f * (fabsf(wi.z) * PG_INVPI + pdf_wh / (4 * dot(wo, wh)));
    }
    }
    return 0;
}
// BxDF::Sample_f of the wrapped BxDF; pdf keeps the caller's 0 on the reference's early `return 0` paths.  wantF = false: the
// value of a NON-specular BxDF is not computed (0 is returned) -- BSDF::Sample_f throws it away and sums f() over all matching
// BxDFs instead (reflection.cpp:768-775); direction, pdf and the specular BxDFs' values are what they always are
template <bool IMP = false, class LB> PG_DEV Spec lobe_sample_f(const LB &b, int lobe, V3 wo, V3 &wi, float u0, float u1, float &pdf, int &sampledType, bool wantF = true) {
    const float ax = b.alpha_x, ay = b.alpha_y;
    switch (lobe) {
    case PG_BXDF_LAMBERT_R: case PG_BXDF_OREN_NAYAR:  // BxDF::Sample_f, :383-390
        wi = cosine_sample_hemisphere(u0, u1);
        if (wo.z < 0) wi.z *= -1;
        pdf = lobe_pdf(b, lobe, wo, wi);
        return wantF ? lobe_f<IMP>(b, lobe, wo, wi) : sp(0);
    case PG_BXDF_LAMBERT_T:  // :396-403
        wi = cosine_sample_hemisphere(u0, u1);
        if (wo.z > 0) wi.z *= -1;
        pdf = lobe_pdf(b, lobe, wo, wi);
        return wantF ? lobe_f<IMP>(b, lobe, wo, wi) : sp(0);
    case PG_BXDF_SPECULAR_R:  // :136-143
        wi = mk(-wo.x, -wo.y, wo.z);
        pdf = 1;
        return (lobe_fresnel(b, wi.z) * sp_of(b.R)) / fabsf(wi.z);
    case PG_BXDF_SPECULAR_T: {  // :151-167
        const bool entering = wo.z > 0;
        const float etaI = entering ? b.eta_a : b.eta_b, etaT = entering ? b.eta_b : b.eta_a;
        const V3 n = (wo.z < 0.f) ? mk(0, 0, -1) : mk(0, 0, 1);
        if (!refract_dir(wo, n, etaI / etaT, wi)) return sp(0);
        pdf = 1;
        Spec ft = sp_of(b.T) * (sp(1.f) - sp(fr_dielectric(wi.z, b.eta_a, b.eta_b)));
        if (!IMP) ft = ft * ((etaI * etaI) / (etaT * etaT));
        return ft / fabsf(wi.z);
    }
    case PG_BXDF_FRESNEL_SPECULAR: {  // :487-521
        const float F = fr_dielectric(wo.z, b.eta_a, b.eta_b);
        if (u0 < F) {
            wi = mk(-wo.x, -wo.y, wo.z);
            sampledType = PG_BSDF_SPECULAR | PG_BSDF_REFLECTION;
            pdf = F;
            return (sp_of(b.R) * F) / fabsf(wi.z);
        }
        const bool entering = wo.z > 0;
        const float etaI = entering ? b.eta_a : b.eta_b, etaT = entering ? b.eta_b : b.eta_a;
        const V3 n = (wo.z < 0.f) ? mk(0, 0, -1) : mk(0, 0, 1);
        if (!refract_dir(wo, n, etaI / etaT, wi)) return sp(0);
        Spec ft = sp_of(b.T) * (1 - F);
        if (!IMP) ft = ft * ((etaI * etaI) / (etaT * etaT));
        sampledType = PG_BSDF_SPECULAR | PG_BSDF_TRANSMISSION;
        pdf = 1 - F;
        return ft / fabsf(wi.z);
    }
    case PG_BXDF_MICROFACET_R: {  // :410-423
        if (wo.z == 0) return sp(0);
        V3 wh = tr2_sample_wh(ax, ay, wo, u0, u1);
        if (dot(wo, wh) < 0) return sp(0);
        wi = reflect_about(wo, wh);
        if (!same_hemisphere(wo, wi)) return sp(0);
        pdf = tr2_pdf(ax, ay, wo, wh) / (4 * dot(wo, wh));
        return wantF ? lobe_f<IMP>(b, lobe, wo, wi) : sp(0);
    }
    case PG_BXDF_MICROFACET_T: {  // :431-442
        if (wo.z == 0) return sp(0);
        V3 wh = tr2_sample_wh(ax, ay, wo, u0, u1);
        if (dot(wo, wh) < 0) return sp(0);
        float eta = wo.z > 0 ? (b.eta_a / b.eta_b) : (b.eta_b / b.eta_a);
        if (!refract_dir(wo, wh, eta, wi)) return sp(0);
        pdf = lobe_pdf(b, lobe, wo, wi);
        return wantF ? lobe_f<IMP>(b, lobe, wo, wi) : sp(0);
    }
    case PG_BXDF_FRESNEL_BLEND: {  // :460-478
        if ((double)u0 < .5) {
            u0 = pmin(2 * u0, PG_ONE_MINUS_EPS);
            wi = cosine_sample_hemisphere(u0, u1);
            if (wo.z < 0) wi.z *= -1;
        } else {
            u0 = pmin(2 * (u0 - .5f), PG_ONE_MINUS_EPS);
            V3 wh = tr2_sample_wh(ax, ay, wo, u0, u1);
            wi = reflect_about(wo, wh);
            if (!same_hemisphere(wo, wi)) return sp(0);
        }
        pdf = lobe_pdf(b, lobe, wo, wi);
        return wantF ? lobe_f<IMP>(b, lobe, wo, wi) : sp(0);
    }
    }
    return sp(0);
}
PG_DEV Spec lobe_scale(const PgBxDF &b, Spec f, int) {  // ScaledBxDF, reflection.cpp:98-107: innermost wrapper first
    for (int i = 0; i < b.n_scales; ++i) f = sp_of(b.scale[i]) * f;
    return f;
}
PG_DEV Spec lobe_scale(const PkLobe &b, Spec f, int recStride) {  // the factors: nine floats in the record behind the lobe's (half a lobe's stride on: a scaled list has two records per lobe)
    const float *sc = reinterpret_cast<const float *>(&b + (recStride >> 1));
    const int n = (int)((b.hdr >> 6) & 3u);
    for (int i = 0; i < n; ++i) f = sp_of(sc + 3 * i) * f;
    return f;
}
template <class LB> PG_DEV int lbsdf_num_components(const LobeBsdfT<LB> &b, int flags) {  // reflection.cpp:672-678
    int num = 0;
    for (int i = 0; i < b.n; ++i) if (lobe_matches(lbsdf_lobe(b, i), flags)) ++num;
    return num;
}
template <class LB> PG_DEV Spec lbsdf_scaled(const LobeBsdfT<LB> &b, int i, Spec f) {
    if (!((b.scaled >> i) & 1u)) return f;
    const auto &L = lobe_at(b, i);
    return lobe_scale(L, f, b.recStride);
}
// BxDF::f and BxDF::Pdf of one BxDF for the same pair of directions.  Each value is what lobe_f / lobe_pdf compute -- the same
// operations in the same order --, but the microfacet BxDFs' half vector, D(wh) and Lambda(wo) are computed once for both (a path
// vertex asks for f AND pdf of the other matching BxDFs inside both of its BSDF::Sample_f calls.  For the light's direction BSDF::f and
// BSDF::Pdf stay two walks: fused there as well the kernel gained nothing on microfacet scenes and lost 20 % on an all-Lambert one --
// a matter of what the register allocator makes of it, profiles/r04l_*).
template <bool IMP = false, class LB> PG_DEV void lobe_f_pdf(const LB &b, int lobe, V3 wo, V3 wi, bool wantF, bool wantPdf, Spec &f, float &pdf) {
    const float ax = b.alpha_x, ay = b.alpha_y;
    f = sp(0); pdf = 0;
    switch (lobe) {
    case PG_BXDF_MICROFACET_R: {  // reflection.cpp:226-238, :425-429
        V3 wh = wi + wo;  // (= wo + wi of Pdf: the same three sums)
        const bool whZero = wh.x == 0 && wh.y == 0 && wh.z == 0;
        wh = normalize(wh);
        const float D = tr2_D(ax, ay, wh), lambdaO = tr2_lambda(ax, ay, wo);
        if (wantPdf && same_hemisphere(wo, wi)) pdf = (D * (1 / (1 + lambdaO)) * absdot(wo, wh) / fabsf(wo.z)) / (4 * dot(wo, wh));
        if (wantF) {
            const float cosThetaO = fabsf(wo.z), cosThetaI = fabsf(wi.z);
            if (!(cosThetaI == 0 || cosThetaO == 0 || whZero)) {
                const V3 whf = (wh.z < 0.f) ? -wh : wh;  // Faceforward(wh, (0,0,1))
                const Spec F = lobe_fresnel(b, dot(wi, whf));
                f = (((sp_of(b.R) * D) * (1 / (1 + lambdaO + tr2_lambda(ax, ay, wi)))) * F) / (4 * cosThetaI * cosThetaO);
            }
        }
        return;
    }
    case PG_BXDF_FRESNEL_BLEND: {  // :295-310, :480-485
        V3 wh = wi + wo;
        const bool whZero = wh.x == 0 && wh.y == 0 && wh.z == 0;
        wh = normalize(wh);
        const float D = tr2_D(ax, ay, wh);
        if (wantPdf && same_hemisphere(wo, wi)) {
            const float pdf_wh = D * tr2_G1(ax, ay, wo) * absdot(wo, wh) / fabsf(wo.z);
            pdf = .5f * (fabsf(wi.z) * PG_INVPI + pdf_wh / (4 * dot(wo, wh)));
        }
        if (wantF && !whZero) {
            const Spec Rd = sp_of(b.R), Rs = sp_of(b.T);
            const Spec diffuse = (((Rd * (28.f / (23.f * PG_PI))) * (sp(1.f) - Rs)) * (1 - pow5f(1 - .5f * fabsf(wi.z)))) * (1 - pow5f(1 - .5f * fabsf(wo.z)));
            const Spec schlick = Rs + (sp(1.f) - Rs) * pow5f(1 - dot(wi, wh));
            f = diffuse + schlick * (D / (4 * absdot(wi, wh) * pmax(fabsf(wi.z), fabsf(wo.z))));
        }
        return;
    }
    }
    if (wantF) f = lobe_f<IMP>(b, lobe, wo, wi);
    if (wantPdf) pdf = lobe_pdf(b, lobe, wo, wi);
}
template <bool IMP = false, class LB> PG_DEV Spec lbsdf_f_local(const LobeBsdfT<LB> &b, V3 wo, V3 wi, bool reflect, int flags) {
    Spec f = sp(0);
    for (int i = 0; i < b.n; ++i) {
        const int lobe = lbsdf_lobe(b, i), type = lobe_type(lobe);
        if ((type & flags) == type && ((reflect && (type & PG_BSDF_REFLECTION)) || (!reflect && (type & PG_BSDF_TRANSMISSION))))
            { const auto &L = lobe_at(b, i); f = f + lbsdf_scaled(b, i, lobe_f<IMP>(L, lobe, wo, wi)); }
    }
    return f;
}
template <bool IMP = false, class LB> PG_DEV Spec lbsdf_f(const LobeBsdfT<LB> &b, V3 woW, V3 wiW, int flags) {  // reflection.cpp:680-693
    V3 wi = world_to_local(b, wiW), wo = world_to_local(b, woW);
    if (wo.z == 0) return sp(0);
    return lbsdf_f_local<IMP>(b, wo, wi, dot(wiW, b.ng) * dot(woW, b.ng) > 0, flags);
}
template <class LB> PG_DEV float lbsdf_pdf(const LobeBsdfT<LB> &b, V3 woW, V3 wiW, int flags) {  // reflection.cpp:781-796
    if (b.n == 0) return 0.f;
    V3 wo = world_to_local(b, woW), wi = world_to_local(b, wiW);
    if (wo.z == 0) return 0.f;
    float pdf = 0.f;
    int matchingComps = 0;
    for (int i = 0; i < b.n; ++i) {
        const int lobe = lbsdf_lobe(b, i);
        if (lobe_matches(lobe, flags)) { ++matchingComps; const auto &L = lobe_at(b, i); pdf += lobe_pdf(L, lobe, wo, wi); }
    }
    return matchingComps > 0 ? pdf / matchingComps : 0.f;
}
// BSDF::Sample_f, reflection.cpp:714-779: returns f, pdf = 0 when there is no sample
template <bool IMP = false, class LB> PG_DEV Spec lbsdf_sample_f(const LobeBsdfT<LB> &b, V3 woWorld, V3 &wiWorld, float u0, float u1, float &pdf, int flags, int &sampledType) {
    const int matchingComps = lbsdf_num_components(b, flags);
    sampledType = 0;
    pdf = 0;
    if (matchingComps == 0) return sp(0);
    int comp = (int)floorf(u0 * matchingComps);
    if (comp > matchingComps - 1) comp = matchingComps - 1;
    int chosen = 0, count = comp;
    for (int i = 0; i < b.n; ++i)
        if (lobe_matches(lbsdf_lobe(b, i), flags) && count-- == 0) { chosen = i; break; }
    const auto &bxdf = lobe_at(b, chosen);
    const int chosenLobe = lbsdf_lobe(b, chosen);
    const float uR0 = pmin(u0 * matchingComps - comp, PG_ONE_MINUS_EPS);
    V3 wi = mk(0, 0, 0), wo = world_to_local(b, woWorld);
    if (wo.z == 0) return sp(0);
    sampledType = lobe_type(chosenLobe);
    const bool bxdfSpecular = (sampledType & PG_BSDF_SPECULAR) != 0;
    Spec f = lbsdf_scaled(b, chosen, lobe_sample_f<IMP>(bxdf, chosenLobe, wo, wi, uR0, u1, pdf, sampledType, bxdfSpecular));
    if (pdf == 0) { sampledType = 0; return sp(0); }
    wiWorld = local_to_world(b, wi);
    if (!bxdfSpecular) {  // :760-775: the other matching BxDFs' pdfs, and f over all matching BxDFs of the hemisphere the pair is in
        const bool reflect = dot(wiWorld, b.ng) * dot(woWorld, b.ng) > 0;
        f = sp(0);
        for (int i = 0; i < b.n; ++i) {
            const int lobe = lbsdf_lobe(b, i), type = lobe_type(lobe);
            if ((type & flags) != type) continue;
            const bool wantPdf = matchingComps > 1 && i != chosen;
            const bool wantF = (reflect && (type & PG_BSDF_REFLECTION)) || (!reflect && (type & PG_BSDF_TRANSMISSION));
            if (!(wantPdf || wantF)) continue;
            Spec fi;
            float pi;
            { const auto &L = lobe_at(b, i); lobe_f_pdf<IMP>(L, lobe, wo, wi, wantF, wantPdf, fi, pi); }
            if (wantPdf) pdf += pi;
            if (wantF) f = f + lbsdf_scaled(b, i, fi);
        }
    }
    if (matchingComps > 1) pdf /= matchingComps;
    return f;
}

// The BSDF at a BSSRDF's exit point: one SeparableBSSRDFAdapter (bssrdf.h:209-225), a BxDF of type BSDF_REFLECTION | BSDF_DIFFUSE
// with f = Sw(wi) * eta^2 (TransportMode::Radiance) and BxDF's own cosine-hemisphere Sample_f / Pdf (reflection.cpp:383-394), under
// BSDF::f / ::Pdf / ::Sample_f (reflection.cpp:680-796) for a list of one.
struct AdapterBsdf { V3 ns, ng, ss, ts; float eta; };
PG_DEV V3 ad_to_local(const AdapterBsdf &b, V3 v) { return mk(dot(v, b.ss), dot(v, b.ts), dot(v, b.ns)); }
PG_DEV V3 ad_to_world(const AdapterBsdf &b, V3 v) {
    return mk(b.ss.x * v.x + b.ts.x * v.y + b.ns.x * v.z, b.ss.y * v.x + b.ts.y * v.y + b.ns.y * v.z, b.ss.z * v.x + b.ts.z * v.y + b.ns.z * v.z);
}
PG_DEV Spec ad_lobe_f(const AdapterBsdf &b, V3 wiLocal) { return sp(bssrdf_adapter_f(b.eta, wiLocal.z, fr_dielectric(wiLocal.z, 1, b.eta))); }
PG_DEV Spec ad_f(const AdapterBsdf &b, V3 woW, V3 wiW, int flags) {
    const V3 wi = ad_to_local(b, wiW), wo = ad_to_local(b, woW);
    if (wo.z == 0) return sp(0);
    const int type = PG_BSDF_REFLECTION | PG_BSDF_DIFFUSE;
    const bool reflect = dot(wiW, b.ng) * dot(woW, b.ng) > 0;
    return ((type & flags) == type && reflect) ? ad_lobe_f(b, wi) : sp(0);
}
PG_DEV float ad_pdf(const AdapterBsdf &b, V3 woW, V3 wiW, int flags) {
    const V3 wo = ad_to_local(b, woW), wi = ad_to_local(b, wiW);
    if (wo.z == 0) return 0.f;
    const int type = PG_BSDF_REFLECTION | PG_BSDF_DIFFUSE;
    if ((type & flags) != type) return 0.f;
    return same_hemisphere(wo, wi) ? fabsf(wi.z) * PG_INVPI : 0;
}
PG_DEV Spec ad_sample_f(const AdapterBsdf &b, V3 woW, V3 &wiW, float u0, float u1, float &pdf, int flags, int &sampledType) {
    const int type = PG_BSDF_REFLECTION | PG_BSDF_DIFFUSE;
    sampledType = 0;
    pdf = 0;
    if ((type & flags) != type) return sp(0);  // matchingComps == 0
    const float uR0 = pmin(u0 * 1 - 0, PG_ONE_MINUS_EPS);  // one matching component: comp = 0
    const V3 wo = ad_to_local(b, woW);
    if (wo.z == 0) return sp(0);
    sampledType = type;
    V3 wi = cosine_sample_hemisphere(uR0, u1);
    if (wo.z < 0) wi.z *= -1;
    pdf = same_hemisphere(wo, wi) ? fabsf(wi.z) * PG_INVPI : 0;
    if (pdf == 0) { sampledType = 0; return sp(0); }
    wiW = ad_to_world(b, wi);
    return (dot(wiW, b.ng) * dot(woW, b.ng) > 0) ? ad_lobe_f(b, wi) : sp(0);
}

// ---- the scattering model at EstimateDirect's reference point (pg_estimate.h), one overload set per model: f * |wi . ns| and the pdf of a given
// pair over the non-specular BxDFs (integrator.cpp:128-131 with bsdfFlags = BSDF_ALL & ~BSDF_SPECULAR), and Sample_f's direction with its f * |cos|
// and pdf (:170-174).  A model that samples nothing leaves wi as it came and pdf = 0.
#define PG_BSDF_NON_SPECULAR (PG_BSDF_ALL & ~PG_BSDF_SPECULAR)
template <class LB> PG_DEV Spec scatter_f_cos(const LobeBsdfT<LB> &b, V3 wo, V3 wi) { return lbsdf_f(b, wo, wi, PG_BSDF_NON_SPECULAR) * absdot(wi, b.ns); }
template <class LB> PG_DEV float scatter_pdf(const LobeBsdfT<LB> &b, V3 wo, V3 wi) { return lbsdf_pdf(b, wo, wi, PG_BSDF_NON_SPECULAR); }
template <class LB> PG_DEV Spec scatter_sample(const LobeBsdfT<LB> &b, V3 wo, V3 &wi, float u0, float u1, float &pdf) {
    int sampledType;
    const Spec f = lbsdf_sample_f(b, wo, wi, u0, u1, pdf, PG_BSDF_NON_SPECULAR, sampledType);
    return f * absdot(wi, b.ns);
}
PG_DEV Spec scatter_f_cos(const AdapterBsdf &b, V3 wo, V3 wi) { return ad_f(b, wo, wi, PG_BSDF_NON_SPECULAR) * absdot(wi, b.ns); }
PG_DEV float scatter_pdf(const AdapterBsdf &b, V3 wo, V3 wi) { return ad_pdf(b, wo, wi, PG_BSDF_NON_SPECULAR); }
PG_DEV Spec scatter_sample(const AdapterBsdf &b, V3 wo, V3 &wi, float u0, float u1, float &pdf) {
    int sampledType;
    const Spec f = ad_sample_f(b, wo, wi, u0, u1, pdf, PG_BSDF_NON_SPECULAR, sampledType);
    return f * absdot(wi, b.ns);
}

#endif  // PG_BXDF_H
