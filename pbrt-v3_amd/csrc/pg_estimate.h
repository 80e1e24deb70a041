// pg_estimate.h -- EstimateDirect's set-up (integrator.cpp:108-215, up to the two rays) as device functions, once for every kernel that shades a
// vertex: the light sample with the scattering model's f * |cos| and pdf for it, and the scattering-sampled direction that becomes the MIS ray.
// The scattering model is whatever has the three overloads scatter_f_cos / scatter_pdf / scatter_sample: LobeBsdfT<.>, AdapterBsdf (pg_bxdf.h) or
// HgPhase (pg_medium.h).  The factors come back apart, as volpath needs them (Li still is to be multiplied by the shadow ray's transmittance);
// direct_light_folded is path's and directlighting's product of them.
//
// What stays with the caller, because it differs per kernel: the choice of the light, the draws, where the rays and the pending terms are kept
// (shadow_ray_to and spawn_ray write them), and WHEN light.Pdf_Li of the sampled direction runs (mis_light_pdf, with what DirectMis names).
//
// Used by k_sss_exit (pg_kernels.hip) and k_direct (pg_direct.h).  k_shade's two vertices keep statements of their own that mirror these, in two halves
// with its register relief between them: every form of the call cost its VOL instantiations registers they do not have (CHANGELOG.md).  EXT as in
// light_sample_li: false leaves the infinite light out.  Included after pg_hit.h.
#ifndef PG_ESTIMATE_H
#define PG_ESTIMATE_H
#include "pg_bxdf.h"
#include "pg_light.h"
#include "pg_medium.h"
#include "pg_hit.h"
#include "pg_resolve.h"

// The light half (integrator.cpp:116-162).  shadow: a shadow ray leaves -- towards ls, to be weighted by what follows; f: f * |wi . ns| (a phase function's p)
struct DirectLight { bool shadow, isDelta; Spec f, Li; float lightPdf, scatteringPdf; V3 wi; LightSample ls; };
// The scattering-sampled half (integrator.cpp:164-212, up to light.Pdf_Li).  cand: the direction wi with f (* |cos|) and pdf is a candidate for the MIS ray;
// (lightPrim, area, inside): what mis_light_pdf asks of the light, for this reference point
struct DirectMis { bool cand, inside; V3 wi; Spec f; float pdf; int lightPrim; float area; };
struct DirectSetup { DirectLight light; DirectMis mis; };

template <bool EXT, class M>
PG_DEV DirectLight direct_light_half(const DScene &sc, const M &m, const LightHot &lh, int lightNum, V3 p, V3 pError, V3 n, V3 wo, float u0, float u1) {
    DirectLight d;
    d.shadow = false;
    d.isDelta = PG_LIGHT_IS_DELTA(lh.type);  // delta lights take no MIS weight (integrator.cpp:155-160)
    d.f = sp(0);
    d.lightPdf = d.scatteringPdf = 0;
    d.wi = mk(0, 0, 0);
    d.Li = light_sample_li_hot<EXT>(sc, lh, sc.lights[lightNum], p, pError, n, u0, u1, d.wi, d.lightPdf, d.ls);
    if (d.lightPdf > 0 && !is_black(d.Li)) {
        d.f = scatter_f_cos(m, wo, d.wi);
        d.scatteringPdf = scatter_pdf(m, wo, d.wi);
        d.shadow = !is_black(d.f);
    }
    return d;
}
// (wiLight: the light half's direction, which a model that samples nothing leaves in place)
template <bool EXT, class M>
PG_DEV DirectMis direct_scatter_half(const DScene &sc, const M &m, const LightHot &lh, int lightNum, V3 p, V3 pError, V3 n, V3 wo, V3 wiLight, float u0, float u1) {
    DirectMis d;
    d.cand = d.inside = false;
    d.wi = wiLight;
    d.f = sp(0);
    d.pdf = 0;
    d.lightPrim = 0;
    d.area = 1;
    if (lh.type == PG_LIGHT_AREA || (EXT && lh.type == PG_LIGHT_INFINITE))  // integrator.cpp:164: if (!IsDeltaLight(light.flags))
        d.f = scatter_sample(m, wo, d.wi, u0, u1, d.pdf);
    if (!is_black(d.f) && d.pdf > 0) {
        d.cand = true;
        d.area = lh.area;
        mis_light_of(sc, lh, lightNum, p, pError, n, d.lightPrim, d.inside);
    }
    return d;
}
// Both halves for the reference point (p, pError, n, wo) and light lightNum; (uL0, uL1) = uLight, (uS0, uS1) = uScattering
template <bool EXT, class M>
PG_DEV DirectSetup estimate_direct_setup(const DScene &sc, const M &m, V3 p, V3 pError, V3 n, V3 wo, int lightNum, float uL0, float uL1, float uS0, float uS1) {
    const LightHot lh = load_light_hot(sc, lightNum);
    DirectSetup s;
    s.light = direct_light_half<EXT>(sc, m, lh, lightNum, p, pError, n, wo, uL0, uL1);
    s.mis = direct_scatter_half<EXT>(sc, m, lh, lightNum, p, pError, n, wo, s.light.wi, uS0, uS1);
    return s;
}

// The light sample's MIS weight as volpath keeps it beside the factors (-1: a delta light) ...
PG_DEV float direct_light_weight(const DirectLight &d) { return vol_light_weight_of(d.isDelta, d.lightPdf, d.scatteringPdf); }
// ... and Ld's first term with unoccluded visibility, integrator.cpp:155-160
PG_DEV Spec direct_light_folded(const DirectLight &d) {
    const Spec f = d.f, Li = d.Li;
    const float lightPdf = d.lightPdf, scatteringPdf = d.scatteringPdf;
    return d.isDelta ? (f * Li) / lightPdf : ((f * Li) * power_heuristic(1, lightPdf, 1, scatteringPdf)) / lightPdf;
}
// volpath: a vertex's light sample waits for its transmittance ray (k_through, k_resolve_vol) by pdi -- Li and the pdf, the sample the ray is heading
// to, the weight (read from here with queue-order state, from pdInfo.w without), and the medium the ray starts in.  Returns the weight.
PG_DEV float store_vol_light_sample(const VolState &vs, int pdi, const DirectLight &d, int medium) {
    const float w = direct_light_weight(d);
    vs.pdLi[pdi] = vol_light_encode(d.Li, d.lightPdf);
    vs.p1[0][pdi] = make_float4(d.ls.p.x, d.ls.p.y, d.ls.p.z, w);
    vs.p1[1][pdi] = make_float4(d.ls.pError.x, d.ls.pError.y, d.ls.pError.z, 0);
    vs.p1[2][pdi] = make_float4(d.ls.n.x, d.ls.n.y, d.ls.n.z, 0);
    vs.trAcc[0][pdi] = through_acc_start(medium);
    return w;
}

#endif  // PG_ESTIMATE_H
