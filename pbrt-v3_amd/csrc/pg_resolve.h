// pg_resolve.h -- what becomes of EstimateDirect once its rays are back: the two "Add ... contribution" sums (integrator.cpp:143-161, 196-212),
// L += beta * Ld / lightPdf (integrator.cpp:104, path.cpp:122-126, volpath.cpp:124-127) and DirectLightingIntegrator's divisions (integrator.cpp:80, 104)
// as device functions, with the record a vertex leaves for them between its shading kernel and the kernel that finishes it.
//
// The record lies in PathState's pdLight / pdBeta / pdMis / pdInfo and, under volpath, VolState's pdLi / trAcc / misLi / p1[0].w.  Its writers (k_shade's
// surface and medium vertices, k_sss_exit, k_direct) go through the *_encode functions, its readers (resolve_entry of k_resolve / k_resolve_list,
// k_resolve_vol, k_through) through the decoders: each takes or returns the array's word, so that a caller still loads and stores only where it did.
// The sums are float operations in the reference's order (-ffp-contract=off: nothing fused, nothing re-associated).  No HIP call, no DScene: what needs
// one (the emitter's Le along the MIS ray) stays with the caller.  Pinned on the host (tests/test_device_headers_on_host.py) and on the device
// (tests/test_gpu_device_arithmetic.py) through tests/resolve_probe.h.
#ifndef PG_RESOLVE_H
#define PG_RESOLVE_H
#include "pg_device.h"
#include "pg_kernels.h"

// ---- the record --------------------------------------------------------------------------------------------------------------------------
// pdInfo: where the vertex's two rays lie in their queues (-1: none left), the light UniformSampleOneLight chose (-1: none was asked for, -2: the scene
// has none), and `where`: the place of the path's L -- >= 0 its position in the next queue's state, < 0 ~slot (the path ended).  Without queue-order
// state (k_resolve_vol<false>: L by slot) `where` holds the bits of volpath's light weight instead.
struct PendingInfo { int posShadow, posMis, lightNum, where; };
PG_DEV PendingInfo pending_info(int4 w) { return PendingInfo{w.x, w.y, w.z, w.w}; }
PG_DEV PendingInfo pending_nothing() { return PendingInfo{-1, -1, -1, 0}; }
PG_DEV bool pending_any(const PendingInfo &p) { return !(p.posShadow < 0 && p.posMis < 0); }  // (else Ld == 0: L += beta * 0 leaves L as it is)
PG_DEV int pending_where(bool pushNext, int posNext, int slot) { return pushNext ? posNext : ~slot; }
PG_DEV int pending_where_weight(float volLightWeight) { return __float_as_int(volLightWeight); }  // (read back by vol_light_weight<false>)
PG_DEV int4 pending_info_encode(int posShadow, int posMis, int lightNum, int where) { return make_int4(posShadow, posMis, lightNum, where); }
PG_DEV float4 *pending_L(const PathState &st, const QueueState &qsNext, int where) { return where >= 0 ? &qsNext.L[where] : &st.L[~where]; }

// pdLight: the light sample's term and the pdf the light was chosen with (integrator.cpp:93-104).  The term is Ld's first summand with unoccluded
// visibility, f * |cos| * Li * weight / lightPdf (direct_light_folded), under path and directlighting; f * |cos| alone under volpath, whose Li still
// is to be multiplied by the shadow ray's transmittance (VolLight)
struct PendingLight { Spec term; float lightSelectPdf; };
PG_DEV PendingLight pending_light(float4 w) { return PendingLight{sp3(w.x, w.y, w.z), w.w}; }
PG_DEV float4 pending_light_encode(Spec term, float lightSelectPdf) { return make_float4(term.r, term.g, term.b, lightSelectPdf); }
// pdBeta: the path throughput the estimate is scaled by, and the MIS weight of the scattering-sampled direction (integrator.cpp:191-192)
struct PendingBeta { Spec beta; float misWeight; };
PG_DEV PendingBeta pending_beta(float4 w) { return PendingBeta{sp3(w.x, w.y, w.z), w.w}; }
PG_DEV float4 pending_beta_encode(Spec beta, float misWeight) { return make_float4(beta.r, beta.g, beta.b, misWeight); }
PG_DEV float pending_mis_weight(float scatteringPdf, float lightPdf) { return power_heuristic(1, scatteringPdf, 1, lightPdf); }
// pdMis: f * |cos| and pdf of the scattering-sampled direction (written for the vertices with a MIS ray only)
struct PendingMis { Spec f; float pdf; };
PG_DEV PendingMis pending_mis(float4 w) { return PendingMis{sp3(w.x, w.y, w.z), w.w}; }
PG_DEV float4 pending_mis_encode(Spec f, float pdf) { return make_float4(f.r, f.g, f.b, pdf); }

// volpath (handleMedia): pdLi = the light sample's Li and pdf; trAcc[kind] = a through ray's transmittance so far and the medium it is in (kind 0 the shadow
// ray, 1 the MIS ray); misLi = the sampled light's radiance along the finished MIS ray; the light sample's MIS weight -- negative: a delta light, which
// takes none (integrator.cpp:155-160) -- waits in p1[0].w with queue-order state and in pdInfo.w without
struct VolLight { Spec Li; float lightPdf; };
PG_DEV VolLight vol_light(float4 w) { return VolLight{sp3(w.x, w.y, w.z), w.w}; }
PG_DEV float4 vol_light_encode(Spec Li, float lightPdf) { return make_float4(Li.r, Li.g, Li.b, lightPdf); }
struct Through { Spec Tr; int medium; };
PG_DEV Through through_acc(float4 w) { return Through{sp3(w.x, w.y, w.z), __float_as_int(w.w)}; }
PG_DEV float4 through_acc_encode(Spec Tr, int medium) { return make_float4(Tr.r, Tr.g, Tr.b, __int_as_float(medium)); }
PG_DEV float4 through_acc_start(int medium) { return through_acc_encode(sp(1.f), medium); }
PG_DEV Spec vol_mis_li(float4 w) { return sp3(w.x, w.y, w.z); }
PG_DEV float4 vol_mis_li_encode(Spec Li) { return make_float4(Li.r, Li.g, Li.b, 0); }
PG_DEV float vol_light_weight_of(bool isDelta, float lightPdf, float scatteringPdf) { return isDelta ? -1.f : power_heuristic(1, lightPdf, 1, scatteringPdf); }
template <bool QS>
PG_DEV float vol_light_weight(const VolState &vs, int pdi, const PendingInfo &info) { return QS ? vs.p1[0][pdi].w : __int_as_float(info.where); }

// ---- the sums ----------------------------------------------------------------------------------------------------------------------------
// "Add light's contribution to reflected radiance", integrator.cpp:143-161, with the folded term: unless the shadow ray was blocked
PG_DEV Spec ld_add_light(Spec Ld, Spec term, bool occluded) { return occluded ? Ld : Ld + term; }
// The same with handleMedia: Li *= visibility.Tr (integrator.cpp:146-150), then f * Li / lightPdf for a delta light and f * Li * weight / lightPdf
// otherwise (:155-160).  weight(): called only for a light that arrives (its word is loaded only then)
template <class Weight>
PG_DEV Spec ld_add_vol_light(Spec Ld, Spec f, Spec Li, Spec Tr, float lightPdf, Weight weight) {
    Li = Li * Tr;
    if (is_black(Li)) return Ld;
    const float w = weight();
    return Ld + (w < 0 ? (f * Li) / lightPdf : ((f * Li) * w) / lightPdf);
}
// "Add light contribution from material sampling", integrator.cpp:196-212: Ld += f * Li * Tr * weight / scatteringPdf when the ray met the sampled
// light.  Tr: the MIS ray's transmittance; path has Spectrum(1.f) there and multiplies by it as the reference does
PG_DEV Spec ld_add_mis(Spec Ld, Spec f, Spec Li, Spec Tr, float weight, float scatteringPdf) {
    if (is_black(Li)) return Ld;
    return Ld + ((((f * Li) * Tr) * weight) / scatteringPdf);
}
// beta * (EstimateDirect(...) / lightPdf), integrator.cpp:104 under path.cpp:122-126: the addend, which "Zero-radiance paths" asks about
PG_DEV Spec direct_addend(Spec beta, Spec Ld, float lightSelectPdf) { return beta * (Ld / lightSelectPdf); }
// L += the addend; L's fourth word (the film position) stays
PG_DEV float4 direct_add_to_L(float4 L4, Spec add) {
    const Spec L = sp3(L4.x, L4.y, L4.z) + add;
    return make_float4(L.r, L.g, L.b, L4.w);
}
// QueueState::pend of a vertex with a shadow ray and no MIS ray: the addend under "not occluded", which the next vertex's k_shade adds once the any-hit
// launch has said so -- the two functions resolve_entry calls, so that the list path and the full-queue pass add the same bits
PG_DEV Spec direct_pend(const PendingLight &pl, const PendingBeta &pb) { return direct_addend(pb.beta, ld_add_light(sp(0), pl.term, false), pl.lightSelectPdf); }
// directlighting: dst += src / divisor -- `L += Ld / nSamples` (integrator.cpp:80), `EstimateDirect(...) / lightPdf` (integrator.cpp:104) and
// `L += UniformSample...Lights(...)` (directlighting.cpp:84-89, divisor 1).  A division, as the reference's Spectrum::operator/(Float) is
PG_DEV float4 direct_fold(float4 dst, float4 src, float divisor) { return make_float4(dst.x + src.x / divisor, dst.y + src.y / divisor, dst.z + src.z / divisor, dst.w); }
// path.cpp:119-126: a vertex for which a light was chosen is one of totalPaths (bit 0), and one of zeroRadiancePaths (bit 1) when its addend is black
PG_DEV int resolve_path_counts(int lightNum, bool addendBlack) { return lightNum == -1 ? 0 : (addendBlack ? 3 : 1); }

#endif  // PG_RESOLVE_H
