// TEST INFRASTRUCTURE: one input's worth of the scattering models EstimateDirect is written over (pbrt-v3_amd/csrc/pg_estimate.h) -- AdapterBsdf's
// f / pdf / sample_f with its scatter_* overloads, HgPhase's overloads, russian_roulette -- as PG_DEV functions over plain arrays, so that the host
// build (tests/device_headers_host.hip) and the device probe (tests/device_probe.hip) run the very same text.  Included after pg_bxdf.h, pg_medium.h
// and pg_sampler.h.
#ifndef SCATTER_PROBE_H
#define SCATTER_PROBE_H

#define SCATTER_ADAPTER_IN 21   // ss, ts, ns, ng (12), eta, wo (3), wi (3), u0, u1
#define SCATTER_ADAPTER_OUT 23  // ad_f rgb, ad_pdf | ad_sample_f rgb, pdf, wi, type | scatter_f_cos rgb, scatter_pdf | scatter_sample rgb, pdf, wi
PG_DEV void probe_adapter_bsdf(const float *in, int flags, float *out) {
    AdapterBsdf b;
    b.ss = mk(in[0], in[1], in[2]); b.ts = mk(in[3], in[4], in[5]); b.ns = mk(in[6], in[7], in[8]); b.ng = mk(in[9], in[10], in[11]);
    b.eta = in[12];
    const V3 wo = mk(in[13], in[14], in[15]), wi = mk(in[16], in[17], in[18]);
    const float u0 = in[19], u1 = in[20];
    const Spec f = ad_f(b, wo, wi, flags);
    out[0] = f.r; out[1] = f.g; out[2] = f.b; out[3] = ad_pdf(b, wo, wi, flags);
    V3 ws = wi;  // (left in place when nothing is sampled)
    float pdf = -1;
    int type = -1;
    const Spec sf = ad_sample_f(b, wo, ws, u0, u1, pdf, flags, type);
    out[4] = sf.r; out[5] = sf.g; out[6] = sf.b; out[7] = pdf; out[8] = ws.x; out[9] = ws.y; out[10] = ws.z; out[11] = (float)type;
    const Spec fc = scatter_f_cos(b, wo, wi);
    out[12] = fc.r; out[13] = fc.g; out[14] = fc.b; out[15] = scatter_pdf(b, wo, wi);
    V3 w2 = wi;
    float pdf2 = -1;
    const Spec s2 = scatter_sample(b, wo, w2, u0, u1, pdf2);
    out[16] = s2.r; out[17] = s2.g; out[18] = s2.b; out[19] = pdf2; out[20] = w2.x; out[21] = w2.y; out[22] = w2.z;
}

#define SCATTER_HG_IN 9    // g, wo (3), wi (3), u0, u1
#define SCATTER_HG_OUT 11  // scatter_f_cos rgb, scatter_pdf | scatter_sample rgb, pdf, wi
PG_DEV void probe_hg_phase(const float *in, float *out) {
    const HgPhase m = {in[0]};
    const V3 wo = mk(in[1], in[2], in[3]), wi = mk(in[4], in[5], in[6]);
    const Spec f = scatter_f_cos(m, wo, wi);
    out[0] = f.r; out[1] = f.g; out[2] = f.b; out[3] = scatter_pdf(m, wo, wi);
    V3 w2 = mk(0, 0, 0);
    float pdf = -1;
    const Spec s = scatter_sample(m, wo, w2, in[7], in[8], pdf);
    out[4] = s.r; out[5] = s.g; out[6] = s.b; out[7] = pdf; out[8] = w2.x; out[9] = w2.y; out[10] = w2.z;
}

#define SCATTER_RR_IN 6   // beta (3), etaScale, rrThreshold, the number a draw returns
#define SCATTER_RR_OUT 5  // beta afterwards (3), numbers drawn, survived
PG_DEV void probe_russian_roulette(const float *in, int bounces, float *out) {
    Spec beta = sp3(in[0], in[1], in[2]);
    int drawn = 0;
    const float u = in[5];
    const bool alive = russian_roulette(beta, in[3], bounces, in[4], [&]() -> float { ++drawn; return u; });
    out[0] = beta.r; out[1] = beta.g; out[2] = beta.b; out[3] = (float)drawn; out[4] = alive ? 1.f : 0.f;
}
#endif
