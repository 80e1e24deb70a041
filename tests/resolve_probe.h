// TEST INFRASTRUCTURE: one vertex's worth of EstimateDirect's pending terms and sums (pbrt-v3_amd/csrc/pg_resolve.h) as PG_DEV functions over plain
// arrays, so that the host build (tests/device_headers_host.hip) and the device probe (tests/device_probe.hip) run the very same text.  Included after
// pg_resolve.h.  probe_resolve_path is resolve_entry (pg_kernels.hip) and probe_resolve_vol is k_resolve_vol with their loads replaced by the row: the calls
// and their order are the kernels'.  What resolve_entry needs a DScene for -- the radiance the MIS ray met -- is an input here.
#ifndef RESOLVE_PROBE_H
#define RESOLVE_PROBE_H

PG_DEV float4 probe_f4(const float *p) { return make_float4(p[0], p[1], p[2], p[3]); }
PG_DEV void probe_put4(float *p, float4 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
PG_DEV void probe_put3(float *p, Spec v) { p[0] = v.r; p[1] = v.g; p[2] = v.b; }
// L of two next-queue entries and of two slots, as the row holds them (8 + 8 floats), behind the structures pending_L looks into
struct ProbeL {
    float4 q[2], s[2];
    PathState st;
    QueueState qs;
    PG_DEV explicit ProbeL(const float *in) : st{}, qs{} {
        for (int k = 0; k < 2; ++k) { q[k] = probe_f4(in + 4 * k); s[k] = probe_f4(in + 8 + 4 * k); }
        st.L = s; qs.L = q;
    }
    PG_DEV void put(float *out) const { for (int k = 0; k < 2; ++k) { probe_put4(out + 4 * k, q[k]); probe_put4(out + 8 + 4 * k, s[k]); } }
};

#define RESOLVE_PATH_IN 31    // pdLight, pdBeta, pdMis (4 each) | the sampled light's radiance along the MIS ray (3) | L of next-queue entries 0, 1 and of slots 0, 1 (16)
#define RESOLVE_PATH_IIN 5    // pdInfo: posShadow, posMis, lightNum, where | occluded[posShadow]
#define RESOLVE_PATH_OUT 22   // the 16 L words afterwards | the addend (0 where nothing is pending) | direct_pend of the record
#define RESOLVE_PATH_IOUT 1   // resolve_path_counts
PG_DEV void probe_resolve_path(const float *in, const int *iin, float *out, int *iout) {
    ProbeL Ls(in + 15);
    const PendingInfo info = pending_info(make_int4(iin[0], iin[1], iin[2], iin[3]));
    const PendingLight pl = pending_light(probe_f4(in));
    const PendingBeta pb = pending_beta(probe_f4(in + 4));
    bool black = true;
    Spec add = sp(0);
    if (pending_any(info)) {
        Spec Ld = sp(0);
        if (info.posShadow >= 0) Ld = ld_add_light(Ld, pl.term, iin[4] != 0);
        if (info.posMis >= 0) {
            const PendingMis pm = pending_mis(probe_f4(in + 8));
            Ld = ld_add_mis(Ld, pm.f, sp3(in[12], in[13], in[14]), sp(1.f), pb.misWeight, pm.pdf);
        }
        float4 *Lp = pending_L(Ls.st, Ls.qs, info.where);
        add = direct_addend(pb.beta, Ld, pl.lightSelectPdf);
        black = is_black(add);
        *Lp = direct_add_to_L(*Lp, add);
    }
    Ls.put(out);
    probe_put3(out + 16, add);
    probe_put3(out + 19, direct_pend(pl, pb));
    iout[0] = resolve_path_counts(info.lightNum, black);
}

#define RESOLVE_VOL_IN 48   // pdLight, pdBeta, pdMis, pdLi, trAcc[0], trAcc[1], misLi, p1[0] (4 each) | the 16 L words as above
#define RESOLVE_VOL_IIN 6   // pdInfo: posShadow, posMis, lightNum, where (QS) or the light weight's bits | QS | the slot L lives in without QS
#define RESOLVE_VOL_OUT 16  // the 16 L words afterwards
template <bool QS>
PG_DEV void probe_resolve_vol_qs(const float *in, const int *iin, float *out) {
    ProbeL Ls(in + 32);
    float4 p10 = probe_f4(in + 28);
    VolState vs{};
    vs.p1[0] = &p10;
    const PendingInfo info = pending_info(make_int4(iin[0], iin[1], iin[2], iin[3]));
    if (pending_any(info)) {
        const PendingLight pl = pending_light(probe_f4(in));
        const PendingBeta pb = pending_beta(probe_f4(in + 4));
        const PendingMis pm = pending_mis(probe_f4(in + 8));
        Spec Ld = sp(0);
        if (info.posShadow >= 0) {
            const VolLight li = vol_light(probe_f4(in + 12));
            Ld = ld_add_vol_light(Ld, pl.term, li.Li, through_acc(probe_f4(in + 16)).Tr, li.lightPdf, [&]() { return vol_light_weight<QS>(vs, 0, info); });
        }
        if (info.posMis >= 0) Ld = ld_add_mis(Ld, pm.f, vol_mis_li(probe_f4(in + 24)), through_acc(probe_f4(in + 20)).Tr, pb.misWeight, pm.pdf);
        float4 *Lp = QS ? pending_L(Ls.st, Ls.qs, info.where) : &Ls.s[iin[5]];
        *Lp = direct_add_to_L(*Lp, direct_addend(pb.beta, Ld, pl.lightSelectPdf));
    }
    Ls.put(out);
}
PG_DEV void probe_resolve_vol(const float *in, const int *iin, float *out) {
    if (iin[4]) probe_resolve_vol_qs<true>(in, iin, out);
    else probe_resolve_vol_qs<false>(in, iin, out);
}

#define RESOLVE_FOLD_IN 9  // dst (4), src (4), divisor
PG_DEV void probe_direct_fold(const float *in, float *out) { probe_put4(out, direct_fold(probe_f4(in), probe_f4(in + 4), in[8])); }

// Every field through its encoder and back through its decoder
#define RESOLVE_RT_IN 24    // term (3), lightSelectPdf | beta (3), misWeight | f (3), pdf | Li (3), lightPdf | Tr (3) | misLi (3) | scatteringPdf, the light weight
#define RESOLVE_RT_IIN 8    // posShadow, posMis, lightNum, pushNext, posNext, slot (0 or 1 each), medium, isDelta
#define RESOLVE_RT_OUT 28   // the 24 decoded | pending_mis_weight(pdf, lightPdf) | vol_light_weight_of(isDelta, lightPdf, scatteringPdf) | the light weight read with QS, without
#define RESOLVE_RT_IOUT 8   // posShadow, posMis, lightNum, where | pending_any | medium | through_acc_start's medium | the L pending_L names: k = next-queue entry k, ~k = slot k
PG_DEV void probe_resolve_roundtrip(const float *in, const int *iin, float *out, int *iout) {
    const PendingLight pl = pending_light(pending_light_encode(sp3(in[0], in[1], in[2]), in[3]));
    const PendingBeta pb = pending_beta(pending_beta_encode(sp3(in[4], in[5], in[6]), in[7]));
    const PendingMis pm = pending_mis(pending_mis_encode(sp3(in[8], in[9], in[10]), in[11]));
    const VolLight vl = vol_light(vol_light_encode(sp3(in[12], in[13], in[14]), in[15]));
    const Through th = through_acc(through_acc_encode(sp3(in[16], in[17], in[18]), iin[6]));
    const Spec ml = vol_mis_li(vol_mis_li_encode(sp3(in[19], in[20], in[21])));
    probe_put3(out, pl.term); out[3] = pl.lightSelectPdf;
    probe_put3(out + 4, pb.beta); out[7] = pb.misWeight;
    probe_put3(out + 8, pm.f); out[11] = pm.pdf;
    probe_put3(out + 12, vl.Li); out[15] = vl.lightPdf;
    probe_put3(out + 16, th.Tr);
    probe_put3(out + 19, ml);
    out[22] = in[22]; out[23] = in[23];
    out[24] = pending_mis_weight(in[11], in[15]);
    out[25] = vol_light_weight_of(iin[7] != 0, in[15], in[22]);
    float4 p10 = make_float4(0, 0, 0, in[23]);
    VolState vs{};
    vs.p1[0] = &p10;
    const PendingInfo byWeight = pending_info(pending_info_encode(iin[0], iin[1], iin[2], pending_where_weight(in[23])));
    out[26] = vol_light_weight<true>(vs, 0, byWeight);
    out[27] = vol_light_weight<false>(vs, 0, byWeight);
    const PendingInfo info = pending_info(pending_info_encode(iin[0], iin[1], iin[2], pending_where(iin[3] != 0, iin[4], iin[5])));
    iout[0] = info.posShadow; iout[1] = info.posMis; iout[2] = info.lightNum; iout[3] = info.where;
    iout[4] = pending_any(info) ? 1 : 0;
    iout[5] = th.medium;
    const Through start = through_acc(through_acc_start(iin[6]));
    iout[6] = (start.Tr.r == 1.f && start.Tr.g == 1.f && start.Tr.b == 1.f) ? start.medium : ~start.medium;
    const float zero[16] = {};
    ProbeL Ls(zero);
    const float4 *Lp = pending_L(Ls.st, Ls.qs, info.where);
    iout[7] = (Lp == &Ls.q[0] || Lp == &Ls.q[1]) ? (int)(Lp - Ls.q) : ~(int)(Lp - Ls.s);
}
#endif
