// pg_material.h -- Material::ComputeScatteringFunctions on the device: MatEval appends a material's BxDFs, textured parameters
// evaluated at the hit (pg_texture.h), to a raw PgBxDF array (LobeOutRaw) or to k_material's packed records (LobeOutPacked).
//
// Used by k_shade<2>, k_material (pg_kernels.hip), k_direct (pg_direct.h) and k_scatter (pg_scatter.h).
#ifndef PG_MATERIAL_H
#define PG_MATERIAL_H
#include "pg_bxdf.h"
#include "pg_texture.h"

PG_DEV Spec sp_clamp0(Spec v) { return sp3(v.r < 0 ? 0 : v.r, v.g < 0 ? 0 : v.g, v.b < 0 ? 0 : v.b); }  // Spectrum::Clamp()
PG_DEV void lobe_init(PgBxDF &b, int type) {
    b.type = type; b.fresnel = PG_FRESNEL_NOOP; b.eta_a = b.eta_b = 1; b.alpha_x = b.alpha_y = 1; b.on_a = 1; b.on_b = 0; b.n_scales = 0;
    for (int i = 0; i < 3; ++i) { b.R[i] = b.T[i] = b.cond_eta[i] = b.cond_k[i] = 0; }
}
PG_DEV void lobe_set(float *dst, Spec v) { dst[0] = v.r; dst[1] = v.g; dst[2] = v.b; }
PG_DEV float roughness_to_alpha(float roughness) {  // microfacet.h:127-132; std::log evaluated in double, rounded once
    roughness = pmax(roughness, 1e-3f);
    const float x = pg_logf(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}
PG_DEV void lobe_tr(PgBxDF &b, float ax, float ay) { b.alpha_x = pmax(0.001f, ax); b.alpha_y = pmax(0.001f, ay); }  // microfacet.h:109-113
// Material::ComputeScatteringFunctions of material `mat` at this hit (materials/): appends its BxDFs to out[n...]; eta receives
// BSDF::eta.  D bounds the nesting of mix materials; cap = the room in out[] (PG_MAX_BXDFS, or the scene's largest list when the
// list goes to k_material's buffer).
// Where MatEval puts a BxDF list: an array of PgBxDFs (the shading kernel's own, MODE 2) or k_material's packed records (LobeBsdfT)
struct LobeOutRaw {
    PgBxDF *p;
    PG_DEV void put(int i, const PgBxDF &b) const { p[i] = b; }
    PG_DEV void add_scale(int i, Spec s) const { if (p[i].n_scales < PG_MAX_BXDF_SCALES) { lobe_set(p[i].scale[p[i].n_scales], s); p[i].n_scales++; } }
};
struct LobeOutPacked {
    float4 *rec;    // record 0 of this thread's list; record r lies r planes on (MatPre)
    int recStride;  // 2: the hit's material is a mix, every lobe is followed by the record of its scale factors
    int plane;      // records per plane = the queue's entries
    PG_DEV void put(int i, const PgBxDF &b) const {
        float4 *q = rec + 3 * ((size_t)(i * recStride) * plane);
        pg_pack_lobe(b, reinterpret_cast<float *>(q));
        if (recStride == 2) pg_pack_lobe_scales(b, reinterpret_cast<float *>(q + 3 * (size_t)plane));
    }
    PG_DEV void add_scale(int i, Spec s) const {  // ScaledBxDF around lobe i (mixmat.cpp:60-65): the next free factor of its scale record
        float4 *q = rec + 3 * ((size_t)(i * recStride) * plane);
        const unsigned hdr = __float_as_uint(q[0].x), ns = (hdr >> 6) & 3u;
        if (ns < PG_MAX_BXDF_SCALES) {
            float *f = reinterpret_cast<float *>(q + 3 * (size_t)plane) + 3 * ns;
            f[0] = s.r; f[1] = s.g; f[2] = s.b;
            q[0].x = __uint_as_float(hdr + (1u << 6));
        }
    }
};
template <int D, int W = 0, class OUT = LobeOutRaw> struct MatEval {
    static PG_DEV_CALL void run(const DScene &sc, int mat, const TexHit &h, OUT out, int &n, float &eta, int capArg) {
        const int cap = W == 0 ? PG_MAX_BXDFS : capArg;  // (the shading kernel's own copies: a constant, no register held for it)
        const PgMaterial &m = sc.materials[mat];
        if (m.type != PG_MAT_TEXTURED) {  // constant parameters: the list the host built
            for (int i = 0; i < m.n_bxdfs && n < cap; ++i) out.put(n++, sc.bxdfs[m.first_bxdf + i]);
            eta = m.bsdf_eta;
            return;
        }
        const PgTexturedMaterial &tm = sc.textured[m.textured_index];
        auto TS = [&](int i) { return TexEval<PG_TEX_DEPTH, W>::s(sc, tm.s[i], h); };
        auto TF = [&](int i) { return TexEval<PG_TEX_DEPTH, W>::f(sc, tm.f[i], h); };
        auto push = [&](const PgBxDF &b) { if (n < cap) out.put(n++, b); };
        PgBxDF b;
        eta = 1;
        switch (tm.kind) {
        case PG_KIND_MATTE: {  // matte.cpp:45-62
            const Spec r = sp_clamp0(TS(0));
            const float sig = clampf(TF(0), 0, 90);
            if (!is_black(r)) {
                lobe_init(b, sig == 0 ? PG_BXDF_LAMBERT_R : PG_BXDF_OREN_NAYAR);
                lobe_set(b.R, r);
                if (sig != 0) {
                    const float sigma = (PG_PI / 180) * sig, sigma2 = sigma * sigma;
                    b.on_a = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
                    b.on_b = 0.45f * sigma2 / (sigma2 + 0.09f);
                }
                push(b);
            }
            break;
        }
        case PG_KIND_PLASTIC: {  // plastic.cpp:45-70
            const Spec kd = sp_clamp0(TS(0));
            if (!is_black(kd)) { lobe_init(b, PG_BXDF_LAMBERT_R); lobe_set(b.R, kd); push(b); }
            const Spec ks = sp_clamp0(TS(1));
            if (!is_black(ks)) {
                lobe_init(b, PG_BXDF_MICROFACET_R); lobe_set(b.R, ks);
                b.fresnel = PG_FRESNEL_DIELECTRIC; b.eta_a = 1.5f; b.eta_b = 1.f;
                float rough = TF(0);
                if (tm.remap_roughness) rough = roughness_to_alpha(rough);
                lobe_tr(b, rough, rough);
                push(b);
            }
            break;
        }
        case PG_KIND_MIRROR: {  // mirror.cpp:44-56
            const Spec R = sp_clamp0(TS(0));
            if (!is_black(R)) { lobe_init(b, PG_BXDF_SPECULAR_R); lobe_set(b.R, R); push(b); }
            break;
        }
        case PG_KIND_GLASS: {  // glass.cpp:45-96
            const float e = TF(2);
            float urough = TF(0), vrough = TF(1);
            const Spec R = sp_clamp0(TS(0)), T = sp_clamp0(TS(1));
            eta = e;
            if (is_black(R) && is_black(T)) break;
            if (urough == 0 && vrough == 0) { lobe_init(b, PG_BXDF_FRESNEL_SPECULAR); lobe_set(b.R, R); lobe_set(b.T, T); b.eta_a = 1.f; b.eta_b = e; push(b); }
            else {
                if (tm.remap_roughness) { urough = roughness_to_alpha(urough); vrough = roughness_to_alpha(vrough); }
                if (!is_black(R)) { lobe_init(b, PG_BXDF_MICROFACET_R); lobe_set(b.R, R); b.fresnel = PG_FRESNEL_DIELECTRIC; b.eta_a = 1.f; b.eta_b = e; lobe_tr(b, urough, vrough); push(b); }
                if (!is_black(T)) { lobe_init(b, PG_BXDF_MICROFACET_T); lobe_set(b.T, T); b.eta_a = 1.f; b.eta_b = e; lobe_tr(b, urough, vrough); push(b); }
            }
            break;
        }
        case PG_KIND_UBER: {  // uber.cpp:45-101
            const float e = TF(3);
            const Spec op = sp_clamp0(TS(4));
            const Spec t = sp_clamp0(op * -1.f + sp(1.f));
            if (!is_black(t)) { lobe_init(b, PG_BXDF_SPECULAR_T); lobe_set(b.T, t); push(b); eta = 1.f; }
            else eta = e;
            const Spec kd = op * sp_clamp0(TS(0));
            if (!is_black(kd)) { lobe_init(b, PG_BXDF_LAMBERT_R); lobe_set(b.R, kd); push(b); }
            const Spec ks = op * sp_clamp0(TS(1));
            if (!is_black(ks)) {
                float roughu = tm.has_u ? TF(1) : TF(0);
                float roughv = tm.has_v ? TF(2) : roughu;
                if (tm.remap_roughness) { roughu = roughness_to_alpha(roughu); roughv = roughness_to_alpha(roughv); }
                lobe_init(b, PG_BXDF_MICROFACET_R); lobe_set(b.R, ks); b.fresnel = PG_FRESNEL_DIELECTRIC; b.eta_a = 1.f; b.eta_b = e; lobe_tr(b, roughu, roughv);
                push(b);
            }
            const Spec kr = op * sp_clamp0(TS(2));
            if (!is_black(kr)) { lobe_init(b, PG_BXDF_SPECULAR_R); lobe_set(b.R, kr); b.fresnel = PG_FRESNEL_DIELECTRIC; b.eta_a = 1.f; b.eta_b = e; push(b); }
            const Spec kt = op * sp_clamp0(TS(3));
            if (!is_black(kt)) { lobe_init(b, PG_BXDF_SPECULAR_T); lobe_set(b.T, kt); b.eta_a = 1.f; b.eta_b = e; push(b); }
            break;
        }
        case PG_KIND_METAL: {  // metal.cpp:61-82
            float uRough = tm.has_u ? TF(1) : TF(0);
            float vRough = tm.has_v ? TF(2) : TF(0);
            if (tm.remap_roughness) { uRough = roughness_to_alpha(uRough); vRough = roughness_to_alpha(vRough); }
            lobe_init(b, PG_BXDF_MICROFACET_R);
            lobe_set(b.R, sp(1.f));
            b.fresnel = PG_FRESNEL_CONDUCTOR;
            lobe_set(b.cond_eta, TS(0)); lobe_set(b.cond_k, TS(1));
            lobe_tr(b, uRough, vRough);
            push(b);
            break;
        }
        case PG_KIND_SUBSTRATE: {  // substrate.cpp:45-65
            const Spec d = sp_clamp0(TS(0)), s2 = sp_clamp0(TS(1));
            float roughu = TF(0), roughv = TF(1);
            if (!is_black(d) || !is_black(s2)) {
                if (tm.remap_roughness) { roughu = roughness_to_alpha(roughu); roughv = roughness_to_alpha(roughv); }
                lobe_init(b, PG_BXDF_FRESNEL_BLEND); lobe_set(b.R, d); lobe_set(b.T, s2); lobe_tr(b, roughu, roughv); push(b);
            }
            break;
        }
        case PG_KIND_TRANSLUCENT: {  // translucent.cpp:45-80
            const float e = 1.5f;
            eta = e;
            const Spec r = sp_clamp0(TS(2)), t = sp_clamp0(TS(3));
            if (is_black(r) && is_black(t)) break;
            const Spec kd = sp_clamp0(TS(0));
            if (!is_black(kd)) {
                if (!is_black(r)) { lobe_init(b, PG_BXDF_LAMBERT_R); lobe_set(b.R, r * kd); push(b); }
                if (!is_black(t)) { lobe_init(b, PG_BXDF_LAMBERT_T); lobe_set(b.T, t * kd); push(b); }
            }
            const Spec ks = sp_clamp0(TS(1));
            if (!is_black(ks) && (!is_black(r) || !is_black(t))) {
                float rough = TF(0);
                if (tm.remap_roughness) rough = roughness_to_alpha(rough);
                if (!is_black(r)) { lobe_init(b, PG_BXDF_MICROFACET_R); lobe_set(b.R, r * ks); b.fresnel = PG_FRESNEL_DIELECTRIC; b.eta_a = 1.f; b.eta_b = e; lobe_tr(b, rough, rough); push(b); }
                if (!is_black(t)) { lobe_init(b, PG_BXDF_MICROFACET_T); lobe_set(b.T, t * ks); b.eta_a = 1.f; b.eta_b = e; lobe_tr(b, rough, rough); push(b); }
            }
            break;
        }
        case PG_KIND_MIX: {  // mixmat.cpp:45-65
            const Spec s1 = sp_clamp0(TS(0));
            const Spec s2 = sp_clamp0(sp(1.f) - s1);
            for (int j = 0; j < 2; ++j) {
                const int first = n;
                float subEta = 1;
                MatEval<D - 1, W, OUT>::run(sc, tm.sub[j], h, out, n, subEta, cap);
                if (j == 0) eta = subEta;  // si->bsdf stays m1's
                const Spec scl = j == 0 ? s1 : s2;
                for (int i = first; i < n; ++i) out.add_scale(i, scl);
            }
            break;
        }
        }
    }
};
template <int W, class OUT> struct MatEval<0, W, OUT> {  // below the deepest mix the host allows: only constant-parameter materials
    static PG_DEV void run(const DScene &sc, int mat, const TexHit &, OUT out, int &n, float &eta, int capArg) {
        const int cap = W == 0 ? PG_MAX_BXDFS : capArg;
        const PgMaterial &m = sc.materials[mat];
        for (int i = 0; i < m.n_bxdfs && n < cap; ++i) out.put(n++, sc.bxdfs[m.first_bxdf + i]);
        eta = m.bsdf_eta;
    }
};

#endif  // PG_MATERIAL_H
