// pg_scatter.h -- the kernel of the scattering queries (pg_scatter_f_at / pg_scatter_sample_at, pg_abi.hip's rayQuery): the BSDF at a ray's closest
// hit as PathIntegrator::Li sees it after isect.ComputeScatteringFunctions(ray, arena, true) -- TransportMode::Radiance, allowMultipleLobes, a ray
// without differentials -- evaluated for a given wi (BSDF::f and BSDF::Pdf) or sampled (BSDF::Sample_f), for an integrator whose Li stays on the host.
// Included at the end of pg_kernels.hip, like pg_interaction.h, whose k_pack_rays filled the queue this kernel walks (ray i is entry i).
//
// The kernel is wiring: the interaction is hit_isect's, what textures read of it tex_hit_setup's, Material::Bump material_bump's, the BxDF list
// MatEval's or the material's own, and BSDF::f / Pdf / Sample_f are lbsdf_f / lbsdf_pdf / lbsdf_sample_f -- the functions k_direct calls, in k_direct's
// order.  A subsurface material's BSDF is reported here, its BSSRDF by pg_subsurfacequery.h; TransportMode::Importance is k_scatter_importance's (pg_cameraimportance.h).
#ifndef PG_SCATTER_H
#define PG_SCATTER_H

// No frame stands behind a ray query: tex_hit_setup is handed a zeroed description and a `meta` whose PG_META_HASDIFF is clear, under which it reads
// nothing of the description, of a PathState or of the queue (ComputeDifferentials' early-out: every texture footprint is zero).
__device__ const PgRenderDesc pg_scatter_no_frame = {};

// PgScatter of every entry of q after its closest-hit launch (hits, sc.hitInst / sc.animXf as k_interaction finds them): one thread per ray, the
// 64-byte record as four float4 stores -- two lanes fill one 128-B line.  `in`: three floats per ray (wi, world space, used as given) or, for
// SAMPLE, two (the Point2f of BSDF::Sample_f); `flags`: the call's BxDFType mask.
template <bool TEX, bool SAMPLE>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_scatter(DScene sc, RayQueue q, const float4 *__restrict__ hits, const float *__restrict__ in, int flags,
                                                             float4 *__restrict__ out) {
    const int i = queue_item<PG_SHADE_BLOCK>(q);
    if (i < 0) return;
    const float4 o4 = q.o[i], d4 = q.d[i], h4 = hits[i];
    const int prim = __float_as_int(h4.x);
    float4 rec[4];
    for (int k = 0; k < 4; ++k) rec[k] = make_float4(0, 0, 0, 0);
    rec[0].x = __int_as_float(prim);
    if (prim >= 0) {
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const Tri tri = load_tri(sc, prim);
        const PgMaterial mtl = sc.materials[tri.material];
        if (mtl.type != PG_MAT_NONE) {  // (a medium boundary has no BSDF: the record stays prim and zeros)
            int inst = sc.hitInst ? sc.hitInst[i] : -1, inst2;
            nest_decode(sc, inst, inst2);
            const InstXf outer = inst_xf(sc, inst, i), inner = inst_xf(sc, inst2, i, true);
            QuadricUv quv;
            Isect is = hit_isect(sc, outer, inner, o4, rayD, h4, prim, tri, quv);
            // ---- the BSDF: a material's BxDF list, or (TEX) ComputeScatteringFunctions with textures
            LobeBsdfT<PgBxDF> lb;
            PgBxDF lobeStore[TEX ? PG_MAX_BXDFS : 1];
            if constexpr (TEX) {
                TexHit th;
                tex_hit_setup(sc, pg_scatter_no_frame, q, i, 0, prim, tri, h4, rayD, outer, inner, quv, is, make_int4(0, 0, 0, 0), 0.f, 0.f, false, false, 0, th, nullptr);
                material_bump(sc, tri.material, th, is);
                int nl = 0;
                float etaL = 1;
                MatEval<2>::run(*sc.self, tri.material, th, LobeOutRaw{lobeStore}, nl, etaL, PG_MAX_BXDFS);
                lbsdf_bind(lb, lobeStore, nl, etaL);
            } else lbsdf_bind(lb, sc.bxdfs + mtl.first_bxdf, mtl.n_bxdfs, mtl.bsdf_eta);
            lb.ns = is.ns; lb.ng = is.n;  // the BSDF's frame (reflection.h:167-172), of the shading geometry as Material::Bump left it
            lb.ss = normalize(is.sdpdu);
            lb.ts = cross(lb.ns, lb.ss);
            Spec f;
            V3 wi = mk(0, 0, 0);
            float pdf;
            int sampledType = 0;
            if constexpr (SAMPLE) {
                f = lbsdf_sample_f(lb, is.wo, wi, in[2 * (size_t)i], in[2 * (size_t)i + 1], pdf, flags, sampledType);
                if (pdf == 0) { f = sp(0); wi = mk(0, 0, 0); sampledType = 0; }
            } else {
                const size_t k = 3 * (size_t)i;
                wi = mk(in[k], in[k + 1], in[k + 2]);
                f = lbsdf_f(lb, is.wo, wi, flags);
                pdf = lbsdf_pdf(lb, is.wo, wi, flags);
            }
            rec[0].y = __int_as_float(lb.n); rec[0].z = __int_as_float(lbsdf_num_components(lb, flags)); rec[0].w = __int_as_float(sampledType);
            rec[1] = make_float4(f.r, f.g, f.b, pdf);
            rec[2] = make_float4(wi.x, wi.y, wi.z, lb.eta);
            rec[3] = make_float4(lb.ns.x, lb.ns.y, lb.ns.z, __uint_as_float(lb.types));
        }
    }
    float4 *dst = out + 4 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = rec[k];
}
void launch_scatter(const DScene &sc, RayQueue q, const float4 *hits, const float *in, bool sample, int flags, PgScatter *out, hipStream_t s) {
    static_assert(sizeof(PgScatter) == 4 * sizeof(float4), "PgScatter is four float4");
    const int nblk = PG_REGIONS * (q.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    float4 *o4 = reinterpret_cast<float4 *>(out);
    const bool tex = sc.hasTextured || sc.hasNest;  // as launch_direct chooses k_direct's mode
    if (tex && sample) hipLaunchKernelGGL((k_scatter<true, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, o4);
    else if (tex) hipLaunchKernelGGL((k_scatter<true, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, o4);
    else if (sample) hipLaunchKernelGGL((k_scatter<false, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, o4);
    else hipLaunchKernelGGL((k_scatter<false, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, o4);
}
#endif
