// pg_subsurfacequery.h -- the kernels of the subsurface queries (pg_subsurface_sample_at / pg_subsurface_f_at / pg_subsurface_sample_f_at, pg_abi.hip's
// subsurfaceQuery and adapterQuery): the BSSRDF branch of PathIntegrator::Li / VolPathIntegrator::Li (path.cpp:152-174, volpath.cpp:151-176) for an
// integrator whose Li stays on the host -- isect.bssrdf at a ray's closest hit po, BSSRDF::Sample_S (bssrdf.cpp:238-251, Sample_Sp :253-328) down to
// the exit point pi with S and its pdf, and BSDF::f / Pdf / Sample_f of the one SeparableBSSRDFAdapter Sample_S installs at pi.  Included at the end of
// pg_kernels.hip, like pg_mediumquery.h, whose wave_append the seed kernel uses.
//
// The kernels are wiring around the renderer's own pieces: k_sss_seed is k_scatter's way to the bound BSDF, then k_shade<., ., SSS>'s BSSRDF block
// (stated once more below as bssrdf_coefficients_at: the shading kernels keep their own text) and bssrdf_probe_segment; the
// chain between seed and emit is sssProbeChains' loop over the existing k_sss_probe, with the SssState indexed by ray number; k_sss_emit is
// k_sss_exit's head (hit_isect of the chosen hit, bssrdf_pdf_sp, bssrdf_sr, prim_interface); k_adapter calls ad_f / ad_pdf / ad_sample_f.
// One thread per ray or job, PG_SHADE_BLOCK threads per block; no kernel here declares __shared__ memory.  (k_sss_seed's code object still reports
// 10240 B of static LDS, 80 B per lane: the compiler places the per-lane sigma_t / rho and spline-weight arrays of bssrdf_probe_segment, indexed by
// the sampled channel, in LDS instead of scratch, as it does in k_sss_exit -- DESIGN.md "Subsurface queries".)  Not tuned or timed.
#ifndef PG_SUBSURFACEQUERY_H
#define PG_SUBSURFACEQUERY_H

// si->bssrdf of a hit on `material` whose BSDF holds nBxdfs BxDFs (subsurface.cpp:87-90, kdsubsurface.cpp:88-93): the bssrdfs[] index or -1, and
// TabulatedBSSRDF's sigma_t / rho there -- the table's own, or (TEX, a textured material) derived from the textures at the hit as the constructor
// does.  k_shade<., ., SSS>'s block (pg_kernels.hip), statement for statement; th is read under TEX only.
template <bool TEX>
PG_DEV int bssrdf_coefficients_at(const DScene &sc, int material, int nBxdfs, const TexHit *th, float sigT[3], float rho[3]) {
    int sssIdx = sc.nBssrdfs > 0 ? sc.materialBssrdf[material] : -1;
    if (sssIdx < 0) return -1;
    const PgBSSRDF &bd = sc.bssrdfs[sssIdx];
    for (int c = 0; c < 3; ++c) { sigT[c] = bd.sigma_t[c]; rho[c] = bd.rho[c]; }
    if (bd.textured) {
        if (nBxdfs == 0) sssIdx = -1;  // ComputeScatteringFunctions returned before it set the BSSRDF (R and T both black)
        else if constexpr (TEX) {
            const Spec ta = sp_clamp0(TexEval<PG_TEX_DEPTH>::s(*sc.self, bd.a, *th)), tb = sp_clamp0(TexEval<PG_TEX_DEPTH>::s(*sc.self, bd.b, *th));
            const float a3[3] = {ta.r, ta.g, ta.b}, b3[3] = {tb.r, tb.g, tb.b};
            const DBssrdf tbl = bssrdf_bind(bd, sc.bssrdfTables);
            for (int c = 0; c < 3; ++c) {
                float sa, ssc;
                if (bd.textured == 1) { sa = a3[c] * bd.scale; ssc = b3[c] * bd.scale; }  // subsurface.cpp:87-88
                else {  // SubsurfaceFromDiffuse(table, Kd, scale * mfp), bssrdf.cpp:182-191
                    const float mfree = b3[c] * bd.scale;
                    const float r = invert_catmull_rom(tbl.nRho, tbl.rhoSamples, tbl.rhoEff, a3[c]);
                    ssc = r / mfree; sa = (1 - r) / mfree;
                }
                sigT[c] = sa + ssc;  // TabulatedBSSRDF's constructor, bssrdf.h:146-150
                rho[c] = sigT[c] != 0 ? (ssc / sigT[c]) : 0;
            }
        }
    }
    return sssIdx;
}

// The start of Sample_S for ray i of the packed queue q after its closest-hit launch (hits, sc.hitInst / sc.animXf as k_interaction finds them): the
// BSDF at po as k_scatter binds it, isect.bssrdf with its coefficients at po, the probe segment from u[3i .. 3i+2] = (u1, u2.x, u2.y).  A ray with a
// segment gets its SssState (slot = i) and its first probe ray in qjob (tag i, the ray's time); every ray gets its whole record -- status -1 (miss),
// 0 (no bssrdf) or 1 (a bssrdf: final where no probe ray leaves, else k_sss_emit's to finish) -- a pi of zeros with prim -1, and chain[i] = 0.
template <bool TEX, bool VOL>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_sss_seed(DScene sc, RayQueue q, const float4 *__restrict__ hits, const float *__restrict__ timesIn,
                                                              const float *__restrict__ u, int n, SssState sss, int *__restrict__ chain, float4 *__restrict__ out,
                                                              float4 *__restrict__ pi) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    bool push = false;
    float4 no = make_float4(0, 0, 0, 0), nd = no;
    if (i < n) {
        const float4 o4 = q.o[i], d4 = q.d[i], h4 = hits[i];
        const int prim = __float_as_int(h4.x);
        int status = -1, sssIdx = -1;
        float eta = 0;
        if (prim >= 0) {
            status = 0;
            const V3 rayD = mk(d4.x, d4.y, d4.z);
            const Tri tri = load_tri(sc, prim);
            const PgMaterial mtl = sc.materials[tri.material];
            if (sc.nBssrdfs > 0 && sc.materialBssrdf[tri.material] >= 0) {  // (any other material: ComputeScatteringFunctions sets no bssrdf)
                int inst = sc.hitInst ? sc.hitInst[i] : -1, inst2;
                nest_decode(sc, inst, inst2);
                const InstXf outer = inst_xf(sc, inst, i), inner = inst_xf(sc, inst2, i, true);
                QuadricUv quv;
                Isect is = hit_isect(sc, outer, inner, o4, rayD, h4, prim, tri, quv);
                // ---- the BSDF, as k_scatter binds it: a material's BxDF list, or (TEX) ComputeScatteringFunctions with textures
                LobeBsdfT<PgBxDF> lb;
                PgBxDF lobeStore[TEX ? PG_MAX_BXDFS : 1];
                float sigT[3], rho[3];
                if constexpr (TEX) {
                    TexHit th;
                    tex_hit_setup(sc, pg_scatter_no_frame, q, i, 0, prim, tri, h4, rayD, outer, inner, quv, is, make_int4(0, 0, 0, 0), 0.f, 0.f, false, false, 0, th, nullptr);
                    material_bump(sc, tri.material, th, is);
                    int nl = 0;
                    float etaL = 1;
                    MatEval<2>::run(*sc.self, tri.material, th, LobeOutRaw{lobeStore}, nl, etaL, PG_MAX_BXDFS);
                    lbsdf_bind(lb, lobeStore, nl, etaL);
                    sssIdx = bssrdf_coefficients_at<true>(sc, tri.material, lb.n, &th, sigT, rho);
                } else {
                    lbsdf_bind(lb, sc.bxdfs + mtl.first_bxdf, mtl.n_bxdfs, mtl.bsdf_eta);
                    sssIdx = bssrdf_coefficients_at<false>(sc, tri.material, lb.n, nullptr, sigT, rho);
                }
                lb.ns = is.ns; lb.ng = is.n;
                lb.ss = normalize(is.sdpdu);
                lb.ts = cross(lb.ns, lb.ss);
                if (sssIdx >= 0) {
                    status = 1;
                    // the first half of SeparableBSSRDF::Sample_Sp (bssrdf.cpp:257-292), as k_shade hands a path over to the probe chains
                    DBssrdf b = bssrdf_bind(sc.bssrdfs[sssIdx], sc.bssrdfTables);
                    for (int c = 0; c < 3; ++c) { b.sigma_t[c] = sigT[c]; b.rho[c] = rho[c]; }
                    eta = b.eta;
                    const size_t k = 3 * (size_t)i;
                    float u1 = u[k];
                    V3 baseP, pTarget;
                    if (bssrdf_probe_segment(b, lb.ss, lb.ts, lb.ns, is.p, u1, u[k + 1], u[k + 2], baseP, pTarget)) {
                        const V3 pd = pTarget - baseP;  // base.SpawnRayTo(pTarget) of an Interaction without normal or error: from baseP itself
                        if (!(pd.x == 0 && pd.y == 0 && pd.z == 0)) {  // bssrdf.cpp:306: a zero direction ends the chain before it starts
                            no = make_float4(baseP.x, baseP.y, baseP.z, 1 - PG_SHADOW_EPS);
                            nd = make_float4(pd.x, pd.y, pd.z, __int_as_float(i));
                            push = true;
                            sss.po[i] = make_float4(is.p.x, is.p.y, is.p.z, u1);
                            sss.frame[0][i] = make_float4(lb.ns.x, lb.ns.y, lb.ns.z, b.eta);
                            sss.frame[1][i] = make_float4(lb.ss.x, lb.ss.y, lb.ss.z, __int_as_float(sssIdx));
                            sss.frame[2][i] = make_float4(lb.ts.x, lb.ts.y, lb.ts.z, __int_as_float(sc.bssrdfs[sssIdx].match_material));
                            sss.coef[0][i] = make_float4(sigT[0], sigT[1], sigT[2], 0);
                            sss.coef[1][i] = make_float4(rho[0], rho[1], rho[2], 0);
                            sss.target[i] = make_float4(pTarget.x, pTarget.y, pTarget.z, 0);
                            sss.count[i] = make_int2(0, 0);
                            if constexpr (VOL) sss.medium[i] = make_int2(0, 0);  // Sample_Sp's `base` has no MediumInterface
                        }
                    }
                }
            }
        }
        chain[i] = 0;
        float4 *dst = out + 4 * (size_t)i;
        dst[0] = make_float4(__int_as_float(status), __int_as_float(prim), __int_as_float(sssIdx), __int_as_float(0));
        dst[1] = make_float4(0, 0, 0, 0);
        dst[2] = make_float4(eta, __int_as_float(-1), __int_as_float(-1), __int_as_float(0));
        dst[3] = make_float4(0, 0, 0, 0);
        float4 *pdst = pi + 8 * (size_t)i;
        pdst[0] = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 1; k < 8; ++k) pdst[k] = make_float4(0, 0, 0, 0);
    }
    // every lane of the block is here
    const int pos = wave_append(sss.qjob, push);
    if (push) {
        sss.qjob.o[pos] = no; sss.qjob.d[pos] = nd;
        if (sc.rayTimes) PG_QUEUE_TIMES(sc, sss.qjob)[pos] = timesIn[i];
    }
}

// chain[tag] += 1 for every probe ray of q: PgSubsurfaceSample::chain_rays, the Scene::Intersect calls of Sample_Sp's loop.  Not atomic: it relies on
// k_sss_probe's invariant that a chain has ONE ray under way, so a tag is in a queue at most once (stated there too).  One launch per step of the first walk.
__global__ __launch_bounds__(PG_BLOCK) void k_sss_tally(RayQueue q, int *__restrict__ chain) {
    const int i = queue_item<PG_BLOCK>(q);
    if (i >= 0) chain[__float_as_int(q.d[i].w)] += 1;
}

// The end of Sample_S for every job of sss.qjob once both walks are through (k_sss_exit's head): the chosen hit rebuilt as a SurfaceInteraction,
// Pdf_Sp / nFound and Sp = Sr(|po - pi|) (bssrdf.cpp:322-327), pi's MediumInterface -- the 64-byte record as four float4 stores and, for status 2,
// pi as eight in k_interaction's layout with wo = shading.n (bssrdf.cpp:243-248), t = 0 and the ray's time.  A job without a hit on the material,
// with a black Sr or a zero pdf keeps the seed's status 1 and pi; its n_found and chain_rays are reported.
template <bool VOL>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_sss_emit(DScene sc, SssState sss, const int *__restrict__ chain, const float *__restrict__ times,
                                                              float4 *__restrict__ out, float4 *__restrict__ pi) {
    const int j = queue_item<PG_SHADE_BLOCK>(sss.qjob);
    if (j < 0) return;
    const int slot = __float_as_int(sss.qjob.d[j].w);
    float4 *dst = out + 4 * (size_t)slot;
    float4 rec[4] = {dst[0], make_float4(0, 0, 0, 0), dst[2], make_float4(0, 0, 0, 0)};  // (status 1, prim, bssrdf, .) and (eta, -1, -1, .) of the seed
    const int nFound = sss.count[slot].x;
    rec[0].w = __int_as_float(nFound);
    rec[2].w = __int_as_float(chain[slot]);
    if (nFound > 0) {  // bssrdf.cpp:318: no hit on the material: Sample_Sp returns black
        const float4 h4 = sss.hit[slot], o4 = sss.hitO[slot], d4 = sss.hitD[slot];
        const int prim = __float_as_int(h4.x);
        int inst = sss.hitInst[slot], inst2;
        nest_decode(sc, inst, inst2);
        const InstXf outer = {sc.instances, sss.hitXf, 0, inst, slot}, inner = {sc.instances, sss.hitXf, sss.hitXfNest, inst2, slot};
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const Tri tri = load_tri(sc, prim);
        QuadricUv quv;
        const Isect is = hit_isect(sc, outer, inner, o4, rayD, h4, prim, tri, quv);
        const float4 po4 = sss.po[slot], f0 = sss.frame[0][slot], f1 = sss.frame[1][slot], f2 = sss.frame[2][slot];
        const V3 poP = mk(po4.x, po4.y, po4.z);
        DBssrdf b = bssrdf_bind(sc.bssrdfs[__float_as_int(f1.w)], sc.bssrdfTables);
        const float4 cs = sss.coef[0][slot], cr = sss.coef[1][slot];
        b.sigma_t[0] = cs.x; b.sigma_t[1] = cs.y; b.sigma_t[2] = cs.z; b.rho[0] = cr.x; b.rho[1] = cr.y; b.rho[2] = cr.z;
        const float pdf = bssrdf_pdf_sp(b, mk(f1.x, f1.y, f1.z), mk(f2.x, f2.y, f2.z), mk(f0.x, f0.y, f0.z), poP, is.p, is.n) / nFound;
        const Spec S = bssrdf_sr(b, sqrtf(lensq(poP - is.p)));
        if (!(is_black(S) || pdf == 0)) {
            int mIn = 0, mOut = 0;  // pi's MediumInterface: the primitive's own, or the medium of the probe ray that found it (index + 1, 0 = none)
            if constexpr (VOL) prim_interface(sc, prim, sss.medium[slot].y, mIn, mOut);
            rec[0].x = __int_as_float(2);
            rec[1] = make_float4(S.r, S.g, S.b, pdf);
            rec[2].y = __int_as_float(mIn - 1); rec[2].z = __int_as_float(mOut - 1);
            float uu = quv.u, vv = quv.v;
            if (!quv.on) {  // uvHit, triangle.cpp:332 (as k_interaction forms it)
                float uv[6];
                load_uv(sc, prim, tri.flags, uv);
                uu = h4.y * uv[0] + h4.z * uv[2] + h4.w * uv[4];
                vv = h4.y * uv[1] + h4.z * uv[3] + h4.w * uv[5];
            }
            float4 *pdst = pi + 8 * (size_t)slot;
            pdst[0] = make_float4(__int_as_float(prim), __int_as_float(inst), __int_as_float(inst2), __int_as_float(tri.material));
            pdst[1] = make_float4(__int_as_float(tri.light), 0.f, times[slot], uu);
            pdst[2] = make_float4(vv, is.p.x, is.p.y, is.p.z);
            pdst[3] = make_float4(is.pError.x, is.pError.y, is.pError.z, is.n.x);
            pdst[4] = make_float4(is.n.y, is.n.z, is.ns.x, is.ns.y);  // pi.wo = pi.shading.n
            pdst[5] = make_float4(is.ns.z, is.ns.x, is.ns.y, is.ns.z);
            pdst[6] = make_float4(is.sdpdu.x, is.sdpdu.y, is.sdpdu.z, is.sdpdv.x);
            pdst[7] = make_float4(is.sdpdv.y, is.sdpdv.z, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = rec[k];
}

// PgScatter of records 0 .. n-1 for the BSDF Sample_S installs at pi[i]: one SeparableBSSRDFAdapter over pi's shading frame with eta[i] (AdapterBsdf).
// in: wi, three floats per record (BSDF::f and BSDF::Pdf) or, for SAMPLE, u, two (BSDF::Sample_f).  Of pi: prim, n, wo, shading_n and shading_dpdu.
template <bool SAMPLE>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_adapter(const float4 *__restrict__ pi, const float *__restrict__ eta, const float *__restrict__ in, int flags, int n,
                                                             float4 *__restrict__ out) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 *r = pi + 8 * (size_t)i;
    const float4 r0 = r[0], r3 = r[3], r4 = r[4], r5 = r[5], r6 = r[6];
    const int prim = __float_as_int(r0.x);
    float4 rec[4];
    for (int k = 0; k < 4; ++k) rec[k] = make_float4(0, 0, 0, 0);
    rec[0].x = __int_as_float(-1);
    if (prim >= 0) {
        AdapterBsdf ab;
        ab.ns = mk(r5.y, r5.z, r5.w); ab.ng = mk(r3.w, r4.x, r4.y);
        ab.ss = normalize(mk(r6.x, r6.y, r6.z));
        ab.ts = cross(ab.ns, ab.ss);
        ab.eta = eta[i];
        const V3 wo = mk(r4.z, r4.w, r5.x);
        const int type = PG_BSDF_REFLECTION | PG_BSDF_DIFFUSE;
        Spec f;
        V3 wi = mk(0, 0, 0);
        float pdf;
        int sampledType = 0;
        if constexpr (SAMPLE) {
            f = ad_sample_f(ab, wo, wi, in[2 * (size_t)i], in[2 * (size_t)i + 1], pdf, flags, sampledType);
            if (pdf == 0) { f = sp(0); wi = mk(0, 0, 0); sampledType = 0; }
        } else {
            const size_t k = 3 * (size_t)i;
            wi = mk(in[k], in[k + 1], in[k + 2]);
            f = ad_f(ab, wo, wi, flags);
            pdf = ad_pdf(ab, wo, wi, flags);
        }
        rec[0] = make_float4(__int_as_float(prim), __int_as_float(1), __int_as_float((type & flags) == type ? 1 : 0), __int_as_float(sampledType));
        rec[1] = make_float4(f.r, f.g, f.b, pdf);
        rec[2] = make_float4(wi.x, wi.y, wi.z, 1.f);  // BSDF::eta: Sample_S builds BSDF(*pi) with the default
        rec[3] = make_float4(ab.ns.x, ab.ns.y, ab.ns.z, __uint_as_float(0u));  // types: the adapter is no PgBxDFType
    }
    float4 *dst = out + 4 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = rec[k];
}

void launch_sss_seed(const DScene &sc, bool vol, RayQueue q, const float4 *hits, const float *timesIn, const float *u, int n, SssState sss, int *chain,
                     PgSubsurfaceSample *out, PgInteraction *pi, hipStream_t s) {
    static_assert(sizeof(PgSubsurfaceSample) == 4 * sizeof(float4) && sizeof(PgInteraction) == 8 * sizeof(float4), "PgSubsurfaceSample is four float4, PgInteraction eight");
    if (n <= 0) return;
    const dim3 g((n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK), b(PG_SHADE_BLOCK);
    float4 *o4 = reinterpret_cast<float4 *>(out), *p4 = reinterpret_cast<float4 *>(pi);
    const bool tex = sc.hasTextured || sc.hasNest;  // as launch_scatter chooses k_scatter's mode
    if (tex && vol) hipLaunchKernelGGL((k_sss_seed<true, true>), g, b, 0, s, sc, q, hits, timesIn, u, n, sss, chain, o4, p4);
    else if (tex) hipLaunchKernelGGL((k_sss_seed<true, false>), g, b, 0, s, sc, q, hits, timesIn, u, n, sss, chain, o4, p4);
    else if (vol) hipLaunchKernelGGL((k_sss_seed<false, true>), g, b, 0, s, sc, q, hits, timesIn, u, n, sss, chain, o4, p4);
    else hipLaunchKernelGGL((k_sss_seed<false, false>), g, b, 0, s, sc, q, hits, timesIn, u, n, sss, chain, o4, p4);
}
void launch_sss_tally(RayQueue q, int *chain, hipStream_t s) {
    const int nblk = PG_REGIONS * (q.regionCap / PG_BLOCK);
    if (nblk == 0) return;
    hipLaunchKernelGGL(k_sss_tally, dim3(nblk), dim3(PG_BLOCK), 0, s, q, chain);
}
void launch_sss_emit(const DScene &sc, bool vol, SssState sss, const int *chain, const float *times, PgSubsurfaceSample *out, PgInteraction *pi, hipStream_t s) {
    const int nblk = PG_REGIONS * (sss.qjob.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    float4 *o4 = reinterpret_cast<float4 *>(out), *p4 = reinterpret_cast<float4 *>(pi);
    if (vol) hipLaunchKernelGGL((k_sss_emit<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, sss, chain, times, o4, p4);
    else hipLaunchKernelGGL((k_sss_emit<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, sss, chain, times, o4, p4);
}
void launch_adapter(const PgInteraction *pi, const float *eta, const float *in, bool sample, int flags, int n, PgScatter *out, hipStream_t s) {
    if (n <= 0) return;
    const dim3 g((n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK), b(PG_SHADE_BLOCK);
    const float4 *p4 = reinterpret_cast<const float4 *>(pi);
    float4 *o4 = reinterpret_cast<float4 *>(out);
    if (sample) hipLaunchKernelGGL((k_adapter<true>), g, b, 0, s, p4, eta, in, flags, n, o4);
    else hipLaunchKernelGGL((k_adapter<false>), g, b, 0, s, p4, eta, in, flags, n, o4);
}
#endif
