// pg_direct.h -- the DirectLightingIntegrator's kernels (integrators/directlighting.cpp:62-95 without its specular bounces, which pg_render_direct
// refuses).  Included at the end of pg_kernels.hip: everything here is built from the pieces that file includes -- the interaction (hit_isect), an emitter's
// L (area_light_l), the BxDF lists and the material evaluators, EstimateDirect's set-up (estimate_direct_setup, pg_estimate.h) with its shadow ray
// (shadow_ray_to) and light.Pdf_Li of the BSDF-sampled direction (mis_light_pdf), the queue appends -- and k_resolve itself finishes every
// EstimateDirect.  None of them is restated here: what k_direct adds is its choice of the light, its draws and where the step's terms go.
//
// A camera ray's closest hit stays in its main queue while the frame walks the (light, sample) steps: every step is ONE launch of k_direct over the
// queue, which rebuilds the hit's interaction and BSDF, draws the step's uLight / uScattering, and leaves a shadow ray, a BSDF-sampled ray and the
// pending terms at the entry's queue position exactly as k_shade does for the path integrator; the two rays are traced, and k_resolve adds the
// step's EstimateDirect to a per-slot accumulator.  k_direct_fold then applies the reference's divisions in the reference's order:
//   UniformSampleAllLights (integrator.cpp:54-83):  Ld = 0; Ld += EstimateDirect (k = 0, 1, ...);  Lall += Ld / nSamples;  ...  L = Le + Lall
//   UniformSampleOneLight  (integrator.cpp:85-106):  L = Le + EstimateDirect / lightPdf,  lightPdf = Float(1) / nLights
// Nothing of the path integrators' state in queue order is used: L, the film position and the sampler's state live by slot.
#ifndef PG_DIRECT_H
#define PG_DIRECT_H

template <int MODE>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_direct(DScene sc, RenderParams rp, PathState st, RayQueue qin, const float4 *__restrict__ hits, RayQueue qnext,
                                                            RayQueue qshadow, RayQueue qmis, unsigned long long *lightTriTests, DirectStep ds) {
    constexpr bool TEX = MODE == 2;
    const int i = queue_item<PG_SHADE_BLOCK>(qin);
    const bool valid = i >= 0;
    bool pushNext = false, pushShadow = false, pushMis = false;
    float4 nextO = make_float4(0, 0, 0, 0), nextD = nextO, shadowO = nextO, shadowD = nextO, misO = nextO, misD = nextO;
    int slot = 0, lightNum = -1;
    unsigned int nLightTests = 0;
    // (lightSelectPdf and beta of 1: k_resolve's beta * (Ld / lightSelectPdf) is Ld itself here, added to the slot's accumulator)
    float4 pdLight = pending_light_encode(sp(0), 1), pdMis = pending_mis_encode(sp(0), 0);
    float misWeight = 0;
    if (valid) {
        const float4 d4 = qin.d[i], h4 = hits[i];
        slot = __float_as_int(d4.w);
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const int prim = __float_as_int(h4.x);
        const PgRenderDesc &rd = rp.rd;
        const float4 L4 = st.L[slot];
        const float filmY = st.beta[slot].w;
        const int4 meta = st.meta[slot];
        const uint64_t index = (uint64_t)(uint32_t)meta.x | ((uint64_t)(uint32_t)meta.y << 32);
        const bool tileSerial = rd.sampler >= PG_SAMPLER_RANDOM;  // (one camera ray per tile in flight, slot = the tile: its stream is drawn in the reference's order)
        const bool found = prim >= 0;
        if (!found) {
            if (ds.first) {  // directlighting.cpp:70-73: every light's Le(ray), in light order (all but the infinite lights' are zero)
                Spec L = sp(0);
                for (int li = 0; li < sc.nLights; ++li)
                    if (sc.lights[li].type == PG_LIGHT_INFINITE) L = L + env_le(sc, sc.lights[li], rayD);
                st.L[slot] = make_float4(L.r, L.g, L.b, L4.w);
            }
        } else {
            const Tri tri = load_tri(sc, prim);
            const PgMaterial mtl = sc.materials[tri.material];
            const bool surface = mtl.type != PG_MAT_NONE;
            if (surface ? (ds.first || ds.light != -1) : ds.first != 0) {
                // ---- the SurfaceInteraction (hit_isect), under the instance's transform or -- MODE 2 -- the two of a hit two levels deep
                int inst = sc.hitInst ? sc.hitInst[i] : -1, inst2 = -1;
                if constexpr (TEX) nest_decode(sc, inst, inst2);
                const InstXf outer = inst_xf(sc, inst, i), inner = inst_xf(sc, inst2, i, true);
                QuadricUv quv;
                Isect is = hit_isect(sc, outer, inner, (tri.flags & PG_PRIM_SPHERE) ? qin.o[i] : make_float4(0, 0, 0, 0), rayD, h4, prim, tri, quv);
                if (surface && ds.first) {  // directlighting.cpp:81: L += isect.Le(wo) -- L is zero before it; an emitter lies under no instance: is.n is its own normal
                    const Spec Le = tri.light >= 0 ? area_light_l(sc.lights[tri.light], is.n, -rayD) : sp(0);
                    st.L[slot] = make_float4(Le.r, Le.g, Le.b, L4.w);
                }
                if (!surface) {  // directlighting.cpp:77-78: no BSDF -- Li(isect.SpawnRay(ray.d), ..., depth): the same depth, a ray without differentials
                    V3 o;
                    spawn_ray(is, rayD, o);
                    nextO = make_float4(o.x, o.y, o.z, PG_INF);
                    nextD = make_float4(rayD.x, rayD.y, rayD.z, __int_as_float(slot));
                    pushNext = true;
                    st.meta[slot] = make_int4(meta.x, meta.y, meta.z, meta.w & ~PG_META_HASDIFF);
                } else if (ds.light != -1) {
                    // ---- the BSDF: a material's BxDF list, or (MODE 2) ComputeScatteringFunctions with textures
                    LobeBsdfT<PgBxDF> lb;
                    PgBxDF lobeStore[TEX ? PG_MAX_BXDFS : 1];
                    if constexpr (TEX) {
                        TexHit th;
                        tex_hit_setup(sc, rd, qin, i, slot, prim, tri, h4, rayD, outer, inner, quv, is, meta, L4.w, filmY, tileSerial, false, index, th, st.L);
                        material_bump(sc, tri.material, th, is);
                        lb.ns = is.ns; lb.ng = is.n;
                        lb.ss = normalize(is.sdpdu);
                        lb.ts = cross(lb.ns, lb.ss);
                        int nl = 0;
                        float etaL = 1;
                        MatEval<2>::run(*sc.self, tri.material, th, LobeOutRaw{lobeStore}, nl, etaL, PG_MAX_BXDFS);
                        lbsdf_bind(lb, lobeStore, nl, etaL);
                    } else {
                        lb.ns = is.ns; lb.ng = is.n;
                        lb.ss = normalize(is.sdpdu);
                        lb.ts = cross(lb.ns, lb.ss);
                        lbsdf_bind(lb, sc.bxdfs + mtl.first_bxdf, mtl.n_bxdfs, mtl.bsdf_eta);
                    }
                    // ---- the step's numbers: Get1D / Get2D of a PixelSampler's stream, or a GlobalSampler's (sample index, dimension)
                    float uSel = 0, uL0, uL1, uS0, uS1;
                    if (tileSerial) {
                        if (ds.light == -2) uSel = ts_get1d(sc, slot);
                        ts_get2d(sc, rd.sampler, slot, uL0, uL1);
                        ts_get2d(sc, rd.sampler, slot, uS0, uS1);
                    } else {
                        uint64_t idx = index;
                        if (ds.arrayN > 0) {
                            int px, py, sn;
                            slot_to_pixel(rp, slot, px, py, sn);
                            idx = sampler_index(sc, rd, px, py, (uint64_t)sn * (uint64_t)ds.arrayN + (uint64_t)ds.arrayK);
                        }
                        if (ds.light == -2) uSel = halton_sample(sc, rd, idx, ds.dimBase - 1);
                        uL0 = halton_sample(sc, rd, idx, ds.dimBase); uL1 = halton_sample(sc, rd, idx, ds.dimBase + 1);
                        uS0 = halton_sample(sc, rd, idx, ds.dimBase + 2); uS1 = halton_sample(sc, rd, idx, ds.dimBase + 3);
                    }
                    lightNum = ds.light;
                    if (ds.light == -2) { lightNum = (int)(uSel * sc.nLights); if (lightNum > sc.nLights - 1) lightNum = sc.nLights - 1; }  // integrator.cpp:95
                    // ---- EstimateDirect (integrator.cpp:108-215) with bsdfFlags = BSDF_ALL & ~BSDF_SPECULAR, up to the two rays
                    const DirectSetup ed = estimate_direct_setup<true>(sc, lb, is.p, is.pError, is.n, is.wo, lightNum, uL0, uL1, uS0, uS1);
                    if (ed.light.shadow) {
                        shadow_ray_to(is.p, is.pError, is.n, ed.light.ls, slot, shadowO, shadowD);
                        pushShadow = true;
                        pdLight = pending_light_encode(direct_light_folded(ed.light), 1);
                    }
                    if (ed.mis.cand) {  // light.Pdf_Li of the sampled direction at once: nothing else is live here
                        V3 misRo;
                        spawn_ray(is, ed.mis.wi, misRo);
                        const float lightPdf2 = mis_light_pdf<true>(sc, ed.mis.lightPrim, ed.mis.area, ed.mis.inside, is.p, misRo, ed.mis.wi, nLightTests);
                        if (lightPdf2 != 0) {
                            misO = make_float4(misRo.x, misRo.y, misRo.z, PG_INF);
                            misD = make_float4(ed.mis.wi.x, ed.mis.wi.y, ed.mis.wi.z, __int_as_float(slot));
                            pushMis = true;
                            pdMis = pending_mis_encode(ed.mis.f, ed.mis.pdf);
                            misWeight = pending_mis_weight(ed.mis.pdf, lightPdf2);
                        }
                    }
                }
                // directlighting.cpp:91-95: while depth + 1 < maxdepth, SpecularReflect and SpecularTransmit each hand BSDF::Sample_f a Get2D
                // (integrator.cpp:217-295) whether or not the BSDF has a specular lobe.  None has here (pg_check_direct_desc), so both return black --
                // but a PixelSampler's stream and dimension counters have moved on by two pairs (a GlobalSampler's dimensions are nobody else's)
                if (surface && ds.first && tileSerial && rd.max_depth >= 2) {
                    float a, b;
                    ts_get2d(sc, rd.sampler, slot, a, b);
                    ts_get2d(sc, rd.sampler, slot, a, b);
                }
            }
        }
    }
    const RayQueue outQ[3] = {qnext, qshadow, qmis};
    const bool outPred[3] = {pushNext, pushShadow, pushMis};
    int outPos[3];
    block_push<3, false, PG_SHADE_BLOCK>(outQ, outPred, outPos);
    if (pushNext) { qnext.o[outPos[0]] = nextO; qnext.d[outPos[0]] = nextD; }
    if (pushShadow) { qshadow.o[outPos[1]] = shadowO; qshadow.d[outPos[1]] = shadowD; }
    if (pushMis) { qmis.o[outPos[2]] = misO; qmis.d[outPos[2]] = misD; }
    store_ray_times(sc, qin, i, outQ, outPred, outPos);
    if (valid) {  // k_resolve's pending terms, by queue position; L is the slot's accumulator: ~slot, what pending_where gives a path that ended (spelled out
                  // here: through that function, or any other, k_direct<1> takes six more VGPRs -- CHANGELOG.md)
        st.pdInfo[i] = pending_info_encode(outPos[1], outPos[2], lightNum, ~slot);
        if (pushShadow || pushMis) {
            st.pdLight[i] = pdLight;
            st.pdMis[i] = pdMis;
            st.pdBeta[i] = pending_beta_encode(sp(1.f), misWeight);
        }
    }
    flush_light_tests(lightTriTests, nLightTests);
}
void launch_direct(const DScene &sc, const RenderParams &rp, PathState st, RayQueue qin, const float4 *hits, RayQueue qnext, RayQueue qshadow, RayQueue qmis,
                   unsigned long long *lightTriTests, const DirectStep &ds, hipStream_t s) {
    const int nblk = PG_REGIONS * (qin.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    if (sc.hasTextured || sc.hasNest) hipLaunchKernelGGL((k_direct<2>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, ds);
    else hipLaunchKernelGGL((k_direct<1>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, ds);
}

// dst[slot].rgb += src[slot].rgb / divisor (direct_fold, pg_resolve.h), then src[slot].rgb = 0 (the .w fields stay)
__global__ __launch_bounds__(PG_BLOCK) void k_direct_fold(float4 *__restrict__ src, float4 *__restrict__ dst, float divisor, int n) {
    const int slot = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (slot >= n) return;
    const float4 a = src[slot];
    dst[slot] = direct_fold(dst[slot], a, divisor);
    src[slot] = make_float4(0, 0, 0, a.w);
}
void launch_direct_fold(float4 *src, float4 *dst, float divisor, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_direct_fold, dim3((n + PG_BLOCK - 1) / PG_BLOCK), dim3(PG_BLOCK), 0, s, src, dst, divisor, n);
}
#endif
