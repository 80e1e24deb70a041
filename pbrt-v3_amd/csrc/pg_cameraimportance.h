// pg_cameraimportance.h -- the kernels a host integrator needs to trace LIGHT subpaths (bdpt, sppm, a light tracer): pg_camera_we_at (PerspectiveCamera::We and
// ::Pdf_We per ray), pg_camera_sample_wi_at (::Sample_Wi per reference point, with the VisibilityTester's ray appended to the test queue) and
// pg_scatter_f_mode_at / pg_scatter_sample_mode_at under mode 1 (the scattering queries with the BSDF of TransportMode::Importance).  Included at the end of
// pg_kernels.hip, after pg_cameraquery.h.
//
// All three are wiring.  The camera kernels call xform_point / m4_vec, interpolate_trs (pg_motion.h: m and mInv, as a moving instance's), concentric_sample_disk,
// offset_ray_origin and shadow_ray_to; k_camera_sample_wi appends its rays as k_light_sample does, and k_light_visibility (pg_lightquery.h) writes the trace's
// answers into its records unchanged.  k_scatter_importance is k_scatter / k_scatter_diff (pg_scatter.h, pg_cameraquery.h) with lbsdf_f / lbsdf_sample_f
// instantiated for IMP (pg_bxdf.h).  One thread per item, PG_SHADE_BLOCK threads per block, no LDS.  Nothing here has been tuned or timed.
// Out of scope: Sample_Le / Pdf_Le, the BSSRDF adapter under Importance (bdpt ignores BSSRDFs), CorrectShadingNormal (host arithmetic on PgInteraction.n and
// PgScatter.shading_n), light-selection distributions, We for cameras other than the perspective one (the reference has none).
#ifndef PG_CAMERAIMPORTANCE_H
#define PG_CAMERAIMPORTANCE_H

// AnimatedTransform::Interpolate(time, &c2w) of a camera that moves (transform.cpp:1144-1169), with the inverse We needs: the start transform up to
// camera_time[0], the end transform from camera_time[1] on -- each with its STORED inverse --, in between both from interpolate_trs<true>.  m is
// camera_matrix_at's (pg_camera.h), which forms no inverse.
PG_DEV void camera_matrices_at(const PgRenderDesc &rd, const PgCameraWeDesc &we, float time, float *m, float *mInv) {
    if (time <= rd.camera_time[0]) { for (int k = 0; k < 16; ++k) { m[k] = rd.camera_to_world[k]; mInv[k] = we.world_to_camera[k]; } return; }
    if (time >= rd.camera_time[1]) { for (int k = 0; k < 16; ++k) { m[k] = rd.camera_to_world_end[k]; mInv[k] = we.world_to_camera_end[k]; } return; }
    const float dt = (time - rd.camera_time[0]) / (rd.camera_time[1] - rd.camera_time[0]);
    interpolate_trs<true>(rd.camera_T, rd.camera_R, rd.camera_S, dt, m, mInv);
}

// PerspectiveCamera::We(ray, &pRaster) and ::Pdf_We(ray, &pdfPos, &pdfDir), perspective.cpp:146-201, for the ray (o, d) under the camera matrix c2w of its time
// and that matrix's inverse w2c.  status as PgCameraImportance's
struct CameraWe { int status; float We, pdfPos, pdfDir, rasterX, rasterY, cosTheta; };
PG_DEV CameraWe camera_we(const PgRenderDesc &rd, const PgCameraWeDesc &we, const float *c2w, const float *w2c, V3 o, V3 d) {
    CameraWe r = {0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float cosTheta = dot(d, m4_vec(c2w, mk(0, 0, 1)));
    if (cosTheta <= 0) return r;
    const V3 pFocus = o + d * ((rd.lens_radius > 0 ? rd.focal_distance : 1) / cosTheta);
    const V3 pRaster = xform_point(we.camera_to_raster, xform_point(w2c, pFocus));  // Inverse(RasterToCamera)(Inverse(c2w)(pFocus))
    r.status = 1; r.rasterX = pRaster.x; r.rasterY = pRaster.y; r.cosTheta = cosTheta;
    if (pRaster.x < rd.sample_bounds[0] || pRaster.x >= rd.sample_bounds[2] || pRaster.y < rd.sample_bounds[1] || pRaster.y >= rd.sample_bounds[3]) return r;
    const float lensArea = rd.lens_radius != 0 ? (PG_PI * rd.lens_radius * rd.lens_radius) : 1;
    const float cos2Theta = cosTheta * cosTheta;
    r.status = 2;
    r.We = 1 / (we.image_area * lensArea * cos2Theta * cos2Theta);
    r.pdfPos = 1 / lensArea;
    r.pdfDir = 1 / (we.image_area * cosTheta * cosTheta * cosTheta);
    return r;
}

// PgCameraImportance of rays 0 .. n-1: one thread per ray, the 32-byte record as two float4 stores.  ANIM: the camera moves -- a still camera's kernel does
// not carry the interpolation
template <bool ANIM>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_camera_we(RenderDescHead rdh, PgCameraWeDesc we, const float *__restrict__ o3, const float *__restrict__ d3,
                                                               const float *__restrict__ time, int n, float4 *__restrict__ out) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PgRenderDesc &rd = rdh;
    const size_t k = 3 * (size_t)i;
    const V3 o = mk(o3[k], o3[k + 1], o3[k + 2]), d = mk(d3[k], d3[k + 1], d3[k + 2]);
    CameraWe r;
    if constexpr (ANIM) {
        float c2w[16], w2c[16];
        camera_matrices_at(rd, we, time ? time[i] : 0.f, c2w, w2c);
        r = camera_we(rd, we, c2w, w2c, o, d);
    } else r = camera_we(rd, we, rd.camera_to_world, we.world_to_camera, o, d);
    out[2 * (size_t)i] = make_float4(__int_as_float(r.status), r.We, r.pdfPos, r.pdfDir);
    out[2 * (size_t)i + 1] = make_float4(r.rasterX, r.rasterY, r.cosTheta, 0.f);
}
void launch_camera_we(const PgRenderDesc &rd, const PgCameraWeDesc &we, const float *o, const float *d, const float *time, int n, PgCameraImportance *out, hipStream_t s) {
    static_assert(sizeof(PgCameraImportance) == 2 * sizeof(float4), "PgCameraImportance is two float4");
    if (n <= 0) return;
    RenderDescHead head;
    head = rd;
    const int nblk = (n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK;
    float4 *o4 = reinterpret_cast<float4 *>(out);
    if (rd.camera_animated) hipLaunchKernelGGL((k_camera_we<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, head, we, o, d, time, n, o4);
    else hipLaunchKernelGGL((k_camera_we<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, head, we, o, d, time, n, o4);
}

// PgCameraSample of samples 0 .. n-1: PerspectiveCamera::Sample_Wi(ref[i], u[2i .. 2i+1]), perspective.cpp:203-225, the 64-byte record as four float4 stores and,
// unless `shadow` is null, the ray of ref.SpawnRayTo(lensIntr) as two more.  A sample with pdf > 0 and We != 0 (what bdpt connects, bdpt.cpp:470-481) appends
// that ray to q with i as its tag and ref[i].time as its time, the way k_light_sample appends (pg_lightquery.h); `visibility` stays -1 until
// k_light_visibility has the trace's answer.
template <bool ANIM>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_camera_sample_wi(RenderDescHead rdh, PgCameraWeDesc we, const float4 *__restrict__ ref, const float *__restrict__ u, int n,
                                                                      RayQueue q, float *__restrict__ times, float4 *__restrict__ out, float4 *__restrict__ shadow) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    bool push = false;
    float4 shO = make_float4(0, 0, 0, 0), shD = shO;
    float time = 0;
    if (i < n) {
        const PgRenderDesc &rd = rdh;
        const LightRef lr = load_light_ref(ref, i);
        const float u0 = u[2 * (size_t)i], u1 = u[2 * (size_t)i + 1];
        float4 rec[4];
        for (int k = 0; k < 4; ++k) rec[k] = make_float4(0, 0, 0, 0);
        rec[0].x = rec[0].y = __int_as_float(-1);
        if (lr.prim >= 0) {
            auto sample = [&](const float *c2w, const float *w2c) {
                float lx, ly;
                concentric_sample_disk(u0, u1, lx, ly);
                LightSample lens;  // lensIntr: a point without an error bound (interaction.h:54-56) and the camera's axis as its normal
                lens.p = xform_point(c2w, mk(rd.lens_radius * lx, rd.lens_radius * ly, 0));
                lens.n = m4_vec(c2w, mk(0, 0, 1));
                lens.pError = mk(0, 0, 0);
                V3 wi = lens.p - lr.p;
                const float dist = sqrtf(lensq(wi));
                wi = vdiv(wi, dist);
                const float lensArea = rd.lens_radius != 0 ? (PG_PI * rd.lens_radius * rd.lens_radius) : 1;
                const float pdf = (dist * dist) / (absdot(lens.n, wi) * lensArea);
                const CameraWe r = camera_we(rd, we, c2w, w2c, offset_ray_origin(lens.p, lens.pError, lens.n, -wi), -wi);  // We(lensIntr.SpawnRay(-wi), pRaster)
                push = pdf > 0 && r.We != 0;
                if (push) { shadow_ray_to(lr.p, lr.pError, lr.n, lens, i, shO, shD); time = lr.time; }
                rec[0] = make_float4(__int_as_float(r.status), __int_as_float(-1), pdf, r.We);
                rec[1] = make_float4(wi.x, wi.y, wi.z, lens.p.x);
                rec[2] = make_float4(lens.p.y, lens.p.z, lens.n.x, lens.n.y);
                rec[3] = make_float4(lens.n.z, r.rasterX, r.rasterY, 0.f);
            };
            if constexpr (ANIM) {
                float c2w[16], w2c[16];
                camera_matrices_at(rd, we, lr.time, c2w, w2c);
                sample(c2w, w2c);
            } else sample(rd.camera_to_world, we.world_to_camera);
        }
        float4 *dst = out + 4 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = rec[k];
        if (shadow) {  // origin, tMax = 1 - ShadowEpsilon, direction, time: zeros where nothing is tested
            shadow[2 * (size_t)i] = shO;
            shadow[2 * (size_t)i + 1] = make_float4(shD.x, shD.y, shD.z, time);
        }
    }
    // every lane of the block is here: the wave's rays take consecutive entries of region blockIdx.x % PG_REGIONS (k_light_sample's append)
    const unsigned long long m = __ballot(push);
    const int lane = lane_id(), r = blockIdx.x & (PG_REGIONS - 1);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(&q.counts[r * PG_COUNT_STRIDE], __popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (push) {
        const int pos = r * q.regionCap + base + __popcll(m & ((1ull << lane) - 1ull));
        q.o[pos] = shO; q.d[pos] = shD;
        times[pos] = time;
    }
}
void launch_camera_sample_wi(const PgRenderDesc &rd, const PgCameraWeDesc &we, const PgInteraction *ref, const float *u, int n, RayQueue q, float *times, PgCameraSample *out,
                             float *shadow, hipStream_t s) {
    static_assert(sizeof(PgCameraSample) == 4 * sizeof(float4) && offsetof(PgCameraSample, visibility) == offsetof(PgLightSample, visibility) &&
                  sizeof(PgCameraSample) == sizeof(PgLightSample), "k_light_visibility writes PgCameraSample::visibility where PgLightSample has it");
    if (n <= 0) return;
    RenderDescHead head;
    head = rd;
    const int nblk = (n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK;
    const float4 *r4 = reinterpret_cast<const float4 *>(ref);
    float4 *o4 = reinterpret_cast<float4 *>(out), *s4 = reinterpret_cast<float4 *>(shadow);
    if (rd.camera_animated) hipLaunchKernelGGL((k_camera_sample_wi<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, head, we, r4, u, n, q, times, o4, s4);
    else hipLaunchKernelGGL((k_camera_sample_wi<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, head, we, r4, u, n, q, times, o4, s4);
}

// k_scatter<TEX, SAMPLE> (pg_scatter.h) under TransportMode::Importance: the same functions in the same order, with lbsdf_f / lbsdf_sample_f instantiated for IMP.
// TEX hits are set up as k_scatter_diff sets them up (pg_cameraquery.h): stL != nullptr hands tex_hit_setup the ray's differentials; stL == nullptr, or twelve
// zeros, is a ray without -- the plain kernel's meta.
template <bool TEX, bool SAMPLE>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_scatter_importance(DScene sc, RayQueue q, const float4 *__restrict__ hits, const float *__restrict__ in, int flags,
                                                                        const float4 *stL, float4 *__restrict__ out) {
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
        if (mtl.type != PG_MAT_NONE) {
            int inst = sc.hitInst ? sc.hitInst[i] : -1, inst2;
            nest_decode(sc, inst, inst2);
            const InstXf outer = inst_xf(sc, inst, i), inner = inst_xf(sc, inst2, i, true);
            QuadricUv quv;
            Isect is = hit_isect(sc, outer, inner, o4, rayD, h4, prim, tri, quv);
            LobeBsdfT<PgBxDF> lb;
            PgBxDF lobeStore[TEX ? PG_MAX_BXDFS : 1];
            if constexpr (TEX) {
                bool hasDiff = false;
                if (stL) {
                    const float4 *df = lens_frame(stL)->differentials + 3 * (size_t)i;
                    const float4 a = df[0], b = df[1], c = df[2];
                    hasDiff = ((__float_as_uint(a.x) | __float_as_uint(a.y) | __float_as_uint(a.z) | __float_as_uint(a.w) | __float_as_uint(b.x) | __float_as_uint(b.y) |
                                __float_as_uint(b.z) | __float_as_uint(b.w) | __float_as_uint(c.x) | __float_as_uint(c.y) | __float_as_uint(c.z) | __float_as_uint(c.w)) << 1) != 0;  // (-0 is zero)
                }
                TexHit th;
                tex_hit_setup(sc, pg_scatter_diff_frame, q, i, i, prim, tri, h4, rayD, outer, inner, quv, is, make_int4(0, 0, 0, hasDiff ? PG_META_HASDIFF : 0), 0.f, 0.f, false, false, 0, th, stL);
                material_bump(sc, tri.material, th, is);
                int nl = 0;
                float etaL = 1;
                MatEval<2>::run(*sc.self, tri.material, th, LobeOutRaw{lobeStore}, nl, etaL, PG_MAX_BXDFS);
                lbsdf_bind(lb, lobeStore, nl, etaL);
            } else lbsdf_bind(lb, sc.bxdfs + mtl.first_bxdf, mtl.n_bxdfs, mtl.bsdf_eta);
            lb.ns = is.ns; lb.ng = is.n;
            lb.ss = normalize(is.sdpdu);
            lb.ts = cross(lb.ns, lb.ss);
            Spec f;
            V3 wi = mk(0, 0, 0);
            float pdf;
            int sampledType = 0;
            if constexpr (SAMPLE) {
                f = lbsdf_sample_f<true>(lb, is.wo, wi, in[2 * (size_t)i], in[2 * (size_t)i + 1], pdf, flags, sampledType);
                if (pdf == 0) { f = sp(0); wi = mk(0, 0, 0); sampledType = 0; }
            } else {
                const size_t k = 3 * (size_t)i;
                wi = mk(in[k], in[k + 1], in[k + 2]);
                f = lbsdf_f<true>(lb, is.wo, wi, flags);
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
void launch_scatter_importance(const DScene &sc, RayQueue q, const float4 *hits, const float *in, bool sample, int flags, const float4 *stL, PgScatter *out, hipStream_t s) {
    const int nblk = PG_REGIONS * (q.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    float4 *o4 = reinterpret_cast<float4 *>(out);
    const bool tex = sc.hasTextured || sc.hasNest;  // as launch_scatter chooses
    if (tex && sample) hipLaunchKernelGGL((k_scatter_importance<true, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, stL, o4);
    else if (tex) hipLaunchKernelGGL((k_scatter_importance<true, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, stL, o4);
    else if (sample) hipLaunchKernelGGL((k_scatter_importance<false, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, stL, o4);
    else hipLaunchKernelGGL((k_scatter_importance<false, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, stL, o4);
}
#endif
