// pg_cameraquery.h -- the kernels of the camera queries, for an integrator whose Li stays on the host: pg_camera_rays_at (Camera::GenerateRayDifferential
// for a batch of CameraSamples) and pg_scatter_f_diff_at / pg_scatter_sample_diff_at (the scattering queries for rays WITH differentials, pg_abi.hip's rayQuery).
// Included at the end of pg_kernels.hip, after pg_scatter.h, whose kernel the second one here repeats with one difference.
//
// Both are wiring.  k_camera_rays calls what k_generate calls -- camera_time, camera_matrix_at, camera_ray + camera_differentials or lens_camera_sample
// (pg_camera.h, pg_lens.h, pg_motion.h) -- on samples the caller drew instead of a frame's, and writes records instead of path state.  k_scatter_diff is
// k_scatter<true, .> handing tex_hit_setup the ray's differentials by the door the realistic camera's frames use (pg_hit.h: camera_type 3 reads them from the
// frame's LensFrame by slot).  Neither is timed or tuned: they serve a host's Li, one call per vertex of a batch.
#ifndef PG_CAMERAQUERY_H
#define PG_CAMERAQUERY_H

// PgCameraRay of samples 0 .. n-1: one thread per sample, the 96-byte record as six float4 stores.  The differentials are the ones Li receives: scaled by
// 1 / sqrt(spp) (integrator.cpp:282-283), as camera_differentials and lens_camera_sample leave them.
// ANIM: the camera moves (PgRenderDesc::camera_animated) -- the sample's camera-to-world matrix is interpolated at its time; a still camera's kernel does not
// carry that code.  REAL: the realistic camera -- the lens block staged from the call's LensFrame into LDS once per block, as k_generate<., true> stages a
// frame's, and the GenerateRay calls counted into that LensFrame's statistics as a frame counts them.
template <bool ANIM, bool REAL>
__global__ __launch_bounds__(PG_BLOCK) void k_camera_rays(RenderDescHead rdh, LensFrame *lf, const float *__restrict__ pFilm, const float *__restrict__ pLens,
                                                          const float *__restrict__ uTime, int n, float4 *__restrict__ out) {
    const PgLensSystem *lensLds = nullptr;
    if constexpr (REAL) {
        __shared__ uint32_t s_lensWords[sizeof(PgLensSystem) / 4];
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&lf->lens);
        for (int k = threadIdx.x; k < (int)(sizeof(PgLensSystem) / 4); k += PG_BLOCK) s_lensWords[k] = src[k];
        __syncthreads();
        lensLds = reinterpret_cast<const PgLensSystem *>(s_lensWords);
    }
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    const bool valid = i < n;
    int lensCalls = 0, lensVignetted = 0;
    bool lensZero = false;
    if (valid) {
        const PgRenderDesc &rd = rdh;
        const float pFilmX = pFilm[2 * (size_t)i], pFilmY = pFilm[2 * (size_t)i + 1];
        const float l0 = pLens ? pLens[2 * (size_t)i] : 0.f, l1 = pLens ? pLens[2 * (size_t)i + 1] : 0.f;
        const float rayTime = camera_time(rd, uTime ? uTime[i] : 0.f);
        V3 o = mk(0, 0, 0), d = mk(0, 0, 0);
        float tMax = 0, weight = 1;
        float4 diff[3];
        // (a function of the matrix, called below from the one place its instantiation keeps: a pointer that is either the description's matrix or a private
        // array would be a generic one)
        auto sample = [&](const float *c2w) {
            if constexpr (REAL) weight = lens_camera_sample(*lensLds, rd, c2w, pFilmX, pFilmY, l0, l1, o, d, tMax, lensCalls, lensVignetted, diff);
            else {
                V3 rxO, rxD, ryO, ryD;
                camera_ray(rd, c2w, pFilmX, pFilmY, l0, l1, o, d, tMax);
                camera_differentials(rd, c2w, pFilmX, pFilmY, l0, l1, o, d, rxO, rxD, ryO, ryD);
                diff[0] = make_float4(rxO.x, rxO.y, rxO.z, rxD.x); diff[1] = make_float4(rxD.y, rxD.z, ryO.x, ryO.y); diff[2] = make_float4(ryO.z, ryD.x, ryD.y, ryD.z);
            }
        };
        if constexpr (ANIM) {
            float c2w[16];
            camera_matrix_at(rd, rayTime, c2w);
            sample(c2w);
        } else sample(rd.camera_to_world);
        lensZero = weight == 0;
        float4 rec[6];
        for (int k = 0; k < 6; ++k) rec[k] = make_float4(0, 0, 0, 0);
        if (!lensZero) {  // (a vignetted sample: Li is not called, integrator.cpp:294-296 -- the record is zeros)
            rec[0] = make_float4(o.x, o.y, o.z, tMax);
            rec[1] = make_float4(d.x, d.y, d.z, rayTime);
            rec[2] = make_float4(weight, __int_as_float(rd.camera_medium), __int_as_float(1), 0.f);
            rec[3] = diff[0]; rec[4] = diff[1]; rec[5] = diff[2];
        }
        float4 *dst = out + 6 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 6; ++k) dst[k] = rec[k];
    }
    if constexpr (REAL) lens_stats_add(lf, lensCalls, lensVignetted, lensZero);
}
void launch_camera_rays(const PgRenderDesc &rd, LensFrame *lf, const float *pFilm, const float *pLens, const float *uTime, int n, PgCameraRay *out, hipStream_t s) {
    static_assert(sizeof(PgCameraRay) == 6 * sizeof(float4) && offsetof(PgCameraRay, differentials) == 3 * sizeof(float4), "PgCameraRay is six float4, the last three the differentials");
    if (n <= 0) return;
    RenderDescHead head;
    head = rd;
    const int nblk = (n + PG_BLOCK - 1) / PG_BLOCK;
    float4 *o4 = reinterpret_cast<float4 *>(out);
    const bool anim = rd.camera_animated != 0;  // (the camera's motion alone: no instance is met here)
    if (rd.camera_type == 3) {
        if (anim) hipLaunchKernelGGL((k_camera_rays<true, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, head, lf, pFilm, pLens, uTime, n, o4);
        else hipLaunchKernelGGL((k_camera_rays<false, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, head, lf, pFilm, pLens, uTime, n, o4);
    } else if (anim) hipLaunchKernelGGL((k_camera_rays<true, false>), dim3(nblk), dim3(PG_BLOCK), 0, s, head, lf, pFilm, pLens, uTime, n, o4);
    else hipLaunchKernelGGL((k_camera_rays<false, false>), dim3(nblk), dim3(PG_BLOCK), 0, s, head, lf, pFilm, pLens, uTime, n, o4);
}

// What tex_hit_setup is handed in place of a frame's description: zeros but for camera_type = 3, under which it reads NOTHING of the description, of a
// PathState or of a sampler and takes the ray's differentials from lens_frame(stL)->differentials + 3 * slot (pg_hit.h:184-187)
constexpr PgRenderDesc pg_scatter_diff_desc() { PgRenderDesc rd = {}; rd.camera_type = 3; return rd; }
__device__ const PgRenderDesc pg_scatter_diff_frame = pg_scatter_diff_desc();

// k_scatter<true, SAMPLE> (pg_scatter.h) for rays with differentials: the same functions in the same order, with tex_hit_setup handed slot = the ray's number, a
// `meta` with PG_META_HASDIFF and the description above.  A ray whose twelve floats are all zero has no differentials (PgCameraRay::has_differentials = 0 comes
// with zeros): its meta is the plain kernel's, and so are its bytes.
template <bool SAMPLE>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_scatter_diff(DScene sc, RayQueue q, const float4 *__restrict__ hits, const float *__restrict__ in, int flags,
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
            const float4 *df = lens_frame(stL)->differentials + 3 * (size_t)i;
            const float4 a = df[0], b = df[1], c = df[2];
            const bool hasDiff = ((__float_as_uint(a.x) | __float_as_uint(a.y) | __float_as_uint(a.z) | __float_as_uint(a.w) | __float_as_uint(b.x) | __float_as_uint(b.y) |
                                   __float_as_uint(b.z) | __float_as_uint(b.w) | __float_as_uint(c.x) | __float_as_uint(c.y) | __float_as_uint(c.z) | __float_as_uint(c.w)) << 1) != 0;  // (-0 is zero)
            LobeBsdfT<PgBxDF> lb;
            PgBxDF lobeStore[PG_MAX_BXDFS];
            TexHit th;
            tex_hit_setup(sc, pg_scatter_diff_frame, q, i, i, prim, tri, h4, rayD, outer, inner, quv, is, make_int4(0, 0, 0, hasDiff ? PG_META_HASDIFF : 0), 0.f, 0.f, false, false, 0, th, stL);
            material_bump(sc, tri.material, th, is);
            int nl = 0;
            float etaL = 1;
            MatEval<2>::run(*sc.self, tri.material, th, LobeOutRaw{lobeStore}, nl, etaL, PG_MAX_BXDFS);
            lbsdf_bind(lb, lobeStore, nl, etaL);
            lb.ns = is.ns; lb.ng = is.n;
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
void launch_scatter_diff(const DScene &sc, RayQueue q, const float4 *hits, const float *in, bool sample, int flags, const float4 *stL, PgScatter *out, hipStream_t s) {
    const int nblk = PG_REGIONS * (q.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    float4 *o4 = reinterpret_cast<float4 *>(out);
    if (sample) hipLaunchKernelGGL((k_scatter_diff<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, stL, o4);
    else hipLaunchKernelGGL((k_scatter_diff<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, in, flags, stL, o4);
}
#endif
