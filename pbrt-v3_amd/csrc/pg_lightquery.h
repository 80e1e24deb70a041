// pg_lightquery.h -- the kernels of the light queries (pg_light_sample_at / pg_light_pdf_at / pg_light_le_at, pg_abi.hip's lightQuery and rayQuery):
// Light::Sample_Li with the VisibilityTester's ray, Light::Pdf_Li, and the radiance a ray meets (isect.Le(-ray.d) at an emissive hit, the infinite
// lights' Le(ray) for an escaped ray), for an integrator whose Li stays on the host.  Included at the end of pg_kernels.hip, like pg_scatter.h.
//
// The kernels are wiring: the sample is load_light_hot + light_sample_li_hot's (pg_light.h), the shadow ray shadow_ray_to's, Pdf_Li is mis_light_of +
// mis_light_pdf's, an emitter's L area_light_le's (pg_hit.h) and an infinite light's env_le's -- the functions the shading kernels call.  EXT as in
// light_sample_li: the plain instantiations serve scenes of triangles with area and delta lights.  One thread per sample, PG_SHADE_BLOCK threads per
// block, no LDS.  Tr through media is pg_mediumquery.h; Sample_Le / Pdf_Le and light-selection distributions are not built.
#ifndef PG_LIGHTQUERY_H
#define PG_LIGHTQUERY_H

// What the light queries read of a reference point: the PgInteraction record's float4s 0 .. 4 (prim; time; p; p_error and n)
struct LightRef { int prim; float time; V3 p, pError, n; };
PG_DEV LightRef load_light_ref(const float4 *__restrict__ ref, int i) {
    const float4 *r = ref + 8 * (size_t)i;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
    LightRef lr;
    lr.prim = __float_as_int(r0.x);
    lr.time = r1.z;
    lr.p = mk(r2.y, r2.z, r2.w);
    lr.pError = mk(r3.x, r3.y, r3.z);
    lr.n = mk(r3.w, r4.x, r4.y);
    return lr;
}

// PgLightSample of samples 0 .. n-1: Light::Sample_Li(ref[i], u[2i .. 2i+1]) of light[i], the 64-byte record as four float4 stores -- two lanes fill
// one 128-B line -- and, unless `shadow` is null, the ray of p0.SpawnRayTo(p1) as two more.  A sample with pdf > 0 and a non-black Li (what
// EstimateDirect tests, integrator.cpp:128-151) appends that ray to q with i as its tag and ref[i].time as its time: one atomic per wave on the
// region counter of the block (block_push's regions, without its LDS: nothing else is appended here).  `visibility` stays -1 until
// k_light_visibility has the trace's answer.
template <bool EXT>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_light_sample(DScene sc, const float4 *__restrict__ ref, const int *__restrict__ light, const float *__restrict__ u,
                                                                  int n, RayQueue q, float *__restrict__ times, float4 *__restrict__ out, float4 *__restrict__ shadow) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    bool push = false;
    float4 shO = make_float4(0, 0, 0, 0), shD = shO;
    float time = 0;
    if (i < n) {
        const LightRef lr = load_light_ref(ref, i);
        const int li = light[i];
        const float u0 = u[2 * (size_t)i], u1 = u[2 * (size_t)i + 1];
        float4 rec[4];
        for (int k = 0; k < 4; ++k) rec[k] = make_float4(0, 0, 0, 0);
        rec[0].x = __int_as_float(-1);
        if (lr.prim >= 0 && li >= 0 && li < sc.nLights) {
            const LightHot lh = load_light_hot(sc, li);
            V3 wi = mk(0, 0, 0);
            float pdf = 0;
            LightSample ls;
            Spec Li = light_sample_li_hot<EXT>(sc, lh, sc.lights[li], lr.p, lr.pError, lr.n, u0, u1, wi, pdf, ls);
            if (pdf == 0) { Li = sp(0); wi = mk(0, 0, 0); ls.p = ls.n = mk(0, 0, 0); }  // (no sample: the reference leaves wi and the tester unset)
            push = pdf > 0 && !is_black(Li);
            if (push) { shadow_ray_to(lr.p, lr.pError, lr.n, ls, i, shO, shD); time = lr.time; }
            rec[0] = make_float4(__int_as_float(li), __int_as_float(-1), pdf, Li.r);
            rec[1] = make_float4(Li.g, Li.b, wi.x, wi.y);
            rec[2] = make_float4(wi.z, ls.p.x, ls.p.y, ls.p.z);
            rec[3] = make_float4(ls.n.x, ls.n.y, ls.n.z, 0.f);
        }
        float4 *dst = out + 4 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = rec[k];
        if (shadow) {  // origin, tMax = 1 - ShadowEpsilon, direction, time: zeros where nothing is tested
            shadow[2 * (size_t)i] = shO;
            shadow[2 * (size_t)i + 1] = make_float4(shD.x, shD.y, shD.z, time);
        }
    }
    // every lane of the block is here: the wave's rays take consecutive entries of region blockIdx.x % PG_REGIONS
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
// `visibility` of the samples whose rays the any-hit launch traced: entry i of q answers for the record its tag names
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_light_visibility(RayQueue q, const int *__restrict__ occluded, int *__restrict__ out) {
    const int i = queue_item<PG_SHADE_BLOCK>(q);
    if (i < 0) return;
    const int tag = __float_as_int(q.d[i].w);
    out[16 * (size_t)tag + 1] = occluded[i] ? 0 : 1;
}
void launch_light_sample(const DScene &sc, const PgInteraction *ref, const int32_t *light, const float *u, int n, RayQueue q, float *times, PgLightSample *out,
                         float *shadow, hipStream_t s) {
    static_assert(sizeof(PgLightSample) == 4 * sizeof(float4) && sizeof(PgInteraction) == 8 * sizeof(float4), "PgLightSample is four float4, PgInteraction eight");
    if (n <= 0) return;
    const int nblk = (n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK;
    const float4 *r4 = reinterpret_cast<const float4 *>(ref);
    float4 *o4 = reinterpret_cast<float4 *>(out), *s4 = reinterpret_cast<float4 *>(shadow);
    if (sc.ext) hipLaunchKernelGGL((k_light_sample<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, r4, light, u, n, q, times, o4, s4);
    else hipLaunchKernelGGL((k_light_sample<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, r4, light, u, n, q, times, o4, s4);
}
void launch_light_visibility(RayQueue q, const int *occluded, PgLightSample *out, hipStream_t s) {
    const int nblk = PG_REGIONS * (q.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    hipLaunchKernelGGL(k_light_visibility, dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, q, occluded, reinterpret_cast<int *>(out));
}

// pdf[i] = Light::Pdf_Li(ref[i], wi[3i .. 3i+2]) of light[i]: 0 for a delta light (and an invalid ref or index); an area light's Shape::Pdf against its
// own shape, on the ray ref.SpawnRay(wi) (shape.cpp:72-87, Sphere::Pdf for a sphere); InfiniteAreaLight::Pdf_Li.  No statistic is counted.
template <bool EXT>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_light_pdf(DScene sc, const float4 *__restrict__ ref, const int *__restrict__ light, const float *__restrict__ wi3,
                                                               int n, float *__restrict__ pdf) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const LightRef lr = load_light_ref(ref, i);
    const int li = light[i];
    const size_t k = 3 * (size_t)i;
    const V3 wi = mk(wi3[k], wi3[k + 1], wi3[k + 2]);
    float result = 0;
    if (lr.prim >= 0 && li >= 0 && li < sc.nLights) {
        const LightHot lh = load_light_hot(sc, li);
        if (lh.type == PG_LIGHT_AREA || (EXT && lh.type == PG_LIGHT_INFINITE)) {
            int lightPrim;
            bool inside;
            mis_light_of(sc, lh, li, lr.p, lr.pError, lr.n, lightPrim, inside);
            const V3 ro = offset_ray_origin(lr.p, lr.pError, lr.n, wi);  // ref.SpawnRay(wi), interaction.h:64-67
            unsigned int nLightTests = 0;
            result = mis_light_pdf<EXT>(sc, lightPrim, lh.area, inside, lr.p, ro, wi, nLightTests);
        }
    }
    pdf[i] = result;
}
void launch_light_pdf(const DScene &sc, const PgInteraction *ref, const int32_t *light, const float *wi, int n, float *pdf, hipStream_t s) {
    if (n <= 0) return;
    const int nblk = (n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK;
    const float4 *r4 = reinterpret_cast<const float4 *>(ref);
    if (sc.ext) hipLaunchKernelGGL((k_light_pdf<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, r4, light, wi, n, pdf);
    else hipLaunchKernelGGL((k_light_pdf<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, r4, light, wi, n, pdf);
}

// Le[3i .. 3i+2] of every entry of q after its closest-hit launch (ray i is entry i): isect.Le(-ray.d) at a hit (interaction.cpp:149-152: the
// primitive's area light's L with the hit's normal, 0 without one), and for an escaped ray the infinite lights' Le(ray) summed in lights[] order
// from 0 (path.cpp:81-85)
template <bool EXT>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_emitted(DScene sc, RayQueue q, const float4 *__restrict__ hits, float *__restrict__ Le) {
    const int i = queue_item<PG_SHADE_BLOCK>(q);
    if (i < 0) return;
    const float4 o4 = q.o[i], d4 = q.d[i], h4 = hits[i];
    const int prim = __float_as_int(h4.x);
    const V3 rayD = mk(d4.x, d4.y, d4.z);
    Spec L = sp(0);
    if (prim >= 0) {
        const Tri tri = load_tri(sc, prim);
        if (tri.light >= 0) L = area_light_le<EXT>(sc, sc.lights[tri.light], prim, tri, h4, o4, rayD);
    } else if (EXT) {
        for (int li = 0; li < sc.nLights; ++li)
            if (sc.lights[li].type == PG_LIGHT_INFINITE) L = L + env_le(sc, sc.lights[li], rayD);
    }
    const size_t k = 3 * (size_t)i;
    Le[k] = L.r; Le[k + 1] = L.g; Le[k + 2] = L.b;
}
void launch_emitted(const DScene &sc, RayQueue q, const float4 *hits, float *Le, hipStream_t s) {
    const int nblk = PG_REGIONS * (q.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    if (sc.ext) hipLaunchKernelGGL((k_emitted<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, Le);
    else hipLaunchKernelGGL((k_emitted<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, q, hits, Le);
}
#endif
