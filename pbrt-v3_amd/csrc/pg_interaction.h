// pg_interaction.h -- the kernels of the ray queries (pg_intersect[_p] and pg_intersect_at / pg_intersect_p_at, pg_abi.hip's rayQuery): the rays into
// the test queue, the results out of it -- for the _at pair Scene::Intersect's SurfaceInteraction per ray at the ray's time, for an integrator whose
// Li stays on the host.  Included at the end of pg_kernels.hip, like pg_direct.h:
// the interaction is hit_isect's (pg_hit.h), under the transforms k_trace left for the hit (hitInst, animXf at the ray's time) -- the very functions
// the shading kernels call, nothing restated.  No material is evaluated: Material::Bump belongs to ComputeScatteringFunctions, not to Intersect.
//
// The queue is the entry points' test queue: ray i is entry i (the regions are filled front to back), its time is float i behind `d`
// (PG_QUEUE_TIMES's layout, kept for every scene: a still scene's k_trace does not read it, the record reports it).
#ifndef PG_INTERACTION_H
#define PG_INTERACTION_H

// The rays as the caller holds them (three floats per origin and direction, device memory) into the test queue, its region counters included.
__global__ __launch_bounds__(PG_BLOCK) void k_pack_rays(const float *__restrict__ o, const float *__restrict__ d, const float *__restrict__ tmax,
                                                         const float *__restrict__ time, int n, RayQueue q, float *__restrict__ times) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i < PG_REGIONS) {  // region r holds rays [r * cap, r * cap + count(r))
        const long long left = (long long)n - (long long)i * q.regionCap;
        q.counts[i * PG_COUNT_STRIDE] = (int)(left < 0 ? 0 : (left > q.regionCap ? q.regionCap : left));
    }
    if (i >= n) return;
    const size_t k = 3 * (size_t)i;
    q.o[i] = make_float4(o[k], o[k + 1], o[k + 2], tmax[i]);
    q.d[i] = make_float4(d[k], d[k + 1], d[k + 2], __int_as_float(i));
    times[i] = time ? time[i] : 0.f;
}
void launch_pack_rays(const float *o, const float *d, const float *tmax, const float *time, int n, RayQueue q, float *times, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pack_rays, dim3((n + PG_BLOCK - 1) / PG_BLOCK), dim3(PG_BLOCK), 0, s, o, d, tmax, time, n, q, times);
}

// PgInteraction of every entry of q after its closest-hit launch (hits, tHit = ray.tMax as k_trace left it, sc.hitInst / sc.animXf): one thread per ray,
// the 128-byte record as eight float4 stores -- a lane fills one whole 128-B line.
__global__ __launch_bounds__(PG_BLOCK) void k_interaction(DScene sc, RayQueue q, const float4 *__restrict__ hits, const float *__restrict__ tHit,
                                                           const float *__restrict__ times, float4 *__restrict__ out) {
    const int i = queue_item<PG_BLOCK>(q);
    if (i < 0) return;
    const float4 o4 = q.o[i], d4 = q.d[i], h4 = hits[i];
    const int prim = __float_as_int(h4.x);
    float4 rec[8];
    for (int k = 0; k < 8; ++k) rec[k] = make_float4(0, 0, 0, 0);
    rec[0].x = __int_as_float(prim);
    rec[1].y = tHit[i]; rec[1].z = times[i];
    if (prim >= 0) {
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const Tri tri = load_tri(sc, prim);
        int inst = sc.hitInst ? sc.hitInst[i] : -1, inst2;
        nest_decode(sc, inst, inst2);
        const InstXf outer = inst_xf(sc, inst, i), inner = inst_xf(sc, inst2, i, true);
        QuadricUv quv;
        const Isect is = hit_isect(sc, outer, inner, o4, rayD, h4, prim, tri, quv);
        float u = quv.u, v = quv.v;
        if (!quv.on) {  // uvHit, triangle.cpp:332 (as tex_hit_setup forms it)
            float uv[6];
            load_uv(sc, prim, tri.flags, uv);
            u = h4.y * uv[0] + h4.z * uv[2] + h4.w * uv[4];
            v = h4.y * uv[1] + h4.z * uv[3] + h4.w * uv[5];
        }
        rec[0].y = __int_as_float(inst); rec[0].z = __int_as_float(inst2); rec[0].w = __int_as_float(tri.material);
        rec[1].x = __int_as_float(tri.light); rec[1].w = u;
        rec[2] = make_float4(v, is.p.x, is.p.y, is.p.z);
        rec[3] = make_float4(is.pError.x, is.pError.y, is.pError.z, is.n.x);
        rec[4] = make_float4(is.n.y, is.n.z, is.wo.x, is.wo.y);
        rec[5] = make_float4(is.wo.z, is.ns.x, is.ns.y, is.ns.z);
        rec[6] = make_float4(is.sdpdu.x, is.sdpdu.y, is.sdpdu.z, is.sdpdv.x);
        rec[7] = make_float4(is.sdpdv.y, is.sdpdv.z, 0.f, 0.f);
    }
    float4 *dst = out + 8 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = rec[k];
}
void launch_interaction(const DScene &sc, RayQueue q, const float4 *hits, const float *tHit, const float *times, PgInteraction *out, hipStream_t s) {
    static_assert(sizeof(PgInteraction) == 8 * sizeof(float4), "PgInteraction is eight float4");
    const int nblk = PG_REGIONS * (q.regionCap / PG_BLOCK);
    if (nblk == 0) return;
    hipLaunchKernelGGL(k_interaction, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, q, hits, tHit, times, reinterpret_cast<float4 *>(out));
}

// pg_intersect's arrays from the closest-hit launch's records: the primitive, t = ray.tMax as k_trace left it, the barycentrics (0 on a miss)
__global__ __launch_bounds__(PG_BLOCK) void k_hit_arrays(const float4 *__restrict__ hits, const float *__restrict__ tHit, int32_t *__restrict__ prim,
                                                          float *__restrict__ t, float *__restrict__ bary, int n) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 h4 = hits[i];
    const bool hit = __float_as_int(h4.x) >= 0;
    const size_t k = 3 * (size_t)i;
    prim[i] = __float_as_int(h4.x);
    t[i] = tHit[i];
    bary[k] = hit ? h4.y : 0.f; bary[k + 1] = hit ? h4.z : 0.f; bary[k + 2] = hit ? h4.w : 0.f;
}
void launch_hit_arrays(const float4 *hits, const float *tHit, int32_t *prim, float *t, float *bary, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_hit_arrays, dim3((n + PG_BLOCK - 1) / PG_BLOCK), dim3(PG_BLOCK), 0, s, hits, tHit, prim, t, bary, n);
}

// k_trace's any-hit answers (one int per ray) as the entry point's bytes
__global__ __launch_bounds__(PG_BLOCK) void k_occluded_bytes(const int *__restrict__ occluded, uint8_t *__restrict__ out, int n) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i < n) out[i] = occluded[i] ? 1 : 0;
}
void launch_occluded_bytes(const int *occluded, uint8_t *out, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_occluded_bytes, dim3((n + PG_BLOCK - 1) / PG_BLOCK), dim3(PG_BLOCK), 0, s, occluded, out, n);
}
#endif
