// pg_mediumquery.h -- the kernels of the medium queries (pg_transmittance_at / pg_intersect_tr_at / pg_medium_sample_at, pg_abi.hip's mediumQuery):
// VisibilityTester::Tr (light.cpp:63-81), Scene::IntersectTr (scene.cpp:57-70) and Medium::Sample (homogeneous.cpp:49-74, grid.cpp:61-86), for an
// integrator whose Li stays on the host.  Included at the end of pg_kernels.hip, like pg_lightquery.h.
//
// The two walks are k_through's loop (pg_kernels.hip) with the per-ray state carried by the ray's TAG -- the original ray number in d.w, as
// k_pack_rays leaves it -- instead of a path slot: every pass is one closest-hit launch over the rays still under way followed by k_tr_step, which
// finishes a ray into its record or appends the re-spawned ray to the other queue.  The kernels are wiring: the segments' transmittance is
// medium_tr's / grid_tr's, the point stepped over through_point's, the interface prim_interface's, the re-spawned rays shadow_ray_to's and
// offset_ray_origin's -- the functions k_through calls.  One thread per entry, PG_SHADE_BLOCK threads per block, no LDS.
#ifndef PG_MEDIUMQUERY_H
#define PG_MEDIUMQUERY_H

// The wave's `push` lanes take consecutive entries of region blockIdx.x % PG_REGIONS of q: one atomic per wave on the region counter
// (k_light_sample's append).  Every lane of the block calls it; -1 for a lane that pushes nothing.
PG_DEV int wave_append(const RayQueue &q, bool push) {
    const unsigned long long m = __ballot(push);
    const int lane = lane_id(), r = blockIdx.x & (PG_REGIONS - 1);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(&q.counts[r * PG_COUNT_STRIDE], __popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    return push ? r * q.regionCap + base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}
// PgTransmittance as its two float4
PG_DEV void store_transmittance(float4 *__restrict__ out, int tag, Spec Tr, int status, int medium, int crossings, int used) {
    float4 *dst = out + 2 * (size_t)tag;
    dst[0] = make_float4(Tr.r, Tr.g, Tr.b, __int_as_float(status));
    dst[1] = make_float4(__int_as_float(medium), __int_as_float(crossings), __int_as_float(used), __int_as_float(0));
}

// The start of both walks: ray i of the packed queue qin (entry i, k_pack_rays) with medium[i] in -1 .. nMedia-1 gets its state and a place in
// qout; any other index ends here with status -1 (and, where interactions are asked for, a record of zeros with prim -1) and is never traced.
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_tr_seed(int nMedia, RayQueue qin, const float *__restrict__ timesIn, const int *__restrict__ medium,
                                                             const float *__restrict__ p1, int n, TrState st, RayQueue qout, float *__restrict__ timesOut,
                                                             float4 *__restrict__ out, float4 *__restrict__ isect) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    bool push = false;
    if (i < n) {
        const int med = medium[i];
        push = med >= -1 && med < nMedia;
        if (push) {
            st.tr[i] = make_float4(1.f, 1.f, 1.f, __int_as_float(med + 1));
            st.cnt[i] = make_int2(0, 0);
            if (p1) { const size_t k = 3 * (size_t)i; st.p1[i] = make_float4(p1[k], p1[k + 1], p1[k + 2], 0.f); }
        } else {
            store_transmittance(out, i, sp(0.f), -1, 0, 0, 0);
            if (isect) {
                float4 *dst = isect + 8 * (size_t)i;
                dst[0] = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 1; k < 8; ++k) dst[k] = make_float4(0, 0, 0, 0);
            }
        }
    }
    const int pos = wave_append(qout, push);
    if (push) { qout.o[pos] = qin.o[i]; qout.d[pos] = qin.d[i]; timesOut[pos] = timesIn[i]; }
}

// One pass of a walk over the entries of qin after their closest-hit launch (hits, hitT, sc.hitInst / sc.animXf by entry).
// ISECT_TR = false, VisibilityTester::Tr: a hit on a primitive with a material blocks (Tr = 0, nothing drawn for that segment); otherwise the segment's
// Tr is applied and a hit re-spawns the ray towards p1 (isect.SpawnRayTo(p1), in isect.GetMedium(d)).
// ISECT_TR = true, Scene::IntersectTr: the segment's Tr is applied first, a hit on a material ends the walk, any other hit re-spawns the ray along its
// direction with tMax = inf (isect.SpawnRay(ray.d)); isectIn = k_interaction's records of this pass by entry, copied to isectOut[tag] where the walk ends.
// GRID: the scene has a GridDensityMedium; its ratio tracking draws u[tag * nU + used++], or 0.5 beyond the stream (`used` keeps counting).
template <bool ISECT_TR, bool GRID>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_tr_step(DScene sc, RayQueue qin, const float *__restrict__ timesIn, const float4 *__restrict__ hits,
                                                             const float *__restrict__ hitT, TrState st, const float *__restrict__ u, int nU, RayQueue qout,
                                                             float *__restrict__ timesOut, float4 *__restrict__ out, const float4 *__restrict__ isectIn,
                                                             float4 *__restrict__ isectOut) {
    const int i = queue_item<PG_SHADE_BLOCK>(qin);
    bool push = false;
    float4 no = make_float4(0, 0, 0, 0), nd = make_float4(0, 0, 0, 0);
    if (i >= 0) {
        const float4 o4 = qin.o[i], d4 = qin.d[i];
        const int tag = __float_as_int(d4.w);
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const float4 h4 = hits[i];
        const int prim = __float_as_int(h4.x);
        const bool surface = prim >= 0;
        const float4 acc = st.tr[tag];
        const int2 cnt = st.cnt[tag];
        Spec Tr = sp3(acc.x, acc.y, acc.z);
        int med = __float_as_int(acc.w), crossings = cnt.x, used = cnt.y;
        Tri tri;
        if (surface) tri = load_tri(sc, prim);
        const bool opaque = surface && sc.materials[tri.material].type != PG_MAT_NONE;  // isect.primitive->GetMaterial() != nullptr
        if (!ISECT_TR && opaque) Tr = sp(0.f);  // light.cpp:70-72: blocked
        else if (GRID && med && sc.mediaGrid[med - 1] >= 0) {
            const PgDensityGrid &gd = sc.grids[sc.mediaGrid[med - 1]];
            const float *stream = u + (size_t)tag * (size_t)nU;
            auto draw = [&]() -> float { const int k = used++; return k < nU ? stream[k] : 0.5f; };
            Tr = Tr * sp(grid_tr(gd, sc.gridDensity + gd.density_offset, mk(o4.x, o4.y, o4.z), rayD, surface ? hitT[i] : o4.w, draw));
        } else if (med) Tr = Tr * medium_tr(sc.media[med - 1], surface ? hitT[i] : o4.w, sqrtf(lensq(rayD)));
        if (surface && !opaque) {
            // a surface without a material: step over it (light.cpp:79 isect.SpawnRayTo(p1), scene.cpp:68 isect.SpawnRay(ray.d))
            V3 p, pError, n;
            through_point<true>(sc, i, o4, rayD, h4, prim, tri, p, pError, n);
            int mIn, mOut;
            prim_interface(sc, prim, med, mIn, mOut);
            V3 d = rayD;
            if (!ISECT_TR) {  // on towards the point the caller gave (interaction.h:69-72: a bare point has neither error bounds nor a normal)
                const float4 a = st.p1[tag];
                const LightSample ls = {mk(a.x, a.y, a.z), mk(0, 0, 0), mk(0, 0, 0)};
                d = shadow_ray_to(p, pError, n, ls, tag, no, nd);
            } else {
                const V3 origin = offset_ray_origin(p, pError, n, rayD);
                no = make_float4(origin.x, origin.y, origin.z, PG_INF);
                nd = make_float4(d.x, d.y, d.z, __int_as_float(tag));
            }
            med = dot(d, n) > 0 ? mOut : mIn;
            ++crossings;
            push = true;
            st.tr[tag] = make_float4(Tr.r, Tr.g, Tr.b, __int_as_float(med));
            st.cnt[tag] = make_int2(crossings, used);
        } else {
            store_transmittance(out, tag, Tr, opaque ? 1 : 0, med - 1, crossings, used);
            if (ISECT_TR && isectOut) {
                const float4 *src = isectIn + 8 * (size_t)i;
                float4 *dst = isectOut + 8 * (size_t)tag;
#pragma unroll
                for (int k = 0; k < 8; ++k) dst[k] = src[k];
            }
        }
    }
    // every lane of the block is here
    const int pos = wave_append(qout, push);
    if (push) { qout.o[pos] = no; qout.d[pos] = nd; timesOut[pos] = timesIn[i]; }
}

// PgMediumSample of rays 0 .. n-1: Medium::Sample(ray, sampler, arena, &mi) of medium[i] on the ray as Scene::Intersect left it (tmax), the 64-byte
// record as four float4 stores.  A HomogeneousMedium always draws two numbers (homogeneous.cpp:51-54), a GridDensityMedium tracks until it scatters
// or leaves (grid.cpp:71-84); the draws are u[i * nU + k], 0.5 beyond the stream.  Nothing is traced.
template <bool GRID>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_medium_sample(DScene sc, int nMedia, const float *__restrict__ o, const float *__restrict__ d,
                                                                   const float *__restrict__ tmax, const int *__restrict__ medium, const float *__restrict__ u,
                                                                   int nU, int n, float4 *__restrict__ out) {
    const int i = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int med = medium[i];
    float4 rec[4];
    for (int k = 0; k < 4; ++k) rec[k] = make_float4(0, 0, 0, 0);
    rec[0].x = __int_as_float(-1);
    if (med >= 0 && med < nMedia) {
        const size_t k3 = 3 * (size_t)i;
        const V3 ro = mk(o[k3], o[k3 + 1], o[k3 + 2]), rd = mk(d[k3], d[k3 + 1], d[k3 + 2]);
        const float tMaxRay = tmax[i];
        const PgMedium &mm = sc.media[med];
        const float *stream = u + (size_t)i * (size_t)nU;
        int used = 0;
        auto draw = [&]() -> float { const int k = used++; return k < nU ? stream[k] : 0.5f; };
        bool inMedium;
        float t = tMaxRay;
        Spec beta = sp(1.f);
        if (GRID && sc.mediaGrid[med] >= 0) {  // GridDensityMedium::Sample: delta tracking
            const PgDensityGrid &gd = sc.grids[sc.mediaGrid[med]];
            float tg = 0;
            inMedium = grid_sample(gd, sc.gridDensity + gd.density_offset, ro, rd, tMaxRay, draw, tg);
            if (inMedium) { t = tg; beta = sp3(mm.sigma_s[0], mm.sigma_s[1], mm.sigma_s[2]) / gd.sigma_t; }
        } else {  // HomogeneousMedium::Sample
            int channel;
            float dist;
            const float uc = draw();
            homogeneous_sample_distance(mm, uc, draw(), channel, dist);
            beta = homogeneous_sample_weight(mm, dist, sqrtf(lensq(rd)), tMaxRay, t, inMedium);
        }
        const V3 p = inMedium ? ro + rd * t : mk(0, 0, 0);
        rec[0] = make_float4(__int_as_float(inMedium ? 1 : 0), __int_as_float(used), beta.r, beta.g);
        rec[1] = make_float4(beta.b, t, p.x, p.y);
        rec[2] = make_float4(p.z, -rd.x, -rd.y, -rd.z);
        rec[3] = make_float4(mm.g, __int_as_float(med), 0.f, 0.f);
    }
    float4 *dst = out + 4 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = rec[k];
}

void launch_tr_seed(int nMedia, RayQueue qin, const float *timesIn, const int32_t *medium, const float *p1, int n, TrState st, RayQueue qout, float *timesOut,
                    PgTransmittance *out, PgInteraction *isect, hipStream_t s) {
    static_assert(sizeof(PgTransmittance) == 2 * sizeof(float4) && sizeof(PgMediumSample) == 4 * sizeof(float4), "PgTransmittance is two float4, PgMediumSample four");
    if (n <= 0) return;
    const int nblk = (n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK;
    hipLaunchKernelGGL(k_tr_seed, dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, nMedia, qin, timesIn, medium, p1, n, st, qout, timesOut, reinterpret_cast<float4 *>(out),
                       reinterpret_cast<float4 *>(isect));
}
void launch_tr_step(const DScene &sc, bool isectTr, RayQueue qin, const float *timesIn, const float4 *hits, const float *hitT, TrState st, const float *u, int nU,
                    RayQueue qout, float *timesOut, PgTransmittance *out, const PgInteraction *isectIn, PgInteraction *isectOut, hipStream_t s) {
    const int nblk = PG_REGIONS * (qin.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    float4 *o4 = reinterpret_cast<float4 *>(out), *io = reinterpret_cast<float4 *>(isectOut);
    const float4 *ii = reinterpret_cast<const float4 *>(isectIn);
    const dim3 g(nblk), b(PG_SHADE_BLOCK);
    const bool grid = sc.nGrids > 0;
    if (isectTr && grid) hipLaunchKernelGGL((k_tr_step<true, true>), g, b, 0, s, sc, qin, timesIn, hits, hitT, st, u, nU, qout, timesOut, o4, ii, io);
    else if (isectTr) hipLaunchKernelGGL((k_tr_step<true, false>), g, b, 0, s, sc, qin, timesIn, hits, hitT, st, u, nU, qout, timesOut, o4, ii, io);
    else if (grid) hipLaunchKernelGGL((k_tr_step<false, true>), g, b, 0, s, sc, qin, timesIn, hits, hitT, st, u, nU, qout, timesOut, o4, ii, io);
    else hipLaunchKernelGGL((k_tr_step<false, false>), g, b, 0, s, sc, qin, timesIn, hits, hitT, st, u, nU, qout, timesOut, o4, ii, io);
}
void launch_medium_sample(const DScene &sc, int nMedia, const float *o, const float *d, const float *tmax, const int32_t *medium, const float *u, int nU, int n,
                          PgMediumSample *out, hipStream_t s) {
    if (n <= 0) return;
    const int nblk = (n + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK;
    float4 *o4 = reinterpret_cast<float4 *>(out);
    if (sc.nGrids > 0) hipLaunchKernelGGL((k_medium_sample<true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, nMedia, o, d, tmax, medium, u, nU, n, o4);
    else hipLaunchKernelGGL((k_medium_sample<false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, nMedia, o, d, tmax, medium, u, nU, n, o4);
}
#endif
