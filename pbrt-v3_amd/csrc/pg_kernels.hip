// pg_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4) of the wavefront
// PathIntegrator.  One process per GPU; every kernel works on SoA ray queues
// (32 B/ray as two float4) instead of pbrt's per-ray recursion:
//
//   k_generate   HaltonSampler + PerspectiveCamera   (sampler.cpp:46-52, halton.cpp:96-127, perspective.cpp:95-144)
//   k_trace      BVHAccel::Intersect / IntersectP + Triangle::Intersect[P]  (pg_traverse.hip)
//   k_shade      PathIntegrator::Li loop body + EstimateDirect set-up      (path.cpp:81-187, integrator.cpp:85-215)
//   k_resolve    EstimateDirect's visibility / MIS terms once rays are back (integrator.cpp:143-212)
//   k_film       SamplerIntegrator::Render's scrub + FilmTile::AddSample    (integrator.cpp:294-320, film.h:121-161; pg_film.h)
//   k_light_tables  SpatialLightDistribution::ComputeDistribution per voxel (lightdistrib.cpp:232-300; pg_lightdistrib.h)
//   k_direct     DirectLightingIntegrator::Li, one (light, sample) step per launch (directlighting.cpp:62-95; pg_direct.h, included at the end)
//   k_interaction  Scene::Intersect's SurfaceInteraction per ray, for pg_intersect_at (pg_interaction.h, included at the end)
//   k_scatter    BSDF::f / Pdf / Sample_f at a ray's closest hit, for pg_scatter_f_at / pg_scatter_sample_at (pg_scatter.h, included at the end)
//   k_light_sample / k_light_visibility / k_light_pdf / k_emitted  Light::Sample_Li with its visibility, Pdf_Li and the radiance a ray meets, for
//                pg_light_sample_at / pg_light_pdf_at / pg_light_le_at (pg_lightquery.h, included at the end)
//   k_tr_seed / k_tr_step / k_medium_sample  VisibilityTester::Tr, Scene::IntersectTr and Medium::Sample per ray, for pg_transmittance_at /
//                pg_intersect_tr_at / pg_medium_sample_at (pg_mediumquery.h, included at the end)
//   k_sss_seed / k_sss_tally / k_sss_emit / k_adapter  BSSRDF::Sample_S per ray around k_sss_probe's chains and the exit point's adapter BSDF, for
//                pg_subsurface_sample_at / pg_subsurface_f_at / pg_subsurface_sample_f_at (pg_subsurfacequery.h, included at the end)
//
// No MFMA: there is no dense contraction on this path; traversal is a
// latency/bandwidth-bound gather over the node and triangle arrays.
//
// This file holds the kernels and their launch_* wrappers only.  The device functions they are built from live in headers, by subject:
// pg_queue.h (queue append, statistics), pg_triangle.h (Tri, Isect, make_isect), pg_sampler.h, pg_camera.h, pg_bxdf.h (Bsdf, LobeBsdfT,
// AdapterBsdf), pg_material.h (MatEval), pg_light.h, pg_medium.h, pg_hit.h (the interaction of any hit; it uses the others), pg_estimate.h
// (EstimateDirect's set-up over any of the scattering models), pg_resolve.h (the record that set-up leaves and EstimateDirect's sums once the rays are
// back: every k_resolve*, k_direct_fold and QueueState::pend), pg_film.h (FilmTile::AddSample and the sample scrub of the three film kernels) and
// pg_lightdistrib.h (ComputeDistribution of the two light-table kernels) -- beside pg_device.h, pg_sphere.h, pg_texture.h, pg_motion.h,
// pg_bssrdf.h, pg_grid.h and pg_lens.h.  A helper of a single kernel (resolve_entry, through_point) stays with its kernel, and so do
// halton_batch and sample_discrete, below the includes.
#include "pg_device.h"
#include "pg_sphere.h"
#include "pg_kernels.h"
#include "pg_texture.h"
#include "pg_motion.h"
#include "pg_bssrdf.h"
#include "pg_grid.h"
#include "pg_lens.h"
#include "pg_queue.h"
#include "pg_triangle.h"
#include "pg_sampler.h"
#include "pg_camera.h"
#include "pg_bxdf.h"
#include "pg_material.h"
#include "pg_light.h"
#include "pg_medium.h"
#include "pg_hit.h"
#include "pg_resolve.h"
#include "pg_estimate.h"
#include "pg_film.h"
#include "pg_lightdistrib.h"

// ---- the two device functions that stay here: each holds an empty `asm volatile` register-scheduling barrier, which the emulated-device
// build (tests/emu/build_emulated.py) drops from this file by text, and only the kernels below call them ----------------------------
// The N Halton dimensions dim0 .. dim0+N-1 of one sample index at once (HaltonSampler::SampleDimension for each, halton.cpp:119-127
// + ScrambledRadicalInverse, lowdiscrepancy.cpp:405-424): the digit loops of the N dimensions run side by side, so the N
// permutation-table loads of a digit position are in flight together and the wave waits once per digit position instead of
// once per digit of every dimension (a shading wave spent a third of its time in these loops, profiles/r02s_*).  Per
// dimension the operations and their order are those of scrambled_radical_inverse().  dim0 is the same in every lane
// (the caller checks), so bases and table offsets are scalar; the index must fit 32 bits.
template <int N>
PG_DEV void halton_batch(const DScene &sc, uint32_t a0, int dim0, float *out) {
    uint32_t base[N], off[N], mul[N], sh[N], a[N];
    uint64_t rev[N];
    float invBase[N], tail[N], invBaseN[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int d = dim0 + j;
        if (d >= sc.nPermDims) d = sc.nPermDims - 1;
        const int4 hd = sc.haltonDims[2 * d], hc = sc.haltonDims[2 * d + 1];
        base[j] = (uint32_t)hd.x; off[j] = (uint32_t)hd.y; mul[j] = (uint32_t)hd.z; sh[j] = (uint32_t)hd.w - 1u;
        invBase[j] = __int_as_float(hc.x); tail[j] = __int_as_float(hc.y);
        a[j] = a0; rev[j] = 0; invBaseN[j] = 1;
    }
    uint32_t any = a0;
    while (any) {
        any = 0;
        uint32_t next[N], p[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {  // the digit of every dimension, and its table entry on the way
            const uint32_t t = __umulhi(mul[j], a[j]);
            next[j] = (t + ((a[j] - t) >> 1)) >> sh[j];  // = a[j] / base[j] (DScene::haltonDims)
            p[j] = sc.perms[off[j] + (a[j] - next[j] * base[j])];
        }
        // all N loads are issued before the first is used (left alone, the compiler sinks each into the branch it makes of the
        // select below and waits for them one by one)
        static_assert(N == 7, "halton_batch: the barrier below names seven values");
        asm volatile("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]), "+v"(p[4]), "+v"(p[5]), "+v"(p[6]));
#pragma unroll
        for (int j = 0; j < N; ++j) {
            // a dimension whose digits are used up stays as it is: it is multiplied by one and gets zero added (exact), which
            // keeps the loop body free of branches
            const bool act = a[j] != 0;
            rev[j] = rev[j] * (act ? base[j] : 1u) + (act ? p[j] : 0u);
            invBaseN[j] *= act ? invBase[j] : 1.f;
            a[j] = next[j];
            any |= next[j];
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
        out[j] = pmin(invBaseN[j] * ((float)rev[j] + tail[j]), PG_ONE_MINUS_EPS);
}
// Distribution1D::SampleDiscrete, sampling.h:90-100 + FindInterval pbrt.h:403-415
PG_DEV int sample_discrete(const float *tab, int n, float u, float &pdf) {
    if (n <= 3) {
        // a table of at most 8 floats (func[n], cdf[n+1], funcInt) is fetched in ONE round trip and searched in registers; the
        // general path below meets it with three or four dependent loads (funcInt, the cdf entries of the search, func)
        float row[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) row[k] = k < 2 * n + 2 ? tab[k] : 0.f;
        asm volatile("" : "+v"(row[0]), "+v"(row[1]), "+v"(row[2]), "+v"(row[3]), "+v"(row[4]), "+v"(row[5]), "+v"(row[6]), "+v"(row[7]));
        auto at = [&](int k) { return k == 0 ? row[0] : (k == 1 ? row[1] : (k == 2 ? row[2] : (k == 3 ? row[3] : (k == 4 ? row[4] : (k == 5 ? row[5] : (k == 6 ? row[6] : row[7])))))); };
        const float funcInt = at(2 * n + 1);
        int size = n + 1, first = 0, len = size;
        while (len > 0) {
            int half = len >> 1, middle = first + half;
            if (at(n + middle) <= u) { first = middle + 1; len -= half + 1; }
            else len = half;
        }
        int offset = first - 1;
        offset = offset < 0 ? 0 : (offset > size - 2 ? size - 2 : offset);
        pdf = (funcInt > 0) ? at(offset) / (funcInt * n) : 0;
        return offset;
    }
    const float *func = tab, *cdf = tab + n;
    float funcInt = tab[2 * n + 1];
    int size = n + 1, first = 0, len = size;
    while (len > 0) {
        int half = len >> 1, middle = first + half;
        if (cdf[middle] <= u) { first = middle + 1; len -= half + 1; }
        else len = half;
    }
    int offset = first - 1;
    offset = offset < 0 ? 0 : (offset > size - 2 ? size - 2 : offset);
    pdf = (funcInt > 0) ? func[offset] / (funcInt * n) : 0;
    return offset;
}

// tileSampler = sampler->Clone(seed), seed = tile.y * nTiles.x + tile.x (integrator.cpp:247-248); RNG::SetSequence, rng.h:129-135
__global__ void k_ts_init(DScene sc, RenderParams rp) {
    const int local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= rp.nTilesBatch) return;
    TileSamplerState t;
    t.state = 0u; t.inc = ((unsigned long long)(rp.rd->tile_first + local * rp.rd->tile_step) << 1u) | 1u;
    rng_u32(t);
    t.state += 0x853c49e6748fea9bULL;
    rng_u32(t);
    t.cur1D = t.cur2D = t.sampleIndex = t.active = 0; t.lens0 = t.lens1 = 0; t.px = t.py = 0; t.draws = 0; t.time = 0;
    sc.ts[local] = t;
}
__global__ void k_ts_start_pixel(DScene sc, RenderParams rp, int lx, int ly) {
    const int local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= rp.nTilesBatch) return;
    TileSamplerState t = sc.ts[local];
    int tile, px, py;
    const bool exists = ts_tile_pixel(rp, local, lx, ly, tile, px, py);
    t.active = 0;
    if (exists) {
        const PgRenderDesc &rd = rp.rd;
        const int n = sc.tsSpp, nd = sc.tsDims;
        ts_start_pixel(sc, rd, t, sc.ts1 + (size_t)local * nd * n, sc.ts2 + (size_t)local * nd * n * 2);
        t.px = px; t.py = py;
        t.active = px >= rd.pixel_bounds[0] && px < rd.pixel_bounds[2] && py >= rd.pixel_bounds[1] && py < rd.pixel_bounds[3];
    }
    sc.ts[local] = t;
}
// tsBatched: <Sampler>::StartPixel for ALL pixels of every tile (integrator.cpp:264-273; the tile's stream is consumed by StartPixel
// alone, pixel after pixel).  One block per tile, one thread per pixel: a StartPixel consumes a fixed count of numbers unless one of
// RNG::UniformUInt32(b)'s rejection loops repeats (rng.h:68-74: probability < b / 2^32 per call), so thread p starts from the tile's
// state advanced by (pixels before it) x (that count), generates its pixel's arrays, and reports what it really consumed; a prefix
// sum over the pixels gives the true starting points, and the pixels whose starting point was wrong run again -- until none is
// (one pass nearly always; a pass per rejection otherwise; the result is the sequential one whatever the first guess was).
__global__ __launch_bounds__(256) void k_ts_start_tile(DScene sc, RenderParams rp) {
    const int local = blockIdx.x, p = threadIdx.x;
    __shared__ unsigned int s_cnt[256];
    __shared__ unsigned long long s_start[256];
    __shared__ unsigned long long s_total;
    __shared__ int s_dirty;
    int tile, px, py;
    const bool exists = ts_tile_pixel(rp, local, p & 15, p >> 4, tile, px, py);
    const TileSamplerState t0 = sc.ts[local];
    const PgRenderDesc &rd = rp.rd;
    const unsigned long long n = (unsigned long long)sc.tsSpp, nd = (unsigned long long)sc.tsDims;
    // numbers one StartPixel takes when no rejection loop repeats (a first guess only)
    unsigned long long nominal = 0;
    if (rd.sampler == PG_SAMPLER_STRATIFIED) nominal = nd * ((rd.strat_jitter ? n : 0) + n) + nd * ((rd.strat_jitter ? 2 * n : 0) + n);
    else if (rd.sampler == PG_SAMPLER_ZEROTWO) nominal = nd * (2 * n + 1) + nd * (2 * n + 2);
    else if (rd.sampler == PG_SAMPLER_MAXMINDIST) nominal = n + nd * (2 * n + 1) + (nd - 1) * (2 * n + 2);
    nominal += (unsigned long long)(long long)rp.tsGuessSkew;
    const int x0 = rd.sample_bounds[0] + (tile % rp.nTilesX) * 16;
    const int wE = rd.sample_bounds[2] - x0 < 16 ? rd.sample_bounds[2] - x0 : 16;  // the tile's existing pixels: wE columns
    unsigned long long start = exists ? (unsigned long long)((p >> 4) * wE + (p & 15)) * nominal : 0;
    const size_t pixel = (size_t)local * 256 + p, len = (size_t)n * nd;
    bool dirty = exists;
    unsigned int cnt = 0;
    for (int pass = 0; pass < 300; ++pass) {
        if (dirty) {
            TileSamplerState t = t0;
            rng_advance(t, start);
            t.draws = 0;
            ts_start_pixel(sc, rd, t, sc.ts1 + pixel * len, sc.ts2 + pixel * len * 2);
            cnt = t.draws;
        }
        s_cnt[p] = exists ? cnt : 0;
        if (p == 0) s_dirty = 0;
        __syncthreads();
        if (p == 0) {
            unsigned long long acc = 0;
            for (int k = 0; k < 256; ++k) { s_start[k] = acc; acc += s_cnt[k]; }
            s_total = acc;
        }
        __syncthreads();
        dirty = exists && s_start[p] != start;
        start = s_start[p];
        if (dirty) s_dirty = 1;
        __syncthreads();
        if (!s_dirty) break;
        __syncthreads();
    }
    // 300 passes without a fixed point would need ~300 rejection-loop repeats inside one tile (probability < 1e-1000): said, not assumed
    if (p == 0 && s_dirty && sc.tsOverflow) atomicOr(sc.tsOverflow, 2);
    if (p == 0) { TileSamplerState t = t0; rng_advance(t, s_total); sc.ts[local] = t; }
}
void launch_ts_start_tile(const DScene &sc, const RenderParams &rp, hipStream_t s) {
    hipLaunchKernelGGL(k_ts_start_tile, dim3(rp.nTilesBatch), dim3(256), 0, s, sc, rp);
}
void launch_ts_init(const DScene &sc, const RenderParams &rp, hipStream_t s) {
    hipLaunchKernelGGL(k_ts_init, dim3((rp.nTilesBatch + 63) / 64), dim3(64), 0, s, sc, rp);
}
void launch_ts_start_pixel(const DScene &sc, const RenderParams &rp, int lx, int ly, hipStream_t s) {
    hipLaunchKernelGGL(k_ts_start_pixel, dim3((rp.nTilesBatch + 63) / 64), dim3(64), 0, s, sc, rp, lx, ly);
}

// REAL: the realistic camera (camera_type 3), an instantiation of its own chosen only for such frames: the lens block is staged from the frame's
// LensFrame into LDS once per block (1.5 KB; every lane walks the interfaces with a uniform index and picks a pupil box with its own), each sample
// runs 3 to 5 lens traces, and the sample's weight goes to the LensFrame's per-slot array.  A sample of weight 0 enters no queue: its path never
// starts (integrator.cpp:294-296: Li is not called), its L stays 0 and it still reaches the film.
template <bool ANIM, bool REAL = false>
__global__ __launch_bounds__(PG_BLOCK) void k_generate(DScene sc, RenderParams rp, PathState st, RayQueue q) {
    const PgLensSystem *lensLds = nullptr;
    if constexpr (REAL) {
        __shared__ uint32_t s_lensWords[sizeof(PgLensSystem) / 4];
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&lens_frame(st.L)->lens);
        for (int k = threadIdx.x; k < (int)(sizeof(PgLensSystem) / 4); k += PG_BLOCK) s_lensWords[k] = src[k];
        __syncthreads();
        lensLds = reinterpret_cast<const PgLensSystem *>(s_lensWords);
    }
    int slot = blockIdx.x * PG_BLOCK + threadIdx.x;
    bool valid = slot < rp.capacity;
    int px = 0, py = 0, sn = 0;
    if (valid) valid = slot_to_pixel(rp, slot, px, py, sn);
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    float tMax = PG_INF, rayTime = 0;
    int lensCalls = 0, lensVignetted = 0;
    bool lensZero = false;
    if (valid) {
        const PgRenderDesc &rd = rp.rd;
        uint64_t index = sc.tsBatched ? 0 : sampler_index(sc, rd, px, py, (uint64_t)sn);
        // GetCameraSample, sampler.cpp:46-52: dims 0,1 film; 2 time; 3,4 lens
        float u0 = 0, u1 = 0, tsl0 = 0, tsl1 = 0, uTime = 0;
        int tsDim = 0;
        if (sc.tsBatched) {  // a PixelSampler's arrays: film 2D, time 1D, lens 2D; the path's state names its pixel and sample
            const int pixel = (rp.tileLocal0 + (slot >> 8) / rp.sCount) * 256 + (slot & 255);
            index = (uint64_t)(uint32_t)pixel | ((uint64_t)(uint32_t)sn << 32);
            tsb_get2d(sc, pixel, sn, tsDim, u0, u1);
            uTime = tsb_get1d(sc, pixel, sn, tsDim);
            tsb_get2d(sc, pixel, sn, tsDim, tsl0, tsl1);
        } else { u0 = halton_sample(sc, rd, index, 0); u1 = halton_sample(sc, rd, index, 1); if (ANIM) uTime = halton_sample(sc, rd, index, 2); }
        if (rd.sampler == 1) {  // SobolSampler::SampleDimension, sobol.cpp:53-56
            u0 = u0 * rd.sobol_resolution + rd.sample_bounds[0];
            u0 = u0 - px;
            u0 = u0 < 0.f ? 0.f : (u0 > PG_ONE_MINUS_EPS ? PG_ONE_MINUS_EPS : u0);
            u1 = u1 * rd.sobol_resolution + rd.sample_bounds[1];
            u1 = u1 - py;
            u1 = u1 < 0.f ? 0.f : (u1 > PG_ONE_MINUS_EPS ? PG_ONE_MINUS_EPS : u1);
        }
        float pFilmX = (float)px + u0, pFilmY = (float)py + u1;
        float l0 = 0, l1 = 0;
        if (sc.tsBatched) { l0 = tsl0; l1 = tsl1; }
        else if (REAL || rd.lens_radius > 0) { l0 = halton_sample(sc, rd, index, 3); l1 = halton_sample(sc, rd, index, 4); }
        float weight = 1;
        if constexpr (REAL) {
            LensFrame *lf = lens_frame(st.L);
            float4 *diff = lf->differentials ? lf->differentials + 3 * (size_t)slot : nullptr;
            if constexpr (ANIM) {
                float c2w[16];
                rayTime = camera_time(rd, uTime);
                camera_matrix_at(rd, rayTime, c2w);
                weight = lens_camera_sample(*lensLds, rd, c2w, pFilmX, pFilmY, l0, l1, o, d, tMax, lensCalls, lensVignetted, diff);
            } else weight = lens_camera_sample(*lensLds, rd, rd.camera_to_world, pFilmX, pFilmY, l0, l1, o, d, tMax, lensCalls, lensVignetted, diff);
            lf->weights[slot] = weight;
            lensZero = weight == 0;
        } else if constexpr (ANIM) {
            float c2w[16];
            rayTime = camera_time(rd, uTime);
            camera_matrix_at(rd, rayTime, c2w);
            camera_ray(rd, c2w, pFilmX, pFilmY, l0, l1, o, d, tMax);
        } else camera_ray(rd, rd.camera_to_world, pFilmX, pFilmY, l0, l1, o, d, tMax);
        st.L[slot] = make_float4(0, 0, 0, pFilmX);
        st.beta[slot] = make_float4(1, 1, 1, pFilmY);
        st.meta[slot] = make_int4((int)(uint32_t)index, (int)(uint32_t)(index >> 32), __float_as_int(1.f), ((sc.tsBatched ? tsDim : 5) << 20) | (lensZero ? PG_META_DONE : PG_META_HASDIFF));
        if (lensZero) valid = false;  // the film takes the sample from its slot; no ray is queued
    } else if (slot < rp.capacity) {
        st.L[slot] = make_float4(0, 0, 0, 0);
        st.meta[slot] = make_int4(0, 0, 0, PG_META_DONE | 0x40000);  // 0x40000: slot holds no sample
    }
    if constexpr (REAL) lens_stats_add(lens_frame(st.L), lensCalls, lensVignetted, lensZero);
    int pos;
    block_push<1, false>(&q, &valid, &pos);
    if (valid) {
        q.o[pos] = make_float4(o.x, o.y, o.z, tMax);
        q.d[pos] = make_float4(d.x, d.y, d.z, __int_as_float(slot));
        if (float *qt = PG_QUEUE_TIMES(sc, q)) qt[pos] = rayTime;  // Ray::time (perspective.cpp:90 / :121), read by k_trace at moving instances
        if (st.qs[0].L) { st.qs[0].L[pos] = st.L[slot]; st.qs[0].beta[pos] = st.beta[slot]; st.qs[0].meta[pos] = st.meta[slot]; }  // just written by this thread
        if (st.qs[0].medium) st.qs[0].medium[pos] = rp.rd->camera_medium + 1;  // volpath: camera rays start in the camera's medium (camera.h:78)
    }
}
void launch_generate(const DScene &sc, const RenderParams &rp, PathState st, RayQueue q, hipStream_t s) {
    int nblk = (rp.capacity + PG_BLOCK - 1) / PG_BLOCK;
    const bool anim = rp.rd->camera_animated || sc.hasMotion;  // (moving instances need the samples' times too)
    if (rp.rd->camera_type == 3) {
        if (anim) hipLaunchKernelGGL((k_generate<true, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, rp, st, q);
        else hipLaunchKernelGGL((k_generate<false, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, rp, st, q);
    } else if (anim) hipLaunchKernelGGL((k_generate<true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, rp, st, q);
    else hipLaunchKernelGGL((k_generate<false>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, rp, st, q);
}

// Tile-serial samplers: sample `sampleIndex` of every tile's current pixel -- StartNextSample's reset, GetCameraSample's draws
// (film 2D, time 1D, lens 2D: always drawn, they advance the stream), the camera ray.  Slot = the tile's local index.
template <bool REAL>
__global__ __launch_bounds__(PG_BLOCK) void k_ts_generate(DScene sc, RenderParams rp, PathState st, RayQueue q, int sampleIndex) {
    const int local = blockIdx.x * PG_BLOCK + threadIdx.x;
    bool valid = local < rp.nTilesBatch && sc.ts[local].active;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    float tMax = PG_INF, rayTime = 0;
    int lensCalls = 0, lensVignetted = 0;
    bool lensZero = false;
    if (valid) {
        const PgRenderDesc &rd = rp.rd;
        TileSamplerState &t = sc.ts[local];
        t.sampleIndex = sampleIndex; t.cur1D = t.cur2D = 0;
        float u0, u1, l0, l1;
        ts_get2d(sc, rd.sampler, local, u0, u1);
        const float uTime = ts_get1d(sc, local);  // time
        ts_get2d(sc, rd.sampler, local, l0, l1);
        t.lens0 = l0; t.lens1 = l1; t.time = uTime;
        const float pFilmX = (float)t.px + u0, pFilmY = (float)t.py + u1;
        float c2w[16];
        rayTime = camera_time(rd, uTime);
        camera_matrix_at(rd, rayTime, c2w);
        if constexpr (REAL) {  // (a handful of lanes per launch: the lens block is read where it lies; a sample of weight 0 has drawn its camera sample and nothing more)
            LensFrame *lf = lens_frame(st.L);
            const float weight = lens_camera_sample(lf->lens, rd, c2w, pFilmX, pFilmY, l0, l1, o, d, tMax, lensCalls, lensVignetted,
                                                    lf->differentials ? lf->differentials + 3 * (size_t)local : nullptr);
            lf->weights[local] = weight;
            lensZero = weight == 0;
        } else camera_ray(rd, c2w, pFilmX, pFilmY, l0, l1, o, d, tMax);
        st.L[local] = make_float4(0, 0, 0, pFilmX);
        st.beta[local] = make_float4(1, 1, 1, pFilmY);
        st.meta[local] = make_int4(0, 0, __float_as_int(1.f), lensZero ? PG_META_DONE : PG_META_HASDIFF);
        if (lensZero) valid = false;
    }
    if constexpr (REAL) lens_stats_add(lens_frame(st.L), lensCalls, lensVignetted, lensZero);
    int pos;
    block_push<1, false>(&q, &valid, &pos);
    if (valid) {
        q.o[pos] = make_float4(o.x, o.y, o.z, tMax);
        q.d[pos] = make_float4(d.x, d.y, d.z, __int_as_float(local));
        if (float *qt = PG_QUEUE_TIMES(sc, q)) qt[pos] = rayTime;
        if (st.qs[0].L) { st.qs[0].L[pos] = st.L[local]; st.qs[0].beta[pos] = st.beta[local]; st.qs[0].meta[pos] = st.meta[local]; }
        if (st.qs[0].medium) st.qs[0].medium[pos] = rp.rd->camera_medium + 1;
    }
}
void launch_ts_generate(const DScene &sc, const RenderParams &rp, PathState st, RayQueue q, int sampleIndex, hipStream_t s) {
    if (rp.rd->camera_type == 3) hipLaunchKernelGGL(k_ts_generate<true>, dim3((rp.nTilesBatch + PG_BLOCK - 1) / PG_BLOCK), dim3(PG_BLOCK), 0, s, sc, rp, st, q, sampleIndex);
    else hipLaunchKernelGGL(k_ts_generate<false>, dim3((rp.nTilesBatch + PG_BLOCK - 1) / PG_BLOCK), dim3(PG_BLOCK), 0, s, sc, rp, st, q, sampleIndex);
}

// ===========================================================================
// Shading
// ===========================================================================

// MODE 0: triangles + matte/plastic/mirror/glass + area and delta lights (specialised BSDF).  MODE 1 (EXT): any material as
// its BxDF list, quadrics, object instances, infinite lights.  MODE 2: MODE 1 + textured materials, evaluated per hit.

// PG_SHADE_MIN_WAVES: waves per SIMD the BxDF-list variants (MODE 1) are compiled for.  Left alone the volumetric one takes 177
// VGPRs = 2 waves; capped at 168 (3 waves, 20 B of scratch) it is 31 % faster (150 -> 104 ms per frame on the 1 M-triangle volpath
// workload, profiles/r02p_*); 4 waves (128 VGPRs, 200 B of scratch) lose most of that again.  The surface-only variant is at 3 already.
#ifndef PG_SHADE_MIN_WAVES
#define PG_SHADE_MIN_WAVES 3
#endif
// the specialised surface kernel (MODE 0): 125 VGPRs = four waves per SIMD without the cap; the cap keeps later edits there
// the per-hit material evaluation (textured materials), path / volpath: the volpath kernel comes out at 259 registers -- three over the
// edge of 2 waves per SIMD -- and gains 36 % from being held to 248 (10 M-triangle divergent stand-in: 556 -> 357 ms per frame); the
// path kernel does not answer to 2 or 3 waves (253 / 258 / 268 ms; profiles/r03e_shade2_occupancy_anyhit_order.txt)
#ifndef PG_SHADE2_WAVES
#define PG_SHADE2_WAVES 1
#endif
#ifndef PG_SHADE2V_WAVES
#define PG_SHADE2V_WAVES 2
#endif
#ifndef PG_SHADE0_WAVES
#define PG_SHADE0_WAVES 4
#endif
// SSS: the scene has materials with a BSSRDF (subsurface / kdsubsurface): a vertex whose sampled direction is a transmission leaves
// through the BSSRDF branch of Li (path.cpp:152-174) -- the lane draws Sample_S's numbers, builds the probe segment of Sample_Sp and
// hands the path over to the probe / exit kernels below instead of pushing its next ray.  A separate instantiation: scenes without
// such materials run the code they ran before.
// GRID: the scene has a GridDensityMedium ("heterogeneous" medium, media/grid.cpp).  Its transmittance is estimated by ratio tracking
// with numbers from the PATH's sampler, drawn inside VisibilityTester::Tr / Scene::IntersectTr -- i.e. after a vertex's uLight /
// uScattering and before its next-direction sample -- so how many the two transmittance rays take decides which dimension (Halton,
// Sobol') or stream position (tile-serial samplers) the next direction is drawn at.  Such scenes shade every vertex in two launches:
// phase 1 = everything up to the MIS candidate (emission, medium sampling incl. delta tracking, the light sample), then the
// transmittance rays (k_through draws and counts), k_resolve_vol, and phase 2 = the vertex rebuilt, its next direction and the
// roulette.  Scenes without a grid medium run the single-pass kernels they ran before (phase 0).
struct GridShade { float4 *vertex; int phase; };  // vertex[slot] = (medium interaction point, kind: 0 none, 1 medium vertex, 2 surface vertex)
template <int MODE, bool VOL, bool SSS = false, bool GRID = false>
__global__ __launch_bounds__(PG_SHADE_BLOCK, MODE == 0 ? PG_SHADE0_WAVES : (((MODE == 1 || MODE == 3) && PG_SHADE_MIN_WAVES > 0) ? PG_SHADE_MIN_WAVES : (MODE == 2 ? (VOL ? PG_SHADE2V_WAVES : PG_SHADE2_WAVES) : 1))) void k_shade(DScene sc, RenderParams rp, PathState st, RayQueue qin, const float4 *__restrict__ hits,
                                                     RayQueue qnext, RayQueue qshadow, RayQueue qmis, unsigned long long *lightTriTests, VolState vs,
                                                     const float *__restrict__ hitT, QueueState qsIn, QueueState qsOut, SssState sss, GridShade gsh, PendJoin pj) {
    // MODE 3: MODE 1 over the lists k_material left for the hits on materials with textured parameters (rp.matPre)
    constexpr bool EXT = MODE >= 1, TEX = MODE == 2, PRE = MODE == 3;
    static_assert(!PRE || (!SSS && !GRID), "materials evaluated ahead: the plain path / volpath kernels");
    static_assert(!GRID || VOL, "grid media: volpath");
    const bool phaseA = GRID && gsh.phase == 1, phaseB = GRID && gsh.phase == 2;
    int vertexKind = 0;  // GRID: what phase 1 found at this entry (phase 2 reads it back)
    static_assert(!SSS || EXT, "materials with a BSSRDF are BxDF-list materials");
    bool pushJob = false;  // SSS: this lane's path goes on through the BSSRDF (its probe ray waits in s_ray[0])
    // path state and pending terms in queue order (see PathState); volpath: unless the scene has BSSRDF materials or a grid medium, whose
    // kernels (the probe chains, the two shading phases) find a path's state by its slot
    constexpr bool QSTATE = !VOL || (!SSS && !GRID);
    // PathIntegrator without BSSRDF materials: a vertex's direct lighting travels to the path's next vertex as QueueState::pend (qsOut.pend != nullptr) and
    // the previous vertex's is added here (qsIn.pend != nullptr); the launch lists the vertices that need k_resolve's arithmetic (PendJoin)
    constexpr bool PENDQ = !VOL && !SSS;
    int i;
    if (rp.retryCount > 0) {  // second pass over the entries that waited for a light-distribution voxel (the list holds their POSITIONS in the shading order)
        const int j = blockIdx.x * PG_SHADE_BLOCK + threadIdx.x;
        i = j < rp.retryCount ? rp.retryList[j] : -1;
    } else i = queue_item<PG_SHADE_BLOCK>(qin);
    if (rp.order && i >= 0) i = rp.order[i];  // k_shade_order: the entries of a window grouped by material class
    bool deferred = false;  // sparse light tables: this vertex met a voxel without a distribution; nothing is committed
    unsigned long long tsState0 = 0;  // tile-serial samplers: the tile's stream position and dimension counters on entry
    int tsCur1D0 = 0, tsCur2D0 = 0;
    const bool valid = i >= 0;
    // Output rays are staged in LDS ([queue][o|d][thread]) the moment they are known and copied to their queues after the
    // block-wide append at the end: holding three rays plus the pending direct-light terms in registers until then had
    // pushed the kernel to 130 VGPRs with scratch spills (3 waves/SIMD).
    __shared__ float4 s_ray[3][2][PG_SHADE_BLOCK];
    __shared__ float4 s_state[QSTATE ? 3 : (MODE == 2 ? 1 : 2)][PG_SHADE_BLOCK];  // QSTATE: (L, beta, meta) until the entry's place in the next queue is known; by slot (volpath): L and the film position wait here
    // EXT: of the seven Halton numbers a vertex computes ahead (halton_batch) the last four -- uScattering and the next direction's pair,
    // drawn late -- wait in LDS: they were what the register allocator put into scratch when the BxDF-list body grew; with them (and L,
    // see below) the kernel stays at 159 - 161 registers without scratch (profiles/r04j_bxdf_list_ab.txt).  (Not MODE 0: 2 KB more LDS
    // per block would cost it a resident block)
    __shared__ float s_pre[EXT ? 4 : 1][PG_SHADE_BLOCK];
    // for the integrator's statistics at the end of the kernel (nothing of them is held in a register across it): the bounce count the path arrived
    // with, | 0x4000: this vertex is one of volpath's volumeInteractions, | 0x8000: of its surfaceInteractions
    __shared__ unsigned short s_stat[PG_SHADE_BLOCK];
    const int tid = threadIdx.x;
    bool pushNext = false, pushShadow = false, pushMis = false;
    int slot = 0;
    int pdi = 0;  // index of this vertex's pending direct-light terms: the ray's queue position (QSTATE), else the slot
    unsigned int nLightTests = 0;
    int lightNum = -1;
    int nextBin = 0;  // direction octant of the continuation ray (groups the next queue, see block_push)
    // candidate of the BSDF-sampling half of MIS, tested against the light's triangle at the end
    bool misCand = false;
    V3 misRo = mk(0, 0, 0), misWi = mk(0, 0, 1), misP = mk(0, 0, 0);
    Spec misF = sp(0);
    float misPdf = 0, misLightArea = 1;
    int misLightPrim = 0;
    bool misInside = false;  // sphere light whose sphere contains the shaded point: Sphere::Pdf falls back to Shape::Pdf
    int misMedium = 0;       // VOL: medium of the BSDF-sampled ray
    int newMed = 0;          // VOL, queue-order state: the medium of the path's next ray
    float volWeight = 0;     // VOL: MIS weight of the light sample (-1: delta light)
    if (valid) {
        const float4 d4 = qin.d[i], h4 = hits[i];
        slot = __float_as_int(d4.w);
        pdi = QSTATE ? i : slot;
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const int prim = __float_as_int(h4.x);
        const PgRenderDesc &rd = rp.rd;
        float4 L4, B4;
        int4 meta;
        float4 P4 = make_float4(0, 0, 0, __int_as_float(-2));
        if constexpr (QSTATE) { L4 = qsIn.L[i]; B4 = qsIn.beta[i]; meta = qsIn.meta[i]; if constexpr (PENDQ) { if (qsIn.pend) P4 = qsIn.pend[i]; } }
        else { L4 = st.L[slot]; B4 = st.beta[slot]; meta = st.meta[slot]; }
        Spec L = sp3(L4.x, L4.y, L4.z), beta = sp3(B4.x, B4.y, B4.z);
        const uint64_t index = (uint64_t)(uint32_t)meta.x | ((uint64_t)(uint32_t)meta.y << 32);
        int dim = (int)((uint32_t)meta.w >> 20);
        // Sampler::Get1D / Get2D in the order the reference calls them: a GlobalSampler (halton, sobol) is indexed by
        // (sample index, dimension); the tile-serial samplers advance their tile's state (slot = tile, one path per tile)
        const bool tileSerial = rd.sampler >= PG_SAMPLER_RANDOM && !sc.tsBatched;
        const bool pixelArrays = sc.tsBatched != 0;  // a PixelSampler's arrays for this path's pixel: index = (pixel, sample), dim = the two dimension counters
        if (tileSerial) { tsState0 = sc.ts[slot].state; tsCur1D0 = sc.ts[slot].cur1D; tsCur2D0 = sc.ts[slot].cur2D; }  // restored if this vertex is deferred (sparse light tables)
        // Halton: the PG_NPRE dimensions a surface vertex usually draws (light choice, uLight, uScattering, the
        // next direction) are computed together before the first draw (halton_batch); preDim0 < 0: not computed
        constexpr int PG_NPRE = 7;
        float pre[PG_NPRE];
        int preDim0 = -1;
        auto sample_dim = [&](int d) -> float {
            const int k = d - preDim0;
            if (preDim0 >= 0 && k >= 0 && k < PG_NPRE) {
                if constexpr (EXT) return k == 0 ? pre[0] : (k == 1 ? pre[1] : (k == 2 ? pre[2] : s_pre[k - 3][tid]));
                return k == 0 ? pre[0] : (k == 1 ? pre[1] : (k == 2 ? pre[2] : (k == 3 ? pre[3] : (k == 4 ? pre[4] : (k == 5 ? pre[5] : pre[6])))));
            }
            return halton_sample(sc, rd, index, d);
        };
        auto draw1 = [&]() -> float { return tileSerial ? ts_get1d(sc, slot) : (pixelArrays ? tsb_get1d(sc, meta.x, meta.y, dim) : sample_dim(dim++)); };
        auto draw2 = [&](float &a, float &b) {
            if (tileSerial) ts_get2d(sc, rd.sampler, slot, a, b);
            else if (pixelArrays) tsb_get2d(sc, meta.x, meta.y, dim, a, b);
            else { a = sample_dim(dim); b = sample_dim(dim + 1); dim += 2; }
        };
        float etaScale = __int_as_float(meta.z);  // path.cpp:79
        int bounces = meta.w & 0xffff;
        s_stat[tid] = (unsigned short)bounces;
        const bool specularBounce = (meta.w & PG_META_SPECULAR) != 0;
        const bool found = prim >= 0;
        // VOL: the ray's medium (index + 1); volpath.cpp:76-78 samples it before anything else happens at the vertex
        int med = 0;
        bool volDead = false, inMedium = false;
        V3 mediumP = mk(0, 0, 0);
        if constexpr (VOL) {
            if constexpr (QSTATE) med = qsIn.medium[i]; else med = vs.medium[slot];
            newMed = med;
            if (phaseB) {  // the medium was sampled in phase 1: beta carries its weight, the vertex record says what came of it
                const float4 v4 = gsh.vertex[slot];
                vertexKind = __float_as_int(v4.w);
                inMedium = vertexKind == 1;
                mediumP = mk(v4.x, v4.y, v4.z);
            } else if (GRID && med && sc.mediaGrid[med - 1] >= 0) {  // GridDensityMedium::Sample, grid.cpp:61-86: delta tracking
                const PgMedium &mm = sc.media[med - 1];
                const PgDensityGrid &gd = sc.grids[sc.mediaGrid[med - 1]];
                const float4 o4 = qin.o[i];
                const float tMaxRay = found ? hitT[i] : o4.w;
                float tg = 0;
                inMedium = grid_sample(gd, sc.gridDensity + gd.density_offset, mk(o4.x, o4.y, o4.z), rayD, tMaxRay, draw1, tg);
                if (inMedium) {
                    mediumP = mk(o4.x, o4.y, o4.z) + rayD * tg;
                    beta = beta * (sp3(mm.sigma_s[0], mm.sigma_s[1], mm.sigma_s[2]) / gd.sigma_t);
                }
            } else if (med) {  // HomogeneousMedium::Sample, homogeneous.cpp:49-74
                const PgMedium &mm = sc.media[med - 1];
                const float4 o4 = qin.o[i];
                int channel;
                float dist;
                if (!GRID && rp.volPre) {  // drawn by k_shade_order (same dimensions, same arithmetic)
                    const float2 pv = rp.volPre[i];
                    channel = __float_as_int(pv.x); dist = pv.y;
                    dim += 2;
                } else {
                    const float uc = draw1();
                    homogeneous_sample_distance(mm, uc, draw1(), channel, dist);
                }
                const float dLen = sqrtf(lensq(rayD));
                const float tMaxRay = found ? hitT[i] : o4.w;  // ray.tMax after Scene::Intersect
                const float t = pmin(dist / dLen, tMaxRay);
                inMedium = t < tMaxRay;
                if (inMedium) mediumP = mk(o4.x, o4.y, o4.z) + rayD * t;
                const Spec sigT = sp3(mm.sigma_t[0], mm.sigma_t[1], mm.sigma_t[2]), sigS = sp3(mm.sigma_s[0], mm.sigma_s[1], mm.sigma_s[2]);
                const Spec Tr = sp_exp((sp3(-sigT.r, -sigT.g, -sigT.b) * pmin(t, PG_MAX_FLOAT)) * dLen);
                const Spec density = inMedium ? sigT * Tr : Tr;
                float pdf = 0;
                pdf += density.r; pdf += density.g; pdf += density.b;
                pdf *= 1 / (float)3;
                if (pdf == 0) pdf = 1;
                beta = beta * (inMedium ? (Tr * sigS) / pdf : Tr / pdf);
            }
            volDead = is_black(beta);  // volpath.cpp:78
        }
        // PENDQ: whether the previous vertex's shadow ray was occluded -- every lane loads (entry 0 where nothing waits), without a branch and beside the
        // triangle's loads: inside a branch the answer was a round trip of its own in front of them, +19 % on the kernel (profiles/shade_resolve_fused_ab.txt)
        int pendOcc = 1;
        if constexpr (PENDQ) { const int code = __float_as_int(P4.w); pendOcc = pj.occluded[code < 0 ? 0 : code]; }
        Tri tri;
        if (found) tri = load_tri(sc, prim);
        // the hit's material record, fetched as soon as its index is known (one round trip, overlapped with the interaction's
        // arithmetic) instead of field by field where each is used
        const PgMaterial mtl = sc.materials[found ? tri.material : 0];
        Isect is;
        float sphU = 0, sphV = 0;  // MODE 2: a quadric hit's (u, v) and geometric dpdu / dpdv, for textures
        V3 sphDpdu = mk(0, 0, 0), sphDpdv = mk(0, 0, 0);
        const bool onSphere = EXT && found && (tri.flags & PG_PRIM_SPHERE);
        // a hit reached through an object instance was computed on the instance-space ray (primitive.cpp:80-82)
        int inst = (EXT && found && sc.hitInst) ? sc.hitInst[i] : -1;
        // MODE 2 also shades the scenes whose hits can lie under TWO transforms (DScene::hasNest: a moving shape inside an object definition): the
        // outer instance's, then the inner TransformedPrimitive's on the way in; InterpolatedPrimToWorld of the inner, then of the outer, on the way out
        int inst2 = -1;
        if constexpr (TEX) nest_decode(sc, inst, inst2);
        // (the interaction is hit_isect's, in its stages: the quadric's here, where Le needs its normal; the triangle's and the way to world space below, at the
        // vertices still alive.  No InstXf is held across the vertex: each stage names the transforms again, and textures take the instance words -- held
        // in two structures, the MODE 2 volpath instantiations took four more registers, past 256)
        V3 shapeRayD = shape_ray_dir(inst_xf(sc, inst, i), inst_xf(sc, inst2, i, true), rayD);
        if (onSphere) {  // the hit record of a sphere carries tHit: Sphere::Intersect's interaction from the ray and the root
            const float4 o4 = qin.o[i];  // (the next three lines mirror shape_ray, on top of the direction above)
            V3 shapeRayO = mk(o4.x, o4.y, o4.z);
            if (inst >= 0) { float dt; instance_ray(inst_xf(sc, inst, i).w2i(), shapeRayO, rayD, shapeRayO, shapeRayD, dt); }
            if (TEX && inst2 >= 0) { float dt; instance_ray(inst_xf(sc, inst2, i, true).w2i(), shapeRayO, shapeRayD, shapeRayO, shapeRayD, dt); }
            const SphereHit sh = sphere_interaction(sc.spheres[__float_as_int(tri.p0.x)], shapeRayO, shapeRayD, h4.y);
            is = sphere_isect(sh);
            if (TEX) { sphU = sh.u; sphV = sh.v; sphDpdu = sh.dpdu; sphDpdv = sh.dpdv; }
        }
        // the previous vertex's direct lighting, now that its shadow ray is back: L += beta * Ld / lightPdf (path.cpp:122-126) BEFORE this vertex's Le, as
        // the reference adds them; what k_resolve counts is noted for the end of the kernel (0x4000: one of totalPaths, 0x8000: of zeroRadiancePaths)
        if constexpr (PENDQ) {
            const int code = __float_as_int(P4.w);
            const bool apply = code >= 0 && !pendOcc;
            const Spec add = sp3(P4.x, P4.y, P4.z);
            L = sp3(apply ? L.r + add.r : L.r, apply ? L.g + add.g : L.g, apply ? L.b + add.b : L.b);
            s_stat[tid] = (unsigned short)(bounces | (code == -2 ? 0 : (apply && !is_black(add) ? 0x4000 : 0xc000)));
        }
        // path.cpp:91-102 emitted light at the vertex (volpath.cpp:103-110: only when no medium interaction was sampled)
        if (phaseB || (VOL && (volDead || inMedium))) {
        } else if ((bounces == 0 || specularBounce) && found && tri.light >= 0) {
            L = L + beta * area_light_l(sc.lights[tri.light], onSphere ? is.n : hit_normal(sc, prim, tri, h4.y, h4.z, h4.w), -rayD);
        } else if ((bounces == 0 || specularBounce) && found) L = L + beta * sp(0);
        else if (EXT && (bounces == 0 || specularBounce) && !found && sc.hasInfinite) {  // path.cpp:96-100: every infinite light's Le(ray)
            for (int li = 0; li < sc.nLights; ++li)
                if (sc.lights[li].type == PG_LIGHT_INFINITE) L = L + beta * env_le(sc, sc.lights[li], rayD);
        }
        // QSTATE: L is final for this launch here (k_resolve adds the vertex's direct lighting), and the camera sample's film position in
        // L.w / beta.w is only carried along: both wait in LDS from here on instead of in five registers across the whole BSDF part --
        // with them the BxDF-list kernels stay under the 168 registers of three waves per SIMD without scratch
        if constexpr (!TEX) {
            s_state[0][tid] = make_float4(L.r, L.g, L.b, L4.w);
            reinterpret_cast<float *>(&s_state[1][tid])[3] = B4.w;
        }
        bool alive = found && bounces < rd.max_depth;  // path.cpp:104
        int newFlags = 0;
        bool handled = false;
        if constexpr (VOL) {
            if (volDead) alive = false;
            else if (inMedium) alive = bounces < rd.max_depth;  // volpath.cpp:83
            // ++volumeInteractions / ++surfaceInteractions (volpath.cpp:87, :99): noted in LDS, counted at the end of the kernel
            if (!phaseB && !volDead) s_stat[tid] = (unsigned short)(bounces | (inMedium ? (alive ? 0x4000 : 0) : 0x8000));
            if (phaseB) alive = vertexKind == 1 || vertexKind == 2;
            if (alive && inMedium) {
                vertexKind = 1;
                // ---- scattering at a point in the medium, volpath.cpp:80-96: MediumInteraction(p, -ray.d, ..., medium, phase)
                handled = true;
                {   // the dimensions of this vertex's draws side by side (as at a surface vertex, below)
                    const int dimU = __builtin_amdgcn_readfirstlane(dim);
                    const bool can = !tileSerial && !pixelArrays && rd.sampler == 0 && (index >> 32) == 0 && dim >= 2;
                    if (__ballot(!can || dim != dimU) == 0) { halton_batch<PG_NPRE>(sc, (uint32_t)index, dimU, pre); preDim0 = dimU; if constexpr (EXT) { s_pre[0][tid] = pre[3]; s_pre[1][tid] = pre[4]; s_pre[2][tid] = pre[5]; s_pre[3][tid] = pre[6]; } }
                }
                const float g = sc.media[med - 1].g;
                const V3 zero = mk(0, 0, 0), wo = -rayD;
                const float *tab = (sc.nLights > 0 && !phaseB) ? light_distribution(sc, mediumP) : nullptr;
                if (sc.nLights > 0 && !phaseB && !tab) deferred = true;
                // (the statements below mirror estimate_direct_setup<true>(sc, HgPhase{g}, mediumP, 0, 0, wo, ...) of pg_estimate.h, which k_sss_exit and k_direct
                // call: called here, the VOL instantiations lose registers they do not have -- MODE 2 with a grid medium a wave per SIMD; CHANGELOG.md)
                if (tab) {  // UniformSampleOneLight(mi, ..., handleMedia = true), integrator.cpp:85-106
                    float lightSelPdf;
                    lightNum = sample_discrete(tab, sc.nLights, draw1(), lightSelPdf);
                    if (lightSelPdf != 0) {
                        float uL0, uL1, uS0, uS1;  // uLight, uScattering (integrator.cpp:101-102)
                        draw2(uL0, uL1);
                        draw2(uS0, uS1);
                        const PgLight &light = sc.lights[lightNum];
                        V3 wi = zero;
                        float lightPdf = 0;
                        float4 pdLight = make_float4(0, 0, 0, 0);
                        LightSample ls;
                        Spec Li = light_sample_li<true>(sc, light, mediumP, zero, zero, uL0, uL1, wi, lightPdf, ls);
                        if (lightPdf > 0 && !is_black(Li)) {
                            const float ph = phase_hg(dot(wo, wi), g);  // integrator.cpp:135-141
                            if (ph != 0) {
                                shadow_ray_to(mediumP, zero, zero, ls, pdi, s_ray[1][0][tid], s_ray[1][1][tid]);  // (transmittance rays find their terms by pdi)
                                pushShadow = true;
                                const bool isDelta = PG_LIGHT_IS_DELTA(light.type);
                                volWeight = vol_light_weight_of(isDelta, lightPdf, ph);
                                pdLight = pending_light_encode(sp(ph), 0);
                                vs.pdLi[pdi] = vol_light_encode(Li, lightPdf);
                                vs.p1[0][pdi] = make_float4(ls.p.x, ls.p.y, ls.p.z, volWeight); vs.p1[1][pdi] = make_float4(ls.pError.x, ls.pError.y, ls.pError.z, 0);
                                vs.p1[2][pdi] = make_float4(ls.n.x, ls.n.y, ls.n.z, 0);
                                vs.trAcc[0][pdi] = through_acc_start(med);  // MediumInteraction::GetMedium(): the medium itself
                            }
                        }
                        if (light.type == PG_LIGHT_AREA || light.type == PG_LIGHT_INFINITE) {  // integrator.cpp:164-212 with the phase function
                            V3 wi2;
                            const float ph2 = hg_sample_p(g, wo, wi2, uS0, uS1);
                            if (ph2 != 0 && ph2 > 0) {
                                misCand = true;
                                misRo = mediumP; misWi = wi2; misF = sp(ph2); misPdf = ph2; misP = mediumP; misMedium = med;
                                misLightPrim = light.type == PG_LIGHT_INFINITE ? -1 - lightNum : light.prim; misLightArea = light.area;
                                if (light.type == PG_LIGHT_AREA) {
                                    const float4 la = sc.tris[PG_TRI_STRIDE * light.prim];
                                    if (__float_as_uint(la.w) & PG_PRIM_SPHERE)
                                        misInside = sc.spheres[__float_as_int(la.x)].shape != PG_SHAPE_SPHERE ||
                                                    sphere_ref_inside(sc.spheres[__float_as_int(la.x)], mediumP, zero, zero);
                                }
                            }
                        }
                        pdLight.w = lightSelPdf;
                        st.pdLight[pdi] = pdLight;
                        st.pdBeta[pdi] = pending_beta_encode(beta, 0.f);
                    }
                }
                if (!phaseA) {
                // mi.phase->Sample_p for the next direction, volpath.cpp:92-95
                V3 wi;
                float u0, u1;
                draw2(u0, u1);
                hg_sample_p(g, wo, wi, u0, u1);
                s_ray[0][0][tid] = make_float4(mediumP.x, mediumP.y, mediumP.z, PG_INF);
                s_ray[0][1][tid] = make_float4(wi.x, wi.y, wi.z, __int_as_float(slot));
                nextBin = dir_octant(wi);
                pushNext = true;  // the path stays in `med`
                Spec rrBeta = beta * etaScale;  // volpath.cpp:178-184
                if (max_component(rrBeta) < rd.rr_threshold && bounces > 3) {
                    float qq = pmax(.05f, 1 - max_component(rrBeta));
                    if (draw1() < qq) pushNext = false;
                    else beta = beta / (1 - qq);
                }
                bounces += 1;
                }
            }
        }
        if (alive && !handled) {
            if (!onSphere) is = make_isect(sc, prim, tri, h4.y, h4.z, h4.w, shapeRayD);
            isect_to_world(inst_xf(sc, inst, i), inst_xf(sc, inst2, i, true), is);
            const PgMaterial &m = mtl;
            int mIn = 0, mOut = 0;  // VOL: isect.mediumInterface
            if constexpr (VOL) prim_interface(sc, prim, med, mIn, mOut);
            if (m.type == PG_MAT_NONE) {  // path.cpp:107-113: skip over medium boundaries
              if (!phaseB) {  // (no draws at such a vertex: phase 1 finishes it)
                V3 nextO;
                spawn_ray(is, rayD, nextO);
                s_ray[0][0][tid] = make_float4(nextO.x, nextO.y, nextO.z, PG_INF);
                s_ray[0][1][tid] = make_float4(rayD.x, rayD.y, rayD.z, __int_as_float(slot));
                pushNext = true;
                newFlags = meta.w & PG_META_SPECULAR;  // `continue` leaves specularBounce as it was
                if constexpr (VOL) { newMed = dot(rayD, is.n) > 0 ? mOut : mIn; if constexpr (!QSTATE) vs.medium[slot] = newMed; }  // Interaction::GetMedium(w), interaction.h:86-88
              }
            } else {
                vertexKind = 2;
                // MatteMaterial::ComputeScatteringFunctions (matte.cpp:45-62), BSDF ctor (reflection.h:167-172)
                // BSDF: the EXT kernel evaluates the material's BxDF list (any material); the plain kernel has the list
                // shapes of matte / plastic / mirror / glass baked in (same arithmetic, fewer registers)
                {
                    // every lane here draws at least the next direction; the batch needs one dimension for the whole wave
                    const int dimU = __builtin_amdgcn_readfirstlane(dim);
                    const bool can = !tileSerial && !pixelArrays && rd.sampler == 0 && (index >> 32) == 0 && dim >= 2;
                    if (__ballot(!can || dim != dimU) == 0) { halton_batch<PG_NPRE>(sc, (uint32_t)index, dimU, pre); preDim0 = dimU; if constexpr (EXT) { s_pre[0][tid] = pre[3]; s_pre[1][tid] = pre[4]; s_pre[2][tid] = pre[5]; s_pre[3][tid] = pre[6]; } }
                }
                Bsdf bsdf;
                LobeBsdfT<typename std::conditional<PRE, PkLobe, PgBxDF>::type> lb;
                int sssIdx = -1;  // SSS: index of the hit's BSSRDF, or none
                PgBxDF lobeStore[TEX ? PG_MAX_BXDFS : 1];  // MODE 2: this hit's BxDF list (ComputeScatteringFunctions with textures)
                if constexpr (EXT) {
                    TexHit th;
                    if constexpr (TEX) {
                        tex_hit_setup(sc, rd, qin, i, slot, prim, tri, h4, rayD, inst, inst2, onSphere, sphU, sphV, sphDpdu, sphDpdv, is, meta, L4.w, B4.w, tileSerial,
                                      pixelArrays, index, th, st.L);
                        material_bump(sc, tri.material, th, is);
                    }
                    const bool preEvaluated = PRE && m.type == PG_MAT_TEXTURED;
                    float4 head0 = make_float4(0, 0, 0, 0), head1 = head0;
                    const int plane = qin.regionCap * PG_REGIONS;  // PRE: k_material's records lie by POSITION in the shading order, one plane per record (MatPre)
                    if (preEvaluated) {  // the shading frame after Material::Bump, as k_material left it
                        const int p = shade_position(rp, qin);
                        head0 = rp.matPre.head[p]; head1 = rp.matPre.head[(size_t)plane + p];
                        is.ns = mk(head0.x, head0.y, head0.z);
                        is.sdpdu = mk(head1.x, head1.y, head1.z);
                    }
                    lb.ns = is.ns; lb.ng = is.n;
                    lb.ss = normalize(is.sdpdu);
                    lb.ts = cross(lb.ns, lb.ss);
                    if constexpr (PRE) {
                        if (preEvaluated)  // k_material's list: head1.w = the number of BxDFs, bit 8: a mix (scale records)
                            lbsdf_bind(lb, reinterpret_cast<const PkLobe *>(rp.matPre.lobes) + shade_position(rp, qin), __float_as_int(head1.w) & 0xff, head0.w, ((__float_as_int(head1.w) & 0x100) ? 2 : 1) * plane);
                        else {  // a material with constant parameters: its list in the same records, packed once at pg_scene_create
                            const int2 pk = sc.matPk[tri.material];
                            lbsdf_bind(lb, reinterpret_cast<const PkLobe *>(sc.bxdfsPk) + pk.x, m.n_bxdfs, m.bsdf_eta, pk.y);
                        }
                    } else if constexpr (TEX) {
                        int nl = 0;
                        float etaL = 1;
                        MatEval<2>::run(*sc.self, tri.material, th, LobeOutRaw{lobeStore}, nl, etaL, PG_MAX_BXDFS);
                        lbsdf_bind(lb, lobeStore, nl, etaL);
                    } else lbsdf_bind(lb, sc.bxdfs + m.first_bxdf, m.n_bxdfs, m.bsdf_eta);
                    if constexpr (SSS) {  // si->bssrdf = TabulatedBSSRDF(...): subsurface.cpp:87-90, kdsubsurface.cpp:88-93
                        sssIdx = sc.materialBssrdf[tri.material];
                        if (sssIdx >= 0) {
                            const PgBSSRDF &bd = sc.bssrdfs[sssIdx];
                            float sigT[3] = {bd.sigma_t[0], bd.sigma_t[1], bd.sigma_t[2]}, rho[3] = {bd.rho[0], bd.rho[1], bd.rho[2]};
                            if (bd.textured) {
                                if (lb.n == 0) sssIdx = -1;  // ComputeScatteringFunctions returned before it set the BSSRDF (R and T both black)
                                else if constexpr (TEX) {
                                    const Spec ta = sp_clamp0(TexEval<PG_TEX_DEPTH>::s(*sc.self, bd.a, th)), tb = sp_clamp0(TexEval<PG_TEX_DEPTH>::s(*sc.self, bd.b, th));
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
                            if (sssIdx >= 0) {
                                sss.coef[0][slot] = make_float4(sigT[0], sigT[1], sigT[2], 0);
                                sss.coef[1][slot] = make_float4(rho[0], rho[1], rho[2], 0);
                            }
                        }
                    }
                } else {
                    bsdf.ns = is.ns; bsdf.ng = is.n;
                    bsdf.ss = normalize(is.sdpdu);
                    bsdf.ts = cross(bsdf.ns, bsdf.ss);
                    bsdf.R = sp3(m.kd[0] < 0 ? 0 : m.kd[0], m.kd[1] < 0 ? 0 : m.kd[1], m.kd[2] < 0 ? 0 : m.kd[2]);
                    bsdf.hasDiff = !is_black(bsdf.R);
                    bsdf.orenNayar = false; bsdf.onA = 1; bsdf.onB = 0;
                    if (m.type == PG_MAT_MATTE) {  // matte.cpp:55-61; OrenNayar ctor, reflection.h:425-431
                        const float sig = clampf(m.sigma, 0, 90);
                        if (sig != 0) {
                            const float sigma = (PG_PI / 180) * sig, sigma2 = sigma * sigma;
                            bsdf.orenNayar = true;
                            bsdf.onA = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
                            bsdf.onB = 0.45f * sigma2 / (sigma2 + 0.09f);
                        }
                    }
                    // PlasticMaterial (plastic.cpp:57-69): m.roughness already holds the distribution's alpha (host: RoughnessToAlpha)
                    bsdf.Ks = sp3(m.ks[0] < 0 ? 0 : m.ks[0], m.ks[1] < 0 ? 0 : m.ks[1], m.ks[2] < 0 ? 0 : m.ks[2]);
                    bsdf.hasSpec = m.type == PG_MAT_PLASTIC && !is_black(bsdf.Ks);
                    bsdf.alpha = m.roughness;
                    bsdf.nBxDFs = (bsdf.hasDiff ? 1 : 0) + (bsdf.hasSpec ? 1 : 0);
                    bsdf.specular = 0; bsdf.eta = 1;
                    bsdf.Kr = sp3(m.kr[0] < 0 ? 0 : m.kr[0], m.kr[1] < 0 ? 0 : m.kr[1], m.kr[2] < 0 ? 0 : m.kr[2]);
                    bsdf.Kt = sp3(m.kt[0] < 0 ? 0 : m.kt[0], m.kt[1] < 0 ? 0 : m.kt[1], m.kt[2] < 0 ? 0 : m.kt[2]);
                    if (m.type == PG_MAT_MIRROR || m.type == PG_MAT_GLASS) {  // mirror.cpp:44-56, glass.cpp:45-65 (smooth)
                        bsdf.hasDiff = false;
                        if (m.type == PG_MAT_MIRROR) bsdf.specular = is_black(bsdf.Kr) ? 0 : 1;
                        else { bsdf.eta = m.eta; bsdf.specular = (is_black(bsdf.Kr) && is_black(bsdf.Kt)) ? 0 : 2; }
                        bsdf.nBxDFs = bsdf.specular ? 1 : 0;
                    }
                }
                const V3 shNs = EXT ? lb.ns : bsdf.ns;
                const int nonSpecular = PG_BSDF_ALL & ~PG_BSDF_SPECULAR;
                bool hasNonSpecular;
                if constexpr (EXT) hasNonSpecular = lbsdf_num_components(lb, nonSpecular) > 0;
                else hasNonSpecular = bsdf.nBxDFs > 0 && !bsdf.specular;
                // ---- direct lighting: UniformSampleOneLight (integrator.cpp:85-106) + EstimateDirect set-up
                // (the statements mirror direct_light_half / direct_scatter_half of pg_estimate.h with this kernel's register relief between and inside them;
                // called here, the plain instantiations keep their registers but the VOL ones do not -- CHANGELOG.md "one EstimateDirect set-up")
                if (!VOL && hasNonSpecular && sc.nLights == 0) lightNum = -2;  // (still one of path.cpp:121's totalPaths -- and a zero-radiance one: k_resolve counts pdInfo.z != -1)
                const bool wantLight = (VOL || hasNonSpecular) && sc.nLights > 0 && !phaseB;  // path.cpp:119: only with non-specular lobes (volpath.cpp:124-127: always)
                const float *tab = wantLight ? light_distribution(sc, is.p) : nullptr;
                if (wantLight && !tab) deferred = true;
                if (tab) {
                    float lightSelPdf;
                    lightNum = sample_discrete(tab, sc.nLights, draw1(), lightSelPdf);
                    if (lightSelPdf != 0) {
                        float uL0, uL1, uS0, uS1;  // uLight, uScattering (integrator.cpp:101-102)
                        draw2(uL0, uL1);
                        draw2(uS0, uS1);
                        const LightHot lh = load_light_hot(sc, lightNum);
                        const PgLight &light = sc.lights[lightNum];
                        V3 wi = mk(0, 0, 0);
                        float lightPdf = 0, scatteringPdf = 0;
                        float4 pdLight = make_float4(0, 0, 0, 0);
                        LightSample ls;
                        Spec Li = light_sample_li_hot<EXT>(sc, lh, light, is.p, is.pError, is.n, uL0, uL1, wi, lightPdf, ls);
                        if (lightPdf > 0 && !is_black(Li)) {
                            Spec f;
                            if constexpr (EXT) { f = lbsdf_f(lb, is.wo, wi, nonSpecular) * absdot(wi, shNs); scatteringPdf = lbsdf_pdf(lb, is.wo, wi, nonSpecular); }
                            else { f = bsdf_f(bsdf, is.wo, wi) * absdot(wi, shNs); scatteringPdf = bsdf_pdf(bsdf, is.wo, wi); }
                            if (!is_black(f)) {
                                [[maybe_unused]] const V3 shD = shadow_ray_to(is.p, is.pError, is.n, ls, VOL ? pdi : slot, s_ray[1][0][tid], s_ray[1][1][tid]);
                                pushShadow = true;
                                // delta lights take no MIS weight (integrator.cpp:155-160)
                                const bool isDelta = PG_LIGHT_IS_DELTA(lh.type);
                                if constexpr (VOL) {  // Li still is to be multiplied by VisibilityTester::Tr (integrator.cpp:146-150): keep the factors apart
                                    volWeight = vol_light_weight_of(isDelta, lightPdf, scatteringPdf);
                                    pdLight = pending_light_encode(f, 0);
                                    vs.pdLi[pdi] = vol_light_encode(Li, lightPdf);
                                    vs.p1[0][pdi] = make_float4(ls.p.x, ls.p.y, ls.p.z, volWeight); vs.p1[1][pdi] = make_float4(ls.pError.x, ls.pError.y, ls.pError.z, 0);
                                    vs.p1[2][pdi] = make_float4(ls.n.x, ls.n.y, ls.n.z, 0);
                                    vs.trAcc[0][pdi] = through_acc_start(dot(shD, is.n) > 0 ? mOut : mIn);
                                } else {
                                    Spec c = isDelta ? (f * Li) / lightPdf : ((f * Li) * power_heuristic(1, lightPdf, 1, scatteringPdf)) / lightPdf;
                                    pdLight = pending_light_encode(c, 0);
                                }
                            }
                        }
                        // pending terms of this vertex, consumed by k_resolve (pdMis and the MIS weight follow below) -- stored HERE: held until after the
                        // BSDF sample below they were five registers at the kernel's peak (tools/reg_pressure.py: lbsdf_sample_f's microfacet terms)
                        // (PENDQ with a pend to write: they wait in the MIS ray's LDS slot instead -- free until the end of the kernel, where most vertices
                        // turn them into one float4 for the next queue entry and the listed ones store them for k_resolve_list)
                        pdLight.w = lightSelPdf;
                        if (PENDQ && qsOut.pend) { s_ray[2][0][tid] = pdLight; s_ray[2][1][tid] = pending_beta_encode(beta, 0.f); }
                        else { st.pdLight[pdi] = pdLight; st.pdBeta[pdi] = pending_beta_encode(beta, 0.f); }
                        // (beta waits in LDS, where it goes at the end anyway, while the BSDF is sampled: three more registers off the same peak)
                        if constexpr (!TEX) { float *sb = reinterpret_cast<float *>(&s_state[1][tid]); sb[0] = beta.r; sb[1] = beta.g; sb[2] = beta.b; }
                        // BSDF sampling half of MIS (integrator.cpp:164-212): sample now, while the BSDF is live; the
                        // light.Pdf_Li triangle test runs at the end of the kernel, when little else is (register pressure)
                        V3 wi2 = wi;
                        float sPdf2 = 0;
                        Spec f2 = sp(0);
                        if (lh.type == PG_LIGHT_AREA || (EXT && lh.type == PG_LIGHT_INFINITE)) {  // integrator.cpp:164: if (!IsDeltaLight(light.flags))
                            if constexpr (EXT) { int st2; f2 = lbsdf_sample_f(lb, is.wo, wi2, uS0, uS1, sPdf2, nonSpecular, st2); }
                            else f2 = bsdf_sample_f(bsdf, is.wo, wi2, uS0, uS1, sPdf2);
                            f2 = f2 * absdot(wi2, shNs);
                        }
                        if (!is_black(f2) && sPdf2 > 0) {
                            misCand = true;
                            spawn_ray(is, wi2, misRo);
                            misWi = wi2; misF = f2; misPdf = sPdf2; misP = is.p;
                            if constexpr (VOL) misMedium = dot(wi2, is.n) > 0 ? mOut : mIn;
                            // (the next lines mirror mis_light_of, with the EXT guards that keep the infinite light and the sphere out of MODE 0)
                            misLightPrim = (EXT && lh.type == PG_LIGHT_INFINITE) ? -1 - lightNum : lh.prim; misLightArea = lh.area;
                            if (EXT && lh.type == PG_LIGHT_AREA && (lh.tri.flags & PG_PRIM_SPHERE)) {  // only the sphere overrides Shape::Pdf (with its cone pdf, from outside)
                                const PgSphere &lsph = sc.spheres[__float_as_int(lh.tri.p0.x)];
                                misInside = lsph.shape != PG_SHAPE_SPHERE || sphere_ref_inside(lsph, is.p, is.pError, is.n);
                            }
                        }
                        if constexpr (!TEX) { const volatile float *sb = reinterpret_cast<const volatile float *>(&s_state[1][tid]); beta = sp3(sb[0], sb[1], sb[2]); }
                    }
                }
                // ---- sample the BSDF for the next direction (path.cpp:130-150)
                if (!phaseA) {
                // (the ray's direction once more from its queue entry: kept from the top of the kernel it was three registers at the peak above)
                const float4 dNow = qin.d[i];
                V3 wo = -mk(dNow.x, dNow.y, dNow.z), wi;
                float pdf;
                float u0, u1;
                draw2(u0, u1);
                int sampledType = 0;
                Spec f;
                float bsdfEta;
                if constexpr (EXT) { f = lbsdf_sample_f(lb, wo, wi, u0, u1, pdf, PG_BSDF_ALL, sampledType); bsdfEta = lb.eta; }
                else { f = bsdf.specular ? bsdf_sample_specular(bsdf, wo, wi, u0, pdf, sampledType) : bsdf_sample_f(bsdf, wo, wi, u0, u1, pdf); bsdfEta = bsdf.eta; }
                if (!(is_black(f) || pdf == 0.f)) {
                    beta = beta * ((f * absdot(wi, shNs)) / pdf);
                    if (sampledType & PG_BSDF_SPECULAR) newFlags |= PG_META_SPECULAR;  // path.cpp:142
                    if ((sampledType & PG_BSDF_SPECULAR) && (sampledType & PG_BSDF_TRANSMISSION))  // path.cpp:143-149
                        etaScale *= (dot(wo, is.n) > 0) ? (bsdfEta * bsdfEta) : 1 / (bsdfEta * bsdfEta);
                    V3 nextO;
                    spawn_ray(is, wi, nextO);
                    s_ray[0][0][tid] = make_float4(nextO.x, nextO.y, nextO.z, PG_INF);
                    s_ray[0][1][tid] = make_float4(wi.x, wi.y, wi.z, __int_as_float(slot));
                    nextBin = dir_octant(wi);
                    pushNext = true;
                    if constexpr (VOL) { newMed = dot(wi, is.n) > 0 ? mOut : mIn; if constexpr (!QSTATE) { if (!deferred) vs.medium[slot] = newMed; } }
                    bool throughBssrdf = false;
                    if constexpr (SSS) {
                        if (sssIdx >= 0 && (sampledType & PG_BSDF_TRANSMISSION)) {
                            // path.cpp:152-156: bssrdf->Sample_S(scene, sampler.Get1D(), sampler.Get2D(), ...) -- the reference build
                            // evaluates the arguments right to left: the 2D sample is drawn first.  Then the first half of
                            // SeparableBSSRDF::Sample_Sp (bssrdf.cpp:257-292): the probe segment; the path ends here when there is none
                            throughBssrdf = true;
                            pushNext = false;
                            float u2x, u2y;
                            draw2(u2x, u2y);
                            float u1 = draw1();
                            DBssrdf b = bssrdf_bind(sc.bssrdfs[sssIdx], sc.bssrdfTables);
                            const float4 cs = sss.coef[0][slot], cr = sss.coef[1][slot];
                            b.sigma_t[0] = cs.x; b.sigma_t[1] = cs.y; b.sigma_t[2] = cs.z; b.rho[0] = cr.x; b.rho[1] = cr.y; b.rho[2] = cr.z;
                            V3 baseP, pTarget;
                            if (bssrdf_probe_segment(b, lb.ss, lb.ts, lb.ns, is.p, u1, u2x, u2y, baseP, pTarget)) {
                                const V3 pd = pTarget - baseP;  // base.SpawnRayTo(pTarget) of an Interaction without normal or error: from baseP itself
                                if (!(pd.x == 0 && pd.y == 0 && pd.z == 0)) {  // bssrdf.cpp:306: a zero direction ends the chain before it starts
                                    s_ray[0][0][tid] = make_float4(baseP.x, baseP.y, baseP.z, 1 - PG_SHADOW_EPS);
                                    s_ray[0][1][tid] = make_float4(pd.x, pd.y, pd.z, __int_as_float(slot));
                                    pushJob = true;
                                    sss.po[slot] = make_float4(is.p.x, is.p.y, is.p.z, u1);
                                    sss.frame[0][slot] = make_float4(lb.ns.x, lb.ns.y, lb.ns.z, b.eta);
                                    sss.frame[1][slot] = make_float4(lb.ss.x, lb.ss.y, lb.ss.z, __int_as_float(sssIdx));
                                    sss.frame[2][slot] = make_float4(lb.ts.x, lb.ts.y, lb.ts.z, __int_as_float(sc.bssrdfs[sssIdx].match_material));
                                    sss.target[slot] = make_float4(pTarget.x, pTarget.y, pTarget.z, 0);
                                    sss.count[slot] = make_int2(0, 0);
                                    if constexpr (VOL) sss.medium[slot] = make_int2(0, 0);  // Sample_Sp's `base` has no MediumInterface
                                }
                            }
                        }
                    }
                    // Russian roulette, path.cpp:176-184 (a path inside the BSSRDF branch: at its exit vertex, k_sss_exit).  (Here and at the medium vertex the
                    // statements mirror russian_roulette of pg_sampler.h: called, k_shade<1, VOL, ., GRID> spills one more register)
                    Spec rrBeta = beta * etaScale;
                    if (!throughBssrdf && max_component(rrBeta) < rd.rr_threshold && bounces > 3) {
                        float qq = pmax(.05f, 1 - max_component(rrBeta));
                        if (draw1() < qq) pushNext = false;
                        else beta = beta / (1 - qq);
                    }
                }
                bounces += 1;
                }
            }
        }
        if (deferred) {
        } else if constexpr (QSTATE) {  // written after the append: to the ray's entry of the next queue, or (path over) L to its slot
            if constexpr (TEX) {
                s_state[0][tid] = make_float4(L.r, L.g, L.b, L4.w);
                s_state[1][tid] = make_float4(beta.r, beta.g, beta.b, B4.w);
            } else {  // (L and beta.w are there already, see above)
                float *sb = reinterpret_cast<float *>(&s_state[1][tid]);
                sb[0] = beta.r; sb[1] = beta.g; sb[2] = beta.b;
            }
            s_state[2][tid] = make_float4(__int_as_float(meta.x), __int_as_float(meta.y), etaScale, __int_as_float((dim << 20) | bounces | newFlags));
        } else {
            // (GRID: phase 1 leaves the incoming flags for phase 2's rebuild of the vertex -- a null-material surface, finished in
            // phase 1, sets its own --; phase 2 leaves L alone: k_resolve_vol has added this vertex's direct lighting to it)
            if (phaseA && vertexKind != 0) newFlags = meta.w & 0xf0000;
            if (!phaseB) { if constexpr (TEX) st.L[slot] = make_float4(L.r, L.g, L.b, L4.w); else st.L[slot] = s_state[0][tid]; }
            // (phase 2 has nothing to do for a vertex that phase 1 finished -- a surface without a material, the end of a path -- and must
            // leave its state alone: writing it back would clear the flags phase 1 set, e.g. "the last bounce was specular", which a
            // path keeps across a material-less surface, path.cpp:107-113)
            if (!(phaseB && vertexKind == 0)) {
                st.beta[slot] = make_float4(beta.r, beta.g, beta.b, TEX ? B4.w : reinterpret_cast<float *>(&s_state[1][tid])[3]);
                st.meta[slot] = make_int4(meta.x, meta.y, __float_as_int(etaScale), (dim << 20) | bounces | newFlags);
            }
            if (phaseA) gsh.vertex[slot] = make_float4(mediumP.x, mediumP.y, mediumP.z, __int_as_float(alive ? vertexKind : 0));
        }
    }
    if (deferred) {  // retried once the voxel's distribution exists: no ray, no state, no pending term leaves this launch
        pushNext = pushShadow = misCand = false;
        if (rp.rd->sampler >= PG_SAMPLER_RANDOM) { sc.ts[slot].state = tsState0; sc.ts[slot].cur1D = tsCur1D0; sc.ts[slot].cur2D = tsCur2D0; }  // nor a draw from the tile's stream
        rp.retryList[atomicAdd(&sc.voxelCounters[1], 1)] = shade_position(rp, qin);
    }
    if (misCand) {
        const float lightPdf2 = mis_light_pdf<EXT>(sc, misLightPrim, misLightArea, misInside, misP, misRo, misWi, nLightTests);
        if (lightPdf2 != 0) {
            if (PENDQ && qsOut.pend) {  // a listed vertex: the terms staged in this slot go to k_resolve_list's records before the ray takes it
                const PendingBeta pb = pending_beta(s_ray[2][1][tid]);
                st.pdLight[pdi] = s_ray[2][0][tid];
                st.pdBeta[pdi] = pending_beta_encode(pb.beta, pending_mis_weight(misPdf, lightPdf2));
            } else st.pdBeta[pdi].w = pending_mis_weight(misPdf, lightPdf2);
            s_ray[2][0][tid] = make_float4(misRo.x, misRo.y, misRo.z, PG_INF);
            s_ray[2][1][tid] = make_float4(misWi.x, misWi.y, misWi.z, __int_as_float(VOL ? pdi : slot));
            pushMis = true;
            st.pdMis[pdi] = pending_mis_encode(misF, misPdf);
            if constexpr (VOL) vs.trAcc[1][pdi] = through_acc_start(misMedium);
        }
    }
    // PENDQ: the vertices that need k_resolve's arithmetic (a MIS ray left, or the path ends here with something to add or count) append their positions to
    // the launch's list as to a fourth queue: by region, in the block's one exchange
    constexpr int NOUT = PENDQ ? 4 : 3;
    const bool listed = PENDQ && qsOut.pend && valid && !deferred && (pushMis || (!pushNext && lightNum != -1));
    const RayQueue outQ[4] = {qnext, qshadow, qmis, RayQueue{nullptr, nullptr, pj.listCounts, qin.regionCap}};
    const bool outPred[4] = {pushNext, pushShadow, pushMis, listed};
    int outPos[4];
    block_push<NOUT, true, PG_SHADE_BLOCK>(outQ, outPred, outPos, nextBin);
    const int posNext = outPos[0], posShadow = outPos[1], posMis = outPos[2];
    if (listed) pj.list[outPos[3]] = pdi;
    if (pushNext) { qnext.o[posNext] = s_ray[0][0][tid]; qnext.d[posNext] = s_ray[0][1][tid]; }
    if (pushShadow) { qshadow.o[posShadow] = s_ray[1][0][tid]; qshadow.d[posShadow] = s_ray[1][1][tid]; }
    if (pushMis) { qmis.o[posMis] = s_ray[2][0][tid]; qmis.d[posMis] = s_ray[2][1][tid]; }
    store_ray_times(sc, qin, i, outQ, outPred, outPos);
    if constexpr (QSTATE) {
        if (valid && !deferred) {
            if (pushNext) {
                const float4 m4 = s_state[2][tid];
                qsOut.L[posNext] = s_state[0][tid]; qsOut.beta[posNext] = s_state[1][tid];
                qsOut.meta[posNext] = make_int4(__float_as_int(m4.x), __float_as_int(m4.y), __float_as_int(m4.z), __float_as_int(m4.w));
                if constexpr (VOL) qsOut.medium[posNext] = newMed;
            } else st.L[slot] = s_state[0][tid];
            if (PENDQ && qsOut.pend) {
                if (pushNext) {
                    float4 p4 = make_float4(0, 0, 0, __int_as_float(pushMis || lightNum == -1 ? -2 : -1));
                    if (pushShadow && !pushMis) {  // resolve_entry's sums (direct_pend), up to the one bit the any-hit launch still owes
                        const Spec add = direct_pend(pending_light(s_ray[2][0][tid]), pending_beta(s_ray[2][1][tid]));
                        p4 = make_float4(add.r, add.g, add.b, __int_as_float(posShadow));
                    }
                    qsOut.pend[posNext] = p4;
                } else if (pushShadow && !pushMis) { st.pdLight[pdi] = s_ray[2][0][tid]; st.pdBeta[pdi] = s_ray[2][1][tid]; }
                if (listed) st.pdInfo[pdi] = pending_info_encode(posShadow, posMis, lightNum, pending_where(pushNext, posNext, slot));
            } else st.pdInfo[pdi] = pending_info_encode(posShadow, posMis, lightNum, pending_where(pushNext, posNext, slot));
        }
    } else if (valid && !deferred && !phaseB) st.pdInfo[slot] = pending_info_encode(posShadow, posMis, lightNum, VOL ? pending_where_weight(volWeight) : 0);
    if constexpr (SSS) {
        // the probe rays of the paths that go on through a BSSRDF, region by region like every other queue; such a path's L went to
        // its slot above (where k_resolve adds this vertex's direct lighting), beta and meta follow it there
        if (deferred) pushJob = false;
        int posJob;
        block_push<1, false, PG_SHADE_BLOCK>(&sss.qjob, &pushJob, &posJob);
        if (pushJob) {
            sss.qjob.o[posJob] = s_ray[0][0][tid]; sss.qjob.d[posJob] = s_ray[0][1][tid];
            if (sc.rayTimes) PG_QUEUE_TIMES(sc, sss.qjob)[posJob] = PG_QUEUE_TIMES(sc, qin)[i];  // the probe rays' time: po's = the ray's (bssrdf.cpp:290-296)
            if constexpr (QSTATE) {
                const float4 m4 = s_state[2][tid];
                st.beta[slot] = s_state[1][tid];
                st.meta[slot] = make_int4(__float_as_int(m4.x), __float_as_int(m4.y), __float_as_int(m4.z), __float_as_int(m4.w));
            }
        }
    }
    flush_light_tests(lightTriTests, nLightTests);
    {   // the integrator's statistics (PgCounters, ABI 28).  "Path length" of the paths that end at this vertex: ReportValue(pathLength, bounces), path.cpp:186,
        // with `bounces` of the reference's loop = the count the path arrived with (a scattering vertex has raised the stored one since).  A path that goes on
        // through a BSSRDF reports in k_sss_exit; a grid scene's vertex reports in the phase that finishes it
        bool ended = valid && !deferred && !pushNext && !pushJob;
        if constexpr (GRID) ended = ended && (phaseA ? vertexKind == 0 : vertexKind != 0);
        const int code = valid ? s_stat[tid] : 0;
        stats_path_end(lightTriTests, ended, code & 0x3fff);
        if constexpr (PENDQ) {  // what k_resolve counted for the previous vertex (a deferred vertex is shaded again by the retry launch)
            if (qsIn.pend) {
                stats_count(lightTriTests, PG_STAT_PATHS, !deferred && (code & 0x4000));
                stats_count(lightTriTests, PG_STAT_PATHS_ZERO, !deferred && (code & 0x8000));
            }
        }
        if constexpr (VOL) {  // (a deferred vertex is shaded again by the retry launch)
            stats_count(lightTriTests, PG_STAT_VOLUME, !deferred && (code & 0x4000));
            stats_count(lightTriTests, PG_STAT_SURFACE, !deferred && (code & 0x8000));
        }
    }
}
// Material::ComputeScatteringFunctions ahead of the shading launch, for the main-queue entries whose hit has a material with
// textured parameters: the interaction (hit_isect), what textures read of it (tex_hit_setup), Material::Bump and the
// material's BxDF list, written to rp.matPre at the entry's index; k_shade<3, .> takes them from there and is the BxDF-list kernel
// otherwise.  Why two launches: evaluated inside the shading kernel (k_shade<2, .>) the texture / material evaluators' registers and
// call frames come on top of a path vertex's whole state -- 251 VGPRs, two waves per SIMD, the list of up to 8 x 120 B in scratch --
// and the kernel waits on dependent fetches (material -> texture node -> MIP level -> texels) with little else resident to run.
// Here only the interaction is live across the evaluators, the list is written where it is read from, and the threads take the
// entries in the same material-class order (rp.order).  An entry the shading kernel will not shade as a surface vertex (the path
// is over, a null material, volpath: the ray scattered in its medium first) is skipped when that is known without drawing.
#ifndef PG_MATERIAL_WAVES
#define PG_MATERIAL_WAVES 3
#endif
template <bool VOL>
__global__ __launch_bounds__(PG_SHADE_BLOCK, PG_MATERIAL_WAVES) void k_material(DScene sc, RenderParams rp, PathState st, RayQueue qin, const float4 *__restrict__ hits,
                                                                               VolState vs, const float *__restrict__ hitT, QueueState qsIn) {
    const int p = queue_item<PG_SHADE_BLOCK>(qin);  // the thread's position in the shading order: where its list goes (MatPre)
    if (p < 0) return;
    const int i = rp.order ? rp.order[p] : p;
    const float4 h4 = hits[i];
    const int prim = __float_as_int(h4.x);
    if (prim < 0) return;
    const Tri tri = load_tri(sc, prim);
    if (sc.materials[tri.material].type != PG_MAT_TEXTURED) return;
    const float4 d4 = qin.d[i];
    const int slot = __float_as_int(d4.w);
    const V3 rayD = mk(d4.x, d4.y, d4.z);
    const PgRenderDesc &rd = rp.rd;
    const bool bySlot = VOL && qsIn.L == nullptr;  // volpath scenes with BSSRDF materials or grid media keep their path state by slot
    const int4 meta = bySlot ? st.meta[slot] : qsIn.meta[i];
    if ((meta.w & 0xffff) >= rd.max_depth) return;  // path.cpp:104
    if constexpr (VOL) {
        if (rp.volPre) {  // the medium sample k_shade_order drew: a ray that scatters before the surface never reaches it (volpath.cpp:76-96)
            const int med = bySlot ? vs.medium[slot] : qsIn.medium[i];
            if (med && !(sc.mediaGrid && sc.mediaGrid[med - 1] >= 0) && rp.volPre[i].y / sqrtf(lensq(rayD)) < hitT[i]) return;
        }
    }
    const bool tileSerial = rd.sampler >= PG_SAMPLER_RANDOM && !sc.tsBatched, pixelArrays = sc.tsBatched != 0;
    const uint64_t index = (uint64_t)(uint32_t)meta.x | ((uint64_t)(uint32_t)meta.y << 32);
    // (the scenes whose hits can lie under two transforms are shaded by k_shade<2>, without this launch: one level here)
    const InstXf outer = inst_xf(sc, sc.hitInst ? sc.hitInst[i] : -1, i), inner = inst_xf(sc, -1, i, true);
    QuadricUv quv;
    Isect is = hit_isect(sc, outer, inner, (tri.flags & PG_PRIM_SPHERE) ? qin.o[i] : make_float4(0, 0, 0, 0), rayD, h4, prim, tri, quv);
    float filmX = 0, filmY = 0;  // the camera sample's pFilm, for the camera ray's differentials
    if (meta.w & PG_META_HASDIFF) { filmX = bySlot ? st.L[slot].w : qsIn.L[i].w; filmY = bySlot ? st.beta[slot].w : qsIn.beta[i].w; }
    TexHit th;
    tex_hit_setup(sc, rd, qin, i, slot, prim, tri, h4, rayD, outer, inner, quv, is, meta, filmX, filmY, tileSerial, pixelArrays, index, th, st.L);
    material_bump<1>(sc, tri.material, th, is);
    int nl = 0;
    float etaL = 1;
    // the list in packed records (LobeBsdfT): stride = the records per entry; a mix's lobes take two each
    const bool mix = sc.textured[sc.materials[tri.material].textured_index].kind == PG_KIND_MIX;
    const int plane = qin.regionCap * PG_REGIONS;
    const LobeOutPacked out = {rp.matPre.lobes + (size_t)p * 3, mix ? 2 : 1, plane};
    MatEval<2, 1, LobeOutPacked>::run(*sc.self, tri.material, th, out, nl, etaL, mix ? rp.matPre.stride / 2 : rp.matPre.stride);
    rp.matPre.head[p] = make_float4(is.ns.x, is.ns.y, is.ns.z, etaL);
    rp.matPre.head[(size_t)plane + p] = make_float4(is.sdpdu.x, is.sdpdu.y, is.sdpdu.z, __int_as_float(nl | (mix ? 0x100 : 0)));
}
static void launch_material(const DScene &sc, const RenderParams &rp, PathState st, VolState vs, RayQueue qin, const float4 *hits, const float *hitT, QueueState qi,
                            bool vol, hipStream_t s) {
    const int nblk = PG_REGIONS * (qin.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    if (vol) hipLaunchKernelGGL(k_material<true>, dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, vs, hitT, qi);
    else hipLaunchKernelGGL(k_material<false>, dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, vs, hitT, qi);
}
// The order in which a shading launch takes the entries of its queue (RenderParams::order): block b sorts the entry indices of
// window b >> 3 of region b & 7 by the material class of the entry's hit -- counting sort, stable, so that the entries of a class stay
// in queue order and neighbouring lanes still read neighbouring entries.  Window and region are those of the consumer's
// blocks (queue_item): the shading blocks of a window run side by side on the region's XCD and find each other's lines in its L2.
// VOL (volpath, GlobalSamplers, no grid medium): the kernel also draws the medium sample of every entry whose ray is in a medium
// (HomogeneousMedium::Sample's two numbers at the path's current dimension; the shading kernel reads channel and distance from
// volPre instead of drawing them) and gives the entries that scatter inside the medium a class of their own.
template <bool VOL>
__global__ __launch_bounds__(1024) void k_shade_order(DScene sc, RayQueue q, const float4 *__restrict__ hits, int *__restrict__ order,
                                                      RenderDescHead rdHead, PathState st, VolState vs, const float *__restrict__ hitT, float2 *__restrict__ volPre, QueueState qs) {
    const PgRenderDesc &rd = rdHead;
    constexpr int NCHUNK = PG_ORDER_WINDOW / 64, ROUNDS = PG_ORDER_WINDOW / 1024, NW = 1024 / 64;
    static_assert(PG_ORDER_WINDOW % 1024 == 0 && PG_ORDER_CLASSES == 16, "k_shade_order: window of whole blocks, 16 classes");
    const int r = blockIdx.x & (PG_REGIONS - 1), base = (blockIdx.x >> 3) * PG_ORDER_WINDOW;
    const int count = q.counts[r * PG_COUNT_STRIDE];
    if (base >= count) return;
    __shared__ int s_cnt[NCHUNK][PG_ORDER_CLASSES + 1];  // entries of a class in a 64-entry chunk, then their first place in the window
    __shared__ int s_total[PG_ORDER_CLASSES];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int cls[ROUNDS], rank[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int chunk = k * NW + wave, j = base + chunk * 64 + lane;
        int c = PG_ORDER_CLASSES - 1;
        if (j < count) {
            const size_t e = (size_t)r * q.regionCap + j;
            const int prim = __float_as_int(hits[e].x);
            c = prim < 0 ? PG_ORDER_CLASSES - 2 : (sc.primClass ? sc.primClass[prim] : 0);
            if constexpr (VOL) {
                const float4 d4 = q.d[e];
                const int slot = __float_as_int(d4.w), med = qs.L ? qs.medium[e] : vs.medium[slot];  // (path state in queue order, or by slot)
                if (med && !(sc.mediaGrid && sc.mediaGrid[med - 1] >= 0)) {
                    const int4 meta = qs.L ? qs.meta[e] : st.meta[slot];
                    const uint64_t index = (uint64_t)(uint32_t)meta.x | ((uint64_t)(uint32_t)meta.y << 32);
                    const int dim = (int)((uint32_t)meta.w >> 20);
                    const float uc = halton_sample(sc, rd, index, dim);
                    int channel;
                    float dist;
                    homogeneous_sample_distance(sc.media[med - 1], uc, halton_sample(sc, rd, index, dim + 1), channel, dist);
                    const float tMaxRay = prim >= 0 ? hitT[e] : q.o[e].w;
                    volPre[e] = make_float2(__int_as_float(channel), dist);
                    if (dist / sqrtf(lensq(mk(d4.x, d4.y, d4.z))) < tMaxRay) c = PG_ORDER_CLASSES - 3;  // (only the grouping depends on this)
                }
            }
        }
        unsigned long long mine = 0;
        for (int b = 0; b < PG_ORDER_CLASSES; ++b) {
            const unsigned long long m = __ballot(c == b);
            if (lane == 0) s_cnt[chunk][b] = __popcll(m);
            if (c == b) mine = m;
        }
        cls[k] = c;
        rank[k] = __popcll(mine & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (threadIdx.x < PG_ORDER_CLASSES) {  // per class: where each chunk's entries start among the class's
        int sum = 0;
        for (int ch = 0; ch < NCHUNK; ++ch) { const int v = s_cnt[ch][threadIdx.x]; s_cnt[ch][threadIdx.x] = sum; sum += v; }
        s_total[threadIdx.x] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int chunk = k * NW + wave, j = base + chunk * 64 + lane;
        if (j >= count) continue;
        int off = s_cnt[chunk][cls[k]] + rank[k];
        for (int b = 0; b < PG_ORDER_CLASSES; ++b) if (b < cls[k]) off += s_total[b];
        order[(size_t)r * q.regionCap + base + off] = r * q.regionCap + j;
    }
}
void launch_shade_order(const DScene &sc, RayQueue qin, const float4 *hits, int *order, hipStream_t s) {
    const int nblk = PG_REGIONS * ((qin.regionCap + PG_ORDER_WINDOW - 1) / PG_ORDER_WINDOW);
    if (nblk == 0 || !sc.primClass || !order) return;
    hipLaunchKernelGGL(k_shade_order<false>, dim3(nblk), dim3(1024), 0, s, sc, qin, hits, order, RenderDescHead{}, PathState{}, VolState{}, (const float *)nullptr, (float2 *)nullptr, QueueState{});
}
void launch_shade_order_vol(const DScene &sc, const RenderParams &rp, PathState st, VolState vs, RayQueue qin, const float4 *hits, const float *hitT,
                            int *order, float2 *volPre, hipStream_t s, int cur) {
    const int nblk = PG_REGIONS * ((qin.regionCap + PG_ORDER_WINDOW - 1) / PG_ORDER_WINDOW);
    if (nblk == 0 || !order) return;
    if (volPre) hipLaunchKernelGGL(k_shade_order<true>, dim3(nblk), dim3(1024), 0, s, sc, qin, hits, order, rp.rd, st, vs, hitT, volPre, st.qs[cur]);
    else launch_shade_order(sc, qin, hits, order, s);
}
void launch_shade(const DScene &sc, const RenderParams &rp, PathState st, RayQueue qin, const float4 *hits, RayQueue qnext,
                  RayQueue qshadow, RayQueue qmis, unsigned long long *lightTriTests, hipStream_t s, int cur, const SssState *sss, PendJoin pj) {
    int nblk = rp.retryCount > 0 ? (rp.retryCount + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK : PG_REGIONS * (qin.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    const VolState vs = {};
    const float *noT = nullptr;
    QueueState qi = st.qs[cur], qo = st.qs[cur ^ 1];
    if (!pj.list || sss) qi.pend = qo.pend = nullptr;  // every vertex's pending terms for the full-queue launch_resolve
    if (pj.first) qi.pend = nullptr;                   // camera rays: nothing waits
    const SssState none = {};
    const GridShade gsh = {nullptr, 0};
    const int mode = pg_shade_mode(sc, rp, false, sss != nullptr, false);  // (the branches below are that function's cases)
    if (sss && sc.nBssrdfs > 0) {  // materials with a BSSRDF are BxDF-list materials: the general kernels
        if (mode == 2) hipLaunchKernelGGL((k_shade<2, false, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, noT, qi, qo, *sss, gsh, pj);
        else hipLaunchKernelGGL((k_shade<1, false, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, noT, qi, qo, *sss, gsh, pj);
    } else if (mode == 3) {  // materials first (not again for the entries a sparse light table sent back: theirs are there)
        if (rp.retryCount == 0) launch_material(sc, rp, st, vs, qin, hits, noT, qi, false, s);
        hipLaunchKernelGGL((k_shade<3, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, noT, qi, qo, none, gsh, pj);
    } else if (mode == 2) hipLaunchKernelGGL((k_shade<2, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, noT, qi, qo, none, gsh, pj);
    else if (mode == 1) hipLaunchKernelGGL((k_shade<1, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, noT, qi, qo, none, gsh, pj);
    else hipLaunchKernelGGL((k_shade<0, false>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, noT, qi, qo, none, gsh, pj);
}
void launch_shade_vol(const DScene &sc, const RenderParams &rp, PathState st, VolState vs, RayQueue qin, const float4 *hits, const float *hitT,
                      RayQueue qnext, RayQueue qshadow, RayQueue qmis, unsigned long long *lightTriTests, hipStream_t s, const SssState *sss,
                      float4 *gridVertex, int phase, int cur) {
    int nblk = rp.retryCount > 0 ? (rp.retryCount + PG_SHADE_BLOCK - 1) / PG_SHADE_BLOCK : PG_REGIONS * (qin.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    const QueueState none = {nullptr, nullptr, nullptr, nullptr};
    const QueueState qi = st.qs[cur], qo = st.qs[cur ^ 1];  // the plain kernels: path state in queue order
    const SssState nosss = {};
    const GridShade gsh = {gridVertex, phase};
    const int mode = pg_shade_mode(sc, rp, true, sss != nullptr, phase != 0);
    if (phase != 0 && sss && sc.nBssrdfs > 0) {  // a grid medium AND BSSRDF materials: the second phase hands a path that goes on through a BSSRDF to the probe chains
        if (mode == 2) hipLaunchKernelGGL((k_shade<2, true, true, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, hitT, none, none, *sss, gsh, PendJoin{});
        else hipLaunchKernelGGL((k_shade<1, true, true, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, hitT, none, none, *sss, gsh, PendJoin{});
    } else if (phase != 0) {  // a scene with a grid medium: the two-phase kernels
        if (mode == 2) hipLaunchKernelGGL((k_shade<2, true, false, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, hitT, none, none, nosss, gsh, PendJoin{});
        else hipLaunchKernelGGL((k_shade<1, true, false, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, hitT, none, none, nosss, gsh, PendJoin{});
    } else if (sss && sc.nBssrdfs > 0) {
        if (mode == 2) hipLaunchKernelGGL((k_shade<2, true, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, hitT, none, none, *sss, gsh, PendJoin{});
        else hipLaunchKernelGGL((k_shade<1, true, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, hitT, none, none, *sss, gsh, PendJoin{});
    } else {
#define PG_LAUNCH_VOL(MODE_) hipLaunchKernelGGL((k_shade<MODE_, true>), dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, qin, hits, qnext, qshadow, qmis, lightTriTests, vs, hitT, qi, qo, nosss, gsh, PendJoin{})
        if (mode == 3) {
            if (rp.retryCount == 0) launch_material(sc, rp, st, vs, qin, hits, hitT, qi, true, s);
            PG_LAUNCH_VOL(3);
        } else if (mode == 2) PG_LAUNCH_VOL(2);
        else PG_LAUNCH_VOL(1);
#undef PG_LAUNCH_VOL
    }
}

// EstimateDirect's two "Add ... contribution" steps (integrator.cpp:143-161, 196-212) and
// L += beta * Ld / lightPdf (integrator.cpp:104, path.cpp:122-126), once both rays are back.
// One vertex: i = the queue position its pending terms lie at, or -1 (every lane of the block calls it: the statistics are counted per wave)
template <bool EXT>
PG_DEV void resolve_entry(const DScene &sc, const PathState &st, int i, const RayQueue &qmis, const int *__restrict__ occluded,
                          const float4 *__restrict__ misHits, const QueueState &qsNext, unsigned long long *stats) {
    // stats != nullptr: the launch over a bounce's main queue counts "Zero-radiance paths" (path.cpp:119-126): a vertex whose pdInfo names a light
    // (k_shade chose one: its BSDF has non-specular BxDFs) is one of totalPaths, and one of zeroRadiancePaths when its Ld comes out black
    PendingInfo info = pending_nothing();
    if (i >= 0) info = pending_info(st.pdInfo[i]);  // the pending terms lie in queue order (PathState)
    bool black = true;
    if (i >= 0 && pending_any(info)) {
        const PendingLight pl = pending_light(st.pdLight[i]);
        const PendingBeta pb = pending_beta(st.pdBeta[i]);
        Spec Ld = sp(0);
        if (info.posShadow >= 0) Ld = ld_add_light(Ld, pl.term, occluded[info.posShadow]);
        if (info.posMis >= 0) {
            const PendingMis pm = pending_mis(st.pdMis[i]);
            const float4 h = misHits[info.posMis];
            const int prim = __float_as_int(h.x);
            Spec Li = sp(0);  // the sampled light's radiance along the MIS ray, integrator.cpp:199-208
            if (prim >= 0) {
                Tri t = load_tri(sc, prim);
                if (t.light == info.lightNum) {  // lightIsect.primitive->GetAreaLight() == &light
                    const float4 d4 = qmis.d[info.posMis];
                    const bool onSphere = EXT && (t.flags & PG_PRIM_SPHERE);
                    Li = area_light_le<EXT>(sc, sc.lights[t.light], prim, t, h, onSphere ? qmis.o[info.posMis] : d4, mk(d4.x, d4.y, d4.z));
                }
            } else if (EXT && sc.lights[info.lightNum].type == PG_LIGHT_INFINITE) {  // integrator.cpp:207-208: no surface hit: Li = light.Le(ray)
                const float4 d4 = qmis.d[info.posMis];
                Li = env_le(sc, sc.lights[info.lightNum], mk(d4.x, d4.y, d4.z));
            }
            Ld = ld_add_mis(Ld, pm.f, Li, sp(1.f), pb.misWeight, pm.pdf);
        }
        // the path's L: with its ray in the next queue's state, or -- the path is over -- in its slot
        float4 *Lp = pending_L(st, qsNext, info.where);
        const Spec add = direct_addend(pb.beta, Ld, pl.lightSelectPdf);  // beta * UniformSampleOneLight(...)
        black = is_black(add);
        *Lp = direct_add_to_L(*Lp, add);
    }
    if (stats) {  // (uniform over the launch)
        const int counts = i >= 0 ? resolve_path_counts(info.lightNum, black) : 0;
        stats_count(stats, PG_STAT_PATHS, (counts & 1) != 0);
        stats_count(stats, PG_STAT_PATHS_ZERO, (counts & 2) != 0);
    }
}
template <bool EXT>
__global__ __launch_bounds__(PG_BLOCK) void k_resolve(DScene sc, PathState st, RayQueue qin, RayQueue qmis, const int *__restrict__ occluded,
                                                       const float4 *__restrict__ misHits, QueueState qsNext, unsigned long long *stats) {
    resolve_entry<EXT>(sc, st, queue_item<>(qin), qmis, occluded, misHits, qsNext, stats);
}
// The same over the vertices k_shade listed (PendJoin): the few with a MIS ray and the paths that ended with something to add or count.  Every other
// vertex's direct lighting is added by the shading launch of the path's next vertex (QueueState::pend).
template <bool EXT>
__global__ __launch_bounds__(PG_BLOCK) void k_resolve_list(DScene sc, PathState st, RayQueue qmis, PendJoin pj, const float4 *__restrict__ misHits,
                                                            QueueState qsNext, unsigned long long *stats, int regionCap) {
    // block b strides over region b & 7 of the list (uniform over the block: resolve_entry counts per wave)
    const int r = blockIdx.x & (PG_REGIONS - 1), n = pj.listCounts[r * PG_COUNT_STRIDE];
    for (int base = (blockIdx.x >> 3) * PG_BLOCK; base < n; base += (gridDim.x >> 3) * PG_BLOCK) {
        const int k = base + threadIdx.x;
        resolve_entry<EXT>(sc, st, k < n ? pj.list[r * regionCap + k] : -1, qmis, pj.occluded, misHits, qsNext, stats);
    }
}
// The grid of both launches: a block per PG_BLOCK entries of the queue's capacity, region by region -- with a bound on the blocks per region, or 0 for none
static int resolve_blocks(const RayQueue &qin, int maxPerRegion) {
    const int perRegion = qin.regionCap / PG_BLOCK;
    return PG_REGIONS * (maxPerRegion > 0 && perRegion > maxPerRegion ? maxPerRegion : perRegion);
}
void launch_resolve_list(const DScene &sc, PathState st, RayQueue qin, RayQueue qmis, PendJoin pj, const float4 *misHits, hipStream_t s,
                         int cur, unsigned long long *stats) {
    // (the list is a few per cent of the queue: the blocks stride over their region instead of a grid for the queue's capacity that would mostly find nothing)
    const int nblk = resolve_blocks(qin, 256);
    if (nblk == 0) return;
    if (sc.ext) hipLaunchKernelGGL(k_resolve_list<true>, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, qmis, pj, misHits, st.qs[cur ^ 1], stats, qin.regionCap);
    else hipLaunchKernelGGL(k_resolve_list<false>, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, qmis, pj, misHits, st.qs[cur ^ 1], stats, qin.regionCap);
}
void launch_resolve(const DScene &sc, PathState st, RayQueue qin, RayQueue qmis, const int *occluded, const float4 *misHits, hipStream_t s,
                    int cur, unsigned long long *stats) {
    const int nblk = resolve_blocks(qin, 0);
    if (nblk == 0) return;
    if (sc.ext) hipLaunchKernelGGL(k_resolve<true>, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, qin, qmis, occluded, misHits, st.qs[cur ^ 1], stats);
    else hipLaunchKernelGGL(k_resolve<false>, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, qin, qmis, occluded, misHits, st.qs[cur ^ 1], stats);
}

// ===========================================================================
// VolPathIntegrator's transmittance rays.  VisibilityTester::Tr (light.cpp:63-81) and Scene::IntersectTr (scene.cpp:57-70)
// are loops of Scene::Intersect calls that step through surfaces without a material; here every loop iteration is one
// closest-hit launch over the queue of rays still under way followed by this kernel, which finishes a ray or re-spawns it.
// ===========================================================================
// p, pError and n of hit_isect's SurfaceInteraction: all that stepping over a surface needs of it (the rest of the interaction is left to the compiler's
// dead-code elimination: nothing else of it is read)
// NEST: the caller can meet hits under two transforms (k_through; the probe chains cannot: scenes with BSSRDF materials and such hits are refused)
template <bool NEST>
PG_DEV void through_point(const DScene &sc, int ri, float4 o4, V3 rayD, float4 h4, int prim, const Tri &tri, V3 &p, V3 &pError, V3 &n) {
    int inst = sc.hitInst ? sc.hitInst[ri] : -1, inst2 = -1;
    if constexpr (NEST) nest_decode(sc, inst, inst2);
    QuadricUv quv;
    const Isect is = hit_isect(sc, inst_xf(sc, inst, ri), inst_xf(sc, inst2, ri, true), o4, rayD, h4, prim, tri, quv);
    p = is.p; pError = is.pError; n = is.n;
}
// GRID: a segment inside a GridDensityMedium is attenuated by ratio tracking (grid.cpp:88-120), whose numbers come from the path's
// sampler: they are drawn here, at the path's current dimension / stream position, which st.meta[slot] keeps for the shading
// kernel's second phase.  The host runs the kind-0 rays of a bounce to their ends before the kind-1 rays start (the reference
// evaluates visibility.Tr before it samples the BSDF: integrator.cpp:146-150, then :164-212).
template <int KIND, bool GRID>
__global__ __launch_bounds__(PG_BLOCK) void k_through(DScene sc, PathState st, VolState vs, RayQueue qin, const float4 *__restrict__ hits,
                                                       const float *__restrict__ hitT, int hitBase, RayQueue qout, RenderParams rp) {
    const int i = queue_item<>(qin);
    bool push = false;
    float4 no = make_float4(0, 0, 0, 0), nd = make_float4(0, 0, 0, 0);
    if (i >= 0) {
        const float4 o4 = qin.o[i], d4 = qin.d[i];
        const int slot = __float_as_int(d4.w);
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const int ri = hitBase + i;
        const float4 h4 = hits[ri];
        const int prim = __float_as_int(h4.x);
        const bool surface = prim >= 0;
        const Through acc = through_acc(vs.trAcc[KIND][slot]);
        Spec Tr = acc.Tr;
        int med = acc.medium;
        Tri tri;
        if (surface) tri = load_tri(sc, prim);
        const bool opaque = surface && sc.materials[tri.material].type != PG_MAT_NONE;  // isect.primitive->GetMaterial() != nullptr
        if (KIND == 0 && opaque) Tr = sp(0.f);  // light.cpp:70-72: blocked
        else {
            if (GRID && med && sc.mediaGrid[med - 1] >= 0) {
                const PgDensityGrid &gd = sc.grids[sc.mediaGrid[med - 1]];
                int4 meta = st.meta[slot];
                const uint64_t index = (uint64_t)(uint32_t)meta.x | ((uint64_t)(uint32_t)meta.y << 32);
                int dim = (int)((uint32_t)meta.w >> 20);
                const bool tileSerial = rp.rd->sampler >= PG_SAMPLER_RANDOM;
                auto draw = [&]() -> float { return tileSerial ? ts_get1d(sc, slot) : halton_sample(sc, rp.rd, index, dim++); };
                Tr = Tr * sp(grid_tr(gd, sc.gridDensity + gd.density_offset, mk(o4.x, o4.y, o4.z), rayD, surface ? hitT[ri] : o4.w, draw));
                meta.w = (int)(((uint32_t)dim << 20) | ((uint32_t)meta.w & 0xfffffu));
                st.meta[slot] = meta;
            } else if (med) Tr = Tr * medium_tr(sc.media[med - 1], surface ? hitT[ri] : o4.w, sqrtf(lensq(rayD)));
            if (KIND == 1 && !(surface && !opaque)) {
                // IntersectTr is over (scene.cpp:64-67): the sampled light's radiance along the ray (integrator.cpp:199-208)
                const int lightNum = pending_info(st.pdInfo[slot]).lightNum;
                Spec Li = sp(0);
                if (surface) {
                    if (tri.light == lightNum) Li = area_light_le<true>(sc, sc.lights[tri.light], prim, tri, h4, o4, rayD);
                } else if (sc.lights[lightNum].type == PG_LIGHT_INFINITE) Li = env_le(sc, sc.lights[lightNum], rayD);
                vs.misLi[slot] = vol_mis_li_encode(Li);
            } else if (surface) {
                // a surface without a material: step over it (light.cpp:79 isect.SpawnRayTo(p1), scene.cpp:68 isect.SpawnRay(ray.d))
                V3 p, pError, n;
                through_point<true>(sc, ri, o4, rayD, h4, prim, tri, p, pError, n);
                int mIn, mOut;
                prim_interface(sc, prim, med, mIn, mOut);
                V3 d = rayD;
                if (KIND == 0) {  // on towards the light sample the vertex kept
                    const float4 a = vs.p1[0][slot], b = vs.p1[1][slot], c = vs.p1[2][slot];
                    const LightSample ls = {mk(a.x, a.y, a.z), mk(c.x, c.y, c.z), mk(b.x, b.y, b.z)};
                    d = shadow_ray_to(p, pError, n, ls, slot, no, nd);
                } else {
                    const V3 origin = offset_ray_origin(p, pError, n, rayD);
                    no = make_float4(origin.x, origin.y, origin.z, PG_INF);
                    nd = make_float4(d.x, d.y, d.z, __int_as_float(slot));
                }
                med = dot(d, n) > 0 ? mOut : mIn;
                push = true;
            }
        }
        vs.trAcc[KIND][slot] = through_acc_encode(Tr, med);
    }
    int pos;
    block_push<1, false>(&qout, &push, &pos);
    if (push) { qout.o[pos] = no; qout.d[pos] = nd; }
    if (push && sc.rayTimes) PG_QUEUE_TIMES(sc, qout)[pos] = PG_QUEUE_TIMES(sc, qin)[i];
}
void launch_through(const DScene &sc, PathState st, VolState vs, int kind, RayQueue qin, const float4 *hits, const float *hitT, int hitBase,
                    RayQueue qout, hipStream_t s, const RenderParams *rpGrid) {
    int nblk = PG_REGIONS * (qin.regionCap / PG_BLOCK);
    if (nblk == 0) return;
    if (rpGrid) {
        if (kind == 0) hipLaunchKernelGGL((k_through<0, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, vs, qin, hits, hitT, hitBase, qout, *rpGrid);
        else hipLaunchKernelGGL((k_through<1, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, vs, qin, hits, hitT, hitBase, qout, *rpGrid);
        return;
    }
    const RenderParams none = {};
    if (kind == 0) hipLaunchKernelGGL((k_through<0, false>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, vs, qin, hits, hitT, hitBase, qout, none);
    else hipLaunchKernelGGL((k_through<1, false>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, vs, qin, hits, hitT, hitBase, qout, none);
}
// EstimateDirect's sums with handleMedia = true (integrator.cpp:143-161, 196-212), once the through rays are finished
// QS: the pending terms lie at the ray's queue position and the path's L with its next ray (queue-order state, PathState) -- else by slot
template <bool QS>
__global__ __launch_bounds__(PG_BLOCK) void k_resolve_vol(DScene sc, PathState st, VolState vs, RayQueue qin, QueueState qsNext) {
    const int i = queue_item<>(qin);
    if (i < 0) return;
    const int slot = QS ? i : __float_as_int(qin.d[i].w);
    const PendingInfo info = pending_info(st.pdInfo[slot]);
    if (!pending_any(info)) return;
    const PendingLight pl = pending_light(st.pdLight[slot]);
    const PendingMis pm = pending_mis(st.pdMis[slot]);
    const PendingBeta pb = pending_beta(st.pdBeta[slot]);
    Spec Ld = sp(0);
    if (info.posShadow >= 0) {
        const VolLight li = vol_light(vs.pdLi[slot]);
        Ld = ld_add_vol_light(Ld, pl.term, li.Li, through_acc(vs.trAcc[0][slot]).Tr, li.lightPdf, [&]() { return vol_light_weight<QS>(vs, slot, info); });
    }
    if (info.posMis >= 0) Ld = ld_add_mis(Ld, pm.f, vol_mis_li(vs.misLi[slot]), through_acc(vs.trAcc[1][slot]).Tr, pb.misWeight, pm.pdf);
    float4 *Lp = QS ? pending_L(st, qsNext, info.where) : &st.L[slot];
    *Lp = direct_add_to_L(*Lp, direct_addend(pb.beta, Ld, pl.lightSelectPdf));
}
void launch_resolve_vol(const DScene &sc, PathState st, VolState vs, RayQueue qin, hipStream_t s, int cur) {
    int nblk = PG_REGIONS * (qin.regionCap / PG_BLOCK);
    if (nblk == 0) return;
    if (st.qs[0].L) hipLaunchKernelGGL(k_resolve_vol<true>, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, vs, qin, st.qs[cur ^ 1]);
    else hipLaunchKernelGGL(k_resolve_vol<false>, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, st, vs, qin, st.qs[0]);
}
__global__ void k_fill_int(int *p, int value, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = value;
}
void launch_fill_int(int *p, int value, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_fill_int, dim3((n + 255) / 256), dim3(256), 0, s, p, value, n);
}

// ===========================================================================
// Subsurface scattering: the rest of the BSSRDF branch of PathIntegrator::Li (path.cpp:152-174) behind k_shade<., ., true>.
// SeparableBSSRDF::Sample_Sp (bssrdf.cpp:253-328) intersects the probe segment base -> pTarget again and again from each hit
// (`base = next->si`), keeps every hit on primitives of the entry point's material in a list and picks entry (int)(u1 * nFound).
// Here a chain is walked twice by the traversal kernel -- a list per path has no bound (degenerate soups give hundreds of hits) --:
// pass 1 counts the hits on the material, pass 2 stops at the chosen one.  Each step is one k_trace<0, .> launch over the
// chains still under way followed by k_sss_probe.
// ===========================================================================
// Invariant others rely on: a chain has ONE probe ray under way -- an entry of qin appends at most one entry to qout, with its own slot as tag -- so a slot
// appears at most once in a queue.  k_sss_tally (pg_subsurfacequery.h) counts a sample's probe rays with a plain chain[tag] += 1 on that ground.
// NEST: DScene::hasNest -- the chain's hits can lie under two transforms (a moving shape inside an object definition)
template <int PASS, bool VOL, bool NEST = false>
__global__ __launch_bounds__(PG_BLOCK) void k_sss_probe(DScene sc, SssState sss, RayQueue qin, const float4 *__restrict__ hits, RayQueue qout, int first) {
    const int i = queue_item<>(qin);
    bool push = false;
    float4 no = make_float4(0, 0, 0, 0), nd = make_float4(0, 0, 0, 0);
    if (i >= 0) {
        const float4 o4 = qin.o[i], d4 = qin.d[i];
        const int slot = __float_as_int(d4.w);
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const float4 h4 = hits[i];
        const int prim = __float_as_int(h4.x);
        int2 cnt = sss.count[slot];
        // volpath: the medium of this probe ray -- base.GetMedium(d) of the previous hit (none for the first ray: Sample_Sp's `base`
        // carries no MediumInterface) -- is what a hit primitive without a transition of its own reports (primitive.cpp:121-125)
        int rayMed = 0;
        if constexpr (VOL) rayMed = first ? 0 : sss.medium[slot].x;
        bool go = prim >= 0;  // bssrdf.cpp:306: no intersection ends the chain
        if (PASS == 2 && cnt.x == 0) go = false;  // nothing to choose from
        if (go) {
            const Tri tri = load_tri(sc, prim);
            if (tri.material == __float_as_int(sss.frame[2][slot].w)) {  // bssrdf.cpp:311: si.primitive->GetMaterial() == this->material
                if (PASS == 1) ++cnt.x;
                else {
                    const float u1 = sss.po[slot].w;
                    int selected = (int)(u1 * cnt.x);  // bssrdf.cpp:321
                    selected = selected < 0 ? 0 : (selected > cnt.x - 1 ? cnt.x - 1 : selected);
                    if (cnt.y == selected) {
                        sss.hit[slot] = h4; sss.hitO[slot] = o4; sss.hitD[slot] = d4;
                        int hInst = sc.hitInst ? sc.hitInst[i] : -1, hInst2 = -1;
                        sss.hitInst[slot] = hInst;  // (NEST: the pair as k_trace wrote it)
                        if constexpr (NEST) nest_decode(sc, hInst, hInst2);
                        if (sss.hitXf && hInst >= 0 && sc.instances[hInst].animated)  // a moving instance: the matrices k_trace interpolated for this probe ray
                            for (int q = 0; q < 33; ++q) sss.hitXf[(size_t)PG_XF_STRIDE * slot + q] = sc.animXf[(size_t)PG_XF_STRIDE * i + q];
                        if (NEST && sss.hitXf && hInst2 >= 0 && sc.instances[hInst2].animated)
                            for (int q = 0; q < 33; ++q) sss.hitXf[(size_t)PG_XF_STRIDE * ((size_t)sss.hitXfNest + slot) + q] = sc.animXf[(size_t)PG_XF_STRIDE * ((size_t)sc.nestXfOff + i) + q];
                        if constexpr (VOL) sss.medium[slot] = make_int2(rayMed, rayMed);
                        go = false;
                    }
                    ++cnt.y;
                }
                sss.count[slot] = cnt;
            }
            if (go) {  // base = next->si; base.SpawnRayTo(pTarget): interaction.h:65-71
                V3 p, pError, n;
                through_point<NEST>(sc, i, o4, rayD, h4, prim, tri, p, pError, n);
                const float4 tg = sss.target[slot];
                const V3 d = mk(tg.x, tg.y, tg.z) - p;
                if (!(d.x == 0 && d.y == 0 && d.z == 0)) {
                    const V3 origin = offset_ray_origin(p, pError, n, d);
                    no = make_float4(origin.x, origin.y, origin.z, 1 - PG_SHADOW_EPS);
                    nd = make_float4(d.x, d.y, d.z, __int_as_float(slot));
                    push = true;
                    if constexpr (VOL) {  // Interaction::GetMedium(d), interaction.h:86-88
                        int mIn, mOut;
                        prim_interface(sc, prim, rayMed, mIn, mOut);
                        sss.medium[slot] = make_int2(dot(d, n) > 0 ? mOut : mIn, 0);
                    }
                }
            }
        }
    }
    int pos;
    block_push<1, false>(&qout, &push, &pos);
    if (push) { qout.o[pos] = no; qout.d[pos] = nd; }
    if (push && sc.rayTimes) PG_QUEUE_TIMES(sc, qout)[pos] = PG_QUEUE_TIMES(sc, qin)[i];
}
void launch_sss_probe(const DScene &sc, SssState sss, int pass, RayQueue qin, const float4 *hits, RayQueue qout, hipStream_t s, bool vol, bool first) {
    int nblk = PG_REGIONS * (qin.regionCap / PG_BLOCK);
    if (nblk == 0) return;
    const int f = first ? 1 : 0;
    if (sc.hasNest) {  // (hits under two transforms: instantiations of their own, the others keep their registers)
        if (vol) {
            if (pass == 1) hipLaunchKernelGGL((k_sss_probe<1, true, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
            else hipLaunchKernelGGL((k_sss_probe<2, true, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
        } else if (pass == 1) hipLaunchKernelGGL((k_sss_probe<1, false, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
        else hipLaunchKernelGGL((k_sss_probe<2, false, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
    } else if (vol) {
        if (pass == 1) hipLaunchKernelGGL((k_sss_probe<1, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
        else hipLaunchKernelGGL((k_sss_probe<2, true>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
    } else if (pass == 1) hipLaunchKernelGGL((k_sss_probe<1, false>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
    else hipLaunchKernelGGL((k_sss_probe<2, false>), dim3(nblk), dim3(PG_BLOCK), 0, s, sc, sss, qin, hits, qout, f);
}

// The exit vertex pi of a path that went through a BSSRDF (path.cpp:157-174): Sp and its pdf (bssrdf.cpp:322-327), beta *= S / pdf,
// direct lighting at pi under the adapter BSDF (UniformSampleOneLight / EstimateDirect: the shadow and MIS rays and their pending terms,
// indexed by the job's queue position, resolved by k_resolve over the job queue), the next direction, Russian roulette (path.cpp:176-184).
// The path's L, beta and meta wait in their slot (k_shade put them there; k_resolve added the entry vertex's direct lighting to L).
// VOL (volpath.cpp:151-176): UniformSampleOneLight with handleMedia -- the two rays are transmittance rays (k_through), their factors
// stay apart for k_resolve_vol, every pending term and the path's state are indexed by slot -- and the next ray starts in pi.GetMedium(wi).
template <bool VOL>
__global__ __launch_bounds__(PG_SHADE_BLOCK) void k_sss_exit(DScene sc, RenderParams rp, PathState st, SssState sss, RayQueue qnext, RayQueue qshadow,
                                                            RayQueue qmis, unsigned long long *lightTriTests, QueueState qsOut, VolState vs, int phase, float4 *exitVertex) {
    // phase (VOL, a scene with a GridDensityMedium): 1 = up to the exit vertex's direct lighting -- its transmittance rays draw ratio tracking's numbers from the
    // path's sampler BEFORE the next direction is drawn (integrator.cpp:146-150, then path.cpp:165-173), as at k_shade's vertices --, 2 = the next direction and
    // Russian roulette, once those rays are through and k_resolve_vol has added the lighting; exitVertex[slot].w says which jobs phase 1 left alive.  0: all at once.
    const int j = queue_item<PG_SHADE_BLOCK>(sss.qjob);
    __shared__ float4 s_ray[3][2][PG_SHADE_BLOCK];
    const int tid = threadIdx.x;
    bool pushNext = false, pushShadow = false, pushMis = false;
    int slot = 0, lightNum = -1, nextBin = 0;
    unsigned int nLightTests = 0;
    float4 outL = make_float4(0, 0, 0, 0), outB = make_float4(0, 0, 0, 0);
    int4 outM = make_int4(0, 0, 0, 0);
    bool alive = false;
    if (j >= 0) {
        slot = __float_as_int(sss.qjob.d[j].w);
        if (phase != 2) st.pdInfo[VOL ? slot : j] = pending_info_encode(-1, -1, -1, VOL ? 0 : ~slot);
        const int2 cnt = sss.count[slot];
        alive = cnt.x > 0;  // bssrdf.cpp:318: no hit on the material: Sample_Sp returns black and the path ends (its L is in its slot)
        if (phase == 2) alive = __float_as_int(exitVertex[slot].w) == 1;
    }
    const int pdi = VOL ? slot : j;  // index of this vertex's pending direct-light terms
    float volWeight = 0;
    if (alive) {
        const PgRenderDesc &rd = rp.rd;
        const float4 L4 = st.L[slot], B4 = st.beta[slot];
        const int4 meta = st.meta[slot];
        Spec L = sp3(L4.x, L4.y, L4.z), beta = sp3(B4.x, B4.y, B4.z);
        const uint64_t index = (uint64_t)(uint32_t)meta.x | ((uint64_t)(uint32_t)meta.y << 32);
        int dim = (int)((uint32_t)meta.w >> 20);
        const float etaScale = __int_as_float(meta.z);
        const int bounces = meta.w & 0xffff;  // already counts this vertex (k_shade)
        const bool tileSerial = rd.sampler >= PG_SAMPLER_RANDOM;
        auto draw1 = [&]() -> float { return tileSerial ? ts_get1d(sc, slot) : halton_sample(sc, rd, index, dim++); };
        auto draw2 = [&](float &a, float &b) {
            if (tileSerial) ts_get2d(sc, rd.sampler, slot, a, b);
            else { a = halton_sample(sc, rd, index, dim); b = halton_sample(sc, rd, index, dim + 1); dim += 2; }
        };
        // ---- pi: the chosen hit as a SurfaceInteraction (the tail of Triangle::Intersect / Sphere::Intersect, then the instance's transform)
        const float4 h4 = sss.hit[slot], o4 = sss.hitO[slot], d4 = sss.hitD[slot];
        const int prim = __float_as_int(h4.x);
        int inst = sss.hitInst[slot], inst2;
        nest_decode(sc, inst, inst2);  // (DScene::hasNest: the chosen hit may lie under two transforms)
        // (a moving instance's matrices: what k_sss_probe kept by slot of k_trace's interpolation for the probe ray that found the hit)
        const InstXf outer = {sc.instances, sss.hitXf, 0, inst, slot}, inner = {sc.instances, sss.hitXf, sss.hitXfNest, inst2, slot};
        const V3 rayD = mk(d4.x, d4.y, d4.z);
        const Tri tri = load_tri(sc, prim);
        QuadricUv quv;
        Isect is = hit_isect(sc, outer, inner, o4, rayD, h4, prim, tri, quv);
        // ---- Sp(pi) = Sr(|po - pi|) and Pdf_Sp(pi) / nFound (bssrdf.cpp:322-327), beta *= S / pdf (path.cpp:158)
        const float4 po4 = sss.po[slot], f0 = sss.frame[0][slot], f1 = sss.frame[1][slot], f2 = sss.frame[2][slot];
        const V3 poP = mk(po4.x, po4.y, po4.z);
        DBssrdf b = bssrdf_bind(sc.bssrdfs[__float_as_int(f1.w)], sc.bssrdfTables);
        const float4 cs = sss.coef[0][slot], cr = sss.coef[1][slot];
        b.sigma_t[0] = cs.x; b.sigma_t[1] = cs.y; b.sigma_t[2] = cs.z; b.rho[0] = cr.x; b.rho[1] = cr.y; b.rho[2] = cr.z;
        const int nFound = sss.count[slot].x;
        bool through = true;  // S and its pdf let the path through (phase 2: phase 1 found that, and beta has the factor)
        if (phase != 2) {
            const float pdf = bssrdf_pdf_sp(b, mk(f1.x, f1.y, f1.z), mk(f2.x, f2.y, f2.z), mk(f0.x, f0.y, f0.z), poP, is.p, is.n) / nFound;
            const Spec S = bssrdf_sr(b, sqrtf(lensq(poP - is.p)));
            through = !(is_black(S) || pdf == 0);
            if (through) beta = beta * (S / pdf);
        }
        if (!through) alive = false;
        else {
            // Sample_S's BSDF at pi (bssrdf.cpp:243-248): shading frame of pi, the adapter; pi.wo = pi.shading.n
            AdapterBsdf ab;
            ab.ns = is.ns; ab.ng = is.n; ab.ss = normalize(is.sdpdu); ab.ts = cross(ab.ns, ab.ss); ab.eta = f0.w;
            is.wo = is.ns;
            int mIn = 0, mOut = 0;  // VOL: pi's MediumInterface (the primitive's own, or the medium of the probe ray that found it)
            if constexpr (VOL) prim_interface(sc, prim, sss.medium[slot].y, mIn, mOut);
            // ---- L += beta * UniformSampleOneLight(pi, ...) (path.cpp:161-163; integrator.cpp:85-215)
            const float *tab = (phase != 2 && sc.nLights > 0) ? light_distribution(sc, is.p) : nullptr;
            if (tab) {
                float lightSelPdf;
                lightNum = sample_discrete(tab, sc.nLights, draw1(), lightSelPdf);
                if (lightSelPdf != 0) {
                    float uL0, uL1, uS0, uS1;
                    draw2(uL0, uL1);
                    draw2(uS0, uS1);
                    const DirectSetup ed = estimate_direct_setup<true>(sc, ab, is.p, is.pError, is.n, is.wo, lightNum, uL0, uL1, uS0, uS1);
                    Spec lightTerm = sp(0);  // (PendingLight::term: volpath keeps f * |cos| apart from Li)
                    if (ed.light.shadow) {
                        [[maybe_unused]] const V3 shD = shadow_ray_to(is.p, is.pError, is.n, ed.light.ls, slot, s_ray[1][0][tid], s_ray[1][1][tid]);
                        pushShadow = true;
                        if constexpr (VOL) {
                            lightTerm = ed.light.f;
                            volWeight = store_vol_light_sample(vs, slot, ed.light, dot(shD, is.n) > 0 ? mOut : mIn);
                        } else lightTerm = direct_light_folded(ed.light);
                    }
                    st.pdLight[pdi] = pending_light_encode(lightTerm, lightSelPdf);
                    st.pdBeta[pdi] = pending_beta_encode(beta, 0.f);
                    if (ed.mis.cand) {
                        V3 misRo;
                        spawn_ray(is, ed.mis.wi, misRo);
                        const float lightPdf2 = mis_light_pdf<true>(sc, ed.mis.lightPrim, ed.mis.area, ed.mis.inside, is.p, misRo, ed.mis.wi, nLightTests);
                        if (lightPdf2 != 0) {
                            s_ray[2][0][tid] = make_float4(misRo.x, misRo.y, misRo.z, PG_INF);
                            s_ray[2][1][tid] = make_float4(ed.mis.wi.x, ed.mis.wi.y, ed.mis.wi.z, __int_as_float(slot));
                            pushMis = true;
                            st.pdMis[pdi] = pending_mis_encode(ed.mis.f, ed.mis.pdf);
                            st.pdBeta[pdi].w = pending_mis_weight(ed.mis.pdf, lightPdf2);
                            if constexpr (VOL) vs.trAcc[1][slot] = through_acc_start(dot(ed.mis.wi, is.n) > 0 ? mOut : mIn);
                        }
                    }
                }
            }
            int newFlags = phase == 1 ? (meta.w & 0xf0000) : 0;  // (phase 1 leaves the flags as they came)
            if (phase != 1) {
            // ---- indirect illumination from pi (path.cpp:165-173), then Russian roulette (:176-184)
            V3 wi;
            float pdf2, u0, u1;
            draw2(u0, u1);
            int sampledType = 0;
            const Spec f = ad_sample_f(ab, is.wo, wi, u0, u1, pdf2, PG_BSDF_ALL, sampledType);
            if (!(is_black(f) || pdf2 == 0.f)) {
                beta = beta * ((f * absdot(wi, ab.ns)) / pdf2);
                if (sampledType & PG_BSDF_SPECULAR) newFlags |= PG_META_SPECULAR;
                V3 nextO;
                spawn_ray(is, wi, nextO);
                s_ray[0][0][tid] = make_float4(nextO.x, nextO.y, nextO.z, PG_INF);
                s_ray[0][1][tid] = make_float4(wi.x, wi.y, wi.z, __int_as_float(slot));
                nextBin = dir_octant(wi);
                if constexpr (VOL) vs.medium[slot] = dot(wi, is.n) > 0 ? mOut : mIn;
                pushNext = russian_roulette(beta, etaScale, bounces - 1, rd.rr_threshold, draw1);  // (`bounces` of the reference's loop: this vertex's, before k_shade's increment)
            }
            }
            outL = make_float4(L.r, L.g, L.b, L4.w);
            outB = make_float4(beta.r, beta.g, beta.b, B4.w);
            outM = make_int4(meta.x, meta.y, __float_as_int(etaScale), (dim << 20) | bounces | newFlags);
        }
    }
    const RayQueue outQ[3] = {qnext, qshadow, qmis};
    const bool outPred[3] = {pushNext, pushShadow, pushMis};
    int outPos[3];
    block_push<3, true, PG_SHADE_BLOCK>(outQ, outPred, outPos, nextBin);
    const int posNext = outPos[0], posShadow = outPos[1], posMis = outPos[2];
    if (pushNext) { qnext.o[posNext] = s_ray[0][0][tid]; qnext.d[posNext] = s_ray[0][1][tid]; }
    if (pushShadow) { qshadow.o[posShadow] = s_ray[1][0][tid]; qshadow.d[posShadow] = s_ray[1][1][tid]; }
    if (pushMis) { qmis.o[posMis] = s_ray[2][0][tid]; qmis.d[posMis] = s_ray[2][1][tid]; }
    store_ray_times(sc, sss.qjob, j, outQ, outPred, outPos);  // the rays leaving pi carry the path's time (the job's probe ray has it)
    if (alive) {
        if constexpr (VOL) {  // by slot: L is there already (k_resolve_vol adds to it), beta and meta follow
            st.beta[slot] = outB; st.meta[slot] = outM;
            if (phase != 2) st.pdInfo[slot] = pending_info_encode(posShadow, posMis, lightNum, pending_where_weight(volWeight));
        } else {
            if (pushNext) { qsOut.L[posNext] = outL; qsOut.beta[posNext] = outB; qsOut.meta[posNext] = outM; }  // (L itself already is in the slot)
            st.pdInfo[j] = pending_info_encode(posShadow, posMis, lightNum, pending_where(pushNext, posNext, slot));
        }
    }
    flush_light_tests(lightTriTests, nLightTests);
    // "Path length" of the paths that end inside the BSSRDF branch (path.cpp:157-174: no probe hit, a black S or f, Russian roulette): the
    // reference's `bounces` is the entry vertex's, the stored count less k_shade's increment
    // (two phases: a job reports where it ends -- in phase 1 when the exit vertex did not come about, in phase 2 otherwise)
    if (VOL && phase == 1 && j >= 0) exitVertex[slot] = make_float4(0, 0, 0, __int_as_float(alive ? 1 : 0));
    stats_path_end(lightTriTests, j >= 0 && !pushNext && (phase == 0 || (phase == 1) != alive), j >= 0 ? (st.meta[slot].w & 0xffff) - 1 : 0);
}
void launch_sss_exit(const DScene &sc, const RenderParams &rp, PathState st, SssState sss, RayQueue qnext, RayQueue qshadow, RayQueue qmis,
                     unsigned long long *lightTriTests, hipStream_t s, int nxt, bool vol, VolState vs, int phase, float4 *exitVertex) {
    int nblk = PG_REGIONS * (sss.qjob.regionCap / PG_SHADE_BLOCK);
    if (nblk == 0) return;
    if (vol) hipLaunchKernelGGL(k_sss_exit<true>, dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, sss, qnext, qshadow, qmis, lightTriTests, st.qs[nxt], vs, phase, exitVertex);
    else hipLaunchKernelGGL(k_sss_exit<false>, dim3(nblk), dim3(PG_SHADE_BLOCK), 0, s, sc, rp, st, sss, qnext, qshadow, qmis, lightTriTests, st.qs[nxt], vs, 0, (float4 *)nullptr);
}

// ===========================================================================
// Film: one lane per pixel of the batch's tiles; samples are added in sample
// order so a pixel's sum is the reference's (integrator.cpp:276-325).
// ===========================================================================
// WEIGHTED: the realistic camera's frames -- AddSample(pFilm, L, rayWeight) with the sample's weight from the LensFrame: (L * sampleWeight) * filterWeight
// (film.h:121-161); the luminance clamp acts on L before it.  The other cameras' weight is 1 and their kernels do not read one.
template <bool WEIGHTED>
__global__ __launch_bounds__(PG_BLOCK) void k_film(RenderParams rp, PathState st, PgFilmPixel *film, PgStraySample *strays, int maxStrays,
                                                    int *nStrays) {
    const int tileInBatch = blockIdx.x;
    const int pix = threadIdx.x;
    const PgRenderDesc &rd = rp.rd;
    int px, py, sn;
    const int slot0 = (tileInBatch * rp.sCount) * 256 + pix;
    if (!slot_to_pixel(rp, slot0, px, py, sn)) return;
    const int local = rp.tileLocal0 + tileInBatch;
    const FilmTileBounds tile = film_tile_bounds(rd, rp.nTilesX, local);
    const float frx = rd.filter_radius[0], fry = rd.filter_radius[1];
    PgFilmPixel *fp = &film[(size_t)local * 256 + pix];
    float r = fp->rgb[0], g = fp->rgb[1], b = fp->rgb[2], w = fp->weight;
    for (int sIdx = 0; sIdx < rp.sCount; ++sIdx) {
        const int slot = (tileInBatch * rp.sCount + sIdx) * 256 + pix;
        const float4 L4 = st.L[slot];
        const float pFilmX = L4.w, pFilmY = st.beta[slot].w;
        const Spec L = film_sample_radiance(rd, sp3(L4.x, L4.y, L4.z));
        const float dx = pFilmX - 0.5f, dy = pFilmY - 0.5f;
        int p0x, p0y, p1x, p1y;
        film_footprint(dx, dy, frx, fry, tile, p0x, p0y, p1x, p1y);
        const Spec c = film_contribution(L, film_sample_weight<WEIGHTED>(st, slot), 1.f);  // box filter => every filterTable entry is 1
        for (int y = p0y; y < p1y; ++y)
            for (int x = p0x; x < p1x; ++x) {
                if (x == px && y == py) { r += c.r; g += c.g; b += c.b; w += 1.f; }
                else film_stray_append(strays, maxStrays, nStrays, x, y, px, py, c);
            }
    }
    fp->rgb[0] = r; fp->rgb[1] = g; fp->rgb[2] = b; fp->weight = w;
}
// ---------------------------------------------------------------------------------------------------------------
// Film for every other pixel filter (gaussian, mitchell, sinc, triangle, wide box): FilmTile::AddSample with the 16x16
// filter table (film.h:121-161).  A sample now lands in every pixel within the filter radius, including pixels owned by
// neighbouring tiles, so a tile's block is its FilmTile pixel bounds (16 + halo), and the kernel GATHERS: one lane per
// block pixel walks the tile's samples in the reference's order (pixels row-major, samples in order) and adds those whose
// footprint covers it.  Deterministic, no atomics, and a pixel's tile-local sum has the reference's summation order;
// the host merges the overlapping blocks in tile order (Film::MergeFilmTile).  All samples of a tile are in one batch.
template <bool WEIGHTED>
__global__ __launch_bounds__(PG_BLOCK) void k_film_general(RenderParams rp, PathState st, PgFilmPixel *film) {
    const int tileInBatch = blockIdx.x;
    const PgRenderDesc &rd = rp.rd;
    const int local = rp.tileLocal0 + tileInBatch;
    const FilmTileBounds tile = film_tile_bounds(rd, rp.nTilesX, local);
    const FilmBlock blk = film_block(rd, tile);
    const int x0 = tile.x0, y0 = tile.y0, x1 = tile.x1, y1 = tile.y1;
    const float frx = rd.filter_radius[0], fry = rd.filter_radius[1];
    const float invRx = 1 / frx, invRy = 1 / fry;  // FilmTile::invFilterRadius, film.h:113
    // source pixels that can reach a pixel: a sample of pixel p has pFilmDiscrete in [p - 0.5, p + 0.5] and covers the pixels
    // ceil(d - r) .. floor(d + r); one more than floor(0.5 + r) against the rounding of those sums -- which a radius <= 0.5 (the box
    // filter on this path: frames whose film positions can round onto the next pixel) cannot need: p + 0.5 + r <= p + 1 is exact
    const int reachX = frx <= 0.5f ? 1 : (int)floorf(0.5f + frx) + 1, reachY = fry <= 0.5f ? 1 : (int)floorf(0.5f + fry) + 1;
    // Radius <= 0.5 (the box filter): almost every sample stays in its own pixel.  Each source pixel's samples are looked at once
    // first -- does one of them cover a pixel besides its own? --, and the gather below visits the samples of OTHER pixels only
    // where that is so (the frame of config 3 at 68 spp: 6.45 ms of film kernel for nine source pixels per pixel)
    __shared__ unsigned char s_reaches[256];
    const bool narrow = frx <= 0.5f && fry <= 0.5f;
    if (narrow) {
        for (int pix = threadIdx.x; pix < 256; pix += PG_BLOCK) {
            const int px = x0 + (pix & 15), py = y0 + (pix >> 4);
            bool reaches = false;
            if (px < x1 && py < y1 && !(px < rd.pixel_bounds[0] || px >= rd.pixel_bounds[2] || py < rd.pixel_bounds[1] || py >= rd.pixel_bounds[3]))
                for (int sIdx = 0; sIdx < rp.sCount && !reaches; ++sIdx) {
                    const int slot = (tileInBatch * rp.sCount + sIdx) * 256 + pix;
                    const float dx = st.L[slot].w - 0.5f, dy = st.beta[slot].w - 0.5f;  // pFilmDiscrete
                    int p0x, p0y, p1x, p1y;
                    film_footprint(dx, dy, frx, fry, tile, p0x, p0y, p1x, p1y);
                    reaches = p0x < px || p1x > px + 1 || p0y < py || p1y > py + 1;
                }
            s_reaches[pix] = reaches ? 1 : 0;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < rd.tile_pixels; e += PG_BLOCK) {
        const int X = blk.bx0 + e % blk.tw, Y = blk.by0 + e / blk.tw;
        if (X < tile.tp0x || X >= tile.tp1x || Y < tile.tp0y || Y >= tile.tp1y) continue;
        float r = 0, g = 0, b = 0, w = 0;
        for (int py = max(y0, Y - reachY); py <= min(y1 - 1, Y + reachY); ++py)
            for (int px = max(x0, X - reachX); px <= min(x1 - 1, X + reachX); ++px) {
                // InsideExclusive(pixel, pixelBounds), integrator.cpp:273
                if (px < rd.pixel_bounds[0] || px >= rd.pixel_bounds[2] || py < rd.pixel_bounds[1] || py >= rd.pixel_bounds[3]) continue;
                const int pix = (py - y0) * 16 + (px - x0);
                if (narrow && !(px == X && py == Y) && !s_reaches[pix]) continue;  // none of that pixel's samples leaves it
                for (int sIdx = 0; sIdx < rp.sCount; ++sIdx) {
                    const int slot = (tileInBatch * rp.sCount + sIdx) * 256 + pix;
                    const float4 L4 = st.L[slot];
                    const float dx = L4.w - 0.5f, dy = st.beta[slot].w - 0.5f;  // pFilmDiscrete
                    int p0, p1;
                    film_footprint_axis(dx, frx, tile.tp0x, tile.tp1x, p0, p1);
                    if (X < p0 || X >= p1) continue;
                    film_footprint_axis(dy, fry, tile.tp0y, tile.tp1y, p0, p1);
                    if (Y < p0 || Y >= p1) continue;
                    const Spec L = film_sample_radiance(rd, sp3(L4.x, L4.y, L4.z));
                    const float fw = film_filter_weight(rd, X, Y, dx, dy, invRx, invRy);
                    const Spec c = film_contribution(L, film_sample_weight<WEIGHTED>(st, slot), fw);
                    r += c.r; g += c.g; b += c.b; w += fw;
                }
            }
        PgFilmPixel *fp = &film[(size_t)local * rd.tile_pixels + e];
        fp->rgb[0] = r; fp->rgb[1] = g; fp->rgb[2] = b; fp->weight = w;
    }
}
// Tile-serial samplers: the one finished sample of every tile, added to the tile's film block exactly as FilmTile::AddSample
// does it (film.h:121-161) -- one lane per tile walks the sample's footprint, so a block's sums have the reference's order.
template <bool WEIGHTED>
__global__ void k_ts_film(DScene sc, RenderParams rp, PathState st, PgFilmPixel *film, PgStraySample *strays, int maxStrays, int *nStrays) {
    const int local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= rp.nTilesBatch || !sc.ts[local].active) return;
    const PgRenderDesc &rd = rp.rd;
    const int px = sc.ts[local].px, py = sc.ts[local].py;
    const FilmTileBounds tile = film_tile_bounds(rd, rp.nTilesX, local);
    const float frx = rd.filter_radius[0], fry = rd.filter_radius[1];
    const float4 L4 = st.L[local];
    const float pFilmX = L4.w, pFilmY = st.beta[local].w;
    const Spec L = film_sample_radiance(rd, sp3(L4.x, L4.y, L4.z));
    const float dx = pFilmX - 0.5f, dy = pFilmY - 0.5f;
    int p0x, p0y, p1x, p1y;
    film_footprint(dx, dy, frx, fry, tile, p0x, p0y, p1x, p1y);
    const float sampleWeight = film_sample_weight<WEIGHTED>(st, local);
    if (rd.filter_general) {
        const FilmBlock blk = film_block(rd, tile);
        const float invRx = 1 / frx, invRy = 1 / fry;
        for (int y = p0y; y < p1y; ++y)
            for (int x = p0x; x < p1x; ++x) {
                const float fw = film_filter_weight(rd, x, y, dx, dy, invRx, invRy);
                const Spec c = film_contribution(L, sampleWeight, fw);
                PgFilmPixel *fp = &film[(size_t)local * rd.tile_pixels + (size_t)(y - blk.by0) * blk.tw + (x - blk.bx0)];
                fp->rgb[0] += c.r; fp->rgb[1] += c.g; fp->rgb[2] += c.b; fp->weight += fw;
            }
        return;
    }
    const Spec c = film_contribution(L, sampleWeight, 1.f);
    for (int y = p0y; y < p1y; ++y)
        for (int x = p0x; x < p1x; ++x) {
            if (x == px && y == py) {
                PgFilmPixel *fp = &film[(size_t)local * 256 + (py - tile.y0) * 16 + (px - tile.x0)];
                fp->rgb[0] += c.r; fp->rgb[1] += c.g; fp->rgb[2] += c.b; fp->weight += 1.f;
            } else film_stray_append(strays, maxStrays, nStrays, x, y, px, py, c);
        }
}
void launch_ts_film(const DScene &sc, const RenderParams &rp, PathState st, PgFilmPixel *film, PgStraySample *strays, int maxStrays, int *nStrays,
                    hipStream_t s) {
    if (rp.rd->camera_type == 3) hipLaunchKernelGGL(k_ts_film<true>, dim3((rp.nTilesBatch + 63) / 64), dim3(64), 0, s, sc, rp, st, film, strays, maxStrays, nStrays);
    else hipLaunchKernelGGL(k_ts_film<false>, dim3((rp.nTilesBatch + 63) / 64), dim3(64), 0, s, sc, rp, st, film, strays, maxStrays, nStrays);
}
void launch_film_general(const RenderParams &rp, PathState st, PgFilmPixel *film, hipStream_t s) {
    if (rp.nTilesBatch == 0) return;
    if (rp.rd->camera_type == 3) hipLaunchKernelGGL(k_film_general<true>, dim3(rp.nTilesBatch), dim3(PG_BLOCK), 0, s, rp, st, film);
    else hipLaunchKernelGGL(k_film_general<false>, dim3(rp.nTilesBatch), dim3(PG_BLOCK), 0, s, rp, st, film);
}
void launch_film(const RenderParams &rp, PathState st, PgFilmPixel *film, PgStraySample *strays, int maxStrays, int *nStrays,
                 hipStream_t s) {
    if (rp.nTilesBatch == 0) return;
    if (rp.rd->camera_type == 3) hipLaunchKernelGGL(k_film<true>, dim3(rp.nTilesBatch), dim3(PG_BLOCK), 0, s, rp, st, film, strays, maxStrays, nStrays);
    else hipLaunchKernelGGL(k_film<false>, dim3(rp.nTilesBatch), dim3(PG_BLOCK), 0, s, rp, st, film, strays, maxStrays, nStrays);
}

// ===========================================================================
// SpatialLightDistribution::ComputeDistribution for every voxel up front
// (lightdistrib.cpp:232-300).  The reference fills voxels lazily through a
// hash table; the distribution is a pure function of the voxel, so a dense
// table holds the same values.  One lane per voxel.
// ===========================================================================
__global__ __launch_bounds__(PG_BLOCK) void k_light_tables(DScene sc, float *table, int nDistributions) {
    const int v = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (v >= nDistributions) return;
    const int nl = sc.nLights;
    float *func = table + (size_t)v * (2 * nl + 2), *cdf = func + nl;
    V3 vmin, vmax;
    voxel_bounds(sc.nVoxels, sc.bmin, sc.bmax, v, vmin, vmax);
    for (int j = 0; j < nl; ++j) func[j] = 0;
    for (int i = 0; i < PG_VOXEL_SAMPLES; ++i) {
        const VoxelSample s = voxel_sample(vmin, vmax, i);
        for (int j = 0; j < nl; ++j) voxel_light_contribution(sc, sc.lights[j], s, func[j]);
    }
    distribution_finish(func, cdf, nl, PG_VOXEL_SAMPLES);
}
// The same for a list of voxels, one BLOCK per voxel (sparse tables: few voxels, possibly thousands of lights): the lights are
// spread over the block's threads -- func[j] is a sum over the 128 sample points in order, independent of the other lights --
// and one thread then runs the reference's sequential sums over the lights (sumContrib, the cdf).
__global__ __launch_bounds__(PG_BLOCK) void k_light_tables_sparse(DScene sc, float *pool, const int *requests, int firstSlot) {
    const int v = requests[blockIdx.x];
    const int nl = sc.nLights;
    float *func = pool + (size_t)(firstSlot + (int)blockIdx.x) * (2 * nl + 2), *cdf = func + nl;
    V3 vmin, vmax;
    voxel_bounds(sc.nVoxels, sc.bmin, sc.bmax, v, vmin, vmax);
    for (int j = threadIdx.x; j < nl; j += PG_BLOCK) {
        float f = 0;
        for (int i = 0; i < PG_VOXEL_SAMPLES; ++i) voxel_light_contribution(sc, sc.lights[j], voxel_sample(vmin, vmax, i), f);
        func[j] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        distribution_finish(func, cdf, nl, PG_VOXEL_SAMPLES);
        sc.voxelSlot[v] = firstSlot + (int)blockIdx.x;  // published at the end of the launch (kernel boundary)
    }
}
void launch_light_tables_sparse(const DScene &sc, float *pool, const int *requests, int n, int firstSlot, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_light_tables_sparse, dim3(n), dim3(PG_BLOCK), 0, s, sc, pool, requests, firstSlot);
}
void launch_light_tables(const DScene &sc, float *table, int nDistributions, hipStream_t s) {
    int nblk = (nDistributions + PG_BLOCK - 1) / PG_BLOCK;
    hipLaunchKernelGGL(k_light_tables, dim3(nblk), dim3(PG_BLOCK), 0, s, sc, table, nDistributions);
}

#include "pg_direct.h"  // the kernels of the DirectLightingIntegrator, built from the pieces above
#include "pg_interaction.h"  // the kernels of the ray queries with per-ray time (pg_intersect_at / pg_intersect_p_at)
#include "pg_scatter.h"  // the kernel of the scattering queries (pg_scatter_f_at / pg_scatter_sample_at)
#include "pg_lightquery.h"  // the kernels of the light queries (pg_light_sample_at / pg_light_pdf_at / pg_light_le_at)
#include "pg_mediumquery.h"  // the kernels of the medium queries (pg_transmittance_at / pg_intersect_tr_at / pg_medium_sample_at)
#include "pg_subsurfacequery.h"  // the kernels of the subsurface queries (pg_subsurface_sample_at / pg_subsurface_f_at / pg_subsurface_sample_f_at)
#include "pg_cameraquery.h"  // the kernels of the camera queries (pg_camera_rays_at / pg_scatter_f_diff_at / pg_scatter_sample_diff_at)
#include "pg_cameraimportance.h"  // camera importance and TransportMode::Importance (pg_camera_we_at / pg_camera_sample_wi_at / pg_scatter_*_mode_at)
