// pg_sampler.h -- the samplers as device functions: HaltonSampler's and SobolSampler's sample index and values (halton_*, sobol_*;
// the batched halton_batch stays in pg_kernels.hip), and the tile-stream PixelSamplers (random / stratified / 02sequence / maxmindist: rng_*, ts_*, tsb_*).
//
// Used by k_generate, k_ts_*, k_shade and the other kernels of pg_kernels.hip that draw numbers.  halton_index is pinned on the host
// (tests/test_device_headers_on_host.py) and on the device (tests/test_gpu_device_arithmetic.py).
#ifndef PG_SAMPLER_H
#define PG_SAMPLER_H
#include "pg_device.h"
#include "pg_kernels.h"

// ===========================================================================
// Sampler
// ===========================================================================
PG_DEV uint64_t inverse_radical_inverse(uint32_t base, uint64_t inverse, int nDigits) {  // lowdiscrepancy.h:80-91
    uint64_t index = 0;
    for (int i = 0; i < nDigits; ++i) {
        uint64_t digit = inverse % base;
        inverse /= base;
        index = index * base + digit;
    }
    return index;
}
PG_DEV int pmod(int a, int b) { int r = a - (a / b) * b; return (r < 0) ? r + b : r; }  // pbrt.h:314-317

// HaltonSampler::GetIndexForSample, halton.cpp:96-117
PG_DEV uint64_t halton_index(const PgRenderDesc &rd, int px, int py, uint64_t sampleNum) {
    uint64_t offsetForCurrentPixel = 0;
    if (rd.sample_stride > 1) {
        int pm0 = pmod(px, 128), pm1 = pmod(py, 128);
        uint64_t dimOffset0 = inverse_radical_inverse(2, pm0, rd.base_exponents[0]);
        uint64_t dimOffset1 = inverse_radical_inverse(3, pm1, rd.base_exponents[1]);
        offsetForCurrentPixel += dimOffset0 * (uint64_t)(rd.sample_stride / rd.base_scales[0]) * (uint64_t)rd.mult_inverse[0];
        offsetForCurrentPixel += dimOffset1 * (uint64_t)(rd.sample_stride / rd.base_scales[1]) * (uint64_t)rd.mult_inverse[1];
        offsetForCurrentPixel %= (uint64_t)rd.sample_stride;
    }
    return offsetForCurrentPixel + sampleNum * (uint64_t)rd.sample_stride;
}
// HaltonSampler::SampleDimension, halton.cpp:119-127
// SobolSampler (samplers/sobol.cpp:41-59): SobolIntervalToIndex and SobolSampleFloat, lowdiscrepancy.h:229-273
PG_DEV uint64_t sobol_interval_to_index(const DScene &sc, uint32_t m, uint64_t frame, int px, int py) {
    if (m == 0) return 0;
    const uint32_t m2 = m << 1;
    uint64_t index = frame << m2;
    uint64_t delta = 0;
    for (int c = 0; frame; frame >>= 1, ++c)
        if (frame & 1) delta ^= sc.vdcSobol[(m - 1) * 52 + c];
    uint64_t b = (((uint64_t)((uint32_t)px) << m) | ((uint32_t)py)) ^ delta;
    for (int c = 0; b; b >>= 1, ++c)
        if (b & 1) index ^= sc.vdcSobolInv[(m - 1) * 52 + c];
    return index;
}
PG_DEV float sobol_sample(const DScene &sc, uint64_t a, int dim) {
    if (dim > 1023) dim = 1023;  // NumSobolDimensions; the reference aborts beyond (sobol.cpp:47-50)
    uint32_t v = 0;
    for (int i = dim * 52; a != 0; a >>= 1, i++)
        if (a & 1) v ^= sc.sobolMatrices[i];
    return pmin(v * 0x1p-32f, PG_ONE_MINUS_EPS);
}
// GlobalSampler::GetIndexForSample of the configured sampler (halton.cpp:96-117, sobol.cpp:41-44)
PG_DEV uint64_t sampler_index(const DScene &sc, const PgRenderDesc &rd, int px, int py, uint64_t sampleNum) {
    if (rd.sampler == 1) return sobol_interval_to_index(sc, (uint32_t)rd.sobol_log2_resolution, sampleNum, px - rd.sample_bounds[0], py - rd.sample_bounds[1]);
    return halton_index(rd, px, py, sampleNum);
}
// SampleDimension of the configured sampler for any dimension >= 2 (dimensions 0 and 1, the film position, are drawn by
// k_generate alone: SobolSampler remaps them with the current pixel, sobol.cpp:53-56)
PG_DEV float halton_sample(const DScene &sc, const PgRenderDesc &rd, uint64_t index, int dim) {
    if (rd.sampler == 1) return sobol_sample(sc, index, dim);
    if (rd.sample_at_pixel_center && (dim == 0 || dim == 1)) return 0.5f;
    if (dim == 0) return radical_inverse_base2(index >> rd.base_exponents[0]);
    if (dim == 1) return radical_inverse(3, index / (uint64_t)rd.base_scales[1]);
    if (dim >= sc.nPermDims) dim = sc.nPermDims - 1;  // host sizes the table from maxdepth; halton.h:71-76 aborts here
    if ((index >> 32) != 0) return scrambled_radical_inverse((uint32_t)sc.primes[dim], sc.perms + sc.permSums[dim], index);
    // 32-bit index: scrambled_radical_inverse's loop with the division done by multiplication (DScene::haltonDims)
    const int4 hd = sc.haltonDims[2 * dim], hc = sc.haltonDims[2 * dim + 1];
    const uint32_t base = (uint32_t)hd.x, mul = (uint32_t)hd.z, sh = (uint32_t)hd.w - 1u;
    const uint16_t *perm = sc.perms + hd.y;
    const float invBase = __int_as_float(hc.x);  // 1.f / (float)base
    uint64_t reversedDigits = 0;
    float invBaseN = 1;
    uint32_t a32 = (uint32_t)index;
    while (a32) {
        const uint32_t t = __umulhi(mul, a32);
        const uint32_t next = (t + ((a32 - t) >> 1)) >> sh;
        reversedDigits = reversedDigits * base + perm[a32 - next * base];
        invBaseN *= invBase;
        a32 = next;
    }
    return pmin(invBaseN * ((float)reversedDigits + __int_as_float(hc.y) /* invBase * perm[0] / (1 - invBase) */), PG_ONE_MINUS_EPS);
}

// ---- the samplers that draw from one RNG stream per tile (RandomSampler; the PixelSamplers, sampler.cpp:100-134) ------------
PG_DEV uint32_t rng_u32(TileSamplerState &t) {  // RNG::UniformUInt32, rng.h:137-143
    const unsigned long long oldstate = t.state;
    ++t.draws;
    t.state = oldstate * 0x5851f42d4c957f2dULL + t.inc;
    const uint32_t xorshifted = (uint32_t)(((oldstate >> 18u) ^ oldstate) >> 27u);
    const uint32_t rot = (uint32_t)(oldstate >> 59u);
    return (xorshifted >> rot) | (xorshifted << ((~rot + 1u) & 31));
}
// the state after `delta` more UniformUInt32 calls (each is one step of the 64-bit LCG): O(log delta), as PCG's advance()
PG_DEV void rng_advance(TileSamplerState &t, unsigned long long delta) {
    unsigned long long accMult = 1, accPlus = 0, curMult = 0x5851f42d4c957f2dULL, curPlus = t.inc;
    for (; delta > 0; delta >>= 1) {
        if (delta & 1) { accMult *= curMult; accPlus = accPlus * curMult + curPlus; }
        curPlus = (curMult + 1) * curPlus;
        curMult *= curMult;
    }
    t.state = accMult * t.state + accPlus;
}
PG_DEV uint32_t rng_u32b(TileSamplerState &t, uint32_t b) {  // rng.h:68-74
    const uint32_t threshold = (~b + 1u) % b;
    for (;;) { const uint32_t r = rng_u32(t); if (r >= threshold) return r % b; }
}
PG_DEV float rng_float(TileSamplerState &t) { return pmin(PG_ONE_MINUS_EPS, (float)rng_u32(t) * 0x1p-32f); }  // rng.h:75-82
PG_DEV float ts_get1d(const DScene &sc, int tile) {  // PixelSampler::Get1D (RandomSampler: tsDims = 0)
    TileSamplerState &t = sc.ts[tile];
    if (t.cur1D < sc.tsDims) return sc.ts1[((size_t)tile * sc.tsDims + t.cur1D++) * sc.tsSpp + t.sampleIndex];
    return rng_float(t);
}
PG_DEV void ts_get2d(const DScene &sc, int kind, int tile, float &a, float &b) {  // PixelSampler::Get2D
    TileSamplerState &t = sc.ts[tile];
    if (t.cur2D < sc.tsDims) {
        const float *p = sc.ts2 + (((size_t)tile * sc.tsDims + t.cur2D++) * sc.tsSpp + t.sampleIndex) * 2;
        a = p[0]; b = p[1];
    } else if (kind == PG_SAMPLER_RANDOM) { a = rng_float(t); b = rng_float(t); }  // random.cpp:50-54: braced list, left to right
    else { b = rng_float(t); a = rng_float(t); }  // `Point2f(rng.UniformFloat(), rng.UniformFloat())` as the reference build (g++) evaluates it: y first
}
// tsBatched (DScene): PixelSampler::Get1D / Get2D of sample `sample` of pixel `pixel`; dim = current2DDimension << 6 | current1DDimension
PG_DEV float tsb_get1d(const DScene &sc, int pixel, int sample, int &dim) {
    const int c = dim & 63;
    if (c >= sc.tsDims) { atomicOr(sc.tsOverflow, 1); return 0.5f; }
    dim += 1;
    return sc.ts1[((size_t)pixel * sc.tsDims + c) * sc.tsSpp + sample];
}
PG_DEV void tsb_get2d(const DScene &sc, int pixel, int sample, int &dim, float &a, float &b) {
    const int c = dim >> 6;
    if (c >= sc.tsDims) { atomicOr(sc.tsOverflow, 1); a = b = 0.5f; return; }
    dim += 64;
    const float *p = sc.ts2 + (((size_t)pixel * sc.tsDims + c) * sc.tsSpp + sample) * 2;
    a = p[0]; b = p[1];
}
PG_DEV void ts_shuffle(float *samp, int count, int width, TileSamplerState &t) {  // Shuffle, sampling.h:151-157
    for (int i = 0; i < count; ++i) {
        const int other = i + (int)rng_u32b(t, (uint32_t)(count - i));
        for (int j = 0; j < width; ++j) { const float v = samp[width * i + j]; samp[width * i + j] = samp[width * other + j]; samp[width * other + j] = v; }
    }
}
PG_DEV void ts_van_der_corput(int n, float *samples, TileSamplerState &t) {  // VanDerCorput(1, n, ...), lowdiscrepancy.h:154-207
    uint32_t v = rng_u32(t);
    for (uint32_t i = 0; i < (uint32_t)n; ++i) {  // GrayCodeSample, C[k] = 1 << (31 - k)
        samples[i] = pmin((float)v * 0x1p-32f, PG_ONE_MINUS_EPS);
        v ^= 0x80000000u >> __builtin_ctz(i + 1);
    }
    for (int i = 0; i < n; ++i) ts_shuffle(samples + i, 1, 1, t);  // a one-element shuffle still draws a number
    ts_shuffle(samples, n, 1, t);
}
PG_DEV void ts_sobol2d(int n, float *samples, TileSamplerState &t) {  // Sobol2D(1, n, ...), lowdiscrepancy.h:209-236
    uint32_t v0 = rng_u32(t), v1 = rng_u32(t);
    for (uint32_t i = 0; i < (uint32_t)n; ++i) {
        samples[2 * i] = pmin((float)v0 * 0x1p-32f, PG_ONE_MINUS_EPS);
        samples[2 * i + 1] = pmin((float)v1 * 0x1p-32f, PG_ONE_MINUS_EPS);
        const int k = __builtin_ctz(i + 1);
        v0 ^= 0x80000000u >> k;
        uint32_t c = 0x80000000u;  // CSobol[1][k]: c_0 = 2^31, c_j = c_(j-1) ^ (c_(j-1) >> 1)
        for (int j = 0; j < k; ++j) c ^= c >> 1;
        v1 ^= c;
    }
    for (int i = 0; i < n; ++i) ts_shuffle(samples + 2 * i, 1, 2, t);
    ts_shuffle(samples, n, 2, t);
}
// a tile's global index, pixel (lx, ly) of it and whether that pixel exists (tiles at the image edge are clipped)
PG_DEV bool ts_tile_pixel(const RenderParams &rp, int local, int lx, int ly, int &t, int &px, int &py) {
    t = rp.rd->tile_first + local * rp.rd->tile_step;
    const int tx = t % rp.nTilesX, ty = t / rp.nTilesX;
    px = rp.rd->sample_bounds[0] + tx * 16 + lx;
    py = rp.rd->sample_bounds[1] + ty * 16 + ly;
    return px < rp.rd->sample_bounds[2] && py < rp.rd->sample_bounds[3];
}
// <Sampler>::StartPixel for pixel (lx, ly) of every tile: the pixel's sample arrays from the tile's stream -- also for pixels
// outside the integrator's pixel bounds, which are then skipped (integrator.cpp:264-273)
PG_DEV void ts_start_pixel(const DScene &sc, const PgRenderDesc &rd, TileSamplerState &t, float *s1, float *s2) {
    {
        const int n = sc.tsSpp, nd = sc.tsDims;
        if (rd.sampler == PG_SAMPLER_STRATIFIED) {  // stratified.cpp:43-70, sampling.cpp:42-60
            const int nx = rd.strat_samples[0], ny = rd.strat_samples[1];
            for (int i = 0; i < nd; ++i) {
                float *p = s1 + (size_t)i * n;
                const float invNSamples = 1.f / (float)n;
                for (int k = 0; k < n; ++k) { const float delta = rd.strat_jitter ? rng_float(t) : 0.5f; p[k] = pmin(((float)k + delta) * invNSamples, PG_ONE_MINUS_EPS); }
                ts_shuffle(p, n, 1, t);
            }
            for (int i = 0; i < nd; ++i) {
                float *p = s2 + (size_t)i * n * 2;
                const float dx = 1.f / (float)nx, dy = 1.f / (float)ny;
                for (int y = 0; y < ny; ++y)
                    for (int x = 0; x < nx; ++x) {
                        const float jx = rd.strat_jitter ? rng_float(t) : 0.5f;
                        const float jy = rd.strat_jitter ? rng_float(t) : 0.5f;
                        p[2 * (y * nx + x)] = pmin(((float)x + jx) * dx, PG_ONE_MINUS_EPS);
                        p[2 * (y * nx + x) + 1] = pmin(((float)y + jy) * dy, PG_ONE_MINUS_EPS);
                    }
                ts_shuffle(p, n, 2, t);
            }
        } else if (rd.sampler == PG_SAMPLER_ZEROTWO) {  // zerotwosequence.cpp:53-69
            for (int i = 0; i < nd; ++i) ts_van_der_corput(n, s1 + (size_t)i * n, t);
            for (int i = 0; i < nd; ++i) ts_sobol2d(n, s2 + (size_t)i * n * 2, t);
        } else if (rd.sampler == PG_SAMPLER_MAXMINDIST) {  // maxmin.cpp:43-69
            int cIndex = 0;
            while ((1 << (cIndex + 1)) <= n) ++cIndex;  // Log2Int(samplesPerPixel)
            const uint32_t *CPixel = sc.cmaxmin + 32 * cIndex;
            const float invSPP = 1.f / (float)n;
            for (int i = 0; i < n; ++i) {
                uint32_t v = 0, a = (uint32_t)i;
                for (int k = 0; a != 0; ++k, a >>= 1) if (a & 1) v ^= CPixel[k];  // MultiplyGenerator, lowdiscrepancy.h:93-98
                s2[2 * i] = (float)i * invSPP;
                s2[2 * i + 1] = pmin((float)v * 0x1p-32f, PG_ONE_MINUS_EPS);
            }
            ts_shuffle(s2, n, 2, t);
            for (int i = 0; i < nd; ++i) ts_van_der_corput(n, s1 + (size_t)i * n, t);
            for (int i = 1; i < nd; ++i) ts_sobol2d(n, s2 + (size_t)i * n * 2, t);
        }  // RandomSampler::StartPixel only fills requested sample arrays: none
    }
}

// Russian roulette on a path's next ray (path.cpp:176-184, volpath.cpp:178-184): whether the path survives, its beta divided by 1 - q when it does.
// `bounces` is the reference loop's count at this vertex; a number is drawn (draw1) only when the test asks for one.
template <class Draw>
PG_DEV bool russian_roulette(Spec &beta, float etaScale, int bounces, float rrThreshold, Draw &&draw1) {
    const Spec rrBeta = beta * etaScale;
    if (max_component(rrBeta) < rrThreshold && bounces > 3) {
        const float q = pmax(.05f, 1 - max_component(rrBeta));
        if (draw1() < q) return false;
        beta = beta / (1 - q);
    }
    return true;
}

#endif  // PG_SAMPLER_H
