// TEST INFRASTRUCTURE: the device arithmetic headers of the product run ON the MI355X, one lane per input -- libpg_devprobe.so, built by
// pbrt-v3_amd/Makefile with exactly the product's GPUFLAGS, loaded only by tests/test_gpu_device_arithmetic.py, which compares what it returns bit
// for bit with the host build of the same source (tests/libm_pin.cpp, tests/device_headers_host.hip: the builds the non-GPU tests pin to glibc
// and to the oracle).  Every entry point takes host pointers, does its own allocation / copies / launch / synchronize / free and returns 0 or
// the hipError_t that stopped it (devprobe_error_string).  Nothing here is linked into libpbrt_gpu.so.  The device library of the shading
// kernels (pg_bxdf.h, pg_medium.h, pg_sampler.h, pg_camera.h) is within reach like every other header: csrc/pg_kernels.hip holds kernels, their
// launchers and a few helpers only kernels call, so no kernel of the product is compiled a second time here.
#include "../pbrt-v3_amd/csrc/pg_device.h"
#include "../pbrt-v3_amd/csrc/pg_sphere.h"
#include "../pbrt-v3_amd/csrc/pg_grid.h"
#include "../pbrt-v3_amd/csrc/pg_bssrdf.h"
#include "../pbrt-v3_amd/csrc/pg_motion.h"
#include "../pbrt-v3_amd/csrc/pg_sampler.h"
#include "../pbrt-v3_amd/csrc/pg_camera.h"
#include "../pbrt-v3_amd/csrc/pg_bxdf.h"
#include "../pbrt-v3_amd/csrc/pg_medium.h"
#include "../pbrt-v3_amd/csrc/pg_resolve.h"
#include "../pbrt-v3_amd/csrc/pg_film.h"
#include "../pbrt-v3_amd/csrc/pg_lightdistrib.h"
#include "libm_chunk.h"
#include "scatter_probe.h"
#include "film_probe.h"
#include "resolve_probe.h"
#include <vector>

#define DP_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)
namespace {
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
struct In { const void *host; size_t bytes; };
struct Out { void *host; size_t bytes; };
// uploads the inputs, allocates the outputs, launch(d) with d = the device pointers (inputs first), synchronizes, downloads the outputs
template <class Launch> int run(const std::vector<In> &in, const std::vector<Out> &out, Launch launch) {
    std::vector<DevBuf> buf(in.size() + out.size());
    std::vector<void *> d(buf.size(), nullptr);
    for (size_t k = 0; k < buf.size(); ++k) {
        const size_t bytes = k < in.size() ? in[k].bytes : out[k - in.size()].bytes;
        if (!bytes) continue;
        DP_TRY(hipMalloc(&buf[k].p, bytes));
        d[k] = buf[k].p;
        if (k < in.size()) DP_TRY(hipMemcpy(d[k], in[k].host, bytes, hipMemcpyHostToDevice));
        else DP_TRY(hipMemset(d[k], 0, bytes));
    }
    launch(d.data());
    DP_TRY(hipGetLastError());
    DP_TRY(hipDeviceSynchronize());
    for (size_t k = 0; k < out.size(); ++k)
        if (out[k].bytes && out[k].host) DP_TRY(hipMemcpy(out[k].host, d[in.size() + k], out[k].bytes, hipMemcpyDeviceToHost));
    return 0;
}
constexpr int LANES = 64;  // threads per block of the batched probes
dim3 blocks(int n) { return dim3((unsigned)((n + LANES - 1) / LANES)); }
template <class T> const T *as(void *p) { return (const T *)p; }
#define DP_LANE() const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return
__device__ V3 v3at(const float *p, int i) { return mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

// ---- pg_libm.h ---------------------------------------------------------------------------------------------------------------------
// function FN (libm_chunk.h) at index i: the results' bits in r, returns the hash term -- tests/libm_pin.cpp's term() for the device
template <int FN> __device__ uint64_t libm_term(uint32_t i, uint32_t r[2]) {
    const float x = pgm_asfloat(i);
    float a = 0, b = 0;
    if (FN == 0) a = pg_sinf(x);
    else if (FN == 1) a = pg_cosf(x);
    else if (FN == 2) pg_sincosf(x, &a, &b);
    else if (FN == 3) a = pg_logf(x);
    else if (FN == 4) a = pg_expf(x);
    else if (FN == 5) a = pg_acosf(x);
    else if (FN == 6) a = pg_atanf(x);
    else {
        uint32_t uy, ux;
        lc_atan2_pair(1, i, 0, &uy, &ux);
        a = pg_atan2f(pgm_asfloat(uy), pgm_asfloat(ux));
    }
    r[0] = pgm_asuint(a); r[1] = pgm_asuint(b);
    return FN == 2 ? lc_term2(i, a, b) : lc_term1(i, a);
}
constexpr int SWEEP_THREADS = 256;
// one block per chunk: every thread sums its share of the 2^22 terms, the block reduces in LDS, thread 0 stores the chunk's sum
template <int FN> __global__ __launch_bounds__(SWEEP_THREADS) void k_libm_sums(uint32_t firstChunk, uint64_t *sums) {
    __shared__ uint64_t part[SWEEP_THREADS];
    const uint32_t first = (firstChunk + blockIdx.x) << LC_CHUNK_BITS;
    uint64_t s = 0;
    for (uint32_t j = threadIdx.x; j < (1u << LC_CHUNK_BITS); j += SWEEP_THREADS) {
        uint32_t r[2];
        s += libm_term<FN>(first + j, r);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = SWEEP_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}
template <int FN> __global__ void k_libm_raw(int special, uint32_t first, uint32_t n, uint32_t *out0, uint32_t *out1) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r[2] = {0, 0};
    if (FN == LC_ATAN2F && special) {
        uint32_t uy, ux;
        lc_atan2_pair(1, first + i, 1, &uy, &ux);
        r[0] = pgm_asuint(pg_atan2f(pgm_asfloat(uy), pgm_asfloat(ux)));
    } else libm_term<FN>(first + i, r);
    out0[i] = r[0]; out1[i] = r[1];
}
template <int FN> void launch_sums(uint32_t firstChunk, uint32_t nChunks, void **d) {
    hipLaunchKernelGGL(k_libm_sums<FN>, dim3(nChunks), dim3(SWEEP_THREADS), 0, 0, firstChunk, (uint64_t *)d[0]);
}
template <int FN> void launch_raw(int special, uint32_t first, uint32_t n, void **d) {
    hipLaunchKernelGGL(k_libm_raw<FN>, dim3((n + 255) / 256), dim3(256), 0, 0, special, first, n, (uint32_t *)d[0], (uint32_t *)d[1]);
}
#define DP_EACH_FN(call) switch (fn) { case 0: call(0); break; case 1: call(1); break; case 2: call(2); break; case 3: call(3); break; \
                                       case 4: call(4); break; case 5: call(5); break; case 6: call(6); break; default: call(7); break; }

// ---- pg_device.h, pg_sphere.h ------------------------------------------------------------------------------------------------------
__global__ void k_tri_test(int n, const float *p0, const float *p1, const float *p2, const float *o, const float *d, const float *tMax, float *out, int *hit) {
    DP_LANE();
    float t = 0, b0 = 0, b1 = 0, b2 = 0;
    hit[i] = tri_test(v3at(p0, i), v3at(p1, i), v3at(p2, i), v3at(o, i), v3at(d, i), tMax[i], t, b0, b1, b2) ? 1 : 0;
    out[4 * i] = t; out[4 * i + 1] = b0; out[4 * i + 2] = b1; out[4 * i + 3] = b2;
}
__global__ void k_quadric_test(int n, const PgSphere *sp, const float *o, const float *d, const float *tMax, float *tHit, int *hit) {
    DP_LANE();
    float t = 0;
    hit[i] = sphere_test(sp[i], v3at(o, i), v3at(d, i), tMax[i], t) ? 1 : 0;
    tHit[i] = t;
}
__global__ void k_offset_ray_origin(int n, const float *p, const float *pError, const float *nrm, const float *w, float *out) {
    DP_LANE();
    const V3 r = offset_ray_origin(v3at(p, i), v3at(pError, i), v3at(nrm, i), v3at(w, i));
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}
__global__ void k_radical_inverse(int n, const uint32_t *base, const uint64_t *a, float *out) {
    DP_LANE();
    out[i] = base[i] == 2 ? radical_inverse_base2(a[i]) : radical_inverse(base[i], a[i]);
}
__global__ void k_scrambled_radical_inverse(int n, const uint32_t *base, const uint16_t *perms, const uint32_t *permOffset, const uint64_t *a, float *out) {
    DP_LANE();
    out[i] = scrambled_radical_inverse(base[i], perms + permOffset[i], a[i]);
}
__global__ void k_concentric_sample_disk(int n, const float *u0, const float *u1, float *out) {
    DP_LANE();
    concentric_sample_disk(u0[i], u1[i], out[2 * i], out[2 * i + 1]);
}
// ---- pg_grid.h: lane i draws from draws[i * nDraws ...] (0.5 beyond its end), used[i] = draws consumed ------------------------------------
struct DrawStream { const float *u; int n, used; PG_DEV float operator()() { const float v = used < n ? u[used] : 0.5f; ++used; return v; } };
__global__ void k_grid_density(int n, const PgDensityGrid *g, const float *den, const float *p, float *out) {
    DP_LANE();
    out[i] = grid_density(*g, den, v3at(p, i));
}
__global__ void k_grid_tr(int n, const PgDensityGrid *g, const float *den, const float *o, const float *d, const float *tMax, const float *draws, int nDraws, int *used, float *out) {
    DP_LANE();
    DrawStream ds{draws + (size_t)i * nDraws, nDraws, 0};
    out[i] = grid_tr(*g, den, v3at(o, i), v3at(d, i), tMax[i], ds);
    used[i] = ds.used;
}
__global__ void k_grid_sample(int n, const PgDensityGrid *g, const float *den, const float *o, const float *d, const float *tMax, const float *draws, int nDraws, int *used, float *t,
                              int *hit) {
    DP_LANE();
    DrawStream ds{draws + (size_t)i * nDraws, nDraws, 0};
    float tt = 0;
    const bool h = grid_sample(*g, den, v3at(o, i), v3at(d, i), tMax[i], ds, tt);
    used[i] = ds.used; t[i] = h ? tt : 0.f; hit[i] = h ? 1 : 0;
}
// ---- pg_bssrdf.h -------------------------------------------------------------------------------------------------------------------
__global__ void k_bssrdf_radial(int n, const PgBSSRDF *bs, const float *tables, const float *r, const float *u, float *out) {
    DP_LANE();
    const DBssrdf b = bssrdf_bind(*bs, tables);
    const Spec sr = bssrdf_sr(b, r[i]);
    out[9 * i] = sr.r; out[9 * i + 1] = sr.g; out[9 * i + 2] = sr.b;
    for (int c = 0; c < 3; ++c) { out[9 * i + 3 + c] = bssrdf_pdf_sr(b, c, r[i]); out[9 * i + 6 + c] = bssrdf_sample_sr(b, c, u[i]); }
}
__global__ void k_fresnel_moment1(int n, const float *eta, float *out) {
    DP_LANE();
    out[i] = fresnel_moment1(eta[i]);
}
__global__ void k_invert_catmull_rom(int n, int nNodes, const float *x, const float *values, const float *u, float *out) {
    DP_LANE();
    out[i] = invert_catmull_rom(nNodes, x, values, u[i]);
}
__global__ void k_bssrdf_pdf_sp(int n, const PgBSSRDF *bs, const float *tables, const float *frame, const float *po, const float *pi, const float *nrm, float *out) {
    DP_LANE();
    out[i] = bssrdf_pdf_sp(bssrdf_bind(*bs, tables), v3at(frame, 3 * i), v3at(frame, 3 * i + 1), v3at(frame, 3 * i + 2), v3at(po, i), v3at(pi, i), v3at(nrm, i));
}
__global__ void k_bssrdf_probe_segment(int n, const PgBSSRDF *bs, const float *tables, const float *frame, const float *po, const float *u1, const float *u2x, const float *u2y,
                                       float *out, int *ok) {
    DP_LANE();
    V3 base = mk(0, 0, 0), target = mk(0, 0, 0);
    float u = u1[i];
    ok[i] = bssrdf_probe_segment(bssrdf_bind(*bs, tables), v3at(frame, 3 * i), v3at(frame, 3 * i + 1), v3at(frame, 3 * i + 2), v3at(po, i), u, u2x[i], u2y[i], base, target) ? 1 : 0;
    float *q = out + 7 * i;
    q[0] = u; q[1] = base.x; q[2] = base.y; q[3] = base.z; q[4] = target.x; q[5] = target.y; q[6] = target.z;
}
// ---- pg_motion.h -------------------------------------------------------------------------------------------------------------------
template <bool INV> __global__ void k_interpolate_trs(int n, const float *T, const float *R, const float *S, const float *dt, float *m, float *mInv) {
    DP_LANE();
    float a[16], b[16];
    for (int k = 0; k < 16; ++k) a[k] = b[k] = 0.f;
    interpolate_trs<INV>((const float(*)[3])(T + 6 * i), (const float(*)[4])(R + 8 * i), (const float(*)[9])(S + 18 * i), dt[i], a, b);
    for (int k = 0; k < 16; ++k) { m[16 * i + k] = a[k]; mInv[16 * i + k] = b[k]; }
}
// ---- pg_bxdf.h: the wrappers of tests/device_headers_host.hip, a lane each (a disagreement among the forms of one evaluation comes back as NaNs) ----
__device__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
__global__ void k_lobe_f_pdf(int n, const PgBxDF *lobes, const float *wo, const float *wi, float *out) {
    DP_LANE();
    const PgBxDF &b = lobes[i];
    const V3 o = v3at(wo, i), w = v3at(wi, i);
    Spec f, fOnly, fNone;
    float pdf, pdfOnly, pdfNone;
    lobe_f_pdf(b, b.type, o, w, true, true, f, pdf);
    lobe_f_pdf(b, b.type, o, w, true, false, fOnly, pdfNone);
    lobe_f_pdf(b, b.type, o, w, false, true, fNone, pdfOnly);
    const Spec fs = lobe_f(b, b.type, o, w);
    const float ps = lobe_pdf(b, b.type, o, w);
    float *q = out + 4 * i;
    q[0] = f.r; q[1] = f.g; q[2] = f.b; q[3] = pdf;
    const bool ok = same_bits(f.r, fOnly.r) && same_bits(f.g, fOnly.g) && same_bits(f.b, fOnly.b) && same_bits(pdf, pdfOnly) &&
                    same_bits(f.r, fs.r) && same_bits(f.g, fs.g) && same_bits(f.b, fs.b) && same_bits(pdf, ps) &&
                    pdfNone == 0 && fNone.r == 0 && fNone.g == 0 && fNone.b == 0;
    if (!ok) q[0] = q[1] = q[2] = q[3] = __builtin_nanf("");
}
__global__ void k_lobe_sample_f(int n, const PgBxDF *lobes, const float *wo, const float *u0, const float *u1, float *out, int *type) {
    DP_LANE();
    const PgBxDF &b = lobes[i];
    V3 wi = mk(0, 0, 0), wi2 = mk(0, 0, 0);
    float pdf = 0, pdf2 = 0;
    int sampledType = lobe_type(b.type), sampledType2 = sampledType;
    const Spec f = lobe_sample_f(b, b.type, v3at(wo, i), wi, u0[i], u1[i], pdf, sampledType);
    lobe_sample_f(b, b.type, v3at(wo, i), wi2, u0[i], u1[i], pdf2, sampledType2, false);
    float *q = out + 7 * i;
    q[0] = f.r; q[1] = f.g; q[2] = f.b; q[3] = pdf; q[4] = wi.x; q[5] = wi.y; q[6] = wi.z;
    if (!(same_bits(pdf, pdf2) && same_bits(wi.x, wi2.x) && same_bits(wi.y, wi2.y) && same_bits(wi.z, wi2.z) && sampledType == sampledType2)) q[3] = __builtin_nanf("");
    type[i] = sampledType;
}
// ---- pg_medium.h, pg_sampler.h, pg_camera.h ----------------------------------------------------------------------------------------------
__global__ void k_henyey_greenstein(int n, const float *g, const float *wo, const float *u, const float *cosTheta, float *p, float *wi, float *phase) {
    DP_LANE();
    V3 w = mk(0, 0, 0);
    p[i] = hg_sample_p(g[i], v3at(wo, i), w, u[2 * i], u[2 * i + 1]);
    wi[3 * i] = w.x; wi[3 * i + 1] = w.y; wi[3 * i + 2] = w.z;
    phase[i] = phase_hg(cosTheta[i], g[i]);
}
__global__ void k_halton_index(int n, const PgRenderDesc *rd, const int *px, const int *py, const long long *sampleNum, long long *out) {
    DP_LANE();
    out[i] = (long long)halton_index(*rd, px[i], py[i], (uint64_t)sampleNum[i]);
}
__global__ void k_camera_ray(int n, const PgRenderDesc *rd, const float *fx, const float *fy, const float *lx, const float *ly, float *out) {
    DP_LANE();
    V3 o, d;
    float tMax;
    camera_ray(*rd, rd->camera_to_world, fx[i], fy[i], lx[i], ly[i], o, d, tMax);
    float *q = out + 7 * i;
    q[0] = o.x; q[1] = o.y; q[2] = o.z; q[3] = d.x; q[4] = d.y; q[5] = d.z; q[6] = tMax;
}
// ---- the scattering models of EstimateDirect's set-up beyond the BxDF lists, and the roulette (scatter_probe.h) -------------------------------
__global__ void k_adapter_bsdf(int n, const float *in, const int *flags, float *out) {
    DP_LANE();
    probe_adapter_bsdf(in + SCATTER_ADAPTER_IN * i, flags[i], out + SCATTER_ADAPTER_OUT * i);
}
__global__ void k_hg_phase(int n, const float *in, float *out) {
    DP_LANE();
    probe_hg_phase(in + SCATTER_HG_IN * i, out + SCATTER_HG_OUT * i);
}
__global__ void k_russian_roulette(int n, const float *in, const int *bounces, float *out) {
    DP_LANE();
    probe_russian_roulette(in + SCATTER_RR_IN * i, bounces[i], out + SCATTER_RR_OUT * i);
}
// ---- the film kernels' AddSample pieces (pg_film.h) and the light-table kernels' ComputeDistribution pieces (pg_lightdistrib.h): film_probe.h ----
__global__ void k_film_tile(int n, const PgRenderDesc *rd, int nTilesX, const int *local, const float *pFilm, int *out) {
    DP_LANE();
    probe_film_tile(*rd, nTilesX, local[i], pFilm + 2 * i, out + FILM_TILE_OUT * i);
}
__global__ void k_film_radiance(int n, const PgRenderDesc *rds, const int *which, const float *in, float *out) {
    DP_LANE();
    probe_film_radiance(rds[which[i]], in + FILM_RADIANCE_IN * i, out + FILM_RADIANCE_OUT * i);
}
__global__ void k_film_filter_weight(int n, const PgRenderDesc *rd, const int *xy, const float *in, float *out) {
    DP_LANE();
    out[i] = probe_film_filter_weight(*rd, xy[2 * i], xy[2 * i + 1], in + FILM_WEIGHT_IN * i);
}
// ---- EstimateDirect's pending terms and sums (pg_resolve.h): resolve_probe.h ---------------------------------------------------------------
__global__ void k_resolve_path(int n, const float *in, const int *iin, float *out, int *iout) {
    DP_LANE();
    probe_resolve_path(in + RESOLVE_PATH_IN * i, iin + RESOLVE_PATH_IIN * i, out + RESOLVE_PATH_OUT * i, iout + RESOLVE_PATH_IOUT * i);
}
__global__ void k_resolve_vol_probe(int n, const float *in, const int *iin, float *out) {
    DP_LANE();
    probe_resolve_vol(in + RESOLVE_VOL_IN * i, iin + RESOLVE_VOL_IIN * i, out + RESOLVE_VOL_OUT * i);
}
__global__ void k_direct_fold_probe(int n, const float *in, float *out) {
    DP_LANE();
    probe_direct_fold(in + RESOLVE_FOLD_IN * i, out + 4 * i);
}
__global__ void k_resolve_roundtrip(int n, const float *in, const int *iin, float *out, int *iout) {
    DP_LANE();
    probe_resolve_roundtrip(in + RESOLVE_RT_IN * i, iin + RESOLVE_RT_IIN * i, out + RESOLVE_RT_OUT * i, iout + RESOLVE_RT_IOUT * i);
}
__global__ void k_voxel(int n, const int *nVoxels, const float *bmin, const float *bmax, const int *v, const int *sample, float *out) {
    DP_LANE();
    probe_voxel(nVoxels, bmin, bmax, v[i], sample[i], out + VOXEL_OUT * i);
}
// lane i's table: 2 nl[i] + 2 floats from offset[i], copied from `in` (lightContrib in front) and finished in `out`
__global__ void k_distribution_finish(int n, const float *in, const int *offset, const int *nl, int nSamples, float *out) {
    DP_LANE();
    float *table = out + offset[i];
    for (int k = 0; k < 2 * nl[i] + 2; ++k) table[k] = in[offset[i] + k];
    probe_distribution_finish(table, nl[i], nSamples);
}
}  // namespace

#define F(k) as<float>(d[k])
#define FB(count) ((size_t)(count) * sizeof(float))
extern "C" {
const char *devprobe_error_string(int status) { return hipGetErrorString((hipError_t)status); }

// sums[k] = the sum of chunk firstChunk + k of function fn (libm_chunk.h), k < nChunks
int devprobe_libm_chunk_sums(int fn, uint32_t firstChunk, uint32_t nChunks, uint64_t *sums) {
    if (fn < 0 || fn >= LC_NUM_FN || firstChunk > LC_NUM_CHUNKS || nChunks > LC_NUM_CHUNKS - firstChunk) return (int)hipErrorInvalidValue;
    if (!nChunks) return 0;
#define CALL(FN) launch_sums<FN>(firstChunk, nChunks, d)
    return run({}, {{sums, nChunks * sizeof(uint64_t)}}, [&](void **d) { DP_EACH_FN(CALL) });
#undef CALL
}
// the result bits at the indices first .. first + count - 1 (out1: sincosf's cosine, may be null); atan2f with `special`: its edge grid
int devprobe_libm_raw(int fn, int special, uint32_t first, uint32_t count, uint32_t *out0, uint32_t *out1) {
    if (fn < 0 || fn >= LC_NUM_FN || count > (1u << 26)) return (int)hipErrorInvalidValue;
    if (!count) return 0;
#define CALL(FN) launch_raw<FN>(special, first, count, d)
    return run({}, {{out0, count * sizeof(uint32_t)}, {out1, count * sizeof(uint32_t)}}, [&](void **d) { DP_EACH_FN(CALL) });
#undef CALL
}

// The batched forms of tests/device_headers_host.hip's wrappers: a leading count n, every per-call argument an array of n.
int devprobe_tri_test(int n, const float *p0, const float *p1, const float *p2, const float *o, const float *dir, const float *tMax, float *out, int *hit) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{p0, FB(3 * n)}, {p1, FB(3 * n)}, {p2, FB(3 * n)}, {o, FB(3 * n)}, {dir, FB(3 * n)}, {tMax, FB(n)}}, {{out, FB(4 * n)}, {hit, n * sizeof(int)}},
               [&](void **d) { hipLaunchKernelGGL(k_tri_test, blocks(n), dim3(LANES), 0, 0, n, F(0), F(1), F(2), F(3), F(4), F(5), (float *)d[6], (int *)d[7]); });
}
int devprobe_quadric_test(int n, const PgSphere *sp, const float *o, const float *dir, const float *tMax, float *tHit, int *hit) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{sp, (size_t)n * sizeof(PgSphere)}, {o, FB(3 * n)}, {dir, FB(3 * n)}, {tMax, FB(n)}}, {{tHit, FB(n)}, {hit, n * sizeof(int)}},
               [&](void **d) { hipLaunchKernelGGL(k_quadric_test, blocks(n), dim3(LANES), 0, 0, n, as<PgSphere>(d[0]), F(1), F(2), F(3), (float *)d[4], (int *)d[5]); });
}
int devprobe_offset_ray_origin(int n, const float *p, const float *pError, const float *nrm, const float *w, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{p, FB(3 * n)}, {pError, FB(3 * n)}, {nrm, FB(3 * n)}, {w, FB(3 * n)}}, {{out, FB(3 * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_offset_ray_origin, blocks(n), dim3(LANES), 0, 0, n, F(0), F(1), F(2), F(3), (float *)d[4]); });
}
int devprobe_radical_inverse(int n, const uint32_t *base, const uint64_t *a, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{base, n * sizeof(uint32_t)}, {a, n * sizeof(uint64_t)}}, {{out, FB(n)}},
               [&](void **d) { hipLaunchKernelGGL(k_radical_inverse, blocks(n), dim3(LANES), 0, 0, n, as<uint32_t>(d[0]), as<uint64_t>(d[1]), (float *)d[2]); });
}
// lane i's permutation: perms[permOffset[i] ... + base[i]) of the nPerms entries
int devprobe_scrambled_radical_inverse(int n, const uint32_t *base, const uint16_t *perms, int nPerms, const uint32_t *permOffset, const uint64_t *a, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    for (int i = 0; i < n; ++i)
        if (base[i] < 2 || (uint64_t)permOffset[i] + base[i] > (uint64_t)nPerms) return (int)hipErrorInvalidValue;
    return run({{base, n * sizeof(uint32_t)}, {perms, nPerms * sizeof(uint16_t)}, {permOffset, n * sizeof(uint32_t)}, {a, n * sizeof(uint64_t)}}, {{out, FB(n)}}, [&](void **d) {
        hipLaunchKernelGGL(k_scrambled_radical_inverse, blocks(n), dim3(LANES), 0, 0, n, as<uint32_t>(d[0]), as<uint16_t>(d[1]), as<uint32_t>(d[2]), as<uint64_t>(d[3]), (float *)d[4]);
    });
}
int devprobe_concentric_sample_disk(int n, const float *u0, const float *u1, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{u0, FB(n)}, {u1, FB(n)}}, {{out, FB(2 * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_concentric_sample_disk, blocks(n), dim3(LANES), 0, 0, n, F(0), F(1), (float *)d[2]); });
}
// den = the grid's own nx * ny * nz floats (density_offset already applied, as the host wrappers take it)
int devprobe_grid_density(int n, const PgDensityGrid *g, const float *den, const float *p, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{g, sizeof(PgDensityGrid)}, {den, FB((size_t)g->nx * g->ny * g->nz)}, {p, FB(3 * n)}}, {{out, FB(n)}},
               [&](void **d) { hipLaunchKernelGGL(k_grid_density, blocks(n), dim3(LANES), 0, 0, n, as<PgDensityGrid>(d[0]), F(1), F(2), (float *)d[3]); });
}
int devprobe_grid_tr(int n, const PgDensityGrid *g, const float *den, const float *o, const float *dir, const float *tMax, const float *draws, int nDraws, int *used, float *out) {
    if (n <= 0 || nDraws < 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{g, sizeof(PgDensityGrid)}, {den, FB((size_t)g->nx * g->ny * g->nz)}, {o, FB(3 * n)}, {dir, FB(3 * n)}, {tMax, FB(n)}, {draws, FB((size_t)n * nDraws)}},
               {{used, n * sizeof(int)}, {out, FB(n)}}, [&](void **d) {
                   hipLaunchKernelGGL(k_grid_tr, blocks(n), dim3(LANES), 0, 0, n, as<PgDensityGrid>(d[0]), F(1), F(2), F(3), F(4), F(5), nDraws, (int *)d[6], (float *)d[7]);
               });
}
int devprobe_grid_sample(int n, const PgDensityGrid *g, const float *den, const float *o, const float *dir, const float *tMax, const float *draws, int nDraws, int *used, float *t,
                         int *hit) {
    if (n <= 0 || nDraws < 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{g, sizeof(PgDensityGrid)}, {den, FB((size_t)g->nx * g->ny * g->nz)}, {o, FB(3 * n)}, {dir, FB(3 * n)}, {tMax, FB(n)}, {draws, FB((size_t)n * nDraws)}},
               {{used, n * sizeof(int)}, {t, FB(n)}, {hit, n * sizeof(int)}}, [&](void **d) {
                   hipLaunchKernelGGL(k_grid_sample, blocks(n), dim3(LANES), 0, 0, n, as<PgDensityGrid>(d[0]), F(1), F(2), F(3), F(4), F(5), nDraws, (int *)d[6], (float *)d[7], (int *)d[8]);
               });
}
// tables = the scene's nTables floats; bs->table indexes them
int devprobe_bssrdf_radial(int n, const PgBSSRDF *bs, const float *tables, long long nTables, const float *r, const float *u, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{bs, sizeof(PgBSSRDF)}, {tables, FB(nTables)}, {r, FB(n)}, {u, FB(n)}}, {{out, FB(9 * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_bssrdf_radial, blocks(n), dim3(LANES), 0, 0, n, as<PgBSSRDF>(d[0]), F(1), F(2), F(3), (float *)d[4]); });
}
int devprobe_fresnel_moment1(int n, const float *eta, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{eta, FB(n)}}, {{out, FB(n)}}, [&](void **d) { hipLaunchKernelGGL(k_fresnel_moment1, blocks(n), dim3(LANES), 0, 0, n, F(0), (float *)d[1]); });
}
int devprobe_invert_catmull_rom(int n, int nNodes, const float *x, const float *values, const float *u, float *out) {
    if (n <= 0 || nNodes < 2) return n ? (int)hipErrorInvalidValue : 0;
    return run({{x, FB(nNodes)}, {values, FB(nNodes)}, {u, FB(n)}}, {{out, FB(n)}},
               [&](void **d) { hipLaunchKernelGGL(k_invert_catmull_rom, blocks(n), dim3(LANES), 0, 0, n, nNodes, F(0), F(1), F(2), (float *)d[3]); });
}
// frame = ss, ts, ns
int devprobe_bssrdf_pdf_sp(int n, const PgBSSRDF *bs, const float *tables, long long nTables, const float *frame, const float *po, const float *pi, const float *nrm, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{bs, sizeof(PgBSSRDF)}, {tables, FB(nTables)}, {frame, FB(9 * n)}, {po, FB(3 * n)}, {pi, FB(3 * n)}, {nrm, FB(3 * n)}}, {{out, FB(n)}},
               [&](void **d) { hipLaunchKernelGGL(k_bssrdf_pdf_sp, blocks(n), dim3(LANES), 0, 0, n, as<PgBSSRDF>(d[0]), F(1), F(2), F(3), F(4), F(5), (float *)d[6]); });
}
int devprobe_bssrdf_probe_segment(int n, const PgBSSRDF *bs, const float *tables, long long nTables, const float *frame, const float *po, const float *u1, const float *u2x,
                                  const float *u2y, float *out, int *ok) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{bs, sizeof(PgBSSRDF)}, {tables, FB(nTables)}, {frame, FB(9 * n)}, {po, FB(3 * n)}, {u1, FB(n)}, {u2x, FB(n)}, {u2y, FB(n)}}, {{out, FB(7 * n)}, {ok, n * sizeof(int)}},
               [&](void **d) {
                   hipLaunchKernelGGL(k_bssrdf_probe_segment, blocks(n), dim3(LANES), 0, 0, n, as<PgBSSRDF>(d[0]), F(1), F(2), F(3), F(4), F(5), F(6), (float *)d[7], (int *)d[8]);
               });
}
// T: n x 2 x 3, R: n x 2 x 4, S: n x 2 x 9 (PgInstance's); m, mInv: n x 16 -- mInv stays 0 without inv (interpolate_trs<false> does not compute it)
int devprobe_interpolate_trs(int n, int inv, const float *T, const float *R, const float *S, const float *dt, float *m, float *mInv) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{T, FB(6 * n)}, {R, FB(8 * n)}, {S, FB(18 * n)}, {dt, FB(n)}}, {{m, FB(16 * n)}, {mInv, FB(16 * n)}}, [&](void **d) {
        if (inv) hipLaunchKernelGGL(k_interpolate_trs<true>, blocks(n), dim3(LANES), 0, 0, n, F(0), F(1), F(2), F(3), (float *)d[4], (float *)d[5]);
        else hipLaunchKernelGGL(k_interpolate_trs<false>, blocks(n), dim3(LANES), 0, 0, n, F(0), F(1), F(2), F(3), (float *)d[4], (float *)d[5]);
    });
}
// lobes: n PgBxDFs, each evaluated as its own type; out: n x (f rgb, pdf)
int devprobe_lobe_f_pdf(int n, const PgBxDF *lobes, const float *wo, const float *wi, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{lobes, (size_t)n * sizeof(PgBxDF)}, {wo, FB(3 * n)}, {wi, FB(3 * n)}}, {{out, FB(4 * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_lobe_f_pdf, blocks(n), dim3(LANES), 0, 0, n, as<PgBxDF>(d[0]), F(1), F(2), (float *)d[3]); });
}
// out: n x (f rgb, pdf, wi); type: the sampled type
int devprobe_lobe_sample_f(int n, const PgBxDF *lobes, const float *wo, const float *u0, const float *u1, float *out, int *type) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{lobes, (size_t)n * sizeof(PgBxDF)}, {wo, FB(3 * n)}, {u0, FB(n)}, {u1, FB(n)}}, {{out, FB(7 * n)}, {type, n * sizeof(int)}},
               [&](void **d) { hipLaunchKernelGGL(k_lobe_sample_f, blocks(n), dim3(LANES), 0, 0, n, as<PgBxDF>(d[0]), F(1), F(2), F(3), (float *)d[4], (int *)d[5]); });
}
// u: n x 2; p = hg_sample_p's value with its direction wi (n x 3), phase = phase_hg(cosTheta, g)
int devprobe_henyey_greenstein(int n, const float *g, const float *wo, const float *u, const float *cosTheta, float *p, float *wi, float *phase) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{g, FB(n)}, {wo, FB(3 * n)}, {u, FB(2 * n)}, {cosTheta, FB(n)}}, {{p, FB(n)}, {wi, FB(3 * n)}, {phase, FB(n)}},
               [&](void **d) { hipLaunchKernelGGL(k_henyey_greenstein, blocks(n), dim3(LANES), 0, 0, n, F(0), F(1), F(2), F(3), (float *)d[4], (float *)d[5], (float *)d[6]); });
}
int devprobe_halton_index(int n, const PgRenderDesc *rd, const int *px, const int *py, const long long *sampleNum, long long *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{rd, sizeof(PgRenderDesc)}, {px, n * sizeof(int)}, {py, n * sizeof(int)}, {sampleNum, n * sizeof(long long)}}, {{out, n * sizeof(long long)}}, [&](void **d) {
        hipLaunchKernelGGL(k_halton_index, blocks(n), dim3(LANES), 0, 0, n, as<PgRenderDesc>(d[0]), as<int>(d[1]), as<int>(d[2]), as<long long>(d[3]), (long long *)d[4]);
    });
}
// the camera of rd at its start transform (rd->camera_to_world), as tests/device_headers_host.hip's wrapper; out: n x (o, d, tMax)
int devprobe_camera_ray(int n, const PgRenderDesc *rd, const float *fx, const float *fy, const float *lx, const float *ly, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{rd, sizeof(PgRenderDesc)}, {fx, FB(n)}, {fy, FB(n)}, {lx, FB(n)}, {ly, FB(n)}}, {{out, FB(7 * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_camera_ray, blocks(n), dim3(LANES), 0, 0, n, as<PgRenderDesc>(d[0]), F(1), F(2), F(3), F(4), (float *)d[5]); });
}
// scatter_probe.h's three functions, one lane per input: in / out are n rows of its SCATTER_*_IN / _OUT floats
int devprobe_adapter_bsdf(int n, const float *in, const int *flags, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{in, FB(SCATTER_ADAPTER_IN * n)}, {flags, n * sizeof(int)}}, {{out, FB(SCATTER_ADAPTER_OUT * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_adapter_bsdf, blocks(n), dim3(LANES), 0, 0, n, F(0), as<int>(d[1]), (float *)d[2]); });
}
int devprobe_hg_phase(int n, const float *in, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{in, FB(SCATTER_HG_IN * n)}}, {{out, FB(SCATTER_HG_OUT * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_hg_phase, blocks(n), dim3(LANES), 0, 0, n, F(0), (float *)d[1]); });
}
int devprobe_russian_roulette(int n, const float *in, const int *bounces, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{in, FB(SCATTER_RR_IN * n)}, {bounces, n * sizeof(int)}}, {{out, FB(SCATTER_RR_OUT * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_russian_roulette, blocks(n), dim3(LANES), 0, 0, n, F(0), as<int>(d[1]), (float *)d[2]); });
}
// film_probe.h's functions, one lane per input.  film_tile: one description and nTilesX for all lanes, local[n], pFilm n x 2, out n x FILM_TILE_OUT
int devprobe_film_tile(int n, const PgRenderDesc *rd, int nTilesX, const int *local, const float *pFilm, int *out) {
    if (n <= 0 || nTilesX <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{rd, sizeof(PgRenderDesc)}, {local, n * sizeof(int)}, {pFilm, FB(2 * n)}}, {{out, (size_t)n * FILM_TILE_OUT * sizeof(int)}},
               [&](void **d) { hipLaunchKernelGGL(k_film_tile, blocks(n), dim3(LANES), 0, 0, n, as<PgRenderDesc>(d[0]), nTilesX, as<int>(d[1]), F(2), (int *)d[3]); });
}
// lane i takes its clamp from rds[which[i]] (nRds descriptions); in n x FILM_RADIANCE_IN, out n x FILM_RADIANCE_OUT
int devprobe_film_radiance(int n, const PgRenderDesc *rds, int nRds, const int *which, const float *in, float *out) {
    if (n <= 0 || nRds <= 0) return n ? (int)hipErrorInvalidValue : 0;
    for (int i = 0; i < n; ++i)
        if (which[i] < 0 || which[i] >= nRds) return (int)hipErrorInvalidValue;
    return run({{rds, (size_t)nRds * sizeof(PgRenderDesc)}, {which, n * sizeof(int)}, {in, FB(FILM_RADIANCE_IN * n)}}, {{out, FB(FILM_RADIANCE_OUT * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_film_radiance, blocks(n), dim3(LANES), 0, 0, n, as<PgRenderDesc>(d[0]), as<int>(d[1]), F(2), (float *)d[3]); });
}
// xy: n x (X, Y); in: n x FILM_WEIGHT_IN, none of them a NaN (the table index of one is not defined)
int devprobe_film_filter_weight(int n, const PgRenderDesc *rd, const int *xy, const float *in, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    for (int i = 0; i < FILM_WEIGHT_IN * n; ++i)
        if (in[i] != in[i]) return (int)hipErrorInvalidValue;
    return run({{rd, sizeof(PgRenderDesc)}, {xy, 2 * n * sizeof(int)}, {in, FB(FILM_WEIGHT_IN * n)}}, {{out, FB(n)}},
               [&](void **d) { hipLaunchKernelGGL(k_film_filter_weight, blocks(n), dim3(LANES), 0, 0, n, as<PgRenderDesc>(d[0]), as<int>(d[1]), F(2), (float *)d[3]); });
}
// one grid (nVoxels, bmin, bmax: 3 each) for all lanes; lane i: voxel v[i], sample point sample[i]; out n x VOXEL_OUT
int devprobe_voxel(int n, const int *nVoxels, const float *bmin, const float *bmax, const int *v, const int *sample, float *out) {
    if (n <= 0 || nVoxels[0] <= 0 || nVoxels[1] <= 0 || nVoxels[2] <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{nVoxels, 3 * sizeof(int)}, {bmin, FB(3)}, {bmax, FB(3)}, {v, n * sizeof(int)}, {sample, n * sizeof(int)}}, {{out, FB(VOXEL_OUT * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_voxel, blocks(n), dim3(LANES), 0, 0, n, as<int>(d[0]), F(1), F(2), as<int>(d[3]), as<int>(d[4]), (float *)d[5]); });
}
// tables: nFloats floats in and out; lane i's distribution is the 2 nl[i] + 2 floats from offset[i] (lightContrib in front); the tables do not overlap
int devprobe_distribution_finish(int n, const float *tables, int nFloats, const int *offset, const int *nl, int nSamples, float *out) {
    if (n <= 0 || nFloats <= 0) return n ? (int)hipErrorInvalidValue : 0;
    for (int i = 0; i < n; ++i)
        if (nl[i] < 1 || offset[i] < 0 || (long long)offset[i] + 2LL * nl[i] + 2 > nFloats || (i && offset[i] < offset[i - 1] + 2 * nl[i - 1] + 2)) return (int)hipErrorInvalidValue;
    return run({{tables, FB(nFloats)}, {offset, n * sizeof(int)}, {nl, n * sizeof(int)}}, {{out, FB(nFloats)}},
               [&](void **d) { hipLaunchKernelGGL(k_distribution_finish, blocks(n), dim3(LANES), 0, 0, n, F(0), as<int>(d[1]), as<int>(d[2]), nSamples, (float *)d[3]); });
}
// resolve_probe.h's functions, one lane per input: in / iin / out / iout are n rows of its RESOLVE_*_IN / _IIN / _OUT / _IOUT words.  The positions a row
// names index the probe's own two-entry arrays: anything else is refused here
static bool resolve_where_ok(int where) { return where >= -2 && where <= 1; }
int devprobe_resolve_path(int n, const float *in, const int *iin, float *out, int *iout) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    for (int i = 0; i < n; ++i)
        if (!resolve_where_ok(iin[RESOLVE_PATH_IIN * i + 3])) return (int)hipErrorInvalidValue;
    return run({{in, FB(RESOLVE_PATH_IN * n)}, {iin, RESOLVE_PATH_IIN * n * sizeof(int)}}, {{out, FB(RESOLVE_PATH_OUT * n)}, {iout, RESOLVE_PATH_IOUT * n * sizeof(int)}},
               [&](void **d) { hipLaunchKernelGGL(k_resolve_path, blocks(n), dim3(LANES), 0, 0, n, F(0), as<int>(d[1]), (float *)d[2], (int *)d[3]); });
}
int devprobe_resolve_vol(int n, const float *in, const int *iin, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    for (int i = 0; i < n; ++i) {
        const int *r = iin + RESOLVE_VOL_IIN * i;
        if (r[4] ? !resolve_where_ok(r[3]) : (r[5] < 0 || r[5] > 1)) return (int)hipErrorInvalidValue;
    }
    return run({{in, FB(RESOLVE_VOL_IN * n)}, {iin, RESOLVE_VOL_IIN * n * sizeof(int)}}, {{out, FB(RESOLVE_VOL_OUT * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_resolve_vol_probe, blocks(n), dim3(LANES), 0, 0, n, F(0), as<int>(d[1]), (float *)d[2]); });
}
int devprobe_direct_fold(int n, const float *in, float *out) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    return run({{in, FB(RESOLVE_FOLD_IN * n)}}, {{out, FB(4 * n)}},
               [&](void **d) { hipLaunchKernelGGL(k_direct_fold_probe, blocks(n), dim3(LANES), 0, 0, n, F(0), (float *)d[1]); });
}
int devprobe_resolve_roundtrip(int n, const float *in, const int *iin, float *out, int *iout) {
    if (n <= 0) return n ? (int)hipErrorInvalidValue : 0;
    for (int i = 0; i < n; ++i) {
        const int *r = iin + RESOLVE_RT_IIN * i;
        if (r[4] < 0 || r[4] > 1 || r[5] < 0 || r[5] > 1) return (int)hipErrorInvalidValue;
    }
    return run({{in, FB(RESOLVE_RT_IN * n)}, {iin, RESOLVE_RT_IIN * n * sizeof(int)}}, {{out, FB(RESOLVE_RT_OUT * n)}, {iout, RESOLVE_RT_IOUT * n * sizeof(int)}},
               [&](void **d) { hipLaunchKernelGGL(k_resolve_roundtrip, blocks(n), dim3(LANES), 0, 0, n, F(0), as<int>(d[1]), (float *)d[2], (int *)d[3]); });
}
}
