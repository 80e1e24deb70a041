// TEST INFRASTRUCTURE: pbrt-v3_amd/csrc/pg_medium.h compiled for the HOST (hipcc --cuda-host-only, -ffp-contract=off), the way
// tests/device_headers_host.hip compiles the device library, for the functions the medium queries added to it:
// tests/test_medium_headers_on_host.py compares them with a float32 NumPy restatement.  Nothing here is linked into the product.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
__host__ inline unsigned int __float_as_uint(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }
__host__ inline float __uint_as_float(unsigned int u) { float f; memcpy(&f, &u, 4); return f; }
__host__ inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
__host__ inline float __int_as_float(int u) { float f; memcpy(&f, &u, 4); return f; }
__host__ inline bool isinf(float v) { return __builtin_isinf(v); }
__host__ inline bool isnan(float v) { return __builtin_isnan(v); }
__host__ inline unsigned long long __brevll(unsigned long long v) { return __builtin_bitreverse64(v); }
#undef __device__
#define __device__ __attribute__((device)) __attribute__((host))
#include "../pbrt-v3_amd/csrc/pg_device.h"
#include "../pbrt-v3_amd/csrc/pg_medium.h"

extern "C" {
// HomogeneousMedium::Sample from its two numbers on: in = sigma_a[3], sigma_s[3], sigma_t[3], g (a PgMedium), then uChannel, uDist, |d|, tMax;
// out = beta[3], t, sampled (0 / 1), channel, dist
void hostdev_homogeneous_sample(const float *in, float *out) {
    PgMedium mm;
    memcpy(&mm, in, sizeof(mm));
    int channel;
    float dist, t;
    bool inMedium;
    homogeneous_sample_distance(mm, in[10], in[11], channel, dist);
    const Spec beta = homogeneous_sample_weight(mm, dist, in[12], in[13], t, inMedium);
    out[0] = beta.r; out[1] = beta.g; out[2] = beta.b; out[3] = t; out[4] = inMedium ? 1.f : 0.f; out[5] = (float)channel; out[6] = dist;
}
// the same with the distance given (dist may be chosen to land on tMax * |d| exactly)
void hostdev_homogeneous_weight(const float *in, float dist, float *out) {
    PgMedium mm;
    memcpy(&mm, in, sizeof(mm));
    float t;
    bool inMedium;
    const Spec beta = homogeneous_sample_weight(mm, dist, in[12], in[13], t, inMedium);
    out[0] = beta.r; out[1] = beta.g; out[2] = beta.b; out[3] = t; out[4] = inMedium ? 1.f : 0.f;
}
}
