// TEST INFRASTRUCTURE: what tests/libm_pin.cpp (host build of pg_libm.h, system libm) and tests/device_probe.hip (gfx950 build of
// pg_libm.h) must agree on to compare a 2^32-argument sweep through 1024 sums -- the NaN rule, the hash of an (argument, result)
// pair, the atan2f pair of an index, the chunking.  Sums are modulo 2^64, so any order of adding gives the same sum.
#ifndef LIBM_CHUNK_H
#define LIBM_CHUNK_H
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LC_FN __host__ __device__ inline
#else
#define LC_FN static inline
#endif

// fn: 0 sinf 1 cosf 2 sincosf 3 logf 4 expf 5 acosf 6 atanf 7 atan2f (seed 1, not special)
#define LC_NUM_FN 8
#define LC_ATAN2F 7
// a chunk = 2^22 consecutive argument bit patterns (atan2f: pair indices), numbered by the top 10 bits
#define LC_CHUNK_BITS 22
#define LC_NUM_CHUNKS 1024
#define LC_ATAN2_NUM_EDGE 22

LC_FN uint32_t lc_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
// any NaN -> the default quiet NaN; everything else, signed zeros included, as it is
LC_FN uint32_t lc_canon(float f) { const uint32_t u = lc_bits(f); return (u & 0x7fffffff) > 0x7f800000 ? 0x7fc00000u : u; }
// splitmix64's finaliser over (argument << 32 | result); slot tells the outputs of one call apart (sincosf: 0 sine, 1 cosine)
LC_FN uint64_t lc_mix(uint32_t arg, uint32_t result, uint32_t slot) {
    uint64_t z = ((uint64_t)arg << 32 | result) + ((uint64_t)slot + 1) * 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
LC_FN uint64_t lc_term1(uint32_t arg, float r) { return lc_mix(arg, lc_canon(r), 0); }
LC_FN uint64_t lc_term2(uint32_t arg, float s, float c) { return lc_mix(arg, lc_canon(s), 0) + lc_mix(arg, lc_canon(c), 1); }

// The atan2f arguments of index i: pseudo-random pairs of bit patterns (a 64-bit LCG per index, seeded), every exponent and sign
// reached; with `special`, both arguments are drawn from a small set of edge values (zeros, infinities, NaN, 1, subnormals, huge ratios)
LC_FN void lc_atan2_pair(uint64_t seed, uint64_t i, int special, uint32_t *py, uint32_t *px) {
    const uint32_t edge[LC_ATAN2_NUM_EDGE] = {0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x3f800000, 0xbf800000, 0x00000001, 0x80000001, 0x007fffff, 0x00800000,
                                              0x7f7fffff, 0xff7fffff, 0x5e800000, 0x1e800000, 0x3f000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000, 0x31000000};
    const int nEdge = LC_ATAN2_NUM_EDGE;
    uint64_t s = (seed + i) * 6364136223846793005ULL + 1442695040888963407ULL;
    s ^= s >> 29; s *= 0xbf58476d1ce4e5b9ULL; s ^= s >> 32;
    uint32_t uy = (uint32_t)s, ux = (uint32_t)(s >> 32);
    if (special) { uy = edge[(i / nEdge) % nEdge]; ux = edge[i % nEdge]; }
    else if ((i & 3) == 1) ux = (ux & 0x807fffff) | (uy & 0x7f800000);                         // same exponent: ratios near 1
    else if ((i & 3) == 2) ux = (ux & 0x807fffff) | (((uy >> 23) + (uint32_t)(s >> 60)) & 0xff) << 23;  // exponents within 16
    *py = uy; *px = ux;
}
#endif
