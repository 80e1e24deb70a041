// pg_queue.h -- what the wavefront kernels share about their SoA ray queues: block sizes, the per-block aggregated queue append
// (block_push) with the octant it bins by (dir_octant), the entry a thread consumes (queue_item, shade_position), the times of the rays a vertex
// spawned (store_ray_times) and the wave-wide statistics counters (flush_light_tests, stats_*).
//
// Used by every kernel of pg_kernels.hip and pg_direct.h.  Device functions only: no kernel and no launcher lives in a header.
#ifndef PG_QUEUE_H
#define PG_QUEUE_H
#include "pg_device.h"
#include "pg_kernels.h"

#define PG_BLOCK 256
// threads per block of the shading kernel: its blocks meet at two barriers around the queue append, so a block is only as fast
// as its slowest wave -- measured on the GPU
#ifndef PG_SHADE_BLOCK
#define PG_SHADE_BLOCK 128
#endif
PG_DEV int lane_id() { return __lane_id(); }

// Queue append, aggregated per block: every wave ballots its pushes, the block sums them through LDS and ONE lane per
// queue does the atomicAdd on the block's region counter (region = blockIdx.x % 8); lanes get consecutive entries in
// (wave, lane) order.  NQ queues are appended to in one exchange (two barriers).  Must be reached by all threads.
// Consumers and producers share one mapping: block b owns entries [(b>>3)*256, +256) of region b & 7.
// With BINNED, queue 0's entries are additionally grouped by `bin0` (0..7) inside the block's range: k_shade bins the next
// bounce's rays by direction octant, so the 64 consecutive rays a traversal wave picks up come from one tile AND mostly
// one octant (same near/far child order, same subtrees) instead of four to eight.
template <int NQ, bool BINNED, int BLOCK = PG_BLOCK>
PG_DEV void block_push(const RayQueue *q, const bool *pred, int *pos, int bin0 = 0) {
    constexpr int NW = BLOCK / 64;
    __shared__ int s_cnt[NQ][NW];
    __shared__ int s_base[NQ];
    __shared__ int s_bin[BINNED ? 8 : 1][NW];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    unsigned long long mask[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        mask[k] = __ballot(pred[k]);
        if (lane == 0) s_cnt[k][wave] = __popcll(mask[k]);
    }
    unsigned long long binMask = 0;
    if (BINNED) {
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot(pred[0] && bin0 == b);
            if (lane == 0) s_bin[b][wave] = __popcll(m);
            if (bin0 == b) binMask = m;
        }
    }
    __syncthreads();
    // lanes 0 .. NQ-1 reserve the NQ queues' entries with ONE atomic instruction (one round trip to the counters instead of
    // NQ dependent ones); the queue's fields are picked by compare-and-select on named copies so that they stay in registers
    if (threadIdx.x < NQ) {
        const int k = threadIdx.x;
        int total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) total += s_cnt[k][w];
        static_assert(NQ <= 4, "block_push: at most four queues");
        int *const c0 = q[0].counts, *const c1 = q[NQ > 1 ? 1 : 0].counts, *const c2 = q[NQ > 2 ? 2 : 0].counts, *const c3 = q[NQ > 3 ? 3 : 0].counts;
        const int cap0 = q[0].regionCap, cap1 = q[NQ > 1 ? 1 : 0].regionCap, cap2 = q[NQ > 2 ? 2 : 0].regionCap, cap3 = q[NQ > 3 ? 3 : 0].regionCap;
        int *const cnt = k == 0 ? c0 : (k == 1 ? c1 : (k == 2 ? c2 : c3));
        const int cap = k == 0 ? cap0 : (k == 1 ? cap1 : (k == 2 ? cap2 : cap3));
        const int r = blockIdx.x & (PG_REGIONS - 1);
        s_base[k] = total ? r * cap + atomicAdd(&cnt[r * PG_COUNT_STRIDE], total) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        int off = s_base[k];
        if (BINNED && k == 0) {
            for (int b = 0; b < 8; ++b)
                for (int w = 0; w < NW; ++w)
                    if (b < bin0 || (b == bin0 && w < wave)) off += s_bin[b][w];
            pos[k] = pred[k] ? off + __popcll(binMask & ((1ull << lane) - 1ull)) : -1;
        } else {
            for (int w = 0; w < wave; ++w) off += s_cnt[k][w];
            pos[k] = pred[k] ? off + __popcll(mask[k] & ((1ull << lane) - 1ull)) : -1;
        }
    }
}
// The queue entry this thread consumes (or -1): block b walks region b & 7.
template <int BLOCK = PG_BLOCK>
PG_DEV int queue_item(const RayQueue &q) {
    const int r = blockIdx.x & (PG_REGIONS - 1);
    const int j = (blockIdx.x >> 3) * BLOCK + threadIdx.x;
    return j < q.counts[r * PG_COUNT_STRIDE] ? r * q.regionCap + j : -1;
}

// block_push's bin of a continuation ray: the octant of its direction
PG_DEV int dir_octant(V3 wi) { return (wi.x < 0 ? 1 : 0) | (wi.y < 0 ? 2 : 0) | (wi.z < 0 ? 4 : 0); }
// Scenes with moving shapes / instances: the rays a vertex spawned (next, shadow, MIS: outQ[k] at pos[k] where pushed[k]) carry the interaction's time
// = the time of the ray that found it, entry i of qsrc (interaction.h:77-95)
PG_DEV void store_ray_times(const DScene &sc, const RayQueue &qsrc, int i, const RayQueue *outQ, const bool *pushed, const int *pos) {
    if (!sc.rayTimes) return;
    const float t = i >= 0 ? PG_QUEUE_TIMES(sc, qsrc)[i] : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (pushed[k]) PG_QUEUE_TIMES(sc, outQ[k])[pos[k]] = t;
}

// A shading thread's POSITION in its launch's order (the index queue_item gave it, before RenderParams::order maps it to an entry; a
// retry launch reads it back from the retry list): recomputed from the block and thread indices where it is needed, not kept in a register.
PG_DEV int shade_position(const RenderParams &rp, const RayQueue &q) {
    if (rp.retryCount > 0) return rp.retryList[blockIdx.x * PG_SHADE_BLOCK + threadIdx.x];
    return (blockIdx.x & (PG_REGIONS - 1)) * q.regionCap + (blockIdx.x >> 3) * PG_SHADE_BLOCK + threadIdx.x;
}

PG_DEV unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// the wave's count of Shape::Pdf triangle tests (mis_light_pdf) to the block's shard of the counters: every lane of the block calls it
PG_DEV void flush_light_tests(unsigned long long *shards, unsigned int n) {
    const unsigned long long nl = wave_sum(n);
    if (lane_id() == 0 && nl) atomicAdd(shards + (blockIdx.x & (PG_LIGHT_TEST_SHARDS - 1)) * PG_LIGHT_TEST_STRIDE, nl);
}
// ReportValue(pathLength, bounces) of the Li calls that end in this wave (path.cpp:186, volpath.cpp:187): every lane of the block calls it
PG_DEV void stats_path_end(unsigned long long *shards, bool ended, int len) {
    const unsigned long long m = __ballot(ended);
    if (m == 0) return;
    const unsigned long long sum = wave_sum(ended ? (unsigned long long)len : 0ull);
    int mn = ended ? len : 0xffff, mx = ended ? len : -1;
    for (int off = 32; off > 0; off >>= 1) { const int a = __shfl_down(mn, off), b = __shfl_down(mx, off); mn = a < mn ? a : mn; mx = b > mx ? b : mx; }
    if (lane_id() == 0) {
        unsigned long long *sh = shards + (blockIdx.x & (PG_LIGHT_TEST_SHARDS - 1)) * PG_LIGHT_TEST_STRIDE;
        atomicAdd(sh + PG_STAT_LEN_SUM, sum); atomicAdd(sh + PG_STAT_LEN_COUNT, (unsigned long long)__popcll(m));
        atomicMax(sh + PG_STAT_LEN_MINC, (unsigned long long)(0xffff - mn)); atomicMax(sh + PG_STAT_LEN_MAXP, (unsigned long long)(mx + 1));
    }
}
// a counter of the same shards raised by the number of lanes for which `pred` holds
PG_DEV void stats_count(unsigned long long *shards, int word, bool pred) {  // (the lanes that are active call it: the first of them for which pred holds adds)
    const unsigned long long m = __ballot(pred);
    if (m != 0 && lane_id() == __ffsll(m) - 1) atomicAdd(shards + (blockIdx.x & (PG_LIGHT_TEST_SHARDS - 1)) * PG_LIGHT_TEST_STRIDE + word, (unsigned long long)__popcll(m));
}

#endif  // PG_QUEUE_H
