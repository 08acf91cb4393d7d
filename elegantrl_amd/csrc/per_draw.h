// One stratified draw from the prioritised-replay trees (per.hip: the layout), shared by every kernel that samples: per_sample_kernel and
// per_sample_rows_kernel (per.hip) and the fused SAC step's first launch (sac_fused.hip actor_fwd_body) compile this arithmetic in this
// order, so a draw is the same bits wherever it runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one stratified draw of sequence q (stratum j of n, `u` its uniform): proportional prioritisation (:285-298) by a full-depth descent,
// then the two row moves; returns the time row and its importance weight.  The descent is bounded by node < L and the moves leave
// the row in [0, cur_size - 2] whatever the trees hold (a NaN compares false and walks right): the row never leaves the ring.
__device__ __forceinline__ int64_t per_draw(const float *__restrict__ sum, const float *__restrict__ mn, int64_t L, int64_t base, int64_t n,
                                            int64_t j, float u, int64_t cur_size, int64_t newest, float beta, float &weight)
{
    const float total = sum[base + 1];
    float v = ((float)j + u) * (total / (float)n);                      // (arange(n) + rand(n)) * (tree[0] / n)   (:287)
    int64_t node = 1;
    while (node < L) {
        const float left = sum[base + 2 * node];
        if (v <= left) node = 2 * node;
        else {
            v -= left;
            node = 2 * node + 1;
        }
    }
    int64_t row = node - L;
    if (row > cur_size - 2) row = cur_size - 2;                        // the last filled position has no successor row (oracle D4)
    if (row == newest) row = newest >= 1 ? newest - 1 : 1;             // full ring: the newest row's successor slot holds the OLDEST data (D6)
    weight = powf(sum[base + L + row] / mn[base + 1], -beta);           // (prob / min prob)^(-beta)   (:296-297)
    return row;
}

// the ring's write cursor `p` when the ring is full (cursor < 0: not full / unknown): the newest row (p - 1) is followed in memory by the
// oldest one, so it has no valid successor either; -1: every filled row but the last has one
inline int64_t per_newest(int64_t cursor, int64_t cur_size, int64_t max_size)
{
    return (cursor >= 0 && cur_size == max_size && max_size >= 3) ? (cursor + max_size - 1) % max_size : -1;
}
