// Workspace of the evaluation kernels (rollout_eval.hip, sac_fused.hip): what the persistent evaluation launch leaves for the
// compaction launch.  [records: (H, N) float2 (return, length) of the episode that ended at (t, env); length 0 = none ended there]
// [counts: (N) int32 episodes finished per env], rounded up to 256 bytes.  Every element is written by the evaluation launch
// (no clearing beforehand).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

struct ErlEvalWs {
    float2 *rec;
    int32_t *cnt;
};

constexpr int64_t kErlEvalMaxCells = (1LL << 31) - 1;      // N * H: the episode total is an int32

static inline int64_t erl_eval_ws_bytes(int64_t N, int64_t H)
{
    if (N < 1 || H < 1 || N > kErlEvalMaxCells / H) return -1;
    return (N * H * 8 + N * 4 + 255) / 256 * 256;
}

static inline ErlEvalWs erl_eval_ws_layout(void *workspace, int64_t N, int64_t H)
{
    ErlEvalWs w;
    w.rec = static_cast<float2 *>(workspace);
    w.cnt = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + N * H * 8);
    return w;
}
