// One PointChasingVecEnv step of one env (the reference's elegantrl/envs/PointChasingEnv.py:84-182: a chaser p1 steered by the action
// runs after a target p0 that drifts by a uniform draw per step), shared by the per-step kernel (erl_pointchasing_step_f32, envs.hip) and
// the one-launch rollouts / evaluations (rollout_fused_impl.h, sac_fused.hip).  `dim` in 1..4 is a run-time value; the observation is
// (p0, v0, p1, v1), `dim` floats each.  Every product, sum, quotient and square root is rounded on its own -- the reference's chain of
// ATen ops -- under the block-scope contraction pragmas below: the three translation units that inline this header are built with
// different flags, and none of them may fuse a multiply into an add here.
//
// Three deliberate deviations from the reference's vec env:
//   D1. After a reset `distance` is recomputed from the drawn positions (as the reference's single env does); the reference's vec env
//       leaves it stale, which gives the first reward of every later episode a spurious term of about -8 sqrt(dim).
//   D2. terminal = caught, truncate = timeout (this package's convention, envs.hip synenv_step_kernel); the reference raises its one
//       `terminal` flag for both, which stops the bootstrap at a time limit.
//   D3. Draws are Philox4x32-10, not torch's generator.  A step makes ONE call, counter (env, kPointChasingUniformTag, episode,
//       step-in-episode), key = the env seed: u_k = (word_k >> 8) * 2^-24.  philox_normal(seed, episode + 1, env, j) -- the reset draws --
//       calls counter (env, j >> 2, ..) with j >> 2 in {0, 1}, so the tag word keeps the two families apart.  A reset (caught or timeout)
//       draws p0_k = philox_normal(seed, episode + 1, env, k), p1_k = philox_normal(seed, episode + 1, env, dim + k) - 8, v0 = v1 = 0, and
//       the post-reset state is what the step returns.
#pragma once
#include "erl_common.h"

namespace {

constexpr int kPointChasingMaxDim = 4;
constexpr uint32_t kPointChasingUniformTag = 0x50434853u;      // second counter word of the per-step uniform call ("PCHS")
constexpr float kPointChasingInitDistance = 8.0f;

// row: the 4 * dim floats of one env's observation (p0, v0, p1, v1), in global memory or LDS.  The step works on it in place, one component
// at a time: held in registers whole (16 floats beside the action and the draw) it put the widest persistent rollouts, which keep their
// weights in registers, into scratch.

// sqrt(sum_k (p0_k - p1_k)^2), the sum in index order
__device__ __forceinline__ float pointchasing_distance(const float *row, int dim)
{
#pragma clang fp contract(off)
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kPointChasingMaxDim; ++k) {
        if (k < dim) {
            const float diff = row[k] - row[2 * dim + k];
            const float sq = diff * diff;
            sum = sum + sq;
        }
    }
    return sqrtf(sum);
}

// the state an env starts episode `episode` with (D3): a draw depends neither on the launch geometry nor on which kernel performs it
__device__ __forceinline__ void pointchasing_reset_draw(uint64_t seed, uint32_t env, uint32_t episode, int dim, float *row)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < kPointChasingMaxDim; ++k) {
        if (k < dim) {
            const float n0 = philox_normal(seed, (uint64_t)episode, env, (uint32_t)k);
            const float n1 = philox_normal(seed, (uint64_t)episode, env, (uint32_t)(dim + k));
            row[k] = n0;
            row[dim + k] = 0.f;
            row[2 * dim + k] = n1 - kPointChasingInitDistance;
            row[3 * dim + k] = 0.f;
        }
    }
}

// row: the state in, the next state -- or the reset draw where the step ends the episode -- out; a: the action (components >= dim are not
// read); distance: the env's carried |p0 - p1| in, that of the state returned out (D1); reward = distance_in - d - 0.02 max(|a|, 1)
// with d the distance BEFORE any reset; terminal = d < dim, truncate = step_count reached max_step and not terminal (D2).
__device__ __forceinline__ void pointchasing_step(float *row, const float (&a)[kPointChasingMaxDim], int dim, float &distance,
                                                  int &step_count, int &episode, int max_step, uint64_t seed, uint32_t env, float &reward,
                                                  bool &terminal, bool &truncate)
{
#pragma clang fp contract(off)
    const Philox4 p = philox4x32_10(env, kPointChasingUniformTag, (uint32_t)episode, (uint32_t)step_count, (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
    const uint32_t word[kPointChasingMaxDim] = {p.x, p.y, p.z, p.w};
    float a2 = 0.f;
#pragma unroll
    for (int k = 0; k < kPointChasingMaxDim; ++k) {
        if (k < dim) {
            const float sq = a[k] * a[k];
            a2 = a2 + sq;
        }
    }
    const float l2 = fmaxf(sqrtf(a2), 1.0f);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kPointChasingMaxDim; ++k) {
        if (k < dim) {
            const float ak = a[k] / l2;
            const float u = (float)(word[k] >> 8) * (1.0f / 16777216.0f);
            const float v1d = row[3 * dim + k] * 0.75f;
            const float v1 = v1d + ak;
            const float p1d = v1 * 0.01f;
            const float p1 = row[2 * dim + k] + p1d;
            const float v0d = row[dim + k] * 0.5f;
            const float v0 = v0d + u;
            const float p0d = v0 * 0.01f;
            const float p0 = row[k] + p0d;
            row[k] = p0;
            row[dim + k] = v0;
            row[2 * dim + k] = p1;
            row[3 * dim + k] = v1;
            const float diff = p0 - p1;
            const float sq = diff * diff;
            sum = sum + sq;
        }
    }
    const float d = sqrtf(sum);
    const float gain = distance - d;
    const float cost = l2 * 0.02f;
    reward = gain - cost;
    const int sc = step_count + 1;
    terminal = d < (float)dim;
    truncate = sc >= max_step && !terminal;
    const bool done = terminal || truncate;
    distance = d;
    if (done) {
        episode += 1;
        pointchasing_reset_draw(seed, env, (uint32_t)episode, dim, row);
        distance = pointchasing_distance(row, dim);
    }
    step_count = done ? 0 : sc;
}

}  // namespace
