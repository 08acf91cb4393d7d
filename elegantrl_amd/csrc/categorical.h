// The categorical policy head's per-row arithmetic (ActorDiscretePPO, elegantrl/agents/AgentPPO.py:393-422), shared by the layered
// path's kernels (mlpn_common.h: sample_categorical_kernel, objective_discrete_kernel) and the one-launch discrete rollout
// (rollout_discrete.hip): softmax, the inverse-CDF draw and the log-prob of the draw are ONE set of statements.
// torch.distributions.Categorical(probs = softmax(z)) works on logits = log(clamp(p, eps, 1 - eps)) with
// eps = float32 machine epsilon: log_prob(a) = logits[a], entropy = -sum p logits; the clamp has zero gradient outside.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kMaxDiscrete = 64;             // action_dim of the discrete path
constexpr float kCatEps = 1.1920928955078125e-07f;

__device__ __forceinline__ void softmax_row(const float *__restrict__ z, int A, float *p)
{
    float mx = z[0];
    for (int a = 1; a < A; ++a) mx = fmaxf(mx, z[a]);
    float sum = 0.f;
    for (int a = 0; a < A; ++a) { p[a] = expf(z[a] - mx); sum += p[a]; }
    const float inv = 1.f / sum;
    for (int a = 0; a < A; ++a) p[a] *= inv;
}

// inverse-CDF draw from softmax(z) with u in [0, 1) and the log-prob of the draw; p: A floats of the caller's (receives softmax(z))
__device__ __forceinline__ void categorical_draw(const float *__restrict__ z, int A, float u, float *p, int &act_out, float &logprob_out)
{
    softmax_row(z, A, p);
    int act = A - 1;
    float c = 0.f;
    for (int a = 0; a < A; ++a) {
        c += p[a];
        if (u < c) { act = a; break; }
    }
    act_out = act;
    logprob_out = logf(fminf(fmaxf(p[act], kCatEps), 1.f - kCatEps));
}

// the greedy action argmax(z) (ActorDiscretePPO.forward); the first index on ties, as torch.argmax
__device__ __forceinline__ int categorical_greedy(const float *__restrict__ z, int A)
{
    int best = 0;
    float mx = z[0];
    for (int a = 1; a < A; ++a)
        if (z[a] > mx) { mx = z[a]; best = a; }
    return best;
}

}  // namespace
