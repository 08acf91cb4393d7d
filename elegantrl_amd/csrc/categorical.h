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

// The PPO objective of the categorical head for ONE sample whose logits are spread over four lanes, as the output tile of the
// register-chained minibatch kernel leaves them (ppo_step_discrete.hip): the lane of group q = lane >> 4 holds z[r] = logit of action
// a = 4 q + r, the three other lanes of the sample are lane ^ 16, ^ 32, ^ 48 (A <= 16).  The math is objective_discrete_kernel's
// (mlpn_common.h), statement for statement; only the sums over the actions cross lanes.  All four lanes of a sample must call it
// together and pass the same per-sample scalars; every one of them gets the same `surr` and `ent` (a + b is commutative, so the two
// butterfly hops give the four lanes the same bits).  dz[r] = dL/dz of this lane's actions, 0 for a >= A.
struct CatPpoTerms {
    float surr, ent;             // adv * ratio * clip scale,  entropy of the row
};
__device__ __forceinline__ float cat_sum4(float v)
{
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ CatPpoTerms categorical_ppo_terms_q4(const float (&z)[4], int q, int A, int act, float adv, float logp_old, float um,
                                                                float ratio_clip, float lambda_entropy, float inv_batch, float (&dz)[4])
{
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = 4 * q + r < A ? fmaxf(mx, z[r]) : mx;
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float p[4], sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        p[r] = 4 * q + r < A ? expf(z[r] - mx) : 0.f;
        sum += p[r];
    }
    const float inv = 1.f / cat_sum4(sum);
    act = act < 0 ? 0 : (act >= A ? A - 1 : act);
    float ent = 0.f, ph = 0.f, p_act = 0.f, h[4];                   // entropy, sum_k p_k h_k with h_k = dH/dp_k
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        p[r] *= inv;
        const bool on = 4 * q + r < A;
        const bool inside = p[r] > kCatEps && p[r] < 1.f - kCatEps;
        const float L = logf(fminf(fmaxf(p[r], kCatEps), 1.f - kCatEps));
        h[r] = -(L + (inside ? 1.f : 0.f));
        ent -= on ? p[r] * L : 0.f;
        ph += on ? p[r] * h[r] : 0.f;
        p_act += 4 * q + r == act ? p[r] : 0.f;
    }
    ent = cat_sum4(ent);
    ph = cat_sum4(ph);
    p_act = cat_sum4(p_act);                                        // three of the four terms are 0: exact
    const bool a_inside = p_act > kCatEps && p_act < 1.f - kCatEps;
    const float lp = logf(fminf(fmaxf(p_act, kCatEps), 1.f - kCatEps));
    const float ratio = expf(lp - logp_old);
    const float w = adv > 0.f ? 1.f - ratio_clip : 1.f + ratio_clip;
    const float surr = adv * ratio * w;
    // loss = -(mean(surr um) - lambda mean(ent um)):  dL/dlp = -surr um / B,  dL/dent = lambda um / B
    const float dlp = a_inside ? -(surr * um) * inv_batch : 0.f;
    const float dent = lambda_entropy * um * inv_batch;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int a = 4 * q + r;
        dz[r] = a < A ? dlp * ((a == act ? 1.f : 0.f) - p[r]) + dent * p[r] * (h[r] - ph) : 0.f;
    }
    return CatPpoTerms{surr, ent};
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
