// Discrete PPO on the device: the per-step kernels of the discrete envs (CartPole-v1, Acrobot-v1, MountainCar-v0), and the one-launch
// rollout / evaluation of the categorical policy on any of them.
//
// Every extern "C" entry is one statement that forwards to the body of its form, templated on the env (<env>: cartpole, acrobot,
// mountaincar):
//   erl_cartpole_step_f32 / erl_acrobot_step_f32 /  rd_step<Env>: env_step_kernel<Env>, one thread per env: cartpole_step.h /
//   erl_mountaincar_step_f32                        acrobot_step.h / mountaincar_step.h on the live state, reward / flag rows out.
//   erl_rollout_discrete_<env>_f32                  rd_rollout<Env, false>: all H steps of AgentDiscretePPO._explore_vec_env in ONE launch
//                                                   (rollout_discrete_kernel<Env, false>).
//   erl_rollout_discrete_<env>_gae_f32              rd_rollout<Env, true>: the rollout with a second phase in the same launch (GAE_): the
//                                                   critic's values of every visited state and of the final one, get_advantages, reward
//                                                   sums and the partial sums of the advantage normalisation (below, "The GAE_ form").
//   erl_eval_discrete_<env>_f32                     rd_eval<Env>: the evaluation form (EV_): the greedy policy argmax(logits), per-episode
//                                                   accounts (eval_ws.h) instead of buffer rows.
// The arguments travel in three packs (RdHead: policy and env up to N, H; RdPlanes: the rollout's draws and planes; RdGaeTail: the GAE_
// form's twelve); rd_fill checks the head for every form, and the kernel's argument is filled in one place per pack.
//
// The env behind the kernels is a trait (CartPoleEnv, AcrobotEnv, MountainCarEnv below): P physical floats per env, an S-wide observation, how an env's
// thread loads and stores both, how it forms the observation from the physical state, the action of an int64, and a step that returns
// the reward.  A further env costs a header with its step, one such struct, its extern "C" forwards (include/erl_hip.h, _hip._SIGNATURES)
// and one Python subclass of _DiscreteGpuVecEnv (envs/vec_envs.py).
//
// rollout_discrete_kernel.  A WAVE owns 16 envs for the whole horizon and never talks to another one: the actor's three layers run
// register-chained on the fp32 matrix cores (mlp_chain.h forward_layer: every layer transposed on the 16-env tile, a layer's result tile
// is the next layer's B operand without leaving the register file), the weights and biases are staged ONCE per launch into zero-padded
// LDS copies straight from the agent's parameter block (W1 b1 W2 b2 W3 b3, no repack), and the physical state and its observation live
// in the registers of the env's lane (q = 0 of its 16-lane group) between steps.  After the one barrier behind the staging there is no
// barrier, no cross-workgroup traffic and no wait of any kind: every workgroup runs to completion on its own.  Per step: states[t] out,
// normalise (feature k of the first k-tile is element k & 3 of lane group q = k >> 2: features past 3 leave the env's lane for its
// q >= 1 lanes by a cross-lane move inside the wave), layers 1-3, the logits meet in the wave's own LDS slot (lane (m, q) holds logits
// 4 q .. 4 q + 3 of env m), the env's lane runs categorical.h (softmax, inverse-CDF draw, log-prob: the per-step kernel's statements)
// and the env's step and observation (the per-step env kernel's statements), and writes the step's buffer cells.  Rows past N in the
// last tile replay env N - 1 and are never stored.
// A launch puts one wave in a workgroup while that fills the device's CUs with one wave each (4096 envs: 256 workgroups), up to four
// beyond; a draw and a reset are keyed by the env, so the geometry is not visible in the results.
// LDS: (h1 * 20 + h2 * lds_ld(h1) + 16 * lds_ld(h2) + 272 + waves * 272) floats: 92 KB at [128, 128], 14 KB at [64, 32].
//
// The GAE_ form.  Behind the H steps, which it runs unchanged, the workgroup meets at ONE barrier (every wave of it runs the same H
// steps, so the barrier is uniform; it also drains each wave's buffer stores) and stages the critic's [S, h1, h2, 1] block over the
// actor's LDS copies: the same layout with A = 1, so the LDS does not grow (two images would not fit at [128, 128]).  A wave then walks
// its own 16 envs back in time, t = H (the final state, still in the env's lane: cri(last_state)), H - 1, ..., 0: the observation of
// step t is read back from out_states, the reward and the flags from their planes, RD_GU steps share one pass over the weights (their
// tiles are independent until the scalar recurrence, and a lone wave's dependent MFMAs leave the pipe idle), the value of env m lands in
// its own lane (q = 0, element 0), which stores it and feeds erl_gae_step (gae_step.h: the exact scan's step) at once: no second pass,
// no LDS, any H.  Per 16-env tile one row of 3 fp64 sums (all, and sum / sum of squares over the [::4, ::4] subsample) goes to
// gae_ws[3 * tile ..]: an env's lane sums in scan order, the 16 lanes are added in lane order, rows past N add nothing and the row is
// indexed by the tile, not the workgroup, so the launch geometry stays invisible.  Still no wait and no cross-workgroup traffic.
// Why the read-back cannot return stale bytes: every byte a wave reads here was stored by THIS wave earlier in the launch and by
// nobody else (rows of its own envs; rows past N are not read), its stores have completed before the loads are issued (the barrier's
// s_waitcnt vmcnt(0)), and the vector L1 is per CU and written through: a line this CU holds was filled after, or updated by, the CU's
// own store, and no other CU's copy is involved.  So the loads are plain vector loads (the addresses differ per lane: nothing takes the
// scalar cache), with no fence and no cache-bypass bit.
#include "acrobot_step.h"
#include "cartpole_step.h"
#include "categorical.h"
#include "eval_ws.h"
#include "gae_step.h"
#include "mlp_chain.h"
#include "mountaincar_step.h"
#include <type_traits>

namespace {

constexpr int RD_GU = 4;                    // steps per pass over the critic's weights in the GAE_ form's second phase
constexpr int RD_MAX_A = 8;                 // logits of an env in its LDS slot
constexpr int RD_SLOT = 17;                 // floats per env slot: 8 logits | 8 probabilities (+ 1: 16 slots on 16 distinct banks)
constexpr int RD_LD1 = lds_ld(16);          // row stride of the W1 copy: one k-tile of 16 columns, zero beyond S

struct RdArgs {
    const float *P, *avg, *std;             // actor parameter block [S, h1, h2, A] without std; state_avg / state_std
    int h1, h2, A;
    int64_t N;
    int H;
    const float *uniform;                   // (H, N) or NULL
    uint64_t seed, counter0;
    float reward_scale;
    float *o_states;
    int32_t *o_actions;
    float *o_logprobs, *o_rewards;
    uint8_t *o_undones, *o_unmasks;
    float *o_last_state, *o_uniform;        // may be NULL
    float *env_state;                       // (N, Env::P) live physical state
    float *obs;                             // (N, Env::S) live observation (CartPole: env_state itself)
    int32_t *step_count, *episode;
    int max_step;
    uint64_t env_seed;
    float2 *ev_rec;                         // evaluation form
    int32_t *ev_cnt;
};

struct RdGaeArgs : RdArgs {                 // the GAE_ form's kernel argument (the other forms keep RdArgs as it is)
    const float *Pc, *cavg, *cstd;          // critic parameter block [S, h1, h2, 1]; its state_avg / state_std
    float *o_values, *o_next_value, *o_adv, *o_ret;
    double *gae_ws;                         // ceil(N / 16) rows of 3 partial sums
    float gamma, lam;
    int vtrace;
};

bool rd_dims_ok(int S, int h1, int h2, int A)
{
    return S >= 1 && S <= 64 && h1 >= 32 && h1 <= 128 && h1 % 32 == 0 && h2 >= 32 && h2 <= 128 && h2 % 32 == 0 && A >= 2 && A <= RD_MAX_A;
}

size_t rd_lds_floats(int h1, int h2, int waves)
{
    return (size_t)h1 * RD_LD1 + (size_t)h2 * lds_ld(h1) + 16 * (size_t)lds_ld(h2) + 128 + 128 + 16 + (size_t)waves * 16 * RD_SLOT;
}

// ---- the envs.  P: physical floats per env (env_state rows), S: observation width (the policy's input); load / store: an env's thread
// and the live buffers (env_state (N, P), obs (N, S)); observe: the observation of a physical state; action: the env's action of the
// int64 the per-step entry is handed; step: one env step on the physical state and the counters, returns the reward.
struct CartPoleEnv {                        // the observation IS the physical state (obs is env_state), the reward is 1
    static constexpr int P = 4, S = 4, A = 0;                  // A = 0: any action_dim the policy shapes allow (actions other than 1 push left)
    static constexpr const char *kName = "CartPole";
    static __device__ __forceinline__ void load(const float *env_state, const float *, int64_t row, float (&p)[P], float (&ob)[S])
    {
        const float4 v = *reinterpret_cast<const float4 *>(env_state + 4 * row);
        p[0] = ob[0] = v.x; p[1] = ob[1] = v.y; p[2] = ob[2] = v.z; p[3] = ob[3] = v.w;
    }
    static __device__ __forceinline__ int action(int64_t a) { return a == 1 ? 1 : 0; }
    static __device__ __forceinline__ void observe(const float (&p)[P], float (&ob)[S])
    {
#pragma unroll
        for (int c = 0; c < 4; ++c) ob[c] = p[c];
    }
    static __device__ __forceinline__ void store_obs(float *dst, const float (&ob)[S])
    {
        *reinterpret_cast<float4 *>(dst) = make_float4(ob[0], ob[1], ob[2], ob[3]);
    }
    static __device__ __forceinline__ void load_obs(const float *src, float (&ob)[S])          // what store_obs wrote (GAE_ form)
    {
        const float4 v = *reinterpret_cast<const float4 *>(src);
        ob[0] = v.x; ob[1] = v.y; ob[2] = v.z; ob[3] = v.w;
    }
    static __device__ __forceinline__ void store(float *env_state, float *, int64_t row, const float (&p)[P], const float (&ob)[S])
    {
        *reinterpret_cast<float4 *>(env_state + 4 * row) = make_float4(p[0], p[1], p[2], p[3]);
    }
    static __device__ __forceinline__ float step(float (&p)[P], int act, int &sc, int &ep, int max_step, uint64_t seed, uint32_t env,
                                                 bool &term, bool &trunc)
    {
        cartpole_step(p, act, sc, ep, max_step, seed, env, term, trunc);
        return 1.0f;
    }
};

struct AcrobotEnv {                         // the physical state (theta1, theta2, omega1, omega2) is of record; obs is the live observation
    static constexpr int P = 4, S = 6, A = 3;
    static constexpr const char *kName = "Acrobot";
    static __device__ __forceinline__ void load(const float *env_state, const float *obs, int64_t row, float (&p)[P], float (&ob)[S])
    {
        const float4 v = *reinterpret_cast<const float4 *>(env_state + 4 * row);
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        load_obs(obs + 6 * row, ob);        // the policy's input at t = 0 is the live observation as handed in, not observe(p)
    }
    static __device__ __forceinline__ int action(int64_t a) { return a == 0 ? 0 : (a == 2 ? 2 : 1); }
    static __device__ __forceinline__ void observe(const float (&p)[P], float (&ob)[S]) { acrobot_observe(p, ob); }
    static __device__ __forceinline__ void store_obs(float *dst, const float (&ob)[S])
    {
#pragma unroll
        for (int c = 0; c < 6; c += 2) *reinterpret_cast<float2 *>(dst + c) = make_float2(ob[c], ob[c + 1]);
    }
    static __device__ __forceinline__ void load_obs(const float *src, float (&ob)[S])          // what store_obs wrote (GAE_ form)
    {
#pragma unroll
        for (int c = 0; c < 6; c += 2) {
            const float2 o = *reinterpret_cast<const float2 *>(src + c);
            ob[c] = o.x; ob[c + 1] = o.y;
        }
    }
    static __device__ __forceinline__ void store(float *env_state, float *obs, int64_t row, const float (&p)[P], const float (&ob)[S])
    {
        *reinterpret_cast<float4 *>(env_state + 4 * row) = make_float4(p[0], p[1], p[2], p[3]);
        store_obs(obs + 6 * row, ob);
    }
    static __device__ __forceinline__ float step(float (&p)[P], int act, int &sc, int &ep, int max_step, uint64_t seed, uint32_t env,
                                                 bool &term, bool &trunc)
    {
        return acrobot_step(p, act, sc, ep, max_step, seed, env, term, trunc);
    }
};

struct MountainCarEnv {                     // the observation IS the physical state (position, velocity); the reward is -1 on every step
    static constexpr int P = 2, S = 2, A = 3;
    static constexpr const char *kName = "MountainCar";
    static __device__ __forceinline__ void load(const float *env_state, const float *, int64_t row, float (&p)[P], float (&ob)[S])
    {
        const float2 v = *reinterpret_cast<const float2 *>(env_state + 2 * row);
        p[0] = ob[0] = v.x; p[1] = ob[1] = v.y;
    }
    static __device__ __forceinline__ int action(int64_t a) { return a == 0 ? 0 : (a == 2 ? 2 : 1); }
    static __device__ __forceinline__ void observe(const float (&p)[P], float (&ob)[S]) { ob[0] = p[0]; ob[1] = p[1]; }
    static __device__ __forceinline__ void store_obs(float *dst, const float (&ob)[S])
    {
        *reinterpret_cast<float2 *>(dst) = make_float2(ob[0], ob[1]);
    }
    static __device__ __forceinline__ void load_obs(const float *src, float (&ob)[S])          // what store_obs wrote (GAE_ form)
    {
        const float2 v = *reinterpret_cast<const float2 *>(src);
        ob[0] = v.x; ob[1] = v.y;
    }
    static __device__ __forceinline__ void store(float *env_state, float *, int64_t row, const float (&p)[P], const float (&ob)[S])
    {
        *reinterpret_cast<float2 *>(env_state + 2 * row) = make_float2(p[0], p[1]);
    }
    static __device__ __forceinline__ float step(float (&p)[P], int act, int &sc, int &ep, int max_step, uint64_t seed, uint32_t env,
                                                 bool &term, bool &trunc)
    {
        mountaincar_step(p, act, sc, ep, max_step, seed, env, term, trunc);
        return -1.0f;
    }
};

// the per-step env kernel: one thread per env, the trait's statements on the live buffers, reward / flag rows out.  env_state and obs are
// not __restrict__: CartPole hands the same buffer in as both.  What load reads of obs is dead here (observe overwrites it before store).
template <typename Env>
__global__ __launch_bounds__(256) void env_step_kernel(float *env_state, float *obs, const int64_t *__restrict__ action,
                                                       int32_t *__restrict__ step_count, int32_t *__restrict__ episode,
                                                       float *__restrict__ reward, uint8_t *__restrict__ terminal,
                                                       uint8_t *__restrict__ truncate, int64_t N, int max_step, uint64_t seed)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s[Env::P], ob[Env::S];
    Env::load(env_state, obs, n, s, ob);
    int sc = step_count[n], ep = episode[n];
    bool term, trunc;
    const float r = Env::step(s, Env::action(action[n]), sc, ep, max_step, seed, (uint32_t)n, term, trunc);
    Env::observe(s, ob);
    Env::store(env_state, obs, n, s, ob);
    reward[n] = r;
    terminal[n] = term;
    truncate[n] = trunc;
    step_count[n] = sc;
    episode[n] = ep;
}

// forward_layer (mlp_chain.h) on U tiles at once (the GAE_ form's value pass): one pass over the weight copy, the U accumulation chains
// interleaved in the matrix pipe.  A tile's own products and sums come in forward_layer's order, so its result does not depend on U.
template <bool ACT, int KT, int U>
__device__ __forceinline__ void forward_layer_u(const float *W, int ldw, const float *bias, int kt_rt, int nout, const f32x4 (&in)[U][8],
                                                f32x4 (&outH)[U][8], int l15, int q)
{
    constexpr int NCH = KT ? (KT + PCH - 1) / PCH : 8 / PCH;           // chunks per output tile
    constexpr int NC = 8 * NCH;
    const int kt = KT ? KT : kt_rt;
    float4 wq[2][PCH];
    auto issue = [&](int c, float4(&dst)[PCH]) {
        const int ot = c / NCH, th = c % NCH;
#pragma unroll
        for (int j = 0; j < PCH; ++j) {
            const int t = PCH * th + j;
            if (ot < nout && t < kt) dst[j] = *reinterpret_cast<const float4 *>(W + (16 * ot + l15) * ldw + 16 * t + 4 * q);
        }
    };
    issue(0, wq[0]);
    f32x4 acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ot = c / NCH, th = c % NCH;
        if (c + 1 < NC) issue(c + 1, wq[(c + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (ot < nout) {
            if (th == 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < PCH; ++j) {
                const int t = PCH * th + j;
                if (t < kt) {
                    const float4 wv = wq[c & 1][j];
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[u] = mfma16(wv.x, in[u][t][0], acc[u]);
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[u] = mfma16(wv.y, in[u][t][1], acc[u]);
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[u] = mfma16(wv.z, in[u][t][2], acc[u]);
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[u] = mfma16(wv.w, in[u][t][3], acc[u]);
                }
            }
            if (th == NCH - 1) {
                const float4 b4 = *reinterpret_cast<const float4 *>(bias + 16 * ot + 4 * q);
                const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float z = acc[u][r] + bb[r];
                        if (ACT) {
                            float y, gd;
                            gelu_and_grad_fast(z, y, gd);
                            outH[u][ot][r] = y;
                        } else {
                            outH[u][ot][r] = z;
                        }
                    }
                }
            }
        }
    }
}

// rows i0 .. of a row-major [rows][cols] block (rows % R == 0) into an LDS copy with row stride ld: R loads per thread are in flight
// before the first one is consumed (a lone wave staging element by element waits out one memory round trip per element).
template <int R>
__device__ __forceinline__ void rd_copy_rows(float *dst, int ld, const float *src, int rows, int cols, int tid, int nthr)
{
    for (int i0 = 0; i0 < rows; i0 += R)
        for (int k = tid; k < cols; k += nthr) {
            float v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = src[(size_t)(i0 + r) * cols + k];
#pragma unroll
            for (int r = 0; r < R; ++r) dst[(i0 + r) * ld + k] = v[r];
        }
}

// the critic's [S, h1, h2, 1] block over the actor's LDS copies (the GAE_ form).  The layout is the actor's with one output row, so the
// padding the kernel's staging zeroed (columns past S / h1 / h2, bias entries past h1 / h2, W3 rows and b3 entries past A) still is
// zero: only the cells that held the actor's numbers are written -- the critic's where it has one, zero in W3 rows / b3 entries 1 .. 15.
// (A function of its own: the other forms' staging stays the statements it was, instruction for instruction.)
template <int S>
__device__ __forceinline__ void rd_stage_critic(const float *P, int h1, int h2, int ld2, int ld3, float *W1, float *W2, float *W3, float *B1,
                                                float *B2, float *B3, int tid, int nthr)
{
    const Dims d{S, h1, h2, 1};
    constexpr int R = 16;
    const float *b1 = P + d.ob1(), *b2 = P + d.ob2(), *w3 = P + d.oW3();
    const float pb1 = tid < h1 ? b1[tid] : 0.f, pb1b = tid + 64 < h1 ? b1[tid + 64] : 0.f;       // (requested ahead of the big block)
    const float pb2 = tid < h2 ? b2[tid] : 0.f, pb2b = tid + 64 < h2 ? b2[tid + 64] : 0.f;
    const float pw3 = tid < h2 ? w3[tid] : 0.f, pw3b = tid + 64 < h2 ? w3[tid + 64] : 0.f;
    const float pb3 = P[d.ob3()];
    for (int e0 = tid; e0 < h1 * S; e0 += R * nthr) {      // W1: rows of S floats, contiguous in the block
        float v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = e0 + r * nthr < h1 * S ? P[d.oW1() + e0 + r * nthr] : 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = e0 + r * nthr, i = e / S;
            if (e < h1 * S) W1[i * RD_LD1 + (e - i * S)] = v[r];
        }
    }
    rd_copy_rows<R>(W2, ld2, P + d.oW2(), h2, h1, tid, nthr);
    if (tid < 64) {                                         // (the first wave: hidden widths are at most 128)
        if (tid < h1) B1[tid] = pb1;
        if (tid + 64 < h1) B1[tid + 64] = pb1b;
        if (tid < h2) { B2[tid] = pb2; W3[tid] = pw3; }
        if (tid + 64 < h2) { B2[tid + 64] = pb2b; W3[tid + 64] = pw3b; }
    }
    for (int e = tid; e < 15 * ld3; e += nthr) W3[ld3 + e] = 0.f;
    if (tid < 16) B3[tid] = tid < 1 ? pb3 : 0.f;
}

// cri(ob[u]) of the wave's 16 envs for U observations each held by the env's lane (`own`: q = 0 of its 16-lane group): the critic's
// normalisation, then the three layers on the LDS copies as in the step loop.  v[u] is valid in the env's lane.  Every lane takes part.
template <int S, int U>
__device__ __forceinline__ void rd_values(const float *W1, const float *W2, const float *W3, const float *B1, const float *B2, const float *B3,
                                          int ld2, int ld3, int n1, int n2, const float (&ob)[U][S], const float (&avg)[S],
                                          const float (&den)[S], bool own, int l15, int q, float (&v)[U])
{
    f32x4 x[U][8], ha[U][8], hb[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float xn[S];
#pragma unroll
        for (int c = 0; c < S; ++c) xn[c] = (ob[u][c] - avg[c]) / den[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float w = (own && c < S) ? xn[c < S ? c : 0] : 0.f;      // (S < 4: elements S .. 3 are zero operands)
#pragma unroll
            for (int qq = 1; 4 * qq < S; ++qq) {
                const float up = 4 * qq + c < S ? __shfl(xn[4 * qq + c < S ? 4 * qq + c : 0], l15, 64) : 0.f;
                w = q == qq ? up : w;
            }
            x[u][0][c] = w;
        }
    }
    forward_layer_u<true, 1, U>(W1, RD_LD1, B1, 1, n1, x, ha, l15, q);
    forward_layer_u<true, 0, U>(W2, ld2, B2, n1, n2, ha, hb, l15, q);
    forward_layer_u<false, 0, U>(W3, ld3, B3, n2, 1, hb, x, l15, q);       // (the input tiles are free again: the one output tile)
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = x[u][0][0];
}

template <typename Env, bool EV_, bool GAE_ = false>
__global__ __launch_bounds__(256) void rollout_discrete_kernel(std::conditional_t<GAE_, RdGaeArgs, RdArgs> g)
{
    static_assert(Env::S >= 1 && Env::S <= 16, "the observation is one k-tile of layer 1");
    static_assert(!(EV_ && GAE_), "the evaluation form leaves no buffer rows to scan");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int h1 = g.h1, h2 = g.h2, A = g.A, n1 = h1 >> 4, n2 = h2 >> 4;
    const int ld2 = lds_ld(h1), ld3 = lds_ld(h2);
    float *W1 = smem, *W2 = W1 + h1 * RD_LD1, *W3 = W2 + h2 * ld2, *B1 = W3 + 16 * ld3, *B2 = B1 + 128, *B3 = B2 + 128, *ZP = B3 + 16;
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q = lane >> 4;
    constexpr int S = Env::S;

    // ---- the weights and biases, once per launch, from the agent's own parameter block into zero-padded LDS copies
    {
        const Dims d{S, h1, h2, A};
        for (int e = tid; e < h1 * RD_LD1; e += nthr) {
            const int i = e / RD_LD1, k = e - i * RD_LD1;
            W1[e] = k < S ? g.P[d.oW1() + (size_t)i * S + k] : 0.f;
        }
        for (int e = tid; e < h2 * ld2; e += nthr) {
            const int i = e / ld2, k = e - i * ld2;
            W2[e] = k < h1 ? g.P[d.oW2() + (size_t)i * h1 + k] : 0.f;
        }
        for (int e = tid; e < 16 * ld3; e += nthr) {
            const int i = e / ld3, k = e - i * ld3;
            W3[e] = (i < A && k < h2) ? g.P[d.oW3() + (size_t)i * h2 + k] : 0.f;
        }
        for (int e = tid; e < 128; e += nthr) {
            B1[e] = e < h1 ? g.P[d.ob1() + e] : 0.f;
            B2[e] = e < h2 ? g.P[d.ob2() + e] : 0.f;
        }
        if (tid < 16) B3[tid] = tid < A ? g.P[d.ob3() + tid] : 0.f;
    }
    __syncthreads();

    const int waves = nthr >> 6;
    const int64_t env = ((int64_t)blockIdx.x * waves + wave) * 16 + l15;
    const bool valid = env < g.N, own = q == 0;              // the env's lane: q = 0 of its 16-lane group
    const int64_t row = valid ? env : g.N - 1;               // rows past N replay env N - 1 (never stored)
    const size_t N = (size_t)g.N;
    const int H = g.H;
    float *slot = ZP + (wave * 16 + l15) * RD_SLOT;

    float s[Env::P], ob[S], avg[S], den[S];                   // physical state, its observation (the env's lane), the normalisation
    Env::load(g.env_state, g.obs, row, s, ob);
#pragma unroll
    for (int c = 0; c < S; ++c) { avg[c] = g.avg[c]; den[c] = g.std[c] + 1e-4f; }
    int sc = g.step_count[row], ep = g.episode[row];
    double ev_ret = 0.0;                                      // (evaluation form) the open episode and the episodes finished
    int ev_len = 0, ev_n = 0;

    for (int t = 0; t < H; ++t) {
        const size_t cell = (size_t)t * N + row;
        // the step's draw: issued before the layers, consumed behind them
        float u = 0.f;
        if constexpr (!EV_) u = g.uniform ? g.uniform[cell] : philox_uniform(g.seed, g.counter0 + (uint64_t)t, (uint32_t)row);
        if constexpr (!EV_)
            if (own && valid) Env::store_obs(g.o_states + S * cell, ob);

        // (ob - avg) / (std + 1e-4) in the env's lane; feature k is element k & 3 of lane group q = k >> 2: features 0..3 stay, those
        // past 3 move to the env's q >= 1 lanes inside the wave (every lane takes part); every other operand element is zero
        // (rd_values restates these statements: as one function shared by both, five of the six forms come out as other machine code)
        f32x4 x[8], ha[8], hb[8], z[8], gd[8];
        float xn[S];
#pragma unroll
        for (int c = 0; c < S; ++c) xn[c] = (ob[c] - avg[c]) / den[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = (own && c < S) ? xn[c < S ? c : 0] : 0.f;      // (S < 4: elements S .. 3 are zero operands)
#pragma unroll
            for (int qq = 1; 4 * qq < S; ++qq) {
                const float up = 4 * qq + c < S ? __shfl(xn[4 * qq + c < S ? 4 * qq + c : 0], l15, 64) : 0.f;
                v = q == qq ? up : v;
            }
            x[0][c] = v;
        }
        forward_layer<true, 1, false>(W1, RD_LD1, B1, 1, n1, x, ha, gd, l15, q);
        forward_layer<true, 0, false>(W2, ld2, B2, n1, n2, ha, hb, gd, l15, q);
        forward_layer<false, 0, false>(W3, ld3, B3, n2, 1, hb, z, gd, l15, q);

        // lane (m, q) holds logits 4 q .. 4 q + 3 of env m: they meet in the env's slot (this wave's lanes only)
        if (q < 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) slot[4 * q + r] = z[0][r];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        if (own) {
            int act;
            float lp = 0.f;
            if constexpr (EV_) act = categorical_greedy(slot, A);
            else categorical_draw(slot, A, u, slot + RD_MAX_A, act, lp);
            bool term, trunc;
            const float reward = Env::step(s, act, sc, ep, g.max_step, g.env_seed, (uint32_t)row, term, trunc);
            Env::observe(s, ob);
            if constexpr (EV_) {
                const bool done = term || trunc;
                ev_ret += (double)reward;
                ev_len += 1;
                if (valid) g.ev_rec[cell] = done ? make_float2((float)ev_ret, (float)ev_len) : make_float2(0.f, 0.f);
                if (done) { ev_n += 1; ev_ret = 0.0; ev_len = 0; }
            } else if (valid) {
                g.o_actions[cell] = act;
                g.o_logprobs[cell] = lp;
                g.o_rewards[cell] = g.reward_scale == 1.0f ? reward : reward * g.reward_scale;  // rewards *= reward_scale
                g.o_undones[cell] = term ? 0 : 1;                                               // logical_not
                g.o_unmasks[cell] = trunc ? 0 : 1;
                if (g.o_uniform) g.o_uniform[cell] = u;
            }
        }
        // the slot is rewritten by the next step's logits: this wave's reads above come first
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // ---- hand the environment back: live state, observation and counters; the agent's own copy of the final state
    if (own && valid) {
        Env::store(g.env_state, g.obs, row, s, ob);
        if (g.o_last_state) Env::store_obs(g.o_last_state + S * row, ob);
        g.step_count[row] = sc;
        g.episode[row] = ep;
        if constexpr (EV_) g.ev_cnt[row] = ev_n;
    }

    // ---- the GAE_ form's second phase (the file header): values, get_advantages (elegantrl/agents/AgentPPO.py:207-232), reward sums
    // (:146) and the sums of the advantage normalisation (:149) for this wave's 16 envs.  out_rewards / out_undones are NOT touched
    // (explore_env returns them as the reference does; the truncation fix-up is applied by erl_ppo_finish_f32 at the end of update_net).
    if constexpr (GAE_) {
        __syncthreads();                    // every wave is done with the actor's copies; this wave's buffer stores have completed
        rd_stage_critic<S>(g.Pc, h1, h2, ld2, ld3, W1, W2, W3, B1, B2, B3, tid, nthr);
        __syncthreads();
        const bool mine = own && valid;
        float cav[S], cden[S];
#pragma unroll
        for (int c = 0; c < S; ++c) { cav[c] = g.cavg[c]; cden[c] = g.cstd[c] + 1e-4f; }

        float nv, a = 0.f;                  // the scan's carry (gae_step.h)
        {                                   // t = H: the final state is still in the env's lane
            float o1[1][S], v1[1];
#pragma unroll
            for (int c = 0; c < S; ++c) o1[0][c] = ob[c];
            rd_values<S, 1>(W1, W2, W3, B1, B2, B3, ld2, ld3, n1, n2, o1, cav, cden, own, l15, q, v1);
            nv = v1[0];
            if (mine) g.o_next_value[row] = nv;
        }
        constexpr int U = RD_GU;
        float o[U][S], r[U];
        uint8_t ud[U], um[U];
        // steps tb, tb - 1, ..., tb - U + 1 of the env's own rows (below 0: step 0 again, not used)
        auto fetch = [&](int tb, float (&o_)[U][S], float (&r_)[U], uint8_t (&ud_)[U], uint8_t (&um_)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t cell = (size_t)max(tb - u, 0) * N + row;
                if (mine) {
                    Env::load_obs(g.o_states + S * cell, o_[u]);
                    r_[u] = g.o_rewards[cell]; ud_[u] = g.o_undones[cell]; um_[u] = g.o_unmasks[cell];
                } else {
#pragma unroll
                    for (int c = 0; c < S; ++c) o_[u][c] = 0.f;
                    r_[u] = 0.f; ud_[u] = 0; um_[u] = 0;
                }
            }
        };
        double s_all = 0, s_sub = 0, q_sub = 0;
        const bool sub_col = (row & 3) == 0;
        fetch(H - 1, o, r, ud, um);
        for (int tb = H - 1; tb >= 0; tb -= U) {
            float on[U][S], rn[U], v[U];
            uint8_t udn[U], umn[U];
            if (tb - U >= 0) fetch(tb - U, on, rn, udn, umn);            // the next pass's rows travel under this pass's layers
            rd_values<S, U>(W1, W2, W3, B1, B2, B3, ld2, ld3, n1, n2, o, cav, cden, own, l15, q, v);
            if (mine) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int t = tb - u;
                    if (t < 0) break;
                    const size_t cell = (size_t)t * N + row;
                    float r_eff;
                    uint8_t ud_eff;
                    const float out = g.vtrace ? erl_gae_step<true>(r[u], v[u], ud[u], um[u], g.gamma, g.lam, nv, a, r_eff, ud_eff)
                                               : erl_gae_step<false>(r[u], v[u], ud[u], um[u], g.gamma, g.lam, nv, a, r_eff, ud_eff);
                    g.o_values[cell] = v[u];
                    g.o_adv[cell] = out;
                    g.o_ret[cell] = erl_add_rn(out, v[u]);
                    s_all += out;
                    if (sub_col && (t & 3) == 0) {
                        s_sub += out;
                        q_sub += (double)out * out;
                    }
                }
            }
            if (tb - U >= 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int c = 0; c < S; ++c) o[u][c] = on[u][c];
                    r[u] = rn[u]; ud[u] = udn[u]; um[u] = umn[u];
                }
            }
        }
        // the tile's row of sums: the 16 env lanes (0..15 of the wave) in lane order; the other lanes hold zeros
        double w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            w0 += __shfl(s_all, i, 64);
            w1 += __shfl(s_sub, i, 64);
            w2 += __shfl(q_sub, i, 64);
        }
        const int64_t tile = (int64_t)blockIdx.x * waves + wave;
        if (lane == 0 && tile * 16 < g.N) {                  // (a wave wholly past N has no row)
            g.gae_ws[3 * tile + 0] = w0;
            g.gae_ws[3 * tile + 1] = w1;
            g.gae_ws[3 * tile + 2] = w2;
        }
    }
}

template <typename Env, bool EV_, bool GAE_ = false>
int rd_launch(const std::conditional_t<GAE_, RdGaeArgs, RdArgs> &g, const char *what, hipStream_t stream)
{
    // one wave per workgroup while that is at most one workgroup per CU of a 256-CU device, up to four waves beyond
    const int64_t tiles = erl_cdiv(g.N, 16);
    int waves = (int)erl_cdiv(tiles, 256);
    waves = waves < 1 ? 1 : (waves > 4 ? 4 : waves);
    const size_t lds = rd_lds_floats(g.h1, g.h2, waves) * sizeof(float);
    ERL_REQUIRE(lds <= 160 * 1024, "%s: %zu bytes of LDS", what, lds);
    if (lds > 48 * 1024) {                  // asked at every such launch (a host-side call): no cache to keep per device and per thread
        int rc = erl_hip_status(hipFuncSetAttribute((const void *)rollout_discrete_kernel<Env, EV_, GAE_>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)lds), "hipFuncSetAttribute(rollout_discrete_kernel)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL((rollout_discrete_kernel<Env, EV_, GAE_>), dim3((unsigned)erl_cdiv(tiles, waves)), dim3(64 * waves), lds, stream, g);
    return erl_hip_status(hipGetLastError(), what);
}

// ---- the entries' argument packs as the C ABI spells them (include/erl_hip.h), in its order
struct RdHead {                             // the policy and the env, up to N, H (CartPole: obs is env_state)
    const float *actor_params, *act_avg, *act_std;
    int S, h1, h2, A;
    float *env_state, *obs;
    int32_t *step_count, *episode;
    int max_step;
    uint64_t env_seed;
    int64_t N, H;
};

struct RdPlanes {                           // the rollout's draws and the planes it writes
    const float *uniform;
    uint64_t seed, counter0;
    float reward_scale;
    float *out_states;
    int32_t *out_actions;
    float *out_logprobs, *out_rewards;
    uint8_t *out_undones, *out_unmasks;
    float *out_last_state, *out_uniform;
};

struct RdGaeTail {                          // the GAE_ form's twelve: the critic, the four planes it leaves, the rows of partial sums, the scan
    const float *critic_params, *cri_avg, *cri_std;
    float *out_values, *out_next_value, *out_advantages, *out_reward_sums;
    void *gae_partials;
    int64_t gae_partials_bytes;
    float gamma, lambda_gae;
    int use_v_trace;
};

template <typename Env>
int rd_fill(RdArgs &g, const char *what, const RdHead &e)
{
    ERL_REQUIRE(e.actor_params && e.act_avg && e.act_std && e.env_state && e.obs && e.step_count && e.episode, "%s: NULL tensor", what);
    ERL_REQUIRE(rd_dims_ok(e.S, e.h1, e.h2, e.A), "%s: unsupported dims S=%d net=[%d,%d] A=%d (one-launch discrete rollout: state_dim <= 64, 2 "
                "hidden layers of 32..128 in steps of 32, 2 <= action_dim <= %d)", what, e.S, e.h1, e.h2, e.A, RD_MAX_A);
    ERL_REQUIRE(e.S == Env::S, "%s: bad environment argument: %s's state_dim is %d, not %d", what, Env::kName, Env::S, e.S);
    ERL_REQUIRE(Env::A == 0 || e.A == Env::A, "%s: bad environment argument: %s's action_dim is %d, not %d", what, Env::kName, Env::A, e.A);
    ERL_REQUIRE(e.N >= 1 && e.H >= 1 && e.H < (1LL << 30) && e.N <= ((1LL << 31) - 1) / e.H && e.max_step >= 1,
                "%s: bad shape N=%lld H=%lld max_step=%d", what, (long long)e.N, (long long)e.H, e.max_step);
    g.P = e.actor_params; g.avg = e.act_avg; g.std = e.act_std;
    g.h1 = e.h1; g.h2 = e.h2; g.A = e.A; g.N = e.N; g.H = (int)e.H;
    g.env_state = e.env_state; g.obs = e.obs; g.step_count = e.step_count; g.episode = e.episode; g.max_step = e.max_step; g.env_seed = e.env_seed;
    return ERL_OK;
}

// the rollout entries' body; the plain form is the GAE_ form without its tail (`c` is not read).  Every pointer of the tail is required.
template <typename Env, bool GAE_>
int rd_rollout(const char *what, const RdHead &e, const RdPlanes &o, const RdGaeTail &c, void *stream)
{
    ERL_REQUIRE(o.out_states && o.out_actions && o.out_logprobs && o.out_rewards && o.out_undones && o.out_unmasks, "%s: NULL tensor", what);
    if constexpr (GAE_) {
        ERL_REQUIRE(c.critic_params, "%s: NULL tensor (critic_params)", what);
        ERL_REQUIRE(c.cri_avg, "%s: NULL tensor (cri_avg)", what);
        ERL_REQUIRE(c.cri_std, "%s: NULL tensor (cri_std)", what);
        ERL_REQUIRE(c.out_values, "%s: NULL tensor (out_values)", what);
        ERL_REQUIRE(c.out_next_value, "%s: NULL tensor (out_next_value)", what);
        ERL_REQUIRE(c.out_advantages, "%s: NULL tensor (out_advantages)", what);
        ERL_REQUIRE(c.out_reward_sums, "%s: NULL tensor (out_reward_sums)", what);
        ERL_REQUIRE(c.gae_partials, "%s: NULL tensor (gae_partials)", what);
    }
    std::conditional_t<GAE_, RdGaeArgs, RdArgs> g{};
    int rc = rd_fill<Env>(g, what, e);
    if (rc) return rc;
    g.uniform = o.uniform; g.seed = o.seed; g.counter0 = o.counter0; g.reward_scale = o.reward_scale;
    g.o_states = o.out_states; g.o_actions = o.out_actions; g.o_logprobs = o.out_logprobs; g.o_rewards = o.out_rewards;
    g.o_undones = o.out_undones; g.o_unmasks = o.out_unmasks; g.o_last_state = o.out_last_state; g.o_uniform = o.out_uniform;
    if constexpr (GAE_) {
        const int64_t need = erl_rollout_discrete_gae_workspace_bytes(e.N);
        ERL_REQUIRE(need > 0 && c.gae_partials_bytes >= need, "%s: gae_partials of %lld bytes, erl_rollout_discrete_gae_workspace_bytes(N) = %lld",
                    what, (long long)c.gae_partials_bytes, (long long)need);
        g.Pc = c.critic_params; g.cavg = c.cri_avg; g.cstd = c.cri_std;
        g.o_values = c.out_values; g.o_next_value = c.out_next_value; g.o_adv = c.out_advantages; g.o_ret = c.out_reward_sums;
        g.gae_ws = (double *)c.gae_partials; g.gamma = c.gamma; g.lam = c.lambda_gae; g.vtrace = c.use_v_trace ? 1 : 0;
    }
    return rd_launch<Env, false, GAE_>(g, what, (hipStream_t)stream);
}

// the evaluation entries' body
template <typename Env>
int rd_eval(const char *what, const RdHead &e, void *workspace, int64_t workspace_bytes, void *stream)
{
    ERL_REQUIRE(workspace, "%s: NULL tensor (workspace)", what);
    RdArgs g{};
    int rc = rd_fill<Env>(g, what, e);
    if (rc) return rc;
    ERL_REQUIRE(erl_eval_ws_bytes(e.N, e.H) > 0 && workspace_bytes >= erl_eval_ws_bytes(e.N, e.H),
                "%s: workspace of %lld bytes, erl_eval_workspace_bytes(N, H) = %lld", what, (long long)workspace_bytes,
                (long long)erl_eval_ws_bytes(e.N, e.H));
    const ErlEvalWs w = erl_eval_ws_layout(workspace, e.N, e.H);
    g.ev_rec = w.rec; g.ev_cnt = w.cnt;
    return rd_launch<Env, true>(g, what, (hipStream_t)stream);
}

// the per-step entries' body (CartPole: obs is env_state)
template <typename Env>
int rd_step(const char *what, float *env_state, float *obs, const int64_t *action, int32_t *step_count, int32_t *episode, float *reward,
            uint8_t *terminal, uint8_t *truncate, int64_t N, int max_step, uint64_t seed, void *stream)
{
    ERL_REQUIRE(env_state && obs && action && step_count && episode && reward && terminal && truncate, "%s: NULL tensor", what);
    ERL_REQUIRE(N >= 1 && N < (1LL << 31) && max_step >= 1, "%s: bad shape N=%lld max_step=%d", what, (long long)N, max_step);
    hipLaunchKernelGGL(env_step_kernel<Env>, dim3((unsigned)erl_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, env_state, obs, action,
                       step_count, episode, reward, terminal, truncate, N, max_step, seed);
    ERL_LAUNCH_CHECK(what);
}

}  // namespace

extern "C" int erl_rollout_discrete_supported(int S, int h1, int h2, int A) { return rd_dims_ok(S, h1, h2, A) ? 1 : 0; }

extern "C" int erl_rollout_discrete_gae_partials(int64_t N) { return N >= 1 && N < (1LL << 31) ? (int)erl_cdiv(N, 16) : -1; }

extern "C" int64_t erl_rollout_discrete_gae_workspace_bytes(int64_t N)
{
    return N >= 1 && N < (1LL << 31) ? erl_cdiv(N, 16) * 3 * (int64_t)sizeof(double) : -1;
}

// ---- CartPole-v1: env_state is both live buffers
extern "C" int erl_cartpole_step_f32(float *state, const int64_t *action, int32_t *step_count, int32_t *episode, float *reward,
                                     uint8_t *terminal, uint8_t *truncate, int64_t N, int max_step, uint64_t seed, void *stream)
{
    return rd_step<CartPoleEnv>("erl_cartpole_step_f32", state, state, action, step_count, episode, reward, terminal, truncate, N, max_step, seed,
                                stream);
}

extern "C" int erl_rollout_discrete_cartpole_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2,
                                                 int A, float *env_state, int32_t *step_count, int32_t *episode, int max_step,
                                                 uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                 uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                 float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                 float *out_last_state, float *out_uniform, void *stream)
{
    return rd_rollout<CartPoleEnv, false>(
        "erl_rollout_discrete_cartpole_f32",
        {actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step, env_seed, N, H},
        {uniform, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks, out_last_state,
         out_uniform}, {}, stream);
}

extern "C" int erl_rollout_discrete_cartpole_gae_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1,
                                                     int h2, int A, float *env_state, int32_t *step_count, int32_t *episode, int max_step,
                                                     uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                     uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                     float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                     float *out_last_state, float *out_uniform, const float *critic_params,
                                                     const float *cri_avg, const float *cri_std, float *out_values, float *out_next_value,
                                                     float *out_advantages, float *out_reward_sums, void *gae_partials,
                                                     int64_t gae_partials_bytes, float gamma, float lambda_gae, int use_v_trace, void *stream)
{
    return rd_rollout<CartPoleEnv, true>(
        "erl_rollout_discrete_cartpole_gae_f32",
        {actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step, env_seed, N, H},
        {uniform, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks, out_last_state,
         out_uniform},
        {critic_params, cri_avg, cri_std, out_values, out_next_value, out_advantages, out_reward_sums, gae_partials, gae_partials_bytes, gamma,
         lambda_gae, use_v_trace}, stream);
}

extern "C" int erl_eval_discrete_cartpole_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2, int A,
                                              float *env_state, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed,
                                              int64_t N, int64_t H, void *workspace, int64_t workspace_bytes, void *stream)
{
    return rd_eval<CartPoleEnv>("erl_eval_discrete_cartpole_f32",
                                {actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step, env_seed, N, H},
                                workspace, workspace_bytes, stream);
}

// ---- Acrobot-v1: phys is of record, obs is the live observation
extern "C" int erl_acrobot_step_f32(float *phys, float *obs, const int64_t *action, int32_t *step_count, int32_t *episode, float *reward,
                                    uint8_t *terminal, uint8_t *truncate, int64_t N, int max_step, uint64_t seed, void *stream)
{
    return rd_step<AcrobotEnv>("erl_acrobot_step_f32", phys, obs, action, step_count, episode, reward, terminal, truncate, N, max_step, seed,
                               stream);
}

extern "C" int erl_rollout_discrete_acrobot_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2,
                                                int A, float *phys, float *obs, int32_t *step_count, int32_t *episode, int max_step,
                                                uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                float *out_last_state, float *out_uniform, void *stream)
{
    return rd_rollout<AcrobotEnv, false>(
        "erl_rollout_discrete_acrobot_f32", {actor_params, act_avg, act_std, S, h1, h2, A, phys, obs, step_count, episode, max_step, env_seed, N, H},
        {uniform, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks, out_last_state,
         out_uniform}, {}, stream);
}

extern "C" int erl_rollout_discrete_acrobot_gae_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1,
                                                    int h2, int A, float *phys, float *obs, int32_t *step_count, int32_t *episode,
                                                    int max_step, uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                    uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                    float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                    float *out_last_state, float *out_uniform, const float *critic_params,
                                                    const float *cri_avg, const float *cri_std, float *out_values, float *out_next_value,
                                                    float *out_advantages, float *out_reward_sums, void *gae_partials,
                                                    int64_t gae_partials_bytes, float gamma, float lambda_gae, int use_v_trace, void *stream)
{
    return rd_rollout<AcrobotEnv, true>(
        "erl_rollout_discrete_acrobot_gae_f32", {actor_params, act_avg, act_std, S, h1, h2, A, phys, obs, step_count, episode, max_step, env_seed, N, H},
        {uniform, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks, out_last_state,
         out_uniform},
        {critic_params, cri_avg, cri_std, out_values, out_next_value, out_advantages, out_reward_sums, gae_partials, gae_partials_bytes, gamma,
         lambda_gae, use_v_trace}, stream);
}

extern "C" int erl_eval_discrete_acrobot_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2, int A,
                                             float *phys, float *obs, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed,
                                             int64_t N, int64_t H, void *workspace, int64_t workspace_bytes, void *stream)
{
    return rd_eval<AcrobotEnv>("erl_eval_discrete_acrobot_f32",
                               {actor_params, act_avg, act_std, S, h1, h2, A, phys, obs, step_count, episode, max_step, env_seed, N, H}, workspace,
                               workspace_bytes, stream);
}

// ---- MountainCar-v0: env_state (N, 2) = (position, velocity) is both live buffers
extern "C" int erl_mountaincar_step_f32(float *state, const int64_t *action, int32_t *step_count, int32_t *episode, float *reward,
                                        uint8_t *terminal, uint8_t *truncate, int64_t N, int max_step, uint64_t seed, void *stream)
{
    return rd_step<MountainCarEnv>("erl_mountaincar_step_f32", state, state, action, step_count, episode, reward, terminal, truncate, N, max_step,
                                   seed, stream);
}

extern "C" int erl_rollout_discrete_mountaincar_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2,
                                                    int A, float *env_state, int32_t *step_count, int32_t *episode, int max_step,
                                                    uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                    uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                    float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                    float *out_last_state, float *out_uniform, void *stream)
{
    return rd_rollout<MountainCarEnv, false>(
        "erl_rollout_discrete_mountaincar_f32",
        {actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step, env_seed, N, H},
        {uniform, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks, out_last_state,
         out_uniform}, {}, stream);
}

extern "C" int erl_rollout_discrete_mountaincar_gae_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1,
                                                        int h2, int A, float *env_state, int32_t *step_count, int32_t *episode, int max_step,
                                                        uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                        uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                        float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                        float *out_last_state, float *out_uniform, const float *critic_params,
                                                        const float *cri_avg, const float *cri_std, float *out_values, float *out_next_value,
                                                        float *out_advantages, float *out_reward_sums, void *gae_partials,
                                                        int64_t gae_partials_bytes, float gamma, float lambda_gae, int use_v_trace, void *stream)
{
    return rd_rollout<MountainCarEnv, true>(
        "erl_rollout_discrete_mountaincar_gae_f32",
        {actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step, env_seed, N, H},
        {uniform, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks, out_last_state,
         out_uniform},
        {critic_params, cri_avg, cri_std, out_values, out_next_value, out_advantages, out_reward_sums, gae_partials, gae_partials_bytes, gamma,
         lambda_gae, use_v_trace}, stream);
}

extern "C" int erl_eval_discrete_mountaincar_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2,
                                                 int A, float *env_state, int32_t *step_count, int32_t *episode, int max_step,
                                                 uint64_t env_seed, int64_t N, int64_t H, void *workspace, int64_t workspace_bytes, void *stream)
{
    return rd_eval<MountainCarEnv>("erl_eval_discrete_mountaincar_f32",
                                   {actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step, env_seed, N, H},
                                   workspace, workspace_bytes, stream);
}
