// Discrete PPO on the device: the per-step kernels of the discrete envs (CartPole-v1, Acrobot-v1), and the one-launch rollout /
// evaluation of the categorical policy on either of them.
//
//   erl_cartpole_step_f32 / erl_acrobot_step_f32    one thread per env: cartpole_step.h / acrobot_step.h on the live state, reward /
//                                                   flag rows out.
//   erl_rollout_discrete_{cartpole,acrobot}_f32     all H steps of AgentDiscretePPO._explore_vec_env in ONE launch
//                                                   (rollout_discrete_kernel<Env, false>).
//   erl_eval_discrete_{cartpole,acrobot}_f32        its evaluation form (EV_): the greedy policy argmax(logits), per-episode accounts
//                                                   (eval_ws.h) instead of buffer rows.
//
// The env behind the kernel is a trait (CartPoleEnv, AcrobotEnv below): P physical floats per env, an S-wide observation, how the env's
// lane loads and stores both, how it forms the observation from the physical state, and a step that returns the reward.  A further env
// is a header with its step and one such struct.
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
#include "acrobot_step.h"
#include "cartpole_step.h"
#include "categorical.h"
#include "eval_ws.h"
#include "mlp_chain.h"

namespace {

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

bool rd_dims_ok(int S, int h1, int h2, int A)
{
    return S >= 1 && S <= 64 && h1 >= 32 && h1 <= 128 && h1 % 32 == 0 && h2 >= 32 && h2 <= 128 && h2 % 32 == 0 && A >= 2 && A <= RD_MAX_A;
}

size_t rd_lds_floats(int h1, int h2, int waves)
{
    return (size_t)h1 * RD_LD1 + (size_t)h2 * lds_ld(h1) + 16 * (size_t)lds_ld(h2) + 128 + 128 + 16 + (size_t)waves * 16 * RD_SLOT;
}

__global__ __launch_bounds__(256) void cartpole_step_kernel(float *__restrict__ state, const int64_t *__restrict__ action,
                                                            int32_t *__restrict__ step_count, int32_t *__restrict__ episode,
                                                            float *__restrict__ reward, uint8_t *__restrict__ terminal,
                                                            uint8_t *__restrict__ truncate, int64_t N, int max_step, uint64_t seed)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float4 v = *reinterpret_cast<const float4 *>(state + 4 * n);
    float s[4] = {v.x, v.y, v.z, v.w};
    int sc = step_count[n], ep = episode[n];
    bool term, trunc;
    cartpole_step(s, action[n] == 1 ? 1 : 0, sc, ep, max_step, seed, (uint32_t)n, term, trunc);      // (compared as int64)
    *reinterpret_cast<float4 *>(state + 4 * n) = make_float4(s[0], s[1], s[2], s[3]);
    reward[n] = 1.0f;
    terminal[n] = term;
    truncate[n] = trunc;
    step_count[n] = sc;
    episode[n] = ep;
}

__global__ __launch_bounds__(256) void acrobot_step_kernel(float *__restrict__ phys, float *__restrict__ obs,
                                                           const int64_t *__restrict__ action, int32_t *__restrict__ step_count,
                                                           int32_t *__restrict__ episode, float *__restrict__ reward,
                                                           uint8_t *__restrict__ terminal, uint8_t *__restrict__ truncate, int64_t N,
                                                           int max_step, uint64_t seed)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float4 v = *reinterpret_cast<const float4 *>(phys + 4 * n);
    float s[4] = {v.x, v.y, v.z, v.w}, ob[6];
    int sc = step_count[n], ep = episode[n];
    const int64_t a = action[n];
    bool term, trunc;
    const float r = acrobot_step(s, a == 0 ? 0 : (a == 2 ? 2 : 1), sc, ep, max_step, seed, (uint32_t)n, term, trunc);      // (compared as int64)
    acrobot_observe(s, ob);
    *reinterpret_cast<float4 *>(phys + 4 * n) = make_float4(s[0], s[1], s[2], s[3]);
#pragma unroll
    for (int c = 0; c < 6; c += 2) *reinterpret_cast<float2 *>(obs + 6 * n + c) = make_float2(ob[c], ob[c + 1]);
    reward[n] = r;
    terminal[n] = term;
    truncate[n] = trunc;
    step_count[n] = sc;
    episode[n] = ep;
}

// ---- the envs of the one-launch kernel.  P: physical floats per env (g.env_state rows), S: observation width (the policy's input);
// load / store: the env's lane and the live buffers; observe: the observation of a physical state; step: one env step on the physical
// state and the counters, returns the reward.
struct CartPoleEnv {                        // the observation IS the physical state, the reward is 1
    static constexpr int P = 4, S = 4, A = 0;                  // A = 0: any action_dim the policy shapes allow (actions other than 1 push left)
    static constexpr const char *kName = "CartPole";
    static __device__ __forceinline__ void load(const RdArgs &g, int64_t row, float (&p)[P], float (&ob)[S])
    {
        const float4 v = *reinterpret_cast<const float4 *>(g.env_state + 4 * row);
        p[0] = ob[0] = v.x; p[1] = ob[1] = v.y; p[2] = ob[2] = v.z; p[3] = ob[3] = v.w;
    }
    static __device__ __forceinline__ void observe(const float (&p)[P], float (&ob)[S])
    {
#pragma unroll
        for (int c = 0; c < 4; ++c) ob[c] = p[c];
    }
    static __device__ __forceinline__ void store_obs(float *dst, const float (&ob)[S])
    {
        *reinterpret_cast<float4 *>(dst) = make_float4(ob[0], ob[1], ob[2], ob[3]);
    }
    static __device__ __forceinline__ void store(const RdArgs &g, int64_t row, const float (&p)[P], const float (&ob)[S])
    {
        *reinterpret_cast<float4 *>(g.env_state + 4 * row) = make_float4(p[0], p[1], p[2], p[3]);
    }
    static __device__ __forceinline__ float step(float (&p)[P], int act, int &sc, int &ep, int max_step, uint64_t seed, uint32_t env,
                                                 bool &term, bool &trunc)
    {
        cartpole_step(p, act, sc, ep, max_step, seed, env, term, trunc);
        return 1.0f;
    }
};

struct AcrobotEnv {                         // the physical state (theta1, theta2, omega1, omega2) is of record; g.obs is the live observation
    static constexpr int P = 4, S = 6, A = 3;
    static constexpr const char *kName = "Acrobot";
    static __device__ __forceinline__ void load(const RdArgs &g, int64_t row, float (&p)[P], float (&ob)[S])
    {
        const float4 v = *reinterpret_cast<const float4 *>(g.env_state + 4 * row);
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
#pragma unroll
        for (int c = 0; c < 6; c += 2) {    // the policy's input at t = 0 is the live observation as handed in, not observe(p)
            const float2 o = *reinterpret_cast<const float2 *>(g.obs + 6 * row + c);
            ob[c] = o.x; ob[c + 1] = o.y;
        }
    }
    static __device__ __forceinline__ void observe(const float (&p)[P], float (&ob)[S]) { acrobot_observe(p, ob); }
    static __device__ __forceinline__ void store_obs(float *dst, const float (&ob)[S])
    {
#pragma unroll
        for (int c = 0; c < 6; c += 2) *reinterpret_cast<float2 *>(dst + c) = make_float2(ob[c], ob[c + 1]);
    }
    static __device__ __forceinline__ void store(const RdArgs &g, int64_t row, const float (&p)[P], const float (&ob)[S])
    {
        *reinterpret_cast<float4 *>(g.env_state + 4 * row) = make_float4(p[0], p[1], p[2], p[3]);
        store_obs(g.obs + 6 * row, ob);
    }
    static __device__ __forceinline__ float step(float (&p)[P], int act, int &sc, int &ep, int max_step, uint64_t seed, uint32_t env,
                                                 bool &term, bool &trunc)
    {
        return acrobot_step(p, act, sc, ep, max_step, seed, env, term, trunc);
    }
};

template <typename Env, bool EV_>
__global__ __launch_bounds__(256) void rollout_discrete_kernel(RdArgs g)
{
    static_assert(Env::S >= 1 && Env::S <= 16, "the observation is one k-tile of layer 1");
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
    Env::load(g, row, s, ob);
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
        f32x4 x[8], ha[8], hb[8], z[8], gd[8];
        float xn[S];
#pragma unroll
        for (int c = 0; c < S; ++c) xn[c] = (ob[c] - avg[c]) / den[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = own ? xn[c] : 0.f;
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
        Env::store(g, row, s, ob);
        if (g.o_last_state) Env::store_obs(g.o_last_state + S * row, ob);
        g.step_count[row] = sc;
        g.episode[row] = ep;
        if constexpr (EV_) g.ev_cnt[row] = ev_n;
    }
}

template <typename Env, bool EV_>
int rd_launch(const RdArgs &g, const char *what, hipStream_t stream)
{
    // one wave per workgroup while that is at most one workgroup per CU of a 256-CU device, up to four waves beyond
    const int64_t tiles = erl_cdiv(g.N, 16);
    int waves = (int)erl_cdiv(tiles, 256);
    waves = waves < 1 ? 1 : (waves > 4 ? 4 : waves);
    const size_t lds = rd_lds_floats(g.h1, g.h2, waves) * sizeof(float);
    ERL_REQUIRE(lds <= 160 * 1024, "%s: %zu bytes of LDS", what, lds);
    if (lds > 48 * 1024) {                  // asked at every such launch (a host-side call): no cache to keep per device and per thread
        int rc = erl_hip_status(hipFuncSetAttribute((const void *)rollout_discrete_kernel<Env, EV_>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)lds), "hipFuncSetAttribute(rollout_discrete_kernel)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL((rollout_discrete_kernel<Env, EV_>), dim3((unsigned)erl_cdiv(tiles, waves)), dim3(64 * waves), lds, stream, g);
    return erl_hip_status(hipGetLastError(), what);
}

template <typename Env>
int rd_fill(RdArgs &g, const char *what, const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2, int A,
            float *env_state, float *obs, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed, int64_t N, int64_t H)
{
    ERL_REQUIRE(actor_params && act_avg && act_std && env_state && obs && step_count && episode, "%s: NULL tensor", what);
    ERL_REQUIRE(rd_dims_ok(S, h1, h2, A), "%s: unsupported dims S=%d net=[%d,%d] A=%d (one-launch discrete rollout: state_dim <= 64, 2 hidden "
                "layers of 32..128 in steps of 32, 2 <= action_dim <= %d)", what, S, h1, h2, A, RD_MAX_A);
    ERL_REQUIRE(S == Env::S, "%s: bad environment argument: %s's state_dim is %d, not %d", what, Env::kName, Env::S, S);
    ERL_REQUIRE(Env::A == 0 || A == Env::A, "%s: bad environment argument: %s's action_dim is %d, not %d", what, Env::kName, Env::A, A);
    ERL_REQUIRE(N >= 1 && H >= 1 && H < (1LL << 30) && N <= ((1LL << 31) - 1) / H && max_step >= 1, "%s: bad shape N=%lld H=%lld max_step=%d", what,
                (long long)N, (long long)H, max_step);
    g.P = actor_params; g.avg = act_avg; g.std = act_std;
    g.h1 = h1; g.h2 = h2; g.A = A; g.N = N; g.H = (int)H;
    g.env_state = env_state; g.obs = obs; g.step_count = step_count; g.episode = episode; g.max_step = max_step; g.env_seed = env_seed;
    return ERL_OK;
}

}  // namespace

extern "C" int erl_rollout_discrete_supported(int S, int h1, int h2, int A) { return rd_dims_ok(S, h1, h2, A) ? 1 : 0; }

extern "C" int erl_cartpole_step_f32(float *state, const int64_t *action, int32_t *step_count, int32_t *episode, float *reward,
                                     uint8_t *terminal, uint8_t *truncate, int64_t N, int max_step, uint64_t seed, void *stream)
{
    ERL_REQUIRE(state && action && step_count && episode && reward && terminal && truncate, "erl_cartpole_step_f32: NULL tensor");
    ERL_REQUIRE(N >= 1 && N < (1LL << 31) && max_step >= 1, "erl_cartpole_step_f32: bad shape N=%lld max_step=%d", (long long)N, max_step);
    hipLaunchKernelGGL(cartpole_step_kernel, dim3((unsigned)erl_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, state, action, step_count,
                       episode, reward, terminal, truncate, N, max_step, seed);
    ERL_LAUNCH_CHECK("erl_cartpole_step_f32");
}

extern "C" int erl_rollout_discrete_cartpole_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2,
                                                 int A, float *env_state, int32_t *step_count, int32_t *episode, int max_step,
                                                 uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                 uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                 float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                 float *out_last_state, float *out_uniform, void *stream)
{
    const char *what = "erl_rollout_discrete_cartpole_f32";
    ERL_REQUIRE(out_states && out_actions && out_logprobs && out_rewards && out_undones && out_unmasks, "%s: NULL tensor", what);
    RdArgs g{};
    int rc = rd_fill<CartPoleEnv>(g, what, actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step,
                                  env_seed, N, H);
    if (rc) return rc;
    g.uniform = uniform; g.seed = seed; g.counter0 = counter0; g.reward_scale = reward_scale;
    g.o_states = out_states; g.o_actions = out_actions; g.o_logprobs = out_logprobs; g.o_rewards = out_rewards;
    g.o_undones = out_undones; g.o_unmasks = out_unmasks; g.o_last_state = out_last_state; g.o_uniform = out_uniform;
    return rd_launch<CartPoleEnv, false>(g, what, (hipStream_t)stream);
}

extern "C" int erl_eval_discrete_cartpole_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2, int A,
                                              float *env_state, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed,
                                              int64_t N, int64_t H, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *what = "erl_eval_discrete_cartpole_f32";
    ERL_REQUIRE(workspace, "%s: NULL tensor (workspace)", what);
    RdArgs g{};
    int rc = rd_fill<CartPoleEnv>(g, what, actor_params, act_avg, act_std, S, h1, h2, A, env_state, env_state, step_count, episode, max_step,
                                  env_seed, N, H);
    if (rc) return rc;
    ERL_REQUIRE(erl_eval_ws_bytes(N, H) > 0 && workspace_bytes >= erl_eval_ws_bytes(N, H),
                "%s: workspace of %lld bytes, erl_eval_workspace_bytes(N, H) = %lld", what, (long long)workspace_bytes,
                (long long)erl_eval_ws_bytes(N, H));
    const ErlEvalWs w = erl_eval_ws_layout(workspace, N, H);
    g.ev_rec = w.rec; g.ev_cnt = w.cnt;
    return rd_launch<CartPoleEnv, true>(g, what, (hipStream_t)stream);
}

extern "C" int erl_acrobot_step_f32(float *phys, float *obs, const int64_t *action, int32_t *step_count, int32_t *episode, float *reward,
                                    uint8_t *terminal, uint8_t *truncate, int64_t N, int max_step, uint64_t seed, void *stream)
{
    ERL_REQUIRE(phys && obs && action && step_count && episode && reward && terminal && truncate, "erl_acrobot_step_f32: NULL tensor");
    ERL_REQUIRE(N >= 1 && N < (1LL << 31) && max_step >= 1, "erl_acrobot_step_f32: bad shape N=%lld max_step=%d", (long long)N, max_step);
    hipLaunchKernelGGL(acrobot_step_kernel, dim3((unsigned)erl_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, phys, obs, action,
                       step_count, episode, reward, terminal, truncate, N, max_step, seed);
    ERL_LAUNCH_CHECK("erl_acrobot_step_f32");
}

extern "C" int erl_rollout_discrete_acrobot_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2,
                                                int A, float *phys, float *obs, int32_t *step_count, int32_t *episode, int max_step,
                                                uint64_t env_seed, int64_t N, int64_t H, const float *uniform, uint64_t seed,
                                                uint64_t counter0, float reward_scale, float *out_states, int32_t *out_actions,
                                                float *out_logprobs, float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks,
                                                float *out_last_state, float *out_uniform, void *stream)
{
    const char *what = "erl_rollout_discrete_acrobot_f32";
    ERL_REQUIRE(out_states && out_actions && out_logprobs && out_rewards && out_undones && out_unmasks, "%s: NULL tensor", what);
    RdArgs g{};
    int rc = rd_fill<AcrobotEnv>(g, what, actor_params, act_avg, act_std, S, h1, h2, A, phys, obs, step_count, episode, max_step, env_seed, N, H);
    if (rc) return rc;
    g.uniform = uniform; g.seed = seed; g.counter0 = counter0; g.reward_scale = reward_scale;
    g.o_states = out_states; g.o_actions = out_actions; g.o_logprobs = out_logprobs; g.o_rewards = out_rewards;
    g.o_undones = out_undones; g.o_unmasks = out_unmasks; g.o_last_state = out_last_state; g.o_uniform = out_uniform;
    return rd_launch<AcrobotEnv, false>(g, what, (hipStream_t)stream);
}

extern "C" int erl_eval_discrete_acrobot_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2, int A,
                                             float *phys, float *obs, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed,
                                             int64_t N, int64_t H, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *what = "erl_eval_discrete_acrobot_f32";
    ERL_REQUIRE(workspace, "%s: NULL tensor (workspace)", what);
    RdArgs g{};
    int rc = rd_fill<AcrobotEnv>(g, what, actor_params, act_avg, act_std, S, h1, h2, A, phys, obs, step_count, episode, max_step, env_seed, N, H);
    if (rc) return rc;
    ERL_REQUIRE(erl_eval_ws_bytes(N, H) > 0 && workspace_bytes >= erl_eval_ws_bytes(N, H),
                "%s: workspace of %lld bytes, erl_eval_workspace_bytes(N, H) = %lld", what, (long long)workspace_bytes,
                (long long)erl_eval_ws_bytes(N, H));
    const ErlEvalWs w = erl_eval_ws_layout(workspace, N, H);
    g.ev_rec = w.rec; g.ev_cnt = w.cnt;
    return rd_launch<AcrobotEnv, true>(g, what, (hipStream_t)stream);
}
