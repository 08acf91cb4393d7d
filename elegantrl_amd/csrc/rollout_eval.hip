// Policy evaluation on the device: the Evaluator's episodes (elegantrl/train/evaluator.py:201-238) in two launches.
//
//   1. the EVALUATION FORM of the persistent PPO rollout (rollout_fused_impl.h, EV_): `H` steps of the deterministic policy
//      tanh(mean) on a device-resident env.  The policy mean and the env step are the training rollout's statements, so what the
//      env sees is, bit for bit, what AgentPPO._explore_vec_env leaves under an all-zero injected noise and reward_scale = 1.  Left
//      out: the critic (every wave runs the actor; no role split), the N(0,1) draws, the log-prob, every rollout buffer row, the
//      reward scale, the bootstrap pass and the advantage epilogue.  Kept instead, by the lane that owns the env's reward: a running
//      return (the fp32 rewards summed in fp64, in time order), a running length and the number of finished episodes.  Where a step is
//      done (terminal | truncate) the lane writes (float(return), length) at record (t, env) and clears both; elsewhere it writes
//      (0, 0): every record is written, nothing has to be cleared first.  An episode still open after the last step leaves no record.
//   2. the COMPACTION (eval_compact_kernel, also behind the SAC evaluation of sac_fused.hip): records + per-env counts -> the
//      (n_episodes, 2) table in the reference's order, env-major and in time order inside an env.  Workgroup b owns envs
//      256 b .. 256 b + 255: it sums the counts of every earlier env (the exclusive prefix at its first env; N ints at most, from
//      L2: N^2 / 512 loads over the launch, nothing at the 4096 .. 65536 envs the rollouts run at -- include/erl_hip.h), scans its own 256 counts in LDS, then every thread walks its env's column (one record per thread and step: a wave reads
//      512 contiguous bytes) and writes its rows.  The last workgroup stores the total.  Plain vector loads and stores; no atomics, no
//      second pass, no workgroup waits for another.
#include "eval_ws.h"
#include "rollout_fused_impl.h"

namespace {

int rf_eval_launch(RfArgs &g, int env_kind, hipStream_t stream)
{
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = (g.S % 4 == 0) && al(g.Pa);
    const dim3 grid((unsigned)erl_cdiv(g.N, 16)), block(512);
    const size_t lds_bytes = kRfLdsBytes;
    static bool attr[6] = {false, false, false, false, false, false};
#define RF_EVAL_LAUNCH(E, V, A_, B_, C_, SLOT)                                                                             \
    do {                                                                                                                   \
        if (!attr[SLOT]) {                                                                                                 \
            int rc = erl_hip_status(hipFuncSetAttribute((const void *)rollout_fused_kernel<E, V, A_, B_, C_, false, true>, \
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRfLdsBytes),     \
                                    "hipFuncSetAttribute(rollout_fused_kernel, evaluation form)");                         \
            if (rc) return rc;                                                                                             \
            attr[SLOT] = true;                                                                                             \
        }                                                                                                                  \
        hipLaunchKernelGGL((rollout_fused_kernel<E, V, A_, B_, C_, false, true>), grid, block, lds_bytes, stream, g);      \
    } while (0)
    switch (rf_shape_class(env_kind, vec, g.S, g.h1, g.h2)) {       // the training launcher's classes (no role split here)
    case RF_SYN_TUNED: RF_EVAL_LAUNCH(ENV_SYN, true, 4, 8, 8, 0); break;                                  // configs 4 / 5
    case RF_SYN_VEC: RF_EVAL_LAUNCH(ENV_SYN, true, 0, 0, 0, 1); break;
    case RF_SYN_SCALAR: RF_EVAL_LAUNCH(ENV_SYN, false, 0, 0, 0, 2); break;
    case RF_PENDULUM_TUNED: RF_EVAL_LAUNCH(ENV_PENDULUM, false, 1, 8, 4, 3); break;                       // config 2
    case RF_PENDULUM_ANY: RF_EVAL_LAUNCH(ENV_PENDULUM, false, 0, 0, 0, 4); break;
    case RF_POINT_ANY: RF_EVAL_LAUNCH(ENV_POINT, false, 0, 0, 0, 5); break;
    }
#undef RF_EVAL_LAUNCH
    return erl_hip_status(hipGetLastError(), "rollout_fused_kernel (evaluation form) launch");
}

// the evaluation entries' body (of RfNets the critic's three are not read)
int rf_eval(const char *what, const RfNets &n, const ContEnv &e, void *workspace, int64_t workspace_bytes, void *stream)
{
    ERL_REQUIRE(n.actor_params && n.act_avg && n.act_std, "%s: NULL network tensor", what);
    ERL_REQUIRE(workspace, "%s: NULL workspace", what);
    ERL_REQUIRE(rf_dims_ok(n.S, n.h1, n.h2, n.A), "%s: unsupported dims S=%d net=[%d,%d] A=%d (fused rollout: state_dim <= %d, 2 hidden "
                "layers of 32..128 in steps of 32, action_dim <= 16)", what, n.S, n.h1, n.h2, n.A, 16 * RF_NSM);
    ERL_REQUIRE(n.N >= 1 && n.H >= 1 && n.H < (1LL << 30) && erl_eval_ws_bytes(n.N, n.H) > 0, "%s: bad shape N=%lld H=%lld", what, (long long)n.N,
                (long long)n.H);
    ERL_REQUIRE(workspace_bytes >= erl_eval_ws_bytes(n.N, n.H), "%s: workspace of %lld bytes, erl_eval_workspace_bytes(N, H) = %lld", what,
                (long long)workspace_bytes, (long long)erl_eval_ws_bytes(n.N, n.H));
    RfArgs g{};
    g.Pa = n.actor_params; g.avg_a = n.act_avg; g.std_a = n.act_std;
    g.S = n.S; g.h1 = n.h1; g.h2 = n.h2; g.A = n.A; g.N = n.N; g.H = (int)n.H;
    g.reward_scale = 1.0f;
    const ErlEvalWs w = erl_eval_ws_layout(workspace, n.N, n.H);
    g.ev_rec = w.rec; g.ev_cnt = w.cnt;
    if (int rc = cont_env_check(what, e, true)) return rc;
    rf_set_env(g, e);
    return rf_eval_launch(g, e.kind, (hipStream_t)stream);
}

constexpr int EC_T = 256;      // threads = envs per workgroup of the compaction
constexpr int EC_U = 16;       // records in flight per thread

__global__ __launch_bounds__(EC_T) void eval_compact_kernel(const float2 *__restrict__ rec, const int32_t *__restrict__ cnt, int64_t N, int H,
                                                            float2 *__restrict__ out, int64_t capacity, int32_t *__restrict__ total)
{
    __shared__ long long red[EC_T];
    __shared__ int scan[EC_T];
    const int tid = threadIdx.x;
    const int64_t env0 = (int64_t)blockIdx.x * EC_T, env = env0 + tid;
    // rows of every earlier env
    long long before = 0;
    for (int64_t i = tid; i < env0; i += EC_T) before += cnt[i];
    red[tid] = before;
    const int mine = env < N ? cnt[env] : 0;
    scan[tid] = mine;
    __syncthreads();
    for (int s = EC_T / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    for (int s = 1; s < EC_T; s <<= 1) {                  // inclusive scan of the workgroup's counts
        const int v = tid >= s ? scan[tid - s] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const long long base = red[0];
    long long pos = base + scan[tid] - mine;
    if (blockIdx.x == gridDim.x - 1 && tid == EC_T - 1) *total = (int32_t)(base + scan[tid]);
    if (env >= N || mine == 0) return;
    for (int t0 = 0; t0 < H; t0 += EC_U) {
        float2 r[EC_U];
#pragma unroll
        for (int j = 0; j < EC_U; ++j) r[j] = rec[(size_t)min(t0 + j, H - 1) * (size_t)N + env];
#pragma unroll
        for (int j = 0; j < EC_U; ++j) {
            if (t0 + j < H && r[j].y > 0.f) {
                if (pos < capacity) out[pos] = r[j];
                ++pos;
            }
        }
    }
}

}  // namespace

extern "C" int64_t erl_eval_workspace_bytes(int64_t N, int64_t H) { return erl_eval_ws_bytes(N, H); }

extern "C" int erl_eval_synenv_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2, int A,
                                   float *env_state, const float *Ws, const float *Wa, int32_t *step_count, int32_t *episode, int max_step,
                                   uint64_t env_seed, int64_t N, int64_t H, void *workspace, int64_t workspace_bytes, void *stream)
{
    return rf_eval("erl_eval_synenv_f32", {actor_params, nullptr, act_avg, act_std, nullptr, nullptr, S, h1, h2, A, N, H},
                   {ENV_SYN, env_state, nullptr, Ws, Wa, step_count, episode, max_step, env_seed}, workspace, workspace_bytes, stream);
}

extern "C" int erl_eval_pendulum_f32(const float *actor_params, const float *act_avg, const float *act_std, int h1, int h2, float *phys,
                                     float *obs, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed, int64_t N, int64_t H,
                                     void *workspace, int64_t workspace_bytes, void *stream)
{
    return rf_eval("erl_eval_pendulum_f32", {actor_params, nullptr, act_avg, act_std, nullptr, nullptr, 3, h1, h2, 1, N, H},
                   {ENV_PENDULUM, obs, phys, nullptr, nullptr, step_count, episode, max_step, env_seed}, workspace, workspace_bytes, stream);
}

extern "C" int erl_eval_pointchasing_f32(const float *actor_params, const float *act_avg, const float *act_std, int S, int h1, int h2, int A,
                                         float *state, float *distance, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed,
                                         int64_t N, int64_t H, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = cont_env_point_dims("erl_eval_pointchasing_f32", S, A)) return rc;
    return rf_eval("erl_eval_pointchasing_f32", {actor_params, nullptr, act_avg, act_std, nullptr, nullptr, S, h1, h2, A, N, H},
                   {ENV_POINT, state, distance, nullptr, nullptr, step_count, episode, max_step, env_seed}, workspace, workspace_bytes, stream);
}

extern "C" int erl_eval_episodes_compact_f32(const void *workspace, int64_t workspace_bytes, int64_t N, int64_t H, float *out_rows,
                                             int64_t out_capacity, int32_t *out_count, void *stream)
{
    ERL_REQUIRE(workspace && out_rows && out_count, "erl_eval_episodes_compact_f32: NULL argument");
    ERL_REQUIRE(N >= 1 && H >= 1 && H < (1LL << 30) && erl_eval_ws_bytes(N, H) > 0 && out_capacity >= 0,
                "erl_eval_episodes_compact_f32: bad shape N=%lld H=%lld out_capacity=%lld", (long long)N, (long long)H, (long long)out_capacity);
    ERL_REQUIRE(workspace_bytes >= erl_eval_ws_bytes(N, H), "erl_eval_episodes_compact_f32: workspace of %lld bytes, erl_eval_workspace_bytes(N, H) = %lld",
                (long long)workspace_bytes, (long long)erl_eval_ws_bytes(N, H));
    const ErlEvalWs w = erl_eval_ws_layout(const_cast<void *>(workspace), N, H);
    hipLaunchKernelGGL(eval_compact_kernel, dim3((unsigned)erl_cdiv(N, EC_T)), dim3(EC_T), 0, (hipStream_t)stream, w.rec, w.cnt, N, (int)H,
                       reinterpret_cast<float2 *>(out_rows), out_capacity, out_count);
    ERL_LAUNCH_CHECK("erl_eval_episodes_compact_f32");
}
