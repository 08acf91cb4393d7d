// Persistent H-step rollout for device-resident environments: ONE launch per AgentPPO.explore_env.  gfx950; hidden layers on the
// bf16 matrix pipe (three-way operand split, rollout_bf16.h), output layers and the environment on the fp32 MFMA.
//
// Replaces the whole loop of AgentPPO._explore_vec_env (elegantrl/agents/AgentPPO.py:87-129): for t in range(H):
// ActorPPO.get_action (:368-376), the three buffer stores (:115-117), convert_action_for_env (:388-390), env.step, the
// reward / flag stores (:121-123); then `rewards *= reward_scale` and the two logical_not (:126-128).  It also evaluates
// CriticPPO (:435-441) on every state it visits -- the value pre-pass of update_net (:141-143) and the bootstrap value
// cri(last_state) (:219-220) -- so that update_net finds them ready (same critic weights: nothing trains during a rollout).
//
// Envs are independent, so a workgroup (8 waves) owns a 16-env tile for all H steps; nothing crosses workgroups and there
// is no launch, no weight re-read and no HBM round trip between steps:
//   * wave w holds rows 16 w .. 16 w + 15 of W2 of BOTH networks and of the actor's W1 in registers for the whole rollout, split
//     once into their three bf16 parts (A operands of v_mfma_f32_16x16x32_bf16: 2 x 48 + 24 VGPRs; the layout of the latency-form
//     step kernel, mlp.hip rollout_split_kernel), and its k-slice of the output layers (fp32); the critic's W1 (split), the
//     biases and -- SynVecEnv -- Ws^T / Wa^T sit in LDS, loaded once per launch: 256 registers per lane are all a wave has at two
//     waves per SIMD, and with a fourth weight block in them the step loop spilled;
//   * the state tile lives in LDS (XS, and normalised + split per network: XA / XC); per step: L1 of both nets -> H1 tiles (split) to LDS -> barrier -> L2 + output-layer
//     partials -> LDS -> barrier -> waves < ceil(S/16) finish the policy head in registers (action, log-prob, tanh) and
//     step the env on the matrix cores, wave 7 finishes the value, waves 4..7 draw the next step's N(0,1) (injected or
//     Philox4x32-10) -> barrier (SynVecEnv only) -> done flags, auto-reset, new state tile -> barrier.  Four (Pendulum: three) LDS-only barriers per step; the
//     per-step chain is MFMA-bound (~100 kFLOP per env-step);
//   * every buffer row is written straight from the kernel: states / actions (pre-tanh) / logprobs / rewards (already
//     multiplied by reward_scale) / undones = !terminal / unmasks = !truncate / values, time-major (H, N, .).
// The arithmetic of a step is instruction-for-instruction that of erl_rollout_step_f32's latency form followed by
// erl_synenv_step_f32's tile form (or erl_pendulum_step_f32), so the six rollout buffers are bit-identical to the per-step
// path under the same Philox keys / injected noise (tests/test_rollout_fused_gpu.py).
#include "rollout_fused_impl.h"

namespace {

int rf_launch(RfArgs &g, int env_kind, hipStream_t stream)
{
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = (g.S % 4 == 0) && al(g.Pa) && al(g.Pc) && al(g.o_states);
    const dim3 grid((unsigned)erl_cdiv(g.N, 16)), block(512);
    g.gae_lds = (g.o_adv && g.H <= kRfGaeLdsSteps) ? 1 : 0;
    const size_t lds_bytes = kRfLdsBytes + kRfRsExtraBytes + (g.gae_lds ? rf_gae_lds_bytes(g.H) : 0);
    static bool attr[8] = {false, false, false, false, false, false, false, false};
    // role split (the critic off the step's dependent chain; see the kernel): the default for the tuned shapes, ERL_RF_ROLE_SPLIT=0 keeps
    // every wave on both networks (read per launch: A/B in one process)
    const bool rs = [] { const char *e = getenv("ERL_RF_ROLE_SPLIT"); return !e || atoi(e) != 0; }();
#define RF_LAUNCH(E, V, A_, B_, C_, SLOT)                                                                                  \
    do {                                                                                                                   \
        if (!attr[SLOT]) {                                                                                                 \
            int rc = erl_hip_status(hipFuncSetAttribute((const void *)rollout_fused_kernel<E, V, A_, B_, C_, (SLOT >= 6)>,  \
                                                        hipFuncAttributeMaxDynamicSharedMemorySize,                         \
                                                        (int)(kRfLdsBytes + kRfRsExtraBytes + rf_gae_lds_bytes(kRfGaeLdsSteps))), \
                                    "hipFuncSetAttribute(rollout_fused_kernel)");                                          \
            if (rc) return rc;                                                                                             \
            attr[SLOT] = true;                                                                                             \
        }                                                                                                                  \
        hipLaunchKernelGGL((rollout_fused_kernel<E, V, A_, B_, C_, (SLOT >= 6)>), grid, block, lds_bytes, stream, g);    \
    } while (0)
    switch (rf_shape_class(env_kind, vec, g.S, g.h1, g.h2)) {
    case RF_SYN_TUNED: if (rs) RF_LAUNCH(ENV_SYN, true, 4, 8, 8, 6); else RF_LAUNCH(ENV_SYN, true, 4, 8, 8, 0); break;                // configs 4 / 5
    case RF_SYN_VEC: RF_LAUNCH(ENV_SYN, true, 0, 0, 0, 1); break;
    case RF_SYN_SCALAR: RF_LAUNCH(ENV_SYN, false, 0, 0, 0, 2); break;
    case RF_PENDULUM_TUNED: if (rs) RF_LAUNCH(ENV_PENDULUM, false, 1, 8, 4, 7); else RF_LAUNCH(ENV_PENDULUM, false, 1, 8, 4, 3); break;  // config 2
    case RF_PENDULUM_ANY: RF_LAUNCH(ENV_PENDULUM, false, 0, 0, 0, 4); break;
    case RF_POINT_ANY: RF_LAUNCH(ENV_POINT, false, 0, 0, 0, 5); break;
    }
#undef RF_LAUNCH
    return erl_hip_status(hipGetLastError(), "rollout_fused_kernel launch");
}

// ---- the entries' arguments as the C ABI spells them (include/erl_hip.h), in its order: RfNets, the env (cont_env_args.h), and
struct RfPlanes {                           // the rollout's draws and the planes it writes (out_values / out_next_value may be NULL)
    const float *noise;
    uint64_t seed, counter0;
    float reward_scale;
    float *out_states, *out_actions, *out_logprobs, *out_rewards;
    uint8_t *out_undones, *out_unmasks;
    float *out_values, *out_next_value;
};
struct RfEpilogue {                         // the kernel's optional tail: all may be NULL
    float *out_last_state, *out_advantages, *out_reward_sums;
    double *gae_stats, *gae_workspace;
    int64_t gae_workspace_bytes;
    float gamma, lambda_gae;
    int use_v_trace;
};

// the rollout entries' body
int rf_rollout(const char *what, const RfNets &n, const ContEnv &e, const RfPlanes &o, const RfEpilogue &c, void *stream)
{
    ERL_REQUIRE(n.actor_params && n.critic_params && n.act_avg && n.act_std && n.cri_avg && n.cri_std, "%s: NULL network tensor", what);
    ERL_REQUIRE(o.out_states && o.out_actions && o.out_logprobs && o.out_rewards && o.out_undones && o.out_unmasks, "%s: NULL rollout buffer", what);
    ERL_REQUIRE(rf_dims_ok(n.S, n.h1, n.h2, n.A), "%s: unsupported dims S=%d net=[%d,%d] A=%d (fused rollout: state_dim <= %d, 2 hidden "
                "layers of 32..128 in steps of 32, action_dim <= 16)", what, n.S, n.h1, n.h2, n.A, 16 * RF_NSM);
    ERL_REQUIRE(n.N >= 1 && n.H >= 1 && n.H < (1LL << 30), "%s: bad shape N=%lld H=%lld", what, (long long)n.N, (long long)n.H);
    RfArgs g{};
    g.Pa = n.actor_params; g.Pc = n.critic_params;
    g.avg_a = n.act_avg; g.std_a = n.act_std; g.avg_c = n.cri_avg; g.std_c = n.cri_std;
    g.S = n.S; g.h1 = n.h1; g.h2 = n.h2; g.A = n.A; g.N = n.N; g.H = (int)n.H;
    g.noise = o.noise; g.seed = o.seed; g.counter0 = o.counter0; g.reward_scale = o.reward_scale;
    g.o_states = o.out_states; g.o_actions = o.out_actions; g.o_logprobs = o.out_logprobs; g.o_rewards = o.out_rewards;
    g.o_undones = o.out_undones; g.o_unmasks = o.out_unmasks; g.o_values = o.out_values; g.o_next_value = o.out_next_value;
    g.o_last_state = c.out_last_state;
    if (c.out_advantages || c.out_reward_sums) {
        ERL_REQUIRE(c.out_advantages && c.out_reward_sums && c.gae_workspace && o.out_values && o.out_next_value,
                    "%s: the advantage epilogue needs out_advantages, out_reward_sums, gae_workspace, out_values and out_next_value", what);
        ERL_REQUIRE(c.gae_workspace_bytes >= erl_rollout_gae_workspace_bytes(n.N), "%s: gae_workspace of %lld bytes, erl_rollout_gae_workspace_bytes(N) = %lld",
                    what, (long long)c.gae_workspace_bytes, (long long)erl_rollout_gae_workspace_bytes(n.N));
    }
    g.o_adv = c.out_advantages; g.o_ret = c.out_reward_sums; g.gae_stats = c.gae_stats; g.gae_ws = c.gae_workspace;
    g.gamma = c.gamma; g.lam = c.lambda_gae; g.vtrace = c.use_v_trace ? 1 : 0;
#ifdef ERL_PROFILE
    g.prof = g_rf_prof;
#endif
    if (int rc = cont_env_check(what, e, true)) return rc;
    rf_set_env(g, e);
    return rf_launch(g, e.kind, (hipStream_t)stream);
}

}  // namespace

#ifdef ERL_PROFILE
// profiling builds only (make EXTRA=-DERL_PROFILE): device buffer of 8 * 16 int64 cycle stamps
extern "C" __attribute__((visibility("default"))) void erl_debug_set_rollout_fused_profile(long long *dev_buf) { g_rf_prof = dev_buf; }
#endif

extern "C" int erl_rollout_fused_supported(int S, int h1, int h2, int A) { return rf_dims_ok(S, h1, h2, A) ? 1 : 0; }

// bytes of `gae_workspace` of the persistent rollouts for N envs: 3 fp64 partial sums per 16-env workgroup (erl_rollout_gae_partials of them)
extern "C" int64_t erl_rollout_gae_workspace_bytes(int64_t N) { return N >= 1 ? 3 * erl_cdiv(N, 16) * 8 : -1; }
extern "C" int erl_rollout_gae_partials(int64_t N) { return N >= 1 ? (int)erl_cdiv(N, 16) : -1; }

extern "C" int erl_rollout_synenv_f32(const float *actor_params, const float *critic_params, const float *act_avg, const float *act_std,
                                      const float *cri_avg, const float *cri_std, int S, int h1, int h2, int A, float *env_state,
                                      const float *Ws, const float *Wa, int32_t *step_count, int32_t *episode, int max_step,
                                      uint64_t env_seed, int64_t N, int64_t H, const float *noise, uint64_t seed, uint64_t counter0,
                                      float reward_scale, float *out_states, float *out_actions, float *out_logprobs,
                                      float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks, float *out_values,
                                      float *out_next_value, float *out_last_state, float *out_advantages, float *out_reward_sums,
                                      double *gae_stats, double *gae_workspace, int64_t gae_workspace_bytes, float gamma,
                                      float lambda_gae, int use_v_trace, void *stream)
{
    return rf_rollout("erl_rollout_synenv_f32", {actor_params, critic_params, act_avg, act_std, cri_avg, cri_std, S, h1, h2, A, N, H},
                      {ENV_SYN, env_state, nullptr, Ws, Wa, step_count, episode, max_step, env_seed},
                      {noise, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks,
                       out_values, out_next_value},
                      {out_last_state, out_advantages, out_reward_sums, gae_stats, gae_workspace, gae_workspace_bytes, gamma, lambda_gae,
                       use_v_trace}, stream);
}

extern "C" int erl_rollout_pendulum_f32(const float *actor_params, const float *critic_params, const float *act_avg,
                                        const float *act_std, const float *cri_avg, const float *cri_std, int h1, int h2, float *phys,
                                        float *obs, int32_t *step_count, int32_t *episode, int max_step, uint64_t env_seed, int64_t N,
                                        int64_t H, const float *noise, uint64_t seed, uint64_t counter0, float reward_scale,
                                        float *out_states, float *out_actions, float *out_logprobs, float *out_rewards,
                                        uint8_t *out_undones, uint8_t *out_unmasks, float *out_values, float *out_next_value,
                                        float *out_last_state, float *out_advantages, float *out_reward_sums, double *gae_stats,
                                        double *gae_workspace, int64_t gae_workspace_bytes, float gamma, float lambda_gae,
                                        int use_v_trace, void *stream)
{
    return rf_rollout("erl_rollout_pendulum_f32", {actor_params, critic_params, act_avg, act_std, cri_avg, cri_std, 3, h1, h2, 1, N, H},
                      {ENV_PENDULUM, obs, phys, nullptr, nullptr, step_count, episode, max_step, env_seed},
                      {noise, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks,
                       out_values, out_next_value},
                      {out_last_state, out_advantages, out_reward_sums, gae_stats, gae_workspace, gae_workspace_bytes, gamma, lambda_gae,
                       use_v_trace}, stream);
}

// ... on the device-resident PointChasingVecEnv (S = 4 A, A = dim in 1..4; state: (N, S) the live observation; distance: (N,) the carried
// |p0 - p1|; pointchasing_step.h's dynamics, operation for operation)
extern "C" int erl_rollout_pointchasing_f32(const float *actor_params, const float *critic_params, const float *act_avg,
                                            const float *act_std, const float *cri_avg, const float *cri_std, int S, int h1, int h2, int A,
                                            float *state, float *distance, int32_t *step_count, int32_t *episode, int max_step,
                                            uint64_t env_seed, int64_t N, int64_t H, const float *noise, uint64_t seed, uint64_t counter0,
                                            float reward_scale, float *out_states, float *out_actions, float *out_logprobs,
                                            float *out_rewards, uint8_t *out_undones, uint8_t *out_unmasks, float *out_values,
                                            float *out_next_value, float *out_last_state, float *out_advantages, float *out_reward_sums,
                                            double *gae_stats, double *gae_workspace, int64_t gae_workspace_bytes, float gamma,
                                            float lambda_gae, int use_v_trace, void *stream)
{
    if (int rc = cont_env_point_dims("erl_rollout_pointchasing_f32", S, A)) return rc;
    return rf_rollout("erl_rollout_pointchasing_f32", {actor_params, critic_params, act_avg, act_std, cri_avg, cri_std, S, h1, h2, A, N, H},
                      {ENV_POINT, state, distance, nullptr, nullptr, step_count, episode, max_step, env_seed},
                      {noise, seed, counter0, reward_scale, out_states, out_actions, out_logprobs, out_rewards, out_undones, out_unmasks,
                       out_values, out_next_value},
                      {out_last_state, out_advantages, out_reward_sums, gae_stats, gae_workspace, gae_workspace_bytes, gamma, lambda_gae,
                       use_v_trace}, stream);
}
