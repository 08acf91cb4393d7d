// TD3 / DDPG update step and exploration action (elegantrl/agents/AgentTD3.py:15-87, AgentBase.py:191-224).  gfx950.
//
// The deterministic off-policy pair on the layered path: Actor = build_mlp([S, *net_dims, A]) with tanh on top, CriticTwin = ONE
// build_mlp([S + A, *net_dims, E]) whose last layer is E heads wide (Critic: E = 1).  Every dense layer is one of the launches
// sac_step_layered uses (mlpn_common.h forward / backward, gemm_tiles.h dense_backward_input): the critic is a single MLP, so there is no
// per-decoder loop.  What is new here are the five row-wise kernels between them, the step that strings them together and the loop that
// runs AgentBase.update_net (:172-189) from one C call.
//
// One step (AgentTD3.update_objectives :34-70):
//   next_action = clip(tanh(act(next_state)) + policy_noise_std * N(0, 1), -1, 1)       the CURRENT actor; the action is clipped, the noise is not
//   q_label     = reward + undone * gamma * min_e cri_target(next_state, next_action)
//   td_error    = mean_e criterion(q_e, q_label) * unmask;   obj_critic = mean_b (td_error [* is_weight])
//   critic: clip + Adam, then soft_update(cri_target, cri)
//   when the actor is updated:  obj_actor = mean_{b, e} cri(state, tanh(act(state)))   -- the critic AFTER its step
//                               actor: clip + Adam on -obj_actor, then soft_update(act_target, act)
//   else obj_actor = nan and the actor, its target and its Adam state stay as they are
// AgentDDPG is the same step with E = 1 and policy_noise_std = 0.
//
// D1 (DDPG only).  AgentBase.update_objectives (:206-207) multiplies a (B, 1) q by a (B,) unmask and compares the (B, B) result with a
// (B,) label, so its "batch mean" runs over B^2 mismatched pairs.  This file implements the per-sample reading,
// criterion(q_i, label_i) * unmask_i: TD3's formula with E = 1.
//
// Parameter blocks (flat fp32, the order of the reference's state_dict):  W0 b0 W1 b1 ... for the actor and for the critic.
#include <math.h>
#include <stdlib.h>

#include "mlpn_common.h"

namespace {

constexpr int TD3_MAXE = 8;

struct Td3Dims {
    int S, A, E;
    NetDims actor, critic;
};

bool make_td3_dims(int S, int A, const int *hidden, int n_hidden, int E, Td3Dims *d)
{
    if (S < 1 || A < 1 || !hidden || n_hidden < 1 || n_hidden > MAXL || E < 1 || E > TD3_MAXE) return false;
    int dims[MAXL + 2];
    dims[0] = S;
    for (int i = 0; i < n_hidden; ++i) dims[i + 1] = hidden[i];
    dims[n_hidden + 1] = A;
    if (!make_dims(dims, n_hidden + 2, false, &d->actor)) return false;
    dims[0] = S + A;
    dims[n_hidden + 1] = E;
    if (!make_dims(dims, n_hidden + 2, false, &d->critic)) return false;
    d->S = S; d->A = A; d->E = E;
    return true;
}

int td3_maxd(const Td3Dims &d)
{
    int m = d.S + d.A;
    for (int l = 1; l <= d.actor.n; ++l) m = d.actor.d[l] > m ? d.actor.d[l] : m;
    return d.E > m ? d.E : m;
}

// Actor.get_action (AgentTD3.py:132-136) on the actor's raw output Y (B, A): action = clip(tanh(y) + std * eps, -1, 1), eps injected or
// Philox keyed by (seed, counter, row, component).  std = 0 is Actor.forward (DDPG's next action, the policy-gradient action): plain tanh.
// xa != NULL: the row [xs | action] of the critic's input is written here (no concat launch); act_out / state_out: the rollout's rows.
__global__ __launch_bounds__(256) void td3_action_kernel(const float *__restrict__ Y, const float *__restrict__ noise, uint64_t seed,
                                                         uint64_t counter, float std, int S, int A, int64_t B, const float *__restrict__ xs,
                                                         float *__restrict__ xa, float *__restrict__ act_out, float *__restrict__ state_out)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int W = S + A;
    if (xa || state_out)
        for (int c = 0; c < S; ++c) {
            const float v = xs[b * S + c];
            if (xa) xa[b * W + c] = v;
            if (state_out) state_out[b * S + c] = v;
        }
    for (int a = 0; a < A; ++a) {
        float t = tanhf(Y[b * A + a]);
        if (std != 0.f) {
            const float eps = noise ? noise[b * A + a] : philox_normal(seed, counter, (uint32_t)b, (uint32_t)a);
            t = fminf(fmaxf(t + std * eps, -1.f), 1.f);
        }
        if (xa) xa[b * W + S + a] = t;
        if (act_out) act_out[b * A + a] = t;
    }
}

// q_label = reward + undone * gamma * min_e q_target[b][e] (AgentTD3.py:45-47) from the (B, E) rows of the target critic; the same thread
// then stages the critic's next input row [state | action] over the one the target critic has just read
__global__ __launch_bounds__(256) void td3_label_kernel(const float *__restrict__ qt, int E, int64_t B, const float *__restrict__ reward,
                                                        const float *__restrict__ undone, float gamma, float *__restrict__ label,
                                                        const float *__restrict__ state, const float *__restrict__ action, int S, int A,
                                                        float *__restrict__ xa)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float m = qt[b * E];
    for (int e = 1; e < E; ++e) m = fminf(m, qt[b * E + e]);
    label[b] = reward[b] + (undone[b] * gamma) * m;
    const int W = S + A;
    for (int c = 0; c < S; ++c) xa[b * W + c] = state[b * S + c];
    for (int a = 0; a < A; ++a) xa[b * W + S + a] = action[b * A + a];
}

// critic objective (AgentTD3.py:49-56; D1 above for E = 1): td = mean_e l(q_e - label) * unmask, obj = mean_b (td w),
// dq[b][e] = l'(q_e - label) unmask w / (E B); l, l' from critic_loss.h, the MSE arm spelled out as in sac.hip.  part[block] = the block's
// sum of td w, folded by td3_fold_kernel in a fixed order.
__global__ __launch_bounds__(256) void td3_critic_obj_kernel(const float *__restrict__ q, const float *__restrict__ label,
                                                             const float *__restrict__ unmask, const float *__restrict__ is_weight, int E,
                                                             int64_t B, float *__restrict__ dq, float *__restrict__ td_out,
                                                             float *__restrict__ part, int crit_kind, float crit_beta)
{
    __shared__ float red[4];
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float td = 0.f;
    if (b < B) {
        const float l = label[b], um = unmask[b], w = is_weight ? is_weight[b] : 1.f;
        float s = 0.f;
        for (int e = 0; e < E; ++e) {
            const float diff = q[b * E + e] - l;
            float d;
            if (crit_kind == ERL_CRIT_MSE) {
                s += diff * diff;
                d = 2.f * diff * um * w / ((float)E * (float)B);
            } else {
                s += critic_loss(crit_kind, crit_beta, diff);
                d = critic_loss_grad(crit_kind, crit_beta, diff) * um * w / ((float)E * (float)B);
            }
            dq[b * E + e] = d;
        }
        td = (s / (float)E) * um;
        if (td_out) td_out[b] = td;
        td *= w;
    }
    const float t = block_sum(td, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// out = scale * sum_i part[i]: one block, thread i takes every 256th partial, block_sum's fixed order finishes (bit-reproducible)
__global__ __launch_bounds__(256) void td3_fold_kernel(const float *__restrict__ part, int64_t n, float scale, float *__restrict__ out)
{
    __shared__ float red[4];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += part[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = t * scale;
}

// actor objective (AgentTD3.py:64-66): obj_actor = mean over heads and batch of q (B, E) -> out (block 0, fixed order), and the gradient
// of -obj_actor with respect to every q, -1 / (E B), into dq (all blocks)
__global__ __launch_bounds__(256) void td3_actor_obj_kernel(const float *__restrict__ q, int64_t n, float *__restrict__ out,
                                                            float *__restrict__ dq)
{
    __shared__ float red[4];
    const float g = -1.0f / (float)n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dq[i] = g;
    if (blockIdx.x != 0) return;
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += q[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = t / (float)n;
}

// dL/d(actor output) = dL/daction * tanh'(y): the action columns of the critic's input gradient dxa (row stride S + A), read in place,
// times 1 - t^2 with t the tanh the forward left in the action columns of xa
__global__ __launch_bounds__(256) void td3_tanh_backward_kernel(const float *__restrict__ dxa, const float *__restrict__ xa, int S, int A,
                                                                int64_t B, float *__restrict__ dY)
{
    const int64_t total = B * A;
    const int W = S + A;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / A;
        const int a = (int)(e - b * A);
        const float t = xa[b * W + S + a];
        dY[e] = dxa[b * W + S + a] * (1.f - t * t);
    }
}

__global__ void td3_set_kernel(float *p, float v)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) p[0] = v;
}

int64_t td3_ws_floats(const Td3Dims &d, int64_t B)
{
    const int maxd = td3_maxd(d);
    const int W = d.S + d.A;
    int64_t f = 2 * (B * W + 64);                                                   // xa, dxa
    for (int l = 1; l <= d.actor.n; ++l) f += 2 * (B * d.actor.d[l] + 64);          // actor activations + GELU'
    for (int l = 1; l <= d.critic.n; ++l) f += 2 * (B * d.critic.d[l] + 64);        // critic activations + GELU'
    f += (B + 64) + (B * d.E + 64) + (B * d.A + 64);                                // label, dq, dY
    f += colsum_scratch_floats(B, maxd) + 64;                                       // bias-gradient partials
    f += 2 * (B * maxd + 64);                                                       // tmpA, tmpB
    f += d.actor.count + d.critic.count + 128 + erl_cdiv(B, 256) + 64;              // gradients, the objective's partials
    return f;
}

// what stays the same over an update loop
struct Td3Call {
    float *actor, *critic, *actor_target, *critic_target, *actor_m, *actor_v, *critic_m, *critic_v;
    int S, A;
    const int *hidden;
    int n_hidden, E;
    const float *state, *action, *reward, *undone, *unmask, *next_state;
    int64_t B;
    uint64_t seed;
    float policy_noise_std, gamma, tau, lr, beta1, beta2, eps_adam, max_norm;
    void *workspace;
    int64_t workspace_bytes;
    void *stream;
    int crit_kind;
    float crit_beta;
};
// what changes from step to step
struct Td3Step {
    const ErlRingSample *ring;            // not NULL: the replay sample is the step's first launch
    const float *is_weight;
    float *td_error_out;
    const float *noise;
    uint64_t counter;
    int32_t step;                         // the critic optimiser's Adam step
    bool update_actor;                    // false: the delay rule / DDPG's buffer_init_size gate skips the actor this step
    int32_t actor_step;                   // the actor optimiser's own Adam step (read when update_actor)
    float *objs_out;
};

// everything an entry refuses, refused before its first launch under the entry's own name
int td3_validate(const char *what, const Td3Call &c, const Td3Step &st, bool sample, bool need_ids, Td3Dims *d)
{
    ERL_REQUIRE(c.actor && c.critic && c.actor_target && c.critic_target && c.actor_m && c.actor_v && c.critic_m && c.critic_v && c.state &&
                    c.action && c.reward && c.undone && c.unmask && c.next_state && st.objs_out && c.workspace && c.hidden,
                "%s: NULL tensor", what);
    ERL_REQUIRE(c.E >= 1 && c.E <= TD3_MAXE, "%s: E=%d outside 1..%d", what, c.E, TD3_MAXE);
    ERL_REQUIRE(make_td3_dims(c.S, c.A, c.hidden, c.n_hidden, c.E, d), "%s: unsupported dims", what);
    ERL_REQUIRE(c.B >= 1 && c.B < (1LL << 24) && st.step >= 1 && st.actor_step >= 0 && (!st.update_actor || st.actor_step >= 1),
                "%s: bad argument B=%lld step=%d actor_step=%d update_actor=%d", what, (long long)c.B, (int)st.step, (int)st.actor_step,
                (int)st.update_actor);
    ERL_REQUIRE(c.policy_noise_std >= 0.f && c.policy_noise_std < INFINITY, "%s: policy_noise_std=%g", what, (double)c.policy_noise_std);
    const int64_t need = td3_ws_floats(*d, c.B) * 4 + 8192;
    ERL_REQUIRE(c.workspace_bytes >= need, "%s: workspace too small (%lld bytes, erl_td3_workspace_bytes = %lld)", what,
                (long long)c.workspace_bytes, (long long)need);
    return sample ? erl_ring_refusals(what, st.ring, need_ids, c.S, c.A) : ERL_OK;
}

// One validated step: 10 L + 20 launches when the actor is updated, 5 L + 11 when it is skipped (L hidden layers; + 1 with a ring; each
// clip + Adam entry counted as one) -- DESIGN.md section 4 lists what each reads and writes.
int td3_step(const char *what, const Td3Call &c, const Td3Dims &d, const Td3Step &st)
{
    const int S = c.S, A = c.A, E = c.E, W = S + A;
    const int64_t B = c.B;
    hipStream_t s = (hipStream_t)c.stream;
    int rc;
    if (st.ring && (rc = erl_ring_sample_enqueue(st.ring, S, A, B, c.state, c.action, c.reward, c.undone, c.unmask, c.next_state, c.stream))) return rc;

    Ws ws{(char *)c.workspace, 0, c.workspace_bytes};
    const int maxd = td3_maxd(d);
    float *xa = ws.take(B * W), *dxa = ws.take(B * W);
    float *aact[MAXL + 2], *agd[MAXL + 2], *cact[MAXL + 2], *cgd[MAXL + 2];
    aact[0] = agd[0] = cgd[0] = nullptr;
    cact[0] = xa;
    for (int l = 1; l <= d.actor.n; ++l) {
        aact[l] = ws.take(B * d.actor.d[l]);
        agd[l] = ws.take(B * d.actor.d[l]);
    }
    for (int l = 1; l <= d.critic.n; ++l) {
        cact[l] = ws.take(B * d.critic.d[l]);
        cgd[l] = ws.take(B * d.critic.d[l]);
    }
    float *q = cact[d.critic.n];                                     // (B, E)
    float *label = ws.take(B), *dq = ws.take(B * E), *dY = ws.take(B * A);
    float *cs_scr = ws.take(colsum_scratch_floats(B, maxd));
    float *tmpA = ws.take(B * maxd), *tmpB = ws.take(B * maxd);
    float *g_actor = ws.take(d.actor.count), *g_critic = ws.take(d.critic.count);
    const int nparts = (int)erl_cdiv(B, 256);
    float *part = ws.take(nparts);
    ERL_REQUIRE(part != nullptr, "%s: workspace layout", what);
    const dim3 rows_grid((unsigned)nparts), blk(256);

    // ---- (1) label: next action from the CURRENT actor, min over the heads of the TARGET critic                 (:44-47)
    aact[0] = const_cast<float *>(c.next_state);
    if ((rc = forward(s, d.actor, c.actor, B, aact, nullptr))) return rc;
    hipLaunchKernelGGL(td3_action_kernel, rows_grid, blk, 0, s, aact[d.actor.n], st.noise, c.seed, st.counter, c.policy_noise_std, S, A, B,
                       c.next_state, xa, (float *)nullptr, (float *)nullptr);
    if ((rc = forward(s, d.critic, c.critic_target, B, cact, nullptr))) return rc;
    hipLaunchKernelGGL(td3_label_kernel, rows_grid, blk, 0, s, q, E, B, c.reward, c.undone, c.gamma, label, c.state, c.action, S, A, xa);

    // ---- (2) critic objective, backward, clip + Adam, soft target update                                         (:49-61)
    if ((rc = forward(s, d.critic, c.critic, B, cact, cgd))) return rc;
    hipLaunchKernelGGL(td3_critic_obj_kernel, rows_grid, blk, 0, s, q, label, c.unmask, st.is_weight, E, B, dq, st.td_error_out, part,
                       c.crit_kind, c.crit_beta);
    hipLaunchKernelGGL(td3_fold_kernel, dim3(1), blk, 0, s, part, (int64_t)nparts, 1.0f / (float)B, st.objs_out);
    if ((rc = backward(s, d.critic, c.critic, B, cact, cgd, dq, g_critic, cs_scr, nullptr, false, tmpA, tmpB))) return rc;
    if ((rc = clip_adam_block(c.critic, g_critic, c.critic_m, c.critic_v, d.critic.count, st.step, c.lr, c.beta1, c.beta2, c.eps_adam, c.max_norm,
                              c.stream)))
        return rc;
    hipLaunchKernelGGL(soft_update_kernel, dim3(grid1d(d.critic.count)), blk, 0, s, c.critic_target, c.critic, c.tau, d.critic.count);

    if (!st.update_actor) {                                          // (:68-69) obj_actor = nan; actor, target and moments untouched
        hipLaunchKernelGGL(td3_set_kernel, dim3(1), dim3(64), 0, s, st.objs_out + 1, __builtin_nanf(""));
        ERL_LAUNCH_CHECK(what);
    }

    // ---- (3) actor objective against the CURRENT critic (after its step), backward into the action, tanh', actor   (:63-67)
    aact[0] = const_cast<float *>(c.state);
    if ((rc = forward(s, d.actor, c.actor, B, aact, agd))) return rc;
    hipLaunchKernelGGL(td3_action_kernel, rows_grid, blk, 0, s, aact[d.actor.n], (const float *)nullptr, (uint64_t)0, (uint64_t)0, 0.f, S, A,
                       B, c.state, xa, (float *)nullptr, (float *)nullptr);
    if ((rc = forward(s, d.critic, c.critic, B, cact, cgd))) return rc;
    hipLaunchKernelGGL(td3_actor_obj_kernel, dim3(grid1d(B * E)), blk, 0, s, q, B * E, st.objs_out + 1, dq);
    if ((rc = backward(s, d.critic, c.critic, B, cact, cgd, dq, nullptr, cs_scr, dxa, false, tmpA, tmpB))) return rc;   // dL/d[state | action]
    hipLaunchKernelGGL(td3_tanh_backward_kernel, dim3(grid1d(B * A)), blk, 0, s, dxa, xa, S, A, B, dY);
    if ((rc = backward(s, d.actor, c.actor, B, aact, agd, dY, g_actor, cs_scr, nullptr, false, tmpA, tmpB))) return rc;
    if ((rc = clip_adam_block(c.actor, g_actor, c.actor_m, c.actor_v, d.actor.count, st.actor_step, c.lr, c.beta1, c.beta2, c.eps_adam,
                              c.max_norm, c.stream)))
        return rc;
    hipLaunchKernelGGL(soft_update_kernel, dim3(grid1d(d.actor.count)), blk, 0, s, c.actor_target, c.actor, c.tau, d.actor.count);
    ERL_LAUNCH_CHECK(what);
}

}  // namespace

extern "C" int erl_td3_param_counts(int S, int A, const int *hidden, int n_hidden, int E, int64_t *actor_count, int64_t *critic_count)
{
    ERL_REQUIRE(E >= 1 && E <= TD3_MAXE, "erl_td3_param_counts: E=%d outside 1..%d", E, TD3_MAXE);
    Td3Dims d;
    ERL_REQUIRE(make_td3_dims(S, A, hidden, n_hidden, E, &d), "erl_td3_param_counts: unsupported dims");
    if (actor_count) *actor_count = d.actor.count;
    if (critic_count) *critic_count = d.critic.count;
    return ERL_OK;
}

extern "C" int64_t erl_td3_workspace_bytes(int S, int A, const int *hidden, int n_hidden, int E, int64_t B)
{
    Td3Dims d;
    if (!make_td3_dims(S, A, hidden, n_hidden, E, &d) || B < 1 || B >= (1LL << 31)) return -1;
    return td3_ws_floats(d, B) * 4 + 8192;
}

// Actor.get_action(state, action_std) for a batch of states (AgentBase.explore_action :76-77): the per-step rollout's launch.  state_out
// (N, S), may be NULL: the rollout's `states[t] = state` written by the same launch.  workspace: erl_td3_workspace_bytes(.., E = 1, N).
extern "C" int erl_td3_explore_action_f32(const float *actor_params, int S, int A, const int *hidden, int n_hidden, const float *state,
                                          int64_t N, const float *noise, uint64_t seed, uint64_t counter, float action_std,
                                          float *action_out, float *state_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *const what = "erl_td3_explore_action_f32";
    ERL_REQUIRE(actor_params && state && action_out && workspace && hidden, "%s: NULL tensor", what);
    Td3Dims d;
    ERL_REQUIRE(make_td3_dims(S, A, hidden, n_hidden, 1, &d), "%s: unsupported dims", what);
    ERL_REQUIRE(N >= 1 && N < (1LL << 24), "%s: bad N=%lld", what, (long long)N);
    ERL_REQUIRE(action_std >= 0.f && action_std < INFINITY, "%s: action_std=%g", what, (double)action_std);
    int64_t need = 0;
    for (int l = 1; l <= d.actor.n; ++l) need += (N * d.actor.d[l] + 64) * 4;
    ERL_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%lld bytes, %lld needed; erl_td3_workspace_bytes(.., 1, N) covers it)", what,
                (long long)workspace_bytes, (long long)need);
    Ws ws{(char *)workspace, 0, workspace_bytes};
    float *aact[MAXL + 2];
    aact[0] = const_cast<float *>(state);
    for (int l = 1; l <= d.actor.n; ++l) aact[l] = ws.take(N * d.actor.d[l]);
    ERL_REQUIRE(aact[d.actor.n] != nullptr, "%s: workspace layout", what);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = forward(s, d.actor, actor_params, N, aact, nullptr)) return rc;
    hipLaunchKernelGGL(td3_action_kernel, dim3((unsigned)erl_cdiv(N, 256)), dim3(256), 0, s, aact[d.actor.n], noise, seed, counter, action_std,
                       S, A, N, state, (float *)nullptr, action_out, state_out);
    ERL_LAUNCH_CHECK(what);
}

// the arguments every update entry names alike
#define TD3_CALL                                                                                                                             \
    Td3Call{actor_params, critic_params, actor_target_params, critic_target_params, actor_m, actor_v, critic_m, critic_v, S, A, hidden,     \
            n_hidden, E, state, action, reward, undone, unmask, next_state, B, seed, policy_noise_std, gamma, tau, lr, beta1, beta2,         \
            eps_adam, max_norm, workspace, workspace_bytes, stream, erl_criterion_of_call().kind, erl_criterion_of_call().beta}

// one step on a finished batch (the route of prioritised replay: is_weight in, td_error_out back to the trees; both may be NULL)
extern "C" int erl_td3_update_f32(float *actor_params, float *critic_params, float *actor_target_params, float *critic_target_params,
                                  float *actor_m, float *actor_v, float *critic_m, float *critic_v, int S, int A, const int *hidden,
                                  int n_hidden, int E, const float *state, const float *action, const float *reward, const float *undone,
                                  const float *unmask, const float *next_state, const float *is_weight, float *td_error_out, int64_t B,
                                  const float *noise, uint64_t seed, uint64_t counter, float policy_noise_std, float gamma, float tau,
                                  float lr, float beta1, float beta2, float eps_adam, float max_norm, int32_t step, int32_t update_actor,
                                  int32_t actor_step, float *objs_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *const what = "erl_td3_update_f32";
    ERL_CRITERION_ENTRY("erl_td3_update_f32");
    const Td3Call c = TD3_CALL;
    const Td3Step st{nullptr, is_weight, td_error_out, noise, counter, step, update_actor != 0, actor_step, objs_out};
    Td3Dims d;
    if (int rc = td3_validate(what, c, st, false, true, &d)) return rc;
    return td3_step(what, c, d, st);
}

// ReplayBuffer.sample(ids) + the step from one call: `ring` names the replay ring and the ids, the batch pointers the staging block
extern "C" int erl_td3_update_ring_f32(float *actor_params, float *critic_params, float *actor_target_params, float *critic_target_params,
                                       float *actor_m, float *actor_v, float *critic_m, float *critic_v, int S, int A, const int *hidden,
                                       int n_hidden, int E, const ErlRingSample *ring, float *state, float *action, float *reward,
                                       float *undone, float *unmask, float *next_state, int64_t B, const float *noise, uint64_t seed,
                                       uint64_t counter, float policy_noise_std, float gamma, float tau, float lr, float beta1, float beta2,
                                       float eps_adam, float max_norm, int32_t step, int32_t update_actor, int32_t actor_step,
                                       float *objs_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *const what = "erl_td3_update_ring_f32";
    ERL_CRITERION_ENTRY("erl_td3_update_ring_f32");
    const Td3Call c = TD3_CALL;
    const Td3Step st{ring, nullptr, nullptr, noise, counter, step, update_actor != 0, actor_step, objs_out};
    Td3Dims d;
    if (int rc = td3_validate(what, c, st, true, true, &d)) return rc;
    return td3_step(what, c, d, st);
}

// AgentBase.update_net's loop (:172-189) from ONE call, validated before step 0.  Step t samples with ids_all[t * B ..], counts as critic
// optimiser step step0 + t, keys its noise with counter0 + t and logs into objs_all[2 t ..].  Whether it updates the actor is decided
// here, on the host: actor_gate != 0 (DDPG: buffer.cur_size >= buffer_init_size, :216; TD3: 1) and t % update_freq == 0 (TD3's delay,
// AgentTD3.py:63; DDPG: update_freq = 1).  The actor's Adam count runs on from actor_step0 and advances only on those steps;
// *actor_updates_out (may be NULL) receives their number.
extern "C" int erl_td3_update_ring_loop_f32(float *actor_params, float *critic_params, float *actor_target_params,
                                            float *critic_target_params, float *actor_m, float *actor_v, float *critic_m, float *critic_v,
                                            int S, int A, const int *hidden, int n_hidden, int E, const ErlRingSample *ring,
                                            const int64_t *ids_all, int64_t n_steps, float *state, float *action, float *reward,
                                            float *undone, float *unmask, float *next_state, int64_t B, uint64_t seed, uint64_t counter0,
                                            float policy_noise_std, float gamma, float tau, float lr, float beta1, float beta2,
                                            float eps_adam, float max_norm, int32_t step0, int32_t actor_step0, int32_t update_freq,
                                            int32_t actor_gate, float *objs_all, int32_t *actor_updates_out, void *workspace,
                                            int64_t workspace_bytes, void *stream)
{
    const char *const what = "erl_td3_update_ring_loop_f32";
    ERL_CRITERION_ENTRY("erl_td3_update_ring_loop_f32");
    ERL_REQUIRE(ids_all, "%s: NULL tensor (ids_all)", what);
    ERL_REQUIRE(update_freq >= 1, "%s: update_freq=%d must be >= 1", what, (int)update_freq);
    ERL_REQUIRE(step0 >= 1 && actor_step0 >= 0 && n_steps >= 0 && n_steps < (1LL << 31) - step0 && n_steps < (1LL << 31) - actor_step0,
                "%s: n_steps=%lld step0=%d actor_step0=%d", what, (long long)n_steps, (int)step0, (int)actor_step0);
    const Td3Call c = TD3_CALL;
    Td3Step st{ring, nullptr, nullptr, nullptr, counter0, step0, false, actor_step0, objs_all};
    Td3Dims d;
    if (int rc = td3_validate(what, c, st, true, false, &d)) return rc;
    ErlRingSample r = *ring;
    st.ring = &r;
    int32_t n_upd = 0;
    for (int64_t t = 0; t < n_steps; ++t) {
        st.update_actor = actor_gate != 0 && t % update_freq == 0;
        if (st.update_actor) { ++n_upd; ++st.actor_step; }
        r.ids = ids_all + t * B;
        if (int rc = td3_step(what, c, d, st)) return rc;
        ++st.step;
        ++st.counter;
        st.objs_out += 2;
    }
    if (actor_updates_out) *actor_updates_out = n_upd;
    return ERL_OK;
}
#undef TD3_CALL
