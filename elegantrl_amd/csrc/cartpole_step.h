// One CartPole-v1 step of one env (gymnasium's physics as CartPoleVecEnv.step states them: gravity 9.8, cart 1.0 kg, pole 0.1 kg,
// half-length 0.5 m, force +-10 N, dt 0.02 s, Euler), shared by the per-step kernel (erl_cartpole_step_f32) and the one-launch
// discrete rollout / evaluation (rollout_discrete.hip).  Every product and sum is rounded on its own (contraction off below, and
// the translation unit is built with -ffp-contract=off), so that the two inlined copies agree bit for bit whatever surrounds them.
#pragma once
#include "erl_common.h"

namespace {

constexpr float kCartPoleXLimit = 2.4f;
constexpr float kCartPoleThetaLimit = 0.20943951023931953f;        // 12 * 2 pi / 360

// component c of the state an env starts episode `episode` with: U[-0.05, 0.05), keyed by (env seed, env, episode, component) --
// a draw depends neither on the launch geometry nor on which kernel performs it
__device__ __forceinline__ void cartpole_reset_draw(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[4])
{
#pragma clang fp contract(off)
    const Philox4 p = philox4x32_10(env, 0x43415254u, episode, 0x504f4c45u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = (float)(w[c] >> 8) * (1.0f / 16777216.0f) * 0.1f - 0.05f;
}

// s: (x, x_dot, theta, theta_dot) in, the next state -- or the reset draw where the step ends the episode -- out; any action other
// than 1 pushes left; terminal is tested on the new state, truncate = step_count reached max_step and not terminal; reward is 1.
__device__ __forceinline__ void cartpole_step(float (&s)[4], int action, int &step_count, int &episode, int max_step, uint64_t seed,
                                              uint32_t env, bool &terminal, bool &truncate)
{
#pragma clang fp contract(off)
    const float x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
    const float force = action == 1 ? 10.0f : -10.0f;
    const float c = cosf(theta), sn = sinf(theta);
    const float temp = (force + 0.05f * theta_dot * theta_dot * sn) / 1.1f;          // polemass_length = 0.05, total mass 1.1
    const float theta_acc = (9.8f * sn - c * temp) / (0.5f * (4.0f / 3.0f - 0.1f * c * c / 1.1f));
    const float x_acc = temp - 0.05f * theta_acc * c / 1.1f;
    s[0] = x + 0.02f * x_dot;
    s[1] = x_dot + 0.02f * x_acc;
    s[2] = theta + 0.02f * theta_dot;
    s[3] = theta_dot + 0.02f * theta_acc;
    const int sc = step_count + 1;
    terminal = fabsf(s[0]) > kCartPoleXLimit || fabsf(s[2]) > kCartPoleThetaLimit;
    truncate = sc >= max_step && !terminal;
    const bool done = terminal || truncate;
    if (done) {
        episode += 1;
        cartpole_reset_draw(seed, env, (uint32_t)episode, s);
    }
    step_count = done ? 0 : sc;
}

}  // namespace
