// One Acrobot-v1 step of one env (gymnasium's "book" dynamics: two links of mass 1 and length 1, centres of mass at 0.5, moments of
// inertia 1, g = 9.8, torque action - 1 on the joint between the links, dt 0.2 s, one RK4 step, angles wrapped into [-pi, pi],
// velocities clipped to +-4 pi / +-9 pi), shared by the per-step kernel (erl_acrobot_step_f32) and the one-launch discrete rollout /
// evaluation (rollout_discrete.hip).  Every product and sum is rounded on its own (contraction off below, and the translation unit
// is built with -ffp-contract=off), so that the two inlined copies agree bit for bit whatever surrounds them.
#pragma once
#include "erl_common.h"

namespace {

constexpr float kAcrobotPi = 3.14159265358979323846f;
constexpr float kAcrobotTwoPi = 6.28318530717958647692f;
constexpr float kAcrobotMaxVel1 = 12.566370614359172f;            // 4 pi
constexpr float kAcrobotMaxVel2 = 28.274333882308138f;            // 9 pi
constexpr int kAcrobotMaxWraps = 16;                              // a step from a state inside the limits needs at most a few

// the physical state (theta1, theta2, omega1, omega2) an env starts episode `episode` with: four U[-0.1, 0.1) draws keyed by
// (env seed, env, episode, component) -- a draw depends neither on the launch geometry nor on which kernel performs it
__device__ __forceinline__ void acrobot_reset_draw(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[4])
{
#pragma clang fp contract(off)
    const Philox4 p = philox4x32_10(env, 0x4143524fu, episode, 0x424f5431u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = (float)(w[c] >> 8) * (1.0f / 16777216.0f) * 0.2f - 0.1f;
}

// d/dt of (theta1, theta2, omega1, omega2) under torque a.  With m1 = m2 = l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1:
//   d1 = m1 lc1^2 + m2 (l1^2 + lc2^2 + 2 l1 lc2 cos theta2) + I1 + I2 = 3.5 + cos theta2
//   d2 = m2 (lc2^2 + l1 lc2 cos theta2) + I2 = 1.25 + 0.5 cos theta2
//   phi2 = m2 lc2 g cos(theta1 + theta2 - pi/2) = 4.9 sin(theta1 + theta2)
//   phi1 = -0.5 omega2^2 sin theta2 - omega2 omega1 sin theta2 + 14.7 sin theta1 + phi2
__device__ __forceinline__ void acrobot_dsdt(const float (&s)[4], float a, float (&d)[4])
{
#pragma clang fp contract(off)
    const float th1 = s[0], th2 = s[1], w1 = s[2], w2 = s[3];
    const float c2 = cosf(th2), s2 = sinf(th2);
    const float d1 = 3.5f + c2;
    const float d2 = 1.25f + 0.5f * c2;
    const float phi2 = 4.9f * sinf(th1 + th2);
    const float phi1 = -0.5f * w2 * w2 * s2 - w2 * w1 * s2 + 14.7f * sinf(th1) + phi2;
    const float acc2 = (a + d2 / d1 * phi1 - 0.5f * w1 * w1 * s2 - phi2) / (1.25f - d2 * d2 / d1);
    const float acc1 = -(d2 * acc2 + phi1) / d1;
    d[0] = w1; d[1] = w2; d[2] = acc1; d[3] = acc2;
}

// theta into [-pi, pi] by whole turns, one at a time as gymnasium's wrap() takes them; the count is bounded so that a state that is
// not finite cannot keep a lane in the loop
__device__ __forceinline__ float acrobot_wrap(float x)
{
#pragma clang fp contract(off)
    for (int i = 0; i < kAcrobotMaxWraps && x > kAcrobotPi; ++i) x -= kAcrobotTwoPi;
    for (int i = 0; i < kAcrobotMaxWraps && x < -kAcrobotPi; ++i) x += kAcrobotTwoPi;
    return x;
}

// the observation (cos theta1, sin theta1, cos theta2, sin theta2, omega1, omega2) of a physical state
__device__ __forceinline__ void acrobot_observe(const float (&s)[4], float (&ob)[6])
{
    ob[0] = cosf(s[0]); ob[1] = sinf(s[0]); ob[2] = cosf(s[1]); ob[3] = sinf(s[1]); ob[4] = s[2]; ob[5] = s[3];
}

// s: the physical state in, the next one -- or the reset draw where the step ends the episode -- out; action 0 / 1 / 2 is torque
// -1 / 0 / +1 and any other value is torque 0; terminal (the tip above the bar by one link) is tested on the new state, truncate =
// step_count reached max_step and not terminal.  Returns the reward: 0 on the terminal step, -1 otherwise.
__device__ __forceinline__ float acrobot_step(float (&s)[4], int action, int &step_count, int &episode, int max_step, uint64_t seed,
                                              uint32_t env, bool &terminal, bool &truncate)
{
#pragma clang fp contract(off)
    const float a = action == 0 ? -1.0f : (action == 2 ? 1.0f : 0.0f);
    const float dt = 0.2f, half = 0.1f;
    float k1[4], k2[4], k3[4], k4[4], y[4];
    acrobot_dsdt(s, a, k1);
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = s[c] + half * k1[c];
    acrobot_dsdt(y, a, k2);
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = s[c] + half * k2[c];
    acrobot_dsdt(y, a, k3);
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = s[c] + dt * k3[c];
    acrobot_dsdt(y, a, k4);
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = s[c] + dt / 6.0f * (k1[c] + 2.0f * k2[c] + 2.0f * k3[c] + k4[c]);
    s[0] = acrobot_wrap(s[0]);
    s[1] = acrobot_wrap(s[1]);
    s[2] = fminf(fmaxf(s[2], -kAcrobotMaxVel1), kAcrobotMaxVel1);
    s[3] = fminf(fmaxf(s[3], -kAcrobotMaxVel2), kAcrobotMaxVel2);
    const int sc = step_count + 1;
    terminal = -cosf(s[0]) - cosf(s[0] + s[1]) > 1.0f;
    truncate = sc >= max_step && !terminal;
    const bool done = terminal || truncate;
    if (done) {
        episode += 1;
        acrobot_reset_draw(seed, env, (uint32_t)episode, s);
    }
    step_count = done ? 0 : sc;
    return terminal ? 0.0f : -1.0f;
}

}  // namespace
