// One MountainCar-v0 step of one env (gymnasium's dynamics: force 0.001, gravity 0.0025, |velocity| <= 0.07, position in [-1.2, 0.6],
// goal at position 0.5 with velocity >= 0), shared by the per-step kernel (erl_mountaincar_step_f32) and the one-launch discrete
// rollout / evaluation (rollout_discrete.hip).  Every product and sum is rounded on its own (contraction off below, and the translation
// unit is built with -ffp-contract=off), so that the two inlined copies agree bit for bit whatever surrounds them; the cosine is cosf,
// not a fast intrinsic.
#pragma once
#include "erl_common.h"

namespace {

constexpr float kMountainCarForce = 0.001f;
constexpr float kMountainCarGravity = 0.0025f;
constexpr float kMountainCarMaxSpeed = 0.07f;
constexpr float kMountainCarMinPos = -1.2f;
constexpr float kMountainCarMaxPos = 0.6f;
constexpr float kMountainCarGoalPos = 0.5f;
constexpr float kMountainCarGoalVel = 0.0f;

// the state an env starts episode `episode` with: position U[-0.6, -0.4) from one draw keyed by (env seed, env, episode, component 0),
// velocity exactly 0 -- a draw depends neither on the launch geometry nor on which kernel performs it
__device__ __forceinline__ void mountaincar_reset_draw(uint64_t seed, uint32_t env, uint32_t episode, float (&s)[2])
{
#pragma clang fp contract(off)
    const Philox4 p = philox4x32_10(env, 0x4d4f554eu, episode, 0x54434152u, (uint32_t)seed, (uint32_t)(seed >> 32));
    s[0] = (float)(p.x >> 8) * (1.0f / 16777216.0f) * 0.2f - 0.6f;
    s[1] = 0.0f;
}

// s: (position, velocity) in, the next state -- or the reset draw where the step ends the episode -- out; action 0 / 1 / 2 pushes left /
// nowhere / right and any other value pushes nowhere; terminal is tested on the new state, truncate = step_count reached max_step and
// not terminal; the reward is -1 on every step, the terminal one included.
__device__ __forceinline__ void mountaincar_step(float (&s)[2], int action, int &step_count, int &episode, int max_step, uint64_t seed,
                                                 uint32_t env, bool &terminal, bool &truncate)
{
#pragma clang fp contract(off)
    float position = s[0], velocity = s[1];
    const float push = action == 0 ? -1.0f : (action == 2 ? 1.0f : 0.0f);
    velocity = velocity + (push * kMountainCarForce + cosf(3.0f * position) * -kMountainCarGravity);
    velocity = fminf(fmaxf(velocity, -kMountainCarMaxSpeed), kMountainCarMaxSpeed);
    position = position + velocity;
    position = fminf(fmaxf(position, kMountainCarMinPos), kMountainCarMaxPos);
    if (position == kMountainCarMinPos && velocity < 0.0f) velocity = 0.0f;
    s[0] = position;
    s[1] = velocity;
    const int sc = step_count + 1;
    terminal = position >= kMountainCarGoalPos && velocity >= kMountainCarGoalVel;
    truncate = sc >= max_step && !terminal;
    const bool done = terminal || truncate;
    if (done) {
        episode += 1;
        mountaincar_reset_draw(seed, env, (uint32_t)episode, s);
    }
    step_count = done ? 0 : sc;
}

}  // namespace
