// The continuous device env as the one-launch entries are handed it.  Host side only: rollout_fused.hip, rollout_eval.hip and sac.hip check
// it here and COPY it into their kernels' own argument structs (RfArgs, sac_fused.hip's SacRolloutArgs); no kernel sees this struct.
#pragma once
#include "erl_common.h"

enum { ENV_SYN = 0, ENV_PENDULUM = 1, ENV_POINT = 2 };

struct ContEnv {
    int kind;                              // ENV_SYN | ENV_PENDULUM | ENV_POINT
    float *env_state;                      // (N, S) live state (SynVecEnv.state; PendulumVecEnv.state = its observation; PointChasingVecEnv.state)
    float *phys;                           // Pendulum: (N, 2) theta, theta_dot; PointChasing: (N,) distance; SynVecEnv: NULL
    const float *Ws, *Wa;                  // SynVecEnv; the others: NULL
    int32_t *step_count, *episode;
    int max_step;
    uint64_t env_seed;
};

// The PPO entries (`ppo`) name a missing buffer and max_step < 1 alike; the SAC entries name a missing buffer as they do their other
// pointers and report max_step beside H (sac.hip).
static inline int cont_env_check(const char *what, const ContEnv &e, bool ppo)
{
    const bool buffers = e.env_state && (e.kind == ENV_SYN ? (e.Ws && e.Wa) : e.phys != nullptr) && e.step_count && e.episode;
    ERL_REQUIRE(buffers && (!ppo || e.max_step >= 1), ppo ? "%s: bad environment argument" : "%s: NULL tensor", what);
    return ERL_OK;
}

// PointChasingVecEnv's shapes: dim = A in 1..4 (pointchasing_step.h), the observation (p0, v0, p1, v1)
static inline int cont_env_point_dims(const char *what, int S, int A)
{
    ERL_REQUIRE(A >= 1 && A <= 4 && S == 4 * A, "%s: bad shape", what);
    return ERL_OK;
}
