// The critic's per-element loss l(d) and its derivative l'(d), d = prediction - target, shared by every kernel that holds a critic
// objective (ppo_step.hip, ppo_step_s3_impl.h, ppo_step_w4_impl.h, ppo_step_wd_impl.h, ppo_step_discrete.hip, mlpn_common.h, sac.hip,
// sac_fused.hip).  `kind` is the reference's args.criterion (elegantrl/agents/AgentBase.py:62; include/erl_hip.h, ERL_CRIT_*), always
// with reduction = 'none': the callers apply unmask, the importance weights and the means themselves
//   (criterion(value, reward_sum) * unmask).mean()        elegantrl/agents/AgentPPO.py:190, :305
//   criterion(q_values, q_labels).mean(dim=1) * unmask    elegantrl/agents/AgentSAC.py:60, :127 (and the lambda_fit_cum_r term, :68, :135)
//   MSE        torch.nn.MSELoss             l = d d                                          l' = 2 d
//   SMOOTH_L1  torch.nn.SmoothL1Loss(beta)  l = |d| < beta ? 0.5 d d / beta : |d| - 0.5 beta       l' = clamp(d, -beta, beta) / beta
//   HUBER      torch.nn.HuberLoss(delta)    l = |d| <= delta ? 0.5 d d : delta (|d| - 0.5 delta)   l' = clamp(d, -delta, delta)
// `kind` and `beta` are uniform over a launch.  Every site keeps its MSE statements as they were, in their order, under
// `kind == ERL_CRIT_MSE` (the bit-identity tests hold the MSE route to its digests) and calls this header in the other arm.
#pragma once
#include "../../include/erl_hip.h"

__device__ __forceinline__ float critic_loss(int kind, float beta, float d)
{
    if (kind == ERL_CRIT_MSE) return d * d;
    const float a = fabsf(d);
    if (kind == ERL_CRIT_SMOOTH_L1) return a < beta ? 0.5f * d * d / beta : a - 0.5f * beta;
    return a <= beta ? 0.5f * d * d : beta * (a - 0.5f * beta);
}

__device__ __forceinline__ float critic_loss_grad(int kind, float beta, float d)
{
    if (kind == ERL_CRIT_MSE) return 2.f * d;
    const float c = fminf(fmaxf(d, -beta), beta);
    return kind == ERL_CRIT_SMOOTH_L1 ? c / beta : c;
}
