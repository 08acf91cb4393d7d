// The two register-chain pieces of the 8-wave 16x16x4 minibatch kernels that are not layer-forward code (mlp_chain.h): the backward
// pass through a layer's input and the feature-major staging of a register tile.  Shared by ppo_step.hip (K6, Gaussian head) and
// ppo_step_discrete.hip (categorical head); see ppo_step.hip's header comment for the formulation.
#pragma once
#include "ppo_step.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// backward through a layer's input on registers:  g[jt] <- g[jt] * ( W^T . dz ),  W = zero-padded LDS copy
// [16 kt][ldw] (A operand = W^T: lane (j, q) supplies W[16 t + 4 q + r][16 jt + j], four ds_read_b32 per k-tile).
// On entry g holds the gate GELU'(z_in) (kept in registers from the forward pass, or read back from the slab).
// ---------------------------------------------------------------------------------------------------------
template <int KT>
__device__ __forceinline__ void backward_input(const float *W, int ldw, int kt_rt, int nin, const f32x4 (&dz)[8], f32x4 (&g)[8],
                                               int l15, int q)
{
    constexpr int NCH = KT ? (KT + PCH - 1) / PCH : 8 / PCH;
    constexpr int NC = 8 * NCH;
    const int kt = KT ? KT : kt_rt;
    float4 wq[2][PCH];
    auto issue = [&](int c, float4(&dst)[PCH]) {
        const int jt = c / NCH, th = c % NCH;
#pragma unroll
        for (int j = 0; j < PCH; ++j) {
            const int t = PCH * th + j;
            if (jt < nin && t < kt) {
                const float *p = W + (16 * t + 4 * q) * ldw + 16 * jt + l15;
                dst[j] = make_float4(p[0], p[ldw], p[2 * ldw], p[3 * ldw]);
            }
        }
    };
    issue(0, wq[0]);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int jt = c / NCH, th = c % NCH;
        if (c + 1 < NC) issue(c + 1, wq[(c + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (jt < nin) {
            if (th == 0) acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < PCH; ++j) {
                const int t = PCH * th + j;
                if (t < kt) {
                    const float4 wv = wq[c & 1][j];
                    acc = mfma16(wv.x, dz[t][0], acc);
                    acc = mfma16(wv.y, dz[t][1], acc);
                    acc = mfma16(wv.z, dz[t][2], acc);
                    acc = mfma16(wv.w, dz[t][3], acc);
                }
            }
            if (th == NCH - 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) g[jt][r] *= acc[r];
            }
        }
    }
}

// stage a register-resident activation (D layout) feature-major into LDS: T[feature][16 w + m]
__device__ __forceinline__ void stage(float *T, const f32x4 (&a)[8], int nt, int col, int q)
{
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (t < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) T[(16 * t + 4 * q + r) * PLD + col] = a[t][r];
        }
}

}  // namespace
