// One PPO minibatch of the categorical policy (AgentDiscretePPO / AgentDiscreteA2C) in ONE launch, gfx950 fp32 MFMA: gather + actor &
// critic forward + objective + full backward.  The fused counterpart of the layered erl_mlpn_ppo_step_discrete_f32 (mlpn.hip: one GEMM
// launch per dense layer, forward and backward, on two streams) for the policy shapes of the one-launch discrete rollout.
//
// The kernel is ppo_step.hip's 8-wave register-chained form (read that file's header comment for the formulation): grid =
// (ceil(B / 128), 2), blockIdx.y = 0 actor, 1 critic; a workgroup of 8 waves owns 128 samples and writes ONE gradient slab, summed in a
// fixed order by erl_grad_reduce_f32.  Exact-fp32 v_mfma_f32_16x16x4_f32 throughout, the same LDS pool, the same seven LDS-only barriers.
// What differs:
//   * the actor head.  After the output layer lane (m = lane & 15, q = lane >> 4) holds the logits a = 4 q + r of sample m; softmax, the
//     clamped log-probs, the entropy and dL/dlogits are formed across the four lane groups (categorical.h, categorical_ppo_terms_q4:
//     objective_discrete_kernel's statements).  There is no action_std_log and no dstd partial sums;
//   * the parameter blocks are the layered path's [W1 b1 W2 b2 W3 b3] without a std slot (the agent's checkpoints keep their layout):
//     Dims' offsets without the std slot are exactly those;
//   * advantages arrive normalised (the agent keeps its erl_adv_normalize launch), actions are int32 indices;
//   * GELU'(z1) always stays in registers: the slab of a discrete policy can be smaller than the 64 KB that ppo_step.hip's tuned shape
//     parks there.
// The critic's branch is ppo_step.hip's, statement for statement.
#include "ppo_step_chain.h"
#include "categorical.h"
#include "critic_loss.h"

namespace {

constexpr int DNW = 8;

struct PpoDArgs {
    const float *P[2];    // actor, critic flat params [W1 b1 W2 b2 W3 b3]
    const float *avg[2];
    const float *sd[2];
    const float *states, *logprobs, *advantages, *reward_sums;
    const int32_t *actions;
    const uint8_t *unmasks;
    const int64_t *ids;
    int64_t H, N, B;
    int S, h1, h2, A;
    float ratio_clip, lambda_entropy, inv_batch;
    float crit_beta;      // the threshold of the call's critic loss (critic_loss.h; its kind is a template parameter).  In what was padding: no
                          // member moved, the struct kept its size, and the MSE kernels their code
    float *slabs;
    int64_t stride, Pa, Pc;
};

// LDS pool (floats), ppo_step.hip's without the dstd partials: [RA: W2 copy, later staged tiles][RB: W1 copy | X^T, later staged tiles]
//                    [RC: dY^T][RW3: W3 copy][s_bias: b1 | b2 | b3(16)][s_red: 16]
constexpr int kDRFloats = 128 * 68 + 64 * PLD > 128 * 132 ? 128 * 68 + 64 * PLD : 128 * 132;
static_assert(kDRFloats >= 128 * PLD && kDRFloats % 4 == 0, "staged tiles must fit the weight-copy regions");
static_assert(kDRFloats >= 128 * lds_ld(128) && kDRFloats >= 128 * lds_ld(64) + 64 * PLD, "weight copies (and X^T next to W1's) must fit");
constexpr int kDRCFloats = 16 * PLD;
constexpr int kDRW3Floats = 16 * 132;
static_assert(kDRW3Floats >= 16 * lds_ld(128), "W3 copy must fit");
constexpr int kDBiasFloats = 128 + 128 + 16;
constexpr size_t kPpoDLdsBytes = (size_t)(2 * kDRFloats + kDRCFloats + kDRW3Floats + kDBiasFloats + 16) * sizeof(float);
static_assert(kPpoDLdsBytes <= 160 * 1024, "one workgroup per CU");

// CRIT: the critic loss, ERL_CRIT_* (critic_loss.h).  A template parameter in this family: as a run-time branch it cost the <1, 4, 2, .>
// kernels 12-13 vector registers, from four waves a SIMD to three (profiles/criterion_kernel_resources.txt); the CRIT = ERL_CRIT_MSE kernels
// are the parent's, byte for byte
template <bool ACTOR, int NS_, int N1_, int N2_, bool VEC, int CRIT>
__device__ __forceinline__ void ppo_discrete_block(const PpoDArgs &g, float *smem)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int net = ACTOR ? 0 : 1;
    const Dims d{g.S, g.h1, g.h2, ACTOR ? g.A : 1};
    const int S = d.S, h1 = N1_ ? 16 * N1_ : d.h1, h2 = N2_ ? 16 * N2_ : d.h2, OUT = d.out;
    const int ns = NS_ ? NS_ : (S + 15) >> 4, n1 = N1_ ? N1_ : h1 >> 4, n2 = N2_ ? N2_ : h2 >> 4;
    const float *P = g.P[net];

    float *RA = smem;                      // W2 copy [h2][ld2], later staged tiles [128][PLD]
    float *RB = RA + kDRFloats;            // W1 copy [h1][ld1], later staged tiles [128][PLD]
    float *RC = RB + kDRFloats;            // [16][PLD]   dY^T
    float *RW3 = RC + kDRCFloats;          // W3 copy [16][ld3] (rows >= OUT are zero)
    float *s_b1 = RW3 + kDRW3Floats, *s_b2 = s_b1 + 128, *s_b3 = s_b2 + 128;
    float *s_red = s_b3 + 16;              // [16] block_sum scratch
    const int ld1 = lds_ld(16 * ns), ld2 = lds_ld(h1), ld3 = lds_ld(h2);

    // ---- prologue: two global round trips.  Trip 1: the sample id and the weight/bias copies.
    const int col = 16 * wave + l15;                       // sample slot inside the workgroup
    const int64_t bidx = (int64_t)blockIdx.x * PB + col;
    const bool valid = bidx < g.B;
    const int64_t id = g.ids[valid ? bidx : 0];
    float4 c2[8], c1[8], c3[1];
    copy_load<VEC, 8, DNW * 64>(c2, P + d.oW2(), h2, h1, h2, h1, tid);
    copy_load<VEC, 8, DNW * 64>(c1, P + d.oW1(), h1, S, h1, 16 * ns, tid);
    copy_load<VEC, 1, DNW * 64>(c3, P + d.oW3(), OUT, h2, 16, h2, tid);
    float bias_pre = 0.f;                                  // b1 | b2 | b3 (one element per thread 0..271)
    if (tid < 128) bias_pre = (tid < h1) ? P[d.ob1() + tid] : 0.f;
    else if (tid < 256) bias_pre = (tid - 128 < h2) ? P[d.ob2() + tid - 128] : 0.f;
    else if (tid < 272) bias_pre = (tid - 256 < OUT) ? P[d.ob3() + tid - 256] : 0.f;

    // ---- trip 2: id -> (t = id % H, n = id // H) -> buffer row t*N + n  (AgentPPO.py:179-187) and its data
    int64_t n_, t_;
    if (g.H * g.N <= 0x7fffffffLL) {       // uniform branch: ids < H N fit 32 bits
        const uint32_t i32 = (uint32_t)id, h32 = (uint32_t)g.H, n32 = i32 / h32;
        n_ = n32;
        t_ = i32 - n32 * h32;
    } else {
        n_ = id / g.H;
        t_ = id - n_ * g.H;
    }
    const int64_t row = valid ? t_ * g.N + n_ : 0;
    // this sample's raw state slice, features 16 t + 4 q + r; normalised by norm_x (AgentPPO.py:360-361)
    const float *srow = g.states + row * S;
    const float *avg = g.avg[net], *sdv = g.sd[net];
    auto load_x_raw = [&](float4(&R)[8]) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (t < ns) R[t] = load4<VEC>(srow, 16 * t + 4 * q, S);
    };
    auto norm_x = [&](const float4(&R)[8], f32x4(&X)[8]) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (t < ns) {
                const int k0 = 16 * t + 4 * q;
                const float4 a4 = load4<VEC>(avg, k0, S), s4 = load4<VEC>(sdv, k0, S);
                const float rr[4] = {R[t].x, R[t].y, R[t].z, R[t].w}, aa[4] = {a4.x, a4.y, a4.z, a4.w},
                            ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float xn = (rr[r] - aa[r]) / (ss[r] + 1e-4f);
                    X[t][r] = (valid && k0 + r < S) ? xn : 0.f;
                }
            }
        }
    };
    float4 XR[8];
    load_x_raw(XR);

    // ---- publish the LDS copies (zero padded to the tile grid), visible after barrier (0)
    copy_store<8, DNW * 64>(c2, RA, ld2, h2, h1, tid);
    copy_store<8, DNW * 64>(c1, RB, ld1, h1, 16 * ns, tid);
    copy_store<1, DNW * 64>(c3, RW3, ld3, 16, h2, tid);
    if (tid < 272) s_b1[tid] = bias_pre;                   // s_b1 | s_b2 | s_b3 are contiguous

    // X^T for dW1 lives next to the W1 copy when both fit (compile-time S <= 64): staged once, here, from the registers
    constexpr bool EARLY_X = NS_ != 0 && NS_ <= 4;
    float *RX = EARLY_X ? RB + 128 * lds_ld(64) : RB;
    float *slab = g.slabs + (size_t)blockIdx.x * g.stride + (ACTOR ? 0 : g.Pa);
    f32x4 H1[8], G1[8], H2[8], G2[8];
    f32x4 X[8];
    norm_x(XR, X);
    if (EARLY_X) stage(RX, X, ns, col, q);
    lds_barrier();                                                   // (0) weight copies visible
    forward_layer<true, NS_>(RB, ld1, s_b1, ns, n1, X, H1, G1, l15, q);
    forward_layer<true, N1_>(RA, ld2, s_b2, n1, n2, H1, H2, G2, l15, q);
    // per-sample scalars: issued here (L2 / MALL hits by now), consumed after the output layer
    const float um = (valid && g.unmasks[row]) ? 1.f : 0.f;
    const float xa = ACTOR ? g.logprobs[row] : g.reward_sums[row];
    const float xb = ACTOR ? g.advantages[row] : 0.f;
    const int act = ACTOR ? g.actions[row] : 0;
    f32x4 Y[8], dummy[8];
    forward_layer<false, N2_>(RW3, ld3, s_b3, n2, 1, H2, Y, dummy, l15, q);

    // ---- objective and dL/dY for this lane's outputs a = 4 q + r   (AgentPPO.py:189-204)
    f32x4 dY[8];
    float loss0 = 0.f, loss1 = 0.f;
    if (!ACTOR) {
        const float diff = Y[0][0] - xa;                  // only (q = 0, r = 0) is the value head
        const bool head = q == 0;
        if (CRIT == ERL_CRIT_MSE) {
            loss0 = head ? diff * diff * um : 0.f;
            dY[0] = f32x4{head ? 2.f * diff * um * g.inv_batch : 0.f, 0.f, 0.f, 0.f};
        } else {                                           // args.criterion other than MSELoss (critic_loss.h)
            loss0 = head ? critic_loss(CRIT, g.crit_beta, diff) * um : 0.f;
            dY[0] = f32x4{head ? critic_loss_grad(CRIT, g.crit_beta, diff) * um * g.inv_batch : 0.f, 0.f, 0.f, 0.f};
        }
    } else {
        const float z[4] = {Y[0][0], Y[0][1], Y[0][2], Y[0][3]};
        float dz[4];
        const CatPpoTerms o = categorical_ppo_terms_q4(z, q, OUT, act, xb, xa, um, g.ratio_clip, g.lambda_entropy, g.inv_batch, dz);
        if (q == 0) {                                      // one lane per sample carries the logged terms; padding rows contribute 0
            loss0 = valid ? o.surr * um : 0.f;
            loss1 = valid ? o.ent * um : 0.f;
        }
        dY[0] = f32x4{valid ? dz[0] : 0.f, valid ? dz[1] : 0.f, valid ? dz[2] : 0.f, valid ? dz[3] : 0.f};
    }

    // ---- dZ2 = (W3^T dY) * GELU'(z2)  (K = 16 outputs: one k-tile);  dZ1 = (W2^T dZ2) * GELU'(z1)
    backward_input<1>(RW3, ld3, 1, n2, dY, G2, l15, q);            // G2 (the gate) <- dZ2
    backward_input<N2_>(RA, ld2, n2, n1, G2, G1, l15, q);          // G1 (the gate) <- dZ1
    lds_barrier();                                                   // (1) every wave is done with the weight copies

    // ---- layer 1: dW1 = dZ1^T . X, db1;  (dY^T is staged alongside for the output layer)
    stage(RA, G1, n1, col, q);                                      // dZ1^T
#pragma unroll
    for (int r = 0; r < 4; ++r) RC[(4 * q + r) * PLD + col] = dY[0][r];
    if (!EARLY_X) {                                                 // generic shapes: re-gather X now (the W1 copy is dead)
        load_x_raw(XR);
        norm_x(XR, X);
        stage(RX, X, ns, col, q);
    }
    lds_barrier();                                                   // (2)
    // (S <= 16 stages 16 rows of X^T and weight_grad reads a block of 32: rows 16..31 are stale LDS, they feed output columns >= 16 only,
    // which cols_real = S masks at the store)
    weight_grad<DNW>(RA, h1 >> 5, RX, (S + 31) >> 5, slab + d.oW1(), S, S, wave, lane);
    bias_grad<DNW>(RA, h1, slab + d.ob1(), wave, lane);
    if (wave == 0) bias_grad<DNW>(RC, OUT, slab + d.ob3(), 0, lane);
    lds_barrier();                                                   // (3) dZ1^T, X^T consumed

    // ---- output layer: dW3 (16 x h2) = dY^T . H2 on 16x16x4 MFMA, one 16-column tile per wave
    stage(RA, H2, n2, col, q);                                      // H2^T
    stage(RB, H1, n1, col, q);                                      // H1^T (for dW2)
    lds_barrier();                                                   // (4)
    for (int it = wave; it < n2; it += DNW) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *a = RC + l15 * PLD + 4 * q;                    // lane group q: samples 16 j + 4 q + {0..3}
        const float *b = RA + (16 * it + l15) * PLD + 4 * q;
#pragma unroll
        for (int j = 0; j < PB / 16; ++j) {
            const float4 av = *reinterpret_cast<const float4 *>(a + 16 * j), bv = *reinterpret_cast<const float4 *>(b + 16 * j);
            acc = mfma16(av.x, bv.x, acc);
            acc = mfma16(av.y, bv.y, acc);
            acc = mfma16(av.z, bv.z, acc);
            acc = mfma16(av.w, bv.w, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a_ = 4 * q + r;
            if (a_ < OUT) slab_store(acc[r], slab + d.oW3() + (size_t)a_ * h2 + 16 * it + l15);
        }
    }
    lds_barrier();                                                   // (5) H2^T consumed
    stage(RA, G2, n2, col, q);                                      // dZ2^T
    lds_barrier();                                                   // (6)

    // ---- layer 2: dW2 = dZ2^T . H1, db2
    weight_grad<DNW>(RA, h2 >> 5, RB, h1 >> 5, slab + d.oW2(), h1, h1, wave, lane);
    bias_grad<DNW>(RA, h2, slab + d.ob2(), wave, lane);

    // ---- objective partial sums (scaled by 1/B so that the slab reduction yields the means)
    const float t0 = block_sum(loss0, s_red);
    const float t1 = block_sum(loss1, s_red);
    float *logs = g.slabs + (size_t)blockIdx.x * g.stride + g.Pa + g.Pc;
    if (ACTOR) {
        if (tid == 0) {
            logs[1] = t0 * g.inv_batch;                              // obj_surrogate = mean(surr um)
            logs[2] = t1 * g.inv_batch;                              // obj_entropy = mean(entropy um), as fold_logs_kernel(is_actor = 2)
        }
    } else {
        const int tail = (int)(g.stride - (g.Pa + g.Pc));            // 4 logs + the row's pad: 4 .. 35 floats
        if (tid == 0) logs[0] = t0 * g.inv_batch;
        else if (tid >= 3 && tid < tail) logs[tid] = 0.f;            // the 4th log and the pad, one lane each
    }
}

// the MSE kernel keeps its name and template list; the other criteria are a kernel of their own
template <int NS_, int N1_, int N2_, bool VEC>
__global__ __launch_bounds__(DNW * 64) void ppo_step_discrete_kernel(PpoDArgs g)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (blockIdx.y == 0) ppo_discrete_block<true, NS_, N1_, N2_, VEC, ERL_CRIT_MSE>(g, smem);
    else ppo_discrete_block<false, NS_, N1_, N2_, VEC, ERL_CRIT_MSE>(g, smem);
}
template <int NS_, int N1_, int N2_, bool VEC, int CRIT>
__global__ __launch_bounds__(DNW * 64) void ppo_step_discrete_crit_kernel(PpoDArgs g)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (blockIdx.y == 0) ppo_discrete_block<true, NS_, N1_, N2_, VEC, CRIT>(g, smem);
    else ppo_discrete_block<false, NS_, N1_, N2_, VEC, CRIT>(g, smem);
}

// the shapes of the one-launch discrete rollout (rollout_discrete.hip, erl_rollout_discrete_supported), which this kernel completes
bool pd_dims_ok(int S, int h1, int h2, int A)
{
    return S >= 1 && S <= 64 && h1 >= 32 && h1 <= 128 && h1 % 32 == 0 && h2 >= 32 && h2 <= 128 && h2 % 32 == 0 && A >= 2 && A <= 8;
}

template <int NS_, int N1_, int N2_, bool VEC, int CRIT>
constexpr auto discrete_kernel_of()
{
    if constexpr (CRIT == ERL_CRIT_MSE) return ppo_step_discrete_kernel<NS_, N1_, N2_, VEC>;       // (no crit kernel is instantiated for MSE)
    else return ppo_step_discrete_crit_kernel<NS_, N1_, N2_, VEC, CRIT>;
}

template <int NS_, int N1_, int N2_, bool VEC, int CRIT>
int launch_discrete_crit(const PpoDArgs &g, int n_slabs, hipStream_t stream)
{
    constexpr auto kernel = discrete_kernel_of<NS_, N1_, N2_, VEC, CRIT>();
    static bool attr_set = false;
    if (!attr_set) {
        int rc = erl_hip_status(hipFuncSetAttribute((const void *)kernel,
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPpoDLdsBytes),
                                "hipFuncSetAttribute(ppo_step_discrete_kernel)");
        if (rc) return rc;
        attr_set = true;
    }
    hipLaunchKernelGGL(kernel, dim3(n_slabs, 2), dim3(DNW * 64), kPpoDLdsBytes, stream, g);
    return erl_hip_status(hipGetLastError(), "erl_ppo_step_discrete_f32");
}

template <int NS_, int N1_, int N2_, bool VEC>
int launch_discrete(const PpoDArgs &g, int crit_kind, int n_slabs, hipStream_t stream)
{
    if (crit_kind == ERL_CRIT_SMOOTH_L1) return launch_discrete_crit<NS_, N1_, N2_, VEC, ERL_CRIT_SMOOTH_L1>(g, n_slabs, stream);
    if (crit_kind == ERL_CRIT_HUBER) return launch_discrete_crit<NS_, N1_, N2_, VEC, ERL_CRIT_HUBER>(g, n_slabs, stream);
    return launch_discrete_crit<NS_, N1_, N2_, VEC, ERL_CRIT_MSE>(g, n_slabs, stream);
}

// validation shared by the two entry points: everything that can be checked on the host, before any launch
int check_discrete(const char *what, const void *const *tensors, int n_tensors, int S, int h1, int h2, int A, int64_t H, int64_t N, int64_t B,
                   int n_slabs)
{
    for (int i = 0; i < n_tensors; ++i) ERL_REQUIRE(tensors[i], "%s: NULL tensor", what);
    ERL_REQUIRE(pd_dims_ok(S, h1, h2, A), "%s: unsupported dims S=%d net=[%d,%d] A=%d (fused discrete minibatch kernel: state_dim <= 64, 2 hidden "
                "layers of 32..128 in steps of 32, 2 <= action_dim <= 8)", what, S, h1, h2, A);
    ERL_REQUIRE(H >= 1 && N >= 1 && B >= 1 && H < (1LL << 31) && N < (1LL << 31), "%s: bad shape H=%lld N=%lld B=%lld", what, (long long)H,
                (long long)N, (long long)B);
    ERL_REQUIRE(n_slabs == erl_ppo_num_slabs(B), "%s: n_slabs=%d, expected erl_ppo_num_slabs(B=%lld)=%d", what, n_slabs, (long long)B,
                erl_ppo_num_slabs(B));
    return ERL_OK;
}

int step_discrete(const float *actor_params, const float *critic_params, const float *act_avg, const float *act_std, const float *cri_avg,
                  const float *cri_std, int S, int h1, int h2, int A, const float *states, const int32_t *actions, const uint8_t *unmasks,
                  const float *logprobs, const float *advantages, const float *reward_sums, int64_t H, int64_t N, const int64_t *ids, int64_t B,
                  float ratio_clip, float lambda_entropy, float inv_batch, float *slabs, int n_slabs, hipStream_t st)
{
    PpoDArgs g;
    g.P[0] = actor_params; g.P[1] = critic_params;
    g.avg[0] = act_avg; g.avg[1] = cri_avg;
    g.sd[0] = act_std; g.sd[1] = cri_std;
    g.states = states; g.actions = actions; g.logprobs = logprobs; g.advantages = advantages; g.reward_sums = reward_sums;
    g.unmasks = unmasks; g.ids = ids;
    g.H = H; g.N = N; g.B = B;
    g.S = S; g.h1 = h1; g.h2 = h2; g.A = A;
    g.ratio_clip = ratio_clip; g.lambda_entropy = lambda_entropy; g.inv_batch = inv_batch;
    const int crit = erl_criterion_of_call().kind;
    g.crit_beta = erl_criterion_of_call().beta;
    g.slabs = slabs;
    g.Pa = Dims{S, h1, h2, A}.count(false);
    g.Pc = Dims{S, h1, h2, 1}.count(false);
    g.stride = erl_ppo_discrete_slab_stride(S, h1, h2, A);
    // 16-byte vector path: every row / parameter block / normalisation vector must be 16-byte aligned (the critic's block follows the
    // actor's in the agent's flat buffer: Pa % 4 == A % 4, so it is for A = 4 and 8)
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = (S % 4 == 0) && al(actor_params) && al(critic_params) && al(states) && al(act_avg) && al(act_std) && al(cri_avg) &&
                     al(cri_std);
    const bool hot = S <= 16 && h1 == 64 && h2 == 32;      // CartPole's (64, 32): compile-time tile counts
    if (hot) return vec ? launch_discrete<1, 4, 2, true>(g, crit, n_slabs, st) : launch_discrete<1, 4, 2, false>(g, crit, n_slabs, st);
    return vec ? launch_discrete<0, 0, 0, true>(g, crit, n_slabs, st) : launch_discrete<0, 0, 0, false>(g, crit, n_slabs, st);
}

}  // namespace

extern "C" int erl_ppo_discrete_supported(int S, int h1, int h2, int A) { return pd_dims_ok(S, h1, h2, A) ? 1 : 0; }

extern "C" int64_t erl_ppo_discrete_slab_stride(int S, int h1, int h2, int A)
{
    if (!pd_dims_ok(S, h1, h2, A)) return -1;
    // [actor Pa | critic Pc | 4 logged values], rounded up to 32 floats (whole 128-byte lines, as erl_ppo_slab_stride); the pad is written as zeros
    const int64_t n = Dims{S, h1, h2, A}.count(false) + Dims{S, h1, h2, 1}.count(false) + 4;
    return (n + 31) / 32 * 32;
}

extern "C" int erl_ppo_step_discrete_f32(const float *actor_params, const float *critic_params, const float *act_avg, const float *act_std,
                                         const float *cri_avg, const float *cri_std, int S, int h1, int h2, int A, const float *states,
                                         const int32_t *actions, const uint8_t *unmasks, const float *logprobs, const float *advantages,
                                         const float *reward_sums, int64_t H, int64_t N, const int64_t *ids, int64_t B, float ratio_clip,
                                         float lambda_entropy, float inv_batch, float *slabs, int n_slabs, void *stream)
{
    const void *const tensors[] = {actor_params, critic_params, act_avg, act_std, cri_avg, cri_std, states, actions,
                                   unmasks,      logprobs,      advantages, reward_sums, ids, slabs};
    ERL_CRITERION_ENTRY("erl_ppo_step_discrete_f32");
    int rc = check_discrete("erl_ppo_step_discrete_f32", tensors, 14, S, h1, h2, A, H, N, B, n_slabs);
    if (rc) return rc;
    return step_discrete(actor_params, critic_params, act_avg, act_std, cri_avg, cri_std, S, h1, h2, A, states, actions, unmasks, logprobs,
                         advantages, reward_sums, H, N, ids, B, ratio_clip, lambda_entropy, inv_batch, slabs, n_slabs, (hipStream_t)stream);
}

// The whole minibatch loop of AgentDiscretePPO.update_net from one call: per minibatch the kernel above, the slab reduction into
// grads[k], the partial norms and clip + Adam -- the existing tail entry points with the arguments AgentPPO.update_net's per-minibatch
// branch gives them, so the weights' bits do not depend on who drives the loop.  Everything on the caller's stream.
extern "C" int erl_ppo_update_discrete_f32(float *flat_params, float *exp_avg, float *exp_avg_sq, const float *act_avg, const float *act_std,
                                           const float *cri_avg, const float *cri_std, int S, int h1, int h2, int A, const float *states,
                                           const int32_t *actions, const uint8_t *unmasks, const float *logprobs, const float *advantages,
                                           const float *reward_sums, int64_t H, int64_t N, const int64_t *ids, int64_t B, int update_times,
                                           float ratio_clip, float lambda_entropy, float *slabs, int n_slabs, float *grads, int32_t first_step,
                                           float lr, float beta1, float beta2, float eps, float max_norm, void *stream)
{
    const char *what = "erl_ppo_update_discrete_f32";
    ERL_CRITERION_ENTRY(what);
    const void *const tensors[] = {flat_params, exp_avg, exp_avg_sq, act_avg, act_std, cri_avg, cri_std, states, actions,
                                   unmasks,     logprobs, advantages, reward_sums, ids, slabs, grads};
    int rc = check_discrete(what, tensors, 16, S, h1, h2, A, H, N, B, n_slabs);
    if (rc) return rc;
    ERL_REQUIRE(update_times >= 1 && first_step >= 1, "%s: bad argument update_times=%d first_step=%d", what, update_times, (int)first_step);
    const int64_t Pa = Dims{S, h1, h2, A}.count(false), Pc = Dims{S, h1, h2, 1}.count(false);
    const int64_t stride = erl_ppo_discrete_slab_stride(S, h1, h2, A);
    const int64_t off[2] = {0, Pa}, len[2] = {Pa, Pc};
    const float inv_batch = (float)(1.0 / (double)B);
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < update_times; ++k) {
        float *gk = grads + (size_t)k * stride;
        rc = step_discrete(flat_params, flat_params + Pa, act_avg, act_std, cri_avg, cri_std, S, h1, h2, A, states, actions, unmasks, logprobs,
                           advantages, reward_sums, H, N, ids + (size_t)k * B, B, ratio_clip, lambda_entropy, inv_batch, slabs, n_slabs, st);
        if (!rc) rc = erl_grad_reduce_f32(slabs, n_slabs, stride, gk, stream);
        if (!rc) rc = erl_grad_sq_partials_f32(gk, stride, off, len, 2, 1.f, stream);
        if (!rc) rc = erl_clip_adam_partials_f32(flat_params, gk, exp_avg, exp_avg_sq, stride, off, len, 2, first_step + k, lr, beta1, beta2, eps,
                                                 max_norm, 1.f, stream);
        if (rc) return rc;
    }
    return ERL_OK;
}
