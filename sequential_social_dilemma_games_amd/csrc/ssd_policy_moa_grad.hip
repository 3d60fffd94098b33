// ssd_policy_moa_grad.hip -- the causal-influence policy's loss, PPOLoss + moa_weight * MOALoss (algorithms/ppo_causal.py:36-75,
// common_funcs.py:70-115), on a sampled fragment with truncated backpropagation through time through both Keras LSTMs, its
// statistics and the gradient of every ConvMOAPolicy parameter: ssd_policy_moa_ppo_grad.  include/ssd.h states the contract (the
// loss, the state rule, the previous actions, the order of the sums); DESIGN.md section 18 the shape, the resource report and
// the measurements.
//
// The fragment is walked window by window by a host loop that only enqueues, as ssd_policy_lstm_grad.hip walks it, with the
// kernels of ssd_bptt_device.hpp instantiated for the two branches below.  Per window, on the caller's scratch:
//   1. features: the trunk kernel's MOA mode (ssd_policy.hip) over the window's rows -> feat [rows][2][32], both stacks;
//   2. the actions branch: ssd_bptt_seq_kernel<C, MoaActBranch> on stack 0 (KerasCell; forward, the PPO terms of a row through
//      ppo_row, backward with the heads' sums in registers, dx of stack 0 to scratch), then ssd_bptt_dw_kernel<C, MoaActBranch>
//      for the LSTM matrix and bias;
//   3. the MOA branch, on the same (state, gates / dz) scratch: ssd_bptt_seq_kernel<C, MoaPredBranch> on [stack 1, the N
//      previous actions in slot order, zeros to 48].  Its head is the prediction h2' pred_w (16 x C . C x (N-1) A) on the matrix
//      cores; a thread per (row, other agent) forms the log-softmax, the cross-entropy (float64 sum) and dpred = moa_weight /
//      (N-1) (softmax - onehot), which goes to scratch; the backward reads it back, dh2' = dpred pred_w^T on the matrix cores,
//      then the cell's backward as in the actions branch.  ssd_bptt_dw_kernel<C, MoaPredBranch> forms the 48 + C rows of the MOA
//      matrix (rows 32 .. 32 + N - 1 from the action inputs, by the same product) and ssd_moa_dpred_kernel pred_w = h2'^T
//      dpred and pred_b, both over the fixed partition of the set's rows lstm_w's kernel uses;
//   4. the trunk's backward from dx, once per stack (ssd_policy_grad.hip's kernel with tanh derivatives); stack 1's launch adds
//      its conv sums to stack 0's.
// Every kernel adds its partial sums to what scratch holds from the windows before (the first window stores).  At the end
// ssd_moa_reduce_kernel adds the partials of every entry in order in float64, scales by 1 / set rows and rounds once.  No
// atomics anywhere: the same inputs give the same bits.
//
// ssd_policy_moa_ac_grad is the same walk with the A3C row loss (include/ssd.h, A3C LOSS AND GRADIENTS):
// the actions branch's sequence kernel and the reduce compiled once more with ssd::kLossAc.  The A3C terms are sums over a set's
// rows and MOALoss a mean, so the MOA branch's scale on dpred carries 1 / rows too; its kernels are the PPO call's as they are.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_bptt_device.hpp"

namespace {

constexpr int kX = SSD_MOA_X;            // a stack's features per row
constexpr int kXM = SSD_MOA_XM;          // input rows of the MOA cell
constexpr int kStatFloats = SSD_PPO_STAT_FLOATS;

using ssd::f32x4;

// The two branches: Keras cells on a stack's half of the 64-float feature rows, each with two rows (h, c) of the four-row state.
struct MoaActBranch {                    // the actions LSTM on stack 0 with the policy head
    using Cell = ssd::KerasCell;
    static constexpr int kIn = kX, kFeatPitch = 2 * kX, kFeat0 = 0, kRingRows = 4, kRing0 = 0, kPad = 36;
    static constexpr bool kPred = false;
    static constexpr int w(int C, int) { return SSD_MOA_LSTM_W(C); }
    static constexpr int b(int C, int) { return SSD_MOA_LSTM_B(C); }
    static constexpr int logits_w(int C) { return SSD_MOA_LOGITS_W(C); }
    static constexpr int value_w(int C) { return SSD_MOA_VALUE_W(C); }
    static constexpr int logits_b(int C, int A) { return SSD_MOA_LOGITS_B(C, A); }
    static constexpr int value_b(int C) { return SSD_MOA_VALUE_B(C); }
};
struct MoaPredBranch {                   // the MOA LSTM on [stack 1, previous actions] with the prediction head
    using Cell = ssd::KerasCell;
    static constexpr int kIn = kXM, kFeatPitch = 2 * kX, kFeat0 = kX, kRingRows = 4, kRing0 = 2, kPad = 20;
    static constexpr bool kPred = true;
    static constexpr int w(int C, int A) { return SSD_MOA_MW(C, A); }
    static constexpr int b(int C, int A) { return SSD_MOA_MB(C, A); }
};

// ------------------------------------------------------------------------------------- pred_w = h2'^T dpred, and pred_b
// As ssd_bptt_dw_kernel with A[c][k] = h2'[row k][c] (the step's own output) and B[k][n] = dpred[row k][n]: workgroup (block of
// 64 prediction columns, split s, set p), C / 16 accumulator tiles a lane; columns beyond (N - 1) A are read as zero.
template <int C>
__global__ void __launch_bounds__(256) ssd_moa_dpred_kernel(ssd::BpttArgs a) {
    constexpr int kMT = C / 16;
    constexpr int kChunk = ssd::kBpttChunk;
    __shared__ float s_b[4 * 64];
    const int tid = threadIdx.x, s = blockIdx.y, p = blockIdx.z;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int n0 = blockIdx.x * 64 + wave * 16, col = n0 + l15;
    const int NA = (a.N - 1) * a.A, PP = a.pred_pitch;
    const int stride = a.P == 1 ? 1 : a.N;
    const int R = a.seqs * a.steps;
    f32x4 acc[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;

    const int chunks = R / kChunk + (R % kChunk != 0);
    for (int chunk = s; chunk < chunks; chunk += a.S) {
        for (int kk = 0; kk < kChunk / 4; ++kk) {
            const int r = chunk * kChunk + 4 * kk + l4;
            const bool valid = r < R;
            const size_t rw = valid ? (size_t)r * stride + p : 0;
            const float b = valid && col < NA ? a.dpred[rw * PP + col] : 0.f;
            bsum += b;
            const float *h = a.st + (rw * 2 + ssd::KerasCell::kRowH) * C;
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const float av = valid ? h[16 * mt + l15] : 0.f;
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, acc[mt], 0, 0, 0);
            }
        }
    }

    float *part = a.part_pred + ((size_t)p * a.S + s) * (size_t)((C + 1) * PP);
    const bool add = a.accumulate != 0;
    if (col < PP) {
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float *dst = part + (size_t)(16 * mt + 4 * l4 + r) * PP + col;
                *dst = add ? *dst + acc[mt][r] : acc[mt][r];
            }
        }
    }
    ssd::bptt_column_sum(s_b, tid, bsum, part + (size_t)C * PP + col, col < PP, add);
}

// ------------------------------------------------------------------------------------------------------ the final reduce
struct ReduceArgs {
    int32_t P, A, N, C, set_floats, set_rows, Gt, Gs, S, pred_pitch;
    double moa_weight;
    const float *part_trunk;       // [P][Gt][SSD_MOA_LSTM_W(C) + kStatFloats]
    const float *part_seq;         // [P][Gs][16 C + 16 + kStatFloats]
    const float *part_wa;          // [P][S][(32 + C) 4C + 4C]
    const float *part_wm;          // [P][S][(48 + C) 4C + 4C]
    const float *part_pred;        // [P][S][(C + 1) pred_pitch]
    float *grads;                  // [P][set_floats]
    double *stats;                 // [P][6]
};

// The partials of every entry added in order in float64, times 1 / set rows, rounded once; the padding floats and the rows
// 32 + N .. 47 of the MOA matrix are zero.  kLossAc: the sums as they are (the A3C terms are sums over rows, and the MOA branch's
// entries carry 1 / set rows from a.moa_scale already); stats [P][5]: a3c_row's four, total with moa_weight * moa_loss, then
// moa_loss, the one statistic still divided by the set's rows.
template <int kLoss>
__global__ void __launch_bounds__(256) ssd_moa_reduce_kernel(ReduceArgs a) {
    constexpr bool kSum = kLoss == ssd::kLossAc;
    const int idx = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y, C = a.C, A = a.A, N = a.N, NA = (N - 1) * A, PP = a.pred_pitch;
    const int seq_pitch = 16 * C + 16 + kStatFloats, trunk_pitch = SSD_MOA_LSTM_W(C) + kStatFloats;
    const int wa_floats = (kX + C) * 4 * C, wa_pitch = wa_floats + 4 * C, wm_floats = (kXM + C) * 4 * C, wm_pitch = wm_floats + 4 * C;
    const int pred_part = (C + 1) * PP;
    const int stack_floats = SSD_POL_FC2_B + 32 - SSD_POL_FC1_W;
    const float *pseq = a.part_seq + (size_t)p * a.Gs * seq_pitch;
    if (idx < a.set_floats) {
        const float *src = nullptr;
        size_t pitch = 0;
        int n = 0;
        if (idx < SSD_MOA_LSTM_W(C)) {
            const bool real = idx < SSD_POL_CONV_B + 6 || (idx >= SSD_MOA_FC && (idx - SSD_MOA_FC) % SSD_MOA_FC_STRIDE < stack_floats);
            if (real) { src = a.part_trunk + (size_t)p * a.Gt * trunk_pitch + idx; pitch = trunk_pitch; n = a.Gt; }
        } else if (idx < SSD_MOA_LSTM_W(C) + wa_floats) {
            src = a.part_wa + (size_t)p * a.S * wa_pitch + (idx - SSD_MOA_LSTM_W(C)); pitch = wa_pitch; n = a.S;
        } else if (idx >= SSD_MOA_LSTM_B(C) && idx < SSD_MOA_LSTM_B(C) + 4 * C) {
            src = a.part_wa + (size_t)p * a.S * wa_pitch + wa_floats + (idx - SSD_MOA_LSTM_B(C)); pitch = wa_pitch; n = a.S;
        } else if (idx >= SSD_MOA_VALUE_W(C) && idx < SSD_MOA_VALUE_W(C) + C) {
            src = pseq + (idx - SSD_MOA_VALUE_W(C)) * 16 + A; pitch = seq_pitch; n = a.Gs;
        } else if (idx == SSD_MOA_VALUE_B(C)) {
            src = pseq + 16 * C + A; pitch = seq_pitch; n = a.Gs;
        } else if (idx >= SSD_MOA_LOGITS_W(C) && idx < SSD_MOA_LOGITS_W(C) + C * A) {
            const int q = idx - SSD_MOA_LOGITS_W(C);
            src = pseq + (q / A) * 16 + q % A; pitch = seq_pitch; n = a.Gs;
        } else if (idx >= SSD_MOA_LOGITS_B(C, A) && idx < SSD_MOA_LOGITS_B(C, A) + A) {
            src = pseq + 16 * C + (idx - SSD_MOA_LOGITS_B(C, A)); pitch = seq_pitch; n = a.Gs;
        } else if (idx >= SSD_MOA_MW(C, A) && idx < SSD_MOA_MW(C, A) + wm_floats) {
            const int q = idx - SSD_MOA_MW(C, A), row = q / (4 * C);
            if (row < kX + N || row >= kXM) { src = a.part_wm + (size_t)p * a.S * wm_pitch + q; pitch = wm_pitch; n = a.S; }
        } else if (idx >= SSD_MOA_MB(C, A) && idx < SSD_MOA_MB(C, A) + 4 * C) {
            src = a.part_wm + (size_t)p * a.S * wm_pitch + wm_floats + (idx - SSD_MOA_MB(C, A)); pitch = wm_pitch; n = a.S;
        } else if (idx >= SSD_MOA_PRED_W(C, A) && idx < SSD_MOA_PRED_W(C, A) + C * NA) {
            const int q = idx - SSD_MOA_PRED_W(C, A);
            src = a.part_pred + (size_t)p * a.S * pred_part + (size_t)(q / NA) * PP + q % NA; pitch = pred_part; n = a.S;
        } else if (idx >= SSD_MOA_PRED_B(C, A, N) && idx < SSD_MOA_PRED_B(C, A, N) + NA) {
            src = a.part_pred + (size_t)p * a.S * pred_part + (size_t)C * PP + (idx - SSD_MOA_PRED_B(C, A, N)); pitch = pred_part; n = a.S;
        }
        double sum = 0.0;
        for (int g = 0; g < n; ++g) sum += (double)src[g * pitch];
        a.grads[(size_t)p * a.set_floats + idx] = kSum ? (float)sum : (float)(sum / (double)a.set_rows);
    }
    if (kSum && blockIdx.x == 0 && threadIdx.x < 5) {
        const int k = threadIdx.x;
        double sum = 0.0, moa = 0.0;
        for (int g = 0; g < a.Gs; ++g) {
            const double *st = reinterpret_cast<const double *>(pseq + (size_t)g * seq_pitch + 16 * C + 16);
            sum += st[k];
            moa += st[5];
        }
        moa /= (double)a.set_rows;
        if (k == 0) sum += a.moa_weight * moa;
        a.stats[p * 5 + k] = k == 4 ? moa : sum;
    }
    if (!kSum && blockIdx.x == 0 && threadIdx.x < 6) {
        const int k = threadIdx.x;
        double sum = 0.0, moa = 0.0;
        for (int g = 0; g < a.Gs; ++g) {
            const double *st = reinterpret_cast<const double *>(pseq + (size_t)g * seq_pitch + 16 * C + 16);
            sum += st[k];
            moa += st[5];
        }
        if (k == 0) sum += a.moa_weight * moa;
        a.stats[p * 6 + k] = sum / (double)a.set_rows;
    }
}

template <int C>
hipError_t launch_window(int loss, ssd::BpttArgs a, const float *wT_act, const float *wT_moa, float *part_wa, float *part_wm,
                         hipStream_t stream) {
    const dim3 seq_grid((unsigned)a.G, (unsigned)a.P), w_grid(4 * C / 64, (unsigned)a.S, (unsigned)a.P);
    a.wT = wT_act; a.part_w = part_wa;
    if (loss == ssd::kLossAc) hipLaunchKernelGGL((ssd::ssd_bptt_seq_kernel<C, MoaActBranch, ssd::kLossAc>), seq_grid, dim3(4 * C), 0, stream, a);
    else hipLaunchKernelGGL((ssd::ssd_bptt_seq_kernel<C, MoaActBranch, ssd::kLossPpo>), seq_grid, dim3(4 * C), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd::ssd_bptt_dw_kernel<C, MoaActBranch>), w_grid, dim3(256), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    a.wT = wT_moa; a.part_w = part_wm;
    hipLaunchKernelGGL((ssd::ssd_bptt_seq_kernel<C, MoaPredBranch>), seq_grid, dim3(4 * C), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd::ssd_bptt_dw_kernel<C, MoaPredBranch>), w_grid, dim3(256), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd_moa_dpred_kernel<C>), dim3((unsigned)((a.pred_pitch + 63) / 64), (unsigned)a.S, (unsigned)a.P), dim3(256), 0,
                       stream, a);
    return hipGetLastError();
}

// Both entry points below: the checks, the window walk and the launches, with the row loss `loss` (the A3C call passes no
// logp_old, vf_preds or behaviour_logits and zeros for the hyper-parameters it does not have, which pass their checks).
int moa_grad(int loss, const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
             const uint8_t *obs_first, const uint8_t *obs, const float *state, const int32_t *prev_actions, const uint8_t *done,
             const int32_t *actions, const float *logp_old, const float *advantages, const float *value_targets,
             const float *vf_preds, const float *behaviour_logits, int32_t n_steps, int32_t num_envs, int32_t num_agents,
             double clip_param, double vf_clip_param, double vf_loss_coeff, double entropy_coeff, double kl_coeff, double moa_weight,
             float *scratch, float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream_) {
    const bool ac = loss == ssd::kLossAc;
    const ssd::GradCall call{ssd::kNetMoa, ac, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, prev_actions,
                             actions, logp_old, advantages, value_targets, vf_preds, behaviour_logits, n_steps, num_envs, num_agents,
                             clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, moa_weight, scratch, grads, stats, flags};
    if (const char *why = ssd::check_policy_grad(call)) return ssd::policy_fail(why);
    if (const int rc = ssd::policy_use_device(device_id)) return rc;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int K = n_steps, E = num_envs, N = num_agents, P = num_sets, A = num_actions, C = cell_size, T = seq_len;
    const int64_t rows = (int64_t)K * E * N;
    const int W = T < K ? T : K;                                     // steps of a whole window
    const size_t SR = (size_t)E * N, win_rows = (size_t)W * SR;
    const int seqs = (int)(SR / P);
    // the scratch: the blocks of SSD_MPPO_SCRATCH_FLOATS, in its order
    ssd::BpttArgs a{};
    a.w = weights; a.P = P; a.A = A; a.N = N; a.C = C; a.set_floats = SSD_MOA_SET_FLOATS(C, A, N);
    a.G = SSD_MPPO_GROUPS(seqs, P);
    a.S = SSD_MPPO_SPLITS((int64_t)W * seqs);
    a.pred_pitch = SSD_MPPO_PRED_PITCH(A, N);
    const int Gt = SSD_PPO_GROUPS((int32_t)(W * (int64_t)seqs), P);
    a.seqs = seqs; a.step_rows = (int32_t)SR;
    a.h = ssd::PpoHyper{(float)clip_param, (float)vf_clip_param, (float)vf_loss_coeff, (float)entropy_coeff, (float)kl_coeff};
    // (the A3C terms are sums over a set's rows and MOALoss a mean: its 1 / rows is folded in here, in double, rounded once)
    a.moa_scale = ac ? (float)(moa_weight / ((double)(N - 1) * (double)(rows / P))) : (float)(moa_weight / (double)(N - 1));
    const size_t wa_floats = (size_t)(kX + C) * 4 * C, wm_floats = (size_t)(kXM + C) * 4 * C;
    float *at = scratch;
    float *wT_act = at; at += (size_t)P * wa_floats;
    float *wT_moa = at; at += (size_t)P * wm_floats;
    a.feat = at; at += win_rows * 2 * kX;
    a.dx = at; at += win_rows * 2 * kX;
    a.st = at; at += win_rows * 2 * C;
    a.gz = at; at += win_rows * 4 * C;
    a.dpred = at; at += win_rows * a.pred_pitch;
    float *part_trunk = at; at += (size_t)P * Gt * (SSD_MOA_LSTM_W(C) + kStatFloats);
    a.part_seq = at; at += (size_t)P * a.G * (16 * C + 16 + kStatFloats);
    float *part_wa = at; at += (size_t)P * a.S * (wa_floats + 4 * C);
    float *part_wm = at; at += (size_t)P * a.S * (wm_floats + 4 * C);
    a.part_pred = at;

    hipLaunchKernelGGL(ssd::ssd_bptt_transpose_kernel, dim3((unsigned)((wa_floats + 255) / 256), (unsigned)P), dim3(256), 0, stream, weights,
                       a.set_floats, SSD_MOA_LSTM_W(C), kX + C, 4 * C, wT_act);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);
    hipLaunchKernelGGL(ssd::ssd_bptt_transpose_kernel, dim3((unsigned)((wm_floats + 255) / 256), (unsigned)P), dim3(256), 0, stream, weights,
                       a.set_floats, SSD_MOA_MW(C, A), kXM + C, 4 * C, wT_moa);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);

    ssd::PolicyArgs f{};
    f.w = weights; f.P = P; f.A = A; f.N = N; f.set_floats = a.set_floats; f.feat = a.feat;
    for (int k0 = 0; k0 < K; k0 += T) {
        const int steps = K - k0 < T ? K - k0 : T;
        const ssd::GradWindow o = ssd::grad_window(obs_first, obs, k0, SR);
        // 1. the features of both stacks
        hipError_t e = ssd::launch_window_features(f, true, o, steps, E, SR * 2 * kX, stream);
        if (e != hipSuccess) return ssd::policy_launched(e);
        // 2, 3. the two branches
        a.steps = steps; a.accumulate = k0 > 0;
        a.ring = state + (size_t)(k0 / T) * SR * 4 * C;
        a.done_prev = done ? done + (size_t)k0 * SR : nullptr;      // step t > 0 of the window looks at done[k0 + t - 1]
        const size_t r0 = (size_t)k0 * SR;
        a.actions = actions + r0; a.prev = prev_actions + r0; a.adv = advantages + r0; a.vt = value_targets + r0;
        a.logp_old = logp_old ? logp_old + r0 : nullptr; a.vf_pred = vf_preds ? vf_preds + r0 : nullptr;
        a.beh = behaviour_logits ? behaviour_logits + r0 * A : nullptr;
        switch (C) {
        case 64: e = launch_window<64>(loss, a, wT_act, wT_moa, part_wa, part_wm, stream); break;
        case 128: e = launch_window<128>(loss, a, wT_act, wT_moa, part_wa, part_wm, stream); break;
        default: e = launch_window<256>(loss, a, wT_act, wT_moa, part_wa, part_wm, stream); break;
        }
        if (e != hipSuccess) return ssd::policy_launched(e);
        // 4. the trunk's backward from dx, once per stack
        ssd::PpoGradArgs tg = ssd::window_trunk_args(f, o, SSD_MOA_LSTM_W(C), Gt, steps * seqs, (int32_t)SR, part_trunk, a.dx, a.accumulate);
        for (int s = 0; s < 2; ++s) {
            tg.stack = s;
            e = ssd::launch_ppo_moa_stack_grad(tg, stream);
            if (e != hipSuccess) return ssd::policy_launched(e);
        }
    }
    ReduceArgs r{};
    r.P = P; r.A = A; r.N = N; r.C = C; r.set_floats = a.set_floats; r.set_rows = (int32_t)(rows / P); r.Gt = Gt; r.Gs = a.G; r.S = a.S;
    r.pred_pitch = a.pred_pitch; r.moa_weight = moa_weight;
    r.part_trunk = part_trunk; r.part_seq = a.part_seq; r.part_wa = part_wa; r.part_wm = part_wm; r.part_pred = a.part_pred;
    r.grads = grads; r.stats = stats;
    const dim3 reduce_grid((unsigned)((a.set_floats + 255) / 256), (unsigned)P);
    if (ac) hipLaunchKernelGGL(ssd_moa_reduce_kernel<ssd::kLossAc>, reduce_grid, dim3(256), 0, stream, r);
    else hipLaunchKernelGGL(ssd_moa_reduce_kernel<ssd::kLossPpo>, reduce_grid, dim3(256), 0, stream, r);
    return ssd::policy_launched(hipGetLastError());
}

}  // namespace

extern "C" int ssd_policy_moa_ppo_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size,
                                       int32_t seq_len, const uint8_t *obs_first, const uint8_t *obs, const float *state,
                                       const int32_t *prev_actions, const uint8_t *done, const int32_t *actions,
                                       const float *logp_old, const float *advantages, const float *value_targets,
                                       const float *vf_preds, const float *behaviour_logits, int32_t n_steps, int32_t num_envs,
                                       int32_t num_agents, double clip_param, double vf_clip_param, double vf_loss_coeff,
                                       double entropy_coeff, double kl_coeff, double moa_weight, float *scratch, float *grads,
                                       double *stats, int32_t device_id, uint32_t flags, void *stream) {
    return moa_grad(ssd::kLossPpo, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, prev_actions, done,
                    actions, logp_old, advantages, value_targets, vf_preds, behaviour_logits, n_steps, num_envs, num_agents,
                    clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, moa_weight, scratch, grads, stats, device_id,
                    flags, stream);
}

extern "C" int ssd_policy_moa_ac_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size,
                                      int32_t seq_len, const uint8_t *obs_first, const uint8_t *obs, const float *state,
                                      const int32_t *prev_actions, const uint8_t *done, const int32_t *actions,
                                      const float *advantages, const float *value_targets, int32_t n_steps, int32_t num_envs,
                                      int32_t num_agents, double vf_loss_coeff, double entropy_coeff, double moa_weight,
                                      float *scratch, float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream) {
    return moa_grad(ssd::kLossAc, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, prev_actions, done,
                    actions, nullptr, advantages, value_targets, nullptr, nullptr, n_steps, num_envs, num_agents, 0.0, 0.0,
                    vf_loss_coeff, entropy_coeff, 0.0, moa_weight, scratch, grads, stats, device_id, flags, stream);
}
