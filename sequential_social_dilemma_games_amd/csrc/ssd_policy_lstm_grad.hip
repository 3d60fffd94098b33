// ssd_policy_lstm_grad.hip -- RLlib's PPO loss of the recurrent policy (the conv-FC trunk under RLlib's LSTM) on a sampled
// fragment with truncated backpropagation through time, its statistics and the gradient of every parameter:
// ssd_policy_lstm_ppo_grad.  include/ssd.h states the contract (the state rule, the rows, the order of the sums); DESIGN.md
// section 17 the shape, the resource report and the measurements.
//
// The fragment is walked window by window (seq_len steps, the last one possibly shorter) by a host loop that only enqueues.
// Per window, on the caller's scratch, with the kernels of ssd_bptt_device.hpp instantiated for LstmBranch below:
//   1. features: the trunk kernel's features mode (ssd_policy.hip) over the window's rows -> feat [rows][32];
//   2. ssd_bptt_seq_kernel: a workgroup of 4 C threads takes 16 sequences of one weight set (persistent over tiles g, g + G,
//      ...).  Forward over the window's steps: h' stays in LDS, the gate activations, c' and h' of every row go to scratch, the
//      loss terms of a row (ppo_row, as ssd_policy_grad.hip) to float64 sums and d row_loss / d (logits, value) to the row's dx
//      slot.  Then backward over the steps in reverse: the heads' kernels and biases summed in registers (fixed entries per
//      thread), dh' = heads^T d + the dh carried from step t + 1, the gate derivatives dz (16 x 4C) to LDS and over the
//      activations in scratch, d [x, h_prev] = dz lstm_w^T on the matrix cores (B from a transposed copy of lstm_w made once
//      per call): dx to scratch, dh_prev and dc_prev stay in the registers of the lane that owns the (row, cell) pair, and are
//      zeroed where the step's state was selected zero;
//   3. ssd_bptt_dw_kernel: d lstm_w = [x, h_prev]^T dz on the matrix cores, split over a fixed partition of the set's rows
//      (split s takes the 64-row chunks s, s + S, ...), lstm_b the column sums of dz;
//   4. the trunk's backward from dx: ssd_policy_grad.hip's kernel, its steps from fc2 down (launch_ppo_trunk_grad).
// Every kernel adds its partial sums to what scratch holds from the windows before (the first window stores).  At the end
// ssd_lstm_reduce_kernel adds the partials of every entry in order in float64, scales by 1 / set rows and rounds once.  No
// atomics anywhere: the same inputs give the same bits.
//
// ssd_policy_lstm_ac_grad is the same walk with the A3C row loss (include/ssd.h, A3C LOSS AND GRADIENTS):
// the sequence kernel and the reduce compiled once more with ssd::kLossAc (a3c_row for ppo_row; no division by the rows).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_bptt_device.hpp"

namespace {

constexpr int kX = SSD_LSTM_X;          // trunk features per row
constexpr int kStatFloats = SSD_PPO_STAT_FLOATS;

// The recurrent policy's one branch: RLlib's cell on the trunk's 32 features, a two-row state (c, h), the policy head.
struct LstmBranch {
    using Cell = ssd::RllibCell;
    static constexpr int kIn = kX, kFeatPitch = kX, kFeat0 = 0, kRingRows = 2, kRing0 = 0, kPad = 36;
    static constexpr bool kPred = false;
    static constexpr int w(int, int) { return SSD_LSTM_W; }
    static constexpr int b(int C, int) { return SSD_LSTM_B(C); }
    static constexpr int logits_w(int C) { return SSD_LSTM_LOGITS_W(C); }
    static constexpr int value_w(int C) { return SSD_LSTM_VALUE_W(C); }
    static constexpr int logits_b(int C, int A) { return SSD_LSTM_LOGITS_B(C, A); }
    static constexpr int value_b(int C) { return SSD_LSTM_VALUE_B(C); }
};

// ------------------------------------------------------------------------------------------------------ the final reduce
struct ReduceArgs {
    int32_t P, A, C, set_floats, set_rows, Gt, Gs, S;
    const float *part_trunk;       // [P][Gt][SSD_LSTM_W + kStatFloats]
    const float *part_seq;         // [P][Gs][16 C + 16 + kStatFloats]
    const float *part_w;           // [P][S][(32 + C) 4C + 4C]
    float *grads;                  // [P][set_floats]
    double *stats;                 // [P][5]
};

// The partials of every entry added in order in float64, times 1 / set rows, rounded once; the padding floats are zero.
// kLossAc: the sums as they are (the A3C loss is a sum over rows), and the four statistics of a3c_row to stats [P][4].
template <int kLoss>
__global__ void __launch_bounds__(256) ssd_lstm_reduce_kernel(ReduceArgs a) {
    constexpr bool kSum = kLoss == ssd::kLossAc;
    constexpr int kStats = kSum ? 4 : 5;
    const int idx = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y, C = a.C, A = a.A;
    const int seq_pitch = 16 * C + 16 + kStatFloats, w_floats = (kX + C) * 4 * C, w_pitch = w_floats + 4 * C;
    const float *pseq = a.part_seq + (size_t)p * a.Gs * seq_pitch;
    if (idx < a.set_floats) {
        const float *src = nullptr;
        size_t pitch = 0;
        int n = 0;
        if (idx < SSD_POL_FC2_B + 32) {
            src = a.part_trunk + (size_t)p * a.Gt * (SSD_LSTM_W + kStatFloats) + idx; pitch = SSD_LSTM_W + kStatFloats; n = a.Gt;
        } else if (idx >= SSD_LSTM_W && idx < SSD_LSTM_W + w_floats) {
            src = a.part_w + (size_t)p * a.S * w_pitch + (idx - SSD_LSTM_W); pitch = w_pitch; n = a.S;
        } else if (idx >= SSD_LSTM_B(C) && idx < SSD_LSTM_B(C) + 4 * C) {
            src = a.part_w + (size_t)p * a.S * w_pitch + w_floats + (idx - SSD_LSTM_B(C)); pitch = w_pitch; n = a.S;
        } else if (idx >= SSD_LSTM_VALUE_W(C) && idx < SSD_LSTM_VALUE_W(C) + C) {
            src = pseq + (idx - SSD_LSTM_VALUE_W(C)) * 16 + A; pitch = seq_pitch; n = a.Gs;
        } else if (idx == SSD_LSTM_VALUE_B(C)) {
            src = pseq + 16 * C + A; pitch = seq_pitch; n = a.Gs;
        } else if (idx >= SSD_LSTM_LOGITS_W(C) && idx < SSD_LSTM_LOGITS_W(C) + C * A) {
            const int q = idx - SSD_LSTM_LOGITS_W(C);
            src = pseq + (q / A) * 16 + q % A; pitch = seq_pitch; n = a.Gs;
        } else if (idx >= SSD_LSTM_LOGITS_B(C, A) && idx < SSD_LSTM_LOGITS_B(C, A) + A) {
            src = pseq + 16 * C + (idx - SSD_LSTM_LOGITS_B(C, A)); pitch = seq_pitch; n = a.Gs;
        }
        double sum = 0.0;
        for (int g = 0; g < n; ++g) sum += (double)src[g * pitch];
        a.grads[(size_t)p * a.set_floats + idx] = kSum ? (float)sum : (float)(sum / (double)a.set_rows);
    }
    if (blockIdx.x == 0 && threadIdx.x < kStats) {
        double sum = 0.0;
        for (int g = 0; g < a.Gs; ++g) sum += reinterpret_cast<const double *>(pseq + (size_t)g * seq_pitch + 16 * C + 16)[threadIdx.x];
        a.stats[p * kStats + threadIdx.x] = kSum ? sum : sum / (double)a.set_rows;
    }
}

template <int C>
hipError_t launch_window(int loss, const ssd::BpttArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.G, (unsigned)a.P);
    if (loss == ssd::kLossAc) hipLaunchKernelGGL((ssd::ssd_bptt_seq_kernel<C, LstmBranch, ssd::kLossAc>), grid, dim3(4 * C), 0, stream, a);
    else hipLaunchKernelGGL((ssd::ssd_bptt_seq_kernel<C, LstmBranch, ssd::kLossPpo>), grid, dim3(4 * C), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd::ssd_bptt_dw_kernel<C, LstmBranch>), dim3(4 * C / 64, (unsigned)a.S, (unsigned)a.P), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// Both entry points below: the checks, the window walk and the launches, with the row loss `loss` (the A3C call passes no
// logp_old, vf_preds or behaviour_logits and zeros for the hyper-parameters it does not have, which pass their checks).
int lstm_grad(int loss, const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
              const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done, const int32_t *actions,
              const float *logp_old, const float *advantages, const float *value_targets, const float *vf_preds,
              const float *behaviour_logits, int32_t n_steps, int32_t num_envs, int32_t num_agents, double clip_param,
              double vf_clip_param, double vf_loss_coeff, double entropy_coeff, double kl_coeff, float *scratch, float *grads,
              double *stats, int32_t device_id, uint32_t flags, void *stream_) {
    const bool ac = loss == ssd::kLossAc;
    const ssd::GradCall call{ssd::kNetLstm, ac, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, nullptr, actions,
                             logp_old, advantages, value_targets, vf_preds, behaviour_logits, n_steps, num_envs, num_agents, clip_param,
                             vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, 0.0, scratch, grads, stats, flags};
    if (const char *why = ssd::check_policy_grad(call)) return ssd::policy_fail(why);
    if (const int rc = ssd::policy_use_device(device_id)) return rc;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int K = n_steps, E = num_envs, N = num_agents, P = num_sets, A = num_actions, C = cell_size, T = seq_len;
    const int64_t rows = (int64_t)K * E * N;
    const int W = T < K ? T : K;                                     // steps of a whole window
    const size_t SR = (size_t)E * N, win_rows = (size_t)W * SR;
    const int seqs = (int)(SR / P);
    // the scratch: the blocks of SSD_RPPO_SCRATCH_FLOATS, in its order
    ssd::BpttArgs a{};
    a.w = weights; a.P = P; a.A = A; a.N = N; a.C = C; a.set_floats = SSD_LSTM_SET_FLOATS(C, A);
    a.G = SSD_RPPO_GROUPS(seqs, P);
    a.S = SSD_RPPO_SPLITS((int64_t)W * seqs);
    const int Gt = SSD_PPO_GROUPS((int32_t)(W * (int64_t)seqs), P);
    a.seqs = seqs; a.step_rows = (int32_t)SR;
    a.h = ssd::PpoHyper{(float)clip_param, (float)vf_clip_param, (float)vf_loss_coeff, (float)entropy_coeff, (float)kl_coeff};
    float *at = scratch;
    float *wT = at; at += (size_t)P * (kX + C) * 4 * C;
    a.wT = wT;
    a.feat = at; at += win_rows * kX;
    a.dx = at; at += win_rows * kX;
    a.st = at; at += win_rows * 2 * C;
    a.gz = at; at += win_rows * 4 * C;
    float *part_trunk = at; at += (size_t)P * Gt * (SSD_LSTM_W + kStatFloats);
    a.part_seq = at; at += (size_t)P * a.G * (16 * C + 16 + kStatFloats);
    a.part_w = at;

    hipLaunchKernelGGL(ssd::ssd_bptt_transpose_kernel, dim3((unsigned)(((kX + C) * 4 * C + 255) / 256), (unsigned)P), dim3(256), 0, stream,
                       weights, a.set_floats, SSD_LSTM_W, kX + C, 4 * C, wT);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);

    ssd::PolicyArgs f{};
    f.w = weights; f.P = P; f.A = A; f.N = N; f.set_floats = a.set_floats; f.feat = a.feat;
    for (int k0 = 0; k0 < K; k0 += T) {
        const int steps = K - k0 < T ? K - k0 : T;
        const ssd::GradWindow o = ssd::grad_window(obs_first, obs, k0, SR);
        // 1. the features
        hipError_t e = ssd::launch_window_features(f, false, o, steps, E, SR * kX, stream);
        if (e != hipSuccess) return ssd::policy_launched(e);
        // 2, 3. the sequences, then lstm_w
        a.steps = steps; a.accumulate = k0 > 0;
        a.ring = state + (size_t)(k0 / T) * SR * 2 * C;
        a.done_prev = done ? done + (size_t)k0 * SR : nullptr;      // step t > 0 of the window looks at done[k0 + t - 1]
        const size_t r0 = (size_t)k0 * SR;
        a.actions = actions + r0; a.adv = advantages + r0; a.vt = value_targets + r0;
        a.logp_old = logp_old ? logp_old + r0 : nullptr; a.vf_pred = vf_preds ? vf_preds + r0 : nullptr;
        a.beh = behaviour_logits ? behaviour_logits + r0 * A : nullptr;
        switch (C) {
        case 64: e = launch_window<64>(loss, a, stream); break;
        case 128: e = launch_window<128>(loss, a, stream); break;
        default: e = launch_window<256>(loss, a, stream); break;
        }
        if (e != hipSuccess) return ssd::policy_launched(e);
        // 4. the trunk's backward from dx
        e = ssd::launch_ppo_trunk_grad(ssd::window_trunk_args(f, o, SSD_LSTM_W, Gt, steps * seqs, (int32_t)SR, part_trunk, a.dx, a.accumulate),
                                       stream);
        if (e != hipSuccess) return ssd::policy_launched(e);
    }
    ReduceArgs r{};
    r.P = P; r.A = A; r.C = C; r.set_floats = a.set_floats; r.set_rows = (int32_t)(rows / P); r.Gt = Gt; r.Gs = a.G; r.S = a.S;
    r.part_trunk = part_trunk; r.part_seq = a.part_seq; r.part_w = a.part_w; r.grads = grads; r.stats = stats;
    const dim3 reduce_grid((unsigned)((a.set_floats + 255) / 256), (unsigned)P);
    if (ac) hipLaunchKernelGGL(ssd_lstm_reduce_kernel<ssd::kLossAc>, reduce_grid, dim3(256), 0, stream, r);
    else hipLaunchKernelGGL(ssd_lstm_reduce_kernel<ssd::kLossPpo>, reduce_grid, dim3(256), 0, stream, r);
    return ssd::policy_launched(hipGetLastError());
}

}  // namespace

extern "C" int ssd_policy_lstm_ppo_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size,
                                        int32_t seq_len, const uint8_t *obs_first, const uint8_t *obs, const float *state,
                                        const uint8_t *done, const int32_t *actions, const float *logp_old,
                                        const float *advantages, const float *value_targets, const float *vf_preds,
                                        const float *behaviour_logits, int32_t n_steps, int32_t num_envs, int32_t num_agents,
                                        double clip_param, double vf_clip_param, double vf_loss_coeff, double entropy_coeff,
                                        double kl_coeff, float *scratch, float *grads, double *stats, int32_t device_id,
                                        uint32_t flags, void *stream) {
    return lstm_grad(ssd::kLossPpo, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, done, actions,
                     logp_old, advantages, value_targets, vf_preds, behaviour_logits, n_steps, num_envs, num_agents, clip_param,
                     vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, scratch, grads, stats, device_id, flags, stream);
}

extern "C" int ssd_policy_lstm_ac_grad(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size,
                                       int32_t seq_len, const uint8_t *obs_first, const uint8_t *obs, const float *state,
                                       const uint8_t *done, const int32_t *actions, const float *advantages,
                                       const float *value_targets, int32_t n_steps, int32_t num_envs, int32_t num_agents,
                                       double vf_loss_coeff, double entropy_coeff, float *scratch, float *grads, double *stats,
                                       int32_t device_id, uint32_t flags, void *stream) {
    return lstm_grad(ssd::kLossAc, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, done, actions, nullptr,
                     advantages, value_targets, nullptr, nullptr, n_steps, num_envs, num_agents, 0.0, 0.0, vf_loss_coeff,
                     entropy_coeff, 0.0, scratch, grads, stats, device_id, flags, stream);
}
