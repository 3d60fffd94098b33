// ssd_policy_grad.hip -- RLlib's PPO loss of the conv-FC policy network on a sampled fragment, its statistics and the gradient of
// every parameter: ssd_policy_ppo_grad.  include/ssd.h states the contract (rows, the observation shift, the loss, the derivatives
// at the kinks, the order of the sums); DESIGN.md section 16 the shape and the measurements.
//
// Workgroups are persistent: workgroup (g, p) of a (G, P) grid takes the 16-row tiles g, g + G, ... of weight set p, so what a
// workgroup sums, and in which order, is a function of (K, E, N, P) alone.  Per tile:
//   1. the forward of ssd_policy.hip from the shared pieces (conv_tile and fc_stack, head): conv output, h1, h2, the logits and
//      the value stay in LDS;
//   2. one thread per row: the loss terms, the statistics (float64 sums) and d row_loss / d (logits, value);
//   3. the backward through the heads, fc2 and fc1 on the VALU (a few kMAC per row), each thread keeping the sums of the
//      gradient entries it owns in registers across tiles;
//   4. dW1 += conv^T dh1 (1014 x 16 . 16 x 32) on the matrix cores, v_mfma_f32_16x16x4_f32: wave w owns rows 256 w .. 256 w + 255
//      of dW1, 32 accumulator tiles = 128 registers a lane, kept across tiles;
//   5. dconv = dh1 W1^T (16 x 32 . 32 x 1014) on the matrix cores, masked by the conv's ReLU and written over the conv output in
//      LDS (wave w writes the 256 columns only it read in 4);
//   6. the conv's weight gradient: thread (tap, slice) sums x[tap] * dconv[f] over every ninth (row, position) for the six
//      filters; the slices are added in order when the workgroup is done.
// At the end a workgroup writes its partial gradient set and statistics to the caller's scratch; a second kernel adds the G
// partials of a set in order (float64), scales by 1 / rows and rounds once.  No atomics anywhere: the same inputs give the same
// bits.  The kernel's second instantiation is the trunk's backward alone, from a given d loss / d fc2's output: what the
// recurrent policy's call (ssd_policy_lstm_grad.hip) runs below its cell.  The third is that backward for one tanh FC stack of
// the MOA policy (ssd_policy_moa_grad.hip), launched once per stack.
//
// ssd_policy_ac_grad is the same call with the A3C row loss (include/ssd.h, A3C LOSS AND GRADIENTS): the
// loss kernel and the reduce compiled once more with ssd::kLossAc -- a3c_row for ppo_row, and the float64 totals rounded as they
// are, without the division by the rows -- from the same host code.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"

namespace {

using namespace ssd::trunk;      // the tile constants, conv_tile and fc_stack (ssd_policy_device.hpp)
using ssd::f32x4;

constexpr int kSlices = 9;                  // step 6: 27 taps x 9 slices = 243 threads
constexpr int kStatFloats = SSD_PPO_STAT_FLOATS;

using GradArgs = ssd::PpoGradArgs;

// kFromDx: the trunk's backward alone, for the recurrent policy (ssd_policy_lstm_grad.hip): steps 1 (to fc2) and 3 (from fc2
// down) to 6, with d loss / d fc2's output read from a.dx instead of formed from the heads; nothing of the heads or the
// statistics is summed or written, and with a.accumulate the partial set is added to what scratch holds (the windows before).
//
// kModeMoaStack: kModeFromDx for stack a.stack of the MOA policy: the stack's weights at SSD_MOA_FC1_W(stack), tanh for ReLU
// after fc1 and fc2 (derivative 1 - h * h), dx rows [.][2][32] of which the stack's half is read, and a partial set in the MOA
// layout's offsets.  The conv's gradient is linear in d conv, so stack 1's launch adds its conv sums onto what stack 0's launch
// left in the same slot (the same workgroup, after it on the stream): the order is fixed.
constexpr int kModeLoss = 0, kModeFromDx = 1, kModeMoaStack = 2;

// kLoss (kModeLoss only): the row loss of step 2, ssd::kLossPpo or ssd::kLossAc (the A3C terms: a3c_row in ppo_row's place, four
// statistics).  Everything else is the same code.
template <int kMode, int kLoss = ssd::kLossPpo>
__global__ void __launch_bounds__(kThreads) ssd_ppo_grad_kernel(GradArgs a) {
    constexpr bool kFromDx = kMode != kModeLoss, kTanh = kMode == kModeMoaStack;
    constexpr int kDxPitch = kTanh ? 64 : 32;
    __shared__ float s_norm[256];
    __shared__ float s_conv[kTile * kPitch + 8];       // the conv output; after step 5, d loss / d conv.  (+ 8: step 4's last A rows)
    __shared__ float s_obsf[(kTile * kObs + 3) / 4];   // the observation bytes
    __shared__ float s_part[512];                      // [2][16][16] fc1 partial sums of the second K half
    __shared__ float s_h1[kTile * kHP], s_h2[kTile * kHP], s_dh1[kTile * kHP], s_dh2[kTile * kHP];
    __shared__ float s_out[kTile * 16];                // logits 0..A-1, value at A
    __shared__ float s_dout[kTile * 16];               // d row_loss / d (logits, value); zero beyond A and for rows past the set
    __shared__ double s_stat[kTile * 5];
    uint8_t *s_obs = reinterpret_cast<uint8_t *>(s_obsf);

    const int tid = threadIdx.x, g = blockIdx.x, p = blockIdx.y;
    const int A = a.A, R = a.set_rows;
    const int stride = a.P == 1 ? 1 : a.N;             // a set's row r is row r * stride + p of the [K][E][N] arrays
    const float *w_set = a.w + (size_t)p * (size_t)(kFromDx ? a.w_pitch : a.set_floats);
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int shift = kTanh ? SSD_MOA_FC1_W(a.stack) - SSD_POL_FC1_W : 0;   // from the trunk's FC offsets to the stack's
    const auto dact = [](float h, float d) { return kTanh ? d * (1.f - h * h) : (h > 0.f ? d : 0.f); };

    s_norm[tid] = (float)(((double)tid - 128.0) / 255.0);
    if (tid < kTile * (kPitch - kFlat)) s_conv[(tid / 3) * kPitch + kFlat + tid % 3] = 0.f;
    if (tid < 8) s_conv[kTile * kPitch + tid] = 0.f;

    // the sums this thread owns, kept across tiles
    f32x4 acc_w1[16][2];                               // step 4: dW1 rows 16 (16 wave + t) + 4 l4 + r, column 16 c + l15
#pragma unroll
    for (int t = 0; t < 16; ++t) acc_w1[t][0] = acc_w1[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float acc_hd[2] = {0.f, 0.f};                      // heads' kernels: entry q = tid + 256 u is (k, j) = (q >> 4, q & 15); j == A: the value
    float acc_w2[4] = {0.f, 0.f, 0.f, 0.f};            // fc2_w entry q = tid + 256 u is (k, n) = (q >> 5, q & 31)
    float acc_b1 = 0.f, acc_b2 = 0.f, acc_bh = 0.f;    // tid < 32: fc1_b, fc2_b; tid < 16: the heads' biases
    float acc_cw[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // step 6: conv_w [tap][f] of this thread's slice
    float acc_cb[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // ... and conv_b [f] (tap 0's threads)
    double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};          // tid < 16: total, policy, vf, kl, entropy of tile row tid

    const int tiles = R / kTile + (R % kTile != 0);
    for (int tile = g; tile < tiles; tile += a.G) {
        const int r0 = tile * kTile;
        // (the weights' address passes through an empty asm each tile: without it every weight load of the body is loop
        // invariant, the compiler hoists some hundreds of them out of the tile loop and spills them)
        asm volatile("" : "+s"(w_set));
        const float *__restrict__ w = w_set;
        const float *__restrict__ ws = w_set + shift;      // the FC layers' base
        __syncthreads();                               // the previous tile's step 6 has read s_obs and s_conv
        // ---- 1. the forward ----
        {   // 16 threads a row, byte c + 16 u of it each (every load of the thread issued before the first store)
            constexpr int kLoads = (kObs + 15) / 16;
            const int m = tid >> 4, c = tid & 15, r = r0 + m;
            const uint8_t *src = nullptr;
            if (r < R) {
                const size_t row = (size_t)r * stride + p;
                if (!a.obs_first) src = a.obs + row * kObs + c;
                else if (row < (size_t)a.step_rows) src = a.obs_first + row * kObs + c;     // k = 0
                else src = a.obs + (row - a.step_rows) * kObs + c;                          // row k reads obs[k - 1]
            }
            uint8_t v[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) v[u] = src && c + 16 * u < kObs ? src[16 * u] : (uint8_t)128;
#pragma unroll
            for (int u = 0; u < kLoads; ++u)
                if (c + 16 * u < kObs) s_obs[m * kObs + c + 16 * u] = v[u];
        }
        __syncthreads();
        conv_tile(w, s_obs, s_norm, s_conv, tid);
        __syncthreads();
        fc_stack<kTanh>(ws, s_conv, s_part, s_h1, tid, s_h2, kHP, kTile);
        __syncthreads();
        if constexpr (!kFromDx) {
            const int m = tid >> 4, j = tid & 15;
            if (j <= A)
                s_out[tid] = ssd::head<32>(s_h2 + m * kHP, w + SSD_POL_LOGITS_W, w + SSD_POL_VALUE_W, w + SSD_POL_LOGITS_W + 32 * A,
                                           w + SSD_POL_VALUE_B, A, j);
            s_dout[tid] = 0.f;
        }
        __syncthreads();

        // ---- 2. the loss terms of row tid and their derivatives ----
        if (!kFromDx && tid < kTile && r0 + tid < R) {
            const size_t row = (size_t)(r0 + tid) * stride + p;
            int act = a.actions[row];
            act = act < 0 ? 0 : (act >= A ? A - 1 : act);
            const ssd::PpoHyper hyper{a.clip, a.vf_clip, a.vf_coeff, a.ent_coeff, a.kl_coeff};
            if constexpr (kLoss == ssd::kLossAc)
                ssd::a3c_row(s_out + tid * 16, s_dout + tid * 16, A, act, a.adv[row], a.vt[row], hyper, st);
            else
                ssd::ppo_row(s_out + tid * 16, s_dout + tid * 16, A, act, a.adv[row], a.vt[row], a.vf_pred[row], a.logp_old[row],
                             a.beh ? a.beh + row * A : nullptr, hyper, st);
        }
        __syncthreads();

        // ---- 3. the backward through the heads, fc2 and fc1's activation ----
        if constexpr (kFromDx) {                       // dh2 from the caller's rows, through h2's ReLU
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int q = tid + u * kThreads, m = q >> 5, n = q & 31;
                const float dh = r0 + m < R ? a.dx[((size_t)(r0 + m) * stride + p) * kDxPitch + (kTanh ? 32 * a.stack : 0) + n] : 0.f;
                s_dh2[m * kHP + n] = dact(s_h2[m * kHP + n], dh);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u) {                  // the heads' kernels, and dh2 through h2's ReLU
                const int q = tid + u * kThreads, k = q >> 4, j = q & 15;
                float sum = 0.f;
#pragma unroll
                for (int m = 0; m < kTile; ++m) sum = fmaf(s_h2[m * kHP + k], s_dout[m * 16 + j], sum);
                acc_hd[u] += sum;
                const int m = q >> 5, n = q & 31;          // dh2[m][n] = sum_j dout[m][j] * W[n][j]
                float dh = 0.f;
                for (int jj = 0; jj < A; ++jj) dh = fmaf(s_dout[m * 16 + jj], w[SSD_POL_LOGITS_W + n * A + jj], dh);
                dh = fmaf(s_dout[m * 16 + A], w[SSD_POL_VALUE_W + n], dh);
                s_dh2[m * kHP + n] = s_h2[m * kHP + n] > 0.f ? dh : 0.f;
            }
            if (tid < 16) {
                float sum = 0.f;
#pragma unroll
                for (int m = 0; m < kTile; ++m) sum += s_dout[m * 16 + tid];
                acc_bh += sum;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {                  // fc2's kernel
            const int q = tid + u * kThreads, k = q >> 5, n = q & 31;
            float sum = 0.f;
#pragma unroll
            for (int m = 0; m < kTile; ++m) sum = fmaf(s_h1[m * kHP + k], s_dh2[m * kHP + n], sum);
            acc_w2[u] += sum;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {                  // dh1[m][k] = sum_n dh2[m][n] * fc2_w[k][n], through h1's ReLU
            const int q = tid + u * kThreads, m = q >> 5, k = q & 31;
            float dh = 0.f;
#pragma unroll 8
            for (int n = 0; n < 32; ++n) dh = fmaf(s_dh2[m * kHP + n], ws[SSD_POL_FC2_W + k * 32 + n], dh);
            s_dh1[m * kHP + k] = dact(s_h1[m * kHP + k], dh);
        }
        if (tid < 32) {
            float sum = 0.f;
#pragma unroll
            for (int m = 0; m < kTile; ++m) sum += s_dh2[m * kHP + tid];
            acc_b2 += sum;
        }
        __syncthreads();
        if (tid < 32) {
            float sum = 0.f;
#pragma unroll
            for (int m = 0; m < kTile; ++m) sum += s_dh1[m * kHP + tid];
            acc_b1 += sum;
        }

        // ---- 4. dW1 += conv^T dh1: A[c][m] = conv[m][c], B[m][n] = dh1[m][n] (the lane layout: ssd_policy_device.hpp) ----
        {
            const float *a_base = s_conv + l4 * kPitch + 256 * wave + l15;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const float b0 = s_dh1[(4 * ks + l4) * kHP + l15], b1 = s_dh1[(4 * ks + l4) * kHP + 16 + l15];
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const float av = a_base[4 * ks * kPitch + 16 * t];
                    acc_w1[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc_w1[t][0], 0, 0, 0);
                    acc_w1[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc_w1[t][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();

        // ---- 5. dconv = dh1 W1^T through the conv's ReLU, over the conv output: A[m][k] = dh1[m][k], B[k][c] = fc1_w[c][k] ----
        {
            float av[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) av[ks] = s_dh1[l15 * kHP + 4 * ks + l4];
#pragma unroll 2
            for (int t = 0; t < 16; ++t) {
                const int c = 256 * wave + 16 * t + l15;
                const float *wc = ws + SSD_POL_FC1_W + (size_t)c * 32 + l4;
                float bv[8];
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) bv[ks] = c < kFlat ? wc[4 * ks] : 0.f;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv[ks], acc, 0, 0, 0);
                if (c < kFlat) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float *dst = s_conv + (4 * l4 + r) * kPitch + c;
                        *dst = *dst > 0.f ? acc[r] : 0.f;
                    }
                }
            }
        }
        __syncthreads();

        // ---- 6. the conv's weight gradient: thread (tap, slice) over (row, position) slice, slice + 9, ... ----
        if (tid < 27 * kSlices) {
            const int tap = tid / kSlices, sl = tid - tap * kSlices;     // tap = dy * 9 + j: byte dy * 45 + j of the window
            const int off = (tap / 9) * 45 + tap % 9;
            for (int q = sl; q < kTile * kPos; q += kSlices) {
                const int m = q / kPos, pos = q - m * kPos, y = pos / 13, x = pos - y * 13;
                const float v = s_norm[s_obs[m * kObs + (y * 15 + x) * 3 + off]];
                const float *dc = s_conv + m * kPitch + pos * 6;
#pragma unroll
                for (int f = 0; f < 6; ++f) acc_cw[f] = fmaf(v, dc[f], acc_cw[f]);
                if (tap == 0) {                            // conv_b: tap 0's nine threads, the same slices
#pragma unroll
                    for (int f = 0; f < 6; ++f) acc_cb[f] += dc[f];
                }
            }
        }
    }

    // ---- the workgroup's partial set and statistics ----
    float *part = a.scratch + ((size_t)p * a.G + g) * (size_t)(a.set_floats + kStatFloats);
    const auto put = [=](int at, float v) {            // kFromDx: onto the sums so far, carried in scratch from window to window
        if constexpr (kFromDx) part[at + shift] = a.accumulate ? part[at + shift] + v : v;
        else part[at] = v;
    };
    __syncthreads();
    float *s_red = s_conv;                             // [27][kSlices][6] conv_w slices, then [kSlices][6] conv_b slices
    if (tid < 27 * kSlices) {
#pragma unroll
        for (int f = 0; f < 6; ++f) s_red[tid * 6 + f] = acc_cw[f];
        if (tid < kSlices) {
#pragma unroll
            for (int f = 0; f < 6; ++f) s_red[27 * kSlices * 6 + tid * 6 + f] = acc_cb[f];
        }
    }
    if (tid < kTile) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s_stat[tid * 5 + k] = st[k];
    }
    __syncthreads();
    if (tid < 168) {                                   // conv_w [27][6], then conv_b [6]: the slices in order
        const float *src = tid < 162 ? s_red + (tid / 6) * kSlices * 6 + tid % 6 : s_red + 27 * kSlices * 6 + (tid - 162);
        float sum = 0.f;
#pragma unroll
        for (int sl = 0; sl < kSlices; ++sl) sum += src[sl * 6];
        if constexpr (kTanh) part[SSD_POL_CONV_W + tid] = a.accumulate || a.stack ? part[SSD_POL_CONV_W + tid] + sum : sum;
        else put(SSD_POL_CONV_W + tid, sum);
    }
    if (!kFromDx && tid < 5) {
        double sum = 0.0;
        for (int m = 0; m < kTile; ++m) sum += s_stat[m * 5 + tid];
        reinterpret_cast<double *>(part + a.set_floats)[tid] = sum;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 256 * wave + 16 * t + 4 * l4 + r;
                if (row < kFlat) put(SSD_POL_FC1_W + row * 32 + 16 * c + l15, acc_w1[t][c][r]);
            }
        }
    }
    if (tid < 32) {
        put(SSD_POL_FC1_B + tid, acc_b1);
        put(SSD_POL_FC2_B + tid, acc_b2);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) put(SSD_POL_FC2_W + tid + u * kThreads, acc_w2[u]);
    if constexpr (kFromDx) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int q = tid + u * kThreads, k = q >> 4, j = q & 15;
        if (j < A) part[SSD_POL_LOGITS_W + k * A + j] = acc_hd[u];
        else if (j == A) part[SSD_POL_VALUE_W + k] = acc_hd[u];
    }
    if (tid < A) part[SSD_POL_LOGITS_W + 32 * A + tid] = acc_bh;
    else if (tid == A) part[SSD_POL_VALUE_B] = acc_bh;
}

// The G partials of a set added in order g = 0 .. G - 1 in float64, times 1 / rows, rounded once; the padding floats are zero.
// kLossAc: the sums as they are (the A3C loss is a sum over rows), and the four statistics of a3c_row to stats [P][4].
template <int kLoss>
__global__ void __launch_bounds__(256) ssd_ppo_reduce_kernel(GradArgs a) {
    constexpr bool kSum = kLoss == ssd::kLossAc;
    constexpr int kStats = kSum ? 4 : 5;
    const int idx = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y, S = a.set_floats;
    const size_t pitch = (size_t)S + kStatFloats;
    const float *part = a.scratch + (size_t)p * a.G * pitch;
    if (idx < S) {
        const bool pad = (idx > SSD_POL_VALUE_B && idx < SSD_POL_LOGITS_W) || idx >= SSD_POL_LOGITS_W + 33 * a.A;
        double sum = 0.0;
        if (!pad)
            for (int g = 0; g < a.G; ++g) sum += (double)part[g * pitch + idx];
        a.grads[(size_t)p * S + idx] = kSum ? (float)sum : (float)(sum / (double)a.set_rows);
    }
    if (blockIdx.x == 0 && threadIdx.x < kStats) {
        double sum = 0.0;
        for (int g = 0; g < a.G; ++g) sum += reinterpret_cast<const double *>(part + g * pitch + S)[threadIdx.x];
        a.stats[p * kStats + threadIdx.x] = kSum ? sum : sum / (double)a.set_rows;
    }
}

}  // namespace

namespace ssd {

hipError_t launch_ppo_trunk_grad(const PpoGradArgs &a, void *stream) {
    hipLaunchKernelGGL(ssd_ppo_grad_kernel<kModeFromDx>, dim3((unsigned)a.G, (unsigned)a.P), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

hipError_t launch_ppo_moa_stack_grad(const PpoGradArgs &a, void *stream) {
    hipLaunchKernelGGL(ssd_ppo_grad_kernel<kModeMoaStack>, dim3((unsigned)a.G, (unsigned)a.P), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

}  // namespace ssd

namespace {

// Both entry points below: the checks and the two launches, with the row loss `loss` (the A3C call passes no logp_old, vf_preds
// or behaviour_logits and zeros for the hyper-parameters it does not have, which pass their checks).
int conv_fc_grad(int loss, const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs_first, const uint8_t *obs,
                 const int32_t *actions, const float *logp_old, const float *advantages, const float *value_targets,
                 const float *vf_preds, const float *behaviour_logits, int32_t n_steps, int32_t num_envs, int32_t num_agents,
                 double clip_param, double vf_clip_param, double vf_loss_coeff, double entropy_coeff, double kl_coeff,
                 float *scratch, float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream) {
    const bool ac = loss == ssd::kLossAc;
    const ssd::GradCall call{ssd::kNetConvFc, ac, weights, num_sets, num_actions, 0, 0, obs_first, obs, nullptr, nullptr, actions, logp_old,
                             advantages, value_targets, vf_preds, behaviour_logits, n_steps, num_envs, num_agents, clip_param,
                             vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, 0.0, scratch, grads, stats, flags};
    if (const char *why = ssd::check_policy_grad(call)) return ssd::policy_fail(why);
    const int64_t rows = (int64_t)n_steps * num_envs * num_agents;
    if (const int rc = ssd::policy_use_device(device_id)) return rc;
    GradArgs a{};
    a.w = weights; a.P = num_sets; a.A = num_actions; a.N = num_agents; a.set_floats = SSD_POL_SET_FLOATS(num_actions);
    a.set_rows = (int32_t)(rows / num_sets);
    a.G = SSD_PPO_GROUPS(a.set_rows, num_sets);
    a.step_rows = num_envs * num_agents;
    a.obs_first = obs_first; a.obs = obs; a.actions = actions; a.logp_old = logp_old; a.adv = advantages; a.vt = value_targets;
    a.vf_pred = vf_preds; a.beh = behaviour_logits;
    a.clip = (float)clip_param; a.vf_clip = (float)vf_clip_param; a.vf_coeff = (float)vf_loss_coeff;
    a.ent_coeff = (float)entropy_coeff; a.kl_coeff = (float)kl_coeff;
    a.scratch = scratch; a.grads = grads; a.stats = stats;
    const dim3 grid((unsigned)a.G, (unsigned)a.P), reduce_grid((unsigned)((a.set_floats + 255) / 256), (unsigned)a.P);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ac) hipLaunchKernelGGL((ssd_ppo_grad_kernel<kModeLoss, ssd::kLossAc>), grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((ssd_ppo_grad_kernel<kModeLoss, ssd::kLossPpo>), grid, dim3(kThreads), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);
    if (ac) hipLaunchKernelGGL(ssd_ppo_reduce_kernel<ssd::kLossAc>, reduce_grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ssd_ppo_reduce_kernel<ssd::kLossPpo>, reduce_grid, dim3(256), 0, s, a);
    return ssd::policy_launched(hipGetLastError());
}

}  // namespace

extern "C" int ssd_policy_ppo_grad(const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs_first,
                                   const uint8_t *obs, const int32_t *actions, const float *logp_old, const float *advantages,
                                   const float *value_targets, const float *vf_preds, const float *behaviour_logits, int32_t n_steps,
                                   int32_t num_envs, int32_t num_agents, double clip_param, double vf_clip_param,
                                   double vf_loss_coeff, double entropy_coeff, double kl_coeff, float *scratch, float *grads,
                                   double *stats, int32_t device_id, uint32_t flags, void *stream) {
    return conv_fc_grad(ssd::kLossPpo, weights, num_sets, num_actions, obs_first, obs, actions, logp_old, advantages, value_targets,
                        vf_preds, behaviour_logits, n_steps, num_envs, num_agents, clip_param, vf_clip_param, vf_loss_coeff,
                        entropy_coeff, kl_coeff, scratch, grads, stats, device_id, flags, stream);
}

extern "C" int ssd_policy_ac_grad(const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs_first,
                                  const uint8_t *obs, const int32_t *actions, const float *advantages, const float *value_targets,
                                  int32_t n_steps, int32_t num_envs, int32_t num_agents, double vf_loss_coeff, double entropy_coeff,
                                  float *scratch, float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream) {
    return conv_fc_grad(ssd::kLossAc, weights, num_sets, num_actions, obs_first, obs, actions, nullptr, advantages, value_targets,
                        nullptr, nullptr, n_steps, num_envs, num_agents, 0.0, 0.0, vf_loss_coeff, entropy_coeff, 0.0, scratch,
                        grads, stats, device_id, flags, stream);
}
