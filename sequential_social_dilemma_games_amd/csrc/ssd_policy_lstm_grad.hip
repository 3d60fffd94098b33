// ssd_policy_lstm_grad.hip -- RLlib's PPO loss of the recurrent policy (the conv-FC trunk under RLlib's LSTM) on a sampled
// fragment with truncated backpropagation through time, its statistics and the gradient of every parameter:
// ssd_policy_lstm_ppo_grad.  include/ssd.h states the contract (the state rule, the rows, the order of the sums); DESIGN.md
// section 17 the shape, the resource report and the measurements.
//
// The fragment is walked window by window (seq_len steps, the last one possibly shorter) by a host loop that only enqueues.
// Per window, on the caller's scratch:
//   1. features: the trunk kernel's features mode (ssd_policy.hip) over the window's rows -> feat [rows][32];
//   2. ssd_lstm_seq_kernel: a workgroup of 4 C threads takes 16 sequences of one weight set (persistent over tiles g, g + G,
//      ...).  Forward over the window's steps from the shared pieces (lstm_gates, cell_update, head): h' stays in LDS, the gate
//      activations, c' and h' of every row go to scratch, the loss terms of a row (ppo_row, as ssd_policy_grad.hip) to float64
//      sums and d row_loss / d (logits, value) to the row's dx slot.  Then backward over the steps in reverse: the heads'
//      kernels and biases summed in registers (fixed entries per thread), dh' = heads^T d + the dh carried from step t + 1,
//      the gate derivatives dz (16 x 4C) to LDS and over the activations in scratch, d [x, h_prev] = dz lstm_w^T on the
//      matrix cores (B from a transposed copy of lstm_w made once per call): dx to scratch, dh_prev and dc_prev stay in the
//      registers of the lane that owns the (row, cell) pair, and are zeroed where the step's state was selected zero;
//   3. ssd_lstm_dw_kernel: d lstm_w = [x, h_prev]^T dz on the matrix cores, split over a fixed partition of the set's rows
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
#include "ssd_policy_device.hpp"

namespace {

constexpr int kX = SSD_LSTM_X;          // trunk features per row
constexpr int kSeqTile = SSD_RPPO_TILE;
constexpr int kChunk = SSD_RPPO_CHUNK;
constexpr int kStatFloats = SSD_PPO_STAT_FLOATS;

using ssd::f32x4;
using Cell = ssd::RllibCell;

static_assert(kSeqTile == 16 && kChunk == 64, "the tiles of the kernels below");

struct WinArgs {
    const float *w;                // P weight sets
    const float *wT;               // [P][4C][32 + C]: lstm_w transposed
    int32_t P, A, N, C, set_floats;
    int32_t G;                     // sequence kernel: workgroups per set
    int32_t S;                     // lstm_w kernel: splits per set
    int32_t seqs;                  // sequences of one set: E (P = N) or E N (P = 1)
    int32_t step_rows;             // E * N
    int32_t steps;                 // the window's steps
    int32_t accumulate;            // add to the partial sums scratch holds (every window but the first)
    const float *ring;             // [E][N][2][C]: the state the window's first step uses
    const uint8_t *done_prev;      // done[k0 - 1 + t] is the flag step t > 0 of the window looks at: u8 [.][E][N], or null
    const int32_t *actions;        // the per-row arrays at the window's first step
    const float *logp_old, *adv, *vt, *vf_pred, *beh;
    ssd::PpoHyper h;
    float *feat;                   // [steps][E][N][32]
    float *dx;                     // [steps][E][N][32]: d row_loss / d (logits, value) in 0..15, then d loss / d x
    float *st;                     // [steps][E][N][2][C]: (c', h') of every row
    float *gz;                     // [steps][E][N][4C]: the gate activations (i, tanh j, f, o), then dz
    float *part_seq;               // [P][G][16 C + 16 + kStatFloats]
    float *part_w;                 // [P][S][(32 + C) 4C + 4C]
};

__device__ __forceinline__ int seq_part_floats(int C) { return 16 * C + 16 + kStatFloats; }

// ------------------------------------------------------------------------------------------------- the transposed lstm_w
__global__ void __launch_bounds__(256) ssd_lstm_transpose_kernel(const float *w, int set_floats, int C, float *wT) {
    const int K = kX + C, n4 = 4 * C, p = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * n4) return;
    const int k = idx / K, n = idx - k * K;                    // wT[k][n] = lstm_w[n][k]
    wT[(size_t)p * K * n4 + idx] = w[(size_t)p * set_floats + SSD_LSTM_W + (size_t)n * n4 + k];
}

// ------------------------------------------------------------------------------------------------- the sequence kernel
// kLoss: the row loss, ssd::kLossPpo (ppo_row) or ssd::kLossAc (a3c_row: the A3C terms, four statistics).
template <int C, int kLoss = ssd::kLossPpo>
__global__ void __launch_bounds__(4 * C) ssd_lstm_seq_kernel(WinArgs a) {
    constexpr int kThreads = 4 * C;
    constexpr int kK = kX + C;          // rows of lstm_w
    constexpr int kPitch = kK + 36;     // LDS pitch of [x, h], = 4 (mod 64)
    constexpr int kZP = 4 * C + 4;      // LDS pitch of dz, = 4 (mod 64)
    __shared__ float s_in[kSeqTile * kPitch];   // rows [x (32), h (C)]; h' after the gates
    __shared__ float s_dz[kSeqTile * kZP];
    __shared__ float s_out[kSeqTile * 16];      // forward: logits 0..A-1 and the value at A; backward: their derivatives
    __shared__ int s_start[kSeqTile];           // the step's state is selected zero (or the row is past the set)
    __shared__ double s_stat[kSeqTile * 5];

    const int tid = threadIdx.x, g = blockIdx.x, p = blockIdx.y;
    const int A = a.A, Q = a.seqs, SR = a.step_rows;
    const int stride = a.P == 1 ? 1 : a.N;      // sequence s of set p is row s * stride + p of a step's [E][N] rows
    const float *__restrict__ w = a.w + (size_t)p * (size_t)a.set_floats;
    const float *__restrict__ wT = a.wT + (size_t)p * kK * 4 * C;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * wave + l15;

    float acc_hd[4] = {0.f, 0.f, 0.f, 0.f};     // heads' kernels: entry q = tid + 4C v is (k, j) = (q >> 4, q & 15); j == A: the value
    float acc_bh = 0.f;                         // tid < 16: the heads' biases
    double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // tid < 16: total, policy, vf, kl, entropy of tile row tid

    const int tiles = Q / kSeqTile + (Q % kSeqTile != 0);
    for (int tile = g; tile < tiles; tile += a.G) {
        const int s0 = tile * kSeqTile;
        const auto srow = [=](int m) { return (size_t)(s0 + m) * stride + p; };
        const auto row = [=](int m) { return ssd::StateRow{s0 + m < Q, srow(m) * 2 * C}; };

        // ---- forward over the window ----
        for (int t = 0; t < a.steps; ++t) {
            __syncthreads();
            if (tid < kSeqTile) {
                const bool live = s0 + tid < Q;
                s_start[tid] = !live || (t > 0 && a.done_prev && a.done_prev[(size_t)(t - 1) * SR + srow(tid)] != 0);
            }
            for (int q = tid; q < kSeqTile * kX; q += kThreads) {
                const int m = q / kX, k = q - m * kX;
                s_in[m * kPitch + k] = s0 + m < Q ? a.feat[((size_t)t * SR + srow(m)) * kX + k] : 0.f;
            }
            __syncthreads();
            for (int q = tid; q < kSeqTile * C; q += kThreads) {     // h: the ring's at t = 0, zero where selected, else h' as it is
                const int m = q / C, k = q - m * C;
                if (t == 0) s_in[m * kPitch + kX + k] = s0 + m < Q ? a.ring[srow(m) * 2 * C + Cell::kRowH * C + k] : 0.f;
                else if (s_start[m]) s_in[m * kPitch + kX + k] = 0.f;
            }
            __syncthreads();
            f32x4 acc[4][1];
            ssd::lstm_gates<C, kK, kPitch, 1>(s_in, w + SSD_LSTM_W, tid, acc);
            __syncthreads();                                         // every wave is done with the h rows of s_in
            const float *state_in = t == 0 ? a.ring : a.st + (size_t)(t - 1) * SR * 2 * C;
            float *state_out = a.st + (size_t)t * SR * 2 * C;
            ssd::cell_update<Cell, C, 1>(acc, w + SSD_LSTM_B(C), s_start, state_in, state_out, s_in + kX, kPitch, tid, row);
            {   // the gate activations of the (row, cell) pairs this lane owns, as Cell::update forms them
                const float *bias = w + SSD_LSTM_B(C);
                const float b0 = bias[u], b1 = bias[C + u], b2 = bias[2 * C + u], b3 = bias[3 * C + u];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 4 * l4 + r;
                    if (s0 + m >= Q) continue;
                    float *gz = a.gz + ((size_t)t * SR + srow(m)) * 4 * C + u;
                    gz[0] = ssd::sigmoidf_(acc[0][0][r] + b0);
                    gz[C] = tanhf(acc[1][0][r] + b1);
                    gz[2 * C] = ssd::sigmoidf_((acc[2][0][r] + b2) + 1.f);
                    gz[3 * C] = ssd::sigmoidf_(acc[3][0][r] + b3);
                }
            }
            __syncthreads();
            if (tid < kSeqTile * 16) {
                const int m = tid >> 4, j = tid & 15;
                if (j <= A)
                    s_out[tid] = ssd::head<C>(s_in + kX + m * kPitch, w + SSD_LSTM_LOGITS_W(C), w + SSD_LSTM_VALUE_W(C),
                                              w + SSD_LSTM_LOGITS_B(C, A), w + SSD_LSTM_VALUE_B(C), A, j);
            }
            __syncthreads();
            if (tid < kSeqTile && s0 + tid < Q) {                    // the loss terms of the row and their derivatives
                const size_t r = (size_t)t * SR + srow(tid);
                int act = a.actions[r];
                act = act < 0 ? 0 : (act >= A ? A - 1 : act);
                float d[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] = 0.f;
                if constexpr (kLoss == ssd::kLossAc)
                    ssd::a3c_row(s_out + tid * 16, d, A, act, a.adv[r], a.vt[r], a.h, st);
                else
                    ssd::ppo_row(s_out + tid * 16, d, A, act, a.adv[r], a.vt[r], a.vf_pred[r], a.logp_old[r],
                                 a.beh ? a.beh + r * A : nullptr, a.h, st);
#pragma unroll
                for (int j = 0; j < 16; ++j) a.dx[r * kX + j] = d[j];
            }
        }

        // ---- backward over the window ----
        float dh_c[4] = {0.f, 0.f, 0.f, 0.f}, dc_c[4] = {0.f, 0.f, 0.f, 0.f};    // carried to step t - 1: rows 4 l4 + r, cell u
        for (int t = a.steps - 1; t >= 0; --t) {
            __syncthreads();
            if (tid < kSeqTile) {
                const bool live = s0 + tid < Q;
                s_start[tid] = !live || (t > 0 && a.done_prev && a.done_prev[(size_t)(t - 1) * SR + srow(tid)] != 0);
            }
            if (tid < kSeqTile * 16) {
                const int m = tid >> 4, j = tid & 15;
                s_out[tid] = s0 + m < Q ? a.dx[((size_t)t * SR + srow(m)) * kX + j] : 0.f;
            }
            for (int q = tid; q < kSeqTile * C; q += kThreads) {     // h' of the step
                const int m = q / C, k = q - m * C;
                s_in[m * kPitch + kX + k] = s0 + m < Q ? a.st[((size_t)t * SR + srow(m)) * 2 * C + Cell::kRowH * C + k] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 4; ++v) {                            // the heads' kernels
                const int q = tid + v * kThreads, k = q >> 4, j = q & 15;
                float sum = 0.f;
#pragma unroll 4
                for (int m = 0; m < kSeqTile; ++m) sum = fmaf(s_in[m * kPitch + kX + k], s_out[m * 16 + j], sum);
                acc_hd[v] += sum;
            }
            if (tid < 16) {
                float sum = 0.f;
#pragma unroll
                for (int m = 0; m < kSeqTile; ++m) sum += s_out[m * 16 + tid];
                acc_bh += sum;
            }
            // the cell: dh' -> d gates -> dz for the (row, cell) pairs this lane owns
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 4 * l4 + r;
                float dz0 = 0.f, dz1 = 0.f, dz2 = 0.f, dz3 = 0.f;
                if (s0 + m < Q) {
                    const size_t rw = (size_t)t * SR + srow(m);
                    float dh = 0.f;
                    for (int j = 0; j < A; ++j) dh = fmaf(s_out[m * 16 + j], w[SSD_LSTM_LOGITS_W(C) + u * A + j], dh);
                    dh = fmaf(s_out[m * 16 + A], w[SSD_LSTM_VALUE_W(C) + u], dh);
                    dh += dh_c[r];
                    float *gz = a.gz + rw * 4 * C + u;
                    const float gi = gz[0], gj = gz[C], gf = gz[2 * C], go = gz[3 * C];
                    const float c2 = a.st[rw * 2 * C + Cell::kRowC * C + u];
                    float c_prev;
                    if (t == 0) c_prev = a.ring[srow(m) * 2 * C + Cell::kRowC * C + u];
                    else c_prev = s_start[m] ? 0.f : a.st[(rw - SR) * 2 * C + Cell::kRowC * C + u];
                    const float tc = tanhf(c2);
                    const float dc = dh * go * (1.f - tc * tc) + dc_c[r];
                    dz0 = dc * gj * (gi * (1.f - gi));
                    dz1 = dc * gi * (1.f - gj * gj);
                    dz2 = dc * c_prev * (gf * (1.f - gf));
                    dz3 = dh * tc * (go * (1.f - go));
                    dc_c[r] = s_start[m] ? 0.f : dc * gf;
                    gz[0] = dz0; gz[C] = dz1; gz[2 * C] = dz2; gz[3 * C] = dz3;
                }
                float *z = s_dz + m * kZP + u;
                z[0] = dz0; z[C] = dz1; z[2 * C] = dz2; z[3 * C] = dz3;
            }
            __syncthreads();
            // d [x, h_prev] = dz lstm_w^T: A[m][k] = dz[m][k], B[k][n] = wT[k][n].  Wave w takes the h columns 16 w .. 16 w + 15
            // (lane (l15, l4) gets dh_prev of cell u for rows 4 l4 + r: the pairs it owns); waves 0 and 1 also the x columns.
            {
                const float *a_row = s_dz + l15 * kZP + l4;
                const float *bh = wT + (size_t)l4 * kK + kX + 16 * wave + l15;
                f32x4 acc_h = {0.f, 0.f, 0.f, 0.f}, acc_x = {0.f, 0.f, 0.f, 0.f};
                if (wave < 2) {
                    const float *bx = wT + (size_t)l4 * kK + 16 * wave + l15;
#pragma unroll 4
                    for (int kk = 0; kk < C; ++kk) {
                        const float av = a_row[4 * kk];
                        acc_h = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bh[(size_t)kk * 4 * kK], acc_h, 0, 0, 0);
                        acc_x = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bx[(size_t)kk * 4 * kK], acc_x, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = 4 * l4 + r;
                        if (s0 + m < Q) a.dx[((size_t)t * SR + srow(m)) * kX + 16 * wave + l15] = acc_x[r];
                    }
                } else {
#pragma unroll 4
                    for (int kk = 0; kk < C; ++kk)
                        acc_h = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], bh[(size_t)kk * 4 * kK], acc_h, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) dh_c[r] = s_start[4 * l4 + r] ? 0.f : acc_h[r];
            }
        }
    }

    // ---- the workgroup's partial sums and statistics ----
    float *part = a.part_seq + ((size_t)p * a.G + g) * (size_t)seq_part_floats(C);
    const bool add = a.accumulate != 0;
    __syncthreads();
    if (tid < kSeqTile) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s_stat[tid * 5 + k] = st[k];
    }
    __syncthreads();
    if (tid < 5) {
        double sum = 0.0;
        for (int m = 0; m < kSeqTile; ++m) sum += s_stat[m * 5 + tid];
        double *dst = reinterpret_cast<double *>(part + 16 * C + 16) + tid;
        *dst = add ? *dst + sum : sum;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int q = tid + v * kThreads;
        part[q] = add ? part[q] + acc_hd[v] : acc_hd[v];
    }
    if (tid < 16) part[16 * C + tid] = add ? part[16 * C + tid] + acc_bh : acc_bh;
}

// ------------------------------------------------------------------------------------- d lstm_w = [x, h_prev]^T dz, lstm_b
// Workgroup (column block, split s, set p): 64 columns of dz (16 a wave), all 32 + C rows of lstm_w (2 + C / 16 accumulator
// tiles a lane), the set's rows of the window in 64-row chunks s, s + S, ... in order.  A[c][k] = [x, h_prev][row k][c],
// B[k][n] = dz[row k][n].
template <int C>
__global__ void __launch_bounds__(256) ssd_lstm_dw_kernel(WinArgs a) {
    constexpr int kMT = 2 + C / 16;
    __shared__ float s_b[4 * 64];
    const int tid = threadIdx.x, s = blockIdx.y, p = blockIdx.z;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const int SR = a.step_rows, stride = a.P == 1 ? 1 : a.N;
    const int R = a.seqs * a.steps;                                  // the set's rows of the window
    f32x4 acc[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;                                                // dz[rows = l4 (mod 4)][n0 + l15]

    const int chunks = R / kChunk + (R % kChunk != 0);
    for (int chunk = s; chunk < chunks; chunk += a.S) {
        for (int kk = 0; kk < kChunk / 4; ++kk) {
            const int r = chunk * kChunk + 4 * kk + l4;
            const bool valid = r < R;
            const size_t rw = valid ? (size_t)r * stride + p : 0;    // row of the window's [steps][E][N] arrays
            const int t = (int)(rw / SR);
            const size_t sr = rw - (size_t)t * SR;
            const float *hp = nullptr;                               // h_prev of the row: the state rule of include/ssd.h
            if (valid) {
                if (t == 0) hp = a.ring + sr * 2 * C + Cell::kRowH * C;
                else if (!(a.done_prev && a.done_prev[(size_t)(t - 1) * SR + sr] != 0)) hp = a.st + (rw - SR) * 2 * C + Cell::kRowH * C;
            }
            const float b = valid ? a.gz[rw * 4 * C + n0 + l15] : 0.f;
            bsum += b;
            float av[kMT];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) av[mt] = valid ? a.feat[rw * kX + 16 * mt + l15] : 0.f;
#pragma unroll
            for (int mt = 2; mt < kMT; ++mt) av[mt] = hp ? hp[16 * (mt - 2) + l15] : 0.f;
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt], 0, 0, 0);
        }
    }

    float *part = a.part_w + ((size_t)p * a.S + s) * (size_t)((kX + C) * 4 * C + 4 * C);
    const bool add = a.accumulate != 0;
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float *dst = part + (size_t)(16 * mt + 4 * l4 + r) * 4 * C + n0 + l15;
            *dst = add ? *dst + acc[mt][r] : acc[mt][r];
        }
    }
    s_b[tid] = bsum;                                                 // [wave][l4][l15]
    __syncthreads();
    if (l4 == 0) {
        const float sum = ((s_b[wave * 64 + l15] + s_b[wave * 64 + 16 + l15]) + s_b[wave * 64 + 32 + l15]) + s_b[wave * 64 + 48 + l15];
        float *dst = part + (size_t)(kX + C) * 4 * C + n0 + l15;
        *dst = add ? *dst + sum : sum;
    }
}

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
hipError_t launch_window(int loss, const WinArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.G, (unsigned)a.P);
    if (loss == ssd::kLossAc) hipLaunchKernelGGL((ssd_lstm_seq_kernel<C, ssd::kLossAc>), grid, dim3(4 * C), 0, stream, a);
    else hipLaunchKernelGGL((ssd_lstm_seq_kernel<C, ssd::kLossPpo>), grid, dim3(4 * C), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd_lstm_dw_kernel<C>), dim3(4 * C / 64, (unsigned)a.S, (unsigned)a.P), dim3(256), 0, stream, a);
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
    using ssd::policy_fail;
    const bool ac = loss == ssd::kLossAc;
    if (!weights) return policy_fail("weights are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetLstm, weights, num_sets, num_agents, num_actions, cell_size)) return policy_fail(why);
    if (n_steps < 1 || num_envs < 1) return policy_fail("n_steps and num_envs must be >= 1");
    if (seq_len < 1) return policy_fail("seq_len must be >= 1");
    const int64_t rows = (int64_t)n_steps * num_envs * num_agents;
    if (rows > INT32_MAX - 16) return policy_fail("n_steps * num_envs * num_agents must be at most 2^31 - 17");
    if (!obs && !(obs_first && n_steps == 1)) return policy_fail("obs is required (it may be null only with obs_first and n_steps 1)");
    if (!state) return policy_fail("state is required");
    if (reinterpret_cast<uintptr_t>(state) & 3u) return policy_fail("state must be 4-byte aligned");
    if (ac && (!actions || !advantages || !value_targets)) return policy_fail("actions, advantages and value_targets are required");
    if (!ac && (!actions || !logp_old || !advantages || !value_targets || !vf_preds))
        return policy_fail("actions, logp_old, advantages, value_targets and vf_preds are required");
    if (!scratch || !grads || !stats) return policy_fail("scratch, grads and stats are required");
    if ((reinterpret_cast<uintptr_t>(scratch) & 7u) || (reinterpret_cast<uintptr_t>(stats) & 7u))
        return policy_fail("scratch and stats must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(grads) & 3u) return policy_fail("grads must be 4-byte aligned");
    if (!(isfinite(clip_param) && isfinite(vf_clip_param) && isfinite(vf_loss_coeff) && isfinite(entropy_coeff) && isfinite(kl_coeff)))
        return policy_fail("the hyper-parameters must be finite");
    if (clip_param < 0.0 || vf_clip_param < 0.0) return policy_fail("clip_param and vf_clip_param must be >= 0");
    if ((kl_coeff != 0.0) != (behaviour_logits != nullptr))
        return policy_fail("behaviour_logits must be given if and only if kl_coeff is not 0");
    if (flags) return policy_fail("flags must be 0");
    if (const int rc = ssd::policy_use_device(device_id)) return rc;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int K = n_steps, E = num_envs, N = num_agents, P = num_sets, A = num_actions, C = cell_size, T = seq_len;
    const int W = T < K ? T : K;                                     // steps of a whole window
    const size_t SR = (size_t)E * N, win_rows = (size_t)W * SR;
    const int seqs = (int)(SR / P);
    // the scratch: the blocks of SSD_RPPO_SCRATCH_FLOATS, in its order
    WinArgs a{};
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

    hipLaunchKernelGGL(ssd_lstm_transpose_kernel, dim3((unsigned)(((kX + C) * 4 * C + 255) / 256), (unsigned)P), dim3(256), 0, stream,
                       weights, a.set_floats, C, wT);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);

    const size_t obs_step = SR * 675;
    for (int k0 = 0; k0 < K; k0 += T) {
        const int steps = K - k0 < T ? K - k0 : T;
        // the observations the window's rows acted on (the shift of include/ssd.h): `first` for its step 0, `rest` from step 1
        const uint8_t *first = nullptr, *rest = nullptr;
        if (!obs_first) rest = obs + (size_t)k0 * obs_step;          // row k reads obs[k]: `rest` from step 0
        else if (k0 == 0) { first = obs_first; rest = obs; }
        else { first = obs + (size_t)(k0 - 1) * obs_step; rest = obs + (size_t)k0 * obs_step; }
        // 1. the features
        ssd::PolicyArgs f{};
        f.w = weights; f.P = P; f.A = A; f.N = N; f.set_floats = a.set_floats;
        hipError_t e = hipSuccess;
        if (first) {
            f.B = E; f.obs = first; f.feat = a.feat;
            e = ssd::launch_policy_features(f, stream);
            if (e == hipSuccess && steps > 1) {
                f.B = (steps - 1) * E; f.obs = rest; f.feat = a.feat + SR * kX;
                e = ssd::launch_policy_features(f, stream);
            }
        } else {
            f.B = steps * E; f.obs = rest; f.feat = a.feat;
            e = ssd::launch_policy_features(f, stream);
        }
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
        ssd::PpoGradArgs tg{};
        tg.w = weights; tg.P = P; tg.A = A; tg.N = N; tg.set_floats = SSD_LSTM_W; tg.w_pitch = a.set_floats; tg.G = Gt;
        tg.set_rows = steps * seqs; tg.step_rows = (int32_t)SR;
        tg.obs_first = first; tg.obs = rest; tg.scratch = part_trunk; tg.dx = a.dx; tg.accumulate = a.accumulate;
        e = ssd::launch_ppo_trunk_grad(tg, stream);
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
