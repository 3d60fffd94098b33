// ssd_policy_moa_grad.hip -- the causal-influence policy's loss, PPOLoss + moa_weight * MOALoss (algorithms/ppo_causal.py:36-75,
// common_funcs.py:70-115), on a sampled fragment with truncated backpropagation through time through both Keras LSTMs, its
// statistics and the gradient of every ConvMOAPolicy parameter: ssd_policy_moa_ppo_grad.  include/ssd.h states the contract (the
// loss, the state rule, the previous actions, the order of the sums); DESIGN.md section 18 the shape, the resource report and
// the measurements.
//
// The fragment is walked window by window by a host loop that only enqueues, as ssd_policy_lstm_grad.hip walks it.  Per window,
// on the caller's scratch:
//   1. features: the trunk kernel's MOA mode (ssd_policy.hip) over the window's rows -> feat [rows][2][32], both stacks;
//   2. the actions branch: ssd_moa_seq_kernel<C, false> on stack 0 (KerasCell; forward, the PPO terms of a row through ppo_row,
//      backward with the heads' sums in registers, dx of stack 0 to scratch), then ssd_moa_dw_kernel<C, false> for the LSTM
//      matrix and bias;
//   3. the MOA branch, on the same (state, gates / dz) scratch: ssd_moa_seq_kernel<C, true> on [stack 1, the N previous actions
//      in slot order, zeros to 48].  Its head is the prediction h2' pred_w (16 x C . C x (N-1) A) on the matrix cores; a thread
//      per (row, other agent) forms the log-softmax, the cross-entropy (float64 sum) and dpred = moa_weight / (N-1) (softmax -
//      onehot), which goes to scratch; the backward reads it back, dh2' = dpred pred_w^T on the matrix cores, then the cell's
//      backward as in the actions branch.  ssd_moa_dw_kernel<C, true> forms the 48 + C rows of the MOA matrix (rows 32 .. 32 + N
//      - 1 from the action inputs, by the same product) and ssd_moa_dpred_kernel pred_w = h2'^T dpred and pred_b, both over
//      the fixed partition of the set's rows lstm_w's kernel uses;
//   4. the trunk's backward from dx, once per stack (ssd_policy_grad.hip's kernel with tanh derivatives); stack 1's launch adds
//      its conv sums to stack 0's.
// Every kernel adds its partial sums to what scratch holds from the windows before (the first window stores).  At the end
// ssd_moa_reduce_kernel adds the partials of every entry in order in float64, scales by 1 / set rows and rounds once.  No
// atomics anywhere: the same inputs give the same bits.
//
// The sequence and split kernels restate ssd_policy_lstm_grad.hip's for the Keras cell (gate order i, f, c~, o, no forget
// bias, state order (h, c) inside a four-row state), an input of 32 or 48 columns and either head; that file's kernels are
// left as they are, so the recurrent policy's call keeps its code and its bits.
//
// ssd_policy_moa_ac_grad is the same walk with the A3C row loss (include/ssd.h, A3C LOSS AND GRADIENTS):
// the actions branch's sequence kernel and the reduce compiled once more with ssd::kLossAc.  The A3C terms are sums over a set's
// rows and MOALoss a mean, so the MOA branch's scale on dpred carries 1 / rows too; its kernels are the PPO call's as they are.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"

namespace {

constexpr int kX = SSD_MOA_X;            // a stack's features per row
constexpr int kXM = SSD_MOA_XM;          // input rows of the MOA cell
constexpr int kSeqTile = SSD_MPPO_TILE;
constexpr int kChunk = SSD_MPPO_CHUNK;
constexpr int kStatFloats = SSD_PPO_STAT_FLOATS;
constexpr int kPP = 228;                 // LDS pitch of the prediction tile: (N - 1) A <= 225 up to whole k-steps of 4; 36 (mod 64)

using ssd::f32x4;
using Cell = ssd::KerasCell;

static_assert(kSeqTile == 16 && kChunk == 64, "the tiles of the kernels below");
static_assert((SSD_MOA_MAX_AGENTS - 1) * SSD_POL_MAX_ACTIONS <= kPP && kPP % 4 == 0, "prediction tile");
static_assert(Cell::kRowH == 0 && Cell::kRowC == 1, "a branch's two rows of a state are (h, c)");

struct WinArgs {
    const float *w;                // P weight sets
    const float *wT;               // [P][4C][in + C]: the branch's LSTM matrix transposed
    int32_t P, A, N, C, set_floats;
    int32_t G;                     // sequence kernel: workgroups per set
    int32_t S;                     // split kernels: splits per set
    int32_t seqs;                  // sequences of one set: E (P = N) or E N (P = 1)
    int32_t step_rows;             // E * N
    int32_t steps;                 // the window's steps
    int32_t accumulate;            // add to the partial sums scratch holds (every window but the first)
    int32_t pred_pitch;            // SSD_MPPO_PRED_PITCH(A, N)
    const float *ring;             // [E][N][4][C]: the state the window's first step uses
    const uint8_t *done_prev;      // done[k0 - 1 + t] is the flag step t > 0 of the window looks at: u8 [.][E][N], or null
    const int32_t *actions;        // the per-row arrays at the window's first step
    const int32_t *prev;           // [steps][E][N]: the joint action each step's MOA read, by agent index
    const float *logp_old, *adv, *vt, *vf_pred, *beh;
    ssd::PpoHyper h;
    float moa_scale;               // moa_weight / (N - 1); the A3C call: moa_weight / ((N - 1) set rows), MOALoss being a mean
    float *feat;                   // [steps][E][N][2][32]
    float *dx;                     // [steps][E][N][2][32]: stack 0's half holds d row_loss / d (logits, value) in 0..15 first
    float *st;                     // [steps][E][N][2][C]: (h', c') of every row, of the branch in hand
    float *gz;                     // [steps][E][N][4C]: the gate activations (i, f, tanh c~, o), then dz
    float *dpred;                  // [steps][E][N][pred_pitch]: d loss / d pred, columns 0 .. (N-1) A - 1 of live rows written
    float *part_seq;               // [P][G][16 C + 16 + kStatFloats]
    float *part_w;                 // [P][S][(in + C) 4C + 4C], the branch's
    float *part_pred;              // [P][S][(C + 1) pred_pitch]
};

__device__ __forceinline__ int seq_part_floats(int C) { return 16 * C + 16 + kStatFloats; }

// ------------------------------------------------------------------------------------------- a transposed LSTM matrix
__global__ void __launch_bounds__(256) ssd_moa_transpose_kernel(const float *w, int set_floats, int at, int K, int n4, float *wT) {
    const int p = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * n4) return;
    const int k = idx / K, n = idx - k * K;                    // wT[k][n] = w[n][k]
    wT[(size_t)p * K * n4 + idx] = w[(size_t)p * set_floats + at + (size_t)n * n4 + k];
}

// ------------------------------------------------------------------------------------------------- the sequence kernel
// kMoa false: the actions LSTM on stack 0 with the PPO head; true: the MOA LSTM on [stack 1, previous actions] with the
// prediction head.  A workgroup of 4 C threads takes 16 sequences of one weight set (persistent over tiles g, g + G, ...).
// kLoss (the actions branch only): the row loss, ssd::kLossPpo (ppo_row) or ssd::kLossAc (a3c_row: the A3C terms, four statistics).
template <int C, bool kMoa, int kLoss = ssd::kLossPpo>
__global__ void __launch_bounds__(4 * C) ssd_moa_seq_kernel(WinArgs a) {
    static_assert(!kMoa || kLoss == ssd::kLossPpo, "the MOA branch has one instantiation: the loss kind reaches it through a.moa_scale");
    constexpr int kThreads = 4 * C;
    constexpr int kIn = kMoa ? kXM : kX;            // input columns
    constexpr int kK = kIn + C;                     // rows of the LSTM matrix
    constexpr int kPitch = kK + (kMoa ? 20 : 36);   // LDS pitch of [x, h], = 4 (mod 64)
    constexpr int kZP = 4 * C + 4;                  // LDS pitch of dz, = 4 (mod 64)
    constexpr int kSt = kMoa ? 2 : 0;               // the branch's first row of a four-row state
    constexpr int kFeat = kMoa ? kX : 0;            // the branch's half of a feat / dx row
    __shared__ float s_in[kSeqTile * kPitch];       // rows [x (kIn), h (C)]; h' after the gates
    __shared__ float s_dz[kSeqTile * kZP];
    __shared__ float s_out[kSeqTile * 16];          // actions: logits 0..A-1 and the value at A; backward: their derivatives
    __shared__ float s_pred[kMoa ? kSeqTile * kPP : 4];   // MOA: the predictions [m][j A + k]; backward: dpred
    __shared__ int s_start[kSeqTile];               // the step's state is selected zero (or the row is past the set)
    __shared__ int s_slot[256];                     // MOA: [agent][slot] -> agent (moa_slots)
    __shared__ double s_stat[256];

    const int tid = threadIdx.x, g = blockIdx.x, p = blockIdx.y;
    const int A = a.A, N = a.N, Q = a.seqs, SR = a.step_rows, NO = N - 1, NA = NO * A;
    const int stride = a.P == 1 ? 1 : N;            // sequence s of set p is row s * stride + p of a step's [E][N] rows
    const float *__restrict__ w = a.w + (size_t)p * (size_t)a.set_floats;
    const float *__restrict__ wT = a.wT + (size_t)p * kK * 4 * C;
    const float *__restrict__ w_lstm = w + (kMoa ? SSD_MOA_MW(C, A) : SSD_MOA_LSTM_W(C));
    const float *__restrict__ b_lstm = w + (kMoa ? SSD_MOA_MB(C, A) : SSD_MOA_LSTM_B(C));
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * wave + l15;

    float acc_hd[4] = {0.f, 0.f, 0.f, 0.f};     // actions: heads' kernels, entry q = tid + 4C v is (k, j) = (q >> 4, q & 15); j == A: the value
    float acc_bh = 0.f;                         // actions, tid < 16: the heads' biases
    double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // actions, tid < 16: total, policy, vf, kl, entropy of tile row tid
    double ce_sum = 0.0;                        // MOA, tid < 16 (N - 1): the cross-entropies of (tile row, other agent) = (tid / NO, tid % NO)

    if constexpr (kMoa) ssd::moa_slots(N, tid, s_slot);

    const int tiles = Q / kSeqTile + (Q % kSeqTile != 0);
    for (int tile = g; tile < tiles; tile += a.G) {
        const int s0 = tile * kSeqTile;
        const auto srow = [=](int m) { return (size_t)(s0 + m) * stride + p; };

        // ---- forward over the window ----
        for (int t = 0; t < a.steps; ++t) {
            __syncthreads();
            if (tid < kSeqTile) {
                const bool live = s0 + tid < Q;
                s_start[tid] = !live || (t > 0 && a.done_prev && a.done_prev[(size_t)(t - 1) * SR + srow(tid)] != 0);
            }
            for (int q = tid; q < kSeqTile * kX; q += kThreads) {
                const int m = q / kX, k = q - m * kX;
                s_in[m * kPitch + k] = s0 + m < Q ? a.feat[((size_t)t * SR + srow(m)) * 2 * kX + kFeat + k] : 0.f;
            }
            __syncthreads();
            if constexpr (kMoa) {                                    // the previous actions in slot order: zero where selected
                for (int q = tid; q < kSeqTile * (kXM - kX); q += kThreads) {
                    const int m = q >> 4, k = q & 15;
                    float v = 0.f;
                    if (k < N && !s_start[m]) {
                        const size_t rr = srow(m);
                        const int e = (int)(rr / N), i = (int)(rr - (size_t)e * N);
                        v = (float)a.prev[(size_t)t * SR + (size_t)e * N + s_slot[i * 16 + k]];
                    }
                    s_in[m * kPitch + kX + k] = v;
                }
            }
            for (int q = tid; q < kSeqTile * C; q += kThreads) {     // h: the ring's at t = 0, zero where selected, else h' as it is
                const int m = q / C, k = q - m * C;
                if (t == 0) s_in[m * kPitch + kIn + k] = s0 + m < Q ? a.ring[(srow(m) * 4 + kSt + Cell::kRowH) * C + k] : 0.f;
                else if (s_start[m]) s_in[m * kPitch + kIn + k] = 0.f;
            }
            __syncthreads();
            f32x4 acc[4][1];
            ssd::lstm_gates<C, kK, kPitch, 1>(s_in, w_lstm, tid, acc);
            __syncthreads();                                         // every wave is done with the h rows of s_in
            {   // the cell update of the (row, cell) pairs this lane owns; h' to LDS, (h', c') and the gate activations to scratch
                const float b0 = b_lstm[u], b1 = b_lstm[C + u], b2 = b_lstm[2 * C + u], b3 = b_lstm[3 * C + u];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 4 * l4 + r;
                    if (s0 + m >= Q) continue;
                    const size_t rw = (size_t)t * SR + srow(m);
                    float c;
                    if (t == 0) c = a.ring[(srow(m) * 4 + kSt + Cell::kRowC) * C + u];
                    else c = s_start[m] ? 0.f : a.st[((rw - SR) * 2 + Cell::kRowC) * C + u];
                    const float zi = acc[0][0][r] + b0, zf = acc[1][0][r] + b1, zc = acc[2][0][r] + b2, zo = acc[3][0][r] + b3;
                    float c2, h2;
                    Cell::update(zi, zf, zc, zo, c, &c2, &h2);
                    s_in[m * kPitch + kIn + u] = h2;
                    a.st[(rw * 2 + Cell::kRowH) * C + u] = h2;
                    a.st[(rw * 2 + Cell::kRowC) * C + u] = c2;
                    float *gz = a.gz + rw * 4 * C + u;
                    gz[0] = ssd::sigmoidf_(zi);
                    gz[C] = ssd::sigmoidf_(zf);
                    gz[2 * C] = tanhf(zc);
                    gz[3 * C] = ssd::sigmoidf_(zo);
                }
            }
            __syncthreads();
            if constexpr (!kMoa) {
                if (tid < kSeqTile * 16) {
                    const int m = tid >> 4, j = tid & 15;
                    if (j <= A)
                        s_out[tid] = ssd::head<C>(s_in + kIn + m * kPitch, w + SSD_MOA_LOGITS_W(C), w + SSD_MOA_VALUE_W(C),
                                                  w + SSD_MOA_LOGITS_B(C, A), w + SSD_MOA_VALUE_B(C), A, j);
                }
                __syncthreads();
                if (tid < kSeqTile && s0 + tid < Q) {                // the loss terms of the row and their derivatives
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
                    for (int j = 0; j < 16; ++j) a.dx[r * 2 * kX + j] = d[j];
                }
            } else {
                // the predictions h2' pred_w + pred_b: wave w takes the 16-column tiles w, w + C / 16, ...
                const int ptiles = (NA + 15) / 16;
                for (int pt = wave; pt < ptiles; pt += C / 16) {
                    const int col = 16 * pt + l15;
                    const float *pw = w + SSD_MOA_PRED_W(C, A) + col;
                    const float *a_row = s_in + l15 * kPitch + kIn + l4;
                    f32x4 pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                    for (int kk = 0; kk < C / 4; ++kk) {
                        const float bv = col < NA ? pw[(size_t)(4 * kk + l4) * NA] : 0.f;
                        pa = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], bv, pa, 0, 0, 0);
                    }
                    if (col < NA) {
                        const float pb = w[SSD_MOA_PRED_B(C, A, N) + col];
#pragma unroll
                        for (int r = 0; r < 4; ++r) s_pred[(4 * l4 + r) * kPP + col] = pa[r] + pb;
                    }
                }
                __syncthreads();
                if (tid < kSeqTile * NO) {                           // (row, other agent): the cross-entropy and dpred
                    const int m = tid / NO, j = tid - m * NO;
                    if (s0 + m < Q) {
                        const size_t rr = srow(m);
                        const int e = (int)(rr / N), i = (int)(rr - (size_t)e * N);
                        int tgt = a.actions[(size_t)t * SR + (size_t)e * N + s_slot[i * 16 + j + 1]];
                        tgt = tgt < 0 ? 0 : (tgt >= A ? A - 1 : tgt);
                        const float *pr = s_pred + m * kPP + j * A;
                        float mx = pr[0];
                        for (int k = 1; k < A; ++k) mx = fmaxf(mx, pr[k]);
                        float s = 0.f;
                        for (int k = 0; k < A; ++k) s += expf(pr[k] - mx);
                        const float lse = mx + logf(s);
                        ce_sum += (double)(lse - pr[tgt]);
                        float *dp = a.dpred + ((size_t)t * SR + rr) * a.pred_pitch + j * A;
                        for (int k = 0; k < A; ++k) dp[k] = a.moa_scale * (expf(pr[k] - lse) - (k == tgt ? 1.f : 0.f));
                    }
                }
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
            f32x4 acc_dh = {0.f, 0.f, 0.f, 0.f};                     // MOA: dh2' of rows 4 l4 + r, cell u, from the head
            if constexpr (!kMoa) {
                if (tid < kSeqTile * 16) {
                    const int m = tid >> 4, j = tid & 15;
                    s_out[tid] = s0 + m < Q ? a.dx[((size_t)t * SR + srow(m)) * 2 * kX + j] : 0.f;
                }
                for (int q = tid; q < kSeqTile * C; q += kThreads) { // h' of the step
                    const int m = q / C, k = q - m * C;
                    s_in[m * kPitch + kIn + k] = s0 + m < Q ? a.st[(((size_t)t * SR + srow(m)) * 2 + Cell::kRowH) * C + k] : 0.f;
                }
                __syncthreads();
#pragma unroll
                for (int v = 0; v < 4; ++v) {                        // the heads' kernels
                    const int q = tid + v * kThreads, k = q >> 4, j = q & 15;
                    float sum = 0.f;
#pragma unroll 4
                    for (int m = 0; m < kSeqTile; ++m) sum = fmaf(s_in[m * kPitch + kIn + k], s_out[m * 16 + j], sum);
                    acc_hd[v] += sum;
                }
                if (tid < 16) {
                    float sum = 0.f;
#pragma unroll
                    for (int m = 0; m < kSeqTile; ++m) sum += s_out[m * 16 + tid];
                    acc_bh += sum;
                }
            } else {
                for (int q = tid; q < kSeqTile * kPP; q += kThreads) {   // dpred of the step, zero beyond (N - 1) A and past the set
                    const int m = q / kPP, k = q - m * kPP;
                    s_pred[q] = s0 + m < Q && k < NA ? a.dpred[((size_t)t * SR + srow(m)) * a.pred_pitch + k] : 0.f;
                }
                __syncthreads();
                // dh2' = dpred pred_w^T: A[m][k] = dpred[m][k], B[k][n] = pred_w[cell 16 wave + n][k]
                const float *a_row = s_pred + l15 * kPP + l4;
                const float *pw = w + SSD_MOA_PRED_W(C, A) + (size_t)u * NA + l4;
                const int ksteps = (NA + 3) / 4;
                for (int kk = 0; kk < ksteps; ++kk) {
                    const float bv = 4 * kk + l4 < NA ? pw[4 * kk] : 0.f;
                    acc_dh = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], bv, acc_dh, 0, 0, 0);
                }
            }
            // the cell: dh' -> d gates -> dz for the (row, cell) pairs this lane owns
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 4 * l4 + r;
                float dz0 = 0.f, dz1 = 0.f, dz2 = 0.f, dz3 = 0.f;
                if (s0 + m < Q) {
                    const size_t rw = (size_t)t * SR + srow(m);
                    float dh = 0.f;
                    if constexpr (kMoa) {
                        dh = acc_dh[r];
                    } else {
                        for (int j = 0; j < A; ++j) dh = fmaf(s_out[m * 16 + j], w[SSD_MOA_LOGITS_W(C) + u * A + j], dh);
                        dh = fmaf(s_out[m * 16 + A], w[SSD_MOA_VALUE_W(C) + u], dh);
                    }
                    dh += dh_c[r];
                    float *gz = a.gz + rw * 4 * C + u;
                    const float gi = gz[0], gf = gz[C], gc = gz[2 * C], go = gz[3 * C];
                    const float c2 = a.st[(rw * 2 + Cell::kRowC) * C + u];
                    float c_prev;
                    if (t == 0) c_prev = a.ring[(srow(m) * 4 + kSt + Cell::kRowC) * C + u];
                    else c_prev = s_start[m] ? 0.f : a.st[((rw - SR) * 2 + Cell::kRowC) * C + u];
                    const float tc = tanhf(c2);
                    const float dc = dh * go * (1.f - tc * tc) + dc_c[r];
                    dz0 = dc * gc * (gi * (1.f - gi));
                    dz1 = dc * c_prev * (gf * (1.f - gf));
                    dz2 = dc * gi * (1.f - gc * gc);
                    dz3 = dh * tc * (go * (1.f - go));
                    dc_c[r] = s_start[m] ? 0.f : dc * gf;
                    gz[0] = dz0; gz[C] = dz1; gz[2 * C] = dz2; gz[3 * C] = dz3;
                }
                float *z = s_dz + m * kZP + u;
                z[0] = dz0; z[C] = dz1; z[2 * C] = dz2; z[3 * C] = dz3;
            }
            __syncthreads();
            // d [x, h_prev] = dz W^T: A[m][k] = dz[m][k], B[k][n] = wT[k][n].  Wave w takes the h columns 16 w .. 16 w + 15
            // (lane (l15, l4) gets dh_prev of cell u for rows 4 l4 + r: the pairs it owns); waves 0 and 1 also the 32 feature
            // columns (the action columns of the MOA input are data: nothing flows into them).
            {
                const float *a_row = s_dz + l15 * kZP + l4;
                const float *bh = wT + (size_t)l4 * kK + kIn + 16 * wave + l15;
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
                        if (s0 + m < Q) a.dx[((size_t)t * SR + srow(m)) * 2 * kX + kFeat + 16 * wave + l15] = acc_x[r];
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
    double *part_st = reinterpret_cast<double *>(part + 16 * C + 16);
    const bool add = a.accumulate != 0;
    __syncthreads();
    if constexpr (kMoa) {
        if (tid < 256) s_stat[tid] = tid < kSeqTile * NO ? ce_sum : 0.0;
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int q = 0; q < kSeqTile * NO; ++q) sum += s_stat[q];
            sum /= (double)NO;
            part_st[5] = add ? part_st[5] + sum : sum;
        }
    } else {
        if (tid < kSeqTile) {
#pragma unroll
            for (int k = 0; k < 5; ++k) s_stat[tid * 5 + k] = st[k];
        }
        __syncthreads();
        if (tid < 5) {
            double sum = 0.0;
            for (int m = 0; m < kSeqTile; ++m) sum += s_stat[m * 5 + tid];
            part_st[tid] = add ? part_st[tid] + sum : sum;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int q = tid + v * kThreads;
            part[q] = add ? part[q] + acc_hd[v] : acc_hd[v];
        }
        if (tid < 16) part[16 * C + tid] = add ? part[16 * C + tid] + acc_bh : acc_bh;
    }
}

// --------------------------------------------------------------- d W = [x, h_prev]^T dz and the bias, of the branch's LSTM
// Workgroup (column block, split s, set p): 64 columns of dz (16 a wave), all in + C rows of the matrix (in / 16 + C / 16
// accumulator tiles a lane), the set's rows of the window in 64-row chunks s, s + S, ... in order.  A[c][k] = [x, h_prev][row k][c],
// B[k][n] = dz[row k][n].  The MOA input's third tile is the previous actions in slot order, zero beyond N and where selected.
template <int C, bool kMoa>
__global__ void __launch_bounds__(256) ssd_moa_dw_kernel(WinArgs a) {
    constexpr int kXT = kMoa ? 3 : 2, kMT = kXT + C / 16;
    constexpr int kSt = kMoa ? 2 : 0, kFeat = kMoa ? kX : 0;
    __shared__ float s_b[4 * 64];
    __shared__ int s_slot[256];
    const int tid = threadIdx.x, s = blockIdx.y, p = blockIdx.z;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const int N = a.N, SR = a.step_rows, stride = a.P == 1 ? 1 : N;
    const int R = a.seqs * a.steps;                                  // the set's rows of the window
    if constexpr (kMoa) {
        ssd::moa_slots(N, tid, s_slot);
        __syncthreads();
    }
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
            const bool reset = valid && t > 0 && a.done_prev && a.done_prev[(size_t)(t - 1) * SR + sr] != 0;
            const float *hp = nullptr;                               // h_prev of the row: the state rule of include/ssd.h
            if (valid) {
                if (t == 0) hp = a.ring + (sr * 4 + kSt + Cell::kRowH) * C;
                else if (!reset) hp = a.st + ((rw - SR) * 2 + Cell::kRowH) * C;
            }
            const float b = valid ? a.gz[rw * 4 * C + n0 + l15] : 0.f;
            bsum += b;
            float av[kMT];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) av[mt] = valid ? a.feat[rw * 2 * kX + kFeat + 16 * mt + l15] : 0.f;
            if constexpr (kMoa) {
                float v = 0.f;
                if (valid && !reset && l15 < N) {
                    const int e = (int)(sr / N), i = (int)(sr - (size_t)e * N);
                    v = (float)a.prev[(size_t)t * SR + (size_t)e * N + s_slot[i * 16 + l15]];
                }
                av[2] = v;
            }
#pragma unroll
            for (int mt = kXT; mt < kMT; ++mt) av[mt] = hp ? hp[16 * (mt - kXT) + l15] : 0.f;
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt], 0, 0, 0);
        }
    }

    float *part = a.part_w + ((size_t)p * a.S + s) * (size_t)((16 * kXT + C) * 4 * C + 4 * C);
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
        float *dst = part + (size_t)(16 * kXT + C) * 4 * C + n0 + l15;
        *dst = add ? *dst + sum : sum;
    }
}

// ------------------------------------------------------------------------------------- pred_w = h2'^T dpred, and pred_b
// As ssd_moa_dw_kernel with A[c][k] = h2'[row k][c] (the step's own output) and B[k][n] = dpred[row k][n]: workgroup (block of
// 64 prediction columns, split s, set p), C / 16 accumulator tiles a lane; columns beyond (N - 1) A are read as zero.
template <int C>
__global__ void __launch_bounds__(256) ssd_moa_dpred_kernel(WinArgs a) {
    constexpr int kMT = C / 16;
    __shared__ float s_b[4 * 64];
    const int tid = threadIdx.x, s = blockIdx.y, p = blockIdx.z;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int n0 = blockIdx.x * 64 + wave * 16, col = n0 + l15;
    const int NA = (a.N - 1) * a.A, PP = a.pred_pitch;
    const int SR = a.step_rows, stride = a.P == 1 ? 1 : a.N;
    const int R = a.seqs * a.steps;
    (void)SR;
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
            const float *h = a.st + (rw * 2 + Cell::kRowH) * C;
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
    s_b[tid] = bsum;                                                 // [wave][l4][l15]
    __syncthreads();
    if (l4 == 0 && col < PP) {
        const float sum = ((s_b[wave * 64 + l15] + s_b[wave * 64 + 16 + l15]) + s_b[wave * 64 + 32 + l15]) + s_b[wave * 64 + 48 + l15];
        float *dst = part + (size_t)C * PP + col;
        *dst = add ? *dst + sum : sum;
    }
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
hipError_t launch_window(int loss, WinArgs a, const float *wT_act, const float *wT_moa, float *part_wa, float *part_wm,
                         hipStream_t stream) {
    const dim3 seq_grid((unsigned)a.G, (unsigned)a.P), w_grid(4 * C / 64, (unsigned)a.S, (unsigned)a.P);
    a.wT = wT_act; a.part_w = part_wa;
    if (loss == ssd::kLossAc) hipLaunchKernelGGL((ssd_moa_seq_kernel<C, false, ssd::kLossAc>), seq_grid, dim3(4 * C), 0, stream, a);
    else hipLaunchKernelGGL((ssd_moa_seq_kernel<C, false, ssd::kLossPpo>), seq_grid, dim3(4 * C), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd_moa_dw_kernel<C, false>), w_grid, dim3(256), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    a.wT = wT_moa; a.part_w = part_wm;
    hipLaunchKernelGGL((ssd_moa_seq_kernel<C, true, ssd::kLossPpo>), seq_grid, dim3(4 * C), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd_moa_dw_kernel<C, true>), w_grid, dim3(256), 0, stream, a);
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
    using ssd::policy_fail;
    const bool ac = loss == ssd::kLossAc;
    if (!weights) return policy_fail("weights are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetMoa, weights, num_sets, num_agents, num_actions, cell_size)) return policy_fail(why);
    if (n_steps < 1 || num_envs < 1) return policy_fail("n_steps and num_envs must be >= 1");
    if (seq_len < 1) return policy_fail("seq_len must be >= 1");
    const int64_t rows = (int64_t)n_steps * num_envs * num_agents;
    if (rows > INT32_MAX - 16) return policy_fail("n_steps * num_envs * num_agents must be at most 2^31 - 17");
    if (!obs && !(obs_first && n_steps == 1)) return policy_fail("obs is required (it may be null only with obs_first and n_steps 1)");
    if (!state) return policy_fail("state is required");
    if (reinterpret_cast<uintptr_t>(state) & 3u) return policy_fail("state must be 4-byte aligned");
    if (!prev_actions) return policy_fail("prev_actions is required");
    if (reinterpret_cast<uintptr_t>(prev_actions) & 3u) return policy_fail("prev_actions must be 4-byte aligned");
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
    if (!isfinite(moa_weight) || moa_weight < 0.0) return policy_fail("moa_weight must be finite and >= 0");
    if ((kl_coeff != 0.0) != (behaviour_logits != nullptr))
        return policy_fail("behaviour_logits must be given if and only if kl_coeff is not 0");
    if (flags) return policy_fail("flags must be 0");
    if (const int rc = ssd::policy_use_device(device_id)) return rc;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int K = n_steps, E = num_envs, N = num_agents, P = num_sets, A = num_actions, C = cell_size, T = seq_len;
    const int W = T < K ? T : K;                                     // steps of a whole window
    const size_t SR = (size_t)E * N, win_rows = (size_t)W * SR;
    const int seqs = (int)(SR / P);
    // the scratch: the blocks of SSD_MPPO_SCRATCH_FLOATS, in its order
    WinArgs a{};
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

    hipLaunchKernelGGL(ssd_moa_transpose_kernel, dim3((unsigned)((wa_floats + 255) / 256), (unsigned)P), dim3(256), 0, stream, weights,
                       a.set_floats, SSD_MOA_LSTM_W(C), kX + C, 4 * C, wT_act);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);
    hipLaunchKernelGGL(ssd_moa_transpose_kernel, dim3((unsigned)((wm_floats + 255) / 256), (unsigned)P), dim3(256), 0, stream, weights,
                       a.set_floats, SSD_MOA_MW(C, A), kXM + C, 4 * C, wT_moa);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);

    const size_t obs_step = SR * 675;
    for (int k0 = 0; k0 < K; k0 += T) {
        const int steps = K - k0 < T ? K - k0 : T;
        // the observations the window's rows acted on (the shift of include/ssd.h): `first` for its step 0, `rest` from step 1
        const uint8_t *first = nullptr, *rest = nullptr;
        if (!obs_first) rest = obs + (size_t)k0 * obs_step;          // row k reads obs[k]: `rest` from step 0
        else if (k0 == 0) { first = obs_first; rest = obs; }
        else { first = obs + (size_t)(k0 - 1) * obs_step; rest = obs + (size_t)k0 * obs_step; }
        // 1. the features of both stacks
        ssd::PolicyArgs f{};
        f.w = weights; f.P = P; f.A = A; f.N = N; f.set_floats = a.set_floats;
        hipError_t e = hipSuccess;
        if (first) {
            f.B = E; f.obs = first; f.feat = a.feat;
            e = ssd::launch_policy_moa_features(f, stream);
            if (e == hipSuccess && steps > 1) {
                f.B = (steps - 1) * E; f.obs = rest; f.feat = a.feat + SR * 2 * kX;
                e = ssd::launch_policy_moa_features(f, stream);
            }
        } else {
            f.B = steps * E; f.obs = rest; f.feat = a.feat;
            e = ssd::launch_policy_moa_features(f, stream);
        }
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
        ssd::PpoGradArgs tg{};
        tg.w = weights; tg.P = P; tg.A = A; tg.N = N; tg.set_floats = SSD_MOA_LSTM_W(C); tg.w_pitch = a.set_floats; tg.G = Gt;
        tg.set_rows = steps * seqs; tg.step_rows = (int32_t)SR;
        tg.obs_first = first; tg.obs = rest; tg.scratch = part_trunk; tg.dx = a.dx; tg.accumulate = a.accumulate;
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
