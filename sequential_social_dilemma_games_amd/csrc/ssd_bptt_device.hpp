// csrc/ssd_bptt_device.hpp -- the device pieces the BPTT gradient kernels are built from, each defined once: the window's
// argument block, the cell's backward, the steps of the sequence kernel (start flags, loads, the forward cell step, the two
// heads, the cell's backward over a lane's rows, dz W^T with the carried dh, the partial sums), the sequence kernel itself, the
// split-K kernel d W = [x, h_prev]^T dz, the column-sum epilogue and the transposer.  Used by ssd_policy_lstm_grad.hip (the
// recurrent policy) and ssd_policy_moa_grad.hip (the MOA policy's two branches); include/ssd.h states the contract, DESIGN.md
// sections 17 and 18 the shape.  ssd_ws_policy_grad.hip (the Watershed policy, section 21) has kernels of its own and calls the
// inline pieces that fit it as they are: cell_state, cell_backward, bptt_column_sum and the transposer.
//
// A user is a Branch, compile-time constants only:
//   Cell                 ssd::RllibCell or ssd::KerasCell (gate order, forget bias, where c and h sit in a state's two rows)
//   kIn                  input columns of the LSTM matrix: 32 features, then 16 action columns where kIn is 48
//   kFeatPitch, kFeat0   floats of a feat / dx row, and where the branch's 32 start in it
//   kRingRows, kRing0    rows of C floats of a ring state, and the first of the branch's two
//   kPad                 LDS pitch of [x, h] is kIn + C + kPad, = 4 (mod 64)
//   kPred                false: the policy head (logits, value; ppo_row / a3c_row); true: the MOA prediction head
//   w(C, A), b(C, A)     float offsets of the LSTM matrix and bias in a weight set
//   logits_w(C), value_w(C), logits_b(C, A), value_b(C)   the policy head's, where kPred is false
// Every sum below is one chain in a fixed order (ssd_policy_device.hpp's rule): a change here changes the bits of all six BPTT
// instantiations, and the tests that hold them to their float64 restatements and to bit-equal repeats see it.
#pragma once
#include "ssd_policy_device.hpp"

namespace ssd {

constexpr int kBpttX = 32;             // a branch's features per row
constexpr int kBpttTile = 16;          // sequences of a sequence-kernel tile (SSD_RPPO_TILE, SSD_MPPO_TILE)
constexpr int kBpttChunk = 64;         // rows of a split-K chunk (SSD_RPPO_CHUNK, SSD_MPPO_CHUNK)
constexpr int kBpttPP = 228;           // LDS pitch of the prediction tile: (N - 1) A <= 225 up to whole k-steps of 4; 36 (mod 64)

static_assert(SSD_RPPO_TILE == kBpttTile && SSD_MPPO_TILE == kBpttTile && SSD_RPPO_CHUNK == kBpttChunk && SSD_MPPO_CHUNK == kBpttChunk,
              "the tiles of the kernels below");
static_assert((SSD_MOA_MAX_AGENTS - 1) * SSD_POL_MAX_ACTIONS <= kBpttPP && kBpttPP % 4 == 0, "prediction tile");

// One window of one branch.  The recurrent policy leaves the MOA fields zero.
struct BpttArgs {
    const float *w;                // P weight sets
    const float *wT;               // [P][4C][in + C]: the branch's LSTM matrix transposed
    int32_t P, A, N, C, set_floats;
    int32_t G;                     // sequence kernel: workgroups per set
    int32_t S;                     // split kernels: splits per set
    int32_t seqs;                  // sequences of one set: E (P = N) or E N (P = 1)
    int32_t step_rows;             // E * N
    int32_t steps;                 // the window's steps
    int32_t accumulate;            // add to the partial sums scratch holds (every window but the first)
    int32_t pred_pitch;            // MOA: SSD_MPPO_PRED_PITCH(A, N)
    const float *ring;             // [E][N][kRingRows][C]: the state the window's first step uses
    const uint8_t *done_prev;      // done[k0 - 1 + t] is the flag step t > 0 of the window looks at: u8 [.][E][N], or null
    const int32_t *actions;        // the per-row arrays at the window's first step
    const int32_t *prev;           // MOA: [steps][E][N], the joint action each step's MOA read, by agent index
    const float *logp_old, *adv, *vt, *vf_pred, *beh;
    PpoHyper h;
    float moa_scale;               // MOA: moa_weight / (N - 1); the A3C call: moa_weight / ((N - 1) set rows), MOALoss being a mean
    float *feat;                   // [steps][E][N][kFeatPitch]
    float *dx;                     // [steps][E][N][kFeatPitch]: d row_loss / d (logits, value) in 0..15 first, then d loss / d x
    float *st;                     // [steps][E][N][2][C]: the branch's two state rows of every row, Cell's order
    float *gz;                     // [steps][E][N][4C]: the gate activations in Cell's column order, then dz
    float *dpred;                  // MOA: [steps][E][N][pred_pitch], d loss / d pred, columns 0 .. (N-1) A - 1 of live rows written
    float *part_seq;               // [P][G][16 C + 16 + SSD_PPO_STAT_FLOATS]
    float *part_w;                 // [P][S][(in + C) 4C + 4C], the branch's
    float *part_pred;              // MOA: [P][S][(C + 1) pred_pitch]
};

template <int C, class Branch> constexpr int kBpttK = Branch::kIn + C;                   // rows of the LSTM matrix
template <int C, class Branch> constexpr int kBpttPitch = Branch::kIn + C + Branch::kPad;  // LDS pitch of [x, h]
template <int C> constexpr int kBpttZP = 4 * C + 4;                                       // LDS pitch of dz, = 4 (mod 64)

// The 16 sequences of set p a tile holds: tile row m is sequence s0 + m, row (s0 + m) stride + p of a step's [E][N] rows.
struct BpttTile {
    int s0, Q, stride, p;
    __device__ __forceinline__ bool live(int m) const { return s0 + m < Q; }
    __device__ __forceinline__ size_t row(int m) const { return (size_t)(s0 + m) * stride + p; }
};

// Entry q of agent row rr's slot order in a step's [E][N] array (the previous actions, or the targets of the prediction).
__device__ __forceinline__ int moa_slot_entry(const int32_t *step, size_t rr, int N, const int *s_slot, int q) {
    const int e = (int)(rr / N), i = (int)(rr - (size_t)e * N);
    return step[(size_t)e * N + s_slot[i * 16 + q]];
}

// ------------------------------------------------------------------------------------------- the cell from its activations
// c' and h' from the activations g = Cell::gates(z) and the c the step used: Cell::update's two products and one sum on the
// values it forms, so the same bits, with each activation evaluated once for the state and for the backward's copy.
template <class Cell>
__device__ __forceinline__ void cell_state(const float (&g)[4], float c, float *c2, float *h2) {
    *c2 = g[Cell::kF] * c + g[Cell::kI] * g[Cell::kJ];
    *h2 = g[Cell::kO] * tanhf(*c2);
}

// ------------------------------------------------------------------------------------------------- the cell's backward
// dh, dc_carry: d loss / d (h', c') of the step, the latter from step t + 1 alone.  g: the stored activations (Cell::gates),
// c2 = c', c_prev the c the step used, start: that state was selected zero.  dz in Cell's column order; *dc_prev is carried on.
template <class Cell>
__device__ __forceinline__ void cell_backward(float dh, float dc_carry, const float (&g)[4], float c2, float c_prev, bool start,
                                              float (&dz)[4], float *dc_prev) {
    const float gi = g[Cell::kI], gj = g[Cell::kJ], gf = g[Cell::kF], go = g[Cell::kO];
    const float tc = tanhf(c2);
    const float dc = dh * go * (1.f - tc * tc) + dc_carry;
    dz[Cell::kI] = dc * gj * (gi * (1.f - gi));
    dz[Cell::kJ] = dc * gi * (1.f - gj * gj);
    dz[Cell::kF] = dc * c_prev * (gf * (1.f - gf));
    dz[Cell::kO] = dh * tc * (go * (1.f - go));
    *dc_prev = start ? 0.f : dc * gf;
}

// ------------------------------------------------------------------------------------------ pieces of the sequence kernel
// The start flags of step t: the step's state is selected zero (or the row is past the set).
__device__ __forceinline__ void bptt_start_flags(const BpttArgs &a, BpttTile tl, int t, int tid, int *s_start) {
    if (tid < kBpttTile)
        s_start[tid] = !tl.live(tid) || (t > 0 && a.done_prev && a.done_prev[(size_t)(t - 1) * a.step_rows + tl.row(tid)] != 0);
}

// The branch's 32 features of step t to columns 0..31 of s_in.
template <int C, class Branch>
__device__ __forceinline__ void bptt_load_feat(const BpttArgs &a, BpttTile tl, int t, int tid, float *s_in) {
    constexpr int kPitch = kBpttPitch<C, Branch>;
    for (int q = tid; q < kBpttTile * kBpttX; q += 4 * C) {
        const int m = q / kBpttX, k = q - m * kBpttX;
        s_in[m * kPitch + k] = tl.live(m) ? a.feat[((size_t)t * a.step_rows + tl.row(m)) * Branch::kFeatPitch + Branch::kFeat0 + k] : 0.f;
    }
}

// MOA: the previous actions in slot order to columns 32..47 of s_in, zero beyond N and where selected.
template <int C, class Branch>
__device__ __forceinline__ void bptt_load_prev(const BpttArgs &a, BpttTile tl, int t, int tid, const int *s_start, const int *s_slot,
                                               float *s_in) {
    constexpr int kPitch = kBpttPitch<C, Branch>;
    for (int q = tid; q < kBpttTile * (Branch::kIn - kBpttX); q += 4 * C) {
        const int m = q >> 4, k = q & 15;
        float v = 0.f;
        if (k < a.N && !s_start[m]) v = (float)moa_slot_entry(a.prev + (size_t)t * a.step_rows, tl.row(m), a.N, s_slot, k);
        s_in[m * kPitch + kBpttX + k] = v;
    }
}

// h the forward step t uses, to the h columns of s_in: the ring's at t = 0, zero where selected, else h' as the step before left it.
template <int C, class Branch>
__device__ __forceinline__ void bptt_load_h(const BpttArgs &a, BpttTile tl, int t, int tid, const int *s_start, float *s_in) {
    using Cell = typename Branch::Cell;
    constexpr int kPitch = kBpttPitch<C, Branch>, kIn = Branch::kIn;
    for (int q = tid; q < kBpttTile * C; q += 4 * C) {
        const int m = q / C, k = q - m * C;
        if (t == 0) s_in[m * kPitch + kIn + k] = tl.live(m) ? a.ring[(tl.row(m) * Branch::kRingRows + Branch::kRing0 + Cell::kRowH) * C + k] : 0.f;
        else if (s_start[m]) s_in[m * kPitch + kIn + k] = 0.f;
    }
}

// c the step t used of tile row m (row rw of the window's arrays), cell u: the state rule of include/ssd.h.
template <int C, class Branch>
__device__ __forceinline__ float bptt_c_prev(const BpttArgs &a, BpttTile tl, int t, int m, size_t rw, int u, const int *s_start) {
    using Cell = typename Branch::Cell;
    if (t == 0) return a.ring[(tl.row(m) * Branch::kRingRows + Branch::kRing0 + Cell::kRowC) * C + u];
    return s_start[m] ? 0.f : a.st[((rw - a.step_rows) * 2 + Cell::kRowC) * C + u];
}

// The forward cell step of the (row, cell) pairs this lane owns from the gates lstm_gates left in acc: h' to LDS, the state and
// the gate activations to scratch.
template <int C, class Branch>
__device__ __forceinline__ void bptt_cell_step(const BpttArgs &a, BpttTile tl, int t, int tid, const f32x4 (&acc)[4][1],
                                               const float *bias, const int *s_start, float *s_in) {
    using Cell = typename Branch::Cell;
    constexpr int kPitch = kBpttPitch<C, Branch>, kIn = Branch::kIn;
    const int lane = tid & 63, l4 = lane >> 4, u = 16 * (tid >> 6) + (lane & 15);
    const float b0 = bias[u], b1 = bias[C + u], b2 = bias[2 * C + u], b3 = bias[3 * C + u];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = 4 * l4 + r;
        if (!tl.live(m)) continue;
        const size_t rw = (size_t)t * a.step_rows + tl.row(m);
        const float c = bptt_c_prev<C, Branch>(a, tl, t, m, rw, u, s_start);
        const float z0 = acc[0][0][r] + b0, z1 = acc[1][0][r] + b1, z2 = acc[2][0][r] + b2, z3 = acc[3][0][r] + b3;
        float c2, h2, g[4];
        Cell::gates(z0, z1, z2, z3, g);
        cell_state<Cell>(g, c, &c2, &h2);
        s_in[m * kPitch + kIn + u] = h2;
        a.st[(rw * 2 + Cell::kRowH) * C + u] = h2;
        a.st[(rw * 2 + Cell::kRowC) * C + u] = c2;
        float *gz = a.gz + rw * 4 * C + u;
        gz[0] = g[0]; gz[C] = g[1]; gz[2 * C] = g[2]; gz[3 * C] = g[3];
    }
}

// The policy head's forward: logits and value of the tile's rows to s_out, then a thread per row forms the loss terms (st) and
// d row_loss / d (logits, value), which go to the row's dx slot.
template <int C, class Branch, int kLoss>
__device__ __forceinline__ void bptt_policy_forward(const BpttArgs &a, BpttTile tl, int t, int tid, const float *w,
                                                    const float *s_in, float *s_out, double (&st)[5]) {
    constexpr int kPitch = kBpttPitch<C, Branch>, kIn = Branch::kIn;
    const int A = a.A;
    if (tid < kBpttTile * 16) {
        const int m = tid >> 4, j = tid & 15;
        if (j <= A)
            s_out[tid] = head<C>(s_in + kIn + m * kPitch, w + Branch::logits_w(C), w + Branch::value_w(C), w + Branch::logits_b(C, A),
                                 w + Branch::value_b(C), A, j);
    }
    __syncthreads();
    if (tid < kBpttTile && tl.live(tid)) {
        const size_t r = (size_t)t * a.step_rows + tl.row(tid);
        int act = a.actions[r];
        act = act < 0 ? 0 : (act >= A ? A - 1 : act);
        float d[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) d[j] = 0.f;
        if constexpr (kLoss == kLossAc)
            a3c_row(s_out + tid * 16, d, A, act, a.adv[r], a.vt[r], a.h, st);
        else
            ppo_row(s_out + tid * 16, d, A, act, a.adv[r], a.vt[r], a.vf_pred[r], a.logp_old[r], a.beh ? a.beh + r * A : nullptr, a.h, st);
#pragma unroll
        for (int j = 0; j < 16; ++j) a.dx[r * Branch::kFeatPitch + Branch::kFeat0 + j] = d[j];
    }
}

// The policy head's backward sums of step t: its derivatives to s_out and h' to the h columns of s_in, then the heads' kernels
// (acc_hd: entry q = tid + 4C v is (k, j) = (q >> 4, q & 15); j == A: the value) and biases (acc_bh, tid < 16).
template <int C, class Branch>
__device__ __forceinline__ void bptt_policy_backward(const BpttArgs &a, BpttTile tl, int t, int tid, float *s_in, float *s_out,
                                                     float (&acc_hd)[4], float &acc_bh) {
    using Cell = typename Branch::Cell;
    constexpr int kPitch = kBpttPitch<C, Branch>, kIn = Branch::kIn, kThreads = 4 * C;
    if (tid < kBpttTile * 16) {
        const int m = tid >> 4, j = tid & 15;
        s_out[tid] = tl.live(m) ? a.dx[((size_t)t * a.step_rows + tl.row(m)) * Branch::kFeatPitch + Branch::kFeat0 + j] : 0.f;
    }
    for (int q = tid; q < kBpttTile * C; q += kThreads) {         // h' of the step
        const int m = q / C, k = q - m * C;
        s_in[m * kPitch + kIn + k] = tl.live(m) ? a.st[(((size_t)t * a.step_rows + tl.row(m)) * 2 + Cell::kRowH) * C + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int q = tid + v * kThreads, k = q >> 4, j = q & 15;
        float sum = 0.f;
#pragma unroll 4
        for (int m = 0; m < kBpttTile; ++m) sum = fmaf(s_in[m * kPitch + kIn + k], s_out[m * 16 + j], sum);
        acc_hd[v] += sum;
    }
    if (tid < 16) {
        float sum = 0.f;
#pragma unroll
        for (int m = 0; m < kBpttTile; ++m) sum += s_out[m * 16 + tid];
        acc_bh += sum;
    }
}

// dh' of cell u from the policy head: heads^T d of the r-th of the lane's four tile rows, d the derivatives [16] of the first
// of them (one LDS base a lane with r a constant offset: four per-row bases were what the C = 256 kernels spilled).
template <int C, class Branch>
__device__ __forceinline__ float bptt_policy_dh(const float *d, int r, const float *w, int A, int u) {
    float dh = 0.f;
    for (int j = 0; j < A; ++j) dh = fmaf(d[r * 16 + j], w[Branch::logits_w(C) + u * A + j], dh);
    return fmaf(d[r * 16 + A], w[Branch::value_w(C) + u], dh);
}

// MOA, the prediction head's forward: h2' pred_w + pred_b on the matrix cores to s_pred [m][j A + k] (wave w takes the
// 16-column tiles w, w + C / 16, ...), then a thread per (row, other agent) forms the cross-entropy (ce_sum) and dpred.
template <int C, class Branch>
__device__ __forceinline__ void bptt_pred_forward(const BpttArgs &a, BpttTile tl, int t, int tid, const float *w,
                                                  const float *s_in, float *s_pred, const int *s_slot, double &ce_sum) {
    constexpr int kPitch = kBpttPitch<C, Branch>, kIn = Branch::kIn;
    const int A = a.A, N = a.N, NO = N - 1, NA = NO * A;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
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
            for (int r = 0; r < 4; ++r) s_pred[(4 * l4 + r) * kBpttPP + col] = pa[r] + pb;
        }
    }
    __syncthreads();
    if (tid < kBpttTile * NO) {
        const int m = tid / NO, j = tid - m * NO;
        if (tl.live(m)) {
            const size_t rr = tl.row(m);
            int tgt = moa_slot_entry(a.actions + (size_t)t * a.step_rows, rr, N, s_slot, j + 1);
            tgt = tgt < 0 ? 0 : (tgt >= A ? A - 1 : tgt);
            const float *pr = s_pred + m * kBpttPP + j * A;
            float mx = pr[0];
            for (int k = 1; k < A; ++k) mx = fmaxf(mx, pr[k]);
            float s = 0.f;
            for (int k = 0; k < A; ++k) s += expf(pr[k] - mx);
            const float lse = mx + logf(s);
            ce_sum += (double)(lse - pr[tgt]);
            float *dp = a.dpred + ((size_t)t * a.step_rows + rr) * a.pred_pitch + j * A;
            for (int k = 0; k < A; ++k) dp[k] = a.moa_scale * (expf(pr[k] - lse) - (k == tgt ? 1.f : 0.f));
        }
    }
}

// MOA, the prediction head's backward: dpred of step t to s_pred (zero beyond (N - 1) A and past the set), then dh2' = dpred
// pred_w^T on the matrix cores: A[m][k] = dpred[m][k], B[k][n] = pred_w[cell 16 wave + n][k]; rows 4 l4 + r, cell u.
template <int C>
__device__ __forceinline__ f32x4 bptt_pred_backward(const BpttArgs &a, BpttTile tl, int t, int tid, const float *w,
                                                    float *s_pred) {
    const int NA = (a.N - 1) * a.A;
    const int lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * (tid >> 6) + l15;
    for (int q = tid; q < kBpttTile * kBpttPP; q += 4 * C) {
        const int m = q / kBpttPP, k = q - m * kBpttPP;
        s_pred[q] = tl.live(m) && k < NA ? a.dpred[((size_t)t * a.step_rows + tl.row(m)) * a.pred_pitch + k] : 0.f;
    }
    __syncthreads();
    const float *a_row = s_pred + l15 * kBpttPP + l4;
    const float *pw = w + SSD_MOA_PRED_W(C, a.A) + (size_t)u * NA + l4;
    const int ksteps = (NA + 3) / 4;
    f32x4 acc_dh = {0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < ksteps; ++kk) {
        const float bv = 4 * kk + l4 < NA ? pw[4 * kk] : 0.f;
        acc_dh = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], bv, acc_dh, 0, 0, 0);
    }
    return acc_dh;
}

// The cell's backward of step t for the (row, cell) pairs this lane owns: dh' = the head's share (dh_pred where the branch
// predicts, else heads^T s_out) + the carried dh, then dz to LDS and over the activations in scratch; dc is carried on.
template <int C, class Branch>
__device__ __forceinline__ void bptt_cell_backward(const BpttArgs &a, BpttTile tl, int t, int tid, const float *w,
                                                   const float *s_out, const int *s_start, f32x4 dh_pred, const float (&dh_c)[4],
                                                   float (&dc_c)[4], float *s_dz) {
    using Cell = typename Branch::Cell;
    const int lane = tid & 63, l4 = lane >> 4, u = 16 * (tid >> 6) + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = 4 * l4 + r;
        float dz[4] = {0.f, 0.f, 0.f, 0.f};
        if (tl.live(m)) {
            const size_t rw = (size_t)t * a.step_rows + tl.row(m);
            float dh;
            if constexpr (Branch::kPred) dh = dh_pred[r];
            else dh = bptt_policy_dh<C, Branch>(s_out + 4 * l4 * 16, r, w, a.A, u);
            dh += dh_c[r];
            float *gz = a.gz + rw * 4 * C + u;
            const float g[4] = {gz[0], gz[C], gz[2 * C], gz[3 * C]};
            const float c2 = a.st[(rw * 2 + Cell::kRowC) * C + u];
            const float c_prev = bptt_c_prev<C, Branch>(a, tl, t, m, rw, u, s_start);
            cell_backward<Cell>(dh, dc_c[r], g, c2, c_prev, s_start[m] != 0, dz, &dc_c[r]);
            gz[0] = dz[0]; gz[C] = dz[1]; gz[2 * C] = dz[2]; gz[3 * C] = dz[3];
        }
        float *z = s_dz + m * kBpttZP<C> + u;
        z[0] = dz[0]; z[C] = dz[1]; z[2 * C] = dz[2]; z[3 * C] = dz[3];
    }
}

// d [x, h_prev] = dz W^T: A[m][k] = dz[m][k], B[k][n] = wT[k][n].  Wave w takes the h columns 16 w .. 16 w + 15 (lane (l15, l4)
// gets dh_prev of cell u for rows 4 l4 + r: the pairs it owns, carried in dh_c and zeroed where the step's state was selected
// zero); waves 0 and 1 also the 32 feature columns, to dx (the action columns of the MOA input are data: nothing flows into them).
template <int C, class Branch>
__device__ __forceinline__ void bptt_dz_wT(const BpttArgs &a, BpttTile tl, int t, int tid, const float *wT,
                                           const float *s_dz, const int *s_start, float (&dh_c)[4]) {
    constexpr int kK = kBpttK<C, Branch>, kZP = kBpttZP<C>;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const float *a_row = s_dz + l15 * kZP + l4;
    const float *bh = wT + (size_t)l4 * kK + Branch::kIn + 16 * wave + l15;
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
            if (tl.live(m)) a.dx[((size_t)t * a.step_rows + tl.row(m)) * Branch::kFeatPitch + Branch::kFeat0 + 16 * wave + l15] = acc_x[r];
        }
    } else {
#pragma unroll 4
        for (int kk = 0; kk < C; ++kk)
            acc_h = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], bh[(size_t)kk * 4 * kK], acc_h, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dh_c[r] = s_start[4 * l4 + r] ? 0.f : acc_h[r];
}

// ------------------------------------------------------------------------------------------------- the sequence kernel
// A workgroup of 4 C threads takes 16 sequences of one weight set (persistent over tiles g, g + G, ...): forward over the
// window's steps, then backward over them in reverse.  kLoss: the policy head's row loss, kLossPpo (ppo_row) or kLossAc
// (a3c_row); the prediction head has one instantiation, the loss kind reaches it through a.moa_scale.
template <int C, class Branch, int kLoss = kLossPpo>
__global__ void __launch_bounds__(4 * C) ssd_bptt_seq_kernel(BpttArgs a) {
    static_assert(!Branch::kPred || kLoss == kLossPpo, "the prediction head has one instantiation");
    constexpr bool kPred = Branch::kPred;
    constexpr int kThreads = 4 * C, kK = kBpttK<C, Branch>, kPitch = kBpttPitch<C, Branch>, kZP = kBpttZP<C>;
    constexpr int kStatFloats = SSD_PPO_STAT_FLOATS;
    __shared__ float s_in[kBpttTile * kPitch];             // rows [x (kIn), h (C)]; h' after the gates
    __shared__ float s_dz[kBpttTile * kZP];
    __shared__ float s_out[kBpttTile * 16];                // policy head: logits 0..A-1 and the value at A; backward: their derivatives
    __shared__ float s_pred[kPred ? kBpttTile * kBpttPP : 4];   // prediction head: [m][j A + k]; backward: dpred
    __shared__ int s_start[kBpttTile];
    __shared__ int s_slot[256];                            // prediction head: [agent][slot] -> agent (moa_slots)
    __shared__ double s_stat[kPred ? 256 : kBpttTile * 5];

    const int tid = threadIdx.x, g = blockIdx.x, p = blockIdx.y;
    const int Q = a.seqs, NO = a.N - 1;
    const float *__restrict__ w = a.w + (size_t)p * (size_t)a.set_floats;
    const float *__restrict__ wT = a.wT + (size_t)p * kK * 4 * C;

    float acc_hd[4] = {0.f, 0.f, 0.f, 0.f};     // policy head: its kernels' sums
    float acc_bh = 0.f;                         // policy head, tid < 16: its biases' sums
    double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // policy head, tid < 16: total, policy, vf, kl, entropy of tile row tid
    double ce_sum = 0.0;                        // prediction head, tid < 16 (N - 1): the cross-entropies of (tile row, other agent)

    if constexpr (kPred) moa_slots(a.N, tid, s_slot);

    const int tiles = Q / kBpttTile + (Q % kBpttTile != 0);
    for (int tile = g; tile < tiles; tile += a.G) {
        const BpttTile tl{tile * kBpttTile, Q, a.P == 1 ? 1 : a.N, p};

        // ---- forward over the window ----
        for (int t = 0; t < a.steps; ++t) {
            __syncthreads();
            bptt_start_flags(a, tl, t, tid, s_start);
            bptt_load_feat<C, Branch>(a, tl, t, tid, s_in);
            __syncthreads();
            if constexpr (Branch::kIn > kBpttX) bptt_load_prev<C, Branch>(a, tl, t, tid, s_start, s_slot, s_in);
            bptt_load_h<C, Branch>(a, tl, t, tid, s_start, s_in);
            __syncthreads();
            f32x4 acc[4][1];
            lstm_gates<C, kK, kPitch, 1>(s_in, w + Branch::w(C, a.A), tid, acc);
            __syncthreads();                                         // every wave is done with the h rows of s_in
            bptt_cell_step<C, Branch>(a, tl, t, tid, acc, w + Branch::b(C, a.A), s_start, s_in);
            __syncthreads();
            if constexpr (kPred) bptt_pred_forward<C, Branch>(a, tl, t, tid, w, s_in, s_pred, s_slot, ce_sum);
            else bptt_policy_forward<C, Branch, kLoss>(a, tl, t, tid, w, s_in, s_out, st);
        }

        // ---- backward over the window ----
        float dh_c[4] = {0.f, 0.f, 0.f, 0.f}, dc_c[4] = {0.f, 0.f, 0.f, 0.f};    // carried to step t - 1: rows 4 l4 + r, cell u
        for (int t = a.steps - 1; t >= 0; --t) {
            __syncthreads();
            bptt_start_flags(a, tl, t, tid, s_start);
            f32x4 dh_pred = {0.f, 0.f, 0.f, 0.f};
            if constexpr (kPred) dh_pred = bptt_pred_backward<C>(a, tl, t, tid, w, s_pred);
            else bptt_policy_backward<C, Branch>(a, tl, t, tid, s_in, s_out, acc_hd, acc_bh);
            bptt_cell_backward<C, Branch>(a, tl, t, tid, w, s_out, s_start, dh_pred, dh_c, dc_c, s_dz);
            __syncthreads();
            bptt_dz_wT<C, Branch>(a, tl, t, tid, wT, s_dz, s_start, dh_c);
        }
    }

    // ---- the workgroup's partial sums and statistics ----
    float *part = a.part_seq + ((size_t)p * a.G + g) * (size_t)(16 * C + 16 + kStatFloats);
    double *part_st = reinterpret_cast<double *>(part + 16 * C + 16);
    const bool add = a.accumulate != 0;
    __syncthreads();
    if constexpr (kPred) {
        if (tid < 256) s_stat[tid] = tid < kBpttTile * NO ? ce_sum : 0.0;
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int q = 0; q < kBpttTile * NO; ++q) sum += s_stat[q];
            sum /= (double)NO;
            part_st[5] = add ? part_st[5] + sum : sum;
        }
    } else {
        if (tid < kBpttTile) {
#pragma unroll
            for (int k = 0; k < 5; ++k) s_stat[tid * 5 + k] = st[k];
        }
        __syncthreads();
        if (tid < 5) {
            double sum = 0.0;
            for (int m = 0; m < kBpttTile; ++m) sum += s_stat[m * 5 + tid];
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

// ------------------------------------------------------------------------------------------------- the split-K kernels
// The column sums of a split-K kernel's B operand: bsum is the lane's sum over its rows (= l4 mod 4) of column n0 + l15; the four
// are added through s_b [wave][l4][l15] in l4 order and, where `write`, stored to or added to *dst by the lanes with l4 == 0.
__device__ __forceinline__ void bptt_column_sum(float *s_b, int tid, float bsum, float *dst, bool write, bool add) {
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    s_b[tid] = bsum;
    __syncthreads();
    if (l4 == 0 && write) {
        const float sum = ((s_b[wave * 64 + l15] + s_b[wave * 64 + 16 + l15]) + s_b[wave * 64 + 32 + l15]) + s_b[wave * 64 + 48 + l15];
        *dst = add ? *dst + sum : sum;
    }
}

// d W = [x, h_prev]^T dz and the bias, of the branch's LSTM.  Workgroup (column block, split s, set p): 64 columns of dz (16 a
// wave), all kIn + C rows of the matrix (kIn / 16 + C / 16 accumulator tiles a lane), the set's rows of the window in 64-row
// chunks s, s + S, ... in order.  A[c][k] = [x, h_prev][row k][c], B[k][n] = dz[row k][n].  h_prev of a row is found by the
// state rule; where kIn is 48 the third input tile is the previous actions in slot order, zero beyond N and where selected.
template <int C, class Branch>
__global__ void __launch_bounds__(256) ssd_bptt_dw_kernel(BpttArgs a) {
    using Cell = typename Branch::Cell;
    constexpr int kXT = Branch::kIn / 16, kMT = kXT + C / 16;
    __shared__ float s_b[4 * 64];
    __shared__ int s_slot[256];
    const int tid = threadIdx.x, s = blockIdx.y, p = blockIdx.z;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const int N = a.N, SR = a.step_rows, stride = a.P == 1 ? 1 : N;
    const int R = a.seqs * a.steps;                                  // the set's rows of the window
    if constexpr (kXT > 2) {
        moa_slots(N, tid, s_slot);
        __syncthreads();
    }
    f32x4 acc[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;                                                // dz[rows = l4 (mod 4)][n0 + l15]

    const int chunks = R / kBpttChunk + (R % kBpttChunk != 0);
    for (int chunk = s; chunk < chunks; chunk += a.S) {
        for (int kk = 0; kk < kBpttChunk / 4; ++kk) {
            const int r = chunk * kBpttChunk + 4 * kk + l4;
            const bool valid = r < R;
            const size_t rw = valid ? (size_t)r * stride + p : 0;    // row of the window's [steps][E][N] arrays
            const int t = (int)(rw / SR);
            const size_t sr = rw - (size_t)t * SR;
            const bool reset = valid && t > 0 && a.done_prev && a.done_prev[(size_t)(t - 1) * SR + sr] != 0;
            const float *hp = nullptr;
            if (valid) {
                if (t == 0) hp = a.ring + (sr * Branch::kRingRows + Branch::kRing0 + Cell::kRowH) * C;
                else if (!reset) hp = a.st + ((rw - SR) * 2 + Cell::kRowH) * C;
            }
            const float b = valid ? a.gz[rw * 4 * C + n0 + l15] : 0.f;
            bsum += b;
            float av[kMT];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) av[mt] = valid ? a.feat[rw * Branch::kFeatPitch + Branch::kFeat0 + 16 * mt + l15] : 0.f;
            if constexpr (kXT > 2) {
                float v = 0.f;
                if (valid && !reset && l15 < N) v = (float)moa_slot_entry(a.prev + (size_t)t * SR, sr, N, s_slot, l15);
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
    bptt_column_sum(s_b, tid, bsum, part + (size_t)(16 * kXT + C) * 4 * C + n0 + l15, true, add);
}

// wT[k][n] = w[n][k] of the K x n4 matrix at float `at` of every weight set: the B operand of dz W^T, made once per call.
static __global__ void __launch_bounds__(256) ssd_bptt_transpose_kernel(const float *w, int set_floats, int at, int K, int n4, float *wT) {
    const int p = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * n4) return;
    const int k = idx / K, n = idx - k * K;
    wT[(size_t)p * K * n4 + idx] = w[(size_t)p * set_floats + at + (size_t)n * n4 + k];
}

}  // namespace ssd
