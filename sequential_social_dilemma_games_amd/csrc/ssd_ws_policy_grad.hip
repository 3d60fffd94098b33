// ssd_ws_policy_grad.hip -- RLlib's PPO loss of the Watershed baselines' policy (LSTMFCNet: dense0, dense1, a Keras LSTM, a
// 5-wide distribution head and a value head) on the sequences of ONE agent id, with truncated backpropagation through time,
// its statistics and the gradient of every parameter of that id's weight set: ssd_ws_policy_ppo_grad.  include/ssd.h
// (WATERSHED PPO LOSS AND GRADIENTS) states the contract; DESIGN.md section 21 the shape, the resources and the measurements.
// ssd_ws_policy_ac_grad is the same call with the reference's A3C row terms (include/ssd.h, WATERSHED A3C LOSS AND GRADIENTS;
// DESIGN.md section 22): the sequence kernel and the reduce compiled once more with ssd::kLossAc -- a3c_row / ws_gauss_ac_row
// for ppo_row / ws_gauss_row, and the float64 totals rounded as they are, without the division by the rows.
//
// The kernels are this file's own (the shared BPTT kernels of ssd_bptt_device.hpp are built around 32 trunk features a row and
// an integer action; this net has 16 and two kinds of head), put together from the inline pieces the headers define once:
// lstm_gates, head, KerasCell, ppo_row (ssd_policy_device.hpp), cell_state, cell_backward, bptt_column_sum and the transposer
// (ssd_bptt_device.hpp), the dense chains, WsGauss and the argument rules (ssd_ws_policy_device.hpp, shared with the rollout
// kernel and the sequence forward).
//
// The fragment is walked window by window (seq_len steps, the last one possibly shorter) by a host loop that only enqueues.
// Per window, on the caller's scratch:
//   1. ssd_ws_seq_kernel: a workgroup of 4 C threads takes 16 sequences (persistent over tiles g, g + G, ...).  Forward over
//      the window's steps: dense0 and dense1 on the VALU (the rollout kernel's chains), the gates on the matrix cores, the cell
//      in registers, the 5 + 1 head outputs; d0, d1, the gate activations, c' and h' of every row go to scratch, the loss terms
//      of a row to float64 sums and d row_loss / d (dist, value) to the row's dx slot.  Then backward over the steps in
//      reverse: the heads' kernels and biases summed in registers, dh' = heads^T d + the carried dh, dz to LDS and over the
//      activations in scratch, d [d1, h_prev] = dz lstm_w^T on the matrix cores (B from a transposed copy made once per call):
//      d d1 to scratch, dh_prev and dc_prev stay in registers, zeroed where the step's state was selected zero;
//   2. ssd_ws_dw_kernel: d lstm_w = [d1, h_prev]^T dz on the matrix cores, split over a fixed partition of the window's rows
//      (split s takes the 64-row chunks s, s + S, ...), lstm_b the column sums of dz;
//   3. ssd_ws_trunk_kernel: the 480 floats of dense0 and dense1 from d d1, d1, d0 and the observations.
// Every kernel adds its partial sums to what scratch holds from the windows before (the first window stores).  At the end
// ssd_ws_reduce_kernel adds the partials of every entry in order in float64, scales by 1 / rows and rounds once.  No atomics
// anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_bptt_device.hpp"
#include "ssd_ws_policy_device.hpp"

namespace {

using namespace ssd::wsp;               // kX, kObs, kOut, kTile, kTrunk, kHd, Cell, the dense chains, WsGauss and the argument rules
using ssd::f32x4;
using ssd::misaligned;
using ssd::PpoHyper;

constexpr int kChunk = SSD_WSPPO_CHUNK; // rows of a split-K chunk
constexpr int kStatFloats = SSD_PPO_STAT_FLOATS;

static_assert(kChunk == 64, "the chunk of the split-K kernel below");

// One window of the call's one weight set.  Rows of the window's arrays: step t of sequence q is row t Q + q.
struct WsGradArgs {
    const float *w;                // the agent id's weight set
    const float *wT;               // [4C][16 + C]: lstm_w transposed
    int32_t C, Q;
    int32_t G;                     // sequence kernel: workgroups
    int32_t S;                     // split kernel: splits
    int32_t TG;                    // trunk kernel: workgroups
    int32_t steps;                 // the window's steps
    int32_t accumulate;            // add to the partial sums scratch holds (every window but the first)
    int32_t comm;                  // the head: Categorical over dist[0:5] (1) or DiagGaussian(dist[0], dist[1]) (0)
    const float *obs;              // [steps][Q][12] the observations the window's rows acted on
    const float *ring;             // [Q][2][C]: the state the window's first step uses
    const uint8_t *starts;         // [steps][Q] at the window's first step (row t > 0 is looked at), or null
    const float *actions, *logp_old, *adv, *vt, *vf_pred;   // the per-row arrays at the window's first step
    const float *beh;              // [steps][Q][5] or null
    PpoHyper h;
    float *d0, *x;                 // [steps][Q][16]: dense0's and dense1's outputs (after their ReLUs)
    float *dx;                     // [steps][Q][16]: d row_loss / d (dist, value) in 0..7 first, then d loss / d x
    float *st;                     // [steps][Q][2][C]: (h', c') of every row
    float *gz;                     // [steps][Q][4C]: the gate activations in Cell's column order, then dz
    float *part_trunk;             // [TG][kTrunk]
    float *part_seq;               // [G][8 C + 8 + kStatFloats]
    float *part_w;                 // [S][(16 + C) 4C + 4C]
};

// The loss terms of an action agent's row (include/ssd.h, WATERSHED PPO LOSS AND GRADIENTS): ppo_row with RLlib's
// one-dimensional DiagGaussian(mean = l[0], log_std = l[1]) in the place of the Categorical.  The ratio, the surrogate, the
// clipped value loss, the derivatives at the kinks and the statistics are ppo_row's lines; d[2..4] = 0 exactly.
__device__ __forceinline__ void ws_gauss_row(const float *l, float *d, float act, float adv, float vt, float vfp, float lpo,
                                             const float *bl, const PpoHyper &a, double (&st)[5]) {
    const WsGauss gs(l[0], l[1]);
    const float mean = gs.mean, log_std = gs.log_std, sd = gs.sd, value = l[kOut];
    const float z = gs.z(act), logp = gs.logp(z), ent = gs.entropy();
    float kl = 0.f, dkl_mean = 0.f, dkl_ls = 0.f;
    if (bl) {
        // divisions, as the header writes them, not products with 1 / var: x * (1 / x) is not always 1 in float32, and a row
        // whose behaviour dist is the current one must give q = 1, kl = 0 and no KL gradient exactly
        const float dm = bl[0] - mean, var = expf(2.f * log_std);
        const float q = (expf(2.f * bl[1]) + dm * dm) / var;     // (var_old + (mean_old - mean)^2) / var
        kl = ((log_std - bl[1]) + 0.5f * q) - 0.5f;
        dkl_mean = -(dm / var);
        dkl_ls = 1.f - q;
    }
    const float ratio = expf(logp - lpo);
    const float lo = 1.f - a.clip, hi = 1.f + a.clip;
    const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, lo), hi);
    const float surr = fminf(s1, s2);
    const float dsurr = ((ratio >= lo && ratio <= hi) || s1 < s2) ? adv : 0.f;     // d surr / d ratio
    const float d1 = value - vt, dv = value - vfp;
    const float d2 = (vfp + fminf(fmaxf(dv, -a.vf_clip), a.vf_clip)) - vt;
    const float vf1 = d1 * d1, vf2 = d2 * d2;
    const float vf = fmaxf(vf1, vf2);
    const float dvf = (fabsf(dv) <= a.vf_clip || vf1 >= vf2) ? 2.f * d1 : 0.f;     // d vf / d value
    const float row_loss = ((-surr + a.kl_coeff * kl) + a.vf_coeff * vf) - a.ent_coeff * ent;
    st[0] += (double)row_loss; st[1] += (double)(-surr); st[2] += (double)vf; st[3] += (double)kl; st[4] += (double)ent;
    const float gl = -dsurr * ratio;           // d row_loss / d logp
    d[0] = gl * (z / sd) + a.kl_coeff * dkl_mean;
    d[1] = (gl * (z * z - 1.f) - a.ent_coeff) + a.kl_coeff * dkl_ls;
    d[2] = 0.f; d[3] = 0.f; d[4] = 0.f;
    d[kOut] = a.vf_coeff * dvf;
}

// The A3C terms of an action agent's row (include/ssd.h, WATERSHED A3C LOSS AND GRADIENTS): a3c_row with ws_gauss_row's logp and
// entropy in the place of the Categorical's.  Only vf_coeff and ent_coeff of the hyper-parameters are read; st receives total,
// policy, vf, entropy in 0..3 (st[4] is left alone).  No kinks; d[2..4] = 0 exactly.
__device__ __forceinline__ void ws_gauss_ac_row(const float *l, float *d, float act, float adv, float vt, const PpoHyper &a,
                                                double (&st)[5]) {
    const WsGauss gs(l[0], l[1]);
    const float sd = gs.sd, value = l[kOut];
    const float z = gs.z(act), logp = gs.logp(z), ent = gs.entropy();
    const float pi = -(logp * adv);
    const float d1 = value - vt;
    const float vf = 0.5f * (d1 * d1);
    const float row_loss = (pi + a.vf_coeff * vf) - a.ent_coeff * ent;
    st[0] += (double)row_loss; st[1] += (double)pi; st[2] += (double)vf; st[3] += (double)ent;
    d[0] = -adv * (z / sd);
    d[1] = (-adv * (z * z - 1.f)) - a.ent_coeff;
    d[2] = 0.f; d[3] = 0.f; d[4] = 0.f;
    d[kOut] = a.vf_coeff * d1;
}

// ------------------------------------------------------------------------------------------------- the sequence kernel
// kLoss: the row loss, ssd::kLossPpo (ppo_row / ws_gauss_row) or ssd::kLossAc (a3c_row / ws_gauss_ac_row, which do not read
// logp_old, vf_pred or beh).
template <int C, int kLoss>
__global__ void __launch_bounds__(4 * C) ssd_ws_seq_kernel(WsGradArgs a) {
    constexpr int kThreads = 4 * C, kK = kX + C, kPitch = kK + 52, kZP = 4 * C + 4;   // both pitches = 4 (mod 64)
    static_assert(kThreads >= kTile * kX, "tile");
    __shared__ float s_in[kTile * kPitch];     // rows [x (16), h (C)]; h' after the gates
    __shared__ float s_dz[kTile * kZP];
    __shared__ float s_obs[kTile * kObs];
    __shared__ float s_d0[kTile * kX];
    __shared__ float s_wd[kTrunk];             // dense0 and dense1 in the packed layout: read per step, where registers would be held
    __shared__ float s_out[kTile * kHd];       // dist 0..4 and the value at 5; backward: their derivatives
    __shared__ int s_start[kTile];
    __shared__ double s_stat[kTile * 5];

    const int tid0 = threadIdx.x, tid = tid0, g = blockIdx.x, Q = a.Q;
    const float *__restrict__ w = a.w;
    const float *__restrict__ wT = a.wT;

    float acc_hd[2] = {0.f, 0.f};               // the heads' kernels: entry q = tid + 4C v is (cell, output) = (q >> 3, q & 7)
    float acc_bh = 0.f;                         // tid < 8: the heads' biases

    // s_stat[m][k]: total, policy, vf, kl, entropy of tile row m, summed over the tiles and steps (thread m's alone)
    if (tid < kTile * 5) s_stat[tid] = 0.0;
    for (int q = tid; q < kTrunk; q += kThreads) s_wd[q] = w[q];
    const int tiles = Q / kTile + (Q % kTile != 0);
    for (int tile = g; tile < tiles; tile += a.G) {
        const int tile0 = tile * kTile;

        // ---- forward over the window ----
        for (int t = 0; t < a.steps; ++t) {
            __syncthreads();
            // (the tile's first sequence and the thread id are made opaque per step: the per-lane addresses that follow from them
            // are formed where they are used, not once and held -- held, they are what the C = 256 kernel spilled)
            int s0 = tile0, tv = tid0;
            asm volatile("" : "+s"(s0), "+v"(tv));
            const int tid = tv, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * wave + l15;
            const int m2 = tid >> 4, j2 = tid & 15;                  // the dense layers' (row, column), tid < 256
            const auto live = [=](int m) { return s0 + m < Q; };
            const auto row = [=](int tt, int m) { return (size_t)tt * Q + (size_t)(s0 + m); };
            if (tid < kTile) s_start[tid] = !live(tid) || (t > 0 && a.starts && a.starts[row(t, tid)] != 0);
            for (int q = tid; q < kTile * kObs; q += kThreads) {
                const int m = q / kObs;
                s_obs[q] = live(m) ? a.obs[row(t, m) * kObs + (q - m * kObs)] : 0.f;
            }
            __syncthreads();
            for (int q = tid; q < kTile * C; q += kThreads) {        // h the step uses: the ring's at t = 0, zero where selected
                const int m = q / C, k = q - m * C;
                if (t == 0) s_in[m * kPitch + kX + k] = live(m) ? a.ring[((size_t)(s0 + m) * 2 + Cell::kRowH) * C + k] : 0.f;
                else if (s_start[m]) s_in[m * kPitch + kX + k] = 0.f;
            }
            if (tid < kTile * kX) {
                const float v = ws_dense0(s_obs, s_wd, m2, j2);
                s_d0[tid] = v;
                if (live(m2)) a.d0[row(t, m2) * kX + j2] = v;
            }
            __syncthreads();
            if (tid < kTile * kX) {
                const float v = ws_dense1(s_d0, s_wd, m2, j2);
                s_in[m2 * kPitch + j2] = v;
                if (live(m2)) a.x[row(t, m2) * kX + j2] = v;
            }
            __syncthreads();
            f32x4 acc[4][1];
            ssd::lstm_gates<C, kK, kPitch, 1>(s_in, w + SSD_WSP_LSTM_W, tid, acc);
            __syncthreads();                                         // every wave is done with the h rows of s_in
            {
                const float *bias = w + SSD_WSP_LSTM_B(C);
                const float b0 = bias[u], b1 = bias[C + u], b2 = bias[2 * C + u], b3 = bias[3 * C + u];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 4 * l4 + r;
                    if (!live(m)) continue;
                    const size_t rw = row(t, m);
                    float c;
                    if (t == 0) c = a.ring[((size_t)(s0 + m) * 2 + Cell::kRowC) * C + u];
                    else c = s_start[m] ? 0.f : a.st[((rw - Q) * 2 + Cell::kRowC) * C + u];
                    float c2, h2, gt[4];
                    Cell::gates(acc[0][0][r] + b0, acc[1][0][r] + b1, acc[2][0][r] + b2, acc[3][0][r] + b3, gt);
                    ssd::cell_state<Cell>(gt, c, &c2, &h2);
                    s_in[m * kPitch + kX + u] = h2;
                    a.st[(rw * 2 + Cell::kRowH) * C + u] = h2;
                    a.st[(rw * 2 + Cell::kRowC) * C + u] = c2;
                    float *gz = a.gz + rw * 4 * C + u;
                    gz[0] = gt[0]; gz[C] = gt[1]; gz[2 * C] = gt[2]; gz[3 * C] = gt[3];
                }
            }
            __syncthreads();
            if (tid < kTile * kHd) {                                 // the heads on h'
                const int m = tid >> 3, j = tid & 7;
                if (j <= kOut)
                    s_out[tid] = ssd::head<C>(s_in + m * kPitch + kX, w + SSD_WSP_OUT_W(C), w + SSD_WSP_VALUE_W(C), w + SSD_WSP_OUT_B(C),
                                              w + SSD_WSP_VALUE_B(C), kOut, j);
            }
            __syncthreads();
            if (tid < kTile && live(tid)) {                          // the row's loss terms and d row_loss / d (dist, value)
                const size_t r = row(t, tid);
                float d[kHd];
#pragma unroll
                for (int j = 0; j < kHd; ++j) d[j] = 0.f;
                double st[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) st[k] = s_stat[tid * 5 + k];
                [[maybe_unused]] const float *bl = a.beh ? a.beh + r * kOut : nullptr;
                if (a.comm) {
                    int act = (int)a.actions[r];
                    act = act < 0 ? 0 : (act >= kOut ? kOut - 1 : act);
                    if constexpr (kLoss == ssd::kLossAc)
                        ssd::a3c_row(s_out + tid * kHd, d, kOut, act, a.adv[r], a.vt[r], a.h, st);
                    else
                        ssd::ppo_row(s_out + tid * kHd, d, kOut, act, a.adv[r], a.vt[r], a.vf_pred[r], a.logp_old[r], bl, a.h, st);
                } else {
                    if constexpr (kLoss == ssd::kLossAc)
                        ws_gauss_ac_row(s_out + tid * kHd, d, a.actions[r], a.adv[r], a.vt[r], a.h, st);
                    else
                        ws_gauss_row(s_out + tid * kHd, d, a.actions[r], a.adv[r], a.vt[r], a.vf_pred[r], a.logp_old[r], bl, a.h, st);
                }
#pragma unroll
                for (int j = 0; j < kHd; ++j) a.dx[r * kX + j] = d[j];
#pragma unroll
                for (int k = 0; k < 5; ++k) s_stat[tid * 5 + k] = st[k];
            }
        }

        // ---- backward over the window ----
        float dh_c[4] = {0.f, 0.f, 0.f, 0.f}, dc_c[4] = {0.f, 0.f, 0.f, 0.f};    // carried to step t - 1: rows 4 l4 + r, cell u
        for (int t = a.steps - 1; t >= 0; --t) {
            __syncthreads();
            // (the tile's first sequence and the thread id are made opaque per step: the per-lane addresses that follow from them
            // are formed where they are used, not once and held -- held, they are what the C = 256 kernel spilled)
            int s0 = tile0, tv = tid0;
            asm volatile("" : "+s"(s0), "+v"(tv));
            const int tid = tv, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * wave + l15;
            const auto live = [=](int m) { return s0 + m < Q; };
            const auto row = [=](int tt, int m) { return (size_t)tt * Q + (size_t)(s0 + m); };
            if (tid < kTile) s_start[tid] = !live(tid) || (t > 0 && a.starts && a.starts[row(t, tid)] != 0);
            if (tid < kTile * kHd) {
                const int m = tid >> 3, j = tid & 7;
                s_out[tid] = live(m) ? a.dx[row(t, m) * kX + j] : 0.f;
            }
            for (int q = tid; q < kTile * C; q += kThreads) {        // h' of the step
                const int m = q / C, k = q - m * C;
                s_in[m * kPitch + kX + k] = live(m) ? a.st[(row(t, m) * 2 + Cell::kRowH) * C + k] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 2; ++v) {                            // the heads' kernels
                const int q = tid + v * kThreads, k = q >> 3, j = q & 7;
                float sum = 0.f;
#pragma unroll 4
                for (int m = 0; m < kTile; ++m) sum = fmaf(s_in[m * kPitch + kX + k], s_out[m * kHd + j], sum);
                acc_hd[v] += sum;
            }
            if (tid < kHd) {
                float sum = 0.f;
#pragma unroll
                for (int m = 0; m < kTile; ++m) sum += s_out[m * kHd + tid];
                acc_bh += sum;
            }
            // the cell's backward of the (row, cell) pairs this lane owns
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 4 * l4 + r;
                float dz[4] = {0.f, 0.f, 0.f, 0.f};
                if (live(m)) {
                    const size_t rw = row(t, m);
                    const float *d = s_out + m * kHd;
                    float dh = 0.f;
#pragma unroll
                    for (int j = 0; j < kOut; ++j) dh = fmaf(d[j], w[SSD_WSP_OUT_W(C) + u * kOut + j], dh);
                    dh = fmaf(d[kOut], w[SSD_WSP_VALUE_W(C) + u], dh);
                    dh += dh_c[r];
                    float *gz = a.gz + rw * 4 * C + u;
                    const float gt[4] = {gz[0], gz[C], gz[2 * C], gz[3 * C]};
                    const float c2 = a.st[(rw * 2 + Cell::kRowC) * C + u];
                    float c_prev;
                    if (t == 0) c_prev = a.ring[((size_t)(s0 + m) * 2 + Cell::kRowC) * C + u];
                    else c_prev = s_start[m] ? 0.f : a.st[((rw - Q) * 2 + Cell::kRowC) * C + u];
                    ssd::cell_backward<Cell>(dh, dc_c[r], gt, c2, c_prev, s_start[m] != 0, dz, &dc_c[r]);
                    gz[0] = dz[0]; gz[C] = dz[1]; gz[2 * C] = dz[2]; gz[3 * C] = dz[3];
                }
                float *zr = s_dz + m * kZP + u;
                zr[0] = dz[0]; zr[C] = dz[1]; zr[2 * C] = dz[2]; zr[3 * C] = dz[3];
            }
            __syncthreads();
            // d [x, h_prev] = dz W^T: A[m][k] = dz[m][k], B[k][n] = wT[k][n].  Wave w takes the h columns 16 w .. 16 w + 15;
            // wave 0 also the 16 x columns, to dx.
            {
                const float *a_row = s_dz + l15 * kZP + l4;
                const float *bh = wT + (size_t)l4 * kK + kX + 16 * wave + l15;
                f32x4 acc_h = {0.f, 0.f, 0.f, 0.f}, acc_x = {0.f, 0.f, 0.f, 0.f};
                if (wave == 0) {
                    const float *bx = wT + (size_t)l4 * kK + l15;
#pragma unroll 4
                    for (int kk = 0; kk < C; ++kk) {
                        const float av = a_row[4 * kk];
                        acc_h = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bh[(size_t)kk * 4 * kK], acc_h, 0, 0, 0);
                        acc_x = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bx[(size_t)kk * 4 * kK], acc_x, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = 4 * l4 + r;
                        if (live(m)) a.dx[row(t, m) * kX + l15] = acc_x[r];
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
    float *part = a.part_seq + (size_t)g * (size_t)(kHd * C + kHd + kStatFloats);
    double *part_st = reinterpret_cast<double *>(part + kHd * C + kHd);
    const bool add = a.accumulate != 0;
    __syncthreads();
    if (tid < 5) {
        double sum = 0.0;
        for (int m = 0; m < kTile; ++m) sum += s_stat[m * 5 + tid];
        part_st[tid] = add ? part_st[tid] + sum : sum;
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int q = tid + v * kThreads;
        part[q] = add ? part[q] + acc_hd[v] : acc_hd[v];
    }
    if (tid < kHd) part[kHd * C + tid] = add ? part[kHd * C + tid] + acc_bh : acc_bh;
}

// ------------------------------------------------------------------------------------------------- the split-K kernel
// d lstm_w = [x, h_prev]^T dz and the bias.  Workgroup (column block, split s): 64 columns of dz (16 a wave), all 16 + C rows of
// the matrix (1 + C / 16 accumulator tiles a lane), the window's rows in 64-row chunks s, s + S, ... in order.
// A[c][k] = [x, h_prev][row k][c], B[k][n] = dz[row k][n].  h_prev of a row is found by the state rule.
template <int C>
__global__ void __launch_bounds__(256) ssd_ws_dw_kernel(WsGradArgs a) {
    constexpr int kMT = 1 + C / 16;
    __shared__ float s_b[4 * 64];
    const int tid = threadIdx.x, s = blockIdx.y, Q = a.Q;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const int R = Q * a.steps;                                       // the window's rows
    f32x4 acc[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;                                                // dz[rows = l4 (mod 4)][n0 + l15]

    const int chunks = R / kChunk + (R % kChunk != 0);
    for (int chunk = s; chunk < chunks; chunk += a.S) {
        for (int kk = 0; kk < kChunk / 4; ++kk) {
            const int r = chunk * kChunk + 4 * kk + l4;
            const bool valid = r < R;
            const size_t rw = valid ? (size_t)r : 0;
            const int t = (int)(rw / Q);
            const size_t sq = rw - (size_t)t * Q;
            const bool reset = valid && t > 0 && a.starts && a.starts[rw] != 0;
            const float *hp = nullptr;
            if (valid) {
                if (t == 0) hp = a.ring + (sq * 2 + Cell::kRowH) * C;
                else if (!reset) hp = a.st + ((rw - Q) * 2 + Cell::kRowH) * C;
            }
            const float b = valid ? a.gz[rw * 4 * C + n0 + l15] : 0.f;
            bsum += b;
            float av[kMT];
            av[0] = valid ? a.x[rw * kX + l15] : 0.f;
#pragma unroll
            for (int mt = 1; mt < kMT; ++mt) av[mt] = hp ? hp[16 * (mt - 1) + l15] : 0.f;
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], b, acc[mt], 0, 0, 0);
        }
    }

    float *part = a.part_w + (size_t)s * (size_t)((kX + C) * 4 * C + 4 * C);
    const bool add = a.accumulate != 0;
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float *dst = part + (size_t)(16 * mt + 4 * l4 + r) * 4 * C + n0 + l15;
            *dst = add ? *dst + acc[mt][r] : acc[mt][r];
        }
    }
    ssd::bptt_column_sum(s_b, tid, bsum, part + (size_t)(kX + C) * 4 * C + n0 + l15, true, add);
}

// -------------------------------------------------------------------------------------------------- the trunk's backward
// dense1 and dense0 from d loss / d x (dx), the layers' outputs and the observations: workgroup g of the TG takes the 16-row
// tiles g, g + TG, ... of the window's rows; thread tid sums the entries tid, tid + 256 and tid + 512 of the packed layout
// below lstm_w (a sum per tile in row order, added to the sum carried so far).  ReLU's derivative at 0 is 0.
__global__ void __launch_bounds__(256) ssd_ws_trunk_kernel(WsGradArgs a) {
    __shared__ float s_obs[kTile * kObs], s_d0[kTile * kX], s_dp1[kTile * kX], s_dp0[kTile * kX];
    const int tid = threadIdx.x, g = blockIdx.x, m = tid >> 4, j = tid & 15;
    const int R = a.Q * a.steps;
    const float *__restrict__ w = a.w;
    float acc[3] = {0.f, 0.f, 0.f};
    const int tiles = R / kTile + (R % kTile != 0);
    for (int tile = g; tile < tiles; tile += a.TG) {
        const int r0 = tile * kTile;
        __syncthreads();
        if (tid < kTile * kObs) {
            const int mm = tid / kObs;
            s_obs[tid] = r0 + mm < R ? a.obs[(size_t)(r0 + mm) * kObs + (tid - mm * kObs)] : 0.f;
        }
        {
            const bool valid = r0 + m < R;
            const size_t at = (size_t)(r0 + m) * kX + j;
            s_d0[tid] = valid ? a.d0[at] : 0.f;
            s_dp1[tid] = valid && a.x[at] > 0.f ? a.dx[at] : 0.f;
        }
        __syncthreads();
        {
            float dd = 0.f;                                          // d loss / d d0[m][j] = sum_n dp1[m][n] dense1_w[j][n]
#pragma unroll
            for (int n = 0; n < kX; ++n) dd = fmaf(s_dp1[m * kX + n], w[SSD_WSP_D1_W + j * kX + n], dd);
            s_dp0[tid] = s_d0[tid] > 0.f ? dd : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const int idx = tid + 256 * v;
            if (idx >= kTrunk) continue;
            const float *lhs = nullptr, *rhs = nullptr;             // sum over the tile's rows of lhs[mm][k] rhs[mm][n] (lhs null: 1)
            int lp = 0, k = 0, n = 0;
            if (idx < SSD_WSP_D0_B) { lhs = s_obs; lp = kObs; k = idx >> 4; n = idx & 15; rhs = s_dp0; }
            else if (idx < SSD_WSP_D0_B + kX) { n = idx - SSD_WSP_D0_B; rhs = s_dp0; }
            else if (idx >= SSD_WSP_D1_W && idx < SSD_WSP_D1_B) { lhs = s_d0; lp = kX; k = (idx - SSD_WSP_D1_W) >> 4; n = idx & 15; rhs = s_dp1; }
            else if (idx >= SSD_WSP_D1_B && idx < SSD_WSP_D1_B + kX) { n = idx - SSD_WSP_D1_B; rhs = s_dp1; }
            if (!rhs) continue;
            float sum = 0.f;
            if (lhs) {
#pragma unroll 4
                for (int mm = 0; mm < kTile; ++mm) sum = fmaf(lhs[mm * lp + k], rhs[mm * kX + n], sum);
            } else {
#pragma unroll 4
                for (int mm = 0; mm < kTile; ++mm) sum += rhs[mm * kX + n];
            }
            acc[v] += sum;
        }
    }
    float *part = a.part_trunk + (size_t)g * kTrunk;
    const bool add = a.accumulate != 0;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const int idx = tid + 256 * v;
        if (idx < kTrunk) part[idx] = add ? part[idx] + acc[v] : acc[v];
    }
}

// ------------------------------------------------------------------------------------------------------ the final reduce
struct WsReduceArgs {
    int32_t C, set_floats, rows, TG, G, S;
    const float *part_trunk, *part_seq, *part_w;
    float *grads;                  // [set_floats]
    double *stats;                 // [5], or [4] of the A3C call
};

// The partials of every entry added in order in float64, times 1 / rows, rounded once; the padding floats are zero.
// kLossAc: the sums as they are (the A3C loss is a sum over rows), and the four statistics of the A3C row terms to stats [4].
template <int kLoss>
__global__ void __launch_bounds__(256) ssd_ws_reduce_kernel(WsReduceArgs a) {
    constexpr bool kSum = kLoss == ssd::kLossAc;
    const int idx = blockIdx.x * 256 + threadIdx.x, C = a.C;
    const int seq_pitch = kHd * C + kHd + kStatFloats, w_floats = (kX + C) * 4 * C, w_pitch = w_floats + 4 * C;
    if (idx < a.set_floats) {
        const float *src = nullptr;
        size_t pitch = 0;
        int n = 0;
        if (idx < kTrunk) {
            src = a.part_trunk + idx; pitch = kTrunk; n = a.TG;
        } else if (idx < SSD_WSP_LSTM_W + w_floats) {
            src = a.part_w + (idx - SSD_WSP_LSTM_W); pitch = w_pitch; n = a.S;
        } else if (idx >= SSD_WSP_LSTM_B(C) && idx < SSD_WSP_LSTM_B(C) + 4 * C) {
            src = a.part_w + w_floats + (idx - SSD_WSP_LSTM_B(C)); pitch = w_pitch; n = a.S;
        } else if (idx >= SSD_WSP_OUT_W(C) && idx < SSD_WSP_OUT_W(C) + kOut * C) {
            const int q = idx - SSD_WSP_OUT_W(C);
            src = a.part_seq + (q / kOut) * kHd + q % kOut; pitch = seq_pitch; n = a.G;
        } else if (idx >= SSD_WSP_OUT_B(C) && idx < SSD_WSP_OUT_B(C) + kOut) {
            src = a.part_seq + kHd * C + (idx - SSD_WSP_OUT_B(C)); pitch = seq_pitch; n = a.G;
        } else if (idx >= SSD_WSP_VALUE_W(C) && idx < SSD_WSP_VALUE_W(C) + C) {
            src = a.part_seq + (idx - SSD_WSP_VALUE_W(C)) * kHd + kOut; pitch = seq_pitch; n = a.G;
        } else if (idx == SSD_WSP_VALUE_B(C)) {
            src = a.part_seq + kHd * C + kOut; pitch = seq_pitch; n = a.G;
        }
        double sum = 0.0;
        for (int g = 0; g < n; ++g) sum += (double)src[g * pitch];
        a.grads[idx] = kSum ? (float)sum : (float)(sum / (double)a.rows);
    }
    if (blockIdx.x == 0 && threadIdx.x < (kSum ? 4 : 5)) {
        double sum = 0.0;
        for (int g = 0; g < a.G; ++g)
            sum += reinterpret_cast<const double *>(a.part_seq + (size_t)g * seq_pitch + kHd * C + kHd)[threadIdx.x];
        a.stats[threadIdx.x] = kSum ? sum : sum / (double)a.rows;
    }
}

template <int C>
hipError_t launch_window(int loss, const WsGradArgs &a, hipStream_t stream) {
    if (loss == ssd::kLossPpo) hipLaunchKernelGGL((ssd_ws_seq_kernel<C, ssd::kLossPpo>), dim3((unsigned)a.G), dim3(4 * C), 0, stream, a);
    else hipLaunchKernelGGL((ssd_ws_seq_kernel<C, ssd::kLossAc>), dim3((unsigned)a.G), dim3(4 * C), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((ssd_ws_dw_kernel<C>), dim3(4 * C / 64, (unsigned)a.S), dim3(256), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(ssd_ws_trunk_kernel, dim3((unsigned)a.TG), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// Both entry points.  loss: ssd::kLossPpo or ssd::kLossAc; the A3C call passes null for logp_old, vf_preds and behaviour_dist
// and 0 for the hyper-parameters it does not have.
int ws_grad(int loss, const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id, int32_t seq_len,
            const float *obs, const float *state, const uint8_t *starts, const float *actions, const float *logp_old,
            const float *advantages, const float *value_targets, const float *vf_preds, const float *behaviour_dist, int32_t n_steps,
            int32_t num_seqs, double clip_param, double vf_clip_param, double vf_loss_coeff, double entropy_coeff, double kl_coeff,
            float *scratch, float *grads, double *stats, int32_t device_id, uint32_t flags, void *stream_) {
    using ssd::policy_fail;
    const bool ac = loss == ssd::kLossAc;
    if (const char *why = ws_check_seq_call(weights, num_sets, cell_size, variant, agent_id, seq_len, n_steps, num_seqs, 0))
        return policy_fail(why);
    if (ac) {
        if (!obs || !state || !actions || !advantages || !value_targets)
            return policy_fail("obs, state, actions, advantages and value_targets are required");
    } else if (!obs || !state || !actions || !logp_old || !advantages || !value_targets || !vf_preds) {
        return policy_fail("obs, state, actions, logp_old, advantages, value_targets and vf_preds are required");
    }
    if (!scratch || !grads || !stats) return policy_fail("scratch, grads and stats are required");
    const double hyper[5] = {clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff};
    for (const double x : hyper)
        if (!isfinite(x)) return policy_fail("the hyper-parameters must be finite");
    if (clip_param < 0.0 || vf_clip_param < 0.0) return policy_fail("clip_param and vf_clip_param must be >= 0");
    if (kl_coeff != 0.0 && !behaviour_dist) return policy_fail("kl_coeff != 0 needs behaviour_dist");
    if (misaligned(scratch, 8) || misaligned(stats, 8)) return policy_fail("scratch and stats must be 8-byte aligned");
    if (misaligned(weights, 4) || misaligned(obs, 4) || misaligned(state, 4) || misaligned(actions, 4) || misaligned(logp_old, 4) ||
        misaligned(advantages, 4) || misaligned(value_targets, 4) || misaligned(vf_preds, 4) || misaligned(behaviour_dist, 4) ||
        misaligned(grads, 4))
        return policy_fail("float buffers must be 4-byte aligned");
    if (flags) return policy_fail("flags must be 0");
    if (const int rc = ssd::policy_use_device(device_id)) return rc;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int M = n_steps, Q = num_seqs, C = cell_size, T = seq_len;
    const int W = T < M ? T : M;                                     // steps of a whole window
    const size_t win_rows = (size_t)W * Q;
    const int set_floats = SSD_WSP_SET_FLOATS(C);
    // the scratch: the blocks of SSD_WSPPO_SCRATCH_FLOATS, in its order
    WsGradArgs a{};
    a.w = weights + (size_t)agent_id * set_floats;
    a.C = C; a.Q = Q;
    a.G = SSD_WSPPO_GROUPS(Q);
    a.S = SSD_WSPPO_SPLITS((int64_t)win_rows);
    a.TG = SSD_WSPPO_TRUNK_GROUPS((int64_t)win_rows);
    a.comm = ws_is_comm(variant, agent_id);
    a.h = PpoHyper{(float)clip_param, (float)vf_clip_param, (float)vf_loss_coeff, (float)entropy_coeff, (float)kl_coeff};
    float *at = scratch;
    float *wT = at; at += (size_t)(kX + C) * 4 * C;
    a.wT = wT;
    a.d0 = at; at += win_rows * kX;
    a.x = at; at += win_rows * kX;
    a.dx = at; at += win_rows * kX;
    a.st = at; at += win_rows * 2 * C;
    a.gz = at; at += win_rows * 4 * C;
    a.part_trunk = at; at += (size_t)a.TG * kTrunk;
    a.part_seq = at; at += (size_t)a.G * (kHd * C + kHd + kStatFloats);
    a.part_w = at;

    hipLaunchKernelGGL(ssd::ssd_bptt_transpose_kernel, dim3((unsigned)(((kX + C) * 4 * C + 255) / 256), 1u), dim3(256), 0, stream, a.w,
                       set_floats, SSD_WSP_LSTM_W, kX + C, 4 * C, wT);
    if (const hipError_t e = hipGetLastError()) return ssd::policy_launched(e);

    for (int m0 = 0; m0 < M; m0 += T) {
        const size_t r0 = (size_t)m0 * Q;
        a.steps = M - m0 < T ? M - m0 : T;
        a.accumulate = m0 > 0;
        a.obs = obs + r0 * kObs;
        a.ring = state + (size_t)(m0 / T) * Q * 2 * C;
        a.starts = starts ? starts + r0 : nullptr;                   // row t > 0 of the window looks at starts[m0 + t]
        a.actions = actions + r0; a.adv = advantages + r0; a.vt = value_targets + r0;
        a.logp_old = ac ? nullptr : logp_old + r0;
        a.vf_pred = ac ? nullptr : vf_preds + r0;
        a.beh = kl_coeff != 0.0 ? behaviour_dist + r0 * kOut : nullptr;
        hipError_t e;
        switch (C) {
        case 64: e = launch_window<64>(loss, a, stream); break;
        case 128: e = launch_window<128>(loss, a, stream); break;
        default: e = launch_window<256>(loss, a, stream); break;
        }
        if (e != hipSuccess) return ssd::policy_launched(e);
    }
    WsReduceArgs r{};
    r.C = C; r.set_floats = set_floats; r.rows = (int32_t)((int64_t)M * Q); r.TG = a.TG; r.G = a.G; r.S = a.S;
    r.part_trunk = a.part_trunk; r.part_seq = a.part_seq; r.part_w = a.part_w; r.grads = grads; r.stats = stats;
    const dim3 reduce_grid((unsigned)((set_floats + 255) / 256));
    if (ac) hipLaunchKernelGGL(ssd_ws_reduce_kernel<ssd::kLossAc>, reduce_grid, dim3(256), 0, stream, r);
    else hipLaunchKernelGGL(ssd_ws_reduce_kernel<ssd::kLossPpo>, reduce_grid, dim3(256), 0, stream, r);
    return ssd::policy_launched(hipGetLastError());
}

}  // namespace

extern "C" int ssd_ws_policy_ppo_grad(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id,
                                      int32_t seq_len, const float *obs, const float *state, const uint8_t *starts,
                                      const float *actions, const float *logp_old, const float *advantages,
                                      const float *value_targets, const float *vf_preds, const float *behaviour_dist,
                                      int32_t n_steps, int32_t num_seqs, double clip_param, double vf_clip_param,
                                      double vf_loss_coeff, double entropy_coeff, double kl_coeff, float *scratch, float *grads,
                                      double *stats, int32_t device_id, uint32_t flags, void *stream_) {
    return ws_grad(ssd::kLossPpo, weights, num_sets, cell_size, variant, agent_id, seq_len, obs, state, starts, actions, logp_old,
                   advantages, value_targets, vf_preds, behaviour_dist, n_steps, num_seqs, clip_param, vf_clip_param, vf_loss_coeff,
                   entropy_coeff, kl_coeff, scratch, grads, stats, device_id, flags, stream_);
}

extern "C" int ssd_ws_policy_ac_grad(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id,
                                     int32_t seq_len, const float *obs, const float *state, const uint8_t *starts,
                                     const float *actions, const float *advantages, const float *value_targets, int32_t n_steps,
                                     int32_t num_seqs, double vf_loss_coeff, double entropy_coeff, float *scratch, float *grads,
                                     double *stats, int32_t device_id, uint32_t flags, void *stream_) {
    return ws_grad(ssd::kLossAc, weights, num_sets, cell_size, variant, agent_id, seq_len, obs, state, starts, actions, nullptr,
                   advantages, value_targets, nullptr, nullptr, n_steps, num_seqs, 0.0, 0.0, vf_loss_coeff, entropy_coeff, 0.0,
                   scratch, grads, stats, device_id, flags, stream_);
}
