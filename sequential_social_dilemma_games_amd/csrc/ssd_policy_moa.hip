// ssd_policy_moa.hip -- the causal-influence (MOA) policy of run_scripts/train_moa.py (MOA_LSTM, models/moa_model.py:121-311)
// on the device: the actions cell with its heads and action, and the MOA cell with its counterfactual predictions and the
// social-influence reward (algorithms/common_funcs.py:134-195).  The trunk is ssd_policy_kernel's MOA mode (ssd_policy.hip),
// which writes both FC stacks' outputs.  include/ssd.h states the network, the weight layout, the start rule and the reward;
// DESIGN.md section 13 the shape and the tile.  ssd_rollout_policy_moa lives in ssd_capi.hip.
//
// Both kernels: one workgroup = 16 envs of ONE agent index i (so its weight set is uniform) and all C cells: 4C threads, one
// wave per 16 cells.  The pieces are ssd_policy_device.hpp's, shared with the LSTM and Watershed kernels: row_start and load_h,
// the gates z = [in, h] @ W on the matrix cores (lstm_gates), wave w holding the four gate tiles of cells 16w .. 16w + 15, so the
// Keras cell update (KerasCell: gates i, f, c, o; no forget bias) runs in registers.
//   actions cell: [y_0, h1] -> (h1', c1') (cell_update), the logits and value on h1' (heads), the action (pick_actions);
//   MOA cell: [y_1, previous actions, 0-padding, h2] -> z once.  Counterfactual a differs only in the own-action input (row 32
//     of W), so z_a = z + (a - a_prev) W[32]: a rank-1 update in registers, then the cell update, h2'_a to LDS, and the
//     prediction h2'_a @ pred_w (16 x C @ C x (N-1)A) on the matrix cores.  The influence is accumulated per (env, other agent)
//     thread across a in log space (online log-sum-exp for log q), so no counterfactual is kept past its own iteration.
// A state may be updated in place: the actions cell owns rows 0, 1 of a state (h1, c1), the MOA cell rows 2, 3 (h2, c2); every
// row a workgroup reads it also writes, and its h rows are in LDS before any is written.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"

namespace {

constexpr int kM = 16;                  // envs per workgroup
constexpr int kX = SSD_MOA_X;           // FC stack outputs per row
constexpr int kXM = SSD_MOA_XM;         // input rows of the MOA cell: 32 features, N <= 16 actions, zero rows
constexpr int kPredPitch = 225;         // LDS pitch of the predictions: (N - 1) A <= 15 * 15, odd

using ssd::f32x4;
using ssd::id_key;              // the agents' string order (ssd_policy_device.hpp)
using Cell = ssd::KerasCell;             // gates i, f, c~, o, no forget bias; a state is (h, c)

static_assert(SSD_MOA_FC1_W(0) >= SSD_POL_CONV_B + 6 && SSD_MOA_FC % 64 == 0 && SSD_MOA_FC_STRIDE % 64 == 0 &&
              SSD_MOA_FC_STRIDE >= SSD_POL_FC2_B + 32 - SSD_POL_FC1_W, "weight layout of include/ssd.h");
static_assert(kXM >= kX + SSD_MOA_MAX_AGENTS && kXM % 4 == 0, "MOA input rows");
static_assert((SSD_MOA_MAX_AGENTS - 1) * SSD_POL_MAX_ACTIONS <= kPredPitch, "prediction tile");

// ------------------------------------------------------------------------------------------------------------ actions cell
template <int C>
__global__ void __launch_bounds__(4 * C) ssd_policy_moa_actions_kernel(ssd::MoaArgs a) {
    constexpr int kThreads = 4 * C;
    constexpr int kK = kX + C;
    constexpr int kPitch = kK + 36;     // = 4 (mod 64), as the LSTM kernel
    __shared__ float s_in[kM * kPitch];
    __shared__ float s_out[kM * 16];    // logits 0..A-1, value at A
    __shared__ int s_start[kM];

    const int tid = threadIdx.x, i = blockIdx.y, b0 = blockIdx.x * kM;
    const int N = a.N, B = a.B, A = a.A;
    const float *__restrict__ w = a.w + (size_t)(a.P == 1 ? 0 : i) * (size_t)a.set_floats;
    // (h1, c1) of tile row m: rows 0, 1 of its state; nothing of a row past the batch is read or written
    const auto row = [=](int m) { return ssd::StateRow{b0 + m < B, ((size_t)(b0 + m) * N + i) * 4 * C}; };

    // ---- 1. start flags, then [y_0, h1] ----
    if (tid < kM) s_start[tid] = ssd::row_start(a.starts, a.hdr, b0 + tid, (size_t)(b0 + tid) * N + i, B);
    __syncthreads();
    for (int q = tid; q < kM * kX; q += kThreads) {
        const int m = q / kX, k = q - m * kX, b = b0 + m;
        s_in[m * kPitch + k] = b < B ? a.feat[((size_t)b * N + i) * 2 * kX + k] : 0.f;
    }
    ssd::load_h<Cell, C, kM>(s_in + kX, kPitch, s_start, a.state_in, a.state_used, tid, row, row);
    __syncthreads();

    // ---- 2. the gates, 3. the cell update in registers ----
    f32x4 acc[4][1];
    ssd::lstm_gates<C, kK, kPitch, 1>(s_in, w + SSD_MOA_LSTM_W(C), tid, acc);
    __syncthreads();                                         // every wave is done with the h rows of s_in
    ssd::cell_update<Cell, C, 1>(acc, w + SSD_MOA_LSTM_B(C), s_start, a.state_in, a.state_out, s_in + kX, kPitch, tid, row);
    __syncthreads();

    // ---- 4. the heads on h1', 5. the action ----
    ssd::heads<C, kM, kThreads>(a, s_in + kX, kPitch, w + SSD_MOA_LOGITS_W(C), w + SSD_MOA_VALUE_W(C), w + SSD_MOA_LOGITS_B(C, A),
                                w + SSD_MOA_VALUE_B(C), s_out, a.logits_scratch, tid, b0, i);
    if (!a.actions) return;
    __syncthreads();
    ssd::pick_actions<kM>(a, s_out, a.actions_copy, tid, b0, i);
}

// ------------------------------------------------------------------------------------------------------------ MOA cell
template <int C>
__global__ void __launch_bounds__(4 * C) ssd_policy_moa_cell_kernel(ssd::MoaArgs a) {
    constexpr int kThreads = 4 * C;
    constexpr int kK = kXM + C;
    constexpr int kPitch = kK + 20;     // = 4 (mod 64)
    __shared__ float s_in[kM * kPitch];           // [y_1, actions, 0, h2]; then h2'_a of the counterfactual in hand
    __shared__ float s_pred[kM * kPredPitch];     // the counterfactual's predictions [m][j A + k]
    __shared__ float s_lpi[kM * 16];              // log pi of this step's action distribution
    __shared__ float s_kl[kM * 16];               // KL per (env, other agent)
    __shared__ int s_start[kM], s_aprev[kM], s_taken[kM];
    __shared__ int s_sorted[SSD_MOA_MAX_AGENTS], s_slot[SSD_MOA_MAX_AGENTS];   // input slot q -> agent index

    const int tid = threadIdx.x, i = blockIdx.y, b0 = blockIdx.x * kM;
    const int N = a.N, B = a.B, A = a.A, NO = N - 1, NA = NO * A;
    const bool infl = a.taken && a.influence && a.pi_logits;
    const float *__restrict__ w = a.w + (size_t)(a.P == 1 ? 0 : i) * (size_t)a.set_floats;
    // (h2, c2) of tile row m: rows 2, 3 of its state; nothing of a row past the batch is read or written
    const auto row = [=](int m) { return ssd::StateRow{b0 + m < B, (((size_t)(b0 + m) * N + i) * 4 + 2) * C}; };

    // ---- 1. the agent order, start flags, own previous action, this step's action and log pi ----
    if (tid < N) {
        int rank = 0;
        for (int n = 0; n < N; ++n) rank += id_key(n) < id_key(tid);
        s_sorted[rank] = tid;
    }
    if (tid < kM) {
        const int m = tid, b = b0 + m, st = ssd::row_start(a.starts, a.hdr, b, (size_t)b * N + i, B);
        s_start[m] = st;
        const int ap = st ? 0 : a.prev[(size_t)b * N + i];
        s_aprev[m] = ap;
        if (a.prev_used && b < B) a.prev_used[(size_t)b * N + i] = ap;
        s_taken[m] = infl && b < B ? a.taken[(size_t)b * N + i] : -1;
        if (infl && b < B) {
            const float *l = a.pi_logits + ((size_t)b * N + i) * a.pi_stride;
            float mx = l[0];
            for (int k = 1; k < A; ++k) mx = fmaxf(mx, l[k]);
            float s = 0.f;
            for (int k = 0; k < A; ++k) s += expf(l[k] - mx);
            const float lse = mx + logf(s);
            for (int k = 0; k < A; ++k) s_lpi[m * 16 + k] = l[k] - lse;
        }
    }
    __syncthreads();
    if (tid < N) {                                           // slot 0: agent i; slots 1 .. N-1: the others in string order
        int own = 0;
        while (s_sorted[own] != i) ++own;
        s_slot[tid] = tid == 0 ? i : s_sorted[tid - 1 < own ? tid - 1 : tid];
    }
    __syncthreads();

    // ---- 2. [y_1, the previous actions (zero at a start), zero rows, h2] ----
    for (int q = tid; q < kM * kXM; q += kThreads) {
        const int m = q / kXM, k = q - m * kXM, b = b0 + m;
        float v = 0.f;
        if (b < B) {
            if (k < kX) v = a.feat[(((size_t)b * N + i) * 2 + 1) * kX + k];
            else if (k - kX < N && !s_start[m]) v = (float)a.prev[(size_t)b * N + s_slot[k - kX]];
        }
        s_in[m * kPitch + k] = v;
    }
    ssd::load_h<Cell, C, kM>(s_in + kXM, kPitch, s_start, a.state_in, a.state_used, tid, row, row);
    __syncthreads();

    // ---- 3. the gates of the true input, once ----
    f32x4 acc1[4][1];
    const float *wm = w + SSD_MOA_MW(C, A);
    ssd::lstm_gates<C, kK, kPitch, 1>(s_in, wm, tid, acc1);
    __syncthreads();                                         // every wave is done with the h rows of s_in

    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * wave + l15;
    float wrow[4], cin[4];                                   // kernel row 32 (the own action) of this lane's cell; c2 of its envs
    f32x4 acc[4];                                            // the gates with the bias
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        wrow[g] = wm[(size_t)kX * 4 * C + g * C + u];
        acc[g] = acc1[g][0] + w[SSD_MOA_MB(C, A) + g * C + u];
    }
    // ---- 4. the true update advances the state (c2 stays in registers for the counterfactuals: not cell_update) ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const ssd::StateRow st = row(4 * l4 + r);
        cin[r] = s_start[4 * l4 + r] ? 0.f : a.state_in[st.at + Cell::kRowC * C + u];
        if (a.state_out && st.mine) {
            float c2, h2;
            Cell::update(acc[0][r], acc[1][r], acc[2][r], acc[3][r], cin[r], &c2, &h2);
            a.state_out[st.at + Cell::kRowH * C + u] = h2;
            a.state_out[st.at + Cell::kRowC * C + u] = c2;
        }
    }

    // ---- 5. the counterfactuals a = 0 .. A-1 and the influence ----
    const int im = tid / (NO > 0 ? NO : 1), ij = tid - im * NO;   // this thread's (env, other agent) of the influence
    const bool mine = infl && tid < kM * NO;
    float lp[16], lqm[16], lqs[16];                          // log p; running max and sum of the log-sum-exp of log q
#pragma unroll
    for (int k = 0; k < 16; ++k) { lp[k] = __builtin_nanf(""); lqm[k] = -INFINITY; lqs[k] = 0.f; }
    const int tiles = (NA + 15) / 16;
    for (int ca = 0; ca < A; ++ca) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * l4 + r;
            const float d = (float)(ca - s_aprev[m]);
            float c2, h2;
            Cell::update(acc[0][r] + d * wrow[0], acc[1][r] + d * wrow[1], acc[2][r] + d * wrow[2], acc[3][r] + d * wrow[3], cin[r],
                         &c2, &h2);
            s_in[m * kPitch + kXM + u] = h2;
        }
        __syncthreads();
        for (int t = wave; t < tiles; t += C / 16) {         // pred: wave w takes the 16-column tiles w, w + C / 16, ...
            const int col = 16 * t + l15;
            const float *pw = w + SSD_MOA_PRED_W(C, A) + col;
            const float *a_row = s_in + l15 * kPitch + kXM + l4;
            f32x4 pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int kk = 0; kk < C / 4; ++kk) {
                const float bv = col < NA ? pw[(size_t)(4 * kk + l4) * NA] : 0.f;
                pa = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], bv, pa, 0, 0, 0);
            }
            if (col < NA) {
                const float pb = w[SSD_MOA_PRED_B(C, A, N) + col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = 4 * l4 + r, b = b0 + m;
                    const float v = pa[r] + pb;
                    s_pred[m * kPredPitch + col] = v;
                    if (b < B) {
                        const size_t row = (size_t)b * N + i;
                        if (a.cf_logits) a.cf_logits[(row * A + ca) * NA + col] = v;
                        if (a.moa_logits && ca == s_aprev[m]) a.moa_logits[row * NA + col] = v;
                    }
                }
            }
        }
        __syncthreads();
        if (mine) {
            const float *pr = s_pred + im * kPredPitch + ij * A;
            float mx = pr[0];
            for (int k = 1; k < A; ++k) mx = fmaxf(mx, pr[k]);
            float s = 0.f;
            for (int k = 0; k < A; ++k) s += expf(pr[k] - mx);
            const float lse = mx + logf(s), lpi = s_lpi[im * 16 + ca];
            const bool taken = ca == s_taken[im];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < A) {
                    const float ls = pr[k] - lse;
                    if (taken) lp[k] = ls;
                    const float v = lpi + ls;
                    if (v > lqm[k]) {
                        lqs[k] = lqs[k] * expf(lqm[k] - v) + 1.f;
                        lqm[k] = v;
                    } else if (v > -INFINITY) {
                        lqs[k] += expf(v - lqm[k]);
                    }
                }
            }
        }
    }
    if (!infl) return;
    if (mine) {
        float kl = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < A) {
                const float p = expf(lp[k]);
                if (p != 0.f) kl += p * (lp[k] - (lqm[k] + logf(lqs[k])));
            }
        }
        s_kl[im * 16 + ij] = kl;
    }
    __syncthreads();
    if (tid < kM && b0 + tid < B) {
        float s = 0.f;
        for (int j = 0; j < NO; ++j) s += s_kl[tid * 16 + j];
        s = isfinite(s) ? fminf(fmaxf(s, -a.clip), a.clip) : 0.f;
        a.influence[(size_t)(b0 + tid) * N + i] = s;
    }
}

template <int C>
hipError_t launch_actions(const ssd::MoaArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kM - 1) / kM), (unsigned)a.N), block(4 * C);
    hipLaunchKernelGGL((ssd_policy_moa_actions_kernel<C>), grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

template <int C>
hipError_t launch_cell(const ssd::MoaArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kM - 1) / kM), (unsigned)a.N), block(4 * C);
    hipLaunchKernelGGL((ssd_policy_moa_cell_kernel<C>), grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

}  // namespace

namespace ssd {

hipError_t launch_policy_moa_actions(const MoaArgs &a, void *stream) {
    switch (a.C) {
    case 64: return launch_actions<64>(a, stream);
    case 128: return launch_actions<128>(a, stream);
    case 256: return launch_actions<256>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_policy_moa_cell(const MoaArgs &a, void *stream) {
    switch (a.C) {
    case 64: return launch_cell<64>(a, stream);
    case 128: return launch_cell<128>(a, stream);
    case 256: return launch_cell<256>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace ssd

extern "C" {

int ssd_policy_moa_forward(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, const uint8_t *obs,
                           const int32_t *prev_actions, const float *state_in, const uint8_t *starts, int32_t batch,
                           int32_t num_agents, float *scratch, float *state_out, float *logits, float *value, float *moa_logits,
                           float *cf_logits, const int32_t *actions, float *influence, float influence_clip, int32_t device_id,
                           uint32_t flags, void *stream) {
    using ssd::policy_fail;
    if (!weights || !obs || !prev_actions || !state_in || !scratch)
        return policy_fail("weights, obs, prev_actions, state_in and scratch are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetMoa, weights, num_sets, num_agents, num_actions, cell_size, scratch))
        return policy_fail(why);
    if (batch < 1) return policy_fail("batch must be >= 1");
    if (flags) return policy_fail("flags must be 0");
    if ((actions == nullptr) != (influence == nullptr)) return policy_fail("actions and influence go together");
    if (influence && !(influence_clip >= 0.f && influence_clip <= 3.0e38f)) return policy_fail("influence_clip must be finite and >= 0");
    if (const char *why = ssd::check_state_out(state_in, state_out, (size_t)batch * num_agents * 4 * cell_size * sizeof(float)))
        return policy_fail(why);
    if (const int rc = ssd::policy_use_device(device_id)) return rc;
    const size_t rows = (size_t)batch * num_agents;
    ssd::PolicyArgs t{};
    t.w = weights; t.P = num_sets; t.A = num_actions; t.B = batch; t.N = num_agents;
    t.set_floats = SSD_MOA_SET_FLOATS(cell_size, num_actions, num_agents); t.obs = obs; t.feat = scratch;
    hipError_t e = ssd::launch_policy_moa_features(t, stream);
    ssd::MoaArgs m{};
    m.w = weights; m.P = num_sets; m.A = num_actions; m.B = batch; m.N = num_agents; m.C = cell_size; m.set_floats = t.set_floats;
    m.feat = scratch; m.state_in = state_in; m.state_out = state_out; m.starts = starts;
    m.logits = logits; m.logits_scratch = scratch + 64 * rows; m.value = value;
    if (e == hipSuccess) e = ssd::launch_policy_moa_actions(m, stream);
    m.prev = prev_actions; m.pi_logits = m.logits_scratch; m.pi_stride = 16; m.taken = actions;
    m.moa_logits = moa_logits; m.cf_logits = cf_logits; m.influence = influence; m.clip = influence_clip;
    if (e == hipSuccess) e = ssd::launch_policy_moa_cell(m, stream);
    return ssd::policy_launched(e);
}

}  // extern "C"
