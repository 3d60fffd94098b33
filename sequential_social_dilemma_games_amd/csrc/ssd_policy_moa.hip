// ssd_policy_moa.hip -- the causal-influence (MOA) policy of run_scripts/train_moa.py (MOA_LSTM, models/moa_model.py:121-311)
// on the device: the actions cell with its heads and action, and the MOA cell with its counterfactual predictions and the
// social-influence reward (algorithms/common_funcs.py:134-195).  The trunk is ssd_policy_kernel's MOA mode (ssd_policy.hip),
// which writes both FC stacks' outputs.  include/ssd.h states the network, the weight layout, the start rule and the reward;
// DESIGN.md section 13 the shape and the tile.  ssd_rollout_policy_moa lives in ssd_capi.hip.
//
// Both kernels: one workgroup = 16 envs of ONE agent index i (so its weight set is uniform) and all C cells: 4C threads, one
// wave per 16 cells.  The gates are the LSTM kernel's (ssd_policy_lstm.hip): z = [in, h] @ W on v_mfma_f32_16x16x4_f32 (exact
// f32: a k-ordered fmaf chain per accumulator), wave w holding the four gate tiles of cells 16w .. 16w + 15, so the Keras cell
// update (gates i, f, c, o; no forget bias) runs in registers.
//   actions cell: [y_0, h1] -> (h1', c1'), the logits and value on h1' (VALU), the action (policy_pick);
//   MOA cell: [y_1, previous actions, 0-padding, h2] -> z once.  Counterfactual a differs only in the own-action input (row 32
//     of W), so z_a = z + (a - a_prev) W[32]: a rank-1 update in registers, then the cell update, h2'_a to LDS, and the
//     prediction h2'_a @ pred_w (16 x C @ C x (N-1)A) on the matrix cores.  The influence is accumulated per (env, other agent)
//     thread across a in log space (online log-sum-exp for log q), so no counterfactual is kept past its own iteration.
// A state may be updated in place: the actions cell owns rows 0, 1 of a state (h1, c1), the MOA cell rows 2, 3 (h2, c2); every
// row a workgroup reads it also writes, and its h rows are in LDS before any is written.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string>

#include "../../include/ssd.h"
#include "ssd_policy.hpp"

namespace {

constexpr int kM = 16;                  // envs per workgroup
constexpr int kX = SSD_MOA_X;           // FC stack outputs per row
constexpr int kXM = SSD_MOA_XM;         // input rows of the MOA cell: 32 features, N <= 16 actions, zero rows
constexpr int kPredPitch = 225;         // LDS pitch of the predictions: (N - 1) A <= 15 * 15, odd

typedef float f32x4 __attribute__((ext_vector_type(4)));

static_assert(SSD_MOA_FC1_W(0) >= SSD_POL_CONV_B + 6 && SSD_MOA_FC % 64 == 0 && SSD_MOA_FC_STRIDE % 64 == 0 &&
              SSD_MOA_FC_STRIDE >= SSD_POL_FC2_B + 32 - SSD_POL_FC1_W, "weight layout of include/ssd.h");
static_assert(kXM >= kX + SSD_MOA_MAX_AGENTS && kXM % 4 == 0, "MOA input rows");
static_assert((SSD_MOA_MAX_AGENTS - 1) * SSD_POL_MAX_ACTIONS <= kPredPitch, "prediction tile");

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// The Keras cell: c' = sigmoid(f) c + sigmoid(i) tanh(c~), h' = sigmoid(o) tanh(c')
__device__ __forceinline__ void keras_cell(float zi, float zf, float zc, float zo, float c, float *c2, float *h2) {
    *c2 = sigmoidf_(zf) * c + sigmoidf_(zi) * tanhf(zc);
    *h2 = sigmoidf_(zo) * tanhf(*c2);
}

// The gates of the 16 rows of s_in (pitch kPitch, K input rows then C h rows): acc[g] = z[., g C + 16 wave + l15] without the
// bias.  v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; D: col l & 15, row 4 (l >> 4) + r
template <int C, int kK, int kPitch>
__device__ __forceinline__ void gates(const float *s_in, const float *__restrict__ wm, int tid, f32x4 acc[4]) {
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const float *a_row = s_in + l15 * kPitch + l4;
    const float *wg = wm + (size_t)l4 * 4 * C + 16 * wave + l15;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int kk = 0; kk < kK / 4; ++kk) {
        const float *wk = wg + (size_t)kk * 16 * C;
        float bv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) bv[g] = wk[g * C];
        const float av = a_row[4 * kk];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[g], acc[g], 0, 0, 0);
    }
}

// start flag of row (b, i): starts[row] in the forward, t == 0 in rollouts; rows past B count as starting (nothing read)
__device__ __forceinline__ int row_start(const ssd::MoaArgs &a, int b, int i) {
    if (b >= a.B) return 1;
    return a.starts ? a.starts[(size_t)b * a.N + i] != 0 : (a.hdr ? a.hdr[b].y == 0u : 0);
}

// ------------------------------------------------------------------------------------------------------------ actions cell
template <int C>
__global__ void __launch_bounds__(4 * C) ssd_policy_moa_actions_kernel(ssd::MoaArgs a) {
    constexpr int kThreads = 4 * C;
    constexpr int kK = kX + C;
    constexpr int kPitch = kK + 36;     // = 4 (mod 64), as the LSTM kernel
    static_assert(kK % 4 == 0 && kPitch % 64 == 4, "tile");
    __shared__ float s_in[kM * kPitch];
    __shared__ float s_out[kM * 16];    // logits 0..A-1, value at A
    __shared__ int s_start[kM];

    const int tid = threadIdx.x, i = blockIdx.y, b0 = blockIdx.x * kM;
    const int N = a.N, B = a.B, A = a.A;
    const float *__restrict__ w = a.w + (size_t)(a.P == 1 ? 0 : i) * (size_t)a.set_floats;

    // ---- 1. start flags, then [y_0, h1] ----
    if (tid < kM) s_start[tid] = row_start(a, b0 + tid, i);
    __syncthreads();
    for (int q = tid; q < kM * kX; q += kThreads) {
        const int m = q / kX, k = q - m * kX, b = b0 + m;
        s_in[m * kPitch + k] = b < B ? a.feat[((size_t)b * N + i) * 2 * kX + k] : 0.f;
    }
    for (int q = tid; q < kM * C; q += kThreads) {
        const int m = q / C, u = q - m * C, b = b0 + m;
        const size_t r = ((size_t)b * N + i) * 4 * C;
        const float h = s_start[m] ? 0.f : a.state_in[r + u];
        s_in[m * kPitch + kX + u] = h;
        if (a.state_used && b < B) {
            a.state_used[r + u] = h;
            a.state_used[r + C + u] = s_start[m] ? 0.f : a.state_in[r + C + u];
        }
    }
    __syncthreads();

    // ---- 2. the gates ----
    f32x4 acc[4];
    gates<C, kK, kPitch>(s_in, w + SSD_MOA_LSTM_W(C), tid, acc);
    __syncthreads();                                         // every wave is done with the h rows of s_in

    // ---- 3. the cell update: lane (l15, l4) holds the four gates of cell u for envs 4 l4 + r ----
    {
        const int lane = tid & 63, u = 16 * (tid >> 6) + (lane & 15), l4 = lane >> 4;
        const float bi = w[SSD_MOA_LSTM_B(C) + u], bf = w[SSD_MOA_LSTM_B(C) + C + u];
        const float bc = w[SSD_MOA_LSTM_B(C) + 2 * C + u], bo = w[SSD_MOA_LSTM_B(C) + 3 * C + u];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * l4 + r, b = b0 + m;
            const size_t row = ((size_t)b * N + i) * 4 * C;
            const float c = s_start[m] ? 0.f : a.state_in[row + C + u];
            float c2, h2;
            keras_cell(acc[0][r] + bi, acc[1][r] + bf, acc[2][r] + bc, acc[3][r] + bo, c, &c2, &h2);
            s_in[m * kPitch + kX + u] = h2;
            if (a.state_out && b < B) {
                a.state_out[row + u] = h2;
                a.state_out[row + C + u] = c2;
            }
        }
    }
    __syncthreads();

    // ---- 4. the heads on h1' ----
    for (int q = tid; q < kM * 16; q += kThreads) {
        const int m = q >> 4, j = q & 15, b = b0 + m;
        if (j > A) continue;                                 // j < A: logit j; j == A: the value
        const float *hw = j < A ? w + SSD_MOA_LOGITS_W(C) + j : w + SSD_MOA_VALUE_W(C);
        const int stride = j < A ? A : 1;
        const float *hr = s_in + m * kPitch + kX;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < C; ++k) s = fmaf(hr[k], hw[k * stride], s);
        s += j < A ? w[SSD_MOA_LOGITS_B(C, A) + j] : w[SSD_MOA_VALUE_B(C)];
        s_out[m * 16 + j] = s;
        if (b < B) {
            const size_t row = (size_t)b * N + i;
            if (j < A) {
                if (a.logits) a.logits[row * A + j] = s;
                if (a.logits_scratch) a.logits_scratch[row * 16 + j] = s;
            } else if (a.value) {
                a.value[row] = s;
            }
        }
    }
    if (!a.actions) return;
    __syncthreads();

    // ---- 5. the action ----
    if (tid < kM && b0 + tid < B) {
        const int b = b0 + tid;
        float lp;
        const int act = ssd::policy_pick(s_out + tid * 16, A, a.greedy, a.greedy ? uint4{} : a.hdr[b], a.seed_lo, a.seed_hi,
                                         a.env_base + (uint32_t)b, (uint32_t)i, &lp);
        const size_t row = (size_t)b * N + i;
        a.actions[row] = act;
        if (a.actions_copy) a.actions_copy[row] = act;
        if (a.logp) a.logp[row] = lp;
    }
}

// Position of agent n in the order of the ids sorted as strings ('agent-10' < 'agent-2'), for n < 100: first digit, then
// the shorter id first, then the second digit.
__device__ __forceinline__ int id_key(int n) { return n < 10 ? 100 * n : 100 * (n / 10) + 1 + n % 10; }

// ------------------------------------------------------------------------------------------------------------ MOA cell
template <int C>
__global__ void __launch_bounds__(4 * C) ssd_policy_moa_cell_kernel(ssd::MoaArgs a) {
    constexpr int kThreads = 4 * C;
    constexpr int kK = kXM + C;
    constexpr int kPitch = kK + 20;     // = 4 (mod 64)
    static_assert(kK % 4 == 0 && kPitch % 64 == 4, "tile");
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

    // ---- 1. the agent order, start flags, own previous action, this step's action and log pi ----
    if (tid < N) {
        int rank = 0;
        for (int n = 0; n < N; ++n) rank += id_key(n) < id_key(tid);
        s_sorted[rank] = tid;
    }
    if (tid < kM) {
        const int m = tid, b = b0 + m, st = row_start(a, b, i);
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
    for (int q = tid; q < kM * C; q += kThreads) {
        const int m = q / C, u = q - m * C, b = b0 + m;
        const size_t r = ((size_t)b * N + i) * 4 * C;
        const float h = s_start[m] ? 0.f : a.state_in[r + 2 * C + u];
        s_in[m * kPitch + kXM + u] = h;
        if (a.state_used && b < B) {
            a.state_used[r + 2 * C + u] = h;
            a.state_used[r + 3 * C + u] = s_start[m] ? 0.f : a.state_in[r + 3 * C + u];
        }
    }
    __syncthreads();

    // ---- 3. the gates of the true input, once ----
    f32x4 acc[4];
    const float *wm = w + SSD_MOA_MW(C, A);
    gates<C, kK, kPitch>(s_in, wm, tid, acc);
    __syncthreads();                                         // every wave is done with the h rows of s_in

    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * wave + l15;
    float wrow[4], cin[4];                                   // kernel row 32 (the own action) of this lane's cell; c2 of its envs
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        wrow[g] = wm[(size_t)kX * 4 * C + g * C + u];
        const float bias = w[SSD_MOA_MB(C, A) + g * C + u];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[g][r] += bias;
    }
    // ---- 4. the true update advances the state ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = 4 * l4 + r, b = b0 + m;
        const size_t row = ((size_t)b * N + i) * 4 * C;
        cin[r] = s_start[m] ? 0.f : a.state_in[row + 3 * C + u];
        if (a.state_out && b < B) {
            float c2, h2;
            keras_cell(acc[0][r], acc[1][r], acc[2][r], acc[3][r], cin[r], &c2, &h2);
            a.state_out[row + 2 * C + u] = h2;
            a.state_out[row + 3 * C + u] = c2;
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
            keras_cell(acc[0][r] + d * wrow[0], acc[1][r] + d * wrow[1], acc[2][r] + d * wrow[2], acc[3][r] + d * wrow[3], cin[r],
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
    if (reinterpret_cast<uintptr_t>(weights) & 3u) return policy_fail("weights must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(scratch) & 3u) return policy_fail("scratch must be 4-byte aligned");
    if (cell_size != 64 && cell_size != 128 && cell_size != 256) return policy_fail("cell_size must be 64, 128 or 256");
    if (num_agents < 2 || num_agents > SSD_MOA_MAX_AGENTS) return policy_fail("the MOA policy needs 2..16 agents");
    if (num_sets != 1 && num_sets != num_agents) return policy_fail("num_sets must be 1 or num_agents");
    if (num_actions < 1 || num_actions > SSD_POL_MAX_ACTIONS) return policy_fail("num_actions must be 1..15");
    if (batch < 1) return policy_fail("batch must be >= 1");
    if (flags) return policy_fail("flags must be 0");
    if ((actions == nullptr) != (influence == nullptr)) return policy_fail("actions and influence go together");
    if (influence && !(influence_clip >= 0.f && influence_clip <= 3.0e38f)) return policy_fail("influence_clip must be finite and >= 0");
    const size_t sb = (size_t)batch * num_agents * 4 * cell_size * sizeof(float);
    if (state_out && state_out != state_in) {
        const char *p = reinterpret_cast<const char *>(state_in), *q = reinterpret_cast<const char *>(state_out);
        if (q < p + sb && p < q + sb) return policy_fail("state_out must be state_in or not overlap it");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return policy_fail("no such HIP device");
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device_id) {
        if (hipSetDevice(device_id) != hipSuccess) { ssd::policy_set_error("hipSetDevice failed"); return SSD_E_DEVICE; }
    }
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
    if (e != hipSuccess) {
        ssd::policy_set_error((std::string("policy launch: ") + hipGetErrorString(e)).c_str());
        return SSD_E_DEVICE;
    }
    return SSD_OK;
}

}  // extern "C"
