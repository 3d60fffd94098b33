// ssd_policy_seq.hip -- a sampled fragment of the two recurrent gridworld policies (the baseline's LSTM, ssd_policy_lstm.hip; the
// MOA policy's actions branch, ssd_policy_moa.hip) under the CURRENT weights, every window in one cell launch:
// ssd_policy_lstm_forward_seq and ssd_policy_moa_forward_seq.  include/ssd.h (SEQUENCE FORWARD) states the contract; DESIGN.md
// section 23 the shape, the resources and the measurements.
//
// What an IMPALA learner needs of the target policy (logits, value, the bootstrap value) used to be K + 1 chained calls of the
// per-step forward, each a trunk launch and a cell launch that read and write the carried state through memory.  The state rule
// (include/ssd.h, RECURRENT PPO LOSS AND GRADIENTS) makes the windows independent of each other -- a window's first step takes
// the ring entry as stored -- and the trunk needs no state, so a fragment is: the trunk over all rows (ssd_policy_kernel's
// features mode; for the MOA policy kModeMoaActions, FC stack 0 alone, which this object instantiates), then ONE launch of
// the kernel below over (env tile, agent index, window).
//
// The kernel keeps the per-step kernels' tile: one workgroup = 16 envs of ONE agent index i and all C cells, 4C threads, one wave
// per 16 cells.  It walks its window's steps itself with h in LDS and c in registers; only logits and value leave per step.
// The workgroup of the last window runs one more step, the bootstrap row.  The arithmetic is the per-step kernels', piece by
// piece (row_start, load_h, lstm_gates, Cell::update on the gates plus bias as cell_update forms them, heads), so logits, value,
// the bootstrap value and the state equal the chained per-step forward's, bit for bit.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"
#include "ssd_policy_trunk.hpp"

namespace {

constexpr int kM = 16;                  // envs per workgroup
constexpr int kX = SSD_LSTM_X;          // trunk features per row
constexpr int kMaxWindows = 65535;      // windows of one launch: the grid's z

static_assert(SSD_MOA_X == kX, "both policies' cells take 32 features");

using ssd::f32x4;
using ssd::misaligned;

// The two nets: the cell rule, the rows of a ring entry (the cell's two are the first), and where the cell and the heads sit
// in a weight set.
struct LstmNet {
    using Cell = ssd::RllibCell;
    static constexpr int kStateRows = 2;
    static __host__ __device__ constexpr int cell_w(int C) { return SSD_LSTM_W; }
    static __host__ __device__ constexpr int cell_b(int C) { return SSD_LSTM_B(C); }
    static __host__ __device__ constexpr int logits_w(int C) { return SSD_LSTM_LOGITS_W(C); }
    static __host__ __device__ constexpr int logits_b(int C, int A) { return SSD_LSTM_LOGITS_B(C, A); }
    static __host__ __device__ constexpr int value_w(int C) { return SSD_LSTM_VALUE_W(C); }
    static __host__ __device__ constexpr int value_b(int C) { return SSD_LSTM_VALUE_B(C); }
};
struct MoaActionsNet {
    using Cell = ssd::KerasCell;
    static constexpr int kStateRows = 4;         // (h1, c1, h2, c2): rows 0, 1 are read
    static __host__ __device__ constexpr int cell_w(int C) { return SSD_MOA_LSTM_W(C); }
    static __host__ __device__ constexpr int cell_b(int C) { return SSD_MOA_LSTM_B(C); }
    static __host__ __device__ constexpr int logits_w(int C) { return SSD_MOA_LOGITS_W(C); }
    static __host__ __device__ constexpr int logits_b(int C, int A) { return SSD_MOA_LOGITS_B(C, A); }
    static __host__ __device__ constexpr int value_w(int C) { return SSD_MOA_VALUE_W(C); }
    static __host__ __device__ constexpr int value_b(int C) { return SSD_MOA_VALUE_B(C); }
};

struct SeqArgs {
    const float *w;                // P weight sets of set_floats floats each
    int32_t P, A, E, N, set_floats;
    int32_t K, T;                  // steps of the fragment, seq_len
    int32_t k0;                    // the launch's first step, a multiple of T; grid z = its windows
    int32_t boot;                  // the launch holds the fragment's last window: that workgroup runs the bootstrap row
    const float *feat;             // [steps of the launch (+ 1)][E][N][32]: step k0's rows first, the bootstrap's after step K - 1's
    const float *state;            // [ceil(K / T)][E][N][kStateRows][C]
    const uint8_t *done;           // [K][E][N] or null
    float *logits;                 // [K][E][N][A] or null
    float *value;                  // [K][E][N] or null
    float *boot_value;             // [E][N] or null
    float *state_out;              // [E][N][2][C] or null: the cell's state after step K - 1
};

// what heads() reads of its argument block: one step's outputs
struct StepOut {
    int32_t A, B, N;
    float *logits, *value;
};

template <class Net, int C>
__global__ void __launch_bounds__(4 * C) ssd_policy_seq_kernel(SeqArgs a) {
    using Cell = typename Net::Cell;
    constexpr int kThreads = 4 * C;     // C / 16 waves
    constexpr int kK = kX + C;          // rows of the cell's matrix: the MFMA's K
    constexpr int kPitch = kK + 36;     // LDS row pitch, = 4 (mod 64), as the per-step kernels
    constexpr int kR = Net::kStateRows;
    __shared__ float s_in[kM * kPitch];  // rows [x (32), h (C)]; h' after the gates
    __shared__ float s_out[kM * 16];     // logits 0..A-1, value at A (heads' own)
    __shared__ int s_start[kM];

    const int tid = threadIdx.x, i = blockIdx.y, b0 = blockIdx.x * kM;
    const int N = a.N, E = a.E, A = a.A, K = a.K;
    const int lane = tid & 63, u = 16 * (tid >> 6) + (lane & 15), l4 = lane >> 4;
    const float *__restrict__ w = a.w + (size_t)(a.P == 1 ? 0 : i) * (size_t)a.set_floats;
    const size_t step_rows = (size_t)E * N;
    const int kw = a.k0 + (int)blockIdx.z * a.T;                     // the window's first step
    const int len = K - kw < a.T ? K - kw : a.T;
    const int steps = len + (a.boot && kw + len == K ? 1 : 0);       // the last window's workgroup: and the bootstrap row
    const float *ring = a.state + (size_t)(kw / a.T) * step_rows * kR * C;
    // the ring entry's cell state of tile row m: the first two of its kR rows; nothing of an env past the batch is read or written
    const auto ring_row = [=](int m) { return ssd::StateRow{b0 + m < E, ((size_t)(b0 + m) * N + i) * kR * C}; };
    const float *bias = w + Net::cell_b(C);
    const float bz0 = bias[u], bz1 = bias[C + u], bz2 = bias[2 * C + u], bz3 = bias[3 * C + u];
    float c_reg[4] = {0.f, 0.f, 0.f, 0.f};                           // c of rows 4 l4 + r, cell u

    for (int t = 0; t < steps; ++t) {
        const int k = kw + t;                                        // k == K: the bootstrap row
        const float *feat = a.feat + (size_t)(k - a.k0) * step_rows * kX;
        // ---- 1. start flags: none at the window's first step (the ring entry as stored), else done[k - 1] ----
        if (tid < kM) {
            const uint8_t *starts = t > 0 && a.done ? a.done + (size_t)(k - 1) * step_rows : nullptr;
            s_start[tid] = ssd::row_start(starts, nullptr, b0 + tid, (size_t)(b0 + tid) * N + i, E);
        }
        // x of this step.  The x columns were last read by step t - 1's gates, which every wave left before that step's
        // barrier (c), so they may be written here, ahead of barrier (a).
        for (int q = tid; q < kM * kX; q += kThreads) {
            const int m = q / kX, j = q - m * kX, b = b0 + m;
            s_in[m * kPitch + j] = b < E ? feat[((size_t)b * N + i) * kX + j] : 0.f;
        }
        __syncthreads();   // (a) s_start is set; and step t - 1's heads are done reading h', which the start rule below zeroes
        if (t == 0) {
            ssd::load_h<Cell, C, kM>(s_in + kX, kPitch, s_start, ring, nullptr, tid, ring_row, ring_row);
        } else {
            for (int q = tid; q < kM * C; q += kThreads) {           // the carried h' stays where it is; zero at a start
                const int m = q / C;
                if (s_start[m]) s_in[m * kPitch + kX + (q - m * C)] = 0.f;
            }
        }
        __syncthreads();   // (b) [x, h] of all rows is in place before the gates read it

        // ---- 2. the gates on the matrix cores ----
        f32x4 acc[4][1];
        ssd::lstm_gates<C, kK, kPitch, 1>(s_in, w + Net::cell_w(C), tid, acc);
        __syncthreads();   // (c) every wave is done reading the h rows (and x) before h' overwrites them
        // ---- 3. the cell update in registers: cell_update's expression, with c held across the steps ----
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * l4 + r;
            const ssd::StateRow st = ring_row(m);
            if (!st.mine) continue;
            float c = c_reg[r];
            if (s_start[m]) c = 0.f;
            else if (t == 0) c = ring[st.at + Cell::kRowC * C + u];
            float c2, h2;
            Cell::update(acc[0][0][r] + bz0, acc[1][0][r] + bz1, acc[2][0][r] + bz2, acc[3][0][r] + bz3, c, &c2, &h2);
            s_in[m * kPitch + kX + u] = h2;
            c_reg[r] = c2;
            if (k == K - 1 && a.state_out) {
                const size_t at = ((size_t)(b0 + m) * N + i) * 2 * C;
                a.state_out[at + Cell::kRowC * C + u] = c2;
                a.state_out[at + Cell::kRowH * C + u] = h2;
            }
        }
        __syncthreads();   // (d) h' of all rows is written before the heads read it; s_start is free for the next step

        // ---- 4. the heads on h': logits and value of step k, or the bootstrap value alone ----
        StepOut o{A, E, N, nullptr, nullptr};
        if (k == K) {
            o.value = a.boot_value;
        } else {
            o.logits = a.logits ? a.logits + (size_t)k * step_rows * A : nullptr;
            o.value = a.value ? a.value + (size_t)k * step_rows : nullptr;
        }
        ssd::heads<C, kM, kThreads>(o, s_in + kX, kPitch, w + Net::logits_w(C), w + Net::value_w(C), w + Net::logits_b(C, A),
                                    w + Net::value_b(C), s_out, nullptr, tid, b0, i);
    }
}

template <class Net>
hipError_t launch_cell(const SeqArgs &a, int C, int windows, void *stream) {
    const dim3 grid((unsigned)((a.E + kM - 1) / kM), (unsigned)a.N, (unsigned)windows), block(4 * C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (C) {
    case 64: hipLaunchKernelGGL((ssd_policy_seq_kernel<Net, 64>), grid, block, 0, st, a); break;
    case 128: hipLaunchKernelGGL((ssd_policy_seq_kernel<Net, 128>), grid, block, 0, st, a); break;
    case 256: hipLaunchKernelGGL((ssd_policy_seq_kernel<Net, 256>), grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// Both entry points: the checks, then the chunks.  A chunk is as many whole windows as the scratch holds (the bootstrap row with
// the last): its rows' features in one trunk launch (two where obs_first splits them), then its windows in one cell launch.
template <class Net>
int forward_seq(ssd::PolicyNet net, const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done, int32_t n_steps,
                int32_t num_envs, int32_t num_agents, float *features, int64_t feature_rows, float *logits, float *value,
                float *bootstrap_value, float *state_out, int32_t device_id, uint32_t flags, void *stream) {
    using ssd::policy_fail;
    if (!weights || !obs || !state || !features) return policy_fail("weights, obs, state and features are required");
    if (const char *why = ssd::check_policy_net(net, weights, num_sets, num_agents, num_actions, cell_size)) return policy_fail(why);
    if (misaligned(state) || misaligned(features) || misaligned(logits) || misaligned(value) || misaligned(bootstrap_value) ||
        misaligned(state_out))
        return policy_fail("float buffers must be 4-byte aligned");
    if (seq_len < 1) return policy_fail("seq_len must be >= 1");
    if (n_steps < 1 || num_envs < 1) return policy_fail("n_steps and num_envs must be >= 1");
    const int64_t step_rows = (int64_t)num_envs * num_agents;
    if (((int64_t)n_steps + 1) * step_rows > (int64_t)INT32_MAX - 16) return policy_fail("at most 2^31 - 17 rows, the bootstrap's included");
    const int64_t cap = feature_rows / step_rows;                    // steps the scratch holds
    if (cap < (int64_t)(seq_len < n_steps ? seq_len : n_steps) + 1)
        return policy_fail("feature_rows must hold one window and the bootstrap row: (min(seq_len, n_steps) + 1) * num_envs * num_agents");
    if (flags) return policy_fail("flags must be 0");
    if (const int rc = ssd::policy_use_device(device_id)) return rc;

    const int K = n_steps, T = seq_len;
    ssd::PolicyArgs f{};
    f.w = weights; f.P = num_sets; f.A = num_actions; f.N = num_agents; f.feat = features;
    f.set_floats = net == ssd::kNetMoa ? SSD_MOA_SET_FLOATS(cell_size, num_actions, num_agents) : SSD_LSTM_SET_FLOATS(cell_size, num_actions);
    const auto trunk = net == ssd::kNetMoa ? launch_policy_mode<kModeMoaActions> : ssd::launch_policy_features;
    SeqArgs a{};
    a.w = weights; a.P = num_sets; a.A = num_actions; a.E = num_envs; a.N = num_agents; a.set_floats = f.set_floats;
    a.K = K; a.T = T; a.feat = features; a.state = state; a.done = done;
    a.logits = logits; a.value = value; a.boot_value = bootstrap_value; a.state_out = state_out;
    const size_t obs_step = (size_t)step_rows * 675;
    for (int k0 = 0; k0 < K;) {
        const int64_t left = (int64_t)K - k0, windows_left = (left + T - 1) / T;
        int64_t windows, steps;                                      // of this chunk; steps counts the bootstrap row
        if (left + 1 <= cap && windows_left <= kMaxWindows) {
            windows = windows_left; steps = left + 1; a.boot = 1;
        } else {                                                     // whole windows, and never the last one without its bootstrap row
            windows = cap / T;
            if (windows > kMaxWindows) windows = kMaxWindows;
            if (windows > windows_left - 1) windows = windows_left - 1;
            steps = windows * T; a.boot = 0;
        }
        // the chunk's rows: row k reads obs_first for k = 0 and obs[k - 1] otherwise (obs[k] without obs_first), by address
        hipError_t e = hipSuccess;
        f.feat = features;
        int64_t rest = steps;
        const uint8_t *rows = obs + (size_t)(obs_first && k0 > 0 ? k0 - 1 : k0) * obs_step;
        if (obs_first && k0 == 0) {
            f.B = num_envs; f.obs = obs_first;
            e = trunk(f, stream);
            f.feat = features + (size_t)step_rows * kX;
            rest = steps - 1;
        }
        if (e == hipSuccess && rest > 0) {
            f.B = (int32_t)(rest * num_envs); f.obs = rows;
            e = trunk(f, stream);
        }
        a.k0 = k0;
        if (e == hipSuccess) e = launch_cell<Net>(a, cell_size, (int)windows, stream);
        if (e != hipSuccess) return ssd::policy_launched(e);
        k0 += (int)(windows * T);                                    // (past K after the last chunk)
    }
    return SSD_OK;
}

}  // namespace

extern "C" {

int ssd_policy_lstm_forward_seq(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                                const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done,
                                int32_t n_steps, int32_t num_envs, int32_t num_agents, float *features, int64_t feature_rows,
                                float *logits, float *value, float *bootstrap_value, float *state_out, int32_t device_id,
                                uint32_t flags, void *stream) {
    return forward_seq<LstmNet>(ssd::kNetLstm, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, done, n_steps,
                                num_envs, num_agents, features, feature_rows, logits, value, bootstrap_value, state_out, device_id,
                                flags, stream);
}

int ssd_policy_moa_forward_seq(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, int32_t seq_len,
                               const uint8_t *obs_first, const uint8_t *obs, const float *state, const uint8_t *done,
                               int32_t n_steps, int32_t num_envs, int32_t num_agents, float *features, int64_t feature_rows,
                               float *logits, float *value, float *bootstrap_value, float *state_out, int32_t device_id,
                               uint32_t flags, void *stream) {
    return forward_seq<MoaActionsNet>(ssd::kNetMoa, weights, num_sets, num_actions, cell_size, seq_len, obs_first, obs, state, done,
                                      n_steps, num_envs, num_agents, features, feature_rows, logits, value, bootstrap_value,
                                      state_out, device_id, flags, stream);
}

}  // extern "C"
