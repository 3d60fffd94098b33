// ssd_policy_lstm.hip -- the recurrent cell of the baseline's policy (RLlib 0.7.6's LSTM on the conv-FC trunk) on the device:
// the cell update, both heads and, in ssd_rollout_policy_lstm (ssd_capi.hip), the action.  The trunk is ssd_policy_kernel's
// features mode (ssd_policy.hip), which writes fc2's output.  include/ssd.h states the network, the weight layout and the start
// rule; DESIGN.md section 12 the shape and the tile.
//
// One workgroup = kM = 16 MT envs of ONE agent index i (so its weight set is uniform) and all C cells: 4C threads, one wave per 16
// cells.
//   1. the start flag of every env (hdr t == 0 or starts[row]), then [x, h] of the kM envs to LDS (h of a starting env is zero
//      and never read); the state used also goes to the state ring;
//   2. z = [x, h] @ lstm_w on the matrix cores, v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain per accumulator):
//      wave w takes cells 16w .. 16w + 15 of all four gates (i, j, f, o), so the D fragments of its 4 x MT accumulators hold
//      the four gates of the same (env, cell) in the same lane and register.  Each weight load of the wave feeds MT MFMAs;
//      the weights stream from L2 (320 KiB per set at C = 128, 1.125 MiB at C = 256) once per workgroup;
//   3. the cell update in registers: c' and h' to the state (in place), h' to LDS;
//   4. logits and value on the VALU (fmaf chains over the C cells of h');
//   5. rollouts: one thread per env picks the action (policy_pick, as ssd_policy_kernel) and its log-probability.
// A state may be updated in place: every row a workgroup reads it also writes, and the h rows are in LDS before any is written.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string>

#include "../../include/ssd.h"
#include "ssd_policy.hpp"

namespace {

constexpr int kX = SSD_LSTM_X;          // trunk features per row

typedef float f32x4 __attribute__((ext_vector_type(4)));

static_assert(SSD_LSTM_W >= SSD_POL_FC2_B + 32 && SSD_LSTM_W % 64 == 0, "weight layout of include/ssd.h");

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

template <int C, int MT>
__global__ void __launch_bounds__(4 * C) ssd_policy_lstm_kernel(ssd::LstmArgs a) {
    constexpr int kThreads = 4 * C;     // C / 16 waves
    constexpr int kM = 16 * MT;         // envs per workgroup
    constexpr int kK = kX + C;          // rows of lstm_w: the MFMA's K
    constexpr int kPitch = kK + 36;     // LDS row pitch, = 4 (mod 64): lane (l15, l4) of an A load hits bank 4 l15 + l4
    static_assert(kK % 4 == 0 && kPitch % 64 == 4, "tile");
    __shared__ float s_in[kM * kPitch];  // rows [x (32), h (C)]; h' after the gates
    __shared__ float s_out[kM * 16];     // logits 0..A-1, value at A
    __shared__ int s_start[kM];

    const int tid = threadIdx.x, i = blockIdx.y, b0 = blockIdx.x * kM;
    const int N = a.N, B = a.B, A = a.A;
    const float *__restrict__ w = a.w + (size_t)(a.P == 1 ? 0 : i) * (size_t)a.set_floats;

    // ---- 1. start flags, then [x, h] ----
    if (tid < kM) {
        const int b = b0 + tid;
        int st = 1;                                          // (rows past B: zero inputs, nothing read or written)
        if (b < B) st = a.starts ? a.starts[(size_t)b * N + i] != 0 : (a.hdr ? a.hdr[b].y == 0u : 0);
        s_start[tid] = st;
    }
    __syncthreads();
    for (int q = tid; q < kM * kX; q += kThreads) {
        const int m = q / kX, k = q - m * kX, b = b0 + m;
        s_in[m * kPitch + k] = b < B ? a.feat[((size_t)b * N + i) * kX + k] : 0.f;
    }
    for (int q = tid; q < kM * C; q += kThreads) {
        const int m = q / C, u = q - m * C, b = b0 + m;
        float h = 0.f;
        if (!s_start[m]) h = a.state_in[((size_t)b * N + i) * 2 * C + C + u];
        s_in[m * kPitch + kX + u] = h;
        if (a.state_used && b < B) {
            const size_t r = ((size_t)b * N + i) * 2 * C;
            a.state_used[r + u] = s_start[m] ? 0.f : a.state_in[r + u];
            a.state_used[r + C + u] = h;
        }
    }
    __syncthreads();

    // ---- 2. the gates on the matrix cores: A[m][k] = s_in row m, B[k][n] = lstm_w[k][g C + 16 wave + n] ----
    // v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; D: col l & 15, row 4 (l >> 4) + r
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int u = 16 * wave + l15;                           // this lane's cell
    const float *a_row = s_in + l15 * kPitch + l4;
    const float *wg = w + SSD_LSTM_W + (size_t)l4 * 4 * C + u;
    f32x4 acc[4][MT];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int s = 0; s < MT; ++s) acc[g][s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int kk = 0; kk < kK / 4; ++kk) {
        const float *wk = wg + (size_t)kk * 16 * C;
        float bv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) bv[g] = wk[g * C];
        float av[MT];
#pragma unroll
        for (int s = 0; s < MT; ++s) av[s] = a_row[s * 16 * kPitch + 4 * kk];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int s = 0; s < MT; ++s) acc[g][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[g], acc[g][s], 0, 0, 0);
    }
    __syncthreads();                                         // every wave is done with the h rows of s_in

    // ---- 3. the cell update: lane (l15, l4) holds the four gates of cell u for envs 16 s + 4 l4 + r ----
    {
        const float bi = w[SSD_LSTM_B(C) + u], bj = w[SSD_LSTM_B(C) + C + u];
        const float bf = w[SSD_LSTM_B(C) + 2 * C + u], bo = w[SSD_LSTM_B(C) + 3 * C + u];
#pragma unroll
        for (int s = 0; s < MT; ++s) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 16 * s + 4 * l4 + r, b = b0 + m;
                const size_t row = ((size_t)b * N + i) * 2 * C;
                const float c = s_start[m] ? 0.f : a.state_in[row + u];
                const float zi = acc[0][s][r] + bi, zj = acc[1][s][r] + bj, zf = acc[2][s][r] + bf, zo = acc[3][s][r] + bo;
                const float c2 = sigmoidf_(zf + 1.f) * c + sigmoidf_(zi) * tanhf(zj);
                const float h2 = sigmoidf_(zo) * tanhf(c2);
                s_in[m * kPitch + kX + u] = h2;
                if (a.state_out && b < B) {
                    a.state_out[row + u] = c2;
                    a.state_out[row + C + u] = h2;
                }
            }
        }
    }
    __syncthreads();

    // ---- 4. the heads on h' ----
    for (int q = tid; q < kM * 16; q += kThreads) {
        const int m = q >> 4, j = q & 15, b = b0 + m;
        if (j > A) continue;                                 // j < A: logit j; j == A: the value
        const float *hw = j < A ? w + SSD_LSTM_LOGITS_W(C) + j : w + SSD_LSTM_VALUE_W(C);
        const int stride = j < A ? A : 1;
        const float *hr = s_in + m * kPitch + kX;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < C; ++k) s = fmaf(hr[k], hw[k * stride], s);
        s += j < A ? w[SSD_LSTM_LOGITS_B(C, A) + j] : w[SSD_LSTM_VALUE_B(C)];
        s_out[m * 16 + j] = s;
        if (b < B) {
            const size_t row = (size_t)b * N + i;
            if (j < A) {
                if (a.logits) a.logits[row * A + j] = s;
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
        if (a.logp) a.logp[row] = lp;
    }
}

// Envs per workgroup = 16 MT.  Measured on Harvest 4096 x 5: MT = 1 was fastest at C = 128 and 256 (the
// more workgroups in flight hide the weight loads better than MT-fold reuse saves bytes).  An experiment build may override it
// (make exp EXP=-DSSD_EXP_LSTM_MT=n).
#ifdef SSD_EXP_LSTM_MT
constexpr int kMT = SSD_EXP_LSTM_MT;
#else
constexpr int kMT = 1;
#endif

template <int C, int MT>
hipError_t launch(const ssd::LstmArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + 16 * MT - 1) / (16 * MT)), (unsigned)a.N), block(4 * C);
    hipLaunchKernelGGL((ssd_policy_lstm_kernel<C, MT>), grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

}  // namespace

namespace ssd {

hipError_t launch_policy_lstm(const LstmArgs &a, void *stream) {
    switch (a.C) {
    case 64: return launch<64, kMT>(a, stream);
    case 128: return launch<128, kMT>(a, stream);
    case 256: return launch<256, kMT>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace ssd

extern "C" {

int ssd_policy_lstm_forward(const float *weights, int32_t num_sets, int32_t num_actions, int32_t cell_size, const uint8_t *obs,
                            const float *state_in, const uint8_t *starts, int32_t batch, int32_t num_agents, float *features,
                            float *state_out, float *logits, float *value, int32_t device_id, uint32_t flags, void *stream) {
    using ssd::policy_fail;
    if (!weights || !obs || !state_in || !features) return policy_fail("weights, obs, state_in and features are required");
    if (reinterpret_cast<uintptr_t>(weights) & 3u) return policy_fail("weights must be 4-byte aligned");
    if (cell_size != 64 && cell_size != 128 && cell_size != 256) return policy_fail("cell_size must be 64, 128 or 256");
    if (num_agents < 1 || num_agents > 64) return policy_fail("num_agents must be 1..64");
    if (num_sets != 1 && num_sets != num_agents) return policy_fail("num_sets must be 1 or num_agents");
    if (num_actions < 1 || num_actions > SSD_POL_MAX_ACTIONS) return policy_fail("num_actions must be 1..15");
    if (batch < 1) return policy_fail("batch must be >= 1");
    if (flags) return policy_fail("flags must be 0");
    const size_t sb = (size_t)batch * num_agents * 2 * cell_size * sizeof(float);
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
    ssd::PolicyArgs t{};
    t.w = weights; t.P = num_sets; t.A = num_actions; t.B = batch; t.N = num_agents;
    t.set_floats = SSD_LSTM_SET_FLOATS(cell_size, num_actions); t.obs = obs; t.feat = features;
    hipError_t e = ssd::launch_policy_features(t, stream);
    if (e == hipSuccess) {
        ssd::LstmArgs a{};
        a.w = weights; a.P = num_sets; a.A = num_actions; a.B = batch; a.N = num_agents; a.C = cell_size; a.set_floats = t.set_floats;
        a.feat = features; a.state_in = state_in; a.state_out = state_out; a.starts = starts; a.logits = logits; a.value = value;
        e = ssd::launch_policy_lstm(a, stream);
    }
    if (e != hipSuccess) {
        ssd::policy_set_error((std::string("policy launch: ") + hipGetErrorString(e)).c_str());
        return SSD_E_DEVICE;
    }
    return SSD_OK;
}

}  // extern "C"
