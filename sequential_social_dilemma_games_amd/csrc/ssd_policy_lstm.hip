// ssd_policy_lstm.hip -- the recurrent cell of the baseline's policy (RLlib 0.7.6's LSTM on the conv-FC trunk) on the device:
// the cell update, both heads and, in ssd_rollout_policy_lstm (ssd_capi.hip), the action.  The trunk is ssd_policy_kernel's
// features mode (ssd_policy.hip), which writes fc2's output.  include/ssd.h states the network, the weight layout and the start
// rule; DESIGN.md section 12 the shape and the tile.
//
// One workgroup = kM = 16 MT envs of ONE agent index i (so its weight set is uniform) and all C cells: 4C threads, one wave per 16
// cells.
//   1. the start flag of every env (row_start: hdr t == 0 or starts[row]), then [x, h] of the kM envs to LDS (load_h: h of a
//      starting env is zero and never read); the state used also goes to the state ring;
//   2. z = [x, h] @ lstm_w on the matrix cores (lstm_gates): wave w takes cells 16w .. 16w + 15 of all four gates (i, j, f, o),
//      so the D fragments of its 4 x MT accumulators hold the four gates of the same (env, cell) in the same lane and register.
//      Each weight load of the wave feeds MT MFMAs; the weights stream from L2 (320 KiB per set at C = 128, 1.125 MiB at
//      C = 256) once per workgroup;
//   3. the cell update in registers (cell_update, RLlib's cell): c' and h' to the state (in place), h' to LDS;
//   4. logits and value on the VALU (heads: fmaf chains over the C cells of h');
//   5. rollouts: one thread per env picks the action (pick_actions, as ssd_policy_kernel) and its log-probability.
// Every step is a piece of ssd_policy_device.hpp, which the MOA and Watershed kernels share; this file keeps the tile.
// A state may be updated in place: every row a workgroup reads it also writes, and the h rows are in LDS before any is written.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"

namespace {

constexpr int kX = SSD_LSTM_X;          // trunk features per row

using ssd::f32x4;
using Cell = ssd::RllibCell;            // gates i, j, f, o, forget bias 1; a state is (c, h)

static_assert(SSD_LSTM_W >= SSD_POL_FC2_B + 32 && SSD_LSTM_W % 64 == 0, "weight layout of include/ssd.h");

template <int C, int MT>
__global__ void __launch_bounds__(4 * C) ssd_policy_lstm_kernel(ssd::LstmArgs a) {
    constexpr int kThreads = 4 * C;     // C / 16 waves
    constexpr int kM = 16 * MT;         // envs per workgroup
    constexpr int kK = kX + C;          // rows of lstm_w: the MFMA's K
    constexpr int kPitch = kK + 36;     // LDS row pitch, = 4 (mod 64)
    __shared__ float s_in[kM * kPitch];  // rows [x (32), h (C)]; h' after the gates
    __shared__ float s_out[kM * 16];     // logits 0..A-1, value at A
    __shared__ int s_start[kM];

    const int tid = threadIdx.x, i = blockIdx.y, b0 = blockIdx.x * kM;
    const int N = a.N, B = a.B, A = a.A;
    const float *__restrict__ w = a.w + (size_t)(a.P == 1 ? 0 : i) * (size_t)a.set_floats;
    // the state of tile row m: [2][C]; nothing of a row past the batch is read or written
    const auto row = [=](int m) { return ssd::StateRow{b0 + m < B, ((size_t)(b0 + m) * N + i) * 2 * C}; };

    // ---- 1. start flags, then [x, h] ----
    if (tid < kM) s_start[tid] = ssd::row_start(a.starts, a.hdr, b0 + tid, (size_t)(b0 + tid) * N + i, B);
    __syncthreads();
    for (int q = tid; q < kM * kX; q += kThreads) {
        const int m = q / kX, k = q - m * kX, b = b0 + m;
        s_in[m * kPitch + k] = b < B ? a.feat[((size_t)b * N + i) * kX + k] : 0.f;
    }
    ssd::load_h<Cell, C, kM>(s_in + kX, kPitch, s_start, a.state_in, a.state_used, tid, row, row);
    __syncthreads();

    // ---- 2. the gates on the matrix cores, 3. the cell update in registers ----
    f32x4 acc[4][MT];
    ssd::lstm_gates<C, kK, kPitch, MT>(s_in, w + SSD_LSTM_W, tid, acc);
    __syncthreads();                                         // every wave is done with the h rows of s_in
    ssd::cell_update<Cell, C, MT>(acc, w + SSD_LSTM_B(C), s_start, a.state_in, a.state_out, s_in + kX, kPitch, tid, row);
    __syncthreads();

    // ---- 4. the heads on h', 5. the action ----
    ssd::heads<C, kM, kThreads>(a, s_in + kX, kPitch, w + SSD_LSTM_LOGITS_W(C), w + SSD_LSTM_VALUE_W(C), w + SSD_LSTM_LOGITS_B(C, A),
                                w + SSD_LSTM_VALUE_B(C), s_out, nullptr, tid, b0, i);
    if (!a.actions) return;
    __syncthreads();
    ssd::pick_actions<kM>(a, s_out, nullptr, tid, b0, i);
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
    if (const char *why = ssd::check_policy_net(ssd::kNetLstm, weights, num_sets, num_agents, num_actions, cell_size)) return policy_fail(why);
    if (batch < 1) return policy_fail("batch must be >= 1");
    if (flags) return policy_fail("flags must be 0");
    if (const char *why = ssd::check_state_out(state_in, state_out, (size_t)batch * num_agents * 2 * cell_size * sizeof(float)))
        return policy_fail(why);
    if (const int rc = ssd::policy_use_device(device_id)) return rc;
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
    return ssd::policy_launched(e);
}

}  // extern "C"
