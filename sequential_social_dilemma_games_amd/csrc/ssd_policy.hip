// ssd_policy.hip -- the conv-FC policy network of models/conv_to_fc_net.py:1-51 on the device: its forward pass
// (ssd_policy_forward) and, in ssd_rollout_policy (ssd_capi.hip), its action selection, one launch per step between the step
// launches.  include/ssd.h states the network, the weight layout and the sampling contract; DESIGN.md section 11 the shape.
//
// One workgroup = 16 envs of ONE agent index i, so the weight set (i, or 0 when shared) is uniform across it:
//   1. the 16 observations (u8, 10.8 KB) go to LDS, with the 256-entry normalisation table float32((u8 - 128) / 255);
//   2. conv 3x3x3 -> 6 with ReLU on the VALU: a thread per (env, output position) keeps the 6 filters' sums in registers; the
//      weights are uniform (scalar loads).  The 16 x 1014 outputs stay in LDS in the flatten order (row, col, channel);
//   3. fc1 (16 x 1014) x (1014 x 32) on the matrix cores, v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain per
//      accumulator): wave w takes the 16 output columns w & 1 over half of K (w >> 1), two accumulators each; the two halves
//      are added through LDS.  fc1's weights stream from L2 (130 KB per set, shared by every workgroup of the set);
//   4. fc2, the logits and the value on the VALU (1.3 kMAC per env);
//   5. rollouts: one thread per env picks the action (greedy or the S_POLICY draw) and its log-probability.
// Steps 3 and 4 to fc2 are fc_stack below; the heads and the action are ssd_policy_device.hpp's (heads, pick_actions), shared
// with the recurrent kernels.  Every sum is in a fixed order, so two calls on the same input agree bit for bit.  kModeFeatures
// stops after fc2 and writes its output instead: the trunk of the recurrent policy (ssd_policy_lstm.hip).  kModeMoa runs
// fc_stack once per FC stack of the MOA policy, with tanh for ReLU, on the same conv output and writes both outputs
// (ssd_policy_moa.hip).  This file also holds the argument checks every policy entry point shares (check_policy_net,
// check_state_out, select_device; declared in ssd_policy.hpp).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"

namespace {

constexpr int kTile = 16;          // envs per workgroup: M of the fc1 tile
constexpr int kThreads = 256;      // 4 waves
constexpr int kObs = 675;          // 15 * 15 * 3 bytes
constexpr int kPos = 169;          // 13 * 13 conv outputs per filter
constexpr int kFlat = 1014;        // 13 * 13 * 6
constexpr int kPitch = 1017;       // LDS pitch (floats) of a row of conv outputs: 1014 + zero padding, odd against bank conflicts
constexpr int kKSteps = 254;       // fc1: K = 1014 padded to 1016 = 254 MFMA k-steps of 4
constexpr int kHalf = kKSteps / 2; // k-steps per wave (odd: 63 pairs and one more)
constexpr int kHP = 33;            // LDS pitch of the hidden layers

static_assert(kThreads == 256, "one thread per entry of the normalisation table");
static_assert(SSD_POL_FC1_B == SSD_POL_FC1_W + kFlat * 32 && SSD_POL_FC2_W == SSD_POL_FC1_B + 32 && SSD_POL_FC2_B == SSD_POL_FC2_W + 1024 &&
              SSD_POL_VALUE_W == SSD_POL_FC2_B + 32 && SSD_POL_VALUE_B == SSD_POL_VALUE_W + 32 && SSD_POL_LOGITS_W >= SSD_POL_VALUE_B + 1,
              "weight layout of include/ssd.h");

using ssd::f32x4;

constexpr int kModeHeads = 0, kModeFeatures = 1, kModeMoa = 2;

// Steps 3 and 4 up to fc2 on the conv output in s_conv: fc1 on the matrix cores, its two K halves added through LDS, fc2 on the
// VALU; ReLU after both layers, or tanh (the MOA policy's stacks).  ws: a weight set's base, moved so that SSD_POL_FC1_W ..
// SSD_POL_FC2_B address the stack's layers.  fc2's output of tile row m < rows goes to out[m * stride + 0..31].
template <bool kTanh>
__device__ __forceinline__ void fc_stack(const float *__restrict__ ws, const float *s_conv, float *s_part, float *s_h1, int tid,
                                         float *out, size_t stride, int rows) {
    const auto act = [](float x) { return kTanh ? tanhf(x) : fmaxf(x, 0.f); };
    // fc1: A[m][k] = conv row m, B[k][n] = fc1_w[k][n] (the lane layout: ssd_policy_device.hpp)
    const int wave = tid >> 6, lane = tid & 63, nt = wave & 1, kh = wave >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const float *a_row = s_conv + l15 * kPitch + l4;
    const float *w1 = ws + SSD_POL_FC1_W + l4 * 32 + nt * 16 + l15;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    // (wave half 0: k-steps 0..126; half 1: 127..253, whose last step is peeled -- its rows 1014, 1015 are padding)
    const int kb = kh * kHalf;
#pragma unroll 4
    for (int p = 0; p < (kHalf - 1) / 2; ++p) {
        const int kk = kb + 2 * p;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk], w1[(size_t)kk * 128], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kk + 4], w1[(size_t)kk * 128 + 128], acc1, 0, 0, 0);
    }
    {
        const int kl = kb + kHalf - 1;
        const float bv = 4 * kl + l4 < kFlat ? w1[(size_t)kl * 128] : 0.f;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[4 * kl], bv, acc0, 0, 0, 0);
    }
    const f32x4 acc = acc0 + acc1;
    if (kh) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s_part[(nt * 16 + l4 * 4 + r) * 16 + l15] = acc[r];
    }
    __syncthreads();
    if (!kh) {
        const int n = nt * 16 + l15;
        const float bias = ws[SSD_POL_FC1_B + n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = l4 * 4 + r;
            s_h1[m * kHP + n] = act(acc[r] + s_part[(nt * 16 + m) * 16 + l15] + bias);
        }
    }
    __syncthreads();
    // fc2: thread (m, n) takes columns n and n + 16 of row m
    const int m = tid >> 4, n = tid & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int nn = n + 16 * h;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) s = fmaf(s_h1[m * kHP + k], ws[SSD_POL_FC2_W + k * 32 + nn], s);
        if (m < rows) out[m * stride + nn] = act(s + ws[SSD_POL_FC2_B + nn]);
    }
}

// kModeFeatures: stop after fc2 and write its output to a.feat (the trunk of the recurrent policy, ssd_policy_lstm.hip).
// kModeMoa: both FC stacks of the MOA policy after the conv (stack s's weights at SSD_MOA_FC1_W(s), the trunk's relative
// offsets), to a.feat [B][N][2][32].
template <int kMode>
__global__ void __launch_bounds__(kThreads) ssd_policy_kernel(ssd::PolicyArgs a) {
    __shared__ float s_norm[256];
    __shared__ float s_conv[kTile * kPitch];
    __shared__ float s_buf[(kTile * kObs + 3) / 4];   // the observation bytes; after the conv, the small buffers below
    uint8_t *s_obs = reinterpret_cast<uint8_t *>(s_buf);
    float *s_part = s_buf;                             // [2][16][16] fc1 partial sums of the second K half
    float *s_h1 = s_buf + 512;                         // [16][kHP]
    float *s_h2 = s_h1 + kTile * kHP;                  // [16][kHP]
    float *s_out = s_h2 + kTile * kHP;                 // [16][16]: logits 0..A-1, value at A
    static_assert(512 + 2 * kTile * kHP + kTile * 16 <= (kTile * kObs + 3) / 4, "small buffers fit the observation area");

    const int tid = threadIdx.x, i = blockIdx.y, b0 = blockIdx.x * kTile;
    const int N = a.N, B = a.B;
    const float *__restrict__ w = a.w + (size_t)(a.P == 1 ? 0 : i) * (size_t)a.set_floats;

    // ---- 1. inputs ----
    s_norm[tid] = (float)(((double)tid - 128.0) / 255.0);
    {   // (every load of the thread issued before the first store: one round trip to memory, not 43)
        constexpr int kLoads = (kTile * kObs + kThreads - 1) / kThreads;
        uint8_t v[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int q = tid + u * kThreads, r = q / kObs, o = q - r * kObs, b = b0 + r;
            v[u] = q < kTile * kObs && b < B ? a.obs[((size_t)b * N + i) * kObs + o] : (uint8_t)128;
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u)
            if (tid + u * kThreads < kTile * kObs) s_obs[tid + u * kThreads] = v[u];
    }
    if (tid < kTile * (kPitch - kFlat)) s_conv[(tid / 3) * kPitch + kFlat + tid % 3] = 0.f;
    __syncthreads();

    // ---- 2. conv 3x3, 6 filters, ReLU; output (row, col, channel) ----
    for (int q = tid; q < kTile * kPos; q += kThreads) {
        const int r = q / kPos, pos = q - r * kPos, y = pos / 13, x = pos - y * 13;
        const uint8_t *src = s_obs + r * kObs + (y * 15 + x) * 3;
        float acc[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) acc[f] = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int j = 0; j < 9; ++j) {                   // (dx, c) = (j / 3, j % 3): 9 contiguous bytes of view row y + dy
                const float v = s_norm[src[dy * 45 + j]];
#pragma unroll
                for (int f = 0; f < 6; ++f) acc[f] = fmaf(v, w[SSD_POL_CONV_W + (dy * 9 + j) * 6 + f], acc[f]);
            }
        }
        float *dst = s_conv + r * kPitch + pos * 6;
#pragma unroll
        for (int f = 0; f < 6; ++f) dst[f] = fmaxf(acc[f] + w[SSD_POL_CONV_B + f], 0.f);
    }
    __syncthreads();

    // ---- 3, 4. fc1, fc2 (fc_stack) ----
    const size_t row0 = (size_t)b0 * N + i;                 // the tile's first row of a [B][N] array; its rows are N apart
    if constexpr (kMode == kModeMoa) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            fc_stack<true>(w + (SSD_MOA_FC1_W(s) - SSD_POL_FC1_W), s_conv, s_part, s_h1, tid, a.feat + (row0 * 2 + s) * 32,
                           (size_t)N * 64, B - b0);
            __syncthreads();                                // s_part and s_h1 are the next stack's
        }
    } else if constexpr (kMode == kModeFeatures) {
        fc_stack<false>(w, s_conv, s_part, s_h1, tid, a.feat + row0 * 32, (size_t)N * 32, B - b0);
    } else {
        fc_stack<false>(w, s_conv, s_part, s_h1, tid, s_h2, kHP, kTile);
        __syncthreads();
        // ---- 4. the heads, 5. the action: argmax, or the first a with u < cumulative softmax (include/ssd.h) ----
        ssd::heads<32, kTile, kThreads>(a, s_h2, kHP, w + SSD_POL_LOGITS_W, w + SSD_POL_VALUE_W, w + SSD_POL_LOGITS_W + 32 * a.A,
                                        w + SSD_POL_VALUE_B, s_out, nullptr, tid, b0, i);
        if (!a.actions) return;
        __syncthreads();
        ssd::pick_actions<kTile>(a, s_out, nullptr, tid, b0, i);
    }
}

thread_local std::string g_policy_error;

int fail(const char *msg) {
    g_policy_error = msg;
    return SSD_E_INVALID;
}

}  // namespace

namespace ssd {

hipError_t launch_policy(const PolicyArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.N), block(kThreads);
    hipLaunchKernelGGL(ssd_policy_kernel<kModeHeads>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

hipError_t launch_policy_features(const PolicyArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.N), block(kThreads);
    hipLaunchKernelGGL(ssd_policy_kernel<kModeFeatures>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

hipError_t launch_policy_moa_features(const PolicyArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.N), block(kThreads);
    hipLaunchKernelGGL(ssd_policy_kernel<kModeMoa>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

int policy_fail(const char *msg) { return fail(msg); }

const char *check_policy_net(PolicyNet net, const float *weights, int32_t num_sets, int32_t num_agents, int32_t num_actions,
                             int32_t cell_size, const float *moa_scratch) {
    if (reinterpret_cast<uintptr_t>(weights) & 3u) return "weights must be 4-byte aligned";
    if (net == kNetMoa && (reinterpret_cast<uintptr_t>(moa_scratch) & 3u)) return "scratch must be 4-byte aligned";
    if (net != kNetConvFc && cell_size != 64 && cell_size != 128 && cell_size != 256) return "cell_size must be 64, 128 or 256";
    if (net == kNetMoa) {
        if (num_agents < 2 || num_agents > SSD_MOA_MAX_AGENTS) return "the MOA policy needs 2..16 agents";
    } else if (num_agents < 1 || num_agents > 64) {
        return "num_agents must be 1..64";
    }
    if (num_sets != 1 && num_sets != num_agents) return "num_sets must be 1 or num_agents";
    if (num_actions < 1 || num_actions > SSD_POL_MAX_ACTIONS) return "num_actions must be 1..15";
    return nullptr;
}

const char *check_state_out(const float *state_in, const float *state_out, size_t bytes) {
    if (!state_out || state_out == state_in) return nullptr;
    const char *p = reinterpret_cast<const char *>(state_in), *q = reinterpret_cast<const char *>(state_out);
    return q < p + bytes && p < q + bytes ? "state_out must be state_in or not overlap it" : nullptr;
}

hipError_t select_device(int device_id) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device_id) return hipSuccess;
    return hipSetDevice(device_id);
}

int policy_use_device(int device_id) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return fail("no such HIP device");
    if (select_device(device_id) != hipSuccess) { g_policy_error = "hipSetDevice failed"; return SSD_E_DEVICE; }
    return SSD_OK;
}

int policy_launched(hipError_t e) {
    if (e == hipSuccess) return SSD_OK;
    g_policy_error = std::string("policy launch: ") + hipGetErrorString(e);
    return SSD_E_DEVICE;
}

}  // namespace ssd

extern "C" {

const char *ssd_policy_last_error(void) { return g_policy_error.c_str(); }

int ssd_policy_forward(const float *weights, int32_t num_sets, int32_t num_actions, const uint8_t *obs, int32_t batch,
                       int32_t num_agents, float *logits, float *value, int32_t device_id, uint32_t flags, void *stream) {
    if (!weights || !obs) return fail("weights and obs are required");
    if (const char *why = ssd::check_policy_net(ssd::kNetConvFc, weights, num_sets, num_agents, num_actions)) return fail(why);
    if (batch < 1) return fail("batch must be >= 1");
    if (flags) return fail("flags must be 0");
    if (const int rc = ssd::policy_use_device(device_id)) return rc;
    ssd::PolicyArgs a{};
    a.w = weights; a.P = num_sets; a.A = num_actions; a.B = batch; a.N = num_agents; a.set_floats = SSD_POL_SET_FLOATS(num_actions);
    a.obs = obs; a.logits = logits; a.value = value;
    return ssd::policy_launched(ssd::launch_policy(a, stream));
}

}  // extern "C"
