// csrc/ssd_policy_trunk.hpp -- ssd_policy_kernel, the conv-FC network's kernel with its modes, as a template that each object
// instantiates for the modes it launches: ssd_policy.hip the three that the forwards and the rollouts use (kModeHeads,
// kModeFeatures, kModeMoa), ssd_policy_seq.hip kModeMoaActions.  One object per set of modes, because instantiations of one
// template that are compiled together change each other's instruction schedule: kModeMoaActions next to kModeMoa moved
// kModeMoa's loads (same registers, another order).  ssd_policy.hip describes the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_policy_device.hpp"

namespace {

using namespace ssd::trunk;      // the tile constants, conv_tile and fc_stack (ssd_policy_device.hpp)

constexpr int kModeHeads = 0, kModeFeatures = 1, kModeMoa = 2, kModeMoaActions = 3;

// kModeFeatures: stop after fc2 and write its output to a.feat (the trunk of the recurrent policy, ssd_policy_lstm.hip).
// kModeMoa: both FC stacks of the MOA policy after the conv (stack s's weights at SSD_MOA_FC1_W(s), the trunk's relative
// offsets), to a.feat [B][N][2][32].
// kModeMoaActions: FC stack 0 of the MOA policy alone (the actions branch's), to a.feat [B][N][32].
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
    conv_tile(w, s_obs, s_norm, s_conv, tid);
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
    } else if constexpr (kMode == kModeMoaActions) {
        fc_stack<true>(w + (SSD_MOA_FC1_W(0) - SSD_POL_FC1_W), s_conv, s_part, s_h1, tid, a.feat + row0 * 32, (size_t)N * 32, B - b0);
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

// hipLaunchKernel of the kernel in mode kMode on `stream`: 16 envs of one agent index per workgroup.
template <int kMode>
hipError_t launch_policy_mode(const ssd::PolicyArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kTile - 1) / kTile), (unsigned)a.N), block(kThreads);
    hipLaunchKernelGGL(ssd_policy_kernel<kMode>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

}  // namespace
