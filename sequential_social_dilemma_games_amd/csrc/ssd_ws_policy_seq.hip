// ssd_ws_policy_seq.hip -- the Watershed baselines' policy (LSTMFCNet, ssd_ws_policy.hip) on the sequences of ONE agent id
// under the current weights, all M own steps and the bootstrap step in one launch: ssd_ws_policy_forward_seq.  include/ssd.h
// (WATERSHED SEQUENCE FORWARD) states the contract; DESIGN.md section 22 the shape, the resources and the measurements.
//
// What an IMPALA learner needs of the target policy (dist, value, the log-probability of the taken action, the bootstrap
// value) used to be M + 1 launches of ssd_ws_policy_forward, each reading and writing the state through memory.  Here a
// workgroup of 4 C threads takes 16 sequences (persistent over tiles g, g + G, ...) and walks the steps itself: it is the
// forward half of ssd_ws_seq_kernel (ssd_ws_policy_grad.hip) without the loss, the scratch stores and the backward.  The 480
// floats of dense0 and dense1 sit in LDS, the gates go through lstm_gates on the matrix cores (for
// C <= 128 with the lane's share of lstm_w held in registers across the steps), h stays in LDS and c in registers across all
// steps of the call; at m % T == 0 the recorded state[m / T] is loaded in their place.
//
// The arithmetic is the rollout kernel's, piece by piece (ws_dense0, ws_dense1 and WsGauss of ssd_ws_policy_device.hpp; lstm_gates,
// Cell::update and head of ssd_policy_device.hpp), so dist, value and the state equal what ssd_ws_policy_forward gives when it
// is chained step by step under the same rule, bit for bit.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_ws_policy_device.hpp"

namespace {

using namespace ssd::wsp;               // kX, kObs, kOut, kTile, kTrunk, kHd, Cell, the dense chains, WsGauss and the argument rules
using ssd::f32x4;
using ssd::misaligned;

struct WsSeqArgs {
    const float *w;                // the agent id's weight set
    int32_t C, Q;
    int32_t G;                     // workgroups
    int32_t M, T;                  // own steps, seq_len
    int32_t comm;                  // the head: Categorical over dist[0:5] (1) or DiagGaussian(dist[0], dist[1]) (0)
    const float *obs;              // [M][Q][12]
    const float *state;            // [ceil(M / T)][Q][2][C]
    const uint8_t *starts;         // [M][Q] or null
    const float *actions;          // [M][Q] or null
    const float *obs_next;         // [Q][12] or null: no bootstrap step
    const uint8_t *start_next;     // [Q] or null
    float *dist;                   // [M][Q][5] or null
    float *value;                  // [M][Q] or null
    float *logp;                   // [M][Q] or null
    float *boot;                   // [Q] or null
    float *state_out;              // [Q][2][C] or null: the state after step M - 1
};

// lstm_gates with B held: the lane's K / 4 x 4 weights of lstm_w are the same at every step, so for C <= 128 they are loaded
// once into registers (wreg[kk][g] = lstm_gates' bv[g] of k-step kk) and a step's gates are LDS loads and MFMAs alone.  Each
// accumulator is the same chain in ascending k as lstm_gates': the same bits.
template <int C, int K, int Pitch>
__device__ __forceinline__ void gates_held(const float *s_in, const float (&wreg)[K / 4][4], int tid, f32x4 (&acc)[4][1]) {
    const int lane = tid & 63;
    const float *a_row = s_in + (lane & 15) * Pitch + (lane >> 4);
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g][0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < K / 4; ++kk) {
        const float av = a_row[4 * kk];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wreg[kk][g], acc[g][0], 0, 0, 0);
    }
}

template <int C>
__global__ void __launch_bounds__(4 * C) ssd_ws_fwd_seq_kernel(WsSeqArgs a) {
    constexpr bool kHeld = C <= 128;           // (C = 256: 272 weights a lane under a bound of 128 registers: they stay in memory)
    constexpr int kThreads = 4 * C, kK = kX + C, kPitch = kK + 52;     // the pitch = 4 (mod 64)
    static_assert(kThreads >= kTile * kX, "tile");
    __shared__ float s_in[kTile * kPitch];     // rows [x (16), h (C)]; h' after the gates
    __shared__ float s_obs[kTile * kObs];
    __shared__ float s_d0[kTile * kX];
    __shared__ float s_wd[kTrunk];             // dense0 and dense1 in the packed layout
    __shared__ float s_out[kTile * kHd];       // dist 0..4 and the value at 5
    __shared__ int s_start[kTile];

    const int tid = threadIdx.x, Q = a.Q, M = a.M, T = a.T;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4, u = 16 * wave + l15;
    const int m2 = tid >> 4, j2 = tid & 15;                          // the dense layers' (row, column), tid < 256
    const float *__restrict__ w = a.w;
    const int last = a.obs_next ? M : M - 1;                         // step M is the bootstrap's

    for (int q = tid; q < kTrunk; q += kThreads) s_wd[q] = w[q];
    float wreg[kHeld ? kK / 4 : 1][4];
    if constexpr (kHeld) {
        const float *wg = w + SSD_WSP_LSTM_W + (size_t)l4 * 4 * C + 16 * wave + l15;
#pragma unroll
        for (int kk = 0; kk < kK / 4; ++kk)
#pragma unroll
            for (int g = 0; g < 4; ++g) wreg[kk][g] = wg[(size_t)kk * 16 * C + g * C];
    }
    const int tiles = Q / kTile + (Q % kTile != 0);
    for (int tile = blockIdx.x; tile < tiles; tile += a.G) {
        const int s0 = tile * kTile;
        const auto live = [=](int m) { return s0 + m < Q; };
        float c_reg[4] = {0.f, 0.f, 0.f, 0.f};                       // c of rows 4 l4 + r, cell u
        int t_in = 0, win = 0;                                       // m = win T + t_in
        for (int m = 0; m <= last; ++m) {
            const bool boot = m == M;
            const bool ring = !boot && t_in == 0;                    // the step uses state[win] as stored
            const float *obs = boot ? a.obs_next : a.obs + (size_t)m * Q * kObs;
            const float *st = a.state + (size_t)win * Q * 2 * C;
            __syncthreads();
            if (tid < kTile) {
                int start = 1;
                if (live(tid)) {
                    if (ring) start = 0;
                    else if (boot) start = a.start_next ? a.start_next[s0 + tid] != 0 : 0;
                    else start = a.starts ? a.starts[(size_t)m * Q + (size_t)(s0 + tid)] != 0 : 0;
                }
                s_start[tid] = start;
            }
            for (int q = tid; q < kTile * kObs; q += kThreads) {
                const int mm = q / kObs;
                s_obs[q] = live(mm) ? obs[(size_t)(s0 + mm) * kObs + (q - mm * kObs)] : 0.f;
            }
            __syncthreads();
            for (int q = tid; q < kTile * C; q += kThreads) {        // h the step uses: the ring's, zero where selected, or h'
                const int mm = q / C, k = q - mm * C;
                if (s_start[mm]) s_in[mm * kPitch + kX + k] = 0.f;
                else if (ring) s_in[mm * kPitch + kX + k] = st[((size_t)(s0 + mm) * 2 + Cell::kRowH) * C + k];
            }
            if (tid < kTile * kX) s_d0[tid] = ws_dense0(s_obs, s_wd, m2, j2);
            __syncthreads();
            if (tid < kTile * kX) s_in[m2 * kPitch + j2] = ws_dense1(s_d0, s_wd, m2, j2);
            __syncthreads();
            f32x4 acc[4][1];
            if constexpr (kHeld) gates_held<C, kK, kPitch>(s_in, wreg, tid, acc);
            else ssd::lstm_gates<C, kK, kPitch, 1>(s_in, w + SSD_WSP_LSTM_W, tid, acc);
            __syncthreads();                                         // every wave is done with the h rows of s_in
            {
                const float *bias = w + SSD_WSP_LSTM_B(C);
                const float b0 = bias[u], b1 = bias[C + u], b2 = bias[2 * C + u], b3 = bias[3 * C + u];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int mm = 4 * l4 + r;
                    if (!live(mm)) continue;
                    float c = c_reg[r];
                    if (s_start[mm]) c = 0.f;
                    else if (ring) c = st[((size_t)(s0 + mm) * 2 + Cell::kRowC) * C + u];
                    float c2, h2;
                    Cell::update(acc[0][0][r] + b0, acc[1][0][r] + b1, acc[2][0][r] + b2, acc[3][0][r] + b3, c, &c2, &h2);
                    s_in[mm * kPitch + kX + u] = h2;
                    c_reg[r] = c2;
                    if (m == M - 1 && a.state_out) {
                        a.state_out[((size_t)(s0 + mm) * 2 + Cell::kRowH) * C + u] = h2;
                        a.state_out[((size_t)(s0 + mm) * 2 + Cell::kRowC) * C + u] = c2;
                    }
                }
            }
            __syncthreads();
            if (tid < kTile * kHd) {                                 // the heads on h'
                const int mm = tid >> 3, j = tid & 7;
                if (j <= kOut) {
                    const float v = ssd::head<C>(s_in + mm * kPitch + kX, w + SSD_WSP_OUT_W(C), w + SSD_WSP_VALUE_W(C),
                                                 w + SSD_WSP_OUT_B(C), w + SSD_WSP_VALUE_B(C), kOut, j);
                    s_out[tid] = v;
                    if (live(mm)) {
                        const size_t row = (size_t)m * Q + (size_t)(s0 + mm);
                        if (boot) {
                            if (j == kOut && a.boot) a.boot[s0 + mm] = v;
                        } else if (j < kOut) {
                            if (a.dist) a.dist[row * kOut + j] = v;
                        } else if (a.value) {
                            a.value[row] = v;
                        }
                    }
                }
            }
            if (a.logp && !boot) {                                   // the taken action under the current dist: the rollout's lines
                __syncthreads();
                if (tid < kTile && live(tid)) {
                    const size_t row = (size_t)m * Q + (size_t)(s0 + tid);
                    const float *l = s_out + tid * kHd;
                    const float act = a.actions[row];
                    float lp;
                    if (a.comm) {
                        int k_act = (int)act;
                        k_act = k_act < 0 ? 0 : (k_act >= kOut ? kOut - 1 : k_act);
                        float mx = l[0];
                        for (int k = 1; k < kOut; ++k)
                            if (l[k] > mx) mx = l[k];
                        float s = 0.f;
                        for (int k = 0; k < kOut; ++k) s += expf(l[k] - mx);
                        lp = l[k_act] - (mx + logf(s));
                    } else {
                        const WsGauss gs(l[0], l[1]);
                        lp = gs.logp(gs.z(act));
                    }
                    a.logp[row] = lp;
                }
            }
            if (++t_in == T) { t_in = 0; ++win; }
        }
    }
}

}  // namespace

extern "C" int ssd_ws_policy_forward_seq(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, int32_t agent_id,
                                         int32_t seq_len, const float *obs, const float *state, const uint8_t *starts,
                                         const float *actions, const float *obs_next, const uint8_t *start_next, int32_t n_steps,
                                         int32_t num_seqs, float *dist, float *value, float *logp, float *bootstrap_value,
                                         float *state_out, int32_t device_id, uint32_t flags, void *stream) {
    using ssd::policy_fail;
    if (const char *why = ws_check_seq_call(weights, num_sets, cell_size, variant, agent_id, seq_len, n_steps, num_seqs, 1))
        return policy_fail(why);
    if (!obs || !state) return policy_fail("obs and state are required");
    if (logp && !actions) return policy_fail("logp needs actions");
    if (bootstrap_value && !obs_next) return policy_fail("bootstrap_value needs obs_next");
    if (misaligned(weights, 4) || misaligned(obs, 4) || misaligned(state, 4) || misaligned(actions, 4) || misaligned(obs_next, 4) ||
        misaligned(dist, 4) || misaligned(value, 4) || misaligned(logp, 4) || misaligned(bootstrap_value, 4) || misaligned(state_out, 4))
        return policy_fail("float buffers must be 4-byte aligned");
    if (flags) return policy_fail("flags must be 0");
    if (const int rc = ssd::policy_use_device(device_id)) return rc;

    WsSeqArgs a{};
    a.w = weights + (size_t)agent_id * SSD_WSP_SET_FLOATS(cell_size);
    a.C = cell_size; a.Q = num_seqs; a.G = SSD_WSPPO_GROUPS(num_seqs); a.M = n_steps; a.T = seq_len;
    a.comm = ws_is_comm(variant, agent_id);
    a.obs = obs; a.state = state; a.starts = starts; a.actions = actions;
    a.obs_next = bootstrap_value ? obs_next : nullptr;               // without its output the bootstrap step is not walked
    a.start_next = start_next;
    a.dist = dist; a.value = value; a.logp = logp; a.boot = bootstrap_value; a.state_out = state_out;
    const dim3 grid((unsigned)a.G), block(4 * cell_size);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (cell_size) {
    case 64: hipLaunchKernelGGL((ssd_ws_fwd_seq_kernel<64>), grid, block, 0, st, a); break;
    case 128: hipLaunchKernelGGL((ssd_ws_fwd_seq_kernel<128>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((ssd_ws_fwd_seq_kernel<256>), grid, block, 0, st, a); break;
    }
    return ssd::policy_launched(hipGetLastError());
}
