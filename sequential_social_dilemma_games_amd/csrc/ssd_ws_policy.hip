// ssd_ws_policy.hip -- the Watershed baselines' policy (LSTMFCNet: two dense layers, a Keras LSTM, a 5-wide distribution head
// and a value head) on the device, one launch per phase: trunk, cell, heads and the action.  include/ssd.h (WATERSHED POLICY
// ROLLOUTS) states the network, the weight layout, the draws and the start rule; DESIGN.md section 14 the shape and the tile.
//
// Watershed is turn-based: each env has ONE acting agent per phase, and each agent id has its own weight set and its own
// recurrent state.  One workgroup = 16 envs and all C cells: 4C threads, one wave per 16 cells.
//   0. per env: the acting agent (-1: nothing to do), the start flag and the draw's (episode, t);
//   1. the observation rows and the actors' h rows to LDS (h of a starting row is zero and never read); the state used
//      also goes to the state ring;
//   then one pass per distinct agent id in the tile (envs reset together stay in lock step, so normally one pass; masked
//   resets mix ids, and a pass keeps its results for the rows of its id only):
//   2. dense0, dense1 on the VALU into the x columns of the [x, h] tile;
//   3. z = [x, h] @ lstm_w on the matrix cores (lstm_gates): a lane ends up with the four gates of its (env, cell);
//   4. the cell update in registers (cell_update, the Keras cell): h' and c' to the actor's row of the state (in place), h' to
//      LDS;
//   5. dist and value on the VALU (head: fmaf chains over the C cells of h');
//   6. rollouts: one thread per env draws the action (policy_pick for the comm agents, the Gaussian rule on policy_key's draws
//      for the action agents) and writes the clipped action where the env's step launch reads it.
// load_h (step 1), lstm_gates, cell_update and head are ssd_policy_device.hpp's, shared with the other policy kernels; the
// constants, the Gaussian's expressions, the comm-agent rule and the argument rules are ssd_ws_policy_device.hpp's, shared with
// the sequence forward (ssd_ws_policy_seq.hip) and the losses (ssd_ws_policy_grad.hip).  Step 2 is that header's ws_dense0 and
// ws_dense1 written out (see there).
// The state may be updated in place: a workgroup reads only rows it owns, and the h rows are in LDS before any is written.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_ws_policy.hpp"
#include "ssd_ws_policy_device.hpp"

namespace {

using namespace ssd::wsp;               // kX, kObs, kOut, kTile, Cell, WsGauss, ws_is_comm and ws_check_net
using ssd::f32x4;
using ssd::misaligned;

constexpr int kM = kTile;               // envs per workgroup

struct WspArgs {
    const float *w;                // num_sets weight sets of set_floats floats each
    int32_t num_sets, B, C, set_floats, variant;
    int32_t NA;                    // agent rows per env of the state: num_sets (rollouts) or 1 (the forward)
    const float *obs;              // [B][12]
    const int8_t *agent;           // [B] the acting agent
    const float *state_in;         // [B][NA][2][C]
    float *state_out;              // [B][NA][2][C], null, or state_in itself
    float *state_used;             // [B][2][C] the state the step used (after the start rule), or null
    const uint8_t *starts;         // [B] start rows (the forward), or null
    const uint8_t *phase;          // [B] the engine's counters (rollouts), or null
    const int32_t *round;
    const uint32_t *episode;
    float *dist;                   // [B][5] or null
    float *value;                  // [B] or null
    float *actions;                // [B] the action as recorded (unclipped), or null: no action selection
    float *clipped;                // [B] the action the env steps with
    int8_t *actor;                 // [B] or null
    float *logp;                   // [B] or null
    uint32_t seed_lo, seed_hi, env_base;
    int32_t greedy;
};

template <int C>
__global__ void __launch_bounds__(4 * C) ssd_ws_policy_kernel(WspArgs a) {
    constexpr int kThreads = 4 * C;     // C / 16 waves; >= 256
    constexpr int kK = kX + C;          // rows of lstm_w: the MFMA's K
    constexpr int kPitch = kK + 52;     // LDS row pitch, = 4 (mod 64)
    static_assert(kThreads >= kM * kX, "tile");
    __shared__ float s_in[kM * kPitch];  // rows [x (16), h (C)]; h' after the gates
    __shared__ float s_obs[kM * kObs];
    __shared__ float s_d0[kM * kX];
    __shared__ float s_out[kM * 8];      // dist 0..4, value at 5
    __shared__ int s_agent[kM], s_start[kM];
    __shared__ uint32_t s_ep[kM], s_t[kM];

    const int tid = threadIdx.x, b0 = blockIdx.x * kM;
    const int B = a.B, NA = a.NA;

    // ---- 0. who acts, and whether its state starts ----
    if (tid < kM) {
        const int b = b0 + tid;
        int ag = -1, st = 1;                                     // (rows past B: zero inputs, nothing read or written)
        uint32_t ep = 0u, t = 0u;
        if (b < B) {
            ag = a.agent[b];
            if (ag < 0 || ag >= a.num_sets) ag = -1;
            if (a.phase) {
                const int ph = a.phase[b], rd = a.round[b];
                if (ph == 0) ag = -1;                            // never reset: left alone
                st = rd == 0 && (a.variant == SSD_WS_SEQ || ph <= 4 || ph >= 9);
                ep = a.episode[b];
                t = (uint32_t)(rd * (a.variant == SSD_WS_SEQ ? 4 : 12) + ph - 1);
            } else {
                st = a.starts ? a.starts[b] != 0 : 0;
            }
        }
        s_agent[tid] = ag; s_start[tid] = ag < 0 ? 1 : st; s_ep[tid] = ep; s_t[tid] = t;   // (nobody acts: nothing read)
    }
    __syncthreads();
    uint32_t present = 0u;                                       // the agent ids of this tile (workgroup-uniform)
#pragma unroll
    for (int m = 0; m < kM; ++m) present |= s_agent[m] >= 0 ? 1u << s_agent[m] : 0u;

    // ---- 1. observations and the actors' h rows ----
    for (int q = tid; q < kM * kObs; q += kThreads) {
        const int m = q / kObs;
        s_obs[q] = s_agent[m] >= 0 ? a.obs[(size_t)(b0 + m) * kObs + (q - m * kObs)] : 0.f;
    }
    ssd::load_h<Cell, C, kM>(
        s_in + kX, kPitch, s_start, a.state_in, a.state_used, tid,
        [=](int m) { return ssd::StateRow{true, ((size_t)(b0 + m) * NA + (NA > 1 ? s_agent[m] : 0)) * 2 * C}; },
        [=](int m) { return ssd::StateRow{b0 + m < B, (size_t)(b0 + m) * 2 * C}; });
    if (tid < kM * 8) s_out[tid] = 0.f;                          // rows nobody acts in report zeros

    while (present) {
        const int g = __ffs(present) - 1;
        present &= present - 1u;
        const float *__restrict__ w = a.w + (size_t)g * (size_t)a.set_floats;
        __syncthreads();                                         // s_obs / the h rows are in; the previous pass is done with s_d0

        // ---- 2. dense0 and dense1: thread (m, j) ----
        const int m2 = tid >> 4, j2 = tid & 15;
        // (ws_dense0 and ws_dense1 written out: called, they give this kernel another register allocation, and the forward
        // measured 4 to 6 % slower -- profiles/r27_ws_shared/)
        if (tid < kM * kX) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < kObs; ++k) s = fmaf(s_obs[m2 * kObs + k], w[SSD_WSP_D0_W + k * kX + j2], s);
            s_d0[tid] = fmaxf(s + w[SSD_WSP_D0_B + j2], 0.f);
        }
        __syncthreads();
        if (tid < kM * kX && s_agent[m2] == g) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < kX; ++k) s = fmaf(s_d0[m2 * kX + k], w[SSD_WSP_D1_W + k * kX + j2], s);
            s_in[m2 * kPitch + j2] = fmaxf(s + w[SSD_WSP_D1_B + j2], 0.f);
        }
        __syncthreads();

        // ---- 3. the gates on the matrix cores, 4. the cell update in registers, for the rows of agent g ----
        f32x4 acc[4][1];
        ssd::lstm_gates<C, kK, kPitch, 1>(s_in, w + SSD_WSP_LSTM_W, tid, acc);
        __syncthreads();                                         // every wave is done with the h rows of s_in
        ssd::cell_update<Cell, C, 1>(acc, w + SSD_WSP_LSTM_B(C), s_start, a.state_in, a.state_out, s_in + kX, kPitch, tid, [=](int m) {
            return ssd::StateRow{s_agent[m] == g, ((size_t)(b0 + m) * NA + (NA > 1 ? g : 0)) * 2 * C};
        });
        __syncthreads();

        // ---- 5. the heads on h': thread (m, j), j < 5 dist, j == 5 the value ----
        if (tid < kM * 8) {
            const int m = tid >> 3, j = tid & 7;
            if (j <= kOut && s_agent[m] == g)
                s_out[m * 8 + j] = ssd::head<C>(s_in + m * kPitch + kX, w + SSD_WSP_OUT_W(C), w + SSD_WSP_VALUE_W(C), w + SSD_WSP_OUT_B(C),
                                                w + SSD_WSP_VALUE_B(C), kOut, j);
        }
    }
    __syncthreads();

    // ---- the outputs of every row of the batch (zeros where nobody acts) ----
    if (tid < kM * 8) {
        const int m = tid >> 3, j = tid & 7, b = b0 + m;
        if (b < B) {
            if (j < kOut) {
                if (a.dist) a.dist[(size_t)b * kOut + j] = s_out[tid];
            } else if (j == kOut && a.value) {
                a.value[b] = s_out[tid];
            }
        }
    }
    if (!a.actions) return;

    // ---- 6. the action ----
    if (tid < kM && b0 + tid < B) {
        const int b = b0 + tid, ag = s_agent[tid];
        const float *l = s_out + tid * 8;
        float act = 0.f, lp = 0.f, clipped = 0.f;
        if (ag >= 0) {
            const uint32_t env = a.env_base + (uint32_t)b;
            if (ws_is_comm(a.variant, ag)) {                     // a comm agent: Categorical over dist[0:5]
                act = (float)ssd::policy_pick(l, kOut, a.greedy, uint4{0u, s_t[tid], s_ep[tid], 0u}, a.seed_lo, a.seed_hi, env,
                                              (uint32_t)ag, &lp);
                clipped = act;
            } else {                                             // an action agent: DiagGaussian(dist[0], dist[1])
                const WsGauss gs(l[0], l[1]);
                float n = 0.f;
                if (!a.greedy) {
                    const uint32_t pk = ssd::policy_key(a.seed_lo, a.seed_hi, env, s_ep[tid], s_t[tid]);
                    const uint32_t d1 = ssd::pol_mix32(pk ^ (uint32_t)ag), d2 = ssd::pol_mix32(pk ^ (uint32_t)(ag + 16));
                    const float u1 = (float)((d1 >> 8) + 1u) * 0x1p-24f, u2 = (float)(d2 >> 8) * 0x1p-24f;
                    n = sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
                }
                act = a.greedy ? gs.mean : gs.mean + gs.sd * n;
                lp = gs.logp(gs.z(act));
                clipped = fminf(fmaxf(act, 0.f), 1.f);
            }
        }
        a.actions[b] = act;
        a.clipped[b] = clipped;
        if (a.actor) a.actor[b] = (int8_t)(ag >= 0 ? ag : 0);
        if (a.logp) a.logp[b] = lp;
    }
}

hipError_t launch(const WspArgs &a, void *stream) {
    const dim3 grid((unsigned)((a.B + kM - 1) / kM)), block(4 * a.C);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (a.C) {
    case 64: hipLaunchKernelGGL((ssd_ws_policy_kernel<64>), grid, block, 0, st, a); break;
    case 128: hipLaunchKernelGGL((ssd_ws_policy_kernel<128>), grid, block, 0, st, a); break;
    case 256: hipLaunchKernelGGL((ssd_ws_policy_kernel<256>), grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

extern "C" {

int ssd_ws_policy_forward(const float *weights, int32_t num_sets, int32_t cell_size, int32_t variant, const float *obs,
                          const int8_t *agent, const float *state_in, const uint8_t *starts, int32_t batch, float *state_out,
                          float *dist, float *value, int32_t device_id, uint32_t flags, void *stream) {
    using ssd::policy_fail;
    if (const char *why = ws_check_net(weights, num_sets, cell_size, variant)) return policy_fail(why);
    if (!obs || !agent || !state_in) return policy_fail("obs, agent and state_in are required");
    if (misaligned(obs, 4) || misaligned(state_in, 4) || misaligned(state_out, 4) || misaligned(dist, 4) || misaligned(value, 4))
        return policy_fail("float buffers must be 4-byte aligned");
    if (batch < 1) return policy_fail("batch must be >= 1");
    if (flags) return policy_fail("flags must be 0");
    if (const char *why = ssd::check_state_out(state_in, state_out, (size_t)batch * 2 * cell_size * sizeof(float))) return policy_fail(why);
    if (const int rc = ssd::policy_use_device(device_id)) return rc;
    WspArgs a{};
    a.w = weights; a.num_sets = num_sets; a.B = batch; a.C = cell_size; a.set_floats = SSD_WSP_SET_FLOATS(cell_size);
    a.variant = variant; a.NA = 1; a.obs = obs; a.agent = agent; a.state_in = state_in; a.state_out = state_out; a.starts = starts;
    a.dist = dist; a.value = value;
    return ssd::policy_launched(launch(a, stream));
}

int ssd_ws_rollout_policy(ssd_ws_env *env, const float *weights, int32_t num_sets, int32_t cell_size, const float *obs_in,
                          const int8_t *agent_in, int32_t n_steps, int32_t step0, float *state, float *state_ring, float *scratch,
                          float *obs, int8_t *agent, double *rew, uint8_t *done, int8_t *actor, float *actions, float *logp,
                          float *value, float *dist, int32_t ring, float *last_value, uint32_t flags, void *stream) {
    if (!env) return SSD_E_INVALID;
    ssd::WsPolicyView v;
    ssd::ws_policy_view(env, &v);
    if (const char *why = ws_check_net(weights, num_sets, cell_size, v.variant)) return ssd::ws_fail_invalid(env, why);
    if (!obs_in || !agent_in || !state || !scratch || !obs || !agent || !actions)
        return ssd::ws_fail_invalid(env, "obs_in, agent_in, state, scratch, obs, agent and actions are required");
    if (n_steps < 1 || step0 < 0 || ring < 1) return ssd::ws_fail_invalid(env, "n_steps >= 1, step0 >= 0 and ring >= 1 are required");
    if ((flags & ~(uint32_t)SSD_POLICY_GREEDY) != 0) return ssd::ws_fail_invalid(env, "unsupported flag");
    if (misaligned(obs_in, 16) || misaligned(obs, 16)) return ssd::ws_fail_invalid(env, "observation rows must be 16-byte aligned");
    if (misaligned(rew, 8)) return ssd::ws_fail_invalid(env, "rew must be 8-byte aligned");
    if (misaligned(state, 4) || misaligned(state_ring, 4) || misaligned(scratch, 4) || misaligned(actions, 4) || misaligned(logp, 4) ||
        misaligned(value, 4) || misaligned(dist, 4) || misaligned(last_value, 4))
        return ssd::ws_fail_invalid(env, "float buffers must be 4-byte aligned");
    hipError_t e = hipSetDevice(v.device);
    if (e != hipSuccess) return ssd::ws_fail_device(env, "hipSetDevice", (int)e);

    const size_t E = (size_t)v.E;
    WspArgs a{};
    a.w = weights; a.num_sets = num_sets; a.B = v.E; a.C = cell_size; a.set_floats = SSD_WSP_SET_FLOATS(cell_size);
    a.variant = v.variant; a.NA = num_sets; a.state_in = state; a.phase = v.phase; a.round = v.round; a.episode = v.episode;
    a.seed_lo = v.seed_lo; a.seed_hi = v.seed_hi; a.env_base = v.env_base; a.greedy = (flags & SSD_POLICY_GREEDY) ? 1 : 0;
    const float *cur_obs = obs_in;
    const int8_t *cur_agent = agent_in;
    for (int k = 0; k < n_steps; ++k) {
        const size_t s = (size_t)((step0 + k) % ring) * E;
        a.obs = cur_obs; a.agent = cur_agent; a.state_out = state;
        a.state_used = state_ring ? state_ring + s * 2 * (size_t)cell_size : nullptr;
        a.dist = dist ? dist + s * kOut : nullptr;
        a.value = value ? value + s : nullptr;
        a.actions = actions + s; a.clipped = scratch;
        a.actor = actor ? actor + s : nullptr;
        a.logp = logp ? logp + s : nullptr;
        e = launch(a, stream);
        if (e != hipSuccess) return ssd::ws_fail_device(env, "policy launch", (int)e);
        const int rc = ssd_ws_step(env, scratch, obs + s * kObs, agent + s, rew ? rew + s : nullptr, done ? done + s : nullptr,
                                   SSD_AUTO_RESET, stream);
        if (rc != SSD_OK) return rc;
        cur_obs = obs + s * kObs;
        cur_agent = agent + s;
    }
    if (last_value) {                                            // the value of the final observation; the state stays
        a.obs = cur_obs; a.agent = cur_agent; a.state_out = nullptr; a.state_used = nullptr; a.dist = nullptr; a.value = last_value;
        a.actions = nullptr; a.clipped = nullptr; a.actor = nullptr; a.logp = nullptr;
        e = launch(a, stream);
        if (e != hipSuccess) return ssd::ws_fail_device(env, "policy launch", (int)e);
    }
    return SSD_OK;
}

}  // extern "C"
