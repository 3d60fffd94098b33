// ssd_watershed.hip -- the Watershed games (include/ssd.h, ssd_ws_*): WatershedSeqEnv / WatershedSeqCommEnv of
// watershedOrderedComm.py:284-637 for E envs, one lane per env.
//
// State is SoA in HBM ([slot][E] for the per-env arrays, so that a wave's loads and stores are contiguous).  The step
// kernel loads an env's state, runs one phase and stores it back; the rollout kernel keeps it in registers for n_steps
// phases and streams only actions in and observations / rewards / dones out.  Every float operation is the reference's,
// in its order, in float32 (NumPy's NEP 50 rules: the Python int / float operands are weak scalars) -- except the
// episode sums and the end-of-episode rewards, which NumPy promotes to float64 -- and the build keeps -ffp-contract=off so
// that no multiply-add is fused.  The square of the reward is libm's powf(x, 2) (ssd_ws_square.hpp), not x*x.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/ssd.h"
#include "ssd_ws_policy.hpp"
#include "ssd_ws_square.hpp"
#include "ssd_ws_stats.hpp"

namespace {

constexpr int kMaxSteps = 10;                                    // max_steps (:289)
constexpr int kBlock = 256;
constexpr int kAhead = 4;                                        // rollout: phases by which an action load leads its use

struct WsDev {                                                   // device arrays of one handle
    uint8_t *season, *phase, *wrapped, *viol;                    // viol: 6 bits
    int32_t *round;
    uint32_t *episode;
    float *hist;                                                 // [8][E]
    float *fr;                                                   // [6][E]
    float *pen;
    double *csum, *run;                                          // [4][E]
    float *prev;                                                 // [4][E]
    uint32_t *status;
};

struct WsParams {
    WsDev d;
    int32_t E, variant, local_obs, local_rew;
    uint32_t seed_lo, seed_hi, env_base;
};

struct Lane {
    uint32_t season, phase, wrapped, viol, episode;
    int32_t round;
    float hist[8], fr[6], pen;
    double csum[4], run[4];
    float prev[4];
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {          // prng.py mix32 (triple32)
    x ^= x >> 17; x *= 0xED5AD4BBu; x ^= x >> 11; x *= 0xAC4C1B51u; x ^= x >> 15; x *= 0x31848BABu; x ^= x >> 14;
    return x;
}

__device__ __forceinline__ uint32_t season_draw(const WsParams &p, uint32_t env, uint32_t episode) {
    uint32_t h = 0x243F6A88u;
    h = mix32(h ^ p.seed_lo); h = mix32(h ^ p.seed_hi); h = mix32(h ^ env); h = mix32(h ^ episode);
    const uint32_t pk = mix32(mix32(h ^ 0u) ^ (uint32_t)SSD_S_SEASON);
    return (uint32_t)(((uint64_t)mix32(pk ^ 0u) * 108u) >> 32);
}

// set_new_season (:67-76): Q1, Q2, S by season % 3; al = all_al[season / 3], the product of :16 in itertools order
__device__ __forceinline__ int q1_of(uint32_t s) { const uint32_t m = s % 3; return m == 0 ? 160 : m == 1 ? 115 : 80; }
__device__ __forceinline__ int q2_of(uint32_t s) { const uint32_t m = s % 3; return m == 0 ? 65 : m == 1 ? 50 : 35; }
__device__ __forceinline__ int s_of(uint32_t s) { const uint32_t m = s % 3; return m == 0 ? 15 : m == 1 ? 12 : 10; }
__device__ __forceinline__ int al_of(uint32_t s, int j) {       // al[j], j = 0..6
    const uint32_t sa = s / 3;                                   // ((i1 * 3 + i2) * 2 + i4) * 3 + i6
    switch (j) {
        case 1: return 8 + 8 * (int)(sa / 18);
        case 2: return 8 + 8 * (int)((sa / 6) % 3);
        case 3: return 8;
        case 4: return 8 + 8 * (int)((sa / 3) % 2);
        case 5: return 15;
        case 6: return 8 + 8 * (int)(sa % 3);
        default: return 0;
    }
}

// agent_in_phases[q]
__device__ __forceinline__ int agent_at(int variant, uint32_t q) {
    return variant == SSD_WS_SEQ ? (int)q : (q < 4 ? (int)q : (int)q - 4);
}

__device__ __forceinline__ void load(const WsParams &p, int e, Lane &s) {
    const WsDev &d = p.d;
    const int E = p.E;
    s.season = d.season[e]; s.phase = d.phase[e]; s.wrapped = d.wrapped[e]; s.viol = d.viol[e];
    s.round = d.round[e]; s.episode = d.episode[e];
    const int nh = p.variant == SSD_WS_SEQ ? 4 : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) s.hist[j] = j < nh ? d.hist[(size_t)j * E + e] : 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) s.fr[j] = d.fr[(size_t)j * E + e];
    s.pen = d.pen[e];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.csum[j] = d.csum[(size_t)j * E + e];
        s.run[j] = d.run[(size_t)j * E + e];
        s.prev[j] = d.prev[(size_t)j * E + e];
    }
}

__device__ __forceinline__ void store(const WsParams &p, int e, const Lane &s) {
    const WsDev &d = p.d;
    const int E = p.E;
    d.season[e] = (uint8_t)s.season; d.phase[e] = (uint8_t)s.phase; d.wrapped[e] = (uint8_t)s.wrapped; d.viol[e] = (uint8_t)s.viol;
    d.round[e] = s.round; d.episode[e] = s.episode;
    const int nh = p.variant == SSD_WS_SEQ ? 4 : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < nh) d.hist[(size_t)j * E + e] = s.hist[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) d.fr[(size_t)j * E + e] = s.fr[j];
    d.pen[e] = s.pen;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d.csum[(size_t)j * E + e] = s.csum[j];
        d.run[(size_t)j * E + e] = s.run[j];
        d.prev[(size_t)j * E + e] = s.prev[j];
    }
}

// incoming_flows[k] (get_personal_state, :87-101 / :456-473) from the current action history; b = slot of action agent 0
__device__ __forceinline__ float flow(const Lane &s, int b, int k) {
    const float q1 = (float)q1_of(s.season), q2 = (float)q2_of(s.season), S = (float)s_of(s.season);
    const float f1 = q1 * (1.0f - s.hist[b + 0]);
    if (k == 0) return q1;
    if (k == 1) return f1;
    if (k == 2) return q2;
    return q2 * (1.0f - s.hist[b + 2]) + (f1 + S) * s.hist[b + 1];
}

__device__ __forceinline__ void reset_lane(const WsParams &p, int e, Lane &s) {
    s.episode += 1u;
    s.season = season_draw(p, p.env_base + (uint32_t)e, s.episode);
    s.phase = 1; s.round = 0; s.wrapped = 0; s.viol = 0; s.pen = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s.hist[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) s.fr[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.csum[j] = 0.0; s.run[j] = 0.0; s.prev[j] = 0.0f; }
}

// cal_rewards + cal_violations (:194-218, :141-180) and the bookkeeping of the round's close (:352-369 / :542-564)
__device__ __forceinline__ void close_round(Lane &s, int b) {
    const float q1 = (float)q1_of(s.season), q2 = (float)q2_of(s.season), S = (float)s_of(s.season);
    const float a0 = s.hist[b], a1 = s.hist[b + 1], a2 = s.hist[b + 2], a3 = s.hist[b + 3];
    const float f1 = q1 * (1.0f - a0);
    const float f3 = q2 * (1.0f - a2) + (f1 + S) * a1;
    float x[6];
    x[0] = q1 * a0;
    x[1] = (f1 + S) * a1;
    x[3] = q2 * a2;
    x[5] = f3 * a3;
    x[2] = q2 - x[3];
    x[4] = (x[1] + x[2]) - x[5];
    const float A[6] = {-0.2f, -0.06f, -0.29f, -0.13f, -0.056f, -0.15f};
    const float B[6] = {6.0f, 2.5f, 6.28f, 6.0f, 3.74f, 7.6f};
    const float C[6] = {-5.0f, 0.0f, -3.0f, -6.0f, -23.0f, -15.0f};
#pragma unroll
    for (int j = 0; j < 6; ++j) s.fr[j] = (A[j] * ws::powf2(x[j]) + B[j] * x[j]) + C[j];
    const float v[6] = {(float)al_of(s.season, 1) - x[0], (float)al_of(s.season, 2) - f1, (float)al_of(s.season, 3) - x[2],
                        (float)al_of(s.season, 4) - x[3], (float)al_of(s.season, 5) - x[4], (float)al_of(s.season, 6) - x[5]};
    float pen = 0.0f;
    uint32_t viol = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if (v[j] > 0.0f) { viol |= 1u << j; pen = pen + (v[j] + 1.0f) * 100.0f; }
    s.pen = pen;
    s.viol = viol;
    s.prev[0] = a0; s.prev[1] = a1; s.prev[2] = a2; s.prev[3] = a3;
    s.csum[0] = s.csum[0] + (double)x[0];
    s.csum[1] = s.csum[1] + (double)x[1];
    s.csum[2] = s.csum[2] + (double)x[3];
    s.csum[3] = s.csum[3] + (double)x[5];
    s.round += 1;
    s.wrapped = 1;
}

__device__ __forceinline__ double temp_of(const Lane &s, int j) {
    const double req = j == 0 ? 240.0 : j == 1 ? 400.0 : j == 2 ? 240.0 : 100.0;    // mybigreq (:290)
    return s.csum[j] / req * 100.0;
}

template <typename T>
__device__ __forceinline__ T pick4(const T a[4], int k) { return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3]; }

// the observation row of agent_in_phases[q] (V, LO, LR: variant, local_obs, local_rew -- the kernels are instantiated per handle kind,
// so that every register-array index below is a constant)
template <int V, int LO>
__device__ __forceinline__ int observe(const Lane &s, uint32_t q, float o[SSD_WS_OBS_WIDTH]) {
    const int agent = agent_at(V, q), k = agent & 3;
#pragma unroll
    for (int j = 0; j < SSD_WS_OBS_WIDTH; ++j) o[j] = 0.0f;
    o[0] = (float)q1_of(s.season); o[1] = (float)q2_of(s.season); o[2] = (float)s_of(s.season);
    constexpr int c = LO ? 4 : 7;
    if (LO) {
        o[3] = (float)al_of(s.season, k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 4 : 6);      // agentID2real
    } else {
        o[3] = (float)al_of(s.season, 1); o[4] = (float)al_of(s.season, 2); o[5] = (float)al_of(s.season, 3);
        o[6] = (float)al_of(s.season, 4);
    }
    if (V == SSD_WS_SEQ) {
        o[c] = flow(s, 0, k);
    } else {
        float cm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cm[j] = q < 4 ? -1.0f : s.hist[j];               // -1s in the first comm round
        const bool act = agent >= 4;                             // action agents: flow, then the comm actions
        o[c] = act ? flow(s, 4, k) : cm[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[c + 1 + j] = act ? cm[j] : (j < 3 ? cm[j + 1] : 0.0f);
    }
    return agent;
}

struct StepOut {
    float obs[SSD_WS_OBS_WIDTH];
    double rew;
    uint32_t done;
    int agent;
};

// One phase of step() (:336-422 / :522-637) on a reset env
template <int V, int LO, int LR>
__device__ __forceinline__ void step_lane(const WsParams &p, int e, Lane &s, float action, bool auto_reset, StepOut &out,
                                          uint32_t &status) {
    constexpr uint32_t P = V == SSD_WS_SEQ ? 4u : 12u;
    constexpr int b = V == SSD_WS_SEQ ? 0 : 4;
    uint32_t ph = s.phase;
    const int slot = agent_at(V, ph - 1);                        // the acting agent
    if (V == SSD_WS_SEQ_COMM && slot < 4 && !(action >= 0.0f && action <= 4.0f && action == floorf(action)))
        status |= SSD_ST_BAD_ACTION;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j == slot) s.hist[j] = action;
    if (ph == P) { close_round(s, b); ph = 0; }
    const bool end = s.round >= kMaxSteps;
    const bool done_all = end && ph == P - 1;
    const int agent = observe<V, LO>(s, ph, out.obs);
    const int k = agent & 3;
    float fsum = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) fsum = fsum + s.fr[j];
    const float r32 = (LR ? pick4(s.fr, k) : fsum) - s.pen;
    double tsum = 0.0, temp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { temp[j] = temp_of(s, j); tsum = tsum + temp[j]; }
    const double r64 = (double)r32 + (LR ? pick4(temp, k) : tsum);
    bool is_int = !s.wrapped;
    bool dagent = end, gets = true;
    if (V == SSD_WS_SEQ_COMM && agent < 4) {
        is_int = is_int || ph >= 4;                              // firstCommStep is False from the second comm round on
        dagent = end && ph >= 4;                                 // ... and lastCommStep True
        gets = false;                                            // comm agents do not add to rew_sum_keeper
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (gets && !is_int && j == k) s.run[j] = end ? s.run[j] + r64 : (double)((float)s.run[j] + r32);
    out.rew = is_int ? 0.0 : end ? r64 : (double)r32;
    out.done = (dagent ? SSD_WS_DONE_AGENT : 0u) | (done_all ? SSD_WS_DONE_ALL : 0u) | (end ? SSD_WS_END : 0u) |
               (is_int ? SSD_WS_REW_INT : end ? SSD_WS_REW_F64 : 0u);
    out.agent = agent;
    s.phase = ph + 1;
    if (done_all && auto_reset) {
        reset_lane(p, e, s);
        out.agent = observe<V, LO>(s, 0, out.obs);
    }
}

__device__ __forceinline__ void write_out(int e, const StepOut &o, float *obs, int8_t *agent, double *rew, uint8_t *done) {
    if (obs) {
        float4 *row = reinterpret_cast<float4 *>(obs + (size_t)e * SSD_WS_OBS_WIDTH);
        row[0] = make_float4(o.obs[0], o.obs[1], o.obs[2], o.obs[3]);
        row[1] = make_float4(o.obs[4], o.obs[5], o.obs[6], o.obs[7]);
        row[2] = make_float4(o.obs[8], o.obs[9], o.obs[10], o.obs[11]);
    }
    if (agent) agent[e] = (int8_t)o.agent;
    if (rew) rew[e] = o.rew;
    if (done) done[e] = (uint8_t)o.done;
}

template <int V, int LO>
__global__ void __launch_bounds__(kBlock) ws_reset_kernel(WsParams p, const uint8_t *mask, float *obs, int8_t *agent) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E || (mask && !mask[e])) return;
    Lane s;
    load(p, e, s);
    reset_lane(p, e, s);
    store(p, e, s);
    StepOut o;
    o.agent = observe<V, LO>(s, 0, o.obs);
    write_out(e, o, obs, agent, nullptr, nullptr);
}

template <int V, int LO, int LR>
__global__ void __launch_bounds__(kBlock) ws_rollout_kernel(WsParams p, const float *actions, int action_ring, int n_steps, int step0,
                                                            float *obs, int8_t *agent, double *rew, uint8_t *done, int ring,
                                                            int auto_reset) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E) return;
    const size_t E = (size_t)p.E;
    Lane s;
    load(p, e, s);
    uint32_t status = 0;
    if (s.phase == 0) {                                          // never reset: left alone, zero outputs
        status |= SSD_ST_NOT_RESET;
        StepOut z = {};
        for (int k = 0; k < n_steps; ++k) {
            const size_t os = (size_t)((step0 + k) % ring) * E;
            write_out(e, z, obs ? obs + os * SSD_WS_OBS_WIDTH : nullptr, agent ? agent + os : nullptr, rew ? rew + os : nullptr,
                      done ? done + os : nullptr);
        }
    } else {
        // the actions are fetched kAhead phases ahead (a window rotated through registers): a phase is a few dozen
        // instructions, so with a one-phase lead every phase of a lane would wait for one memory round trip
        float win[kAhead];
#pragma unroll
        for (int i = 0; i < kAhead; ++i) win[i] = i < n_steps ? actions[(size_t)((step0 + i) % action_ring) * E + e] : 0.0f;
        for (int k = 0; k < n_steps; ++k) {
            const float a = win[0];
#pragma unroll
            for (int i = 0; i + 1 < kAhead; ++i) win[i] = win[i + 1];
            win[kAhead - 1] = k + kAhead < n_steps ? actions[(size_t)((step0 + k + kAhead) % action_ring) * E + e] : 0.0f;
            StepOut o;
            step_lane<V, LO, LR>(p, e, s, a, auto_reset != 0, o, status);
            const size_t os = (size_t)((step0 + k) % ring) * E;
            write_out(e, o, obs ? obs + os * SSD_WS_OBS_WIDTH : nullptr, agent ? agent + os : nullptr, rew ? rew + os : nullptr,
                      done ? done + os : nullptr);
        }
        store(p, e, s);
    }
    if (status) atomicOr(p.d.status, status);
}

// ws_rollout_kernel with an attached statistics handle (ssd_ws_stats.hpp): the lane's open episode is
// loaded from the handle, folded in registers step by step, finalised into the handle's accumulators where a step sets
// SSD_WS_DONE_ALL, and stored back.  A kernel of its own, not a branch of the one above: the instances above are launched exactly
// when no handle is attached and stay, instruction for instruction, what they were before the statistics existed.
template <int V, int LO, int LR>
__global__ void __launch_bounds__(kBlock) ws_rollout_stats_kernel(WsParams p, ssd::WsStatsDev sd, const float *actions, int action_ring,
                                                                  int n_steps, int step0, float *obs, int8_t *agent, double *rew,
                                                                  uint8_t *done, int ring, int auto_reset) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E) return;
    const size_t E = (size_t)p.E;
    Lane s;
    load(p, e, s);
    uint32_t status = 0;
    if (s.phase == 0) {                                          // never reset: left alone, zero outputs, no statistics
        status |= SSD_ST_NOT_RESET;
        StepOut z = {};
        for (int k = 0; k < n_steps; ++k) {
            const size_t os = (size_t)((step0 + k) % ring) * E;
            write_out(e, z, obs ? obs + os * SSD_WS_OBS_WIDTH : nullptr, agent ? agent + os : nullptr, rew ? rew + os : nullptr,
                      done ? done + os : nullptr);
        }
    } else {
        ssd::WsOpenEpisode<V == SSD_WS_SEQ ? 4 : 8> ep;
        ep.load(sd, e);
        float win[kAhead];                                       // as above
#pragma unroll
        for (int i = 0; i < kAhead; ++i) win[i] = i < n_steps ? actions[(size_t)((step0 + i) % action_ring) * E + e] : 0.0f;
        for (int k = 0; k < n_steps; ++k) {
            const float a = win[0];
#pragma unroll
            for (int i = 0; i + 1 < kAhead; ++i) win[i] = win[i + 1];
            win[kAhead - 1] = k + kAhead < n_steps ? actions[(size_t)((step0 + k + kAhead) % action_ring) * E + e] : 0.0f;
            StepOut o;
            // the phase without its auto-reset, so that viol and running_rew are still the finished episode's
            step_lane<V, LO, LR>(p, e, s, a, false, o, status);
            if (ep.open) ep.step(o.rew, o.agent, s.viol);
            if (o.done & SSD_WS_DONE_ALL) {
                if (ep.open) ep.finish(sd, e, s.run);
                ep.clear();
                ep.open = auto_reset != 0;                       // closed until the env's next reset
                if (auto_reset) {                                // what step_lane does itself when it is told to
                    reset_lane(p, e, s);
                    o.agent = observe<V, LO>(s, 0, o.obs);
                }
            }
            const size_t os = (size_t)((step0 + k) % ring) * E;
            write_out(e, o, obs ? obs + os * SSD_WS_OBS_WIDTH : nullptr, agent ? agent + os : nullptr, rew ? rew + os : nullptr,
                      done ? done + os : nullptr);
        }
        store(p, e, s);
        ep.store(sd, e);
    }
    if (status) atomicOr(p.d.status, status);
}

__global__ void __launch_bounds__(kBlock) ws_info_kernel(WsParams p, uint8_t *viol, uint8_t *true_end, double *running, double *temp,
                                                         int64_t *other) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E) return;
    Lane s;
    load(p, e, s);
    const uint32_t P = p.variant == SSD_WS_SEQ ? 4u : 12u;
    const bool end = s.round >= kMaxSteps;
    if (viol)
        for (int j = 0; j < 6; ++j) viol[(size_t)e * 6 + j] = (s.viol >> j) & 1u;
    if (true_end) true_end[e] = end && s.phase == P;
    if (running)
        for (int j = 0; j < 4; ++j) running[(size_t)e * 4 + j] = s.run[j];
    if (temp) {
        double t = 0.0;
        for (int j = 0; j < 4; ++j) t = t + temp_of(s, j);
        temp[e] = end ? t : 0.0;
    }
    if (other) {
        const int k = agent_at(p.variant, s.phase > 0 ? s.phase - 1 : 0) & 3;
        for (int j = 0; j < 3; ++j) other[(size_t)e * 3 + j] = (int64_t)s.prev[j + (j >= k ? 1 : 0)];
    }
}

std::string g_ws_create_error;

}  // namespace

struct ssd_ws_env {
    WsParams p;
    int device;
    ssd_ws_stats *stats;                                         // attached episode statistics, or null
    void *block;                                                 // the one device allocation behind p.d
    std::string err;
};

namespace {

int ws_fail(ssd_ws_env *env, const char *what, hipError_t e) {
    env->err = std::string(what) + ": " + hipGetErrorString(e);
    return SSD_E_DEVICE;
}

#define WS_HIP(env, call)                                                  \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) return ws_fail((env), #call, e_);            \
    } while (0)

int grid(const ssd_ws_env *env) { return (env->p.E + kBlock - 1) / kBlock; }

// the fields of the state in host order (row-major [E,n]) and device order ([n][E])
template <typename F>
void for_each_field(ssd_ws_env *env, const ssd_ws_state *st, F f) {
    const WsDev &d = env->p.d;
    f(d.season, st->season, 1, 1); f(d.phase, st->phase, 1, 1); f(d.wrapped, st->wrapped, 1, 1);
    f(d.round, st->round, 1, 4); f(d.episode, st->episode, 1, 4);
    f(d.hist, st->hist, 8, 4); f(d.fr, st->f_rew, 6, 4); f(d.pen, st->pen, 1, 4);
    f(d.csum, st->current_sums, 4, 8); f(d.run, st->running_rew, 4, 8); f(d.prev, st->prev_actions, 4, 4);
}

}  // namespace

// ssd_ws_policy.hpp: the policy rollouts' read-only view of a handle (host code; no kernel of this file knows of it)
namespace ssd {

void ws_policy_view(const ssd_ws_env *env, WsPolicyView *v) {
    const WsParams &p = env->p;
    v->phase = p.d.phase; v->round = p.d.round; v->episode = p.d.episode;
    v->E = p.E; v->variant = p.variant; v->device = env->device;
    v->seed_lo = p.seed_lo; v->seed_hi = p.seed_hi; v->env_base = p.env_base;
}

int ws_fail_invalid(ssd_ws_env *env, const char *msg) {
    env->err = msg;
    return SSD_E_INVALID;
}

int ws_fail_device(ssd_ws_env *env, const char *what, int hip_error) { return ws_fail(env, what, (hipError_t)hip_error); }

}  // namespace ssd

extern "C" {

const char *ssd_ws_last_error(const ssd_ws_env *env) { return env ? env->err.c_str() : g_ws_create_error.c_str(); }

int ssd_ws_create(const ssd_ws_config *cfg, ssd_ws_env **out) {
    if (!cfg || !out) { g_ws_create_error = "null argument"; return SSD_E_INVALID; }
    *out = nullptr;
    if (cfg->struct_size != sizeof(ssd_ws_config)) { g_ws_create_error = "ssd_ws_config.struct_size mismatch"; return SSD_E_INVALID; }
    if (cfg->variant != SSD_WS_SEQ && cfg->variant != SSD_WS_SEQ_COMM) { g_ws_create_error = "unknown variant"; return SSD_E_INVALID; }
    if (cfg->num_envs < 1 || cfg->num_envs > (1 << 26)) { g_ws_create_error = "num_envs must be 1..2^26"; return SSD_E_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_ws_create_error = "no HIP device available: this engine has no CPU path";
        return SSD_E_DEVICE;
    }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) { g_ws_create_error = "device_id out of range"; return SSD_E_INVALID; }
    if (hipSetDevice(cfg->device_id) != hipSuccess) { g_ws_create_error = "hipSetDevice failed"; return SSD_E_DEVICE; }
    ssd_ws_env *env = new ssd_ws_env();
    env->device = cfg->device_id;
    env->stats = nullptr;
    WsParams &p = env->p;
    const size_t E = (size_t)cfg->num_envs;
    p.E = cfg->num_envs; p.variant = cfg->variant; p.local_obs = cfg->local_obs != 0; p.local_rew = cfg->local_rew != 0;
    p.seed_lo = (uint32_t)cfg->seed; p.seed_hi = (uint32_t)(cfg->seed >> 32); p.env_base = cfg->env_index_base;
    // one block: 8-byte fields first, then 4-byte, then 1-byte (every field stays aligned)
    const size_t bytes = E * (8 * 8) + E * (4 * (1 + 1 + 8 + 6 + 1 + 4)) + E * 4 + 64;
    if (hipMalloc(&env->block, bytes) != hipSuccess) {
        g_ws_create_error = "hipMalloc failed";
        delete env;
        return SSD_E_NOMEM;
    }
    char *c = static_cast<char *>(env->block);
    auto take = [&](size_t n) { char *r = c; c += n; return r; };
    WsDev &d = p.d;
    d.csum = (double *)take(E * 32); d.run = (double *)take(E * 32);
    d.round = (int32_t *)take(E * 4); d.episode = (uint32_t *)take(E * 4);
    d.hist = (float *)take(E * 32); d.fr = (float *)take(E * 24); d.pen = (float *)take(E * 4); d.prev = (float *)take(E * 16);
    d.status = (uint32_t *)take(64);
    d.season = (uint8_t *)take(E); d.phase = (uint8_t *)take(E); d.wrapped = (uint8_t *)take(E); d.viol = (uint8_t *)take(E);
    if (hipMemset(env->block, 0, bytes) != hipSuccess || hipMemset(d.episode, 0xFF, E * 4) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        g_ws_create_error = "device initialisation failed";
        (void)hipFree(env->block);
        delete env;
        return SSD_E_DEVICE;
    }
    *out = env;
    return SSD_OK;
}

int ssd_ws_destroy(ssd_ws_env *env) {
    if (!env) return SSD_E_INVALID;
    (void)hipSetDevice(env->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(env->block);
    if (env->stats) env->stats->attached -= 1;
    delete env;
    return SSD_OK;
}

int ssd_ws_reset(ssd_ws_env *env, const uint8_t *env_mask, float *obs, int8_t *agent, void *stream) {
    if (!env) return SSD_E_INVALID;
    WS_HIP(env, hipSetDevice(env->device));
    const WsParams &p = env->p;
    const hipStream_t st = (hipStream_t)stream;
    const int g = grid(env);
    if (env->stats) WS_HIP(env, (hipError_t)ssd::ws_stats_discard(env->stats, env_mask, true, stream));   // truncated; a new episode opens
    if (p.variant == SSD_WS_SEQ) {
        if (p.local_obs) ws_reset_kernel<SSD_WS_SEQ, 1><<<g, kBlock, 0, st>>>(p, env_mask, obs, agent);
        else ws_reset_kernel<SSD_WS_SEQ, 0><<<g, kBlock, 0, st>>>(p, env_mask, obs, agent);
    } else {
        if (p.local_obs) ws_reset_kernel<SSD_WS_SEQ_COMM, 1><<<g, kBlock, 0, st>>>(p, env_mask, obs, agent);
        else ws_reset_kernel<SSD_WS_SEQ_COMM, 0><<<g, kBlock, 0, st>>>(p, env_mask, obs, agent);
    }
    WS_HIP(env, hipGetLastError());
    return SSD_OK;
}

int ssd_ws_rollout_actions(ssd_ws_env *env, const float *actions, int32_t action_ring, int32_t n_steps, int32_t step0, float *obs,
                           int8_t *agent, double *rew, uint8_t *done, int32_t ring, uint32_t flags, void *stream) {
    if (!env) return SSD_E_INVALID;
    if (!actions || action_ring < 1 || ring < 1 || n_steps < 0 || step0 < 0) { env->err = "bad rollout arguments"; return SSD_E_INVALID; }
    if ((flags & ~(uint32_t)SSD_AUTO_RESET) != 0) { env->err = "unsupported flag"; return SSD_E_INVALID; }
    if (n_steps == 0) return SSD_OK;
    WS_HIP(env, hipSetDevice(env->device));
    const WsParams &p = env->p;
    const int ar = (flags & SSD_AUTO_RESET) ? 1 : 0;
    // the instances without the statistics are launched exactly when no handle is attached
#define WS_ROLLOUT(V, LO, LR)                                                                                               \
    if (env->stats)                                                                                                         \
        ws_rollout_stats_kernel<V, LO, LR><<<grid(env), kBlock, 0, (hipStream_t)stream>>>(p, env->stats->d, actions, action_ring, n_steps, \
                                                                                           step0, obs, agent, rew, done, ring, ar);  \
    else                                                                                                                    \
        ws_rollout_kernel<V, LO, LR><<<grid(env), kBlock, 0, (hipStream_t)stream>>>(p, actions, action_ring, n_steps, step0, obs,    \
                                                                                     agent, rew, done, ring, ar)
    switch ((p.variant == SSD_WS_SEQ_COMM ? 4 : 0) | (p.local_obs ? 2 : 0) | (p.local_rew ? 1 : 0)) {
        case 0: WS_ROLLOUT(SSD_WS_SEQ, 0, 0); break;
        case 1: WS_ROLLOUT(SSD_WS_SEQ, 0, 1); break;
        case 2: WS_ROLLOUT(SSD_WS_SEQ, 1, 0); break;
        case 3: WS_ROLLOUT(SSD_WS_SEQ, 1, 1); break;
        case 4: WS_ROLLOUT(SSD_WS_SEQ_COMM, 0, 0); break;
        case 5: WS_ROLLOUT(SSD_WS_SEQ_COMM, 0, 1); break;
        case 6: WS_ROLLOUT(SSD_WS_SEQ_COMM, 1, 0); break;
        default: WS_ROLLOUT(SSD_WS_SEQ_COMM, 1, 1); break;
    }
#undef WS_ROLLOUT
    WS_HIP(env, hipGetLastError());
    return SSD_OK;
}

int ssd_ws_stats_attach(ssd_ws_env *env, ssd_ws_stats *stats) {
    if (!env) return SSD_E_INVALID;
    if (stats && (stats->variant != env->p.variant || stats->d.E != env->p.E || stats->device != env->device)) {
        env->err = "the statistics handle's variant, env count or device differ from the engine's";
        return SSD_E_INVALID;
    }
    if (env->stats) env->stats->attached -= 1;
    env->stats = stats;
    if (stats) stats->attached += 1;
    return SSD_OK;
}

int ssd_ws_step(ssd_ws_env *env, const float *actions, float *obs, int8_t *agent, double *rew, uint8_t *done, uint32_t flags,
                void *stream) {
    return ssd_ws_rollout_actions(env, actions, 1, 1, 0, obs, agent, rew, done, 1, flags, stream);
}

int ssd_ws_info(ssd_ws_env *env, uint8_t *viol, uint8_t *true_end, double *running_rew, double *temp, int64_t *other_agent_actions,
                void *stream) {
    if (!env) return SSD_E_INVALID;
    WS_HIP(env, hipSetDevice(env->device));
    ws_info_kernel<<<grid(env), kBlock, 0, (hipStream_t)stream>>>(env->p, viol, true_end, running_rew, temp, other_agent_actions);
    WS_HIP(env, hipGetLastError());
    return SSD_OK;
}

int ssd_ws_get_state(ssd_ws_env *env, const ssd_ws_state *st) {
    if (!env || !st) return SSD_E_INVALID;
    WS_HIP(env, hipSetDevice(env->device));
    WS_HIP(env, hipDeviceSynchronize());
    const size_t E = (size_t)env->p.E;
    std::vector<char> buf;
    int rc = SSD_OK;
    for_each_field(env, st, [&](const void *dev, void *host, int n, int w) {
        if (!host || rc != SSD_OK) return;
        buf.resize(E * n * w);
        if (hipMemcpy(buf.data(), dev, buf.size(), hipMemcpyDeviceToHost) != hipSuccess) { rc = SSD_E_DEVICE; return; }
        for (size_t e = 0; e < E; ++e)                           // [n][E] -> [E][n]
            for (int j = 0; j < n; ++j) memcpy((char *)host + (e * n + j) * w, buf.data() + ((size_t)j * E + e) * w, w);
    });
    if (rc == SSD_OK && st->viol) {
        std::vector<uint8_t> v(E);
        if (hipMemcpy(v.data(), env->p.d.viol, E, hipMemcpyDeviceToHost) != hipSuccess) rc = SSD_E_DEVICE;
        for (size_t e = 0; e < E && rc == SSD_OK; ++e)
            for (int j = 0; j < 6; ++j) st->viol[e * 6 + j] = (v[e] >> j) & 1u;
    }
    if (rc != SSD_OK) env->err = "state copy failed";
    return rc;
}

int ssd_ws_set_state(ssd_ws_env *env, const ssd_ws_state *st) {
    if (!env || !st) return SSD_E_INVALID;
    const size_t E = (size_t)env->p.E;
    const uint32_t P = env->p.variant == SSD_WS_SEQ ? 4u : 12u;
    if (!st->season || !st->phase || !st->wrapped || !st->viol || !st->round || !st->episode || !st->hist || !st->f_rew || !st->pen ||
        !st->current_sums || !st->running_rew || !st->prev_actions) {
        env->err = "set_state needs every field";
        return SSD_E_INVALID;
    }
    for (size_t e = 0; e < E; ++e)
        if (st->season[e] >= 108 || st->phase[e] > P || st->round[e] < 0) { env->err = "state out of range"; return SSD_E_INVALID; }
    WS_HIP(env, hipSetDevice(env->device));
    WS_HIP(env, hipDeviceSynchronize());
    std::vector<char> buf;
    int rc = SSD_OK;
    for_each_field(env, st, [&](void *dev, const void *host, int n, int w) {
        if (rc != SSD_OK) return;
        buf.resize(E * n * w);
        for (size_t e = 0; e < E; ++e)
            for (int j = 0; j < n; ++j) memcpy(buf.data() + ((size_t)j * E + e) * w, (const char *)host + (e * n + j) * w, w);
        if (hipMemcpy(dev, buf.data(), buf.size(), hipMemcpyHostToDevice) != hipSuccess) rc = SSD_E_DEVICE;
    });
    if (rc == SSD_OK) {
        std::vector<uint8_t> v(E, 0);
        for (size_t e = 0; e < E; ++e)
            for (int j = 0; j < 6; ++j) v[e] |= (st->viol[e * 6 + j] ? 1u : 0u) << j;
        if (hipMemcpy(env->p.d.viol, v.data(), E, hipMemcpyHostToDevice) != hipSuccess) rc = SSD_E_DEVICE;
    }
    if (rc != SSD_OK) env->err = "state copy failed";
    return rc;
}

int ssd_ws_device_status(ssd_ws_env *env, uint32_t *status, int clear) {
    if (!env || !status) return SSD_E_INVALID;
    WS_HIP(env, hipSetDevice(env->device));
    WS_HIP(env, hipDeviceSynchronize());
    WS_HIP(env, hipMemcpy(status, env->p.d.status, 4, hipMemcpyDeviceToHost));
    if (clear) WS_HIP(env, hipMemset(env->p.d.status, 0, 4));
    return SSD_OK;
}

}  // extern "C"
