// csrc/ssd_ws_stats.hpp -- Watershed episode statistics (include/ssd.h, ssd_ws_stats_*): the handle, its
// device layout and the per-lane pieces the stepping kernel's stats instances run (ssd_watershed.hip).  The handle's own
// kernels and C ABI are in ssd_ws_stats.hip.  Every float64 operation is one IEEE operation in the order written (the build
// keeps -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string>

#include "../../include/ssd.h"

namespace ssd {

// 8-byte fields of a handle, SoA [slot][E] behind WsStatsDev::q8 (float64 unless marked i64)
enum WsStatsSlot {
    WSS_O_REW = 0,                  // the open episode: reward so far
    WSS_O_AGENT = 1,                // ... [8] per receiving agent
    WSS_COUNTS = 9,                 // i64 [3] episodes, truncated, sum of lengths
    WSS_REW_SUM = 12,
    WSS_AGENT_SUMS = 13,            // [8]
    WSS_M_SUM = 21,                 // [3] violations, Equality, Utility: sums of the finite values
    WSS_M_CNT = 24,                 // i64 [3]
    WSS_M_MIN = 27,                 // [3]
    WSS_M_MAX = 30,                 // [3]
    WSS_L_LEN = 33,                 // i64; the last finished episode
    WSS_L_REW = 34,
    WSS_L_AGENT = 35,               // [8]
    WSS_L_TOT = 43,                 // [4]
    WSS_L_MET = 47,                 // [3]
    WSS_SLOTS8 = 50
};
// 4-byte fields [slot][E] behind q4: the open episode's length, sum of popcount(viol) and number of viol entries
enum { WSS_O_LEN = 0, WSS_O_VSUM = 1, WSS_O_VCNT = 2, WSS_SLOTS4 = 3 };

struct WsStatsDev {
    char *q8;                       // [WSS_SLOTS8][E] 8-byte fields
    int32_t *q4;                    // [WSS_SLOTS4][E]
    uint8_t *open;                  // [E] 1 while an episode that began at a reset is being counted
    int32_t E;

    __host__ __device__ double *f64(int slot, int e) const { return reinterpret_cast<double *>(q8) + (size_t)slot * E + e; }
    __host__ __device__ int64_t *i64(int slot, int e) const { return reinterpret_cast<int64_t *>(q8) + (size_t)slot * E + e; }
    __host__ __device__ int32_t *i32(int slot, int e) const { return q4 + (size_t)slot * E + e; }
};

// The open episode of one lane, in registers for the length of a launch.  NA: 4 (Seq) or 8 (SeqComm) agents.
template <int NA>
struct WsOpenEpisode {
    uint32_t open;
    int32_t len, vsum, vcnt;
    double rew, agent[NA];

    __device__ __forceinline__ void clear() {
        len = 0; vsum = 0; vcnt = 0; rew = 0.0;
#pragma unroll
        for (int j = 0; j < NA; ++j) agent[j] = 0.0;
    }

    __device__ __forceinline__ void load(const WsStatsDev &d, int e) {
        open = d.open[e];
        len = *d.i32(WSS_O_LEN, e); vsum = *d.i32(WSS_O_VSUM, e); vcnt = *d.i32(WSS_O_VCNT, e);
        rew = *d.f64(WSS_O_REW, e);
#pragma unroll
        for (int j = 0; j < NA; ++j) agent[j] = *d.f64(WSS_O_AGENT + j, e);
    }

    __device__ __forceinline__ void store(const WsStatsDev &d, int e) const {
        d.open[e] = (uint8_t)open;
        *d.i32(WSS_O_LEN, e) = len; *d.i32(WSS_O_VSUM, e) = vsum; *d.i32(WSS_O_VCNT, e) = vcnt;
        *d.f64(WSS_O_REW, e) = rew;
#pragma unroll
        for (int j = 0; j < NA; ++j) *d.f64(WSS_O_AGENT + j, e) = agent[j];
    }

    // One step of an open episode: `r` is the value the rew ring gets, `receiver` the agent it was delivered to, `viol` the
    // env's n_viol bits after the step.  on_episode_step appends agent-0's latest viol once agent-0 has an info, which is
    // from the episode's 4th step on in both variants, and from then on that viol is the env's current one.
    __device__ __forceinline__ void step(double r, int receiver, uint32_t viol) {
        len += 1;
        rew = rew + r;
        // Every agent's sum takes an add, the others' of +0.0: written as `if (j == receiver)` the compiler indexes the array by
        // `receiver` and moves it to scratch memory.  The bits are the same: a sum here starts at +0.0 and so is never -0.0.
#pragma unroll
        for (int j = 0; j < NA; ++j) agent[j] = agent[j] + (j == receiver ? r : 0.0);
        if (len >= 4) { vsum += __popc(viol); vcnt += 6; }
    }

    // The DONE_ALL step: on_episode_end on running_rew as the env reports it at that step.  The episode goes into the lane's
    // last-episode record, and the record is then folded into the lane's accumulators slot by slot in rolled loops (the lane
    // reads back what it has just written): unrolled, the loads of some thirty accumulators would be live at once in a loop
    // body that otherwise needs none of them.
    __device__ __forceinline__ void finish(const WsStatsDev &d, int e, const double tot[4]) const {
        double usum = 0.0, num = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) usum = usum + tot[i];
        const double utility = 2.0 * usum;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) num = num + fabs(tot[i] - tot[j]);
        *d.i64(WSS_L_LEN, e) = len;
        *d.f64(WSS_L_REW, e) = rew;
#pragma unroll
        for (int j = 0; j < 8; ++j) *d.f64(WSS_L_AGENT + j, e) = j < NA ? agent[j < NA ? j : 0] : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) *d.f64(WSS_L_TOT + j, e) = tot[j];
        *d.f64(WSS_L_MET + 0, e) = (double)vsum / (double)vcnt;
        *d.f64(WSS_L_MET + 1, e) = 1.0 - num / utility;
        *d.f64(WSS_L_MET + 2, e) = utility;
        *d.i64(WSS_COUNTS + 0, e) += 1;
        *d.i64(WSS_COUNTS + 2, e) += len;
        *d.f64(WSS_REW_SUM, e) = *d.f64(WSS_REW_SUM, e) + rew;
#pragma unroll 1
        for (int j = 0; j < NA; ++j) *d.f64(WSS_AGENT_SUMS + j, e) = *d.f64(WSS_AGENT_SUMS + j, e) + *d.f64(WSS_L_AGENT + j, e);
#pragma unroll 1
        for (int m = 0; m < 3; ++m) {
            const double v = *d.f64(WSS_L_MET + m, e);
            if (isfinite(v)) {
                *d.f64(WSS_M_SUM + m, e) = *d.f64(WSS_M_SUM + m, e) + v;
                *d.i64(WSS_M_CNT + m, e) += 1;
                if (v < *d.f64(WSS_M_MIN + m, e)) *d.f64(WSS_M_MIN + m, e) = v;
                if (v > *d.f64(WSS_M_MAX + m, e)) *d.f64(WSS_M_MAX + m, e) = v;
            }
        }
    }
};

}  // namespace ssd

struct ssd_ws_stats {
    ssd::WsStatsDev d;
    int32_t variant, device;
    int32_t attached;               // engines holding this handle (ssd_ws_stats_attach): destroy refuses while > 0
    void *block;                    // the one device allocation behind d
    std::string err;
};

namespace ssd {

// Enqueue the discard of the open episodes selected by env_mask (u8 [E] device, NULL = all): one with at least one step counts
// as truncated.  reopen: the selected envs then begin a new episode (what ssd_ws_reset does on an attached engine).
// Returns a hipError_t as int.
int ws_stats_discard(ssd_ws_stats *st, const uint8_t *env_mask, bool reopen, void *stream);

}  // namespace ssd
