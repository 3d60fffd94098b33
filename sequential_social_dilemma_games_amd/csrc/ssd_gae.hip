// ssd_gae.hip -- advantages and value targets of rollout batches (include/ssd.h, ssd_advantages): RLlib's compute_advantages
// (generalised advantage estimation, or discounted returns with or without a critic) over the [ring, L] rings the rollout
// calls write, with the episode cuts (done) and the fragment bootstrap (last_value).  DESIGN.md section 15 states the contract.
//
// One lane per trajectory (an (env, agent) pair, L = E * N of them), walking its column backwards in time: the recurrence
// is sequential in k, and a time-split scan would reorder its float operations, so there is none.  Every operation is one
// IEEE float64 operation in the order the header gives (the build has -ffp-contract=off: no fused multiply-add); the two
// results are rounded to float32 once, when they are stored.  A row is contiguous across lanes, so a wave's loads and
// stores are whole 256-byte (64-byte for done) segments.
//
// At 4096 envs x 5 agents there are 320 waves for 256 CUs: nothing hides a load's latency but the wave's own other loads.
// The loads do not depend on the recurrence, so a block of kLoad steps is requested first, and the next block's while the
// dependent chain of the current one runs (two register buffers).  Blocks are one wave (64 threads) so that the waves spread
// over as many CUs as there are.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_batch.hpp"

#ifndef SSD_GAE_LOAD_BLOCK
#define SSD_GAE_LOAD_BLOCK 16                                    // DESIGN.md section 15 has the lengths tried
#endif

namespace {

constexpr int kBlock = 64;
constexpr int kLoad = SSD_GAE_LOAD_BLOCK;                        // steps whose loads are issued together

enum { kGae = 0, kReturnsCritic = 1, kReturns = 2 };

struct GaeArgs {
    const int32_t *rew;
    const float *bonus, *value, *last_value;
    const uint8_t *done;
    float *adv, *vt;
    double bonus_weight, gamma, gl;
    int32_t L, ring, step0, K;
};

template <int kMode, bool kBonus, bool kDone>
struct Rows {                                                    // the inputs of kLoad steps of one lane, in registers
    int32_t r[kLoad], d[kLoad];
    float v[kLoad], b[kLoad];

    // kLoad rows (kFull), or the first n of them, walking down from the row in slot `slot`; returns the slot kLoad rows
    // further down.  Two things keep this in registers and the loads in flight.  Every index is a constant once the loops
    // are unrolled (no early exit from them): indexed at run time the arrays go to scratch.  And a full block is straight-line
    // code: behind a per-row guard the loaded values meet at a join, and the compiler waits for all of them there.
    template <bool kFull>
    __device__ __forceinline__ int load(const GaeArgs &a, size_t lane, int n, int slot) {
#pragma unroll
        for (int u = 0; u < kLoad; ++u) {
            const bool ok = kFull || u < n;
            const size_t off = (size_t)slot * (size_t)a.L + lane;
            r[u] = ok ? a.rew[off] : 0;
            if (kMode != kReturns) v[u] = ok ? a.value[off] : 0.0f;
            if (kBonus) b[u] = ok ? a.bonus[off] : 0.0f;
            if (kDone) d[u] = ok ? (int32_t)a.done[off] : 0;
            if (--slot < 0) slot = a.ring - 1;
        }
        return slot;
    }
};

struct Walk {                                                    // what the recurrence carries from row k + 1 to row k
    double v_after;                                              // the value of the row after k (last_value at the start)
    double run;                                                  // A (or G) of row k + 1
    int slot;                                                    // of row k
    bool last;                                                   // k = K - 1
};

// the rows of `in` (all kLoad, or the first n), in their order: the dependent chain, and the stores
template <bool kFull, int kMode, bool kBonus, bool kDone>
__device__ __forceinline__ void chain(const GaeArgs &a, size_t lane, int n, const Rows<kMode, kBonus, kDone> &in, Walk &w) {
#pragma unroll
    for (int u = 0; u < kLoad; ++u) {
        if (!kFull && u >= n) continue;
        const size_t off = (size_t)w.slot * (size_t)a.L + lane;
        const bool dn = kDone && in.d[u] != 0;
        const bool cut = dn || w.last;
        double r = (double)in.r[u];
        if (kBonus) {
            const double wb = a.bonus_weight * (double)in.b[u];
            r = r + wb;
        }
        const double v_next = dn ? 0.0 : w.v_after;
        if (kMode == kGae) {
            const double vk = (double)in.v[u];
            const double carry = cut ? 0.0 : w.run;
            const double gv = a.gamma * v_next;
            const double delta = (r + gv) - vk;
            const double gc = a.gl * carry;
            const double A = delta + gc;
            a.adv[off] = (float)A;
            a.vt[off] = (float)(A + vk);
            w.run = A;
            w.v_after = vk;
        } else {
            const double g_next = cut ? v_next : w.run;          // (v_after stays last_value: only the last row reads it)
            const double gg = a.gamma * g_next;
            const double G = r + gg;
            if (kMode == kReturnsCritic) {
                a.adv[off] = (float)(G - (double)in.v[u]);
                a.vt[off] = (float)G;
            } else {
                a.adv[off] = (float)G;
                a.vt[off] = 0.0f;
            }
            w.run = G;
        }
        w.last = false;
        if (--w.slot < 0) w.slot = a.ring - 1;
    }
}

template <int kMode, bool kBonus, bool kDone>
__global__ void __launch_bounds__(kBlock) gae_kernel(GaeArgs a) {
    const size_t lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (lane >= (size_t)a.L) return;                             // the last wave's spare lanes
    Walk w;
    w.v_after = a.last_value ? (double)a.last_value[lane] : 0.0;
    w.run = 0.0;
    w.slot = (int)(((int64_t)a.step0 + a.K - 1) % a.ring);
    w.last = true;
    // the full blocks, through two buffers that swap roles (no copy between them): while one's chain runs, the other's loads
    // are in flight
    Rows<kMode, kBonus, kDone> even, odd;
    int full = a.K / kLoad;
    if (full > 0) {
        int load_slot = even.template load<true>(a, lane, kLoad, w.slot);
        for (;;) {
            if (full == 1) { chain<true>(a, lane, kLoad, even, w); break; }
            load_slot = odd.template load<true>(a, lane, kLoad, load_slot);
            chain<true>(a, lane, kLoad, even, w);
            --full;
            if (full == 1) { chain<true>(a, lane, kLoad, odd, w); break; }
            load_slot = even.template load<true>(a, lane, kLoad, load_slot);
            chain<true>(a, lane, kLoad, odd, w);
            --full;
        }
    }
    // the rows left at the start of the fragment, fewer than kLoad
    const int left = a.K % kLoad;
    if (left > 0) {
        even.template load<false>(a, lane, left, w.slot);
        chain<false>(a, lane, left, even, w);
    }
}

thread_local ssd::BatchError g_adv_error;

int fail(const char *msg) { return g_adv_error.invalid(msg); }

template <int kMode>
void launch(const GaeArgs &a, dim3 grid, hipStream_t s) {
    ssd::with_bonus_done(a.bonus != nullptr, a.done != nullptr, [&](auto kBonus, auto kDone) {
        hipLaunchKernelGGL((gae_kernel<kMode, decltype(kBonus)::value, decltype(kDone)::value>), grid, dim3(kBlock), 0, s, a);
    });
}

}  // namespace

extern "C" {

const char *ssd_advantages_last_error(void) { return g_adv_error.c_str(); }

int ssd_advantages(const int32_t *rew, const float *bonus, double bonus_weight, const float *value, const uint8_t *done,
                   const float *last_value, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps, double gamma,
                   double lambda, uint32_t flags, float *advantages, float *value_targets, int32_t device_id, void *stream) {
    if (const char *msg = ssd::check_ring(lanes, ring, step0, n_steps)) return fail(msg);
    if ((flags & ~(uint32_t)(SSD_ADV_GAE | SSD_ADV_CRITIC)) != 0) return fail("unsupported flag");
    const bool gae = (flags & SSD_ADV_GAE) != 0, critic = (flags & SSD_ADV_CRITIC) != 0;
    if (gae && !critic) return fail("generalised advantage estimation needs the critic: set both flags");
    if (!rew) return fail("rew is required");
    if (!advantages || !value_targets) return fail("advantages and value_targets are required");
    if (critic && !value) return fail("value is required when the critic is used");
    if (!isfinite(gamma) || !isfinite(lambda)) return fail("gamma and lambda must be finite");
    if (bonus && !isfinite(bonus_weight)) return fail("bonus_weight must be finite");
    if (const int rc = ssd::use_device(g_adv_error, device_id)) return rc;
    GaeArgs a{};
    a.rew = rew; a.bonus = bonus; a.value = value; a.last_value = last_value; a.done = done;
    a.adv = advantages; a.vt = value_targets;
    a.bonus_weight = bonus_weight; a.gamma = gamma; a.gl = gamma * lambda;
    a.L = lanes; a.ring = ring; a.step0 = step0; a.K = n_steps;
    const dim3 grid((unsigned)(((int64_t)lanes + kBlock - 1) / kBlock));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (gae) launch<kGae>(a, grid, s);
    else if (critic) launch<kReturnsCritic>(a, grid, s);
    else launch<kReturns>(a, grid, s);
    return g_adv_error.launched("advantages");
}

}  // extern "C"
