// ssd_vtrace.hip -- V-trace targets of rollout batches (include/ssd.h, ssd_vtrace): vtrace.from_importance_weights of RLlib
// 0.7.6 (IMPALA; Espeholt et al. 2018) over the [ring, L] rings the rollout calls write, with the episode cuts (done) in the
// discount and the fragment bootstrap.  DESIGN.md section 20 states the contract.
//
// Built as ssd_gae.hip is: one lane per trajectory walking its column backwards in time, every
// operation one IEEE float64 operation in the order the header gives (-ffp-contract=off), the two results rounded to float32
// once at the store; one-wave blocks; the loads of a block of kLoad steps requested together, and the next block's while the
// current block's dependent chain runs (two register buffers that swap roles).  The importance weights are an input: the
// kernel computes no exp, so that it and the NumPy path agree bit for bit.
//
// Of a row's arithmetic only acc = delta + dc * acc is on the dependent chain (one multiply, one add).  delta and dc read
// loaded values alone; pg reads the vs of the row after it, a side branch that nothing waits for.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_batch.hpp"

#ifndef SSD_VTRACE_LOAD_BLOCK
#define SSD_VTRACE_LOAD_BLOCK 16                                 // DESIGN.md section 20 has the lengths tried
#endif

namespace {

constexpr int kBlock = 64;
constexpr int kLoad = SSD_VTRACE_LOAD_BLOCK;                     // steps whose loads are issued together

struct VtArgs {
    const int32_t *rew;
    const float *bonus, *value, *rhos, *bootstrap;
    const uint8_t *done;
    float *vs, *pg;
    double bonus_weight, gamma, clip_rho, clip_pg;
    int32_t L, ring, step0, K;
};

template <bool kBonus, bool kDone>
struct Rows {                                                    // the inputs of kLoad steps of one lane, in registers
    int32_t r[kLoad], d[kLoad];
    float v[kLoad], rho[kLoad], b[kLoad];

    // kLoad rows (kFull), or the first n of them, walking down from the row in slot `slot`; returns the slot kLoad rows
    // further down.  As ssd_gae.hip's loader: every index is a constant once the loops are unrolled (indexed at run time
    // the arrays go to scratch), and a full block is straight-line code (behind a per-row guard the loaded values meet at a
    // join, and the compiler waits for all of them there).
    template <bool kFull>
    __device__ __forceinline__ int load(const VtArgs &a, size_t lane, int n, int slot) {
#pragma unroll
        for (int u = 0; u < kLoad; ++u) {
            const bool ok = kFull || u < n;
            const size_t off = (size_t)slot * (size_t)a.L + lane;
            r[u] = ok ? a.rew[off] : 0;
            v[u] = ok ? a.value[off] : 0.0f;
            rho[u] = ok ? a.rhos[off] : 0.0f;
            if (kBonus) b[u] = ok ? a.bonus[off] : 0.0f;
            if (kDone) d[u] = ok ? (int32_t)a.done[off] : 0;
            if (--slot < 0) slot = a.ring - 1;
        }
        return slot;
    }
};

struct Walk {                                                    // what the recurrence carries from row k + 1 to row k
    double v_after;                                              // the value of the row after k (the bootstrap at the start)
    double vs_after;                                             // the unrounded vs of the row after k (the bootstrap at the start)
    double acc;                                                  // vs - v of row k + 1 (0.0 at the start: dc * 0.0 is the contract's)
    int slot;                                                    // of row k
};

// the rows of `in` (all kLoad, or the first n), in their order: the dependent chain, and the stores
template <bool kFull, bool kBonus, bool kDone>
__device__ __forceinline__ void chain(const VtArgs &a, size_t lane, int n, const Rows<kBonus, kDone> &in, Walk &w) {
#pragma unroll
    for (int u = 0; u < kLoad; ++u) {
        if (!kFull && u >= n) continue;
        const size_t off = (size_t)w.slot * (size_t)a.L + lane;
        double r = (double)in.r[u];
        if (kBonus) {
            const double wb = a.bonus_weight * (double)in.b[u];
            r = r + wb;
        }
        const double disc = (kDone && in.d[u] != 0) ? 0.0 : a.gamma;
        const double v = (double)in.v[u];
        const double rho = (double)in.rho[u];
        const double dv = disc * w.v_after;
        const double delta = fmin(a.clip_rho, rho) * ((r + dv) - v);
        const double dc = disc * fmin(1.0, rho);
        const double da = dc * w.acc;
        const double acc = delta + da;
        const double vs = v + acc;
        const double dvs = disc * w.vs_after;
        const double pg = fmin(a.clip_pg, rho) * ((r + dvs) - v);
        a.vs[off] = (float)vs;
        a.pg[off] = (float)pg;
        w.acc = acc;
        w.v_after = v;
        w.vs_after = vs;
        if (--w.slot < 0) w.slot = a.ring - 1;
    }
}

template <bool kBonus, bool kDone>
__global__ void __launch_bounds__(kBlock) vtrace_kernel(VtArgs a) {
    const size_t lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (lane >= (size_t)a.L) return;                             // the last wave's spare lanes
    Walk w;
    w.v_after = w.vs_after = a.bootstrap ? (double)a.bootstrap[lane] : 0.0;
    w.acc = 0.0;
    w.slot = (int)(((int64_t)a.step0 + a.K - 1) % a.ring);
    // the full blocks, through two buffers that swap roles (no copy between them): while one's chain runs, the other's loads
    // are in flight
    Rows<kBonus, kDone> even, odd;
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

thread_local ssd::BatchError g_vt_error;

int fail(const char *msg) { return g_vt_error.invalid(msg); }

}  // namespace

extern "C" {

const char *ssd_vtrace_last_error(void) { return g_vt_error.c_str(); }

int ssd_vtrace(const int32_t *rew, const float *bonus, double bonus_weight, const float *value, const float *rhos,
               const uint8_t *done, const float *bootstrap_value, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps,
               double gamma, double clip_rho_threshold, double clip_pg_rho_threshold, uint32_t flags, float *vs,
               float *pg_advantages, int32_t device_id, void *stream) {
    if (const char *msg = ssd::check_ring(lanes, ring, step0, n_steps)) return fail(msg);
    if (flags != 0) return fail("unsupported flag");
    if (!rew) return fail("rew is required");
    if (!value) return fail("value is required: the target policy's values");
    if (!rhos) return fail("rhos is required: the importance weights of the taken actions");
    if (!vs || !pg_advantages) return fail("vs and pg_advantages are required");
    if (!isfinite(gamma)) return fail("gamma must be finite");
    if (!(clip_rho_threshold > 0.0) || !(clip_pg_rho_threshold > 0.0))
        return fail("clip_rho_threshold and clip_pg_rho_threshold must be > 0 (+inf: no clip)");
    if (bonus && !isfinite(bonus_weight)) return fail("bonus_weight must be finite");
    if (const int rc = ssd::use_device(g_vt_error, device_id)) return rc;
    VtArgs a{};
    a.rew = rew; a.bonus = bonus; a.value = value; a.rhos = rhos; a.bootstrap = bootstrap_value; a.done = done;
    a.vs = vs; a.pg = pg_advantages;
    a.bonus_weight = bonus_weight; a.gamma = gamma; a.clip_rho = clip_rho_threshold; a.clip_pg = clip_pg_rho_threshold;
    a.L = lanes; a.ring = ring; a.step0 = step0; a.K = n_steps;
    const dim3 grid((unsigned)(((int64_t)lanes + kBlock - 1) / kBlock));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    ssd::with_bonus_done(bonus != nullptr, done != nullptr, [&](auto kBonus, auto kDone) {
        hipLaunchKernelGGL((vtrace_kernel<decltype(kBonus)::value, decltype(kDone)::value>), grid, dim3(kBlock), 0, s, a);
    });
    return g_vt_error.launched("vtrace");
}

}  // extern "C"
