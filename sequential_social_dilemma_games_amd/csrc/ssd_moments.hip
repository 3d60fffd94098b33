// ssd_moments.hip -- per-weight-set moments of rollout batches (include/ssd.h, BATCH MOMENTS): ssd_standardize, the step RLlib
// 0.7.6's PPO optimizer takes between compute_advantages and the SGD epochs (standardize_fields=["advantages"]), and
// ssd_explained_variance, the trainer's vf_explained_var.  DESIGN.md section 25 states the contract.
//
// Both are two-pass moments in float64 whose summation order is fixed by the header: a thread adds SSD_MOM_ITEMS elements a
// stride of SSD_MOM_BLOCK apart, one after the other; a workgroup folds its SSD_MOM_BLOCK thread sums by halving (t += t + off,
// off = 128 ... 1); the chunk partials are added in chunk order.  The build has -ffp-contract=off (no fused multiply-add), and
// there is no floating-point atomic: every partial is stored by its one owner.  The passes are separate launches on the
// caller's stream -- no cooperative launch, no grid-wide barrier -- and every later launch adds up the earlier one's partials
// again, which is what keeps a pass from waiting on anything but the kernel boundary: a workgroup stages SSD_MOM_BLOCK partials
// at a time in LDS (one coalesced load), its first wave adds them up in chunk order (broadcast reads) and hands the sum to the
// others through LDS.  The chain of dependent adds is the cost: read one by one from memory each add waited for its own load,
// and with every wave adding for itself the call took longer again (DESIGN.md section 25 has the three timings).
//
// Grid: x = the chunks of one set, y = the sets.  Element j of set p is flat element j * P + p of the call, so with P > 1 a
// wave reads every P-th float of a row: the sets' workgroups of one chunk share their cache lines through the L2.  The order
// above says nothing about how the elements are fetched; a staged fetch would keep the bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/ssd.h"
#include "ssd_batch.hpp"

namespace {

constexpr int kBlock = SSD_MOM_BLOCK;
constexpr int kItems = SSD_MOM_ITEMS;
static_assert(kBlock == 256, "block_sum's tree is written for four waves");

struct MomArgs {
    const float *x, *pred;                                       // pred: explained variance only
    float *out;                                                  // standardised values, or explained variance [P]
    double *scratch, *moments;
    double min_std;
    int64_t n;                                                   // elements per set
    int64_t base, split;                                         // flat element i of the call is x[i + base] for i < split,
                                                                 // x[i - split] past the ring's end
    int32_t P, chunks;
};

__device__ __forceinline__ int64_t address(const MomArgs &a, int64_t j, int p) {
    const int64_t i = j * a.P + p;
    return i < a.split ? i + a.base : i - a.split;
}

// the kV values of set element j: x; or y and y - pred, the difference formed in float64
template <int kV>
__device__ __forceinline__ void values(const MomArgs &a, int64_t at, double (&v)[kV]) {
    v[0] = (double)a.x[at];
    if (kV == 2) v[1] = v[0] - (double)a.pred[at];
}

// the workgroup's thread sums folded by halving; the result is thread 0's
__device__ __forceinline__ double block_sum(double v, double *lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    if (t < 128) lds[t] = lds[t] + lds[t + 128];
    __syncthreads();
    double r = 0.0;
    if (t < 64) {                                                // the first wave, whole
        r = lds[t] + lds[t + 64];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) r = r + __shfl_down(r, off, 64);
    }
    __syncthreads();                                             // lds is free again
    return r;
}

// the chunk partials of one set and one quantity, in chunk order: added up by the first wave, returned to every thread
__device__ __forceinline__ double combine(const double *part, int chunks, double *lds) {
    const int t = threadIdx.x;
    double s = 0.0;
    for (int c0 = 0; c0 < chunks; c0 += kBlock) {
        const int m = chunks - c0 < kBlock ? chunks - c0 : kBlock;
        if (t < m) lds[t] = part[c0 + t];
        __syncthreads();
        if (t < 64) {
            if (m == kBlock) {
#pragma unroll 16
                for (int c = 0; c < kBlock; ++c) s = s + lds[c];
            } else {
                for (int c = 0; c < m; ++c) s = s + lds[c];
            }
        }
        __syncthreads();                                         // lds is free again
    }
    if (t == 0) lds[0] = s;
    __syncthreads();
    s = lds[0];
    __syncthreads();
    return s;
}

// partials of quantity q, set p: scratch[(q * P + p) * chunks + c]
__device__ __forceinline__ double *partials(const MomArgs &a, int q, int p) {
    return a.scratch + ((size_t)q * a.P + p) * (size_t)a.chunks;
}

// pass 1 (kSecond = false): the sums.  pass 2: the sums of squared deviations from the means of pass 1.
template <int kV, bool kSecond>
__global__ void __launch_bounds__(kBlock) moments_pass(MomArgs a) {
    __shared__ double lds[kBlock];
    const int p = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const int64_t j0 = (int64_t)c * (kBlock * kItems) + t;
    double v[kItems][kV] = {};
#pragma unroll
    for (int u = 0; u < kItems; ++u) {                           // the loads first: nothing below depends on them until the
        const int64_t j = j0 + (int64_t)u * kBlock;              // chain, and the means' partials are added up meanwhile
        if (j < a.n) values<kV>(a, address(a, j, p), v[u]);
    }
    double mean[kV], acc[kV];
#pragma unroll
    for (int q = 0; q < kV; ++q) {
        acc[q] = 0.0;
        mean[q] = kSecond ? combine(partials(a, q, p), a.chunks, lds) / (double)a.n : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kItems; ++u) {
        if (j0 + (int64_t)u * kBlock >= a.n) continue;
#pragma unroll
        for (int q = 0; q < kV; ++q) {
            if (kSecond) {
                const double d = v[u][q] - mean[q];
                const double dd = d * d;
                acc[q] = acc[q] + dd;
            } else {
                acc[q] = acc[q] + v[u][q];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kV; ++q) {
        const double s = block_sum(acc[q], lds);
        if (t == 0) partials(a, (kSecond ? kV : 0) + q, p)[c] = s;
    }
}

__device__ __forceinline__ double variance(const MomArgs &a, int q, int p, double *lds) {
    return combine(partials(a, q, p), a.chunks, lds) / (double)a.n;
}

// pass 3 of ssd_standardize
__global__ void __launch_bounds__(kBlock) standardize_pass(MomArgs a) {
    __shared__ double lds[kBlock];
    const int p = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const int64_t j0 = (int64_t)c * (kBlock * kItems) + t;
    float v[kItems] = {};
#pragma unroll
    for (int u = 0; u < kItems; ++u) {
        const int64_t j = j0 + (int64_t)u * kBlock;
        if (j < a.n) v[u] = a.x[address(a, j, p)];
    }
    const double mean = combine(partials(a, 0, p), a.chunks, lds) / (double)a.n;
    const double sd = sqrt(variance(a, 1, p, lds));
    const double denom = sd > a.min_std ? sd : a.min_std;
    if (a.moments && c == 0 && t == 0) {
        a.moments[2 * p] = mean;
        a.moments[2 * p + 1] = sd;
    }
#pragma unroll
    for (int u = 0; u < kItems; ++u) {
        const int64_t j = j0 + (int64_t)u * kBlock;
        if (j < a.n) a.out[address(a, j, p)] = (float)(((double)v[u] - mean) / denom);
    }
}

// pass 3 of ssd_explained_variance: one workgroup per set
__global__ void __launch_bounds__(kBlock) explained_variance_pass(MomArgs a) {
    __shared__ double lds[kBlock];
    const int p = blockIdx.x;
    const double var_y = variance(a, 2, p, lds), var_d = variance(a, 3, p, lds);
    const double r = 1.0 - var_d / var_y;
    if (threadIdx.x == 0) a.out[p] = (float)(r < -1.0 ? -1.0 : r);   // (a NaN stays one)
}

thread_local ssd::BatchError g_mom_error;

int fail(const char *msg) { return g_mom_error.invalid(msg); }

// the checks both calls share, then the device; fills what the passes share of `a`
int prepare(int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps, int32_t num_sets, const void *scratch, int32_t device_id,
            MomArgs &a) {
    if (const char *msg = ssd::check_ring(lanes, ring, step0, n_steps)) return fail(msg);
    if (num_sets < 1) return fail("num_sets must be >= 1");
    if (lanes % num_sets != 0) return fail("num_sets must divide lanes: lane l belongs to set l % num_sets");
    if (!scratch) return fail("scratch is required");
    if ((uintptr_t)scratch % sizeof(double) != 0) return fail("scratch must be aligned to 8 bytes");
    const int64_t chunks = SSD_MOM_CHUNKS(n_steps, lanes, num_sets);
    if (chunks > 0x7fffffff || num_sets > 65535) return fail("too many chunks or sets for one grid");
    if (const int rc = ssd::use_device(g_mom_error, device_id)) return rc;
    const int64_t s0 = step0 % ring;
    a.n = (int64_t)n_steps * (lanes / num_sets);
    a.base = s0 * lanes;
    a.split = (ring - s0) * (int64_t)lanes;
    a.P = num_sets;
    a.chunks = (int32_t)chunks;
    a.scratch = (double *)scratch;
    return SSD_OK;
}

bool misaligned(const void *p, size_t to) { return (uintptr_t)p % to != 0; }

}  // namespace

extern "C" {

const char *ssd_moments_last_error(void) { return g_mom_error.c_str(); }

int ssd_standardize(const float *x, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps, int32_t num_sets, double min_std,
                    double *scratch, double *moments, float *out, int32_t device_id, void *stream) {
    if (!x || !out) return fail("x and out are required");
    if (misaligned(x, sizeof(float)) || misaligned(out, sizeof(float))) return fail("x and out must be aligned to 4 bytes");
    if (misaligned(moments, sizeof(double))) return fail("moments must be aligned to 8 bytes");
    if (!isfinite(min_std) || min_std <= 0.0) return fail("min_std must be finite and > 0");
    MomArgs a{};
    const int rc = prepare(lanes, ring, step0, n_steps, num_sets, scratch, device_id, a);
    if (rc != SSD_OK) return rc;
    a.x = x; a.out = out; a.moments = moments; a.min_std = min_std;
    const dim3 grid((unsigned)a.chunks, (unsigned)a.P);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL((moments_pass<1, false>), grid, dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL((moments_pass<1, true>), grid, dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(standardize_pass, grid, dim3(kBlock), 0, s, a);
    return g_mom_error.launched("standardize");
}

int ssd_explained_variance(const float *y, const float *pred, int32_t lanes, int32_t ring, int32_t step0, int32_t n_steps,
                           int32_t num_sets, double *scratch, float *out, int32_t device_id, void *stream) {
    if (!y || !pred || !out) return fail("y, pred and out are required");
    if (misaligned(y, sizeof(float)) || misaligned(pred, sizeof(float)) || misaligned(out, sizeof(float)))
        return fail("y, pred and out must be aligned to 4 bytes");
    MomArgs a{};
    const int rc = prepare(lanes, ring, step0, n_steps, num_sets, scratch, device_id, a);
    if (rc != SSD_OK) return rc;
    a.x = y; a.pred = pred; a.out = out;
    const dim3 grid((unsigned)a.chunks, (unsigned)a.P);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL((moments_pass<2, false>), grid, dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL((moments_pass<2, true>), grid, dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(explained_variance_pass, dim3((unsigned)a.P), dim3(kBlock), 0, s, a);
    return g_mom_error.launched("explained variance");
}

}  // extern "C"
