// ssd_ws_stats.hip -- the Watershed episode-statistics handle (include/ssd.h, ssd_ws_stats_*): its
// allocation, the discard and drain kernels and the C ABI.  The folding itself happens in the stepping kernel's stats instances
// (ssd_watershed.hip) through the lane pieces of ssd_ws_stats.hpp.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string>

#include "../../include/ssd.h"
#include "ssd_ws_stats.hpp"

namespace {

using ssd::WsStatsDev;

constexpr int kBlock = 256;

__device__ __forceinline__ void clear_accumulators(const WsStatsDev &d, int e) {
    for (int s = ssd::WSS_COUNTS; s < ssd::WSS_SLOTS8; ++s) *d.i64(s, e) = 0;            // +0.0 and 0 are the same bits
    for (int m = 0; m < 3; ++m) {
        *d.f64(ssd::WSS_M_MIN + m, e) = INFINITY;
        *d.f64(ssd::WSS_M_MAX + m, e) = -INFINITY;
    }
}

__global__ void __launch_bounds__(kBlock) ws_stats_init_kernel(WsStatsDev d) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < d.E) clear_accumulators(d, e);
}

__global__ void __launch_bounds__(kBlock) ws_stats_discard_kernel(WsStatsDev d, const uint8_t *mask, int reopen) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= d.E || (mask && !mask[e])) return;
    if (d.open[e] && *d.i32(ssd::WSS_O_LEN, e) > 0) *d.i64(ssd::WSS_COUNTS + 1, e) += 1;
    d.open[e] = reopen ? 1 : 0;
    for (int s = 0; s < ssd::WSS_SLOTS4; ++s) *d.i32(s, e) = 0;
    for (int s = ssd::WSS_O_REW; s < ssd::WSS_COUNTS; ++s) *d.f64(s, e) = 0.0;
}

struct DrainOut {
    int64_t *counts, *metric_counts, *last_len;
    double *reward_sum, *agent_sums, *metric_sums, *metric_min, *metric_max, *last_reward, *last_agent, *last_total_rews, *last_metrics;
};

// [n][E] -> [E,n]
__device__ __forceinline__ void put(const WsStatsDev &d, int e, int slot, int n, double *out) {
    if (out)
        for (int j = 0; j < n; ++j) out[(size_t)e * n + j] = *d.f64(slot + j, e);
}
__device__ __forceinline__ void put(const WsStatsDev &d, int e, int slot, int n, int64_t *out) {
    if (out)
        for (int j = 0; j < n; ++j) out[(size_t)e * n + j] = *d.i64(slot + j, e);
}

__global__ void __launch_bounds__(kBlock) ws_stats_drain_kernel(WsStatsDev d, DrainOut o, int keep) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= d.E) return;
    put(d, e, ssd::WSS_COUNTS, 3, o.counts);
    put(d, e, ssd::WSS_REW_SUM, 1, o.reward_sum);
    put(d, e, ssd::WSS_AGENT_SUMS, 8, o.agent_sums);
    put(d, e, ssd::WSS_M_SUM, 3, o.metric_sums);
    put(d, e, ssd::WSS_M_CNT, 3, o.metric_counts);
    put(d, e, ssd::WSS_M_MIN, 3, o.metric_min);
    put(d, e, ssd::WSS_M_MAX, 3, o.metric_max);
    put(d, e, ssd::WSS_L_LEN, 1, o.last_len);
    put(d, e, ssd::WSS_L_REW, 1, o.last_reward);
    put(d, e, ssd::WSS_L_AGENT, 8, o.last_agent);
    put(d, e, ssd::WSS_L_TOT, 4, o.last_total_rews);
    put(d, e, ssd::WSS_L_MET, 3, o.last_metrics);
    if (!keep) clear_accumulators(d, e);
}

std::string g_create_error;

int grid(const ssd_ws_stats *st) { return (st->d.E + kBlock - 1) / kBlock; }

int fail(ssd_ws_stats *st, const char *what, hipError_t e) {
    st->err = std::string(what) + ": " + hipGetErrorString(e);
    return SSD_E_DEVICE;
}

}  // namespace

namespace ssd {

int ws_stats_discard(ssd_ws_stats *st, const uint8_t *env_mask, bool reopen, void *stream) {
    ws_stats_discard_kernel<<<grid(st), kBlock, 0, (hipStream_t)stream>>>(st->d, env_mask, reopen ? 1 : 0);
    return (int)hipGetLastError();
}

}  // namespace ssd

extern "C" {

const char *ssd_ws_stats_last_error(const ssd_ws_stats *st) { return st ? st->err.c_str() : g_create_error.c_str(); }

int ssd_ws_stats_create(int32_t variant, int32_t num_envs, int32_t device_id, ssd_ws_stats **out) {
    if (!out) { g_create_error = "null argument"; return SSD_E_INVALID; }
    *out = nullptr;
    if (variant != SSD_WS_SEQ && variant != SSD_WS_SEQ_COMM) { g_create_error = "unknown variant"; return SSD_E_INVALID; }
    if (num_envs < 1 || num_envs > (1 << 26)) { g_create_error = "num_envs must be 1..2^26"; return SSD_E_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_error = "no HIP device available: the statistics have no CPU path";
        return SSD_E_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { g_create_error = "device_id out of range"; return SSD_E_INVALID; }
    if (hipSetDevice(device_id) != hipSuccess) { g_create_error = "hipSetDevice failed"; return SSD_E_DEVICE; }
    ssd_ws_stats *st = new ssd_ws_stats();
    st->variant = variant; st->device = device_id; st->attached = 0;
    const size_t E = (size_t)num_envs;
    const size_t bytes = E * 8 * ssd::WSS_SLOTS8 + E * 4 * ssd::WSS_SLOTS4 + E;          // 8-byte fields first: all stay aligned
    if (hipMalloc(&st->block, bytes) != hipSuccess) {
        g_create_error = "hipMalloc failed";
        delete st;
        return SSD_E_NOMEM;
    }
    WsStatsDev &d = st->d;
    d.E = num_envs;
    d.q8 = static_cast<char *>(st->block);
    d.q4 = reinterpret_cast<int32_t *>(d.q8 + E * 8 * ssd::WSS_SLOTS8);
    d.open = reinterpret_cast<uint8_t *>(d.q4 + E * ssd::WSS_SLOTS4);
    hipError_t e = hipMemset(st->block, 0, bytes);
    if (e == hipSuccess) {
        ws_stats_init_kernel<<<grid(st), kBlock>>>(d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        g_create_error = std::string("device initialisation failed: ") + hipGetErrorString(e);
        (void)hipFree(st->block);
        delete st;
        return SSD_E_DEVICE;
    }
    *out = st;
    return SSD_OK;
}

int ssd_ws_stats_destroy(ssd_ws_stats *st) {
    if (!st) return SSD_E_INVALID;
    if (st->attached > 0) { st->err = "still attached to an engine: detach it first (ssd_ws_stats_attach(env, NULL))"; return SSD_E_INVALID; }
    (void)hipSetDevice(st->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(st->block);
    delete st;
    return SSD_OK;
}

int ssd_ws_stats_discard(ssd_ws_stats *st, const uint8_t *env_mask, void *stream) {
    if (!st) return SSD_E_INVALID;
    hipError_t e = hipSetDevice(st->device);
    if (e != hipSuccess) return fail(st, "hipSetDevice", e);
    e = (hipError_t)ssd::ws_stats_discard(st, env_mask, false, stream);
    if (e != hipSuccess) return fail(st, "discard launch", e);
    return SSD_OK;
}

int ssd_ws_stats_drain(ssd_ws_stats *st, int64_t *counts, double *reward_sum, double *agent_sums, double *metric_sums,
                       int64_t *metric_counts, double *metric_min, double *metric_max, int64_t *last_len, double *last_reward,
                       double *last_agent, double *last_total_rews, double *last_metrics, uint32_t flags, void *stream) {
    if (!st) return SSD_E_INVALID;
    if ((flags & ~(uint32_t)SSD_STATS_KEEP) != 0) { st->err = "unsupported flag"; return SSD_E_INVALID; }
    hipError_t e = hipSetDevice(st->device);
    if (e != hipSuccess) return fail(st, "hipSetDevice", e);
    DrainOut o;
    o.counts = counts; o.metric_counts = metric_counts; o.last_len = last_len;
    o.reward_sum = reward_sum; o.agent_sums = agent_sums; o.metric_sums = metric_sums; o.metric_min = metric_min;
    o.metric_max = metric_max; o.last_reward = last_reward; o.last_agent = last_agent; o.last_total_rews = last_total_rews;
    o.last_metrics = last_metrics;
    ws_stats_drain_kernel<<<grid(st), kBlock, 0, (hipStream_t)stream>>>(st->d, o, (flags & SSD_STATS_KEEP) ? 1 : 0);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(st, "drain launch", e);
    return SSD_OK;
}

}  // extern "C"
