// ssd_stats.hip -- per-episode statistics of batched rollouts (include/ssd.h, ssd_stats_*), folded on the device from the
// step outputs rew i32 [ring,E,N] (and optionally done u8 [ring,E,N]).  DESIGN.md section 10 states the definitions.
//
// A step's reward decodes into its parts: r = a - f - 50h with a, f in {0,1}, so h = floor((1 - r) / 50) and r > 0 iff a
// step ate an apple with no cost and no hit.  Per open episode and agent the fold keeps R (sum of r), pos (#{r > 0}), tsum
// (sum of the in-episode step index t of those steps), tagged (#{h > 0}) and hits (sum of h); an episode end turns them
// into the four metrics of Perolat et al. 2017 and adds everything to per-env accumulators that ssd_stats_drain hands out.
//
// Work is split over time as well as envs.  Lanes are (env, agent) pairs packed whole envs per wave (64 / N envs of N lanes
// each), so that the agents of one env exchange values with wave shuffles.  Pass 1, one thread per (chunk of L steps, env,
// agent): the partial sums of the chunk's "head" (its steps up to and including its first episode end, or all of it) and
// "tail" (after its last end), and per env the number of ends and where the first and last fall.  Pass 2, one thread per
// (env, agent), walks the chunks in order: it adds a head to the open episode, closes it at the first end, re-reads the steps
// between the first and the last end of a chunk that holds more than one (episodes shorter than a chunk), and opens the tail.
// Every float operation -- the metrics and their sums -- happens in pass 2 in the order a sequential loop over the steps
// would do it, so the results do not depend on L.  There are no atomics; integers stay integers until a metric is formed.
// L, the number of chunks, both grids and the scratch carve come from ssd_stats_plan.hpp (no HIP, 64-bit, tested on the host).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string>

#include "../../include/ssd.h"
#include "ssd_stats_plan.hpp"

namespace {

namespace plan = ssd::stats_plan;                                // L, C, the grids and the scratch: decided there, in 64 bits
using plan::kBlock;
using plan::kWave;
constexpr int kBatch = 8;                                        // pass 1: steps whose loads are issued together

struct Seg {                                                     // sums of one agent over a run of steps
    int64_t R, tsum, hits, pos, tagged;
};

struct Part {                                                    // pass-1 output: SoA [chunk][E*N] (pos, tagged <= L)
    int64_t *R, *tsum, *hits;
    int32_t *pos, *tagged;
};

struct StatsDev {                                                // persistent state; [E] per env, [E*N] per (env, agent)
    // the open episode
    int64_t *t;                                                  // [E] steps so far
    int64_t *oR, *otsum, *ohits, *opos, *otagged;                // [E*N]
    // accumulators since the last drain
    int64_t *episodes, *truncated, *sum_len, *sum_coll;          // [E]
    int64_t *sum_ret, *sum_hits, *sum_tagged;                    // [E*N]
    double *msum;                                                // [4][E]: efficiency, equality, sustainability, peace
    int64_t *mcnt;                                               // [4][E]: finite values among them
    int64_t *last_len;                                           // [E] 0: no episode ended since the last drain
    int64_t *last_R;                                             // [E*N]
    double *last_m;                                              // [4][E]
};

struct Lanes {                                                   // the (env, agent) of a thread within its wave
    int e, i, base;                                              // base: the wave lane of agent 0 of env e
    bool ok;
};

__device__ __forceinline__ Lanes lanes_of(int wave_in_row, int lane, int E, int N) {
    const int per = kWave / N;                                   // envs per wave
    Lanes l;
    const int g = lane / N;
    l.i = lane - g * N;
    l.e = wave_in_row * per + g;
    l.base = g * N;
    l.ok = g < per && l.e < E;
    return l;
}

__device__ __forceinline__ int64_t hits_of(int32_t r) {          // floor((1 - r) / 50)
    const int64_t x = 1 - (int64_t)r;
    return x >= 0 ? x / 50 : -((-x + 49) / 50);
}

__device__ __forceinline__ void seg_add(Seg &s, int32_t r, int64_t t) {
    const int64_t h = hits_of(r);
    s.R += r;
    s.hits += h;
    if (r > 0) { s.pos += 1; s.tsum += t; }
    if (h > 0) s.tagged += 1;
}

__device__ __forceinline__ bool ends_at(const uint8_t *done, size_t slot_off, int e, int N, int64_t g1, int32_t reset_every) {
    // g1 = step0 + k + 1 of the step at fold index k
    if (done && done[slot_off + (size_t)e * N] != 0) return true;
    return reset_every > 0 && g1 % reset_every == 0;
}

// ---------------------------------------------------------------- pass 1: chunk partials
__global__ void __launch_bounds__(kBlock) stats_chunk_kernel(const int32_t *__restrict__ rew, const uint8_t *__restrict__ done,
                                                             int32_t ring, int32_t step0, int32_t n_steps, int32_t reset_every,
                                                             int32_t E, int32_t N, int32_t L, int32_t C, int32_t waves_per_row,
                                                             Part head, Part tail, int4 *__restrict__ meta) {
    const int wave = (int)((blockIdx.x * (unsigned)kBlock + threadIdx.x) / kWave);
    const int c = wave / waves_per_row;
    const Lanes l = lanes_of(wave - c * waves_per_row, threadIdx.x % kWave, E, N);
    if (!l.ok || !plan::wave_has_chunk(c, C)) return;            // (the spare waves of the last block: no product of c to wrap)
    // k0 < k1 <= n_steps fit an int; the batch loop runs up to 7 past k1, and n_steps may be INT32_MAX: 64 bits
    const int64_t k0 = plan::chunk_begin(c, L), k1 = plan::chunk_end(k0, L, n_steps);
    const size_t EN = (size_t)E * N, lane_off = (size_t)l.e * N + l.i;
    int slot = (int)(((int64_t)step0 + k0) % ring);
    Seg cur = {0, 0, 0, 0, 0}, hd = cur;
    int64_t t = 0;
    int nb = 0, first = -1, last = -1;
    for (int64_t kb = k0; kb < k1; kb += kBatch) {
        // the batch's loads first (they do not depend on the sums), then the steps in order
        int32_t r[kBatch];
        bool end[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int64_t k = kb + u;
            const size_t off = (size_t)slot * EN;
            r[u] = k < k1 ? rew[off + lane_off] : 0;
            end[u] = k < k1 && ends_at(done, off, l.e, N, plan::global_step1(step0, k), reset_every);
            if (++slot == ring) slot = 0;
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int64_t k = kb + u;
            if (k >= k1) break;
            seg_add(cur, r[u], ++t);
            if (end[u]) {
                if (nb == 0) { hd = cur; first = (int)k; }
                last = (int)k;
                ++nb;
                cur = Seg{0, 0, 0, 0, 0};
                t = 0;
            }
        }
    }
    if (nb == 0) hd = cur;
    const size_t o = (size_t)c * EN + lane_off;
    head.R[o] = hd.R; head.tsum[o] = hd.tsum; head.hits[o] = hd.hits; head.pos[o] = (int32_t)hd.pos; head.tagged[o] = (int32_t)hd.tagged;
    if (nb > 0) {
        tail.R[o] = cur.R; tail.tsum[o] = cur.tsum; tail.hits[o] = cur.hits; tail.pos[o] = (int32_t)cur.pos; tail.tagged[o] = (int32_t)cur.tagged;
    }
    if (l.i == 0) meta[(size_t)c * E + l.e] = make_int4(nb, first, last, 0);
}

// ---------------------------------------------------------------- pass 2: chunks in order, episodes closed
struct Acc {                                                     // one lane's copy of its env's accumulators, and its agent's
    int64_t episodes, truncated, sum_len, sum_coll;
    double msum[4];
    int64_t mcnt[4];
    int64_t last_len;
    double last_m[4];
    int64_t sum_ret, sum_hits, sum_tagged, last_R;
};

template <typename T>
__device__ __forceinline__ T from_lane(T v, int src) { return __shfl(v, src, kWave); }

// Close the open episode of T steps: every lane of the env computes the same metrics (sums over agents in index order).
__device__ void close_episode(Acc &a, const Seg &s, int64_t T, const Lanes &l, int N) {
    int64_t C = 0, tag = 0, g = 0;
    double ssum = 0.0;
    int64_t scnt = 0;
    for (int j = 0; j < N; ++j) {
        const int64_t Rj = from_lane(s.R, l.base + j);
        const int64_t tj = from_lane(s.tsum, l.base + j);
        const int64_t pj = from_lane(s.pos, l.base + j);
        C += Rj;
        tag += from_lane(s.tagged, l.base + j);
        g += s.R >= Rj ? s.R - Rj : Rj - s.R;                    // this agent's row of the Gini sum
        if (pj > 0) { ssum = ssum + (double)tj / (double)pj; ++scnt; }
    }
    int64_t G = 0;
    for (int j = 0; j < N; ++j) G += from_lane(g, l.base + j);
    double m[4];
    m[0] = (double)C / (double)T;
    m[1] = 1.0 - (double)G / (double)(2 * (int64_t)N * C);
    m[2] = ssum / (double)scnt;
    m[3] = (double)((int64_t)N * T - tag) / (double)T;
    a.episodes += 1;
    a.sum_len += T;
    a.sum_coll += C;
    for (int q = 0; q < 4; ++q) {
        if (isfinite(m[q])) { a.msum[q] = a.msum[q] + m[q]; a.mcnt[q] += 1; }
        a.last_m[q] = m[q];
    }
    a.last_len = T;
    a.sum_ret += s.R;
    a.sum_hits += s.hits;
    a.sum_tagged += s.tagged;
    a.last_R = s.R;
}

__device__ __forceinline__ void add_shifted(Seg &o, const Part &p, size_t idx, int64_t t) {
    // a chunk's partial, whose step indices count from 1 at the chunk start, appended to an open episode of t steps
    const int32_t pos = p.pos[idx];
    o.R += p.R[idx];
    o.tsum += p.tsum[idx] + (int64_t)pos * t;
    o.hits += p.hits[idx];
    o.pos += pos;
    o.tagged += p.tagged[idx];
}

__global__ void __launch_bounds__(kBlock) stats_combine_kernel(StatsDev d, const int32_t *__restrict__ rew,
                                                               const uint8_t *__restrict__ done, int32_t ring, int32_t step0,
                                                               int32_t n_steps, int32_t reset_every, int32_t E, int32_t N, int32_t L,
                                                               int32_t C, Part head, Part tail, const int4 *__restrict__ meta) {
    const int wave = (int)((blockIdx.x * (unsigned)kBlock + threadIdx.x) / kWave);
    const Lanes l = lanes_of(wave, threadIdx.x % kWave, E, N);
    if (!l.ok) return;
    const int e = l.e;
    const size_t EN = (size_t)E * N, li = (size_t)e * N + l.i;
    Acc a;
    a.episodes = d.episodes[e]; a.truncated = d.truncated[e]; a.sum_len = d.sum_len[e]; a.sum_coll = d.sum_coll[e];
    for (int q = 0; q < 4; ++q) {
        a.msum[q] = d.msum[(size_t)q * E + e]; a.mcnt[q] = d.mcnt[(size_t)q * E + e]; a.last_m[q] = d.last_m[(size_t)q * E + e];
    }
    a.last_len = d.last_len[e];
    a.sum_ret = d.sum_ret[li]; a.sum_hits = d.sum_hits[li]; a.sum_tagged = d.sum_tagged[li]; a.last_R = d.last_R[li];
    int64_t t = d.t[e];
    Seg o = {d.oR[li], d.otsum[li], d.ohits[li], d.opos[li], d.otagged[li]};
    if (reset_every > 0 && step0 % reset_every == 0 && t > 0) {  // the rollout resets every env before its first step
        a.truncated += 1;
        t = 0;
        o = Seg{0, 0, 0, 0, 0};
    }
    for (int c = 0; c < C; ++c) {
        const int4 mt = meta[(size_t)c * E + e];
        const int k0 = (int)plan::chunk_begin(c, L), k1 = (int)plan::chunk_end(k0, L, n_steps);   // k0 < k1 <= n_steps
        const size_t pi = (size_t)c * EN + li;
        add_shifted(o, head, pi, t);
        if (mt.x == 0) { t += k1 - k0; continue; }
        close_episode(a, o, t + (mt.y - k0 + 1), l, N);
        o = Seg{0, 0, 0, 0, 0};
        t = 0;
        if (mt.x > 1) {                                          // episodes that start and end inside this chunk: re-read them
            int slot = (int)(((int64_t)step0 + mt.y + 1) % ring);
            for (int k = mt.y + 1; k <= mt.z; ++k) {
                const size_t off = (size_t)slot * EN;
                seg_add(o, rew[off + li], ++t);
                if (ends_at(done, off, e, N, plan::global_step1(step0, k), reset_every)) {
                    close_episode(a, o, t, l, N);
                    o = Seg{0, 0, 0, 0, 0};
                    t = 0;
                }
                if (++slot == ring) slot = 0;
            }
        }
        o = Seg{tail.R[pi], tail.tsum[pi], tail.hits[pi], tail.pos[pi], tail.tagged[pi]};
        t = k1 - 1 - mt.z;
    }
    d.oR[li] = o.R; d.otsum[li] = o.tsum; d.ohits[li] = o.hits; d.opos[li] = o.pos; d.otagged[li] = o.tagged;
    d.sum_ret[li] = a.sum_ret; d.sum_hits[li] = a.sum_hits; d.sum_tagged[li] = a.sum_tagged; d.last_R[li] = a.last_R;
    if (l.i == 0) {
        d.t[e] = t;
        d.episodes[e] = a.episodes; d.truncated[e] = a.truncated; d.sum_len[e] = a.sum_len; d.sum_coll[e] = a.sum_coll;
        for (int q = 0; q < 4; ++q) {
            d.msum[(size_t)q * E + e] = a.msum[q]; d.mcnt[(size_t)q * E + e] = a.mcnt[q]; d.last_m[(size_t)q * E + e] = a.last_m[q];
        }
        d.last_len[e] = a.last_len;
    }
}

// ---------------------------------------------------------------- discard / drain
__global__ void __launch_bounds__(kBlock) stats_discard_kernel(StatsDev d, const uint8_t *__restrict__ mask, int32_t E, int32_t N) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= E || (mask && mask[e] == 0) || d.t[e] == 0) return;
    d.truncated[e] += 1;
    d.t[e] = 0;
    for (int i = 0; i < N; ++i) {
        const size_t li = (size_t)e * N + i;
        d.oR[li] = 0; d.otsum[li] = 0; d.ohits[li] = 0; d.opos[li] = 0; d.otagged[li] = 0;
    }
}

__global__ void __launch_bounds__(kBlock) stats_drain_kernel(StatsDev d, int32_t E, int32_t N, int64_t *counts, int64_t *agent_sums,
                                                             double *metric_sums, int64_t *metric_counts, int64_t *last_len,
                                                             int64_t *last_ret, double *last_metrics, int keep) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    if (counts) {
        counts[(size_t)e * 4 + 0] = d.episodes[e]; counts[(size_t)e * 4 + 1] = d.truncated[e];
        counts[(size_t)e * 4 + 2] = d.sum_len[e]; counts[(size_t)e * 4 + 3] = d.sum_coll[e];
    }
    for (int q = 0; q < 4; ++q) {
        if (metric_sums) metric_sums[(size_t)e * 4 + q] = d.msum[(size_t)q * E + e];
        if (metric_counts) metric_counts[(size_t)e * 4 + q] = d.mcnt[(size_t)q * E + e];
        if (last_metrics) last_metrics[(size_t)e * 4 + q] = d.last_m[(size_t)q * E + e];
    }
    if (last_len) last_len[e] = d.last_len[e];
    for (int i = 0; i < N; ++i) {
        const size_t li = (size_t)e * N + i;
        if (agent_sums) {
            agent_sums[((size_t)e * 3 + 0) * N + i] = d.sum_ret[li];
            agent_sums[((size_t)e * 3 + 1) * N + i] = d.sum_hits[li];
            agent_sums[((size_t)e * 3 + 2) * N + i] = d.sum_tagged[li];
        }
        if (last_ret) last_ret[li] = d.last_R[li];
    }
    if (keep) return;
    d.episodes[e] = 0; d.truncated[e] = 0; d.sum_len[e] = 0; d.sum_coll[e] = 0; d.last_len[e] = 0;
    for (int q = 0; q < 4; ++q) { d.msum[(size_t)q * E + e] = 0.0; d.mcnt[(size_t)q * E + e] = 0; d.last_m[(size_t)q * E + e] = 0.0; }
    for (int i = 0; i < N; ++i) {
        const size_t li = (size_t)e * N + i;
        d.sum_ret[li] = 0; d.sum_hits[li] = 0; d.sum_tagged[li] = 0; d.last_R[li] = 0;
    }
}

std::string g_stats_create_error;

}  // namespace

struct ssd_stats {
    int32_t E, N, device, chunk;                                 // chunk: steps per pass-1 chunk, 0 = automatic
    StatsDev d;
    void *block;                                                 // the persistent state
    void *scratch;                                               // pass-1 partials, grown on demand
    size_t scratch_bytes;
    std::string err;
};

namespace {

int stats_fail(ssd_stats *st, const char *what, hipError_t e) {
    st->err = std::string(what) + ": " + hipGetErrorString(e);
    return SSD_E_DEVICE;
}

#define ST_HIP(st, call)                                                   \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) return stats_fail((st), #call, e_);          \
    } while (0)

Part carve_part(char *&c, size_t lanes) {
    Part p;
    p.R = (int64_t *)c; c += lanes * 8;
    p.tsum = (int64_t *)c; c += lanes * 8;
    p.hits = (int64_t *)c; c += lanes * 8;
    p.pos = (int32_t *)c; c += lanes * 4;
    p.tagged = (int32_t *)c; c += lanes * 4;
    return p;
}

}  // namespace

extern "C" {

const char *ssd_stats_last_error(const ssd_stats *st) { return st ? st->err.c_str() : g_stats_create_error.c_str(); }

int ssd_stats_create(int32_t num_envs, int32_t num_agents, int32_t device_id, ssd_stats **out) {
    if (!out) { g_stats_create_error = "null argument"; return SSD_E_INVALID; }
    *out = nullptr;
    if (num_envs < 1 || num_envs > (1 << 26)) { g_stats_create_error = "num_envs must be 1..2^26"; return SSD_E_INVALID; }
    if (num_agents < 1 || num_agents > 64) { g_stats_create_error = "num_agents must be 1..64"; return SSD_E_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_stats_create_error = "no HIP device available: this engine has no CPU path";
        return SSD_E_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { g_stats_create_error = "device_id out of range"; return SSD_E_INVALID; }
    if (hipSetDevice(device_id) != hipSuccess) { g_stats_create_error = "hipSetDevice failed"; return SSD_E_DEVICE; }
    ssd_stats *st = new ssd_stats();
    st->E = num_envs; st->N = num_agents; st->device = device_id; st->chunk = 0;
    st->scratch = nullptr; st->scratch_bytes = 0;
    const size_t E = (size_t)num_envs, EN = E * num_agents;
    // every array is 8-byte: [E] x 6 + [4][E] x 3 + [E*N] x 9
    const size_t bytes = 8 * (E * 6 + 4 * E * 3 + EN * 9);
    if (hipMalloc(&st->block, bytes) != hipSuccess) {
        g_stats_create_error = "hipMalloc failed";
        delete st;
        return SSD_E_NOMEM;
    }
    char *c = static_cast<char *>(st->block);
    auto i64 = [&](size_t n) { int64_t *r = (int64_t *)c; c += n * 8; return r; };
    auto f64 = [&](size_t n) { double *r = (double *)c; c += n * 8; return r; };
    StatsDev &d = st->d;
    d.t = i64(E); d.episodes = i64(E); d.truncated = i64(E); d.sum_len = i64(E); d.sum_coll = i64(E); d.last_len = i64(E);
    d.msum = f64(4 * E); d.mcnt = i64(4 * E); d.last_m = f64(4 * E);
    d.oR = i64(EN); d.otsum = i64(EN); d.ohits = i64(EN); d.opos = i64(EN); d.otagged = i64(EN);
    d.sum_ret = i64(EN); d.sum_hits = i64(EN); d.sum_tagged = i64(EN); d.last_R = i64(EN);
    if (hipMemset(st->block, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        g_stats_create_error = "device initialisation failed";
        (void)hipFree(st->block);
        delete st;
        return SSD_E_DEVICE;
    }
    *out = st;
    return SSD_OK;
}

int ssd_stats_destroy(ssd_stats *st) {
    if (!st) return SSD_E_INVALID;
    (void)hipSetDevice(st->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(st->block);
    if (st->scratch) (void)hipFree(st->scratch);
    delete st;
    return SSD_OK;
}

int ssd_stats_set_chunk(ssd_stats *st, int32_t steps) {
    if (!st) return SSD_E_INVALID;
    if (steps < 0) { st->err = "chunk must be >= 0"; return SSD_E_INVALID; }
    st->chunk = steps;
    return SSD_OK;
}

int ssd_stats_fold(ssd_stats *st, const int32_t *rew, const uint8_t *done, int32_t ring, int32_t step0, int32_t n_steps,
                   int32_t reset_every, uint32_t flags, void *stream) {
    if (!st) return SSD_E_INVALID;
    if (!rew || ring < 1 || n_steps < 0 || step0 < 0 || reset_every < 0) { st->err = "bad fold arguments"; return SSD_E_INVALID; }
    if (n_steps > ring) { st->err = "n_steps > ring: a fold reads each step's slot once"; return SSD_E_INVALID; }
    if (flags != 0) { st->err = "unsupported flag"; return SSD_E_INVALID; }
    if (n_steps == 0) return SSD_OK;
    ST_HIP(st, hipSetDevice(st->device));
    const hipStream_t s = (hipStream_t)stream;
    plan::Plan p;
    if (!plan::plan_fold(st->E, st->N, n_steps, st->chunk, p)) { st->err = p.why; return SSD_E_INVALID; }
    static_assert(sizeof(int4) == plan::kMetaBytes, "the plan's meta record");
    const size_t need = p.scratch_bytes;
    if (need > st->scratch_bytes) {
        // the partials of the previous fold may still be read on another stream: wait before the buffer goes
        ST_HIP(st, hipDeviceSynchronize());
        if (st->scratch) { (void)hipFree(st->scratch); st->scratch = nullptr; st->scratch_bytes = 0; }
        if (hipMalloc(&st->scratch, need) != hipSuccess) { st->err = "hipMalloc of the fold's scratch failed"; return SSD_E_NOMEM; }
        st->scratch_bytes = need;
    }
    char *c = static_cast<char *>(st->scratch);
    int4 *meta = (int4 *)c; c += p.meta_bytes;
    const Part head = carve_part(c, p.part_lanes), tail = carve_part(c, p.part_lanes);
    stats_chunk_kernel<<<p.grid1, kBlock, 0, s>>>(rew, done, ring, step0, n_steps, reset_every, st->E, st->N, p.L, p.C, p.rows, head,
                                                  tail, meta);
    ST_HIP(st, hipGetLastError());
    stats_combine_kernel<<<p.grid2, kBlock, 0, s>>>(st->d, rew, done, ring, step0, n_steps, reset_every, st->E, st->N, p.L, p.C, head,
                                                    tail, meta);
    ST_HIP(st, hipGetLastError());
    return SSD_OK;
}

int ssd_stats_discard(ssd_stats *st, const uint8_t *env_mask, void *stream) {
    if (!st) return SSD_E_INVALID;
    ST_HIP(st, hipSetDevice(st->device));
    stats_discard_kernel<<<(st->E + kBlock - 1) / kBlock, kBlock, 0, (hipStream_t)stream>>>(st->d, env_mask, st->E, st->N);
    ST_HIP(st, hipGetLastError());
    return SSD_OK;
}

int ssd_stats_drain(ssd_stats *st, int64_t *counts, int64_t *agent_sums, double *metric_sums, int64_t *metric_counts,
                    int64_t *last_len, int64_t *last_ret, double *last_metrics, uint32_t flags, void *stream) {
    if (!st) return SSD_E_INVALID;
    if ((flags & ~(uint32_t)SSD_STATS_KEEP) != 0) { st->err = "unsupported flag"; return SSD_E_INVALID; }
    ST_HIP(st, hipSetDevice(st->device));
    stats_drain_kernel<<<(st->E + kBlock - 1) / kBlock, kBlock, 0, (hipStream_t)stream>>>(
        st->d, st->E, st->N, counts, agent_sums, metric_sums, metric_counts, last_len, last_ret, last_metrics,
        (flags & SSD_STATS_KEEP) ? 1 : 0);
    ST_HIP(st, hipGetLastError());
    return SSD_OK;
}

}  // extern "C"
