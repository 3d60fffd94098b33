// csrc/ssd_rollout.hip -- ssd_rollout_random and ssd_rollout_actions: the same launches, through the library's own dispatch queues
// (ssd_aql.hip; what goes out is decided in ssd_rollout_plan.hpp, this file does it) or, where those are not taken, through HIP
// streams with one chain worker per extra chain.
#include <hip/hip_runtime.h>

#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ssd.h"
#include "ssd_internal.hpp"
#include "ssd_env.hpp"
#include "ssd_aql.hpp"
#include "ssd_rollout_plan.hpp"

using ssd::Params;
namespace plan = ssd::plan;

// One persistent host thread per extra rollout chain (ssd_rollout_random / ssd_rollout_actions through HIP streams).  Created on the first multi-chain call, bound
// to the handle's device once, then parked: a job is handed over through `state` (0 idle, 1 posted, 2 finished, 3 quit).
// After a job the thread keeps polling for the next one for a short while before it sleeps on the condition variable, so a
// loop of short rollout calls (rollout.py:58-70 called per training iteration) pays neither a thread creation + per-thread
// HIP initialisation (~250 us per call: round 1) nor a futex wake-up per call.
struct ChainJob {
    int chain = 0, e_begin = 0, e_end = 0;
    int32_t num_actions = 0, n_steps = 0, reset_every = 0, step0 = 0, ring = 1;
    // caller-supplied actions (ssd_rollout_actions): i32 [action_ring][E][N], step k reads slot (step0 + k) % action_ring;
    // null: every step draws its actions on the device (ssd_rollout_random)
    const int32_t *actions = nullptr; int32_t action_ring = 0;
    const uint8_t *order = nullptr;                  // [action_ring][E][N] action-dict orders (null: index order), same slots
    uint8_t *obs = nullptr; int32_t *rew = nullptr; uint8_t *done = nullptr;
    uint32_t flags = 0;
    hipStream_t s = nullptr;
};
struct ChainWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<int> state{0};
    ChainJob job;
    int rc = 0;
};

// ssd_rollout_random's own dispatch path (ssd_aql.hip): one HSA queue per chain; per (chain, ring slot) the kernel arguments of
// the step launch and of the reset launch, written once into device memory and reused by every packet ("sets", keyed by what
// the caller passed); a small ring of HSA signals for the fork from the caller's stream.
struct AqlState : plan::SplitBuffers {          // (the buffers of split rollouts: world_buf, agents_buf, beam_list, snap_grid, mid_*)
    bool tried = false, ok = false;
    ssd::aql::Queue *q[8] = {};
    int nq = 0;
    static constexpr int kForks = 16;
    uint64_t fork_sig[kForks] = {};
    uint64_t fork_used[kForks][8] = {};             // index of the packet that waits for the fork, per chain (+1; 0 = unused)
    int fork_next = 0;
    unsigned long long *fork_counter = nullptr;     // device memory: += 1 by a one-wave kernel on the caller's stream per forked call
    unsigned long long forks = 0;
    uint8_t *fork_kernarg = nullptr;                // host kernarg memory: kForks blocks of kForkBlock bytes (the chains' waiting kernel)
    static constexpr size_t kForkBlock = 256;
    ssd::aql::Kernel wait_kernel{};
    unsigned long long *join_counter = nullptr;     // device memory: += 1 by every chain's last packet of a call
    unsigned long long joins = 0;                   // value it reaches when everything enqueued so far is done
    void *flag_kernarg = nullptr;                   // host kernarg block: the flag kernel's argument (= join_counter)
    // the join's stream-side wait gave up (SSD_ST_WAIT_TIMEOUT): set by that kernel in host memory, so that the handle's next call
    // sees it without a device round trip; STICKY until ssd_synchronize or the next rollout call has reported it (after_timeout)
    uint32_t *timed_out_host = nullptr, *timed_out_dev = nullptr;
    using Key = plan::Key;
    struct Geo { ssd::aql::Kernel k; uint32_t grid_x = 0, block_x = 0, lds = 0; };
    struct Set {
        bool valid = false;
        Key key;
        uint8_t *dev = nullptr;                     // [chains][slots][n_dense] blocks of kBlock bytes; a long set: then [chains][slots][n_long] of kLongBlock
        size_t cap = 0;
        Geo geo[8][plan::kAllKinds];                // per chain and kind
        plan::KindTable kinds;                      // the kinds the key's calls can use, and their blocks' places in one (chain, slot)
        plan::LongKindTable long_kinds;             // ... and the long kinds' (a long set's; else none)
        size_t long_at = 0;                         // where the long blocks begin
        // the argument block of a packet: chain c, block index `block`, kind
        uint8_t *block_of(int c, size_t block, int kind) const {
            if (plan::is_long_kind(kind))
                return dev + long_at + (((size_t)c * key.slots + block) * long_kinds.n_dense + long_kinds.dense[kind - plan::kKinds]) * kLongBlock;
            return dev + (((size_t)c * key.slots + block) * kinds.n_dense + kinds.dense[kind]) * kBlock;
        }
        uint64_t last_use[8] = {};                  // index of the last join packet after a use, per chain (+1)
        uint64_t stamp = 0;
    };
    static constexpr int kSets = 4;
    static constexpr size_t kBlock = 896;           // >= sizeof(ssd::PairKernArgs), a multiple of 64
    static constexpr size_t kLongBlock = 1216;      // >= sizeof(ssd::LongKernArgs), a multiple of 64
    bool long_tried = false;                        // the long mid sets were asked for once (SplitBuffers::long_*: all there, or none)
    Set sets[kSets];
    uint64_t clock = 0;
};
static_assert(AqlState::kBlock >= sizeof(ssd::PairKernArgs), "an argument block holds the largest kernarg segment");
static_assert(AqlState::kLongBlock >= sizeof(ssd::LongKernArgs) && AqlState::kLongBlock % 64 == 0, "a long block holds a long launch's kernarg segment");

void RolloutDelete::operator()(ChainWorker *w) const { delete w; }
void RolloutDelete::operator()(AqlState *a) const { delete a; }

// The launches of step k of a plain (not fused) chain: a full reset when one is due, then the step.
struct ChainCursor : plan::ChainRings {          // (the chain's output and action rings: obs, rew, done, actions, order, ...)
    Params p;
    hipStream_t s;
    int32_t reset_every, step0, ring;
};
using plan::cursor_actions;
static ChainCursor chain_cursor(const ssd_env *env, const ChainJob &j) {
    ChainCursor c;
    const bool f32 = (j.flags & SSD_OBS_F32) != 0;
    c.p = env->p;
    c.p.obs_f32 = f32 ? 1 : 0;
    c.p.e_begin = j.e_begin; c.p.E = j.e_end;
    c.s = j.s; c.obs = j.obs; c.rew = j.rew; c.done = j.done;
    c.actions = j.actions; c.order = j.order; c.action_ring = j.action_ring;
    c.en = (size_t)env->E * env->N; c.ob = obs_bytes(env, f32);
    c.p.obs_nt = plan::ring_past_cache(j.obs, j.ring, c.ob) ? 1 : 0;
    c.num_actions = j.num_actions; c.reset_every = j.reset_every; c.step0 = j.step0; c.ring = j.ring;
    return c;
}
static inline void chain_launch_step(const ssd_env *env, ChainCursor &c, int k) {
    Params &p = c.p;
    const size_t slot = (size_t)((c.step0 + k) % c.ring);
    p.obs = c.obs ? c.obs + slot * c.ob : nullptr;
    if (c.reset_every > 0 && (c.step0 + k) % c.reset_every == 0) {
        p.mode = ssd::kModeReset; p.rotate = 0; p.num_actions_random = 0; p.actions = nullptr; p.order = nullptr; p.rew = nullptr; p.done = nullptr;
        ssd::launch(p, env->game, c.s);
    }
    p.mode = ssd::kModeStep; p.rotate = 1;
    cursor_actions(c, p, (size_t)(c.step0 + k));
    p.rew = c.rew ? c.rew + slot * c.en : nullptr; p.done = c.done ? c.done + slot * c.en : nullptr;
    ssd::launch(p, env->game, c.s);
}

// One chain of a rollout: the launches of steps [0, n_steps) for envs [e_begin, e_end), enqueued on j.s by the calling thread
// (which is on the handle's device).
static int rollout_chain(ssd_env *env, const ChainJob &j) {
    const int32_t n_steps = j.n_steps;
    hipStream_t s = j.s;
    if (j.flags & SSD_ROLLOUT_FUSED) {
        // ONE launch for the whole chain: the kernel keeps each env in LDS / registers across its n_steps steps
        if (n_steps == 0) return SSD_OK;
        Params p = env->p;
        p.obs_f32 = 0;
        p.e_begin = j.e_begin; p.E = j.e_end;
        p.mode = ssd::kModeRollout; p.rotate = 1;
        p.num_actions_random = j.actions ? 0 : j.num_actions;
        p.actions = j.actions; p.order = j.actions ? j.order : nullptr; p.action_ring = j.actions ? j.action_ring : 0;
        p.n_steps = n_steps; p.reset_every = j.reset_every; p.step0 = j.step0; p.ring = j.ring;
        p.obs = j.obs; p.rew = j.rew; p.done = j.done;
        p.obs_nt = plan::ring_past_cache(j.obs, j.ring, obs_bytes(env, false)) ? 1 : 0;
        ssd::launch(p, env->game, s);
        return hipGetLastError() == hipSuccess ? SSD_OK : SSD_E_DEVICE;
    }
    ChainCursor c = chain_cursor(env, j);
    for (int k = 0; k < n_steps; ++k) chain_launch_step(env, c, k);
    return hipGetLastError() == hipSuccess ? SSD_OK : SSD_E_DEVICE;
}

// Body of a chain worker thread (see ChainWorker).
static void chain_worker_main(ssd_env *env, ChainWorker *w) {
    const bool on_device = hipSetDevice(env->device) == hipSuccess;       // once per thread
    static const int spin_us = SSD_HOOK("SSD_WORKER_SPIN_US", 200);
    for (;;) {
        int st = w->state.load(std::memory_order_acquire);
        if (st != 1 && st != 3) {
            // poll for a while (the caller of a rollout loop is back within microseconds), then sleep
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                st = w->state.load(std::memory_order_acquire);
                if (st == 1 || st == 3) break;
                __builtin_ia32_pause();
                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
            }
            if (st != 1 && st != 3) {
                std::unique_lock<std::mutex> lk(w->mu);
                w->cv.wait(lk, [&] { const int v = w->state.load(std::memory_order_acquire); return v == 1 || v == 3; });
                st = w->state.load(std::memory_order_acquire);
            }
        }
        if (st == 3) return;
        w->rc = on_device ? rollout_chain(env, w->job) : SSD_E_DEVICE;
        w->state.store(2, std::memory_order_release);
    }
}
static void post_job(ChainWorker *w, const ChainJob &j) {
    w->job = j;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->state.store(1, std::memory_order_release);
    }
    w->cv.notify_one();
}
static int wait_job(ChainWorker *w) {
    // the worker finishes within microseconds of the caller's own chain: poll
    for (int spins = 0; w->state.load(std::memory_order_acquire) != 2; ++spins) {
        if (spins < 4096) __builtin_ia32_pause();
        else std::this_thread::yield();
    }
    w->state.store(0, std::memory_order_relaxed);
    return w->rc;
}
void stop_workers(ssd_env *env) {
    for (auto &w : env->workers) {
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->state.store(3, std::memory_order_release);
        }
        w->cv.notify_one();
        if (w->th.joinable()) w->th.join();
    }
    env->workers.clear();
}

// Everything the handle ever put into the library's queues has completed when this returns (or a queue has failed).
// hipDeviceSynchronize() does not cover queues the HIP runtime does not own, so whoever frees memory those packets name --
// ssd_destroy, an error path that leaves a call's work behind without a stream-side wait -- drains them on the host first.
static void aql_drain(ssd_env *env) {
    if (!env->aql) return;
    AqlState &A = *env->aql;
    if (!A.ok && !A.nq) return;
    if (!A.joins || !A.flag_kernarg) return;                        // (nothing was ever enqueued)
    std::lock_guard<std::mutex> enqueue_lock(ssd::aql::enqueue_mutex(env->device));
    for (int c = 0; c < A.nq; ++c) {
        if (!A.q[c] || ssd::aql::queue_failed(A.q[c])) continue;
        if (ssd::aql::join_and_wait(A.q[c], A.flag_kernarg)) A.joins += 1;
    }
}

// A wait of one of the handle's rollout calls timed out: the call had returned SSD_OK long before, the caller's
// stream went on, and the chains' packets may still be running and writing obs / rew / done and the state pair.  The first API
// call that notices -- the next rollout call, ssd_synchronize -- drains the library's queues on the host (bounded: a queue that
// is stuck for good is left alone), takes the handle off the library's own dispatch path (later calls issue the same launches
// through hipLaunchKernel) and reports SSD_E_DEVICE once.  Until then the call's buffers must not be freed or reused.
int after_timeout(ssd_env *env) {
    if (!env->aql || !env->aql->timed_out_host) return SSD_OK;
    AqlState &A = *env->aql;
    if (!__atomic_load_n(A.timed_out_host, __ATOMIC_ACQUIRE)) return SSD_OK;
    bool drained = true;
    if (A.joins && A.flag_kernarg) {
        std::lock_guard<std::mutex> enqueue_lock(ssd::aql::enqueue_mutex(env->device));
        for (int c = 0; c < A.nq; ++c) {
            if (!A.q[c] || ssd::aql::queue_failed(A.q[c])) continue;
            if (ssd::aql::join_and_wait(A.q[c], A.flag_kernarg, 10.0)) A.joins += 1; else drained = false;
        }
    }
    __atomic_store_n(A.timed_out_host, 0u, __ATOMIC_RELEASE);
    A.ok = false;
    env->err = drained ? "a rollout call's wait for the library's dispatch queues timed out (the WAIT_TIMEOUT status bit): its outputs may be incomplete; "
                         "the queues have been drained and the handle now steps through hipLaunchKernel"
                       : "a rollout call's wait for the library's dispatch queues timed out (the WAIT_TIMEOUT status bit) and the queues did not "
                         "drain within 10 s: its buffers may still be written to";
    return SSD_E_DEVICE;
}

void aql_teardown(ssd_env *env) {
    if (!env->aql) return;
    AqlState &A = *env->aql;
    // (the queues belong to the device's pool and stay; the handle's work in them must be over before its memory goes)
    aql_drain(env);
    for (uint64_t h : A.fork_sig) ssd::aql::signal_destroy(h);
    if (A.join_counter) (void)hipFree(A.join_counter);
    if (A.fork_counter) (void)hipFree(A.fork_counter);
    ssd::aql::host_kernarg_free(A.flag_kernarg);
    ssd::aql::host_kernarg_free(A.fork_kernarg);
    for (auto &st : A.sets) if (st.dev) (void)hipFree(st.dev);
    // (of the state pair, world_buf[0] / agents_buf[0] are the handle's original allocations: freed with env->allocs; if the
    // current state sits in the other pair, ssd_destroy frees whichever pointers env->p does not hold)
    for (int i = 0; i < 2; ++i) { if (A.snap_grid[i]) (void)hipFree(A.snap_grid[i]); if (A.beam_list[i]) (void)hipFree(A.beam_list[i]); }
    if (A.world_buf[1]) (void)hipFree(A.world_buf[1]);
    if (A.agents_buf[1]) (void)hipFree(A.agents_buf[1]);
    for (int k = 0; k < plan::kMids; ++k)
        for (int i = 0; i < 2; ++i)
            for (void *m : {(void *)A.mid_world[k][i], (void *)A.mid_snap[k][i], (void *)A.mid_agents[k][i], (void *)A.mid_list[k][i]}) if (m) (void)hipFree(m);
    for (int k = 0; k < plan::kLongMids - plan::kMids; ++k)
        for (int i = 0; i < 2; ++i)
            for (void *m : {(void *)A.long_world[k][i], (void *)A.long_snap[k][i], (void *)A.long_agents[k][i], (void *)A.long_list[k][i]}) if (m) (void)hipFree(m);
    env->aql.reset();
}

// Queues for `chains` chains, fork signals: created once.  false: use hipLaunchKernel.
static bool aql_ready(ssd_env *env, int chains) {
    if (!env->aql) env->aql.reset(new AqlState());
    AqlState &A = *env->aql;
    if (A.tried && !A.ok) return false;
    if (!A.tried) {
        A.tried = true;
        if (!ssd::aql::available(env->device)) return false;
        for (int i = 0; i < AqlState::kForks; ++i) {
            A.fork_sig[i] = ssd::aql::signal_create(0);
            if (!A.fork_sig[i]) return false;
        }
        void *ptr = nullptr;
        if (hipMalloc(&ptr, 8) != hipSuccess || hipMemset(ptr, 0, 8) != hipSuccess) { (void)hipGetLastError(); return false; }
        A.join_counter = static_cast<unsigned long long *>(ptr);
        A.flag_kernarg = ssd::aql::host_kernarg_alloc(env->device, 64);
        if (!A.flag_kernarg) return false;
        std::memcpy(A.flag_kernarg, &A.join_counter, sizeof(void *));
        {
            void *h = nullptr, *d = nullptr;
            if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
            A.timed_out_host = static_cast<uint32_t *>(h); A.timed_out_dev = static_cast<uint32_t *>(d);
            *A.timed_out_host = 0;
            env->host_allocs.push_back(h);
        }
        ptr = nullptr;
        if (hipMalloc(&ptr, 8) != hipSuccess || hipMemset(ptr, 0, 8) != hipSuccess) { (void)hipGetLastError(); return false; }
        A.fork_counter = static_cast<unsigned long long *>(ptr);
        A.fork_kernarg = static_cast<uint8_t *>(ssd::aql::host_kernarg_alloc(env->device, AqlState::kForks * AqlState::kForkBlock));
        if (!A.fork_kernarg || !ssd::aql::lookup(env->device, ssd::wait_kernel_fn(), &A.wait_kernel) || A.wait_kernel.kernarg_size > AqlState::kForkBlock) return false;
        {   // first launches of the two helper kernels now (the runtime resolves a kernel on its first launch: ~50 us), not
            // inside somebody's first short rollout -- and before the pool's first queue is probed (the probe launches one of them)
            ssd::aql::signal_set(A.fork_sig[0], 1);
            ssd::launch_signal_kernel(ssd::aql::signal_value_ptr(A.fork_sig[0]), nullptr);
            ssd::launch_wait_counter_kernel(A.join_counter, 0, nullptr, 0, nullptr, nullptr, nullptr);
            ssd::launch_flag_kernel(A.fork_counter, nullptr); A.forks = 1;
            if (hipStreamSynchronize(nullptr) != hipSuccess) { (void)hipGetLastError(); return false; }
        }
        A.q[0] = ssd::aql::pool_queue(env->device, 0);
        if (!A.q[0]) return false;
        A.nq = 1;
        A.ok = true;
    }
    if (chains > ssd::aql::pool_size(env->device)) return false;   // (more chains than the device's pool has queues: HIP streams)
    while (A.nq < chains) {
        // (a queue the probe turns down is not an error of the path: this call goes through HIP streams, later automatic
        // choices stay within the smaller pool)
        A.q[A.nq] = ssd::aql::pool_queue(env->device, A.nq);
        if (!A.q[A.nq]) return false;
        A.nq++;
    }
    for (int c = 0; c < A.nq; ++c) if (ssd::aql::queue_failed(A.q[c])) { A.ok = false; return false; }
    return true;
}

static inline void aql_wait_consumed(ssd::aql::Queue *q, uint64_t idx_plus_1) {
    // (bounded in practice: the packets in question belong to calls made long ago)
    while (idx_plus_1 && ssd::aql::read_index(q) < idx_plus_1 && !ssd::aql::queue_failed(q)) __builtin_ia32_pause();
}

// The second state buffers, the render side buffers of split rollouts and the `mid` sets of step runs (one per pass before a run's
// last and orientation), once per handle: all thirty or none.
static bool aql_split_buffers(ssd_env *env) {
    AqlState &A = *env->aql;
    if (A.world_buf[1]) return true;                                // (set last, below)
    const size_t grid = (size_t)env->E * env->S, agents = (size_t)env->E * (env->N ? env->N : 1) * 4;
    const size_t lists = (size_t)env->E * 128 * 4;                  // (beam lists: [E][64] + a second [E][64] for steps whose beams took two passes)
    constexpr int kBufs = 6 + 8 * plan::kMids;
    size_t sizes[kBufs] = {grid, agents, grid, grid, lists, lists};
    for (int k = 0; k < plan::kMids; ++k) {
        const size_t mids[8] = {grid, grid, grid, grid, agents, agents, lists, lists};
        for (int j = 0; j < 8; ++j) sizes[6 + 8 * k + j] = mids[j];
    }
    void *buf[kBufs] = {};
    for (int i = 0; i < kBufs; ++i)
        if (hipMalloc(&buf[i], sizes[i]) != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j < i; ++j) (void)hipFree(buf[j]);
            return false;
        }
    A.world_buf[0] = env->p.world; A.agents_buf[0] = env->p.agents;
    A.agents_buf[1] = static_cast<uint32_t *>(buf[1]);
    A.snap_grid[0] = static_cast<uint8_t *>(buf[2]); A.snap_grid[1] = static_cast<uint8_t *>(buf[3]);
    A.beam_list[0] = static_cast<uint32_t *>(buf[4]); A.beam_list[1] = static_cast<uint32_t *>(buf[5]);
    for (int k = 0; k < plan::kMids; ++k)
        for (int i = 0; i < 2; ++i) {
            void **b = buf + 6 + 8 * k;
            A.mid_world[k][i] = static_cast<uint8_t *>(b[i]); A.mid_snap[k][i] = static_cast<uint8_t *>(b[2 + i]);
            A.mid_agents[k][i] = static_cast<uint32_t *>(b[4 + i]); A.mid_list[k][i] = static_cast<uint32_t *>(b[6 + i]);
        }
    A.world_buf[1] = static_cast<uint8_t *>(buf[0]);
    return true;
}

// The mid sets of a long call's runs of eight beyond those of runs of four (four more per orientation), with the handle's first long
// argument set: all thirty-two buffers or none.  false: the handle's long calls keep runs of four.
static bool aql_long_buffers(ssd_env *env) {
    AqlState &A = *env->aql;
    constexpr int kSets = plan::kLongMids - plan::kMids;
    if (A.long_tried) return A.long_world[0][0] != nullptr;
    A.long_tried = true;
    const size_t grid = (size_t)env->E * env->S, agents = (size_t)env->E * (env->N ? env->N : 1) * 4, lists = (size_t)env->E * 128 * 4;
    const size_t mids[8] = {grid, grid, grid, grid, agents, agents, lists, lists};
    void *buf[8 * kSets] = {};
    for (int i = 0; i < 8 * kSets; ++i)
        if (hipMalloc(&buf[i], mids[i % 8]) != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j < i; ++j) (void)hipFree(buf[j]);
            return false;
        }
    for (int k = 0; k < kSets; ++k)
        for (int i = 0; i < 2; ++i) {
            void **b = buf + 8 * k;
            A.long_world[k][i] = static_cast<uint8_t *>(b[i]); A.long_snap[k][i] = static_cast<uint8_t *>(b[2 + i]);
            A.long_agents[k][i] = static_cast<uint32_t *>(b[4 + i]); A.long_list[k][i] = static_cast<uint32_t *>(b[6 + i]);
        }
    return true;
}

// The kernel-argument set for this call's parameters: found among the cached ones, or built, uploaded (synchronously) and cached.
// Argument block `i` of a chain serves the steps whose index is i modulo key.slots = lcm(output ring, action ring): its output slot
// is i % ring, its action slot i % action_ring.
static AqlState::Set *aql_set(ssd_env *env, const AqlState::Key &key, int chains, const ChainJob *jobs) {
    AqlState &A = *env->aql;
    A.clock++;
    for (auto &st : A.sets) if (st.valid && st.key == key) { st.stamp = A.clock; return &st; }
    AqlState::Set *victim = &A.sets[0];
    for (auto &st : A.sets) { if (!st.valid) { victim = &st; break; } if (st.stamp < victim->stamp) victim = &st; }
    AqlState::Set &st = *victim;
    if (st.valid) for (int c = 0; c < 8 && c < A.nq; ++c) aql_wait_consumed(A.q[c], st.last_use[c]);   // nobody reads the old blocks any more
    st.valid = false;
    st.key = key;                                   // (block_of() goes by the key's slots)
    st.kinds = plan::kind_table(key.split, key.pairs);
    st.long_kinds = plan::long_kind_table(key.long_cap);
    const int n_dense = st.kinds.n_dense;
    st.long_at = (size_t)chains * key.slots * n_dense * AqlState::kBlock;
    const size_t need = st.long_at + (size_t)chains * key.slots * st.long_kinds.n_dense * AqlState::kLongBlock;
    if (need > st.cap) {
        if (st.dev) (void)hipFree(st.dev);
        st.dev = nullptr; st.cap = 0;
        void *ptr = nullptr;
        if (hipMalloc(&ptr, need) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        st.dev = static_cast<uint8_t *>(ptr); st.cap = need;
    }
    if (key.split && !aql_split_buffers(env)) return nullptr;
    std::vector<uint8_t> host(need, 0);
    for (int c = 0; c < chains; ++c) {
        const ChainCursor cur = chain_cursor(env, jobs[c]);
        for (int i = 0; i < key.slots; ++i)
            for (int kind = 0; kind < plan::kKinds; ++kind) {
                if (st.kinds.dense[kind] < 0) continue;         // (no call of this key uses the kind)
                Params p;
                ssd::PairParams q;
                plan::fill_block(cur.p, cur, key, A, kind, i, p, q);
                ssd::Launch L;
                if (!ssd::select(p, env->game, &L, &q)) return nullptr;
                AqlState::Geo &g = st.geo[c][kind];
                if (i == 0) {
                    if (!ssd::aql::lookup(env->device, L.fn, &g.k) || g.k.kernarg_size > AqlState::kBlock || g.k.kernarg_size < sizeof(ssd::KernArgs)) return nullptr;
                    g.grid_x = L.grid_x; g.block_x = L.block_x; g.lds = L.lds;
                }
                std::memcpy(host.data() + (((size_t)c * key.slots + i) * n_dense + st.kinds.dense[kind]) * AqlState::kBlock, &L.args, L.args_bytes());
            }
        // (a long set: the long kinds' blocks behind the others -- the launch's KernArgs, then its LongParams)
        for (int i = 0; i < key.slots; ++i)
            for (int kind = plan::kKinds; kind < plan::kAllKinds; ++kind) {
                if (st.long_kinds.dense[kind - plan::kKinds] < 0) continue;
                Params p;
                ssd::LongParams q;
                plan::fill_long_block(cur.p, cur, key, A, kind, i, p, q);
                ssd::Launch L;
                if (!ssd::select(p, env->game, &L)) return nullptr;
                AqlState::Geo &g = st.geo[c][kind];
                if (i == 0) {
                    if (!ssd::aql::lookup(env->device, L.fn, &g.k) || g.k.kernarg_size > AqlState::kLongBlock || g.k.kernarg_size < sizeof(ssd::KernArgs)) return nullptr;
                    g.grid_x = L.grid_x; g.block_x = L.block_x; g.lds = L.lds;
                }
                uint8_t *at = host.data() + (st.block_of(c, (size_t)i, kind) - st.dev);
                std::memcpy(at, &L.args, sizeof(ssd::KernArgs));
                std::memcpy(at + sizeof(ssd::KernArgs), &q, sizeof q);
            }
    }
    if (hipMemcpy(st.dev, host.data(), need, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    st.key = key; st.valid = true; st.stamp = A.clock;
    for (auto &u : st.last_use) u = 0;
    return &st;
}

// FORK: the chains wait (barrier-AND) for a signal that a one-wave kernel on the caller's stream zeroes -- unless the
// stream has nothing pending, in which case there is nothing to wait for and the first step can start at once
static int aql_fork(ssd_env *env, int chains, hipStream_t s, bool sync_mode) {
    AqlState &A = *env->aql;
    static const bool always_fork = SSD_HOOK("SSD_AQL_ALWAYS_FORK", 0) != 0;
    if (sync_mode) { SSD_HIP(env, hipStreamSynchronize(s)); env->last_path |= SSD_PATH_SYNC; }
    bool stream_idle = sync_mode || (!always_fork && hipStreamQuery(s) == hipSuccess);
    if (!stream_idle && !always_fork) {
        // a marker or an event record just ahead of the call drains within microseconds: look again for a moment before paying
        // for a fork (a kernel launch on the stream + a barrier packet that polls its signal: ~20 us until the first step starts)
        static const int spin_us = SSD_HOOK("SSD_AQL_FORK_SPIN_US", 8);
        const auto t0 = std::chrono::steady_clock::now();
        while (!stream_idle && std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(spin_us))
            stream_idle = hipStreamQuery(s) == hipSuccess;
    }
    if (!stream_idle) {
        (void)hipGetLastError();                                       // (hipErrorNotReady is not an error here)
        const int slot = A.fork_next;
        A.fork_next = (A.fork_next + 1) % AqlState::kForks;
        for (int c = 0; c < A.nq; ++c) { aql_wait_consumed(A.q[c], A.fork_used[slot][c]); A.fork_used[slot][c] = 0; }
        // Two forms.  (1) A one-wave kernel on the stream bumps a counter in device memory, and every chain starts with a one-wave
        // dispatch that polls it (the join's construct, the other way round).  (0) A kernel on the stream zeroes an HSA signal that a
        // barrier-AND packet at the head of every chain waits on: the command processor then polls the signal, at its own pace
        // (measured: a 20-step call from a stream with a 2 us kernel pending: 13.4 us per step against 6.5 from an idle stream).
        static const int fork_kind = SSD_HOOK("SSD_AQL_FORK_KIND", 1);
        if (fork_kind == 1) {
            A.forks++;
            ssd::launch_flag_kernel(A.fork_counter, s);
            // (nothing is in the library's queues yet: an error here leaves nothing behind)
            if (hipGetLastError() != hipSuccess) { A.forks--; env->err = "fork kernel launch failed"; return SSD_E_DEVICE; }
            // (the wait is bounded -- a minute: what the stream holds ahead of the call may be a whole training step)
            ssd::WaitArgs wa{A.fork_counter, A.forks, ssd::aql::abort_flag_dev(env->device), 6000000000ull, env->p.status, A.timed_out_dev};
            uint8_t *ka = A.fork_kernarg + (size_t)slot * AqlState::kForkBlock;
            std::memcpy(ka, &wa, sizeof wa);
            for (int c = 0; c < chains; ++c) {
                ssd::aql::dispatch(A.q[c], A.wait_kernel, 1, 64, 0, ka, /*barrier=*/true, 0, 0);
                A.fork_used[slot][c] = ssd::aql::write_index(A.q[c]);
            }
        } else {
            ssd::aql::signal_set(A.fork_sig[slot], 1);
            ssd::launch_signal_kernel(ssd::aql::signal_value_ptr(A.fork_sig[slot]), s);
            // (nothing is in the library's queues yet: an error here leaves nothing behind)
            if (hipGetLastError() != hipSuccess) { env->err = "fork kernel launch failed"; return SSD_E_DEVICE; }
            for (int c = 0; c < chains; ++c) {
                ssd::aql::barrier_and(A.q[c], A.fork_sig[slot]);
                A.fork_used[slot][c] = ssd::aql::write_index(A.q[c]);     // (= index of the barrier packet + 1)
            }
        }
        env->last_path |= SSD_PATH_FORKED;
    }
    return SSD_OK;
}

// JOIN: every chain ends by bumping the join counter; a one-wave kernel on the caller's stream sleeps until all have
static int aql_join(ssd_env *env, AqlState::Set *st, int chains, int32_t n_steps, hipStream_t s, bool sync_mode) {
    AqlState &A = *env->aql;
    auto host_join = [&]() -> bool {                      // the synchronous form: the HOST waits for every chain
        bool ok = true;
        for (int c = 0; c < chains; ++c) ssd::aql::ring(A.q[c]);
        for (int c = 0; c < chains; ++c) { ok = ssd::aql::join_and_wait(A.q[c], A.flag_kernarg) && ok; st->last_use[c] = ssd::aql::write_index(A.q[c]); }
        A.joins += (unsigned long long)chains;
        return ok;
    };
    if (sync_mode) {
        if (!host_join()) { env->err = "the HSA runtime reported an error on a dispatch queue"; A.ok = false; return SSD_E_DEVICE; }
        return SSD_OK;
    }
    for (int c = 0; c < chains; ++c) {
        ssd::aql::join(A.q[c], A.flag_kernarg);
        st->last_use[c] = ssd::aql::write_index(A.q[c]);
    }
    A.joins += (unsigned long long)chains;
    // (the stream-side wait is bounded: seconds beyond any healthy call -- ssd_kernels.hip, ssd_wait_counter_kernel)
    unsigned long long timeout_ticks = (unsigned long long)((2.0 + 0.002 * (double)n_steps) * 1e8);
    // (test hooks: wait for a count that never comes / with a short bound -- tests/test_hip_fullsize.py, test_join_wait_is_bounded)
    static const int test_lost = SSD_HOOK("SSD_AQL_TEST_LOST_JOIN", 0), test_timeout_ms = SSD_HOOK("SSD_AQL_TEST_TIMEOUT_MS", 0);
    if (test_timeout_ms > 0) timeout_ticks = (unsigned long long)test_timeout_ms * 100000ull;
    (void)hipGetLastError();                              // (an earlier, unrelated sticky error of the caller's must not be read as ours)
    ssd::launch_wait_counter_kernel(A.join_counter, A.joins + (test_lost ? 1000000ull : 0ull), ssd::aql::abort_flag_dev(env->device), timeout_ticks,
                                    env->p.status, A.timed_out_dev, s);
    if (hipGetLastError() != hipSuccess) {
        // the chains' packets are out and nothing on the stream waits for them: wait here, so that the call's work is over (and
        // its results in place) when the error is returned -- nobody frees or reuses memory under running kernels
        bool ok = true;
        for (int c = 0; c < chains; ++c) ok = ssd::aql::join_and_wait(A.q[c], A.flag_kernarg) && ok;
        A.joins += (unsigned long long)chains;
        env->err = "join kernel launch failed (the call's work was waited for on the host)"; A.ok = false;
        return SSD_E_DEVICE;
    }
    for (int c = 0; c < chains; ++c) if (ssd::aql::queue_failed(A.q[c])) { env->err = "the HSA runtime reported an error on a dispatch queue"; A.ok = false; return SSD_E_DEVICE; }
    return SSD_OK;
}

// A rollout through the library's own queues: the call's form, its argument set, the fork from the caller's stream, the packets of
// the plan (ssd_rollout_plan.hpp), the join.  Returns SSD_OK, an error, or 1 = "not taken" (the caller then issues the same
// launches through hipLaunchKernel).
static int rollout_aql(ssd_env *env, int chains, const ChainJob *jobs, hipStream_t s) {
    if (!aql_ready(env, chains)) return 1;
    AqlState &A = *env->aql;
    const ChainJob &j0 = jobs[0];
    // FORM (plan::choose_form has the rules and what they were measured by)
    AqlState::Key key;
    key.obs = j0.obs; key.rew = j0.rew; key.done = j0.done; key.ring = j0.ring; key.f32 = (j0.flags & SSD_OBS_F32) ? 1 : 0;
    key.num_actions = j0.num_actions; key.chains = chains; key.horizon = env->p.horizon;
    key.actions = j0.actions; key.order = j0.actions ? j0.order : nullptr; key.action_ring = j0.actions ? j0.action_ring : 0;
    key.slots = plan::block_slots(key.ring, key.action_ring, chains);
    if (!key.slots) return 1;
    key.stamps = env->p.stamps; key.dbg_skip = env->p.dbg_skip;
    static const int env_coh = SSD_KNOB("SSD_AQL_COHERENT", 1);
    static const int env_alternate = SSD_HOOK("SSD_AQL_ALTERNATE", 0);
    static const int env_split = SSD_KNOB("SSD_AQL_SPLIT", 1);
    static const int env_pairs = SSD_HOOK("SSD_AQL_PAIRS", 1);
    static const int env_run = SSD_HOOK("SSD_AQL_RUN", ssd::kLongRun);
    plan::FormIn in;
    in.per_launch = (env->E + chains - 1) / chains; in.chains = chains;
    in.f32 = key.f32 != 0; in.order = key.order != nullptr; in.obs = j0.obs != nullptr; in.n_steps = j0.n_steps;
    in.fast_profile = ssd::fast_profile(env->p, env->game); in.pair_profile = ssd::pair_profile(env->p, env->game);
    in.aql_coherent = env_coh; in.aql_split = env_split; in.aql_alternate = env_alternate; in.aql_pairs = env_pairs; in.aql_run = env_run;
    in.long_profile = ssd::long_profile(env->p, env->game);
    plan::Form form = plan::choose_form(in);
    // (a long set names four more mid sets per orientation; a handle that cannot have them keeps runs of four, and says nothing)
    if (form.key_long && !aql_long_buffers(env)) form.key_long = form.long_cap = 0;
    const bool coherent = form.coherent != 0, split = form.split;
    key.coherent = form.coherent; key.split = form.key_split; key.pairs = form.pairs; key.long_cap = form.key_long;
    // (a split set holds its launches for both orientations of the state pair; any other set names the buffer that is current now)
    key.world = key.split ? nullptr : env->p.world;
    // SET
    AqlState::Set *st = aql_set(env, key, chains, jobs);
    if (!st) return 1;
    // (only now is the call certain to take this path: ssd_rollout_path() must not name a path the launches did not take)
    env->last_path |= SSD_PATH_AQL | (coherent ? SSD_PATH_COHERENT : 0) | (split ? SSD_PATH_SPLIT : 0);
    if (j0.n_steps == 0) return SSD_OK;
    // (the queues are the device's, shared with the other handles on it: one call writes packets at a time)
    std::lock_guard<std::mutex> enqueue_lock(ssd::aql::enqueue_mutex(env->device));
    // Sync mode: the call itself waits -- for the stream before, for the chains after -- and no kernel waits for another queue's
    // kernel.  Chosen automatically when a profiling tool is attached (aql_sync_mode), or with SSD_AQL_SYNC=1.
    const bool sync_mode = ssd::aql::sync_mode();
    // FORK
    if (const int rc = aql_fork(env, chains, s, sync_mode)) return rc;
    // ENQUEUE the plan, group by group: a group's packets are written and rung before the next group is planned
    // Fence scopes of the step packets (hsa_fence_scope_t: 0 none, 1 agent, 2 system).  Test-hook build only: SSD_AQL_ACQ /
    // SSD_AQL_REL override them -- for the plain kernels anything weaker than agent / agent gives up the visibility a HIP stream
    // provides, which is why the product does not read them.
    static const int env_acq = SSD_HOOK("SSD_AQL_ACQ", -1);
    static const int env_rel = SSD_HOOK("SSD_AQL_REL", -1);
    // Coherent chains: only the first packet of the call acquires (what the caller's stream did before -- a set_state, another
    // kernel -- may sit in caches); between the chain's own launches nothing is read through a cache that could be stale
    // (-0.14 us per step); the renderer workgroups of a split rollout read state and beam lists with agent-scope loads as well.
    const int kAcq = env_acq >= 0 ? env_acq : (coherent ? 0 : 1), kRel = env_rel >= 0 ? env_rel : (coherent ? 0 : 1);
    const bool obs_wb = !key.f32 && plan::ring_past_cache(j0.obs, j0.ring, obs_bytes(env, false));   // (chain_cursor's obs_nt)
    const int o = plan::start_orientation(key.split, A.world_buf[1] && env->p.world == A.world_buf[1]);
    plan::Schedule sched(j0.n_steps, j0.step0, j0.reset_every, j0.ring, key.slots, split, form.run_cap, coherent, obs_wb, kAcq, kRel, o, form.long_cap);
    plan::Group g;
    while (sched.next(g))
        for (int c = 0; c < chains; ++c) {
            for (int j = 0; j < g.n_packets; ++j) {
                const plan::Packet &pk = g.packet[j];
                const AqlState::Geo &geo = st->geo[c][pk.kind];
                ssd::aql::dispatch(A.q[c], geo.k, geo.grid_x, geo.block_x, geo.lds, st->block_of(c, pk.block, pk.kind), /*barrier=*/true, pk.acquire, pk.release);
            }
            if (g.ring) ssd::aql::ring(A.q[c]);
        }
    if (sched.longest() > 1) env->last_path |= SSD_PATH_PAIRS;
    env->last_path = (env->last_path & ~(15 << SSD_PATH_RUN_SHIFT)) | (sched.longest() << SSD_PATH_RUN_SHIFT);
    if (split) {                                          // the current state now sits in buffer orientation()
        env->p.world = A.world_buf[sched.orientation()]; env->p.agents = A.agents_buf[sched.orientation()];
    }
    // JOIN
    return aql_join(env, st, chains, j0.n_steps, s, sync_mode);
}

// ssd_rollout_random and ssd_rollout_actions: the same launches, the actions drawn on the device or read from the caller's ring.
static int rollout(ssd_env *env, const int32_t *actions, const uint8_t *order, int32_t action_ring, int32_t num_actions, int32_t n_steps,
                   int32_t reset_every, int32_t step0, void *obs, int32_t *rew, uint8_t *done, int32_t ring, uint32_t flags, void *stream) {
    if (obs && (reinterpret_cast<uintptr_t>(obs) & 3u)) { env->err = "obs must be 4-byte aligned"; return SSD_E_INVALID; }
    // SSD_ROLLOUT_AUTO: the form of the call is the library's choice.  The fused kernel is the fastest form there is (4096 Harvest
    // envs: 3.5 us per step of a long call against 5.4 through the chains, 4.5 against 6.1 - 6.6 in 20-step calls) wherever it
    // applies: uint8 observations, index action order, and more than one step (a single step is one launch either way, and the
    // per-step kernels are the shorter ones).  ssd_rollout_path() reports the form that ran.
    if (flags & SSD_ROLLOUT_AUTO) {
        flags &= ~(uint32_t)SSD_ROLLOUT_AUTO;
        if (!(flags & SSD_OBS_F32) && !order && n_steps >= 2) flags |= SSD_ROLLOUT_FUSED;
    }
    if ((flags & SSD_ROLLOUT_FUSED) && (flags & SSD_OBS_F32)) { env->err = "the fused rollout kernel writes uint8 observations"; return SSD_E_INVALID; }
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != env->device) SSD_HIP(env, hipSetDevice(env->device));
    }
    if (const int rc = after_timeout(env)) return rc;               // (an earlier call's join gave up: reported once, here or in ssd_synchronize)
    hipStream_t s = static_cast<hipStream_t>(stream);
    env->last_stream = s; env->last_stream_set = true;
    uint8_t *o = static_cast<uint8_t *>(obs);
    // Envs are independent, so a rollout is as many independent launch chains as we like.  Two chains in two queues keep the
    // GPU busy while the other chain's kernel drains and the next one is dispatched -- the ~2 us per launch that a single
    // chain of dependent kernels cannot hide.  SSD_ROLLOUT_CHAINS overrides.
    static const int forced = SSD_KNOB("SSD_ROLLOUT_CHAINS", 0);
    auto by_size = [&]() { return env->E < 2048 ? 1 : (env->E >= 6144 && env->E <= 24576) ? 3 : 2; };   // measured: profiles/r01_sweep_envs.txt
    int chains = env->rollout_chains > 0 ? env->rollout_chains : forced > 0 ? forced : by_size();
    if ((flags & SSD_ROLLOUT_FUSED) && env->rollout_chains <= 0 && forced <= 0) chains = 1;   // one launch already covers the whole rollout
    const bool automatic = env->rollout_chains <= 0 && forced <= 0;
    // (an automatic choice stays within the library's own dispatch queues -- ssd_aql.hip, pool_size() -- and where the probe found
    // the process past the hardware-queue cliff already, every further active queue or stream would be time-sliced against the
    // others: one chain on the caller's own stream)
    auto clamp_chains = [&]() {
        if (automatic && ssd::aql::pool_size(env->device) >= 1 && chains > ssd::aql::pool_size(env->device)) chains = ssd::aql::pool_size(env->device);
        if (automatic && ssd::aql::over_the_cliff(env->device)) chains = 1;
        if (chains > 8) chains = 8;
        if (chains > env->E) chains = env->E;
        if (chains < 1) chains = 1;
        env->last_path = (chains << 8) | ((flags & SSD_ROLLOUT_FUSED) ? SSD_PATH_FUSED : 0);
    };
    clamp_chains();
    auto range = [&](int c) { return (int)(((long long)env->E * c) / chains); };
    auto job_of = [&](int c, hipStream_t cs) {
        ChainJob j;
        j.chain = c; j.e_begin = range(c); j.e_end = range(c + 1);
        j.num_actions = num_actions; j.n_steps = n_steps; j.reset_every = reset_every; j.step0 = step0; j.ring = ring;
        j.actions = actions; j.order = order; j.action_ring = action_ring;
        j.obs = o; j.rew = rew; j.done = done; j.flags = flags; j.s = cs;
        return j;
    };
    if (!(flags & SSD_ROLLOUT_FUSED)) {
        // the library's own dispatch path: the same launches as below, written as AQL packets into its own queues
        for (int attempt = 0; attempt < 2; ++attempt) {
            ChainJob jobs[8];
            for (int c = 0; c < chains; ++c) jobs[c] = job_of(c, s);
            const int pool_before = ssd::aql::pool_size(env->device);
            const int rc = rollout_aql(env, chains, jobs, s);
            env->last_path |= ssd::aql::pool_report(env->device);
            if (rc <= 0) return rc;
            env->last_path &= ~(SSD_PATH_AQL | SSD_PATH_COHERENT | SSD_PATH_SPLIT | SSD_PATH_PAIRS | SSD_PATH_SYNC | SSD_PATH_FORKED | (15 << SSD_PATH_RUN_SHIFT));
            // (this call created a queue that failed its probe: an automatic chain count is chosen again for the pool that is left)
            if (!automatic || ssd::aql::pool_size(env->device) >= pool_before) break;
            chains = by_size();
            clamp_chains();
            env->last_path |= ssd::aql::pool_report(env->device);
        }
    }
    if (chains <= 1) {
        int rc = rollout_chain(env, job_of(0, s));
        if (rc) env->err = "kernel launch failed in a rollout call";
        return rc;
    }
    while ((int)env->chain_streams.size() < chains - 1) {
        hipStream_t ns; hipEvent_t ne;
        SSD_HIP(env, hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
        SSD_HIP(env, hipEventCreateWithFlags(&ne, hipEventDisableTiming));
        env->chain_streams.push_back(ns); env->chain_events.push_back(ne);
    }
    if (!env->fork_event) SSD_HIP(env, hipEventCreateWithFlags(&env->fork_event, hipEventDisableTiming));
    // Who enqueues.  The chains' launches either come from this thread, step by step across the chains (no other thread
    // involved: a short call costs its launches and nothing else), or each extra chain from its persistent worker thread
    // (long calls: two threads enqueue ~10 % faster than one).  (Test-hook build: SSD_ROLLOUT_THREADS=0 / 1 forces one or the other.)
    static const int env_threads = SSD_HOOK("SSD_ROLLOUT_THREADS", -1);
    static const int inline_steps = SSD_HOOK("SSD_ROLLOUT_INLINE_STEPS", 256);
    bool threads = !(flags & SSD_ROLLOUT_FUSED) && n_steps > inline_steps;
    if (env_threads == 0) threads = false;
    if (env_threads == 1) threads = true;
    // fork: the extra chains start after whatever the caller's stream holds so far
    SSD_HIP(env, hipEventRecord(env->fork_event, s));
    for (int c = 1; c < chains; ++c) SSD_HIP(env, hipStreamWaitEvent(env->chain_streams[c - 1], env->fork_event, 0));
    int rc_all = SSD_OK;
    if (threads) {
        while ((int)env->workers.size() < chains - 1) {
            env->workers.emplace_back(new ChainWorker());
            ChainWorker *w = env->workers.back().get();
            w->th = std::thread(chain_worker_main, env, w);
        }
        for (int c = 1; c < chains; ++c) post_job(env->workers[c - 1].get(), job_of(c, env->chain_streams[c - 1]));
        rc_all = rollout_chain(env, job_of(0, s));
        for (int c = 1; c < chains; ++c) { const int rc = wait_job(env->workers[c - 1].get()); if (rc && !rc_all) rc_all = rc; }
    } else if (flags & SSD_ROLLOUT_FUSED) {
        for (int c = 0; c < chains; ++c) { const int rc = rollout_chain(env, job_of(c, c ? env->chain_streams[c - 1] : s)); if (rc && !rc_all) rc_all = rc; }
    } else {
        ChainCursor cur[8];
        for (int c = 0; c < chains; ++c) cur[c] = chain_cursor(env, job_of(c, c ? env->chain_streams[c - 1] : s));
        for (int k = 0; k < n_steps; ++k)
            for (int c = 0; c < chains; ++c) chain_launch_step(env, cur[c], k);
        if (hipGetLastError() != hipSuccess) rc_all = SSD_E_DEVICE;
    }
    // join: the caller's stream continues after every chain
    for (int c = 1; c < chains; ++c) {
        SSD_HIP(env, hipEventRecord(env->chain_events[c - 1], env->chain_streams[c - 1]));
        SSD_HIP(env, hipStreamWaitEvent(s, env->chain_events[c - 1], 0));
    }
    if (rc_all) env->err = "kernel launch failed in a rollout call";
    return rc_all;
}

extern "C" {

int ssd_rollout_random(ssd_env *env, int32_t num_actions, int32_t n_steps, int32_t reset_every, int32_t step0,
                       void *obs, int32_t *rew, uint8_t *done, int32_t ring, uint32_t flags, void *stream) {
    if (!env || n_steps < 0 || reset_every < 0 || step0 < 0 || ring < 1) return SSD_E_INVALID;
    if (flags & SSD_HOST_PTRS) { env->err = "ssd_rollout_random takes device pointers"; return SSD_E_INVALID; }
    if (num_actions < 1 || num_actions > game_actions(env)) { env->err = "num_actions outside the game's Discrete(n)"; return SSD_E_INVALID; }
    return rollout(env, nullptr, nullptr, 0, num_actions, n_steps, reset_every, step0, obs, rew, done, ring, flags, stream);
}

int ssd_rollout_actions(ssd_env *env, const int32_t *actions, const uint8_t *order, int32_t action_ring, int32_t n_steps, int32_t reset_every,
                        int32_t step0, void *obs, int32_t *rew, uint8_t *done, int32_t ring, uint32_t flags, void *stream) {
    if (!env || n_steps < 0 || reset_every < 0 || step0 < 0 || ring < 1 || action_ring < 1) return SSD_E_INVALID;
    if (flags & SSD_HOST_PTRS) { env->err = "ssd_rollout_actions takes device pointers"; return SSD_E_INVALID; }
    if (!actions && env->N > 0) { env->err = "actions is null"; return SSD_E_INVALID; }
    return rollout(env, actions, order, action_ring, 0, n_steps, reset_every, step0, obs, rew, done, ring, flags, stream);
}

int ssd_profiler_attached(void) { return ssd::aql::tool_attached_now(); }

int ssd_rollout_path(const ssd_env *env) { return env ? env->last_path : SSD_E_INVALID; }

int ssd_set_rollout_chains(ssd_env *env, int32_t chains) {
    if (!env || chains < 0 || chains > 8) return SSD_E_INVALID;
    env->rollout_chains = chains;
    return SSD_OK;
}

}  // extern "C"
