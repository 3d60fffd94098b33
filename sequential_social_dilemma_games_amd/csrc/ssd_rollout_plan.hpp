// csrc/ssd_rollout_plan.hpp -- the decisions of a rollout through the library's own dispatch queues, as pure host code: which form a
// call takes, which kinds of launches an argument set holds blocks for, what every block's kernel parameters are, and which
// packets go out in which order with which fences and doorbells.  No HIP here: ssd_rollout.hip does what this header decides,
// and tests/native/rollout_plan_driver.cpp walks it on the CPU.  (ssd_internal.hpp names uint4: a host compiler's includer
// defines it first.)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ssd_internal.hpp"

#ifndef SSD_RING_EVERY            // (experiment switch: 1 = a doorbell per step and chain)
#define SSD_RING_EVERY 4
#endif

namespace ssd {
namespace plan __attribute__((visibility("hidden"))) {     // (inline host code: none of it is part of the library's surface)

// Kinds of launches a rollout is made of, each for both ORIENTATIONS o of the handle's pair of state buffers (o = which
// of the two holds the current state; a launch of a split rollout reads buffer o and writes buffer 1 - o):
//   kS   step with observations, state in place (rollouts that are not split)     kR   reset with observations, in place
//   kRn  reset that renders nothing (inside a split rollout), in place
//   kA   the first step of a split rollout: env waves only                        kAB  env waves + renderer workgroups for the step before
//   kB   renderer workgroups only, for the step that produced buffer o (ends a split rollout, and precedes a reset inside one)
// Step runs (key.pairs = the longest run, 2 .. kMaxRun; the step-pair kernel, ssd::kModeStepPair): a launch whose env waves take n
// steps -- block i then serves steps i .. i + n - 1 -- and the launches that follow one, whose renderer workgroups deliver all of
// its steps' observations:
//   run_kind(n, rendered)   n = 1 .. kMaxRun steps + renderers for the `rendered` = 0 .. kMaxRun steps of the launch before
//   run_kind(0, rendered)   renderer workgroups only, for the run that produced buffer o
// (a single step behind nothing or behind a single step is kA / kAB, the renderers for a single step kB, as without runs)
enum Kind { kS = 0, kR = 1, kRn = 2, kA = 3, kAB = 4, kB = 5, kRun = 6, kKindsPerO = kRun + (kMaxRun + 1) * (kMaxRun + 1), kKinds = 2 * kKindsPerO };
constexpr int run_kind(int n, int rendered) { return kRun + n * (kMaxRun + 1) + rendered; }
// the step counts a launch takes under a run cap (0: no runs): 1, 2 and the cap itself -- 4 in the product, 3 under the test hook
constexpr bool run_len(int n, int cap) { return n == 1 || (n == 2 && cap >= 2) || (n > 2 && n == cap); }
// whether a key with this run cap has a block for kind `base` (of either orientation)
constexpr bool run_kind_used(int base, int cap) {
    const int n = (base - kRun) / (kMaxRun + 1), rd = (base - kRun) % (kMaxRun + 1);
    if (n > 0 ? !run_len(n, cap) : rd == 0) return false;
    if (rd > 0 && !run_len(rd, cap)) return false;
    return n >= 2 || rd >= 2;
}

// The kinds the calls of a key (its `split`, its `pairs`) can use, and their places among the blocks of one chain and slot: only
// those have a block (-1: none; without the pair of state buffers there is one orientation).  The schedule below names no other.
struct KindTable { int8_t dense[kKinds]; int n_dense; };
inline KindTable kind_table(int split, int pairs) {
    KindTable t;
    t.n_dense = 0;
    for (int kind = 0; kind < kKinds; ++kind) {
        const int o = kind / kKindsPerO, base = kind % kKindsPerO;
        const bool split_kind = base >= kRn, run = base >= kRun;
        const bool used = !(split_kind && !split) && !(run && !run_kind_used(base, pairs)) && !(!split && o == 1);
        t.dense[kind] = used ? (int8_t)t.n_dense++ : (int8_t)-1;
    }
    return t;
}

// Long launches (long calls alone -- choose_form; the long kernels, ssd::kModeStepLong): the launches that take or render a run of
// kLongRun = 8 steps.  A family of kinds of its own, numbered behind kKinds, with a dense table of its own: (n, rendered) with n or
// rendered equal to kLongRun and the other one of 0, 1, 2, 4, kLongRun.  Per orientation: the five (kLongRun, rendered) in that
// order of `rendered`, then the four (n, kLongRun) with n below kLongRun.  Only a key whose set is long (Key::long_cap) holds blocks
// for them; every other launch of a long call is of the kinds above, as in a call that is not long.
constexpr int kLongLens = 5;
constexpr int kLongLen[kLongLens] = {0, 1, 2, 4, kLongRun};
constexpr int kLongPerO = 2 * kLongLens - 1, kLongKinds = 2 * kLongPerO, kAllKinds = kKinds + kLongKinds;
constexpr int long_len_index(int n) { return n == 0 ? 0 : n == 1 ? 1 : n == 2 ? 2 : n == 4 ? 3 : n == kLongRun ? 4 : -1; }
constexpr bool is_long_kind(int kind) { return kind >= kKinds; }
// (n, rendered) is a long launch
constexpr bool long_counts(int n, int rendered) {
    return (n == kLongRun && long_len_index(rendered) >= 0) || (rendered == kLongRun && long_len_index(n) >= 0);
}
constexpr int long_kind(int o, int n, int rendered) {
    return kKinds + o * kLongPerO + (n == kLongRun ? long_len_index(rendered) : kLongLens + long_len_index(n));
}
constexpr int long_kind_o(int kind) { return (kind - kKinds) / kLongPerO; }
constexpr int long_kind_n(int kind) { return (kind - kKinds) % kLongPerO < kLongLens ? kLongRun : kLongLen[(kind - kKinds) % kLongPerO - kLongLens]; }
constexpr int long_kind_rendered(int kind) { return (kind - kKinds) % kLongPerO < kLongLens ? kLongLen[(kind - kKinds) % kLongPerO] : kLongRun; }
// their places among the long blocks of one chain and slot: dense[kind - kKinds] (-1: none)
struct LongKindTable { int8_t dense[kLongKinds]; int n_dense; };
inline LongKindTable long_kind_table(int long_cap) {
    LongKindTable t;
    t.n_dense = 0;
    for (int k = 0; k < kLongKinds; ++k) t.dense[k] = long_cap == kLongRun ? (int8_t)t.n_dense++ : (int8_t)-1;
    return t;
}

// What an argument set is cached by: everything the caller passed that its blocks name.
struct Key {
    const void *obs = nullptr, *rew = nullptr, *done = nullptr;
    int32_t ring = 0, f32 = 0, num_actions = 0, chains = 0, horizon = 0, coherent = 0, split = 0, pairs = 0;
    const void *actions = nullptr, *order = nullptr; int32_t action_ring = 0;  // caller-supplied actions: part of every step launch's arguments
    int32_t slots = 0;                                       // argument blocks per chain and kind: lcm(ring, action_ring)
    const void *stamps = nullptr; uint32_t dbg_skip = 0;     // (diagnostic builds: part of the kernel arguments too)
    const void *world = nullptr;                             // sets that are not split: the state buffer their blocks name
    int32_t long_cap = 0;                                    // kLongRun: the set also holds the long launches' blocks (Form::key_long)
    bool operator==(const Key &o) const {
        return long_cap == o.long_cap && stamps == o.stamps && dbg_skip == o.dbg_skip && world == o.world && obs == o.obs && rew == o.rew && done == o.done && ring == o.ring && f32 == o.f32 && num_actions == o.num_actions &&
               chains == o.chains && horizon == o.horizon && coherent == o.coherent && split == o.split && pairs == o.pairs && actions == o.actions && order == o.order &&
               action_ring == o.action_ring && slots == o.slots;
    }
};

// One argument block per chain, kind and residue of the step index modulo lcm(output ring, action ring; 0 = none).  0: refused.
inline int32_t block_slots(int32_t ring, int32_t action_ring, int chains) {
    const long long ar = action_ring > 0 ? action_ring : 1;
    long long a = ring, b = ar;
    while (b) { const long long t = a % b; a = b; b = t; }
    const long long l = (long long)ring / a * ar;
    if (l * chains > 2048) return 0;                            // (up to 36 x 896 B per chain and block index, a long set's 18 x 1216 B more)
    return (int32_t)l;
}

// The form of a call.  The knobs are the values of the environment variables of their names (read by the caller, once per process).
struct FormIn {
    int per_launch, chains;                  // envs per launch, chains of the call
    bool f32, order, obs;                    // float32 observations; an explicit action order; observations wanted at all
    int n_steps;
    int fast_profile, pair_profile;          // ssd::fast_profile(), ssd::pair_profile() of the handle
    int aql_coherent, aql_split, aql_alternate, aql_pairs, aql_run;   // SSD_AQL_COHERENT, _SPLIT, _ALTERNATE, _PAIRS, _RUN
    int long_profile;                        // ssd::long_profile() of the handle: kLongRun where its kernel has a long form, else 0
};
struct Form {
    int coherent;                            // key.coherent: 0 plain kernels, 1 coherent, 2 coherent with alternating geometries
    int key_split;                           // key.split: the argument set holds the split launches
    bool split;                              // this call is split
    int pairs;                               // key.pairs: the longest run the set has blocks for (0: none)
    int run_cap;                             // the longest run of this call (0: single steps)
    int long_cap;                            // kLongRun: this call is LONG -- runs of kLongRun wherever that many steps remain, run_cap elsewhere (0: not)
    int key_long;                            // key.long_cap: kLongRun where the argument set also holds the long launches (the form CAN be long)
};
// A call is long from this many steps on.  (Above 45, the longest call the suite pins to runs of four.  Measured, EXPERIMENTS.md
// round 28: a long call's closing renderer-only launch delivers eight steps per wave instead of four, some 10 us more per call --
// behind calls of its own length a 64-step call gains nothing, a 128-step call 0.06 us per step, calls of 600 and 1000 steps 0.15;
// and a process's FIRST long call runs a kernel no launch has run before, 20 us: at 64 steps a loss of 0.3 us per step.  From 256
// steps on a call gains even there.)
constexpr int kLongCallSteps = 256;
inline Form choose_form(const FormIn &in) {
    Form f;
    // Coherent chains: with a map-specific uint8 kernel (and its write-through observation stores: up to 16 384 envs per launch)
    // state and outputs move with agent-scope accesses only, so the step packets need no release fence (ssd_kernels.hip, COH).
    // SSD_AQL_COHERENT=0 keeps the plain kernels with agent-scope acquire + release on every packet; SSD_AQL_ALTERNATE=1 (test
    // hook) makes every other launch use half the envs per workgroup -- an env then changes workgroup, and with it XCD and L2,
    // from one launch to the next that touches it.
    // (measured, us per step: 2048 envs per launch 5.5 split / 5.9 coherent / 6.2 plain; 2730: 9.7 / 8.6 / 8.7; 5461: 19.1 / 15.2 /
    // 14.3 -- once a launch is several rounds of waves the kernel is bandwidth-bound, and re-reading state from an L2 that still
    // holds it beats fetching it from memory: coherent chains up to 4096 envs per launch, split ones up to 2304 -- 3072 in a single chain, below)
    // (an explicit action order takes the general kernels: no coherent variant)
    const bool coherent = in.aql_coherent != 0 && !in.f32 && !in.order && in.fast_profile > 0 && in.per_launch <= 4096;
    f.coherent = coherent ? (in.aql_alternate != 0 ? 2 : 1) : 0;
    // Split rollouts (coherent chains with observations, 4 steps or more): the wave that steps an env does not render its
    // observations; the NEXT step's launch carries a second set of workgroups that render them while that step is being computed,
    // from the very state that launch steps from (the handle's state lives in a pair of buffers: a launch reads one and writes the
    // other) plus the step's beam marks, which travel as a list; a last launch of renderer workgroups alone delivers the last step's.
    // Still one launch per step and env range (+ 1 per call and per reset inside it), every step's observations in its ring slot
    // when the call's work is done; but the observation phase (1.2 of 5.7 us) is off the chain of dependent launches.  (Two
    // launches per step in one queue -- step, then an observe launch beside the next step -- do not work: kernels of one queue run
    // one after the other on this device even without the barrier bit: two chains' launches in ONE queue take 10.6 us per step, in
    // two queues 5.8.)  SSD_AQL_SPLIT=0 turns it off.
    // The split cap depends on the chains: with two chains of 2730 envs the split launches no longer fit one round of waves, hence
    // 2304; a single chain (a pool of one queue) gains from splitting up to 3072 envs and loses at 4096 (measured, Harvest, us per
    // step split / unsplit: 3072 envs 4.88 / 6.30, 4096 envs 6.96 / 6.54; profiles/r05_ab/).
    const int split_cap = in.chains == 1 ? 3072 : 2304;
    f.key_split = (coherent && in.aql_split != 0 && in.obs && in.per_launch <= split_cap) ? 1 : 0;   // (the argument set holds both forms' launches)
    f.split = f.key_split && in.n_steps >= 4;
    // Step runs: a split chain's launches advance their envs by a RUN of steps each -- four wherever four steps remain before the
    // call's end and before the next reset, else two where two remain, else one -- a quarter of the dependent launches, and every
    // step behind a launch's first starts from the env as it stands in LDS and registers, without a prologue.  Every step still
    // lands in its ring slot and is rendered by the next launch's extra workgroups, a whole run per renderer wave.  As long as the
    // form's step-pair kernel is built for (ssd_kernels.hip, pair_profile: four, two, or no runs at all); the argument set then holds
    // all forms' launches.  (Test-hook build: SSD_AQL_PAIRS=0 keeps single steps, SSD_AQL_RUN=1 .. 4 caps the run -- at 3 the launches
    // take three steps, two and one, which no product call does -- same results.)
    int cap = (f.key_split && in.aql_pairs != 0) ? in.pair_profile : 1;
    if (in.aql_run >= 1 && in.aql_run < cap) cap = in.aql_run;
    f.pairs = cap >= 2 ? cap : 0;
    f.run_cap = f.split ? f.pairs : 0;
    // Long calls: a split call of kLongCallSteps steps or more whose kernel has a long form takes runs of kLongRun = 8 -- half the
    // dependent launches again, the fixed cost of a launch (2.4 us) spread over eight steps.  The call's length decides once, for
    // the whole call; every shorter call plans exactly as above.  Only beside runs of four (a capped run has no long form), and not
    // under SSD_AQL_RUN = 1 .. 7 (test-hook build: SSD_AQL_RUN=4 gives a long call the plan of a call that is not).
    // The argument set holds the long launches wherever the form can be long, whatever this call's length (as a split set holds the
    // launches of calls too short to be split): a handle's first long call then finds its blocks and its mid sets in place, and
    // pays for neither in the middle of a loop of calls.
    f.key_long = (f.key_split && f.pairs == kMaxRun && in.long_profile >= kLongRun && (in.aql_run < 1 || in.aql_run >= kLongRun)) ? kLongRun : 0;
    f.long_cap = (f.key_long && f.split && in.n_steps >= kLongCallSteps) ? kLongRun : 0;
    return f;
}

// An observation ring that does not fit the device's 256-MB memory-side cache: the write-through stores bypass it (non-temporal).
// One slot rewritten every step lives in that cache (4096 envs: 13.8 MB, 5.43 us per step; 6.91 if it bypassed it); 16 slots
// (221 MB) still do: 5.50 (7.06 bypassing); 32 slots (442 MB) thrash it: 8.07 us per step, with non-temporal stores 7.03
// (`python bench.py --ring R`, alternating fresh processes).
inline bool ring_past_cache(const void *obs, int32_t ring, size_t obs_bytes) { return obs && (size_t)ring * obs_bytes > ((size_t)232 << 20); }

// A chain's output and action rings: slot s of a ring lies s * en elements (observations: s * ob bytes) behind its base.
struct ChainRings {
    uint8_t *obs; int32_t *rew; uint8_t *done;
    const int32_t *actions; const uint8_t *order; int32_t action_ring;
    size_t en, ob;
    int32_t num_actions;
};
// the step launch's action source: the caller's slot of the action ring, or the device's own draw
inline void cursor_actions(const ChainRings &c, Params &p, size_t step_index) {
    if (c.actions) {
        const size_t at = (step_index % (size_t)c.action_ring) * c.en;
        p.actions = c.actions + at; p.order = c.order ? c.order + at : nullptr; p.num_actions_random = 0;
    } else { p.actions = nullptr; p.order = nullptr; p.num_actions_random = c.num_actions; }
}

// The buffers of split rollouts, once per handle.
constexpr int kMids = kMaxRun - 1, kLongMids = kLongRun - 1;
struct SplitBuffers {
    uint8_t *world_buf[2] = {};                     // the pair of state buffers ([0]: the handle's original ones)
    uint32_t *agents_buf[2] = {};
    uint32_t *beam_list[2] = {};                    // [2][E][64] beam marks left by a launch of orientation o (second half: a second pass's)
    uint8_t *snap_grid[2] = {};                     // [E][S] overlay snapshot left by a launch of orientation o (rare steps)
    // the same four for what pass k of a run launch of orientation o left, for every pass but the run's last: [k][o] (read by the next
    // launch's renderers alone)
    uint8_t *mid_world[kMids][2] = {}, *mid_snap[kMids][2] = {};
    uint32_t *mid_agents[kMids][2] = {}, *mid_list[kMids][2] = {};
    // long calls: the mid sets of passes kMids .. kLongRun - 2 of a run of kLongRun, [k - kMids][o] (allocated with the handle's first
    // long argument set, all or none)
    uint8_t *long_world[kLongMids - kMids][2] = {}, *long_snap[kLongMids - kMids][2] = {};
    uint32_t *long_agents[kLongMids - kMids][2] = {}, *long_list[kLongMids - kMids][2] = {};
    // mid set [k][o], k = 0 .. kLongRun - 2, wherever it lives
    struct MidSet { uint8_t *world; uint32_t *agents; uint32_t *list; uint8_t *snap; };
    MidSet mid_set(int k, int o) const {
        if (k < kMids) return MidSet{mid_world[k][o], mid_agents[k][o], mid_list[k][o], mid_snap[k][o]};
        return MidSet{long_world[k - kMids][o], long_agents[k - kMids][o], long_list[k - kMids][o], long_snap[k - kMids][o]};
    }
};

// The step-run part of a block, for the step-pair kernels' PairParams (kMax = kMaxRun) and the long kernels' LongParams (kMax =
// kLongRun) alike: Q's arrays hold kMax pass records and kMax - 1 mid inputs.
// Block i serves steps i .. i + n - 1 (output slots r .. r + n - 1, action slots likewise).  The env waves read buffer o, leave pass
// k of their first n - 1 in mid set [k][o] and their last in buffer 1 - o with its marks in list o, as a single step's.  The
// renderer workgroups deliver the `rd` steps of the launch before (orientation 1 - o): its last step -- or a single step -- from
// buffer o and list 1 - o, the steps before it from mid sets [.][1 - o]; into the rd slots before r (renderer workgroups only: the
// run is this block's own, slots r .. r + rd - 1).
template <int kMax, class Q>
inline void fill_run(const ChainRings &cur, const Key &key, const SplitBuffers &A, int o, int n, int rd, int i, int r, int mode, Params &p, Q &q) {
    auto ring_slot = [&](int d) { return ((r + d) % key.ring + key.ring) % key.ring; };
    auto slot_obs = [&](int sl) { return cur.obs ? cur.obs + (size_t)sl * cur.ob : nullptr; };
    p.mode = mode;
    p.obs = nullptr;
    p.snap_mode = (n == 0 ? 4 : 1) | (rd > 0 ? 2 : 0);
    p.world_out = A.world_buf[1 - o]; p.agents_out = A.agents_buf[1 - o];
    p.beam_list = A.beam_list[o]; p.snap = A.snap_grid[o];
    p.beam_list_in = A.beam_list[1 - o]; p.snap_in = A.snap_grid[1 - o];
    // (the env waves' records, one per pass of the launch: every pass but the last into its mid set of orientation
    // o, the launch's last step as a single step's -- each with the ring and action slots of its own step)
    q.n_pass = n; q.n_render = rd;
    for (int k = 0; k < n; ++k) {
        const int rk = ring_slot(k);
        PassRec &rec = q.pass[k];
        const SplitBuffers::MidSet m = k + 1 < n ? A.mid_set(k, o) : SplitBuffers::MidSet{p.world_out, p.agents_out, p.beam_list, p.snap};
        rec = PassRec{m.world, m.agents, m.list, m.snap, nullptr, nullptr, nullptr};
        rec.rew = cur.rew ? cur.rew + (size_t)rk * cur.en : nullptr;
        rec.done = cur.done ? cur.done + (size_t)rk * cur.en : nullptr;
        rec.actions = cur.actions ? cur.actions + ((size_t)(i + k) % (size_t)cur.action_ring) * cur.en : nullptr;
    }
    // (the renderers' inputs, laid out from the run's end: slot kMax - 1 is its last step -- p.beam_list_in, p.snap_in,
    // p.obs_b -- and slot t the step kMax - 1 - t before it, which is step j = t - (kMax - rd) of the run)
    const int first = n == 0 ? 0 : -rd;      // (ring slot of the run's first step, relative to r)
    for (int t = kMax - rd; t < kMax - 1; ++t) {
        if (t < 0) continue;
        const int j = t - (kMax - rd);
        const SplitBuffers::MidSet m = A.mid_set(j, 1 - o);
        q.mid_in[t] = MidIn{m.world, m.agents, m.list, m.snap};
        q.obs_b0[t] = slot_obs(ring_slot(first + j));
    }
    p.obs_b = slot_obs(ring_slot(first + rd - 1));
}

// The kernel parameters of argument block (kind, i) of a chain: `base` is the chain's Params (its env range, the call's constant
// fields), block i serves the steps whose index is i modulo key.slots -- output slot i % key.ring, action slot i % action_ring.
// q is the block of a step-run kind (else left empty).
inline void fill_block(const Params &base, const ChainRings &cur, const Key &key, const SplitBuffers &A, int kind, int i, Params &p, PairParams &q) {
    const int r = i % key.ring;
    const int o = kind / kKindsPerO, kb = kind % kKindsPerO;
    const bool pair_kind = kb >= kRun;
    p = base;
    q = PairParams{};
    if (key.split) { p.world = A.world_buf[o]; p.agents = A.agents_buf[o]; }     // the launch reads buffer o
    p.obs = cur.obs ? cur.obs + (size_t)r * cur.ob : nullptr;
    // (test hook: launches of orientation 1 use the other geometry)
    p.coherent = key.coherent ? ((key.coherent == 2 && o == 1) ? 2u : 1u) : 0u;
    if (kb == kR || kb == kRn) {
        p.mode = kModeReset; p.rotate = 0; p.num_actions_random = 0; p.actions = nullptr; p.order = nullptr; p.rew = nullptr; p.done = nullptr;
        // (every reset of a rollout is followed by a step that writes the same observation slot)
        if (kb == kRn) p.obs = nullptr;
        return;
    }
    p.mode = kModeStep; p.rotate = 1;
    cursor_actions(cur, p, (size_t)i);
    p.rew = cur.rew ? cur.rew + (size_t)r * cur.en : nullptr; p.done = cur.done ? cur.done + (size_t)r * cur.en : nullptr;
    if (pair_kind) {
        fill_run<kMaxRun>(cur, key, A, o, (kb - kRun) / (kMaxRun + 1), (kb - kRun) % (kMaxRun + 1), i, r, kModeStepPair, p, q);
    } else if (kb >= kA) {
        // env waves: read buffer o, write buffer 1 - o, leave their beam marks in list o.  Renderer workgroups of
        // a kAB launch: the step before produced buffer o (a launch of orientation 1 - o: its marks are in list
        // 1 - o), its observations go to the ring slot before this one; of a kB launch: the same for THIS slot.
        uint8_t *obs_r = p.obs;
        uint8_t *obs_prev = cur.obs ? cur.obs + (size_t)((r + key.ring - 1) % key.ring) * cur.ob : nullptr;
        p.obs = nullptr;
        p.snap_mode = 1;
        p.world_out = A.world_buf[1 - o]; p.agents_out = A.agents_buf[1 - o];
        p.beam_list = A.beam_list[o]; p.snap = A.snap_grid[o];
        if (kb != kA) {
            p.snap_mode = kb == kB ? (2 | 4) : (1 | 2);
            p.beam_list_in = A.beam_list[1 - o]; p.snap_in = A.snap_grid[1 - o];
            p.obs_b = kb == kB ? obs_r : obs_prev;
        }
    }
}

// The same for a long kind (is_long_kind; a long set): the step launch's Params with ssd::kModeStepLong, and the launch's LongParams.
inline void fill_long_block(const Params &base, const ChainRings &cur, const Key &key, const SplitBuffers &A, int kind, int i, Params &p, LongParams &q) {
    const int r = i % key.ring, o = long_kind_o(kind);
    p = base;
    q = LongParams{};
    p.world = A.world_buf[o]; p.agents = A.agents_buf[o];
    p.coherent = key.coherent ? ((key.coherent == 2 && o == 1) ? 2u : 1u) : 0u;
    p.rotate = 1;
    cursor_actions(cur, p, (size_t)i);
    p.rew = cur.rew ? cur.rew + (size_t)r * cur.en : nullptr; p.done = cur.done ? cur.done + (size_t)r * cur.en : nullptr;
    fill_run<kLongRun>(cur, key, A, o, long_kind_n(kind), long_kind_rendered(kind), i, r, kModeStepLong, p, q);
}

// The orientation a call starts from: which buffer of the pair holds the current state (always 0 until the first split rollout of
// the handle).  Only a split set has blocks for both; any other set names the current buffer in the blocks of its one orientation
// (Key::world), wherever the state sits.
inline int start_orientation(int key_split, bool state_in_second_buffer) { return key_split && state_in_second_buffer ? 1 : 0; }

// The packets of a call, for ONE chain (every chain's are the same): group by group -- a group is one step launch with what goes
// ahead of it (a reset, and ahead of that the renderers of the run before) and, at the call's end, behind it -- so that the caller
// writes and rings a group before the next is planned.  Every packet carries the barrier bit.
struct Packet {
    size_t block;                // argument block of the chain: (step0 + step) % slots of the step it serves
    int kind;                    // Kind + orientation * kKindsPerO
    int acquire, release;        // fence scopes (hsa_fence_scope_t: 0 none, 1 agent, 2 system)
};
struct Group {
    Packet packet[4]; int n_packets;
    int step, steps;             // the step launch takes steps step .. step + steps - 1 of the call
    bool reset;                  // ... behind a reset
    bool ring;                   // ring the doorbell after this group
};
class Schedule {
public:
    // split: the call is split (launches alternate between the state buffers, from orientation o); run_cap: its longest run (0: single
    // steps; split calls only); coherent: coherent chains (the doorbell rule); obs_wb: the output ring is written with write-back
    // stores (ring_past_cache, uint8); acq / rel: the fence scopes of the chain's own packets; long_cap: kLongRun in a long call
    // (Form::long_cap: a launch takes kLongRun steps wherever that many remain before the call's end and the next reset, else
    // what run_cap gives; launches that take or render such a run are of the long kinds), else 0.
    Schedule(int n_steps, int step0, int reset_every, int ring, int slots, bool split, int run_cap, bool coherent, bool obs_wb, int acq, int rel, int o,
             int long_cap = 0)
        : n_steps_(n_steps), step0_(step0), reset_every_(reset_every), ring_(ring), slots_(slots), split_(split), run_cap_(split ? run_cap : 0),
          long_cap_((split && run_cap == kMaxRun && long_cap == kLongRun) ? kLongRun : 0), coherent_(coherent), obs_wb_(obs_wb), kAcq(acq), kRel(rel), o_(o) {}
    __attribute__((always_inline)) bool next(Group &g) {       // (into the enqueue loop: its state then lives in registers)
        const int k = k_;
        if (k >= n_steps_) return false;
        const int KO = kKindsPerO;
        const size_t i = (size_t)((step0_ + k) % slots_);   // argument block of this step (output slot i % ring, action slot i % action_ring)
        const bool reset = reset_every_ > 0 && (step0_ + k) % reset_every_ == 0;
        // (a run never spans a reset or the call's end: the steps left before either go as shorter runs and single launches)
        int avail = n_steps_ - k;
        if (reset_every_ > 0) { const int to_reset = reset_every_ - (step0_ + k) % reset_every_; if (to_reset < avail) avail = to_reset; }
        const int n = (long_cap_ > 0 && avail >= long_cap_) ? long_cap_ : (run_cap_ > 2 && avail >= run_cap_) ? run_cap_ : (run_cap_ >= 2 && avail >= 2) ? 2 : 1;
        const bool last = k + n >= n_steps_;
        const int acq = k == 0 ? 1 : kAcq;                                 // (the call's first launch of the chain)
        Packet *pk = g.packet;
        if (reset) {
            // (a reset works in place: the launch before it must have been rendered from that buffer first)
            if (split_ && pending_) *pk++ = Packet{i_prev_, render_kind(o_, pending_), kAcq, kRel};
            *pk++ = Packet{i, o_ * KO + (split_ ? kRn : kR), acq, kRel};
        }
        const int rendered = reset ? 0 : pending_;
        const int base = !split_ ? (int)kS
                         : (n == 1 && rendered <= 1) ? (rendered == 1 ? (int)kAB : (int)kA)
                                                     : run_kind(n, rendered);
        // (an output ring past the memory-side cache is written with write-back stores, ssd_kernels.hip select(): one launch per
        // round of the ring releases at agent scope, so that whatever of a slot still sits dirty in an L2 is in memory before
        // the slot's bytes are written again -- possibly through another XCD's L2; a run releases for any of its steps)
        bool round = false;
        for (int j = 0; j < n; ++j) round = round || (step0_ + k + j) % ring_ == 0;
        const int rel = (obs_wb_ && round) ? 1 : kRel;
        // (a launch that takes or renders a run of kLongRun: its long kind)
        const int kind = (n == kLongRun || rendered == kLongRun) ? long_kind(o_, n, rendered) : o_ * KO + base;
        *pk++ = Packet{i, kind, reset ? kAcq : acq, rel};
        if (split_ && last) *pk++ = Packet{i, render_kind(1 - o_, n), kAcq, kRel};   // (renders the buffer this launch wrote)
        g.n_packets = (int)(pk - g.packet);
        g.step = k; g.steps = n; g.reset = reset;
        // (the doorbell -- an uncached write across the bus, 0.3 - 0.5 us -- after the first two launches, so that the device starts
        // at once, and then after every fourth: the device needs 5 us per step, the host under 1, it never runs dry; the join
        // rings for the rest.  Runs longer than two: after every launch -- one lasts some 14 us, and four of them unannounced
        // would leave the device with nothing to start on after the first two)
#if SSD_RING_EVERY > 1
        g.ring = !coherent_ || launches_ < 2 || run_cap_ > 2 || (launches_ % SSD_RING_EVERY) == SSD_RING_EVERY - 1;   // (large launches: every step, as ever)
#else
        g.ring = true;
#endif
        if (split_) { o_ = 1 - o_; pending_ = n; i_prev_ = i; }
        if (n > longest_) longest_ = n;
        launches_++;
        k_ = k + n;
        return true;
    }
    int orientation() const { return o_; }       // after the last group: the buffer of the pair that holds the current state
    int longest() const { return longest_; }     // the longest run one launch took
    // (the renderer workgroups that deliver a run of `rendered` steps, alone: a single step's are kB)
    static constexpr int render_only(int rendered) { return rendered == 1 ? (int)kB : run_kind(0, rendered); }
    // (... of orientation o, with the orientation in the kind: a run of kLongRun takes the long kind)
    static constexpr int render_kind(int o, int rendered) { return rendered == kLongRun ? long_kind(o, 0, rendered) : o * kKindsPerO + render_only(rendered); }

private:
    int n_steps_, step0_, reset_every_, ring_, slots_;
    bool split_; int run_cap_, long_cap_; bool coherent_, obs_wb_;
    int kAcq, kRel;
    int o_;                      // orientation: which buffer of the pair holds the current state
    int k_ = 0;
    int pending_ = 0;            // steps of the launch before whose observations are still to be rendered (split rollouts)
    size_t i_prev_ = 0;
    int launches_ = 0;           // step launches so far
    int longest_ = 0;
};

}  // namespace plan
}  // namespace ssd
