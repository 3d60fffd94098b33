// tests/native/rollout_plan_driver.cpp -- walks csrc/ssd_rollout_plan.hpp (what a rollout through the library's own dispatch queues
// sends: kinds, argument blocks, packets, fences, doorbells, the form of a call) over a grid of calls and checks every plan by a
// symbolic run of its packets.  Compiled with g++ by tests/test_rollout_plan_cpu.py; prints one line per group, "ok" last.
#include <cstdio>
#include <cstring>

struct uint4 { unsigned x, y, z, w; };      // (ssd_internal.hpp names HIP's vector type in pointers only)
#include "ssd_rollout_plan.hpp"

using namespace ssd;
using namespace ssd::plan;

static_assert(sizeof(Params) == 416 && sizeof(PairKernArgs) == 824, "the kernel argument layout the library is built with");

#define REQUIRE(cond)                                                                                                  \
    do {                                                                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n   in %s\n", __LINE__, #cond, g_case); return false; }         \
    } while (0)
static char g_case[256] = "(no case)";

// Fake device memory: every buffer is one 64-byte cell of an arena, so a pointer names its buffer and nothing is ever dereferenced.
static uint8_t g_arena[1 << 16];
constexpr int kCell = 64, kStateCells = 64;          // (the state, list and snapshot buffers are the arena's first cells)
static int cell_of(const void *ptr) { return (int)((static_cast<const uint8_t *>(ptr) - g_arena) / kCell); }
// the output and action rings: slot s lies s * en = 16 elements (observations: s * ob = 64 bytes) behind the ring's base
static uint8_t *const kObs = g_arena + 100 * kCell, *const kDone = g_arena + 400 * kCell, *const kOrder = g_arena + 700 * kCell;
static int32_t *const kRew = reinterpret_cast<int32_t *>(g_arena + 200 * kCell);
static const int32_t *const kActions = reinterpret_cast<const int32_t *>(g_arena + 500 * kCell);

namespace {

struct Case { int n_steps, step0, reset_every, ring, action_ring, cap, split, o0, coherent; };

// What the buffers hold.  State buffers (grid, agents): 2 * k + r = the state step k starts from, r = its reset applied (so the
// state step k leaves is 2 * (k + 1)); mark lists and snapshots: the step whose marks they hold.  -1: nothing yet.
struct Machine {
    Case c;
    int slots;
    Key key;
    SplitBuffers B;
    Params base;
    ChainRings rings;
    int tag[kStateCells];
    int next_step = 0;                       // steps computed so far
    int delivered[32] = {};                  // observations written, per step
    bool reset_due(int k) const { return c.reset_every > 0 && (c.step0 + k) % c.reset_every == 0; }
    int out_slot(int k) const { return (c.step0 + k) % c.ring; }

    explicit Machine(const Case &cs) : c(cs) {
        std::memset(&base, 0, sizeof base);
        for (int &t : tag) t = -1;
        uint8_t *a = g_arena;
        auto cell = [&]() { a += kCell; return a; };
        for (int o = 0; o < 2; ++o) {
            B.world_buf[o] = cell(); B.agents_buf[o] = reinterpret_cast<uint32_t *>(cell());
            B.beam_list[o] = reinterpret_cast<uint32_t *>(cell()); B.snap_grid[o] = cell();
            for (int k = 0; k < kMids; ++k) {
                B.mid_world[k][o] = cell(); B.mid_snap[k][o] = cell();
                B.mid_agents[k][o] = reinterpret_cast<uint32_t *>(cell()); B.mid_list[k][o] = reinterpret_cast<uint32_t *>(cell());
            }
        }
        // a call that is not split reaches orientation 1 only through a split set (start_orientation): short calls of a handle
        // whose longer calls are split
        key.split = c.split || c.o0;
        key.pairs = (c.split && c.cap >= 2) ? c.cap : 0;
        key.ring = c.ring; key.action_ring = c.action_ring; key.coherent = c.coherent;
        slots = block_slots(c.ring, c.action_ring, 1);
        key.slots = slots;
        base.E = 48; base.e_begin = 16;
        base.world = B.world_buf[c.o0]; base.agents = B.agents_buf[c.o0];         // the handle's current state
        tag[cell_of(base.world)] = tag[cell_of(base.agents)] = 0;
        rings = ChainRings{kObs, kRew, kDone, c.action_ring ? kActions : nullptr, (c.action_ring && !c.split) ? kOrder : nullptr, c.action_ring, 16, 64, 8};
    }

    // the env waves' step k: from `in` (pass 0 of a launch alone reads memory) into the record's buffers
    bool env_step(int k, const uint8_t *in_world, const uint32_t *in_agents, const PassRec &out, const uint8_t *order) {
        REQUIRE(k == next_step && k < c.n_steps);                              // every step once, in order
        if (in_world) REQUIRE(tag[cell_of(in_world)] == 2 * k + reset_due(k) && tag[cell_of(in_agents)] == 2 * k + reset_due(k));
        tag[cell_of(out.world)] = tag[cell_of(out.agents)] = 2 * (k + 1);
        if (out.beam_list) tag[cell_of(out.beam_list)] = tag[cell_of(out.snap)] = k;
        REQUIRE(out.rew == kRew + out_slot(k) * 16 && out.done == kDone + out_slot(k) * 16);
        if (c.action_ring) {
            REQUIRE(out.actions == kActions + ((c.step0 + k) % c.action_ring) * 16);
            if (order) REQUIRE(order == kOrder + ((c.step0 + k) % c.action_ring) * 16);
        } else REQUIRE(!out.actions);
        next_step++;
        return true;
    }
    // a renderer wave delivers step k: from the state the step left, its marks and its snapshot, into the step's ring slot
    bool render(int k, const uint8_t *world, const uint32_t *agents, const uint32_t *list, const uint8_t *snap, const uint8_t *obs) {
        REQUIRE(k >= 0 && k < next_step);                                      // never before the step was computed
        REQUIRE(tag[cell_of(world)] == 2 * (k + 1) && tag[cell_of(agents)] == 2 * (k + 1));
        REQUIRE(tag[cell_of(list)] == k && tag[cell_of(snap)] == k);
        REQUIRE(obs == kObs + out_slot(k) * 64);
        REQUIRE(delivered[k] == 0);
        delivered[k] = 1;
        return true;
    }
    // One packet, by the kernels' contract (ssd_internal.hpp, PairParams; ssd_rollout_plan.hpp, Kind).  steps: the steps its env
    // waves take (0: none).
    bool execute(const Packet &pk, const KindTable &table, int *steps) {
        REQUIRE(pk.kind >= 0 && pk.kind < kKinds && table.dense[pk.kind] >= 0);            // the set has a block for it
        REQUIRE(pk.block < (size_t)slots);
        Params p; PairParams q;
        fill_block(base, rings, key, B, pk.kind, (int)pk.block, p, q);
        const int o = pk.kind / kKindsPerO, kb = pk.kind % kKindsPerO, k = next_step;
        REQUIRE(p.E == base.E && p.e_begin == base.e_begin);
        REQUIRE(p.coherent == (c.coherent ? 1u : 0u));
        *steps = 0;
        if (kb == kS || kb == kR || kb == kRn) {                               // in place, on the buffer that holds the current state
            REQUIRE(!p.world_out && !p.agents_out && p.snap_mode == 0);
            REQUIRE(p.world == (key.split ? B.world_buf[o] : base.world) && p.agents == (key.split ? B.agents_buf[o] : base.agents));
            if (kb == kS) {
                REQUIRE(p.mode == kModeStep && p.rotate == 1);
                if (!env_step(k, p.world, p.agents, PassRec{p.world, p.agents, nullptr, nullptr, p.rew, p.done, p.actions}, p.order)) return false;
                REQUIRE(p.num_actions_random == (c.action_ring ? 0 : 8) && (p.order != nullptr) == (rings.order != nullptr));
                REQUIRE(p.obs == kObs + out_slot(k) * 64 && delivered[k] == 0);
                delivered[k] = 1;
                *steps = 1;
                return true;
            }
            // a reset: of the state step k starts from, once everything before it has been rendered from that buffer
            REQUIRE(p.mode == kModeReset && p.rotate == 0 && !p.actions && !p.order && !p.rew && !p.done);
            REQUIRE(k < c.n_steps && reset_due(k));
            REQUIRE(tag[cell_of(p.world)] == 2 * k && tag[cell_of(p.agents)] == 2 * k);
            for (int j = 0; j < k; ++j) REQUIRE(delivered[j] == 1);
            tag[cell_of(p.world)] = tag[cell_of(p.agents)] = 2 * k + 1;
            // (kR's own observations go to the slot of the step behind it, which writes them again)
            REQUIRE(kb == kRn ? !p.obs : p.obs == kObs + out_slot(k) * 64);
            return true;
        }
        // the split kinds: read buffer o (+ what the launch before left), write buffer 1 - o, list o, snapshot o and mid sets [.][o]
        REQUIRE(key.split && !p.obs);
        REQUIRE(p.world == B.world_buf[o] && p.agents == B.agents_buf[o]);
        REQUIRE(p.world_out == B.world_buf[1 - o] && p.agents_out == B.agents_buf[1 - o] && p.beam_list == B.beam_list[o] && p.snap == B.snap_grid[o]);
        int n, rd;
        if (kb >= kRun) {
            n = (kb - kRun) / (kMaxRun + 1); rd = (kb - kRun) % (kMaxRun + 1);
            REQUIRE(p.mode == kModeStepPair && q.n_pass == n && q.n_render == rd && p.snap_mode == ((n == 0 ? 4 : 1) | (rd > 0 ? 2 : 0)));
            REQUIRE(run_kind_used(kb, key.pairs));
        } else {
            n = kb == kB ? 0 : 1; rd = kb == kA ? 0 : 1;
            REQUIRE(p.mode == kModeStep && p.snap_mode == (kb == kA ? 1 : kb == kAB ? 3 : 6));
        }
        // no launch writes what it or its renderers read
        const void *reads[2 + 2 + 4 * kMids], *writes[4 * kMaxRun];
        int n_reads = 0, n_writes = 0;
        if (n > 0 || rd > 0) { reads[n_reads++] = p.world; reads[n_reads++] = p.agents; }
        // the renderers: the rd steps of the launch before, the last of them from this launch's input state
        if (rd > 0) {
            reads[n_reads++] = p.beam_list_in; reads[n_reads++] = p.snap_in;
            for (int j = 0; j + 1 < rd; ++j) {
                const int t = kMaxRun - rd + j;
                const MidIn &m = q.mid_in[t];
                reads[n_reads++] = m.world; reads[n_reads++] = m.agents; reads[n_reads++] = m.beam_list; reads[n_reads++] = m.snap;
                if (!render(k - rd + j, m.world, m.agents, m.beam_list, m.snap, q.obs_b0[t])) return false;
            }
            if (!render(k - 1, p.world, p.agents, p.beam_list_in, p.snap_in, p.obs_b)) return false;
        }
        // the env waves: n passes, every one but the last into its mid set, the last as a single step's
        for (int j = 0; j < n; ++j) {
            PassRec rec = kb >= kRun ? q.pass[j] : PassRec{p.world_out, p.agents_out, p.beam_list, p.snap, p.rew, p.done, p.actions};
            if (j + 1 == n) REQUIRE(rec.world == p.world_out && rec.agents == p.agents_out && rec.beam_list == p.beam_list && rec.snap == p.snap);
            else REQUIRE(rec.world == B.mid_world[j][o] && rec.agents == B.mid_agents[j][o] && rec.beam_list == B.mid_list[j][o] && rec.snap == B.mid_snap[j][o]);
            if (j == 0) REQUIRE(rec.actions == p.actions && rec.rew == p.rew && rec.done == p.done);   // (the first pass's: Params' own, the same pointers)
            writes[n_writes++] = rec.world; writes[n_writes++] = rec.agents; writes[n_writes++] = rec.beam_list; writes[n_writes++] = rec.snap;
            if (!env_step(k + j, j == 0 ? p.world : nullptr, p.agents, rec, nullptr)) return false;
        }
        if (n > 0) REQUIRE(p.num_actions_random == (c.action_ring ? 0 : 8));
        for (int a = 0; a < n_reads; ++a)
            for (int b = 0; b < n_writes; ++b) REQUIRE(reads[a] != writes[b]);
        for (int a = 0; a < n_writes; ++a)
            for (int b = 0; b < a; ++b) REQUIRE(writes[a] != writes[b]);
        *steps = n;
        return true;
    }
};

static bool is_reset(int kind) { const int kb = kind % kKindsPerO; return kb == kR || kb == kRn; }
static bool is_render_only(int kind) { const int kb = kind % kKindsPerO; return kb == kB || (kb >= kRun && (kb - kRun) / (kMaxRun + 1) == 0); }

// One call of the grid: plan it, check every group's shape, fences and doorbell, run its packets.
static bool check_case(const Case &c) {
    std::snprintf(g_case, sizeof g_case, "n_steps %d step0 %d reset_every %d ring %d action_ring %d cap %d split %d o %d coherent %d",
                  c.n_steps, c.step0, c.reset_every, c.ring, c.action_ring, c.cap, c.split, c.o0, c.coherent);
    Machine m(c);
    REQUIRE(m.slots > 0 && m.slots % c.ring == 0 && (c.action_ring == 0 || m.slots % c.action_ring == 0));
    const KindTable table = kind_table(m.key.split, m.key.pairs);
    const bool obs_wb = (c.n_steps + c.step0 + c.ring) % 3 == 0;      // (a property of the caller's ring: any case may have it)
    const int kAcq = c.coherent ? 0 : 1, kRel = c.coherent ? 0 : 1;
    const int run_cap = c.split ? c.cap : 0;
    Schedule sched(c.n_steps, c.step0, c.reset_every, c.ring, m.slots, c.split != 0, c.cap, c.coherent != 0, obs_wb, kAcq, kRel, c.o0);
    Group g;
    int groups = 0, longest = 0, flips = 0;
    bool first_packet = true, ended = false;
    size_t prev_block = 0;
    while (sched.next(g)) {
        REQUIRE(!ended && g.n_packets >= 1 && g.n_packets <= 4);
        REQUIRE(g.step == m.next_step && run_len(g.steps, run_cap) && g.step + g.steps <= c.n_steps);
        REQUIRE(g.reset == m.reset_due(g.step));
        for (int j = 1; j < g.steps; ++j) REQUIRE(!m.reset_due(g.step + j));               // a run never spans a reset
        const size_t block = (size_t)((c.step0 + g.step) % m.slots);
        // the group's shape: [renderers of the run before] [reset] step [renderers of this run, at the call's end]
        int at = 0;
        const bool pre_render = g.reset && c.split && g.step > 0;
        if (pre_render) { REQUIRE(is_render_only(g.packet[at].kind) && g.packet[at].block == prev_block); at++; }
        if (g.reset) { REQUIRE(is_reset(g.packet[at].kind) && g.packet[at].block == block); at++; }
        const int step_at = at;
        REQUIRE(!is_reset(g.packet[at].kind) && !is_render_only(g.packet[at].kind) && g.packet[at].block == block);
        at++;
        const bool last = g.step + g.steps == c.n_steps;
        if (last && c.split) { REQUIRE(is_render_only(g.packet[at].kind) && g.packet[at].block == block); at++; }
        REQUIRE(at == g.n_packets);
        // fences: the chain's first packet of the call acquires at agent scope; a ring written with write-back stores is released
        // once per round, by the launch that takes the round's first step
        bool round = false;
        for (int j = 0; j < g.steps; ++j) round = round || (c.step0 + g.step + j) % c.ring == 0;
        for (int j = 0; j < g.n_packets; ++j) {
            REQUIRE(g.packet[j].acquire == (first_packet ? 1 : kAcq));
            REQUIRE(g.packet[j].release == ((j == step_at && obs_wb && round) ? 1 : kRel));
            first_packet = false;
        }
        // the doorbell: every group of chains that are not coherent or run longer than two; else after the first two and every
        // SSD_RING_EVERY-th
        const bool want_ring = !c.coherent || groups < 2 || run_cap > 2 || SSD_RING_EVERY <= 1 || groups % SSD_RING_EVERY == SSD_RING_EVERY - 1;
        REQUIRE(g.ring == want_ring);
        for (int j = 0; j < g.n_packets; ++j) {
            int steps = 0;
            if (!m.execute(g.packet[j], table, &steps)) return false;
            REQUIRE(steps == (j == step_at ? g.steps : 0));
        }
        if (c.split) flips++;
        if (g.steps > longest) longest = g.steps;
        prev_block = block;
        ended = last;
        groups++;
    }
    // (what the last group left unrung, the join rings: every chain's join packet follows its last group at once)
    REQUIRE(ended == (c.n_steps > 0) && m.next_step == c.n_steps && sched.longest() == longest);
    for (int k = 0; k < c.n_steps; ++k) REQUIRE(m.delivered[k] == 1);
    // the current state sits where the planner says
    const int o_end = sched.orientation();
    REQUIRE(o_end == (c.o0 + flips) % 2);
    const uint8_t *world = m.key.split ? m.B.world_buf[o_end] : m.base.world;
    const uint32_t *agents = m.key.split ? m.B.agents_buf[o_end] : m.base.agents;
    REQUIRE(m.tag[cell_of(world)] == 2 * c.n_steps && m.tag[cell_of(agents)] == 2 * c.n_steps);
    return true;
}

static long walk_grid() {
    const int resets[] = {0, 1, 2, 3, 4, 5, 6, 7, 9}, action_rings[] = {0, 1, 3, 5}, caps[] = {0, 2, 3, 4};
    long cases = 0;
    for (int n_steps = 0; n_steps <= 21; ++n_steps)
        for (int step0 = 0; step0 <= 6; ++step0)
            for (int reset_every : resets) {
                const int rings[] = {1, 2, 3, 5, 8, n_steps};
                for (int ring : rings) {
                    if (ring < 1) continue;                     // (no such ring)
                    for (int action_ring : action_rings)
                        for (int cap : caps)
                            for (int split = 0; split < 2; ++split)
                                for (int o0 = 0; o0 < 2; ++o0)
                                    for (int coherent = 0; coherent < 2; ++coherent) {
                                        if (!check_case(Case{n_steps, step0, reset_every, ring, action_ring, cap, split, o0, coherent})) return -1;
                                        cases++;
                                    }
                }
            }
    return cases;
}

// The blocks an argument set holds, per chain and slot.  From aql_set's rule: a set that is not split has kS and kR of orientation 0:
// 2.  A split set has, per orientation, kS kR kRn kA kAB kB = 6 and the run kinds (n, rd) with n and rd each 0 or a length the cap
// allows, not both below 2, and (0, 0) and (0, 1) = kB left out.  Cap 2 (lengths 1, 2): (1,2) (2,0) (2,1) (2,2) (0,2) = 5, so
// 2 * 11 = 22.  Caps 3 and 4 (lengths 1, 2 and the cap): n > 0: 3 * 4 = 12 less (1,0) (1,1) = 10, n = 0: (0,2) (0,cap) = 2, so
// 2 * (6 + 12) = 36.
static bool check_tables() {
    std::snprintf(g_case, sizeof g_case, "kind tables");
    const int caps[] = {0, 2, 3, 4}, want_split[] = {12, 22, 36, 36};
    for (int i = 0; i < 4; ++i) {
        REQUIRE(kind_table(0, caps[i]).n_dense == 2);
        const KindTable t = kind_table(1, caps[i]);
        REQUIRE(t.n_dense == want_split[i]);
        int seen = 0;
        for (int kind = 0; kind < kKinds; ++kind) if (t.dense[kind] >= 0) REQUIRE(t.dense[kind] == seen++);
        REQUIRE(seen == t.n_dense);
    }
    REQUIRE(kKinds == 62 && kKindsPerO == 31);
    REQUIRE(start_orientation(0, true) == 0 && start_orientation(1, true) == 1 && start_orientation(1, false) == 0 && start_orientation(0, false) == 0);
    return true;
}

// Two schedules by hand.
struct Want { size_t block; int kind; };
static bool same_plan(Schedule &sched, const Want *want, const int *group_sizes, int n_groups) {
    Group g;
    int at = 0;
    for (int i = 0; i < n_groups; ++i) {
        REQUIRE(sched.next(g) && g.n_packets == group_sizes[i]);
        for (int j = 0; j < g.n_packets; ++j, ++at) REQUIRE(g.packet[j].block == want[at].block && g.packet[j].kind == want[at].kind);
    }
    REQUIRE(!sched.next(g));
    return true;
}
static bool check_by_hand() {
    const int KO = kKindsPerO;
    {   // 11 steps, cap 4, no reset, from orientation 0, ring 11: runs of 4, 4, 2 and 1, then the renderers of the last alone
        std::snprintf(g_case, sizeof g_case, "by hand: 11 steps");
        Schedule s(11, 0, 0, 11, 11, true, 4, true, false, 0, 0, 0);
        const Want want[] = {{0, run_kind(4, 0)}, {4, KO + run_kind(4, 4)}, {8, run_kind(2, 4)}, {10, KO + run_kind(1, 2)}, {10, kB}};
        const int sizes[] = {1, 1, 1, 2};
        if (!same_plan(s, want, sizes, 4)) return false;
        REQUIRE(s.orientation() == 0 && s.longest() == 4);
    }
    {   // reset_every 6, step0 1, 20 steps, cap 4, ring 20: steps 0 .. 3 and 4 (indices 1 .. 5), a reset at index 6 = step 5, then
        // 4 + 2 to the next reset at step 11, again at step 17, and the last three steps as 2 + 1
        std::snprintf(g_case, sizeof g_case, "by hand: 20 steps, reset_every 6");
        Schedule s(20, 1, 6, 20, 20, true, 4, true, false, 0, 0, 0);
        const Want want[] = {
            {1, run_kind(4, 0)}, {5, KO + run_kind(1, 4)},                                              // steps 0 .. 3, 4
            {5, kB}, {6, kRn}, {6, run_kind(4, 0)}, {10, KO + run_kind(2, 4)},                          // renderers for step 4, reset, 5 .. 8, 9 .. 10
            {10, run_kind(0, 2)}, {12, kRn}, {12, run_kind(4, 0)}, {16, KO + run_kind(2, 4)},           // renderers for two, reset, 11 .. 14, 15 .. 16
            {16, run_kind(0, 2)}, {18, kRn}, {18, run_kind(2, 0)}, {0, KO + run_kind(1, 2)}, {0, kB}};  // ..., reset, 17 .. 18, 19, its renderers
        const int sizes[] = {1, 1, 3, 1, 3, 1, 3, 2};
        if (!same_plan(s, want, sizes, 8)) return false;
        REQUIRE(s.orientation() == 0 && s.longest() == 4);
    }
    return true;
}

// The form of a call at its thresholds, and the argument blocks per chain.
static bool check_form() {
    std::snprintf(g_case, sizeof g_case, "form");
    // Harvest's shipped map with five agents: a map-specific kernel (fast_profile 1) with runs of four (pair_profile 4)
    const FormIn std_in = {2048, 2, false, false, true, 20, 1, 4, 1, 1, 0, 1, kMaxRun};
    auto form = [&](auto change) { FormIn in = std_in; change(in); return choose_form(in); };
    auto is = [](const Form &f, int coherent, int key_split, bool split, int pairs, int run_cap) {
        return f.coherent == coherent && f.key_split == key_split && f.split == split && f.pairs == pairs && f.run_cap == run_cap;
    };
    REQUIRE(is(choose_form(std_in), 1, 1, true, 4, 4));
    // envs per launch: coherent up to 4096, split up to 2304 with several chains and 3072 with one
    REQUIRE(is(form([](FormIn &in) { in.per_launch = 4096; }), 1, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.per_launch = 4097; }), 0, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.per_launch = 2304; }), 1, 1, true, 4, 4));
    REQUIRE(is(form([](FormIn &in) { in.per_launch = 2305; }), 1, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.per_launch = 2305; in.chains = 3; }), 1, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.per_launch = 3072; in.chains = 1; }), 1, 1, true, 4, 4));
    REQUIRE(is(form([](FormIn &in) { in.per_launch = 3073; in.chains = 1; }), 1, 0, false, 0, 0));
    // short calls: the set is a split one, the call is not
    REQUIRE(is(form([](FormIn &in) { in.n_steps = 4; }), 1, 1, true, 4, 4));
    REQUIRE(is(form([](FormIn &in) { in.n_steps = 3; }), 1, 1, false, 4, 0));
    REQUIRE(is(form([](FormIn &in) { in.n_steps = 0; }), 1, 1, false, 4, 0));
    // what takes the general kernels: float32 observations, an explicit order, no map-specific kernel; no observations: nothing to split
    REQUIRE(is(form([](FormIn &in) { in.f32 = true; }), 0, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.order = true; }), 0, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.fast_profile = 0; in.pair_profile = 1; }), 0, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.obs = false; }), 1, 0, false, 0, 0));
    // the step-pair kernel the form is built with: none, pairs
    REQUIRE(is(form([](FormIn &in) { in.pair_profile = 1; }), 1, 1, true, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.pair_profile = 2; }), 1, 1, true, 2, 2));
    // every knob
    REQUIRE(is(form([](FormIn &in) { in.aql_coherent = 0; }), 0, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_split = 0; }), 1, 0, false, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_alternate = 1; }), 2, 1, true, 4, 4));
    REQUIRE(is(form([](FormIn &in) { in.aql_pairs = 0; }), 1, 1, true, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 1; }), 1, 1, true, 0, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 2; }), 1, 1, true, 2, 2));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 3; }), 1, 1, true, 3, 3));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 0; }), 1, 1, true, 4, 4));           // (below 1: no cap)
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 9; }), 1, 1, true, 4, 4));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 3; in.n_steps = 3; }), 1, 1, false, 3, 0));
    // argument blocks per chain: lcm(ring, action ring), refused past 2048 over all chains
    REQUIRE(block_slots(1, 0, 2) == 1 && block_slots(20, 0, 2) == 20 && block_slots(20, 20, 2) == 20);
    REQUIRE(block_slots(4, 6, 1) == 12 && block_slots(5, 3, 8) == 15 && block_slots(8, 1, 1) == 8);
    REQUIRE(block_slots(1024, 0, 2) == 1024 && block_slots(1025, 0, 2) == 0);
    REQUIRE(block_slots(2048, 0, 1) == 2048 && block_slots(2049, 0, 1) == 0 && block_slots(64, 33, 1) == 0 && block_slots(64, 32, 1) == 64);
    REQUIRE(block_slots(256, 0, 8) == 256 && block_slots(257, 0, 8) == 0);
    REQUIRE(block_slots(65536, 65521, 1) == 0);                                        // (no overflow on the way)
    // the observation ring past the memory-side cache: 232 MiB
    REQUIRE(!ring_past_cache(kObs, 1, (size_t)232 << 20) && ring_past_cache(kObs, 1, ((size_t)232 << 20) + 1) && !ring_past_cache(nullptr, 64, (size_t)232 << 20));
    REQUIRE(!ring_past_cache(kObs, 16, 13824000) && ring_past_cache(kObs, 32, 13824000));
    return true;
}

}  // namespace

int main() {
    if (!check_tables()) return 1;
    std::printf("kind tables: ok\n");
    if (!check_by_hand()) return 1;
    std::printf("schedules by hand: ok\n");
    if (!check_form()) return 1;
    std::printf("form and slots: ok\n");
    const long cases = walk_grid();
    if (cases < 0) return 1;
    std::printf("grid: %ld cases ok\n", cases);
    std::printf("ok\n");
    return 0;
}
