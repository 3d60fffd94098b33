// tests/native/rollout_plan_long_driver.cpp -- walks csrc/ssd_rollout_plan.hpp over LONG calls (choose_form's long cap: runs of
// kLongRun = 8 steps per launch beside the runs of four, two and one; the long kinds and their LongParams blocks) and checks every
// plan by a symbolic run of its packets, as tests/native/rollout_plan_driver.cpp does for the calls that are not long.  Compiled
// with g++ by tests/test_rollout_plan_long_cpu.py; prints one line per group of checks, "ok" last.
#include <cstdio>
#include <cstring>

struct uint4 { unsigned x, y, z, w; };      // (ssd_internal.hpp names HIP's vector type in pointers only)
#include "ssd_rollout_plan.hpp"

using namespace ssd;
using namespace ssd::plan;

static_assert(sizeof(LongKernArgs) == sizeof(KernArgs) + 8 * sizeof(PassRec) + 8 + 7 * sizeof(MidIn) + 7 * sizeof(void *), "a long block: 8 pass records, 7 mid inputs");
static_assert(kLongRun == 8 && kMaxRun == 4 && kLongKinds == 18 && kAllKinds == kKinds + 18, "the long family sits behind the kinds of old");

#define REQUIRE(cond)                                                                                                  \
    do {                                                                                                               \
        if (!(cond)) { std::printf("FAILED line %d: %s\n   in %s\n", __LINE__, #cond, g_case); return false; }         \
    } while (0)
static char g_case[256] = "(no case)";

// Fake device memory: every buffer is one 64-byte cell of an arena, so a pointer names its buffer and nothing is ever dereferenced.
static uint8_t g_arena[1 << 16];
constexpr int kCell = 64, kStateCells = 96;          // (the state, list and snapshot buffers are the arena's first cells)
static int cell_of(const void *ptr) { return (int)((static_cast<const uint8_t *>(ptr) - g_arena) / kCell); }
// the output and action rings: slot s lies s * en = 16 elements (observations: s * ob = 64 bytes) behind the ring's base
static uint8_t *const kObs = g_arena + 100 * kCell, *const kDone = g_arena + 400 * kCell;
static int32_t *const kRew = reinterpret_cast<int32_t *>(g_arena + 200 * kCell);
static const int32_t *const kActions = reinterpret_cast<const int32_t *>(g_arena + 500 * kCell);
constexpr int kMaxSteps = 96;

namespace {

struct Case { int n_steps, step0, reset_every, ring, action_ring, o0, long_cap; };

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
    int delivered[kMaxSteps] = {};           // observations written, per step
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
            // (a handle that has made no long call has none of these: a plan that is not long must not name one)
            for (int k = 0; c.long_cap && k < kLongMids - kMids; ++k) {
                B.long_world[k][o] = cell(); B.long_snap[k][o] = cell();
                B.long_agents[k][o] = reinterpret_cast<uint32_t *>(cell()); B.long_list[k][o] = reinterpret_cast<uint32_t *>(cell());
            }
        }
        key.split = 1; key.pairs = kMaxRun; key.long_cap = c.long_cap;
        key.ring = c.ring; key.action_ring = c.action_ring; key.coherent = 1;
        slots = block_slots(c.ring, c.action_ring, 1);
        key.slots = slots;
        base.E = 48; base.e_begin = 16;
        base.world = B.world_buf[c.o0]; base.agents = B.agents_buf[c.o0];         // the handle's current state
        tag[cell_of(base.world)] = tag[cell_of(base.agents)] = 0;
        rings = ChainRings{kObs, kRew, kDone, c.action_ring ? kActions : nullptr, nullptr, c.action_ring, 16, 64, 8};
    }

    // the env waves' step k: from `in` (pass 0 of a launch alone reads memory) into the record's buffers
    bool env_step(int k, const uint8_t *in_world, const uint32_t *in_agents, const PassRec &out) {
        REQUIRE(k == next_step && k < c.n_steps);                              // every step once, in order
        if (in_world) REQUIRE(tag[cell_of(in_world)] == 2 * k + reset_due(k) && tag[cell_of(in_agents)] == 2 * k + reset_due(k));
        REQUIRE(out.world && out.agents && out.beam_list && out.snap && cell_of(out.world) < kStateCells);
        tag[cell_of(out.world)] = tag[cell_of(out.agents)] = 2 * (k + 1);
        tag[cell_of(out.beam_list)] = tag[cell_of(out.snap)] = k;
        REQUIRE(out.rew == kRew + out_slot(k) * 16 && out.done == kDone + out_slot(k) * 16);
        if (c.action_ring) REQUIRE(out.actions == kActions + ((c.step0 + k) % c.action_ring) * 16);
        else REQUIRE(!out.actions);
        next_step++;
        return true;
    }
    // a renderer wave delivers step k: from the state the step left, its marks and its snapshot, into the step's ring slot
    bool render(int k, const uint8_t *world, const uint32_t *agents, const uint32_t *list, const uint8_t *snap, const uint8_t *obs) {
        REQUIRE(k >= 0 && k < next_step);                                      // never before the step was computed
        REQUIRE(world && agents && list && snap);
        REQUIRE(tag[cell_of(world)] == 2 * (k + 1) && tag[cell_of(agents)] == 2 * (k + 1));
        REQUIRE(tag[cell_of(list)] == k && tag[cell_of(snap)] == k);
        REQUIRE(obs == kObs + out_slot(k) * 64);
        REQUIRE(delivered[k] == 0);
        for (int j = 0; j < k; ++j) REQUIRE(delivered[j] == 1);               // strictly in step order
        delivered[k] = 1;
        return true;
    }
    // A launch of env waves and renderers by the step kernels' contract (ssd_internal.hpp, PairParams / LongParams; kMax: the slots
    // of the block's arrays): the renderers deliver the rd steps of the launch before, the env waves take n.
    bool run_launch(const Params &p, int o, int n, int rd, int kMax, const PassRec *pass, const MidIn *mid_in, uint8_t *const *obs_b0) {
        const int k = next_step;
        REQUIRE(p.world == B.world_buf[o] && p.agents == B.agents_buf[o]);
        REQUIRE(p.world_out == B.world_buf[1 - o] && p.agents_out == B.agents_buf[1 - o] && p.beam_list == B.beam_list[o] && p.snap == B.snap_grid[o]);
        REQUIRE(p.snap_mode == ((n == 0 ? 4 : 1) | (rd > 0 ? 2 : 0)) && !p.obs);
        // no launch writes what it or its renderers read
        const void *reads[4 + 4 * kLongMids], *writes[4 * kLongRun];
        int n_reads = 0, n_writes = 0;
        if (n > 0 || rd > 0) { reads[n_reads++] = p.world; reads[n_reads++] = p.agents; }
        if (rd > 0) {
            reads[n_reads++] = p.beam_list_in; reads[n_reads++] = p.snap_in;
            for (int j = 0; j + 1 < rd; ++j) {
                const int t = kMax - rd + j;
                const MidIn &m = mid_in[t];
                reads[n_reads++] = m.world; reads[n_reads++] = m.agents; reads[n_reads++] = m.beam_list; reads[n_reads++] = m.snap;
                if (!render(k - rd + j, m.world, m.agents, m.beam_list, m.snap, obs_b0[t])) return false;
            }
            if (!render(k - 1, p.world, p.agents, p.beam_list_in, p.snap_in, p.obs_b)) return false;
        }
        for (int j = 0; j < n; ++j) {
            const PassRec rec = pass ? pass[j] : PassRec{p.world_out, p.agents_out, p.beam_list, p.snap, p.rew, p.done, p.actions};
            const SplitBuffers::MidSet m = j + 1 < n ? B.mid_set(j, o) : SplitBuffers::MidSet{p.world_out, p.agents_out, p.beam_list, p.snap};
            REQUIRE(rec.world == m.world && rec.agents == m.agents && rec.beam_list == m.list && rec.snap == m.snap);
            if (j == 0) REQUIRE(rec.actions == p.actions && rec.rew == p.rew && rec.done == p.done);   // (the first pass's: Params' own, the same pointers)
            writes[n_writes++] = rec.world; writes[n_writes++] = rec.agents; writes[n_writes++] = rec.beam_list; writes[n_writes++] = rec.snap;
            if (!env_step(k + j, j == 0 ? p.world : nullptr, p.agents, rec)) return false;
        }
        if (n > 0) REQUIRE(p.num_actions_random == (c.action_ring ? 0 : 8));
        for (int a = 0; a < n_reads; ++a)
            for (int b = 0; b < n_writes; ++b) REQUIRE(reads[a] != writes[b]);
        for (int a = 0; a < n_writes; ++a)
            for (int b = 0; b < a; ++b) REQUIRE(writes[a] != writes[b]);
        return true;
    }
    // One packet.  steps: the steps its env waves take (0: none).
    bool execute(const Packet &pk, const KindTable &table, const LongKindTable &long_table, int *steps) {
        REQUIRE(pk.kind >= 0 && pk.kind < kAllKinds && pk.block < (size_t)slots);
        const int k = next_step;
        *steps = 0;
        if (is_long_kind(pk.kind)) {
            REQUIRE(key.long_cap == kLongRun && long_table.dense[pk.kind - kKinds] >= 0);   // the set has a long block for it
            Params p; LongParams q;
            fill_long_block(base, rings, key, B, pk.kind, (int)pk.block, p, q);
            const int o = long_kind_o(pk.kind), n = long_kind_n(pk.kind), rd = long_kind_rendered(pk.kind);
            REQUIRE(long_counts(n, rd) && (n == kLongRun || rd == kLongRun) && long_kind(o, n, rd) == pk.kind);
            REQUIRE(p.E == base.E && p.e_begin == base.e_begin && p.coherent == 1u && p.rotate == 1);
            REQUIRE(p.mode == kModeStepLong && q.n_pass == n && q.n_render == rd);
            if (!run_launch(p, o, n, rd, kLongRun, q.pass, q.mid_in, q.obs_b0)) return false;
            *steps = n;
            return true;
        }
        REQUIRE(table.dense[pk.kind] >= 0);                                    // the set has a block for it
        Params p; PairParams q;
        fill_block(base, rings, key, B, pk.kind, (int)pk.block, p, q);
        const int o = pk.kind / kKindsPerO, kb = pk.kind % kKindsPerO;
        REQUIRE(p.E == base.E && p.e_begin == base.e_begin && p.coherent == 1u);
        REQUIRE(kb != kS && kb != kR);                                         // (a split call)
        if (kb == kRn) {
            // a reset: of the state step k starts from, in place, once everything before it has been rendered from that buffer
            REQUIRE(!p.world_out && !p.agents_out && p.snap_mode == 0 && p.world == B.world_buf[o] && p.agents == B.agents_buf[o]);
            REQUIRE(p.mode == kModeReset && p.rotate == 0 && !p.actions && !p.order && !p.rew && !p.done && !p.obs);
            REQUIRE(k < c.n_steps && reset_due(k));
            REQUIRE(tag[cell_of(p.world)] == 2 * k && tag[cell_of(p.agents)] == 2 * k);
            for (int j = 0; j < k; ++j) REQUIRE(delivered[j] == 1);
            tag[cell_of(p.world)] = tag[cell_of(p.agents)] = 2 * k + 1;
            return true;
        }
        int n, rd;
        if (kb >= kRun) {
            n = (kb - kRun) / (kMaxRun + 1); rd = (kb - kRun) % (kMaxRun + 1);
            REQUIRE(p.mode == kModeStepPair && q.n_pass == n && q.n_render == rd && run_kind_used(kb, key.pairs));
            if (!run_launch(p, o, n, rd, kMaxRun, q.pass, q.mid_in, q.obs_b0)) return false;
        } else {
            n = kb == kB ? 0 : 1; rd = kb == kA ? 0 : 1;
            REQUIRE(p.mode == kModeStep);
            if (!run_launch(p, o, n, rd, kMaxRun, nullptr, q.mid_in, q.obs_b0)) return false;
        }
        *steps = n;
        return true;
    }
};

static bool is_reset(int kind) { return !is_long_kind(kind) && kind % kKindsPerO == kRn; }
static bool is_render_only(int kind) {
    if (is_long_kind(kind)) return long_kind_n(kind) == 0;
    const int kb = kind % kKindsPerO;
    return kb == kB || (kb >= kRun && (kb - kRun) / (kMaxRun + 1) == 0);
}
static bool same_group(const Group &a, const Group &b) {
    if (a.n_packets != b.n_packets || a.step != b.step || a.steps != b.steps || a.reset != b.reset || a.ring != b.ring) return false;
    for (int j = 0; j < a.n_packets; ++j)
        if (a.packet[j].block != b.packet[j].block || a.packet[j].kind != b.packet[j].kind || a.packet[j].acquire != b.packet[j].acquire ||
            a.packet[j].release != b.packet[j].release) return false;
    return true;
}

// One call of the grid: plan it, check every group's shape, fences and doorbell, run its packets.
static bool check_case(const Case &c) {
    std::snprintf(g_case, sizeof g_case, "n_steps %d step0 %d reset_every %d ring %d action_ring %d o %d long_cap %d",
                  c.n_steps, c.step0, c.reset_every, c.ring, c.action_ring, c.o0, c.long_cap);
    Machine m(c);
    REQUIRE(m.slots > 0 && m.slots % c.ring == 0 && (c.action_ring == 0 || m.slots % c.action_ring == 0));
    const KindTable table = kind_table(1, kMaxRun);
    const LongKindTable long_table = long_kind_table(c.long_cap);
    REQUIRE(long_table.n_dense == (c.long_cap ? kLongKinds : 0));
    const bool obs_wb = (c.n_steps + c.step0 + c.ring) % 3 == 0;      // (a property of the caller's ring: any case may have it)
    Schedule sched(c.n_steps, c.step0, c.reset_every, c.ring, m.slots, true, kMaxRun, true, obs_wb, 0, 0, c.o0, c.long_cap);
    Schedule today(c.n_steps, c.step0, c.reset_every, c.ring, m.slots, true, kMaxRun, true, obs_wb, 0, 0, c.o0);   // (the constructor without a long cap)
    Group g;
    int groups = 0, longest = 0, flips = 0;
    bool first_packet = true, ended = false;
    size_t prev_block = 0;
    while (sched.next(g)) {
        REQUIRE(!ended && g.n_packets >= 1 && g.n_packets <= 4);
        if (!c.long_cap) { Group t; REQUIRE(today.next(t) && same_group(g, t)); }
        // the run: eight wherever eight steps remain before the call's end and before the next reset, else four, else two, else one
        int avail = c.n_steps - g.step;
        if (c.reset_every > 0) { const int to_reset = c.reset_every - (c.step0 + g.step) % c.reset_every; if (to_reset < avail) avail = to_reset; }
        const int want = (c.long_cap && avail >= 8) ? 8 : avail >= 4 ? 4 : avail >= 2 ? 2 : 1;
        REQUIRE(g.step == m.next_step && g.steps == want && g.step + g.steps <= c.n_steps);
        REQUIRE(g.reset == m.reset_due(g.step));
        for (int j = 1; j < g.steps; ++j) REQUIRE(!m.reset_due(g.step + j));               // a run never spans a reset
        const size_t block = (size_t)((c.step0 + g.step) % m.slots);
        // the group's shape: [renderers of the run before] [reset] step [renderers of this run, at the call's end]
        int at = 0;
        if (g.reset && g.step > 0) { REQUIRE(is_render_only(g.packet[at].kind) && g.packet[at].block == prev_block); at++; }
        if (g.reset) { REQUIRE(is_reset(g.packet[at].kind) && g.packet[at].block == block); at++; }
        const int step_at = at;
        REQUIRE(!is_reset(g.packet[at].kind) && !is_render_only(g.packet[at].kind) && g.packet[at].block == block);
        at++;
        const bool last = g.step + g.steps == c.n_steps;
        if (last) { REQUIRE(is_render_only(g.packet[at].kind) && g.packet[at].block == block); at++; }
        REQUIRE(at == g.n_packets);
        // fences: the chain's first packet of the call acquires at agent scope; a ring written with write-back stores is released
        // once per round, by the launch that takes the round's first step.  A doorbell after every launch.
        bool round = false;
        for (int j = 0; j < g.steps; ++j) round = round || (c.step0 + g.step + j) % c.ring == 0;
        for (int j = 0; j < g.n_packets; ++j) {
            REQUIRE(g.packet[j].acquire == (first_packet ? 1 : 0));
            REQUIRE(g.packet[j].release == ((j == step_at && obs_wb && round) ? 1 : 0));
            first_packet = false;
        }
        REQUIRE(g.ring);
        for (int j = 0; j < g.n_packets; ++j) {
            int steps = 0;
            if (!m.execute(g.packet[j], table, long_table, &steps)) return false;
            REQUIRE(steps == (j == step_at ? g.steps : 0));
        }
        flips++;
        if (g.steps > longest) longest = g.steps;
        prev_block = block;
        ended = last;
        groups++;
    }
    if (!c.long_cap) { Group t; REQUIRE(!today.next(t) && today.orientation() == sched.orientation() && today.longest() == sched.longest()); }
    REQUIRE(ended && m.next_step == c.n_steps && sched.longest() == longest);
    for (int k = 0; k < c.n_steps; ++k) REQUIRE(m.delivered[k] == 1);
    // the current state sits where the planner says
    const int o_end = sched.orientation();
    REQUIRE(o_end == (c.o0 + flips) % 2);
    REQUIRE(m.tag[cell_of(m.B.world_buf[o_end])] == 2 * c.n_steps && m.tag[cell_of(m.B.agents_buf[o_end])] == 2 * c.n_steps);
    return true;
}

static long walk_grid() {
    const int resets[] = {0, 7, 8, 9, 13, 64}, action_rings[] = {0, 5}, long_caps[] = {0, kLongRun};
    long cases = 0;
    for (int n_steps = 56; n_steps <= 90; ++n_steps)
        for (int step0 = 0; step0 <= 9; ++step0)
            for (int reset_every : resets) {
                const int rings[] = {1, 3, 8, 9, n_steps};
                for (int ring : rings)
                    for (int action_ring : action_rings)
                        for (int o0 = 0; o0 < 2; ++o0)
                            for (int long_cap : long_caps) {
                                if (!check_case(Case{n_steps, step0, reset_every, ring, action_ring, o0, long_cap})) return -1;
                                cases++;
                            }
            }
    return cases;
}

// One schedule by hand: 75 steps, long, no reset, from orientation 0, one ring slot per step: nine runs of eight, a pair and a single
// step, then the renderers of the last alone.
struct Want { size_t block; int kind; };
static bool check_by_hand() {
    std::snprintf(g_case, sizeof g_case, "by hand: 75 steps");
    const int KO = kKindsPerO;
    Schedule s(75, 0, 0, 75, 75, true, kMaxRun, true, false, 0, 0, 0, kLongRun);
    const Want want[] = {{0, long_kind(0, 8, 0)},  {8, long_kind(1, 8, 8)},  {16, long_kind(0, 8, 8)}, {24, long_kind(1, 8, 8)}, {32, long_kind(0, 8, 8)},
                         {40, long_kind(1, 8, 8)}, {48, long_kind(0, 8, 8)}, {56, long_kind(1, 8, 8)}, {64, long_kind(0, 8, 8)},
                         {72, long_kind(1, 2, 8)}, {74, run_kind(1, 2)}, {74, KO + kB}};
    const int sizes[] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2};
    Group g;
    int at = 0;
    for (int i = 0; i < 11; ++i) {
        REQUIRE(s.next(g) && g.n_packets == sizes[i] && g.steps == (i < 9 ? 8 : i == 9 ? 2 : 1));
        for (int j = 0; j < g.n_packets; ++j, ++at) REQUIRE(g.packet[j].block == want[at].block && g.packet[j].kind == want[at].kind);
    }
    REQUIRE(!s.next(g) && s.orientation() == 1 && s.longest() == 8);
    // the long kinds' numbers: behind kKinds, nine per orientation, and back
    REQUIRE(long_kind(0, 8, 0) == kKinds && long_kind(0, 8, 8) == kKinds + 4 && long_kind(0, 0, 8) == kKinds + 5 && long_kind(1, 4, 8) == kAllKinds - 1);
    for (int kind = kKinds; kind < kAllKinds; ++kind) REQUIRE(long_kind(long_kind_o(kind), long_kind_n(kind), long_kind_rendered(kind)) == kind);
    REQUIRE(!long_counts(8, 3) && !long_counts(4, 4) && long_counts(8, 4) && long_counts(0, 8));
    return true;
}

// The form of a call around the threshold, kLongCallSteps.
static bool check_form() {
    std::snprintf(g_case, sizeof g_case, "form");
    // Harvest's shipped map with five agents: runs of four (pair_profile 4) and a long kernel (long_profile 8); no knob set
    FormIn std_in = {2048, 2, false, false, true, kLongCallSteps, 1, 4, 1, 1, 0, 1, kLongRun, kLongRun};
    auto form = [&](auto change) { FormIn in = std_in; change(in); return choose_form(in); };
    auto is = [](const Form &f, bool split, int pairs, int run_cap, int long_cap) {
        return f.coherent == 1 && f.key_split == 1 && f.split == split && f.pairs == pairs && f.run_cap == run_cap && f.long_cap == long_cap;
    };
    // (the threshold began at 64 and was moved by the measurements its comment names: one step below it and at it, and at 63 and 64)
    REQUIRE(kLongCallSteps == 256 && kLongCallSteps > 45);
    REQUIRE(is(choose_form(std_in), true, 4, 4, 8));
    REQUIRE(is(form([](FormIn &in) { in.n_steps = kLongCallSteps - 1; }), true, 4, 4, 0));
    REQUIRE(is(form([](FormIn &in) { in.n_steps = 63; }), true, 4, 4, 0) && is(form([](FormIn &in) { in.n_steps = 64; }), true, 4, 4, 0));
    // (the argument set is long wherever the form can be, whatever the call's length; not under a knob or a kernel that keeps fours)
    REQUIRE(choose_form(std_in).key_long == 8 && form([](FormIn &in) { in.n_steps = 3; }).key_long == 8);
    REQUIRE(form([](FormIn &in) { in.aql_run = 4; }).key_long == 0 && form([](FormIn &in) { in.long_profile = 0; }).key_long == 0);
    REQUIRE(form([](FormIn &in) { in.pair_profile = 2; }).key_long == 0 && form([](FormIn &in) { in.per_launch = 2305; }).key_long == 0);
    REQUIRE(is(form([](FormIn &in) { in.n_steps = 3000; }), true, 4, 4, 8));
    REQUIRE(is(form([](FormIn &in) { in.n_steps = 20; }), true, 4, 4, 0));
    // a form without a long kernel, a kernel held to pairs, single steps by the knob
    REQUIRE(is(form([](FormIn &in) { in.long_profile = 0; }), true, 4, 4, 0));
    REQUIRE(is(form([](FormIn &in) { in.pair_profile = 2; }), true, 2, 2, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_pairs = 0; }), true, 0, 0, 0));
    // SSD_AQL_RUN: 4 gives a long call today's plan, 8 and "no cap" leave it long
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 4; }), true, 4, 4, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 7; }), true, 4, 4, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 3; }), true, 3, 3, 0));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 0; }), true, 4, 4, 8));
    REQUIRE(is(form([](FormIn &in) { in.aql_run = 9; }), true, 4, 4, 8));
    // a call that is not split is not long
    Form f = form([](FormIn &in) { in.per_launch = 2305; });
    REQUIRE(f.key_split == 0 && !f.split && f.long_cap == 0);
    // the Schedule takes a long cap only beside runs of four
    Schedule s(64, 0, 0, 64, 64, true, 2, true, false, 0, 0, 0, kLongRun);
    Group g;
    REQUIRE(s.next(g) && g.steps == 2);
    return true;
}

}  // namespace

int main() {
    if (!check_by_hand()) return 1;
    std::printf("schedule by hand: ok\n");
    if (!check_form()) return 1;
    std::printf("form: ok\n");
    const long cases = walk_grid();
    if (cases < 0) return 1;
    std::printf("grid: %ld cases ok\n", cases);
    std::printf("ok\n");
    return 0;
}
