"""Spawn-table scenarios: what tests/test_spawn_tables_cpu.py and tests/test_spawn_tables_gpu.py share.

The step kernel's spawn phase (harvest.py:69-104 spawn_apples; cleanup.py:113-171 compute_probabilities +
spawn_apples_and_waste) reads its probabilities from tables of ssd_config.  At the reference's constants the phase is nearly
idle; a table chosen by the test makes every step decide something.  A case here is a table, start worlds, actions and
-- because a busy scenario must not hide that it was idle -- the coverage it claims (`guards`), computed from the oracle's own
states (`trajectory`) and asserted by both test files, so that an edit of a recipe is caught without a GPU.

Everything is a pure function of the case: the oracle's trajectory is computed once per case and shared (read only).
"""
import functools

import numpy as np

import golden_util as G
from oracle import pyoracle
from sequential_social_dilemma_games_amd import config as cfgmod
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd import prng

T32 = 1 << 32


def u64(*v):
    return np.array(v, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------- tables
H_COUNT = u64(1 << 26, T32, 0, T32)                  # p = (1/64, 1, 0, 1): the exact neighbour count decides, no draw
H_ALWAYS = u64(T32, T32, T32, T32)
H_ALWAYS_WIDE = u64(1 << 40, 1 << 40, 1 << 40, 1 << 40)
H_NEVER = u64(0, 0, 0, 0)
H_DENSE = np.array([prng.threshold(p) for p in (0.25, 0.5, 0.75, 1.0)], dtype=np.uint64)   # the draw decides, often


def potential(amap):
    return cfgmod.potential_waste_area(amap)


def c_parity(amap):
    """apple[n] = 2^32 for even n, else 0; waste[n] = 2^32 for n % 3 != 0, else 0: a count off by one flips the whole orchard."""
    n = np.arange(potential(amap) + 1)
    return (np.where(n % 2 == 0, T32, 0).astype(np.uint64), np.where(n % 3 != 0, T32, 0).astype(np.uint64))


def c_waste_always(amap):
    n = potential(amap) + 1
    return np.zeros(n, np.uint64), np.full(n, T32, np.uint64)


def c_apples_always(amap):
    n = potential(amap) + 1
    return np.full(n, T32, np.uint64), np.zeros(n, np.uint64)


def c_wide(amap):
    """Entries at and above 2^32, up to 2^63 (the 64-bit compare), beside draw-decided and zero ones."""
    n = np.arange(potential(amap) + 1)
    apple = np.choose(n % 4, [1 << 63, T32 + 5, 1 << 31, 0]).astype(np.uint64)
    waste = np.choose(n % 3, [1 << 63, 1 << 33, 1 << 31]).astype(np.uint64)
    return apple, waste


def default_tables(amap):
    """The reference's constants as explicit tables (what VecEngine derives when it is given none)."""
    return cfgmod.harvest_thresholds(), cfgmod.cleanup_thresholds(potential(amap))


# ---------------------------------------------------------------------------------------------------- start states
EMPTIED = (0, 63, 64, 65, 80, 100, 130, 155)         # apple points emptied, by env: both sides of the 64-candidate compaction edge


def cells(amap, chars):
    return np.array([(r, c) for r in range(len(amap)) for c in range(len(amap[0])) if amap[r][c] in chars])


def start_emptied(case, st, rng):
    """Harvest: env e starts with EMPTIED[e % 8] of its apple points empty."""
    ap = cells(case.amap, "A")
    assert len(ap) >= max(EMPTIED)
    world = st["world"].copy()
    for e in range(case.E):
        for r, c in ap[rng.permutation(len(ap))[:EMPTIED[e % len(EMPTIED)]]]:
            world[e, r, c] = ord(" ")
    return dict(world=world)


def start_in_orchard(case, st, rng):
    """Harvest: the agents stand on distinct apple points, facing anywhere; the world is the reset's (every apple there)."""
    ap = cells(case.amap, "A")
    pos, orient = st["pos"].copy(), st["orient"].copy()
    for e in range(case.E):
        pos[e] = ap[rng.permutation(len(ap))[:case.N]]
        orient[e] = rng.randint(0, 4, size=case.N)
    return dict(pos=pos, orient=orient)


def _crowd(case, st, rng, anchors):
    """The agents on the N cells nearest to a random anchor cell, in random order, facing anywhere (two thirds of the envs;
    the recipe of test_cleanup_steps_with_many_shooters, anchored where the case says)."""
    fr = cells(case.amap, " PHRSB")
    pos, orient = st["pos"].copy(), st["orient"].copy()
    for e in range(case.E):
        if e % 3 == 2:
            continue
        anchor = anchors[rng.randint(len(anchors))]
        near = np.argsort(np.abs(fr - anchor).sum(1) + 0.01 * rng.rand(len(fr)))[:case.N]
        pos[e] = fr[near[rng.permutation(case.N)]]
        orient[e] = rng.randint(0, 4, size=case.N)
    return pos, orient


def start_river_crowd(case, st, rng):
    """Cleanup: crowded starts on and beside the river, the orchard picked empty (the reset's spawn pass may have filled it:
    the first step that reads an "always" entry then grows every apple at once)."""
    pos, orient = _crowd(case, st, rng, cells(case.amap, "HR"))
    world = st["world"].copy()
    world[world == ord("A")] = ord(" ")
    return dict(world=world, pos=pos, orient=orient)


def _waste_world(case, st, rng, count_of_env):
    wp = cells(case.amap, "HR")
    world = st["world"].copy()
    world[world == ord("A")] = ord(" ")              # (the orchard picked empty, as in start_river_crowd)
    for e in range(case.E):
        n = count_of_env(e, len(wp))
        world[e, wp[:, 0], wp[:, 1]] = ord("R")
        pick = wp[rng.permutation(len(wp))[:min(n, len(wp))]]
        world[e, pick[:, 0], pick[:, 1]] = ord("H")
        if n > len(wp):                              # more 'H' than waste points: on stream cells (the count then lies past the tables' end)
            sp = cells(case.amap, "S")
            extra = sp[rng.permutation(len(sp))[:n - len(wp)]]
            world[e, extra[:, 0], extra[:, 1]] = ord("H")
    return world


def start_river_crowd_counts(case, st, rng):
    """Cleanup: env e holds e mod (potential + 1) cells of 'H' -- every table entry is some env's first -- from crowded starts."""
    pos, orient = _crowd(case, st, rng, cells(case.amap, "HR"))
    return dict(world=_waste_world(case, st, rng, lambda e, p: e % (p + 1)), pos=pos, orient=orient)


def start_full_empty_over(case, st, rng):
    """Cleanup: by env, every waste point 'H' (the tables' last entry); none (the first); every waste point and six stream
    cells (a count past the end: the clamp).  Crowded on the river."""
    pos, orient = _crowd(case, st, rng, cells(case.amap, "HR"))
    return dict(world=_waste_world(case, st, rng, lambda e, p: (p, 0, p + 6)[e % 3]), pos=pos, orient=orient)


# ---------------------------------------------------------------------------------------------------- actions
def act_random(case, rng):
    return rng.randint(0, 8 if case.game == K.GAME_HARVEST else 9, size=(case.steps, case.E, case.N)).astype(np.int32)


def act_movers(case, rng):
    """Mostly MOVE (0..3), some STAY / turns: agents walking through the orchard."""
    a = rng.randint(0, 4, size=(case.steps, case.E, case.N))
    other = rng.randint(0, 7, size=a.shape)
    return np.where(rng.rand(*a.shape) < 0.8, a, other).astype(np.int32)


def act_clean_heavy(case, rng):
    """Half of the actions CLEAN, a tenth FIRE, the rest anything: the waste count moves by 0..several per step, both ways."""
    a = rng.randint(0, 9, size=(case.steps, case.E, case.N))
    u = rng.rand(*a.shape)
    return np.where(u < 0.5, 8, np.where(u < 0.6, 7, a)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- cases
class Case(object):
    def __init__(self, name, game, amap, E, N, steps, start, actions, seed, harvest=None, cleanup=None, view_len=7, guards=(),
                 horizon=0, masked_reset=None, reset_every=0, step0=0, modes=("calls", "chains", "fused"), split=True):
        self.name, self.game, self.amap, self.E, self.N, self.steps = name, game, amap, E, N, steps
        self.start, self.actions, self.seed, self.view_len = start, actions, seed, view_len
        self.harvest, self.cleanup = harvest, cleanup      # the tables; None = the reference's constants
        self.guards = tuple(guards)                  # what the case claims to reach (check_guards)
        self.horizon = horizon                       # > 0: per-call steps with SSD_AUTO_RESET, envs out of phase (t = e % horizon)
        self.masked_reset = masked_reset             # step index before which every third env is reset (ssd_reset with a mask)
        # reset_every > 0: every env is reset before step k whenever (step0 + k) % reset_every == 0 -- inside the rollout calls
        # (the reset pass of the rollout kernels); step k reads action slot and writes output slot (step0 + k) % steps
        self.reset_every, self.step0 = reset_every, step0
        self.modes = modes
        self.split = split and view_len == 7         # the chains are expected to take the split coherent path (map-specific kernels)

    def slot(self, k):
        return (self.step0 + k) % self.steps

    def full_reset_before(self, k):
        return self.reset_every > 0 and (self.step0 + k) % self.reset_every == 0

    def tables_kw(self):
        return dict(harvest_thresholds=self.harvest, cleanup_thresholds=self.cleanup)


HG = ("over64", "upto64", "adjacent")                # the Harvest guards: both forms of the candidate pass, adjacent same-step apples
CG = ("counts20", "under_agent")                     # the Cleanup guards
H, C = K.GAME_HARVEST, K.GAME_CLEANUP
C25, C48 = K.CLEANUP_MAP, K.cleanup_map_48x36()

CASES = [
    # Harvest, count-decided: the map-specific kernels of 5 and 10 agents, and the general kernel
    Case("h_count_n5", H, K.HARVEST_MAP, 64, 5, 40, start_emptied, act_random, 501, harvest=H_COUNT, guards=HG),
    Case("h_count_n10", H, K.HARVEST_MAP, 64, 10, 30, start_emptied, act_random, 502, harvest=H_COUNT, guards=HG),
    Case("h_count_v6", H, K.HARVEST_MAP, 64, 5, 30, start_emptied, act_random, 503, harvest=H_COUNT, view_len=6, guards=HG),
    # always (2^32 and a wider entry) and never
    Case("h_always", H, K.HARVEST_MAP, 64, 5, 30, start_emptied, act_random, 504, harvest=H_ALWAYS, guards=("over64", "upto64", "refilled")),
    Case("h_always_wide", H, K.HARVEST_MAP, 64, 5, 30, start_emptied, act_random, 505, harvest=H_ALWAYS_WIDE, guards=("over64", "upto64", "refilled")),
    Case("h_never", H, K.HARVEST_MAP, 64, 5, 60, start_in_orchard, act_movers, 506, harvest=H_NEVER, guards=("no_new_apples", "eaten")),
    # draw-decided dense
    Case("h_dense", H, K.HARVEST_MAP, 64, 5, 40, start_emptied, act_random, 507, harvest=H_DENSE, guards=HG),
    # Cleanup, count parity: the shipped map with 5 and 10 agents, the enlarged map, the general kernel
    Case("c_parity_n5", C, C25, 64, 5, 40, start_river_crowd, act_clean_heavy, 511, cleanup=c_parity(C25), guards=CG + ("both_ways",)),
    Case("c_parity_n10", C, C25, 64, 10, 30, start_river_crowd, act_clean_heavy, 512, cleanup=c_parity(C25), guards=CG + ("both_ways",)),
    Case("c_parity_48x36", C, C48, 64, 10, 30, start_river_crowd, act_clean_heavy, 513, cleanup=c_parity(C48), guards=CG + ("both_ways",)),
    Case("c_parity_v6", C, C25, 64, 5, 30, start_river_crowd, act_clean_heavy, 514, cleanup=c_parity(C25), view_len=6, guards=CG + ("both_ways",)),
    Case("c_waste_always", C, C25, 120, 5, 30, start_river_crowd_counts, act_clean_heavy, 515, cleanup=c_waste_always(C25),
         guards=CG + ("no_new_apples", "all_free")),
    Case("c_apples_always", C, C25, 64, 5, 30, start_river_crowd, act_clean_heavy, 516, cleanup=c_apples_always(C25),
         guards=("refilled", "no_new_waste")),
    Case("c_wide", C, C25, 66, 5, 30, start_full_empty_over, act_clean_heavy, 517, cleanup=c_wide(C25),
         guards=CG + ("first_entry", "last_entry", "past_end")),
    # resets: the step after a reset must use the reset world's count
    Case("h_count_auto", H, K.HARVEST_MAP, 64, 5, 30, start_emptied, act_random, 521, harvest=H_COUNT, horizon=5, modes=("calls",),
         guards=("auto_resets",)),
    Case("c_parity_auto", C, C25, 64, 5, 30, start_river_crowd_counts, act_clean_heavy, 522, cleanup=c_parity(C25), horizon=5, modes=("calls",),
         guards=CG + ("auto_resets",)),
    Case("c_parity_masked", C, C25, 64, 5, 30, start_river_crowd, act_clean_heavy, 523, cleanup=c_parity(C25), masked_reset=13,
         guards=CG),
    Case("h_count_every", H, K.HARVEST_MAP, 64, 5, 30, start_emptied, act_random, 524, harvest=H_COUNT, reset_every=7, step0=3,
         guards=("upto64", "adjacent")),
    Case("c_parity_every", C, C25, 64, 5, 30, start_river_crowd_counts, act_clean_heavy, 525, cleanup=c_parity(C25), reset_every=7, step0=3,
         guards=CG),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------- the oracle's run
class Traj(object):
    pass


def make_oracle(case):
    ora = pyoracle.Oracle(case.game, case.amap, case.E, case.N, G.default_lut(), view_len=case.view_len, seed=case.seed)
    ora.set_tables(harvest=case.harvest, cleanup=case.cleanup)
    return ora


def reset_mask(case):
    return (np.arange(case.E) % 3 == 1).astype(np.uint8)


@functools.lru_cache(maxsize=2)
def trajectory(name):
    """The oracle's run of case `name`: start state, the action ring (step k reads slot case.slot(k)), every step's expected outputs (obs, rew, done, waste count used),
    the final state, and per env-step what the guards count.  Computed once, shared, never written to."""
    case = BY_NAME[name]
    rng = np.random.RandomState(case.seed)
    ora = make_oracle(case)
    ora.reset()
    st = ora.get_state()
    tr = Traj()
    tr.start = case.start(case, st, rng)
    if case.horizon:
        tr.start["t"] = (np.arange(case.E) % case.horizon).astype(np.uint32)
    ora.set_state(**tr.start)
    tr.actions = case.actions(case, rng)
    ap = cells(case.amap, "A" if case.game == H else "B")
    E, N = case.E, case.N
    tr.obs, tr.rew, tr.done, tr.waste = [], [], [], []
    stats = dict(empties=[], adjacent=[], new_apples=[], new_waste=[], under_agent=[], eaten=[], unfilled=[], free_waste=[],
                 auto_resets=0)
    wp = cells(case.amap, "HR") if case.game == C else np.zeros((0, 2), int)
    for k in range(case.steps):
        if case.masked_reset is not None and k == case.masked_reset:
            ora.reset(mask=reset_mask(case))
        if case.full_reset_before(k):
            ora.reset()
        w0 = ora.get_state()["world"]
        obs, rew, _ = ora.step(tr.actions[case.slot(k)])
        s1 = ora.get_state()
        w1, pos = s1["world"], s1["pos"]
        used = ora.waste_count()
        # ---- what the guards count (from the states before any automatic reset)
        a0, a1 = w0[:, ap[:, 0], ap[:, 1]] == ord("A"), w1[:, ap[:, 0], ap[:, 1]] == ord("A")      # [E, apple points]
        new = a1 & ~a0                               # (an eaten apple cannot return in the same step: its eater stands on it)
        stats["empties"].append(ap.shape[0] - (a0 & a1).sum(1))    # apple points without an apple when the spawn pass looked
        grid = np.zeros(w1.shape, bool)
        grid[:, ap[:, 0], ap[:, 1]] = new
        adj = np.zeros(E, bool)
        for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
            sh = np.roll(np.roll(grid, -dr, 1), -dc, 2)          # (the border is wall: nothing wraps)
            adj |= (grid & sh).any((1, 2))
        stats["adjacent"].append(adj)
        stats["new_apples"].append(new.sum(1))
        stats["eaten"].append((a0 & ~a1).sum(1))
        occupied = np.zeros(w1.shape, bool)
        for i in range(N):
            occupied[np.arange(E), pos[:, i, 0], pos[:, i, 1]] = True
        stats["unfilled"].append((~a1 & ~occupied[:, ap[:, 0], ap[:, 1]]).sum(1))     # empty unoccupied apple points after the step
        if case.game == C:
            h0, h1 = w0 == ord("H"), w1 == ord("H")
            nw = h1 & ~h0
            stats["new_waste"].append(nw.sum((1, 2)))
            stats["under_agent"].append((nw & occupied).any((1, 2)))
            # free waste points when the spawn pass looked = not 'H' after the step, plus the one it filled
            stats["free_waste"].append((~h1[:, wp[:, 0], wp[:, 1]]).sum(1) + nw.sum((1, 2)))
        done = np.zeros((E, N), np.uint8)
        if case.horizon:
            d = s1["t"] >= case.horizon
            done[d] = 1
            if d.any():                              # SSD_AUTO_RESET: reset by the same launch, the obs rows are the reset's
                robs = ora.reset(mask=d.astype(np.uint8))
                obs[d] = robs[d]
                stats["auto_resets"] += int(d.sum())
                used = ora.waste_count()
        tr.obs.append(obs); tr.rew.append(rew); tr.done.append(done); tr.waste.append(used)
    tr.final = ora.get_state()
    tr.stats = {k: (np.array(v) if isinstance(v, list) else v) for k, v in stats.items()}
    return tr


def check_guards(case, tr):
    """Asserts that the oracle's run reaches what the case claims.  Returns the figures (for -s runs)."""
    s, P = tr.stats, potential(case.amap) if case.game == C else 0
    steps = case.E * case.steps
    used = np.array(tr.waste)
    fig = dict(over64=int((s["empties"] > 64).sum()), upto64=int(((s["empties"] >= 1) & (s["empties"] <= 64)).sum()),
               adjacent=float(s["adjacent"].sum()) / steps, new_apples=int(s["new_apples"].sum()), eaten=int(s["eaten"].sum()),
               counts=len(set(used.ravel().tolist())) if case.game == C else 0,
               under_agent=int(s["under_agent"].sum()) if case.game == C else 0, auto_resets=s["auto_resets"])
    for g in case.guards:
        if g == "over64":
            assert fig["over64"] > 0, fig            # the general form of the candidate pass
        elif g == "upto64":
            assert fig["upto64"] > 0, fig            # the compacting form
        elif g == "adjacent":
            assert fig["adjacent"] >= 0.05, fig      # counts must use the pre-spawn map: adjacent apples of the same step
        elif g == "refilled":
            assert int(s["unfilled"].sum()) == 0 and fig["new_apples"] > 0, fig    # always: every empty unoccupied point is an apple
        elif g == "no_new_apples":
            assert fig["new_apples"] == 0, fig
        elif g == "eaten":
            assert fig["eaten"] > 100, fig
        elif g == "counts20":
            assert fig["counts"] >= 20, fig          # distinct waste counts the thresholds were read at
        elif g == "under_agent":
            assert fig["under_agent"] >= 1, fig      # waste landed under an agent standing in the river
        elif g == "both_ways":
            d = np.diff(used.astype(np.int64), axis=0)
            assert (d > 0).any() and (d < -1).any(), fig    # the count rises, and falls by several in one step
        elif g == "all_free":
            assert int(s["free_waste"].max()) == P, fig     # the argmin ran over every waste point
        elif g == "no_new_waste":
            assert int(s["new_waste"].sum()) == 0, fig
        elif g == "first_entry":
            assert (used == 0).any(), fig
        elif g == "last_entry":
            assert (used == P).any(), fig
        elif g == "past_end":
            assert (used > P).any(), fig             # the clamp to the tables' last entry
        elif g == "auto_resets":
            assert fig["auto_resets"] >= 5 * case.E, fig
        else:
            raise AssertionError("unknown guard " + g)
    return fig


# ---------------------------------------------------------------------------------------------------- the library's own tables
def library_case(game):
    """The runs of the library-tables test (one step in which everybody STAYs, then device-drawn actions; the reference's
    constants): Cleanup with 130 envs whose start worlds hold e mod 120 cells of waste, Harvest from the emptied worlds."""
    if game == C:
        return Case("lib_c", C, C25, 130, 5, 40, start_river_crowd_counts, None, 531)
    return Case("lib_h", H, K.HARVEST_MAP, 64, 5, 40, start_emptied, None, 532)


def library_case_counts(case):
    """The waste counts the oracle reads its thresholds at over the run of a library case."""
    ora = pyoracle.Oracle(case.game, case.amap, case.E, case.N, G.default_lut(), seed=case.seed)
    ora.reset()
    ora.set_state(**case.start(case, ora.get_state(), np.random.RandomState(case.seed)))
    ora.step(np.full((case.E, case.N), 4, np.int32))             # everybody STAYs: the thresholds are read at the start counts
    used = set(ora.waste_count().tolist())
    for _ in range(case.steps - 1):
        ora.step_random(want_obs=False)
        used |= set(ora.waste_count().tolist())
    return used
