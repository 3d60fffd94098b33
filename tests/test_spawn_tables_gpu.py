"""The step kernel's spawn phase under caller-supplied probability tables, kernel against oracle bit for bit.

At the reference's constants the phase (ssd_kernels.hip after the beams: Harvest spawn_apples, harvest.py:69-104; Cleanup
compute_probabilities + spawn_apples_and_waste, cleanup.py:113-171) is nearly idle: two adjacent apples of one step in 0.2 % of
the env-steps, never more than 64 empty apple points, Cleanup mostly in depletion.  The tables of tests/spawn_tables.py make
every step decide: thresholds of 2^32 ("always": thr_h_always, the 64-bit compare of the Cleanup tables), of 0, count-decided
ones (p = 1/64, 1, 0, 1: a neighbour count off by one shows at once), count-parity ones for Cleanup (a waste count off by one
shows at once), start worlds on both sides of the 64-candidate compaction edge, and waste counts from 0 to past the tables' end.

Resets: SSD_AUTO_RESET with a horizon of 5 and envs out of phase (per-call steps: the flag is ssd_step's), a masked ssd_reset
mid-run, and full resets inside the rollout calls (reset_every): the step after a reset must use the reset world's count.

Every case runs through per-call stepping, rollout chains (the split coherent path where the environment expects it) and the fused
kernel; every step's observations, rewards and dones and the final world / pos / orient / episode / t are compared, and for Cleanup
ssd_get_waste_count after every per-call step.  Each case also asserts, from the oracle's states, the coverage it claims
(spawn_tables.check_guards; tests/test_spawn_tables_cpu.py does the same without a GPU).

The oracle with tables is pinned to the reference by the t??_* fixtures (tests/test_oracle_golden.py; the kernel replays them in
tests/test_hip_parity.py)."""
import os

import numpy as np
import pytest

import spawn_tables as ST
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.engine import VecEngine

pytestmark = pytest.mark.gpu


def _split_expected():
    """The split coherent chains are the library's default; the documented knobs can turn each layer off."""
    return all(os.environ.get(k, "1") != "0" for k in ("SSD_AQL", "SSD_AQL_COHERENT", "SSD_AQL_SPLIT"))


def _engine(case, tr):
    eng = VecEngine(case.game, case.amap, num_envs=case.E, num_agents=case.N, view_len=case.view_len, seed=case.seed,
                    **case.tables_kw())
    eng.reset()
    eng.set_state(**tr.start)
    if case.horizon:
        eng.set_horizon(case.horizon)
    return eng


def _same_final(eng, tr, case):
    a = eng.get_state()
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], tr.final[key], err_msg=key)
    if case.game == K.GAME_CLEANUP:
        np.testing.assert_array_equal(eng.waste_count(), tr.waste[-1], err_msg="waste count of the last step")
    assert eng.status() == 0


PAIRS = [(c.name, m) for c in ST.CASES for m in c.modes]       # (case-major: a case's oracle run is computed once and shared)


@pytest.mark.parametrize("name,mode", PAIRS)
def test_spawn_phase_under_tables(name, mode):
    import torch
    case = ST.BY_NAME[name]
    tr = ST.trajectory(name)
    if mode == case.modes[0]:
        print(name, ST.check_guards(case, tr))
    E, N, V, steps = case.E, case.N, 2 * case.view_len + 1, case.steps
    eng = _engine(case, tr)
    a_dev = torch.from_numpy(tr.actions).cuda()
    mask = torch.from_numpy(ST.reset_mask(case)).cuda()
    if mode == "calls":
        for k in range(steps):
            if case.masked_reset == k:
                eng.reset(mask=mask)
            if case.full_reset_before(k):
                eng.reset()
            o, r, d = eng.step(a_dev[case.slot(k)], auto_reset=bool(case.horizon))
            np.testing.assert_array_equal(r.cpu().numpy(), tr.rew[k], err_msg="rewards of step %d" % k)
            assert np.array_equal(o.cpu().numpy(), tr.obs[k]), "observations of step %d differ" % k
            np.testing.assert_array_equal(d.cpu().numpy(), tr.done[k], err_msg="dones of step %d" % k)
            if case.game == K.GAME_CLEANUP:          # the count the step's thresholds were read at (after a reset: the reset world's)
                np.testing.assert_array_equal(eng.waste_count(), tr.waste[k], err_msg="waste count of step %d" % k)
    else:
        obs = torch.zeros((steps, E, N, V, V, 3), dtype=torch.uint8, device="cuda")
        rew = torch.zeros((steps, E, N), dtype=torch.int32, device="cuda")
        done = torch.ones((steps, E, N), dtype=torch.uint8, device="cuda")
        eng.set_rollout_chains(2 if mode == "chains" else 1)
        m = case.masked_reset
        for lo, hi in ([(0, steps)] if m is None else [(0, m), (m, steps)]):
            if lo:
                eng.reset(mask=mask)
            eng.rollout_actions(a_dev, hi - lo, obs, rew, done, reset_every=case.reset_every, step0=case.step0 + lo,
                                fused=(mode == "fused"))
            path = eng.rollout_path()
            if mode == "fused":
                assert path["fused"], path
            elif case.split and _split_expected():
                assert path["aql"] and path["coherent"] and path["split"] and not path["fused"] and path["chains"] == 2, path
        g_obs, g_rew, g_done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        for k in range(steps):                       # (rings of `steps` slots: every step's outputs are there)
            np.testing.assert_array_equal(g_rew[case.slot(k)], tr.rew[k], err_msg="rewards of step %d" % k)
            assert np.array_equal(g_obs[case.slot(k)], tr.obs[k]), "observations of step %d differ" % k
            np.testing.assert_array_equal(g_done[case.slot(k)], tr.done[k], err_msg="dones of step %d" % k)
    _same_final(eng, tr, case)
    eng.close()


@pytest.mark.parametrize("game", [K.GAME_HARVEST, K.GAME_CLEANUP])
def test_library_derives_the_tables_a_null_pointer_asks_for(game):
    """library_tables=True passes NULL for the three tables and the colour table -- what a C caller following INTEGRATION.md
    does --: ssd_create derives them itself (ssd_capi.hip).  Against the default handle (tables and colours derived in Python)
    with the same seed: a step of STAYs and 39 device-drawn steps, identical observations, rewards and state, identical render_full (the colours).
    Cleanup: 130 envs whose start worlds hold e mod 120 cells of waste, so that every entry of both tables is indexed (asserted
    through ssd_get_waste_count); Harvest: the emptied start worlds.
    A threshold off by one unit in 2^32 cannot be seen this way (a draw would have to hit that very value): the test guards the
    constants and the indexing of the library's derivation, not its rounding."""
    import torch
    case = ST.library_case(game)
    engs = [VecEngine(game, case.amap, num_envs=case.E, num_agents=case.N, seed=case.seed, library_tables=lib) for lib in (False, True)]
    obs0 = [e.reset() for e in engs]
    assert torch.equal(obs0[0], obs0[1])
    start = case.start(case, engs[0].get_state(), np.random.RandomState(case.seed))
    used = set()
    for e in engs:
        e.set_state(**start)
    stay = torch.full((case.E, case.N), 4, dtype=torch.int32, device="cuda")
    for k in range(case.steps):                      # (first everybody STAYs: the thresholds are read at the start counts)
        outs = [e.step(stay) if k == 0 else e.step_random() for e in engs]
        for a, b, what in zip(outs[0], outs[1], ("observations", "rewards", "dones")):
            assert torch.equal(a, b), "%s of step %d differ" % (what, k)
        if game == K.GAME_CLEANUP:
            wc = [e.waste_count() for e in engs]
            np.testing.assert_array_equal(wc[0], wc[1])
            used |= set(wc[0].tolist())
    a, b = (e.get_state() for e in engs)
    for key in ("world", "pos", "orient", "episode", "t"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    if game == K.GAME_CLEANUP:
        assert used >= set(range(ST.potential(case.amap) + 1)), sorted(set(range(120)) - used)
        assert (a["world"] == ord("A")).any()        # (apples grew: the apple table was not all zero)
    for e in (0, 1, case.E - 1):
        rgb = [x.render_full(e) for x in engs]
        assert np.array_equal(rgb[0], rgb[1]) and len(np.unique(rgb[0].reshape(-1, 3), axis=0)) >= 4
    for e in engs:
        assert e.status() == 0
        e.close()
