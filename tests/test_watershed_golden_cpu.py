"""The Watershed mirror (tests/watershed_mirror.py) against every reference fixture in tests/golden/watershed/, step for step,
bit for bit: observations, observing agent, reward value and type, dones, and the info fields.  Plus the reference test that
regenerates one scenario per class and compares it with the committed fixture."""
import glob
import os

import numpy as np
import pytest

from watershed_mirror import (DONE_AGENT, DONE_ALL, END, REW_F64, REW_INT, SEQ, SEQ_COMM, WatershedMirror, close_crafted_rounds)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "watershed", "ws_*.npz")))


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_there_are_sixteen_fixtures():
    assert len(FIXTURES) == 16


def replay_mirror(g):
    """Drive the mirror with a fixture's actions; yields (t, obs, agent, rew, flags, info or None)."""
    comm, rao, lr, lo, seed, n, episodes, L = [int(v) for v in g["meta"]]
    m = WatershedMirror(SEQ_COMM if comm else SEQ, n, seed=seed, local_obs=bool(lo), local_rew=bool(lr))
    t = 0
    for ep in range(episodes):
        obs, agent = m.reset()
        yield t, obs, agent, None, None, None
        t += 1
        for k in range(L):
            obs, agent, rew, flags = m.step(g["action"][:, t].astype(np.float32))
            yield t, obs, agent, rew, flags, m.info()
            t += 1
    assert m.status == 0


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_mirror_matches_reference_fixture(path):
    g = load(path)
    from sequential_social_dilemma_games_amd.watershed import obs_dtype_is_float, obs_len
    comm, rao, lr, lo = [int(v) for v in g["meta"][:4]]
    for t, obs, agent, rew, flags, info in replay_mirror(g):
        assert np.array_equal(agent, g["agent"][:, t]), t
        assert np.array_equal(obs.astype(np.float64), g["obs"][:, t]), (t, obs, g["obs"][:, t])
        for e in range(len(agent)):
            assert obs_len(comm, lo, agent[e]) == g["obs_len"][e, t]
            assert obs_dtype_is_float(comm, agent[e]) == bool(g["obs_dtype"][e, t])
        if rew is None:
            continue
        assert np.array_equal(rew, g["rew"][:, t]), (t, rew, g["rew"][:, t])
        want_type = np.where(flags & REW_INT, 0, np.where(flags & REW_F64, 2, 1))
        assert np.array_equal(want_type, g["rew_type"][:, t]), t
        assert np.array_equal((flags & DONE_AGENT) != 0, g["done_agent"][:, t] != 0), t
        assert np.array_equal((flags & DONE_ALL) != 0, g["done_all"][:, t] != 0), t
        assert np.array_equal((flags & END) != 0, g["end"][:, t] != 0), t
        viol, true_end, running, temp, other = info
        assert np.array_equal(viol, g["viol"][:, t]), t
        assert np.array_equal(true_end, g["true_end"][:, t]), t
        assert np.array_equal(running, g["running"][:, t]), (t, running, g["running"][:, t])
        assert np.array_equal(temp, g["temp"][:, t]), t
        d = g["obs_is_dict"][:, t] != 0
        assert np.array_equal(other[d], g["other"][d, t]), t


SWEEP = os.path.join(HERE, "golden", "watershed", "square_sweep.npz")


def test_mirror_matches_the_reference_square_sweep():
    """square_sweep.npz holds the reference's own cal_rewards over a dense sweep of the flows -- including every round of the
    sweep where x*x in place of NumPy's square changes a reward.  The mirror reproduces f_rew, pen and the violations of every
    round; and the sweep does tell the two squares apart (in the rounds so flagged, x*x gives other rewards)."""
    g = load(SWEEP)
    n = len(g["season"])
    m = WatershedMirror(SEQ, n, seed=1)
    m.reset()
    close_crafted_rounds(m, g["season"], g["actions"])
    assert np.array_equal(m.fr, g["f_rew"])
    assert np.array_equal(m.pen, g["pen"]) and np.array_equal(m.viol, g["viol"])
    assert int(g["xx_differs"].sum()) >= 500
    # the same rounds with x*x: wrong exactly where flagged
    q1 = np.array([160, 115, 80], np.float32)[g["season"] % 3]
    q2 = np.array([65, 50, 35], np.float32)[g["season"] % 3]
    s = np.array([15, 12, 10], np.float32)[g["season"] % 3]
    a = g["actions"]
    f1 = q1 * (np.float32(1) - a[:, 0])
    f3 = q2 * (np.float32(1) - a[:, 2]) + (f1 + s) * a[:, 1]
    x4 = q2 * a[:, 2]
    x = [q1 * a[:, 0], (f1 + s) * a[:, 1], q2 - x4, x4, None, f3 * a[:, 3]]
    x[4] = (x[1] + x[2]) - x[5]
    A = [np.float32(v) for v in (-.2, -.06, -.29, -.13, -.056, -.15)]
    B = [np.float32(v) for v in (6, 2.5, 6.28, 6, 3.74, 7.6)]
    Cc = [np.float32(v) for v in (-5, 0, -3, -6, -23, -15)]
    xx = np.stack([(A[j] * (x[j] * x[j]) + B[j] * x[j]) + Cc[j] for j in range(6)], 1)
    assert np.array_equal((xx != g["f_rew"]).any(1), g["xx_differs"] != 0)


@pytest.mark.reference
def test_regenerated_square_sweep_equals_committed_fixture():
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gen_golden_watershed as gen
    fresh = gen.record_square_sweep(gen.import_reference())
    old = load(SWEEP)
    assert set(fresh) == set(old)
    for k in fresh:
        assert np.array_equal(fresh[k], old[k]), k


@pytest.mark.reference
@pytest.mark.parametrize("comm", [0, 1])
def test_regenerated_scenario_equals_committed_fixture(comm):
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gen_golden_watershed as gen
    W = gen.import_reference()
    rao, lr, lo = (1, 1, 0) if comm else (0, 0, 1)
    fresh = gen.record(W, comm, rao, lr, lo)
    old = load(os.path.join(HERE, "golden", "watershed", gen.name_of(comm, rao, lr, lo)))
    assert set(fresh) == set(old)
    for k in fresh:
        assert np.array_equal(fresh[k], old[k]), k
