"""The Watershed games on the MI355X: the dict drop-ins replay every reference fixture; WatershedVecEngine equals the NumPy mirror
(tests/watershed_mirror.py) at 4096 and 65536 envs over full episodes with masked and automatic resets; one rollout launch equals
the same single steps; and crafted states that sweep the reward's square densely tell libm's powf(x, 2) from x*x."""
import glob
import os

import numpy as np
import pytest

from watershed_mirror import SEQ, SEQ_COMM, ST_BAD_ACTION, ST_NOT_RESET, WatershedMirror

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "watershed", "ws_*.npz")))
TYPES = {0: int, 1: np.float32, 2: np.float64, 3: np.int64}


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_dropin_replays_reference_fixture(path):
    from sequential_social_dilemma_games_amd import WatershedSeqCommEnv, WatershedSeqEnv
    g = load(path)
    comm, rao, lr, lo, seed, n, episodes, L = [int(v) for v in g["meta"]]
    cls = WatershedSeqCommEnv if comm else WatershedSeqEnv
    for s in range(n):
        env = cls(return_agent_actions=bool(rao), local_rew=bool(lr), local_obs=bool(lo), seed=seed, env_index=s)
        t = 0
        for ep in range(episodes):
            obs = env.reset()
            for k in range(L + 1):
                if k:
                    acting = int(g["agent"][s, t - 1])
                    aid = "agent-%d" % acting
                    if comm and acting < 4:
                        ad = {aid: int(g["action"][s, t])}
                    else:
                        ad = {aid: np.array([g["action"][s, t]], dtype=np.float32)}
                    obs, rew, done, info = env.step(ad)
                    assert type(ad[aid]) is TYPES[int(g["mutated_type"][s, t])], "the action dict is rewritten in place"
                aid = "agent-%d" % int(g["agent"][s, t])
                assert list(obs) == [aid], (t, list(obs))
                o = obs[aid]
                assert isinstance(o, dict) == bool(g["obs_is_dict"][s, t]), t
                if isinstance(o, dict):
                    assert np.array_equal(o["other_agent_actions"], g["other"][s, t]) and o["other_agent_actions"].dtype == np.int64
                    assert np.array_equal(o["visible_agents"], [1, 1, 1])
                    o = o["curr_obs"]
                assert o.dtype == (np.float64 if g["obs_dtype"][s, t] else np.int64), t
                assert len(o) == g["obs_len"][s, t] and np.array_equal(o, g["obs"][s, t, :len(o)]), (t, o, g["obs"][s, t])
                if k:
                    r = rew[aid]
                    assert type(r) is TYPES[int(g["rew_type"][s, t])] and r == g["rew"][s, t], (t, r, g["rew"][s, t])
                    assert done == {aid: bool(g["done_agent"][s, t]), "__all__": bool(g["done_all"][s, t])}, t
                    inf = info[aid]
                    assert inf["viol"] == list(g["viol"][s, t]), t
                    assert type(inf["temp"]) is TYPES[int(g["temp_type"][s, t])] and inf["temp"] == g["temp"][s, t], t
                    assert inf["end"] is bool(g["end"][s, t]) and inf["true_end"] is bool(g["true_end"][s, t]), t
                    assert [type(v) for v in inf["running_rew"]] == [TYPES[int(c)] for c in g["running_type"][s, t]], t
                    assert list(inf["running_rew"]) == list(g["running"][s, t]), t
                    nk = int(g["acts_n"][s, t])
                    assert list(inf["acts"]) == ["agent-%d" % a for a in g["acts_keys"][s, t, :nk]], t
                    assert [float(v) for v in inf["acts"].values()] == list(g["acts"][s, t, :nk]), t
                t += 1
        assert env._eng.status() == 0
        env.close()


def _actions(rng, agent, variant, E):
    """Random actions for the acting agents: comm agents an integer 0..4, action agents U[0,1) with exact 0 / 1 / 1/2 and unclipped
    values in [-1, 2)."""
    a = rng.random(E).astype(np.float32)
    k = rng.random(E)
    a[k < 0.05] = 0.0
    a[(k >= 0.05) & (k < 0.1)] = 1.0
    a[(k >= 0.1) & (k < 0.15)] = 0.5
    wide = k >= 0.85
    a[wide] = (rng.random(int(wide.sum())) * 3.0 - 1.0).astype(np.float32)
    if variant == SEQ_COMM:
        comm = agent < 4
        a[comm] = rng.integers(0, 5, int(comm.sum())).astype(np.float32)
    return a


def _compare(got, want, what):
    for name, x, y in zip(("obs", "agent", "rew", "done"), got, want):
        x = x.cpu().numpy()
        assert np.array_equal(x, y), "%s: %s differs in %d envs" % (what, name, int((x != y).reshape(len(y), -1).any(1).sum()))


@pytest.mark.parametrize("E", [4096, 65536])
@pytest.mark.parametrize("variant", [SEQ, SEQ_COMM])
def test_vec_engine_equals_mirror(variant, E):
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    flags = dict(local_obs=E == 4096, local_rew=variant == SEQ_COMM)
    eng = WatershedVecEngine(variant, E, seed=77, env_index_base=5, **flags)
    m = WatershedMirror(variant, E, seed=77, env_index_base=5, **flags)
    rng = np.random.default_rng(E + variant)
    obs, agent = eng.reset()
    mo, ma = m.reset()
    assert np.array_equal(obs.cpu().numpy(), mo) and np.array_equal(agent.cpu().numpy(), ma)
    L = 43 if variant == SEQ else 131
    agent_h = ma
    for k in range(3 * L):
        auto = k >= L                                              # the first episode ends without, the later ones with auto-reset
        if k == L // 2 or k == 2 * L + 7:                          # masked resets in the middle of an episode
            mask = rng.random(E) < 0.3
            o, a = eng.reset(torch.from_numpy(mask.astype(np.uint8)))
            mo, ma = m.reset(mask)
            assert np.array_equal(o.cpu().numpy(), mo) and np.array_equal(a.cpu().numpy(), ma)
            agent_h = np.where(mask, ma, agent_h)
        if k == L:                                                 # episode 1 ended everywhere except the masked envs: reset all
            eng.reset()
            _, agent_h = m.reset()
        act = _actions(rng, agent_h, variant, E)
        got = eng.step(torch.from_numpy(act), auto_reset=auto)
        want = m.step(act, auto_reset=auto)
        _compare(got, want, "step %d" % k)
        agent_h = want[1]
        if k % 17 == 0 or k == 3 * L - 1:
            inf = eng.info()
            for name, w in zip(("viol", "true_end", "running_rew", "temp", "other_agent_actions"), m.info()):
                assert np.array_equal(inf[name].cpu().numpy(), w), (k, name)
    assert eng.status() == 0 and m.status == 0


@pytest.mark.parametrize("variant", [SEQ, SEQ_COMM])
def test_rollout_equals_single_steps(variant):
    """rollout_actions(K = 131) -- one launch, the state in registers -- equals 131 ssd_ws_step calls bit for bit, auto-reset included,
    and both equal the mirror."""
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    E, K = 4096, 131
    a = WatershedVecEngine(variant, E, seed=3, local_obs=True)
    b = WatershedVecEngine(variant, E, seed=3, local_obs=True)
    m = WatershedMirror(variant, E, seed=3, local_obs=True)
    a.reset(), b.reset()
    _, agent_h = m.reset()
    rng = np.random.default_rng(11)
    acts = np.zeros((K, E), np.float32)
    wants = []
    for k in range(K):
        acts[k] = _actions(rng, agent_h, variant, E)
        wants.append(m.step(acts[k], auto_reset=True))
        agent_h = wants[-1][1]
    dev_acts = torch.from_numpy(acts).cuda()
    obs, agent, rew, done = a._outputs((K,))
    a.rollout_actions(dev_acts, K, obs, agent, rew, done, auto_reset=True)
    for k in range(K):
        got = b.step(dev_acts[k], auto_reset=True)
        for x, y in zip(got, (obs[k], agent[k], rew[k], done[k])):
            assert torch.equal(x, y), k
        _compare(got, wants[k], "step %d" % k)
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert a.status() == 0 and b.status() == 0


def test_crafted_states_sweep_the_square():
    """Every env closes one round from a crafted state whose flows x sweep [-60, 400] densely; the six rewards f_rew then hold
    a * x**2 + b * x + c with NumPy's square (libm powf).  A kernel that squared with x*x fails here: the sweep is checked to hold
    many x where the two squares give different f_rew."""
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    E = 1 << 18
    eng = WatershedVecEngine(SEQ, E, seed=9)
    m = WatershedMirror(SEQ, E, seed=9)
    eng.reset()
    m.reset()
    rng = np.random.default_rng(5)
    st = eng.get_state()
    assert np.array_equal(st["season"], m.season)
    st["phase"][:] = 4                                             # the next step closes the round
    st["hist"][:, :3] = (rng.random((E, 3)) * 2.6 - 0.3).astype(np.float32)
    eng.set_state(st)
    m.p[:] = 4
    m.hist[:, :3] = st["hist"][:, :3]
    act = (rng.random(E) * 2.6 - 0.3).astype(np.float32)
    got = eng.step(torch.from_numpy(act))
    want = m.step(act)
    _compare(got, want, "crafted step")
    fr = eng.get_state()["f_rew"]
    assert np.array_equal(fr, m.fr)
    # how many of those rewards x*x would have got wrong
    q1 = np.array([160, 115, 80], np.float32)[m.season % 3]
    x1 = q1 * m.hist[:, 0]
    sq_pow = np.array([np.float32(v) ** 2 for v in x1], np.float32)
    wrong = (np.float32(-.2) * (x1 * x1) + np.float32(6) * x1 + np.float32(-5)) != (np.float32(-.2) * sq_pow + np.float32(6) * x1 + np.float32(-5))
    assert wrong.sum() > 20, int(wrong.sum())
    assert eng.status() == 0


def test_bad_comm_action_sets_the_status_bit():
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    eng = WatershedVecEngine(SEQ_COMM, 64, seed=1)
    eng.reset()
    eng.step(torch.full((64,), 2.5))                               # agent 0's message must be an integer 0..4
    assert eng.status() & ST_BAD_ACTION
    assert eng.status() == 0                                       # (cleared by the read before)


def test_kernel_matches_the_reference_square_sweep():
    """The reference's own cal_rewards over a dense sweep of the flows (tests/golden/watershed/square_sweep.npz, with 500+ rounds
    where x*x would give other rewards): the kernel closes the same rounds to the same f_rew, pen and violations."""
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    with np.load(os.path.join(HERE, "golden", "watershed", "square_sweep.npz")) as z:
        g = {k: z[k] for k in z.files}
    n = len(g["season"])
    eng = WatershedVecEngine(SEQ, n, seed=1)
    eng.reset()
    st = eng.get_state()
    st["season"][:] = g["season"]
    st["phase"][:] = 4
    st["hist"][:, :3] = g["actions"][:, :3]
    eng.set_state(st)
    eng.step(torch.from_numpy(np.ascontiguousarray(g["actions"][:, 3])))
    st = eng.get_state()
    assert np.array_equal(st["f_rew"], g["f_rew"]), int((st["f_rew"] != g["f_rew"]).any(1).sum())
    assert np.array_equal(st["pen"], g["pen"]) and np.array_equal(st["viol"], g["viol"])
    assert eng.status() == 0


@pytest.mark.parametrize("variant", [SEQ, SEQ_COMM])
def test_rollout_rings_and_step0(variant):
    """A rollout call whose action ring (7) and output ring (5) are shorter than the call (40 phases) and that starts at step0 = 3:
    phase k reads action slot (3 + k) % 7 and writes output slot (3 + k) % 5 -- the same as 40 single steps."""
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    E, K, R, RING, S0 = 2048, 40, 7, 5, 3
    a = WatershedVecEngine(variant, E, seed=21)
    b = WatershedVecEngine(variant, E, seed=21)
    a.reset(), b.reset()
    acts = torch.randint(0, 2, (R, E), device="cuda").float()      # 0 / 1: valid for comm and action agents alike
    obs, agent, rew, done = a._outputs((RING,))
    a.rollout_actions(acts, K, obs, agent, rew, done, step0=S0, auto_reset=True)
    last = {}
    for k in range(K):
        last[(S0 + k) % RING] = b.step(acts[(S0 + k) % R], auto_reset=True)
    for slot, got in last.items():
        for x, y in zip(got, (obs[slot], agent[slot], rew[slot], done[slot])):
            assert torch.equal(x, y), slot
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert a.status() == 0 and b.status() == 0


def test_never_reset_envs_are_left_alone():
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    E = 300
    eng = WatershedVecEngine(SEQ, E, seed=2)
    before = eng.get_state()
    obs, agent, rew, done = eng._outputs((2,))
    for t in (obs, agent, rew, done):
        t.fill_(7)
    eng.rollout_actions(torch.full((1, E), 0.5, device="cuda"), 3, obs, agent, rew, done)
    assert eng.status() == ST_NOT_RESET
    for t in (obs, agent, rew, done):
        assert not t.any()
    after = eng.get_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key


def test_mis_shaped_buffers_raise_before_any_launch():
    """Every buffer the engine hands a kernel is checked on the host: device, dtype, exact shape, contiguity, alignment."""
    import torch
    from sequential_social_dilemma_games_amd import WatershedVecEngine
    E = 256
    eng = WatershedVecEngine(SEQ_COMM, E, seed=4)
    eng.reset()
    before = eng.get_state()
    good = eng._outputs()
    bad_outs = [
        (torch.empty((E - 1, 12), device="cuda"),) + good[1:],                                 # obs for a smaller batch
        (torch.empty((E, 12), dtype=torch.float16, device="cuda"),) + good[1:],              # wrong dtype
        (torch.empty((E, 12)),) + good[1:],                                                    # host memory
        (torch.empty((12, E), device="cuda").t(),) + good[1:],                                 # not contiguous
        (torch.empty(E * 12 + 1, device="cuda")[1:].view(E, 12),) + good[1:],                 # rows not 16-byte aligned
        good[:1] + (torch.empty(E - 8, dtype=torch.int8, device="cuda"),) + good[2:],         # short agent
        good[:2] + (torch.empty(E, dtype=torch.float32, device="cuda"),) + good[3:],          # f32 rewards
    ]
    acts = torch.zeros(E, device="cuda")
    for out in bad_outs:
        with pytest.raises(ValueError):
            eng.step(acts, out=out)
    with pytest.raises(ValueError):
        eng.step(torch.zeros(E - 1, device="cuda"))
    with pytest.raises(ValueError):
        eng.reset(torch.ones(E // 2, dtype=torch.uint8, device="cuda"))
    ring = eng._outputs((4,))
    with pytest.raises(ValueError):                                                            # rings of different lengths
        eng.rollout_actions(torch.zeros((4, E), device="cuda"), 8, ring[0], ring[1][:2], ring[2], ring[3])
    with pytest.raises(ValueError):
        eng.rollout_actions(torch.zeros((4, E + 1), device="cuda"), 8, *ring)
    torch.cuda.synchronize()
    after = eng.get_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert eng.status() == 0

