"""Watershed episode statistics on the MI355X (the stats instances of csrc/ssd_watershed.hip, csrc/ssd_ws_stats.hip): an
attached engine's drain against the NumPy restatement (tests/ws_stats_ref.py) fed by an unattached engine stepped one step at
a time with info() after each; rings and state untouched by the handle; call-split and ring invariance; envs out of lock step
after a masked reset; the policy path; keep, discard, detach and the refusals.

Shapes: E = 257 (a second block with one live lane) and E = 1; both variants, local_rew 0 and 1; K = two episodes + 5 steps."""
import functools

import numpy as np
import pytest
import torch

from sequential_social_dilemma_games_amd import WatershedEpisodeStats, _capi
from sequential_social_dilemma_games_amd.watershed import EPISODE_STEPS, WatershedVecEngine
from sequential_social_dilemma_games_amd.watershed_stats import summarize
from ws_stats_ref import WsStatsRef, assert_drains_equal, assert_summaries_equal

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEQ, SEQ_COMM = _capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM
DONE_ALL = _capi.SSD_WS_DONE_ALL
SEED = 77
CASES = [(v, lr) for v in (SEQ, SEQ_COMM) for lr in (0, 1)]
IDS = ["%s-r%d" % ("seqcomm" if v else "seq", lr) for v, lr in CASES]


def steps_of(variant):
    return 2 * EPISODE_STEPS[variant] + 5                        # 91 / 267


def make_actions(variant, K, pos):
    """f32 [K, E]: uniform in [0, 1] for the action agents, messages 0..4 for the comm agents.  pos int [E]: how many steps into
    its episode each env is at step 0 (auto-reset: the count wraps at the episode length); SeqComm's comm agents act in the first
    8 of every 12 phases."""
    rng = np.random.default_rng(1234 + 10 * variant + K)
    E, L = len(pos), EPISODE_STEPS[variant]
    a = rng.random((K, E)).astype(np.float32)
    a[rng.random((K, E)) < 0.03] = 1.0
    if variant == SEQ_COMM:
        at = (np.asarray(pos)[None, :] + np.arange(K)[:, None]) % L
        comm = (at % 12) < 8
        a[comm] = rng.integers(0, 5, int(comm.sum())).astype(np.float32)
    return a


def engine(variant, lr, E, attached=True):
    eng = WatershedVecEngine(variant, E, seed=SEED, local_rew=bool(lr), env_index_base=5)
    stats = None
    if attached:
        stats = WatershedEpisodeStats(variant, E)
        eng.attach_stats(stats)
    return eng, stats


def rings(E, R):
    return (torch.zeros((R, E, 12), dtype=torch.float32, device=DEV), torch.zeros((R, E), dtype=torch.int8, device=DEV),
            torch.zeros((R, E), dtype=torch.float64, device=DEV), torch.zeros((R, E), dtype=torch.uint8, device=DEV))


def stepwise_reference(variant, lr, E, actions, reset_odd_after=None):
    """The restatement's drain for these actions: an UNATTACHED engine stepped one step at a time, info() after each step and
    before the reset of the envs whose episode ended (what auto-reset does inside the kernel)."""
    eng, _ = engine(variant, lr, E, attached=False)
    ref = WsStatsRef(variant, E)
    eng.reset()
    ref.reset()
    for k in range(actions.shape[0]):
        if reset_odd_after is not None and k == reset_odd_after:
            odd = np.arange(E) % 2 == 1
            eng.reset(mask=odd)
            ref.reset(mask=odd)
        _, agent, rew, done = eng.step(torch.from_numpy(actions[k]).to(DEV))
        inf = eng.info()
        done_h = done.cpu().numpy()
        ref.step(rew.cpu().numpy(), done_h, agent.cpu().numpy(), inf["viol"].cpu().numpy(), inf["running_rew"].cpu().numpy(),
                 auto_reset=True)
        ended = (done_h & DONE_ALL) != 0
        if ended.any():
            eng.reset(mask=ended)
    assert eng.status() == 0
    state = eng.get_state()
    eng.close()
    return ref.drain(), state


@functools.lru_cache(maxsize=None)
def lockstep(variant, lr, E):
    """(actions, the restatement's drain, the final state) of K lock-step steps from a reset: computed once, shared, never changed."""
    K = steps_of(variant)
    actions = make_actions(variant, K, np.zeros(E, np.int64))
    drain, state = stepwise_reference(variant, lr, E, actions)
    return actions, drain, state


def close(eng, stats):
    assert eng.status() == 0
    eng.close()
    if stats is not None:
        stats.close()


@pytest.mark.parametrize("E", [257, 1])
@pytest.mark.parametrize("variant,lr", CASES, ids=IDS)
def test_one_rollout_call_against_the_restatement(variant, lr, E):
    actions, want, want_state = lockstep(variant, lr, E)
    K = steps_of(variant)
    acts = torch.from_numpy(actions).to(DEV)
    eng, stats = engine(variant, lr, E)
    eng.reset()
    out = rings(E, K)
    eng.rollout_actions(acts, K, *out, auto_reset=True)
    got = stats.drain(keep=True)
    assert_drains_equal(got, want, "drain")
    assert got["counts"].tolist() == [[2, 0, 2 * EPISODE_STEPS[variant]]] * E
    assert_summaries_equal(stats.summary(), summarize(want, variant))
    if lr == 0:
        assert (got["last_metrics"][:, 1] == 1.0).all(), "Equality is exactly 1 when every agent gets the collective reward"
    # the handle changes nothing of what the engine computes: an unattached twin, and the stepwise engine
    twin, _ = engine(variant, lr, E, attached=False)
    twin.reset()
    tout = rings(E, K)
    twin.rollout_actions(acts, K, *tout, auto_reset=True)
    for name, a, b in zip(("obs", "agent", "rew", "done"), out, tout):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    sa, sb = eng.get_state(), twin.get_state()
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k
        assert np.array_equal(sa[k].view(np.uint8), want_state[k].view(np.uint8)), k
    close(twin, None)
    close(eng, stats)


@pytest.mark.parametrize("outputs", ["ring5", "none"])
@pytest.mark.parametrize("variant,lr", CASES, ids=IDS)
def test_call_splits_and_rings_do_not_matter(variant, lr, outputs):
    E = 257
    actions, want, _ = lockstep(variant, lr, E)
    K = steps_of(variant)
    acts = torch.from_numpy(actions).to(DEV)
    eng, stats = engine(variant, lr, E)
    eng.reset()
    out = rings(E, 5) if outputs == "ring5" else (None, None, None, None)
    eng.step(acts[0], auto_reset=True)
    eng.rollout_actions(acts, 7, *out, step0=1, auto_reset=True)
    eng.rollout_actions(acts, K - 8, *out, step0=8, auto_reset=True)
    assert_drains_equal(stats.drain(), want, outputs)
    close(eng, stats)


@pytest.mark.parametrize("variant,lr", CASES, ids=IDS)
def test_out_of_lock_step_after_a_masked_reset(variant, lr):
    E, K, L = 257, steps_of(variant), EPISODE_STEPS[variant]
    odd = np.arange(E) % 2 == 1
    head = make_actions(variant, 10, np.zeros(E, np.int64))
    tail = make_actions(variant, K - 10, np.where(odd, 0, 10))
    actions = np.concatenate([head, tail])
    want, want_state = stepwise_reference(variant, lr, E, actions, reset_odd_after=10)
    eng, stats = engine(variant, lr, E)
    eng.reset()
    acts = torch.from_numpy(actions).to(DEV)
    eng.rollout_actions(acts, 10, auto_reset=True)
    eng.reset(mask=odd)
    eng.rollout_actions(acts, K - 10, step0=10, auto_reset=True)
    got = stats.drain()
    assert_drains_equal(got, want, "masked reset")
    # the even envs finish at steps L and 2L, the odd ones at 10 + L and, only where 10 + 2L <= K, once more: one truncated each
    assert got["counts"][~odd].tolist() == [[2, 0, 2 * L]] * int((~odd).sum())
    assert got["counts"][odd].tolist() == [[1, 1, L]] * int(odd.sum())
    state = eng.get_state()
    for k in state:
        assert np.array_equal(state[k].view(np.uint8), want_state[k].view(np.uint8)), k
    close(eng, stats)


@pytest.mark.parametrize("variant", [SEQ, SEQ_COMM], ids=["seq", "seqcomm"])
def test_policy_path_equals_a_replay_of_its_actions(variant):
    from sequential_social_dilemma_games_amd.policy import WatershedLSTMPolicy
    E, K = 257, steps_of(variant)
    policy = WatershedLSTMPolicy(variant, cell_size=64, seed=3).to(DEV)
    eng, stats = engine(variant, 1, E)
    eng.reset()
    batch = eng.sample(policy, K)
    got = stats.drain()
    assert got["counts"].tolist() == [[2, 0, 2 * EPISODE_STEPS[variant]]] * E
    # the actions as the env saw them: an action agent's clipped to [0, 1], a comm agent's message as it is
    a, actor = batch["actions"], batch["actor"]
    comm = (actor < 4) if variant == SEQ_COMM else torch.zeros_like(actor, dtype=torch.bool)
    clipped = torch.where(comm, a, torch.clamp(a, 0.0, 1.0)).contiguous()
    twin, tstats = engine(variant, 1, E)
    twin.reset()
    out = rings(E, K)
    twin.rollout_actions(clipped, K, *out, auto_reset=True)
    assert torch.equal(out[2].view(torch.uint8), batch["rew"].view(torch.uint8)), "the replay is the same trajectory"
    assert_drains_equal(got, tstats.drain(), "policy path")
    close(twin, tstats)
    close(eng, stats)


def test_keep_discard_detach_and_refusals():
    variant, E, L = SEQ, 257, EPISODE_STEPS[SEQ]
    actions, want, _ = lockstep(variant, 0, E)
    acts = torch.from_numpy(actions).to(DEV)
    eng, stats = engine(variant, 0, E)
    # a handle of another variant, env count or device kind is refused, and the engine keeps the one it has
    for bad in (WatershedEpisodeStats(SEQ_COMM, E), WatershedEpisodeStats(SEQ, E + 1)):
        with pytest.raises(_capi.SsdError, match="differ"):
            eng.attach_stats(bad)
        bad.close()
    with pytest.raises(ValueError):
        eng.attach_stats(object())
    with pytest.raises(_capi.SsdError, match="attached"):
        stats.close()                                             # not while the engine holds it
    # steps before any reset are not counted; a never-reset env is ignored
    eng.rollout_actions(acts, 3)
    assert eng.status() == _capi.SSD_ST_NOT_RESET
    assert not stats.drain()["counts"].any()
    eng.reset()
    eng.rollout_actions(acts, L + 2, auto_reset=True)            # one episode, and two steps of the next
    kept = stats.drain(keep=True)
    assert kept["counts"].tolist() == [[1, 0, L]] * E
    assert_drains_equal(stats.drain(keep=True), kept, "keep does not clear")
    last = stats.last_episode()
    assert np.array_equal(last["len"], kept["last_len"]) and np.array_equal(last["Utility"], kept["last_metrics"][:, 2])
    assert_drains_equal(stats.drain(), kept, "the clearing drain")
    cleared = stats.drain(keep=True)
    assert not cleared["counts"].any() and not cleared["last_len"].any() and np.isinf(cleared["metric_min"]).all()
    # discard drops the open episodes of the masked envs: truncated, and closed until their next reset
    first = np.arange(E) < 100
    stats.discard(first)
    eng.rollout_actions(acts, L - 2, step0=L + 2, auto_reset=True)   # every env's second episode ends here
    d = stats.drain()
    assert d["counts"][first].tolist() == [[0, 1, 0]] * 100 and d["counts"][~first].tolist() == [[1, 0, L]] * (E - 100)
    assert np.array_equal(d["last_reward"][~first].view(np.int64), want["last_reward"][~first].view(np.int64))
    # ... the auto-reset reopened all of them; detached, nothing is counted, and the rings go on
    eng.attach_stats(None)
    out = rings(E, 5)
    eng.rollout_actions(acts, 5, *out, step0=2 * L, auto_reset=True)
    assert bool(out[1].any()), "the engine still steps"
    assert not stats.drain()["counts"].any()
    stats.close()                                                 # free now that the engine let go of it
    close(eng, None)
