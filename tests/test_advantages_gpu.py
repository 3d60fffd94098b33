"""Advantages and value targets on the device (csrc/ssd_gae.hip): the kernel against the tests'
restatement (gae_ref.py) bit for bit -- the synthetic matrix of the CPU suite, every kernel instance at every count of full
blocks of 16 steps (gae_ref.block_matrix()), the full-size shapes, out= and a stream of the caller's -- and
SSDVectorEnv.sample(..., gamma=...) end to end for the three Harvest / Cleanup policies."""
import numpy as np
import pytest
import torch

import gae_ref
from gae_ref import advantages_ref, make_rings, same_bits
from sequential_social_dilemma_games_amd import ConvFCPolicy, ConvLSTMPolicy, ConvMOAPolicy
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd.postprocessing import compute_advantages
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = gae_ref.matrix()
BLOCK_CASES = gae_ref.block_matrix()


def _dev(c):
    return {k: None if v is None else torch.from_numpy(v).to(DEV) for k, v in c.items()}


def _check(c, call, **extra):
    t = _dev(c)
    adv, vt = compute_advantages(t["rew"], t["value"], t["last_value"], t["done"], bonus=t["bonus"], **call, **extra)
    want_a, want_t = advantages_ref(c["rew"], c["value"], c["last_value"], c["done"], bonus=c["bonus"], **call)
    adv, vt = adv.cpu().numpy(), vt.cpu().numpy()
    assert same_bits(adv, want_a), np.argwhere(gae_ref.bits(adv) != gae_ref.bits(want_a))[:5]
    assert same_bits(vt, want_t), np.argwhere(gae_ref.bits(vt) != gae_ref.bits(want_t))[:5]
    return adv, vt


@pytest.mark.parametrize("name,rings,call", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_restatement(name, rings, call):
    _check(make_rings(**rings), call)


@pytest.mark.parametrize("name,rings,call", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_blocks_buffers_and_waves(name, rings, call):
    """Every kernel instance at no, one, two and three full blocks of 16 steps, each alone, one step short and one over; whole
    and partial last waves; test_advantages_cpu.py asserts what the cases cover."""
    _check(gae_ref.build(rings, call), call)


@pytest.mark.parametrize("mode", sorted(gae_ref.MODES))
def test_full_size(mode):
    """4096 envs x 5 agents, 1000 steps.  The restatement runs on 1500 of the lanes (scipy per lane and segment); every lane is
    checked against the package's host path, which the CPU suite pins to the restatement."""
    c = make_rings(seed=11, R=1000, trailing=(4096, 5), done_mode="some", with_bonus=True)
    call = dict(gamma=0.99, lambda_=0.95, bonus_weight=0.25, **gae_ref.MODES[mode])
    t = _dev(c)
    adv, vt = compute_advantages(t["rew"], t["value"], t["last_value"], t["done"], bonus=t["bonus"], **call)
    adv, vt = adv.cpu().numpy(), vt.cpu().numpy()
    h = {k: None if v is None else torch.from_numpy(v) for k, v in c.items()}
    host_a, host_t = compute_advantages(h["rew"], h["value"], h["last_value"], h["done"], bonus=h["bonus"], **call)
    assert same_bits(adv, host_a.numpy()) and same_bits(vt, host_t.numpy())
    e = slice(0, 4096, 14)                                       # 293 envs x 5 agents, the first and last waves among them
    sub = {k: None if v is None else np.ascontiguousarray(v[e] if k == "last_value" else v[:, e]) for k, v in c.items()}
    want_a, want_t = advantages_ref(sub["rew"], sub["value"], sub["last_value"], sub["done"], bonus=sub["bonus"], **call)
    assert same_bits(adv[:, e], want_a) and same_bits(vt[:, e], want_t)


@pytest.mark.parametrize("mode", sorted(gae_ref.MODES))
def test_one_lane(mode):
    c = make_rings(seed=12, R=1000, trailing=(1,), done_mode="some", with_bonus=True)
    _check(c, dict(gamma=0.99, lambda_=0.95, bonus_weight=0.25, **gae_ref.MODES[mode]))
    c = make_rings(seed=13, R=33, trailing=(), done_mode="none")                  # [R]: no trailing shape at all
    _check(c, dict(gamma=0.5, lambda_=1.0, **gae_ref.MODES[mode]))


def test_out_and_a_stream_of_the_callers():
    c = make_rings(seed=14, R=130, trailing=(9, 5), done_mode="some")
    call = dict(gamma=0.99, lambda_=0.95, step0=100, n_steps=90)
    out = (torch.full((130, 9, 5), 9.0, device=DEV), torch.full((130, 9, 5), 8.0, device=DEV))
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        t = _dev(c)
        adv, vt = compute_advantages(t["rew"], t["value"], t["last_value"], t["done"], out=out, **call)
    s.synchronize()
    assert adv is out[0] and vt is out[1]
    want_a, want_t = advantages_ref(c["rew"], c["value"], c["last_value"], c["done"], **call)
    rows = [(100 + k) % 130 for k in range(90)]
    rest = [r for r in range(130) if r not in rows]
    adv, vt = adv.cpu().numpy(), vt.cpu().numpy()
    assert same_bits(adv[rows], want_a[rows]) and same_bits(vt[rows], want_t[rows])
    assert np.all(adv[rest] == 9.0) and np.all(vt[rest] == 8.0)  # rows outside the call are left alone


def test_device_argument_checks():
    t = _dev(make_rings(seed=15, R=4, trailing=(3,), done_mode="some"))
    with pytest.raises(ValueError):
        compute_advantages(t["rew"], t["value"].cpu(), t["last_value"], t["done"])
    with pytest.raises(ValueError):
        compute_advantages(t["rew"], t["value"], t["last_value"], t["done"], out=(torch.empty(4, 3), torch.empty(4, 3)))


# ---------------------------------------------------------------------------------------------------- the adapter
E, N, HORIZON, STEPS = 16, 5, 12, 8


def _policy(kind):
    if kind == "fc":
        return ConvFCPolicy(8, N, seed=3).to(DEV)
    if kind == "lstm":
        return ConvLSTMPolicy(8, 1, 64, seed=4).to(DEV)
    return ConvMOAPolicy(8, N, 1, 64, seed=5).to(DEV)


def _adapter(pol, seed):
    """An adapter five steps into its episodes, except envs 0..3, which have just been reset: in the next 8 steps the others
    reach the horizon (12) and these do not."""
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=HORIZON, seed=seed)
    env.reset()
    env.sample(pol, 5)
    for e in range(4):
        env.try_reset(e)
    return env


@pytest.mark.parametrize("use_gae", [True, False])
@pytest.mark.parametrize("kind", ["fc", "lstm", "moa"])
def test_sample_with_gamma_equals_the_restatement(kind, use_gae):
    pol = _policy(kind)
    kw = dict(influence_weight=0.25) if kind == "moa" else {}
    plain = _adapter(pol, 31).sample(pol, STEPS, **kw)
    batch = _adapter(pol, 31).sample(pol, STEPS, gamma=0.99, lambda_=0.95, use_gae=use_gae, **kw)
    # the feature does not disturb the rollout: today's keys without gamma, and the same tensors with it
    want_keys = {"obs", "actions", "logp", "value", "rew", "done", "last_value"}
    want_keys |= {"fc": set(), "lstm": {"state_in"}, "moa": {"state_in", "influence", "prev_actions", "rewards"}}[kind]
    assert set(plain) == want_keys and set(batch) == want_keys | {"advantages", "value_targets"}
    for k in plain:
        assert torch.equal(plain[k], batch[k]), k
    h = {k: v.cpu().numpy() for k, v in batch.items()}
    assert h["advantages"].shape == (STEPS, E, N) and h["advantages"].dtype == np.float32
    ended = h["done"].any(axis=0)
    assert ended.any() and not ended.all()                       # both branches: lanes with an episode end, lanes without
    assert h["done"][:STEPS - 1].any()                           # ... an end inside the fragment, not only in its last row
    bonus = dict(bonus=h["influence"], bonus_weight=0.25) if kind == "moa" else {}
    want_a, want_t = advantages_ref(h["rew"], h["value"], h["last_value"], h["done"], gamma=0.99, lambda_=0.95, use_gae=use_gae,
                                    **bonus)
    assert same_bits(h["advantages"], want_a) and same_bits(h["value_targets"], want_t)
    if kind == "moa" and h["influence"].any():                   # (the bonus counts: the plain rewards give other advantages)
        no_a, _ = advantages_ref(h["rew"], h["value"], h["last_value"], h["done"], gamma=0.99, lambda_=0.95, use_gae=use_gae)
        assert not same_bits(h["advantages"], no_a)


def test_sample_without_a_critic_and_its_checks():
    pol = _policy("fc")
    env = _adapter(pol, 32)
    b = env.sample(pol, STEPS, gamma=0.9, use_gae=False, use_critic=False)
    h = {k: v.cpu().numpy() for k, v in b.items()}
    want_a, want_t = advantages_ref(h["rew"], None, h["last_value"], h["done"], gamma=0.9, use_gae=False, use_critic=False)
    assert same_bits(h["advantages"], want_a) and same_bits(h["value_targets"], want_t) and not h["value_targets"].any()
    for bad in (dict(gamma=float("nan")), dict(gamma=0.9, lambda_=float("inf")), dict(gamma=0.9, use_critic=False)):
        with pytest.raises(ValueError):
            env.sample(pol, STEPS, **bad)
