"""ssd_ws_policy_forward_seq / evaluate_sequences on the MI355X (csrc/ssd_ws_policy_seq.hip): one launch for all M own steps and
the bootstrap, bit-equal to ssd_ws_policy_forward chained step by step under the same state rule (every starts mode, the three
cell sizes, the persistent loop's second tile, the bootstrap with and without start_next); a fresh sample()'s rows given back
to the bit under unchanged weights; NULL outputs honoured; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from sequential_social_dilemma_games_amd import WatershedVecEngine, _capi, evaluate_sequences
from ws_a3c_ref import SEQ, SEQ_COMM, STARTS_MODES, as_numpy_u32, gather_own_steps, make_policy, make_starts

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_ENGINES = {}


def _engine(variant):
    """One small engine per variant, for policy_forward (the forward call does not touch the envs)."""
    if variant not in _ENGINES:
        _ENGINES[variant] = WatershedVecEngine(variant, 1, seed=0)
    return _ENGINES[variant]


def _inputs(pol, agent, M, Q, T, seed, starts_mode, start_next=True):
    g = torch.Generator().manual_seed(seed)
    comm = pol.variant == SEQ_COMM and agent < 4
    t = {"obs": torch.rand((M, Q, 12), generator=g), "state": 0.5 * torch.randn((-(-M // T), Q, 2, pol.cell_size), generator=g),
         "actions": torch.randint(-1, 7, (M, Q), generator=g).float() if comm else torch.randn((M, Q), generator=g),
         "obs_next": torch.rand((Q, 12), generator=g)}
    starts = make_starts(starts_mode, M, Q, T, g)
    if starts is not None:
        t["starts"] = starts
    if start_next:
        t["start_next"] = (torch.rand((Q,), generator=g) < 0.4).to(torch.uint8)
    return {k: v.to(DEV).contiguous() for k, v in t.items()}


def _chained(pol, agent, t, T):
    """M + 1 launches of ssd_ws_policy_forward under the state rule -> (dist, value, bootstrap, the state after step M - 1)."""
    eng = _engine(pol.variant)
    M, Q = t["actions"].shape
    ag = torch.full((Q,), agent, dtype=torch.int8, device=DEV)
    dists, values, st = [], [], None
    for m in range(M):
        if m % T == 0:
            st, s = t["state"][m // T].contiguous(), None
        else:
            s = t["starts"][m] if "starts" in t else None
        d, v, st = eng.policy_forward(pol, t["obs"][m].contiguous(), ag, st, s)
        dists.append(d)
        values.append(v)
    boot = eng.policy_forward(pol, t["obs_next"], ag, st, t.get("start_next"))[1]
    return torch.stack(dists), torch.stack(values), boot, st


def _raw(pol, agent, t, T, outs, **over):
    """The entry point itself; outs: dict of output tensors or None by name.  -> rc."""
    M, Q = t["actions"].shape
    ptr = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())   # noqa: E731
    a = dict(weights=pol.packed(), num_sets=pol.num_sets, cell_size=pol.cell_size, variant=pol.variant, agent_id=agent, seq_len=T,
             obs=t["obs"], state=t["state"], starts=t.get("starts"), actions=t.get("actions"), obs_next=t.get("obs_next"),
             start_next=t.get("start_next"), n_steps=M, num_seqs=Q, flags=0)
    a.update(outs)
    a.update(over)
    rc = _capi.lib().ssd_ws_policy_forward_seq(
        ptr(a["weights"]), a["num_sets"], a["cell_size"], a["variant"], a["agent_id"], a["seq_len"], ptr(a["obs"]), ptr(a["state"]),
        ptr(a["starts"]), ptr(a["actions"]), ptr(a["obs_next"]), ptr(a["start_next"]), a["n_steps"], a["num_seqs"], ptr(a["dist"]),
        ptr(a["value"]), ptr(a["logp"]), ptr(a["bootstrap_value"]), ptr(a["state_out"]), 0, a["flags"],
        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc


def _outs(M, Q, Cs, fill=float("nan")):
    f = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=DEV)   # noqa: E731
    return dict(dist=f(M, Q, 5), value=f(M, Q), logp=f(M, Q), bootstrap_value=f(Q), state_out=f(Q, 2, Cs))


def _same(a, b, what):
    assert np.array_equal(as_numpy_u32(a), as_numpy_u32(b)), what


def _logp_f32(dist, actions, comm):
    """The contract's float32 expression restated on the device's own dist, in float64 (a tolerance check of logp; the bit
    check is the fresh sample's)."""
    d = dist.double()
    if comm:
        a = actions.long().clamp(0, 4).unsqueeze(-1)
        return torch.log_softmax(d, -1).gather(-1, a).squeeze(-1)
    z = (actions.double() - d[..., 0]) / d[..., 1].exp()
    return -0.5 * z * z - d[..., 1] - float(np.float32(0.9189385))


@pytest.mark.parametrize("Cs", [64, 128, 256])
@pytest.mark.parametrize("starts_mode", STARTS_MODES)
def test_one_launch_equals_the_chained_forward(Cs, starts_mode):
    """M = 7, T = 3, Q = 17: a short last window, a tile and a one-row tail; a comm id and an action id."""
    M, T, Q = 7, 3, 17
    pol = make_policy(SEQ_COMM, Cs, seed=3).to(DEV)
    for agent in (1, 5):
        t = _inputs(pol, agent, M, Q, T, seed=10 * Cs + agent, starts_mode=starts_mode)
        want = _chained(pol, agent, t, T)
        outs = _outs(M, Q, Cs)
        assert _raw(pol, agent, t, T, outs) == _capi.SSD_OK
        for name, w in zip(("dist", "value", "bootstrap_value", "state_out"), want):
            _same(outs[name], w, (agent, name))
        assert bool(torch.isfinite(outs["logp"]).all())
        ref = _logp_f32(outs["dist"], t["actions"], agent < 4)
        err = float(((outs["logp"].double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
        # (float32's 1.2e-7 some thirty times over: a handful of roundings at the logits' magnitude, below 16 here, against a
        # logp that may be near 0; the Gaussian's z^2 doubles z's relative error)
        assert err <= 4e-6, (agent, err)
        # and through the Python call
        dist, value, logp, boot = evaluate_sequences(pol, agent, t, T)
        torch.cuda.synchronize()
        for got, name in ((dist, "dist"), (value, "value"), (logp, "logp"), (boot, "bootstrap_value")):
            _same(got, outs[name], (agent, name, "python"))


def test_bootstrap_without_start_next_and_with_a_window_boundary():
    """M = 6, T = 3: the bootstrap row sits where a window would start, and still takes the carried state (state has no entry
    for it); without start_next no row starts."""
    M, T, Q = 6, 3, 17
    pol = make_policy(SEQ, 64, seed=4).to(DEV)
    t = _inputs(pol, 2, M, Q, T, seed=21, starts_mode="per_seq", start_next=False)
    want = _chained(pol, 2, t, T)
    outs = _outs(M, Q, 64)
    assert _raw(pol, 2, t, T, outs) == _capi.SSD_OK
    for name, w in zip(("dist", "value", "bootstrap_value", "state_out"), want):
        _same(outs[name], w, name)
    every = dict(t, start_next=torch.ones((Q,), dtype=torch.uint8, device=DEV))
    outs2 = _outs(M, Q, 64)
    assert _raw(pol, 2, every, T, outs2) == _capi.SSD_OK
    _same(outs2["bootstrap_value"], _chained(pol, 2, every, T)[2], "all start")
    assert not torch.equal(outs2["bootstrap_value"], outs["bootstrap_value"])
    _same(outs2["state_out"], outs["state_out"], "the bootstrap step leaves state_out alone")


def test_persistent_loop_takes_a_second_tile():
    """Q = 16 * 1024 + 5, M = 2, C = 64: 1025 tiles for 1024 workgroups; workgroup 0's second tile has five live rows."""
    G = _capi.SSD_WSPPO_GROUPS(10 ** 6)
    M, T, Q = 2, 2, 16 * G + 5
    assert _capi.SSD_WSPPO_GROUPS(Q) == G == 1024
    pol = make_policy(SEQ_COMM, 64, seed=5).to(DEV)
    t = _inputs(pol, 5, M, Q, T, seed=31, starts_mode="per_seq")
    want = _chained(pol, 5, t, T)
    outs = _outs(M, Q, 64)
    assert _raw(pol, 5, t, T, outs) == _capi.SSD_OK
    for name, w in zip(("dist", "value", "bootstrap_value", "state_out"), want):
        _same(outs[name], w, name)
    assert bool(torch.isfinite(outs["logp"]).all())


@pytest.mark.parametrize("agent", [1, 5])
def test_a_fresh_sample_is_given_back_to_the_bit(agent):
    """sample(policy, 131) of 32 SeqComm envs, unchanged weights: the id's own rows but the last evaluate to the recorded dist,
    value and logp, and the bootstrap of the last own step's observation to its recorded value: rhos == 1 exactly."""
    E, T = 32, 4
    eng = WatershedVecEngine(SEQ_COMM, E, seed=7)
    pol = make_policy(SEQ_COMM, 64, seed=6).to(DEV)
    first = eng.reset()[0].clone()
    batch = eng.sample(pol, 131)
    seq, ks = gather_own_steps(batch, first, agent, T)
    M = len(ks) - 1
    assert M >= 8
    t = {k: seq[k][:M].contiguous() for k in ("obs", "actions", "starts")}
    t["state"] = seq["state"][:-(-M // T)].contiguous()
    t["obs_next"], t["start_next"] = seq["obs"][M].contiguous(), seq["starts"][M].contiguous()
    dist, value, logp, boot = evaluate_sequences(pol, agent, t, T)
    torch.cuda.synchronize()
    _same(dist, seq["dist"][:M], "dist")
    _same(value, seq["value"][:M], "value")
    _same(logp, seq["logp"][:M], "logp")
    _same(boot, seq["value"][M], "bootstrap")
    rhos = torch.exp(logp - seq["logp"][:M])
    assert torch.equal(rhos, torch.ones_like(rhos))


def test_null_outputs_are_honoured():
    M, T, Q = 5, 2, 17
    pol = make_policy(SEQ_COMM, 64, seed=8).to(DEV)
    t = _inputs(pol, 5, M, Q, T, seed=41, starts_mode="mid")
    full = _outs(M, Q, 64)
    assert _raw(pol, 5, t, T, full) == _capi.SSD_OK
    for keep in ("dist", "value", "logp", "bootstrap_value", "state_out"):
        outs = {k: None for k in full}
        outs[keep] = torch.full_like(full[keep], float("nan"))
        canary = torch.full((64,), 7.0, dtype=torch.float32, device=DEV)     # allocated next: a stray store would likely land here
        assert _raw(pol, 5, t, T, outs) == _capi.SSD_OK, keep
        _same(outs[keep], full[keep], keep)
        assert float((canary - 7.0).abs().max()) == 0.0
    # neither actions nor obs_next are needed for dist and value alone
    outs = dict(dist=torch.full_like(full["dist"], float("nan")), value=None, logp=None, bootstrap_value=None, state_out=None)
    bare = {k: v for k, v in t.items() if k not in ("obs_next", "start_next")}
    assert _raw(pol, 5, bare, T, outs, actions=None) == _capi.SSD_OK
    _same(outs["dist"], full["dist"], "dist alone")


def test_refusals():
    """Every SSD_E_INVALID case of the contract: refused before the launch (the outputs keep what they held) with a reason."""
    M, T, Q = 4, 2, 5
    pol = make_policy(SEQ_COMM, 64, seed=9).to(DEV)
    t = _inputs(pol, 5, M, Q, T, seed=51, starts_mode="none")
    bad = [(dict(agent_id=8), b"agent_id"), (dict(agent_id=-1), b"agent_id"), (dict(cell_size=96), b"cell_size"),
           (dict(seq_len=0), b"seq_len"), (dict(n_steps=0), b"n_steps"), (dict(num_seqs=0), b"num_seqs"),
           (dict(weights=None), b"weights"), (dict(obs=None), b"obs and state are required"),
           (dict(state=None), b"obs and state are required"), (dict(actions=None), b"logp needs actions"),
           (dict(obs_next=None), b"bootstrap_value needs obs_next"), (dict(variant=7), b"variant"), (dict(num_sets=4), b"num_sets"),
           (dict(flags=1), b"flags"), (dict(obs=t["obs"].data_ptr() + 2), b"aligned"), (dict(n_steps=2 ** 30, num_seqs=4), b"rows")]
    for over, words in bad:
        outs = _outs(M, Q, 64)
        rc = _raw(pol, 5, t, T, outs, **over)
        msg = _capi.lib().ssd_policy_last_error()
        assert rc == _capi.SSD_E_INVALID and words in msg, (over, msg)
        assert all(bool(torch.isnan(v).all()) for v in outs.values()), over      # nothing was launched
    seq_pol = make_policy(SEQ, 64, seed=9).to(DEV)
    assert _raw(seq_pol, 4, t, T, _outs(M, Q, 64)) == _capi.SSD_E_INVALID          # id 4 is outside Seq's 0 .. 3
    outs = _outs(M, Q, 64)
    assert _raw(pol, 5, t, T, outs) == _capi.SSD_OK and all(bool(torch.isfinite(v).all()) for v in outs.values())
