"""The four policy forwards called straight through the C ABI (include/ssd.h: ssd_policy_forward, ssd_policy_lstm_forward,
ssd_policy_moa_forward, ssd_ws_policy_forward) with policy.packed() and torch device tensors on the current stream -- no engine,
so every A in 1..15 and every N the header allows is reachable, not only a game's.

Every output buffer is allocated with TAIL_ROWS extra batch rows behind the [B, ...] part, and the whole allocation -- body and
tail -- is filled with the bit pattern SENTINEL (a NaN) before the call.  After the call and a synchronise the tail must still
hold it: a forward writes nothing past row B.  (That is a read of the test's own memory.)  The body's fill shows what a call
left unwritten.  An in-place call (state_out == state_in) has the one state buffer, with the same tail."""
import ctypes as C

import numpy as np
import torch

from sequential_social_dilemma_games_amd import _capi

TAIL_ROWS = 64
SENTINEL = 0x7FC5A3E1               # as float32 a quiet NaN with a payload no arithmetic produces; as int32 positive


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


class Tailed:
    """A float32 device buffer of (B + TAIL_ROWS) rows of `row` floats each, all SENTINEL; .view is the [B, *shape] part."""

    def __init__(self, name, B, shape, dev, init=None):
        self.name, self.B = name, int(B)
        self.row = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        self.full = torch.empty((self.B + TAIL_ROWS) * self.row, dtype=torch.float32, device=dev)
        self.full.view(torch.int32).fill_(SENTINEL)
        self.view = self.full[: self.B * self.row].view((self.B,) + tuple(shape))
        if init is not None:
            self.view.copy_(init)

    def check_tail(self):
        tail = self.full[self.B * self.row:].view(torch.int32)
        touched = int((tail != SENTINEL).sum().item())
        assert touched == 0, "%s: %d floats written past row B = %d" % (self.name, touched, self.B)


def unwritten(t):
    """bool, t's shape: where a buffer of this module still holds the fill."""
    return t.contiguous().view(torch.int32) == SENTINEL


def _finish(bufs):
    torch.cuda.synchronize()
    for b in bufs:
        if b is not None:
            b.check_tail()


def _u8(starts):
    return None if starts is None else starts.to(torch.uint8).contiguous()


def conv_fc(policy, obs, logits=True, value=True, weights=None, num_sets=None):
    """ssd_policy_forward: obs u8 [B, N, 15, 15, 3] -> (logits [B, N, A] or None, value [B, N] or None).  weights / num_sets:
    a packed buffer and set count to use instead of the policy's own."""
    B, N = int(obs.shape[0]), int(obs.shape[1])
    A, dev = policy.num_actions, obs.device
    w = policy.packed() if weights is None else weights
    P = policy.num_sets if num_sets is None else num_sets
    lg = Tailed("logits", B, (N, A), dev) if logits else None
    v = Tailed("value", B, (N,), dev) if value else None
    obs = obs.contiguous()
    _capi.policy_check(_capi.lib().ssd_policy_forward(_ptr(w), P, A, _ptr(obs), B, N, _ptr(lg and lg.full), _ptr(v and v.full),
                                                      _index(dev), 0, _stream(dev)))
    _finish((lg, v))
    return (lg.view if lg else None), (v.view if v else None)


def lstm(policy, obs, state, starts=None, in_place=False):
    """ssd_policy_lstm_forward: obs u8 [B, N, 15, 15, 3], state [B, N, 2, C], starts [B, N] or None -> (logits [B, N, A], value
    [B, N], new state [B, N, 2, C], features [B, N, 32]).  in_place: state_out is state_in (a tailed copy of `state`)."""
    B, N = int(obs.shape[0]), int(obs.shape[1])
    A, Cs, dev = policy.num_actions, policy.cell_size, obs.device
    lg, v = Tailed("logits", B, (N, A), dev), Tailed("value", B, (N,), dev)
    feat = Tailed("features", B, (N, 32), dev)
    if in_place:
        s_out = s_in = Tailed("state (in place)", B, (N, 2, Cs), dev, init=state)
        p_in = s_in.full
    else:
        s_out, p_in = Tailed("state_out", B, (N, 2, Cs), dev), state.contiguous()
    st, obs = _u8(starts), obs.contiguous()
    _capi.policy_check(_capi.lib().ssd_policy_lstm_forward(_ptr(policy.packed()), policy.num_sets, A, Cs, _ptr(obs), _ptr(p_in), _ptr(st),
                                                           B, N, _ptr(feat.full), _ptr(s_out.full), _ptr(lg.full), _ptr(v.full),
                                                           _index(dev), 0, _stream(dev)))
    _finish((lg, v, feat, s_out))
    return lg.view, v.view, s_out.view, feat.view


def moa(policy, obs, prev_actions, state, starts=None, actions=None, clip=10.0, in_place=False):
    """ssd_policy_moa_forward: obs u8 [B, N, 15, 15, 3], prev_actions i32 [B, N], state [B, N, 4, C], starts [B, N] or None,
    actions i32 [B, N] or None -> dict(logits, value, moa_logits, cf_logits, state, influence (None without actions))."""
    B, N = int(obs.shape[0]), int(obs.shape[1])
    A, Cs, dev = policy.num_actions, policy.cell_size, obs.device
    lg, v = Tailed("logits", B, (N, A), dev), Tailed("value", B, (N,), dev)
    moa_lg, cf = Tailed("moa_logits", B, (N, N - 1, A), dev), Tailed("cf_logits", B, (N, A, N - 1, A), dev)
    scratch = Tailed("scratch", B, (_capi.SSD_MOA_SCRATCH_FLOATS(N),), dev)
    infl = Tailed("influence", B, (N,), dev) if actions is not None else None
    if in_place:
        s_out = s_in = Tailed("state (in place)", B, (N, 4, Cs), dev, init=state)
        p_in = s_in.full
    else:
        s_out, p_in = Tailed("state_out", B, (N, 4, Cs), dev), state.contiguous()
    st, obs, prev = _u8(starts), obs.contiguous(), prev_actions.to(torch.int32).contiguous()
    acts = None if actions is None else actions.to(torch.int32).contiguous()
    _capi.policy_check(_capi.lib().ssd_policy_moa_forward(
        _ptr(policy.packed()), policy.num_sets, A, Cs, _ptr(obs), _ptr(prev), _ptr(p_in), _ptr(st), B, N, _ptr(scratch.full),
        _ptr(s_out.full), _ptr(lg.full), _ptr(v.full), _ptr(moa_lg.full), _ptr(cf.full), _ptr(acts), _ptr(infl and infl.full),
        float(clip), _index(dev), 0, _stream(dev)))
    _finish((lg, v, moa_lg, cf, scratch, infl, s_out))
    return {"logits": lg.view, "value": v.view, "moa_logits": moa_lg.view, "cf_logits": cf.view, "state": s_out.view,
            "influence": infl.view if infl else None}


def watershed(policy, obs, agent, state, starts=None, in_place=False):
    """ssd_ws_policy_forward: obs f32 [B, 12], agent i8 [B], state [B, 2, C], starts [B] or None -> (dist [B, 5], value [B], new
    state [B, 2, C]).  Out of place, a state_out row the call does not write still holds the fill (unwritten())."""
    B = int(obs.shape[0])
    Cs, dev = policy.cell_size, obs.device
    dist, v = Tailed("dist", B, (5,), dev), Tailed("value", B, (), dev)
    if in_place:
        s_out = s_in = Tailed("state (in place)", B, (2, Cs), dev, init=state)
        p_in = s_in.full
    else:
        s_out, p_in = Tailed("state_out", B, (2, Cs), dev), state.contiguous()
    st, obs, ag = _u8(starts), obs.to(torch.float32).contiguous(), agent.to(torch.int8).contiguous()
    _capi.policy_check(_capi.lib().ssd_ws_policy_forward(_ptr(policy.packed()), policy.num_sets, Cs, policy.variant, _ptr(obs), _ptr(ag),
                                                         _ptr(p_in), _ptr(st), B, _ptr(s_out.full), _ptr(dist.full), _ptr(v.full),
                                                         _index(dev), 0, _stream(dev)))
    _finish((dist, v, s_out))
    return dist.view, v.view, s_out.view
