"""The conv-FC policy network of the reference (models/conv_to_fc_net.py:1-51, ConvToFCNet: the model of Jaques et al. 2019)
as a torch module whose weights the device kernels read (include/ssd.h, SSD_POL_*; csrc/ssd_policy.hip), ConvLSTMPolicy, the
same trunk under RLlib's LSTM (SSD_LSTM_*; csrc/ssd_policy_lstm.hip), and ConvMOAPolicy, the causal-influence policy of
train_moa.py with its social-influence reward, influence() (SSD_MOA_*; csrc/ssd_policy_moa.hip).  WatershedLSTMPolicy, at the
end of the file, is the LSTM-FC network of the Watershed launchers (SSD_WSP_*; csrc/ssd_ws_policy.hip).  All four are built on
PolicyBase (parameters from layout(), load_arrays(), packed(), initial_state(), and what an engine asks of a policy) and on
the forward pieces that follow it.

    policy = ConvFCPolicy(num_actions=8, num_sets=5).cuda()       # one weight set per agent, as train_baseline.py:87-96
    logits, value = policy(obs_u8)                                # [..., N, 15, 15, 3] -> [..., N, A], [..., N]
    eng.rollout_policy(policy, obs0, 100, obs_ring, ...)          # the same network, on the device, in the loop

Per weight set: conv 3x3 (6 filters, stride 1, no padding) + ReLU, flatten in (row, col, channel) order -- TF's flatten of
NHWC --, fc1 1014 -> 32 + ReLU, fc2 32 -> 32 + ReLU, logits 32 -> A, and a value head 32 -> 1 on the same trunk (RLlib's
value_function() of a v1 Model).  The parameters are stored in TF's layouts (conv kernel [kh, kw, c_in, c_out], dense kernels
[in, out]) with a leading weight-set axis, so they map one to one onto a TF checkpoint's and onto the packed layout.
"""
import collections

import numpy as np
import torch

from . import _capi
from .vector_env import _NORMALISE

VIEW = _capi.SSD_POL_VIEW
FLAT = _capi.SSD_POL_FLAT
HIDDEN = _capi.SSD_POL_HIDDEN
FILTERS = _capi.SSD_POL_FILTERS

# (name, shape of one set, float offset in a packed set); logits_w / logits_b depend on A and are added per instance
_FIXED = (("conv_w", (3, 3, 3, FILTERS), _capi.SSD_POL_CONV_W), ("conv_b", (FILTERS,), _capi.SSD_POL_CONV_B),
          ("fc1_w", (FLAT, HIDDEN), _capi.SSD_POL_FC1_W), ("fc1_b", (HIDDEN,), _capi.SSD_POL_FC1_B),
          ("fc2_w", (HIDDEN, HIDDEN), _capi.SSD_POL_FC2_W), ("fc2_b", (HIDDEN,), _capi.SSD_POL_FC2_B),
          ("value_w", (HIDDEN, 1), _capi.SSD_POL_VALUE_W), ("value_b", (1,), _capi.SSD_POL_VALUE_B))


def normc(shape, std, generator):
    """RLlib's normc_initializer(std) for a [..., in, out] kernel: every column (output unit) has norm std."""
    out = torch.randn(shape, generator=generator, dtype=torch.float64)
    return out * (std / out.square().sum(dim=-2, keepdim=True).sqrt())


def _glorot(shape, fan_in, fan_out, generator):
    """Glorot uniform: the default kernel initializer of slim.conv2d, of TF's LSTMCell and of Keras' layers."""
    limit = float(np.sqrt(6.0 / (fan_in + fan_out)))
    return (torch.rand(shape, generator=generator, dtype=torch.float64) * 2 - 1) * limit


def _orthogonal(P, rows, cols, generator):
    """Keras' Orthogonal initializer for [rows, cols] kernels (rows <= cols), one per weight set."""
    out = torch.empty((P, rows, cols), dtype=torch.float64)
    for p in range(P):
        q, r = torch.linalg.qr(torch.randn((cols, rows), generator=generator, dtype=torch.float64))
        out[p] = (q * torch.sign(torch.diagonal(r))).T
    return out


class PolicyBase(torch.nn.Module):
    """What the four policy modules share.  A subclass sets num_sets (and cell_size, if it has a state), defines layout() and
    set_floats, and registers its parameters with _register().  The class attributes are what an engine asks of a policy to
    run it on the device."""
    STATE_ROWS = 0                  # a state is [..., STATE_ROWS, cell_size]; 0: the policy has none
    TAKES_PREV_ACTIONS = False      # the network reads the previous joint action (and gives the influence reward)
    REF_PARAM = "conv_w"            # the parameter whose dtype and device stand for the module's
    C_FORWARD = C_ROLLOUT = None    # the library's forward and rollout entry points of this network (include/ssd.h)

    @staticmethod
    def _check_ranges(num_actions=None, num_sets=None, cell_size=None):
        if num_actions is not None and not 1 <= num_actions <= _capi.SSD_POL_MAX_ACTIONS:
            raise ValueError("num_actions must be 1..%d" % _capi.SSD_POL_MAX_ACTIONS)
        if num_sets is not None and not 1 <= num_sets <= 64:
            raise ValueError("num_sets must be 1..64")
        if cell_size is not None and cell_size not in _capi.LSTM_CELL_SIZES:
            raise ValueError("cell_size must be one of %s" % (_capi.LSTM_CELL_SIZES,))

    def _register(self, init):
        """Registers every parameter of layout(), in its order, from init {name: float64 [entries, *shape of one set]}; one
        that init does not name (a bias) starts at zero."""
        for name, shape, _ in self.layout():
            t = init.get(name)
            if t is None:
                t = torch.zeros((self._entries(name),) + shape, dtype=torch.float64)
            self.register_parameter(name, torch.nn.Parameter(t.to(torch.float32)))
        self._packed = None
        self._tables = {}

    def _entries(self, name):
        """The length of parameter `name`'s leading axis: num_sets, or fewer where several sets share one layer."""
        return self.num_sets

    def scratch_shape(self, rows):
        """The float32 scratch the library's calls need for `rows` (env, agent) rows, or None."""
        return None

    def load_arrays(self, weights):
        """Set the parameters from a dict of arrays {name: [P, *shape of one set]} in the layouts above (a TF checkpoint's
        kernels and biases, stacked over the weight sets), cast to the parameters' dtype and device."""
        with torch.no_grad():
            for name, shape, _ in self.layout():
                src = torch.as_tensor(np.asarray(weights[name]))
                dst = getattr(self, name)
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError("%s must have shape %s, got %s" % (name, tuple(dst.shape), tuple(src.shape)))
                dst.copy_(src.to(dst.dtype))
        return self

    def packed(self):
        """All weight sets as ONE contiguous float32 tensor on the parameters' device, in the layout of include/ssd.h: set p
        at p * set_floats.  A parameter with fewer entries than sets is repeated into them (entry k serves sets k, k +
        entries, ...).  Rebuilt from the parameters on every call by device copies on the current stream (no host
        synchronisation), so an optimiser's update takes effect on the next call.  The buffer is reused between calls."""
        P, S = self.num_sets, self.set_floats
        dev = getattr(self, self.REF_PARAM).device
        if self._packed is None or self._packed.device != dev:
            self._packed = torch.zeros(P * S, dtype=torch.float32, device=dev)
        v = self._packed.view(P, S)
        with torch.no_grad():
            for name, shape, off in self.layout():
                n = int(np.prod(shape))
                t = getattr(self, name).reshape(-1, n)
                if t.shape[0] != P:
                    t = t.repeat(P // t.shape[0], 1)
                v[:, off:off + n].copy_(t)
        return self._packed

    def initial_state(self, lead, device=None):
        """A zero state [*lead, STATE_ROWS, C] (the parameters' dtype, on their device unless given)."""
        lead = (int(lead),) if isinstance(lead, int) else tuple(int(n) for n in lead)
        ref = getattr(self, self.REF_PARAM)
        return torch.zeros(lead + (self.STATE_ROWS, self.cell_size), dtype=ref.dtype, device=ref.device if device is None else device)


# ---- the forward pieces the policies share ----

def _dense(h, w, b):
    """Per weight set p: h [M, P, K] @ w [P, K, J] + b [P, J]."""
    return torch.einsum("mpk,pkj->mpj", h, w) + b


def _heads(h, logits_w, logits_b, value_w, value_b):
    """(logits [M, P, A], value [M, P]) on h [M, P, K]."""
    return _dense(h, logits_w, logits_b), _dense(h, value_w, value_b)[..., 0]


def _conv_flat(module, obs, G, conv_w, conv_b):
    """uint8 observations [..., G, 15, 15, 3] (any leading shape of M x G rows) -> the conv layer's output [M, G, 1014]:
    float((u8 - 128) / 255) from a table, the G weight sets conv_w [G, 3, 3, 3, 6] / conv_b [G, 6] as conv groups, ReLU, and
    TF's flatten of NHWC."""
    dt = module.conv_w.dtype
    key = (obs.device, dt)
    if key not in module._tables:                                # float((u8 - 128) / 255), from the float64 values
        module._tables[key] = torch.from_numpy(_NORMALISE).to(dt).to(obs.device)
    x = module._tables[key][obs.long()].reshape(-1, G, VIEW, VIEW, 3)
    M = x.shape[0]
    x = x.permute(0, 1, 4, 2, 3).reshape(M, G * 3, VIEW, VIEW)    # NHWC -> NCHW, the sets as conv groups
    wc = conv_w.permute(0, 4, 3, 1, 2).reshape(G * FILTERS, 3, 3, 3)
    h = torch.relu(torch.nn.functional.conv2d(x, wc, conv_b.reshape(G * FILTERS), groups=G))
    return h.reshape(M, G, FILTERS, 13, 13).permute(0, 1, 3, 4, 2).reshape(M, G, FLAT)   # flatten (row, col, channel)


def _zero_where(starts, t, tail):
    """The start rule: t with the rows where starts (t's shape less its last `tail` axes) is true replaced by zero --
    selected, not multiplied: whatever t holds there is never used."""
    m = starts.to(torch.bool).reshape(t.shape[:t.dim() - tail] + (1,) * tail).to(t.device)
    return torch.where(m, torch.zeros((), dtype=t.dtype, device=t.device), t)


def _unroll(step, T, state, resets):
    """step(t, state, resets[t] or None) -> (outputs..., new state) for t = 0 .. T - 1; returns the outputs stacked over t and
    the final state."""
    rows = []
    for t in range(T):
        *out, state = step(t, state, None if resets is None else resets[t])
        rows.append(out)
    return tuple(torch.stack(col) for col in zip(*rows)) + (state,)


def _trunk(module, obs):
    """The conv-FC trunk shared by both policies: uint8 observations [..., (P,) 15, 15, 3] -> (fc2's output [M, P, 32], the
    leading shape of one row per observation)."""
    P = module.num_sets
    if obs.shape[-3:] != (VIEW, VIEW, 3):
        raise ValueError("observations must end in (15, 15, 3), got %s" % (tuple(obs.shape),))
    if P > 1 and (obs.dim() < 4 or obs.shape[-4] != P):
        raise ValueError("with %d weight sets the observations need an agent axis of %d: [..., %d, 15, 15, 3]" % (P, P, P))
    h = _conv_flat(module, obs, P, module.conv_w, module.conv_b)
    h = torch.relu(_dense(h, module.fc1_w, module.fc1_b))
    return torch.relu(_dense(h, module.fc2_w, module.fc2_b)), obs.shape[:-3]


class ConvFCPolicy(PolicyBase):
    """num_sets P independent weight sets: P = 1 is one policy shared by every agent, P = N one per agent (agent i uses
    set i).  Input: uint8 observations [..., 15, 15, 3] (P = 1) or [..., P, 15, 15, 3], normalised as float((u8 - 128) / 255)
    (the reference observation, map_env.py:199).  Output: (logits [..., A], value [...])."""
    C_FORWARD, C_ROLLOUT = "ssd_policy_forward", "ssd_rollout_policy"

    def __init__(self, num_actions, num_sets=1, seed=0):
        super().__init__()
        A, P = int(num_actions), int(num_sets)
        self._check_ranges(A, P)
        self.num_actions, self.num_sets = A, P
        g = torch.Generator().manual_seed(int(seed))
        self._register({"conv_w": _glorot((P, 3, 3, 3, FILTERS), 27, 9 * FILTERS, g),
                        "fc1_w": normc((P, FLAT, HIDDEN), 1.0, g), "fc2_w": normc((P, HIDDEN, HIDDEN), 1.0, g),
                        "value_w": normc((P, HIDDEN, 1), 1.0, g), "logits_w": normc((P, HIDDEN, A), 0.01, g)})

    def layout(self):
        """(name, shape of one set, float offset within a packed set) of every parameter, in packed order."""
        A = self.num_actions
        return _FIXED + (("logits_w", (HIDDEN, A), _capi.SSD_POL_LOGITS_W), ("logits_b", (A,), _capi.SSD_POL_LOGITS_B(A)))

    @property
    def set_floats(self):
        return _capi.SSD_POL_SET_FLOATS(self.num_actions)

    def ppo_scratch_shape(self, set_rows):
        """The float32 scratch ssd_policy_ppo_grad needs for a fragment with `set_rows` rows per weight set (K E for num_sets =
        N, K E N for num_sets = 1): the workgroups' partial gradient sets and statistics."""
        return (_capi.SSD_PPO_SCRATCH_FLOATS(set_rows, self.num_sets, self.num_actions),)

    def forward(self, obs):
        h, lead = _trunk(self, obs)
        logits, value = _heads(h, self.logits_w, self.logits_b, self.value_w, self.value_b)
        return logits.reshape(lead + (self.num_actions,)), value.reshape(lead)


class ConvLSTMPolicy(PolicyBase):
    """The baseline's recurrent policy (run_scripts/train_baseline.py:146-147, "use_lstm": True): the trunk of ConvFCPolicy
    (conv, fc1, fc2) and RLlib 0.7.6's LSTM of cell_size C cells on fc2's output, with the logits and the value on the LSTM's
    output h' (include/ssd.h, RECURRENT POLICY ROLLOUTS).  The cell is TF's LSTMCell: z = [x, h] @ lstm_w + lstm_b split into
    (i, j, f, o); c' = sigmoid(f + 1) c + sigmoid(i) tanh(j); h' = sigmoid(o) tanh(c').  A state is [..., 2, C] (c, then h).

        policy = ConvLSTMPolicy(8, num_sets=5, cell_size=128).cuda()
        state = policy.initial_state((E, 5))
        logits, value, state = policy(obs_u8, state, starts)            # starts: rows whose episode begins (state zeroed)
        logits, value, final = policy.forward_sequence(obs_seq, state_in, resets)   # the learner's BPTT path

    Parameters in TF's layouts with a leading weight-set axis: the trunk's, lstm_w [P, 32 + C, 4C], lstm_b [P, 4C], logits_w
    [P, C, A], logits_b [P, A], value_w [P, C, 1], value_b [P, 1]."""
    STATE_ROWS = 2
    C_FORWARD, C_ROLLOUT = "ssd_policy_lstm_forward", "ssd_rollout_policy_lstm"

    def __init__(self, num_actions, num_sets=1, cell_size=128, seed=0):
        super().__init__()
        A, P, C = int(num_actions), int(num_sets), int(cell_size)
        self._check_ranges(A, P, C)
        self.num_actions, self.num_sets, self.cell_size = A, P, C
        g = torch.Generator().manual_seed(int(seed))
        self._register({"conv_w": _glorot((P, 3, 3, 3, FILTERS), 27, 9 * FILTERS, g),
                        "fc1_w": normc((P, FLAT, HIDDEN), 1.0, g), "fc2_w": normc((P, HIDDEN, HIDDEN), 1.0, g),
                        "lstm_w": _glorot((P, HIDDEN + C, 4 * C), HIDDEN + C, 4 * C, g),
                        "value_w": normc((P, C, 1), 1.0, g), "logits_w": normc((P, C, A), 0.01, g)})

    def layout(self):
        """(name, shape of one set, float offset within a packed set) of every parameter, in packed order."""
        A, C = self.num_actions, self.cell_size
        return _FIXED[:6] + (("lstm_w", (HIDDEN + C, 4 * C), _capi.SSD_LSTM_W), ("lstm_b", (4 * C,), _capi.SSD_LSTM_B(C)),
                             ("value_w", (C, 1), _capi.SSD_LSTM_VALUE_W(C)), ("value_b", (1,), _capi.SSD_LSTM_VALUE_B(C)),
                             ("logits_w", (C, A), _capi.SSD_LSTM_LOGITS_W(C)), ("logits_b", (A,), _capi.SSD_LSTM_LOGITS_B(C, A)))

    @property
    def set_floats(self):
        return _capi.SSD_LSTM_SET_FLOATS(self.cell_size, self.num_actions)

    def scratch_shape(self, rows):
        """The trunk's features: f32 [rows, 32]."""
        return (rows, _capi.SSD_LSTM_X)

    def ppo_scratch_shape(self, n_steps, num_envs, num_agents, seq_len):
        """The float32 scratch ssd_policy_lstm_ppo_grad needs for a [n_steps, num_envs, num_agents] fragment walked in windows
        of seq_len steps: what is kept of one window's rows for the backward, and the partial gradient sums."""
        return (_capi.SSD_RPPO_SCRATCH_FLOATS(n_steps, num_envs, num_agents, self.num_sets, self.num_actions, self.cell_size,
                                                  seq_len),)

    def forward(self, obs, state, starts=None):
        """obs u8 [..., (P,) 15, 15, 3], state [..., 2, C] (the same leading shape), starts bool [...] or None: rows whose state
        is replaced by zero (selected, not multiplied: whatever the state holds there is never used).  Returns (logits [..., A],
        value [...], new state [..., 2, C])."""
        P, A, C = self.num_sets, self.num_actions, self.cell_size
        x, lead = _trunk(self, obs)
        M = x.shape[0]
        if tuple(state.shape) != tuple(lead) + (2, C):
            raise ValueError("state must have shape %s, got %s" % (tuple(lead) + (2, C), tuple(state.shape)))
        st = state.to(x.dtype).reshape(M, P, 2, C)
        if starts is not None:
            if tuple(starts.shape) != tuple(lead):
                raise ValueError("starts must have shape %s, got %s" % (tuple(lead), tuple(starts.shape)))
            st = _zero_where(starts, st, 2)
        c, h = st[:, :, 0], st[:, :, 1]
        z = _dense(torch.cat([x, h], dim=-1), self.lstm_w, self.lstm_b)
        zi, zj, zf, zo = z[..., :C], z[..., C:2 * C], z[..., 2 * C:3 * C], z[..., 3 * C:]
        c2 = torch.sigmoid(zf + 1.0) * c + torch.sigmoid(zi) * torch.tanh(zj)
        h2 = torch.sigmoid(zo) * torch.tanh(c2)
        logits, value = _heads(h2, self.logits_w, self.logits_b, self.value_w, self.value_b)
        new_state = torch.stack([c2, h2], dim=2)
        return logits.reshape(tuple(lead) + (A,)), value.reshape(lead), new_state.reshape(tuple(lead) + (2, C))

    def forward_sequence(self, obs, state, resets=None):
        """T steps for truncated BPTT: obs u8 [T, ..., (P,) 15, 15, 3], state [..., 2, C] before step 0, resets bool [T, ...] or
        None (resets[t]: the state step t uses is zero, as the start rule of forward()).  Differentiable.  Returns (logits
        [T, ..., A], value [T, ...], the state after step T - 1)."""
        T = int(obs.shape[0])
        if resets is not None and int(resets.shape[0]) != T:
            raise ValueError("resets must have T = %d rows" % T)
        return _unroll(lambda t, st, reset: self.forward(obs[t], st, reset), T, state, resets)


def _softmax_cdf(logits):
    """The float32 cumulative softmax as the device accumulates it (include/ssd.h): logits [..., A] -> (logits as float32, their
    maximum mx [...], the sum s [...] of exp(logits - mx), the cumulative probabilities cdf [..., A])."""
    lg = np.asarray(logits, dtype=np.float32)
    mx = lg.max(axis=-1)
    e = np.exp(lg - mx[..., None]).astype(np.float32)
    s = np.zeros(mx.shape, np.float32)
    for a in range(lg.shape[-1]):
        s = (s + e[..., a]).astype(np.float32)
    c = np.zeros(mx.shape, np.float32)
    cdf = np.empty(lg.shape, np.float32)
    for a in range(lg.shape[-1]):
        c = (c + (e[..., a] / s).astype(np.float32)).astype(np.float32)
        cdf[..., a] = c
    return lg, mx, s, cdf


def sample_host(logits, u, greedy=False):
    """The rollout's action selection in NumPy float32 (include/ssd.h): logits [..., A] float32, u [...] float32 from
    prng.policy_uniforms.  Returns (actions int32, logp float32).  The device uses expf / logf, so an action may differ where
    u lies within an ulp or so of a boundary of the cumulative softmax."""
    lg, mx, s, cdf = _softmax_cdf(logits)
    A = lg.shape[-1]
    if greedy:
        act = lg.argmax(axis=-1).astype(np.int32)                    # the first of equal maxima
    else:
        u = np.asarray(u, dtype=np.float32)
        act = np.full(mx.shape, A - 1, np.int32)
        found = np.zeros(mx.shape, bool)
        for a in range(A):
            hit = ~found & (u < cdf[..., a])
            act[hit] = a
            found |= hit
    la = np.take_along_axis(lg, act[..., None].astype(np.int64), axis=-1)[..., 0]
    logp = (la - (mx + np.log(s).astype(np.float32))).astype(np.float32)
    return act, logp


def cdf_margin(logits, u):
    """Distance of u from the nearest boundary of the float32 cumulative softmax of logits (for deciding which sampled actions
    a host mirror may legitimately get differently)."""
    lg, mx, _, cdf = _softmax_cdf(logits)
    margin = np.full(mx.shape, np.inf)
    for a in range(lg.shape[-1]):
        margin = np.minimum(margin, np.abs(np.asarray(u, np.float64) - cdf[..., a].astype(np.float64)))
    return margin


def agent_order(num_agents):
    """Agent indices in the order of their ids sorted as strings ('agent-10' < 'agent-2'): map_env.py:202's order."""
    return sorted(range(int(num_agents)), key=lambda n: "agent-%d" % n)


def other_agents(num_agents):
    """others [N, N-1]: row i lists the agents other than i in string-sorted id order (the j of the MOA's predictions)."""
    order = agent_order(num_agents)
    return np.array([[n for n in order if n != i] for i in range(int(num_agents))], dtype=np.int64).reshape(int(num_agents), -1)


def keras_lstm(x, h, c, kernel, recurrent, bias):
    """One Keras LSTM step (TF 2.0): z = x @ kernel + h @ recurrent + bias, gates (i, f, c, o), no forget bias at run time."""
    C = h.shape[-1]
    z = x @ kernel + h @ recurrent + bias
    zi, zf, zc, zo = z[..., :C], z[..., C:2 * C], z[..., 2 * C:3 * C], z[..., 3 * C:]
    c2 = torch.sigmoid(zf) * c + torch.sigmoid(zi) * torch.tanh(zc)
    return torch.sigmoid(zo) * torch.tanh(c2), c2


class ConvMOAPolicy(PolicyBase):
    """The causal-influence policy of run_scripts/train_moa.py (MOA_LSTM, models/moa_model.py:121-311): the trunk's conv, two
    tanh FC stacks (32, 32), a Keras LSTM of cell_size C cells for the actions (logits and value on its output) and one for the
    model of other agents (MOA), whose input is the MOA stack's output and the N previous actions, own first and the others in
    string-sorted id order, and whose output predicts the others' next actions, pred [N-1, A] (include/ssd.h, MOA POLICY
    ROLLOUTS).  A state is [..., 4, C]: (h1, c1, h2, c2).

        policy = ConvMOAPolicy(8, num_agents=5, num_sets=5).cuda()
        state = policy.initial_state((E, 5))
        logits, value, moa_logits, cf_logits, state = policy(obs_u8, prev_actions, state, starts)
        r = influence(logits, cf_logits, actions, clip=10.0)             # the social-influence reward of each row

    Parameters in Keras' layouts with a leading weight-set axis: conv_w, conv_b; a_fc1_w [1014, 32] ... a_fc2_b (actions stack),
    m_fc1_w ... m_fc2_b (MOA stack); lstm_kernel [32, 4C], lstm_recurrent [C, 4C], lstm_bias [4C], logits_w [C, A], logits_b,
    value_w [C, 1], value_b; moa_kernel [32 + N, 4C], moa_recurrent [C, 4C], moa_bias [4C], pred_w [C, (N-1) A], pred_b."""
    STATE_ROWS = 4
    TAKES_PREV_ACTIONS = True
    C_FORWARD, C_ROLLOUT = "ssd_policy_moa_forward", "ssd_rollout_policy_moa"

    def __init__(self, num_actions, num_agents, num_sets=1, cell_size=128, seed=0):
        super().__init__()
        A, N, P, C = int(num_actions), int(num_agents), int(num_sets), int(cell_size)
        self._check_ranges(num_actions=A)
        if not 2 <= N <= _capi.SSD_MOA_MAX_AGENTS:
            raise ValueError("the MOA policy needs 2..%d agents" % _capi.SSD_MOA_MAX_AGENTS)
        if P not in (1, N):
            raise ValueError("num_sets must be 1 or num_agents")
        self._check_ranges(cell_size=C)
        self.num_actions, self.num_agents, self.num_sets, self.cell_size = A, N, P, C
        g = torch.Generator().manual_seed(int(seed))
        init = {"conv_w": _glorot((P, 3, 3, 3, FILTERS), 27, 9 * FILTERS, g),
                "lstm_kernel": _glorot((P, HIDDEN, 4 * C), HIDDEN, 4 * C, g), "lstm_recurrent": _orthogonal(P, C, 4 * C, g),
                "logits_w": _glorot((P, C, A), C, A, g), "value_w": normc((P, C, 1), 0.01, g),
                "moa_kernel": _glorot((P, HIDDEN + N, 4 * C), HIDDEN + N, 4 * C, g), "moa_recurrent": _orthogonal(P, C, 4 * C, g),
                "pred_w": _glorot((P, C, (N - 1) * A), C, (N - 1) * A, g)}
        for s in ("a", "m"):
            init[s + "_fc1_w"] = normc((P, FLAT, HIDDEN), 1.0, g)
            init[s + "_fc2_w"] = normc((P, HIDDEN, HIDDEN), 1.0, g)
        for name in ("lstm_bias", "moa_bias"):                  # Keras' unit_forget_bias: 1 in the forget block
            b = torch.zeros((P, 4 * C), dtype=torch.float64)
            b[:, C:2 * C] = 1.0
            init[name] = b
        self._register(init)
        self.register_buffer("_others", torch.from_numpy(other_agents(N)), persistent=False)

    def layout(self):
        """(name, shape of one set, float offset within a packed set) of every parameter, in packed order.  (The MOA input's
        zero rows 32 + N .. 47 belong to no parameter: packed() never writes them.)"""
        A, N, C = self.num_actions, self.num_agents, self.cell_size
        out = list(_FIXED[:2])
        for s, p in ((0, "a"), (1, "m")):
            out += [(p + "_fc1_w", (FLAT, HIDDEN), _capi.SSD_MOA_FC1_W(s)), (p + "_fc1_b", (HIDDEN,), _capi.SSD_MOA_FC1_B(s)),
                    (p + "_fc2_w", (HIDDEN, HIDDEN), _capi.SSD_MOA_FC2_W(s)), (p + "_fc2_b", (HIDDEN,), _capi.SSD_MOA_FC2_B(s))]
        lw, mw = _capi.SSD_MOA_LSTM_W(C), _capi.SSD_MOA_MW(C, A)
        out += [("lstm_kernel", (HIDDEN, 4 * C), lw), ("lstm_recurrent", (C, 4 * C), lw + HIDDEN * 4 * C),
                ("lstm_bias", (4 * C,), _capi.SSD_MOA_LSTM_B(C)),
                ("value_w", (C, 1), _capi.SSD_MOA_VALUE_W(C)), ("value_b", (1,), _capi.SSD_MOA_VALUE_B(C)),
                ("logits_w", (C, A), _capi.SSD_MOA_LOGITS_W(C)), ("logits_b", (A,), _capi.SSD_MOA_LOGITS_B(C, A)),
                ("moa_kernel", (HIDDEN + N, 4 * C), mw), ("moa_recurrent", (C, 4 * C), mw + _capi.SSD_MOA_XM * 4 * C),
                ("moa_bias", (4 * C,), _capi.SSD_MOA_MB(C, A)),
                ("pred_w", (C, (N - 1) * A), _capi.SSD_MOA_PRED_W(C, A)), ("pred_b", ((N - 1) * A,), _capi.SSD_MOA_PRED_B(C, A, N))]
        return tuple(out)

    @property
    def set_floats(self):
        return _capi.SSD_MOA_SET_FLOATS(self.cell_size, self.num_actions, self.num_agents)

    def scratch_shape(self, rows):
        return (_capi.SSD_MOA_SCRATCH_FLOATS(rows),)

    def ppo_scratch_shape(self, n_steps, num_envs, num_agents, seq_len):
        """The float32 scratch ssd_policy_moa_ppo_grad needs for a [n_steps, num_envs, num_agents] fragment walked in windows
        of seq_len steps (include/ssd.h, SSD_MPPO_SCRATCH_FLOATS)."""
        return (_capi.SSD_MPPO_SCRATCH_FLOATS(n_steps, num_envs, num_agents, self.num_sets, self.num_actions, self.cell_size,
                                              seq_len),)

    def _per_agent(self, name):
        """Parameter `name` with one entry per agent [N, ...] (set i, or set 0 for all when shared)."""
        t = getattr(self, name)
        return t.expand((self.num_agents,) + tuple(t.shape[1:])) if self.num_sets == 1 else t

    def _stacks(self, obs):
        """u8 [..., N, 15, 15, 3] -> (actions-stack output [M, N, 32], MOA-stack output [M, N, 32], leading shape [..., N])."""
        N, w = self.num_agents, self._per_agent
        if obs.shape[-3:] != (VIEW, VIEW, 3) or obs.dim() < 4 or obs.shape[-4] != N:
            raise ValueError("observations must be [..., %d, 15, 15, 3], got %s" % (N, tuple(obs.shape)))
        h = _conv_flat(self, obs, N, w("conv_w"), w("conv_b"))
        out = []
        for p in ("a", "m"):
            y = torch.tanh(_dense(h, w(p + "_fc1_w"), w(p + "_fc1_b")))
            out.append(torch.tanh(_dense(y, w(p + "_fc2_w"), w(p + "_fc2_b"))))
        return out[0], out[1], tuple(obs.shape[:-3])

    def _step(self, obs, prev_actions, state, starts, counterfactuals):
        N, A, C = self.num_agents, self.num_actions, self.cell_size
        ya, ym, lead = self._stacks(obs)
        M = ya.shape[0]
        if tuple(state.shape) != lead + (4, C):
            raise ValueError("state must have shape %s, got %s" % (lead + (4, C), tuple(state.shape)))
        if tuple(prev_actions.shape) != lead:
            raise ValueError("prev_actions must have shape %s, got %s" % (lead, tuple(prev_actions.shape)))
        st = state.to(ya.dtype).reshape(M, N, 4, C)
        prev = prev_actions.reshape(M, N).to(ya.device)
        if starts is not None:
            if tuple(starts.shape) != lead:
                raise ValueError("starts must have shape %s, got %s" % (lead, tuple(starts.shape)))
            st = _zero_where(starts, st, 2)
        h1, c1 = keras_lstm(ya[:, :, None, :], st[:, :, 0, None], st[:, :, 1, None], self._per_agent("lstm_kernel"),
                            self._per_agent("lstm_recurrent"), self._per_agent("lstm_bias")[:, None])
        h1, c1 = h1[:, :, 0], c1[:, :, 0]
        logits, value = _heads(h1, self._per_agent("logits_w"), self._per_agent("logits_b"), self._per_agent("value_w"),
                               self._per_agent("value_b"))
        # the MOA input of row (m, i): own previous action, then the others' in string order (zero at a start)
        others = prev[:, self._others.to(prev.device)]                           # [M, N, N-1]
        acts = torch.cat([prev[..., None], others], dim=-1)                      # [M, N, N]
        if starts is not None:                                  # a starting row's whole vector is zero (selected)
            acts = _zero_where(starts, acts, 1)
        acts = acts.to(ya.dtype)
        mk, mr, mb = self._per_agent("moa_kernel"), self._per_agent("moa_recurrent"), self._per_agent("moa_bias")[:, None]
        h2s, c2s = st[:, :, 2, None], st[:, :, 3, None]
        if counterfactuals:                                     # own slot replaced by a = 0 .. A-1: [M, N, A, 32 + N]
            cf_acts = acts[:, :, None, :].repeat(1, 1, A, 1)
            cf_acts[..., 0] = torch.arange(A, dtype=ya.dtype, device=ya.device)
            inp = torch.cat([ym[:, :, None, :].expand(M, N, A, HIDDEN), cf_acts], dim=-1)
            hcf, _ = keras_lstm(inp, h2s.expand(M, N, A, C), c2s.expand(M, N, A, C), mk, mr, mb)
            cf = torch.einsum("mnak,nkj->mnaj", hcf, self._per_agent("pred_w")) + self._per_agent("pred_b")[:, None]
            cf = cf.reshape(M, N, A, N - 1, A)
            own = acts[..., 0].long().clamp(0, A - 1)
            moa = torch.gather(cf, 2, own[:, :, None, None, None].expand(M, N, 1, N - 1, A))[:, :, 0]
        h2, c2 = keras_lstm(torch.cat([ym, acts], dim=-1)[:, :, None, :], h2s, c2s, mk, mr, mb)
        h2, c2 = h2[:, :, 0], c2[:, :, 0]
        if not counterfactuals:
            moa = _dense(h2, self._per_agent("pred_w"), self._per_agent("pred_b")).reshape(M, N, N - 1, A)
            cf = None
        new_state = torch.stack([h1, c1, h2, c2], dim=2)
        out = (logits.reshape(lead + (A,)), value.reshape(lead), moa.reshape(lead + (N - 1, A)),
               None if cf is None else cf.reshape(lead + (A, N - 1, A)), new_state.reshape(lead + (4, C)))
        return out

    def forward(self, obs, prev_actions, state, starts=None):
        """obs u8 [..., N, 15, 15, 3], prev_actions int [..., N] (the previous joint action of each row's env, by agent
        index), state [..., N, 4, C], starts bool [..., N] or None: rows whose state and previous actions are taken as zero
        (selected: whatever they hold there is never used).  Returns (logits [..., N, A], value [..., N], moa_logits
        [..., N, N-1, A], cf_logits [..., N, A, N-1, A], new state [..., N, 4, C]); moa_logits is cf_logits at the own
        previous action."""
        return self._step(obs, prev_actions, state, starts, True)

    def forward_sequence(self, obs, prev_actions, state, resets=None):
        """T steps for truncated BPTT, without counterfactuals: obs u8 [T, ..., N, 15, 15, 3], prev_actions [T, ..., N],
        state [..., N, 4, C] before step 0, resets bool [T, ..., N] or None (the start rule of forward()).  Differentiable.
        Returns (logits [T, ..., N, A], value [T, ..., N], moa_logits [T, ..., N, N-1, A], the state after step T - 1)."""
        T = int(obs.shape[0])
        if int(prev_actions.shape[0]) != T or (resets is not None and int(resets.shape[0]) != T):
            raise ValueError("prev_actions and resets must have T = %d rows" % T)

        def step(t, st, reset):
            lg, v, moa, _, st = self._step(obs[t], prev_actions[t], st, reset, False)
            return lg, v, moa, st
        return _unroll(step, T, state, resets)

    def moa_loss(self, moa_logits, actions, weight=1.0):
        """MOALoss (algorithms/common_funcs.py:70-95): the mean over rows and other agents of the cross-entropy of moa_logits
        [..., N, N-1, A] against the other agents' actions [..., N] taken at the SAME step (the reference pairs row t with row
        t + 1's other_agent_actions and drops the last row; here the targets are in the same actions ring), times weight."""
        N, A = self.num_agents, self.num_actions
        others = actions.long()[..., self._others.to(actions.device)]            # [..., N, N-1]
        ce = torch.nn.functional.cross_entropy(moa_logits.reshape(-1, A), others.reshape(-1), reduction="mean")
        return ce * weight


def influence(logits, cf_logits, actions, clip=10.0):
    """The social-influence reward of each row (include/ssd.h): logits [..., A] of this step's action distribution pi,
    cf_logits [..., A, N-1, A] the counterfactual predictions, actions [...] the actions taken.  For each other agent j,
    KL(p || q) with p = softmax(cf[a_t][j]) and q = sum_a pi(a) softmax(cf[a][j]), in log space; summed over j, clipped to
    [-clip, clip]; a non-finite row gives 0."""
    logits, cf = logits.to(torch.float32), cf_logits.to(torch.float32)
    lpi = torch.log_softmax(logits, dim=-1)                                       # [..., A]
    ls = torch.log_softmax(cf, dim=-1)                                            # [..., A, N-1, A]
    idx = actions.long()[..., None, None, None].expand(ls.shape[:-3] + (1,) + ls.shape[-2:])
    lp = torch.gather(ls, -3, idx)[..., 0, :, :]                                  # [..., N-1, A]
    lq = torch.logsumexp(lpi[..., :, None, None] + ls, dim=-3)
    p = lp.exp()
    kl = torch.where(p != 0, p * (lp - lq), torch.zeros((), dtype=p.dtype, device=p.device)).sum(-1).sum(-1)
    kl = torch.where(torch.isfinite(kl), kl, torch.zeros((), dtype=kl.dtype, device=kl.device))
    return kl.clamp(-float(clip), float(clip))


# ---- the PPO loss and its gradients for the conv-FC policy (include/ssd.h, PPO LOSS AND GRADIENTS; csrc/ssd_policy_grad.hip) ----

PPO_STATS = ("total_loss", "policy_loss", "vf_loss", "kl", "entropy")      # the columns of the library's stats, in order
_PPO_KEYS = (("obs", ("obs",)), ("actions", ("actions",)), ("logp_old", ("logp_old", "logp")),
             ("advantages", ("advantages",)), ("value_targets", ("value_targets",)), ("vf_pred", ("vf_pred", "value")),
             ("behaviour_logits", ("behaviour_logits", "logits")))
_A3C_ROWS = ("advantages", "value_targets")                                # the A3C loss's float per-row inputs


# The argument checks the loss functions share.  Each function calls them in its own order (the PPO functions look at the state
# ring before the device's type, the A3C functions after it), so which of two faults is named stays as it was.

def _check_seq_len(seq_len):
    if isinstance(seq_len, bool) or int(seq_len) != seq_len or int(seq_len) < 1:
        raise ValueError("seq_len must be an integer >= 1")
    return int(seq_len)


def _check_hyper(hyper, clips):
    """Finite hyper-parameters; clips: the first two are the PPO loss's clip parameters, which must not be negative."""
    finite = all(np.isfinite(hyper))
    if clips and (not finite or hyper[0] < 0 or hyper[1] < 0):
        raise ValueError("the hyper-parameters must be finite, clip_param and vf_clip_param >= 0")
    if not finite:
        raise ValueError("the hyper-parameters must be finite")


def _check_same_device(policy, dev, what="batch"):
    ref = getattr(policy, policy.REF_PARAM)
    if ref.device != dev:
        raise ValueError("the policy is on %s, the %s on %s" % (ref.device, what, dev))


def _check_device_type(dev):
    if dev.type not in ("cuda", "cpu"):
        raise ValueError("the tensors must be on the CPU or on a GPU, not on %s" % (dev,))


def _check_float32(policy, dev):
    if dev.type == "cuda" and getattr(policy, policy.REF_PARAM).dtype != torch.float32:
        raise ValueError("the device path needs a float32 policy")


def _check_tensor(x, dtype, shape, name, dev):
    if not isinstance(x, torch.Tensor) or x.dtype != dtype or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, shape, dev))


def _ppo_tensors(policy, batch, obs_first, kl_coeff, a3c=False):
    """The loss's inputs by their contract names from the dict sample() returns (logp as logp_old, value as vf_pred, logits
    as behaviour_logits) or a tuple in _PPO_KEYS' order, checked against each other: K from actions [K, E, N].  a3c: the A3C
    loss's inputs -- logp_old, vf_pred and behaviour_logits are not looked at (None); a tuple is (obs, actions, advantages,
    value_targets)."""
    per_row = _A3C_ROWS if a3c else ("logp_old", "advantages", "value_targets", "vf_pred")
    if isinstance(batch, dict):
        t = {name: next((batch[k] for k in keys if k in batch), None) for name, keys in _PPO_KEYS}
    elif a3c:
        vals = tuple(batch)
        if len(vals) != 4:
            raise ValueError("the tensors are (obs, actions, advantages, value_targets)")
        t = dict(zip(("obs", "actions") + _A3C_ROWS, vals))
    else:
        vals = tuple(batch)
        if not 6 <= len(vals) <= 7:
            raise ValueError("the tensors are (obs, actions, logp_old, advantages, value_targets, vf_pred[, behaviour_logits])")
        t = dict(zip((name for name, _ in _PPO_KEYS), vals + (None,) * (7 - len(vals))))
    if a3c:
        t["logp_old"] = t["vf_pred"] = t["behaviour_logits"] = None
    for name in ("actions",) + per_row:
        if not isinstance(t[name], torch.Tensor):
            raise ValueError("%s is required" % name)
    acts = t["actions"]
    if acts.dim() != 3 or acts.numel() == 0:
        raise ValueError("actions must be [K, E, N], got %s" % (tuple(acts.shape),))
    K, E, N = (int(n) for n in acts.shape)
    A, P, dev = policy.num_actions, policy.num_sets, acts.device
    if P not in (1, N):
        raise ValueError("the policy must have 1 or N = %d weight sets, not %d" % (N, P))
    if K * E * N > 2 ** 31 - 17:
        raise ValueError("the fragment must have at most 2^31 - 17 rows")
    if float(kl_coeff) == 0.0:
        t["behaviour_logits"] = None                        # not part of the loss
    elif t["behaviour_logits"] is None:
        raise ValueError("kl_coeff != 0 needs behaviour_logits (the logits the actions were sampled from)")
    _check_tensor(acts, torch.int32, (K, E, N), "actions", dev)
    for name in per_row:
        _check_tensor(t[name], torch.float32, (K, E, N), name, dev)
    if t["behaviour_logits"] is not None:
        _check_tensor(t["behaviour_logits"], torch.float32, (K, E, N, A), "behaviour_logits", dev)
    obs = t["obs"]
    need = K if obs_first is None else K - 1                # with obs_first the last row of obs is never read
    if need or obs is not None:
        if not isinstance(obs, torch.Tensor) or obs.dim() != 6 or obs.shape[0] < need:
            raise ValueError("obs must be a uint8 tensor [K, E, N, 15, 15, 3] of at least %d steps" % need)
        _check_tensor(obs, torch.uint8, (int(obs.shape[0]), E, N, VIEW, VIEW, 3), "obs", dev)
    if obs_first is not None:
        _check_tensor(obs_first, torch.uint8, (E, N, VIEW, VIEW, 3), "obs_first", dev)
    t["obs_first"] = obs_first
    return t, (K, E, N)


def ppo_terms(logits, value, t, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """RLlib 0.7.6's PPOLoss (use_gae=True) per row in plain torch, in the dtype of logits: (row_loss, -surr, vf, kl, ent),
    each of actions' shape.  t: the inputs by their contract names (include/ssd.h)."""
    dt = logits.dtype
    logp_all = torch.log_softmax(logits, dim=-1)
    p_all = logp_all.exp()
    logp = logp_all.gather(-1, t["actions"].long().unsqueeze(-1)).squeeze(-1)
    adv, vt, vfp = t["advantages"].to(dt), t["value_targets"].to(dt), t["vf_pred"].to(dt)
    ratio = torch.exp(logp - t["logp_old"].to(dt))
    surr = torch.minimum(adv * ratio, adv * ratio.clamp(1.0 - clip_param, 1.0 + clip_param))
    ent = -(p_all * logp_all).sum(-1)
    if t.get("behaviour_logits") is not None:
        blp = torch.log_softmax(t["behaviour_logits"].to(dt), dim=-1)
        kl = (blp.exp() * (blp - logp_all)).sum(-1)
    else:
        kl = torch.zeros_like(ent)
    vf1 = (value - vt).square()
    vf2 = (vfp + (value - vfp).clamp(-vf_clip_param, vf_clip_param) - vt).square()
    vf = torch.maximum(vf1, vf2)
    return -surr + kl_coeff * kl + vf_loss_coeff * vf - entropy_coeff * ent, -surr, vf, kl, ent


def _set_means(x, P):
    """The means of x [K, E, N] over each weight set's rows: [P]."""
    return x.mean().reshape(1) if P == 1 else x.reshape(-1, P).mean(0)


def _ppo_obs(t, K):
    """The observation each row acted on, by an explicit copy (the torch path): obs_first, then obs[:K - 1]."""
    if t["obs_first"] is None:
        return t["obs"][:K]
    return t["obs_first"].unsqueeze(0) if K == 1 else torch.cat([t["obs_first"].unsqueeze(0), t["obs"][:K - 1]])


def unpack_gradient(policy, grads, scale=None, only_set=None):
    """A packed gradient [P, set_floats] (the layout packed() writes) as one tensor per parameter of policy.layout(), in its
    order and the parameter's shape, times scale where given.  For a parameter with fewer entries than sets -- packed() wrote
    entry k into sets k, k + entries, ... -- the sets' gradients are summed (no ConvFCPolicy parameter is shared this way; a
    WatershedLSTMPolicy's dense1 with share_comm_layer is).  only_set: grads is [set_floats], the gradient of that one weight
    set (ssd_ws_policy_ppo_grad's); it goes to entry only_set % entries of each parameter, every other entry is exactly zero."""
    P = policy.num_sets
    out = []
    for name, shape, off in policy.layout():
        n = int(np.prod(shape))
        entries = getattr(policy, name).shape[0]
        if only_set is not None:
            g = grads.reshape(-1)[off:off + n]
            if scale is not None:
                g = g * scale
            full = torch.zeros((entries, n), dtype=g.dtype, device=g.device)
            full[int(only_set) % entries] = g
            out.append(full.reshape((entries,) + tuple(shape)))
            continue
        g = grads[:, off:off + n]
        if entries != P:
            g = g.reshape(P // entries, entries, n).sum(0)
        if scale is not None:
            g = g * scale
        out.append(g.reshape((entries,) + tuple(shape)))
    return out


def _state_tensors(policy, batch, K, E, N, seq_len, dev, need_prev=True):
    """The state ring [S, E, N, STATE_ROWS, C], done [K, E, N] (or None) and, for a ConvMOAPolicy, prev_actions [K, E, N] (else
    None) of a recurrent fragment, checked.  need_prev False: a ConvMOAPolicy's prev_actions may be missing (None then)."""
    C, R, S = policy.cell_size, policy.STATE_ROWS, -(-K // seq_len)
    state = batch.get("state")
    if state is None and seq_len >= K and batch.get("state_in") is not None:
        state = batch["state_in"].unsqueeze(0)                    # one window: the state step 0 used
    if not isinstance(state, torch.Tensor):
        raise ValueError("state is required: the ring sample(..., state_every=seq_len) records (state_in serves when seq_len >= K)")
    if state.dim() != 5 or tuple(state.shape[1:4]) != (E, N, R) or state.shape[0] < S:
        raise ValueError("state must be [S, %d, %d, %d, C] with S >= ceil(K / seq_len) = %d, got %s" % (E, N, R, S, tuple(state.shape)))
    if state.shape[-1] != C:
        raise ValueError("state has %d cells, the policy %d" % (state.shape[-1], C))
    if state.dtype != torch.float32 or state.device != dev or not state.is_contiguous():
        raise ValueError("state must be a contiguous torch.float32 tensor on %s" % (dev,))
    done, prev = batch.get("done"), None
    if done is not None:
        _check_tensor(done, torch.uint8, (K, E, N), "done", dev)
    if isinstance(policy, ConvMOAPolicy):
        prev = batch.get("prev_actions")
        if need_prev or prev is not None:
            _check_tensor(prev, torch.int32, (K, E, N), "prev_actions", dev)
    return state, done, prev


def _forward_windows(policy, obs, prev_actions, state, done, seq_len):
    """The window walk of the state rule of include/ssd.h: forward_sequence on steps k0 .. k1 - 1 of each window from ring entry
    state[w] (data), step k of a window reset where done[k - 1] is set -> forward_sequence's outputs joined over the windows,
    then the state after the last step.  prev_actions: None for a ConvLSTMPolicy."""
    K, T = int(obs.shape[0]), int(seq_len)
    dt = policy.conv_w.dtype
    windows = []
    for w, k0 in enumerate(range(0, K, T)):
        k1 = min(k0 + T, K)
        resets = None
        if done is not None and k1 - k0 > 1:
            resets = torch.cat([torch.zeros_like(done[:1]), done[k0:k1 - 1]]).to(torch.bool)
        rows = (obs[k0:k1],) if prev_actions is None else (obs[k0:k1], prev_actions[k0:k1])
        *out, last = policy.forward_sequence(*rows, state[w].detach().to(dt), resets)
        windows.append(out)
    return tuple(torch.cat(col) for col in zip(*windows)) + (last,)


def _moa_set_ce(policy, moa_logits, actions):
    """policy.moa_loss of each weight set's rows [P]: the mean cross-entropy of moa_logits [K, E, N, N-1, A] against the other
    agents' actions [K, E, N] (clamped to 0 .. A - 1) of the same step."""
    A, P = policy.num_actions, policy.num_sets
    acts = actions.clamp(0, A - 1)
    if P == 1:
        return policy.moa_loss(moa_logits, acts).reshape(1)
    others = acts.long()[..., policy._others.to(acts.device)]       # [K, E, N, N-1]; set p's rows are agent p's: its N - 1 predictions
    return torch.stack([torch.nn.functional.cross_entropy(moa_logits[:, :, p].reshape(-1, A), others[:, :, p].reshape(-1))
                        for p in range(P)])


def _cpu_result(per_set, names, ce=None, moa_weight=0.0):
    """The end of a CPU path: per_set, the loss's terms reduced over each weight set's rows ([P] each, the total first), and
    for the MOA policy the sets' cross-entropy ce [P], added to the total with its weight -> (loss, stats by `names`)."""
    if ce is not None:
        per_set[0] = per_set[0] + moa_weight * ce
        per_set.append(ce)
    return per_set[0].sum(), {name: m.detach() for name, m in zip(names, per_set)}


def _ppo_prepare(policy, batch, obs_first, seq_len, hyper):
    """The checks the three PPO functions share -> (t, (K, E, N), seq_len, hyper as floats, dev).  seq_len None: the conv-FC
    policy's call; hyper: the five of PPOLoss and, for the MOA policy, moa_weight."""
    if seq_len is not None:
        if not isinstance(batch, dict):
            raise ValueError("batch must be the dict sample() returns")
        seq_len = _check_seq_len(seq_len)
    hyper = tuple(float(x) for x in hyper)
    _check_hyper(hyper, clips=True)
    if len(hyper) > 5 and hyper[5] < 0:
        raise ValueError("moa_weight must be >= 0")
    t, (K, E, N) = _ppo_tensors(policy, batch, obs_first, hyper[4])
    if isinstance(policy, ConvMOAPolicy) and N != policy.num_agents:
        raise ValueError("the policy is for %d agents, the batch has %d" % (policy.num_agents, N))
    dev = t["actions"].device
    _check_same_device(policy, dev)
    if seq_len is not None:
        t["state"], t["done"], t["prev_actions"] = _state_tensors(policy, batch, K, E, N, seq_len, dev)
    _check_float32(policy, dev)
    _check_device_type(dev)
    return t, (K, E, N), seq_len, hyper, dev


def ppo_loss(policy, batch, *, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, obs_first=None):
    """RLlib 0.7.6's PPO loss (PPOLoss with use_gae=True) of a ConvFCPolicy on a sampled fragment -> (loss, stats): loss a
    scalar tensor that backpropagates into the policy's parameters, stats a dict of [P] tensors (PPO_STATS: the set means of
    the total, policy, value-function, KL and entropy terms).  include/ssd.h (PPO LOSS AND GRADIENTS) states the loss, the
    rows of a weight set, the derivatives at the clip boundaries and the order of the sums; loss is the sum over the weight
    sets of each set's mean row loss.

        first = env.reset().clone()
        batch = env.sample(policy, 128, gamma=0.99, lambda_=0.95)
        loss, stats = ppo_loss(policy, batch, clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=1e-3,
                               kl_coeff=0.0, obs_first=first)
        loss.backward(); optimiser.step()

    batch: the dict sample() returns (obs, actions, logp as logp_old, value as vf_pred, advantages, value_targets and, where
    present, logits as behaviour_logits; the contract names are accepted too), or the tensors as a tuple in that order:
    obs u8 [K,E,N,15,15,3], actions i32, the rest f32 [K,E,N], behaviour_logits f32 [K,E,N,A] (needed if and only if kl_coeff
    != 0).  obs_first u8 [E,N,15,15,3]: row k acted on obs_first for k = 0 and on obs[k - 1] otherwise, as sample() records
    them; None: on obs[k].  A minibatch of steps k0 .. k1 - 1 is the leading-axis slices [k0:k1] of every tensor with
    obs_first = obs[k0 - 1].
    CUDA tensors go to the library (ssd_policy_ppo_grad: two launches on torch's current stream, no synchronisation, no
    activation kept); CPU tensors run the same loss in plain torch under autograd."""
    if not isinstance(policy, ConvFCPolicy):
        raise ValueError("ppo_loss is for a ConvFCPolicy (the recurrent policies need backpropagation through time)")
    hyper = (clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff)
    t, (K, E, N), _, hyper, dev = _ppo_prepare(policy, batch, obs_first, None, hyper)
    if dev.type == "cuda":
        return _device_loss(policy, (ConvFCPolicy, "ppo"), t, (K, E, N), 0, hyper)
    logits, value = policy(_ppo_obs(t, K))
    return _cpu_result([_set_means(x, policy.num_sets) for x in ppo_terms(logits, value, t, *hyper)], PPO_STATS)


# ---- the same loss for the recurrent policy, with truncated BPTT (include/ssd.h, RECURRENT PPO LOSS AND GRADIENTS) ----

def recurrent_forward(policy, obs, state, done, seq_len):
    """The learner's forward of a ConvLSTMPolicy over a fragment, in plain torch under autograd, by the state rule of
    include/ssd.h: obs u8 [K, E, N, 15, 15, 3] (the observation each row acted on), the ring state [S, E, N, 2, C] (detached:
    data), done u8 [K, E, N] or None -> (logits [K, E, N, A], value [K, E, N]).  Window by window through forward_sequence;
    step k of a window resets where done[k - 1] is set."""
    return _forward_windows(policy, obs, None, state, done, seq_len)[:2]


def ppo_loss_recurrent(policy, batch, *, seq_len, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, obs_first=None):
    """ppo_loss for a ConvLSTMPolicy: the same loss, rows, observation shift and statistics, with truncated backpropagation
    through time over windows of seq_len steps (RLlib's max_seq_len) -> (loss, stats).  include/ssd.h (RECURRENT PPO LOSS AND
    GRADIENTS) states the state rule: a window starts from the recorded state (no gradient into it), a step after a done row
    starts from zero, every other step from the state the step before it computed with the current weights.

        first = env.reset().clone()
        batch = env.sample(policy, 128, state_every=16, gamma=0.99, lambda_=0.95)
        loss, stats = ppo_loss_recurrent(policy, batch, seq_len=16, clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4,
                                         entropy_coeff=1e-3, kl_coeff=0.0, obs_first=first)
        loss.backward(); optimiser.step()

    batch: the dict sample(policy, K, state_every=seq_len, gamma=...) returns -- ppo_loss's keys and besides "state" f32
    [S,E,N,2,C], S = ceil(K / seq_len) ("state_in" serves when seq_len >= K) and "done" u8 [K,E,N] (absent or None: no episode
    ends inside the fragment).  A minibatch of steps k0 .. k1 - 1 with k0 a multiple of seq_len is the slices [k0:k1] of the
    per-row tensors, state[k0 // seq_len:] and obs_first = obs[k0 - 1].
    CUDA tensors go to the library (ssd_policy_lstm_ppo_grad on torch's current stream, no synchronisation; the scratch is
    kept on the policy); CPU tensors run forward_sequence per window and ppo_terms under autograd."""
    if not isinstance(policy, ConvLSTMPolicy):
        raise ValueError("ppo_loss_recurrent is for a ConvLSTMPolicy (ppo_loss is the ConvFCPolicy's)")
    hyper = (clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff)
    t, (K, E, N), seq_len, hyper, dev = _ppo_prepare(policy, batch, obs_first, seq_len, hyper)
    if dev.type == "cuda":
        return _device_loss(policy, (ConvLSTMPolicy, "ppo"), t, (K, E, N), seq_len, hyper)
    logits, value = recurrent_forward(policy, _ppo_obs(t, K), t["state"], t["done"], seq_len)
    return _cpu_result([_set_means(x, policy.num_sets) for x in ppo_terms(logits, value, t, *hyper)], PPO_STATS)


# ---- PPOLoss + moa_weight * MOALoss for the MOA policy, with truncated BPTT (include/ssd.h, MOA PPO LOSS AND GRADIENTS) ----

MOA_PPO_STATS = PPO_STATS + ("moa_loss",)


def moa_forward(policy, obs, prev_actions, state, done, seq_len):
    """The learner's forward of a ConvMOAPolicy over a fragment, in plain torch under autograd, by the state rule of
    include/ssd.h: obs u8 [K, E, N, 15, 15, 3] (the observation each row acted on), prev_actions int [K, E, N], the ring state
    [S, E, N, 4, C] (detached: data), done u8 [K, E, N] or None -> (logits [K, E, N, A], value [K, E, N], moa_logits
    [K, E, N, N-1, A]).  Window by window through forward_sequence; step k of a window resets where done[k - 1] is set."""
    return _forward_windows(policy, obs, prev_actions, state, done, seq_len)[:3]


def ppo_loss_moa(policy, batch, *, seq_len, moa_weight, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff,
                 obs_first=None):
    """The causal-influence trainer's loss for a ConvMOAPolicy, PPOLoss + moa_weight * MOALoss (algorithms/ppo_causal.py:36-75),
    with truncated backpropagation through time through both LSTMs over windows of seq_len steps -> (loss, stats): loss a
    scalar tensor that backpropagates into every parameter, stats a dict of [P] tensors (MOA_PPO_STATS: ppo_loss's five, whose
    total_loss includes the weighted MOA term, then moa_loss, the mean cross-entropy without the weight).  include/ssd.h (MOA
    PPO LOSS AND GRADIENTS) states the loss and the state rule.  Per weight set the MOA term is policy.moa_loss of the set's
    rows: the targets of row (k, e, i) are the other agents' actions of step k.  The influence reward is data: it is inside the
    advantages sample(..., influence_weight=...) computed.

        first = env.reset().clone()
        batch = env.sample(policy, 128, state_every=16, gamma=0.99, lambda_=0.95, influence_weight=1.0)
        loss, stats = ppo_loss_moa(policy, batch, seq_len=16, moa_weight=10.0, clip_param=0.3, vf_clip_param=10.0,
                                   vf_loss_coeff=1e-4, entropy_coeff=1e-3, kl_coeff=0.0, obs_first=first)
        loss.backward(); optimiser.step()

    batch: the dict sample(policy, K, state_every=seq_len, gamma=...) returns -- ppo_loss_recurrent's keys with "state" f32
    [S,E,N,4,C], and "prev_actions" i32 [K,E,N], the joint action each step's MOA read.  A minibatch of steps k0 .. k1 - 1 with
    k0 a multiple of seq_len is the slices [k0:k1] of the per-row tensors (prev_actions among them), state[k0 // seq_len:] and
    obs_first = obs[k0 - 1].
    CUDA tensors go to the library (ssd_policy_moa_ppo_grad on torch's current stream, no synchronisation; the scratch is kept
    on the policy); CPU tensors run forward_sequence per window, ppo_terms and moa_loss per set under autograd."""
    if not isinstance(policy, ConvMOAPolicy):
        raise ValueError("ppo_loss_moa is for a ConvMOAPolicy (ppo_loss and ppo_loss_recurrent are the other policies')")
    hyper = (clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff, moa_weight)
    t, (K, E, N), seq_len, hyper, dev = _ppo_prepare(policy, batch, obs_first, seq_len, hyper)
    if dev.type == "cuda":
        return _device_loss(policy, (ConvMOAPolicy, "ppo"), t, (K, E, N), seq_len, hyper)
    logits, value, moa = moa_forward(policy, _ppo_obs(t, K), t["prev_actions"], t["state"], t["done"], seq_len)
    means = [_set_means(x, policy.num_sets) for x in ppo_terms(logits, value, t, *hyper[:5])]
    return _cpu_result(means, MOA_PPO_STATS, _moa_set_ce(policy, moa, t["actions"]), hyper[5])


# ---- the A3C loss of the three policies (include/ssd.h, A3C LOSS AND GRADIENTS) ----

A3C_STATS = ("total_loss", "policy_loss", "vf_loss", "policy_entropy")      # the columns of the library's stats, in order
MOA_A3C_STATS = A3C_STATS + ("moa_loss",)


def a3c_terms(logits, value, t, vf_loss_coeff, entropy_coeff):
    """The reference's A3C loss (algorithms/a3c_causal.py:28-46) per row in plain torch, in the dtype of logits: (row_loss, pi,
    vf, ent), each of actions' shape.  t: actions (clamped to 0 .. A - 1), advantages and value_targets by their contract names."""
    dt = logits.dtype
    logp_all = torch.log_softmax(logits, dim=-1)
    acts = t["actions"].long().clamp(0, logits.shape[-1] - 1)
    logp = logp_all.gather(-1, acts.unsqueeze(-1)).squeeze(-1)
    pi = -(logp * t["advantages"].to(dt))
    vf = 0.5 * (value - t["value_targets"].to(dt)).square()
    ent = -(logp_all.exp() * logp_all).sum(-1)
    return (pi + vf_loss_coeff * vf) - entropy_coeff * ent, pi, vf, ent


def _set_sums(x, P):
    """The sums of x [K, E, N] over each weight set's rows: [P]."""
    return x.sum().reshape(1) if P == 1 else x.reshape(-1, P).sum(0)


def _a3c_prepare(policy, batch, obs_first, seq_len, hyper):
    """The checks the three A3C functions share -> (t, (K, E, N), seq_len, dev).  seq_len None: the conv-FC policy's call; hyper:
    (vf_loss_coeff, entropy_coeff) and, for the MOA policy, moa_weight."""
    if seq_len is not None:
        if not isinstance(batch, dict):
            raise ValueError("batch must be the dict sample() returns")
        seq_len = _check_seq_len(seq_len)
    _check_hyper(hyper, clips=False)
    t, (K, E, N) = _ppo_tensors(policy, batch, obs_first, 0.0, a3c=True)
    dev = t["actions"].device
    _check_same_device(policy, dev)
    _check_device_type(dev)
    _check_float32(policy, dev)
    if len(hyper) > 2 and hyper[2] < 0:
        raise ValueError("moa_weight must be >= 0")
    if isinstance(policy, ConvMOAPolicy) and N != policy.num_agents:
        raise ValueError("the policy is for %d agents, the batch has %d" % (policy.num_agents, N))
    if seq_len is not None:
        t["state"], t["done"], t["prev_actions"] = _state_tensors(policy, batch, K, E, N, seq_len, dev)
    return t, (K, E, N), seq_len, dev


def a3c_loss(policy, batch, *, vf_loss_coeff, entropy_coeff, obs_first=None):
    """The reference's A3C loss (algorithms/a3c_causal.py:28-46, the baseline's default algorithm) of a ConvFCPolicy on a
    sampled fragment -> (loss, stats), as ppo_loss: loss a scalar tensor that backpropagates into the policy's parameters,
    stats a dict of [P] tensors (A3C_STATS: the set SUMS of the total, policy, value-function and entropy terms).  include/ssd.h
    (A3C LOSS AND GRADIENTS) states the loss: per row -logp * adv + vf_loss_coeff * 0.5 (value - vt)^2 - entropy_coeff * ent,
    summed (not averaged) over a weight set's rows, then over the sets.

        first = env.reset().clone()
        batch = env.sample(policy, 128, gamma=0.99, use_gae=False)
        loss, stats = a3c_loss(policy, batch, vf_loss_coeff=0.5, entropy_coeff=0.01, obs_first=first)
        loss.backward(); clip_grad_by_set_norm(policy, 40.0); optimiser.step()

    batch: the dict sample() returns (obs, actions, advantages and value_targets are read; logp, value and logits are
    ignored), or the tuple (obs, actions, advantages, value_targets).  obs_first and minibatches: as ppo_loss.
    CUDA tensors go to the library (ssd_policy_ac_grad: two launches on torch's current stream); CPU tensors run a3c_terms in
    plain torch under autograd."""
    if not isinstance(policy, ConvFCPolicy):
        raise ValueError("a3c_loss is for a ConvFCPolicy (a3c_loss_recurrent and a3c_loss_moa are the other policies')")
    hyper = (float(vf_loss_coeff), float(entropy_coeff))
    t, (K, E, N), _, dev = _a3c_prepare(policy, batch, obs_first, None, hyper)
    if dev.type == "cuda":
        return _device_loss(policy, (ConvFCPolicy, "a3c"), t, (K, E, N), 0, hyper)
    logits, value = policy(_ppo_obs(t, K))
    return _cpu_result([_set_sums(x, policy.num_sets) for x in a3c_terms(logits, value, t, *hyper)], A3C_STATS)


def a3c_loss_recurrent(policy, batch, *, seq_len, vf_loss_coeff, entropy_coeff, obs_first=None):
    """a3c_loss for a ConvLSTMPolicy (the baseline's default: A3C on the recurrent policy), with truncated backpropagation
    through time over windows of seq_len steps as ppo_loss_recurrent -> (loss, stats).  The state rule, the batch's keys
    ("state", "done") and the minibatch slices are ppo_loss_recurrent's.

        batch = env.sample(policy, 128, state_every=16, gamma=0.99, use_gae=False)
        loss, stats = a3c_loss_recurrent(policy, batch, seq_len=16, vf_loss_coeff=0.5, entropy_coeff=0.01, obs_first=first)

    CUDA tensors go to the library (ssd_policy_lstm_ac_grad); CPU tensors run recurrent_forward and a3c_terms under autograd."""
    if not isinstance(policy, ConvLSTMPolicy):
        raise ValueError("a3c_loss_recurrent is for a ConvLSTMPolicy (a3c_loss is the ConvFCPolicy's)")
    hyper = (float(vf_loss_coeff), float(entropy_coeff))
    t, (K, E, N), seq_len, dev = _a3c_prepare(policy, batch, obs_first, seq_len, hyper)
    if dev.type == "cuda":
        return _device_loss(policy, (ConvLSTMPolicy, "a3c"), t, (K, E, N), seq_len, hyper)
    logits, value = recurrent_forward(policy, _ppo_obs(t, K), t["state"], t["done"], seq_len)
    return _cpu_result([_set_sums(x, policy.num_sets) for x in a3c_terms(logits, value, t, *hyper)], A3C_STATS)


def a3c_loss_moa(policy, batch, *, seq_len, moa_weight, vf_loss_coeff, entropy_coeff, obs_first=None):
    """The causal-influence trainer's A3C loss for a ConvMOAPolicy, the A3C terms + moa_weight * MOALoss (algorithms/
    a3c_causal.py:60-76), with truncated BPTT through both LSTMs as ppo_loss_moa -> (loss, stats): stats a dict of [P] tensors
    (MOA_A3C_STATS: a3c_loss's four sums, total_loss including the weighted MOA term, then moa_loss).  The A3C terms are SUMS
    over a set's rows while MOALoss is the MEAN cross-entropy of the set's rows, as in the reference.  The batch's keys
    ("state", "done", "prev_actions"), the pairing of predictions and targets and the minibatch slices are ppo_loss_moa's.

        batch = env.sample(policy, 128, state_every=16, gamma=0.99, use_gae=False, influence_weight=1.0)
        loss, stats = a3c_loss_moa(policy, batch, seq_len=16, moa_weight=10.0, vf_loss_coeff=0.5, entropy_coeff=0.01,
                                   obs_first=first)

    CUDA tensors go to the library (ssd_policy_moa_ac_grad); CPU tensors run moa_forward, a3c_terms and moa_loss per set."""
    if not isinstance(policy, ConvMOAPolicy):
        raise ValueError("a3c_loss_moa is for a ConvMOAPolicy (a3c_loss and a3c_loss_recurrent are the other policies')")
    hyper = (float(vf_loss_coeff), float(entropy_coeff), float(moa_weight))
    t, (K, E, N), seq_len, dev = _a3c_prepare(policy, batch, obs_first, seq_len, hyper)
    if dev.type == "cuda":
        return _device_loss(policy, (ConvMOAPolicy, "a3c"), t, (K, E, N), seq_len, hyper)
    logits, value, moa = moa_forward(policy, _ppo_obs(t, K), t["prev_actions"], t["state"], t["done"], seq_len)
    sums = [_set_sums(x, policy.num_sets) for x in a3c_terms(logits, value, t, *hyper[:2])]
    return _cpu_result(sums, MOA_A3C_STATS, _moa_set_ce(policy, moa, t["actions"]), hyper[2])


# ---- the IMPALA loss of the three policies: V-trace targets under the current weights, then the A3C loss's path
# ---- (include/ssd.h, V-TRACE TARGETS) ----

def _fragment_tensors(policy, batch, obs_first, seq_len, one_call=False):
    """What evaluate_fragment reads of the dict sample() returns, checked -> (t, (K, E, N), seq_len).  The observations must
    reach one row further than a loss call's: the bootstrap reads obs[K - 1] (obs[K] without obs_first).  one_call with CUDA
    tensors: a ConvMOAPolicy's prev_actions is not read and may be missing."""
    if not isinstance(batch, dict):
        raise ValueError("batch must be the dict sample() returns")
    acts, obs = batch.get("actions"), batch.get("obs")
    if not isinstance(acts, torch.Tensor) or acts.dim() != 3 or acts.numel() == 0:
        raise ValueError("actions must be an int32 tensor [K, E, N]")
    K, E, N = (int(n) for n in acts.shape)
    dev, P = acts.device, policy.num_sets
    if P not in (1, N):
        raise ValueError("the policy must have 1 or N = %d weight sets, not %d" % (N, P))
    if (K + 1) * E * N > 2 ** 31 - 17:
        raise ValueError("the fragment must have fewer than 2^31 - 17 rows")
    if acts.dtype != torch.int32 or not acts.is_contiguous():
        raise ValueError("actions must be a contiguous torch.int32 tensor")
    need = K if obs_first is not None else K + 1
    if (not isinstance(obs, torch.Tensor) or obs.dim() != 6 or obs.shape[0] < need or obs.dtype != torch.uint8 or obs.device != dev
            or tuple(obs.shape[1:]) != (E, N, VIEW, VIEW, 3) or not obs.is_contiguous()):
        raise ValueError("obs must be a contiguous uint8 tensor [R, %d, %d, 15, 15, 3] on %s with R >= %d: the bootstrap reads the "
                         "observation after the last row" % (E, N, dev, need))
    if obs_first is not None:
        if (not isinstance(obs_first, torch.Tensor) or obs_first.dtype != torch.uint8 or obs_first.device != dev
                or tuple(obs_first.shape) != (E, N, VIEW, VIEW, 3) or not obs_first.is_contiguous()):
            raise ValueError("obs_first must be a contiguous uint8 tensor of shape %s on %s" % ((E, N, VIEW, VIEW, 3), dev))
    _check_same_device(policy, dev)
    _check_device_type(dev)
    _check_float32(policy, dev)
    t = {"actions": acts, "obs": obs, "obs_first": obs_first}
    if isinstance(policy, ConvFCPolicy):
        return t, (K, E, N), None
    if seq_len is None:
        raise ValueError("seq_len must be an integer >= 1")
    seq_len = _check_seq_len(seq_len)
    if isinstance(policy, ConvMOAPolicy) and N != policy.num_agents:
        raise ValueError("the policy is for %d agents, the batch has %d" % (policy.num_agents, N))
    t["state"], t["done"], t["prev_actions"] = _state_tensors(policy, batch, K, E, N, seq_len, dev,
                                                              need_prev=not (one_call and dev.type == "cuda"))
    return t, (K, E, N), seq_len


def _evaluate_device(policy, t, dims, T):
    """evaluate_fragment through the library's forward entry points on torch's current stream, rows 0 .. K - 1 and the
    bootstrap as row K of one allocation."""
    K, E, N = dims
    A, P, dev = policy.num_actions, policy.num_sets, t["actions"].device
    weights = policy.packed()
    logits = torch.empty((K + 1, E, N, A), dtype=torch.float32, device=dev)
    value = torch.empty((K + 1, E, N), dtype=torch.float32, device=dev)
    ptr, index, stream = _device_handles(dev)
    L = _capi.lib()
    obs, first = t["obs"], t["obs_first"]
    if isinstance(policy, ConvFCPolicy):                          # one launch, or two: obs_first's row, then obs[0 .. K - 1]
        if first is None:
            calls = ((obs, (K + 1) * E, logits, value),)
        else:
            calls = ((first, E, logits[0], value[0]), (obs, K * E, logits[1:], value[1:]))
        for o, B, lg, v in calls:
            _capi.policy_check(L.ssd_policy_forward(ptr(weights), P, A, ptr(o), B, N, ptr(lg), ptr(v), index, 0, stream))
        return logits[:K], value[:K], value[K]
    moa = isinstance(policy, ConvMOAPolicy)
    Cs, done = policy.cell_size, t["done"]
    need = int(np.prod(policy.scratch_shape(E * N)))
    scratch = getattr(policy, "_eval_scratch", None)              # kept between calls, as _ppo_scratch is
    if scratch is None or scratch.device != dev or scratch.numel() < need:
        scratch = policy._eval_scratch = torch.empty(need, dtype=torch.float32, device=dev)
    carry = torch.empty((E, N, policy.STATE_ROWS, Cs), dtype=torch.float32, device=dev)
    for k in range(K + 1):                                        # one launch per step; row K is the bootstrap
        boot = k == K
        o = obs[k] if first is None else (first if k == 0 else obs[k - 1])
        if not boot and k % T == 0:
            s_in, starts = t["state"][k // T], None               # the ring's entry, as stored
        else:
            s_in, starts = carry, (None if done is None else done[k - 1])
        s_out, lg = (None, None) if boot else (carry, logits[k])
        if moa:
            prev = t["actions"][K - 1] if boot else t["prev_actions"][k]
            rc = L.ssd_policy_moa_forward(ptr(weights), P, A, Cs, ptr(o), ptr(prev), ptr(s_in), ptr(starts), E, N, ptr(scratch),
                                          ptr(s_out), ptr(lg), ptr(value[k]), None, None, None, None, 0.0, index, 0, stream)
        else:
            rc = L.ssd_policy_lstm_forward(ptr(weights), P, A, Cs, ptr(o), ptr(s_in), ptr(starts), E, N, ptr(scratch), ptr(s_out),
                                           ptr(lg), ptr(value[k]), index, 0, stream)
        _capi.policy_check(rc)
    return logits[:K], value[:K], value[K]


def _seq_scratch_rows(policy, dims, T):
    """The feature rows of the one-call evaluation's scratch: the whole fragment's, the bootstrap's included, when those take no
    more memory than the policy's loss call needs for this batch anyway (ppo_scratch_shape: one window's rows and the partial
    sums); otherwise as many whole windows as fit in that size, and never less than one window and the bootstrap row."""
    K, E, N = dims
    whole, least = (K + 1) * E * N, (min(T, K) + 1) * E * N
    limit = int(policy.ppo_scratch_shape(K, E, N, T)[0]) // _capi.SSD_LSTM_X
    if whole <= limit:
        return whole
    return max(least, ((limit // (E * N) - 1) // T * T + 1) * E * N)


def _evaluate_device_seq(policy, t, dims, T):
    """evaluate_fragment through ssd_policy_lstm_forward_seq / ssd_policy_moa_forward_seq on torch's current stream: one call,
    a trunk launch and a cell launch per chunk of windows."""
    K, E, N = dims
    A, P, Cs, dev = policy.num_actions, policy.num_sets, policy.cell_size, t["actions"].device
    weights = policy.packed()
    logits = torch.empty((K, E, N, A), dtype=torch.float32, device=dev)
    value = torch.empty((K, E, N), dtype=torch.float32, device=dev)
    boot = torch.empty((E, N), dtype=torch.float32, device=dev)
    rows = _seq_scratch_rows(policy, dims, T)
    scratch = getattr(policy, "_eval_seq_scratch", None)          # kept between calls, as _eval_scratch is
    if scratch is None or scratch.device != dev or scratch.numel() < rows * _capi.SSD_LSTM_X:
        scratch = policy._eval_seq_scratch = torch.empty(rows * _capi.SSD_LSTM_X, dtype=torch.float32, device=dev)
    ptr, index, stream = _device_handles(dev)
    L = _capi.lib()
    call = L.ssd_policy_moa_forward_seq if isinstance(policy, ConvMOAPolicy) else L.ssd_policy_lstm_forward_seq
    _capi.policy_check(call(ptr(weights), P, A, Cs, T, ptr(t["obs_first"]), ptr(t["obs"]), ptr(t["state"]), ptr(t["done"]), K, E, N,
                            ptr(scratch), rows, ptr(logits), ptr(value), ptr(boot), None, index, 0, stream))
    return logits, value, boot


def _evaluate_host(policy, t, dims, T):
    """evaluate_fragment in plain torch: the loss calls' forwards window by window, and one more step for the bootstrap."""
    K, E, N = dims
    obs, first = t["obs"], t["obs_first"]
    rows = obs[:K] if first is None else _ppo_obs(t, K)
    last = obs[K] if first is None else obs[K - 1]
    if isinstance(policy, ConvFCPolicy):
        logits, value = policy(rows)
        return logits, value, policy(last)[1]
    moa, done = isinstance(policy, ConvMOAPolicy), t["done"]
    logits, value, *_, st = _forward_windows(policy, rows, t["prev_actions"], t["state"], done, T)
    starts = None if done is None else done[K - 1].to(torch.bool)
    boot = policy(last, t["actions"][K - 1], st, starts)[1] if moa else policy(last, st, starts)[1]
    return logits, value, boot


def evaluate_fragment(policy, batch, obs_first=None, seq_len=None, one_call=False):
    """A sampled fragment under the policy's CURRENT weights -> (logits [K,E,N,A], value [K,E,N], bootstrap_value [E,N]),
    without gradient: what V-trace needs of the target policy (postprocessing.vtrace) when the weights have moved since
    sample() ran.  Row k reads obs_first for k = 0 and obs[k - 1] otherwise (the loss calls' shift, by address; obs_first None:
    row k reads obs[k]), and bootstrap_value is the value of the observation after the last row: obs[K - 1], which this call
    does read (obs[K] without obs_first).

    batch: the dict sample() returns.  ConvFCPolicy: "obs" and "actions" (for the shape), seq_len unused.  ConvLSTMPolicy and
    ConvMOAPolicy: seq_len = T and the keys of ppo_loss_recurrent / ppo_loss_moa ("state", "done", "prev_actions"), under the
    state rule of include/ssd.h (RECURRENT PPO LOSS AND GRADIENTS): step k uses state[k // T] as stored when k % T == 0, else
    the state step k - 1 computed, zero where done[k - 1]; the bootstrap row uses the carried state with the start rule of
    done[K - 1], never a ring entry.  The MOA policy reads prev_actions[k] as stored (actions[K - 1] for the bootstrap row,
    whose value does not depend on it).
    CUDA tensors go to the library's forward entry points on torch's current stream, no synchronisation: one or two launches
    of ssd_policy_forward for the whole fragment, K + 1 launches of ssd_policy_lstm_forward / ssd_policy_moa_forward (their
    feature scratch is kept on the policy).  With unchanged weights on a fresh sample(..., state_every=T) they give back
    batch["value"] and batch["last_value"] to the bit.  CPU tensors run the modules' forwards under no_grad.
    one_call=True with CUDA tensors sends a ConvLSTMPolicy or a ConvMOAPolicy through ssd_policy_lstm_forward_seq /
    ssd_policy_moa_forward_seq instead (include/ssd.h, SEQUENCE FORWARD): one library call, the trunk over
    all rows and one cell launch that walks every window, the same bits as the K + 1 launches.  Of the MOA policy only the
    actions branch runs, so "prev_actions" may be missing from the batch then.  Its feature scratch is kept on the policy too
    and is never larger than the scratch of the loss call that follows.  For a ConvFCPolicy and for CPU tensors the keyword
    has no effect."""
    if not isinstance(policy, (ConvFCPolicy, ConvLSTMPolicy, ConvMOAPolicy)):
        raise ValueError("evaluate_fragment is for a ConvFCPolicy, ConvLSTMPolicy or ConvMOAPolicy")
    t, dims, T = _fragment_tensors(policy, batch, obs_first, seq_len, bool(one_call))
    with torch.no_grad():
        if t["actions"].device.type == "cuda":
            if one_call and not isinstance(policy, ConvFCPolicy):
                return _evaluate_device_seq(policy, t, dims, T)
            return _evaluate_device(policy, t, dims, T)
        return _evaluate_host(policy, t, dims, T)


def _impala_targets(policy, batch, obs_first, seq_len, gamma, clip_rho_threshold, clip_pg_rho_threshold, bonus_key=None,
                    bonus_weight=1.0, one_call=False):
    """Steps 1 to 3 of the IMPALA calls -> the batch with "advantages" = pg_advantages and "value_targets" = vs (data)."""
    from .postprocessing import vtrace
    if not isinstance(batch, dict):
        raise ValueError("batch must be the dict sample() returns")
    for key in ("logp", "rew") + ((bonus_key,) if bonus_key else ()):
        if not isinstance(batch.get(key), torch.Tensor):
            raise ValueError("%s is required" % key)
    logits, value, boot = evaluate_fragment(policy, batch, obs_first, seq_len, one_call)
    acts, logp = batch["actions"], batch["logp"]
    if logp.dtype != torch.float32 or tuple(logp.shape) != tuple(acts.shape) or logp.device != acts.device:
        raise ValueError("logp must be a torch.float32 tensor of shape %s on %s" % (tuple(acts.shape), acts.device))
    with torch.no_grad():
        a = acts.long().clamp(0, logits.shape[-1] - 1).unsqueeze(-1)
        logp_target = torch.log_softmax(logits, dim=-1).gather(-1, a).squeeze(-1)      # float32 torch for a float32 policy
        rhos = torch.exp(logp_target - logp).float()
        vs, pg = vtrace(batch["rew"], value.float().contiguous(), rhos, boot.float().contiguous(), batch.get("done"), gamma=gamma,
                        clip_rho_threshold=clip_rho_threshold, clip_pg_rho_threshold=clip_pg_rho_threshold,
                        bonus=batch[bonus_key] if bonus_key else None, bonus_weight=bonus_weight)
    return dict(batch, advantages=pg, value_targets=vs)


def impala_loss(policy, batch, *, gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01, clip_rho_threshold=1.0,
                clip_pg_rho_threshold=1.0, obs_first=None):
    """The reference's IMPALA loss (algorithms/impala_causal.py; RLlib 0.7.6's VTraceLoss) of a ConvFCPolicy on a sampled
    fragment -> (loss, stats), as a3c_loss: -sum logp * pg_advantages + vf_loss_coeff * 0.5 sum (value - vs)^2 - entropy_coeff
    * sum entropy, where vs and pg_advantages are the V-trace targets (stop-gradient data) of the fragment under the policy's
    CURRENT weights.  For a learner whose weights have moved since the fragment was sampled: several passes over one
    fragment, or actors that lag the learner.

        first = env.reset().clone()
        batch = env.sample(policy, 128)
        for _ in range(passes):
            loss, stats = impala_loss(policy, batch, gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01, obs_first=first)
            optimiser.zero_grad(); loss.backward(); clip_grad_by_set_norm(policy, 40.0); optimiser.step()

    The call is (1) evaluate_fragment, (2) logp_target = log_softmax(logits)[a] and rhos = exp(logp_target - batch["logp"]) in
    float32 torch, (3) postprocessing.vtrace(batch["rew"], value, rhos, bootstrap_value, batch["done"], ...), (4) a3c_loss's
    path with advantages = pg_advantages and value_targets = vs; stats are A3C_STATS.  batch: the dict sample() returns, of
    which obs (one row further than a3c_loss reads: the bootstrap's), actions, logp, rew and, where present, done are read;
    the recorded value, last_value, advantages and value_targets are not.  obs_first and minibatches: as ppo_loss.
    One difference from the reference: RLlib cuts the batch into sequences of T rows, drops each sequence's last row from the
    loss and bootstraps from its value; here every row is a loss row and the bootstrap is the current value of the
    observation after the fragment (include/ssd.h, V-TRACE TARGETS).  There is no row mask.
    CUDA tensors stay on the device, on torch's current stream without a host synchronisation."""
    if not isinstance(policy, ConvFCPolicy):
        raise ValueError("impala_loss is for a ConvFCPolicy (impala_loss_recurrent and impala_loss_moa are the other policies')")
    batch = _impala_targets(policy, batch, obs_first, None, gamma, clip_rho_threshold, clip_pg_rho_threshold)
    return a3c_loss(policy, batch, vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff, obs_first=obs_first)


def impala_loss_recurrent(policy, batch, *, seq_len, gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01, clip_rho_threshold=1.0,
                          clip_pg_rho_threshold=1.0, obs_first=None, one_call=False):
    """impala_loss for a ConvLSTMPolicy, with truncated BPTT over windows of seq_len steps as a3c_loss_recurrent -> (loss,
    stats).  The evaluation under the current weights follows the same state rule as the loss (evaluate_fragment): K + 1
    forward launches on the device, or with one_call=True the sequence forward's one call (evaluate_fragment: the same bits).
    The batch's keys ("state", "done") and the minibatch slices are ppo_loss_recurrent's.

        batch = env.sample(policy, 128, state_every=16)
        loss, stats = impala_loss_recurrent(policy, batch, seq_len=16, gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01,
                                            clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0, obs_first=first)"""
    if not isinstance(policy, ConvLSTMPolicy):
        raise ValueError("impala_loss_recurrent is for a ConvLSTMPolicy (impala_loss is the ConvFCPolicy's)")
    batch = _impala_targets(policy, batch, obs_first, seq_len, gamma, clip_rho_threshold, clip_pg_rho_threshold, one_call=one_call)
    return a3c_loss_recurrent(policy, batch, seq_len=seq_len, vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff,
                              obs_first=obs_first)


def impala_loss_moa(policy, batch, *, seq_len, moa_weight, influence_weight=1.0, gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01,
                    clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0, obs_first=None, one_call=False):
    """The causal-influence trainer's IMPALA loss for a ConvMOAPolicy: impala_loss_recurrent's terms + moa_weight * MOALoss as
    a3c_loss_moa -> (loss, stats), stats MOA_A3C_STATS.  The V-trace reward is rew + influence_weight * batch["influence"]
    (the reference's causal_postprocess_trajectory), formed in float64 inside the scan.  The batch's keys ("state", "done",
    "prev_actions", and "influence") and the minibatch slices are ppo_loss_moa's.  one_call: as impala_loss_recurrent (the
    evaluation then runs the actions branch alone; the loss that follows reads prev_actions as before).

        batch = env.sample(policy, 128, state_every=16)
        loss, stats = impala_loss_moa(policy, batch, seq_len=16, moa_weight=10.0, influence_weight=1.0, obs_first=first)"""
    if not isinstance(policy, ConvMOAPolicy):
        raise ValueError("impala_loss_moa is for a ConvMOAPolicy (impala_loss and impala_loss_recurrent are the other policies')")
    batch = _impala_targets(policy, batch, obs_first, seq_len, gamma, clip_rho_threshold, clip_pg_rho_threshold, "influence",
                            influence_weight, one_call=one_call)
    return a3c_loss_moa(policy, batch, seq_len=seq_len, moa_weight=moa_weight, vf_loss_coeff=vf_loss_coeff,
                        entropy_coeff=entropy_coeff, obs_first=obs_first)


def clip_grad_by_set_norm(policy, max_norm):
    """tf.clip_by_global_norm of algorithms/a3c_causal.py:125-131, per weight set and in place on the parameters' .grad: each
    agent's policy is its own graph in the reference, so each set is clipped on its own (torch.nn.utils.clip_grad_norm_ would
    clip over all sets at once).  Set p's gradient is scaled by max_norm / max(norm_p, max_norm), norm_p the 2-norm over every
    parameter's entry that set p reads.  Returns the [P] norms before clipping (the reference's grad_gnorm).  A parameter with
    fewer entries than sets (unpack_gradient's case) counts in the norm of each set that reads it, and is scaled by the smallest
    factor among them.  Parameters without a gradient are skipped."""
    max_norm = float(max_norm)
    if not np.isfinite(max_norm) or max_norm <= 0:
        raise ValueError("max_norm must be finite and > 0")
    P = policy.num_sets
    grads = [g for g in (getattr(policy, name).grad for name, _, _ in policy.layout()) if g is not None]
    if not grads:
        raise ValueError("no parameter of the policy has a gradient")
    sq = torch.zeros(P, dtype=grads[0].dtype, device=grads[0].device)
    for g in grads:
        sq = sq + g.reshape(g.shape[0], -1).square().sum(1).repeat(P // g.shape[0])      # set s reads entry s % entries
    norms = sq.sqrt()
    scale = max_norm / norms.clamp(min=max_norm)
    for g in grads:
        f = scale.reshape(P // g.shape[0], g.shape[0]).min(0).values
        g.mul_(f.reshape((-1,) + (1,) * (g.dim() - 1)))
    return norms


# ---- the Watershed baselines' policy (include/ssd.h, WATERSHED POLICY ROLLOUTS; csrc/ssd_ws_policy.hip) ----

WS_OBS = _capi.SSD_WS_OBS_WIDTH
WS_X = _capi.SSD_WSP_X
WS_OUT = _capi.SSD_WSP_OUT


def ws_is_comm(variant, agent):
    """True where `agent` (ids, scalar or array) is a comm agent: its action is Categorical(5), not the Gaussian."""
    return (int(variant) == _capi.SSD_WS_SEQ_COMM) & (np.asarray(agent) < 4)


def ws_policy_start(variant, rnd, phase):
    """The start rule as a function of the engine's (round, phase) before an action: True where the acting agent acts for the
    first time in its episode, so that the state it uses is zero.  Every agent acts in round 0; a comm agent of SeqComm acts
    there twice, and phases 5-8 are its second message."""
    rnd, phase = np.asarray(rnd), np.asarray(phase)
    first = rnd == 0
    if int(variant) == _capi.SSD_WS_SEQ_COMM:
        first = first & ((phase <= 4) | (phase >= 9))
    return first


def ws_policy_t(variant, rnd, phase):
    """The t of the action draw: round * P + phase - 1 (0 for the first action after a reset)."""
    P = 4 if int(variant) == _capi.SSD_WS_SEQ else 12
    return np.asarray(rnd, np.int64) * P + np.asarray(phase, np.int64) - 1


def sample_gaussian_host(mean, log_std, u1, u2, greedy=False, dtype=np.float32):
    """The rollout's Gaussian action in NumPy (include/ssd.h), float32 as the device computes it (or dtype=np.float64 for the
    same expressions evaluated exactly enough to judge the float32 ones): n = sqrt(-2 log u1) cos(2 pi u2), a = mean + std n
    with std = exp(log_std), logp = -0.5 ((a - mean) / std)^2 - log_std - 0.9189385.  greedy: a = mean.  Returns (a, logp,
    the clipped action min(max(a, 0), 1) the env steps with, a NaN giving 0)."""
    f = np.dtype(dtype).type
    mean, log_std = np.asarray(mean, dtype=dtype), np.asarray(log_std, dtype=dtype)
    sd = np.exp(log_std).astype(dtype)
    if greedy:
        a = mean.copy()
    else:
        u1, u2 = np.asarray(u1, dtype=dtype), np.asarray(u2, dtype=dtype)
        r = np.sqrt((f(-2.0) * np.log(u1).astype(dtype)).astype(dtype)).astype(dtype)
        n = (r * np.cos((f(np.float32(6.2831855)) * u2).astype(dtype)).astype(dtype)).astype(dtype)
        a = (mean + (sd * n).astype(dtype)).astype(dtype)
    z = ((a - mean).astype(dtype) / sd).astype(dtype)
    logp = (((f(-0.5) * (z * z).astype(dtype)).astype(dtype) - log_std).astype(dtype) - f(np.float32(0.9189385))).astype(dtype)
    return a, logp, np.fmin(np.fmax(a, f(0.0)), f(1.0)).astype(dtype)


class WatershedLSTMPolicy(PolicyBase):
    """LSTMFCNet of the reference's Watershed launchers (models/watershed_nets.py:94-177): per agent id its own weight set of
    dense0 (obs -> 16, ReLU), dense1 (16 -> 16, ReLU), a Keras LSTM of cell_size C cells and, on its output, a 5-wide
    distribution head and a value head.  One agent acts per env and phase; a row uses the set of its acting agent.

        policy = WatershedLSTMPolicy(SEQ_COMM, cell_size=128).cuda()         # 8 weight sets
        out = eng.sample(policy, 131)                                        # the closed loop on the device
        dist, value, state = policy(obs, agent, state, starts)               # the same network in torch
        dist, value, final = policy.forward_sequence(5, obs_seq, state_in)   # BPTT over agent 5's own steps

    dist is the input of the action distribution: the five logits of a comm agent's Categorical, or (mean, log_std, 3 unused) of
    an action agent's DiagGaussian.  A state is [..., 2, C]: (h, c); a rollout's carried state is initial_state((E, num_sets)).
    Parameters in Keras' layouts with a leading weight-set axis: dense0_w [S, 12, 16] (the rows beyond an agent's observation
    length meet the zero padding of the engine's rows), dense0_b, dense1_w [S, 16, 16], dense1_b, lstm_kernel [S, 16, 4C],
    lstm_recurrent [S, C, 4C], lstm_bias [S, 4C], out_w [S, C, 5], out_b, value_w [S, C, 1], value_b.  share_comm_layer: dense1
    of agents k and k + 4 is ONE layer (the reference's shared_layers[id % 4]): dense1_w / dense1_b have 4 entries, and packed()
    writes each into both sets."""
    STATE_ROWS = 2
    REF_PARAM = "dense0_w"
    C_FORWARD, C_ROLLOUT = "ssd_ws_policy_forward", "ssd_ws_rollout_policy"

    def __init__(self, variant, local_obs=False, cell_size=128, share_comm_layer=False, seed=0):
        super().__init__()
        from .watershed import obs_len
        V, C = int(variant), int(cell_size)
        if V not in (_capi.SSD_WS_SEQ, _capi.SSD_WS_SEQ_COMM):
            raise ValueError("variant must be SEQ or SEQ_COMM")
        self._check_ranges(cell_size=C)
        S = 4 if V == _capi.SSD_WS_SEQ else 8
        self.variant, self.local_obs, self.cell_size, self.num_sets = V, bool(local_obs), C, S
        self.share_comm_layer = bool(share_comm_layer)
        self.num_dense1 = 4 if self.share_comm_layer else S
        self.obs_lens = tuple(obs_len(V, self.local_obs, i) for i in range(S))
        g = torch.Generator().manual_seed(int(seed))
        d0 = torch.zeros((S, WS_OBS, WS_X), dtype=torch.float64)
        for i, n in enumerate(self.obs_lens):                    # Keras' Glorot uniform on the [n, 16] kernel the agent has
            d0[i, :n] = _glorot((n, WS_X), n, WS_X, g)
        self._register({"dense0_w": d0, "dense1_w": normc((self.num_dense1, WS_X, WS_X), 1.0, g),
                        "lstm_kernel": _glorot((S, WS_X, 4 * C), WS_X, 4 * C, g), "lstm_recurrent": _orthogonal(S, C, 4 * C, g),
                        "out_w": _glorot((S, C, WS_OUT), C, WS_OUT, g), "value_w": _glorot((S, C, 1), C, 1, g)})

    def _entries(self, name):
        return self.num_dense1 if name.startswith("dense1") else self.num_sets

    def layout(self):
        """(name, shape of one set, float offset within a packed set) of every parameter, in packed order."""
        C = self.cell_size
        lw = _capi.SSD_WSP_LSTM_W
        return (("dense0_w", (WS_OBS, WS_X), _capi.SSD_WSP_D0_W), ("dense0_b", (WS_X,), _capi.SSD_WSP_D0_B),
                ("dense1_w", (WS_X, WS_X), _capi.SSD_WSP_D1_W), ("dense1_b", (WS_X,), _capi.SSD_WSP_D1_B),
                ("lstm_kernel", (WS_X, 4 * C), lw), ("lstm_recurrent", (C, 4 * C), lw + WS_X * 4 * C),
                ("lstm_bias", (4 * C,), _capi.SSD_WSP_LSTM_B(C)),
                ("out_w", (C, WS_OUT), _capi.SSD_WSP_OUT_W(C)), ("out_b", (WS_OUT,), _capi.SSD_WSP_OUT_B(C)),
                ("value_w", (C, 1), _capi.SSD_WSP_VALUE_W(C)), ("value_b", (1,), _capi.SSD_WSP_VALUE_B(C)))

    @property
    def set_floats(self):
        return _capi.SSD_WSP_SET_FLOATS(self.cell_size)

    def _set(self, name, i):
        """Parameter `name` of agent id i (a shared dense1 is entry i % 4)."""
        t = getattr(self, name)
        return t[i % t.shape[0]]

    def _cell(self, i, x, h, c):
        """Set i on rows x [M, 12], (h, c) [M, C] -> (dist [M, 5], value [M], h', c')."""
        d0 = torch.relu(x @ self._set("dense0_w", i) + self._set("dense0_b", i))
        d1 = torch.relu(d0 @ self._set("dense1_w", i) + self._set("dense1_b", i))
        h2, c2 = keras_lstm(d1, h, c, self.lstm_kernel[i], self.lstm_recurrent[i], self.lstm_bias[i])
        return h2 @ self.out_w[i] + self.out_b[i], (h2 @ self.value_w[i] + self.value_b[i])[..., 0], h2, c2

    def forward(self, obs, agent, state, starts=None):
        """obs [..., 12], agent int [...] (the acting agent of each row, ids may mix), state [..., 2, C] (each row's OWN state:
        that of its acting agent), starts bool [...] or None: rows whose state is taken as zero (selected: whatever it holds is
        never used).  Returns (dist [..., 5], value [...], new state [..., 2, C]).  A row whose agent is no id of this variant
        gets zeros and keeps its state.  (The rows of each id are gathered by index, which synchronises with the device.)"""
        C = self.cell_size
        lead = tuple(agent.shape)
        if tuple(obs.shape) != lead + (WS_OBS,) or tuple(state.shape) != lead + (2, C):
            raise ValueError("obs must be %s and state %s, got %s and %s" % (lead + (WS_OBS,), lead + (2, C), tuple(obs.shape),
                                                                              tuple(state.shape)))
        dt = self.dense0_w.dtype
        x, st, ag = obs.to(dt).reshape(-1, WS_OBS), state.to(dt).reshape(-1, 2, C), agent.reshape(-1).long()
        new_state = st
        if starts is not None:
            if tuple(starts.shape) != lead:
                raise ValueError("starts must have shape %s, got %s" % (lead, tuple(starts.shape)))
            st = _zero_where(starts, st, 2)
        M = x.shape[0]
        dist = torch.zeros((M, WS_OUT), dtype=dt, device=x.device)
        value = torch.zeros((M,), dtype=dt, device=x.device)
        for i in range(self.num_sets):
            idx = torch.nonzero(ag == i)[:, 0]
            if idx.numel() == 0:
                continue
            d, v, h2, c2 = self._cell(i, x[idx], st[idx, 0], st[idx, 1])
            dist = dist.index_copy(0, idx, d)
            value = value.index_copy(0, idx, v)
            new_state = new_state.index_copy(0, idx, torch.stack([h2, c2], dim=1))
        return dist.reshape(lead + (WS_OUT,)), value.reshape(lead), new_state.reshape(lead + (2, C))

    def forward_sequence(self, agent_id, obs, state, resets=None):
        """T of agent agent_id's own steps for truncated BPTT: obs [T, ..., 12] (the observations it acted on, in order), state
        [..., 2, C] before step 0, resets bool [T, ...] or None (resets[t]: the state step t uses is zero, as the start rule).
        Differentiable.  Returns (dist [T, ..., 5], value [T, ...], the state after step T - 1)."""
        i, C, T = int(agent_id), self.cell_size, int(obs.shape[0])
        if not 0 <= i < self.num_sets:
            raise ValueError("agent_id must be 0..%d" % (self.num_sets - 1))
        if resets is not None and int(resets.shape[0]) != T:
            raise ValueError("resets must have T = %d rows" % T)
        lead = tuple(obs.shape[1:-1])
        dt = self.dense0_w.dtype
        st = state.to(dt).reshape(-1, 2, C)

        def step(t, hc, reset):
            h, c = hc if reset is None else (_zero_where(reset, hc[0], 1), _zero_where(reset, hc[1], 1))
            d, v, h, c = self._cell(i, obs[t].to(dt).reshape(-1, WS_OBS), h, c)
            return d.reshape(lead + (WS_OUT,)), v.reshape(lead), (h, c)
        dists, values, hc = _unroll(step, T, (st[:, 0], st[:, 1]), resets)
        return dists, values, torch.stack(hc, dim=1).reshape(lead + (2, C))


# ---- the PPO loss for the Watershed policy, one agent id a call (include/ssd.h, WATERSHED PPO LOSS AND GRADIENTS) ----

def ws_ppo_terms(dist, value, t, is_comm, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """RLlib 0.7.6's PPO loss per row for a Watershed head in plain torch, in the dtype of dist: (row_loss, -surr, vf, kl, ent),
    each of actions' shape.  dist [..., 5], value [...]; t: actions, logp_old, advantages, value_targets, vf_pred and, for the
    KL term, behaviour_dist.  is_comm: Categorical over the 5 outputs (ppo_terms with A = 5; actions hold the message index),
    else a one-dimensional DiagGaussian with mean = dist[..., 0], log_std = dist[..., 1] (actions hold the unclipped sample):
    logp = -0.5 z^2 - log_std - 0.9189385 with z = (a - mean) / exp(log_std), entropy = log_std + 1.4189385 and
    kl = log_std - log_std_old + (exp(2 log_std_old) + (mean_old - mean)^2) / (2 exp(2 log_std)) - 0.5 (the behaviour's against
    the current one, RLlib's prev_dist.kl(curr_dist))."""
    dt = dist.dtype
    if is_comm:
        tt = dict(t)
        tt["actions"] = t["actions"].to(torch.int64).clamp(0, WS_OUT - 1)
        tt["behaviour_logits"] = t.get("behaviour_dist")
        return ppo_terms(dist, value, tt, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff)
    mean, log_std = dist[..., 0], dist[..., 1]
    z = (t["actions"].to(dt) - mean) / torch.exp(log_std)
    logp = -0.5 * (z * z) - log_std - torch.tensor(np.float32(0.9189385), dtype=dt)
    ent = log_std + torch.tensor(np.float32(1.4189385), dtype=dt)
    adv, vt, vfp = t["advantages"].to(dt), t["value_targets"].to(dt), t["vf_pred"].to(dt)
    ratio = torch.exp(logp - t["logp_old"].to(dt))
    surr = torch.minimum(adv * ratio, adv * ratio.clamp(1.0 - clip_param, 1.0 + clip_param))
    if t.get("behaviour_dist") is not None:
        b = t["behaviour_dist"].to(dt)
        kl = (log_std - b[..., 1]) + 0.5 * (torch.exp(2.0 * b[..., 1]) + (b[..., 0] - mean).square()) / torch.exp(2.0 * log_std) - 0.5
    else:
        kl = torch.zeros_like(ent)
    vf1 = (value - vt).square()
    vf2 = (vfp + (value - vfp).clamp(-vf_clip_param, vf_clip_param) - vt).square()
    vf = torch.maximum(vf1, vf2)
    return -surr + kl_coeff * kl + vf_loss_coeff * vf - entropy_coeff * ent, -surr, vf, kl, ent


_WS_PPO_KEYS = (("obs", ("obs",)), ("actions", ("actions",)), ("logp_old", ("logp_old", "logp")), ("advantages", ("advantages",)),
                ("value_targets", ("value_targets",)), ("vf_pred", ("vf_pred", "value")),
                ("behaviour_dist", ("behaviour_dist", "dist")), ("starts", ("starts",)), ("state", ("state",)))


def _ws_ppo_tensors(policy, seq, seq_len, kl_coeff, a3c=False):
    """The Watershed loss's inputs by their contract names from a dict of [M, Q, ...] tensors, checked against each other.
    a3c: the A3C loss's inputs -- logp_old, vf_pred and behaviour_dist are not looked at (None)."""
    if not isinstance(seq, dict):
        raise ValueError("seq must be a dict of [M, Q, ...] tensors")
    t = {name: next((seq[k] for k in keys if seq.get(k) is not None), None) for name, keys in _WS_PPO_KEYS}
    if a3c:
        t["logp_old"] = t["vf_pred"] = t["behaviour_dist"] = None
    acts = t["actions"]
    if not isinstance(acts, torch.Tensor) or acts.dim() != 2 or acts.numel() == 0:
        raise ValueError("actions must be a float32 tensor [M, Q]")
    M, Q = (int(n) for n in acts.shape)
    C, T, dev = policy.cell_size, int(seq_len), acts.device
    if M * Q > 2 ** 31 - 17:
        raise ValueError("the sequences must have at most 2^31 - 17 rows")
    if float(kl_coeff) == 0.0:
        t["behaviour_dist"] = None                           # not part of the loss
    elif t["behaviour_dist"] is None:
        raise ValueError("kl_coeff != 0 needs dist (the dist the actions were sampled from)")
    for name in ("actions",) + (_A3C_ROWS if a3c else ("logp_old", "advantages", "value_targets", "vf_pred")):
        _check_tensor(t[name], torch.float32, (M, Q), name, dev)
    _check_tensor(t["obs"], torch.float32, (M, Q, WS_OBS), "obs", dev)
    if t["behaviour_dist"] is not None:
        _check_tensor(t["behaviour_dist"], torch.float32, (M, Q, WS_OUT), "dist", dev)
    if t["starts"] is not None:
        if t["starts"].dtype == torch.bool:
            t["starts"] = t["starts"].to(torch.uint8)
        _check_tensor(t["starts"], torch.uint8, (M, Q), "starts", dev)
    S = -(-M // T)
    st = t["state"]
    if not isinstance(st, torch.Tensor) or st.dim() != 4 or st.shape[0] < S or tuple(st.shape[1:]) != (Q, 2, C):
        raise ValueError("state must be [S, %d, 2, %d] with S >= ceil(M / seq_len) = %d" % (Q, C, S))
    _check_tensor(st, torch.float32, tuple(st.shape), "state", dev)
    return t, (M, Q)


def ws_forward_windows(policy, agent_id, obs, state, starts, seq_len, return_state=False):
    """The learner's forward of a WatershedLSTMPolicy over one agent's sequences, in plain torch under autograd, by the state
    rule of include/ssd.h: obs [M, Q, 12], state [S, Q, 2, C] (detached: data), starts u8/bool [M, Q] or None -> (dist [M, Q, 5],
    value [M, Q]), and with return_state the state [Q, 2, C] after step M - 1.  Window by window through forward_sequence;
    starts at a window's first step are not looked at."""
    M, T = int(obs.shape[0]), int(seq_len)
    dt = policy.dense0_w.dtype
    dists, values = [], []
    for w, m0 in enumerate(range(0, M, T)):
        m1 = min(m0 + T, M)
        resets = None
        if starts is not None and m1 - m0 > 1:
            resets = torch.cat([torch.zeros_like(starts[:1]), starts[m0 + 1:m1]]).to(torch.bool)
        d, v, last = policy.forward_sequence(agent_id, obs[m0:m1], state[w].detach().to(dt), resets)
        dists.append(d)
        values.append(v)
    if return_state:
        return torch.cat(dists), torch.cat(values), last
    return torch.cat(dists), torch.cat(values)


def _ws_agent(name, policy, agent_id):
    """The policy and the agent id of a Watershed call `name`, checked -> the id as an int."""
    if not isinstance(policy, WatershedLSTMPolicy):
        raise ValueError("%s is for a WatershedLSTMPolicy" % name)
    if isinstance(agent_id, bool) or int(agent_id) != agent_id or not 0 <= int(agent_id) < policy.num_sets:
        raise ValueError("agent_id must be 0..%d" % (policy.num_sets - 1))
    return int(agent_id)


def _ws_loss_prepare(name, policy, agent_id, seq, seq_len, hyper, a3c):
    """The checks the Watershed loss functions share, in the PPO call's order -> (agent_id, seq_len, hyper, t, (M, Q), dev).
    hyper: the PPO call's five, or (vf_loss_coeff, entropy_coeff) of the A3C call."""
    agent_id = _ws_agent(name, policy, agent_id)
    seq_len = _check_seq_len(seq_len)
    hyper = tuple(float(x) for x in hyper)
    _check_hyper(hyper, clips=not a3c)
    t, dims = _ws_ppo_tensors(policy, seq, seq_len, 0.0 if a3c else hyper[4], a3c=a3c)
    dev = t["actions"].device
    _check_same_device(policy, dev, "sequences")
    _check_float32(policy, dev)
    return agent_id, seq_len, hyper, t, dims, dev


def ppo_loss_watershed(policy, agent_id, seq, *, seq_len, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """RLlib 0.7.6's PPO loss of ONE agent id of a WatershedLSTMPolicy on that agent's own steps, with truncated backpropagation
    through time over windows of seq_len steps -> (loss, stats): loss a scalar tensor that backpropagates into row agent_id of
    every parameter (every other row's gradient is exactly zero; a shared dense1 gets entry agent_id % 4), stats a dict of
    scalar tensors (PPO_STATS).  In the reference each agent's policy has its own loss, so a learner makes one call per id.
    include/ssd.h (WATERSHED PPO LOSS AND GRADIENTS) states the rows, the state rule and the two heads' terms.

        loss, stats = ppo_loss_watershed(policy, 5, seq, seq_len=16, clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4,
                                         entropy_coeff=1e-3, kl_coeff=0.0)
        loss.backward(); optimiser.step()

    seq: a dict of tensors over the agent's M own steps of Q sequences (one env's trajectory each), gathered by the caller:
    obs f32 [M,Q,12] (the observation each step acted on), actions f32 [M,Q] (the message index for a comm agent, the unclipped
    Gaussian sample for an action agent: what sample() records), logp (or logp_old), advantages, value_targets, value (or
    vf_pred) f32 [M,Q], state f32 [ceil(M / seq_len),Q,2,C] (the (h, c) each window starts from), optionally dist (or
    behaviour_dist) f32 [M,Q,5] (needed if kl_coeff != 0) and starts u8 or bool [M,Q] (the state step m uses is zero; not looked
    at where m is a window's first step, whose state is the recorded one).  Which reward is credited to which step is the
    caller's choice: advantages and value_targets are inputs (compute_advantages accepts any [R, L] tensors).
    CUDA tensors go to the library (ssd_ws_policy_ppo_grad on torch's current stream, no synchronisation; the scratch is kept
    on the policy); CPU tensors run forward_sequence per window and ws_ppo_terms under autograd."""
    hyper = (clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff)
    agent_id, seq_len, hyper, t, (M, Q), dev = _ws_loss_prepare("ppo_loss_watershed", policy, agent_id, seq, seq_len, hyper, False)
    if dev.type == "cuda":
        return _device_loss(policy, (WatershedLSTMPolicy, "ppo"), t, (M, Q), seq_len, hyper, only_set=agent_id)
    _check_device_type(dev)
    dist, value = ws_forward_windows(policy, agent_id, t["obs"], t["state"], t["starts"], seq_len)
    terms = ws_ppo_terms(dist, value, t, bool(ws_is_comm(policy.variant, agent_id)), *hyper)
    means = [x.mean() for x in terms]
    return means[0], {name: m.detach() for name, m in zip(PPO_STATS, means)}


# ---- the A3C and the IMPALA loss for the Watershed policy (include/ssd.h, WATERSHED A3C LOSS AND GRADIENTS and WATERSHED
# ---- SEQUENCE FORWARD) ----

def ws_logp(dist, actions, is_comm):
    """The log-probability of the taken actions under dist [..., 5] in plain torch, in the dtype of dist: the Categorical's
    log_softmax(dist)[a] with the message index clamped to 0 .. 4 for a comm agent, else the Gaussian's
    -0.5 z^2 - log_std - 0.9189385 with z = (a - mean) / exp(log_std) on the unclipped sample."""
    dt = dist.dtype
    if is_comm:
        a = actions.to(torch.int64).clamp(0, WS_OUT - 1).unsqueeze(-1)
        return torch.log_softmax(dist, dim=-1).gather(-1, a).squeeze(-1)
    mean, log_std = dist[..., 0], dist[..., 1]
    z = (actions.to(dt) - mean) / torch.exp(log_std)
    return -0.5 * (z * z) - log_std - torch.tensor(np.float32(0.9189385), dtype=dt)


def ws_a3c_terms(dist, value, t, is_comm, vf_loss_coeff, entropy_coeff):
    """The reference's A3C loss (algorithms/a3c_causal.py:28-46) per row for a Watershed head in plain torch, in the dtype of
    dist: (row_loss, pi, vf, ent), each of actions' shape.  dist [..., 5], value [...]; t: actions, advantages and value_targets.
    is_comm: Categorical over the 5 outputs (a3c_terms with A = 5; actions hold the message index), else the one-dimensional
    DiagGaussian of ws_ppo_terms: logp as ws_logp, entropy = log_std + 1.4189385."""
    if is_comm:
        return a3c_terms(dist, value, t, vf_loss_coeff, entropy_coeff)
    dt = dist.dtype
    logp = ws_logp(dist, t["actions"], False)
    ent = dist[..., 1] + torch.tensor(np.float32(1.4189385), dtype=dt)
    pi = -(logp * t["advantages"].to(dt))
    vf = 0.5 * (value - t["value_targets"].to(dt)).square()
    return (pi + vf_loss_coeff * vf) - entropy_coeff * ent, pi, vf, ent


def a3c_loss_watershed(policy, agent_id, seq, *, seq_len, vf_loss_coeff, entropy_coeff):
    """The reference's A3C loss (algorithms/a3c_causal.py:28-46; every Watershed launcher offers it next to PPO) of ONE agent id
    of a WatershedLSTMPolicy on that agent's own steps, with truncated backpropagation through time over windows of seq_len
    steps -> (loss, stats), as ppo_loss_watershed: loss a scalar tensor that backpropagates into row agent_id of every
    parameter, stats a dict of scalar tensors (A3C_STATS: the SUMS over the M Q rows of the total, policy, value-function and
    entropy terms).  Per row -logp * adv + vf_loss_coeff * 0.5 (value - vt)^2 - entropy_coeff * ent, summed, not averaged
    (include/ssd.h, WATERSHED A3C LOSS AND GRADIENTS).

        adv, vt = compute_advantages(rew, value, last_value, done, gamma=0.99, use_gae=False, bonus=...)
        loss, stats = a3c_loss_watershed(policy, 5, dict(seq, advantages=adv, value_targets=vt), seq_len=16,
                                         vf_loss_coeff=0.5, entropy_coeff=0.01)
        loss.backward(); clip_grad_by_set_norm(policy, 40.0); optimiser.step()

    seq: ppo_loss_watershed's dict, of which obs, actions, advantages, value_targets, state and, where present, starts are
    read; logp, value and dist are ignored.  The state rule and the argument checks are ppo_loss_watershed's.
    CUDA tensors go to the library (ssd_ws_policy_ac_grad on torch's current stream, no synchronisation; the scratch is the
    PPO call's); CPU tensors run forward_sequence per window and ws_a3c_terms under autograd."""
    agent_id, seq_len, hyper, t, (M, Q), dev = _ws_loss_prepare("a3c_loss_watershed", policy, agent_id, seq, seq_len,
                                                                (vf_loss_coeff, entropy_coeff), True)
    if dev.type == "cuda":
        return _device_loss(policy, (WatershedLSTMPolicy, "a3c"), t, (M, Q), seq_len, hyper, only_set=agent_id)
    _check_device_type(dev)
    dist, value = ws_forward_windows(policy, agent_id, t["obs"], t["state"], t["starts"], seq_len)
    sums = [x.sum() for x in ws_a3c_terms(dist, value, t, bool(ws_is_comm(policy.variant, agent_id)), *hyper)]
    return sums[0], {name: x.detach() for name, x in zip(A3C_STATS, sums)}


def _ws_eval_tensors(policy, seq, seq_len):
    """What evaluate_sequences reads of a dict of [M, Q, ...] tensors, checked against each other -> (t, (M, Q))."""
    if not isinstance(seq, dict):
        raise ValueError("seq must be a dict of [M, Q, ...] tensors")
    t = {name: seq.get(name) for name in ("obs", "actions", "state", "starts", "obs_next", "start_next")}
    acts = t["actions"]
    if not isinstance(acts, torch.Tensor) or acts.dim() != 2 or acts.numel() == 0:
        raise ValueError("actions must be a float32 tensor [M, Q]")
    M, Q = (int(n) for n in acts.shape)
    C, T, dev = policy.cell_size, int(seq_len), acts.device
    if (M + 1) * Q > 2 ** 31 - 17:
        raise ValueError("the sequences must have at most 2^31 - 17 rows, the bootstrap's included")
    _check_tensor(acts, torch.float32, (M, Q), "actions", dev)
    _check_tensor(t["obs"], torch.float32, (M, Q, WS_OBS), "obs", dev)
    for name, shape in (("starts", (M, Q)), ("start_next", (Q,))):
        if t[name] is not None:
            if isinstance(t[name], torch.Tensor) and t[name].dtype == torch.bool:
                t[name] = t[name].to(torch.uint8)
            _check_tensor(t[name], torch.uint8, shape, name, dev)
    if t["obs_next"] is not None:
        _check_tensor(t["obs_next"], torch.float32, (Q, WS_OBS), "obs_next", dev)
    elif t["start_next"] is not None:
        raise ValueError("start_next needs obs_next")
    S = -(-M // T)
    st = t["state"]
    if not isinstance(st, torch.Tensor) or st.dim() != 4 or st.shape[0] < S or tuple(st.shape[1:]) != (Q, 2, C):
        raise ValueError("state must be [S, %d, 2, %d] with S >= ceil(M / seq_len) = %d" % (Q, C, S))
    _check_tensor(st, torch.float32, tuple(st.shape), "state", dev)
    return t, (M, Q)


def evaluate_sequences(policy, agent_id, seq, seq_len):
    """One agent id's sequences under the policy's CURRENT weights -> (dist [M,Q,5], value [M,Q], logp [M,Q], bootstrap_value
    [Q] or None), without gradient: what V-trace needs of the target policy (postprocessing.vtrace) when the weights have moved
    since sample() ran.  The Watershed counterpart of evaluate_fragment, on the rows ppo_loss_watershed takes.

    seq: obs f32 [M,Q,12], actions f32 [M,Q], state f32 [ceil(M / seq_len),Q,2,C], optionally starts u8 or bool [M,Q] (the loss
    calls' state rule), obs_next f32 [Q,12] (the observation after the last own step) and start_next u8 or bool [Q].  logp is
    the log-probability of actions under dist (ws_logp's expressions).  bootstrap_value is the value of obs_next under the state
    step M - 1 computed, zero where start_next, never a state entry; without obs_next it is None.
    CUDA tensors go to the library: ssd_ws_policy_forward_seq, ONE launch on torch's current stream for all M steps and the
    bootstrap, no scratch and no synchronisation; with unchanged weights on a fresh sample()'s rows of the id it gives back
    the recorded dist, value and logp to the bit.  CPU tensors run ws_forward_windows and one forward step under no_grad."""
    agent_id = _ws_agent("evaluate_sequences", policy, agent_id)
    seq_len = _check_seq_len(seq_len)
    t, (M, Q) = _ws_eval_tensors(policy, seq, seq_len)
    dev = t["actions"].device
    _check_same_device(policy, dev, "sequences")
    _check_device_type(dev)
    _check_float32(policy, dev)
    is_comm = bool(ws_is_comm(policy.variant, agent_id))
    with torch.no_grad():
        if dev.type == "cuda":
            dist = torch.empty((M, Q, WS_OUT), dtype=torch.float32, device=dev)
            value, logp = (torch.empty((M, Q), dtype=torch.float32, device=dev) for _ in range(2))
            boot = None if t["obs_next"] is None else torch.empty((Q,), dtype=torch.float32, device=dev)
            ptr, index, stream = _device_handles(dev)
            rc = _capi.lib().ssd_ws_policy_forward_seq(ptr(policy.packed()), policy.num_sets, policy.cell_size, policy.variant,
                                                       agent_id, seq_len, ptr(t["obs"]), ptr(t["state"]), ptr(t["starts"]),
                                                       ptr(t["actions"]), ptr(t["obs_next"]), ptr(t["start_next"]), M, Q,
                                                       ptr(dist), ptr(value), ptr(logp), ptr(boot), None, index, 0, stream)
            _capi.policy_check(rc)
            return dist, value, logp, boot
        dist, value, last = ws_forward_windows(policy, agent_id, t["obs"], t["state"], t["starts"], seq_len, return_state=True)
        boot = None
        if t["obs_next"] is not None:
            agent = torch.full((Q,), agent_id, dtype=torch.int64)
            starts = None if t["start_next"] is None else t["start_next"].to(torch.bool)
            boot = policy(t["obs_next"], agent, last, starts)[1]
        return dist, value, ws_logp(dist, t["actions"], is_comm), boot


def impala_loss_watershed(policy, agent_id, seq, *, seq_len, gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01,
                          clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0):
    """The reference's IMPALA loss (algorithms/impala_causal.py:79-143; RLlib 0.7.6's VTraceLoss, which takes
    action_dist.logp(actions) and the recorded behaviour_action_logp and so serves the Box actions of the action agents as well
    as the comm agents' messages) of ONE agent id of a WatershedLSTMPolicy -> (loss, stats), as a3c_loss_watershed:
    -sum logp * pg_advantages + vf_loss_coeff * 0.5 sum (value - vs)^2 - entropy_coeff * sum entropy, where vs and
    pg_advantages are the V-trace targets (stop-gradient data) of the sequences under the policy's CURRENT weights.

        for _ in range(passes):
            loss, stats = impala_loss_watershed(policy, 5, seq, seq_len=16, gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01)
            optimiser.zero_grad(); loss.backward(); clip_grad_by_set_norm(policy, 40.0); optimiser.step()

    The call is (1) evaluate_sequences, (2) rhos = exp(logp - seq["logp"]) in float32 torch, (3) postprocessing.vtrace(zero
    int32 rewards, value, rhos, bootstrap_value, seq["done"], bonus=seq["rew"], bonus_weight=1.0, ...): the float rewards go
    through vtrace's bonus input, the one examples/ppo_train_watershed.py gives compute_advantages, (4) a3c_loss_watershed
    with advantages = pg_advantages and value_targets = vs; stats are A3C_STATS.
    seq: a3c_loss_watershed's dict (advantages and value_targets are not read) and logp f32 [M,Q] (the behaviour policy's, as
    sample() records it), rew f32 [M,Q] (the reward credited to own step m: the caller's choice), done u8 [M,Q] (the episode
    ended after own step m), obs_next f32 [Q,12] and optionally start_next u8 [Q] (default done[M - 1]).
    One difference from the reference, as with the other IMPALA calls: RLlib cuts the batch into sequences of T rows, drops
    each sequence's last row from the loss (drop_last) and bootstraps from its value; here every row is a loss row and the
    bootstrap is the current value of obs_next (include/ssd.h, V-TRACE TARGETS).  There is no row mask.
    CUDA tensors stay on the device, on torch's current stream without a host synchronisation."""
    from .postprocessing import vtrace
    _ws_agent("impala_loss_watershed", policy, agent_id)
    if not isinstance(seq, dict):
        raise ValueError("seq must be a dict of [M, Q, ...] tensors")
    for key in ("logp", "rew", "done", "obs_next"):
        if not isinstance(seq.get(key), torch.Tensor):
            raise ValueError("%s is required" % key)
    done = seq["done"].to(torch.uint8) if seq["done"].dtype == torch.bool else seq["done"]
    acts = seq.get("actions")
    if seq.get("start_next") is None and isinstance(acts, torch.Tensor) and tuple(done.shape) == tuple(acts.shape) and acts.dim() == 2 \
            and acts.numel() and done.dtype == torch.uint8:
        seq = dict(seq, start_next=done[-1].contiguous())     # (a done of another shape is refused below, by its name)
    dist, value, logp, boot = evaluate_sequences(policy, agent_id, seq, seq_len)
    shape, dev = tuple(value.shape), value.device
    _check_tensor(seq["logp"], torch.float32, shape, "logp", dev)
    _check_tensor(seq["rew"], torch.float32, shape, "rew", dev)
    _check_tensor(done, torch.uint8, shape, "done", dev)
    with torch.no_grad():
        rhos = torch.exp(logp.float() - seq["logp"])                  # float32 torch for a float32 policy
        vs, pg = vtrace(torch.zeros(shape, dtype=torch.int32, device=dev), value.float().contiguous(), rhos,
                        boot.float().contiguous(), done, gamma=gamma, clip_rho_threshold=clip_rho_threshold,
                        clip_pg_rho_threshold=clip_pg_rho_threshold, bonus=seq["rew"], bonus_weight=1.0)
    return a3c_loss_watershed(policy, agent_id, dict(seq, advantages=pg, value_targets=vs), seq_len=seq_len,
                              vf_loss_coeff=vf_loss_coeff, entropy_coeff=entropy_coeff)


# ---- the device path of the eleven loss calls and of evaluate_fragment: one record of what to call, one torch function ----

def _device_handles(dev):
    """What a library call on torch's current stream of `dev` needs besides its own arguments: (ptr: the address of a tensor,
    or NULL for None; the device index; the stream handle)."""
    import ctypes as C
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    return ptr, index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# (policy class, loss) -> (the entry point, its arguments up to `scratch` in the order and by the names of include/ssd.h -- but
# vf_pred, the contract name, for vf_preds --, broken into lines where the header breaks them; the columns of its stats).  After
# them every entry point takes scratch, grads, stats, device_id, flags and stream.  A name stands for the call's tensor or number
# of that name, else for the policy's attribute.
_LOSS_CALLS = {
    (ConvFCPolicy, "ppo"): ("ssd_policy_ppo_grad",
                            "weights num_sets num_actions obs_first obs "
                            "actions logp_old advantages value_targets "
                            "vf_pred behaviour_logits n_steps num_envs "
                            "num_agents clip_param vf_clip_param vf_loss_coeff entropy_coeff "
                            "kl_coeff", PPO_STATS),
    (ConvLSTMPolicy, "ppo"): ("ssd_policy_lstm_ppo_grad",
                              "weights num_sets num_actions cell_size seq_len "
                              "obs_first obs state done "
                              "actions logp_old advantages value_targets "
                              "vf_pred behaviour_logits n_steps num_envs "
                              "num_agents clip_param vf_clip_param vf_loss_coeff "
                              "entropy_coeff kl_coeff", PPO_STATS),
    (ConvMOAPolicy, "ppo"): ("ssd_policy_moa_ppo_grad",
                             "weights num_sets num_actions cell_size seq_len "
                             "obs_first obs state prev_actions "
                             "done actions logp_old advantages "
                             "value_targets vf_pred behaviour_logits n_steps "
                             "num_envs num_agents clip_param vf_clip_param vf_loss_coeff "
                             "entropy_coeff kl_coeff moa_weight", MOA_PPO_STATS),
    (ConvFCPolicy, "a3c"): ("ssd_policy_ac_grad",
                            "weights num_sets num_actions obs_first obs "
                            "actions advantages value_targets n_steps "
                            "num_envs num_agents vf_loss_coeff entropy_coeff", A3C_STATS),
    (ConvLSTMPolicy, "a3c"): ("ssd_policy_lstm_ac_grad",
                              "weights num_sets num_actions cell_size seq_len "
                              "obs_first obs state done "
                              "actions advantages value_targets n_steps "
                              "num_envs num_agents vf_loss_coeff entropy_coeff", A3C_STATS),
    (ConvMOAPolicy, "a3c"): ("ssd_policy_moa_ac_grad",
                             "weights num_sets num_actions cell_size seq_len "
                             "obs_first obs state prev_actions "
                             "done actions advantages value_targets "
                             "n_steps num_envs num_agents vf_loss_coeff entropy_coeff "
                             "moa_weight", MOA_A3C_STATS),
    (WatershedLSTMPolicy, "ppo"): ("ssd_ws_policy_ppo_grad",
                                   "weights num_sets cell_size variant agent_id "
                                   "seq_len obs state starts actions "
                                   "logp_old advantages value_targets vf_pred "
                                   "behaviour_dist n_steps num_seqs clip_param "
                                   "vf_clip_param vf_loss_coeff entropy_coeff kl_coeff", PPO_STATS),
    (WatershedLSTMPolicy, "a3c"): ("ssd_ws_policy_ac_grad",
                                   "weights num_sets cell_size variant agent_id "
                                   "seq_len obs state starts actions "
                                   "advantages value_targets n_steps num_seqs "
                                   "vf_loss_coeff entropy_coeff", A3C_STATS)}
_LOSS_CALLS = {key: (symbol, tuple(names.split()), stats) for key, (symbol, names, stats) in _LOSS_CALLS.items()}
_HYPER = {"ppo": ("clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff", "moa_weight"),
          "a3c": ("vf_loss_coeff", "entropy_coeff", "moa_weight")}


# One call of a loss-and-gradient entry point: its symbol, its arguments up to `scratch` (tensors and numbers, in the entry
# point's order), the float32 scratch it needs, the shapes of its grads and stats, and only_set: the one weight set whose
# gradient grads [set_floats] is (the Watershed call's agent id), or None for grads [P, set_floats].
_LossCall = collections.namedtuple("_LossCall", "symbol args scratch_floats grads_shape stats_shape only_set")


class _LossFunction(torch.autograd.Function):
    """A loss-and-gradient entry point as a torch function of the policy's parameters: forward enqueues the library's launches
    on the current stream and keeps the packed gradient, backward scatters it into the parameters' shapes by layout()."""

    @staticmethod
    def forward(ctx, policy, call, *params):
        dev = call.args[0].device
        scratch = getattr(policy, "_ppo_scratch", None)          # kept between calls, as packed()'s buffer is: one buffer
        if scratch is None or scratch.device != dev or scratch.numel() < call.scratch_floats:      # serves every loss call
            scratch = policy._ppo_scratch = torch.empty(call.scratch_floats, dtype=torch.float32, device=dev)
        grads = torch.empty(call.grads_shape, dtype=torch.float32, device=dev)
        stats = torch.empty(call.stats_shape, dtype=torch.float64, device=dev)
        ptr, index, stream = _device_handles(dev)
        args = [ptr(a) if isinstance(a, torch.Tensor) else a for a in call.args]      # numbers and None as they are
        _capi.policy_check(getattr(_capi.lib(), call.symbol)(*args, ptr(scratch), ptr(grads), ptr(stats), index, 0, stream))
        ctx.policy, ctx.only_set = policy, call.only_set
        ctx.save_for_backward(grads)
        ctx.mark_non_differentiable(stats)
        loss = stats[:, 0].sum() if call.only_set is None else stats[0]     # the sum over the weight sets; the one set's
        return loss.to(torch.float32), stats

    @staticmethod
    def backward(ctx, g_loss, g_stats):
        (grads,) = ctx.saved_tensors
        out = unpack_gradient(ctx.policy, grads, g_loss, only_set=ctx.only_set)
        return (None, None) + tuple(g if needs else None for g, needs in zip(out, ctx.needs_input_grad[2:]))


def _device_loss(policy, key, t, dims, seq_len, hyper, only_set=None):
    """The loss call `key` of _LOSS_CALLS on the checked tensors t -> (loss, stats by name).  dims: (K, E, N), or (M, Q) of the
    Watershed call, whose agent id is only_set."""
    symbol, names, stat_names = _LOSS_CALLS[key]
    P = policy.num_sets
    values = dict(t, weights=policy.packed(), seq_len=seq_len, agent_id=only_set)
    values.update(zip(("n_steps", "num_seqs") if only_set is not None else ("n_steps", "num_envs", "num_agents"), dims))
    values.update(zip(_HYPER[key[1]], hyper))
    args = tuple(values[name] if name in values else getattr(policy, name) for name in names)
    if only_set is not None:
        scratch_floats = _capi.SSD_WSPPO_SCRATCH_FLOATS(*dims, policy.cell_size, seq_len)
    elif isinstance(policy, ConvFCPolicy):
        scratch_floats = policy.ppo_scratch_shape(dims[0] * dims[1] * dims[2] // P)[0]
    else:
        scratch_floats = policy.ppo_scratch_shape(*dims, seq_len)[0]
    lead = () if only_set is not None else (P,)
    call = _LossCall(symbol, args, scratch_floats, lead + (policy.set_floats,), lead + (len(stat_names),), only_set)
    params = tuple(getattr(policy, name) for name, _, _ in policy.layout())
    loss, stats = _LossFunction.apply(policy, call, *params)
    return loss, dict(zip(stat_names, stats.unbind(-1)))             # the columns: [P] each, scalars for the Watershed call
