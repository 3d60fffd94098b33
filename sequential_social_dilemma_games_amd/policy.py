"""The conv-FC policy network of the reference (models/conv_to_fc_net.py:1-51, ConvToFCNet: the model of Jaques et al. 2019)
as a torch module whose weights the device kernels read (include/ssd.h, SSD_POL_*; csrc/ssd_policy.hip).

    policy = ConvFCPolicy(num_actions=8, num_sets=5).cuda()       # one weight set per agent, as train_baseline.py:87-96
    logits, value = policy(obs_u8)                                # [..., N, 15, 15, 3] -> [..., N, A], [..., N]
    eng.rollout_policy(policy, obs0, 100, obs_ring, ...)          # the same network, on the device, in the loop

Per weight set: conv 3x3 (6 filters, stride 1, no padding) + ReLU, flatten in (row, col, channel) order -- TF's flatten of
NHWC --, fc1 1014 -> 32 + ReLU, fc2 32 -> 32 + ReLU, logits 32 -> A, and a value head 32 -> 1 on the same trunk (RLlib's
value_function() of a v1 Model).  The parameters are stored in TF's layouts (conv kernel [kh, kw, c_in, c_out], dense kernels
[in, out]) with a leading weight-set axis, so they map one to one onto a TF checkpoint's and onto the packed layout.
"""
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


class ConvFCPolicy(torch.nn.Module):
    """num_sets P independent weight sets: P = 1 is one policy shared by every agent, P = N one per agent (agent i uses
    set i).  Input: uint8 observations [..., 15, 15, 3] (P = 1) or [..., P, 15, 15, 3], normalised as float((u8 - 128) / 255)
    (the reference observation, map_env.py:199).  Output: (logits [..., A], value [...])."""

    def __init__(self, num_actions, num_sets=1, seed=0):
        super().__init__()
        A, P = int(num_actions), int(num_sets)
        if not 1 <= A <= _capi.SSD_POL_MAX_ACTIONS:
            raise ValueError("num_actions must be 1..%d" % _capi.SSD_POL_MAX_ACTIONS)
        if not 1 <= P <= 64:
            raise ValueError("num_sets must be 1..64")
        self.num_actions, self.num_sets = A, P
        g = torch.Generator().manual_seed(int(seed))
        limit = float(np.sqrt(6.0 / (27 + 9 * FILTERS)))        # slim.conv2d's default initializer: Glorot uniform
        init = {"conv_w": (torch.rand((P, 3, 3, 3, FILTERS), generator=g, dtype=torch.float64) * 2 - 1) * limit,
                "fc1_w": normc((P, FLAT, HIDDEN), 1.0, g), "fc2_w": normc((P, HIDDEN, HIDDEN), 1.0, g),
                "value_w": normc((P, HIDDEN, 1), 1.0, g), "logits_w": normc((P, HIDDEN, A), 0.01, g)}
        for name, shape, _ in self.layout():
            t = init.get(name)
            if t is None:
                t = torch.zeros((P,) + shape, dtype=torch.float64)       # biases start at zero
            self.register_parameter(name, torch.nn.Parameter(t.to(torch.float32)))
        self._packed = None
        self._tables = {}

    def layout(self):
        """(name, shape of one set, float offset within a packed set) of every parameter, in packed order."""
        A = self.num_actions
        return _FIXED + (("logits_w", (HIDDEN, A), _capi.SSD_POL_LOGITS_W), ("logits_b", (A,), _capi.SSD_POL_LOGITS_B(A)))

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

    @property
    def set_floats(self):
        return _capi.SSD_POL_SET_FLOATS(self.num_actions)

    def packed(self):
        """All weight sets as ONE contiguous float32 tensor on the parameters' device, in the layout of include/ssd.h: set p
        at p * SSD_POL_SET_FLOATS(A).  Rebuilt from the parameters on every call by device copies on the current stream (no
        host synchronisation), so an optimiser's update takes effect on the next call.  The buffer is reused between calls."""
        P, S = self.num_sets, self.set_floats
        dev = self.conv_w.device
        if self._packed is None or self._packed.device != dev:
            self._packed = torch.zeros(P * S, dtype=torch.float32, device=dev)
        v = self._packed.view(P, S)
        with torch.no_grad():
            for name, shape, off in self.layout():
                n = int(np.prod(shape))
                v[:, off:off + n].copy_(getattr(self, name).reshape(P, n))
        return self._packed

    def forward(self, obs):
        P, A = self.num_sets, self.num_actions
        if obs.shape[-3:] != (VIEW, VIEW, 3):
            raise ValueError("observations must end in (15, 15, 3), got %s" % (tuple(obs.shape),))
        if P > 1 and (obs.dim() < 4 or obs.shape[-4] != P):
            raise ValueError("with %d weight sets the observations need an agent axis of %d: [..., %d, 15, 15, 3]" % (P, P, P))
        lead = obs.shape[:-3]
        dt = self.conv_w.dtype
        key = (obs.device, dt)
        if key not in self._tables:                                  # float((u8 - 128) / 255), from the float64 values
            self._tables[key] = torch.from_numpy(_NORMALISE).to(dt).to(obs.device)
        x = self._tables[key][obs.long()]
        x = x.reshape(-1, P, VIEW, VIEW, 3)
        M = x.shape[0]
        x = x.permute(0, 1, 4, 2, 3).reshape(M, P * 3, VIEW, VIEW)    # NHWC -> NCHW, the sets as conv groups
        wc = self.conv_w.permute(0, 4, 3, 1, 2).reshape(P * FILTERS, 3, 3, 3)
        h = torch.relu(torch.nn.functional.conv2d(x, wc, self.conv_b.reshape(P * FILTERS), groups=P))
        h = h.reshape(M, P, FILTERS, 13, 13).permute(0, 1, 3, 4, 2).reshape(M, P, FLAT)   # flatten (row, col, channel)
        h = torch.relu(torch.einsum("mpk,pkj->mpj", h, self.fc1_w) + self.fc1_b)
        h = torch.relu(torch.einsum("mpk,pkj->mpj", h, self.fc2_w) + self.fc2_b)
        logits = torch.einsum("mpk,pkj->mpj", h, self.logits_w) + self.logits_b
        value = (torch.einsum("mpk,pkj->mpj", h, self.value_w) + self.value_b)[..., 0]
        return logits.reshape(lead + (A,)), value.reshape(lead)


def sample_host(logits, u, greedy=False):
    """The rollout's action selection in NumPy float32 (include/ssd.h): logits [..., A] float32, u [...] float32 from
    prng.policy_uniforms.  Returns (actions int32, logp float32).  The device uses expf / logf, so an action may differ where
    u lies within an ulp or so of a boundary of the cumulative softmax."""
    lg = np.asarray(logits, dtype=np.float32)
    A = lg.shape[-1]
    mx = lg.max(axis=-1)
    e = np.exp(lg - mx[..., None]).astype(np.float32)
    s = np.zeros(mx.shape, np.float32)
    for a in range(A):
        s = (s + e[..., a]).astype(np.float32)
    if greedy:
        act = lg.argmax(axis=-1).astype(np.int32)                    # the first of equal maxima
    else:
        u = np.asarray(u, dtype=np.float32)
        act = np.full(mx.shape, A - 1, np.int32)
        found = np.zeros(mx.shape, bool)
        c = np.zeros(mx.shape, np.float32)
        for a in range(A):
            c = (c + (e[..., a] / s).astype(np.float32)).astype(np.float32)
            hit = ~found & (u < c)
            act[hit] = a
            found |= hit
    la = np.take_along_axis(lg, act[..., None].astype(np.int64), axis=-1)[..., 0]
    logp = (la - (mx + np.log(s).astype(np.float32))).astype(np.float32)
    return act, logp


def cdf_margin(logits, u):
    """Distance of u from the nearest boundary of the float32 cumulative softmax of logits (for deciding which sampled actions
    a host mirror may legitimately get differently)."""
    lg = np.asarray(logits, dtype=np.float32)
    mx = lg.max(axis=-1)
    e = np.exp(lg - mx[..., None]).astype(np.float32)
    s = np.zeros(mx.shape, np.float32)
    for a in range(lg.shape[-1]):
        s = (s + e[..., a]).astype(np.float32)
    c = np.zeros(mx.shape, np.float32)
    margin = np.full(mx.shape, np.inf)
    for a in range(lg.shape[-1]):
        c = (c + (e[..., a] / s).astype(np.float32)).astype(np.float32)
        margin = np.minimum(margin, np.abs(np.asarray(u, np.float64) - c.astype(np.float64)))
    return margin
