#!/usr/bin/env python3
"""A few A3C updates on Harvest with the baseline's defaults (run_scripts/train_baseline.py: algorithm A3C, the recurrent policy),
sampler and learner both on the device: sample a fragment with discounted returns for advantages (SSDVectorEnv.sample(...,
state_every=seq_len, gamma=, use_gae=False)), then one pass of window-aligned step-range fragments through a3c_loss_recurrent
-- the loss with truncated backpropagation through time, its statistics and every gradient from one library call --, the
reference's gradient clip per weight set (clip_grad_by_set_norm: each agent's policy is clipped on its own) and Adam.  The A3C
twin of examples/ppo_train_lstm.py: an example of how the pieces fit, not a trainer.

    python examples/a3c_train_lstm.py [envs] [steps] [iterations]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sequential_social_dilemma_games_amd import ConvLSTMPolicy, a3c_loss_recurrent, clip_grad_by_set_norm  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    N, seq_len, windows = 5, 8, 2                                # an update is `windows` whole windows of seq_len steps
    hyper = dict(vf_loss_coeff=0.5, entropy_coeff=0.01)          # a3c_causal.py's defaults; its grad_clip is 40
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=0)
    policy = ConvLSTMPolicy(env.engine.num_actions, num_sets=N, cell_size=128, seed=0).cuda()     # train_baseline.py:146-147
    optim = torch.optim.Adam(policy.parameters(), lr=1e-4)

    first = env.reset().clone()                      # sample() leaves the fragment's last observation in this buffer
    for it in range(iterations):
        batch = env.sample(policy, steps, state_every=seq_len, gamma=0.99, use_gae=False)
        print("iteration %d: %d envs x %d agents x %d steps, reward sum %d" % (it, E, N, steps, int(batch["rew"].sum())))
        for k0 in range(0, steps, seq_len * windows):
            k1 = min(k0 + seq_len * windows, steps)
            # views: the rows' slices, the ring from the first window, and the observation step k0 acted on
            mb = {k: batch[k][k0:k1] for k in ("obs", "actions", "advantages", "value_targets", "done")}
            mb["state"] = batch["state"][k0 // seq_len:]
            loss, stats = a3c_loss_recurrent(policy, mb, seq_len=seq_len, obs_first=first if k0 == 0 else batch["obs"][k0 - 1], **hyper)
            optim.zero_grad()
            loss.backward()
            norms = clip_grad_by_set_norm(policy, 40.0)          # a3c_causal.py:125-131, one global norm per agent's policy
            optim.step()                                         # the next call packs the updated parameters
            rows = (k1 - k0) * E                                 # the statistics are sums over a set's rows
            print("  steps %d..%d: total %.5f, policy %.5f, vf %.4f, entropy %.4f per row (means over sets), grad norms %s" %
                  ((k0, k1 - 1) + tuple(float(stats[k].mean()) / rows for k in ("total_loss", "policy_loss", "vf_loss", "policy_entropy"))
                   + (" ".join("%.1f" % x for x in norms.tolist()),)))
        first = batch["obs"][steps - 1].clone()      # the next fragment's first step acts on this one's last observation


if __name__ == "__main__":
    main()
