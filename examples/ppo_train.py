#!/usr/bin/env python3
"""A few PPO iterations on Harvest with the conv-FC policy, sampler and learner both on the device: sample a fragment with
advantages and value targets (SSDVectorEnv.sample(..., gamma=, lambda_=)), then a few epochs of step-range minibatches through
ppo_loss -- the loss, its statistics and every gradient from one library call, no activation kept -- and Adam.  An example of
how the pieces fit, not a trainer: no advantage standardisation, no adaptive KL coefficient, no shuffling across steps.

    python examples/ppo_train.py [envs] [steps] [iterations]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sequential_social_dilemma_games_amd import ConvFCPolicy, ppo_loss  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    N, epochs, mb_steps = 5, 3, 8
    hyper = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=1e-3, kl_coeff=0.0)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=0)
    policy = ConvFCPolicy(env.engine.num_actions, num_sets=N, seed=0).cuda()        # one policy per agent
    optim = torch.optim.Adam(policy.parameters(), lr=1e-4)

    first = env.reset().clone()                      # sample() leaves the fragment's last observation in this buffer
    for it in range(iterations):
        batch = env.sample(policy, steps, gamma=0.99, lambda_=0.95)
        print("iteration %d: %d envs x %d agents x %d steps, reward sum %d" % (it, E, N, steps, int(batch["rew"].sum())))
        for epoch in range(epochs):
            sums, count = None, 0
            for k0 in range(0, steps, mb_steps):
                # step k acted on the observation before it: the slices are views, and obs_first shifts by address
                mb = {k: batch[k][k0:k0 + mb_steps] for k in ("obs", "actions", "logp", "value", "advantages", "value_targets")}
                loss, stats = ppo_loss(policy, mb, obs_first=first if k0 == 0 else batch["obs"][k0 - 1], **hyper)
                optim.zero_grad()
                loss.backward()
                optim.step()                         # the next call packs the updated parameters
                row = torch.stack([stats[k].mean() for k in ("total_loss", "policy_loss", "vf_loss", "entropy")])
                sums, count = row if sums is None else sums + row, count + 1
            print("  epoch %d: total %.5f, policy %.5f, vf %.4f, entropy %.4f (means over sets and minibatches)" %
                  ((epoch,) + tuple(float(x) for x in sums / count)))
        first = batch["obs"][steps - 1].clone()      # the next fragment's first step acts on this one's last observation


if __name__ == "__main__":
    main()
