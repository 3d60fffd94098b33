#!/usr/bin/env python3
"""A few PPO iterations on Harvest with the conv-FC policy, sampler and learner both on the device: sample a fragment with
advantages and value targets (SSDVectorEnv.sample(..., gamma=, lambda_=, standardize=True): the advantages standardised per
weight set once per batch, as RLlib's PPO optimizers do before the SGD epochs), then a few epochs of step-range minibatches
through ppo_loss -- the loss, its statistics and every gradient from one library call, no activation kept -- and Adam, with
the KL coefficient adapted from the sampled KL after every iteration (update_kl_coeff) and vf_explained_var printed per
weight set.  An example of how the pieces fit, not a trainer: no shuffling across steps.

    python examples/ppo_train.py [envs] [steps] [iterations]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sequential_social_dilemma_games_amd import ConvFCPolicy, evaluate_fragment, explained_variance, ppo_loss, update_kl_coeff  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    N, epochs, mb_steps = 5, 3, 8
    hyper = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=1e-3)
    kl_coeff, kl_target = 0.2, 0.01                  # RLlib's PPO defaults; one coefficient for all weight sets
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=0)
    policy = ConvFCPolicy(env.engine.num_actions, num_sets=N, seed=0).cuda()        # one policy per agent
    optim = torch.optim.Adam(policy.parameters(), lr=1e-4)

    first = env.reset().clone()                      # sample() leaves the fragment's last observation in this buffer
    for it in range(iterations):
        batch = env.sample(policy, steps, gamma=0.99, lambda_=0.95, standardize=True)
        batch["logits"] = evaluate_fragment(policy, batch, first)[0]         # the behaviour logits: the weights have not moved yet
        print("iteration %d: %d envs x %d agents x %d steps, reward sum %d, kl_coeff %.4f" %
              (it, E, N, steps, int(batch["rew"].sum()), kl_coeff))
        print("  vf_explained_var per set: %s" % " ".join("%.3f" % v for v in explained_variance(batch["value_targets"], batch["value"], num_sets=N).tolist()))
        for epoch in range(epochs):
            sums, count = None, 0
            for k0 in range(0, steps, mb_steps):
                # step k acted on the observation before it: the slices are views, and obs_first shifts by address
                mb = {k: batch[k][k0:k0 + mb_steps] for k in ("obs", "actions", "logp", "value", "advantages", "value_targets", "logits")}
                loss, stats = ppo_loss(policy, mb, obs_first=first if k0 == 0 else batch["obs"][k0 - 1], kl_coeff=kl_coeff, **hyper)
                optim.zero_grad()
                loss.backward()
                optim.step()                         # the next call packs the updated parameters
                row = torch.stack([stats[k].mean() for k in ("total_loss", "policy_loss", "vf_loss", "entropy", "kl")])
                sums, count = row if sums is None else sums + row, count + 1
            print("  epoch %d: total %.5f, policy %.5f, vf %.4f, entropy %.4f, kl %.5f (means over sets and minibatches)" %
                  ((epoch,) + tuple(float(x) for x in sums / count)))
        kl_coeff = update_kl_coeff(kl_coeff, float(sums[4] / count), kl_target)      # from the last epoch's sampled KL
        first = batch["obs"][steps - 1].clone()      # the next fragment's first step acts on this one's last observation


if __name__ == "__main__":
    main()
