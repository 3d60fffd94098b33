#!/usr/bin/env python3
"""One PPO update on Harvest with the conv-FC policy: sample a fragment with advantages and value targets computed on the
device (SSDVectorEnv.sample(..., gamma=, lambda_=)), then the clipped surrogate plus the value loss on the returned tensors
and one optimiser step, all in torch.  An example of how the pieces fit, not a trainer: no minibatches, no epochs, no
advantage standardisation.

    python examples/ppo_update.py [envs] [steps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sequential_social_dilemma_games_amd import ConvFCPolicy  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    N, clip, vf_coeff, entropy_coeff = 5, 0.3, 1e-4, 1e-3
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=0)
    policy = ConvFCPolicy(env.engine.num_actions, num_sets=N, seed=0).cuda()        # one policy per agent
    optim = torch.optim.Adam(policy.parameters(), lr=1e-3)

    first = env.reset().clone()                      # sample() leaves the fragment's last observation in this buffer
    batch = env.sample(policy, steps, gamma=0.99, lambda_=0.95)
    # step k acted on the observation before it: the reset's for k = 0, then row k - 1 (row k is the one after step k)
    obs = torch.cat([first.unsqueeze(0), batch["obs"][:-1]])
    actions, adv, targets = batch["actions"].long(), batch["advantages"], batch["value_targets"]

    logits, value = policy(obs)                      # [K, E, N, A], [K, E, N]
    logp_all = torch.log_softmax(logits, dim=-1)
    logp = logp_all.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    ratio = torch.exp(logp - batch["logp"])
    surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv)
    entropy = -(logp_all.exp() * logp_all).sum(-1)
    vf_loss = (value - targets).square()
    loss = (-surrogate + vf_coeff * vf_loss - entropy_coeff * entropy).mean()
    optim.zero_grad()
    loss.backward()
    optim.step()                                     # the next sample() packs the updated parameters

    print("fragment: %d envs x %d agents x %d steps, reward sum %d, episode ends %d" %
          (E, N, steps, int(batch["rew"].sum()), int(batch["done"][:, :, 0].sum())))
    print("before the step: ratio %.6f (1 expected), surrogate %.4f, value loss %.4f, entropy %.4f, loss %.4f" %
          tuple(float(x.detach().mean()) for x in (ratio, surrogate, vf_loss, entropy, loss)))
    after = env.sample(policy, steps, gamma=0.99, lambda_=0.95)
    print("next fragment with the updated policy: mean advantage %.4f, mean value target %.4f" %
          (float(after["advantages"].mean()), float(after["value_targets"].mean())))


if __name__ == "__main__":
    main()
