#!/usr/bin/env python3
"""A few IMPALA updates on Harvest with the recurrent policy (the reference's third trainer, algorithms/impala_causal.py), sampler
and learner both on the device: sample a fragment ONCE (SSDVectorEnv.sample(..., state_every=seq_len): no advantages are asked
for), then several passes over the same fragment through impala_loss_recurrent -- the fragment evaluated under the current
weights, the importance weights rho = pi / mu against the recorded logp, the V-trace scan, and the A3C call's loss with
truncated backpropagation through time and every gradient --, the reference's gradient clip per weight set and Adam.  In the
first pass the weights are the sampler's and rho is 1 up to rounding; from the second pass on they have moved and V-trace
corrects for it.  The IMPALA twin of examples/a3c_train_lstm.py: an example of how the pieces fit, not a trainer.

    python examples/impala_train_lstm.py [envs] [steps] [iterations] [passes]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sequential_social_dilemma_games_amd import ConvLSTMPolicy, clip_grad_by_set_norm, evaluate_fragment, impala_loss_recurrent  # noqa: E402
from sequential_social_dilemma_games_amd import constants as K  # noqa: E402
from sequential_social_dilemma_games_amd.vector_env import SSDVectorEnv  # noqa: E402


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    passes = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    N, seq_len = 5, 8
    hyper = dict(gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0)
    env = SSDVectorEnv(K.GAME_HARVEST, E, N, horizon=1000, seed=0)
    policy = ConvLSTMPolicy(env.engine.num_actions, num_sets=N, cell_size=128, seed=0).cuda()
    optim = torch.optim.Adam(policy.parameters(), lr=1e-4)

    first = env.reset().clone()                      # sample() leaves the fragment's last observation in this buffer
    for it in range(iterations):
        batch = env.sample(policy, steps, state_every=seq_len)
        print("iteration %d: %d envs x %d agents x %d steps, reward sum %d" % (it, E, N, steps, int(batch["rew"].sum())))
        for p in range(passes):
            # what the call is about to see (for the print only: the call evaluates the fragment itself)
            logits, _, _ = evaluate_fragment(policy, batch, first, seq_len)
            logp = torch.log_softmax(logits, -1).gather(-1, batch["actions"].long().unsqueeze(-1)).squeeze(-1)
            rhos = torch.exp(logp - batch["logp"])
            loss, stats = impala_loss_recurrent(policy, batch, seq_len=seq_len, obs_first=first, one_call=True, **hyper)
            optim.zero_grad()
            loss.backward()
            norms = clip_grad_by_set_norm(policy, 40.0)          # one global norm per agent's policy
            optim.step()                                         # the next pass evaluates under the updated parameters
            rows = steps * E                                     # the statistics are sums over a set's rows
            print("  pass %d: rho in [%.4f, %.4f]; total %.5f, policy %.5f, vf %.4f, entropy %.4f per row (means over sets), grad norms %s" %
                  ((p, float(rhos.min()), float(rhos.max()))
                   + tuple(float(stats[k].mean()) / rows for k in ("total_loss", "policy_loss", "vf_loss", "policy_entropy"))
                   + (" ".join("%.1f" % x for x in norms.tolist()),)))
        first = batch["obs"][steps - 1].clone()      # the next fragment's first step acts on this one's last observation


if __name__ == "__main__":
    main()
