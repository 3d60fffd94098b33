#!/usr/bin/env python3
"""IMPALA on Watershed SeqComm with the baselines' LSTM-FC policy, sampler and learner both on the device: sample a lock-step
batch once (WatershedVecEngine.sample), gather each agent id's own steps, then make two passes per id over the same batch --
impala_loss_watershed evaluates the sequences under the CURRENT weights in one launch (ssd_ws_policy_forward_seq), forms the
V-trace targets against the recorded behaviour log-probabilities and runs the A3C loss with truncated backpropagation through
time (ssd_ws_policy_ac_grad) --, each with the reference's per-policy gradient clip and an optimiser step.  In the first pass
the importance weights are exactly 1, in the second they are not.  An example of how the pieces fit, not a trainer.

The gather (own_steps) is examples/ppo_train_watershed.py's, returning rew, done and obs_next instead of advantages: agent
i's own steps are the steps k with actor[k] == i (the same k in every env, or it raises); the observation step k acted on is
obs[k - 1], or the observation from before the call for k = 0; starts[m] says that the episode ended between own steps m - 1
and m.  The fragment's last own step has no next observation yet: it is dropped from the loss, and its observation is obs_next,
from whose current value V-trace bootstraps.

The reward credited to an own step is THIS EXAMPLE'S CHOICE, and no test compares it with RLlib's sampler (ray is not
available to check against).  It follows the env's own dict: the reward the env delivers together with agent i's next observation
(the step before its next own step; the episode's last step if the episode ends first) is credited to the own step before it.
Rewards are float64 in this game; impala_loss_watershed takes them as float32 through vtrace's bonus input.

    python examples/impala_train_watershed.py [envs] [steps] [passes]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sequential_social_dilemma_games_amd import (WatershedEpisodeStats, WatershedLSTMPolicy, WatershedVecEngine, _capi, clip_grad_by_set_norm,  # noqa: E402
                                                 impala_loss_watershed)


def own_steps(batch, obs_before, agent_id, seq_len):
    """Agent agent_id's sequences of a lock-step batch, ready for impala_loss_watershed: a dict of [M, E, ...] tensors over its
    first M = (own steps - 1) own steps (the docstring above says why the last is dropped), or None if it acted fewer than twice."""
    actor = batch["actor"]
    if not bool((actor == actor[:, :1]).all()):
        raise ValueError("the envs are not in lock step: actor[k] differs between envs")
    ks = torch.nonzero(actor[:, 0] == agent_id).flatten().tolist()
    if len(ks) < 2:
        return None
    M, E, dev = len(ks) - 1, actor.shape[1], actor.device
    idx = torch.tensor(ks[:M], device=dev)
    prev = torch.cat([obs_before.unsqueeze(0), batch["obs"][:-1]])          # the observation each step acted on
    ended = (batch["done"] & _capi.SSD_WS_DONE_ALL) != 0                    # [K, E]: the episode ended with step k
    rew = torch.empty((M, E), dtype=torch.float32, device=dev)
    done = torch.zeros((M, E), dtype=torch.uint8, device=dev)
    starts = torch.zeros((M, E), dtype=torch.uint8, device=dev)
    for m in range(M):
        span = ended[ks[m]:ks[m + 1]]                                       # the steps up to the agent's next observation
        done[m] = span.any(0).to(torch.uint8)
        last = torch.where(span.any(0), ks[m] + span.to(torch.uint8).argmax(0), ks[m + 1] - 1)
        rew[m] = batch["rew"].gather(0, last.unsqueeze(0))[0].to(torch.float32)
        if m > 0:
            starts[m] = done[m - 1]
    return {"obs": prev[idx].contiguous(), "actions": batch["actions"][idx].contiguous(), "logp": batch["logp"][idx].contiguous(),
            "starts": starts, "state": batch["state_in"][idx[::seq_len]].contiguous(), "rew": rew, "done": done,
            "obs_next": prev[ks[M]].contiguous()}                           # start_next defaults to done[M - 1]


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 131                   # one SeqComm episode
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    seq_len = 4
    hyper = dict(gamma=0.99, vf_loss_coeff=0.5, entropy_coeff=0.01, clip_rho_threshold=1.0, clip_pg_rho_threshold=1.0)
    eng = WatershedVecEngine(_capi.SSD_WS_SEQ_COMM, E, seed=0)
    policy = WatershedLSTMPolicy(_capi.SSD_WS_SEQ_COMM, cell_size=128, seed=0).cuda()
    optim = torch.optim.Adam(policy.parameters(), lr=1e-4)

    episodes = WatershedEpisodeStats(_capi.SSD_WS_SEQ_COMM, E)              # what the launchers' callbacks log, folded by the stepping kernel
    eng.attach_stats(episodes)                                               # ... before the reset that opens the first episodes
    before = eng.reset()[0].clone()
    batch = eng.sample(policy, steps)
    s = episodes.summary()
    print("%d envs x %d phases: %d episodes, episode_reward_mean %.1f, custom_metrics %s"
          % (E, steps, s["episodes"], s["episode_reward_mean"], {k: round(v, 3) for k, v in s["custom_metrics"].items() if k.endswith("_mean")}))
    for agent_id in range(policy.num_sets):                                  # one loss per agent id, as the reference's policies
        seq = own_steps(batch, before, agent_id, seq_len)
        if seq is None:
            continue
        for p in range(passes):
            loss, stats = impala_loss_watershed(policy, agent_id, seq, seq_len=seq_len, **hyper)
            optim.zero_grad()
            loss.backward()                                                  # fills row agent_id of every parameter's .grad
            norms = clip_grad_by_set_norm(policy, 40.0)                      # a3c_causal.py's grad_clip, per policy
            optim.step()                                                     # the next call packs the updated parameters
            print("  agent %d pass %d: %d own steps, total %.4f, policy %.4f, vf %.4f, entropy %.4f, gradient norm %.3f" %
                  (agent_id, p, seq["actions"].shape[0], float(stats["total_loss"]), float(stats["policy_loss"]),
                   float(stats["vf_loss"]), float(stats["policy_entropy"]), float(norms[agent_id])))


if __name__ == "__main__":
    main()
