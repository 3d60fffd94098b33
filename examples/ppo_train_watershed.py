#!/usr/bin/env python3
"""A few PPO iterations on Watershed SeqComm with the baselines' LSTM-FC policy, sampler and learner both on the device: sample a
lock-step batch (WatershedVecEngine.sample), gather each agent id's own steps, form advantages with compute_advantages and
standardise them over the id's [M, E] rows (standardize_advantages, one weight set: an agent id is one RLlib policy), then one
ppo_loss_watershed call per agent id -- the loss with truncated backpropagation through time, its statistics and the gradient of
that id's weight set from one library call -- and one Adam step; vf_explained_var is printed per id.  An example of how the pieces fit, not a trainer.

The gather (own_steps): Watershed is turn-based, one agent acts per phase.  Agent i's own steps are the steps k with
actor[k] == i; envs reset together stay in lock step, so that is the same k in every env (it raises if not).  The observation
step k acted on is obs[k - 1], or the observation from before the call for k = 0.  starts[m] says that the episode ended (the
done flags' SSD_WS_DONE_ALL bit) between own steps m - 1 and m, so own step m starts from a zero state.

The reward credited to an own step is THIS EXAMPLE'S CHOICE, and no test compares it with RLlib's sampler (ray is not
available to check against).  It follows the env's own dict: the reward the env delivers together with agent i's next observation
(the step before its next own step; the episode's last step if the episode ends first) is credited to the own step before it.
The fragment's last own step has no next observation yet: it is dropped from the loss, and the advantages bootstrap from its
value.  Rewards are float64 in this game; compute_advantages takes them as its float32 bonus on a zero integer reward.

    python examples/ppo_train_watershed.py [envs] [steps] [iterations]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sequential_social_dilemma_games_amd import (WatershedEpisodeStats, WatershedLSTMPolicy, WatershedVecEngine, _capi,  # noqa: E402
                                                 compute_advantages, explained_variance, ppo_loss_watershed,
                                                 standardize_advantages)


def own_steps(batch, obs_before, agent_id, seq_len, gamma=0.99, lambda_=0.95):
    """Agent agent_id's sequences of a lock-step batch, ready for ppo_loss_watershed: a dict of [M, E, ...] tensors over its
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
    value = batch["value"][idx].contiguous()
    adv, vt = compute_advantages(torch.zeros((M, E), dtype=torch.int32, device=dev), value, last_value=batch["value"][ks[M]].contiguous(),
                                 done=done, gamma=gamma, lambda_=lambda_, bonus=rew, bonus_weight=1.0)
    standardize_advantages(adv, num_sets=1, out=adv)                        # once per batch, before the epochs, as RLlib's PPO
    return {"obs": prev[idx].contiguous(), "actions": batch["actions"][idx].contiguous(), "logp": batch["logp"][idx].contiguous(),
            "value": value, "dist": batch["dist"][idx].contiguous(), "advantages": adv, "value_targets": vt, "starts": starts,
            "state": batch["state_in"][idx[::seq_len]].contiguous()}


def format_summary(s):
    """One line of a WatershedEpisodeStats.summary(): RLlib's episode means and the launchers' three custom metrics."""
    c = s["custom_metrics"]
    return ("%d episodes (%d truncated), len %.1f, episode_reward_mean %.1f, violations %.3f, Equality %.3f, Utility %.1f"
            % (s["episodes"], s["truncated"], s["episode_len_mean"], s["episode_reward_mean"], c["violations_mean"],
               c["Equality_mean"], c["Utility_mean"]))


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 131                   # one SeqComm episode
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    seq_len = 4
    hyper = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=1e-3, kl_coeff=0.0)   # the launchers' PPO settings
    eng = WatershedVecEngine(_capi.SSD_WS_SEQ_COMM, E, seed=0)
    policy = WatershedLSTMPolicy(_capi.SSD_WS_SEQ_COMM, cell_size=128, seed=0).cuda()
    optim = torch.optim.Adam(policy.parameters(), lr=1e-4)

    episodes = WatershedEpisodeStats(_capi.SSD_WS_SEQ_COMM, E)              # what the launchers' callbacks log, folded by the stepping kernel
    eng.attach_stats(episodes)                                               # ... before the reset that opens the first episodes
    before = eng.reset()[0].clone()
    for it in range(iterations):
        batch = eng.sample(policy, steps)
        print("iteration %d: %d envs x %d phases: %s" % (it, E, steps, format_summary(episodes.summary())))
        optim.zero_grad()
        for agent_id in range(policy.num_sets):                              # one loss per agent id, as the reference's policies
            seq = own_steps(batch, before, agent_id, seq_len)
            if seq is None:
                continue
            loss, stats = ppo_loss_watershed(policy, agent_id, seq, seq_len=seq_len, **hyper)
            loss.backward()                                                  # fills row agent_id of every parameter's .grad
            print("  agent %d: %d own steps, total %.5f, policy %.5f, vf %.4f, entropy %.4f, vf_explained_var %.3f" %
                  (agent_id, seq["actions"].shape[0], float(stats["total_loss"]), float(stats["policy_loss"]), float(stats["vf_loss"]),
                   float(stats["entropy"]), float(explained_variance(seq["value_targets"], seq["value"])[0])))
        optim.step()                                                         # the next call packs the updated parameters
        before = batch["obs"][steps - 1].clone()                             # the next batch's first step acts on this one's last observation


if __name__ == "__main__":
    main()
