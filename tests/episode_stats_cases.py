"""The case matrix of the episode-statistics fold (csrc/ssd_stats.hip), built from the branch points of its two passes, and
features(): which of those paths a case takes, derived from the case's arrays alone.  NumPy only, no device code; the
reference stays episode_stats_ref.RefStats.  tests/test_episode_stats_edges_cpu.py asserts that the matrix reaches every path
in REQUIRED and every lane-packing pair in PACK_PAIRS, tests/test_episode_stats_edges_gpu.py runs every case on the device.

A case is {"name", "E", "N", "ops"}; an op is ("fold", {rew, done or None, step0, n_steps, reset_every, chunk}) -- the ring is
rew.shape[0] --, ("discard", mask or None) or ("drain", keep).  Every runner drains once more at the end.  Nothing here is
drawn: rewards come from a table by an arithmetic pattern, episode ends are placed by hand.  E * N * sum(n_steps) stays below
5 * 10^4, RefStats being a Python loop."""
import numpy as np

import episode_stats_ref as ref

K_BATCH = 8                                                      # pass 1 issues the loads of 8 steps together
AUTO_CHUNK = 64
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
USUAL = [1, 0, 0, -1, -50, -49, -51, -100, -101, -150, 1, 1, 0]  # apples, FIRE costs, single and multiple hits
SPECIAL = [2, 49, 50, 51, 100, -49, -50, -51, I32_MAX, I32_MIN]  # every int32 decodes: h = floor((1 - r) / 50)
PACK_N = [1, 2, 3, 5, 7, 10, 21, 32, 33, 63, 64]
PACK_CLASSES = ["1", "per", "per+1", "4per", "4per+1"]           # one env; a full wave; a second wave with one env; a full
#                                                                  block of pass 2; a second block with one live env
BATCH_L = [1, 7, 8, 9, 15, 16, 17, 64, 65]

REQUIRED = (
    # chunk level
    ["chunk_ends_0", "chunk_ends_1", "chunk_ends_2", "chunk_ends_3plus", "first_end_on_chunk_first_step",
     "last_end_on_chunk_last_step", "consecutive_ends", "reread_wraps", "reread_no_wrap", "head_pos_onto_open_t",
     "tsum_shift_changes_S"]
    # batch level
    + ["L_%d" % L for L in BATCH_L] + ["short_last_%d" % n for n in (1, 7, 8, 9)]
    + ["end_at_batch_pos_0", "end_at_batch_pos_7", "wrap_inside_batch", "wrap_between_batches"]
    # fold level
    + ["no_end_fold_carried", "fold_last_step_end", "ten_one_step_folds", "n_steps_eq_ring", "step0_ge_ring", "step0_near_2^31",
       "done_and_reset_same_step", "reset_every_1", "fold_start_truncates_open", "fold_start_on_t0"]
    # values
    + ["rew_%d" % r for r in SPECIAL] + ["C0_G0_nan", "C0_Gpos_neginf", "C_neg", "agents_with_and_without_pos"]
    # the done ring
    + ["done_other_agents_only_no_end", "done_agent0_only_ends"]
    # lane packing and the handle
    + ["wave_has_0_1_many", "wave_neighbours_differ", "discard_t0", "discard_t>0"])

PACK_PAIRS = [(N, cls) for N in PACK_N for cls in PACK_CLASSES]


def effective_chunk(chunk, n_steps):
    return max(1, min(chunk if chunk > 0 else AUTO_CHUNK, n_steps))


def pack_classes(N, E):
    per = 64 // N
    return {c for c, v in zip(PACK_CLASSES, (1, per, per + 1, 4 * per, 4 * per + 1)) if v == E}


def features(case, info=None):
    """The set of path names the case takes (REQUIRED lists them; plus ("pack", N, class)).  info, if given, receives
    "episodes" (one record per closed episode: e, T, R, pos, tsum, and tsum_unshifted -- what the fold would sum if a chunk's
    head were appended to the open episode without the pos * t shift), "peak" (the largest magnitude among G, 2 N C and the
    tsums) and "agent_steps"."""
    E, N = case["E"], case["N"]
    F = {("pack", N, c) for c in pack_classes(N, E)}
    per = 64 // N
    episodes, peak, agent_steps = [], 0, 0
    t = [0] * E
    zero = lambda: {k: [0] * N for k in ("R", "pos", "tsum", "ns")}
    o = [zero() for _ in range(E)]
    no_end_before = [False] * E                                  # the fold before had no end in this env
    one_step_run = 0
    for kind, a in case["ops"]:
        if kind == "drain":
            continue
        if kind == "discard":
            for e in range(E):
                if a is None or a[e]:
                    F.add("discard_t>0" if t[e] > 0 else "discard_t0")
                    t[e], o[e], no_end_before[e] = 0, zero(), False
            one_step_run = 0
            continue
        rew, done, step0, n, re, chunk = a["rew"], a["done"], a["step0"], a["n_steps"], a["reset_every"], a["chunk"]
        ring = rew.shape[0]
        assert rew.dtype == np.int32 and rew.shape == (ring, E, N) and 1 <= n <= ring
        assert done is None or (done.dtype == np.uint8 and done.shape == rew.shape)
        agent_steps += E * N * n
        L = effective_chunk(chunk, n)
        C = (n + L - 1) // L
        F.add("L_%d" % L)
        if C > 1 and n - (C - 1) * L < L:
            F.add("short_last_%d" % (n - (C - 1) * L))
        if n == ring:
            F.add("n_steps_eq_ring")
        if step0 >= ring:
            F.add("step0_ge_ring")
        if re == 1:
            F.add("reset_every_1")
        one_step_run = one_step_run + 1 if n == 1 else 0
        if one_step_run >= 10:
            F.add("ten_one_step_folds")
        if step0 == 2 ** 31 - 5 and n == 8 and re > 0 and any(step0 + k + 1 >= 2 ** 31 and (step0 + k + 1) % re == 0 for k in range(n)):
            F.add("step0_near_2^31")
        slots = [(step0 + k) % ring for k in range(n)]
        for r in np.unique(rew[slots]).tolist():
            if r in SPECIAL:
                F.add("rew_%d" % r)
        by_reset = [re > 0 and (step0 + k + 1) % re == 0 for k in range(n)]
        ends_class = [[0] * C for _ in range(E)]
        for e in range(E):
            if re > 0 and step0 % re == 0:
                F.add("fold_start_truncates_open" if t[e] > 0 else "fold_start_on_t0")
                t[e], o[e] = 0, zero()
            elif no_end_before[e] and t[e] > 0:
                F.add("no_end_fold_carried")
            end = list(by_reset)
            for k in range(n):
                if done is not None:
                    d0, others = done[slots[k], e, 0] != 0, bool(done[slots[k], e, 1:].any())
                    if d0 and by_reset[k]:
                        F.add("done_and_reset_same_step")
                    if not d0 and others and not by_reset[k]:
                        F.add("done_other_agents_only_no_end")
                    if d0 and N > 1 and not others and not by_reset[k]:
                        F.add("done_agent0_only_ends")
                    end[k] = end[k] or d0
            if end[n - 1]:
                F.add("fold_last_step_end")
            no_end_before[e] = not any(end)
            for c in range(C):
                k0, k1 = c * L, min(n, c * L + L)
                ks = [k for k in range(k0, k1) if end[k]]
                nb = len(ks)
                ends_class[e][c] = min(nb, 2)
                F.add("chunk_ends_%s" % (nb if nb < 3 else "3plus"))
                if nb and ks[0] == k0 and k1 - k0 > 1:
                    F.add("first_end_on_chunk_first_step")
                if nb and ks[-1] == k1 - 1:
                    F.add("last_end_on_chunk_last_step")
                for k in ks:
                    if (k - k0) % K_BATCH in (0, K_BATCH - 1):
                        F.add("end_at_batch_pos_%d" % ((k - k0) % K_BATCH))
                if nb > 1:
                    if any(b == a_ + 1 for a_, b in zip(ks, ks[1:])):
                        F.add("consecutive_ends")            # a one-step episode inside the re-read
                    F.add("reread_wraps" if slots[ks[0] + 1] > slots[ks[-1]] else "reread_no_wrap")
                for k in range(k0, k1 - 1):                      # the wrap falls behind step k, inside this chunk
                    if slots[k] == ring - 1:
                        F.add("wrap_between_batches" if (k - k0) % K_BATCH == K_BATCH - 1 else "wrap_inside_batch")
                head_last = ks[0] if nb else k1 - 1
                if t[e] > 0 and (rew[slots[k0:head_last + 1], e] > 0).any():
                    F.add("head_pos_onto_open_t")
                for k in range(k0, k1):
                    t[e] += 1
                    oe = o[e]
                    for i in range(N):
                        r = int(rew[slots[k], e, i])
                        oe["R"][i] += r
                        if r > 0:
                            oe["pos"][i] += 1
                            oe["tsum"][i] += t[e]
                            oe["ns"][i] += k - k0 + 1 if k <= head_last else t[e]
                    if end[k]:
                        Cr = sum(oe["R"])
                        G = sum(abs(x - y) for x in oe["R"] for y in oe["R"])
                        peak = max([peak, abs(G), abs(2 * N * Cr)] + oe["tsum"])
                        if Cr == 0:
                            F.add("C0_G0_nan" if G == 0 else "C0_Gpos_neginf")
                        if Cr < 0:
                            F.add("C_neg")
                        if any(oe["pos"]) and not all(oe["pos"]):
                            F.add("agents_with_and_without_pos")
                        if ref.metrics(oe["R"], oe["pos"], oe["tsum"], [0] * N, t[e])[2] != ref.metrics(oe["R"], oe["pos"], oe["ns"], [0] * N, t[e])[2]:
                            F.add("tsum_shift_changes_S")
                        episodes.append({"e": e, "T": t[e], "R": oe["R"], "pos": oe["pos"], "tsum": oe["tsum"], "tsum_unshifted": oe["ns"]})
                        t[e], o[e] = 0, zero()
        for w in range((E + per - 1) // per):                    # the envs one wave holds, chunk by chunk
            envs = range(w * per, min(E, w * per + per))
            for c in range(C):
                cls = [ends_class[e][c] for e in envs]
                if len(set(cls)) == 3:
                    F.add("wave_has_0_1_many")
                if any(x != y for x, y in zip(cls, cls[1:])):
                    F.add("wave_neighbours_differ")
    if info is not None:
        info.update(episodes=episodes, peak=peak, agent_steps=agent_steps)
    return F


# ---------------------------------------------------------------- running a case
def run(stats, case, to_device=lambda x: x, chunk_of=None):
    """The case's ops on `stats` (a RefStats, or an EpisodeStats with to_device); returns the drains, the final one included.
    chunk_of(n_steps): a chunk length in place of each fold's own."""
    out = []
    for kind, a in case["ops"]:
        if kind == "fold":
            if hasattr(stats, "set_chunk"):
                stats.set_chunk(a["chunk"] if chunk_of is None else chunk_of(a["n_steps"]))
            stats.fold(to_device(a["rew"]), None if a["done"] is None else to_device(a["done"]), step0=a["step0"],
                       n_steps=a["n_steps"], reset_every=a["reset_every"])
        elif kind == "discard":
            stats.discard(None if a is None else to_device(a))
        else:
            out.append(stats.drain(keep=a))
    out.append(stats.drain())
    return out


def in_pieces(case):
    """The same case with every fold cut into folds of one step."""
    ops = []
    for kind, a in case["ops"]:
        if kind == "fold":
            ops += [("fold", dict(a, step0=a["step0"] + k, n_steps=1)) for k in range(a["n_steps"])]
        else:
            ops.append((kind, a))
    return dict(case, name=case["name"] + "/pieces", ops=ops)


# ---------------------------------------------------------------- building the matrix
def pattern(ring, E, N, table=USUAL, salt=0):
    k, e, i = np.ogrid[:ring, :E, :N]
    return np.asarray(table, np.int64)[(k * 7 + e * 3 + i * 5 + salt) % len(table)].astype(np.int32)


def fold(rew, done=None, step0=0, n_steps=None, reset_every=0, chunk=0):
    return ("fold", {"rew": rew, "done": done, "step0": step0, "n_steps": rew.shape[0] if n_steps is None else n_steps,
                     "reset_every": reset_every, "chunk": chunk})


def done_ring(rew, step0, ends, agents=None):
    """done with the byte of every agent (or of `agents`) set at the slots of the fold steps ends[e] = [k, ...]."""
    ring = rew.shape[0]
    done = np.zeros(rew.shape, np.uint8)
    for e, ks in ends.items():
        for k in ks:
            if agents is None:
                done[(step0 + k) % ring, e, :] = 1 + (k % 3) * 100   # any non-zero byte ends
            else:
                done[(step0 + k) % ring, e, agents] = 1
    return done


def _chunk_cases():
    out = []
    # L = 6, four chunks.  env 0: no end at all.  env 1: one end, on the first step of chunk 1, whose head (that one step, an
    # apple for agent 0) is appended to the 6 open steps.  env 2: ends on 10 and 11, the last step of chunk 1: an empty tail.
    # env 3: 13, 14 and 17 in chunk 2.  env 4: one end in the middle of chunk 2, apples before it in chunks 0 .. 2.
    ends = {1: [6], 2: [10, 11], 3: [13, 14, 17], 4: [15]}
    for name, ring, step0 in (("chunks", 24, 0), ("chunks_wrap_in_reread", 24, 8), ("chunks_step0_past_ring", 29, 71)):
        rew = pattern(ring, 5, 3)
        rew[(step0 + 6) % ring, 1, 0] = 1
        for k in (2, 7, 13, 14):
            rew[(step0 + k) % ring, 4, 1] = 1
        out.append({"name": name, "E": 5, "N": 3, "ops": [fold(rew, done_ring(rew, step0, ends), step0, 24, 0, 6)]})
    return out


def _batch_cases():
    out = []
    # (L, n_steps): the last chunk is 1, 7, 8 or 9 steps where L allows one.  env 0 ends on batch positions 7 (chunk 0) and 0
    # (chunk 1), env 1 on 3 and 4 and on the fold's last step.  The ring is 3 longer than the fold and the first step is placed
    # so that the wrap falls behind step 7 (between the first two batches of chunk 0) or behind step 2 (inside the first).
    for L, n in ((1, 12), (7, 15), (8, 23), (9, 26), (15, 24), (16, 33), (17, 41), (64, 72), (65, 74)):
        for where, lead in (("between", 8), ("inside", 3)):
            ring = n + 3
            step0 = ring - lead
            rew = pattern(ring, 2, 2, salt=L)
            ends = {0: sorted({min(7, L - 1), L}), 1: [3, 4, n - 1]}
            out.append({"name": "batch_L%d_wrap_%s" % (L, where), "E": 2, "N": 2,
                        "ops": [fold(rew, done_ring(rew, step0, ends), step0, n, 0, L)]})
    return out


def _fold_cases():
    out = []
    # the first fold-level case (the chunk-extreme tests run it too): no end in six steps, carried into a fold that ends env 0
    # on its last step, then the whole ring at a first step beyond it
    rew = pattern(10, 3, 2)
    rew[:, 2, :] = np.asarray([[1, 0], [0, 1]], np.int32)[np.arange(10) % 2]
    out.append({"name": "fold_carry", "E": 3, "N": 2, "ops": [
        fold(rew, None, 0, 6), fold(rew, done_ring(rew, 6, {0: [3]}), 6, 4), ("drain", True),
        fold(rew, done_ring(rew, 20, {1: [0, 9], 2: [4]}), 20, 10)]})
    # ten folds of one step and four more, ends on some
    rew = pattern(4, 3, 2, salt=5)
    done = [done_ring(rew, s, {0: [0]} if s % 3 == 0 else {1: [0]} if s % 5 == 0 else {}) for s in range(14)]
    out.append({"name": "fold_one_step_x14", "E": 3, "N": 2, "ops": [fold(rew, done[s], s, 1) for s in range(14)]})
    # step0 = 2^31 - 5: the global steps 2^31 - 4 .. 2^31 + 3; 3 divides 2^31 - 2 and 2^31 + 1; 715827883 only 2^31 + 1
    for re in (3, 715827883):
        rew = pattern(8, 2, 3, salt=re % 11)
        out.append({"name": "fold_step0_near_2^31_re%d" % re, "E": 2, "N": 3,
                    "ops": [fold(rew, None, 2 ** 31 - 5, 8, re, 3), fold(rew, None, 2 ** 31 - 5, 8, re, 0)]})
    # done and reset_every on the same step: one episode, not two; done alone two steps later
    rew = pattern(12, 2, 2, salt=2)
    out.append({"name": "fold_done_and_reset", "E": 2, "N": 2,
                "ops": [fold(rew, done_ring(rew, 0, {0: [3, 5], 1: [7]}), 0, 12, 4, 5)]})
    # reset_every = 1 onto an open episode: truncated, then every step an episode
    rew = pattern(6, 2, 2, salt=3)
    out.append({"name": "fold_reset_every_1", "E": 2, "N": 2, "ops": [fold(rew, None, 0, 4), fold(rew, None, 4, 6, 1, 4)]})
    # a fold that starts on a multiple of reset_every: env 0 closed its episode on the step before (t = 0, not truncated), env 1
    # is four steps in (truncated)
    rew = pattern(9, 2, 2, salt=4)
    out.append({"name": "fold_start_truncation", "E": 2, "N": 2, "ops": [
        fold(rew, done_ring(rew, 4, {0: [3]}), 4, 4), ("drain", True), fold(rew, None, 8, 7, 4, 3)]})
    return out


def _value_cases():
    # five steps, one episode per env (reset_every = 5).  env 0: the special rewards.  env 1: all zero (C = 0, G = 0: NaN).
    # env 2: returns 1, -1, 0, 0 (C = 0, G > 0: -inf).  env 3: C < 0.  env 4: agents 0 and 2 eat, 1 and 3 never do.
    # env 5: the usual pattern.
    rew = pattern(5, 6, 4)
    rew[:, :5] = 0
    rew[:, 0] = np.asarray([[2, 49, 50, 51], [100, -49, -50, -51], [I32_MAX, I32_MIN, 2, 0], [I32_MIN, I32_MAX, 49, 1],
                            [1, 100, 51, I32_MAX]], np.int32)
    rew[1, 2, 0], rew[3, 2, 1] = 1, -1
    rew[0, 3, 0], rew[2, 3, 1] = -50, -1
    rew[[0, 2, 3], 4, 0], rew[[1, 4], 4, 2] = 1, 1
    return [{"name": "values_chunk%d" % c, "E": 6, "N": 4, "ops": [fold(rew, None, 0, 5, 5, c)]} for c in (0, 2)]


def _done_cases():
    # env 0: the bytes of agents 1 and 2 alone, at step 2: no end.  env 1: agent 0's byte alone, at step 3: an end.  env 2: every
    # byte at step 5.  env 3: agent 0 alone at 1, the others alone at 4, all at 6.
    rew = pattern(8, 4, 3, salt=1)
    done = done_ring(rew, 0, {0: [2], 3: [4]}, agents=[1, 2]) | done_ring(rew, 0, {1: [3], 3: [1]}, agents=[0]) | \
        done_ring(rew, 0, {2: [5], 3: [6]})
    return [{"name": "done_bytes_chunk%d" % c, "E": 4, "N": 3, "ops": [fold(rew, done, 0, 8, 0, c)]} for c in (0, 3)]


def _pack_cases():
    out = []
    # 24 steps as one chunk, then 24 more in chunks of 3, on a ring of 31.  Envs e % 3 == 0 never end, e % 3 == 1 end once in a
    # fold and e % 3 == 2 six times, so the neighbours in a wave close episodes at different trips of the chunk loop: the chunk
    # [12, 15) of the second fold holds none, one (13) and three (12, 13, 14).
    for N in PACK_N:
        per = 64 // N
        for E in sorted({1, per, per + 1, 4 * per, 4 * per + 1}):
            rew = pattern(31, E, N, salt=N)
            ends = {e: ([13] if e % 3 == 1 else [4, 5, 12, 13, 14, 22]) for e in range(E) if e % 3}
            out.append({"name": "pack_N%d_E%d" % (N, E), "E": E, "N": N, "ops": [
                fold(rew, done_ring(rew, 5, ends), 5, 24, 0, 0), fold(rew, done_ring(rew, 29, ends), 29, 24, 0, 3)]})
    return out


def _handle_cases():
    # discard(mask) over envs with t == 0 (env 0 has just ended) and t > 0, then discard(None); drains in between
    rew = pattern(6, 3, 2, salt=6)
    mask = np.asarray([1, 1, 0], np.uint8)
    return [{"name": "discards", "E": 3, "N": 2, "ops": [
        fold(rew, done_ring(rew, 0, {0: [5], 2: [2]}), 0, 6), ("discard", mask), ("drain", True), fold(rew, None, 6, 3),
        ("discard", None), ("drain", False), fold(rew, done_ring(rew, 9, {1: [1]}), 9, 4), ("discard", None)]}]


def matrix():
    cases = _chunk_cases() + _batch_cases() + _fold_cases() + _value_cases() + _done_cases() + _pack_cases() + _handle_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def first_fold_case():
    return _fold_cases()[0]
