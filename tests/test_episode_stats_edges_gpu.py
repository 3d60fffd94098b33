"""The device fold of the episode statistics (csrc/ssd_stats.hip) against the sequential restatement (episode_stats_ref.py), bit
for bit, on the case matrix built from the branch points of its two passes (episode_stats_cases.py; what each case reaches is
asserted in test_episode_stats_edges_cpu.py), on the handle's own paths -- drains that keep, a scratch that shrinks and grows,
a side stream, drains with output pointers left NULL -- and at chunk lengths above n_steps up to 2^31 - 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_stats_cases as cases
from episode_stats_ref import RefStats, same
from sequential_social_dilemma_games_amd import _capi
from sequential_social_dilemma_games_amd.episode_stats import EpisodeStats

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MATRIX = cases.matrix()
REFERENCE = {}
KEYS = ("counts", "agent_sums", "metric_sums", "metric_counts", "last_len", "last_ret", "last_metrics")


def to_device(a):
    return torch.from_numpy(a).to(DEV)


def reference(case):
    """The restatement's drains of a case, computed once and shared."""
    if case["name"] not in REFERENCE:
        REFERENCE[case["name"]] = cases.run(RefStats(case["E"], case["N"]), case)
    return REFERENCE[case["name"]]


def differing(got, want):
    return [(n, k, g[k], w[k]) for n, (g, w) in enumerate(zip(got, want)) for k in g if not same(g[k], w[k])]


@pytest.mark.parametrize("case", MATRIX, ids=[c["name"] for c in MATRIX])
def test_matrix_case_folds_to_the_restatement(case):
    got, want = cases.run(EpisodeStats(case["E"], case["N"]), case, to_device), reference(case)
    assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want)), differing(got, want)


@pytest.mark.parametrize("chunk_of", [lambda n: n, lambda n: n + 1, lambda n: 2 ** 30, lambda n: 2 ** 31 - 1],
                         ids=["n_steps", "n_steps+1", "2^30", "2^31-1"])
def test_a_chunk_above_n_steps_acts_as_n_steps(chunk_of):
    case = cases.first_fold_case()
    auto = cases.run(EpisodeStats(case["E"], case["N"]), case, to_device, chunk_of=lambda n: 0)
    got = cases.run(EpisodeStats(case["E"], case["N"]), case, to_device, chunk_of=chunk_of)
    assert all(same(g, a) for g, a in zip(got, auto)), differing(got, auto)
    assert all(same(g, w) for g, w in zip(got, reference(case))), differing(got, reference(case))


def _closed_fold(E, N, n, salt):
    """n steps that leave no episode open: reset_every = n ends every env on the last step; done ends some before."""
    rew = cases.pattern(n, E, N, salt=salt)
    done = cases.done_ring(rew, 0, {e: [(e * 7 + salt) % n, (e * 7 + salt + 1) % n][:1 + (e // 2) % 2] for e in range(0, E, 2)})
    return rew, done


def test_keeping_drains_then_a_clearing_one():
    E, N = 5, 3
    rew, done = _closed_fold(E, N, 20, 1)
    st, ref = EpisodeStats(E, N), RefStats(E, N)
    st.set_chunk(4)
    st.fold(to_device(rew), to_device(done), reset_every=20)
    ref.fold(rew, done, reset_every=20)
    want = ref.drain()
    for keep in (True, True, False):
        assert same(st.drain(keep=keep), want)
    assert same(st.drain(), ref.drain()) and not st.drain()["counts"].any()


def test_a_scratch_that_shrinks_and_grows_again():
    """A fold of 200 chunks, one of a single chunk, one of 67 chunks of another length on one handle: each as on a fresh one."""
    E, N = 37, 5
    st = EpisodeStats(E, N)
    for n, chunk, salt in ((200, 1, 2), (5, 0, 3), (200, 3, 4)):
        rew, done = _closed_fold(E, N, n, salt)
        fresh, ref = EpisodeStats(E, N), RefStats(E, N)
        for s in (st, fresh):
            s.set_chunk(chunk)
            s.fold(to_device(rew), to_device(done), reset_every=n)
        ref.fold(rew, done, reset_every=n)
        got, alone, want = st.drain(), fresh.drain(), ref.drain()
        assert same(got, want) and same(alone, want), (n, chunk)
        assert int(want["counts"][:, 0].sum()) > E and not want["counts"][:, 1].any()


def test_a_fold_on_a_side_stream():
    E, N = 37, 5
    rew, done = _closed_fold(E, N, 40, 5)
    st, ref = EpisodeStats(E, N), RefStats(E, N)
    r, d = to_device(rew), to_device(done)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        st.set_chunk(7)
        st.fold(r, d, reset_every=40)
        got = st.drain()
    ref.fold(rew, done, reset_every=40)
    assert same(got, ref.drain())


def test_drain_with_output_pointers_left_null():
    """ssd_stats_drain: "any may be NULL".  One output at a time equals the full drain's, the others untouched because absent;
    under SSD_STATS_KEEP the handle is unchanged, also after a drain with every pointer NULL; without it, that drain clears."""
    E, N = 5, 3
    rew, done = _closed_fold(E, N, 20, 6)
    st = EpisodeStats(E, N)
    st.fold(to_device(rew), to_device(done), reset_every=20)
    full = st.drain(keep=True)
    assert full["counts"][:, 0].all()
    L, stream = _capi.lib(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for idx, key in enumerate(KEYS):
        buf = torch.from_numpy(np.full(full[key].shape, 77, full[key].dtype)).to(DEV)
        ptrs = [None] * 7
        ptrs[idx] = C.c_void_p(buf.data_ptr())
        assert L.ssd_stats_drain(st._h, *ptrs, _capi.SSD_STATS_KEEP, stream) == 0
        assert same(buf.cpu().numpy(), full[key]), key
    assert L.ssd_stats_drain(st._h, *([None] * 7), _capi.SSD_STATS_KEEP, stream) == 0
    assert same(st.drain(keep=True), full)
    assert L.ssd_stats_drain(st._h, *([None] * 7), 0, stream) == 0
    cleared = st.drain()
    assert not any(cleared[k].any() for k in KEYS)
