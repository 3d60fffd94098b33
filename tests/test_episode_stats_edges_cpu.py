"""The case matrix of the episode-statistics fold (episode_stats_cases.py) without a GPU: that it reaches every path of the two
passes it was built for (features() reads them off the cases' arrays), every lane-packing pair, and the conditions on the
reference's side -- the pos * t shift of a chunk's head changes sustainability, nothing leaves int64 -- and that RefStats gives
the same drains whether a case's steps are folded as the case has them or one by one."""
import numpy as np
import pytest

import episode_stats_cases as cases
from episode_stats_ref import RefStats, metrics, same

MATRIX = cases.matrix()
INFO = {}
FEATURES = {}
for _c in MATRIX:
    INFO[_c["name"]] = {}
    FEATURES[_c["name"]] = cases.features(_c, INFO[_c["name"]])
REFERENCE = {}


def reference(case):
    """The reference's drains of a case, computed once and shared."""
    if case["name"] not in REFERENCE:
        REFERENCE[case["name"]] = cases.run(RefStats(case["E"], case["N"]), case)
    return REFERENCE[case["name"]]


def test_the_matrix_reaches_every_path():
    reached = set().union(*FEATURES.values())
    missing = [f for f in cases.REQUIRED if f not in reached]
    assert not missing, missing
    assert len(cases.REQUIRED) == len(set(cases.REQUIRED)) == 58
    # the paths that must meet in one case
    assert {"reread_wraps", "consecutive_ends", "chunk_ends_3plus"} <= FEATURES["chunks_wrap_in_reread"]
    assert {"step0_near_2^31", "fold_start_on_t0"} <= FEATURES["fold_step0_near_2^31_re3"]
    assert {"no_end_fold_carried", "fold_last_step_end", "n_steps_eq_ring", "step0_ge_ring"} <= FEATURES["fold_carry"]
    assert {"fold_start_truncates_open", "fold_start_on_t0"} <= FEATURES["fold_start_truncation"]
    assert {"fold_start_truncates_open", "reset_every_1"} <= FEATURES["fold_reset_every_1"]
    for L in cases.BATCH_L:
        assert "L_%d" % L in FEATURES["batch_L%d_wrap_inside" % L] and "L_%d" % L in FEATURES["batch_L%d_wrap_between" % L]


def test_every_lane_packing_pair_is_present():
    reached = set().union(*FEATURES.values())
    assert len(cases.PACK_PAIRS) == 55
    missing = [p for p in cases.PACK_PAIRS if ("pack",) + p not in reached]
    assert not missing, missing
    for c in MATRIX:
        if not c["name"].startswith("pack_"):
            continue
        F, per = FEATURES[c["name"]], 64 // c["N"]
        assert {"L_24", "L_3", "chunk_ends_0"} <= F and ({"chunk_ends_1", "chunk_ends_3plus"} <= F) == (c["E"] >= 3), c["name"]
        # neighbours in one wave close episodes at different trips of the chunk loop wherever a wave has neighbours
        assert ("wave_neighbours_differ" in F) == (per >= 2 and c["E"] >= 2), c["name"]
        assert ("wave_has_0_1_many" in F) == (per >= 3 and c["E"] >= 3), c["name"]


def test_the_cases_stay_small_and_inside_int64():
    for c in MATRIX:
        info = INFO[c["name"]]
        assert info["agent_steps"] < 5 * 10 ** 4, c["name"]
        assert info["peak"] < 2 ** 62, c["name"]                 # G, 2 N C and the tsums, as Python integers
    assert INFO["values_chunk0"]["peak"] > 2 ** 33              # (the int32 extremes are in there)


def test_features_read_the_cases_as_the_reference_does():
    """The episodes features() closes are the reference's: count, lengths and collective returns per env."""
    for c in MATRIX:
        if any(kind == "drain" and not keep for kind, keep in c["ops"]):
            continue                                             # (a clearing drain in the middle: the last drain is partial)
        counts = reference(c)[-1]["counts"]
        eps = INFO[c["name"]]["episodes"]
        for e in range(c["E"]):
            mine = [x for x in eps if x["e"] == e]
            assert [len(mine), sum(x["T"] for x in mine), sum(sum(x["R"]) for x in mine)] == counts[e, [0, 2, 3]].tolist(), c["name"]


def test_the_shift_of_a_head_changes_sustainability():
    """A chunk's head with a positive reward appended to an open episode: without pos * t the episode's sustainability differs,
    and the reference has the shifted one."""
    c = next(x for x in MATRIX if x["name"] == "chunks")
    assert {"head_pos_onto_open_t", "tsum_shift_changes_S"} <= FEATURES["chunks"]
    ep = [x for x in INFO["chunks"]["episodes"] if x["e"] == 1]
    assert len(ep) == 1 and ep[0]["T"] == 7 and ep[0]["tsum"] != ep[0]["tsum_unshifted"]
    N = c["N"]
    S = metrics(ep[0]["R"], ep[0]["pos"], ep[0]["tsum"], [0] * N, 7)[2]
    S_unshifted = metrics(ep[0]["R"], ep[0]["pos"], ep[0]["tsum_unshifted"], [0] * N, 7)[2]
    got = reference(c)[-1]["last_metrics"][1, 2]
    assert np.isfinite(S) and np.isfinite(S_unshifted) and S != S_unshifted and got == S


def test_the_value_cases_give_the_non_finite_metrics():
    d = reference(next(x for x in MATRIX if x["name"] == "values_chunk0"))[-1]
    eq = d["last_metrics"][:, 1]
    assert np.isnan(eq[1]) and eq[2] == -np.inf and d["counts"][3, 3] < 0 and d["counts"][2, 3] == 0
    assert d["metric_counts"][1, 1] == 0 and d["metric_counts"][2, 1] == 0
    assert np.isnan(d["last_metrics"][1, 2]) and np.isfinite(d["last_metrics"][4, 2])
    # r = 2 .. INT32_MAX: negative "hits", floor not truncation: (1 - 2) // 50 = -1, (1 - 49) // 50 = -1, (1 - 100) // 50 = -2
    assert d["agent_sums"][0, 1, 2] == (1 - 50) // 50 + (1 + 50) // 50 + (1 - 2) // 50 + (1 - 49) // 50 + (1 - 51) // 50 == -3


@pytest.mark.parametrize("case", MATRIX, ids=[c["name"] for c in MATRIX])
def test_one_call_and_its_pieces_fold_alike(case):
    pieces = cases.run(RefStats(case["E"], case["N"]), cases.in_pieces(case))
    whole = reference(case)
    assert len(pieces) == len(whole) and all(same(a, b) for a, b in zip(pieces, whole))
