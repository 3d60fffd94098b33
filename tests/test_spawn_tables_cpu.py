"""Spawn tables without a GPU: the oracle's setter, the fixtures' tables, the engine's argument checks, and the coverage that
the scenarios of tests/spawn_tables.py claim -- the same computations tests/test_spawn_tables_gpu.py asserts beside its
comparisons, so that an edit of a recipe that empties a scenario is caught here."""
import numpy as np
import pytest

import golden_util as G
import spawn_tables as ST
from oracle import pyoracle
from sequential_social_dilemma_games_amd import config as cfgmod
from sequential_social_dilemma_games_amd import constants as K
from sequential_social_dilemma_games_amd import prng
from sequential_social_dilemma_games_amd.engine import VecEngine

TABLE_FIXTURES = [n for n in G.group_names() if n.startswith("t")]


def _run(game, amap, N, set_tables, steps=60, E=8, seed=9):
    ora = pyoracle.Oracle(game, amap, E, N, G.default_lut(), seed=seed)
    set_tables(ora)
    out = [ora.reset()]
    for _ in range(steps):
        act, obs, rew, _ = ora.step_random()
        out += [act, obs, rew, ora.waste_count()]
    st = ora.get_state()
    return out + [st[k] for k in ("world", "pos", "orient", "episode", "t")]


@pytest.mark.parametrize("game,amap", [(K.GAME_HARVEST, K.HARVEST_MAP), (K.GAME_CLEANUP, K.CLEANUP_MAP)])
def test_default_tables_set_explicitly_change_nothing(game, amap):
    """The reference's constants as explicit tables, tables set and taken back, and no call at all: identical runs.  (Cleanup
    from a world cleaned to below the depletion threshold would be busier; 60 random steps at the shipped start cover the
    derivation's three branches only through the tables compared entry by entry below.)"""
    h, c = ST.default_tables(amap)
    base = _run(game, amap, 5, lambda o: None)
    explicit = _run(game, amap, 5, lambda o: o.set_tables(harvest=h, cleanup=c))

    def set_and_take_back(o):
        o.set_tables(harvest=ST.H_ALWAYS, cleanup=ST.c_parity(amap) if game == K.GAME_CLEANUP else None)
        o.set_tables()
    back = _run(game, amap, 5, set_and_take_back)
    for a, b, c2 in zip(base, explicit, back):
        assert np.array_equal(a, b) and np.array_equal(a, c2)
    if game == K.GAME_CLEANUP:                       # the derived thresholds, entry by entry, are the explicit table's
        ora = pyoracle.Oracle(game, amap, 1, 0, G.default_lut())
        for n in range(ora.potential_waste_area + 1):
            assert ora.cleanup_thresholds(n) == (int(c[0][n]), int(c[1][n]))
        assert len(set(c[0].tolist())) > 10 and c[0][0] == prng.threshold(0.05) and c[0][-1] == 0


def test_explicit_default_tables_from_a_cleaned_river():
    """The same identity where the Cleanup tables are read at many counts: from worlds with 0 .. potential cells of waste."""
    amap, E = K.CLEANUP_MAP, 120
    case = ST.Case("x", K.GAME_CLEANUP, amap, E, 5, 0, None, None, 0)
    runs = []
    for explicit in (False, True):
        ora = pyoracle.Oracle(K.GAME_CLEANUP, amap, E, 5, G.default_lut(), seed=4)
        if explicit:
            h, c = ST.default_tables(amap)
            ora.set_tables(harvest=h, cleanup=c)
        ora.reset()
        ora.set_state(world=ST._waste_world(case, ora.get_state(), np.random.RandomState(1), lambda e, p: e % (p + 1)))
        out, used = [], set()
        for _ in range(20):
            out += list(ora.step_random()[1:3])
            used |= set(ora.waste_count().tolist())
        runs.append(out + [ora.get_state()["world"]])
    assert len(used) == ST.potential(amap) + 1
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_oracle_setter_rejects_bad_tables():
    ora = pyoracle.Oracle(K.GAME_CLEANUP, K.CLEANUP_MAP, 1, 1, G.default_lut())
    with pytest.raises(ValueError):
        ora.set_tables(harvest=np.zeros(3, np.uint64))
    with pytest.raises(ValueError):
        ora.set_tables(cleanup=(np.zeros(5, np.uint64), np.zeros(5, np.uint64)))


def test_oracle_indexes_past_the_tables_end_as_the_kernel_clamps():
    """More 'H' cells than waste points (waste on stream cells): the count lies past the tables' end and the last entry is used."""
    amap = K.CLEANUP_MAP
    P = ST.potential(amap)
    apple, waste = np.zeros(P + 1, np.uint64), np.zeros(P + 1, np.uint64)
    apple[P] = ST.T32                                # only the last entry grows apples
    ora = pyoracle.Oracle(K.GAME_CLEANUP, amap, 1, 0, G.default_lut())
    ora.set_tables(cleanup=(apple, waste))
    ora.reset()
    case = ST.Case("x", K.GAME_CLEANUP, amap, 1, 0, 0, None, None, 0)
    ora.set_state(world=ST._waste_world(case, ora.get_state(), np.random.RandomState(0), lambda e, p: p + 6))
    ora.step(np.zeros((1, 0), np.int32))
    assert ora.waste_count()[0] == P + 6
    w = ora.get_state()["world"][0]
    assert (w == ord("A")).sum() == sum(r.count("B") for r in amap)


@pytest.mark.parametrize("name", TABLE_FIXTURES)
def test_fixture_tables_are_the_thresholds_of_the_recorded_probabilities(name):
    """A fixture recorded with the reference's constants rebound carries the probabilities and the thresholds; the thresholds
    must be prng.threshold of the probabilities (Cleanup: of compute_probabilities, cleanup.py:156-171, at every count)."""
    g = G.load(name)
    assert g.tables, name
    if "harvest" in g.tables:
        want = [prng.threshold(float(p)) for p in g.tables["harvest_p"]]
        assert g.tables["harvest"].dtype == np.uint64 and g.tables["harvest"].tolist() == want
    else:
        apple_p, waste_p, depletion, restoration = (float(x) for x in g.tables["cleanup_consts"])
        P = cfgmod.potential_waste_area(g.map)
        assert len(g.tables["cleanup_apple"]) == len(g.tables["cleanup_waste"]) == P + 1
        for n in range(P + 1):
            density = 1 - (P - n) / P
            if density >= depletion:
                pa, pw = 0, 0
            elif density <= restoration:
                pa, pw = apple_p, waste_p
            else:
                pa, pw = (1 - (density - restoration) / (depletion - restoration)) * apple_p, waste_p
            assert int(g.tables["cleanup_apple"][n]) == prng.threshold(pa), n
            assert int(g.tables["cleanup_waste"][n]) == prng.threshold(pw), n


def test_table_fixtures_are_there():
    tags = sorted(n.split("_v")[1][2:] for n in TABLE_FIXTURES)
    assert tags == ["allspawn", "count", "count", "dense", "dense", "nowaste"], TABLE_FIXTURES


def test_fixture_replay_needs_its_tables():
    """The replay of a table fixture fails without the tables: the fixtures do pin the setter."""
    g = G.load([n for n in TABLE_FIXTURES if n.endswith("count")][0])
    o = pyoracle.Oracle(g.game, g.map, 1, g.N, G.default_lut(), view_len=g.view_len, seed=g.seed, env_base=g.env)
    s, differs = g.steps, 0
    for k in range(g.n_steps):
        o.set_state(world=s["pre_world"][k][None], beam=np.zeros_like(s["pre_world"][k][None]), pos=s["pre_pos"][k][None],
                    orient=s["pre_orient"][k][None], episode=np.array([s["episode"][k]], np.uint32),
                    t=np.array([s["t"][k] - 1], np.uint32))
        o.step(s["act"][k][None], order=s["order"][k][None])
        differs += not np.array_equal(o.get_state()["world"][0], s["world"][k])
    assert differs > g.n_steps // 2


@pytest.mark.parametrize("kw", [
    dict(harvest_thresholds=[1, 2, 3, 4]),                                       # not an array
    dict(harvest_thresholds=np.zeros(4, np.int64)),                              # not uint64
    dict(harvest_thresholds=np.zeros(5, np.uint64)),                             # not 4 entries
    dict(cleanup_thresholds=np.zeros(120, np.uint64)),                           # not a pair
    dict(cleanup_thresholds=(np.zeros(120, np.uint64), np.zeros(119, np.uint64))),   # not potential_waste_area + 1 entries
    dict(cleanup_thresholds=(np.zeros(120, np.uint32), np.zeros(120, np.uint32))),
    dict(library_tables=True, harvest_thresholds=np.zeros(4, np.uint64)),        # exclusive
    dict(library_tables=True, cleanup_thresholds=(np.zeros(120, np.uint64), np.zeros(120, np.uint64))),
])
def test_engine_checks_its_tables_before_it_creates_anything(kw, monkeypatch):
    """ValueError on the host, before ssd_create (which would need the library -- and a device -- to be reached at all)."""
    from sequential_social_dilemma_games_amd import _capi

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_capi, "lib", no_library)
    assert ST.potential(K.CLEANUP_MAP) == 119
    with pytest.raises(ValueError):
        VecEngine(K.GAME_CLEANUP, K.CLEANUP_MAP, num_envs=1, num_agents=1, **kw)


@pytest.mark.parametrize("name", [c.name for c in ST.CASES])
def test_scenarios_reach_what_they_claim(name):
    """The coverage guards on the oracle alone: more than 64 and 1..64 empty apple points, adjacent same-step apples in at least
    5 % of the env-steps, 20 distinct waste counts, waste under an agent, ... (spawn_tables.check_guards), per case."""
    case = ST.BY_NAME[name]
    fig = ST.check_guards(case, ST.trajectory(name))
    print(name, fig)


def test_library_tables_run_indexes_every_entry():
    """The Cleanup run of the library-tables test reads the thresholds at every count 0 .. potential_waste_area."""
    case = ST.library_case(K.GAME_CLEANUP)
    assert ST.library_case_counts(case) >= set(range(ST.potential(case.amap) + 1))
