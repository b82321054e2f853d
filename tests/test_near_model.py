"""
The near-solved table's NumPy model (tests/near_model.py) against what is known about the cube and against the reference's own
queues, the pure planning step of librubiks/solving/near.py, and the ctypes mirrors against the compiled structs.  No GPU.
"""
import ctypes
import os

import numpy as np
import pytest

import near_model as nm
from conftest import GOLDEN
from near_model import DETOUR, F_, L_, R_, T_, B_, f_, r_, t_
from oracle import cube as oc


@pytest.fixture(scope="module")
def m5():
    return nm.NearModel(5)


@pytest.fixture(scope="module")
def fixtures():
    mcts, egvm = nm.fixture_queues(GOLDEN)
    assert len(mcts) == 54 and len(egvm) == 15
    return mcts, egvm


def test_sphere_sizes_are_the_quarter_turn_counts(m5, golden):
    assert m5.counts == [1, 12, 114, 1068, 10011, 93840] and m5.n_nodes == 105046
    assert len(np.unique(m5.states, axis=0)) == m5.n_nodes                       # a state is one node
    assert list(m5.node_depth[:13]) == [0] + [1] * 12 and list(m5.node_action[:13]) == [0] + list(range(12))
    # a shallower table is the deeper one's beginning, and the committed move-table fixture builds the same table as oracle.cube
    m3 = nm.NearModel(3, lut=nm.lut_from_deltas(golden["maps"]))
    n3 = m3.n_nodes
    assert n3 == 1195 and np.array_equal(m3.states, m5.states[:n3]) and np.array_equal(m3.node_action, m5.node_action[:n3])
    assert np.array_equal(m3.node_depth, m5.node_depth[:n3])


def test_solve_is_optimal_for_every_state_of_depth_three():
    m3, m2 = nm.NearModel(3), nm.NearModel(2)
    queues, lens = m3.solve(m3.states)
    assert np.array_equal(lens, m3.node_depth)
    for v in range(m3.n_nodes):
        assert len(queues[v]) == m3.node_depth[v] and oc.is_solved(nm.replay(m3.states[v], queues[v]))
        assert np.array_equal(nm.replay(oc.get_solved(), m3.sequence(v)), m3.states[v])
        assert (m2.node(m3.states[v]) < 0) == (m3.node_depth[v] == 3)            # no shorter queue: not in the table one level down
    beyond = m3.next_level()[:50]
    assert (m3.depths(beyond) == -1).all() and (m3.solve(beyond)[1] == -1).all() and (nm.NearModel(4).depths(beyond) == 4).all()


def test_tighten_on_constructed_queues(m5):
    for m in (nm.NearModel(1), nm.NearModel(3), m5):
        assert m.tighten_one([R_, r_]) == []
        assert m.tighten_one([R_, F_, f_, r_], window=4) == [] and m.tighten_one([R_, F_, f_, r_]) == []
        assert m.tighten_one([R_, F_, f_, r_], window=1) == [R_, F_, f_, r_]
        assert m.tighten_one([R_, R_, R_]) == [r_]
        assert m.tighten_one([]) == [] and m.tighten_one([T_]) == [T_]
    assert m5.tighten_one([R_, F_, f_, r_], window=3) == [R_, r_]              # (the stretch F f goes, and R .. r is then out of reach)


def test_a_detour_of_depth_two_loses_four_moves_from_depth_two_on(m5):
    for a, b in ((F_, F_), (T_, B_), (F_, t_)):
        q = [a] + DETOUR + [b]
        assert nm.NearModel(1).tighten_one(q) == q and m5.tighten_one(q, depth=1) == q
        for K in (2, 3, 4, 5):
            got = m5.tighten_one(q, depth=K)
            assert len(got) == len(q) - 4
            if K == 2:                                                          # (deeper tables may also rewrite a .. or .. b)
                assert got[0] == a and got[-1] == b and sorted(got[1:3]) == [9, 11]   # r l, in the table's order
            assert np.array_equal(nm.replay(oc.get_solved(), got), nm.replay(oc.get_solved(), q))
        assert nm.NearModel(2).tighten_one(q) == m5.tighten_one(q, depth=2)
        assert len(m5.tighten_one(q, window=5, depth=2)) == len(q)              # at depth 2 no stretch of the detour but the whole is near


def test_a_tie_goes_to_the_smallest_start():
    # R L R at K = 2: best[2] is 2 by (0, 2) and by (1, 2), best[3] is 3 by (1, 3) and by (2, 3).  The smallest start keeps
    # R + table(L R); the other choice would give table(R L) + R.  R L and L R are one state, which L (the lower parent) discovers.
    m2 = nm.NearModel(2)
    v = m2.node(nm.replay(oc.get_solved(), [R_, L_]))
    assert m2.sequence(v) == [L_, R_]
    assert m2.tighten_one([R_, L_, R_]) == [R_, L_, R_]
    assert m2.tighten_one([L_, R_, L_]) == [L_, L_, R_]


def test_fixture_queues_get_no_longer_and_keep_their_product(m5, fixtures):
    mcts, egvm = fixtures
    rng = np.random.RandomState(0)
    for K in (4, 5):
        for name, queues in (("mcts", mcts), ("egvm", egvm)):
            rows, status = m5.tighten(queues, depth=K)
            assert (status == nm.OK).all()
            root = nm.replay(oc.get_solved(), rng.randint(0, 12, 30))
            for q, row in zip(queues, rows):
                assert len(row) <= len(q) and np.array_equal(nm.replay(root, row), nm.replay(root, q))
            before, after = sum(map(len, queues)), sum(map(len, rows))
            print(f"{name} K={K}: mean {before / len(queues):.2f} -> {after / len(rows):.2f}")
            if name == "mcts" and K == 5:
                assert after < before
    rows, _ = m5.tighten(mcts, depth=4, window=7)
    assert sum(map(len, rows)) >= sum(map(len, m5.tighten(mcts, depth=4)[0]))  # a window only takes choices away


def test_status_codes_for_a_bad_byte_and_unselected_games(m5):
    queues = [[R_, r_], [R_, 12, r_], [R_, r_, T_], [F_, f_]]
    rows, status = m5.tighten(queues, select=[True, True, True, False])
    assert list(status) == [nm.OK, nm.BAD_ACTION, nm.OK, nm.SKIPPED]
    assert rows == [[], [R_, 12, r_], [T_], [F_, f_]]


def test_planning_is_pure_and_respects_the_budget():
    from librubiks.solving.near import band_bytes, plan_tighten_chunks, workspace_bytes
    lens = np.array([100, -1, 0, 300, 64, 7])
    assert list(band_bytes(lens)) == [10000, 0, 0, 90000, 4096, 49] and list(band_bytes(lens, 32)) == [3200, 0, 0, 9600, 2048, 49]
    assert workspace_bytes(100, 11) == 256 + 2 * 256 and workspace_bytes(0, 1) == 512
    assert plan_tighten_chunks(lens) == [(0, 6)] and plan_tighten_chunks([]) == []
    one = workspace_bytes(90000, 301)
    chunks = plan_tighten_chunks(lens, None, one)
    assert chunks == [(0, 3), (3, 4), (4, 6)]
    for lo, hi in chunks:
        eff = lens[lo:hi]
        assert workspace_bytes(band_bytes(eff).sum(), np.where(eff < 0, 0, eff + 1).sum()) <= one
    assert plan_tighten_chunks(lens, 32, one) == [(0, 6)]
    with pytest.raises(ValueError):
        plan_tighten_chunks(lens, None, one - 1)
    assert plan_tighten_chunks(lens, None, one) == chunks                       # nothing but its arguments decides


def test_struct_mirrors_have_the_compiled_sizes():
    from librubiks import _hip
    from librubiks.solving import near
    lib = _hip.load()
    assert lib.rc_near_struct_bytes() == ctypes.sizeof(near._NearStruct)
    assert lib.rc_near_tighten_struct_bytes() == ctypes.sizeof(near._TightenStruct)
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "rubiks_hip.h")).read()
    for mirror, name in ((near._NearStruct, "rc_near"), (near._TightenStruct, "rc_near_tighten")):
        body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name}_t;")]
        import re
        declared = re.findall(r"^\s+(?:const\s+)?\w+\s+\*?(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
        assert [f.rstrip("_") for f, _ in mirror._fields_] == declared
    assert (near.OK, near.SKIPPED, near.BAD_ACTION, near.FAILED, near.NO_ROOM) == (nm.OK, nm.SKIPPED, nm.BAD_ACTION, nm.FAILED, nm.NO_ROOM)
    assert sum(near.SPHERE_SIZES[:7]) == 983926 and near.MAX_DEPTH == 8
    with pytest.raises(ValueError):
        near.NearTable.__init__(near.NearTable.__new__(near.NearTable), depth=9)
