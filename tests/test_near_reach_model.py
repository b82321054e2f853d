"""
The rule of the search beyond the near-solved table (tests/near_reach_model.py), checked against what a deeper table knows: with
the depth-5 dict cut at K and J more moves walked, every state gets its own depth when that is <= K + J and -1 otherwise; the
solutions solve; leaving out the sequences the device does not walk changes nothing, the tie included; the per-launch model ends
where the rule ends whatever the ranges and the prefix length; and the ctypes mirror of rc_near_reach_t has the compiled size.
"""
import ctypes

import numpy as np
import pytest

import near_model as nm
import near_reach_model as rm
from oracle import cube as oc

SPLITS = [(2, 2), (1, 3), (3, 2), (2, 3)]


@pytest.fixture(scope="module")
def m5():
    return nm.NearModel(5)


@pytest.fixture(scope="module")
def reach5(m5):
    return rm.ReachModel(m5)


@pytest.fixture(scope="module")
def sample(m5):
    pick = np.random.RandomState(0).choice(np.arange(127, m5.n_nodes), 300, replace=False)
    return np.concatenate([np.arange(127), np.sort(pick)])


def test_canonical_counts():
    # 12, then every move but the inverse and (after the higher of two opposite faces) the two of the lower face
    assert [int(rm.canonical(j).sum()) for j in range(3)] == [1, 12, 12 * 11 - 6 * 2]
    assert rm.digits(9 * 144 + 11 * 12 + 1, 3) == [9, 11, 1]
    # ... and sequence by sequence, the three rules spelled out on the moves' names
    names, opposite = "FfBbTtDdLlRr", {"F": "B", "T": "D", "L": "R"}
    for j in (3, 4):
        for index in range(12 ** j):
            q = [names[a] for a in rm.digits(index, j)]
            bad = any(a != b and a.upper() == b.upper() for a, b in zip(q, q[1:]))
            bad |= any(a == b == c for a, b, c in zip(q, q[1:], q[2:]))
            bad |= any(opposite.get(b.upper()) == a.upper() for a, b in zip(q, q[1:]))
            assert rm.canonical(j)[index] == (not bad), q


@pytest.mark.parametrize("K,J", SPLITS)
def test_every_state_gets_its_own_depth(m5, reach5, sample, K, J):
    states, own = m5.states[sample], m5.node_depth[sample].astype(np.int64)
    want = np.where(own <= K + J, own, -1)
    assert (want == -1).sum() > 20 or K + J == 5
    dist, levels, lengths, queues = reach5.reach(states, J, depth=K)
    assert np.array_equal(dist, want) and np.array_equal(lengths, want)
    assert np.array_equal(levels, np.where(want >= 0, np.maximum(own - K, 0), -1))          # the first level with a hit is max(0, D - K)
    for s, q, d in zip(states, queues, dist):
        assert len(q) == max(d, 0) and (d < 0 or oc.is_solved(nm.replay(s, q)))
    # the sequences the device leaves out change nothing, the tie included
    pruned = reach5.reach(states, J, depth=K, pruned=True)
    assert np.array_equal(pruned[0], dist) and np.array_equal(pruned[1], levels) and pruned[3] == queues


@pytest.mark.parametrize("K,J", SPLITS)
def test_depth_six_is_beyond_five(m5, reach5, K, J):
    far = m5.next_level()[:40]
    for pruned in (False, True):
        dist, levels, _, queues = reach5.reach(far, J, depth=K, pruned=pruned)
        assert (dist == -1).all() and (levels == -1).all() and queues == [[]] * 40
    if (K, J) == (3, 2):                                                                  # one more move reaches them
        dist, levels, _, queues = reach5.reach(far, 3, depth=3)
        assert (dist == 6).all() and (levels == 3).all()
        assert all(len(q) == 6 and oc.is_solved(nm.replay(s, q)) for s, q in zip(far, queues))


def test_the_tie_goes_to_the_smallest_index(m5, reach5):
    state = nm.replay(oc.get_solved(), [nm.R_, nm.L_])
    for pruned in (False, True):
        dist, levels, _, queues = reach5.reach([state], 1, depth=1, pruned=pruned)
        assert dist[0] == 2 and levels[0] == 1 and queues[0] == [nm.l_, nm.r_]           # l (9) first, not r (11)
    assert rm.canonical(2)[nm.L_ * 12 + nm.R_] and not rm.canonical(2)[nm.R_ * 12 + nm.L_]


def test_no_extra_moves_is_depths_and_solve(m5, reach5, sample):
    states = np.concatenate([m5.states[sample], m5.next_level()[:10]])
    for K in (2, 5):
        dist, levels, lengths, queues = reach5.reach(states, 0, depth=K)
        assert np.array_equal(dist, m5.depths(states, depth=K)) and np.array_equal(levels, np.where(dist >= 0, 0, -1))
        want_q, want_l = m5.solve(states)
        assert all(q == (w if d >= 0 else []) for q, w, d in zip(queues, want_q, dist))
        assert np.array_equal(lengths, np.where(dist >= 0, want_l, -1))


@pytest.mark.parametrize("P,per", [(0, 5), (1, 1), (2, 7), (2, 145), (3, 100000)])
def test_launches_end_where_the_rule_ends(m5, reach5, P, per):
    rng = np.random.RandomState(3)
    states = np.concatenate([m5.states[[0, 5, 77]], m5.states[rng.choice(np.arange(127, m5.n_nodes), 9, replace=False)], m5.next_level()[:2]])
    K, J = 2, 3
    run = rm.Launches(reach5, states, P, depth=K)
    run.begin()
    assert run.unresolved() == (m5.depths(states, depth=K) < 0).sum()
    for level in range(1, J + 1):
        if run.unresolved() == 0:
            break
        for first in range(0, run.items(level), per):
            run.level(level, first, min(per, run.items(level) - first))
    dist, levels, _, _ = reach5.reach(states, J, depth=K)
    for i, w in enumerate(run.best):
        if dist[i] < 0:
            assert w == rm.NO_WORD
        else:
            d, level, index = rm.unpack(w)
            assert (d + level, level) == (dist[i], levels[i]) and w == reach5.best(states[i], level, K)


def test_struct_mirror_and_item_counts():
    """Host-only calls: no GPU needed."""
    from librubiks import _hip
    from librubiks.solving import near
    lib = _hip.load()
    assert lib.rc_near_reach_struct_bytes() == ctypes.sizeof(near._ReachStruct)
    assert near.MAX_EXTRA == rm.MAX_EXTRA == 10 and int(near.NO_WORD) == int(rm.NO_WORD)
    for level in range(12):
        for P in range(12):
            want = 12 ** min(level, P) if max(level, P) <= 10 else 0
            assert lib.rc_near_reach_items(level, P) == want
            if want:
                assert near.reach_items(level, P) == want
    assert near.default_prefix(1024, 8) == 5 and near.default_prefix(1, 2) == 2 and near.default_prefix(1 << 22, 3) == 0
    assert near.default_launch_items(8, 5) == near.DEFAULT_LAUNCH_LEAVES // 1728 and near.default_launch_items(2, 5) == near.DEFAULT_LAUNCH_LEAVES
