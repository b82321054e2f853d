"""
The NumPy model of the batched BFS kernels (tests/bfs_batch_model.py) on the CPU.  Every game that the scenarios of
tests/test_bfs_batch_kernels_gpu.py put through the model -- same slot count, chunks, node rows and caps -- ends as
oracle.agents.BFS ends it: solved flag, len(agent) and the action queue, and after every step the node rows the model has committed
are a prefix of the oracle's discovery order.  That is what makes the model a reference rather than a copy of the kernels.  Also
here, because it needs no GPU: the scenarios reach every case they are meant to reach (the seeds are chosen here), and the host's
check of a block of per-slot words (`bfs_batch_device.check_words`) on hand-made blocks.
"""
import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
import bfs_batch_model as bm


def drive(m: bm.BfsBatchModel, scenario, pinned: bool = True) -> list:
    """Applies the scenario to the model; with `pinned`, compares every tenant with the oracle.  -> the calls' ops."""
    tenant, ops = {}, []

    def settle(s):
        root, ms = tenant.pop(s)
        ok, seen, queue, _ = bm.oracle_game(root.tobytes(), ms)
        if m.status(s) != bm.FAILED:   # (the reference has no queue row to overflow and no words to corrupt)
            assert m.game(s) == (ok, seen, queue), (s, m.words[:, s].tolist())

    for call in scenario:
        if call["op"] == "plant" and pinned:
            for i, s in enumerate(call["slots"].tolist()):
                if 0 <= s < m.S:
                    if s in tenant:
                        assert m.status(s) != bm.RUNNING
                        settle(s)
                    tenant[s] = ((call["roots"][i].astype(np.int64) & 31).astype(np.int8), min(int(call["max_states"][i]), m.room))
        bm.apply(m, call)
        ops.append(call["op"])
        if call["op"] == "step" and pinned:
            for s, (root, _) in tenant.items():
                n = int(m.committed[s])
                order = bm.oracle_game(root.tobytes(), m.cap)[3]
                if m.status(s) not in (bm.ROOT_SOLVED, bm.FAILED):
                    assert n <= len(order) and [k.tobytes() for k in m.states[s, :n]] == order[:n], (s, n)
                    index = {k: i for i, k in enumerate(order)}
                    for i in range(1, n):   # parent and action lead from a stored state to this one
                        p, a = int(m.parent[s, i]), int(m.action[s, i])
                        assert p < i and bm.oc.rotate(m.states[s, p], *bm.oc.ACTION_SPACE[a]).tobytes() == order[i]
                        assert index[m.states[s, p].tobytes()] == p
    if pinned:
        for s in list(tenant):
            if m.status(s) != bm.RUNNING:
                settle(s)
    return ops


@pytest.mark.parametrize("C", list(bm.SHAPES))
def test_the_seeded_scenarios_end_as_the_oracle_and_reach_their_cases(C):
    m = bm.make_model(C)
    assert (m.S, m.H) == (4, 2 * m.cap) and m.H == bm.min_hash_size(m.cap)
    ops = drive(m, bm.seeded_scenario(m, bm.SEEDS[C]))
    missing = [k for k in bm.SEEDED_WANTED[C] if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    assert {"plant", "step"} == set(ops) and not (m.words[bm.W_STATUS] == bm.RUNNING).any()
    assert m.count["failed_on_words"] == m.count["failed_on_path"] == 0


@pytest.mark.parametrize("Q", [1, 2])
def test_the_queue_row_scenario_fills_a_row_and_overflows_one(Q):
    m = bm.make_model(bm.QUEUE_C, Q)
    before = m.queues.copy()
    drive(m, bm.queue_scenario(m))
    missing = [k for k in bm.QUEUE_WANTED if m.count[k] < 1]
    assert not missing, (missing, dict(m.count))
    for s in range(m.S):
        ok, seen, queue, _ = bm.oracle_game(m.states[s, 0].tobytes(), m.room)
        assert ok and len(queue) == Q + s % 2
        if s % 2:   # one move too many: the slot fails and its row is what it was
            assert m.status(s) == bm.FAILED and m.words[bm.W_QUEUE_LEN, s] == 0 and np.array_equal(m.queues[s], before[s])
            assert m.words[bm.W_NODES, s] == seen   # (the count of the reference's search stands)
        else:
            assert m.game(s) == (True, seen, queue)


def test_the_range_check_scenario_fails_the_victim_and_nobody_else():
    m = bm.make_model(bm.RANGE_C)
    calls = []

    def watched():
        for call in bm.range_scenario(m, 77):
            calls.append(call)
            others = None if "corruption" not in call else m.words[:, :bm.VICTIM].copy()
            nodes = [getattr(m, name)[bm.VICTIM].copy() for name in m.NODE_ARRAYS] + [m.queues[bm.VICTIM].copy()]
            yield call
            if others is not None and call["corruption"] != "none":   # the failing step
                assert m.status(bm.VICTIM) == bm.FAILED and (m.words[bm.W_STATUS, :bm.VICTIM] != bm.FAILED).all()
                after = [getattr(m, name)[bm.VICTIM] for name in m.NODE_ARRAYS] + [m.queues[bm.VICTIM]]
                assert all(np.array_equal(a, b) for a, b in zip(nodes, after))

    drive(m, watched(), pinned=False)
    names = [c["corruption"] for c in calls if "corruption" in c]
    assert names == list(bm.RUNNING_CORRUPTIONS + bm.PATH_CORRUPTIONS)
    assert m.count["failed_on_words"] == len(bm.RUNNING_CORRUPTIONS) and m.count["failed_on_path"] == len(bm.PATH_CORRUPTIONS) - 1
    assert m.count["replanted_over_larger_tenant"] >= len(names) - 1


def test_every_hand_made_value_stays_within_eight_rows_of_its_array():
    """The condition under which the range-check scenario may run on a shared GPU: were a value used unchecked, the access would
    still land inside the arena (its arrays lie 256 guard bytes apart, and a row is at most 16 bytes)."""
    m = bm.make_model(bm.RANGE_C)
    seen = 0
    for call in bm.range_scenario(m, 77):
        if call["op"] == "write":
            seen += 1
            word = call["index"][0] if call["name"] == "words" else None
            if call["name"] == "words" and word in (bm.W_LO, bm.W_LEVEL_END, bm.W_NODES, bm.W_SOLVED_PARENT, bm.W_MAX_STATES):
                assert 0 <= call["value"] <= m.cap + 8, call
            else:
                assert -1 <= call["value"] <= max(m.C + 1, 12), call
        bm.apply(m, call)
        if call["op"] == "write" and call["name"] == "words":
            lo, n_par = m.words[bm.W_LO, bm.VICTIM], m.words[bm.W_N_PAR, bm.VICTIM]
            assert lo + n_par <= m.cap + 8 and n_par <= m.C + 1
    assert seen >= len(bm.RUNNING_CORRUPTIONS) + 4 * len(bm.PATH_CORRUPTIONS)


# ---- the host's check of the words ---------------------------------------------------------------------------------------------
def _block(S=7, capacity=100):
    """One slot of every legal status; the EMPTY slot's other words are anything."""
    w = np.zeros((7, S), dtype=np.int64)
    w[bm.W_STATUS] = [bm.RUNNING, bm.SOLVED, bm.CUT, bm.ROOT_SOLVED, bm.GRAPH_DONE, bm.EMPTY, bm.EMPTY]
    w[bm.W_NODES], w[bm.W_LEVEL_END], w[bm.W_LO] = 40, 30, 20
    w[bm.W_QUEUE_LEN] = [0, 64, 0, 0, 0, 0, 0]
    w[:, 3] = [bm.ROOT_SOLVED, 0, 0, 0, 0, 0, 5]
    w[1:, 5] = [-7, 10 ** 12, 99, 10 ** 9, 3, -1]
    w[1:, 6] = np.frombuffer(bytes([bm.FILL]) * 48, dtype=np.int64)
    w[bm.W_NODES, 2] = capacity   # nodes == capacity is still inside the arrays
    return w


def test_check_words_accepts_every_legal_status_and_refuses_the_rest():
    from librubiks import _hip
    from librubiks.solving.bfs_batch_device import check_words
    check_words(_block(), 100)
    bad = []
    for status in (bm.FAILED, -1, 7, 1 << 40):
        w = _block()
        w[bm.W_STATUS, 2] = status
        bad.append(w)
    for word, value in ((bm.W_LO, 31), (bm.W_LEVEL_END, 41), (bm.W_NODES, 101), (bm.W_QUEUE_LEN, 65), (bm.W_LO, -1)):
        w = _block()
        w[word, 0] = value   # lo > level_end, level_end > nodes, nodes > capacity, queue_len > 64, lo < 0
        bad.append(w)
    for w in bad:
        with pytest.raises(_hip.RubiksHipError, match="slot [02] failed"):
            check_words(w, 100)
    # the same counters on an EMPTY slot are nobody's
    w = _block()
    w[bm.W_LO, 5], w[bm.W_NODES, 5], w[bm.W_QUEUE_LEN, 5] = 10 ** 6, -3, 1000
    check_words(w, 100)
