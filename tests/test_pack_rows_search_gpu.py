"""
MCTSForest.pack_rows: the one-launch step runs the network on the rows that hold a state (packed in list order, outputs scattered
back to the row slots) instead of on all 11 slots of every listed tree.  A row's outputs do not depend on the other rows of a
launch, so every node must receive exactly the bits it receives with the switch off: the same trees, array for array -- in a plain
lock-step batch, with a pool of slots that is refilled (plants into a running forest, a changing list) and with the forest
narrowed along its ladder of launch sizes (set_active moves trees to other list positions).
"""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import cube as oc

pytestmark = pytest.mark.gpu

G, DEPTH, CAP = 96, 12, 2000


@pytest.fixture(scope="module")
def trained():
    from librubiks.model import Model
    np.random.seed(12)
    return Model.load(os.path.join(ROOT, "weights", "fc_small_r1")).eval(), np.array([oc.scramble(DEPTH, True)[0] for _ in range(G)])


def _search(net, states, pack: bool, sync_every: int = 8, **kw):
    from librubiks.model import F32_SPLIT
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    before = md.MCTSForest.pack_rows
    md.MCTSForest.pack_rows = pack
    packed_steps = [0]
    row_map = md.MCTSForest.row_map

    def counting(self):
        packed_steps[0] += 1
        return row_map(self)

    md.MCTSForest.row_map = counting
    try:
        # (a fixed path store: these shallow trees need no address space reserved for descents of any length)
        agent = MCTS(net, c=0.6, search_graph=True, net_dtype=F32_SPLIT, sync_every=sync_every, max_path=4096)
        agent.snapshot_trees = {}
        res = agent.search_batch(states, None, CAP, **kw)
        torch.cuda.synchronize()
    finally:
        md.MCTSForest.pack_rows, md.MCTSForest.row_map = before, row_map
    assert (packed_steps[0] > 0) == pack, "the switch decides whether the row map is built"
    return agent, res


@pytest.mark.parametrize("how", ["lock_step", "pool_of_32", "narrowed"])
def test_trees_are_the_same_with_packed_rows(trained, how):
    net, states = trained
    # (narrowed: the host looks at the trees after every step, so that the forest passes through both smaller launch sizes)
    kw = {"lock_step": dict(compact=False), "pool_of_32": dict(slots=32), "narrowed": dict(compact=True, sync_every=1)}[how]
    a_on, on = _search(net, states, True, **kw)
    a_off, off = _search(net, states, False, **kw)
    if how == "pool_of_32":
        assert a_on.refill_stats["refills"] >= 2
    if how == "narrowed":
        assert a_on.refill_stats["compactions"] >= 2       # 96 -> 64 -> 32 listed trees
    assert np.array_equal(on.solved, off.solved) and np.array_equal(on.iterations, off.iterations) and np.array_equal(on.nodes, off.nodes)
    assert 0 < int(on.solved.sum()) and int(on.iterations.max()) > 20
    assert all(list(p) == list(q) for p, q in zip(on.queues, off.queues))
    assert sorted(a_on.snapshot_trees) == sorted(a_off.snapshot_trees) == list(range(G))
    for g in range(G):
        t_on, t_off = a_on.snapshot_trees[g], a_off.snapshot_trees[g]
        assert t_on.keys() == t_off.keys()
        for name in t_on:
            assert np.array_equal(np.asarray(t_on[name]), np.asarray(t_off[name])), (how, g, name)
