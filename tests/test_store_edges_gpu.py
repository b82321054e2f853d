"""
The node store's edges, pinned to the oracle (oracle/agents.py) and to the reference's recorded traces:

A. Fallbacks.  Without HIP virtual memory the descent paths of a forest live in one fixed block (`MCTSForest._make_path_store`) and
   its node rows are allocated up front: the struct the kernels read must describe those arrays (max_path = the block, ring lines
   no longer than it), and the searches must still be the oracle's -- or end PATH_OVERFLOW exactly where the oracle's descent does
   not fit the block.
B. Copies into a forest of another capacity (the results forests of a search bounded by time alone): rc_mcts_copy_trees marks a tree
   that does not fit the destination's rows RC_MCTS_CORRUPT and writes nothing of it; the trees that fit arrive whole, their hash
   tables rebuilt by the probe rule.
C. Line following reads hints only (csrc/rubiks_mcts.hip, `line_tag`): a path number that wraps at 65 536 iterations, and ring lines
   and tags scrambled into valid-but-wrong ones, leave every tree the oracle's, in every form of the tree kernel.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden_cases
from mcts_lockstep import TREE_KEYS, WRAP, check_hash_table, compare_tree, drive, load_trees, oracle_arrays

pytestmark = pytest.mark.gpu

from oracle import agents as oa  # noqa: E402  (checker only)
from oracle import cube as oc  # noqa: E402

_G = np.load(f"{GOLDEN}/agents_golden.npz")


@pytest.fixture(scope="module")
def net_gpu(standin_net):
    return standin_net.cuda()


@pytest.fixture
def knobs(monkeypatch):
    from librubiks.solving import mcts_device as md

    def set_(lds, block, ring):
        monkeypatch.setattr(md, "LDS_LEVELS", lds)
        monkeypatch.setattr(md, "PATH_BLOCK", block)
        monkeypatch.setattr(md, "RING_LEVELS", ring)
    return set_


@pytest.fixture
def no_vmm(monkeypatch):
    """no_vmm("path") / no_vmm("node") / no_vmm("path", "node"): VmmArray.take fails for the descent paths (taken without a chunk
    size) and / or the per-node arrays (taken with one), as on a runtime without HIP virtual memory management."""
    from librubiks import _hip
    from librubiks.solving import mcts_device as md
    take = md.VmmArray.take

    def set_(*what):
        def fake(cls, nbytes, device, chunk=None):
            if ("node" if chunk is not None else "path") in what:
                raise _hip.RubiksHipError("rc_vmm_reserve: not supported (test)")
            return take(nbytes, device) if chunk is None else take(nbytes, device, chunk)
        monkeypatch.setattr(md.VmmArray, "take", classmethod(fake))
    return set_


# ---- A. fallbacks ---------------------------------------------------------------------------------------------------------------

def test_path_store_fallback_describes_its_arrays(knobs, no_vmm):
    """Host side only (the constructor's zero fills run, no search kernel does): after the fallback the struct's path limit is the
    block the arrays have, nothing says deeper blocks have memory, and the ring lines are as long as the struct says."""
    from librubiks.solving import mcts_device as md
    knobs(8, 8, 32)
    no_vmm("path")
    with pytest.warns(RuntimeWarning, match="paths are limited to 8 levels"):
        f = md.MCTSForest(48, 1500)
    s = f.struct
    assert not f.path_vmm and f.max_path == 8 == s.max_path and f.path_blocks == 1
    assert s.path_rows is None and f.path_rows is None and (f.path_rows_host == 8).all()
    for name in ("path_node", "path_act", "path_next", "short_act"):
        assert tuple(getattr(f, name).shape) == (1, 48, 8), name
    assert f.ring_levels == s.ring_levels == 8
    assert f.ring_node.shape == f.ring_act.shape == (48, md.RING_K, s.ring_levels)
    sub = md.MCTSForest(4, 1500, f.max_path, _results_only=True, vmm=False, path_block=8, ring_levels=f.ring_levels)
    assert sub.struct.max_path == 8 and sub.ring_node.shape[-1] == sub.struct.ring_levels == 8


@pytest.fixture(scope="module")
def overflow_refs(net_gpu):
    np.random.seed(4)
    states = np.array([oc.scramble(20, True)[0] for _ in range(48)])
    onet = oa.TorchNet(net_gpu, device="cuda")
    refs = []
    for s in states:
        ref = oa.MCTS(onet, c=0.2, search_graph=True)
        refs.append((ref.search(s, 1500), len(ref), list(ref.action_queue), ref.iterations, ref.deepest_path))
    return states, refs


@pytest.mark.parametrize("use_graph", [False, True])
def test_path_overflow_on_the_fallback_store(use_graph, net_gpu, knobs, no_vmm, overflow_refs):
    """test_search_edge_gpu.py::test_path_overflow's criterion on a store that fell back to one 8-level block: exactly the trees whose
    oracle descent is deeper than 8 levels end PATH_OVERFLOW with 7 queued actions, every other tree is the oracle's."""
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    knobs(8, 8, 32)
    no_vmm("path")
    states, refs = overflow_refs
    agent = MCTS(net_gpu, c=0.2, search_graph=True, net_dtype=torch.float32, use_graph=use_graph)
    with pytest.warns(RuntimeWarning, match="paths are limited to 8 levels"):
        res = agent.search_batch(states, None, 1500, compact=False)
    f = agent.forest
    assert f.max_path == 8 == f.struct.max_path and not f.path_vmm and f.ring_node.shape[-1] == f.struct.ring_levels == 8
    overflowed = 0
    for t, (ok, n, queue, iterations, deepest) in enumerate(refs):
        too_deep = deepest > 8
        assert (res.status[t] == md.PATH_OVERFLOW) == too_deep, f"tree {t}"
        if too_deep:
            assert not res.solved[t] and len(res.queues[t]) == 7 and res.nodes[t] <= n, f"tree {t}"
            overflowed += 1
        else:
            assert bool(res.solved[t]) == ok and res.nodes[t] == n and list(res.queues[t]) == queue, f"tree {t}"
            assert res.iterations[t] == iterations, f"tree {t}"
    assert overflowed >= 8 and res.path_overflow_trees == overflowed


def test_continuous_batching_on_the_fallback_store(net_gpu, knobs, no_vmm):
    """search_batch(slots=32) copies finished trees into results forests (`subset` / `bury`) and plants new games into their slots: on a
    store that fell back to one 16-level block (ring lines shortened with it) the games are those of a plain batch."""
    from librubiks.solving.agents import MCTS
    knobs(8, 16, 64)
    no_vmm("path")
    np.random.seed(21)
    states = np.array([oc.scramble(1 + g % 7, True)[0] for g in range(150)])
    states[17] = oc.get_solved()
    out = {}
    for slots in (None, 32):
        agent = MCTS(net_gpu, c=0.6, search_graph=True, net_dtype=torch.float32, sync_every=4)
        with pytest.warns(RuntimeWarning, match="paths are limited to 16 levels"):
            out[slots] = agent.search_batch(states, None, 600, slots=slots)
        f = agent.forest
        assert f.max_path == 16 == f.struct.max_path and f.ring_node.shape[-1] == f.struct.ring_levels == 16
    plain, pooled = out[None], out[32]
    assert np.array_equal(pooled.solved, plain.solved) and np.array_equal(pooled.status, plain.status)
    assert np.array_equal(pooled.lengths, plain.lengths) and np.array_equal(pooled.nodes, plain.nodes)
    assert np.array_equal(pooled.iterations, plain.iterations)
    assert [list(q) for q in pooled.queues] == [list(q) for q in plain.queues]
    assert 0 < plain.solved.sum() < 150


@pytest.mark.parametrize("fail", [("node",), ("node", "path")])
def test_reference_traces_on_up_front_node_rows(fail, agents_golden, net_gpu, knobs, no_vmm, monkeypatch):
    """Every forest would be mapped on demand (VMM_MIN_BYTES = 0), but the node rows cannot be reserved: they are allocated up front --
    with a warning -- and every tree the reference recorded is rebuilt node for node; alone, and with the path store fallen back to one
    512-level block as well (the deepest recorded descent has 358 levels)."""
    from librubiks.solving import mcts_device as md
    from librubiks.solving.agents import MCTS
    monkeypatch.setattr(md.MCTSForest, "VMM_MIN_BYTES", 0)
    knobs(4096, 512, 4096)
    no_vmm(*fail)
    for case in golden_cases(_G, "mcts_"):
        g = lambda k: agents_golden[f"mcts_{case}_{k}"]   # noqa: E731
        depth, c, graph, max_states, solved, n = g("params")
        agent = MCTS(net_gpu, c=float(c), search_graph=bool(graph), net_dtype=torch.float32)
        with pytest.warns(RuntimeWarning, match="node rows cannot be reserved on demand"):
            assert agent.search(g("state"), None, int(max_states)) == bool(solved), case
        f = agent._last_forest
        assert not f.vmm and f.mapped_rows is None and f.struct.mapped_rows is None
        assert f.path_vmm == ("path" not in fail)
        if "path" in fail:
            assert f.max_path == 512 == f.struct.max_path and f.ring_levels == f.struct.ring_levels == f.ring_node.shape[-1] == 512
        assert len(agent) == int(n), case
        assert list(agent.action_queue) == list(g("queue")), case
        compare_tree(agent._host_tree(), {k: g(k) for k in TREE_KEYS}, int(n))


# ---- B. copies into forests of another capacity ---------------------------------------------------------------------------------

def _rows(f, name, t, n):
    lo = t * (f.C + 1)
    return getattr(f, name)[lo:lo + n + 1].cpu().numpy()


def test_copy_into_smaller_forests_refuses_trees_that_do_not_fit(net_gpu):
    """rc_mcts_copy_trees called directly: three trees of a 3 000-node forest, grown to different sizes, into forests whose capacity is
    the middle tree's node count (full and results-only), and into one of the source's capacity (the control: hash tables travel as
    they are).  The tree above the capacity ends RC_MCTS_CORRUPT with nothing of it written; the others arrive row for row, and their
    rebuilt hash tables follow the probe rule."""
    import ctypes
    from librubiks import _hip
    from librubiks.cube import DeviceCubes
    from librubiks.model import GenericNet
    from librubiks.solving import mcts_device as md
    np.random.seed(9)
    states = np.array([oc.scramble(20, True)[0] for _ in range(3)])
    src = md.MCTSForest(3, 3000, vmm=False)
    src.set_net(GenericNet(net_gpu), torch.float32)
    src.reset(DeviceCubes.from_numpy(states))
    for trees, steps in ((None, 61), ([1, 2], 40), ([2], 40)):    # the trees stop at different sizes
        src.set_active(None if trees is None else np.array(trees))
        for _ in range(steps):
            src.step(0.6, 3000, use_graph=False)
    src.set_active(None)
    torch.cuda.synchronize()
    n = src.n_nodes.cpu().numpy().astype(np.int64)
    assert (src.status.cpu().numpy() == md.RUNNING).all() and n[0] < n[1] < n[2] < 3000, n
    order = [2, 0, 1]                 # into destination slots 1, 2, 3: above, below and at the destination's capacity
    idx = torch.tensor(order, dtype=torch.int32, device="cuda")
    cap = int(n[1])
    dests = {"full": md.MCTSForest(4, cap, vmm=False), "results": md.MCTSForest(4, cap, _results_only=True, vmm=False),
             "same": md.MCTSForest(4, 3000, vmm=False)}
    for kind, dst in dests.items():
        assert dst.C == (3000 if kind == "same" else cap)
        rc = src.lib.rc_mcts_copy_trees(ctypes.byref(src.struct), ctypes.byref(dst.struct), idx.data_ptr(), 3, 1, _hip.stream_ptr())
        assert rc == 0, (kind, rc)
        torch.cuda.synchronize()
        status = dst.status.cpu().numpy()
        fits = [kind == "same" or n[t] <= cap for t in order]
        assert fits == [kind == "same", True, True]
        assert status[0] == md.RUNNING and list(status[1:]) == [md.RUNNING if ok else md.CORRUPT for ok in fits], (kind, status)
        assert not dst.keys[:dst.C + 1].any() and not dst.hash[0].any()          # slot 0 was not a destination
        for pos, (t, ok) in enumerate(zip(order, fits), start=1):
            if not ok:                                                            # nothing of the oversize tree was written
                lo = pos * (dst.C + 1)
                assert not dst.keys[lo:lo + dst.C + 1].any() and not dst.leaf[lo:lo + dst.C + 1].any() and not dst.hash[pos].any()
                assert not (dst.nbr if kind == "results" else dst.node)[lo:lo + dst.C + 1].any()
                continue
            k = int(n[t])
            names = ("keys", "leaf", "nbr") if kind == "results" else ("keys", "leaf", "V", "node")
            for name in names:
                assert np.array_equal(_rows(dst, name, pos, k), _rows(src, name, t, k)), (kind, t, name)
            if kind == "same":
                assert torch.equal(dst.hash[pos], src.hash[t])
            else:
                check_hash_table(dst.hash[pos].cpu().numpy(), _rows(dst, "keys", pos, k), k)


def test_stale_node_count_in_a_time_only_harvest_raises(net_gpu, monkeypatch):
    """A search bounded by time alone hands its finished trees to results forests of other capacities: the shared one ("grave",
    COPY_CAPACITY_MAX rows per tree) takes the trees whose `nodes_seen` fits it, the others get forests of their own.  COPY_CAPACITY_MAX
    is lowered to 64 here, so that small trees take both paths.  A node count that is stale low sends a larger tree to the grave: the
    copy refuses it (RC_MCTS_CORRUPT, nothing of it written), the search raises naming its game, and the trees buried with it arrive
    whole, their hash tables rebuilt by the probe rule."""
    from librubiks import _hip
    from librubiks.solving import agents as ag
    from librubiks.solving import mcts_device as md
    monkeypatch.setattr(md.MCTSForest, "COPY_CAPACITY_MAX", 64)
    harvest, adopt, seen = ag.MCTSRun._harvest, md.MCTSForest.adopt, {}

    def stale_harvest(self, idx_np):
        f = self.forest
        if "stale" not in seen:
            real = f.n_nodes.cpu().numpy()[idx_np]                      # (synchronises: the trees are finished)
            big = idx_np[(real > 64) & (self.owner[idx_np] != 0)]
            if len(big):
                t = int(big[0])
                seen["stale"] = (t, int(self.owner[t]))
                f.nodes_seen[t] = 13                                     # the host's copy of its node count is stale
        return harvest(self, idx_np)

    def checked_adopt(self, pos, other, trees):
        adopt(self, pos, other, trees)
        if "stale" in seen and "checked" not in seen and seen["stale"][0] in trees:
            assert self.results_only and self.C == 64 and other.C > 64
            torch.cuda.synchronize()
            status, real = self.status.cpu().numpy(), other.n_nodes.cpu().numpy()
            for i, t in enumerate(np.asarray(trees, dtype=np.int64), start=pos):
                k = int(real[t])
                if t == seen["stale"][0]:
                    assert k > 64 and status[i] == md.CORRUPT and not self.hash[i].any()
                    assert not self.keys[i * 65:(i + 1) * 65].any() and not self.nbr[i * 65:(i + 1) * 65].any()
                    continue
                assert status[i] != md.CORRUPT
                for name in ("keys", "leaf", "nbr"):
                    assert np.array_equal(_rows(self, name, i, k), _rows(other, name, int(t), k)), (t, name)
                check_hash_table(self.hash[i].cpu().numpy(), _rows(self, "keys", i, k), k)
            seen["checked"] = len(trees)

    monkeypatch.setattr(ag.MCTSRun, "_harvest", stale_harvest)
    monkeypatch.setattr(md.MCTSForest, "adopt", checked_adopt)
    np.random.seed(31)
    onet = oa.TorchNet(net_gpu, device="cuda")
    states = []
    while len(states) < 16:     # scrambles the stand-in net solves (a search bounded by time alone ends no other way): 1 in 4 large
        big = len(states) % 4 == 3
        cand = oc.scramble(5 if big else 1, True)[0]
        ref = oa.MCTS(onet, c=20.0, search_graph=True)
        if ref.search(cand, 3000) and (not big or len(ref) > 100):
            states.append(cand)
    agent = ag.MCTS(net_gpu, c=20.0, search_graph=True, net_dtype=torch.float32, sync_every=4)
    with pytest.raises(_hip.RubiksHipError, match="rows that are not theirs") as err:
        agent.search_batch(np.array(states), time_limit=60.0, slots=8)
    assert "stale" in seen and "checked" in seen
    assert f"game {seen['stale'][1]}," in str(err.value)
    torch.cuda.synchronize()                  # the process is alive and the GPU answers


# ---- C. line following: tag wrap and valid-but-wrong rings -----------------------------------------------------------------------

S1, S2, C_LINES = 120, 300, 0.6


@pytest.fixture(scope="module")
def line_refs(net_gpu):
    """8 depth-20 scrambles and the oracle's naive trees after S1 + S2 iterations (c = 0.6: deep, repeated descents)."""
    np.random.seed(3)
    states = np.array([oc.scramble(20, True)[0] for _ in range(8)])
    onet = oa.TorchNet(net_gpu, device="cuda")
    refs = []
    for s in states:
        ref = oa.MCTS(onet, c=C_LINES, search_graph=False)
        ref.search(s, 12 * (S1 + S2) + 64, max_iterations=S1 + S2)
        refs.append(ref)
    return states, refs


_CHILD = """
import os, sys
import numpy as np
sys.path[:0] = [{root!r}, os.path.join({root!r}, "rl-rubiks_amd"), os.path.join({root!r}, "tests")]
from conftest import GOLDEN
from mcts_lockstep import drive, save_trees, standin_from_golden
net = standin_from_golden(np.load(os.path.join(GOLDEN, "agents_golden.npz"))).cuda()
states = np.load(sys.argv[1])
save_trees(sys.argv[2], drive(net, states, {c!r}, "one_launch", {s1}, {s2}, sys.argv[3], seed=5))
"""


@pytest.mark.parametrize("what", ["wrap", "rings"])
@pytest.mark.parametrize("form", ["select0", "three_phase", "one_launch", "one_launch_lw1"])
def test_line_following_reads_hints_only(form, what, net_gpu, line_refs, tmp_path):
    """wrap: after S1 iterations every tree's iteration number is set to 65 536 - 48, and S2 more run: the 16-bit path number crosses
    0 (no line written), then the tags written before the jump read as 1 .. 32 iterations old and name ring slots that hold newer
    lines.  rings: after S1 iterations the ring slots are permuted and the tags rewritten (mcts_lockstep._scramble_rings).  Either
    way every tree is the oracle's after S1 + S2 iterations, node for node, and the iteration counts advance by S2 -- in the
    three-phase forms (k_mcts_select<0>, k_mcts_select<1>: one wave checks a line) and the one-launch step (four waves for 8 trees;
    one wave in a child process with RUBIKS_LINE_WAVES=1, which the library reads once per process)."""
    states, refs = line_refs
    if form == "one_launch_lw1":
        np.save(tmp_path / "states.npy", states)
        code = _CHILD.format(root=ROOT, c=C_LINES, s1=S1, s2=S2)
        env = {**{k: v for k, v in os.environ.items() if not k.startswith("RUBIKS_")}, "RUBIKS_LINE_WAVES": "1"}
        p = subprocess.run([sys.executable, "-c", code, str(tmp_path / "states.npy"), str(tmp_path / "out.npz"), what], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        out = load_trees(str(tmp_path / "out.npz"))
    else:
        out = drive(net_gpu, states, C_LINES, form, S1, S2, what, seed=5)
    for t, ref in enumerate(refs):
        n = len(ref)
        compare_tree(out["trees"][t], oracle_arrays(ref), n)
        base = WRAP if what == "wrap" else out["it_at"][t]
        assert out["it_at"][t] + out["it_end"][t] - base == ref.iterations, f"tree {t}"
    assert (out["status"] == 0).sum() >= 6                # (nearly) every tree ran the whole window
    assert out["rounds"] > 0                              # lines were followed after the disturbance
    if what == "wrap":
        assert out["aliasing"] > 100                      # tags the wrapped path number makes look young ...
        assert out["window_rounds"] > 0                   # ... and line rounds while they did
