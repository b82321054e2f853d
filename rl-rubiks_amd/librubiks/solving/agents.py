"""
Search agents of the hot path with the reference's API (librubiks/solving/agents.py):

    MCTS(net, c, search_graph).search(state, time_limit=None, max_states=None) -> bool
    .action_queue (deque of action indices), len(agent) (states explored), str(agent), .tt

plus a batched entry point the reference lacks -- `search_batch(states, ...)` runs one tree per
scramble in lock step on one MI355X; `search` is `search_batch` with a single tree.  The trees are
built by the rc_mcts_* HIP kernels (csrc/rubiks_mcts.hip) with the reference's exact per-tree
semantics; the network runs through an engine of librubiks.model chosen by `net_dtype`: F32_SPLIT (the default: fp32
accuracy, the reference's precision, on the f16 matrix cores), torch.bfloat16 (the fast engine) or torch.float32.
"""
import warnings
import weakref
from collections import deque
from time import perf_counter

import numpy as np
import torch

from librubiks import _hip, gpu, no_grad
from librubiks.cube.device import DeviceCubes, encode
from librubiks.model import F32_SPLIT, F32_SPLIT_DET, Model, net_fingerprint
from librubiks.solving import astar_device as ad
from librubiks.solving import bfs_batch_device as bb
from librubiks.solving import bfs_device as bd
from librubiks.solving import egvm_device as ed
from librubiks.solving import mcts_device as md
from librubiks.solving import rollout_device as rd
from librubiks.solving import shorten as sh
from librubiks.solving.results import BatchResult, QueueTable   # noqa: F401  (also this module's names: callers import them from here)
from librubiks.utils import TickTock

DEFAULT_NODE_CAP = 1 << 18   # least per-tree / per-problem node capacity of a search bounded by time only
ASTAR_TIME_ONLY_BYTES = 32 << 30   # A* bounded by time only: what its per-node arrays (57 bytes per node, allocated up front) may take


def astar_time_only_capacity(n_problems: int) -> int:
    """Node capacity per problem of an A* search bounded by wall time only (the reference's arrays double without bound,
    agents.py:396-404): 2^18 nodes at least, 2^26 at most, and in between what 32 GB of node arrays allow for the batch --
    one problem gets 2^26 nodes (3.8 GB), 4 096 problems keep 2^18 each."""
    return int(max(DEFAULT_NODE_CAP, min(1 << 26, ASTAR_TIME_ONLY_BYTES // (57 * max(1, int(n_problems))))))
TIME_ONLY_HASH_BYTES = 32 << 30   # MCTS bounded by time only: what the trees' hash tables (the one per-node array that must exist up front) may take


def time_only_capacity(n_trees: int) -> int:
    """Node capacity per tree of an MCTS search bounded by wall time only.  The reference's arrays double for as long as the time
    limit lets the tree grow (agents.py:450-459): there is no node limit.  Here a tree's node rows are address space that gets
    memory as the tree grows (`MCTSForest.grow`), so the capacity is what the kernels can address -- 2^24 - 2 nodes per tree -- or,
    in large batches, what 32 GB of hash tables (8 bytes per node, cleared when a tree is planted) allow; what really ends such a
    search is its time limit or the HBM behind the rows running out (the trees then stop growing and the time limit ends it)."""
    if md.MCTSForest.VMM_MIN_BYTES is None:     # node rows allocated up front (RUBIKS_VMM_MIN_GB=never): the old fixed capacity
        return DEFAULT_NODE_CAP
    return int(max(DEFAULT_NODE_CAP, min(md.MAX_CAPACITY, TIME_ONLY_HASH_BYTES // (8 * max(1, int(n_trees))) - 1)))
bd_MAX_STATES = 1 << 26      # BFS bounded by time only: node slots for 2^26 states (~4 GB)
BFS_BATCH_BYTES = 32 << 30   # pooled BFS: what the slots' node rows, hash tables and child rows (allocated up front) may take


class Agent:
    _explored_states = 0

    def __init__(self):
        self.action_queue = deque()
        self.tt = TickTock()

    def reset(self, time_limit, max_states):
        self._explored_states = 0
        self.action_queue = deque()
        self.tt.reset()
        if hasattr(self, "net") and hasattr(self.net, "eval"):
            self.net.eval()
        assert time_limit or max_states   # reference agents.py:54
        return time_limit or 1e10, max_states or int(1e10)

    def __len__(self):
        return self._explored_states

    # `shorten=True` (EGVM, RandomSearch, PolicySearch, ValueSearch): the action queue of every SOLVED game is replaced by the route the
    # reference's graph shortening (agents.py:597-633, which it applies to MCTS(search_graph=True) only) finds through the states the
    # queue itself visits (librubiks/solving/shorten.py).  Solved flag, len(agent), status and the times of the search are what they
    # are without it; an unsolved game's queue -- a best guess, not a solution -- stays.
    shorten = False

    def _shortened(self, res: BatchResult, states) -> BatchResult:
        """The assembled result of a `search_batch`, shortened once if the agent was asked to."""
        return res.shortened(states) if self.shorten else res

    def _shorten_own_queue(self, state: np.ndarray, solved: bool):
        """`search` under `shorten=True`: the agent's action_queue after a solved search of `state`."""
        if self.shorten and solved and len(self.action_queue):
            queues, status = sh.shorten_queues(np.asarray(state)[None], [list(self.action_queue)])
            if status[0] != sh.OK:
                raise RuntimeError(f"shortening the action queue failed (status {int(status[0])})")
            self.action_queue = queues[0]


def _unbounded(limit) -> bool:
    """True for what `Agent.reset` returns in place of a limit that was not given: the search is bounded by the other one alone."""
    return limit >= 1e10


class DeepAgent(Agent):
    """
    Agents that evaluate a network.  `net_dtype` selects the inference engine (librubiks.model.make_inference_net): the default
    F32_SPLIT is the reference's precision (its forward is fp32, agents.py:551-552) on the f16 matrix cores; torch.bfloat16 is the
    fast engine, torch.float32 the plain fp32 GEMM chain; `deterministic=True` asks for the split engine's one-plan form (see `MCTS`).
    """

    def __init__(self, net, net_dtype=F32_SPLIT, deterministic: bool = False):
        super().__init__()
        if deterministic:
            if net_dtype not in (F32_SPLIT, F32_SPLIT_DET):
                raise ValueError("deterministic=True runs on the split engine (net_dtype=F32_SPLIT): the library GEMMs of the other engines "
                                 "choose their kernels by batch shape")
            net_dtype = F32_SPLIT_DET
        self.net, self.net_dtype = net, net_dtype
        self.deterministic = net_dtype == F32_SPLIT_DET
        self._fp32_for = None   # (fingerprint of `net`, fp32 engine) once a search on the split engine left half range

    def _search_net(self):
        """What this search's engine is built from: `net`, or -- after a search on the f16x3 split engine saw an activation
        beyond IEEE half's range -- the fp32 GEMM chain of exactly those weights."""
        if self._fp32_for is not None and self._fp32_for[0] == net_fingerprint(self.net, self.net_dtype):
            return self._fp32_for[1]
        return self.net

    def _overflowed(self, engine) -> bool:
        """True if `engine` (the split engine) wrote an activation it cannot represent during the search just finished: the
        caller repeats the search, which `_search_net` then runs in fp32.  Synchronises (call where results are collected)."""
        if not (hasattr(engine, "overflowed") and engine.overflowed()):
            return False
        fallback = engine.fallback()    # (deterministic mode: raises -- the fp32 chain is not bit-reproducible across batch shapes)
        warnings.warn("SplitF32Net: a hidden activation left IEEE half's range (|x| > 65504) during this search; it is repeated "
                      "on the fp32 GEMM chain, and so are later searches with these weights", RuntimeWarning)
        self._fp32_for = (net_fingerprint(self.net, self.net_dtype), fallback)
        return True

    @classmethod
    def from_saved(cls, loc: str, use_best: bool, **kwargs):
        return cls(Model.load(loc, load_best=use_best).to(gpu), **kwargs)


class BFS(Agent):
    """
    Breadth-first search (reference agents.py:92-131) with whole levels expanded on the GPU; solution,
    `len(agent)` and the stop rule are those of the reference's FIFO loop (csrc/rubiks_bfs.hip).
    `time_limit` is tested between launch sequences instead of before every pop.  `search_batch(..., slots=S)` searches a
    pool of games together, one game per slot (csrc/rubiks_bfs_batch.hip); `chunk` is a speed knob in both forms.
    """

    def __init__(self, chunk: int = None, steps_per_round: int = 4):
        super().__init__()
        self.chunk = chunk
        self.steps_per_round = int(steps_per_round)   # pooled form: steps between two looks at the slots' words (4: profiles/bfs_batch_probe.txt)
        self._dev = None
        self._pool = None

    def _device_for(self, max_states: int) -> bd.BFSDevice:
        cap = int(min(max_states, bd_MAX_STATES))
        if self._dev is None or self._dev.max_states < cap:
            self._dev = None   # frees the old buffers first
            self._dev = bd.BFSDevice(cap, self.chunk)
        return self._dev

    def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
        time_limit, max_states = self.reset(time_limit, max_states)
        self.tt.tick()
        dev = self._device_for(max_states)
        deadline = None if _unbounded(time_limit) else (lambda: self.tt.tock() >= time_limit)
        solved, actions, seen = dev.search(np.asarray(state), int(min(max_states, dev.max_states)), deadline)
        self._explored_states = seen
        self.action_queue = deque(actions)
        return solved

    def search_batch(self, states, time_limit: float = None, max_states: int = None, slots: int = None) -> BatchResult:
        """
        With slots=None: one search after the other (each one fills the GPU by itself); same result layout as the deep agents.
        slots: search at most this many games at a time, all advancing together on the device, chunk by chunk
        (librubiks/solving/bfs_batch_device.py); finished games hand their slots to the scrambles still waiting (continuous
        batching, as `AStar.search_batch`).  Every game ends exactly -- solved flag, len(agent), action queue, status -- as its
        own `search` does, whoever shares the batch, however many slots there are and whatever the chunk.  A round is
        `steps_per_round` steps and one look at the slots' words; the clock is looked at between rounds only, and `time_limit`
        bounds the whole pool.  Games that never got a slot before the time limit end unsolved, with 0 nodes, status EXHAUSTED
        and 0 seconds.  The number of slots is bounded by BFS_BATCH_BYTES of per-slot arrays (`bfs_batch_plan`).
        `BatchResult.iterations` is the number of levels per game, `game_seconds` the pool's per-game intervals.
        """
        if slots is not None:
            time_limit, max_states = self.reset(time_limit, max_states)
            return self._search_pool(DeviceCubes.of(states), time_limit, max_states, slots)
        states = states.numpy() if isinstance(states, DeviceCubes) else np.asarray(states)
        B = len(states)
        solved, lengths, nodes = np.zeros(B, dtype=bool), np.full(B, -1, dtype=np.int64), np.zeros(B, dtype=np.int64)
        queues, levels, each = [], np.zeros(B, dtype=np.int64), np.zeros(B)
        tt = TickTock()
        tt.tick()
        for g in range(B):
            t0 = tt.tock()
            solved[g] = self.search(states[g], time_limit, max_states)
            each[g] = tt.tock() - t0
            queues.append(self.action_queue)
            nodes[g], levels[g] = len(self), self._dev.levels
            if solved[g]:
                lengths[g] = len(self.action_queue)
        status = np.where(solved, np.where(nodes == 0, 4, 1), 2)
        return BatchResult(solved, lengths, nodes, QueueTable.from_queues(queues), tt.tock(), levels, status, each)

    def _pool_for(self, n_slots: int, max_states: int, chunk: int) -> bb.BFSBatch:
        b = self._pool
        if b is None or (b.S, b.C) != (n_slots, chunk) or b.max_states < max_states or b.max_states > 4 * max_states:
            self._pool = None   # frees the old buffers first
            torch.cuda.empty_cache()
            b = self._pool = bb.BFSBatch(n_slots, max_states, chunk)
        return b

    def _search_pool(self, roots: DeviceCubes, time_limit: float, max_states: int, slots) -> BatchResult:
        """`search_batch(slots=...)` behind `reset`: both limits are set (one may be `reset`'s stand-in for a limit not given)."""
        S, C, _, _, _ = bb.bfs_batch_plan(roots.n, max_states, slots, self.chunk)
        cap = int(min(max_states, bd_MAX_STATES))
        pool = SlotPool(roots.n, S, self.tt.tock)
        S, owner = pool.S, pool.owner
        batch = self._pool_for(S, cap, C)
        caps = np.full(S, cap, dtype=np.int64)

        def plant(into, first):
            batch.plant(into, roots, first, caps[:len(into)])
        self.tt.tick()
        plant(np.arange(S), 0)                            # the first S scrambles; the others move in as games finish
        host, ev = batch.snapshot()
        ev.synchronize()
        final = host.numpy().copy()
        while self.tt.tock() < time_limit:                # (the reference tests the clock before every pop, agents.py:105)
            live = owner >= 0
            ended = live & (final[bb.W_STATUS] != bb.RUNNING)
            done = np.flatnonzero(ended)
            pool.sighted(done, self.tt.tock())
            if not (live & ~ended).any() and not pool.waiting:
                break
            if pool.waiting and len(done):
                # the finished slots' results leave without waiting, then the waiting scrambles are planted there
                pool.take(done, final, batch)
                pool.refill(done, plant)
            batch.step(self.steps_per_round)
            host, ev = batch.snapshot()
            ev.synchronize()
            final = host.numpy().copy()
            bb.check_words(final, batch.capacity)
        seconds = self.tt.tock()
        left = np.flatnonzero(owner >= 0)
        pool.sighted(left[final[bb.W_STATUS, left] != bb.RUNNING], seconds)
        return pool.collect(self, batch, final, seconds, 2)

    @staticmethod
    def _part(words: np.ndarray, host: torch.Tensor, ev) -> BatchResult:
        """Slots' words and queue rows as the serial form reports them: a cut, an exhausted graph and a game the time limit
        stopped are all status 2 there."""
        ev.synchronize()
        status, nodes, levels, qlen = words[bb.W_STATUS], words[bb.W_NODES], words[bb.W_LEVELS], words[bb.W_QUEUE_LEN]
        solved = (status == bb.SOLVED) | (status == bb.ROOT_SOLVED)
        qlen = np.where(solved, qlen, 0)
        return BatchResult(solved, np.where(solved, qlen, -1), nodes.copy(), QueueTable(host.numpy().copy(), qlen), 0.0, levels.copy(),
                           np.where(solved, status, 2))

    def __str__(self):
        return "Breadth-first search"


class _Harvest:
    """
    The trees of `forest` on their way to becoming per-game results: graph completion and BFS shortening of the
    solved trees (device kernels), then asynchronous copies of the per-tree words and paths into pinned host
    memory, all on the current stream; `result()` assembles the BatchResult once the copies have landed.
    """
    _pinned = {}

    @classmethod
    def _host_like(cls, t: torch.Tensor) -> torch.Tensor:
        """Pinned host tensor shaped like t, from a pool keyed by the row count rounded up to a power of two (harvests
        come in all sizes; a fresh hipHostMalloc per harvest would cost more than the harvest)."""
        rows = 1 << max(4, int(np.ceil(np.log2(max(1, t.shape[0])))))
        key = (rows, tuple(t.shape[1:]), t.dtype)
        free = cls._pinned.setdefault(key, [])
        buf = free.pop() if free else torch.empty((rows,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=True)
        return buf

    def __init__(self, agent, forest: md.MCTSForest, games: np.ndarray, n: int = None, trees: torch.Tensor = None,
                 trees_host: np.ndarray = None):
        """n: only the first n trees of the forest are real (a partly filled results forest).
        trees: int32 device list -- only these (finished) trees of a forest that may still be running are turned into
        results, where they lie; games[i] is the game of trees[i].  trees_host: the same list on the host (a forest whose rows
        are mapped on demand gives the BFS scratch of exactly these trees its memory)."""
        self.games, self.graph = games, agent.search_graph
        # (the first block of the blocked path arrays: a queue longer than that -- rare -- is fetched by `result`)
        src = {"status": forest.status, "nodes": forest.n_nodes, "iterations": forest.iterations,
               "plen": forest.path_len, "sol": forest.solved_action, "pact": forest.path_act[0]}
        if self.graph:
            forest.complete_graphs(trees)       # _complete_graph of all solved trees in one launch
            forest.shorten_launch(trees, trees_host)   # ... and their BFS shortening in another
            src["slen"], src["sact"] = forest.short_len, forest.short_act[0]
        self.host, self.n = {}, (forest.B if n is None else n) if trees is None else int(trees.numel())
        self.tree_ids = np.arange(self.n) if trees is None else np.asarray(trees_host, dtype=np.int64)
        pick = None if trees is None else trees.long()
        # the list is read by kernels queued on THIS (side) stream; it was allocated under another one, whose allocator would hand
        # the block out again the moment the caller drops it: it lives as long as this harvest, and the allocator is told as well
        self.trees = trees
        if trees is not None:
            trees.record_stream(torch.cuda.current_stream())
        for name, t in src.items():
            part = t[:self.n] if pick is None else t[pick]
            self.host[name] = self._host_like(part)
            self.host[name][:self.n].copy_(part, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        self.forest = forest   # keeps the buffers alive until the copies have landed

    def ready(self) -> bool:
        return self.event.query()

    def result(self) -> BatchResult:
        self.event.synchronize()
        h = {k: v.numpy()[:self.n] for k, v in self.host.items()}
        status, plen = h["status"].astype(np.int64), h["plen"].astype(np.int64)
        bad = np.flatnonzero(status == md.CORRUPT)
        if len(bad):   # graph completion / BFS shortening met indices that name no node of the tree: not the tree's rows (never seen since the
            # node store flushes translations; a loud error with the addresses instead of the GPU fault a wild index would be)
            t = int(self.tree_ids[bad[0]])
            raise _hip.RubiksHipError(f"MCTS result extraction: {len(bad)} tree(s) hold rows that are not theirs (first: tree {t}, game "
                                      f"{int(self.games[bad[0]])}, {int(h['nodes'][bad[0]])} nodes): {self.forest.describe_rows(t)}")
        acts = h["pact"].copy()
        width = acts.shape[1]                             # one path block
        lens = plen - 1                                   # the actions taken: the best guess of an unsolved tree (agents.py:492)
        won = np.flatnonzero(status == md.SOLVED)
        fits = won[plen[won] <= width]
        acts[fits, plen[fits] - 1] = h["sol"][fits]       # agents.py:483
        lens[won] = plen[won]
        shortened = np.zeros(len(status), dtype=bool)
        if self.graph and len(won):
            short = won[h["slen"][won] >= 0]
            acts[short] = h["sact"][short]
            lens[short] = h["slen"][short]
            shortened[short] = True
        lens[status == md.ROOT_SOLVED] = 0
        solved = (status == md.SOLVED) | (status == md.ROOT_SOLVED)
        queues = QueueTable(acts, lens)
        for i in np.flatnonzero(lens > width):            # a queue that goes beyond the first path block: read where it lies
            t = int(self.tree_ids[i])
            if shortened[i]:
                q = self.forest.read_path("short_act", t, lens[i])
            else:
                q = self.forest.read_path("path_act", t, plen[i] - 1)
                if status[i] == md.SOLVED:
                    q = np.append(q, np.uint8(h["sol"][i]))
            queues.set_row(int(i), q)
        out = BatchResult(solved, np.where(solved, lens, -1), h["nodes"].astype(np.int64), queues, 0.0,
                          h["iterations"].astype(np.int64), status)
        for name, t in self.host.items():
            self._pinned[(t.shape[0], tuple(t.shape[1:]), t.dtype)].append(t)
        self.host, self.forest, self.trees = None, None, None
        return out


class MCTS(DeepAgent):
    """Batched PUCT graph search with virtual loss and max-backup (reference agents.py:415-645)."""

    nu = 100
    sweep_parameters = ("c",)   # what `search_batch` takes per game: a grid over these can be searched as one pool
    snapshot_trees = None      # test hook: a dict -> {game: tree_arrays()} of every tree as its search left it (before graph completion)

    def __init__(self, net, c: float, search_graph: bool, net_dtype=F32_SPLIT, use_graph: bool = True,
                 max_path: int = None, sync_every: int = 16, level_budget="auto", deterministic: bool = False):
        """
        deterministic: bit-reproducible searches.  The default engines pick a layer plan by row count (whole-K tiles, K cut into
        2..32 chunks), so a state's network outputs carry rounding that depends on how many states share its launch, and a near-tie
        in a PUCT argmax can fall the other way: per-game results agree across batch shapes on > 98 % of games, not on all.  With
        deterministic=True the split engine runs ONE plan for every row count (`SplitF32Net(deterministic=True)`): a game searched
        alone, in a batch, on fewer `slots` or in a narrowed forest builds the same tree, bit for bit (tests/test_full_size_gpu.py).
        It costs throughput at both ends of the row-count range: see DESIGN.md section 3.3 for the measured figures.
        max_path: None (default) = PUCT descents of any length, as in the reference (agents.py:575-595): the select kernel works
        on a path's first 4 096 levels in LDS and on deeper ones where they lie in HBM, and the path arrays get memory block by
        block for the trees that go that deep (`MCTSForest.ensure_path`).  A number bounds the path store instead (a resource
        bound the reference does not have: a tree whose descent fills it ends unsolved with status PATH_OVERFLOW, counted in
        `BatchResult.path_overflow_trees`).  With the ADI-trained net, 39 of 1 024 depth-20 trees needed more than 1 024
        levels and none more than 2 048 (longest solution found: 804 moves).
        level_budget: how many NEW tree levels a PUCT descent may walk per lock-step iteration before it is
        suspended until the next one (0 = unlimited).  Every tree still performs exactly the reference's
        sequence of iterations; a budget only stops the deepest descent of the batch from pacing all trees.
        Measured on 1 024 depth-20 trees with trained weights: over a fixed number of lock-step iterations a
        budget of 32 gains 4 % (23.9 vs 22.9 M nodes/s), but a run to completion gets 2.5x SLOWER (6.1 s vs
        2.4 s: the last stragglers are suspended over and over), so "auto" means 0 (strict lock step).
        """
        super().__init__(net, net_dtype, deterministic)
        self.level_budget = level_budget
        self.c, self.search_graph = float(c), bool(search_graph)
        self.use_graph, self.max_path, self.sync_every = use_graph, max_path, sync_every
        self.forest = None
        self._last_forest = None   # the forest the last search ended in (a compacted one after `compact`)
        self._tree = None      # host copy of game 0's tree, for the reference's inspectable attributes
        self._tree_src = None  # (forest, tree index) holding game 0's tree after the last search

    @classmethod
    def from_saved(cls, loc: str, use_best: bool, c: float, search_graph: bool, **kwargs):
        return cls(Model.load(loc, load_best=use_best).to(gpu), c=c, search_graph=search_graph, **kwargs)

    def __str__(self):
        return ("BFS" if self.search_graph else "Naive") + f" MCTS (c={self.c})"

    # ---- batched search --------------------------------------------------------------------------
    def _forest_for(self, n_trees: int, capacity: int) -> md.MCTSForest:
        f = self.forest
        if f is None or f.B != n_trees or f.C < capacity or f.C_asked > 4 * capacity:
            self.forest = None
            if f is not None:
                # what still points into the forest that is about to hand its memory on: game 0's tree is read out now (the
                # reference's inspectable attributes keep working), the pointers are dropped
                if self._tree_src is not None and self._tree_src[0] is f:
                    if self._tree is None:
                        try:
                            self._host_tree()
                        except Exception:   # noqa: BLE001 -- a forest whose search never finished has no tree to show
                            pass
                    self._tree_src = None
                if self._last_forest is f:
                    self._last_forest = None
                run = getattr(f, "_run", None)
                run = run() if run is not None else None
                if run is None or run.done:
                    f.close()         # node store mapped on demand: parked for the next forest of that shape (not left to __del__)
                # (a run started with `start_batch` and not finished still steps this forest: it keeps it -- and its memory -- until it
                # is finished or dropped; the forest is then collected like any object, `MCTSForest.__del__`)
                del f
            torch.cuda.empty_cache()
            f = self.forest = md.MCTSForest(n_trees, capacity, self.max_path)
        f.set_net(self._search_net(), self.net_dtype)   # every search: `net` may have been trained or replaced since the last one
        f.level_budget = 0 if self.level_budget == "auto" else int(self.level_budget)
        return f

    @no_grad
    def prepare(self, n_trees: int, max_states: int, per_game_c: bool = False):
        """One-off set-up of a batched search with `n_trees` concurrent trees of capacity `max_states`, so that the search
        itself starts at full speed: allocates the forest (HBM, zero-filled), builds the inference engine and captures the HIP
        graph of every launch size the forest will be narrowed to (~0.1 s per size for the split engine: the allocations of
        its activations).  Optional: a search on an unprepared agent does the same work on the way.
        per_game_c: the graphs of a search that brings c per game (`search_batch(c=...)`), which serve every value of c."""
        cap_states = int(max_states) if max_states and not _unbounded(max_states) else time_only_capacity(n_trees)
        forest = self._forest_for(int(n_trees), max(cap_states, 16))
        if self.use_graph:
            forest.capture_all(md.C_PER_TREE if per_game_c else self.c, cap_states)

    def sweep_refusal(self):
        """Why `Evaluator.eval_sweep` must not pool this agent's settings, or None.  A sweep promises the rows of one `eval` per
        setting.  The default split engine picks a layer plan by row count (see `deterministic`), and a PUCT near-tie then falls
        differently in a pool than in a point's own batch: the engine has a form without that, so the sweep asks for it instead of
        returning rows that the loop would not.  (The other engines have no such form: they are taken as they are.)"""
        if self.net_dtype == F32_SPLIT:
            return (f"{self} runs the split engine with a layer plan per row count, so a pooled game need not end as the same game "
                    "searched point by point; build the agent with deterministic=True")
        return None

    def _per_game_c(self, n_games: int, c):
        """None where the search runs under the agent's own c (c not given, or a scalar equal to it), else a float64 (G,) host
        array with game g's c, checked: numbers, finite, one per game."""
        if c is None:
            return None
        arr = np.asarray(c)
        if arr.dtype == object or arr.dtype.kind not in "iuf":
            raise ValueError(f"c: real numbers expected, got dtype {arr.dtype}")
        if arr.ndim == 0:
            if np.isfinite(arr) and float(arr) == self.c:
                return None
            arr = np.full(n_games, arr[()])
        if arr.shape != (n_games,):
            raise ValueError(f"c: shape {arr.shape} given, ({n_games},) expected: one value per game")
        arr = arr.astype(np.float64)
        bad = np.flatnonzero(~np.isfinite(arr))
        if len(bad):   # a NaN score wins no argmax, and an infinite c times a prior of 0 is NaN
            raise ValueError(f"c: game {int(bad[0])} has {arr[bad[0]]}; every value must be finite")
        return arr

    @no_grad
    def search_batch(self, states, time_limit: float = None, max_states: int = None,
                     max_iterations: int = None, compact: bool = True, slots: int = None, c=None) -> BatchResult:
        """
        One MCTS tree per row of `states` ((G,20) int8 NumPy array or DeviceCubes).  `max_states` is the
        reference's per-tree cap (stop when len + 12 > max_states); `time_limit` bounds the wall time of the
        whole batch; `max_iterations` bounds every tree's number of expansions (lock-step batches only).
        See `MCTSRun` for how the batch is driven.
        slots: run at most this many trees at a time and give the places of finished trees to the scrambles
        still waiting (continuous batching): the GPU stays full until the last games instead of idling on the
        stragglers of every batch.  Per-game results are those of a plain batch (trees are independent).
            compact: once nobody is waiting, finished trees are dropped from the launches as the running ones become fewer
        (`MCTSForest.set_active`: a shorter list of trees, nothing moves in memory), so the stragglers continue on small
        network batches; the finished trees are turned into results where they lie, on a side stream.
        c: None (the agent's own c), a scalar, or an array of shape (G,) with game g's own exploration constant: game g then
        ends exactly -- status, nodes, iterations, queue, the tree itself -- as game g of `MCTS(net, c[g], ...).search_batch` on
        the same scramble, wherever the network's outputs do not depend on the batch (deterministic=True).  So a grid over c is
        searched as one pool (the reference searches it point by point, hyper_optim.py:102-110): every slot keeps its game's c
        from the plant of its root on (`MCTSForest.c_slot`), and one captured graph per launch size serves every value.  Every
        value must be a finite real number (ValueError otherwise, before anything touches the device).  None, or a scalar equal
        to the agent's c, is the search as it always was: the scalar kernel entry points, graphs keyed by the value.
        """
        # a bounded number of iterations must end on a completed one: the three-phase form (the one-launch form of an iteration
        # expands the NEXT leaf at its end)
        run = self.start_batch(states, time_limit, max_states, compact=compact, slots=slots, one_launch=max_iterations is None, c=c)
        assert max_iterations is None or run.S == run.n_games, "max_iterations applies to lock-step batches only"
        # a tree's first expansion (its root's) takes two lock-step iterations, every later one a single iteration
        steps = None if max_iterations is None else max_iterations + 1
        while not run.done and (steps is None or run.it < steps):
            run.round(None if steps is None else steps - run.it)
        if max_iterations is not None:
            run.catch_up(max_iterations)
        return run.finish()

    @no_grad
    def start_batch(self, states, time_limit: float = None, max_states: int = None, compact: bool = True,
                    slots: int = None, one_launch: bool = True, c=None) -> "MCTSRun":
        """c: as for `search_batch`."""
        per_game_c = self._per_game_c(states.n if isinstance(states, DeviceCubes) else len(states), c)   # (raises before anything touches the device)
        time_limit, max_states = self.reset(time_limit, max_states)
        return MCTSRun(self, DeviceCubes.of(states), time_limit, max_states, compact, slots, one_launch, per_game_c)

    # ---- the reference's single-state API ----------------------------------------------------------
    def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
        res = self.search_batch(np.asarray(state)[None], time_limit, max_states)
        return bool(res.solved[0])

    def _host_tree(self):
        """Game 0's tree, read from the forest it was harvested in (after a solved graph search the device arrays
        hold the completed graph)."""
        if self._tree is None:
            forest, t = self._tree_src
            self._tree = forest.tree_arrays(t)
        return self._tree

    # inspectable attributes relied on by the reference's tests (tests/test_agents.py:54-92)
    states = property(lambda self: self._host_tree()["states"])
    neighbors = property(lambda self: self._host_tree()["neighbors"])
    leaves = property(lambda self: self._host_tree()["leaves"])
    P = property(lambda self: self._host_tree()["P"])
    V = property(lambda self: self._host_tree()["V"])
    W = property(lambda self: self._host_tree()["W"])
    N = property(lambda self: self._host_tree()["N"])
    L = property(lambda self: self._host_tree()["L"])

    @property
    def indices(self) -> dict:
        tree = self._host_tree()
        return {s.tobytes(): i for i, s in enumerate(tree["states"][1:tree["n"] + 1], start=1)}


def _to_device_async(arr: np.ndarray, device) -> torch.Tensor:
    """Host array -> device tensor without blocking the host: a copy from pageable memory makes the caller wait until the
    GPU has reached that point of the stream, i.e. until everything queued ahead of it has run."""
    return torch.from_numpy(np.ascontiguousarray(arr)).pin_memory().to(device, non_blocking=True)


class SlotPool:
    """
    Continuous batching on the host: `n_games` games go, in order, through the S slots of a device batch.  `owner[s]` is the game in
    slot s (-1: its result is taken and nobody moved in), `next_game` the first game still waiting.  A game's wall interval
    (`BatchResult.game_seconds`) runs on `clock` (the agent's `tt.tock`) from the plant of its root to the host's first sighting of it
    finished, or to the end of the search.
    """

    def __init__(self, n_games: int, slots, clock):
        self.n_games, self.clock = n_games, clock
        self.S = n_games if slots is None else max(1, min(int(slots), n_games))
        self.owner = np.arange(self.S)              # the first S games start in the slots; the others move in as games finish
        self.next_game = self.S
        self._t_start = np.zeros(n_games)           # per game: when its root was planted ...
        self._t_end = np.full(n_games, np.nan)      # ... and when the host first saw it finished (NaN: not yet)
        self.taken = []                             # `take`: (games, their words, their queue rows on the way to the host)

    @property
    def waiting(self) -> bool:
        return self.next_game < self.n_games

    def sighted(self, done: np.ndarray, now: float):
        """The host has just seen the games in slots `done` finished: the first sighting of a game counts."""
        g = self.owner[done]
        self._t_end[g[np.isnan(self._t_end[g])]] = now

    def refill(self, done: np.ndarray, plant) -> np.ndarray:
        """Slots `done` (results taken) go to the games still waiting, if any: `plant(slots, first)` queues the roots of games first,
        first + 1, ... into `slots`; their intervals begin when it returns.  -> the slots that got a game (the others stay empty)."""
        first, k = self.next_game, min(len(done), self.n_games - self.next_game)
        plant(done[:k], first)
        self.owner[done] = -1
        self.owner[done[:k]] = np.arange(first, first + k)
        self._t_start[first:first + k] = self.clock()
        self.next_game += k
        return done[:k]

    def close(self, result: BatchResult, seconds: float, exhausted_status: int):
        """The search ended after `seconds`: games that never got a slot end there, unsolved and with nothing explored, and so do the
        intervals of the games still running; -> `result.game_seconds`."""
        if self.waiting:
            result.status[self.next_game:] = exhausted_status
            self._t_start[self.next_game:] = seconds
        result.game_seconds = np.where(np.isnan(self._t_end), seconds, self._t_end) - self._t_start

    # ---- batches whose slots show a block of words and a queue row (BFSBatch, EGVMBatch, RolloutBatch) ----
    def take(self, done: np.ndarray, words: np.ndarray, batch):
        """The results of the finished slots `done` leave without waiting (before a `refill` plants there): their columns of
        `words` (the host's copy of the batch's snapshot) and their queue rows, on the way into pinned memory."""
        w = words[:, done].copy()
        self.taken.append((self.owner[done].copy(), w, batch.take_queues(done, w[batch.queue_len_row].max())))

    def collect(self, agent, batch, words: np.ndarray, seconds: float, exhausted_status: int) -> BatchResult:
        """The search ended after `seconds`: -> the games' results -- what `take` set aside and the slots still occupied, as
        `words` shows them, through `agent._part(words, queue rows, event)` -- merged and closed; game 0's is the agent's own."""
        left = np.flatnonzero(self.owner >= 0)
        parts = [(games, agent._part(w, q[0], q[1])) for games, w, q in self.taken]
        if len(left):
            w = words[:, left]
            parts.append((self.owner[left], agent._part(w, *batch.take_queues(left, w[batch.queue_len_row].max())[:2])))
        result = BatchResult.merge(self.n_games, parts, seconds)
        self.close(result, seconds, exhausted_status)
        agent._explored_states = int(result.nodes[0])
        agent.action_queue = result.queues[0]
        return result


def lockstep_search(agent, batch, pool: SlotPool, roots: DeviceCubes, time_limit: float, cap: int, played_cap: int, by_states: bool,
                    streams, rounds_fit: bool = True):
    """
    The host's round loop of the lock-step agents (EGVM; RandomSearch, PolicySearch, ValueSearch): the games of `roots` go through
    the `pool.S` slots of `batch` (an EGVMBatch or a RolloutBatch), one `batch.round(table, cap)` after the other.  Round r + 1's
    table is drawn from the games' `streams` (None: the agent draws nothing) while round r runs, for the games that have played
    fewer than `played_cap` moves or rounds (`batch.unit` per round).  A search that is not `by_states` (bounded by time only)
    widens the queue rows between rounds.  rounds_fit=False (EGVM: max_states below one round): the roots are planted, so that
    solved scrambles are seen, and no round runs.  What else differs between the families is the batch's to say (`LockstepBatch`).
    -> the BatchResult, or None where the split engine left half range: the caller repeats the search, which then runs in fp32.
    """
    S, owner = pool.S, pool.owner
    tables = batch.host_tables()                      # two: one is drawn into while the other's round runs
    views = [None if t is None else t.numpy() for t in tables]
    played = np.zeros(S, dtype=np.int64)              # moves / rounds queued for the slot's game so far
    stats = agent.batch_stats = {"rounds": 0, "draw_s": 0.0, "draw_exposed_s": 0.0, "wait_s": 0.0, "device_round_ms": []}

    def draw(into, which):
        """The next round's draws of the games in slots `which`."""
        if streams is None:
            return 0.0
        t0 = perf_counter()
        batch.draw_round(streams, owner[which], which, into)
        dt = perf_counter() - t0
        stats["draw_s"] += dt
        return dt

    def adopt(which):
        if streams is not None:
            streams.start(owner[which])               # every game's own np.random stream starts when the game is planted
        played[which] = 0

    def plant(into, first):
        batch.plant(_to_device_async(into.astype(np.int32), batch.device), roots, first)
    agent.tt.tick()
    batch.reset(roots)                                # the first S scrambles; the others move in as games finish
    host, ev = batch.snapshot()
    adopt(np.arange(S))
    ev.synchronize()
    final = host.numpy().copy()
    status = final[0]                                 # (root-solved games are known before the first round.)  A VIEW: see the refill below
    r = 0
    if rounds_fit and ((status == ed.RUNNING).any() or pool.waiting):
        stats["draw_exposed_s"] += draw(views[0], np.flatnonzero(status == ed.RUNNING))
        while True:
            if not by_states:
                batch.grow_queues(batch.width_after(int(played.max()), cap))
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            batch.round(tables[r % 2], cap)
            t1.record()
            host, ev = batch.snapshot()
            live = owner >= 0
            played[live & (status == ed.RUNNING)] += batch.unit
            # round r + 1 is drawn while round r runs, for every game that can still be running then: a game always makes a whole
            # round's draws, so its move t uses draw t of its stream whatever ends the game sooner (the draws of a game that is
            # over are ones the reference would not have made)
            draw(views[(r + 1) % 2], np.flatnonzero(live & (status == ed.RUNNING) & (played < played_cap)))
            t_wait = perf_counter()
            ev.synchronize()
            stats["wait_s"] += perf_counter() - t_wait
            stats["device_round_ms"].append(t0.elapsed_time(t1))
            stats["rounds"] = r = r + 1
            final = host.numpy().copy()
            status = final[0]
            batch.check_status(status, owner, played, agent)
            now = agent.tt.tock()
            ended = live & (status != ed.RUNNING)
            done = np.flatnonzero(ended)
            pool.sighted(done, now)
            if now >= time_limit or not (live & ~ended).any() and not pool.waiting:
                break
            if pool.waiting and len(done):
                # the finished slots' results leave without waiting, then the waiting scrambles are planted there
                pool.take(done, final, batch)
                fresh = pool.refill(done, plant)
                adopt(fresh)
                # (`status` is row 0 of `final`: these two writes also edit the block `collect` reads for the slots still occupied)
                status[done] = ed.EXHAUSTED           # (an empty slot is not played)
                status[fresh] = ed.RUNNING            # (a solved scramble shows ROOT_SOLVED in the next block; its draws are not used)
                stats["draw_exposed_s"] += draw(views[r % 2], fresh)   # (r has been incremented: the table of the round about to run)
    torch.cuda.synchronize()
    if batch.engine is not None and agent._overflowed(batch.engine):   # the split engine could not represent an activation
        return None
    result = pool.collect(agent, batch, final, agent.tt.tock(), ed.EXHAUSTED)
    if batch.time_limit_exhausts or not rounds_fit:   # (rounds_fit: agents.py:665 is false before the first round)
        result.status[result.status == ed.RUNNING] = ed.EXHAUSTED   # the time limit ended these
    return result


class MCTSRun(SlotPool):
    """
    A batched MCTS search in progress: `round()` queues the next lock-step iterations, `finish()` returns the
    per-game BatchResult.  All trees of the forest advance together, `sync_every` iterations per round; the host
    never waits for the round it has just queued: it reads the tree states of the PREVIOUS round (an asynchronous
    copy into pinned memory) while the GPU works on the current one, so the launch queue never runs dry.
    Finished trees are turned into results on a side stream.  With `slots` < games their places go to the scrambles
    still waiting, so what result extraction reads of them is first copied into a results forest (`bury`), then `plant`
    clears the slots' hash tables and writes the new roots, which the next two iterations evaluate and expand in step
    with everybody else.  Once nobody is waiting the finished trees stay where they are: they are post-processed in place
    (`_Harvest(trees=...)`) and dropped from the iteration launches by a shorter list of trees (`MCTSForest.set_active`),
    so narrowing a forest costs nothing, whatever the per-tree capacity (copying the survivors of 1 024 trees of capacity
    175 000, the reference's default max_states, took 0.55 s per halving).
    """

    def __init__(self, agent: "MCTS", roots: DeviceCubes, time_limit: float, max_states: int, compact: bool, slots, one_launch: bool = True,
                 c_games: np.ndarray = None):
        """c_games: None -- every tree under `agent.c` --, or game g's own c (float64 [G], checked: `MCTS._per_game_c`): every plant
        hands its slots their games' values and the iterations go through the per-tree entry points (`md.C_PER_TREE`)."""
        super().__init__(roots.n, slots, agent.tt.tock)
        self.agent, self.roots, self.time_limit, self.compact = agent, roots, time_limit, compact
        self.max_states, self.slots, self.one_launch = max_states, slots, one_launch
        self.c_games = c_games
        self.c = agent.c if c_games is None else md.C_PER_TREE     # what `steps` / `step` / `close_pending` get
        S = self.S
        self.cap_states = time_only_capacity(S) if _unbounded(max_states) else int(max_states)
        forest = self.forest = agent._forest_for(S, max(self.cap_states, 16))
        forest._run = weakref.ref(self)     # who steps this forest: an agent does not hand its memory on under a run that is not done
        agent.tt.tick()
        forest.set_active(None)
        self.plant_states = self.cap_states if one_launch else None   # one-launch iterations: roots expanded by the plant itself
        self.c_dev = None if c_games is None else _to_device_async(c_games, forest.device)
        forest.plant(None, roots, 0, self.plant_states, c=self.c_dev)   # the first S scrambles; the others move in as trees finish
        # iterations that may be queued before the host has looked at the node counts: what a planted tree's first rows cover
        # (16 384 rows: its first ~1 360 iterations), so that a long `sync_every` cannot make trees sit out behind the kernel's guard
        forest._steps_covered = min(2 * agent.sync_every, max(1, (forest._first_rows() - 14) // 12))
        self.stale_until = np.full(S, -1)  # snapshots up to this index predate the tree that now lives in the slot
        self.min_refill = max(8, S // 32)
        self.stats = agent.refill_stats = {"iterations": 0, "harvests": 0, "refills": 0, "compactions": 0,
                                           "host_enqueue_s": 0.0, "host_wait_s": 0.0, "host_process_s": 0.0}
        self.side = torch.cuda.Stream()
        self.harvests = []                 # _Harvest objects in flight
        self.grave, self.grave_fill, self.grave_event, self.grave_games = None, 0, None, None
        self.resting = []                  # finished trees left in the forest, waiting for their (batched) result extraction
        self.parts = []                    # (game ids, BatchResult)
        agent._tree, agent._tree_src = None, None
        self.snapshots = deque()           # (index, forest, event, pinned status) of rounds nobody has looked at yet
        self.it, self.q, self.done = 0, 0, False

    def _drain(self, block: bool):
        for h in list(self.harvests):
            if block or h.ready():
                self.parts.append((h.games, h.result()))
                self.harvests.remove(h)

    def _extract(self, forest: md.MCTSForest, games: np.ndarray, **which) -> _Harvest:
        """Result extraction of trees of `forest` (`which`: see `_Harvest`) on the side stream, behind all that this stream has queued."""
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            h = _Harvest(self.agent, forest, games, **which)
        self.harvests.append(h)
        return h

    GRAVE = 256   # finished trees collected before their graph completion / BFS shortening is launched

    def _flush_grave(self):
        """Result extraction for the trees collected so far: ONE launch sequence over up to GRAVE trees on the side stream.
        Post-processing the ~30 trees of every refill by themselves keeps ~30 CUs busy for milliseconds each time, and the
        library GEMMs of the running forest (one workgroup per CU) then take two rounds instead of one."""
        if self.grave is None or self.grave_fill == 0:
            return
        g, n = self.grave, self.grave_fill
        self.stats["flushes"] = self.stats.get("flushes", 0) + 1
        g.status[n:] = md.RUNNING          # slots beyond the fill are not trees
        h = self._extract(g, self.grave_games[:n].copy(), n=n, trees_host=np.arange(n))
        self.grave_event, self.grave_fill = h.event, 0

    def _flush_resting(self):
        """Result extraction of the finished trees left in the forest, where they lie: one launch sequence on the side stream."""
        if not self.resting:
            return
        idx_np = np.concatenate(self.resting)
        self.resting = []
        forest = self.forest
        trees = _to_device_async(idx_np.astype(np.int32), forest.status.device)
        games = self.games_of_resting[idx_np].copy()
        self.stats["flushes"] = self.stats.get("flushes", 0) + 1
        self._extract(forest, games, trees=trees, trees_host=idx_np)

    def _snapshot(self, idx_np: np.ndarray):
        if self.agent.snapshot_trees is not None:
            for t in idx_np:
                self.agent.snapshot_trees[int(self.owner[t])] = self.forest.tree_arrays(int(t))

    def _rest(self, idx_np: np.ndarray):
        """The finished trees `idx_np` are done with iterations and nobody needs their slots: they stay in the forest and are
        turned into results GRAVE trees at a time (few, large launch sequences next to the running iterations: see _flush_grave)."""
        self._snapshot(idx_np)
        if not hasattr(self, "games_of_resting"):
            self.games_of_resting = np.full(self.forest.B, -1, dtype=np.int64)
        self.games_of_resting[idx_np] = self.owner[idx_np]
        if self.agent._tree_src is None and (self.owner[idx_np] == 0).any():   # game 0's tree stays inspectable, where it is
            self.agent._tree_src = (self.forest, int(idx_np[self.owner[idx_np] == 0][0]))
        self.resting.append(idx_np.copy())
        self.stats["harvests"] += 1

    def _harvest(self, idx_np: np.ndarray):
        """Copies the finished trees `idx_np` out of the forest (their slots are needed or dropped): what result extraction
        reads of them goes into the results forest, which is processed GRAVE trees at a time on the side stream."""
        forest, agent = self.forest, self.agent
        self.stats["harvests"] += 1
        self._snapshot(idx_np)
        games = self.owner[idx_np].copy()
        if agent._tree_src is None and (games == 0).any():
            # game 0's tree stays inspectable (the reference's attributes): a search forest of its own, with this one tree
            first = idx_np[games == 0][:1]
            one = forest.subset(first, results_only=False)
            self._extract(one, np.zeros(1, dtype=np.int64))
            agent._tree_src = (one, 0)
            idx_np, games = idx_np[games != 0], games[games != 0]
            if len(idx_np) == 0:
                return
        # a last path beyond the first block, or (searches bounded by time alone) more nodes than the grave's rows: a results forest of its own
        deep = (forest.paths_seen[idx_np] > forest.path_block) | (forest.nodes_seen[idx_np] + 13 > min(forest.C, forest.COPY_CAPACITY_MAX))
        if deep.any():
            self._extract(forest.subset(idx_np[deep], results_only=True), games[deep])
            idx_np, games = idx_np[~deep], games[~deep]
            if len(idx_np) == 0:
                return
        if len(idx_np) < self.GRAVE // 2:
            if self.grave is None:
                self.grave = md.MCTSForest(self.GRAVE, min(forest.C, forest.COPY_CAPACITY_MAX), forest.path_block, forest.device, _results_only=True, vmm=False,
                                           path_block=forest.path_block, lds_levels=forest.lds_levels, ring_levels=forest.ring_levels)
                self.grave_games = np.zeros(self.GRAVE, dtype=np.int64)
            if self.grave_fill + len(idx_np) > self.GRAVE:
                self._flush_grave()
            if self.grave_event is not None:     # the previous batch must have been read before its slots are overwritten
                torch.cuda.current_stream().wait_event(self.grave_event)
                self.grave_event = None
            self.grave.bury(self.grave_fill, forest, idx_np)
            self.grave_games[self.grave_fill:self.grave_fill + len(idx_np)] = games
            self.grave_fill += len(idx_np)
            return
        self._extract(forest.subset(idx_np, results_only=True), games)

    def round(self, max_steps: int = None):
        """Queues up to `sync_every` iterations, then acts on the tree states of the round before."""
        agent, forest = self.agent, self.forest
        n_steps = min(agent.sync_every, max(1, self.it))   # short first rounds: a batch that is solved at once ends at once
        if max_steps is not None:
            n_steps = min(n_steps, max_steps)
        t0 = perf_counter()
        forest.steps(n_steps, self.c, self.cap_states, agent.use_graph)
        self.it += n_steps
        self.stats["iterations"] = self.it
        self.snapshots.append((self.q, forest, *forest.status_snapshot(), self.it))
        self.q += 1
        t1 = perf_counter()
        self.stats["host_enqueue_s"] += t1 - t0
        if len(self.snapshots) < 2 and self.it > 1:
            return            # look at round r - 1 while round r runs
        qi, f_snap, ev, st_host, it_then = self.snapshots.popleft()
        ev.synchronize()
        t2 = perf_counter()
        self.stats["host_wait_s"] += t2 - t1   # time the host had to spare: it waited for the GPU, not the other way round
        if f_snap is forest and int(st_host[3, 0]) != 0:
            # The split engine left half range: from then on its outputs are inf / NaN, and a PUCT descent over NaN scores need
            # never meet a leaf (nor does the reference's on such numbers).  The search stops here; `finish` repeats it in fp32.
            self.done = True
            return
        try:
            if f_snap is forest:
                # the host's look at the node counts: rows for everything the iterations queued since that snapshot, the next
                # round and one more can reach (forests mapped on demand; otherwise only the counts are noted)
                queued = self.it - it_then
                forest.paths_seen = st_host[2].numpy().astype(np.int64)   # (what `_harvest` sizes its copies by, whatever happens below)
                try:
                    forest.grow(st_host[1].numpy(), queued + 2 * agent.sync_every)
                    forest.grow_paths(st_host[2].numpy())      # ... and the next path block for the trees whose descents near the end of theirs
                except _hip.RubiksHipError as e:
                    # HBM has run out behind the node rows / path blocks.  The trees that need more sit out behind the kernels'
                    # guards (exact: nothing is half-written); a search with a time limit ends there, others are stopped here.
                    if not getattr(self, "_hbm_warned", False):
                        warnings.warn(f"MCTS: no more HBM behind the trees' node rows ({e}); the trees that need more stop growing", RuntimeWarning)
                        self._hbm_warned = True
                    if _unbounded(self.time_limit):
                        self.done = True
                        return
                forest._steps_covered = 2 * agent.sync_every
                self.stats["mapped_gb"] = round(forest.bytes_allocated() / 1e9, 2)
            self._act_on(qi, f_snap, st_host[0])
        finally:
            self.stats["host_process_s"] += perf_counter() - t2

    def _act_on(self, qi: int, f_snap, st_host):
        """Harvest / refill / compaction decisions from the tree states of round qi."""
        agent, forest = self.agent, self.forest
        if f_snap is not forest:
            return            # taken before a compaction
        status = st_host.numpy()
        owner = self.owner
        live = owner >= 0
        fresh = self.stale_until < qi
        running = live & ((status == md.RUNNING) | ~fresh)      # a slot refilled after the snapshot runs by definition
        done = np.flatnonzero(live & fresh & (status != md.RUNNING))
        self.sighted(done, agent.tt.tock())
        n_run = int(running.sum())
        out_of_time = agent.tt.tock() >= self.time_limit
        waiting = self.waiting
        self._drain(False)
        if out_of_time or (n_run == 0 and not waiting):
            self.done = True
            return
        if waiting and len(done) and (len(done) >= self.min_refill or n_run == 0):
            self._harvest(done)
            def plant(slots, first):   # the waiting scrambles move in: roots evaluated by the next two iterations
                idx = _to_device_async(slots.astype(np.int32), forest.status.device)
                forest.plant(idx, self.roots, first, self.plant_states, slots_host=slots, c=self.c_dev)
            self.stale_until[self.refill(done, plant)] = self.q - 1     # every snapshot queued so far predates the adoption
            self.stats["refills"] += 1
        elif not waiting and self.compact and forest.rung_for(n_run) < forest.G:
            # fewer running trees than the next smaller launch size: the finished ones rest where they are, the iterations
            # go on with a shorter list of trees (nothing is copied)
            if len(done):
                self._rest(done)
                owner[done] = -1
            forest.set_active(np.flatnonzero(owner >= 0))
            self.stats["compactions"] += 1
            if sum(len(r) for r in self.resting) >= self.GRAVE:
                self._flush_resting()

    def catch_up(self, iterations: int):
        """A search bounded by a number of iterations (lock-step batches, three-phase form) must leave every running tree after
        exactly that many expansions and the descent that follows the last one (agents.py:476-490).  A tree sits an iteration out
        when its next node rows or path block have no memory yet (the kernels' guards); such trees -- rare: the host maps ahead --
        are stepped on their own here until they are where the others are."""
        forest = self.forest
        listed, stepped = forest._listed, False
        for _ in range(4 * iterations + 64):
            torch.cuda.synchronize()
            it, st, pend = (x.cpu().numpy() for x in (forest.iterations, forest.status, forest.pending))
            lag = np.flatnonzero((self.owner >= 0) & (st == md.RUNNING) & ((it < iterations) | (pend != 0)))
            if len(lag) == 0:
                break
            forest.grow(forest.n_nodes.cpu().numpy(), 2)
            forest.grow_paths(forest.path_len.cpu().numpy())
            forest._steps_covered = 2
            forest.set_active(lag)
            forest.step(self.c, self.cap_states, self.agent.use_graph)
            self.it += 1
            stepped = True
        if stepped:
            forest.set_active(None if listed is None else listed[listed >= 0])

    def nodes_now(self) -> int:
        """Nodes in the trees currently in the forest plus those of the trees already harvested (synchronises)."""
        self._drain(True)
        live = self.owner >= 0
        if self.resting:
            live = live.copy()
            live[np.concatenate(self.resting)] = True
        live = torch.from_numpy(live).to(self.forest.n_nodes.device)
        buried = int(self.grave.n_nodes[:self.grave_fill].sum().item()) if self.grave_fill else 0
        return int(self.forest.n_nodes[live].sum().item()) + buried + sum(int(r.nodes.sum()) for _, r in self.parts)

    def finish(self) -> BatchResult:
        agent, forest, owner = self.agent, self.forest, self.owner
        if self.one_launch and bool(forest.expanded.any().item()):
            # the search stopped on time or on a step count (or its last step solved a tree): the expansions that step left
            # pending are backed up and followed by their descent, as the reference's loop would have done (agents.py:476-490)
            forest.close_pending(self.c)
        torch.cuda.synchronize()
        seconds = agent.tt.tock()
        forest.grow(forest.n_nodes.cpu().numpy(), 0)     # the final node counts (what result extraction reads of a tree)
        forest.grow_paths(forest.path_len.cpu().numpy())  # ... and path lengths
        left = np.flatnonzero(owner >= 0)
        if len(left) == forest.B:
            self._snapshot(left)
            self.harvests.append(_Harvest(agent, forest, owner.copy()))
            if agent._tree_src is None and (owner == 0).any():
                agent._tree_src = (forest, int(np.flatnonzero(owner == 0)[0]))
        elif len(left):
            self._rest(left)
        self._flush_resting()
        self._flush_grave()
        self._drain(True)
        result = BatchResult.merge(self.n_games, self.parts, seconds)
        self.close(result, seconds, md.EXHAUSTED)
        self.done = True
        if agent._overflowed(forest.engine):   # the split engine could not represent an activation: the same search in fp32
            again = MCTSRun(agent, self.roots, self.time_limit, self.max_states, self.compact, self.slots, self.one_launch, self.c_games)
            while not again.done:
                again.round()
            return again.finish()
        agent._last_forest = forest
        agent._explored_states = int(result.nodes[0])
        agent.action_queue = result.queues[0]
        return result


class AStar(DeepAgent):
    """
    Batch weighted A* (DeepCubeA style; reference agents.py:171-413): every iteration expands the
    `expansions` open nodes of lowest cost  lambda * G(node) - value_net(node).
    `search_batch` runs one such search per scramble, all on one GPU; `search` is the batch of one.
    """

    sweep_parameters = ("lambda_", "expansions")   # what `search_batch` takes per game: a grid over these can be searched as one pool
    MAX_EXPANSIONS = (2 ** 31 - 2) // 12           # 12 N + 1 node rows must be a 32-bit count
    plant_order = "descending"                     # per-game expansions: "descending" plants the widest games first, "given" the caller's order

    def __init__(self, net, lambda_: float, expansions: int, net_dtype=F32_SPLIT, deterministic: bool = False):
        """deterministic: as for `MCTS` -- one layer plan of the split engine for every row count, so a problem's search does not depend
        on which other problems share its batch."""
        super().__init__(net, net_dtype, deterministic)
        self.lambda_, self.expansions = float(lambda_), int(expansions)
        self._lambda0 = None   # game 0's lambda in the last search, where the games brought their own (`cost`)
        self.batch = None
        self._arrays = None

    @classmethod
    def from_saved(cls, loc: str, use_best: bool, lambda_: float, expansions: int, **kwargs):
        return cls(Model.load(loc, load_best=use_best).to(gpu), lambda_=lambda_, expansions=expansions, **kwargs)

    def __str__(self):
        return f"AStar (lambda={self.lambda_}, N={self.expansions})"

    def _batch_for(self, n_problems: int, capacity: int, expansions: int = None):
        """expansions: the staging's row stride -- the agent's N, or the largest N of a search with per-game values."""
        b, n_exp = self.batch, self.expansions if expansions is None else int(expansions)
        if b is None or b.B != n_problems or b.N != n_exp or b.C < capacity or b.C > 4 * capacity:
            self.batch = None
            torch.cuda.empty_cache()
            b = self.batch = ad.AStarBatch(n_problems, capacity, n_exp)
        b.set_net(self._search_net(), self.net_dtype)   # every search: `net` may have been trained or replaced since the last one
        return b

    @no_grad
    def search_batch(self, states, time_limit: float = None, max_states: int = None,
                     max_iterations: int = None, slots: int = None, lambda_=None, expansions=None) -> BatchResult:
        """
        One A* problem per row of `states` ((G,20) int8 NumPy array or DeviceCubes).  `max_states` is the reference's per-problem
        cap (stop when len + 12 N > max_states); `time_limit` bounds the wall time of the whole search; `max_iterations` bounds
        every problem's number of iterations (plain batches only).
        slots: search at most this many problems at a time and give the slots of finished problems to the scrambles still
        waiting (continuous batching, as `MCTS.search_batch`): after an iteration's status read, the finished slots' queues are
        walked on the device (rc_astar_solutions) and copied out without waiting, then the waiting scrambles are planted there
        (rc_astar_plant).  Problems are independent, so a game's search is that of a plain batch wherever the network's values do
        not depend on the batch (deterministic=True).  Games that never got a slot before the time limit end unsolved, with 0
        nodes, status EXHAUSTED and 0 seconds.
        lambda_, expansions: None (the agent's own value), a scalar, or an array of shape (G,) with game g's own value: game g
        then ends exactly -- status, nodes, iterations, length, queue -- as game g of `AStar(net, lambda_[g],
        expansions[g]).search_batch` on the same scramble, under the condition stated for `slots`.  So a grid of settings is
        searched as one pool (the reference searches it point by point, hyper_optim.py:102-110).  lambda_ must be finite,
        expansions an integer >= 1; `max_states` stays one number: a game with 1 + 12 expansions[g] > max_states ends EXHAUSTED
        at its first pop, as in the reference (agents.py:236).  The batch's staging is sized for the largest expansions[g].
        The pool plants such games -- after game 0 -- by descending expansions[g] (`plant_order`), so that the slots running at one time cost alike
        an iteration; the result is in the caller's order.
        """
        n_games = states.n if isinstance(states, DeviceCubes) else len(states)
        per_game = self._per_game(n_games, lambda_, expansions)   # (raises before anything touches the device)
        time_limit, max_states = self.reset(time_limit, max_states)
        roots = DeviceCubes.of(states)
        self._lambda0 = None if per_game is None else float(per_game[0][0])
        if per_game is None:
            return self._search(roots, time_limit, max_states, max_iterations, slots)
        order = np.arange(n_games)
        if self.plant_order == "descending":   # game 0 stays first: it always gets a slot, and the inspectable attributes describe it
            rest = order[1:]
            order = np.concatenate([order[:1], rest[np.argsort(-per_game[1][rest], kind="stable")]])
        if np.array_equal(order, np.arange(n_games)):
            return self._search(roots, time_limit, max_states, max_iterations, slots, per_game)
        pick = torch.as_tensor(order, device=roots.soa.device)
        shuffled = DeviceCubes.empty(n_games, roots.soa.device)
        shuffled.soa[:, :n_games] = roots.soa[:, pick]
        got = self._search(shuffled, time_limit, max_states, max_iterations, slots, (per_game[0][order], per_game[1][order]))
        result = BatchResult.merge(n_games, [(order, got)], got.seconds)
        result.game_seconds = np.empty(n_games)
        result.game_seconds[order] = got.game_seconds
        self._explored_states = int(result.nodes[0])
        self.action_queue = result.queues[0]
        return result

    def _per_game(self, n_games: int, lambda_, expansions):
        """None if neither argument was given, else (float64 [G] lambdas, int32 [G] expansions) on the host, checked."""
        if lambda_ is None and expansions is None:
            return None
        out = []
        for name, given, own, dtype in (("lambda_", lambda_, self.lambda_, np.float64), ("expansions", expansions, self.expansions, None)):
            arr = np.asarray(own if given is None else given)
            if arr.dtype == object or arr.dtype.kind not in "iuf":
                raise ValueError(f"{name}: numbers expected, got dtype {arr.dtype}")
            if arr.ndim == 0:
                arr = np.full(n_games, arr[()])
            if arr.shape != (n_games,):
                raise ValueError(f"{name}: shape {arr.shape} given, ({n_games},) expected: one value per game")
            out.append(arr if dtype is None else arr.astype(dtype))
        lam, n_exp = out
        bad = np.flatnonzero(~np.isfinite(lam))
        if len(bad):   # NaN has no place in the open list's order, and an infinite lambda times G 0 is NaN
            raise ValueError(f"lambda_: game {int(bad[0])} has {lam[bad[0]]}; every value must be finite")
        as_float = n_exp.astype(np.float64)
        bad = np.flatnonzero(~np.isfinite(as_float) | (as_float != np.floor(as_float)) | (as_float < 1) | (as_float > self.MAX_EXPANSIONS))
        if len(bad):
            raise ValueError(f"expansions: game {int(bad[0])} has {n_exp[bad[0]]}; every value must be an integer in 1 .. {self.MAX_EXPANSIONS}")
        return lam, n_exp.astype(np.int32)

    def _search(self, roots: DeviceCubes, time_limit: float, max_states: int, max_iterations, slots, per_game=None) -> BatchResult:
        """`search_batch` behind `reset`: both limits are set (one may be `reset`'s stand-in for a limit that was not given).
        per_game: (lambdas, expansions) of `_per_game` in the order of `roots`."""
        pool = SlotPool(roots.n, slots, self.tt.tock)
        S, owner = pool.S, pool.owner
        if max_iterations is not None and pool.waiting:
            raise ValueError("max_iterations applies to plain batches only (slots >= number of games)")
        cap_states = astar_time_only_capacity(S) if _unbounded(max_states) else int(max_states)
        n_max = self.expansions if per_game is None else int(per_game[1].max())
        batch = self._batch_for(S, max(cap_states, 12 * n_max + 1), n_max)
        each = () if per_game is None else tuple(torch.as_tensor(x, device=batch.device) for x in per_game)
        self._arrays = None
        self.tt.tick()
        batch.reset(roots, *each)                   # the first S scrambles; the others move in as problems finish
        planted_at = np.zeros(S, dtype=np.int64)    # loop iteration at which the slot's problem was planted
        it, taken = 0, []                           # taken: (games, pinned copies, event) of extracted slots

        def plant(into, first):
            assert ((into >= 0) & (into < S)).all()   # (on the host: a per-slot write through a bad index would abort on the device)
            batch.plant(_to_device_async(into.astype(np.int32), batch.device), roots, first, *each)
        while max_iterations is None or it < max_iterations:
            batch.iteration(self.lambda_, cap_states)
            it += 1
            status = batch.status.cpu().numpy()     # (the loop synchronises here anyway)
            now = self.tt.tock()
            live = owner >= 0
            ended = live & (status != ad.RUNNING)
            done = np.flatnonzero(ended)
            pool.sighted(done, now)
            if now >= time_limit or not (live & ~ended).any() and not pool.waiting:
                break
            if pool.waiting and len(done):
                # a queue is no longer than its problem's G at the goal, and G <= the iterations since the plant (G[parent] + 1,
                # relaxations only lower it, children are appended one iteration after their parent): this width always fits
                width = int(max(1, (it - planted_at[done]).max()))
                taken.append(self._take(batch, done, owner[done].copy(), width))
                if 0 in owner[done]:
                    self._arrays = batch.problem_arrays(int(np.flatnonzero(owner == 0)[0]))   # game 0 stays inspectable
                planted_at[pool.refill(done, plant)] = it
        torch.cuda.synchronize()
        if self._overflowed(batch.engine):   # the split engine could not represent an activation: the same search in fp32
            return self._search(roots, time_limit, max_states, max_iterations, slots, per_game)
        seconds = self.tt.tock()
        left = np.flatnonzero(owner >= 0)
        parts = [self._result(*t) for t in taken]
        if len(left):
            status, nodes, iters = (x[torch.as_tensor(left, device=batch.device)].cpu().numpy().astype(np.int64)
                                    for x in (batch.status, batch.n_nodes, batch.iterations))
            lens, queues = batch.solutions(left)
            parts.append((owner[left], self._part(status, nodes, iters, lens, queues)))
        result = BatchResult.merge(pool.n_games, parts, seconds)
        pool.close(result, seconds, ad.EXHAUSTED)
        self._explored_states = int(result.nodes[0])
        self.action_queue = result.queues[0]
        return result

    @staticmethod
    def _take(batch, slots: np.ndarray, games: np.ndarray, width: int):
        """Result extraction of the finished `slots` before they are replanted: queues walked on the device, then status, nodes,
        iterations, lengths and queues copied into pinned memory on the current stream (nothing waits; `_result` reads them)."""
        idx = _to_device_async(slots.astype(np.int32), batch.device)
        table, lengths = batch.solutions_launch(idx, width)
        pick = idx.long()
        words = torch.stack([batch.status[pick], batch.n_nodes[pick], batch.iterations[pick], lengths])
        host = (torch.empty(words.shape, dtype=words.dtype, pin_memory=True), torch.empty(table.shape, dtype=table.dtype, pin_memory=True))
        host[0].copy_(words, non_blocking=True)
        host[1].copy_(table, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return games, host, ev, (idx, table, words)   # (the device tensors live until the copies have landed)

    @staticmethod
    def _part(status, nodes, iters, lens, queues) -> BatchResult:
        solved = (status == ad.SOLVED) | (status == ad.ROOT_SOLVED)
        return BatchResult(solved, np.where(solved, lens, -1), nodes, queues, 0.0, iters, status)

    def _result(self, games, host, ev, _keep):
        ev.synchronize()
        status, nodes, iters, lens = host[0].numpy().astype(np.int64)
        ad.check_lengths(lens, games, "game")
        acts = host[1].numpy().copy()
        if (lens > acts.shape[1]).any():   # (cannot happen: see the width in search_batch)
            raise _hip.RubiksHipError(f"A* solution extraction: game {int(games[np.argmax(lens > acts.shape[1])])}'s queue is longer "
                                      f"than its iterations allow")
        return games, self._part(status, nodes, iters, lens, QueueTable(acts, np.maximum(lens, 0)))

    def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
        return bool(self.search_batch(np.asarray(state)[None], time_limit, max_states).solved[0])

    # ---- inspectable attributes relied on by the reference's tests (tests/test_agents.py:110-145) ----
    def _host(self):
        if self._arrays is None:   # (a pooled search snapshots game 0 before its slot is replanted)
            self._arrays = self.batch.problem_arrays(0)
        return self._arrays

    states = property(lambda self: self._host()["states"])
    G = property(lambda self: self._host()["G"])
    parents = property(lambda self: self._host()["parents"])
    parent_actions = property(lambda self: self._host()["parent_actions"])
    open_queue = property(lambda self: self._host()["open_queue"])

    @property
    def indices(self) -> dict:
        h = self._host()
        return {s.tobytes(): i for i, s in enumerate(h["states"][1:h["n"] + 1], start=1)}

    @no_grad
    def cost(self, states: np.ndarray, indeces: np.ndarray) -> np.ndarray:
        """lambda * G[indeces] - value_net(states) (agents.py:369-383), evaluated on the device net."""
        from librubiks.model import make_inference_net
        eng = self.batch.engine if self.batch is not None else make_inference_net(self._search_net(), self.net_dtype)
        h = -eng.value(encode(eng, DeviceCubes.from_numpy(np.asarray(states)))).cpu().numpy().astype(np.float64)
        return (self.lambda_ if self._lambda0 is None else self._lambda0) * np.asarray(self.G)[indeces] + h


# =================================================================================================
# Rollout agents (reference agents.py:82-90, 132-169, 649-726), batched over games on the device
# =================================================================================================
DEFAULT_STEP_CAP = 1000   # steps per game when a rollout search is bounded by time only


def _evaluate(engine, cubes: DeviceCubes):
    """(policy logits float32[n,12], values float32[n]) of device-resident states."""
    if getattr(engine, "supports_cubes", False):
        return engine.forward_cubes(cubes)
    return engine(encode(engine, cubes))


def _values(engine, cubes: DeviceCubes):
    if getattr(engine, "supports_cubes", False):
        return engine.value_cubes(cubes)
    return engine.value(encode(engine, cubes))


class _StepAgent(Agent):
    """
    Agents that take one move per step.  The reference bounds them by wall time only (its
    `len(self) < max_states` test reads a counter that is updated after the loop, agents.py:30-38);
    here `max_states` additionally caps the number of moves per game, which keeps runs deterministic.
    All games of a batch step together; a finished game idles on the identity action.

    `search` and a plain `search_batch` are driven move by move from the host and draw from the global np.random stream;
    `search_batch(..., seeds=, slots=)` plays the games in lock step on the device, each on its own stream
    (csrc/rubiks_rollout.hip, librubiks/solving/rollout_device.py).
    """
    kind = None                # which game of rollout_device.KINDS the lock-step search plays
    use_graph = True           # the lock-step search replays a round as one captured graph
    steps_per_round = 8        # moves per round of the lock-step search: the host looks at the games once per round
    QUEUE_STEPS = 64           # queue rows of a lock-step search bounded by time only start at this many moves and double between rounds
    batch = None
    batch_stats = None

    def _actions(self, cubes: DeviceCubes, running: torch.Tensor):
        """-> (uint8 actions [n_padded], bool solved_after [n]) for the current states."""
        raise NotImplementedError

    def search_batch(self, states, time_limit: float = None, max_states: int = None, seeds=None, slots: int = None) -> BatchResult:
        """
        With neither `seeds` nor `slots`: the games step together, driven move by move from the host; random agents draw from the
        global np.random stream, one draw per game and step in game order.  Otherwise the games run in lock step on the device
        (librubiks/solving/rollout_device.py), `steps_per_round` moves between two looks of the host: game g draws from its own
        stream np.random.RandomState(seeds[g]) and ends exactly -- solved flag, len(agent), action queue -- as the reference's
        `search(states[g])` would right after np.random.seed(seeds[g]) if it stopped after `max_states` moves, whoever shares the
        batch, however many slots there are and whatever `steps_per_round` is, wherever the network's rows do not depend on the
        batch (the deterministic engine).  One difference remains for the greedy policy: the move is the first maximum of the 12
        logits, where the reference takes the first maximum of their fp32 softmax (agents.py:139-140); the two differ only where
        the softmax rounds two distinct logits to one probability.  The clock is looked at between rounds only, and
        `time_limit` bounds the whole search.
        seeds: integer array [G], or one integer s for RandomState(s).randint(0, 2**31 - 1, size=G); None (with `slots`): one
        such call on the global stream at entry.  Agents that draw nothing accept it and ignore its values.
        slots: play at most this many games at a time; finished games hand their slots to the scrambles still waiting
        (continuous batching, as `AStar.search_batch`).  Games that never got a slot before the time limit end unsolved, with 0
        nodes, status EXHAUSTED and 0 seconds.  `nodes`, `iterations` and the queue length of a game are its number of moves.
        """
        if seeds is None and slots is None:
            return self._shortened(self._search_stepwise(states, time_limit, max_states), states)
        roots = DeviceCubes.of(states)
        if self.kind in rd.RolloutBatch.TABLE_DTYPE:
            seeds = ed.game_seeds(seeds, roots.n)
        time_limit, max_states = Agent.reset(self, time_limit, max_states)
        return self._shortened(self._search_lockstep(roots, time_limit, max_states, seeds, slots), roots)

    @no_grad
    def _search_stepwise(self, states, time_limit: float = None, max_states: int = None) -> BatchResult:
        time_limit, max_states = self.reset(time_limit, max_states)
        cubes = DeviceCubes.of(states)
        cubes = DeviceCubes(cubes.soa.clone(), cubes.n)
        B = cubes.n
        cap = DEFAULT_STEP_CAP if _unbounded(max_states) else int(max_states)
        self.tt.tick()
        solved = cubes.is_solved().clone()
        root_solved = solved.clone()
        running = ~solved
        history, stamps = [], []     # stamps[i]: seconds on the agent's clock when step i had been queued and the loop's test had waited for step i - 1
        steps = torch.zeros(B, dtype=torch.int64, device=solved.device)
        while len(history) < cap and bool(running.any()) and self.tt.tock() < time_limit:
            actions = self._actions(cubes, running)
            actions[:B][~running] = 12                        # identity padding of the move table
            cubes.multi_rotate(actions, out=cubes)
            history.append(actions[:B].clone())
            steps += running
            now = cubes.is_solved()
            solved |= now & running
            running &= ~now
            stamps.append(self.tt.tock())
        torch.cuda.synchronize()
        seconds = self.tt.tock()
        hist = torch.stack(history, 1).cpu().numpy() if history else np.zeros((B, 0), dtype=np.uint8)
        steps, solved_h = steps.cpu().numpy(), solved.cpu().numpy()
        queues = [deque(int(a) for a in hist[g, :steps[g]]) for g in range(B)]
        lengths = np.where(solved_h, steps, -1)
        self._explored_states = int(steps[0])
        self.action_queue = queues[0]
        status = np.where(root_solved.cpu().numpy(), 4, np.where(solved_h, 1, 2))
        # a game's wall interval: from the start of the batch to the host's first look after its last move (`running.any()` synchronises
        # every step, so the look behind step i sees it done); games that ran to the end: the batch's seconds
        after = np.array(stamps[1:] + [seconds]) if stamps else np.zeros(0)
        each = np.where(steps > 0, after[np.maximum(steps, 1) - 1] if len(after) else seconds, stamps[0] if stamps else seconds)
        each = np.asarray(each, dtype=np.float64)
        return BatchResult(solved_h, lengths, steps.astype(np.int64), QueueTable.from_queues(queues), seconds, steps, status, each)

    def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
        res = self.search_batch(np.asarray(state)[None], time_limit, max_states)
        if self.shorten:
            self.action_queue = res.queues[0]
        return bool(res.solved[0])

    def _batch_for(self, n_slots: int, queue_width: int) -> "rd.RolloutBatch":
        b, want = self.batch, (n_slots, self.kind, int(self.steps_per_round), bool(self.use_graph))
        if b is None or (b.S, b.kind, b.K, b.use_graph) != want or b.Q < queue_width or b.Q > 4 * queue_width:
            self.batch = None
            torch.cuda.empty_cache()
            b = self.batch = rd.RolloutBatch(*want[:3], queue_width, use_graph=want[3])
        if self.kind != "random":
            b.set_net(self._search_net(), self.net_dtype)   # every search: `net` may have been trained or replaced since the last one
        return b

    @no_grad
    def _search_lockstep(self, roots: DeviceCubes, time_limit: float, max_states: int, seeds, slots) -> BatchResult:
        """`search_batch` behind `reset`: both limits are set (one may be `reset`'s stand-in for a limit that was not given).
        The host counts a game's moves: a game is drawn for while it has made fewer than `cap`."""
        by_states = not _unbounded(max_states)
        cap = int(max_states) if by_states else DEFAULT_STEP_CAP
        pool = SlotPool(roots.n, slots, self.tt.tock)
        batch = self._batch_for(pool.S, cap if by_states else min(cap, self.QUEUE_STEPS))
        streams = ed.GameStreams(seeds) if batch.table is not None else None   # (the greedy policy and the value agent draw nothing)
        res = lockstep_search(self, batch, pool, roots, time_limit, cap, cap, by_states, streams)
        # (None: the split engine could not represent an activation: the same search, same seeds, in fp32)
        return self._search_lockstep(roots, time_limit, max_states, seeds, slots) if res is None else res

    @staticmethod
    def _part(words: np.ndarray, host: torch.Tensor, ev) -> BatchResult:
        ev.synchronize()
        status, steps = words
        solved = (status == rd.SOLVED) | (status == rd.ROOT_SOLVED)
        return BatchResult(solved, np.where(solved, steps, -1), steps.copy(), QueueTable(host.numpy().copy(), steps), 0.0, steps.copy(),
                           status.copy())


def _pad16(t: torch.Tensor) -> torch.Tensor:
    n = t.numel()
    out = torch.zeros((n + 15) // 16 * 16, dtype=torch.uint8, device=t.device)
    out[:n] = t
    return out


class RandomSearch(_StepAgent):
    """Uniformly random moves from np.random (reference agents.py:82-90); one draw per running game per step."""
    kind = "random"

    def __init__(self, shorten: bool = False):
        """shorten: solved games return the shortest route through the states their walk visited (see `Agent.shorten`)."""
        super().__init__()
        self.shorten = bool(shorten)

    def _actions(self, cubes, running):
        a = torch.from_numpy(np.random.randint(12, size=cubes.n).astype(np.uint8)).to(cubes.soa.device)
        return _pad16(a)

    def __str__(self):
        return "Random depth-first search"


class _DeepStepAgent(_StepAgent, DeepAgent):
    def __init__(self, net, net_dtype=F32_SPLIT, deterministic: bool = False, use_graph: bool = True, steps_per_round: int = 8,
                 shorten: bool = False):
        """deterministic: as for `MCTS` -- one layer plan of the split engine for every row count, so a game of a lock-step search
        (`search_batch` with `seeds` or `slots`) does not depend on which other games share its batch.
        use_graph, steps_per_round: the lock-step search replays a round of that many (network pass, move) pairs as one
        captured graph.
        shorten: solved games return the shortest route through the states they visited (see `Agent.shorten`)."""
        DeepAgent.__init__(self, net, net_dtype, deterministic)
        self.use_graph, self.steps_per_round = use_graph, steps_per_round
        self.shorten = bool(shorten)
        self._engine = None

    def reset(self, time_limit, max_states):
        from librubiks.model import make_inference_net
        out = Agent.reset(self, time_limit, max_states)
        self._engine = make_inference_net(self._search_net(), self.net_dtype)   # rebuilt per search: weights may have been trained
        return out

    def _search_stepwise(self, states, time_limit: float = None, max_states: int = None) -> BatchResult:
        res = _StepAgent._search_stepwise(self, states, time_limit, max_states)
        if self._overflowed(self._engine):   # the split engine could not represent an activation: the same search in fp32
            res = _StepAgent._search_stepwise(self, states, time_limit, max_states)
        return res


class PolicySearch(_DeepStepAgent):
    """Follows the policy head: greedy argmax of softmax(policy), or samples it (reference agents.py:132-151)."""

    def __init__(self, net, sample_policy=False, net_dtype=F32_SPLIT, **kw):
        super().__init__(net, net_dtype, **kw)
        self.sample_policy = sample_policy

    @property
    def kind(self) -> str:
        return "sampled" if self.sample_policy else "greedy"

    @classmethod
    def from_saved(cls, loc: str, use_best: bool, sample_policy=False, **kw):
        return cls(Model.load(loc, load_best=use_best).to(gpu), sample_policy, **kw)

    def _actions(self, cubes, running):
        logits, _ = _evaluate(self._engine, cubes)
        p = torch.softmax(logits, dim=1)
        if self.sample_policy:   # np.random.choice per game, in game order (agents.py:140)
            pn = p.double().cpu().numpy()
            a = np.array([np.random.choice(12, p=row / row.sum()) for row in pn], dtype=np.uint8)
            return _pad16(torch.from_numpy(a).to(p.device))
        return _pad16(p.argmax(dim=1).to(torch.uint8))

    def __str__(self):
        return f"{'Sampled' if self.sample_policy else 'Greedy'} policy"


class ValueSearch(_DeepStepAgent):
    """Moves to the child of highest value; a solved child is taken at once (reference agents.py:154-169)."""
    kind = "value"

    def _actions(self, cubes, running):
        kids = cubes.expand12()
        solved = kids.is_solved().view(cubes.n, 12)
        v = _values(self._engine, kids).view(cubes.n, 12)
        best = v.argmax(dim=1)
        first_solved = solved.to(torch.uint8).argmax(dim=1)   # first True (argmax returns the first maximum)
        return _pad16(torch.where(solved.any(dim=1), first_solved, best).to(torch.uint8))

    def __str__(self):
        return "Greedy value"


class EGVM(DeepAgent):
    """
    Epsilon-greedy value maximisation (reference agents.py:649-726): `workers` epsilon-greedy policy
    rollouts of `depth` moves from the current state, then jump to the visited state of highest value.
    The random draws follow the reference's np.random call order, so a game is reproducible against
    it; the workers of a game run in parallel on the device.  `search` and a plain `search_batch` play the games one
    after another on the global stream; `search_batch(..., seeds=, slots=)` advances all games together on the device,
    each on its own stream (csrc/rubiks_egvm.hip, librubiks/solving/egvm_device.py).
    """

    def __init__(self, net, epsilon: float, workers: int, depth: int, net_dtype=F32_SPLIT, deterministic: bool = False,
                 use_graph: bool = True, shorten: bool = False):
        """deterministic: as for `MCTS` -- one layer plan of the split engine for every row count, so a game of a batched search
        (`search_batch` with `seeds` or `slots`) does not depend on which other games share its batch.
        use_graph: the batched search replays a round (D network passes and depth steps) as one captured graph.
        shorten: a solved game returns the shortest route through the states its queue visited instead of the queue itself, which
        strings together one epsilon-greedy path prefix per round and so wanders through states it has been in (see `Agent.shorten`)."""
        super().__init__(net, net_dtype, deterministic)
        self.epsilon, self.workers, self.depth = epsilon, workers, depth
        self.use_graph = use_graph
        self.shorten = bool(shorten)
        self.batch = None
        self.batch_stats = None

    @classmethod
    def from_saved(cls, loc: str, use_best: bool, epsilon: float, workers: int, depth: int, **kw):
        return cls(Model.load(loc, load_best=use_best).to(gpu), epsilon, workers, depth, **kw)

    def __str__(self):
        return f"EGVM (e={self.epsilon}, w={self.workers}, d={self.depth})"

    def search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
        ok = self._search_raw(state, time_limit, max_states)
        self._shorten_own_queue(state, ok)
        return ok

    def _search_raw(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
        rng = np.random.get_state()
        ok = self._search(state, time_limit, max_states)
        if self._overflowed(self._engine):   # the split engine could not represent an activation: the same search (same draws) in fp32
            np.random.set_state(rng)
            ok = self._search(state, time_limit, max_states)
        return ok

    @no_grad
    def _search(self, state: np.ndarray, time_limit: float = None, max_states: int = None) -> bool:
        from librubiks.model import make_inference_net
        time_limit, max_states = self.reset(time_limit, max_states)
        engine = self._engine = make_inference_net(self._search_net(), self.net_dtype)
        self.tt.tick()
        cur = DeviceCubes.from_numpy(np.asarray(state)[None])
        if bool(cur.is_solved()[0]):
            return True
        W, D = self.workers, self.depth
        while self.tt.tock() < time_limit and len(self) + W * D <= max_states:
            cubes = DeviceCubes.empty(W)
            cubes.soa[:, :W] = cur.soa[:, :1]
            paths = np.empty((W, D), dtype=int)
            visited = DeviceCubes.empty(W * D)
            hit = None
            for d in range(D):
                use_random = np.random.choice(2, W, p=[1 - self.epsilon, self.epsilon]).astype(bool)
                actions = np.empty(W, dtype=int)
                actions[use_random] = np.random.randint(0, 12, use_random.sum())
                if (~use_random).any():
                    logits, _ = _evaluate(engine, cubes)
                    actions[~use_random] = logits.argmax(dim=1).cpu().numpy()[~use_random]
                paths[:, d] = actions
                cubes.multi_rotate(_pad16(torch.from_numpy(actions.astype(np.uint8)).cuda()), out=cubes)
                solved = cubes.is_solved().cpu().numpy()
                if solved.any():
                    self._explored_states += (d + 1) * W
                    hit = (int(np.flatnonzero(solved)[0]), d + 1)
                    break
                visited.soa[:, d:W * D:D] = cubes.soa[:, :W]     # row w * depth + d (agents.py:681-682,714)
            if hit is not None:
                self.action_queue += deque(int(a) for a in paths[hit[0], :hit[1]])
                return True
            self._explored_states += W * D
            best = int(_values(engine, visited).argmax())
            cur = DeviceCubes.empty(1)
            cur.soa[:, :1] = visited.soa[:, best:best + 1]
            worker, depth = best // D, best % D
            self.action_queue += deque(int(a) for a in paths[worker, :depth + 1])
        return False

    def search_batch(self, states, time_limit: float = None, max_states: int = None, seeds=None, slots: int = None) -> BatchResult:
        """
        With neither `seeds` nor `slots`: one `search` after the other, drawing from the global np.random stream in the reference's
        call order.  Otherwise all games advance together on the device (librubiks/solving/egvm_device.py), round by round:
        game g draws from its own stream np.random.RandomState(seeds[g]) in the reference's order, and ends exactly -- solved
        flag, len(agent), action queue -- as the reference's `search(states[g])` would right after np.random.seed(seeds[g]),
        whoever shares the batch and however many slots there are, wherever the network's rows do not depend on the batch (the
        deterministic engine).  The clock is looked at between rounds only (agents.py:665), and `time_limit` bounds the whole search.
        seeds: integer array [G], or one integer s for RandomState(s).randint(0, 2**31 - 1, size=G); None (with `slots`): one
        such call on the global stream at entry.
        slots: search at most this many games at a time; finished games hand their slots to the scrambles still waiting
        (continuous batching, as `AStar.search_batch`).  Games that never got a slot before the time limit end unsolved, with 0
        nodes, status EXHAUSTED and 0 seconds.  `BatchResult.iterations` is the number of rounds per game.
        """
        if seeds is None and slots is None:
            return self._shortened(self._search_serial(states, time_limit, max_states), states)
        roots = DeviceCubes.of(states)
        seeds = ed.game_seeds(seeds, roots.n)
        time_limit, max_states = self.reset(time_limit, max_states)
        return self._shortened(self._search_lockstep(roots, time_limit, max_states, seeds, slots), roots)

    def _batch_for(self, n_slots: int, queue_width: int) -> "ed.EGVMBatch":
        b = self.batch
        if b is None or (b.S, b.W, b.D, b.use_graph) != (n_slots, self.workers, self.depth, bool(self.use_graph)) \
                or b.Q < queue_width or b.Q > 4 * queue_width:
            self.batch = None
            torch.cuda.empty_cache()
            b = self.batch = ed.EGVMBatch(n_slots, self.workers, self.depth, queue_width, use_graph=self.use_graph)
        b.set_net(self._search_net(), self.net_dtype)   # every search: `net` may have been trained or replaced since the last one
        b.set_epsilon(self.epsilon)
        return b

    QUEUE_ROUNDS = 64   # queue rows of a search bounded by time only start at this many rounds and double between rounds

    @no_grad
    def _search_lockstep(self, roots: DeviceCubes, time_limit: float, max_states: int, seeds: np.ndarray, slots) -> BatchResult:
        """`search_batch` behind `reset`: both limits are set (one may be `reset`'s stand-in for a limit that was not given).
        The host counts a game's rounds: a game is drawn for while it has played fewer than `rounds_cap`."""
        by_states = not _unbounded(max_states)
        rounds_cap = ed.queue_rounds(max_states, self.workers, self.depth)   # rounds a game can complete (agents.py:665)
        # (no round fits: every game is planted at once, so that solved scrambles are seen -- agents.py:661 comes before :665)
        pool = SlotPool(roots.n, slots if rounds_cap >= 1 else None, self.tt.tock)
        batch = self._batch_for(pool.S, self.depth * max(1, rounds_cap if by_states else self.QUEUE_ROUNDS))
        res = lockstep_search(self, batch, pool, roots, time_limit, int(max_states), rounds_cap, by_states, ed.GameStreams(seeds),
                              rounds_fit=rounds_cap >= 1)
        # (None: the split engine could not represent an activation: the same search, same seeds, in fp32)
        return self._search_lockstep(roots, time_limit, max_states, seeds, slots) if res is None else res

    @staticmethod
    def _part(words: np.ndarray, host: torch.Tensor, ev) -> BatchResult:
        ev.synchronize()
        status, nodes, qlen, rounds = words
        solved = (status == ed.SOLVED) | (status == ed.ROOT_SOLVED)
        return BatchResult(solved, np.where(solved, qlen, -1), nodes.copy(), QueueTable(host.numpy().copy(), qlen), 0.0, rounds.copy(),
                           status.copy())

    def _search_serial(self, states, time_limit: float = None, max_states: int = None) -> BatchResult:
        states = states.numpy() if isinstance(states, DeviceCubes) else np.asarray(states)
        solved, lengths, nodes, queues = [], [], [], []
        tt = TickTock()
        tt.tick()
        for s in states:
            ok = self._search_raw(s, time_limit, max_states)
            solved.append(ok), lengths.append(len(self.action_queue) if ok else -1)
            nodes.append(len(self)), queues.append(self.action_queue)
        solved = np.array(solved)
        return BatchResult(solved, np.array(lengths), np.array(nodes, dtype=np.int64), QueueTable.from_queues(queues), tt.tock(),
                           np.zeros(len(states), dtype=int), np.where(solved, 1, 2))
