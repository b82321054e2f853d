"""What a batched search returns: `BatchResult` (per-scramble outcome arrays) and the `QueueTable` of its action queues."""
from collections import deque

import numpy as np

from librubiks.solving.mcts_device import PATH_OVERFLOW


class QueueTable:
    """
    Action queues of a batch kept as rows of a (games, max_len) uint8 array plus a length per game; a
    `deque` of ints is only built for the games somebody indexes (`table[g]`, iteration).  Behaves like
    the list of deques it replaces.
    """

    def __init__(self, acts: np.ndarray = None, lens: np.ndarray = None, n: int = None):
        if acts is not None:
            self._rows = [(acts, i) for i in range(len(lens))]
            self._lens = np.asarray(lens, dtype=np.int64).copy()
        else:
            self._rows = [None] * n
            self._lens = np.zeros(n, dtype=np.int64)

    @classmethod
    def from_queues(cls, queues) -> "QueueTable":
        """The table of a list of per-game queues (agents that search one game after the other, or keep their moves per game)."""
        table = cls(n=len(queues))
        table[:] = queues
        return table

    def put(self, g: int, other: "QueueTable", i: int):
        self._rows[g], self._lens[g] = other._rows[i], other._lens[i]

    def set_row(self, g: int, acts: np.ndarray):
        """Game g's queue from an array of its own (a queue longer than the rows of the shared array)."""
        arr = np.ascontiguousarray(acts, dtype=np.uint8).reshape(1, -1)
        self._rows[g], self._lens[g] = (arr, 0), arr.shape[1]

    def lengths(self) -> np.ndarray:
        return self._lens

    def padded(self, games=None, fill: int = 255):
        """(uint8 [len(games), longest] array of the games' action queues padded with `fill`, their lengths): the queues of many
        games at once without building a deque per game (replaying / scoring whole result sets)."""
        games = np.arange(len(self)) if games is None else np.asarray(games, dtype=np.int64)
        lens = self._lens[games]
        out = np.full((len(games), int(lens.max()) if len(games) else 0), fill, dtype=np.uint8)
        for o, g in enumerate(games):
            src = self._rows[g]
            if src is not None and lens[o]:
                out[o, :lens[o]] = src[0][src[1], :lens[o]]
        return out, lens

    def __len__(self):
        return len(self._rows)

    def __getitem__(self, g):
        if isinstance(g, slice):
            return [self[i] for i in range(*g.indices(len(self)))]
        src = self._rows[g]
        if src is None:
            return deque()
        acts, i = src
        return deque(int(a) for a in acts[i, :self._lens[g]])

    def __setitem__(self, g, q):
        if isinstance(g, slice):
            for i, qq in zip(range(*g.indices(len(self))), q):
                self[i] = qq
            return
        arr = np.fromiter(q, dtype=np.uint8, count=len(q)).reshape(1, -1)
        self._rows[g], self._lens[g] = (arr, 0), len(q)

    def __iter__(self):
        return (self[g] for g in range(len(self)))


class BatchResult:
    """Per-scramble outcome of a batched search (shapes (B,)); `queues[t]` is tree t's action queue (a `QueueTable`)."""

    def __init__(self, solved, lengths, nodes, queues, seconds, iterations, status, game_seconds=None):
        self.solved, self.lengths, self.nodes, self.queues = solved, lengths, nodes, queues
        self.seconds, self.iterations, self.status = seconds, iterations, status
        # Per-game wall interval (float64 [B]) where the agent keeps one: from the moment the game's search starts (its tree is
        # planted / its problem enters the batch) to the moment the host sees it finished -- what the reference's Evaluator times
        # around agent.search (evaluation.py:45-52).  Games of one batch share the GPU, so these intervals OVERLAP: their sum is not
        # the batch's wall time (`seconds`).  None: the agent does not record them.
        self.game_seconds = game_seconds
        # Set by `shortened` on the result it returns: the lengths the search itself found, and the wall seconds of the shortening.
        self.raw_lengths, self.shorten_seconds = None, None
        # Set by `tightened` on the result it returns (which also sets raw_lengths where nothing has yet).
        self.tighten_seconds = None

    def shortened(self, states, budget_bytes: int = None) -> "BatchResult":
        """
        The result with every SOLVED game's queue replaced by the route the reference's graph shortening (agents.py:597-633 of
        the reference) finds through the states the queue visits (librubiks/solving/shorten.py): same end state, never longer,
        a function of the game alone.  `states`: the scrambles the search was given ((n, 20) int8 or DeviceCubes).  Unsolved
        games keep their queues (a best guess, not a solution).  `queues` and `lengths` are the shortened ones, `raw_lengths`
        what the search returned, `shorten_seconds` the wall time this took; `solved`, `nodes`, `status`, `iterations`,
        `seconds` and `game_seconds` are the search's.
        """
        import time

        from librubiks.solving import shorten as sh
        t0 = time.perf_counter()
        solved = np.asarray(self.solved, dtype=bool)
        queues, status = sh.shorten_queues(states, self.queues, select=solved & (self.queues.lengths() > 0), budget_bytes=budget_bytes)
        bad = np.flatnonzero((status != sh.OK) & (status != sh.SKIPPED))
        if len(bad):
            raise RuntimeError(f"shortening failed for games {bad[:8].tolist()}: {[sh.STATUS_NAMES[int(s)] for s in status[bad[:8]]]}")
        lengths = np.where(solved, queues.lengths(), self.lengths).astype(np.asarray(self.lengths).dtype)
        out = BatchResult(self.solved, lengths, self.nodes, queues, self.seconds, self.iterations, self.status, self.game_seconds)
        out.raw_lengths, out.shorten_seconds = np.asarray(self.lengths).copy(), time.perf_counter() - t0
        return out

    def tightened(self, table, window: int = None, budget_bytes: int = None) -> "BatchResult":
        """
        The result with every SOLVED game's non-empty queue replaced by what `table` (a NearTable, librubiks/solving/near.py)
        makes of it: every stretch of at most `window` moves (None: the whole queue) whose product lies within the table's depth
        of solved gives way to that product's optimal sequence, chosen so that the queue is as short as such replacements can make
        it.  Same product, hence still a solution; never longer.  Unsolved games keep their queues.  `raw_lengths` stays what an
        earlier `shortened` recorded, else becomes this result's lengths, so `result.shortened(states).tightened(table)` still
        tells what the search returned; `tighten_seconds` is the wall time this took; everything else is the search's.
        """
        import time

        from librubiks.solving import near
        t0 = time.perf_counter()
        solved = np.asarray(self.solved, dtype=bool)
        queues, status = table.tighten(self.queues, select=solved & (self.queues.lengths() > 0), window=window, budget_bytes=budget_bytes)
        bad = np.flatnonzero((status != near.OK) & (status != near.SKIPPED))
        if len(bad):
            raise RuntimeError(f"tightening failed for games {bad[:8].tolist()}: {[near.STATUS_NAMES[int(s)] for s in status[bad[:8]]]}")
        lengths = np.where(solved, queues.lengths(), self.lengths).astype(np.asarray(self.lengths).dtype)
        out = BatchResult(self.solved, lengths, self.nodes, queues, self.seconds, self.iterations, self.status, self.game_seconds)
        out.raw_lengths = np.asarray(self.lengths).copy() if self.raw_lengths is None else self.raw_lengths
        out.shorten_seconds, out.tighten_seconds = self.shorten_seconds, time.perf_counter() - t0
        return out

    def excess(self, table, states, extra: int = 0, launch_items: int = None) -> np.ndarray:
        """
        int32 [B]: for every SOLVED game its solution's length minus the exact distance of its scramble, found by
        `table.reach(states, extra)` (a NearTable, librubiks/solving/near.py) -- 0 is an optimal solution; -1 where the game is
        unsolved or the scramble lies farther than the table's depth + `extra`.  `states`: the scrambles the search was given
        ((n, 20) int8 or DeviceCubes).  Only the solved games are searched.  Composes with the other two:
        `result.shortened(states).tightened(table).excess(table, states, extra=4)`.
        """
        from librubiks.cube.device import DeviceCubes
        solved = np.flatnonzero(np.asarray(self.solved, dtype=bool))
        out = np.full(len(self.solved), -1, dtype=np.int32)
        if len(solved):
            rows = states.numpy() if isinstance(states, DeviceCubes) else np.asarray(states)
            dist = table.reach(rows[solved], extra=extra, launch_items=launch_items).distances.astype(np.int32)
            out[solved] = np.where(dist >= 0, np.asarray(self.lengths)[solved].astype(np.int32) - dist, -1)
        return out

    @property
    def states_per_sec(self) -> float:
        return float(self.nodes.sum()) / max(self.seconds, 1e-12)

    @property
    def path_overflow_trees(self) -> int:
        """Trees that ended because a descent filled the path store (status PATH_OVERFLOW).  The reference has no such limit
        (agents.py:575-595): with the default store (MCTS(max_path=None)) this is HBM / address space running out and is 0 in
        every run on record; a caller who bounds the store (max_path=...) reads here what that bound cost."""
        return int((np.asarray(self.status) == PATH_OVERFLOW).sum())

    def select(self, mask: np.ndarray) -> "BatchResult":
        idx = np.flatnonzero(mask)
        queues = QueueTable(n=len(idx))
        for o, i in enumerate(idx):
            queues.put(o, self.queues, int(i))
        return BatchResult(self.solved[idx], self.lengths[idx], self.nodes[idx], queues,
                           self.seconds, self.iterations[idx], self.status[idx],
                           None if self.game_seconds is None else self.game_seconds[idx])

    @staticmethod
    def merge(n: int, parts, seconds: float) -> "BatchResult":
        """Reassembles per-game results from (original indices, BatchResult) pieces."""
        solved, lengths = np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int64)
        nodes, iters, status = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        queues = QueueTable(n=n)
        for owner, r in parts:
            solved[owner], lengths[owner], nodes[owner] = r.solved, r.lengths, r.nodes
            iters[owner], status[owner] = r.iterations, r.status
            for i, o in enumerate(owner):
                queues.put(int(o), r.queues, i)
        return BatchResult(solved, lengths, nodes, queues, seconds, iters, status)
