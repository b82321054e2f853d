"""
The near-solved table (csrc/rubiks_near.hip, rc_near_* in include/rubiks_hip.h): every state within K quarter turns of the solved
cube, built once on the device by the reference's breadth-first search (librubiks/solving/agents.py:92-131 of the reference)
started at the solved state, with each state's exact depth and the move that discovered it.  It answers what nothing else in the
package can: how far a state really is from solved, an optimal solution of a near state, and -- by a dynamic programme over a
queue's moves -- the queue with every stretch whose product lies in the table replaced by that product's optimal sequence.

    NearTable(depth=K) / NearTable.get(K)   builds (caches) the table
    table.depths(states)                    exact distances, -1 beyond K
    table.solve(states)                     optimal solutions of the states within K
    table.tighten(queues, ...)              tighter queues with the same product; plan_tighten_chunks is its pure planning step
    table.reach(states, extra=J)            exact distances and optimal solutions up to K + J (csrc/rubiks_near_reach.hip)
    BatchResult.tightened(table)            the solved games of a search result (librubiks/solving/results.py)
    BatchResult.excess(table, states, J)    how many moves each solution is longer than the optimum
"""
import ctypes
from collections import namedtuple
from ctypes import Structure, c_size_t, c_uint32, c_void_p

import numpy as np
import torch

from librubiks import _hip
from librubiks.cube.device import DeviceCubes
from librubiks.solving.results import QueueTable
from librubiks.solving.shorten import _as_table

MAX_DEPTH = 8                # RC_NEAR_MAX_DEPTH: node ids and cells are int32, a depth is four bits; K = 8 takes about 2.5 GB
CORRUPT = 1                  # RC_NEAR_CORRUPT
OK, SKIPPED, BAD_ACTION, FAILED, NO_ROOM = 0, 1, 2, 3, 4   # RC_NEAR_T_*: the numbers of shorten.py's statuses
STATUS_NAMES = {OK: "ok", SKIPPED: "skipped", BAD_ACTION: "bad action", FAILED: "failed", NO_ROOM: "no room"}
MAX_LEN = (1 << 27) - 2      # RC_NEAR_T_MAX_LEN
# States at exactly d quarter turns, d = 0 .. 8 (the published quarter-turn counts; tests/test_near_model.py computes the first
# six from the move tables and the device build is checked against them level by level).  They size the node rows only: a build
# that finds another count raises.
SPHERE_SIZES = (1, 12, 114, 1068, 10011, 93840, 878880, 8221632, 76843595)
# Not tuned.  profiles/near_table_probe.txt: a larger K tightens more (MCTS solutions 155.5 -> 122.2 at K = 6, 86.0 at K = 8) for the
# same milliseconds per batch, and costs memory (24 MiB at K = 6, 2.4 GiB at K = 8); nothing there weighs that against a search's own.
DEFAULT_DEPTH = 6            # 983 926 states, about 25 MB
DEFAULT_WINDOW = None        # the whole queue
DEFAULT_BUDGET_BYTES = 2 << 30
DEFAULT_CHUNK_ROWS = 12 << 19   # child rows per launch of the build: 28 bytes each


class _NearStruct(Structure):   # mirrors rc_near_t (include/rubiks_hip.h)
    _fields_ = [(name, c_uint32) for name in ("depth", "capacity", "hash_size", "n_nodes", "chunk_rows", "reserved")] + \
               [(name, c_void_p) for name in ("keys", "meta", "hash", "words", "child_keys", "child_slot", "flags", "prefix", "scan_tmp")] + \
               [("scan_tmp_bytes", c_size_t)]


class _TightenStruct(Structure):   # mirrors rc_near_tighten_t
    _fields_ = [(name, c_uint32) for name in ("n_games", "queue_width", "out_width", "max_len", "window", "reserved")] + \
               [("total_positions", c_size_t), ("total_band", c_size_t)] + \
               [(name, c_void_p) for name in ("queues", "lens", "select", "band_off", "pos_off", "band", "best", "from_", "out_queues",
                                              "out_lens", "status")]


TIGHTEN_POINTERS = [name for name, _ in _TightenStruct._fields_[8:]]
STEPS = ("rc_near_tighten_distances", "rc_near_tighten_route")

# ---- beyond the table (rc_near_reach_*) ----
MAX_EXTRA = 10               # RC_NEAR_REACH_MAX_EXTRA: 12^10 sequence numbers fit the 36 bits a best word has for them
NO_WORD = np.uint64((1 << 64) - 1)   # a best word without a hit; else depth << 40 | level << 36 | index
REACH_POINTERS = ("soa", "live", "best", "dist_out", "level_out", "out_queues", "out_lens", "status")
# A work item is (state, the first min(level, P) moves); the lane of an item walks the 12^(level - P) sequences behind them.
# P is the smallest that gives a level 2^22 items (each of the device's lanes some) and leaves an item at most REACH_WALK moves:
# the walk keeps a key per move in registers, and three moves (1 728 sequences, about 840 of them canonical) keep four waves a SIMD.
REACH_ITEMS_TARGET = 1 << 22
REACH_WALK = 3
# Sequences (12^(level - P) an item, the pruned ones counted) that one launch may cover: launch_items=None cuts a level into launches
# of DEFAULT_LAUNCH_LEAVES // 12^(level - P) items.  profiles/near_reach_probe.txt, 1 024 states, K = 8 (2.4 GiB of table), J = 8:
# the launches of level 8 (2 485 513 items of 12^3) take at most 0.060 s, of level 7 (29 826 161 items of 12^2) 0.046 s, a whole
# level 6 in one launch 0.044 s; at K = 6 the longest is 0.070 s.  15-22 G probes/s, so 2^32 sequences could take 0.3 s if none were
# pruned and every state were live: well under a second, and a level of 1 024 states at J = 8 is still about a hundred launches.
DEFAULT_LAUNCH_LEAVES = 1 << 32


class _ReachStruct(Structure):   # mirrors rc_near_reach_t
    _fields_ = [("n", c_size_t), ("stride", c_size_t)] + [(name, c_uint32) for name in ("extra", "prefix", "out_width", "reserved")] + \
               [(name, c_void_p) for name in REACH_POINTERS]


ReachResult = namedtuple("ReachResult", "distances queues lengths levels items seconds")
ReachResult.__doc__ = """What `NearTable.reach` returns: distances int8 [n] (-1: farther than K + extra), queues (a QueueTable of optimal
solutions, empty where there is no distance), lengths int32 [n] (= distances), levels int8 [n] (moves walked before the table
was hit, -1 without a distance), items (work items launched at the levels >= 1) and the wall seconds."""


def reach_items(level: int, prefix: int) -> int:
    """rc_near_reach_items: work items per state of a level."""
    return 12 ** min(int(level), int(prefix))


def default_prefix(n: int, extra: int) -> int:
    P = 0
    while P < extra and n * 12 ** P < REACH_ITEMS_TARGET:
        P += 1
    return max(P, extra - REACH_WALK)


def default_launch_items(level: int, prefix: int) -> int:
    return max(1, DEFAULT_LAUNCH_LEAVES // 12 ** (level - min(level, prefix)))


# ---- planning (pure) ---------------------------------------------------------------------------------------------------------
def band_bytes(lengths, window=None) -> np.ndarray:
    """Bytes of d(i, j) a game of `lengths` moves takes: L * min(L, window); 0 for a game that is left alone (L < 0)."""
    L = np.maximum(np.asarray(lengths, dtype=np.int64), 0)
    return L * (L if window is None else np.minimum(L, int(window)))


def workspace_bytes(band: int, positions: int) -> int:
    """The band and the two int32 words (best, from) per position, each array rounded up to 256 bytes."""
    r = lambda x: (int(x) + 255) // 256 * 256   # noqa: E731
    return r(band) + 2 * r(4 * int(positions))


def plan_tighten_chunks(lengths, window=None, budget_bytes: int = DEFAULT_BUDGET_BYTES) -> list:
    """
    Game ranges [(lo, hi), ...] that cover range(len(lengths)) in order, each as long as the workspace of its games fits
    `budget_bytes`.  lengths[g] < 0: game g is left alone and costs nothing.  A game that alone exceeds the budget raises
    ValueError (a smaller `window` makes it fit).
    """
    L = np.asarray(lengths, dtype=np.int64)
    band, pos = band_bytes(L, window), np.where(L < 0, 0, L + 1)
    chunks, lo, B, P = [], 0, 0, 0
    for g in range(len(L)):
        b, p = int(band[g]), int(pos[g])
        if workspace_bytes(b, p) > budget_bytes:
            raise ValueError(f"game {g}: a queue of {int(L[g])} moves needs {workspace_bytes(b, p)} bytes of workspace with window {window}, "
                             f"the budget is {budget_bytes}")
        if g > lo and workspace_bytes(B + b, P + p) > budget_bytes:
            chunks.append((lo, g))
            lo, B, P = g, 0, 0
        B, P = B + b, P + p
    if len(L) > lo:
        chunks.append((lo, len(L)))
    return chunks


def _cells_for(capacity: int) -> int:
    cells = 2
    while cells < 2 * capacity:
        cells *= 2
    return cells


# ---- one chunk of queues on the device -------------------------------------------------------------------------------------------
class TightenBatch:
    """The device arrays of one chunk and the rc_near_tighten_t that names them (tests fill one by hand, e.g. a narrow out_width)."""

    def __init__(self, table: "NearTable", queues: np.ndarray, lens: np.ndarray, select: np.ndarray, window=None, out_width: int = None):
        self.table, self.lib = table, _hip.lib()
        dev = table.device
        lens, select = np.asarray(lens, dtype=np.int32), np.asarray(select).astype(np.uint8)
        G = len(lens)
        queues = np.ascontiguousarray(queues, dtype=np.uint8)
        queues = queues.reshape(G, -1) if queues.size else np.zeros((G, 1), dtype=np.uint8)
        assert G >= 1 and select.shape == (G,)
        chosen = select != 0
        max_len = int(lens[chosen].max()) if chosen.any() else 0
        if max_len > min(MAX_LEN, queues.shape[1]) or (chosen.any() and int(lens[chosen].min()) < 0):
            raise ValueError(f"queue lengths {int(lens[chosen].min())} .. {max_len}: they lie in 0 .. min({MAX_LEN}, row width {queues.shape[1]})")
        if window is not None and int(window) < 1:
            raise ValueError(f"window {window}: at least 1 (None: the whole queue)")
        eff = np.where(chosen, lens.astype(np.int64), -1)
        self.band_off_h = np.concatenate([[0], np.cumsum(band_bytes(eff, window))]).astype(np.uint64)
        self.pos_off_h = np.concatenate([[0], np.cumsum(np.where(eff < 0, 0, eff + 1))]).astype(np.uint64)
        B, P = int(self.band_off_h[-1]), max(1, int(self.pos_off_h[-1]))
        self.G, self.max_len, self.bytes = G, max_len, workspace_bytes(B, P)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)     # noqa: E731
        self.queues, self.lens, self.select = up(queues), up(lens), up(select)
        self.band_off, self.pos_off = up(self.band_off_h.view(np.int64)), up(self.pos_off_h.view(np.int64))
        self.band, self.best, self.from_ = z((max(1, B),), torch.uint8), z((P,), torch.int32), z((P,), torch.int32)
        W = max(1, max_len if out_width is None else int(out_width))
        self.out_queues, self.out_lens, self.status = z((G, W), torch.uint8), z((G,), torch.int32), z((G,), torch.int32)
        s = _TightenStruct()
        s.n_games, s.queue_width, s.out_width, s.max_len = G, queues.shape[1], W, max_len
        s.window = max(1, min(max_len, MAX_LEN) if window is None else min(int(window), MAX_LEN))
        s.total_positions, s.total_band = P, B
        for name in TIGHTEN_POINTERS:
            setattr(s, name, getattr(self, name).data_ptr())
        self.struct = s

    def step(self, name: str):
        _hip.check(getattr(self.lib, name)(ctypes.byref(self.table.struct), ctypes.byref(self.struct), _hip.stream_ptr()), name)

    def run(self, timings: dict = None):
        """The two steps; with `timings`, each between two events: timings[step] gets a list of (start, end) event pairs."""
        if timings is None:
            return self.step("rc_near_tighten")
        for name in STEPS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.step(name)
            b.record()
            timings.setdefault(name, []).append((a, b))


# ---- one batch of states searched beyond the table -----------------------------------------------------------------------------
class ReachBatch:
    """The device arrays of one `reach` and the rc_near_reach_t that names them; `begin`, `level` and `finish` are the three entry
    points (tests drive them by hand and read `words()` and `live` in between)."""

    def __init__(self, table: "NearTable", states, extra: int, prefix: int = None, out_width: int = None):
        self.table, self.lib = table, _hip.lib()
        if ctypes.sizeof(_ReachStruct) != self.lib.rc_near_reach_struct_bytes():
            raise _hip.RubiksHipError(f"rc_near_reach_t has {self.lib.rc_near_reach_struct_bytes()} bytes, its mirror {ctypes.sizeof(_ReachStruct)}")
        extra = int(extra)
        if not 0 <= extra <= MAX_EXTRA:
            raise ValueError(f"extra {extra}: 0 .. {MAX_EXTRA}")
        if prefix is not None and not 0 <= int(prefix) <= MAX_EXTRA:
            raise ValueError(f"prefix {prefix}: 0 .. {MAX_EXTRA}")
        self.cubes = DeviceCubes.of(states)
        n, dev = self.cubes.n, table.device
        assert n >= 1
        self.n, self.extra = n, extra
        self.prefix = default_prefix(n, extra) if prefix is None else int(prefix)
        W = max(1, table.depth + extra if out_width is None else int(out_width))
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        self.soa = self.cubes.soa
        self.live, self.best = z((n,), torch.uint8), z((n,), torch.int64)    # (the words are unsigned: `words`)
        self.dist_out, self.level_out = z((n,), torch.int8), z((n,), torch.int8)
        self.out_queues, self.out_lens, self.status = z((n, W), torch.uint8), z((n,), torch.int32), z((2,), torch.int32)
        s = _ReachStruct()
        s.n, s.stride, s.extra, s.prefix, s.out_width = n, self.cubes.stride, extra, self.prefix, W
        for name in REACH_POINTERS:
            setattr(s, name, getattr(self, name).data_ptr())
        self.struct = s

    def _args(self):
        return ctypes.byref(self.table.struct), ctypes.byref(self.struct)

    def begin(self):
        _hip.check(self.lib.rc_near_reach_begin(*self._args(), _hip.stream_ptr()), "rc_near_reach_begin")

    def level(self, level: int, first: int, count: int):
        _hip.check(self.lib.rc_near_reach_level(*self._args(), level, first, count, _hip.stream_ptr()), "rc_near_reach_level")

    def finish(self):
        _hip.check(self.lib.rc_near_reach_finish(*self._args(), _hip.stream_ptr()), "rc_near_reach_finish")

    def items(self, level: int) -> int:
        """Work items of the whole batch at `level`."""
        return self.n * reach_items(level, self.prefix)

    def unresolved(self) -> int:
        """The one read between two levels: states without a distance after the calls so far."""
        return int(self.status[1].item())

    def words(self) -> np.ndarray:
        return self.best.cpu().numpy().view(np.uint64)


# ---- the table -----------------------------------------------------------------------------------------------------------------
class NearTable:
    """
    Every state within `depth` quarter turns of solved, resident on `device`: `.counts` (states per depth, depth + 1 ints),
    `.n_nodes`, `.bytes` (keys, meta bytes and cells), `.build_seconds`.  chunk_rows: child rows per launch of the build (the
    table does not depend on it).
    """
    DEFAULT_DEPTH = DEFAULT_DEPTH
    DEFAULT_WINDOW = DEFAULT_WINDOW
    _cache = {}

    def __init__(self, depth: int = None, device=None, chunk_rows: int = None):
        import time
        depth = DEFAULT_DEPTH if depth is None else int(depth)
        if not 1 <= depth <= MAX_DEPTH:
            raise ValueError(f"depth {depth}: the table holds depths 1 .. {MAX_DEPTH} (node ids and cells are int32; depth {MAX_DEPTH} takes about 2.5 GB)")
        self.lib = _hip.lib()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.depth = depth
        capacity = int(sum(SPHERE_SIZES[:depth + 1]))
        cells = _cells_for(capacity)
        widest = 12 * max(SPHERE_SIZES[:depth])          # rows of the largest level's children
        rows = min(int(chunk_rows or DEFAULT_CHUNK_ROWS), widest)
        if rows < 12:
            raise ValueError(f"chunk_rows {chunk_rows}: at least 12 (one parent)")
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)   # noqa: E731
            self.keys, self.meta, self.hash = z((capacity, 4), torch.int32), z((capacity,), torch.uint8), z((cells,), torch.int32)
            words = z((4,), torch.int32)
            scan_bytes = int(self.lib.rc_near_scan_bytes(rows))
            work = [z((rows, 4), torch.int32), z((rows,), torch.int32), z((rows,), torch.int32), z((rows,), torch.int32), z((scan_bytes,), torch.uint8)]
            s = _NearStruct()
            s.depth, s.capacity, s.hash_size, s.n_nodes, s.chunk_rows = depth, capacity, cells, 0, rows
            s.keys, s.meta, s.hash, s.words = self.keys.data_ptr(), self.meta.data_ptr(), self.hash.data_ptr(), words.data_ptr()
            s.child_keys, s.child_slot, s.flags, s.prefix, s.scan_tmp = (w.data_ptr() for w in work)
            s.scan_tmp_bytes = scan_bytes
            self.struct = s
            stream = _hip.stream_ptr()
            _hip.check(self.lib.rc_near_begin(ctypes.byref(s), stream), "rc_near_begin")
            counts, lo, n = [1], 0, 1
            per_launch = rows // 12
            for level in range(1, depth + 1):
                for p in range(lo, n, per_launch):     # the frontier: nodes lo .. n - 1
                    _hip.check(self.lib.rc_near_expand(ctypes.byref(s), p, min(per_launch, n - p), level, stream), "rc_near_expand")
                stored, overflow = (int(w) for w in words[:2].cpu())   # the one read of the level: its count
                if overflow or stored - n != SPHERE_SIZES[level]:
                    raise _hip.RubiksHipError(f"near table: level {level} brought {stored - n} states (overflow {overflow}), {SPHERE_SIZES[level]} exist")
                counts.append(stored - n)
                lo, n = n, stored
            s.n_nodes = n
            for name in ("words", "child_keys", "child_slot", "flags", "prefix", "scan_tmp"):   # the build's arrays are freed
                setattr(s, name, None)
            s.scan_tmp_bytes, s.chunk_rows = 0, 0
        self.counts, self.n_nodes = np.array(counts, dtype=np.int64), n
        self.bytes = capacity * 17 + cells * 4
        self.build_seconds = time.perf_counter() - t0

    @classmethod
    def get(cls, depth: int = None, device=None) -> "NearTable":
        """The table of (device, depth), built on first use and kept."""
        depth = DEFAULT_DEPTH if depth is None else int(depth)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        key = (str(dev), depth)
        if key not in cls._cache:
            cls._cache[key] = cls(depth, dev)
        return cls._cache[key]

    # ---- the table's arrays on the host (tests compare them with the model node for node) -------------------------------------
    def nodes(self):
        """(keys uint32 [n, 4], depth uint8 [n], action uint8 [n]) in discovery order."""
        meta = self.meta[:self.n_nodes].cpu().numpy()
        return self.keys[:self.n_nodes].cpu().numpy().view(np.uint32), meta >> 4, meta & 15

    def _status(self):
        return torch.zeros(1, dtype=torch.int32, device=self.device)

    def _check(self, status, what):
        if int(status.item()) != 0:
            raise _hip.RubiksHipError(f"{what}: the near table's cells or meta bytes are not what the build wrote (RC_NEAR_CORRUPT)")

    def depths(self, states, with_nodes: bool = False):
        """int8 [n]: the exact distance of every state, -1 for "farther than depth".  states: (n, 20) int8 or DeviceCubes.
        with_nodes: -> (depths, int32 [n] node ids, -1 where there is none)."""
        cubes = DeviceCubes.of(states)
        n = cubes.n
        out = torch.empty((max(n, 1),), dtype=torch.int8, device=self.device)
        nodes = torch.empty((max(n, 1),), dtype=torch.int32, device=self.device) if with_nodes else None
        if n:
            status = self._status()
            _hip.check(self.lib.rc_near_depth(ctypes.byref(self.struct), cubes.soa.data_ptr(), n, cubes.stride, out.data_ptr(),
                                              nodes.data_ptr() if with_nodes else None, status.data_ptr(), _hip.stream_ptr()), "rc_near_depth")
            self._check(status, "rc_near_depth")
        d = out[:n].cpu().numpy()
        return (d, nodes[:n].cpu().numpy()) if with_nodes else d

    def solve(self, states):
        """-> (QueueTable, int32 [n] lengths): an optimal solution of every state within `depth` (its length is the state's exact
        distance), and length -1 with an empty queue for the states beyond."""
        cubes = DeviceCubes.of(states)
        n = cubes.n
        rows = torch.zeros((max(n, 1), self.depth), dtype=torch.uint8, device=self.device)
        lens = torch.full((max(n, 1),), -1, dtype=torch.int32, device=self.device)
        if n:
            status = self._status()
            _hip.check(self.lib.rc_near_solve(ctypes.byref(self.struct), cubes.soa.data_ptr(), n, cubes.stride, rows.data_ptr(), self.depth,
                                              lens.data_ptr(), status.data_ptr(), _hip.stream_ptr()), "rc_near_solve")
            self._check(status, "rc_near_solve")
        lengths = lens[:n].cpu().numpy()
        return QueueTable(rows[:n].cpu().numpy(), np.maximum(lengths, 0)), lengths

    def reach(self, states, extra: int = 0, launch_items: int = None, timings: dict = None, prefix: int = None) -> ReachResult:
        """
        Exact distances and optimal solutions up to depth + `extra` quarter turns: the table is one half of a bidirectional search,
        and this walks the other half.  For j = 0 .. extra in turn every sequence of j moves is applied to a state and the result
        probed in the table; the first level with a hit gives the distance j + (smallest depth hit), and the hit with the smallest
        (depth, sequence number) followed by its state's `solve` is the solution (the rule, and why walking only canonical
        sequences changes nothing: include/rubiks_hip.h).  A level runs only while a state is without a distance.
        states: (n, 20) int8 or DeviceCubes.  extra=0 is exactly `depths` and `solve`.  launch_items: work items per launch at
        most (None: DEFAULT_LAUNCH_LEAVES sequences a launch); prefix: the moves a work item's number holds (None: chosen from n
        and extra).  The result depends on neither.  timings: a dict that receives, per level, the HIP event pairs of its launches.
        """
        import time
        extra = int(extra)
        if not 0 <= extra <= MAX_EXTRA:
            raise ValueError(f"extra {extra}: 0 .. {MAX_EXTRA} (a sequence's number has 36 bits)")
        if launch_items is not None and int(launch_items) < 1:
            raise ValueError(f"launch_items {launch_items}: at least 1 (None: {DEFAULT_LAUNCH_LEAVES} sequences a launch)")
        if prefix is not None and not 0 <= int(prefix) <= MAX_EXTRA:
            raise ValueError(f"prefix {prefix}: 0 .. {MAX_EXTRA}")
        cubes = DeviceCubes.of(states)
        n = cubes.n
        if n == 0:
            return ReachResult(np.zeros(0, dtype=np.int8), QueueTable(n=0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int8), 0, 0.0)
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):
            batch = ReachBatch(self, cubes, extra, prefix)
            batch.begin()
            items = 0
            for level in range(1, extra + 1):
                if batch.unresolved() == 0:
                    break
                total = batch.items(level)
                per = default_launch_items(level, batch.prefix) if launch_items is None else int(launch_items)
                for first in range(0, total, per):
                    count = min(per, total - first)
                    if timings is not None:
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                    batch.level(level, first, count)
                    if timings is not None:
                        b.record()
                        timings.setdefault(level, []).append((a, b))
                    items += count
            batch.finish()
            status = int(batch.status[0].item())
            if status != 0:
                raise _hip.RubiksHipError("rc_near_reach: the near table's cells or meta bytes are not what the build wrote (RC_NEAR_CORRUPT)")
            dist, levels, lengths = batch.dist_out.cpu().numpy(), batch.level_out.cpu().numpy(), batch.out_lens.cpu().numpy()
            queues = QueueTable(batch.out_queues.cpu().numpy(), np.maximum(lengths, 0))
        return ReachResult(dist, queues, lengths, levels, items, time.perf_counter() - t0)

    def tighten(self, queues, lengths=None, select=None, window=None, budget_bytes: int = None, timings: dict = None, info: dict = None):
        """
        -> (QueueTable, status int32 [n]).  queues: a QueueTable, a padded uint8 array [n, width] with `lengths`, or a list of
        action sequences; select: bool [n], the games to tighten (default: all); window: the longest stretch replaced at once
        (None: the whole queue).  Row g of the result is, where status[g] == OK, the shortest queue that can be made from game g's
        by replacing stretches of at most `window` moves whose product lies in the table by that product's optimal sequence: never
        longer, the same product, hence the same end state from any root.  Everywhere else it is the queue as it came (SKIPPED:
        not selected; BAD_ACTION: a byte >= 12 inside its length).  The games are cut into chunks whose workspace fits
        `budget_bytes` (`plan_tighten_chunks`); the result does not depend on the cut.
        timings: a dict that receives, per launch, the HIP event pairs of every chunk; info: receives workspace bytes and chunks.
        """
        if isinstance(queues, np.ndarray) and queues.ndim == 2 and lengths is None:
            raise ValueError("a padded array of queues needs `lengths`")
        table = _as_table(queues, lengths, None)
        n = len(table)
        lens = table.lengths().astype(np.int64)
        chosen = np.ones(n, dtype=bool) if select is None else np.asarray(select).astype(bool)
        window = DEFAULT_WINDOW if window is None else int(window)
        chunks = plan_tighten_chunks(np.where(chosen, lens, -1), window, DEFAULT_BUDGET_BYTES if budget_bytes is None else int(budget_bytes))
        out, status = QueueTable(n=n), np.full(n, SKIPPED, dtype=np.int32)
        for g in range(n):
            out.put(g, table, g)
        peak = 0
        with torch.cuda.device(self.device):
            for lo, hi in chunks:
                if not chosen[lo:hi].any():
                    continue
                acts, ls = table.padded(np.arange(lo, hi), fill=0)
                batch = TightenBatch(self, acts, ls, chosen[lo:hi], window)
                batch.run(timings)
                peak = max(peak, batch.bytes)
                rows, out_lens, st = batch.out_queues.cpu().numpy(), batch.out_lens.cpu().numpy(), batch.status.cpu().numpy()
                status[lo:hi] = st
                done = np.flatnonzero(st == OK)
                if len(done):
                    part = QueueTable(rows, np.where(st == OK, out_lens, 0))
                    for i in done:
                        out.put(lo + int(i), part, int(i))
        if info is not None:
            info.update(chunks=len(chunks), workspace_bytes=peak)
        return out, status
