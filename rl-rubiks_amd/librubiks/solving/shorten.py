"""
Shortening action queues through the graph of the states they visit (csrc/rubiks_shorten.hip, rc_shorten_* in
include/rubiks_hip.h): the reference's `_complete_graph` and `_shorten_action_queue` (librubiks/solving/agents.py:597-633 of the
reference), which it applies to a solved MCTS(search_graph=True) only, run on the path of any queue.  The nodes are the distinct
states a queue passes through, the edges every move between two of them -- not only the moves the queue made --, and the result is
the route the reference's ordered breadth-first search finds from the root to the queue's end state: never longer than the
queue, ending in the same state, and a function of the game alone.

    shorten_queues(states, queues)          uploads, plans chunks under a memory budget, launches, reads back
    plan_chunks(lengths, budget_bytes)      the pure planning step
    BatchResult.shortened(states)           the solved games of a search result (librubiks/solving/results.py)
"""
import ctypes
from ctypes import POINTER, Structure, c_size_t, c_uint32, c_void_p

import numpy as np
import torch

from librubiks import _hip
from librubiks.cube.device import DeviceCubes, _stride_for
from librubiks.solving.results import QueueTable

OK, SKIPPED, BAD_ACTION, FAILED, NO_ROOM = 0, 1, 2, 3, 4
STATUS_NAMES = {OK: "ok", SKIPPED: "skipped", BAD_ACTION: "bad action", FAILED: "failed", NO_ROOM: "no room"}
MAX_LEN = (1 << 27) - 2      # RC_SHORTEN_MAX_LEN: parent << 4 | action and the scan index 12 i + a are int32 words
# Workspace a chunk of games may take.  Not tuned: nothing has been measured yet that would prefer another value; it only has to
# be small beside HBM and large enough that a batch of ordinary queues is one chunk.
DEFAULT_BUDGET_BYTES = 2 << 30


class _ShortenStruct(Structure):   # mirrors rc_shorten_t (include/rubiks_hip.h)
    _fields_ = [("n_games", c_uint32), ("queue_width", c_uint32), ("out_width", c_uint32), ("max_len", c_uint32),
                ("stride", c_size_t), ("total_positions", c_size_t), ("total_hash_cells", c_size_t)] + \
               [(name, c_void_p) for name in ("roots_soa", "queues", "lens", "select", "pos_off", "hash_off", "keys", "ids", "nbr", "claim",
                                              "frontier_a", "frontier_b", "hash", "out_queues", "out_lens", "status")]


POINTER_FIELDS = [name for name, _ in _ShortenStruct._fields_[7:]]
STEPS = ("rc_shorten_index", "rc_shorten_neighbours", "rc_shorten_bfs")

_hip.register({
    "rc_shorten_struct_bytes": [],
    "rc_shorten_workspace_bytes": [c_size_t, c_size_t],
    "rc_shorten_index": [POINTER(_ShortenStruct), c_void_p],
    "rc_shorten_neighbours": [POINTER(_ShortenStruct), c_void_p],
    "rc_shorten_bfs": [POINTER(_ShortenStruct), c_void_p],
    "rc_shorten": [POINTER(_ShortenStruct), c_void_p],
}, {"rc_shorten_struct_bytes": c_size_t, "rc_shorten_workspace_bytes": c_size_t})


# ---- planning (pure) ---------------------------------------------------------------------------------------------------------
def table_cells(lengths) -> np.ndarray:
    """Hash cells of games of `lengths` moves: the power of two >= 2 (L + 1); 0 for a game that is left alone (L < 0)."""
    L = np.asarray(lengths, dtype=np.int64)
    need = 2 * (np.maximum(L, 0) + 1)
    cells = np.left_shift(np.int64(1), np.ceil(np.log2(need)).astype(np.int64))
    cells = np.where(cells < need, cells * 2, cells)   # (log2 of an exact power may round either way)
    return np.where(L < 0, 0, cells).astype(np.int64)


def workspace_bytes(total_positions: int, total_hash_cells: int) -> int:
    """rc_shorten_workspace_bytes: keys 16 B, ids 4 B, neighbours 48 B, claim and parent 8 B and two frontiers of 4 B per position,
    4 B per hash cell (2 .. 4 cells per position), every array rounded up to 256 B: 92 .. 100 B per position."""
    r = lambda x: (int(x) + 255) // 256 * 256   # noqa: E731
    P, H = int(total_positions), int(total_hash_cells)
    return r(16 * P) + r(4 * P) + r(48 * P) + r(8 * P) + 2 * r(4 * P) + r(4 * H)


def plan_chunks(lengths, budget_bytes: int = DEFAULT_BUDGET_BYTES) -> list:
    """
    Game ranges [(lo, hi), ...] that cover range(len(lengths)) in order, each as long as the workspace of its games fits
    `budget_bytes` (`workspace_bytes` of its positions and cells).  lengths[g] < 0: game g is left alone and costs nothing.
    A game that alone exceeds the budget raises ValueError.
    """
    L = np.asarray(lengths, dtype=np.int64)
    pos, cells = np.where(L < 0, 0, L + 1), table_cells(L)
    chunks, lo, P, H = [], 0, 0, 0
    for g in range(len(L)):
        p, h = int(pos[g]), int(cells[g])
        if workspace_bytes(p, h) > budget_bytes:
            raise ValueError(f"game {g}: a queue of {int(L[g])} moves needs {workspace_bytes(p, h)} bytes of workspace, the budget is {budget_bytes}")
        if g > lo and workspace_bytes(P + p, H + h) > budget_bytes:
            chunks.append((lo, g))
            lo, P, H = g, 0, 0
        P, H = P + p, H + h
    if len(L) > lo:
        chunks.append((lo, len(L)))
    return chunks


# ---- one chunk on the device ---------------------------------------------------------------------------------------------------
class ShortenBatch:
    """The device arrays of one chunk and the rc_shorten_t that names them (tests fill one by hand to look at every array)."""

    def __init__(self, roots: DeviceCubes, queues: np.ndarray, lens: np.ndarray, select: np.ndarray, out_width: int = None, device=None):
        self.lib = _hip.lib()
        dev = device or roots.soa.device
        G = roots.n
        queues = np.ascontiguousarray(queues, dtype=np.uint8)
        queues = queues.reshape(G, -1) if queues.size else np.zeros((G, 1), dtype=np.uint8)   # (empty queues only: a row of one byte)
        lens, select = np.asarray(lens, dtype=np.int32), np.asarray(select).astype(np.uint8)
        assert G >= 1 and lens.shape == (G,) and select.shape == (G,)
        chosen = select != 0
        max_len = int(lens[chosen].max()) if chosen.any() else 0
        if max_len > min(MAX_LEN, queues.shape[1]) or (chosen.any() and int(lens[chosen].min()) < 0):
            raise ValueError(f"queue lengths {int(lens[chosen].min())} .. {max_len}: they lie in 0 .. min({MAX_LEN}, row width {queues.shape[1]})")
        eff = np.where(chosen, lens.astype(np.int64), -1)
        self.pos_off_h = np.concatenate([[0], np.cumsum(np.where(eff < 0, 0, eff + 1))]).astype(np.uint64)
        self.hash_off_h = np.concatenate([[0], np.cumsum(table_cells(eff))]).astype(np.uint64)
        P, H = max(1, int(self.pos_off_h[-1])), max(2, int(self.hash_off_h[-1]))
        self.G, self.P, self.H, self.max_len = G, P, H, max_len
        self.bytes = workspace_bytes(P, H)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)     # noqa: E731
        self.roots = roots
        self.queues, self.lens, self.select = up(queues), up(lens), up(select)
        self.pos_off, self.hash_off = up(self.pos_off_h.view(np.int64)), up(self.hash_off_h.view(np.int64))
        self.keys, self.ids, self.nbr, self.claim = z((P, 4), torch.int32), z((P,), torch.int32), z((P, 12), torch.int32), z((P, 2), torch.int32)
        self.frontier_a, self.frontier_b, self.hash = z((P,), torch.int32), z((P,), torch.int32), z((H,), torch.int32)
        W = max(1, max_len if out_width is None else int(out_width))
        self.out_queues, self.out_lens, self.status = z((G, W), torch.uint8), z((G,), torch.int32), z((G,), torch.int32)
        s = _ShortenStruct()
        s.n_games, s.queue_width, s.out_width, s.max_len = G, queues.shape[1], W, max_len
        s.stride, s.total_positions, s.total_hash_cells = roots.stride, P, H
        s.roots_soa = roots.soa.data_ptr()
        for name in POINTER_FIELDS[1:]:
            setattr(s, name, getattr(self, name).data_ptr())
        self.struct = s

    def step(self, name: str):
        _hip.check(getattr(self.lib, name)(ctypes.byref(self.struct), _hip.stream_ptr()), name)

    def run(self, timings: dict = None):
        """The three steps; with `timings`, each between two events: timings[step] gets a list of (start, end) event pairs."""
        if timings is None:
            return self.step("rc_shorten")
        for name in STEPS:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.step(name)
            b.record()
            timings.setdefault(name, []).append((a, b))


def _as_table(queues, lengths, n: int):
    if isinstance(queues, QueueTable):
        return queues
    if isinstance(queues, np.ndarray) and queues.ndim == 2:
        if lengths is None:
            raise ValueError("a padded array of queues needs `lengths`")
        return QueueTable(np.ascontiguousarray(queues, dtype=np.uint8), np.asarray(lengths, dtype=np.int64))
    return QueueTable.from_queues([list(q) for q in queues])


def _window(cubes: DeviceCubes, lo: int, hi: int) -> DeviceCubes:
    if lo == 0 and hi == cubes.n:
        return cubes
    soa = torch.zeros((cubes.soa.shape[0], _stride_for(hi - lo)), dtype=torch.int8, device=cubes.soa.device)
    soa[:, :hi - lo] = cubes.soa[:, lo:hi]
    return DeviceCubes(soa, hi - lo)


def shorten_queues(states, queues, lengths=None, select=None, budget_bytes: int = None, timings: dict = None, info: dict = None):
    """
    -> (QueueTable, status int32 [n]).  states: (n, 20) int8 or DeviceCubes, the games' roots; queues: a QueueTable, a padded uint8
    array [n, width] with `lengths`, or a list of action sequences; select: bool [n], the games to shorten (default: all).
    Row g of the result is the shortened queue where status[g] == OK and game g's queue as it came everywhere else (SKIPPED: not
    selected; BAD_ACTION: a byte >= 12 inside its length; FAILED / NO_ROOM do not happen with the arrays this function makes).
    The games are cut into chunks whose workspace fits `budget_bytes` (`plan_chunks`); the result does not depend on the cut.
    timings: a dict that receives, per launch, the HIP event pairs of every chunk; info: receives workspace bytes and chunks.
    """
    roots = DeviceCubes.of(states)
    n = roots.n
    table = _as_table(queues, lengths, n)
    if len(table) != n:
        raise ValueError(f"{n} states, {len(table)} queues")
    lens = table.lengths().astype(np.int64)
    chosen = np.ones(n, dtype=bool) if select is None else np.asarray(select).astype(bool)
    chunks = plan_chunks(np.where(chosen, lens, -1), DEFAULT_BUDGET_BYTES if budget_bytes is None else int(budget_bytes))
    out, status = QueueTable(n=n), np.full(n, SKIPPED, dtype=np.int32)
    for g in range(n):
        out.put(g, table, g)
    peak = 0
    for lo, hi in chunks:
        if not chosen[lo:hi].any():
            continue
        games = np.arange(lo, hi)
        acts, ls = table.padded(games, fill=0)
        batch = ShortenBatch(_window(roots, lo, hi), acts, ls, chosen[lo:hi])
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
