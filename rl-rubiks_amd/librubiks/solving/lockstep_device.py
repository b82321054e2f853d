"""What the device batches of the lock-step agents share (EGVMBatch, RolloutBatch; BFSBatch for the two pinned copies): the head of
every row, the captured rounds, the queue rows, the words the host reads per round, and the games' seeds and np.random streams."""
from ctypes import c_uint32, c_void_p

import numpy as np
import torch

from librubiks import _hip
from librubiks.cube.device import encode
from librubiks.model import SplitF32Net, _CubeWindow, make_inference_net, net_fingerprint
from librubiks.solving.astar_device import NET_CHUNK

N_ACT = 12
RUNNING, SOLVED, EXHAUSTED, QUEUE_FULL, ROOT_SOLVED = 0, 1, 2, 3, 4   # a slot's status, the same numbers in both families' kernels

_hip.register({"rc_rollout_seed": [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p]})


# ---- the host's draws ------------------------------------------------------------------------------------------------------
class GameStreams:
    """
    The games' np.random streams as the library's host generator runs them (rc_egvm_draw, rc_rollout_draw): game g's MT19937
    state is that of np.random.RandomState(seeds[g]) from `start(g)` on, and `draw` advances it exactly as the reference's calls
    advance the RandomState (per depth step `choice(2, W, p=[1 - eps, eps])`, then `randint(0, 12, k)`, agents.py:694-698) -- the
    same table, the same state afterwards (tests/test_egvm_streams.py) -- at a few nanoseconds per 32-bit output instead of two
    NumPy calls per depth step and game.
    """

    def __init__(self, seeds: np.ndarray):
        self.seeds = np.asarray(seeds, dtype=np.int64)
        self.keys = np.zeros((len(self.seeds), 624), dtype=np.uint32)
        self.pos = np.full(len(self.seeds), 624, dtype=np.int32)

    def start(self, games):
        """The listed games' generators as np.random.RandomState(seed) starts them, seeded in the library (rc_rollout_seed,
        tests/test_rollout_draw.py: a NumPy object per game costs 20 us, which a batch of short games notices)."""
        games = np.ascontiguousarray(games, dtype=np.int32)
        _hip.check(_hip.load().rc_rollout_seed(self.keys.ctypes.data, self.pos.ctypes.data, len(self.seeds), games.ctypes.data,
                                               len(games), self.seeds.ctypes.data), "rc_rollout_seed")

    def state(self, g: int) -> tuple:
        """Game g's stream as `RandomState.set_state` takes it."""
        return ("MT19937", self.keys[g].copy(), int(self.pos[g]), 0, 0.0)

    def draw(self, games, slots, cdf0: float, workers: int, depth: int, table: np.ndarray, n_rows: int):
        """The next round of `games` (playing in `slots`) into table (uint8 [depth, stride] host array, rows slot W + w)."""
        games, slots = np.ascontiguousarray(games, dtype=np.int32), np.ascontiguousarray(slots, dtype=np.int32)
        assert table.dtype == np.uint8 and table.ndim == 2 and table.shape[0] == depth and table.strides == (table.shape[1], 1)
        _hip.check(_hip.load().rc_egvm_draw(self.keys.ctypes.data, self.pos.ctypes.data, len(self.seeds), games.ctypes.data,
                                            slots.ctypes.data, len(games), float(cdf0), int(workers), int(depth), table.ctypes.data,
                                            table.shape[1], int(n_rows)), "rc_egvm_draw")


def game_seeds(seeds, n_games: int) -> np.ndarray:
    """The per-game seeds of a batched search: an integer array [G] as it is, one integer s as
    RandomState(s).randint(0, 2**31 - 1, size=G), None as one such call on the global stream."""
    if seeds is None:
        return np.random.randint(0, 2 ** 31 - 1, size=n_games).astype(np.int64)
    if np.ndim(seeds) == 0:
        return np.random.RandomState(int(seeds)).randint(0, 2 ** 31 - 1, size=n_games).astype(np.int64)
    seeds = np.asarray(seeds)
    if seeds.shape != (n_games,) or not np.issubdtype(seeds.dtype, np.integer):
        raise ValueError(f"seeds: one integer or an integer array of shape ({n_games},), got {seeds.dtype} {seeds.shape}")
    return seeds.astype(np.int64)


# ---- what the host reads of a batch ----------------------------------------------------------------------------------------
def pinned_copy(src: torch.Tensor):
    """(pinned host copy of `src` on its way, event recorded behind it on the current stream)."""
    host = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
    host.copy_(src, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return host, ev


def take_queue_rows(queues: torch.Tensor, slots: np.ndarray, width: int):
    """Rows `slots` of `queues` (uint8 [S, Q] on the device), their first `width` bytes, on their way into pinned memory:
    (host tensor, event, keep-alive)."""
    idx = torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).pin_memory().to(queues.device, non_blocking=True)
    rows = queues[idx, :max(1, int(width))]
    return pinned_copy(rows) + ((idx, rows),)


class LockstepBatch:
    """What EGVMBatch and RolloutBatch share: the engine for `net` and the head (12 logits + value) of every row of `self.rows` (a
    DeviceCubes of `self.R` rows on `self.device`), the captured rounds, the queue rows (`self.queues` [S, Q], named by
    `self.struct`) and the block of words the host reads per round (`self.words`).  Beside `reset`, `plant` and `round`, a subclass
    tells the host's round loop (agents.lockstep_search) what differs between the families: `unit`, `queue_len_row`,
    `time_limit_exhausts`, `host_tables`, `draw_round`, `width_after` and `check_status`."""

    def set_net(self, net, dtype=torch.bfloat16):
        """Builds the inference engine for `net`; a no-op when the batch already runs exactly these weights."""
        fp = net_fingerprint(net, dtype)
        if self.engine is not None and fp == self._net_fp:
            return
        self._net_fp = fp
        self.engine = make_inference_net(net, dtype)
        self._fused = bool(getattr(self.engine, "supports_cubes", False))
        rows = min(NET_CHUNK, self.R)
        self._x1 = self.engine.workspace(rows) if self._fused else None
        self._oh = None if self._fused else torch.empty((rows, getattr(self.engine, "input_width", 480)), dtype=self.engine.input_dtype, device=self.device)
        # the head of all rows where it does not come out of the engine as one tensor (several chunks, or logits and values apart)
        self._head_buf = None if self._fused and self.R <= NET_CHUNK else torch.zeros((self.R, 16), dtype=torch.float32, device=self.device)
        self._graphs, self._graph_pool = {}, None

    def _head_of(self, lo: int, n: int) -> torch.Tensor:
        """Engine output for rows lo .. lo + n (lo % 16 == 0): [n, >= 13], 12 logits then the value, float32 or bf16."""
        eng, rows = self.engine, self.rows
        if self._fused:
            x1 = None if self._x1 is None else self._x1[:n]
            if lo == 0 and n == rows.n:
                return eng.head_cubes(rows, x1)
            if isinstance(eng, SplitF32Net):
                return eng._forward_cubes(rows, eng.layers, lo, n)
            return eng.head_cubes(_CubeWindow(rows.soa.data_ptr() + lo, n, rows.stride), x1)
        logits, values = eng(encode(eng, rows, self._oh[:n], lo, n))
        out = self._head_buf[lo:lo + n]
        out[:, :N_ACT].copy_(logits)
        out[:, N_ACT].copy_(values)
        return out

    def _head(self) -> torch.Tensor:
        """12 logits + value of every row's current state, chunked as the A* batch chunks its value passes."""
        if self._fused and self.R <= NET_CHUNK:
            return self._head_of(0, self.R)
        for lo in range(0, self.R, NET_CHUNK):
            n = min(NET_CHUNK, self.R - lo)
            out = self._head_of(lo, n)
            if self._fused:
                self._head_buf[lo:lo + n, :N_ACT + 1].copy_(out[:, :N_ACT + 1])
        return self._head_buf

    def reset(self, roots):
        """Slot s starts from roots[s] (roots may hold more scrambles: the rest wait for `plant`)."""
        assert roots.n >= self.S
        self.plant(torch.arange(self.S, dtype=torch.int32, device=self.device), roots, 0)

    @property
    def Q(self) -> int:
        return self.queues.shape[1]

    def _set_queues(self, queues: torch.Tensor):
        self.queues = queues
        self.struct.queues, self.struct.queue_width = queues.data_ptr(), queues.shape[1]
        self._graphs = {}   # (the captured rounds hold the old row address and width)

    def grow_queues(self, width: int):
        """Queue rows of at least `width` bytes (doubling): between two rounds, contents kept."""
        if width <= self.Q:
            return
        wider = torch.zeros((self.S, max(int(width), 2 * self.Q)), dtype=torch.uint8, device=self.device)
        wider[:, :self.Q] = self.queues
        self._set_queues(wider)

    def _run(self, limit: int):
        """`self._round(limit)`: launched as it is, or -- `use_graph` -- as the replay of its captured graph; the first round of a
        limit runs eagerly and is then captured (the capture records launches, it does not advance the search)."""
        if not self.use_graph:
            return self._round(limit)
        g = self._graphs.get(limit)
        if g is not None:
            return g.replay()
        self._round(limit)
        torch.cuda.synchronize()
        if self._graph_pool is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._graph_pool):
            self._round(limit)
        self._graphs[limit] = g

    def snapshot(self):
        """(pinned int64 copy of `words` (per slot: status and the counters), event): the one block the host reads per round."""
        return pinned_copy(self.words)

    def take_queues(self, slots: np.ndarray, width: int):
        """Queue rows of `slots`, their first `width` bytes, on their way into pinned memory: (host tensor, event, keep-alive)."""
        return take_queue_rows(self.queues, slots, width)
