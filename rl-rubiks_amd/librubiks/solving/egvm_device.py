"""
Device-resident batch of EGVM games and the round that drives the rc_egvm_* kernels (csrc/rubiks_egvm.hip).

S slots hold one game each; a game's W workers are rows g W + w of one cube batch, which is the network's input.  A round is
D x (engine forward on all S W rows, rc_egvm_step), one more forward for the values of the last depth and rc_egvm_round_end:
no host synchronisation in it, and replayable as one captured graph (the row count never changes: finished and empty slots idle
on the identity action).  The host's part is the random decisions, which do not depend on the device: one uint8 [D][rows] table
per round, drawn per game from the game's own np.random stream in the reference's call order (librubiks/solving/agents.py:694-698
of the reference) and uploaded once from pinned memory.

Per row and step ~100 B (52 B of head, 2 x 20 B of state, the path byte, the running best) beside the network's 24.9 MFLOP.
"""
import ctypes
from ctypes import POINTER, Structure, c_double, c_int, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import torch

from librubiks import _hip
from librubiks.cube.device import DeviceCubes, encode
from librubiks.model import SplitF32Net, _CubeWindow, make_inference_net, net_fingerprint
from librubiks.solving.astar_device import NET_CHUNK

RUNNING, SOLVED, EXHAUSTED, QUEUE_FULL, ROOT_SOLVED = 0, 1, 2, 3, 4
POLICY = 255          # decision byte: take the policy's argmax; 0 .. 11: that action
N_ACT = 12
MAX_WORKERS, MAX_DEPTH = 0xffff, 0x8000


class _EgStruct(Structure):   # mirrors rc_egvm_t (include/rubiks_hip.h)
    _fields_ = [("n_slots", c_uint32), ("workers", c_uint32), ("depth", c_uint32), ("queue_width", c_uint32), ("stride", c_size_t)] + \
               [(name, c_void_p) for name in ("rows_soa", "best_soa", "best_value", "best_depth", "paths", "hit", "current", "queues",
                                              "status", "nodes", "queue_len", "rounds")]


_hip.register({
    "rc_egvm_step": [POINTER(_EgStruct), c_uint32, c_void_p, c_void_p, c_size_t, c_int, c_void_p],
    "rc_egvm_round_end": [POINTER(_EgStruct), c_void_p, c_uint64, c_void_p],
    "rc_egvm_plant": [POINTER(_EgStruct), c_void_p, c_uint32, c_void_p, c_size_t, c_size_t, c_void_p],
    "rc_egvm_draw": [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_double, c_uint32, c_uint32, c_void_p, c_size_t, c_size_t],
})


# ---- the host's draws ------------------------------------------------------------------------------------------------------
def choice_cdf(epsilon: float) -> float:
    """The threshold `RandomState.choice(2, n, p=[1 - epsilon, epsilon])` compares its uniforms with: it normalises the
    cumulative sum of p and looks every uniform up in it (`searchsorted(..., side="right")`), so the draw is 1 iff u >= cdf[0]
    (what rc_egvm_draw is given)."""
    cdf = np.array([1 - epsilon, epsilon], dtype=np.float64).cumsum()
    cdf /= cdf[-1]
    return float(cdf[0])


class GameStreams:
    """
    The games' np.random streams as the library's host generator runs them (rc_egvm_draw): game g's MT19937 state is that of
    np.random.RandomState(seeds[g]) from `start(g)` on, and `draw` advances it exactly as the reference's calls advance the
    RandomState (per depth step `choice(2, W, p=[1 - eps, eps])`, then `randint(0, 12, k)`, agents.py:694-698) -- the same
    table, the same state afterwards (tests/test_egvm_streams.py) -- at a few nanoseconds per 32-bit output instead of two
    NumPy calls per depth step and game.
    """

    def __init__(self, seeds: np.ndarray):
        self.seeds = np.asarray(seeds, dtype=np.int64)
        self.keys = np.zeros((len(self.seeds), 624), dtype=np.uint32)
        self.pos = np.full(len(self.seeds), 624, dtype=np.int32)

    def start(self, games):
        for g in np.atleast_1d(games):
            _, key, pos = np.random.RandomState(int(self.seeds[g])).get_state()[:3]
            self.keys[g], self.pos[g] = key, pos

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


def queue_rounds(max_states: int, workers: int, depth: int) -> int:
    """Rounds a game can complete under max_states (agents.py:665): its queue row holds that many path prefixes of <= D actions."""
    return int(max_states) // (workers * depth)


class LockstepBatch:
    """What the device batches of the lock-step agents share (EGVMBatch, rollout_device.RolloutBatch): the engine for `net` and the
    head (12 logits + value) of every row of `self.rows` (a DeviceCubes of `self.R` rows on `self.device`), the captured rounds, the
    queue rows (`self.queues` [S, Q], named by `self.struct`) and the block of words the host reads per round (`self.words`)."""

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
        host = torch.empty(self.words.shape, dtype=torch.int64, pin_memory=True)
        host.copy_(self.words, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev

    def take_queues(self, slots: np.ndarray, width: int):
        """Queue rows of `slots`, their first `width` bytes, on their way into pinned memory: (host tensor, event, keep-alive)."""
        idx = torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).pin_memory().to(self.device, non_blocking=True)
        rows = self.queues[idx, :max(1, int(width))]
        host = torch.empty(rows.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(rows, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev, (idx, rows)


class EGVMBatch(LockstepBatch):
    def __init__(self, n_slots: int, workers: int, depth: int, queue_width: int, device=None, use_graph: bool = True):
        self.lib = _hip.lib()
        dev = device or torch.device("cuda", torch.cuda.current_device())
        S, W, D = int(n_slots), int(workers), int(depth)
        if not (S > 0 and 0 < W <= MAX_WORKERS and 0 < D <= MAX_DEPTH and S * W <= 1 << 30):
            raise ValueError(f"EGVM batch: {S} slots, {W} workers (1 .. {MAX_WORKERS}), depth {D} (1 .. {MAX_DEPTH})")
        self.S, self.W, self.D, self.device, self.use_graph = S, W, D, dev, bool(use_graph)
        self.R = S * W
        self.R16 = (self.R + 15) // 16 * 16
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        self.rows = DeviceCubes.empty(self.R, dev)                  # the workers' current states = network input
        self.best = DeviceCubes.empty(self.R, dev)
        self.best_value = z((self.R,), torch.float32)
        self.best_depth = torch.full((self.R,), -1, dtype=torch.int32, device=dev)
        self.paths = z((S, W, D), torch.uint8)
        self.hit = torch.full((S,), -1, dtype=torch.int32, device=dev)      # RC_EGVM_NO_HIT
        self.current = z((S, 20), torch.int8)
        self.words = z((4, S), torch.int64)                         # status, nodes, queue_len, rounds: what the host reads per round
        self.words[0] = EXHAUSTED                                   # nothing planted yet: no slot is played
        self.status, self.nodes, self.queue_len, self.rounds = self.words
        self.queues = z((S, max(1, int(queue_width))), torch.uint8)
        self.decisions = torch.full((D, self.R16), POLICY, dtype=torch.uint8, device=dev)   # this round's table (static: graphs)
        self.values_last = z((self.R,), torch.float32)
        s = _EgStruct()
        s.n_slots, s.workers, s.depth, s.stride = S, W, D, self.rows.stride
        for name, src in (("rows_soa", self.rows.soa), ("best_soa", self.best.soa)):
            setattr(s, name, src.data_ptr())
        for name in ("best_value", "best_depth", "paths", "hit", "current", "status", "nodes", "queue_len", "rounds"):
            setattr(s, name, getattr(self, name).data_ptr())
        self.struct = s
        self._set_queues(self.queues)
        self.engine, self._net_fp = None, None
        self._graphs, self._graph_pool = {}, None

    # ---- search phases ---------------------------------------------------------------------------
    def reset(self, roots: DeviceCubes):
        """Slot s starts from roots[s] (roots may hold more scrambles: the rest wait for `plant`)."""
        assert roots.n >= self.S and self.engine is not None
        self.plant(torch.arange(self.S, dtype=torch.int32, device=self.device), roots, 0)

    def plant(self, slots: torch.Tensor, roots: DeviceCubes, first: int):
        """Slots `slots` (int32 device tensor) restart from roots[first], roots[first + 1], ...; the others are not touched."""
        assert slots.dtype == torch.int32 and slots.is_cuda and slots.is_contiguous() and first + slots.numel() <= roots.n
        _hip.check(self.lib.rc_egvm_plant(ctypes.byref(self.struct), slots.data_ptr(), int(slots.numel()), roots.soa.data_ptr(),
                                          roots.stride, int(first), _hip.stream_ptr()), "rc_egvm_plant")

    def _round(self, max_states: int):
        e, st, lib = ctypes.byref(self.struct), _hip.stream_ptr(), self.lib
        for d in range(self.D):
            head = self._head()
            _hip.check(lib.rc_egvm_step(e, d, self.decisions.data_ptr() + d * self.R16, head.data_ptr(), head.stride(0),
                                        int(head.dtype == torch.bfloat16), st), "rc_egvm_step")
        # the states after the last depth have no next step whose forward would bring their value: one more pass.  It is the
        # merged head's value column again, so that all D values of a worker come out of one function with one rounding.
        self.values_last.copy_(self._head()[:, N_ACT])
        _hip.check(lib.rc_egvm_round_end(e, self.values_last.data_ptr(), int(max_states), st), "rc_egvm_round_end")

    def round(self, decisions: torch.Tensor, max_states: int):
        """Queues one round of every running game: `decisions` (uint8 [D, R16] host tensor, pinned for an upload that does not
        wait) is this round's table.  Nothing synchronises, except that the first round of a shape runs eagerly and is then
        captured (the capture records launches, it does not advance the search); later rounds replay the graph."""
        assert decisions.dtype == torch.uint8 and tuple(decisions.shape) == (self.D, self.R16) and self.engine is not None
        self.decisions.copy_(decisions, non_blocking=True)
        self._run(int(max_states))
