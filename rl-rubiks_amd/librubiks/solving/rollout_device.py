"""
Device-resident batch of one-step games and the round that drives the rc_rollout_* kernels (csrc/rubiks_rollout.hip).

S slots hold one game each of RandomSearch, PolicySearch (greedy or sampled) or ValueSearch.  A round is K x (engine forward,
step kernel): for the policy kinds the forward runs on the S current states, for the value kind on their 12 S children, which the
step kernel itself writes; the random kind has no forward.  Nothing in a round synchronises with the host, and it is replayable
as one captured graph (finished and empty slots idle on the identity action).  The host's part is the random numbers, which do
not depend on the device: one [K][S16] table per round -- action bytes for the random kind, uniforms for the sampled kind --
drawn per game from the game's own np.random stream (rc_rollout_draw), so that step t of a game always uses draw t of its
stream, and uploaded once from pinned memory.
"""
import ctypes
from ctypes import POINTER, Structure, c_int, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import torch

from librubiks import _hip
from librubiks.cube.device import DeviceCubes, _stride_for
from librubiks.solving.lockstep_device import (EXHAUSTED, N_ACT, QUEUE_FULL, ROOT_SOLVED, RUNNING, SOLVED,  # noqa: F401  (also this module's names)
                                               GameStreams, LockstepBatch)

BAD_POLICY = 5        # a slot's status beyond the shared ones: a NaN among the sampled policy's probabilities
POLICY = 255          # decision byte: ask the network; 0 .. 11: that action
KINDS = ("random", "greedy", "sampled", "value")
DRAW_BYTES, DRAW_UNIFORMS = 0, 1   # rc_rollout_draw's modes


class _RoStruct(Structure):   # mirrors rc_rollout_t (include/rubiks_hip.h)
    _fields_ = [("n_slots", c_uint32), ("queue_width", c_uint32), ("stride", c_size_t)] + \
               [(name, c_void_p) for name in ("states_soa", "kids_soa", "kid_solved", "queues", "status", "steps")]


_hip.register({
    "rc_rollout_struct_bytes": [],
    "rc_rollout_plant": [POINTER(_RoStruct), c_void_p, c_uint32, c_void_p, c_size_t, c_size_t, c_int, c_void_p],
    "rc_rollout_step_policy": [POINTER(_RoStruct), c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_uint64, c_void_p],
    "rc_rollout_step_value": [POINTER(_RoStruct), c_void_p, c_uint64, c_void_p],
    "rc_rollout_draw": [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_int, c_uint32, c_void_p, c_size_t],
}, {"rc_rollout_struct_bytes": c_size_t})


start = GameStreams.start   # start(streams, games): the older name of `streams.start(games)`


def draw(streams: GameStreams, games, slots, table: np.ndarray):
    """The next table.shape[0] draws of `games` (playing in `slots`) into the columns `slots` of table: a uint8 [K, stride] host
    array gets actions as RandomState.randint(12) draws them, a float64 one uniforms as random_sample does; the streams advance
    as NumPy's would."""
    games, slots = np.ascontiguousarray(games, dtype=np.int32), np.ascontiguousarray(slots, dtype=np.int32)
    assert table.ndim == 2 and table.dtype in (np.uint8, np.float64) and table.strides == (table.shape[1] * table.itemsize, table.itemsize)
    mode = DRAW_BYTES if table.dtype == np.uint8 else DRAW_UNIFORMS
    _hip.check(_hip.load().rc_rollout_draw(streams.keys.ctypes.data, streams.pos.ctypes.data, len(streams.seeds), games.ctypes.data,
                                           slots.ctypes.data, len(games), mode, table.shape[0], table.ctypes.data, table.shape[1]),
               "rc_rollout_draw")


class RolloutBatch(LockstepBatch):
    TABLE_DTYPE = {"random": torch.uint8, "sampled": torch.float64}   # what the host draws per game and step, by kind

    def __init__(self, n_slots: int, kind: str, steps_per_round: int = 8, queue_width: int = 64, device=None, use_graph: bool = True):
        self.lib = _hip.lib()
        dev = device or torch.device("cuda", torch.cuda.current_device())
        S, K = int(n_slots), int(steps_per_round)
        if kind not in KINDS or not (0 < S <= 1 << 26 and K > 0):
            raise ValueError(f"rollout batch: kind {kind!r} (one of {KINDS}), {S} slots, {K} steps per round")
        self.S, self.K, self.kind, self.device, self.use_graph = S, K, kind, dev, bool(use_graph)
        self.S16 = (S + 15) // 16 * 16
        stride = _stride_for(S)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        self.states = DeviceCubes(z((20, stride), torch.int8), S)
        self.words = z((2, S), torch.int64)                         # status, steps: what the host reads per round
        self.words[0] = EXHAUSTED                                   # nothing planted yet: no slot is played
        self.status, self.steps = self.words
        s = _RoStruct()
        s.n_slots, s.stride, s.states_soa = S, stride, self.states.soa.data_ptr()
        s.status, s.steps = self.status.data_ptr(), self.steps.data_ptr()
        if kind == "value":   # the network reads the children, which the step kernel leaves behind for it
            self.rows = DeviceCubes(z((20, 12 * stride), torch.int8), 12 * S)
            self.kid_solved = z((12 * stride,), torch.uint8)
            self.values = z((12 * S,), torch.float32)
            s.kids_soa, s.kid_solved = self.rows.soa.data_ptr(), self.kid_solved.data_ptr()
        else:
            self.rows = self.states
        self.R = self.rows.n
        dt = self.TABLE_DTYPE.get(kind)
        self.table = None if dt is None else z((K, self.S16), dt)   # this round's draws (static: graphs)
        self._host_tables = None
        self.struct = s
        self._set_queues(z((S, max(1, int(queue_width))), torch.uint8))
        self.engine, self._net_fp = None, None
        self._graphs, self._graph_pool = {}, None

    def host_tables(self) -> list:
        """Two pinned host tables for `round`, one to draw into while the other's round runs (None for the kinds that draw
        nothing); they belong to the batch, so a search that reuses it allocates none."""
        if self.table is not None and self._host_tables is None:
            self._host_tables = [torch.zeros(self.table.shape, dtype=self.table.dtype).pin_memory() for _ in range(2)]
        return self._host_tables or [None, None]

    # ---- search phases ---------------------------------------------------------------------------
    def plant(self, slots: torch.Tensor, roots: DeviceCubes, first: int):
        """Slots `slots` (int32 device tensor) restart from roots[first], roots[first + 1], ...; the others are not touched."""
        assert slots.dtype == torch.int32 and slots.is_cuda and slots.is_contiguous() and first + slots.numel() <= roots.n
        _hip.check(self.lib.rc_rollout_plant(ctypes.byref(self.struct), slots.data_ptr(), int(slots.numel()), roots.soa.data_ptr(),
                                             roots.stride, int(first), int(self.kind == "value"), _hip.stream_ptr()), "rc_rollout_plant")

    def _round(self, max_steps: int):
        r, st, lib = ctypes.byref(self.struct), _hip.stream_ptr(), self.lib
        for i in range(self.K):
            if self.kind == "value":
                self.values.copy_(self._head()[:, N_ACT])
                _hip.check(lib.rc_rollout_step_value(r, self.values.data_ptr(), int(max_steps), st), "rc_rollout_step_value")
                continue
            row = None if self.table is None else self.table.data_ptr() + i * self.table.stride(0) * self.table.element_size()
            if self.kind == "random":
                args = (None, 0, 0, row, None)
            else:
                head = self._head()
                args = (head.data_ptr(), head.stride(0), int(head.dtype == torch.bfloat16), None, row)
            _hip.check(lib.rc_rollout_step_policy(r, *args, int(max_steps), st), "rc_rollout_step_policy")

    def round(self, table: torch.Tensor, max_steps: int):
        """Queues K moves of every running game: `table` (one of `host_tables`, filled by `draw`) holds this round's draws.
        Nothing synchronises, except that the first round of a limit runs eagerly and is then captured; later rounds replay
        the graph."""
        assert (self.engine is None) == (self.kind == "random")
        if self.table is not None:
            assert table.dtype == self.table.dtype and table.shape == self.table.shape
            self.table.copy_(table, non_blocking=True)
        self._run(int(max_steps))

    # ---- what the host's round loop asks (agents.lockstep_search) ----------------------------------
    unit = property(lambda self: self.K)   # the host counts a game's moves: K per round
    queue_len_row = 1             # the row of `words` that holds the queue length (`steps`)
    time_limit_exhausts = True    # a game the pool's time limit stops ends EXHAUSTED
    draw_round = staticmethod(draw)

    def width_after(self, played: int, cap: int) -> int:
        """Queue bytes that one more round can need after `played` moves (a search bounded by time only)."""
        return min(cap, played + self.K)

    def check_status(self, status: np.ndarray, owner: np.ndarray, played: np.ndarray, agent):
        if (status == QUEUE_FULL).any():
            raise _hip.RubiksHipError(f"{agent}: the queue row of slot {int(np.argmax(status == QUEUE_FULL))} is full ({self.Q} bytes)")
        if (status == BAD_POLICY).any():       # where np.random.choice raises (reference agents.py:140)
            raise ValueError(f"{agent}: probabilities contain NaN (game {int(owner[np.argmax(status == BAD_POLICY)])})")
