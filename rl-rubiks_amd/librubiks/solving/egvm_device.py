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
from librubiks.cube.device import DeviceCubes
from librubiks.solving.lockstep_device import (EXHAUSTED, N_ACT, QUEUE_FULL, ROOT_SOLVED, RUNNING, SOLVED,  # noqa: F401  (also this module's names)
                                               GameStreams, LockstepBatch, game_seeds)

POLICY = 255          # decision byte: take the policy's argmax; 0 .. 11: that action
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


def queue_rounds(max_states: int, workers: int, depth: int) -> int:
    """Rounds a game can complete under max_states (agents.py:665): its queue row holds that many path prefixes of <= D actions."""
    return int(max_states) // (workers * depth)


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

    # ---- what the host's round loop asks (agents.lockstep_search) ----------------------------------
    unit = 1                      # the host counts a game's rounds
    queue_len_row = 2             # the row of `words` that holds the queue length
    time_limit_exhausts = False   # a game the pool's time limit stops keeps status RUNNING (deliberate by history, unlike RolloutBatch)

    def set_epsilon(self, epsilon: float):
        self.cdf0 = choice_cdf(epsilon)

    def host_tables(self) -> list:
        """Two pinned host tables for `round`, one to draw into while the other's round runs: new ones per search, so that the
        columns of slots nobody draws for say POLICY."""
        return [torch.full((self.D, self.R16), POLICY, dtype=torch.uint8).pin_memory() for _ in range(2)]

    def draw_round(self, streams: GameStreams, games, slots, table: np.ndarray):
        streams.draw(games, slots, self.cdf0, self.W, self.D, table, self.R)

    def width_after(self, played: int, cap: int) -> int:
        """Queue bytes that one more round can need after `played` rounds (a search bounded by time only)."""
        return self.D * (played + 1)

    def check_status(self, status: np.ndarray, owner: np.ndarray, played: np.ndarray, agent):
        if (status == QUEUE_FULL).any():
            raise _hip.RubiksHipError(f"EGVM: the queue row of slot {int(np.argmax(status == QUEUE_FULL))} is full "
                                      f"({self.Q} bytes, {int(played.max())} rounds)")
