"""
Generalised move patterns in solutions (librubiks/analysis/pattern_mining.py of the reference), mined on the device
(csrc/rubiks_patterns.hip, rc_patterns_* in include/rubiks_hip.h).  A pattern is a contiguous sub-sequence of a solution, of two
moves or more, with its faces renamed in order of first appearance -- `R T r` and `F L f` are both `ABa` --, counted once per
solution that holds it; the result is the reference's dict {pattern: share of the solutions}, its order included.

    find_generalized_patterns(sequence_list, support)   the reference's function; also takes a QueueTable or (acts, lens)
    generate_actions(agent, games, max_time)            the reference's games, played as one agent.search_batch
    mine(agent, games, max_time, support)               both
    PatternBatch                                        the device arrays of one batch and the rc_patterns_t that names them
    workspace_bytes(total_positions), min_count(n, support), table_cells(keys), generalize(actions)   pure helpers
"""
import ctypes
import logging
from ctypes import POINTER, Structure, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import torch

from librubiks import _hip, cube
from librubiks.solving.results import QueueTable

OK, BAD_ACTION, FAILED, NO_ROOM = 0, 1, 2, 3
STATUS_NAMES = {OK: "ok", BAD_ACTION: "bad action", FAILED: "failed", NO_ROOM: "no room"}
# Workspace a batch may take.  Not tuned: nothing has been measured yet that would prefer another value; it only has to be small
# beside HBM and large enough for the batches a search produces (100 000 solutions of 25 moves need about 0.3 GB).
DEFAULT_BUDGET_BYTES = 2 << 30

# action a is written as its face's name, lower-cased for the positive direction (pattern_mining.py:57-58 of the reference)
SYMBOLS = tuple(cube.action_names[f].lower() if d else cube.action_names[f] for f, d in cube.action_space)
_ACTION_OF = {name: a for a, name in enumerate(SYMBOLS)}

log = logging.getLogger(__name__).info


class _PatternsStruct(Structure):   # mirrors rc_patterns_t (include/rubiks_hip.h)
    _fields_ = [("n_seqs", c_uint32), ("width", c_uint32), ("level", c_uint32), ("min_count", c_uint32),
                ("total_positions", c_size_t), ("node_cells", c_size_t), ("seen_cells", c_size_t), ("out_cap", c_size_t)] + \
               [(name, c_void_p) for name in ("acts", "lens", "pos_off", "lane_seq", "lane_state", "lane_node", "node_keys", "node_count",
                                              "node_first", "seen_keys", "out_rows", "counters", "status")]


POINTER_FIELDS = [name for name, _ in _PatternsStruct._fields_[8:]]
STEPS = ("rc_patterns_begin", "rc_patterns_extend", "rc_patterns_close")

_hip.register({
    "rc_patterns_struct_bytes": [],
    "rc_patterns_table_cells": [c_size_t],
    "rc_patterns_workspace_bytes": [c_size_t],
    "rc_patterns_hash": [c_uint64],
    "rc_patterns_begin": [POINTER(_PatternsStruct), c_void_p],
    "rc_patterns_extend": [POINTER(_PatternsStruct), c_void_p],
    "rc_patterns_close": [POINTER(_PatternsStruct), c_void_p],
    "rc_patterns_level": [POINTER(_PatternsStruct), c_void_p],
}, {"rc_patterns_struct_bytes": c_size_t, "rc_patterns_table_cells": c_size_t, "rc_patterns_workspace_bytes": c_size_t,
    "rc_patterns_hash": c_uint64})


# ---- pure helpers --------------------------------------------------------------------------------------------------------------
def table_cells(keys: int) -> int:
    """rc_patterns_table_cells: the smallest power of two >= max(2 keys, 2)."""
    cells = 2
    while cells < 2 * int(keys):
        cells *= 2
    return cells


def workspace_bytes(total_positions: int) -> int:
    """rc_patterns_workspace_bytes: three lane words of 4 B and an output row of 16 B per position, 28 B per table cell (2 .. 4 cells
    per position) and the counters, every array rounded up to 256 B: 84 .. 140 B per position, whatever the support."""
    r = lambda x: (int(x) + 255) // 256 * 256   # noqa: E731
    P, C = int(total_positions), table_cells(total_positions)
    return 3 * r(4 * P) + r(8 * C) + r(4 * C) + r(8 * C) + r(8 * C) + r(16 * P) + 256


def min_count(n: int, support) -> int:
    """The smallest integer c in 0 .. n with c / n >= support as Python divides, n + 1 if there is none: a pattern is reported iff
    its count is at least this (c / n does not fall as c grows, so one threshold says it all)."""
    n = int(n)
    c = 0
    while c <= n and not c / n >= support:
        c += 1
    return c


def generalize(actions) -> str:
    """The generalised form of a sequence of action indices (the token rule of include/rubiks_hip.h)."""
    seen, letters, out = set(), {}, []
    for a in actions:
        a = int(a)
        f = a // 2
        if f not in letters:
            letters[f] = chr(65 + len(letters))
            out.append(letters[f])
        else:
            out.append(letters[f] if a in seen else letters[f].lower())
        seen.add(a)
    return "".join(out)


def as_actions(sequence_list):
    """-> (acts uint8 [n, width >= 1], lens int64 [n]) of a list of lists of the 12 one-letter names (the reference's form), a
    QueueTable, or an (acts, lens) pair of action indices, which is taken as it is: what its bytes are is the kernels' to say."""
    if isinstance(sequence_list, QueueTable):
        acts, lens = sequence_list.padded(fill=0)
    elif isinstance(sequence_list, tuple) and len(sequence_list) == 2 and isinstance(sequence_list[0], np.ndarray) and sequence_list[0].ndim == 2:
        acts, lens = np.ascontiguousarray(sequence_list[0], dtype=np.uint8), np.asarray(sequence_list[1], dtype=np.int64).reshape(-1)
        if len(lens) != len(acts) or (len(lens) and (lens.min() < 0 or lens.max() > acts.shape[1])):
            raise ValueError(f"lengths {lens.min() if len(lens) else None} .. {lens.max() if len(lens) else None} of {len(lens)} "
                             f"sequences do not fit an array of shape {acts.shape}")
    else:
        rows = []
        for s, seq in enumerate(sequence_list):
            try:
                rows.append([_ACTION_OF[name] for name in seq])
            except (KeyError, TypeError):
                raise ValueError(f"sequence {s}: {[x for x in seq if not isinstance(x, str) or x not in _ACTION_OF][:4]} "
                                 f"are no moves; the moves are {' '.join(SYMBOLS)}") from None
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        acts = np.zeros((len(rows), int(lens.max()) if len(rows) else 0), dtype=np.uint8)
        for s, r in enumerate(rows):
            acts[s, :len(r)] = r
    if acts.shape[1] == 0:
        acts = np.zeros((len(lens), 1), dtype=np.uint8)
    return acts, lens.astype(np.int64)


def result_of(rows: np.ndarray, acts: np.ndarray, n: int) -> dict:
    """The reference's dict of the device's rows {count, first s, first i, length}: by falling count, ties by the first (s, i, j)
    at which the reference's loops meet the pattern; the string is rebuilt from that occurrence."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    order = np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], -rows[:, 0]))
    return {generalize(acts[s, i:i + j]): int(c) / n for c, s, i, j in rows[order].tolist()}


# ---- one batch on the device -----------------------------------------------------------------------------------------------------
class PatternBatch:
    """The device arrays of one batch and the rc_patterns_t that names them (tests fill one by hand to look at every array)."""

    def __init__(self, acts: np.ndarray, lens: np.ndarray, min_count: int, device=None):
        self.lib = _hip.lib()
        dev = device or torch.device("cuda", torch.cuda.current_device())
        acts, lens = np.ascontiguousarray(acts, dtype=np.uint8), np.asarray(lens, dtype=np.int64)
        n, width = acts.shape
        assert n >= 1 and width >= 1 and lens.shape == (n,)
        self.pos_off_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        P = int(self.pos_off_h[-1])
        if P < 1:
            raise ValueError("a batch without a move has no patterns and nothing to launch")
        self.n, self.P, self.cap = n, P, table_cells(P)
        self.bytes = workspace_bytes(P)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)     # noqa: E731
        self.acts, self.lens, self.pos_off = up(acts), up(lens.astype(np.int32)), up(self.pos_off_h.view(np.int64))
        self.lane_seq, self.lane_state, self.lane_node = z((P,), torch.int32), z((P,), torch.int32), z((P,), torch.int32)
        self.node_keys, self.node_count, self.node_first = z((self.cap,), torch.int64), z((self.cap,), torch.int32), z((self.cap,), torch.int64)
        self.seen_keys = z((self.cap,), torch.int64)
        self.out_rows, self.counters, self.status = z((P, 4), torch.int32), z((4,), torch.int32), z((n,), torch.int32)
        s = _PatternsStruct()
        s.n_seqs, s.width, s.level, s.min_count = n, width, 1, int(min_count)
        s.total_positions, s.node_cells, s.seen_cells, s.out_cap = P, self.cap, self.cap, P
        for name in POINTER_FIELDS:
            setattr(s, name, getattr(self, name).data_ptr())
        self.struct = s
        self.live = None   # live lanes after the last step; None before `begin`

    def step(self, name: str):
        _hip.check(getattr(self.lib, name)(ctypes.byref(self.struct), _hip.stream_ptr()), name)

    def _counters(self) -> np.ndarray:
        c = self.counters.cpu().numpy().view(np.uint32)
        self.live = int(c[0])
        return c

    def begin(self) -> int:
        """Level 1 -> the number of live lanes."""
        self.struct.level = 1
        self.step("rc_patterns_begin")
        self._counters()
        return self.live

    def level(self, node_cells: int = None, seen_cells: int = None) -> np.ndarray:
        """The next level, in tables sized for the lanes that are live -> its rows uint32 [k, 4] {count, first s, first i, length}."""
        s = self.struct
        s.level += 1
        s.node_cells = table_cells(self.live) if node_cells is None else int(node_cells)
        s.seen_cells = table_cells(self.live) if seen_cells is None else int(seen_cells)
        assert max(s.node_cells, s.seen_cells) <= self.cap
        self.step("rc_patterns_level")
        c = self._counters()
        if c[2]:
            raise _hip.RubiksHipError(f"level {s.level}: {int(c[2])} rows found the output array of {s.out_cap} rows full")
        return self.out_rows[:int(c[1])].cpu().numpy().view(np.uint32)

    def run(self):
        """-> (rows of every level, status int32 [n])."""
        rows = [np.zeros((0, 4), dtype=np.uint32)]
        self.begin()
        while self.live > 0:
            rows.append(self.level())
        return np.concatenate(rows), self.status.cpu().numpy()


def find_generalized_patterns(sequence_list, support, budget_bytes: int = None) -> dict:
    """
    The reference's function (pattern_mining.py:8-45): {pattern: count / n} of the patterns with count / n >= support, by falling
    count, ties in the order in which the reference's loops first meet them.  sequence_list: see `as_actions`.  The count runs over
    all sequences, so a batch cannot be cut into chunks: one whose workspace (`workspace_bytes`) exceeds `budget_bytes` raises
    ValueError, and so does a name that is no move; a sequence the kernels end with another status than OK raises RubiksHipError.
    """
    acts, lens = as_actions(sequence_list)
    n, P = len(lens), int(lens.sum())
    budget = DEFAULT_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
    if workspace_bytes(P) > budget:
        raise ValueError(f"{n} sequences of {P} moves need {workspace_bytes(P)} bytes of workspace, the budget is {budget}; "
                         "patterns are counted over all sequences, so the batch cannot be split")
    if P == 0:
        return {}
    batch = PatternBatch(acts, lens, min_count(n, support))
    rows, status = batch.run()
    bad = np.flatnonzero(status != OK)
    if len(bad):
        raise _hip.RubiksHipError(f"pattern mining failed for sequences {bad[:8].tolist()}: {[STATUS_NAMES.get(int(s), int(s)) for s in status[bad[:8]]]}")
    return result_of(rows, acts, n)


def names_of(queue) -> list:
    return [SYMBOLS[int(a)] for a in queue]


def generate_actions(agent, games: int, max_time: float, max_states: int = None, **search_kwargs) -> list:
    """
    The reference's generate_actions (pattern_mining.py:48-61) as one `agent.search_batch`: the scrambles are the ones its loop
    draws (depths from np.random.randint(100, 1000), never solved) for every agent that draws nothing from np.random while it
    searches; the solved games' queues as lists of names, in game order; unsolved games are logged and left out.
    """
    states, _, _ = cube.scramble_batch(games, lambda: np.random.randint(100, 1000), True)
    res = agent.search_batch(states, max_time, max_states, **search_kwargs)
    sequences = []
    for g in range(games):
        if not res.solved[g]:
            log(f"Game {g + 1} was not won")
        else:
            sequences.append(names_of(res.queues[g]))
    return sequences


def mine(agent, games: int, max_time: float, support: float, max_states: int = None, budget_bytes: int = None, **search_kwargs):
    """-> (patterns, sequences): `generate_actions`, then `find_generalized_patterns` of what it returns."""
    sequences = generate_actions(agent, games, max_time, max_states, **search_kwargs)
    return find_generalized_patterns(sequences, support, budget_bytes), sequences
