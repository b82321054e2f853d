"""
Device-resident batch of breadth-first searches driving the rc_bfs_batch_* kernels (csrc/rubiks_bfs_batch.hip).

S slots hold one game each: its own node store (16-byte packed key, parent, action), its own hash table and a segment of 12 C
child rows.  A step expands the next chunk (at most C parents) of every running slot and makes, on the device, the decision that
`BFSDevice.search` makes on the host after each chunk (librubiks/solving/agents.py:104-129 of the reference): solved, cut, or
commit and advance.  Nothing synchronises in `plant` and `step`; the host looks at seven words per slot per round (`snapshot`).

HBM per slot: 21 B per node row + 4 B per hash cell (a power of two >= twice the node rows) + 28 B per child row, all allocated
up front (`bfs_batch_plan`).
"""
import ctypes
from ctypes import POINTER, Structure, c_size_t, c_uint32, c_void_p

import numpy as np
import torch

from librubiks import _hip
from librubiks.cube.device import DeviceCubes
from librubiks.solving.keys import unpack_keys
from librubiks.solving.lockstep_device import pinned_copy, take_queue_rows

RUNNING, SOLVED, CUT, FAILED, ROOT_SOLVED, GRAPH_DONE, EMPTY = 0, 1, 2, 3, 4, 5, 6
W_STATUS, W_NODES, W_LEVELS, W_QUEUE_LEN, W_LO, W_LEVEL_END, W_MAX_STATES = range(7)
HOST_WORDS, N_WORDS = 7, 14
N_ACT = 12
MAX_DEPTH = 64          # bytes per queue row (God's number in quarter turns is 26)
NODE_BYTES, CELL_BYTES, ROW_BYTES = 21, 4, 28
# Parents per slot and step where the caller names none: from tools/bfs_batch_probe.py (profiles/bfs_batch_probe.txt: 2 500 games of
# depths 1-5 in 2 500 slots, all games in ms).  C = 64 / 256 / 1 024 take 1.47 / 1.56 / 2.91 at max_states 2 000, 5.00 / 3.52 / 4.08
# at 20 000 and 19.3 / 10.2 / 9.6 at 175 000: every launch of a step passes over the whole row space 12 C S, dead rows included,
# which a large C pays for at small searches, and a small C needs more steps at large ones.  256 is within 6 % of the best at
# all three.  The same run has K = 4 steps per round (`BFS(steps_per_round=)`) ahead of 1 and 2 at C = 256 at all three sizes.
DEFAULT_CHUNK = 256


class _BfsBatchStruct(Structure):   # mirrors rc_bfs_batch_t (include/rubiks_hip.h)
    _fields_ = [(name, c_uint32) for name in ("n_slots", "chunk", "capacity", "hash_size", "queue_width", "reserved")] + \
               [(name, c_void_p) for name in ("keys", "parent", "action", "hash", "child_keys", "child_slot", "flags", "prefix", "words",
                                              "queues", "scan_tmp")] + [("scan_tmp_bytes", c_size_t)]


_hip.register({
    "rc_bfs_batch_struct_bytes": [],
    "rc_bfs_batch_scan_bytes": [c_uint32, c_uint32],
    "rc_bfs_batch_plant": [POINTER(_BfsBatchStruct), c_void_p, c_uint32, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p],
    "rc_bfs_batch_step": [POINTER(_BfsBatchStruct), c_void_p],
}, {"rc_bfs_batch_struct_bytes": c_size_t, "rc_bfs_batch_scan_bytes": c_size_t})


def slot_shape(max_states: int, chunk: int) -> tuple:
    """(node rows, hash cells, bytes) of one slot that searches up to `max_states` states in chunks of `chunk` parents."""
    cap_slot = int(max_states) + N_ACT * int(chunk) + 1
    hash_size = max(32, 1 << int(2 * cap_slot - 1).bit_length())
    per_slot = cap_slot * NODE_BYTES + hash_size * CELL_BYTES + N_ACT * chunk * ROW_BYTES + N_WORDS * 8 + MAX_DEPTH
    return cap_slot, hash_size, per_slot


def bfs_batch_plan(n_games: int, max_states: int, slots: int = None, chunk: int = None, budget: int = None) -> tuple:
    """
    -> (S, C, cap_slot, hash_size, total bytes) of the batch that searches `n_games` games under `max_states` (capped at
    agents.bd_MAX_STATES, as `BFS._device_for` caps it).  S is `slots`, or with slots=None the number of games, and in both
    cases at most what `budget` bytes (agents.BFS_BATCH_BYTES) hold and what keeps the row space S 12 C below 2^31.
    C is `chunk` or DEFAULT_CHUNK, and never more than max_states (a level has fewer parents than there are states).
    Raises ValueError when not even one slot fits.
    """
    from librubiks.solving import agents   # (the constants live next to the other budgets)
    budget = agents.BFS_BATCH_BYTES if budget is None else int(budget)
    if n_games < 1 or max_states < 1 or (slots is not None and slots < 1) or (chunk is not None and chunk < 1):
        raise ValueError(f"BFS batch: {n_games} games, max_states {max_states}, slots {slots}, chunk {chunk}")
    ms = int(min(max_states, agents.bd_MAX_STATES))
    C = int(min(chunk or DEFAULT_CHUNK, ms))
    cap_slot, hash_size, per_slot = slot_shape(ms, C)
    fit = min(budget // per_slot, (2 ** 31 - 1) // (N_ACT * C))
    if fit < 1 or cap_slot >= 2 ** 30:
        raise ValueError(f"BFS batch: one slot for max_states {ms} at chunk {C} takes {per_slot} bytes ({cap_slot} node rows); "
                         f"the budget is {budget} bytes and a slot holds fewer than 2^30 node rows")
    S = int(min(n_games if slots is None else min(int(slots), n_games), fit))
    return S, C, cap_slot, hash_size, S * per_slot


class BFSBatch:
    def __init__(self, n_slots: int, max_states_cap: int, chunk: int = None, device=None):
        self.lib = _hip.lib()
        dev = device or torch.device("cuda", torch.cuda.current_device())
        S, C = int(n_slots), int(chunk or min(DEFAULT_CHUNK, max_states_cap))
        if not (S >= 1 and C >= 1 and max_states_cap >= 1 and S * N_ACT * C < 2 ** 31):
            raise ValueError(f"BFS batch: {S} slots, chunk {C}, max_states {max_states_cap} (S 12 C < 2^31)")
        self.S, self.C, self.max_states, self.device = S, C, int(max_states_cap), dev
        self.capacity, self.hash_size, per_slot = slot_shape(self.max_states, C)
        if self.capacity >= 2 ** 30:
            raise ValueError(f"BFS batch: max_states {max_states_cap} too large for 32-bit hash cells")
        self.bytes = S * per_slot
        rows = S * N_ACT * C
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)   # noqa: E731
        self.keys = e((S, self.capacity, 4), torch.int32)
        self.parent = e((S, self.capacity), torch.int32)
        self.action = e((S, self.capacity), torch.uint8)
        self.hash = e((S, self.hash_size), torch.int32)
        self.child_keys = e((rows, 4), torch.int32)
        self.child_slot = e((rows,), torch.int32)
        self.flags = e((rows,), torch.int32)
        self.prefix = e((rows,), torch.int32)
        self.words = torch.zeros((N_WORDS, S), dtype=torch.int64, device=dev)
        self.words[W_STATUS] = EMPTY                                # nothing planted yet: no slot does anything
        self.queues = torch.zeros((S, MAX_DEPTH), dtype=torch.uint8, device=dev)
        scan_bytes = int(self.lib.rc_bfs_batch_scan_bytes(S, C))
        if scan_bytes == 0:
            raise _hip.RubiksHipError("rc_bfs_batch_scan_bytes failed")
        self.scan_tmp = e((scan_bytes,), torch.uint8)
        s = _BfsBatchStruct()
        s.n_slots, s.chunk, s.capacity, s.hash_size, s.queue_width, s.reserved = S, C, self.capacity, self.hash_size, MAX_DEPTH, 0
        for name in ("keys", "parent", "action", "hash", "child_keys", "child_slot", "flags", "prefix", "words", "queues", "scan_tmp"):
            setattr(s, name, getattr(self, name).data_ptr())
        s.scan_tmp_bytes = scan_bytes
        self.struct = s

    def plant(self, slots: np.ndarray, roots: DeviceCubes, first: int, max_states: np.ndarray):
        """Slots `slots` (host integers; entries -1 and S are skipped) restart from roots[first], roots[first + 1], ... with
        max_states[i] each (at most the batch's cap); the others are not touched.  Queued on the stream."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        caps = np.minimum(np.ascontiguousarray(max_states, dtype=np.int64), self.max_states).astype(np.int32)
        assert slots.ndim == 1 and caps.shape == slots.shape and first + len(slots) <= roots.stride and (caps >= 0).all()
        if not len(slots):
            return
        d_slots = torch.from_numpy(slots).pin_memory().to(self.device, non_blocking=True)
        d_caps = torch.from_numpy(caps).pin_memory().to(self.device, non_blocking=True)
        _hip.check(self.lib.rc_bfs_batch_plant(ctypes.byref(self.struct), d_slots.data_ptr(), len(slots), roots.soa.data_ptr(),
                                               roots.stride, int(first), d_caps.data_ptr(), _hip.stream_ptr()), "rc_bfs_batch_plant")

    def step(self, k: int = 1):
        """Queues k steps of every running slot (finished and empty slots do nothing in them)."""
        b, st = ctypes.byref(self.struct), _hip.stream_ptr()
        for _ in range(k):
            _hip.check(self.lib.rc_bfs_batch_step(b, st), "rc_bfs_batch_step")

    queue_len_row = W_QUEUE_LEN   # the row of a snapshot that holds the queue length

    def snapshot(self):
        """(pinned int64 copy [7, S] of the per-slot words status, nodes, levels, queue_len, lo, level_end, max_states; event)."""
        return pinned_copy(self.words[:HOST_WORDS])

    def take_queues(self, slots: np.ndarray, width: int):
        """Queue rows of `slots`, their first `width` bytes, on their way into pinned memory: (host tensor, event, keep-alive)."""
        return take_queue_rows(self.queues, slots, min(int(width), MAX_DEPTH))

    def node_arrays(self, slot: int, n: int) -> dict:
        """Host copies of the first n node rows of `slot` (for tests)."""
        return {"states": unpack_keys(self.keys[slot, :n].cpu().numpy().view(np.uint32)),
                "parent": self.parent[slot, :n].cpu().numpy(), "action": self.action[slot, :n].cpu().numpy()}


def check_words(words: np.ndarray, capacity: int):
    """Raises for a block of per-slot words (`snapshot`) that shows a failed slot or counters that do not fit the slot's arrays."""
    status = words[W_STATUS]
    bad = (status == FAILED) | (status < 0) | (status > EMPTY)
    live = ~bad & (status != EMPTY)
    bad |= live & ~((0 <= words[W_LO]) & (words[W_LO] <= words[W_LEVEL_END]) & (words[W_LEVEL_END] <= words[W_NODES]) &
                    (words[W_NODES] <= capacity) & (words[W_QUEUE_LEN] <= MAX_DEPTH))
    if bad.any():
        s = int(np.argmax(bad))
        raise _hip.RubiksHipError(f"BFS batch: slot {s} failed (words {words[:, s].tolist()}): an index out of range or a parent "
                                  f"chain longer than {MAX_DEPTH}")
