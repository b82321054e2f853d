"""
A NumPy model of the six entry points of the lock-step agents (rc_egvm_plant / rc_egvm_step / rc_egvm_round_end and
rc_rollout_plant / rc_rollout_step_policy / rc_rollout_step_value), launch by launch, on host copies of exactly the arrays
rc_egvm_t and rc_rollout_t name.  A plain module, imported by tests/test_lockstep_model.py (which pins the model to the oracle's
agents on the CPU) and tests/test_lockstep_kernels_gpu.py (which compares the kernels with it after every launch, bit for bit).

It restates the comments of include/rubiks_hip.h on the two structs and oracle/agents.py (_StepAgent, PolicySearch, ValueSearch,
EGVM), and nothing of the kernels' code: cube moves and solved tests are oracle.cube's, and every "which is the maximum" -- the
12 logits, the 12 child values, a row's running best against a new value, the round's best over the workers -- is np.argmax on
float32 data, so order and NaN behaviour are NumPy's.  A bf16 head is widened to float32 (exactly) before the model sees it.

Arrays start filled with the sentinel byte the arena (below) fills device memory with, so that what no launch has written
compares too.  The model also counts, per instance, which branch decided what (`count`): the scenarios further down are the
seeded launch sequences both test modules use, and their coverage is asserted, not hoped for.
"""
import collections
import ctypes

import numpy as np

from oracle import cube as oc

N_ACT = 12
FILL = 0xA5                       # sentinel byte: no status, no action, no cube code (codes are < 24), and not a NaN as a float
NO_HIT = 0xFFFFFFFF
POLICY = 255
EG_RUNNING, EG_SOLVED, EG_EXHAUSTED, EG_QUEUE_FULL, EG_ROOT_SOLVED = range(5)
RO_RUNNING, RO_SOLVED, RO_EXHAUSTED, RO_QUEUE_FULL, RO_ROOT_SOLVED, RO_BAD_POLICY = range(6)
PER_WORKGROUP = 4 * 256           # rows one workgroup of the step kernels covers: a dword (four rows) per lane
# exact in bf16; -0.0 and 0.0 are equal, so the earlier of the two wins wherever they meet
PALETTE = np.array([-np.inf, -2.0, -0.0, 0.0, 0.5, 3.0, np.inf], dtype=np.float32)
_ALL12 = np.arange(N_ACT)


def filled(shape, dtype, fill=FILL) -> np.ndarray:
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64))
    return np.full(n * dtype.itemsize, fill, dtype=np.uint8).view(dtype).reshape(shape)


def bits(a: np.ndarray) -> np.ndarray:
    """Floats as uint32, so that NaNs and the sign of zero compare."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def children(states: np.ndarray) -> np.ndarray:
    """Child row 12 g + k = action k on state g."""
    return oc.multi_rotate_actions(np.repeat(states, N_ACT, axis=0), np.tile(_ALL12, len(states)))


def first_max(x: np.ndarray, axis=None):
    return np.argmax(np.asarray(x, dtype=np.float32), axis=axis)


def _mixed_dwords(group: np.ndarray, live: np.ndarray) -> int:
    """Dwords (four consecutive rows) that hold rows of more than one game of which some are played and some are not."""
    n = len(group)
    pad = -n % 4
    g = np.concatenate([group, np.full(pad, group[-1])]).reshape(-1, 4)
    lv = np.concatenate([live, np.zeros(pad, dtype=bool)]).reshape(-1, 4)
    real = np.concatenate([np.ones(n, dtype=bool), np.zeros(pad, dtype=bool)]).reshape(-1, 4)
    straddles = (g != g[:, :1]).any(axis=1)
    return int((straddles & lv.any(axis=1) & (real & ~lv).any(axis=1)).sum())


# =====================================================================================================================
# EGVM
# =====================================================================================================================
class EgvmModel:
    ARRAYS = ("rows", "best", "best_value", "best_depth", "paths", "hit", "current", "queues", "status", "nodes", "queue_len", "rounds")

    def __init__(self, n_slots: int, workers: int, depth: int, queue_width: int):
        S, W, D, Q = self.S, self.W, self.D, self.Q = int(n_slots), int(workers), int(depth), int(queue_width)
        R = self.R = S * W
        self.rows, self.best = filled((R, 20), np.int8), filled((R, 20), np.int8)
        self.best_value, self.best_depth = filled((R,), np.float32), filled((R,), np.int32)
        self.paths = filled((S, W, D), np.uint8)
        self.hit = filled((S,), np.uint32)
        self.current = filled((S, 20), np.int8)
        self.queues = filled((S, Q), np.uint8)
        self.status, self.nodes, self.queue_len, self.rounds = (filled((S,), np.int64) for _ in range(4))
        self.count = collections.Counter()
        self._depth_ties = np.zeros(R, dtype=np.int64)   # (bookkeeping of the counters, no device array)

    # ---- rc_egvm_plant ---------------------------------------------------------------------------------------------------
    def plant(self, slots, roots):
        """roots[i] ([n, 20]) is column first_col + i of the caller's roots_soa."""
        for i, s in enumerate(np.asarray(slots).tolist()):
            if not 0 <= s < self.S:
                self.count["ignored_slot"] += 1
                continue
            state = (roots[i].astype(np.int64) & 31).astype(np.int8)
            lo = s * self.W
            self.current[s] = state
            self.rows[lo:lo + self.W] = state
            self.best_depth[lo:lo + self.W] = -1
            self.status[s] = EG_ROOT_SOLVED if oc.multi_is_solved(state[None])[0] else EG_RUNNING
            self.nodes[s] = self.queue_len[s] = self.rounds[s] = 0
            self.hit[s] = NO_HIT

    # ---- rc_egvm_step ----------------------------------------------------------------------------------------------------
    def step(self, d: int, decisions_row: np.ndarray, head: np.ndarray):
        """head: float32 [R, >= 13], 12 logits then the value."""
        W, R = self.W, self.R
        head = np.asarray(head, dtype=np.float32)
        game = np.arange(R) // W
        # liveness is judged on the hit words as they were before the launch
        live = (self.status[game] == EG_RUNNING) & ((self.hit[game] >> 16) >= d)
        self.count["straddle_one_live"] += _mixed_dwords(game, live)
        lv = np.flatnonzero(live)
        if not len(lv):
            return
        if d > 0:   # this forward's value belongs to the state reached at depth d - 1
            v = head[lv, N_ACT]
            had = self.best_depth[lv] >= 0
            take = ~had | (first_max(np.stack([self.best_value[lv], v], axis=1), axis=1) == 1)
            self._depth_ties[lv[had & ~take & (v == self.best_value[lv])]] += 1
            t = lv[take]
            self.best_value[t], self.best_depth[t], self.best[t] = v[take], d - 1, self.rows[t]
            self._depth_ties[t] = 0
        acts = decisions_row[lv].astype(np.int64)
        pol = acts >= N_ACT
        if pol.any():
            logits = head[lv[pol], :N_ACT]
            acts[pol] = first_max(logits, axis=1)
            self.count["policy_nan_after_first"] += int((np.isnan(logits[:, 1:]).any(axis=1) & ~np.isnan(logits[:, 0])).sum())
            self.count["policy_tie"] += int(((logits == logits.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        self.paths.reshape(R, self.D)[lv, d] = acts
        self.rows[lv] = oc.multi_rotate_actions(self.rows[lv], acts)
        won = lv[oc.multi_is_solved(self.rows[lv])]
        for g in np.unique(game[won]).tolist():
            ws = won[game[won] == g] - g * W
            self.hit[g] = min(int(self.hit[g]), (d << 16) | int(ws.min()))   # first depth, then lowest worker
            self.count["hit"] += 1
            self.count["hit_depth_%d" % d] += 1
            if len(ws) > 1:
                self.count["multi_hit"] += 1
                if (g * W + ws.max()) // PER_WORKGROUP != (g * W + ws.min()) // PER_WORKGROUP:
                    self.count["multi_hit_across_workgroups"] += 1

    # ---- rc_egvm_round_end -----------------------------------------------------------------------------------------------
    def round_end(self, values_last: np.ndarray, max_states: int):
        W, D, Q = self.W, self.D, self.Q
        values_last = np.asarray(values_last, dtype=np.float32)
        running = self.status == EG_RUNNING
        self.count["straddle_round_end"] += _mixed_dwords(np.arange(self.R) // W, np.repeat(running, W))
        for g in range(self.S):
            lo = g * W
            sl = slice(lo, lo + W)
            if running[g]:
                was_hit = self.hit[g] != NO_HIT
                qlen = int(self.queue_len[g])
                if was_hit:
                    w_end, n = int(self.hit[g] & 0xFFFF), int(self.hit[g] >> 16) + 1
                else:
                    last = values_last[sl]   # the value of the state after the last depth
                    had = self.best_depth[sl] >= 0
                    take = ~had | (first_max(np.stack([self.best_value[sl], last], axis=1), axis=1) == 1)
                    self._depth_ties[sl][had & ~take & (last == self.best_value[sl])] += 1
                    self.best_value[sl][take], self.best_depth[sl][take] = last[take], D - 1
                    self._depth_ties[sl][take] = 0
                    w_end = int(first_max(self.best_value[sl]))   # np.argmax over w D + d: the best row of lowest index
                    n = int(self.best_depth[lo + w_end]) + 1
                    top = self.best_value[lo + w_end]
                    self.count["round_without_hit"] += 1
                    if np.isnan(top):
                        self.count["nan_win"] += 1
                    else:
                        if (self.best_value[sl] == top).sum() > 1:
                            self.count["tie_workers"] += 1
                            if w_end >= 256 or np.flatnonzero(self.best_value[sl] == top)[-1] >= 256:
                                self.count["tie_workers_across_passes"] += 1
                        if self._depth_ties[lo + w_end]:
                            self.count["tie_depths"] += 1
                    if w_end >= 256:
                        self.count["winner_beyond_first_pass"] += 1
                if qlen + n <= Q:
                    self.queues[g, qlen:qlen + n] = self.paths[g, w_end, :n]
                    if not was_hit:   # every worker of the next round starts from the best state
                        state = (self.rows if n == D else self.best)[lo + w_end].copy()
                        self.current[g] = state
                        self.rows[sl] = state
                    self.nodes[g] += n * W if was_hit else W * D
                    self.queue_len[g] = qlen + n
                    self.rounds[g] += 1
                    if was_hit:
                        self.status[g] = EG_SOLVED
                    elif self.nodes[g] + W * D > max_states:
                        self.status[g] = EG_EXHAUSTED
                    elif self.nodes[g] + W * D == max_states:
                        self.count["on_max_states_equality"] += 1
                else:   # the prefix does not fit: nothing is written for this round
                    self.status[g] = EG_QUEUE_FULL
                    self.count["queue_full_on_hit" if was_hit else "queue_full_without_hit"] += 1
            else:
                self.count["idle_after_status_%d" % self.status[g]] += 1
            self.best_depth[sl] = -1
            self.hit[g] = NO_HIT

    # ---- comparison with the device ----------------------------------------------------------------------------------------
    def differences(self, dev: dict) -> list:
        """Names of the arrays of `dev` (name -> host copy shaped as rc_egvm_t lays it out, rows_soa / best_soa as [20, stride])
        that are not bit for bit the model's; columns >= R of a plane are padding."""
        out = []
        for name in self.ARRAYS:
            mine = getattr(self, name)
            theirs = dev[name + "_soa"][:, :self.R].T if name in ("rows", "best") else dev[name].reshape(mine.shape)
            if not np.array_equal(bits(mine), bits(theirs)):
                out.append(name)
        return out

    def games(self) -> list:
        """[(solved, nodes, queue)] per slot, as the tests of the device batch report a game."""
        return [(bool(self.status[g] in (EG_SOLVED, EG_ROOT_SOLVED)), int(self.nodes[g]), self.queues[g, :self.queue_len[g]].tolist())
                for g in range(self.S)]


# =====================================================================================================================
# the one-step agents
# =====================================================================================================================
def sample12(logits: np.ndarray, u: float):
    """np.random.choice(12, p=softmax(logits)) for its uniform u, as the header words it: (action or 12 for a NaN probability,
    distance of u to the nearest cdf edge)."""
    with np.errstate(all="ignore"):
        x = np.asarray(logits, dtype=np.float32)
        e = np.exp(x - x.max())
        p = e / np.cumsum(e, dtype=np.float32)[-1]
        if np.isnan(p).any():
            return N_ACT, np.inf
        cdf = np.cumsum(p.astype(np.float64))
        cdf /= cdf[-1]
    return min(int(cdf.searchsorted(u, side="right")), N_ACT - 1), float(np.abs(cdf[:-1] - u).min())


class RolloutModel:
    ARRAYS = ("states", "kids", "kid_solved", "queues", "status", "steps")

    def __init__(self, n_slots: int, queue_width: int):
        S, Q = self.S, self.Q = int(n_slots), int(queue_width)
        self.states, self.kids = filled((S, 20), np.int8), filled((N_ACT * S, 20), np.int8)
        self.kid_solved = filled((N_ACT * S,), np.uint8)
        self.queues = filled((S, Q), np.uint8)
        self.status, self.steps = filled((S,), np.int64), filled((S,), np.int64)
        self.count = collections.Counter()
        self.min_margin = np.inf    # of the sampled moves: how close a uniform came to a cdf edge

    def _write_children(self, g: np.ndarray):
        if len(g):
            kid_rows = (N_ACT * g[:, None] + _ALL12).ravel()
            self.kids[kid_rows] = children(self.states[g])
            self.kid_solved[kid_rows] = oc.multi_is_solved(self.kids[kid_rows])

    # ---- rc_rollout_plant --------------------------------------------------------------------------------------------------
    def plant(self, slots, roots, with_children: bool):
        for i, s in enumerate(np.asarray(slots).tolist()):
            if not 0 <= s < self.S:
                self.count["ignored_slot"] += 1
                continue
            state = (roots[i].astype(np.int64) & 31).astype(np.int8)
            self.states[s] = state
            self.status[s] = RO_ROOT_SOLVED if oc.multi_is_solved(state[None])[0] else RO_RUNNING
            self.steps[s] = 0
            if with_children:
                self._write_children(np.array([s]))

    def _count_neighbours(self, played: np.ndarray):
        """Games in a final state that share a dword with a game that is played in this launch."""
        S = self.S
        pad = -S % 4
        pl = np.concatenate([played, np.zeros(pad, dtype=bool)]).reshape(-1, 4)
        st = np.concatenate([np.where(played, RO_RUNNING, self.status), np.zeros(pad, dtype=np.int64)]).reshape(-1, 4)
        some = pl.any(axis=1)
        for final in (RO_SOLVED, RO_EXHAUSTED, RO_QUEUE_FULL, RO_ROOT_SOLVED, RO_BAD_POLICY):
            self.count["dword_shared_with_status_%d" % final] += int((some & (st == final).any(axis=1)).sum())

    def _move(self, g: np.ndarray, acts: np.ndarray, max_steps: int, solved_by_flag=None):
        """Games g make the moves acts (all 0 .. 11)."""
        n = self.steps[g]
        self.queues[g, n] = acts
        self.steps[g] = n + 1
        self.states[g] = oc.multi_rotate_actions(self.states[g], acts)
        solved = oc.multi_is_solved(self.states[g]) if solved_by_flag is None else solved_by_flag
        self.status[g[solved]] = RO_SOLVED
        self.status[g[~solved & (n + 1 >= max_steps)]] = RO_EXHAUSTED
        self.count["solved"] += int(solved.sum())
        self.count["exhausted"] += int((~solved & (n + 1 >= max_steps)).sum())

    # ---- rc_rollout_step_policy --------------------------------------------------------------------------------------------
    def step_policy(self, head, decisions_row, uniforms_row, max_steps: int):
        """head: float32 [S, >= 12] or None; decisions_row: uint8 [S] or None; uniforms_row: float64 [S] or None."""
        run = np.flatnonzero(self.status == RO_RUNNING)
        full = self.steps[run] >= self.Q
        self.status[run[full]] = RO_QUEUE_FULL   # the move's byte does not fit: the move is not made
        self.count["queue_full"] += int(full.sum())
        g = run[~full]
        want = np.full(len(g), POLICY, dtype=np.int64) if decisions_row is None else decisions_row[g].astype(np.int64)
        ask = want >= N_ACT
        if head is not None and ask.any():
            logits = np.asarray(head, dtype=np.float32)[g[ask], :N_ACT]
            if uniforms_row is None:
                want[ask] = first_max(logits, axis=1)
                self.count["greedy_nan"] += int(np.isnan(logits).any(axis=1).sum())
                self.count["greedy_tie"] += int(((logits == logits.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
            else:
                drawn = [sample12(row, u) for row, u in zip(logits, uniforms_row[g[ask]])]
                want[ask] = [a for a, _ in drawn]
                self.min_margin = min([self.min_margin] + [m for _, m in drawn])
                self.count["sampled"] += sum(a < N_ACT for a, _ in drawn)
        bad = want >= N_ACT   # a NaN probability, or a byte that asks a network that is not there
        self.status[g[bad]] = RO_BAD_POLICY
        self.count["bad_policy"] += int(bad.sum())
        played = np.zeros(self.S, dtype=bool)
        played[g[~bad]] = True
        self._count_neighbours(played)
        self._move(g[~bad], want[~bad], max_steps)

    # ---- rc_rollout_step_value ---------------------------------------------------------------------------------------------
    def step_value(self, values: np.ndarray, max_steps: int):
        """values: float32 [12 S] in child order."""
        run = np.flatnonzero(self.status == RO_RUNNING)
        full = self.steps[run] >= self.Q
        self.status[run[full]] = RO_QUEUE_FULL
        self.count["queue_full"] += int(full.sum())
        g = run[~full]
        played = np.zeros(self.S, dtype=bool)
        played[g] = True
        self._count_neighbours(played)
        if not len(g):
            return
        v = np.asarray(values, dtype=np.float32).reshape(self.S, N_ACT)[g]
        flags = self.kid_solved.reshape(self.S, N_ACT)[g] != 0
        won = flags.any(axis=1)
        first = np.argmax(flags, axis=1)   # np.where(solutions)[0][0]
        acts = np.where(won, first, first_max(v, axis=1))
        with np.errstate(invalid="ignore"):
            chosen = v[np.arange(len(g)), first]
            beaten = won & ((v > chosen[:, None]).any(axis=1) | (np.isnan(v).any(axis=1) & ~np.isnan(chosen)))
        self.count["kid_solved_against_larger_value"] += int(beaten.sum())
        self.count["kid_solved_at_action_0"] += int((won & (first == 0)).sum())
        self.count["two_kids_solved"] += int((flags.sum(axis=1) > 1).sum())
        self.count["value_nan"] += int((~won & np.isnan(v).any(axis=1)).sum())
        self.count["value_tie"] += int((~won & ((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1)).sum())
        self._move(g, acts, max_steps, solved_by_flag=won)
        self._write_children(g)   # of the new states, for the next forward pass

    def differences(self, dev: dict) -> list:
        """As EgvmModel.differences, on rc_rollout_t's arrays (states_soa [20, stride], kids_soa [20, 12 stride]).  Where no plant
        wrote children, kids and kid_solved must still be what they were: the model's sentinel."""
        out = []
        for name in self.ARRAYS:
            mine = getattr(self, name)
            if name == "states":
                theirs = dev["states_soa"][:, :self.S].T
            elif name == "kids":
                theirs = dev["kids_soa"][:, :N_ACT * self.S].T
            elif name == "kid_solved":
                theirs = dev[name][:N_ACT * self.S]
            else:
                theirs = dev[name].reshape(mine.shape)
            if not np.array_equal(mine, theirs):
                out.append(name)
        return out

    def games(self) -> list:
        return [(bool(self.status[g] in (RO_SOLVED, RO_ROOT_SOLVED)), int(self.steps[g]), self.queues[g, :self.steps[g]].tolist())
                for g in range(self.S)]


# =====================================================================================================================
# device memory with guards
# =====================================================================================================================
GUARD = 256


class Arena:
    """All arrays of a struct in one uint8 device tensor filled with the sentinel byte: every array 16-byte aligned, with at
    least GUARD sentinel bytes before and after it, so that a store outside an array shows as a changed guard byte."""

    def __init__(self, specs, device="cuda", fill=FILL):
        """specs: [(name, dtype, shape)]."""
        import torch
        self.fill, self.layout, off = fill, {}, GUARD
        for name, dtype, shape in specs:
            dtype = np.dtype(dtype)
            off = (off + 15) // 16 * 16
            nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
            self.layout[name] = (off, nbytes, dtype, tuple(shape))
            off += nbytes + GUARD
        self.nbytes = off
        self.guard = np.ones(off, dtype=bool)
        for o, n, _, _ in self.layout.values():
            self.guard[o:o + n] = False
        self.mem = torch.full((off,), fill, dtype=torch.uint8, device=device)
        assert self.mem.data_ptr() % 16 == 0

    def ptr(self, name: str) -> int:
        return self.mem.data_ptr() + self.layout[name][0]

    def read(self) -> dict:
        """Host copies of all arrays; raises if a guard byte is no longer the sentinel."""
        host = self.mem.cpu().numpy()
        touched = np.flatnonzero(host[self.guard] != self.fill)
        assert not len(touched), f"{len(touched)} guard bytes changed, the first at arena offset {np.flatnonzero(self.guard)[touched[0]]}"
        return {name: host[o:o + n].view(dt).reshape(shape) for name, (o, n, dt, shape) in self.layout.items()}

    def poke(self, name: str, index: int, value: int):
        """One byte of a uint8 array (hand-made flags)."""
        assert self.layout[name][2] == np.uint8
        self.mem[self.layout[name][0] + index] = value

    def write(self, name: str, index, value):
        """array[index] = value on the flat array `name` in its own dtype (index: an int or a slice)."""
        import torch
        o, n, dt, _ = self.layout[name]
        self.mem[o:o + n].view(getattr(torch, dt.name))[index] = value


def egvm_arena(S, W, D, Q, stride, device="cuda"):
    """(Arena, filled egvm_device._EgStruct) for an S x W x D batch with queue rows of Q bytes."""
    from librubiks.solving.egvm_device import _EgStruct
    R = S * W
    assert stride % 16 == 0 and stride >= (R + 15) // 16 * 16
    arena = Arena([("rows_soa", np.int8, (20, stride)), ("best_soa", np.int8, (20, stride)), ("best_value", np.float32, (R,)),
                   ("best_depth", np.int32, (R,)), ("paths", np.uint8, (S, W, D)), ("hit", np.uint32, (S,)), ("current", np.int8, (S, 20)),
                   ("queues", np.uint8, (S, Q)), ("status", np.int64, (S,)), ("nodes", np.int64, (S,)), ("queue_len", np.int64, (S,)),
                   ("rounds", np.int64, (S,))], device)
    s = _EgStruct()
    s.n_slots, s.workers, s.depth, s.queue_width, s.stride = S, W, D, Q, stride
    for name in arena.layout:
        setattr(s, name, arena.ptr(name))
    return arena, s


def rollout_arena(S, Q, stride, device="cuda"):
    from librubiks.solving.rollout_device import _RoStruct
    assert stride % 16 == 0 and stride >= (S + 15) // 16 * 16
    arena = Arena([("states_soa", np.int8, (20, stride)), ("kids_soa", np.int8, (20, N_ACT * stride)), ("kid_solved", np.uint8, (N_ACT * stride,)),
                   ("queues", np.uint8, (S, Q)), ("status", np.int64, (S,)), ("steps", np.int64, (S,))], device)
    s = _RoStruct()
    s.n_slots, s.queue_width, s.stride = S, Q, stride
    for name in arena.layout:
        setattr(s, name, arena.ptr(name))
    assert ctypes.sizeof(s) >= 16
    return arena, s


# =====================================================================================================================
# the scenarios: seeded launch sequences, generated beside the model (they read nothing but the model's state)
# =====================================================================================================================
def head_bits(head32: np.ndarray, bf16: bool):
    """(what the device is given, what the model sees) for a float32 head whose entries are exact in bf16."""
    head32 = np.ascontiguousarray(head32, dtype=np.float32)
    if not bf16:
        return head32, head32
    u = head32.view(np.uint32)
    assert not (u & 0xFFFF).any(), "the head is not exact in bf16"
    half = (u >> 16).astype(np.uint16)
    return half, (half.astype(np.uint32) << 16).view(np.float32)   # widened exactly


def near_roots(rng, n: int, p_solved: float, far: bool = False) -> np.ndarray:
    """n states one or two moves from the solved cube (or, with p_solved, the solved cube); far: ten random moves from it."""
    states = np.tile(oc.get_solved(), (n, 1))
    if far:
        for _ in range(10):
            states = oc.multi_rotate_actions(states, rng.randint(0, N_ACT, n))
        return states.astype(np.int8)
    first = rng.randint(0, N_ACT, n)
    second = rng.randint(0, N_ACT, n)
    kind = rng.random_sample(n)
    one = kind >= p_solved
    two = one & (kind >= p_solved + (1 - p_solved) * 0.55) & (second != (first ^ 1))
    states[one] = oc.multi_rotate_actions(states[one], first[one])
    states[two] = oc.multi_rotate_actions(states[two], second[two])
    return states.astype(np.int8)


def with_nans(rng, a: np.ndarray, rate: float) -> np.ndarray:
    """NaN in one column of about `rate` of the rows of a [n, k] float32 array."""
    rows = np.flatnonzero(rng.random_sample(len(a)) < rate)
    a[rows, rng.randint(0, a.shape[1], len(rows))] = np.nan
    return a


def replant_list(rng, finished: np.ndarray, S: int) -> np.ndarray:
    """Some finished slots in random order, with -1 and S among them as far as the list (at most S entries) has room."""
    pick = finished[rng.random_sample(len(finished)) < 0.5] if len(finished) else np.array([0])
    if not len(pick):
        pick = finished[:1]
    slots = rng.permutation(pick)[:max(1, S - 2)].tolist()
    for bad in (-1, S):
        if len(slots) < S:
            slots.insert(rng.randint(0, len(slots) + 1), bad)
    return np.array(slots, dtype=np.int32)


# (S, W, D) -> (queue rows of D + 1 bytes?, the counters the case is meant to reach).  Seeds: chosen on the CPU, see
# tests/test_lockstep_model.py::test_the_scenarios_reach_their_branches.
_FINAL = tuple("idle_after_status_%d" % s for s in (EG_SOLVED, EG_EXHAUSTED, EG_QUEUE_FULL, EG_ROOT_SOLVED))
EGVM_CASES = {
    (1, 1, 1): (False, ("round_without_hit", "hit", "on_max_states_equality")),
    (3, 5, 2): (True, ("straddle_one_live", "tie_workers", "tie_depths", "multi_hit", "queue_full_without_hit", "ignored_slot",
                       "on_max_states_equality")),
    (7, 21, 3): (True, ("straddle_one_live", "nan_win", "tie_workers", "tie_depths", "multi_hit", "hits_at_two_depths",
                        "queue_full_on_hit", "queue_full_without_hit", "on_max_states_equality", "ignored_slot",
                        "policy_nan_after_first") + _FINAL),
    (2, 257, 2): (False, ("nan_win", "tie_workers", "tie_workers_across_passes", "winner_beyond_first_pass", "tie_depths", "multi_hit",
                          "on_max_states_equality", "ignored_slot", "policy_nan_after_first")),
    (1, 1300, 3): (False, ("nan_win", "tie_workers", "tie_workers_across_passes", "winner_beyond_first_pass", "tie_depths", "multi_hit",
                           "multi_hit_across_workgroups", "hits_at_two_depths", "on_max_states_equality", "policy_nan_after_first")),
    (1027, 1, 2): (True, ("straddle_one_live", "nan_win", "tie_depths", "queue_full_on_hit", "queue_full_without_hit",
                          "on_max_states_equality", "ignored_slot", "policy_nan_after_first") + _FINAL),
}
EGVM_HEADS = {"f32_ld13": (13, False), "f32_ld16": (16, False), "bf16_ld13": (13, True)}
# (S, W, D, head kind) -> seed
EGVM_SEEDS = {
    (1, 1, 1): dict(zip(EGVM_HEADS, (100, 10101, 20100))),
    (3, 5, 2): dict(zip(EGVM_HEADS, (30102, 40115, 50119))),
    (7, 21, 3): dict(zip(EGVM_HEADS, (60391, 70443, 82245))),
    (2, 257, 2): dict(zip(EGVM_HEADS, (90134, 100141, 110101))),
    (1, 1300, 3): dict(zip(EGVM_HEADS, (120198, 130160, 140136))),
    (1027, 1, 2): dict(zip(EGVM_HEADS, (150100, 160100, 170100))),
}
EGVM_SEEDS = {case + (kind,): seed for case, seeds in EGVM_SEEDS.items() for kind, seed in seeds.items()}
EGVM_ROUNDS = 6


def _solving_paths(current: np.ndarray, D: int, deep: bool) -> list:
    """Per state: {depth j: codes of the action sequences of length j + 1 <= D (base 12, first action first) that reach the
    solved cube at depth j and not before}."""
    n = len(current)
    k1 = children(current)
    s1 = oc.multi_is_solved(k1).reshape(n, 12)
    levels = [s1]
    if D >= 2:
        k2 = children(k1)
        s2 = oc.multi_is_solved(k2).reshape(n, 12, 12)
        levels.append((s2 & ~s1[:, :, None]).reshape(n, 144))
        if D >= 3 and deep:
            s3 = oc.multi_is_solved(children(k2)).reshape(n, 12, 12, 12)
            levels.append((s3 & ~s1[:, :, None, None] & ~s2[:, :, :, None]).reshape(n, 1728))
    return [{j: np.flatnonzero(lv[i]) for j, lv in enumerate(levels) if lv[i].any()} for i in range(n)]


def _egvm_round_inputs(m: EgvmModel, rng, ld: int):
    """Decision bytes [D, R], heads [D][R, ld] and the last values [R] of one round."""
    S, W, D, R = m.S, m.W, m.D, m.R
    dec = np.where(rng.random_sample((D, R)) < 0.5, POLICY, rng.randint(0, N_ACT, (D, R))).astype(np.uint8)
    # values: column j is the value of the state a row reaches at depth j.  Per game either anything from the palette, or
    # everything below a ceiling that a few (worker, depth) places hold: ties between workers and depths decide, anywhere in W
    val = rng.randint(0, len(PALETTE), (R, D))
    for g in np.flatnonzero(rng.randint(0, 3, S) > 0).tolist():
        top = rng.randint(2, len(PALETTE))
        block = rng.randint(0, top, (W, D))
        places = [(rng.randint(0, W), rng.randint(0, D)) for _ in range(rng.randint(1, 4))]
        if rng.random_sample() < 0.3:   # the last worker: the last pass of a strided loop over the workers
            places[0] = (W - 1, places[0][1])
        if rng.random_sample() < 0.5:
            places.append((places[0][0], rng.randint(0, D)))
        for w, d in places:
            block[w, d] = top
        val[g * W:(g + 1) * W] = block
    val = PALETTE[val]
    nan_rate = 0.02 if rng.random_sample() < 0.5 else 0.0
    heads = []
    for d in range(D):
        head = np.full((R, ld), 99.0, dtype=np.float32)   # (what lies beyond the value column is neither logit nor value)
        head[:, :N_ACT] = PALETTE[rng.randint(0, len(PALETTE), (R, N_ACT))]
        head[:, N_ACT] = val[:, d - 1] if d > 0 else PALETTE[rng.randint(0, len(PALETTE), R)]   # (step 0 reads no value)
        head[:, :N_ACT + 1] = with_nans(rng, head[:, :N_ACT + 1].copy(), nan_rate)
        heads.append(head)
    last = val[:, D - 1].copy()
    last[rng.random_sample(R) < nan_rate / 4] = np.nan
    # chosen workers are handed moves that solve the cube at a chosen depth
    running = np.flatnonzero(m.status == EG_RUNNING)
    if len(running):
        plans = _solving_paths(m.current[running], D, deep=S <= 8)
        for g, plan in zip(running.tolist(), plans):
            if not plan or rng.random_sample() >= 0.5:
                continue
            j0 = min(plan)
            assign = [(int(w), j0) for w in rng.choice(W, min(W, rng.randint(1, 4)), replace=False)]
            later = [j for j in plan if j > j0]
            if later and W > len(assign) and rng.random_sample() < 0.6:   # a worker that would be solved at a later depth: it must lose
                taken = [w for w, _ in assign]
                free = [w for w in range(min(W, max(taken) + 40)) if w not in taken]
                lower = [w for w in free if w < min(taken)]
                assign.append((int(rng.choice(lower if lower and rng.random_sample() < 0.7 else free)), later[rng.randint(0, len(later))]))
                m.count["hits_at_two_depths"] += 1
            for w, depth in assign:
                code = int(rng.choice(plan[depth]))
                for dd in range(depth, -1, -1):
                    dec[dd, g * W + w] = code % N_ACT
                    code //= N_ACT
    return dec, heads, last


def egvm_scenario(m: EgvmModel, seed: int, ld: int, rounds: int = EGVM_ROUNDS):
    """Yields the launches of a case one by one; the caller applies each to the model (and to the device) before asking for the
    next, which may depend on where the model's games stand."""
    rng = np.random.RandomState(seed)
    S, W, D = m.S, m.W, m.D
    narrow = m.Q == D + 1
    # a game that plays on without a hit sits on nodes + W D == max_states after its round `on` and ends after the next
    on = 1 if narrow else 2
    max_states = (on + 1) * W * D
    # with many workers a game near the solved cube is solved in its first round by chance: those start far from it, play rounds
    # without a hit, and meet the near roots when they are planted again
    yield {"op": "plant", "slots": np.arange(S, dtype=np.int32), "roots": near_roots(rng, S, 0.08 if S >= 3 else 0.0, far=W >= 64),
           "first_col": 0}
    for t in range(rounds):
        dec, heads, last = _egvm_round_inputs(m, rng, ld)
        for d in range(D):
            yield {"op": "step", "d": d, "decisions": dec[d], "head": heads[d]}
        yield {"op": "round_end", "values": last, "max_states": max_states}
        if t == on:   # once per case: some finished slots restart, from column 16 on of another table of roots
            slots = replant_list(rng, np.flatnonzero(m.status != EG_RUNNING), S)
            yield {"op": "plant", "slots": slots, "roots": near_roots(rng, len(slots), 0.08 if S >= 3 else 0.0), "first_col": 16}


def apply_egvm(m: EgvmModel, launch: dict, bf16: bool = False):
    if launch["op"] == "plant":
        m.plant(launch["slots"], launch["roots"])
    elif launch["op"] == "step":
        m.step(launch["d"], launch["decisions"], head_bits(launch["head"], bf16)[1])
    else:
        m.round_end(launch["values"], launch["max_states"])


# ---- the one-step agents ---------------------------------------------------------------------------------------------------
ROLLOUT_CASES = [(1, 8), (5, 2), (21, 8), (21, 2), (1027, 8), (1027, 2)]   # (S, queue width)
# (kind, S, Q) -> seed
ROLLOUT_SEEDS = {(kind, S, Q): seed for kind, seeds in (
    ('value', (5000, 15000, 25000, 35000, 45000, 55000)),
    ('policy', (65000, 75000, 85005, 95003, 105000, 115000)),
) for (S, Q), seed in zip(ROLLOUT_CASES, seeds)}
_SHARED = tuple("dword_shared_with_status_%d" % s for s in (RO_SOLVED, RO_ROOT_SOLVED))


def rollout_wanted(kind: str, S: int, Q: int) -> tuple:
    """The counters a case is meant to reach."""
    if S < 21:
        return ("solved",) if S > 1 else ()
    want = ("solved", "ignored_slot", "queue_full" if Q == 2 else "exhausted") + _SHARED
    want += ("dword_shared_with_status_%d" % (RO_QUEUE_FULL if Q == 2 else RO_EXHAUSTED),)
    if kind == "value":
        return want + ("kid_solved_against_larger_value", "kid_solved_at_action_0", "two_kids_solved", "value_nan", "value_tie")
    return want + ("sampled", "greedy_nan", "greedy_tie", "bad_policy", "dword_shared_with_status_%d" % RO_BAD_POLICY)


def _solving_action(states: np.ndarray) -> np.ndarray:
    """Per state the action that solves it, or -1."""
    flags = oc.multi_is_solved(children(states)).reshape(len(states), N_ACT)
    return np.where(flags.any(axis=1), np.argmax(flags, axis=1), -1)


def value_scenario(m: RolloutModel, seed: int, moves: int = 7, max_steps: int = 4):
    rng = np.random.RandomState(seed)
    S = m.S
    yield {"op": "plant", "slots": np.arange(S, dtype=np.int32), "roots": near_roots(rng, S, 0.08 if S >= 3 else 0.0), "first_col": 0,
           "with_children": True}
    for t in range(moves):
        if t in (1, 4):   # hand-made flags: two children of a game that has no solved child are called solved
            free = np.flatnonzero((m.status == RO_RUNNING) & (m.steps < m.Q) & ~(m.kid_solved.reshape(S, N_ACT) != 0).any(axis=1))
            if len(free):
                g = int(rng.choice(free))
                yield {"op": "flags", "index": (N_ACT * g + np.sort(rng.choice(N_ACT, 2, replace=False))).tolist()}
        values = PALETTE[rng.randint(0, len(PALETTE), N_ACT * S)]
        values[rng.random_sample(N_ACT * S) < 0.01] = np.nan
        yield {"op": "value", "values": values, "max_steps": max_steps}
        if t == 3:
            slots = replant_list(rng, np.flatnonzero(m.status != RO_RUNNING), S)
            yield {"op": "plant", "slots": slots, "roots": near_roots(rng, len(slots), 0.08 if S >= 3 else 0.0), "first_col": 16,
                   "with_children": True}


# per move: (head: None, "greedy" or "sampled"; bf16; ld; decision bytes: None, "actions" or "mixed")
POLICY_MOVES = [(None, False, 0, "actions"), ("greedy", False, 13, None), ("sampled", False, 16, None), ("greedy", True, 13, "mixed"),
                (None, False, 0, "mixed"), ("sampled", True, 13, "mixed"), ("greedy", False, 16, "mixed"), ("sampled", False, 13, None)]
MARGIN = 1e-5   # a sampled move's uniform stays this far from every cdf edge: an fp32 softmax differs between implementations
                # by a few ulp per term, at most about 3e-6 on an edge over 12 terms (tests/test_rollout_batch_gpu.py)


def policy_scenario(m: RolloutModel, seed: int, max_steps: int = 5):
    rng = np.random.RandomState(seed)
    S = m.S
    yield {"op": "plant", "slots": np.arange(S, dtype=np.int32), "roots": near_roots(rng, S, 0.08 if S >= 3 else 0.0), "first_col": 0,
           "with_children": False}
    for t, (kind, bf16, ld, bytes_) in enumerate(POLICY_MOVES):
        solve = _solving_action(m.states)
        solve[rng.random_sample(S) >= 0.3] = -1   # some games one move from solved are led there
        dec = head = uni = None
        if bytes_ is not None:
            dec = rng.randint(0, N_ACT, S)
            dec[solve >= 0] = solve[solve >= 0]
            if bytes_ == "mixed":   # (without a head, a byte that asks the network ends the game)
                dec[rng.random_sample(S) < (0.5 if kind else 0.03)] = POLICY
            dec = dec.astype(np.uint8)
        if kind == "greedy":
            head = np.full((S, ld), 99.0, dtype=np.float32)
            head[:, :N_ACT] = with_nans(rng, PALETTE[rng.randint(0, len(PALETTE), (S, N_ACT))], 0.02)
            led = np.flatnonzero(solve >= 0)
            head[led, :N_ACT] = PALETTE[rng.randint(0, len(PALETTE) - 1, (len(led), N_ACT))]
            head[led, solve[led]] = np.inf
        elif kind == "sampled":
            head = np.full((S, ld), 99.0, dtype=np.float32)
            logits = PALETTE[rng.randint(1, len(PALETTE) - 1, (S, N_ACT))]
            logits[rng.random_sample((S, N_ACT)) < 0.1] = -np.inf
            odd = np.flatnonzero(rng.random_sample(S) < 0.03)   # a NaN probability: a NaN, +inf (inf - inf), or nothing but -inf
            logits[odd, rng.randint(0, N_ACT, len(odd))] = np.where(rng.random_sample(len(odd)) < 0.5, np.nan, np.inf)
            if len(odd):
                logits[odd[0]] = -np.inf
            head[:, :N_ACT] = logits
            uni = rng.random_sample(S)
            for g in range(S):
                while sample12(logits[g], uni[g])[1] < 2 * MARGIN:
                    uni[g] = rng.random_sample()
        yield {"op": "policy", "head": head, "bf16": bf16, "decisions": dec, "uniforms": uni, "max_steps": max_steps}
        if t == 3:
            slots = replant_list(rng, np.flatnonzero(m.status != RO_RUNNING), S)
            yield {"op": "plant", "slots": slots, "roots": near_roots(rng, len(slots), 0.08 if S >= 3 else 0.0), "first_col": 16,
                   "with_children": False}


def apply_rollout(m: RolloutModel, launch: dict):
    op = launch["op"]
    if op == "plant":
        m.plant(launch["slots"], launch["roots"], launch["with_children"])
    elif op == "flags":
        m.kid_solved[launch["index"]] = 1
    elif op == "value":
        m.step_value(launch["values"], launch["max_steps"])
    else:
        head = None if launch["head"] is None else head_bits(launch["head"], launch["bf16"])[1]
        m.step_policy(head, launch["decisions"], launch["uniforms"], launch["max_steps"])
