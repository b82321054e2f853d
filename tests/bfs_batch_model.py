"""
A NumPy/Python model of the two entry points of the batched breadth-first search (rc_bfs_batch_plant / rc_bfs_batch_step), call
by call, on host copies of every array rc_bfs_batch_t names.  A plain module, imported by tests/test_bfs_batch_model.py (which pins
the model to oracle.agents.BFS on the CPU and chooses the scenarios' seeds) and tests/test_bfs_batch_kernels_gpu.py (which compares
the kernels with it after every call).

It restates the reference's FIFO loop (oracle/agents.py, class BFS) and the comments of include/rubiks_hip.h, and nothing of the
kernels' code: per slot a dict from state.tobytes() to node index, oracle.cube.expand12 for the twelve children of a chunk's
parents, first occurrence in row order for new states, and the cut test "stored states >= max_states before a parent's pop".
key_hash and the 5-bit packing (tests/keys_model.py) are used for two things only: to write `keys` /
`child_keys`, and to classify hashing events for the counters.

What `differences` compares, after every call:
  bit for bit   all 14 words of every slot; keys, parent, action over all `capacity` rows of every slot (rows no call has written
                are still the sentinel, or a former tenant's: the model keeps them); child_keys over the whole row space (dead rows
                keep what they held); flags (1 exactly on the lowest row of each state of a working slot's chunk that is neither
                solved nor stored, 0 on dead rows and on every row of a slot that did nothing); prefix (the exclusive sum of the
                flags over the whole row space); queues (bytes beyond a written path are what they were).
  child_slot    exact for a row whose state is stored (node index + 1) and for a solved row (0); an unseen row holds -(h) - 1,
                and hash[h] must be the committed index + 1 of that row's state, or, where the step committed nothing,
                -(lowest row of that state + 1).  Once checked, the device's value is what the model keeps for that row.
  hash          which thread wins a free cell decides the layout, so: a never-planted slot's row is still the sentinel, a
                root-solved slot's row is zero; otherwise the positive cells are exactly 1 .. the committed node count, each once,
                the negative cells are exactly -(row + 1) of the flagged rows of a chunk that ended its slot without a commit
                (none after a commit), and every node and every pending row is found by linear probing from
                key_hash(key) & mask without crossing an empty cell.
  a failed slot in the step that fails it on its words (not on its path): its child rows, flags, hash row and FIRST_SOLVED are
                unspecified; the model adopts them.  Its other words, node rows and queue row are compared as everywhere.

The reference has no queue row and no corrupted words: what the model expects there is the header's sentence on RC_BFSB_FAILED.
"""
import collections
import functools

import numpy as np

from astar_model import U32_MAX, after
from keys_model import check_hash_table, home_cell, pack_keys
from lockstep_model import FILL, N_ACT, Arena, filled, near_roots, replant_list
from oracle import cube as oc

RUNNING, SOLVED, CUT, FAILED, ROOT_SOLVED, GRAPH_DONE, EMPTY = range(7)
(W_STATUS, W_NODES, W_LEVELS, W_QUEUE_LEN, W_LO, W_LEVEL_END, W_MAX_STATES, W_N_PAR, W_FIRST_SOLVED, W_C_ROWS, W_C_BASE, W_C_LO,
 W_SOLVED_PARENT, W_LAST_ACTION) = range(14)
N_WORDS = 14
NO_ROW = -1   # ~0 as an int64


def min_hash_size(capacity: int) -> int:
    """The smallest hash row the entry points admit: a power of two >= 2 * capacity and >= 32."""
    return max(32, 1 << int(2 * capacity - 1).bit_length())


class BfsBatchModel:
    NODE_ARRAYS = ("keys", "parent", "action")

    def __init__(self, n_slots: int, chunk: int, capacity: int, hash_size: int, queue_width: int):
        S, C, cap, H, Q = self.S, self.C, self.cap, self.H, self.Q = int(n_slots), int(chunk), int(capacity), int(hash_size), int(queue_width)
        assert cap >= N_ACT * C + 2 and H & (H - 1) == 0 and H >= max(32, 2 * cap) and Q >= 1
        self.seg = N_ACT * C
        self.room = cap - N_ACT * C - 1   # the most states a slot's node rows let a search store before a pop
        R = self.R = S * self.seg
        self.words = filled((N_WORDS, S), np.int64)
        self.words[W_STATUS] = EMPTY      # all the header asks of the caller
        self.keys = filled((S, cap, 4), np.uint32)
        self.parent = filled((S, cap), np.uint32)
        self.action = filled((S, cap), np.uint8)
        self.child_keys = filled((R, 4), np.uint32)
        self.child_slot = filled((R,), np.int32)
        self.flags, self.prefix = filled((R,), np.uint32), filled((R,), np.uint32)
        self.queues = filled((S, Q), np.uint8)
        # bookkeeping, no device arrays
        self.states = np.zeros((S, cap, 20), dtype=np.int8)
        self.index = [{} for _ in range(S)]
        self.committed = np.zeros(S, dtype=np.int64)     # node rows written so far (the hash row's positive cells)
        self.pending = [[] for _ in range(S)]            # local rows whose negative cells a step without a commit left behind
        self.hash_state = ["untouched"] * S              # untouched | zero | table | unspecified
        self.taken = np.zeros((S, H), dtype=bool)        # occupied cells: under linear probing the set does not depend on the order
        self.unseen = {}                                 # global row -> the value its hash cell must hold (checked by `differences`)
        self.loose = set()                               # slots failed on their words in the last step
        self.never_planted = np.ones(S, dtype=bool)
        self.count = collections.Counter()

    def status(self, s: int) -> int:
        return int(self.words[W_STATUS, s])

    # ---- rc_bfs_batch_plant ---------------------------------------------------------------------------------------------
    def plant(self, slots, roots: np.ndarray, max_states):
        """roots[i] is column first_col + i of the caller's table, max_states[i] its cap as handed to the device."""
        w = self.words
        for i, s in enumerate(np.asarray(slots).tolist()):
            if not 0 <= s < self.S:
                self.count["ignored_slot"] += 1
                continue
            ms = int(max_states[i])
            self.count["max_states_above_room"] += int(ms > self.room)
            if ms < 2:
                self.count["max_states_%d" % ms] += 1
            self.count["replanted_over_larger_tenant"] += int(self.committed[s] > 1)
            self.never_planted[s] = False
            state = (roots[i].astype(np.int64) & 31).astype(np.int8)
            solved = bool(oc.is_solved(state))
            self.states[s, 0] = state
            self.keys[s, 0] = pack_keys(state[None])[0]
            self.parent[s, 0] = self.action[s, 0] = 0
            self.taken[s] = False
            self.pending[s] = []
            w[W_MAX_STATES, s] = min(ms, self.room)
            for word in (W_QUEUE_LEN, W_LO, W_C_ROWS, W_C_BASE, W_C_LO, W_SOLVED_PARENT, W_LAST_ACTION):
                w[word, s] = 0
            w[W_FIRST_SOLVED, s] = NO_ROW
            if solved:   # the reference returns before it stores anything
                self.index[s], self.committed[s], self.hash_state[s] = {}, 0, "zero"
                w[W_STATUS, s], w[W_NODES, s], w[W_LEVELS, s], w[W_LEVEL_END, s], w[W_N_PAR, s] = ROOT_SOLVED, 0, 0, 0, 0
                self.count["root_solved"] += 1
                continue
            self.index[s], self.committed[s], self.hash_state[s] = {state.tobytes(): 0}, 1, "table"
            self.taken[s, home_cell(self.keys[s, :1], self.H)[0]] = True
            w[W_STATUS, s], w[W_NODES, s], w[W_LEVELS, s], w[W_LEVEL_END, s] = RUNNING, 1, 1, 1
            self._next_chunk(s)

    def _next_chunk(self, s: int):
        """`while len(self) < max_states` before the pop, else the parents of the slot's next chunk."""
        w = self.words
        if w[W_NODES, s] >= w[W_MAX_STATES, s]:
            w[W_STATUS, s], w[W_N_PAR, s] = CUT, 0
            self.count["cut_by_next_chunk"] += 1
            self.count["cut_by_next_chunk_on_max_states_exactly"] += int(w[W_NODES, s] == w[W_MAX_STATES, s] and w[W_NODES, s] > 1)
        else:
            w[W_N_PAR, s] = min(self.C, w[W_LEVEL_END, s] - w[W_LO, s])
        w[W_FIRST_SOLVED, s] = NO_ROW

    # ---- rc_bfs_batch_step ----------------------------------------------------------------------------------------------
    def step(self):
        w, c = self.words, self.count
        self.loose = set()
        wild = self._wild()
        working = [s for s in range(self.S) if w[W_STATUS, s] == RUNNING and s not in wild]
        c["never_planted_slot_idle_beside_workers"] += int(bool(working)) * int(self.never_planted.sum())
        for s in range(self.S):
            lo_row = s * self.seg
            if s in wild:   # a running slot whose words do not fit its arrays: it fails, whatever else it holds
                w[W_STATUS, s], w[W_C_ROWS, s], w[W_N_PAR, s] = FAILED, 0, 0
                self.loose.add(s)
                self.hash_state[s] = "unspecified"
                c["failed_on_words"] += 1
                continue
            if w[W_STATUS, s] != RUNNING:   # finished and empty slots do nothing
                w[W_C_ROWS, s], w[W_N_PAR, s] = 0, 0
                self.flags[lo_row:lo_row + self.seg] = 0
                if w[W_STATUS, s] == SOLVED and w[W_QUEUE_LEN, s] < 0:   # (only a hand-made block gets here)
                    self._path(s)
                continue
            self._chunk(s)
        self.prefix[:] = np.concatenate([[0], np.cumsum(self.flags.astype(np.uint64))[:-1]]).astype(np.uint32)

    def _wild(self) -> set:
        """Running slots whose words are not those of a search in its arrays (hand-made, see `write`)."""
        w, out = self.words, set()
        for s in np.flatnonzero(w[W_STATUS] == RUNNING).tolist():
            n, lo, end, ms, n_par = (int(w[x, s]) for x in (W_NODES, W_LO, W_LEVEL_END, W_MAX_STATES, W_N_PAR))
            if not (1 <= n_par <= self.C and 0 <= lo < end <= n < ms <= self.room and end - lo >= n_par):
                out.add(s)
        return out

    def _chunk(self, s: int):
        w, c, C = self.words, self.count, self.C
        n, lo, end, ms, n_par = (int(w[x, s]) for x in (W_NODES, W_LO, W_LEVEL_END, W_MAX_STATES, W_N_PAR))
        assert n == self.committed[s] == len(self.index[s])
        rows, row0, index = N_ACT * n_par, s * self.seg, self.index[s]
        c["chunk_shorter_than_C_at_level_end"] += int(n_par < C)
        c["level_ends_on_a_full_chunk"] += int(n_par == C and lo + n_par == end)
        c["chunk_spans_two_workgroups"] += int(row0 // 256 != (row0 + rows - 1) // 256)
        children = oc.expand12(self.states[s, lo:lo + n_par])
        keys = [k.tobytes() for k in children]
        solved = oc.multi_is_solved(children)
        seen = np.array([k in index for k in keys])
        first_row, new = {}, np.zeros(rows, dtype=bool)
        for r, k in enumerate(keys):
            if not solved[r] and not seen[r] and k not in first_row:
                first_row[k] = r
                new[r] = True
        before = np.concatenate([[0], np.cumsum(new)])   # before[r]: new states in rows below r
        packed = pack_keys(children)
        self.child_keys[row0:row0 + rows] = packed
        self.flags[row0:row0 + self.seg] = 0
        self.flags[row0:row0 + rows] = new
        # ---- what the loop of agents.py does with these rows ----
        cut = next((j for j in range(n_par) if n + before[N_ACT * j] >= ms), n_par)   # the first parent that is not popped
        assert cut >= 1
        fs = int(np.argmax(solved)) if solved.any() else None
        if fs is not None:
            w[W_FIRST_SOLVED, s] = fs
        w[W_C_ROWS, s] = w[W_N_PAR, s] = 0
        c["two_solved_rows_in_one_chunk"] += int(solved.sum() >= 2)
        c["row_of_a_stored_state"] += int(seen.sum())
        # rows that lose the election for a new state
        for r, k in enumerate(keys):
            if not solved[r] and not seen[r] and not new[r]:
                c["duplicate_new_state_in_one_chunk"] += 1
                c["duplicate_loser_has_the_lower_action"] += int(r % N_ACT < first_row[k] % N_ACT)
                c["duplicate_across_workgroups"] += int((row0 + r) // 256 != (row0 + first_row[k]) // 256)
        mask = self.H - 1
        new_rows = np.flatnonzero(new)
        homes = home_cell(packed[new_rows], self.H).tolist()
        c["two_new_states_one_home_cell"] += len(homes) - len(set(homes))
        taken = self.taken[s].copy()   # the cells the new states claim, whether or not the step commits them
        for h in homes:
            x = h
            while taken[x]:
                x = (x + 1) & mask
            taken[x] = True
            c["probe_wrapped"] += int(x < h)
        commit = False
        if fs is not None and fs < N_ACT * cut:   # the solved child is met before the cut
            w[W_NODES, s] = n + before[fs]
            w[W_SOLVED_PARENT, s], w[W_LAST_ACTION, s] = lo + fs // N_ACT, fs % N_ACT
            w[W_STATUS, s], w[W_QUEUE_LEN, s] = SOLVED, -1
            c["solved"] += 1
            c["solved_row_before_the_cut_parent"] += int(cut < n_par)
            self._path(s)
        elif cut < n_par:
            w[W_NODES, s] = n + before[N_ACT * cut]
            w[W_STATUS, s] = CUT
            c["cut_inside_a_chunk"] += 1
            c["solved_row_at_or_after_the_cut_parent"] += int(fs is not None)
            c["solved_row_is_the_cut_parents_first_row"] += int(fs == N_ACT * cut)
        else:
            commit = True
            idx = n + np.arange(len(new_rows))
            assert n + len(new_rows) <= self.cap
            self.states[s, idx] = children[new_rows]
            self.keys[s, idx] = packed[new_rows]
            self.parent[s, idx] = lo + new_rows // N_ACT
            self.action[s, idx] = new_rows % N_ACT
            for k, i in zip((keys[r] for r in new_rows), idx.tolist()):
                index[k] = i
            self.taken[s] = taken
            self.committed[s] = n + len(new_rows)
            w[W_C_ROWS, s], w[W_C_BASE, s], w[W_C_LO, s] = rows, n, lo
            w[W_NODES, s], w[W_LO, s] = n + len(new_rows), lo + n_par
            if lo + n_par == end:
                assert len(new_rows) or n > lo + n_par   # (a level without a new state: no real cube gets there)
                w[W_LEVEL_END, s] = n + len(new_rows)
                w[W_LEVELS, s] += 1
            self._next_chunk(s)
        self.pending[s] = [] if commit else new_rows.tolist()
        # child_slot
        mine = self.child_slot[row0:row0 + rows]
        for r, k in enumerate(keys):
            self.unseen.pop(row0 + r, None)
            if solved[r]:
                mine[r] = 0
            elif seen[r]:
                mine[r] = index[k] + 1
            else:
                self.unseen[row0 + r] = index[k] + 1 if commit else -(first_row[k] + 1)

    def _path(self, s: int):
        """The actions from the root to the solved child, root first; a chain that does not fit the queue row, or words and
        indices that are out of range, fail the slot and leave the row alone."""
        w, c = self.words, self.count
        start, last = int(w[W_SOLVED_PARENT, s]), int(w[W_LAST_ACTION, s])
        ok = 0 <= start < self.cap and 0 <= last < N_ACT
        queue, node = [], start
        while ok and node != 0:   # a parent has a lower index than its child, which bounds the walk
            p, a = int(self.parent[s, node]), int(self.action[s, node])
            ok = p < node and a < N_ACT
            queue.insert(0, a)
            node = p
        if not ok or len(queue) + 1 > self.Q:
            w[W_QUEUE_LEN, s], w[W_STATUS, s] = 0, FAILED
            c["failed_on_path"] += 1
            c["solution_one_longer_than_the_row"] += int(ok and len(queue) + 1 == self.Q + 1)
            return
        queue.append(last)
        self.queues[s, :len(queue)] = queue
        w[W_QUEUE_LEN, s] = len(queue)
        c["solution_written"] += 1
        c["solution_fills_the_row"] += int(len(queue) == self.Q)

    def write(self, name: str, index, value: int):
        """A hand-made change of one entry of `words` ((word, slot)), `parent` or `action` ((slot, node))."""
        getattr(self, name)[index] = value

    # ---- what the reference's attributes would be -------------------------------------------------------------------------
    def game(self, s: int) -> tuple:
        """(solved, len(agent), action queue) of slot s, as the reference reports a search."""
        w = self.words[:, s]
        solved = int(w[W_STATUS]) in (SOLVED, ROOT_SOLVED)
        return solved, int(w[W_NODES]), self.queues[s, :w[W_QUEUE_LEN]].tolist() if solved else []

    # ---- comparison with the device -----------------------------------------------------------------------------------------
    def differences(self, dev: dict) -> list:
        """Names of the arrays of `dev` (name -> host copy of the device array) that are not the model's by the rules of the
        module docstring.  What those rules leave open is adopted from the device once it has passed its check."""
        S, H, seg, out = self.S, self.H, self.seg, []
        theirs = {name: np.ascontiguousarray(dev[name]).reshape(-1).view(getattr(self, name).dtype).reshape(getattr(self, name).shape)
                  for name in ("words", "keys", "parent", "action", "child_keys", "child_slot", "flags", "prefix", "queues")}
        tab = np.ascontiguousarray(dev["hash"]).reshape(S, H).astype(np.int64)
        for s in self.loose:
            rows = slice(s * seg, (s + 1) * seg)
            for name in ("child_keys", "child_slot", "flags"):
                getattr(self, name)[rows] = theirs[name][rows]
            for r in range(rows.start, rows.stop):
                self.unseen.pop(r, None)
            self.words[W_FIRST_SOLVED, s] = theirs["words"][W_FIRST_SOLVED, s]
        if self.loose:
            self.prefix[:] = np.concatenate([[0], np.cumsum(self.flags.astype(np.uint64))[:-1]]).astype(np.uint32)
            self.loose = set()
        # child_slot
        for r, want in list(self.unseen.items()):
            h = -int(theirs["child_slot"][r]) - 1
            if 0 <= h < H and tab[r // seg, h] == want:
                self.child_slot[r] = theirs["child_slot"][r]
                del self.unseen[r]
        for name, mine in ((name, getattr(self, name)) for name in theirs):
            if not np.array_equal(mine, theirs[name]):
                out.append(name)
        # hash
        for s in range(S):
            if not self._hash_ok(s, tab[s], np.ascontiguousarray(dev["hash"]).reshape(S, H)[s]):
                out.append("hash[%d]" % s)
        return out

    def _hash_ok(self, s: int, row: np.ndarray, raw: np.ndarray) -> bool:
        kind = self.hash_state[s]
        if kind == "unspecified":
            return True
        if kind == "untouched":
            return bool((raw.view(np.uint8) == FILL).all())
        if kind == "zero":
            return not row.any()
        n, mask = int(self.committed[s]), self.H - 1
        neg = np.flatnonzero(row < 0)
        if sorted((-row[neg] - 1).tolist()) != sorted(self.pending[s]):
            return False
        try:   # nodes 1 .. n of check_hash_table are this slot's rows 0 .. n - 1
            check_hash_table(np.where(row > 0, row, 0), np.concatenate([np.zeros((1, 4), dtype=np.uint32), self.keys[s, :n]]), n)
        except AssertionError:
            return False
        # a positive cell may sit behind pending cells, and a pending cell behind either: no empty cell on the way
        cells = np.flatnonzero(row)
        key_of = np.array([self.keys[s, row[x] - 1] if row[x] > 0 else self.child_keys[s * self.seg - row[x] - 1] for x in cells], dtype=np.uint32)
        home = home_cell(key_of.reshape(-1, 4), self.H)
        for x, h in zip(cells.tolist(), home.tolist()):
            if any(row[(h + j) & mask] == 0 for j in range((x - h) & mask)):
                return False
        return True


# =====================================================================================================================
# device memory with guards
# =====================================================================================================================
def bfs_batch_arena(m: BfsBatchModel, scan_bytes: int, device="cuda"):
    """(Arena, filled bfs_batch_device._BfsBatchStruct) for the model's shapes: sentinel everywhere -- the words too -- except that
    every status is EMPTY, which is all the header asks for."""
    from librubiks.solving.bfs_batch_device import _BfsBatchStruct
    S, cap, H, R, Q = m.S, m.cap, m.H, m.R, m.Q
    arena = Arena([("keys", np.int32, (S, cap, 4)), ("parent", np.int32, (S, cap)), ("action", np.uint8, (S, cap)), ("hash", np.int32, (S, H)),
                   ("child_keys", np.int32, (R, 4)), ("child_slot", np.int32, (R,)), ("flags", np.int32, (R,)), ("prefix", np.int32, (R,)),
                   ("words", np.int64, (N_WORDS, S)), ("queues", np.uint8, (S, Q)), ("scan_tmp", np.uint8, (scan_bytes,))], device)
    arena.write("words", slice(W_STATUS * S, (W_STATUS + 1) * S), EMPTY)
    s = _BfsBatchStruct()
    s.n_slots, s.chunk, s.capacity, s.hash_size, s.queue_width, s.reserved = S, m.C, cap, H, Q, 0
    for name in arena.layout:
        setattr(s, name, arena.ptr(name))
    s.scan_tmp_bytes = scan_bytes
    return arena, s


# =====================================================================================================================
# the scenarios: call sequences generated beside the model (they read nothing but the model's state)
# =====================================================================================================================
SHAPES = {1: 16, 5: 128, 22: 512}   # chunk -> capacity: hash_size is 2 * capacity, the smallest the entry points admit
S_SLOTS = 4
SEEDED_Q = 3                         # queue rows of the seeded scenario: rows at odd offsets, solutions of up to two moves
F_PRIME = 1


def make_model(C: int, queue_width: int = SEEDED_Q) -> BfsBatchModel:
    cap = SHAPES[C]
    assert min_hash_size(cap) == 2 * cap
    return BfsBatchModel(S_SLOTS, C, cap, 2 * cap, queue_width)


def _level1_cap(root: np.ndarray, j: int) -> int:
    """For a root at least two moves from solved: the max_states with which the j-th parent of level 1 is the first not popped."""
    level1 = oc.expand12(root[None])
    known = {root.tobytes()} | {k.tobytes() for k in level1}
    new = set()
    for k, ok in zip(oc.expand12(level1[:j]), oc.multi_is_solved(oc.expand12(level1[:j]))):
        if not ok and k.tobytes() not in known:
            new.add(k.tobytes())
    return 1 + N_ACT + len(new)


@functools.lru_cache(maxsize=None)
def _boundaries(C: int, root_bytes: bytes) -> list:
    """Node counts of an uncut search of the root after each of its committing steps, as long as it runs."""
    m = BfsBatchModel(1, C, SHAPES[C], 2 * SHAPES[C], 64)
    m.plant([0], np.frombuffer(root_bytes, dtype=np.int8)[None], [U32_MAX])
    out = []
    while m.status(0) == RUNNING:
        m.step()
        if m.status(0) == RUNNING:
            out.append(int(m.words[W_NODES, 0]))
    return out


def _games(m: BfsBatchModel, rng, n: int):
    """n roots with a max_states each: near and far roots, twins in neighbouring entries, caps 0 and 1, caps above what the
    node rows hold, caps that put the cut on a chosen parent of level 1 or exactly on a chunk boundary."""
    C, room = m.C, m.room
    roots = near_roots(rng, n, 0.12)
    far = np.flatnonzero(rng.random_sample(n) < 0.35)
    roots[far] = near_roots(rng, len(far), 0.0, far=True)
    caps = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if C >= 2 and rng.random_sample() < 0.2:
            # solved . F' . b: the parent root . b^-1 of level 1 has the solved cube as its first row
            b = int(rng.choice([x for x in range(N_ACT) if x not in (0, 1) and (x ^ 1) % C and _level1_cap(
                after_actions(oc.get_solved(), (F_PRIME, x)), x ^ 1) <= room]))
            roots[i] = after_actions(oc.get_solved(), (F_PRIME, b))
            caps[i] = _level1_cap(roots[i], b ^ 1)
            continue
        if i and rng.random_sample() < 0.25:
            roots[i] = roots[i - 1]
        kind = rng.random_sample()
        deep = not oc.is_solved(roots[i]) and not oc.multi_is_solved(oc.expand12(roots[i][None])).any()
        if kind < 0.07:
            caps[i] = 0
        elif kind < 0.14:
            caps[i] = 1
        elif kind < 0.26:
            caps[i] = room + rng.randint(1, 40)
        elif kind < 0.32:
            caps[i] = U32_MAX
        elif kind < 0.6 and deep:
            caps[i] = _level1_cap(roots[i], rng.randint(1, N_ACT))
            if caps[i] > room:
                caps[i] = room
        elif kind < 0.8 and _boundaries(C, roots[i].tobytes()):
            caps[i] = rng.choice(_boundaries(C, roots[i].tobytes()))
        else:
            caps[i] = rng.randint(2, room + 1)
    return roots.astype(np.int8), caps


def after_actions(state: np.ndarray, actions) -> np.ndarray:
    for a in actions:
        state = oc.rotate(state, *oc.ACTION_SPACE[a])
    return state


def _plant(slots, roots, caps):
    return {"op": "plant", "slots": np.asarray(slots, dtype=np.int32), "roots": roots, "max_states": np.asarray(caps, dtype=np.uint32), "first_col": 16}


SEEDED_STEPS = 12
IDLE_STEPS = 5   # the last slot is planted for the first time after this many steps


def seeded_scenario(m: BfsBatchModel, seed: int):
    """Yields the calls one by one; the caller applies each to the model (and to the device) before asking for the next."""
    rng = np.random.RandomState(seed)
    S = m.S
    roots, caps = _games(m, rng, S - 1)
    roots[1] = roots[0]   # the same scramble in neighbouring slots, each with its own cap
    yield _plant(np.arange(S - 1), roots, caps)
    for t in range(SEEDED_STEPS):
        yield {"op": "step"}
        if t % 2 == 1:
            finished = np.flatnonzero(m.words[W_STATUS] != RUNNING)
            if t < IDLE_STEPS:
                finished = finished[finished != S - 1]
            slots = replant_list(rng, finished, S)
            if not len(finished):
                slots = slots[(slots < 0) | (slots >= S)]
            if len(slots):
                roots, caps = _games(m, rng, len(slots))
                yield _plant(slots, roots, caps)
    for _ in range(8):   # whoever still runs ends here, and a step in which nobody runs follows
        yield {"op": "step"}
    assert not (m.words[W_STATUS] == RUNNING).any()


_COMMON = ("solved", "cut_by_next_chunk", "root_solved", "two_new_states_one_home_cell", "probe_wrapped", "max_states_above_room",
           "max_states_0", "max_states_1", "replanted_over_larger_tenant", "never_planted_slot_idle_beside_workers", "ignored_slot",
           "solution_written")
_WIDE = ("solved_row_before_the_cut_parent", "solved_row_at_or_after_the_cut_parent", "solved_row_is_the_cut_parents_first_row",
         "two_solved_rows_in_one_chunk", "cut_inside_a_chunk", "cut_by_next_chunk_on_max_states_exactly",
         "chunk_shorter_than_C_at_level_end", "duplicate_new_state_in_one_chunk", "duplicate_loser_has_the_lower_action",
         "row_of_a_stored_state")
# chunk -> the counters its seeded scenario must reach.  With C = 1 a chunk is the twelve distinct children of one parent and the
# node rows hold no second level: no cut inside a chunk, no second solved row, no duplicate, no stored state, and 13 states where a
# cap is at most 3.  A level of these searches has 1, 12 or about 114 parents, so only C = 1 ends a level on a full chunk.
SEEDED_WANTED = {1: _COMMON + ("level_ends_on_a_full_chunk",), 5: _COMMON + _WIDE,
                 22: _COMMON + _WIDE + ("chunk_spans_two_workgroups", "duplicate_across_workgroups")}
# chunk -> seed, chosen on the CPU: tests/test_bfs_batch_model.py::test_the_seeded_scenarios_reach_their_branches
SEEDS = {1: 100, 5: 644, 22: 3096}


# ---- queue rows of one and two bytes ---------------------------------------------------------------------------------------------
QUEUE_C = 22   # (the node rows of the smaller shapes end a search before it reaches a third level)
QUEUE_ROOTS = {1: "R", 2: "R U", 3: "R U F'"}   # solution length -> moves from the solved cube
QUEUE_WANTED = ("solution_fills_the_row", "solution_one_longer_than_the_row", "failed_on_path")


def queue_scenario(m: BfsBatchModel):
    """Slots 0 and 2 hold a solution exactly as long as the queue row, slots 1 and 3 one that is a move longer: the byte after
    slot 1's row is slot 2's, the byte after slot 3's is the guard's."""
    Q = m.Q
    roots = np.array([after(oc.get_solved(), QUEUE_ROOTS[Q + i % 2]) for i in range(m.S)], dtype=np.int8)
    yield _plant(np.arange(m.S), roots, np.full(m.S, m.room))
    for _ in range(Q + 3):
        yield {"op": "step"}
    assert [m.status(s) for s in range(m.S)] == [SOLVED, FAILED, SOLVED, FAILED]


# ---- words and indices that do not fit the arrays ----------------------------------------------------------------------------------
RANGE_C = 5
RUNNING_CORRUPTIONS = ("n_par_C_plus_1", "lo_is_level_end", "level_end_above_nodes", "nodes_is_max_states", "max_states_above_room",
                       "past_capacity_by_1", "past_capacity_by_8")
PATH_CORRUPTIONS = ("none", "solved_parent_is_capacity", "solved_parent_is_capacity_plus_3", "last_action_12", "parent_is_itself",
                    "parent_above_child", "action_12_on_the_chain")
VICTIM = 3
PATH_NODE = 5   # a node of level 1: its chain is one step long


def _corruption(m: BfsBatchModel, name: str) -> list:
    """[(array, index, value)] of a hand-made change to the victim.  Every value is chosen so that the access it would cause,
    were it not checked, stays within eight rows of the slot's own arrays."""
    w, s, cap = m.words, VICTIM, m.cap
    word = lambda x, v: ("words", (x, s), int(v))   # noqa: E731
    if name in RUNNING_CORRUPTIONS:
        assert w[W_STATUS, s] == RUNNING and w[W_N_PAR, s] >= 1
    if name == "n_par_C_plus_1":
        return [word(W_N_PAR, m.C + 1)]
    if name == "lo_is_level_end":
        return [word(W_LO, w[W_LEVEL_END, s])]
    if name == "level_end_above_nodes":
        return [word(W_LEVEL_END, w[W_NODES, s] + 1)]
    if name == "nodes_is_max_states":
        return [word(W_NODES, w[W_MAX_STATES, s])]
    if name == "max_states_above_room":
        return [word(W_MAX_STATES, m.room + 1)]
    if name.startswith("past_capacity_by_"):
        shift = cap + int(name.rsplit("_", 1)[1]) - int(w[W_N_PAR, s]) - int(w[W_LO, s])
        return [word(x, w[x, s] + shift) for x in (W_LO, W_LEVEL_END, W_NODES)]
    # the path cases: a finished slot is made to look as if it had just solved
    assert w[W_STATUS, s] == CUT and w[W_N_PAR, s] == 0 and m.committed[s] > PATH_NODE + 1 and m.parent[s, PATH_NODE] == 0
    out = [word(W_STATUS, SOLVED), word(W_QUEUE_LEN, -1), word(W_SOLVED_PARENT, PATH_NODE), word(W_LAST_ACTION, 3)]
    if name == "solved_parent_is_capacity":
        out[2] = word(W_SOLVED_PARENT, cap)
    elif name == "solved_parent_is_capacity_plus_3":
        out[2] = word(W_SOLVED_PARENT, cap + 3)
    elif name == "last_action_12":
        out[3] = word(W_LAST_ACTION, 12)
    elif name == "parent_is_itself":
        out.append(("parent", (s, PATH_NODE), PATH_NODE))
    elif name == "parent_above_child":
        out.append(("parent", (s, PATH_NODE), PATH_NODE + 1))
    elif name == "action_12_on_the_chain":
        out.append(("action", (s, PATH_NODE), 12))
    return out


def range_scenario(m: BfsBatchModel, seed: int):
    """Slots 0-2 play ordinary games and are planted again when they end; between two steps the victim's words (or one parent /
    action entry) are overwritten by hand, the next step must fail it and nothing else, and a replant makes it a fresh slot."""
    rng = np.random.RandomState(seed)
    S = m.S
    far = lambda n: near_roots(rng, n, 0.0, far=True).astype(np.int8)   # noqa: E731
    others = np.arange(S - 1)
    yield _plant(others, far(S - 1), rng.randint(20, m.room + 1, S - 1))
    for name in RUNNING_CORRUPTIONS + PATH_CORRUPTIONS:
        done = np.array([s for s in others if m.status(s) != RUNNING], dtype=np.int32)
        slots = np.concatenate([done, [VICTIM]])
        path_case = name in PATH_CORRUPTIONS
        caps = np.concatenate([rng.randint(20, m.room + 1, len(done)), [30 if path_case else m.room]])
        yield _plant(slots, far(len(slots)), caps)
        # path cases: cut inside the second chunk, 13 node rows written.  past_capacity: the root's own chunk, where lo + n_par,
        # level_end and nodes are one number, so that none of the three words goes more than 8 beyond the capacity
        for _ in range(2 if path_case else 0 if name.startswith("past_capacity") else 1):
            yield {"op": "step"}
        for array, index, value in _corruption(m, name):
            yield {"op": "write", "name": array, "index": index, "value": value}
        yield {"op": "step", "corruption": name}
        want = SOLVED if name == "none" else FAILED
        assert m.status(VICTIM) == want and m.words[W_C_ROWS, VICTIM] == 0 and m.words[W_N_PAR, VICTIM] == 0, name
        assert not path_case or m.words[W_QUEUE_LEN, VICTIM] == (2 if name == "none" else 0)
        yield {"op": "step"}   # a failed slot does nothing


def apply(m: BfsBatchModel, call: dict):
    op = call["op"]
    if op == "plant":
        m.plant(call["slots"], call["roots"], call["max_states"])
    elif op == "step":
        m.step()
    else:
        m.write(call["name"], call["index"], call["value"])


@functools.lru_cache(maxsize=None)
def oracle_game(root_bytes: bytes, max_states: int) -> tuple:
    """(solved, len(agent), action queue, states in discovery order) of the reference's search."""
    from oracle import agents as oa
    ref = oa.BFS()
    ok = ref.search(np.frombuffer(root_bytes, dtype=np.int8).copy(), max_states)
    return ok, len(ref), list(ref.action_queue), list(ref.states.keys())
