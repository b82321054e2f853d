"""
Pattern mining restated twice, for the tests of librubiks/analysis/pattern_mining.py and the rc_patterns_* kernels:

    mine_plain(sequences, support)   the rules of the reference's find_generalized_patterns in plain Python, on lists of action indices
    Batch                            a NumPy model of every launch (rc_patterns_begin / _extend / _close) with the arrays of
                                     rc_patterns_t (include/rubiks_hip.h); its lanes insert one after the other, in position order
    mine_model(acts, lens, support)  the level-wise loop over Batch, with pruning, as the host drives the kernels

Where a key lands in a table depends on the order of the inserts, so a device table is compared through look-ups, not cell by cell.
"""
import numpy as np

OK, BAD_ACTION, FAILED, NO_ROOM = 0, 1, 2, 3
SYMBOLS = ("f", "F", "b", "B", "t", "T", "d", "D", "l", "L", "r", "R")   # action a: face a // 2, lower case for even a
M64 = (1 << 64) - 1
FREE_FIRST = M64


def actions_of(names) -> list:
    return [SYMBOLS.index(x) for x in names]


def names_of(actions) -> list:
    return [SYMBOLS[int(a)] for a in actions]


# ---- the plain restatement ---------------------------------------------------------------------------------------------------
def token(sub, k: int, given: list) -> str:
    """Token of position k of the sub-sequence `sub` of action indices; given: the tokens of the positions before k."""
    c, before = sub[k], list(sub[:k])
    faces = [b // 2 for b in before]
    if c // 2 not in faces:
        return chr(65 + len(set(faces)))             # a new face: the next unused capital
    letter = given[faces.index(c // 2)]                # the face's first occurrence, a capital
    return letter if c in before else letter.lower()   # the very symbol again: capital; the other direction: lower case


def generalized(sub) -> str:
    out = []
    for k in range(len(sub)):
        out.append(token(sub, k, out))
    return "".join(out)


def mine_plain(sequences, support) -> dict:
    """sequences: lists of action indices.  Counts every pattern once per sequence, remembers where it was first met, orders by
    falling count and then by that first meeting (sequence, start, length)."""
    n = len(sequences)
    count, first = {}, {}
    for s, q in enumerate(sequences):
        q = [int(a) for a in q]
        here = set()
        for i in range(len(q)):
            tail, given = q[i:], []
            for j in range(1, len(tail) + 1):   # the token at a position depends on the symbols before it only: one pass per start
                given.append(token(tail, j - 1, given))
                if j >= 2:
                    g = "".join(given)
                    first.setdefault(g, (s, i, j))
                    here.add(g)
        for g in here:
            count[g] = count.get(g, 0) + 1
    kept = [g for g in count if count[g] / n >= support]
    kept.sort(key=lambda g: (-count[g], first[g]))
    return {g: count[g] / n for g in kept}


def min_count(n: int, support) -> int:
    for c in range(n + 1):
        if c / n >= support:
            return c
    return n + 1


# ---- the launches ------------------------------------------------------------------------------------------------------------
def hash64(x: int) -> int:
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def table_cells(keys: int) -> int:
    cells = 2
    while cells < 2 * keys:
        cells *= 2
    return cells


def workspace_bytes(P: int) -> int:
    r = lambda x: (x + 255) // 256 * 256   # noqa: E731
    C = table_cells(P)
    return 3 * r(4 * P) + r(8 * C) + r(4 * C) + r(8 * C) + r(8 * C) + r(16 * P) + 256


def find_or_insert(keys: np.ndarray, cells: int, key: int):
    """-> (cell or -1, created): linear probing from hash64(key) in the first `cells` cells."""
    h = hash64(key) & (cells - 1)
    for _ in range(cells):
        c = int(keys[h])
        if c == 0:
            keys[h] = key
            return h, True
        if c == key:
            return h, False
        h = (h + 1) & (cells - 1)
    return -1, False


def lookup(keys: np.ndarray, cells: int, key: int) -> int:
    """The cell of `key` in a table somebody else filled, -1 if it is not there."""
    h = hash64(key) & (cells - 1)
    for _ in range(cells):
        c = int(keys[h])
        if c == 0:
            return -1
        if c == key:
            return h
        h = (h + 1) & (cells - 1)
    return -1


class Batch:
    ARRAYS = ("lane_seq", "lane_state", "lane_node", "node_keys", "node_count", "node_first", "seen_keys", "out_rows", "counters", "status")

    def __init__(self, acts, lens, min_count: int, fill: int = 0):
        self.acts, self.lens = np.ascontiguousarray(acts, dtype=np.uint8), np.asarray(lens, dtype=np.int64)
        self.n, self.width = self.acts.shape
        self.pos_off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.P = P = int(self.pos_off[-1])
        self.cap = C = table_cells(P)
        self.min_count, self.level, self.node_cells, self.seen_cells, self.live = int(min_count), 1, C, C, None
        full = lambda shape, dt: np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dtype=dt).reshape(shape).copy()   # noqa: E731
        self.lane_seq, self.lane_state, self.lane_node = full((P,), np.uint32), full((P,), np.uint32), full((P,), np.int32)
        self.node_keys, self.node_count, self.node_first, self.seen_keys = full((C,), np.uint64), full((C,), np.uint32), full((C,), np.uint64), full((C,), np.uint64)
        self.out_rows, self.counters, self.status = full((P, 4), np.uint32), full((4,), np.uint32), full((self.n,), np.int32)
        self.distinct = {}   # level -> nodes created (what support 0 reports)

    def begin(self):
        for s in range(self.n):
            L, p0, p1 = int(self.lens[s]), int(self.pos_off[s]), int(self.pos_off[s + 1])
            if L < 0 or L > self.width or p1 - p0 != L:
                self.status[s] = FAILED
            else:
                self.status[s] = BAD_ACTION if (self.acts[s, :L] >= 12).any() else OK
        live = 0
        for s in range(self.n):
            p0, L = int(self.pos_off[s]), int(self.lens[s])
            for i in range(L):
                self.lane_seq[p0 + i] = s
                self.lane_node[p0 + i] = -1
                if self.status[s] == OK:
                    self.lane_state[p0 + i] = 1 << int(self.acts[s, i])
                    if i + 2 <= L:
                        self.lane_node[p0 + i] = 0
                        live += 1
        self.counters[:] = (live, 0, 0, 0)
        self.level, self.live = 1, live

    def next_level(self, node_cells: int = None, seen_cells: int = None):
        """What PatternBatch.level sets before the two launches."""
        self.level += 1
        self.node_cells = table_cells(self.live) if node_cells is None else node_cells
        self.seen_cells = table_cells(self.live) if seen_cells is None else seen_cells

    def extend(self):
        j, NC, SC = self.level, self.node_cells, self.seen_cells
        self.node_keys[:NC], self.node_count[:NC], self.node_first[:NC], self.seen_keys[:SC] = 0, 0, FREE_FIRST, 0
        self.counters[:] = 0
        self.tokens = {}   # position -> token word, for the test's look at the keys
        created_nodes = 0
        for p in range(self.P):
            parent = int(self.lane_node[p])
            if parent < 0:
                continue
            s = int(self.lane_seq[p])
            i = p - int(self.pos_off[s])
            c = int(self.acts[s, i + j - 1])
            state = int(self.lane_state[p])
            f = c >> 1
            shift = 12 + 3 * f
            letter, lower = (state >> shift) & 7, 0
            if not (state >> (2 * f)) & 3:
                letter = bin((state | state >> 1) & 0x555).count("1")
                state |= letter << shift
            elif not (state >> c) & 1:
                lower = 1
            state |= 1 << c
            self.lane_state[p] = state
            tok = 2 * letter + lower
            self.tokens[p] = tok
            node, created = find_or_insert(self.node_keys, NC, (parent + 1) << 8 | (tok + 1))
            if node < 0:
                self.status[s], self.lane_node[p] = NO_ROOM, -1
                continue
            created_nodes += created
            cell, new = find_or_insert(self.seen_keys, SC, (node + 1) << 32 | (s + 1))
            if cell < 0:
                self.status[s], self.lane_node[p] = NO_ROOM, -1
                continue
            self.lane_node[p] = node
            if new:
                self.node_count[node] += 1
            self.node_first[node] = min(int(self.node_first[node]), s << 32 | i)
        self.distinct[j] = created_nodes

    def close(self):
        j, NC = self.level, self.node_cells
        rows = [(int(self.node_count[h]), int(self.node_first[h]) >> 32, int(self.node_first[h]) & 0xFFFFFFFF, j)
                for h in range(NC) if self.node_keys[h] != 0 and self.node_count[h] >= self.min_count]
        self.rows = np.array(rows, dtype=np.uint32).reshape(-1, 4)
        k = min(len(rows), len(self.out_rows))
        self.out_rows[:k] = self.rows[:k]
        live = 0
        for p in range(self.P):
            node = int(self.lane_node[p])
            if node < 0:
                continue
            s = int(self.lane_seq[p])
            i = p - int(self.pos_off[s])
            if self.node_count[node] >= self.min_count and i + j + 1 <= int(self.lens[s]):
                live += 1
            else:
                self.lane_node[p] = -1
        self.counters[:] = (live, len(rows), len(rows) - k, 0)
        self.live = live


def result_of(rows, acts, n: int) -> dict:
    rows = sorted((-int(c), int(s), int(i), int(j)) for c, s, i, j in rows)
    return {generalized([int(a) for a in acts[s, i:i + j]]): -c / n for c, s, i, j in rows}


def mine_model(acts, lens, support) -> dict:
    """The host's loop over the model's launches: a level per pattern length until no lane is live."""
    acts, lens = np.asarray(acts, dtype=np.uint8), np.asarray(lens, dtype=np.int64)
    n = len(lens)
    if n == 0 or lens.sum() == 0:
        return {}
    b = Batch(acts, lens, min_count(n, support))
    b.begin()
    rows = []
    while b.live > 0:
        b.next_level()
        b.extend()
        b.close()
        rows += b.rows.tolist()
    assert (b.status == OK).all()
    return result_of(rows, acts, n)


# ---- batches the tests share ---------------------------------------------------------------------------------------------------
def padded(sequences):
    lens = np.array([len(q) for q in sequences], dtype=np.int64)
    acts = np.zeros((len(sequences), max(1, int(lens.max()) if len(lens) else 1)), dtype=np.uint8)
    for s, q in enumerate(sequences):
        acts[s, :len(q)] = q
    return acts, lens


def ragged_batch(with_bad_byte: bool = True):
    """12 sequences: lengths 0, 1, 2, 63, 64, 65 and 300 (more starts than one workgroup), two identical ones, 200 equal moves (every
    start on one node at every level), all 12 actions in the first 12 moves, and one with a byte 12 inside its length."""
    rng = np.random.RandomState(11)
    walk = lambda L, k=12: rng.randint(0, k, L).tolist()   # noqa: E731
    twin = walk(9, 4)
    bad = walk(7)
    bad[3] = 12
    seqs = [[], [5], [3, 2], walk(63, 6), walk(64), walk(65, 4), walk(300, 3), twin, [7] * 200, list(twin),
            list(rng.permutation(12)) + walk(5), bad if with_bad_byte else walk(7)]
    return padded(seqs)
