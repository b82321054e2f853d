"""
NumPy model of the three rc_shorten_* entry points (include/rubiks_hip.h, "shortening action queues"), written from the header's
comments: it works on host copies of the struct's arrays and leaves in them what the header says a launch leaves.  Moves come
from oracle.cube; a game's hash table is a dict from the packed key to the node (the kernels' cell placement depends on the
order of the inserts and is not modelled: tables are compared through look-ups).  `counts[g]` says which branch decided what.
"""
import numpy as np

from keys_model import home_cell, pack_keys
from oracle import cube

OK, SKIPPED, BAD_ACTION, FAILED, NO_ROOM = 0, 1, 2, 3, 4
MAX_LEN = (1 << 27) - 2
INT_MAX = 2 ** 31 - 1
BLOCK = 256      # threads of the search's workgroup: a level's scan items are compacted BLOCK at a time
N_ACT = 12


def lookup(cells: np.ndarray, keys: np.ndarray, key) -> int:
    """What a probe of a game's table (its `cells`, its rows of `keys`) finds for `key`: the node, 0 if there is none."""
    mask = len(cells) - 1
    h = int(home_cell(np.asarray(key, dtype=np.uint32)[None], len(cells))[0])
    for _ in range(len(cells)):
        c = int(cells[h])
        if c == 0:
            return 0
        assert 1 <= c <= len(keys), "a cell that names no position of the game"
        if tuple(int(x) for x in keys[c - 1]) == tuple(int(x) for x in key):
            return c
        h = (h + 1) & mask
    raise AssertionError("a table without a free cell")


def table_cells(L: int) -> int:
    need, cells = 2 * (L + 1), 1
    while cells < need:
        cells *= 2
    return cells


def workspace_bytes(P: int, H: int) -> int:
    r = lambda x: (x + 255) // 256 * 256   # noqa: E731
    return r(16 * P) + r(4 * P) + r(48 * P) + r(8 * P) + 2 * r(4 * P) + r(4 * H)


class Batch:
    """Host copies of an rc_shorten_t's arrays.  roots (G, 20) int8, queues: list of byte sequences, select: bools."""

    def __init__(self, roots, queues, select=None, out_width=None, fill=0, lens=None, queue_width=None):
        G = len(queues)
        self.G = G
        self.roots = np.asarray(roots, dtype=np.int8).reshape(G, 20)
        self.lens = np.array([len(q) for q in queues] if lens is None else lens, dtype=np.int32)
        width = max(1, max((len(q) for q in queues), default=0)) if queue_width is None else queue_width
        self.queues = np.zeros((G, width), dtype=np.uint8)
        for g, q in enumerate(queues):
            self.queues[g, :len(q)] = np.asarray(list(q), dtype=np.uint8)
        self.select = np.ones(G, dtype=np.uint8) if select is None else np.asarray(select).astype(np.uint8)
        chosen = self.select != 0
        self.max_len = int(self.lens[chosen].max()) if chosen.any() else 0
        pos = np.where(chosen, self.lens.astype(np.int64) + 1, 0)
        cells = np.array([table_cells(int(L)) if c else 0 for L, c in zip(self.lens, chosen)], dtype=np.int64)
        self.pos_off = np.concatenate([[0], np.cumsum(pos)]).astype(np.uint64)
        self.hash_off = np.concatenate([[0], np.cumsum(cells)]).astype(np.uint64)
        P, H = max(1, int(self.pos_off[-1])), max(2, int(self.hash_off[-1]))
        self.P, self.H = P, H
        self.out_width = max(1, self.max_len) if out_width is None else out_width
        # `fill`: the byte every array holds before the first launch (what a launch does not write must still be there after it)
        f = lambda shape, dt: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, fill, dtype=np.uint8).view(dt).reshape(shape)   # noqa: E731
        self.keys, self.ids, self.nbr, self.claim = f((P, 4), np.uint32), f((P,), np.int32), f((P, 12), np.int32), f((P, 2), np.int32)
        self.frontier_a, self.frontier_b = f((P,), np.int32), f((P,), np.int32)
        self.out_queues, self.out_lens, self.status = f((G, self.out_width), np.uint8), f((G,), np.int32), f((G,), np.int32)
        self.tables = [dict() for _ in range(G)]     # packed key (its bytes) -> node
        self.states = [None] * G                     # (L + 1, 20) of the games that were replayed
        self.counts = [dict() for _ in range(G)]

    def game(self, g):
        """(L, p0) of game g if what the struct says about it holds together, else None (the kernels' load_game)."""
        L, p0, p1 = int(self.lens[g]), int(self.pos_off[g]), int(self.pos_off[g + 1])
        h0, h1 = int(self.hash_off[g]), int(self.hash_off[g + 1])
        cells = h1 - h0
        if L < 0 or L > self.max_len or p1 < p0 or p1 > self.P or p1 - p0 < L + 1 or h1 < h0 or h1 > self.H:
            return None
        if cells < 2 * (L + 1) or cells & (cells - 1) or cells > 1 << 30:
            return None
        return L, p0

    def result(self, g) -> list:
        return [int(a) for a in self.out_queues[g, :self.out_lens[g]]]


def _bump(c: dict, name: str, by: int = 1):
    c[name] = c.get(name, 0) + by


def index(b: Batch):
    """rc_shorten_index."""
    for g in range(b.G):
        c = b.counts[g]
        b.out_lens[g] = -1
        if not b.select[g]:
            b.status[g] = SKIPPED
            _bump(c, "skipped")
            continue
        gm = b.game(g)
        if gm is None:
            b.status[g] = FAILED
            _bump(c, "failed_layout")
            continue
        L, p0 = gm
        acts = b.queues[g, :L]
        if (acts >= N_ACT).any():
            b.status[g] = BAD_ACTION
            _bump(c, "bad_action")
            continue
        b.status[g] = OK
        states = np.empty((L + 1, 20), dtype=np.int8)
        states[0] = b.roots[g]
        for i, a in enumerate(acts):
            states[i + 1] = cube.rotate(states[i], *cube.ACTION_SPACE[int(a)])
        b.states[g] = states
        table = b.tables[g] = {}
        b.keys[p0:p0 + L + 1] = pack_keys(states)
        for p in range(L + 1):
            k = b.keys[p0 + p].tobytes()
            if k in table:
                _bump(c, "revisits")
            else:
                table[k] = p + 1          # positions in order: the first occurrence is the smallest
                _bump(c, "nodes")
            b.ids[p0 + p] = table[k]


def neighbours(b: Batch):
    """rc_shorten_neighbours."""
    for g in range(b.G):
        if b.status[g] != OK or b.game(g) is None:
            continue
        (L, p0), c, table = b.game(g), b.counts[g], b.tables[g]
        for p in range(L + 1):
            if b.ids[p0 + p] != p + 1:
                continue
            kids = pack_keys(cube.expand12(b.states[g][p][None]))
            for a in range(N_ACT):
                v = table.get(kids[a].tobytes(), 0)
                b.nbr[p0 + p, a] = v
                _bump(c, "edges" if v else "no_edge")


def bfs(b: Batch):
    """rc_shorten_bfs: level-synchronous, the smallest scan index 12 i + a claims a node, winners in scan-index order."""
    for g in range(b.G):
        if b.status[g] != OK or b.game(g) is None:
            continue
        (L, p0), c = b.game(g), b.counts[g]
        n = L + 1
        ids, nbr, claim = b.ids[p0:p0 + n], b.nbr[p0:p0 + n], b.claim[p0:p0 + n]
        target = int(ids[L])
        if target == 1:
            b.out_lens[g] = 0
            _bump(c, "target_is_root")
            continue
        claim[:, 0], claim[:, 1] = INT_MAX, 0
        cur, nxt = b.frontier_a[p0:p0 + n], b.frontier_b[p0:p0 + n]
        cur[0] = 1
        claim[0, 1] = -1
        fsize, done = 1, False
        while fsize > 0:
            _bump(c, "levels")
            work = fsize * N_ACT
            _bump(c, "passes", (work + BLOCK - 1) // BLOCK)
            for idx in range(work):
                v = int(nbr[cur[idx // N_ACT] - 1, idx % N_ACT])
                if v == 0:
                    continue
                if claim[v - 1, 1] != 0:
                    _bump(c, "visited_skipped")
                    continue
                if idx < claim[v - 1, 0]:
                    claim[v - 1, 0] = idx
            wins = 0
            visited = claim[:, 1] != 0   # before this level
            for idx in range(work):
                p = int(cur[idx // N_ACT])
                v = int(nbr[p - 1, idx % N_ACT])
                if v == 0 or visited[v - 1]:
                    continue
                if claim[v - 1, 0] != idx:
                    _bump(c, "claims_lost")
                    continue
                nxt[wins] = v
                wins += 1
                claim[v - 1, 1] = (p << 4) | (idx % N_ACT)
                done |= v == target
            fsize = wins
            if done:
                break
            cur, nxt = nxt, cur
        if not done:
            b.status[g] = FAILED
            _bump(c, "failed_search")
            continue
        acts, v = [], target
        while v != 1:
            word = int(claim[v - 1, 1])
            acts.append(word & 15)
            v = word >> 4
        acts.reverse()
        b.out_lens[g] = len(acts)
        if len(acts) > b.out_width:
            b.status[g] = NO_ROOM
            _bump(c, "no_room")
            continue
        b.out_queues[g, :len(acts)] = acts
        _bump(c, "shorter" if len(acts) < L else "same_length")


def shorten(roots, queues, select=None) -> Batch:
    """All three steps on a fresh batch."""
    b = Batch(roots, queues, select)
    index(b)
    neighbours(b)
    bfs(b)
    return b


# ---- the cases the tests share -----------------------------------------------------------------------------------------------
def replay(state: np.ndarray, actions) -> np.ndarray:
    for a in actions:
        state = cube.rotate(state, *cube.ACTION_SPACE[int(a)])
    return state


def euler_tour(depth: int) -> list:
    """Moves of the depth-first walk over all move sequences of up to `depth` moves that never undo the move before, every edge
    there and back: 288 moves for depth 2 (12 + 12 * 11 edges), 3 192 for depth 3; it ends where it starts."""
    moves = []

    def visit(d, last):
        if d == depth:
            return
        for a in range(N_ACT):
            if last is not None and a == (last ^ 1):
                continue
            moves.append(a)
            visit(d + 1, a)
            moves.append(a ^ 1)
    visit(0, None)
    return moves


def scrambled(seed: int, depth: int = 20) -> np.ndarray:
    rng = np.random.RandomState(seed)
    return replay(cube.get_solved(), rng.randint(0, N_ACT, depth))


def random_walk(seed: int, n_moves: int, back_prob: float = 0.3) -> list:
    """A random walk that now and then retraces its last few moves backwards."""
    rng = np.random.RandomState(seed)
    moves = []
    while len(moves) < n_moves:
        if moves and rng.rand() < back_prob:
            k = int(rng.randint(1, 6))
            moves += [a ^ 1 for a in reversed(moves[-k:])]
        else:
            moves.append(int(rng.randint(0, N_ACT)))
    return moves[:n_moves]


F, Fp, B, Bp = 0, 1, 2, 3   # a = 2 * face + (1 - direction); faces F, B, T, D, L, R


def small_cases() -> list:
    """(name, root, queue) of the hand-made cases."""
    s = scrambled(5)
    return [
        ("empty", s, []),
        ("one move", s, [4]),
        ("there and back", s, [6, 7]),
        ("one move four times", s, [8, 8, 8, 8]),
        ("commuting shortcut", s, [F, B, Fp]),                    # ends in s B: one move, an edge the queue never took
        ("two routes, FIFO decides", s, [F, B, Fp, Bp, B, F]),    # ends in s F B = s B F
    ]


def ball_cases() -> list:
    out = []
    for depth, seed in ((2, 7), (3, 8)):
        s = scrambled(seed)
        tour = euler_tour(depth)
        rim = [1, 5, 9][:depth]        # a state on the rim: `depth` moves on three different axes
        out.append((f"depth-{depth} ball", s, tour + rim))
    return out


def long_case():
    """The depth-3 ball and a target one move outside it: the search scans all of level 3 (1 068 nodes, 12 816 scan items, 51
    passes of 256) before it meets the target."""
    return ("depth-3 ball and one move beyond", scrambled(9), euler_tour(3) + [1, 5, 9, 1])


def walk_cases(n_moves: int = 5000) -> list:
    return [(f"walk {seed}", scrambled(100 + seed), random_walk(seed, n_moves)) for seed in (1, 2)]
