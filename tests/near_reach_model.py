"""
A plain restatement of the search beyond the near-solved table (csrc/rubiks_near_reach.hip, NearTable.reach) on top of
near_model.NearModel, which is used as it is.  The rule (include/rubiks_hip.h): for j = 0, 1, .., J in turn every sequence q of j
actions -- a base-12 number, the first move the most significant digit -- is applied to the state and the result looked up in the
dict; q is a hit if it is there at a depth d <= K.  The first level with a hit gives the distance j + min d, no hit up to J gives
-1, and the solution is the hit with the smallest (d, index) followed by that state's `solve`.

`ReachModel` enumerates ALL 12^j sequences of a state with `_children` applied j times (row 12 p + k is action k on row p, so the
row number IS the sequence's index); `pruned=True` leaves out the sequences the device does not walk (`canonical`), which must not
change anything.  `Launches` is the model of the entry points one call at a time: the best words and live bytes after `begin`
and after every `level` call on a range of work items.
"""
import numpy as np

import near_model as nm

MAX_EXTRA = 10
NO_WORD = np.uint64((1 << 64) - 1)
NONE = 255
DEPTH_SHIFT, LEVEL_SHIFT = 40, 36
INDEX_MASK = (1 << LEVEL_SHIFT) - 1

_canonical = {}


def digits(index: int, j: int) -> list:
    return [index // 12 ** (j - 1 - t) % 12 for t in range(j)]


def canonical(j: int) -> np.ndarray:
    """bool [12^j]: the sequences without an action right after its inverse, without a third equal quarter turn in a row, and
    without an action on the higher-numbered of two opposite faces (faces f, f ^ 1) directly followed by one on the lower."""
    if j not in _canonical:
        idx = np.arange(12 ** j, dtype=np.int64)
        dig = [idx // 12 ** (j - 1 - t) % 12 for t in range(j)]
        ok = np.ones(12 ** j, dtype=bool)
        for t in range(1, j):
            a, p = dig[t], dig[t - 1]
            ok &= a != (p ^ 1)
            ok &= ~(((a >> 1) == ((p >> 1) ^ 1)) & ((p >> 1) > (a >> 1)))
            if t >= 2:
                ok &= ~((a == p) & (a == dig[t - 2]))
        _canonical[j] = ok
    return _canonical[j]


def unpack_keys(w: np.ndarray) -> np.ndarray:
    """keys_model.pack_keys backwards: uint32 [n, 4] -> int8 [n, 20] codes (the states of a table's own nodes)."""
    w = np.asarray(w).astype(np.uint32)
    return np.stack([(w[:, j // 6] >> np.uint32(5 * (j % 6))) & np.uint32(31) for j in range(20)], axis=1).astype(np.int8)


def word(d, level: int, index):
    return (np.uint64(d) << np.uint64(DEPTH_SHIFT)) | np.uint64(level << LEVEL_SHIFT) | np.uint64(index)


def unpack(w):
    """(d, level, index) of a best word that is not NO_WORD."""
    w = int(w)
    return w >> DEPTH_SHIFT, (w >> LEVEL_SHIFT) & 15, w & INDEX_MASK


class ReachModel:
    def __init__(self, model: nm.NearModel):
        self.m = model
        self._leaves = {}

    def leaf_depths(self, state, j: int) -> np.ndarray:
        """uint8 [12^j]: the dict's depth of the state turned by sequence number i, NONE where it is not in the dict."""
        state = np.asarray(state).astype(np.uint8)
        key = (state.tobytes(), j)
        if key not in self._leaves:
            rows = state[None]
            for _ in range(j):
                rows = self.m._children(rows)
            buf, out = rows.tobytes(), np.full(len(rows), NONE, dtype=np.uint8)
            for r in range(len(rows)):
                v = self.m.index.get(buf[20 * r:20 * r + 20], -1)
                if v >= 0:
                    out[r] = self.m.node_depth[v]
            self._leaves[key] = out
        return self._leaves[key]

    def words(self, state, j: int, depth: int = None, pruned: bool = False) -> np.ndarray:
        """uint64 [12^j]: the best word of every sequence of level j that is a hit, NO_WORD for the others."""
        K = self.m.depth if depth is None else depth
        d = self.leaf_depths(state, j)
        hit = d <= K                                                    # (NONE = 255 > K)
        if pruned:
            hit = hit & canonical(j)
        return np.where(hit, word(d.astype(np.uint64), j, np.arange(len(d), dtype=np.uint64)), NO_WORD)

    def best(self, state, j: int, depth: int = None, pruned: bool = False, lo: int = 0, hi: int = None):
        """The smallest (d, index) among the hits of level j with lo <= index < hi, as a word."""
        w = self.words(state, j, depth, pruned)[lo:hi]
        return w.min() if len(w) else NO_WORD

    def solution(self, state, w) -> list:
        d, j, index = unpack(w)
        q = digits(index, j)
        tail, length = self.m.solve([nm.replay(state, q, self.m.lut)])
        assert length[0] == d
        return q + tail[0]

    def reach(self, states, extra: int, depth: int = None, pruned: bool = False):
        """-> (distances int8, levels int8, lengths int32, queues: list of lists)"""
        n = len(states)
        dist, levels, queues = np.full(n, -1, dtype=np.int8), np.full(n, -1, dtype=np.int8), [[] for _ in range(n)]
        for i, s in enumerate(states):
            for j in range(extra + 1):
                w = self.best(s, j, depth, pruned)
                if w != NO_WORD:
                    dist[i], levels[i], queues[i] = unpack(w)[0] + j, j, self.solution(s, w)
                    break
        return dist, levels, dist.astype(np.int32), queues


class Launches:
    """rc_near_reach_begin / rc_near_reach_level one call at a time: `best` (uint64 [n]) and `live` (uint8 [n]) after each.  A work
    item w of level j is (state w // I, prefix w % I), I = 12^min(j, P); it covers the 12^(j - min(j, P)) sequences that begin with
    its prefix, the pruned ones left out as on the device."""

    def __init__(self, rm: ReachModel, states, prefix: int, depth: int = None):
        self.rm, self.states, self.P, self.K = rm, states, prefix, depth
        self.best = np.full(len(states), NO_WORD, dtype=np.uint64)
        self.live = np.zeros(len(states), dtype=np.uint8)

    def items(self, level: int) -> int:
        return len(self.states) * 12 ** min(level, self.P)

    def begin(self):
        self.best = np.array([self.rm.best(s, 0, self.K) for s in self.states], dtype=np.uint64)
        self.live = (self.best == NO_WORD).astype(np.uint8)

    def level(self, level: int, first: int, count: int):
        at = ((self.best >> np.uint64(LEVEL_SHIFT)) & np.uint64(15)).astype(np.int64)
        self.live = ((self.best == NO_WORD) | (at == level)).astype(np.uint8)
        per = 12 ** min(level, self.P)
        span = 12 ** (level - min(level, self.P))
        for i in range(first // per, (first + count - 1) // per + 1):
            if not self.live[i]:
                continue
            lo, hi = max(first, i * per) - i * per, min(first + count, (i + 1) * per) - i * per
            w = self.rm.best(self.states[i], level, self.K, pruned=True, lo=lo * span, hi=hi * span)
            self.best[i] = min(self.best[i], w)

    def unresolved(self) -> int:
        return int((self.best == NO_WORD).sum())
