"""
A plain restatement of the near-solved table (csrc/rubiks_near.hip, librubiks/solving/near.py): a dict keyed by a state's 20 codes,
filled by a breadth-first search from the solved state in discovery order, and on top of it `depths`, `solve` and `tighten` with the
rule that a tie goes to the smallest start.  NumPy and a move table only: oracle.cube's by default, or any uint8 [12, 2, 24] table
such as the one the committed fixture cube_golden.npz is made from.

Numbering (as rubiks_bfs.hip): node 0 is the solved state; the frontier of a level is a contiguous node range; child row 12 p + k is
action k on the p-th frontier node; a row is a new node iff its state is not in the dict; new nodes are appended in row order and
remember k.  a_1 .. a_d along the discoverers lead from solved to the node's state.
"""
import numpy as np

from oracle import cube as oc

OK, SKIPPED, BAD_ACTION, FAILED, NO_ROOM = 0, 1, 2, 3, 4
NONE = 255
KIND = oc.KIND


def lut_from_deltas(maps: np.ndarray) -> np.ndarray:
    """uint8 [12, 2, 24] from the reference's int8 [2(dir), 6(face), 2(kind), 24] table of deltas (cube_golden.npz's `maps`)."""
    lut = np.empty((12, 2, 24), dtype=np.uint8)
    for a in range(12):
        lut[a] = np.arange(24) + maps[1 - a % 2, a // 2]
    return lut


class NearModel:
    def __init__(self, depth: int, lut: np.ndarray = None):
        self.depth, self.lut = depth, (oc.move_lut() if lut is None else lut).astype(np.int64)
        solved = oc.get_solved().astype(np.uint8)
        self.index = {solved.tobytes(): 0}
        states, self.node_depth, self.node_action, self.counts = [solved[None]], [0], [0], [1]
        frontier = solved[None]
        for level in range(1, depth + 1):
            fresh, actions = self._new_children(frontier, register=True)
            states.append(fresh)
            self.node_depth += [level] * len(fresh)
            self.node_action += actions
            self.counts.append(len(fresh))
            frontier = fresh
        self.states = np.concatenate(states)
        self.node_depth, self.node_action = np.array(self.node_depth, dtype=np.uint8), np.array(self.node_action, dtype=np.uint8)
        self.frontier = frontier
        self._bands = {}

    def _children(self, frontier: np.ndarray) -> np.ndarray:
        return self.lut[np.arange(12)[None, :, None], KIND[None, None, :], frontier.astype(np.int64)[:, None, :]].reshape(-1, 20).astype(np.uint8)

    def _new_children(self, frontier, register: bool):
        """The rows of the frontier's children, in row order, whose state is in neither the dict nor a lower row; with their k."""
        rows = self._children(frontier)
        buf, seen, keep, actions = rows.tobytes(), ({} if not register else self.index), [], []
        n = len(self.index)
        for r in range(len(rows)):
            key = buf[20 * r:20 * r + 20]
            if key in self.index or key in seen:
                continue
            seen[key] = n + len(keep)
            keep.append(r)
            actions.append(r % 12)
        return rows[keep], actions

    def next_level(self) -> np.ndarray:
        """The states at exactly depth + 1, in discovery order; the table is left as it is."""
        return self._new_children(self.frontier, register=False)[0]

    @property
    def n_nodes(self):
        return len(self.states)

    # ---- lookups -------------------------------------------------------------------------------------------------------------
    def node(self, state) -> int:
        return self.index.get(np.asarray(state).astype(np.uint8).tobytes(), -1)

    def depths(self, states, depth: int = None) -> np.ndarray:
        K = self.depth if depth is None else depth
        out = np.full(len(states), -1, dtype=np.int8)
        for i, s in enumerate(states):
            v = self.node(s)
            if v >= 0 and self.node_depth[v] <= K:
                out[i] = self.node_depth[v]
        return out

    def sequence(self, v: int) -> list:
        """a_1 .. a_d of node v: walk back d times -- a = action(node), state <- state turned by rev(a), looked up."""
        t, back = self.states[v].astype(np.int64), []
        for _ in range(int(self.node_depth[v])):
            a = int(self.node_action[v])
            back.append(a)
            t = self.lut[a ^ 1, KIND, t]
            v = self.node(t)
            assert v >= 0
        return back[::-1]

    def solve(self, states):
        """-> (queues, lengths): the reverse of a_1 .. a_d with every move inverted; length -1 and no moves beyond the table."""
        queues, lens = [], []
        for s in states:
            v = self.node(s)
            seq = self.sequence(v) if v >= 0 else []
            queues.append([a ^ 1 for a in reversed(seq)])
            lens.append(len(seq) if v >= 0 else -1)
        return queues, np.array(lens, dtype=np.int32)

    # ---- tighten -------------------------------------------------------------------------------------------------------------
    def band(self, q) -> np.ndarray:
        """int [L, L]: band[i, k] = node of solved turned by q[i] .. q[i + k], or -1 (also where i + k >= L).  All starts advance
        together, one move a step; kept per queue, whatever window and depth are asked for later."""
        q = np.asarray(q, dtype=np.int64)
        key = q.tobytes()
        if key not in self._bands:
            L = len(q)
            nodes = np.full((L, L), -1, dtype=np.int64)
            t = np.tile(oc.get_solved().astype(np.int64), (L, 1))
            for k in range(L):
                live = L - k                                        # starts 0 .. L - k - 1 have a move q[i + k]
                t[:live] = self.lut[q[k:k + live, None], KIND[None, :], t[:live]]
                buf = t[:live].astype(np.uint8).tobytes()
                for i in range(live):
                    nodes[i, k] = self.index.get(buf[20 * i:20 * i + 20], -1)
            self._bands[key] = nodes
        return self._bands[key]

    def tighten_one(self, q, window: int = None, depth: int = None) -> list:
        """best[0] = 0; best[j] = min over max(0, j - W) <= i < j with d(i, j) defined of best[i] + d(i, j), the smallest i among
        equals; the chosen i followed back from L; every chosen segment gives the a_1 .. a_d of its product."""
        L, K = len(q), self.depth if depth is None else depth
        W = L if window is None else min(L, window)
        nodes = self.band(q)
        best, frm = [0] + [None] * L, [0] * (L + 1)
        for j in range(1, L + 1):
            for i in range(max(0, j - W), j):
                v = nodes[i, j - i - 1]
                if v < 0 or self.node_depth[v] > K:
                    continue
                cost = best[i] + int(self.node_depth[v])
                if best[j] is None or cost < best[j]:              # (strictly: the smallest i keeps a tie)
                    best[j], frm[j] = cost, i
        out, j = [], L
        while j > 0:
            i = frm[j]
            out = self.sequence(int(nodes[i, j - i - 1])) + out
            j = i
        assert len(out) == best[L] <= L
        return out

    def tighten(self, queues, select=None, window: int = None, depth: int = None):
        """-> (rows, status): row g is the tightened queue where status[g] == OK, else the queue as it came."""
        rows, status = [], np.full(len(queues), SKIPPED, dtype=np.int32)
        for g, q in enumerate(queues):
            q = [int(a) for a in q]
            if select is not None and not select[g]:
                rows.append(q)
            elif any(a >= 12 for a in q):
                status[g] = BAD_ACTION
                rows.append(q)
            else:
                status[g] = OK
                rows.append(self.tighten_one(q, window, depth))
        return rows, status


def replay(state, q, lut=None) -> np.ndarray:
    lut = oc.move_lut() if lut is None else lut
    t = np.asarray(state).astype(np.int64)
    for a in q:
        t = lut[int(a), KIND, t].astype(np.int64)
    return t.astype(np.int8)


# ---- inputs the CPU and GPU tests share ---------------------------------------------------------------------------------------
F_, f_, B_, b_, T_, t_, D_, d_, L_, l_, R_, r_ = range(12)
DETOUR = [R_, L_, R_, L_, R_, L_]      # R and L commute: the product is r l (depth 2), and no stretch of it has a product of depth < 2


def fixture_queues(golden_dir: str):
    """(the reference's graph-shortened queues of its solved depth-20 MCTS games, its EGVM queues) from the committed fixtures."""
    import os
    g = np.load(os.path.join(golden_dir, "solve_golden.npz"))
    mcts = [[int(a) for a in q[:n]] for q, n, s in zip(g["mcts_queues"], g["mcts_qlen"], g["mcts_solved"]) if s and n > 0]
    z = np.load(os.path.join(golden_dir, "simple_agents_golden.npz"))
    egvm = [[int(a) for a in z[k]] for k in sorted(z.files) if k.startswith("egvm") and k.endswith("_queue") and len(z[k]) > 2]
    return mcts, egvm


def detour_queues(n: int = 256, seed: int = 4):
    """n queues made as random prefix + detour + suffix; the lengths 0, 1, 2, 63, 64, 65 and 300 are present."""
    rng = np.random.RandomState(seed)
    fixed = [0, 1, 2, 63, 64, 65, 300]
    queues = []
    for g in range(n):
        L = fixed[g] if g < len(fixed) else int(rng.randint(0, 121))
        if L < len(DETOUR) + 1:
            queues.append([int(a) for a in rng.randint(0, 12, L)])
            continue
        pre = int(rng.randint(0, L - len(DETOUR) + 1))
        detour = DETOUR if g % 3 else [int(a) for a in rng.permutation(DETOUR)]
        queues.append([int(a) for a in rng.randint(0, 12, pre)] + list(detour) + [int(a) for a in rng.randint(0, 12, L - len(DETOUR) - pre)])
    return queues
