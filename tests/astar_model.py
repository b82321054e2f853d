"""
A NumPy model of the six entry points of the batched weighted A* (rc_astar_init / rc_astar_plant / rc_astar_pop_expand /
rc_astar_gather_new / rc_astar_push_relax / rc_astar_solutions), launch by launch, on host copies of every array rc_astar_t names.
A plain module, imported by tests/test_astar_model.py (which pins the model to oracle.agents.AStar on the CPU) and
tests/test_astar_kernels_gpu.py (which compares the kernels with it after every launch).

It restates the reference's semantics (oracle/agents.py, class AStar) and the comments of include/rubiks_hip.h, and nothing of the
kernels' code: a dict from state.tobytes() to index per problem, heapq on (cost, index) for the open list, first occurrence in row
order, oracle.cube.expand12 for the children, the two fancy assignments of AStar._relax_seen literally -- so gather-before-scatter
and last-write-wins are NumPy's own -- and cost = lambda * G - value in float64 from the float32 value, product and sum rounded
separately.  key_hash and the 5-bit packing (tests/keys_model.py) are used for two things only: to write
`keys` / `child_keys`, and to classify hashing events for the counters.

What `differences` compares, after every launch:
  bit for bit   G, parents, parent_actions, keys over all C + 1 rows (rows above n_nodes and row 0 are still the sentinel, or a
                former tenant's rows after a replant: the model keeps them); popped, child_keys, row_flags, row_tmp over all rows
                (rows at or above 12 n_popped are what they were; row_tmp is what it was after a push_relax that ends on a win);
                heap_size, n_nodes, status, solved_idx, iterations, n_popped, new_count; claim, INT32_MAX everywhere; out_soa,
                queues and lengths, where every byte no launch writes is still the sentinel.
  open list     heap_cost[:size] (as uint64) / heap_idx[:size] sorted equals the model's heapq content, and the device array has
                the heap property under (cost, index).  Entries at or above `size` are the serial heap's leftovers: they are the
                only bytes inside an array that are not compared.  Pop order is compared exactly through `popped`.
  child_node    exact for a seen row (the node) and for a row that created a node (the new index); a row that lost the election
                for a new state holds -(h) - 1, and hash[h] must be the index of that row's state.  Once checked, the device's
                value is what the model keeps for that row.
  hash          which wave wins a slot decides the layout, so: no negative entry, the non-zero entries are exactly 1 .. n_nodes
                each once (a problem whose root is solved holds node 1 in its row although it reports no node: rc_astar_init
                writes the root before it looks at it), and every node is found by linear probing from key_hash(key) & mask
                without crossing an empty slot.

No NaN among the values: the reference's open list is a heapq of tuples, whose order under NaN depends on the sift algorithm, so
there is nothing to be equal to.
"""
import collections
import heapq

import numpy as np

from keys_model import home_cell, pack_keys
from lockstep_model import FILL, N_ACT, filled, near_roots, replant_list
from oracle import agents as oa
from oracle import cube as oc

INT_MAX = 2 ** 31 - 1
U32_MAX = 2 ** 32 - 1
RUNNING, SOLVED, EXHAUSTED, OPEN_EMPTY, ROOT_SOLVED = range(5)
PATH_UNSOLVED, PATH_NO_PROBLEM = -1, -3
PALETTE = np.array([-np.inf, -2.0, -0.0, 0.0, 0.5, 3.0, np.inf], dtype=np.float32)
SCALARS = ("heap_size", "n_nodes", "status", "solved_idx", "iterations", "n_popped", "new_count")
FILL_I8 = FILL - 256


def min_hash_size(C: int) -> int:
    """The smallest hash row check_astar admits: a power of two >= 2 (C + 1)."""
    return 1 << int(2 * (C + 1) - 1).bit_length()


class AStarModel:
    def __init__(self, B: int, N: int, C: int, hash_size: int, out_bytes: int = 0, list_len: int = 0, width: int = 1):
        """out_bytes: size of the out_soa allocation; list_len, width: rows and the widest row of the solutions table."""
        B, N, C, H = self.B, self.N, self.C, self.H = int(B), int(N), int(C), int(hash_size)
        assert C >= 12 * N + 1 and H & (H - 1) == 0 and H >= 2 * (C + 1)
        R = self.R = N_ACT * N
        self.keys = filled((B, C + 1, 4), np.uint32)
        self.G, self.parents = filled((B, C + 1), np.int32), filled((B, C + 1), np.int32)
        self.parent_actions = filled((B, C + 1), np.uint8)
        self.claim = np.full((B, C + 1), INT_MAX, dtype=np.int32)
        self.heap = [[] for _ in range(B)]   # heapq lists of (cost, index): heap_cost / heap_idx below heap_size
        for name in SCALARS:
            setattr(self, name, filled((B,), np.int32))
        self.popped = filled((B, N), np.int32)
        self.child_keys = filled((B, R, 4), np.uint32)
        self.child_node, self.row_tmp = filled((B, R), np.int32), filled((B, R), np.int32)
        self.row_flags = filled((B, R), np.uint8)
        self.out_soa = filled((out_bytes,), np.int8)
        self.queues, self.lengths = filled((list_len * width,), np.uint8), filled((list_len,), np.int32)
        # bookkeeping, no device arrays
        self.states = np.zeros((B, C + 1, 20), dtype=np.int8)
        self.index = [{} for _ in range(B)]
        self.taken = np.zeros((B, H), dtype=bool)   # occupied hash slots: under linear probing the set does not depend on the order
        self.lost = np.zeros((B, R), dtype=bool)    # rows whose child_node the next `differences` checks through the hash row
        self.lost_idx = np.zeros((B, R), dtype=np.int32)
        self.count = collections.Counter()

    # ---- hashing, for the counters only ---------------------------------------------------------------------------------
    def _probe(self, b: int, home: int) -> int:
        """The first free slot of problem b's row from `home` on."""
        h = home
        while self.taken[b, h]:
            h = (h + 1) & (self.H - 1)
        return h

    def _start(self, b: int, root: np.ndarray) -> bool:
        """What rc_astar_init writes for a problem; the hash row is empty when it does."""
        state = (root.astype(np.int64) & 31).astype(np.int8)
        solved = bool(oc.is_solved(state))
        self.states[b, 1] = state
        self.keys[b, 1] = pack_keys(state[None])[0]
        self.taken[b] = False
        self.taken[b, home_cell(self.keys[b, 1:2], self.H)[0]] = True
        self.G[b, 1] = self.parents[b, 1] = self.parent_actions[b, 1] = 0
        self.index[b] = {} if solved else {state.tobytes(): 1}   # the reference returns before it inserts a solved root
        self.heap[b] = [] if solved else [(0.0, 1)]
        self.heap_size[b] = self.n_nodes[b] = 0 if solved else 1
        self.status[b] = ROOT_SOLVED if solved else RUNNING
        self.solved_idx[b] = -1
        self.iterations[b] = self.n_popped[b] = self.new_count[b] = 0
        return solved

    # ---- rc_astar_init --------------------------------------------------------------------------------------------------
    def init(self, roots: np.ndarray):
        for b in range(self.B):
            self.count["root_solved_at_init"] += self._start(b, roots[b])

    # ---- rc_astar_plant -------------------------------------------------------------------------------------------------
    def plant(self, slots, roots: np.ndarray):
        """roots[i] is column first_col + i of the caller's table."""
        for i, s in enumerate(np.asarray(slots).tolist()):
            if not 0 <= s < self.B:
                self.count["plant_skipped_bad_slot"] += 1
                continue
            self.count["replanted_over_larger_tenant"] += int(self.n_nodes[s] > 1)
            self.count["root_solved_at_plant"] += self._start(s, roots[i])

    # ---- rc_astar_pop_expand --------------------------------------------------------------------------------------------
    def pop_expand(self, max_states: int):
        N, C, c = self.N, self.C, self.count
        for b in range(self.B):
            self.new_count[b] = self.n_popped[b] = 0
            if self.status[b] != RUNNING:
                continue
            n, heap = int(self.n_nodes[b]), self.heap[b]
            if n + N_ACT * N > max_states or n + N_ACT * N > C:
                self.status[b] = EXHAUSTED
                c["exhausted_by_max_states" if n + N_ACT * N > max_states else "exhausted_by_capacity"] += 1
                c["exhausted_at_max_states_plus_1"] += int(n + N_ACT * N == max_states + 1)
                continue
            c["ran_at_max_states_exactly"] += int(n + N_ACT * N == max_states)
            c["ran_at_capacity_exactly"] += int(n + N_ACT * N == C)
            n_pop = min(len(heap), N)
            if n_pop == 0:
                self.status[b] = OPEN_EMPTY
                c["open_empty"] += 1
                continue
            c["open_list_shorter_than_N"] += int(n_pop < N)
            entries = [heapq.heappop(heap) for _ in range(n_pop)]
            costs = [e[0] for e in entries] + ([heap[0][0]] if heap else [])
            c["cost_tie_popped_by_index"] += int(any(x == y for x, y in zip(costs, costs[1:])))
            batch = np.array([e[1] for e in entries], dtype=int)
            self.popped[b, :n_pop] = batch
            self.heap_size[b] = len(heap)
            self.n_popped[b] = n_pop
            self.iterations[b] += 1
            rows = n_pop * N_ACT
            c["block_scan_per_%d" % -(-rows // 256)] += 1
            # ---- AStar._expand_batch up to the open-list pushes ----
            index = self.index[b]
            parent_of_row = np.repeat(batch, N_ACT)
            action_of_row = np.tile(np.arange(N_ACT), n_pop)
            children = oc.expand12(self.states[b, batch])
            keys = [k.tobytes() for k in children]
            seen = np.array([k in index for k in keys])
            first = np.zeros(rows, dtype=bool)
            first_row = {}
            for r, k in enumerate(keys):
                if k not in first_row:
                    first_row[k] = r
                    first[r] = True
            first_seen, first_unseen = first & seen, first & ~seen
            new_idx = n + 1 + np.arange(int(first_unseen.sum()))
            for k, i in zip((k for k, f in zip(keys, first_unseen) if f), new_idx):
                index[k] = int(i)
            child_idx = np.array([index[k] for k in keys])
            self.states[b, new_idx] = children[first_unseen]
            new_parent = parent_of_row[first_unseen]
            self.G[b, new_idx] = self.G[b, new_parent] + 1
            self.parent_actions[b, new_idx] = action_of_row[first_unseen]
            self.parents[b, new_idx] = new_parent
            # ---- the staging the header names ----
            packed = pack_keys(children)
            self.child_keys[b, :rows] = packed
            self.keys[b, new_idx] = packed[first_unseen]
            self.row_flags[b, :rows] = first_unseen + 2 * first_seen
            self.n_nodes[b] = n + len(new_idx)
            self.new_count[b] = len(new_idx)
            lost = ~seen & ~first
            c["duplicate_new_state_same_parent_batch"] += int(lost.sum())
            c["seen_node_reached_by_two_rows"] += int((seen & ~first).sum())
            # hashing: where the read-only probe of a new state stops in the row as it was before the launch
            mask = self.H - 1
            homes = home_cell(packed[first_unseen], self.H).tolist()
            stops = [self._probe(b, h) for h in homes]
            c["two_new_states_one_probe_stop"] += len(stops) - len(set(stops))
            c["probe_wrapped"] += sum(s < h for s, h in zip(stops, homes))
            c["probe_length_ge_3"] += sum(((s - h) & mask) >= 2 for s, h in zip(stops, homes))
            slot_of = {}
            for i, h in zip(new_idx.tolist(), homes):
                slot_of[i] = self._probe(b, h)
                self.taken[b, slot_of[i]] = True
            self.child_node[b, :rows] = np.where(lost, [-slot_of.get(i, 0) - 1 for i in child_idx.tolist()], child_idx)
            self.lost[b] = False
            self.lost[b, :rows] = lost
            self.lost_idx[b, :rows] = child_idx

    # ---- rc_astar_gather_new --------------------------------------------------------------------------------------------
    def gather_new(self, new_offset: np.ndarray, stride: int):
        """The caller hands over an out_soa of nothing but sentinel bytes."""
        self.out_soa[:] = FILL_I8
        for b in np.flatnonzero(self.new_count).tolist():
            cnt, n = int(self.new_count[b]), int(self.n_nodes[b])
            col = int(new_offset[b])
            assert col + cnt <= stride and 20 * stride <= len(self.out_soa)
            self.out_soa[:20 * stride].reshape(20, stride)[:, col:col + cnt] = self.states[b, n - cnt + 1:n + 1].T

    def new_states(self, b: int) -> np.ndarray:
        cnt, n = int(self.new_count[b]), int(self.n_nodes[b])
        return self.states[b, n - cnt + 1:n + 1]

    # ---- rc_astar_push_relax --------------------------------------------------------------------------------------------
    def push_relax(self, new_offset: np.ndarray, values: np.ndarray, lambda_: float):
        values, c = np.asarray(values, dtype=np.float32), self.count
        lam = np.float64(lambda_)
        for b in np.flatnonzero(self.n_popped).tolist():
            n_pop, cnt, n = int(self.n_popped[b]), int(self.new_count[b]), int(self.n_nodes[b])
            G, parents, parent_actions = self.G[b], self.parents[b], self.parent_actions[b]
            new_idx = n - cnt + 1 + np.arange(cnt)
            h = -values[int(new_offset[b]):int(new_offset[b]) + cnt]
            assert not np.isnan(h).any()
            cost = lam * G[new_idx].astype(np.float64) + h.astype(np.float64)   # AStar.cost: two roundings
            for x, i in zip(cost.tolist(), new_idx.tolist()):
                heapq.heappush(self.heap[b], (x, i))
            self.heap_size[b] = len(self.heap[b])
            rows = n_pop * N_ACT
            first_seen = self.row_flags[b, :rows] == 2
            state_idx = self.child_node[b, :rows][first_seen].astype(int)
            parent_idx = np.repeat(self.popped[b, :n_pop], N_ACT)[first_seen].astype(int)
            actions = np.tile(np.arange(N_ACT), n_pop)[first_seen]
            won = np.flatnonzero(oc.multi_is_solved(self.states[b, new_idx]))
            if len(won):   # the win check is on the new states only, and the reference returns before it relaxes
                self.status[b] = SOLVED
                self.solved_idx[b] = new_idx[won[0]]
                assert len(won) == 1   # new states are distinct
                pending = (G[parent_idx] + 1 < G[state_idx]).any() or (G[state_idx] + 1 < G[parent_idx]).any()
                c["win_with_relaxations_pending"] += int(pending)
                continue
            row_of = np.flatnonzero(first_seen)
            # ---- AStar._relax_seen, literally ----
            better = G[parent_idx] + 1 < G[state_idx]
            s, p = state_idx[better], parent_idx[better]
            c["relax_case1"] += int(better.sum())
            c["relax_target_is_also_a_popped_parent"] += int(np.isin(s, parent_idx).sum())
            # rows of a popped parent that case 1 is about to lower, which compare otherwise with its new G than with the G
            # they gathered: what they write depends on gather-before-scatter
            for ra, sa, ga in zip(row_of[better].tolist(), s.tolist(), (G[p] + 1).tolist()):
                rb = row_of[(parent_idx == sa) & ((G[sa] + 1 < G[state_idx]) != (ga + 1 < G[state_idx]))]
                c["case1_outcome_depends_on_gather_before_scatter"] += len(rb)
                c["case1_writer_and_reader_in_different_waves"] += int(((rb % 256) // 64 != (ra % 256) // 64).sum())
                c["case1_reader_in_a_later_pass"] += int((rb // 256 > ra // 256).sum())
            G[s] = G[p] + 1
            parent_actions[s] = actions[better]
            parents[s] = p

            shortcut = G[state_idx] + 1 < G[parent_idx]
            s, p = state_idx[shortcut], parent_idx[shortcut]
            c["relax_case2"] += int(shortcut.sum())
            c["case2_parent_claimed_by_two_rows"] += len(p) - len(set(p.tolist()))
            c["case2_row_0"] += int(shortcut.any() and row_of[shortcut][0] == 0)
            c["relax_target_is_also_a_popped_parent"] += int(np.isin(p, state_idx).sum())
            # rows whose seen child is a popped parent that case 2 is about to lower, likewise
            for ra, pa, ga in zip(row_of[shortcut].tolist(), p.tolist(), (G[s] + 1).tolist()):
                rb = row_of[(state_idx == pa) & ((G[pa] + 1 < G[parent_idx]) != (ga + 1 < G[parent_idx]))]
                c["case2_outcome_depends_on_gather_before_scatter"] += len(rb)
                c["case2_writer_and_reader_in_different_waves"] += int(((rb % 256) // 64 != (ra % 256) // 64).sum())
                c["case2_reader_in_a_later_pass"] += int((rb // 256 > ra // 256).sum())
            self.row_tmp[b, :rows] = 0
            self.row_tmp[b, row_of[shortcut]] = G[s] + 1
            G[p] = G[s] + 1
            parent_actions[p] = oa._REV[actions[shortcut]]
            parents[p] = s

    # ---- rc_astar_solutions ---------------------------------------------------------------------------------------------
    def solutions(self, problems, width: int):
        """The caller hands over `queues` and `lengths` of nothing but sentinel bytes; the table's rows are `width` bytes."""
        self.queues[:], self.lengths[:] = FILL, filled((1,), np.int32)[0]
        table = self.queues
        assert len(problems) * width <= len(table)
        for i, b in enumerate(np.asarray(problems).tolist()):
            if not 0 <= b < self.B:
                self.lengths[i] = PATH_NO_PROBLEM
                self.count["solutions_skipped_bad_problem"] += 1
            elif self.status[b] != SOLVED:
                self.lengths[i] = 0 if self.status[b] == ROOT_SOLVED else PATH_UNSOLVED
            else:
                queue, x = [], int(self.solved_idx[b])
                while x != 1:   # AStar.resume
                    assert len(queue) < self.n_nodes[b]
                    queue.insert(0, int(self.parent_actions[b, x]))
                    x = int(self.parents[b, x])
                self.lengths[i] = len(queue)
                if len(queue) <= width:
                    table[i * width:i * width + len(queue)] = queue
                    self.count["solution_written"] += 1
                    self.count["solution_of_two_or_more_written"] += int(len(queue) >= 2)
                else:
                    self.count["solution_longer_than_width"] += 1

    def write(self, name: str, index: int, value: int):
        """A hand-made change of one entry of a per-problem scalar; an emptied open list is emptied here too."""
        getattr(self, name)[index] = value
        if name == "heap_size":
            assert value == 0
            self.heap[index] = []

    # ---- what the reference's attributes would be ---------------------------------------------------------------------------
    def problem(self, b: int) -> dict:
        n = int(self.n_nodes[b])
        queue, x = [], int(self.solved_idx[b]) if self.status[b] == SOLVED else 1
        while x != 1:
            queue.insert(0, int(self.parent_actions[b, x]))
            x = int(self.parents[b, x])
        return {"n": n, "states": self.states[b, :n + 1], "G": self.G[b, :n + 1], "parents": self.parents[b, :n + 1],
                "parent_actions": self.parent_actions[b, :n + 1], "open": sorted(self.heap[b]),
                "solved": bool(self.status[b] in (SOLVED, ROOT_SOLVED)), "queue": queue, "status": int(self.status[b])}

    # ---- comparison with the device -------------------------------------------------------------------------------------------
    def differences(self, dev: dict) -> list:
        """Names of the arrays of `dev` (name -> host copy of the flat device array) that are not the model's by the rules of the
        module docstring.  A lost row's child_node that passes its check is adopted, see there."""
        B, C, H, out = self.B, self.C, self.H, []
        same = lambda mine, theirs: np.array_equal(mine.reshape(-1), theirs.reshape(-1).view(mine.dtype))   # noqa: E731
        for name in ("G", "parents", "parent_actions", "keys", "claim", "popped", "child_keys", "row_flags", "row_tmp", "out_soa",
                     "queues", "lengths") + SCALARS:
            if name in dev and not same(getattr(self, name), dev[name]):
                out.append(name)
        # hash
        tab = dev["hash"].reshape(B, H).astype(np.int64)
        n = np.where(self.status == ROOT_SOLVED, 1, self.n_nodes).astype(np.int64)
        pb, slot = np.nonzero(tab)
        node = tab[pb, slot]
        ok = (tab >= 0).all() and np.array_equal((tab != 0).sum(axis=1), n) and (node <= n[pb]).all() \
            and len(np.unique(pb * (C + 2) + node)) == len(node)
        if ok and len(node):
            mask = H - 1
            home = home_cell(self.keys[pb, node], H)
            dist = (slot - home) & mask
            for k in range(int(dist.max())):
                far = dist > k
                ok = ok and (tab[pb[far], (home[far] + k) & mask] != 0).all()
        if not ok:
            out.append("hash")
        # child_node
        theirs = dev["child_node"].reshape(B, self.R).copy()
        lb, lr = np.nonzero(self.lost)
        if len(lb):
            h = -theirs[lb, lr].astype(np.int64) - 1
            good = (h >= 0) & (h < H)
            good[good] = tab[lb[good], h[good]] == self.lost_idx[lb[good], lr[good]]
            self.child_node[lb[good], lr[good]] = theirs[lb[good], lr[good]]
            self.lost[lb[good], lr[good]] = False
        if not np.array_equal(self.child_node, theirs):
            out.append("child_node")
        # open list
        cost = dev["heap_cost"].reshape(B, C + 1).view(np.uint64)
        idx = dev["heap_idx"].reshape(B, C + 1)
        size = np.array([len(h) for h in self.heap])
        if "heap_size" not in out:
            live = np.arange(C + 1)[None, :] < size[:, None]
            pb, j = np.nonzero(live)
            fc, fi = cost[pb, j].view(np.float64), idx[pb, j]
            order = np.lexsort((fi, fc, pb))
            mine = [e for h in self.heap for e in sorted(h)]
            mine_cost = np.array([e[0] for e in mine], dtype=np.float64)
            mine_idx = np.array([e[1] for e in mine], dtype=np.int32)
            if not (np.array_equal(fc[order].view(np.uint64), mine_cost.view(np.uint64)) and np.array_equal(fi[order], mine_idx)):
                out.append("heap_cost/heap_idx")
            child = j >= 1
            up = (j[child] - 1) // 2
            cc, ci = fc[child], fi[child]
            uc, ui = cost[pb[child], up].view(np.float64), idx[pb[child], up]
            if ((cc < uc) | ((cc == uc) & (ci < ui))).any():
                out.append("heap property")
        return out


# =====================================================================================================================
# device memory with guards
# =====================================================================================================================
def astar_arena(m: AStarModel, device="cuda"):
    """(Arena, filled astar_device._AsStruct) for the model's shapes: sentinel everywhere, claim INT32_MAX, the hash rows zero."""
    from librubiks.solving.astar_device import _AsStruct
    from lockstep_model import Arena
    B, C, N, H, R = m.B, m.C, m.N, m.H, m.R
    rows = B * (C + 1)
    arena = Arena([("keys", np.uint32, (rows, 4)), ("G", np.int32, (rows,)), ("parents", np.int32, (rows,)),
                   ("parent_actions", np.uint8, (rows,)), ("claim", np.int32, (rows,)), ("hash", np.int32, (B, H)),
                   ("heap_cost", np.float64, (rows,)), ("heap_idx", np.int32, (rows,))] +
                  [(name, np.int32, (B,)) for name in SCALARS] +
                  [("popped", np.int32, (B, N)), ("child_keys", np.uint32, (B * R, 4)), ("child_node", np.int32, (B, R)),
                   ("row_tmp", np.int32, (B, R)), ("row_flags", np.uint8, (B, R)), ("out_soa", np.int8, m.out_soa.shape),
                   ("queues", np.uint8, m.queues.shape), ("lengths", np.int32, m.lengths.shape)], device)
    arena.write("claim", slice(None), INT_MAX)
    arena.write("hash", slice(None), 0)
    s = _AsStruct()
    s.n_problems, s.capacity, s.hash_size, s.expansions = B, C, H, N
    for name, _ in _AsStruct._fields_[4:]:
        setattr(s, name, arena.ptr(name))
    return arena, s


# =====================================================================================================================
# the scenarios: launch sequences generated beside the model (they read nothing but the model's state)
# =====================================================================================================================
LAMBDAS = (0.0, 0.2, 1.0, 0.5)   # 0.2: its product with G is inexact, a fused multiply-add would show; 0.5 ties with the palette


def offsets(m: AStarModel) -> np.ndarray:
    """The exclusive prefix sum of new_count (B + 1 entries), which the header leaves to the caller."""
    return np.concatenate([[0], np.cumsum(m.new_count)]).astype(np.int32)


def out_stride(total: int, slack: int) -> int:
    return max(16, (total + 15) // 16 * 16) + slack


WIDE = 16   # bytes a row of the solutions table may have: no scenario runs that many iterations, and a queue is no longer


def make_model(B: int, N: int, C: int, slack: int) -> AStarModel:
    return AStarModel(B, N, C, min_hash_size(C), out_bytes=20 * out_stride(B * N_ACT * N, slack), list_len=B + 2, width=WIDE)


def _read_queues(m: AStarModel, problems: np.ndarray):
    """rc_astar_solutions twice: with rows of one byte, so that longer queues report their length and leave their row alone,
    and with rows that hold the longest queue, odd if it can be, so that row i starts at an odd offset."""
    yield {"op": "solutions", "problems": problems, "width": 1}
    longest = max([len(m.problem(b)["queue"]) for b in range(m.B)] + [2])
    assert longest + 1 <= WIDE
    yield {"op": "solutions", "problems": problems, "width": longest + (longest % 2 == 0)}


def _iteration(m: AStarModel, max_states: int, lam: float, slack: int, values_of):
    """pop, gather, push; values_of(offsets) is asked once the pop has run on the model."""
    yield {"op": "pop", "max_states": int(max_states)}
    off = offsets(m)
    yield {"op": "gather", "new_offset": off, "stride": out_stride(int(off[-1]), slack)}
    yield {"op": "push", "new_offset": off, "values": values_of(off), "lambda": lam}


def _all_with_strays(rng, B: int) -> np.ndarray:
    """Every problem in random order with -1 and B among them."""
    problems = rng.permutation(B).tolist()
    for bad in (-1, B):
        problems.insert(rng.randint(0, len(problems) + 1), bad)
    return np.array(problems, dtype=np.int32)


# (B, N, C) -> (max_states per iteration: None = unbounded, "eq" = a running problem of median size sits on n + 12 N == max_states,
#               "plus1" = it sits on max_states + 1; the iteration after which queues are read and slots planted again)
SEEDED_CASES = {
    (1, 1, 13): (("eq", None, None, None), 1),
    (5, 2, 63): ((None, "eq", None, "plus1", None, None, None), 2),
    (37, 5, 255): ((None, None, "eq", "plus1", None, None, "eq", None), 3),
    (3, 22, 1023): ((None,) * 7 + ("eq", "plus1"), 3),
    (3, 43, 2047): ((None,) * 7 + ("eq", "plus1"), 3),
    (1027, 1, 31): ((None, "eq", "plus1", None, None), 1),
}
# the counters a seeded case is meant to reach under every lambda (the scripted searches reach the relaxations, the pending win,
# the emptied open list); block_scan_per_k: a launch whose 12 n_popped rows need k rows a lane in the block-wide scan
_BOUNDS = ("ran_at_max_states_exactly", "exhausted_by_max_states", "exhausted_at_max_states_plus_1", "exhausted_by_capacity")
_SLOTS = ("plant_skipped_bad_slot", "solutions_skipped_bad_problem", "replanted_over_larger_tenant", "solution_written")
_ROWS = ("open_list_shorter_than_N", "cost_tie_popped_by_index", "seen_node_reached_by_two_rows", "two_new_states_one_probe_stop",
         "probe_length_ge_3")
SEEDED_WANTED = {
    (1, 1, 13): ("ran_at_max_states_exactly", "ran_at_capacity_exactly", "exhausted_by_capacity", "replanted_over_larger_tenant",
                 "solutions_skipped_bad_problem"),
    (5, 2, 63): _BOUNDS + _SLOTS + _ROWS,
    (37, 5, 255): _BOUNDS + _SLOTS + _ROWS + ("duplicate_new_state_same_parent_batch", "probe_wrapped", "solution_longer_than_width",
                                              "solution_of_two_or_more_written", "root_solved_at_init"),
    (3, 22, 1023): _BOUNDS + _SLOTS + _ROWS + ("duplicate_new_state_same_parent_batch", "block_scan_per_2"),
    (3, 43, 2047): _BOUNDS + _SLOTS + _ROWS + ("duplicate_new_state_same_parent_batch", "block_scan_per_3"),
    (1027, 1, 31): _BOUNDS + _SLOTS + ("cost_tie_popped_by_index", "two_new_states_one_probe_stop", "probe_length_ge_3", "probe_wrapped",
                                       "solution_longer_than_width", "solution_of_two_or_more_written", "root_solved_at_init",
                                       "root_solved_at_plant"),
}
# (B, N, C) -> seed per lambda, chosen on the CPU: tests/test_astar_model.py::test_the_seeded_scenarios_reach_their_branches
SEEDS = {(1, 1, 13): (1001, 2001, 3001, 4001), (5, 2, 63): (1010, 2005, 3008, 4005), (37, 5, 255): (1037, 2037, 3037, 4037),
         (3, 22, 1023): (1004, 2007, 3015, 4003), (3, 43, 2047): (1004, 2007, 3011, 4003), (1027, 1, 31): (2027, 3027, 4027, 5027)}
SLACK = {0.0: 0, 0.2: 16, 1.0: 0, 0.5: 16}   # out_soa: the smallest stride that holds the new states, and 16 columns more


def seeded_roots(rng, n: int, far_share: float) -> np.ndarray:
    """One to three moves from solved, with duplicates and solved roots among them; far_share of them ten moves away."""
    roots = near_roots(rng, n, 0.08 if n >= 3 else 0.0)
    third = np.flatnonzero(rng.random_sample(n) < 0.3)
    roots[third] = oc.multi_rotate_actions(roots[third], rng.randint(0, N_ACT, len(third)))
    far = np.flatnonzero(rng.random_sample(n) < far_share)
    roots[far] = near_roots(rng, len(far), 0.0, far=True)
    return roots.astype(np.int8)


def seeded_scenario(m: AStarModel, seed: int, lam: float, slack: int):
    """Yields the launches one by one; the caller applies each to the model (and to the device) before asking for the next."""
    rng = np.random.RandomState(seed)
    B, N = m.B, m.N
    schedule, read_after = SEEDED_CASES[B, N, m.C]
    far = 0.5 if N >= 5 else 0.2   # wide searches near the solved cube end at once
    palette = lambda off: PALETTE[rng.randint(0, len(PALETTE), int(off[-1]))]   # noqa: E731
    yield {"op": "init", "roots": seeded_roots(rng, B, far)}
    for t, bound in enumerate(schedule):
        sizes = np.sort(m.n_nodes[m.status == RUNNING])
        if bound is None or not len(sizes):
            max_states = U32_MAX
        else:
            max_states = int(sizes[len(sizes) // 2]) + N_ACT * N - (bound == "plus1")
        yield from _iteration(m, max_states, lam, slack, palette)
        if t == read_after:
            yield from _read_queues(m, _all_with_strays(rng, B))
            slots = replant_list(rng, np.flatnonzero(m.status != RUNNING), B)
            yield {"op": "plant", "slots": slots, "roots": seeded_roots(rng, len(slots), far), "first_col": 16}
    yield from _iteration(m, 0, lam, slack, palette)   # whoever still runs ends here
    assert not (m.status == RUNNING).any()
    yield {"op": "pop", "max_states": U32_MAX}   # nobody runs: only new_count and n_popped may be written
    yield from _read_queues(m, _all_with_strays(rng, B))


# ---- scripted searches: one script a problem, values chosen per state ----------------------------------------------------------
ACT = {name: i for i, name in enumerate(("F", "F'", "B", "B'", "U", "U'", "D", "D'", "L", "L'", "R", "R'"))}


def after(state: np.ndarray, moves: str) -> np.ndarray:
    for name in moves.split():
        state = oc.rotate(state, *oc.ACTION_SPACE[ACT[name]])
    return state


_START = "F U R' D L B' U F"      # far from solved: no scripted search meets the solved cube by accident
_CHAIN = (("R", 100.0), ("R R", 90.0), ("R R L", 80.0))   # R R L creates R R L R = R' L with G 4
# name -> (N, moves from the solved cube to the root, ((moves from the root, value) ...), iterations, counters it reaches,
#          iteration after which the open list is emptied by hand or None)
# Values are spaced wider than lambda * G, so the named states are popped in the order of their values under every lambda; the
# other states get -100.
SCRIPTS = {
    # ... R' is popped with G 1: its child R' L is seen with G 4 -> case 1
    "case1": (1, _START, _CHAIN + (("R'", 70.0),), 5, ("relax_case1",), None),
    # ... R' L is popped with G 4: its children R' (row 9) and L (row 10) are seen with G 1 -> case 2 from two rows, the larger
    # stands; its child R' L F' is created with G 5 and popped: row 0 leads back to R' L with G 2 -> case 2 from row 0
    "case2": (1, _START, _CHAIN + (("R' L", 70.0), ("R' L F'", 60.0)), 6,
              ("relax_case2", "case2_parent_claimed_by_two_rows", "case2_row_0"), None),
    # the root is R' F from solved: when R' is popped, R' L waits for case 1 and R' F is the solved cube
    "win": (1, "F' R", _CHAIN + (("R'", 70.0),), 5, ("win_with_relaxations_pending", "solution_longer_than_width",
                                                       "solution_of_two_or_more_written"), None),
    "open_empty": (1, _START, (("R", 100.0),), 3, ("open_empty",), 1),
    "root_solved": (1, "", (), 1, ("root_solved_at_init",), None),
    # R and L are popped together (equal cost, by index): both create R L, both lead back to the root
    "duplicate": (2, _START, (("R", 100.0), ("L", 100.0)), 2,
                  ("duplicate_new_state_same_parent_batch", "seen_node_reached_by_two_rows", "cost_tie_popped_by_index",
                   "open_list_shorter_than_N"), None),
    # a second chain on the other side of the cube fills the pairs; then R' (G 1) and R' L (G 4) are popped together: the G
    # that R' 's row writes is the G of the other popped parent, which that parent's rows read in the same pass
    "target_popped": (2, _START, (("R", 100.0), ("B", 95.0), ("R R", 90.0), ("B B", 85.0), ("R R L", 80.0), ("B B D", 75.0),
                                  ("R'", 70.0), ("R' L", 69.0)), 5, ("relax_case1", "relax_target_is_also_a_popped_parent"), None),
    "win2": (2, "F' R", (("R", 100.0), ("B", 95.0), ("R R", 90.0), ("B B", 85.0), ("R R L", 80.0), ("B B D", 75.0),
                         ("R'", 70.0), ("B B D D", 69.0)), 5, ("win_with_relaxations_pending",), None),
}


def _wide(last: tuple) -> tuple:
    """Searches with N 22: 264 child rows, so rows 256-263 -- actions 4 to 11 of the last popped parent -- are a second pass of
    the first wave's lanes, made while the other waves, which have one pass, go on.  Iteration 2 pops the root's twelve children.
    Iterations 3 to 6 pop U R, U R R, U R R L and U R R L L -- which creates U R' L and U R R L L with G 5, then U R R L L R =
    U R' L L with G 6 -- each with 21 states from the other side of the cube.  `last` names the seventh and the last state popped
    in iteration 7; twenty more from the other side come before and between them."""
    axis = lambda move: ACT[move] // 4   # noqa: E731  (F B | U D | L R)
    names = list(ACT)
    side = [a + " " + b for a in ("B", "B'", "D", "D'") for b in names if axis(b) != axis(a)][:21]
    valued = []
    for chain, value in (("U R", 160.0), ("U R R", 140.0), ("U R R L", 120.0), ("U R R L L", 100.0)):
        valued += [(chain, value)] + [(f, value) for f in side]
        side = [f + " " + next(x for x in ("F", "U", "R") if axis(x) != axis(f.split()[-1])) for f in side]   # a child of each
    valued += [(f, 80.0) for f in side[:6]] + [last[0]] + [(f, 65.0) for f in side[6:20]] + [last[1]]
    return tuple(valued)


SCRIPTS.update({
    # U R' (G 2) lowers G[U R' L] from 5 to 3 in case 1 (row 80, second wave); U R' L's row 260 leads to U R' L L with G 6:
    # 5 + 1 < 6 is false, as NumPy gathered it, 3 + 1 < 6 is true
    "order1": (22, _START, _wide((("U R'", 70.0), ("U R' L", 60.0))), 7,
               ("relax_case1", "relax_target_is_also_a_popped_parent", "case1_outcome_depends_on_gather_before_scatter",
                "case1_writer_and_reader_in_different_waves", "case1_reader_in_a_later_pass", "block_scan_per_2"), None),
    # U R' L (rows 81 and 82 claim it, 82 writes) gets G 3 in case 2; U R' L L (G 6) has it as a seen child in row 261:
    # 5 + 1 < 6 is false, 3 + 1 < 6 is true
    "order2": (22, _START, _wide((("U R' L", 70.0), ("U R' L L", 60.0))), 7,
               ("relax_case2", "case2_parent_claimed_by_two_rows", "case2_outcome_depends_on_gather_before_scatter",
                "case2_writer_and_reader_in_different_waves", "case2_reader_in_a_later_pass", "block_scan_per_2"), None),
})
SCRIPTED_CASES = {1: 127, 2: 255, 22: 2047}   # N -> C
DEFAULT_VALUE = np.float32(-100.0)


def scripts_for(N: int) -> list:
    names = [k for k, v in SCRIPTS.items() if v[0] == N]
    if N == 22:   # what a kernel without a barrier would write there hangs on the waves' timing: every workgroup is a chance
        return names * 4
    return names + names[:1]   # (the first once more: two problems with the same search)


def scripted_model(N: int, slack: int) -> AStarModel:
    return make_model(len(scripts_for(N)), N, SCRIPTED_CASES[N], slack)


def scripted_scenario(m: AStarModel, lam: float, slack: int):
    names = scripts_for(m.N)
    roots, tables = [], []
    for name in names:
        _, start, valued, _, _, _ = SCRIPTS[name]
        root = after(oc.get_solved(), start)
        roots.append(root)
        tables.append({after(root, moves).tobytes(): np.float32(v) for moves, v in valued})

    def values_of(off):
        values = np.full(int(off[-1]), DEFAULT_VALUE, dtype=np.float32)
        for b, table in enumerate(tables):
            for i, state in enumerate(m.new_states(b)):
                values[off[b] + i] = table.get(state.tobytes(), DEFAULT_VALUE)
        return values

    yield {"op": "init", "roots": np.array(roots, dtype=np.int8)}
    for t in range(max(SCRIPTS[name][3] for name in names)):
        yield from _iteration(m, U32_MAX, lam, slack, values_of)
        for b, name in enumerate(names):
            if SCRIPTS[name][5] == t + 1:
                yield {"op": "write", "name": "heap_size", "index": b, "value": 0}
        # a script that is over goes on with the other states, all of the same value: cost ties, popped by index
    yield from _read_queues(m, np.arange(m.B, dtype=np.int32))


def scripted_wanted(N: int) -> tuple:
    return tuple(sorted({k for name in scripts_for(N) for k in SCRIPTS[name][4]}))


def apply(m: AStarModel, launch: dict):
    op = launch["op"]
    if op == "init":
        m.init(launch["roots"])
    elif op == "plant":
        m.plant(launch["slots"], launch["roots"])
    elif op == "pop":
        m.pop_expand(launch["max_states"])
    elif op == "gather":
        m.gather_new(launch["new_offset"], launch["stride"])
    elif op == "push":
        m.push_relax(launch["new_offset"], launch["values"], launch["lambda"])
    elif op == "solutions":
        m.solutions(launch["problems"], launch["width"])
    else:
        m.write(launch["name"], launch["index"], launch["value"])
