"""
What a batch driven through rc_astar_pop_expand_each / rc_astar_push_relax_each must hold, launch by launch: problem b of a batch
whose staging has the row stride Nmax evolves exactly as the single problem of its own AStarModel(1, N_b, C, ...) (tests/
astar_model.py, pinned to oracle.agents.AStar by tests/test_astar_model.py) that is fed the same root, the same values and
lambda[b].  A plain module: tests/test_astar_each_model.py runs the scenarios on the models alone (the seeds are chosen there, on the
CPU), tests/test_astar_each_kernels_gpu.py compares the kernels with them after every launch.

`EachPool.differences` hands every model its problem's slices of the arena -- all C + 1 node rows, the scalars, popped[:N_b], the
staging rows [:12 N_b], the hash row, the open list -- and requires popped[N_b:] and the staging rows [12 N_b:] to be what no
launch of this problem's tenant wrote: the sentinel, or, after a slot was planted again with a smaller N, the rows its former
tenant left there.
"""
import collections

import numpy as np

import astar_model as am
from lockstep_model import N_ACT, filled, near_roots

NS = (1, 22, 2, 22)         # Nmax 22: 264 child rows, a second pass of the 256-thread stride; a 1 beside a 22
LAMBDAS = am.LAMBDAS        # (0.0, 0.2, 1.0, 0.5)
CAPACITY = 511              # the third pop of an N 22 problem (about 140 nodes + 264) fits, the fourth does not
STAGING = (("popped", 1), ("child_keys", N_ACT), ("child_node", N_ACT), ("row_tmp", N_ACT), ("row_flags", N_ACT))
NODE_ROWS = ("keys", "G", "parents", "parent_actions", "claim")


class EachPool:
    def __init__(self, Ns=NS, lambdas=LAMBDAS, C: int = CAPACITY):
        self.B, self.C, self.H, self.Nmax = len(Ns), int(C), am.min_hash_size(C), max(Ns)
        self.N, self.lam = [int(n) for n in Ns], [float(x) for x in lambdas]
        self.models = [am.AStarModel(1, n, C, self.H) for n in self.N]
        self.shell = am.make_model(self.B, self.Nmax, C, 0)   # the arena's shapes (am.astar_arena); never run
        self.rest = {name: getattr(self.shell, name).copy() for name, _ in STAGING}   # what rows at or above N_b / 12 N_b hold
        self.count = collections.Counter()

    def counters(self) -> collections.Counter:
        return sum((m.count for m in self.models), collections.Counter()) + self.count

    def expansions(self) -> np.ndarray:
        return np.array(self.N, dtype=np.int32)

    def lambdas(self) -> np.ndarray:
        return np.array(self.lam, dtype=np.float64)

    def scalar(self, name: str) -> np.ndarray:
        return np.array([int(getattr(m, name)[0]) for m in self.models], dtype=np.int32)

    def offsets(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.scalar("new_count"))]).astype(np.int32)

    # ---- the launches -----------------------------------------------------------------------------------------------------------
    def apply(self, launch: dict):
        op = launch["op"]
        if op == "init":
            for b, m in enumerate(self.models):
                m.init(launch["roots"][b:b + 1])
        elif op == "pop":
            before = self.counters()
            for b, m in enumerate(self.models):
                n_b = int(np.clip(launch["expansions"][b], 0, self.Nmax))   # what the header says the kernel reads
                if n_b == self.N[b]:
                    m.pop_expand(launch["max_states"])
                else:   # a clamped 0: nothing is popped, the open list "ran dry"
                    assert n_b == 0 and m.status[0] == am.RUNNING and m.n_nodes[0] <= min(launch["max_states"], self.C)
                    m.write("n_popped", 0, 0), m.write("new_count", 0, 0), m.write("status", 0, am.OPEN_EMPTY)
                    self.count["clamped_to_0_ends_open_empty"] += 1
                    self.count["negative_read_as_0"] += int(launch["expansions"][b] < 0)
                if launch["expansions"][b] > self.Nmax and m.n_popped[0] == self.Nmax:
                    self.count["clamped_to_Nmax_pops_Nmax"] += 1
            after = self.counters()
            gained = lambda k: after[k] > before[k]   # noqa: E731
            self.count["eq_and_plus1_in_one_launch"] += int(gained("ran_at_max_states_exactly") and gained("exhausted_at_max_states_plus_1"))
        elif op == "push":
            off = launch["new_offset"]
            for b, m in enumerate(self.models):
                cnt = int(m.new_count[0])
                m.push_relax(np.array([0, cnt]), launch["values"][off[b]:off[b] + cnt], launch["lambda"][b])
        elif op == "plant":
            for i, s in enumerate(launch["slots"].tolist()):
                self._replant(s, launch["roots"][i], launch["N"][i], launch["lam"][i])
        else:
            raise ValueError(op)

    def _replant(self, s: int, root: np.ndarray, n_new: int, lam_new: float):
        """Slot s goes to a tenant with its own (lambda, N): the new model starts from everything the old one leaves in the slot."""
        old, new = self.models[s], am.AStarModel(1, n_new, self.C, self.H)
        for name in NODE_ROWS + am.SCALARS:
            getattr(new, name)[:] = getattr(old, name)
        for name, per in STAGING:
            row = self.rest[name][s]
            row[:per * old.N] = getattr(old, name)[0]
            getattr(new, name)[0] = row[:per * n_new]
        self.count += old.count
        self.count["replanted_with_other_lambda_and_N"] += int(n_new != old.N and lam_new != self.lam[s])
        self.count["replanted_with_smaller_N"] += int(n_new < old.N)
        self.models[s], self.N[s], self.lam[s] = new, int(n_new), float(lam_new)
        new.plant([0], root[None])

    # ---- comparison with the device -------------------------------------------------------------------------------------------
    def differences(self, dev: dict) -> list:
        """dev: Arena.read() of am.astar_arena(self.shell)."""
        B, C, out = self.B, self.C, []
        per_node = lambda name: dev[name].reshape(B, C + 1, -1)   # noqa: E731
        for b, m in enumerate(self.models):
            view = {name: per_node(name)[b] for name in NODE_ROWS + ("heap_cost", "heap_idx")}
            view["hash"] = dev["hash"].reshape(B, self.H)[b]
            view.update({name: dev[name][b:b + 1] for name in am.SCALARS})
            for name, per in STAGING:
                rows = dev[name].reshape(B, per * self.Nmax, -1)[b]
                view[name] = rows[:per * m.N]
                if not np.array_equal(rows[per * m.N:].reshape(-1), self.rest[name][b].reshape(per * self.Nmax, -1)[per * m.N:].reshape(-1)):
                    out.append(f"problem {b}: {name} at or above its own N")
            out += [f"problem {b}: {what}" for what in m.differences(view)]
        return out


# =====================================================================================================================
# the scenarios (they read nothing but the models' state)
# =====================================================================================================================
def _bound_for_a_pair(pool: EachPool) -> int:
    """max_states such that, in the next pop, one running problem sits on n + 12 N_b == max_states (and runs) while another sits
    on max_states + 1 (and is exhausted); problems of different N first.  U32_MAX if there is no such pair."""
    need = {b: int(m.n_nodes[0]) + N_ACT * pool.N[b] for b, m in enumerate(pool.models) if m.status[0] == am.RUNNING}
    pairs = [(pool.N[a] == pool.N[c], a, c) for a in need for c in need if need[c] == need[a] + 1 and need[a] <= pool.C]
    if not pairs:
        return am.U32_MAX
    same_n, a, _ = min(pairs)
    pool.count["pair_at_the_bound_has_different_N"] += int(not same_n)
    return need[a]


def _iteration(pool: EachPool, rng, max_states: int, expansions=None):
    yield {"op": "pop", "max_states": int(max_states), "expansions": pool.expansions() if expansions is None else expansions}
    off = pool.offsets()
    yield {"op": "push", "new_offset": off, "values": am.PALETTE[rng.randint(0, len(am.PALETTE), int(off[-1]))], "lambda": pool.lambdas()}


REPLANT = {"after": 3, "slot": 3, "N": 3, "lam": 0.2}   # the former tenant ran with N 22 and lambda 0.5
ITERATIONS = 8
WANTED = ("ran_at_max_states_exactly", "exhausted_at_max_states_plus_1", "eq_and_plus1_in_one_launch", "pair_at_the_bound_has_different_N",
          "exhausted_by_capacity", "block_scan_per_2", "open_list_shorter_than_N", "cost_tie_popped_by_index",
          "duplicate_new_state_same_parent_batch", "seen_node_reached_by_two_rows", "replanted_over_larger_tenant",
          "replanted_with_other_lambda_and_N", "replanted_with_smaller_N")
SEED = 54   # chosen on the CPU: tests/test_astar_each_model.py


def seeded_scenario(pool: EachPool, seed: int):
    """Yields the launches one by one; the caller applies each to the pool (and to the device) before asking for the next."""
    rng = np.random.RandomState(seed)
    yield {"op": "init", "roots": am.seeded_roots(rng, pool.B, 0.75)}
    bounded = False
    for t in range(ITERATIONS):
        max_states = am.U32_MAX if bounded else _bound_for_a_pair(pool)
        bounded |= max_states != am.U32_MAX
        yield from _iteration(pool, rng, max_states)
        if t == REPLANT["after"]:
            yield {"op": "plant", "slots": np.array([REPLANT["slot"]], dtype=np.int32), "roots": near_roots(rng, 1, 0.0, far=True),
                   "first_col": 16, "N": [REPLANT["N"]], "lam": [REPLANT["lam"]]}
    yield from _iteration(pool, rng, 0)   # whoever still runs ends here
    assert not any(m.status[0] == am.RUNNING for m in pool.models)


CLAMP_WANTED = ("clamped_to_Nmax_pops_Nmax", "clamped_to_0_ends_open_empty", "negative_read_as_0", "block_scan_per_2")
CLAMP_SEED = 0


def clamp_scenario(pool: EachPool, seed: int):
    """Two iterations as they should be, then a pop that is handed Nmax + 1 for problem 1 (not the last problem: even a kernel that
    does not clamp stays inside the arena), then one that is handed 0 for problem 2, then one that is handed -1 for problem 0 (as an
    unsigned count that would be 2^32 - 1: the lower clamp makes it the 0 the header promises)."""
    rng = np.random.RandomState(seed)
    yield {"op": "init", "roots": near_roots(rng, pool.B, 0.0, far=True)}
    for _ in range(2):
        yield from _iteration(pool, rng, am.U32_MAX)
    assert all(m.status[0] == am.RUNNING for m in pool.models)
    over = pool.expansions()
    over[1] = pool.Nmax + 1
    yield from _iteration(pool, rng, am.U32_MAX, over)
    assert pool.models[2].status[0] == am.RUNNING
    none = pool.expansions()
    none[2] = 0
    yield from _iteration(pool, rng, am.U32_MAX, none)
    assert pool.models[2].status[0] == am.OPEN_EMPTY and pool.models[0].status[0] == am.RUNNING
    negative = pool.expansions()
    negative[0] = -1
    yield from _iteration(pool, rng, am.U32_MAX, negative)
    assert pool.models[0].status[0] == am.OPEN_EMPTY
