"""
One-step agents recorded from the IMPORTED REFERENCE (librubiks/solving/agents.py RandomSearch, PolicySearch greedy and sampled,
ValueSearch) driven by tests/standin_net.StandInNet, every game right after np.random.seed(game seed).  Run like make_golden.py, with
the reference's checkout first on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg PYTHONPATH=<reference> python tests/golden/make_golden_rollout.py

The reference bounds these agents by wall time only (agents.py:30), so a game is recorded up to its 64th move: whether it was
solved within 64 moves, and its first <= 64 actions.  Only arrays are written (tests/golden/rollout_golden.npz).
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from standin_net import StandInNet  # noqa: E402

CAP = 64
DEPTHS, SEEDS = (1, 2, 3), range(100)


def sampled_margins(net, cube, state, seed, actions):
    """Smallest |u - cdf edge| over the game's moves, recomputed from RandomState(seed).random_sample: how far the closest
    draw was from choosing another action.  Asserts that the recomputation takes the reference's actions."""
    rs = np.random.RandomState(seed)
    margin = np.inf
    for a in actions:
        with torch.no_grad():
            p = torch.nn.functional.softmax(net(cube.as_oh(state), value=False).cpu(), dim=1).numpy().squeeze()
        cdf = p.astype(np.float64).cumsum()
        cdf /= cdf[-1]
        u = rs.random_sample()
        assert int(cdf.searchsorted(u, side="right")) == a
        margin = min(margin, float(np.abs(cdf - u).min()))
        state = cube.rotate(state, *cube.action_space[a])
    return margin


def make_rollout():
    from librubiks import cube
    from librubiks.solving.agents import PolicySearch, RandomSearch, ValueSearch
    torch.set_num_threads(1)
    net = StandInNet(seed=0)
    agents = {"random": lambda: RandomSearch(), "greedy": lambda: PolicySearch(net), "sampled": lambda: PolicySearch(net, sample_policy=True),
              "value": lambda: ValueSearch(net)}
    states, seeds = [], []
    for depth in DEPTHS:
        for seed in SEEDS:
            np.random.seed(1000 * depth + seed)
            states.append(cube.scramble(depth, True)[0])
            seeds.append(7000 + 1000 * depth + seed)
    fx = {"states": np.array(states), "seeds": np.array(seeds, dtype=np.int64)}
    for name, make in agents.items():
        solved, queues = [], []
        for state, seed in zip(states, seeds):
            agent = make()
            np.random.seed(seed)
            ok = agent.search(state, time_limit=0.15)
            q = list(agent.action_queue)
            ok = bool(ok) and len(q) <= CAP
            assert ok or len(q) >= CAP, (name, seed, len(q))   # an unsolved game made at least CAP moves in its time
            q = q[:CAP]
            solved.append(ok)
            queues.append(q + [-1] * (CAP - len(q)))
        fx[f"{name}_solved"], fx[f"{name}_queues"] = np.array(solved), np.array(queues, dtype=np.int16)
        print(name, "solved", int(np.sum(solved)), "of", len(solved))
    fx["sampled_margin"] = np.array([sampled_margins(net, cube, s, int(seed), [a for a in q if a >= 0])
                                     for s, seed, q in zip(states, seeds, fx["sampled_queues"])])
    print("sampled: margins under 1e-5:", int((fx["sampled_margin"] < 1e-5).sum()), "smallest", fx["sampled_margin"].min())
    path = os.path.join(OUT, "rollout_golden.npz")
    np.savez_compressed(path, **fx)
    print("rollout_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    make_rollout()
