"""
librubiks.solving.hyper_optim on the CPU: the reference's own GridSearch test restated (tests/test_hyper_optim.py:17-21), the grid
enumeration and its order against the formula of the reference's hyper_optim.py:96-99, and the two score forms of :60-66 on
hand-made results.  The reference module cannot be imported where `bayes_opt` is missing, so the expected values come from the
formulas, not from a recording.
"""
import importlib.util

import numpy as np
import pytest

import conftest  # noqa: F401
from librubiks.solving.hyper_optim import BayesianOptimizer, GridSearch, Optimizer, grid_points, score_of


def f(params):
    return -params["x"] + 42, np.empty(5), np.empty(5)


def test_GS():
    gs = GridSearch(f, {"x": (0, 42)})
    gs.optimize(2)
    assert len(gs.score_history) == 2
    assert gs.highscore >= gs.score_history[1]
    assert gs.score_history == [42.0, 0.0] and gs.optimal == {"x": 0.0} and gs.highscore == 42.0
    assert gs.parameter_history == [{"x": 0.0}, {"x": 42.0}]


def _formula(parameters: dict, iterations: int) -> list:
    """hyper_optim.py:96-99,102-104, spelt out with explicit loops."""
    k = len(parameters)
    n = int(iterations ** (1 / k) + 1e-6)
    spaces = [np.linspace(lo, hi, n) for lo, hi in parameters.values()]
    points, index = [], [0] * k
    for _ in range(n ** k):
        points.append({kw: spaces[j][index[j]] for j, kw in enumerate(parameters)})
        for j in reversed(range(k)):   # row-major: the last parameter varies fastest
            index[j] += 1
            if index[j] < n:
                break
            index[j] = 0
    return points


@pytest.mark.parametrize("parameters, iterations, n", [
    ({"c": (0.1, 100)}, 7, 7),
    ({"lambda_": (0, 0.4), "expansions": (1, 1000)}, 125, 11),     # the reference's default A* grid
    ({"lambda_": (0, 0.4), "expansions": (1, 1000)}, 9, 3),
    ({"lambda_": (0, 0.4), "expansions": (1, 1000)}, 8, 2),        # 8 ** 0.5 = 2.83 -> 2 values each
    ({"epsilon": (0, 0.5), "workers": (1, 500), "depth": (1, 250)}, 27, 3),   # 27 ** (1 / 3) is just below 3 in float64
])
def test_grid_enumeration_and_order(parameters, iterations, n):
    points = grid_points(parameters, iterations)
    assert len(points) == n ** len(parameters)
    assert points == _formula(parameters, iterations)
    assert [list(p) for p in points] == [list(parameters)] * len(points)
    seen = []
    gs = GridSearch(lambda p: (seen.append(p) or 0.0, None, None), parameters)
    gs.optimize(iterations)
    assert seen == points and gs.parameter_history == points


def test_the_default_astar_grid():
    points = grid_points({"lambda_": (0, 0.4), "expansions": (1, 1000)}, 125)
    assert len(points) == 121
    assert [p["lambda_"] for p in points[::11]] == np.linspace(0, 0.4, 11).tolist()
    assert [int(p["expansions"]) for p in points[:11]] == [1, 100, 200, 300, 400, 500, 600, 700, 800, 900, 1000]
    assert points[12] == {"lambda_": np.linspace(0, 0.4, 11)[1], "expansions": np.linspace(1, 1000, 11)[1]}


def test_score_forms():
    res = np.array([[4, -1, 6], [-1, 2, -1]])                  # 3 of 6 solved, mean length 4
    assert score_of(res, False) == (0.5, 0.5, 4.0)
    assert score_of(res, True) == (0.125, 0.5, 4.0)
    nothing = np.full((2, 3), -1)
    assert score_of(nothing, False) == (0, 0, -1)
    score, share, mean_length = score_of(nothing, True)
    assert score == 0 and share == 0 and mean_length == -1      # 0 / -1: no division by a mean of nothing


def test_objective_from_evaluator_scores_what_the_evaluator_returns():
    class FakeEvaluator:
        max_states, made = 100, []

        def eval(self, agent):
            self.made.append(agent)
            res = np.array([[3, -1, 5, -1]]) if agent["expansions"] == 2 else np.full((1, 4), -1)
            return res, np.full((1, 4), 7), np.full((1, 4), 0.5)

    def prep(p):
        p["expansions"] = int(p["expansions"])
        return p
    for optim_lengths, best in ((False, 0.5), (True, 0.125)):
        ev = FakeEvaluator()
        ev.made = []
        gs = GridSearch(None, {"expansions": (1, 2.9)})
        gs.objective_from_evaluator(ev, lambda **kw: kw, {"net": "n"}, param_prepper=prep, optim_lengths=optim_lengths)
        score, states, times = gs.target_function({"expansions": 2.9})
        assert score == best and states.shape == times.shape == (1, 4)
        assert gs.optimize(2) == {"expansions": 2.9} and gs.highscore == best and gs.score_history == [0, best]
        assert ev.made == [{"net": "n", "expansions": 2}, {"net": "n", "expansions": 1}, {"net": "n", "expansions": 2}]
        assert gs.parameter_history == [{"expansions": 1.0}, {"expansions": 2.9}]     # the history keeps the unprepped values


def test_pooled_none_picks_the_pool_only_where_it_applies():
    class Sweepable:
        sweep_parameters = ("lambda_", "expansions")

    class Ev:
        def __init__(self, max_states, slots=64):
            self.max_states, self.slots = max_states, slots

        def eval_sweep(self, agent, params):
            raise NotImplementedError
    gs = GridSearch(None, {"lambda_": (0, 0.4), "expansions": (1, 1000)})
    assert not gs.pooled_route_applies()                                        # no evaluator yet
    gs.objective_from_evaluator(Ev(1000), Sweepable, {})
    assert gs.pooled_route_applies()
    gs.objective_from_evaluator(Ev(None), Sweepable, {})
    assert not gs.pooled_route_applies()                                        # bounded by time only: the routes would differ
    gs.objective_from_evaluator(Ev(1000, slots=None), Sweepable, {})
    assert not gs.pooled_route_applies()                                        # no slots: the pool would hold every game at once
    gs.objective_from_evaluator(Ev(1000), dict, {})
    assert not gs.pooled_route_applies()                                        # the agent takes nothing per game
    gs = GridSearch(None, {"c": (0.1, 100)})
    gs.objective_from_evaluator(Ev(1000), Sweepable, {})
    assert not gs.pooled_route_applies()                                        # not a sweepable parameter
    gs = GridSearch(None, {"lambda_": (0, 0.4), "expansions": (1, 1000)})
    gs.objective_from_evaluator(Ev(1000), lambda **kw: Sweepable(), {})
    gs.agent_class.sweep_parameters = Sweepable.sweep_parameters
    with pytest.raises(NotImplementedError):                                    # pooled=None went to eval_sweep
        gs.optimize(4)
    with pytest.raises(ValueError, match="objective_from_evaluator"):
        GridSearch(f, {"x": (0, 42)}, pooled=True).optimize(2)


def test_optimizer_base_and_bayesian():
    with pytest.raises(NotImplementedError):
        Optimizer(f, {"x": (0, 1)}).optimize(1)
    assert Optimizer.format_params({"a": 1, "b": 2.5}) == "a=1, b=2.5"
    assert Optimizer.format_params({"a": 1.5}, prep=lambda p: {**p, "a": int(p["a"])}) == "a=1"
    if importlib.util.find_spec("bayes_opt") is None:
        with pytest.raises(ImportError, match="bayes_opt"):
            BayesianOptimizer(f, {"x": (0, 42)}, n_restarts=2)
