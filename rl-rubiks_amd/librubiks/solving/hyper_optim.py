"""
Hyper-parameter optimisation of the search agents behind the reference's interface (its librubiks/solving/hyper_optim.py:22-186:
class names, constructor and method signatures, the four result attributes), written for this code base:

    gs = GridSearch(None, {"lambda_": (0, 0.4), "expansions": (1, 1000)})
    gs.objective_from_evaluator(Evaluator(100, [depth], max_states=..., slots=4096), AStar, {"net": net}, param_prepper=prep)
    best = gs.optimize(125)          # 11 x 11 points; gs.score_history, gs.parameter_history, gs.optimal, gs.highscore

The reference walks a grid point by point, with a new agent and one `Evaluator.eval` each.  A point is ~100 games -- a small batch for
a 256-CU device -- and every point sets up and drops a batch of its own.  Where the agent's `search_batch` takes the grid's
parameters per game (`agent_class.sweep_parameters`; AStar: lambda_, expansions; MCTS: c), the whole grid is ONE continuous-batching pool
(`Evaluator.eval_sweep`): `GridSearch(..., pooled=True)`.  Both routes draw the same scrambles from the global np.random stream and,
with deterministic agents under a `max_states` bound, end with the same histories.

The reference's command line (`agent_optimize`) has no counterpart here; `BayesianOptimizer` needs the `bayes_opt` package.
"""
from typing import Callable

import numpy as np

from librubiks.utils import NullLogger

# `GridSearch(pooled=None)` where the pooled route applies: the measured choice (profiles/astar_sweep_probe.txt).
POOLED_BY_DEFAULT = True
# ... and per agent class (its name, or that of a base class), each from that class's own measurement: AStar as above (loop 140-148 s,
# pool 33 s); MCTS profiles/mcts_grid_probe.txt (the reference's 125-point grid over c: loop 108 s, pool 31 s).
POOLED_BY_DEFAULT_FOR = {"AStar": True, "MCTS": True}
# Exploration constants of the acquisition function handed to bayes_opt: the reference's values (hyper_optim.py:161).
ACQUISITION_KAPPA, ACQUISITION_XI = 2.5, 0.2


def score_of(res: np.ndarray, optim_lengths: bool):
    """The reference's objective for one setting (hyper_optim.py:60-66) -> (score, solved share, mean solution length or -1).
    res holds solution lengths, -1 for an unsolved game.  The score is the share, or the share divided by the mean length;
    when nothing is solved that is 0 (as 0 / -1)."""
    res = np.asarray(res).ravel()
    won = res != -1
    share = won.mean() if won.any() else 0
    mean_length = res[won].mean() if share else -1
    return (share / mean_length if optim_lengths else share), share, mean_length


def grid_points(parameters: dict, iterations: int) -> list:
    """The reference's grid (hyper_optim.py:96-99,102-104): n = int(iterations ** (1 / k) + 1e-6) values per parameter,
    np.linspace over its interval, every combination in row-major order (the last parameter varies fastest)."""
    k = len(parameters)
    n = int(iterations ** (1 / k) + 1e-6)
    spaces = [np.linspace(*interval, n) for interval in parameters.values()]
    return [{kw: space[i] for kw, space, i in zip(parameters, spaces, index)} for index in np.ndindex(*[n] * k)]


class Optimizer:
    """Maximises `target_function(params: dict) -> (score, states, times)` over `parameters` (name -> (low, high)).  After
    `optimize`: `score_history` and `parameter_history` (one entry per evaluated setting, in order), `optimal`, `highscore`."""

    def __init__(self, target_function, parameters: dict, logger=NullLogger()):
        self.target_function, self.parameters, self.logger = target_function, parameters, logger
        self.score_history, self.parameter_history = [], []
        self.optimal = self.highscore = None
        # set by `objective_from_evaluator`
        self.evaluator = self.agent_class = self.persistent_agent_params = self.param_prepper = None
        self.optim_lengths = False
        self.logger.log(f"{self}: searching {self.format_params(parameters)}")

    def optimize(self, iterations: int):
        raise NotImplementedError(f"{type(self).__name__} does not say how it chooses settings")

    def objective_from_evaluator(self, evaluator, agent_class, persistent_agent_params: dict, param_prepper: Callable = lambda x: x,
                                 optim_lengths: bool = False):
        """Makes the target an evaluation: a setting's score (`score_of`) is that of `evaluator.eval` on the agent
        `agent_class(**persistent_agent_params, **param_prepper(setting))`."""
        self.evaluator, self.agent_class, self.persistent_agent_params = evaluator, agent_class, persistent_agent_params
        self.param_prepper, self.optim_lengths = param_prepper, optim_lengths
        self.target_function = lambda setting: self._scored(*self.evaluator.eval(self._agent_for(setting)))

    def _agent_for(self, setting: dict):
        prepared = self.param_prepper(dict(setting))     # (a copy: the history keeps the setting as it was chosen)
        return self.agent_class(**self.persistent_agent_params, **prepared)

    def _scored(self, res, states, times):
        score, share, mean_length = score_of(res, self.optim_lengths)
        self.logger.log(f"\tsolved {100 * share:.2f} % of the games, mean solution length {mean_length}; "
                        f"{states.mean():.0f} states and {times.mean():.2f} s a game on average")
        return score, states, times

    def _keep(self, step: int, setting: dict, score):
        self.parameter_history.append(setting)
        self.score_history.append(score)
        self.logger(f"setting {step} ({self.format_params(setting, prep=self.param_prepper)}): score {score}")

    def _conclude(self):
        best = int(np.argmax(self.score_history))
        self.optimal, self.highscore = self.parameter_history[best], self.score_history[best]
        self.logger(f"{self}: best score {self.highscore} with {self.format_params(self.optimal, prep=self.param_prepper)}")
        return self.optimal

    @staticmethod
    def format_params(params: dict, prep=None) -> str:
        shown = params if prep is None else prep(dict(params))
        return ", ".join(f"{name}={value}" for name, value in shown.items())


class GridSearch(Optimizer):
    """
    Every point of a regular grid (`grid_points`).  pooled: False -- the reference's loop, `target_function` point by point;
    True -- after `objective_from_evaluator`, the whole grid in one `evaluator.eval_sweep` (the agent class must take every grid
    parameter per game); None -- the pool where it applies (`pooled_route_applies`) and has been measured faster
    for the agent class (`POOLED_BY_DEFAULT`, `POOLED_BY_DEFAULT_FOR`) and the agent does not refuse it (`sweep_refusal`), else the
    loop.
    """

    def __init__(self, target_function, parameters: dict, logger=NullLogger(), pooled: bool = None):
        super().__init__(target_function, parameters, logger)
        self.pooled = pooled

    def pooled_route_applies(self) -> bool:
        """True where the automatic choice may take the pool: the agent class takes every grid parameter per game; the evaluator
        is bounded by `max_states` (so both routes give the same results) and has `slots` (without them the pool would be one plain
        batch of ALL the grid's games -- 121 x 100 problems with their node rows in HBM at once, where the loop holds 100); one rank."""
        ev = self.evaluator
        if ev is None or self.agent_class is None or not hasattr(ev, "eval_sweep"):
            return False
        from librubiks.solving.evaluation import _world_size
        sweepable = getattr(self.agent_class, "sweep_parameters", ())
        return all(kw in sweepable for kw in self.parameters) and bool(ev.max_states) and bool(getattr(ev, "slots", None)) and _world_size() == 1

    def pooled_by_default(self) -> bool:
        """The measured choice for the agent class (`POOLED_BY_DEFAULT_FOR`), else `POOLED_BY_DEFAULT`."""
        for cls in getattr(self.agent_class, "__mro__", ()):
            if cls.__name__ in POOLED_BY_DEFAULT_FOR:
                return POOLED_BY_DEFAULT_FOR[cls.__name__]
        return POOLED_BY_DEFAULT

    def optimize(self, iterations: int):
        points = grid_points(self.parameters, iterations)
        pooled = (self.pooled_by_default() and self.pooled_route_applies()) if self.pooled is None else bool(self.pooled)
        if pooled and self.evaluator is None:
            raise ValueError("GridSearch(pooled=True) evaluates the grid through an Evaluator: call objective_from_evaluator first")
        agent = self._agent_for(points[0]) if pooled else None
        if pooled and self.pooled is None and getattr(agent, "sweep_refusal", lambda: None)():
            pooled = False     # the automatic choice takes no pool that `eval_sweep` would refuse (MCTS on a batch-dependent engine)
        self.logger.section(f"{self}: {len(points)} settings, " + ("searched as one pool" if pooled else "one after the other"))
        if pooled:
            prepared = [self.param_prepper(dict(p)) for p in points]   # (as the loop prepares each setting before it builds the agent)
            per_setting = {kw: np.array([p[kw] for p in prepared]) for kw in self.parameters}
            res, states, times = self.evaluator.eval_sweep(agent, per_setting)
            scores = [self._scored(res[i], states[i], times[i])[0] for i in range(len(points))]
            for step, (setting, score) in enumerate(zip(points, scores)):
                self._keep(step, setting, score)
        else:
            scores = []
            for step, setting in enumerate(points):     # (the histories grow as the loop goes: a run that is cut short keeps them)
                scores.append(self.target_function(setting)[0])
                self._keep(step, setting, scores[-1])
        self._conclude()
        n = int(iterations ** (1 / len(self.parameters)) + 1e-6)
        self.logger("scores over the grid (first parameter along the first axis)\n" + str(np.array(scores).reshape([n] * len(self.parameters))))
        return self.optimal

    def __str__(self):
        return "Grid Search"


def _bayes_opt():
    try:
        import bayes_opt
    except ImportError as e:
        raise ImportError("BayesianOptimizer needs the package bayes_opt (bayesian-optimization), which is not installed; "
                          "GridSearch needs nothing beyond NumPy") from e
    return bayes_opt


class BayesianOptimizer(Optimizer):
    """Gaussian-process optimisation through the `bayes_opt` package's ask-and-tell interface (`suggest` / `register`): every
    setting depends on the scores before it, so each is its own `target_function` call -- there is nothing to pool.
    alpha: the noise the process assumes in the scores; n_restarts: restarts of its fit; acquisition: 'ei', 'ucb' or 'poi'."""

    def __init__(self, target_function, parameters: dict, alpha: float = 1e-5, n_restarts: int = 20, acquisition: str = "ei",
                 logger=NullLogger()):
        package = _bayes_opt()
        super().__init__(target_function, parameters, logger)
        self.optimizer = package.BayesianOptimization(f=None, pbounds=dict(parameters), verbose=0)   # f=None: this class asks and tells
        self.optimizer.set_gp_params(alpha=alpha, n_restarts_optimizer=n_restarts)
        self.utility = package.UtilityFunction(kind=acquisition, kappa=ACQUISITION_KAPPA, xi=ACQUISITION_XI)
        self.logger(f"{self}: acquisition {acquisition}, alpha {alpha}, {n_restarts} restarts of the fit")

    def optimize(self, iterations: int):
        for step in range(iterations):
            setting = self.optimizer.suggest(self.utility)
            score = self.target_function(setting)[0]
            self._keep(step, setting, score)
            self.optimizer.register(params=setting, target=score)
        return self._conclude()

    def __str__(self):
        return "Bayesian Optimizer"
