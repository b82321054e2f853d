"""
Shared by tests/test_train_parity_gpu.py and tests/test_train_golden.py: reading tests/golden/train_golden.npz (the reference's
training loop recorded rollout by rollout, tests/golden/make_golden_train.py) and driving the product's `Train` the way the
generator drove the reference's -- wrappers from the outside and a stub evaluator, no hook inside the product.
"""
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_golden.npz")
_fx = np.load(GOLDEN)
META = json.loads(str(_fx["meta_json"]))
SCHEDULE, NUMERICS = META["schedule"], META["numerics"]
HEAD = META["head"]


def fixture(prefix: str, case: str) -> dict:
    pre = f"{prefix}_{case}_"
    return {k[len(pre):]: _fx[k] for k in _fx.files if k.startswith(pre)}


def summarize(state_dict) -> np.ndarray:
    """float64[T, 2 + HEAD] per tensor, in state_dict order: sum, sum of squares, the first HEAD values (zero padded)."""
    rows = []
    for t in state_dict.values():
        x = t.detach().cpu().double().reshape(-1).numpy()
        head = np.zeros(HEAD)
        head[:min(HEAD, len(x))] = x[:HEAD]
        rows.append(np.concatenate([[x.sum(), (x * x).sum()], head]))
    return np.array(rows)


class StubEvaluator:
    """Scripted results (the share of `games` solved at the 1st, 2nd, ... call); no searches, no random numbers."""

    def __init__(self, script, rollout_of_call, games):
        self.script, self.rollout_of_call, self.n_games = list(script or []), rollout_of_call, games
        self.scrambling_depths = np.array([3])
        self.calls, self.nets = [], []

    def eval(self, agent):
        self.calls.append(self.rollout_of_call())
        self.nets.append(summarize(agent.net.state_dict()))
        solved = int(round(self.script[len(self.calls) - 1] * self.n_games))
        results = np.array([[5] * solved + [-1] * (self.n_games - solved)])
        return results, np.zeros_like(results), np.zeros(results.shape)


def run_product(case: dict, optim=torch.optim.Adam, record_generator: bool = False, **train_kw) -> dict:
    """One `Train.train` of the product for a recorded case; the quantities of the fixture under the fixture's names."""
    from librubiks.model import Model, ModelConfig
    from librubiks.solving.agents import MCTS, PolicySearch
    from librubiks.solving.evaluation import Evaluator
    from librubiks.train import Train

    torch.manual_seed(case["seed"])
    np.random.seed(case["seed"])
    net = Model.create(ModelConfig())
    rec = {"init": summarize(net.state_dict()), "alpha": [], "lr": [], "ohcols": [], "weights": [], "policy": [], "value": [],
           "eval_pos": [], "eval_key": [], "generator": []}
    kept = {}

    def optim_fn(params, lr):
        kept["optimizer"] = optim(params, lr=lr)
        return kept["optimizer"]

    if case["evaluator"] == "real":
        evaluator = Evaluator(**META["real_evaluator"])
        plain_eval, calls = evaluator.eval, []

        def recording_eval(agent):
            state = np.random.get_state()
            rec["eval_pos"].append(int(state[2]))
            rec["eval_key"].append(hashlib.sha256(state[1].tobytes()).hexdigest())
            calls.append(len(rec["alpha"]) - 1)
            return plain_eval(agent)
        evaluator.eval = recording_eval
        agent = MCTS(net, c=0.6, search_graph=True)
    else:
        evaluator = StubEvaluator(case["script"], lambda: len(rec["alpha"]) - 1, META["stub_games"])
        calls = evaluator.calls
        agent = PolicySearch(None)

    train = Train(rollouts=case["rollouts"], batch_size=case["batch_size"], rollout_games=case["games"], rollout_depth=case["depth"],
                  optim_fn=optim_fn, alpha_update=case["alpha_update"], lr=case["lr"], gamma=case["gamma"],
                  update_interval=case["update_interval"], agent=agent, evaluator=evaluator,
                  evaluation_interval=case["evaluation_interval"], with_analysis=False, tau=case["tau"],
                  reward_method=case["reward_method"], **train_kw)
    plain_adi = train.ADI_traindata

    def recording_adi(generator, alpha):
        oh, policy, value, weights = plain_adi(generator, alpha)
        rec["alpha"].append(float(alpha))
        rec["lr"].append(float(kept["optimizer"].param_groups[0]["lr"]))
        rec["ohcols"].append(np.nonzero(oh.cpu().numpy())[1].reshape(len(oh), 20).astype(np.int16))
        rec["weights"].append(weights.cpu().numpy().copy())
        rec["policy"].append(policy.cpu().numpy().copy())
        rec["value"].append(value.cpu().numpy().copy())
        return oh, policy, value, weights
    train.ADI_traindata = recording_adi

    if record_generator:
        plain_update = train._update_gen_net

        def recording_update(generator, net):
            before = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in (generator, net)]
            out = plain_update(generator, net)
            rec["generator"].append((*before, {k: v.detach().cpu().clone() for k, v in out.state_dict().items()}))
            return out
        train._update_gen_net = recording_update

    net, best = train.train(net)
    out = {k: (v if k == "generator" else np.array(v)) for k, v in rec.items()}
    out["evaluation_rollouts"] = np.asarray(train.evaluation_rollouts, dtype=np.int64)
    out["eval_calls"] = np.array(calls, dtype=np.int64)
    out["policy_losses"], out["value_losses"] = train.policy_losses.copy(), train.value_losses.copy()
    out["final"] = summarize(net.state_dict())
    out["draw"] = np.array(np.random.randint(0, 2 ** 31), dtype=np.int64)
    if case["evaluator"] == "stub":   # which rollout's network `best_net` is; -1: the clone taken before the first rollout
        best_sum = summarize(best.state_dict())
        hits = [r for r, s in zip(evaluator.calls, evaluator.nets) if np.array_equal(s, best_sum)]
        if np.array_equal(best_sum, rec["init"]):
            hits.append(-1)
        out["best"] = hits
    return out
