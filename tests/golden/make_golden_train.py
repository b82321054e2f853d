"""
The training loop recorded from the IMPORTED REFERENCE (librubiks/train.py Train.train), rollout by rollout.
See make_golden.py for how to run (`train`).  The reference is driven from the outside only: a recording wrapper around
its `ADI_traindata`, an `optim_fn` that keeps the optimizer it returns, a stub evaluator with scripted results.

(a) schedule cases: exact quantities of tiny configurations -- alpha, learning rate, training states, loss weights of every
    rollout, the evaluation schedule, the chosen best net, the position of the global NumPy stream after training;
(b) numerics cases: targets, losses and final parameters of three rollouts with SGD, run twice by the reference: in fp32 as it
    is, and in float64 (module cast with .double(), one-hot input cast at the module boundary).  The distance between the
    two runs is the yardstick `e_ref` of tests/test_train_parity_gpu.py.

One torch thread, so that a second run writes the same bytes.
"""
import hashlib
import json
import os
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))

GAP = 1e-4            # a policy target counts only where best - second best of value + reward exceeds this (float64 run)
MAX_SHARE = 0.02      # ... and at most this share of a rollout's states may fall below it
HEAD = 16             # leading values kept per tensor

_BASE = dict(rollouts=3, games=2, depth=3, batch_size=3, evaluation_interval=0, update_interval=0, alpha_update=0.0, gamma=1.0,
             tau=1.0, reward_method="lapanfix", lr=1e-4, script=None, evaluator="stub")


def _case(name, seed, **kw):
    assert set(kw) <= set(_BASE), kw
    return dict(_BASE, name=name, seed=seed, **kw)


# script: the share of solved games (of 4) the stub evaluator reports at its 1st, 2nd, ... call
SCHEDULE_CASES = [
    _case("r1_plain", 101, rollouts=1),
    _case("r1_ei2", 102, rollouts=1, evaluation_interval=2, script=[0.5]),
    _case("r2_ei0_never_evaluates", 103, rollouts=2, script=[1.0, 1.0]),
    _case("r2_ei1_all_zero", 104, rollouts=2, evaluation_interval=1, update_interval=1, alpha_update=0.5, gamma=0.5, tau=0.3,
          reward_method="schultzfix", script=[0.0, 0.0]),
    _case("r3_ei1_tie_then_better", 105, evaluation_interval=1, script=[0.5, 0.5, 0.75]),
    _case("r3_ei1_ties_only", 106, evaluation_interval=1, script=[0.5, 0.5, 0.5]),
    _case("r3_ei2", 107, evaluation_interval=2, script=[0.0, 0.25, 0.25], games=3, depth=4, batch_size=5),
    _case("r4_ei3_best_in_middle", 108, rollouts=4, evaluation_interval=3, script=[0.25, 0.75, 0.5]),
    _case("r5_ei9_all_zero", 109, rollouts=5, evaluation_interval=9, script=[0.0, 0.0]),
    _case("r6_ei2_late_improvement", 110, rollouts=6, evaluation_interval=2, script=[0.25, 0.25, 0.5, 0.5], depth=4, batch_size=4),
    _case("r5_ui2_au03_g05", 111, rollouts=5, update_interval=2, alpha_update=0.3, gamma=0.5),
    _case("r7_ui1_au03_clamp", 112, rollouts=7, update_interval=1, alpha_update=0.3),
    _case("r7_ui3_au05_g05", 113, rollouts=7, update_interval=3, alpha_update=0.5, gamma=0.5, evaluation_interval=3,
          script=[0.0, 0.5, 0.5, 1.0]),
    _case("r6_ui1_au05", 114, rollouts=6, update_interval=1, alpha_update=0.5, games=3, depth=3, batch_size=7),
    _case("r4_ui1_au1", 115, rollouts=4, update_interval=1, alpha_update=1.0, gamma=0.5),
    _case("r4_ui0_au1", 116, rollouts=4, update_interval=0, alpha_update=1.0, gamma=0.5),
    _case("r5_ui1_au0_g05", 117, rollouts=5, update_interval=1, gamma=0.5),
    _case("r5_ui2_au03_tau03", 118, rollouts=5, update_interval=2, alpha_update=0.3, tau=0.3, games=2, depth=4, batch_size=3),
    _case("r3_paper", 119, reward_method="paper", games=3, depth=4, batch_size=5, update_interval=1, alpha_update=0.5),
    _case("r3_lapanfix", 120, reward_method="lapanfix", games=3, depth=4, batch_size=5, update_interval=1, alpha_update=0.5),
    _case("r3_schultzfix", 121, reward_method="schultzfix", games=3, depth=4, batch_size=5, update_interval=1, alpha_update=0.5),
    _case("r3_reward0", 122, reward_method="reward0", games=3, depth=4, batch_size=5, update_interval=1, alpha_update=0.5),
    _case("r3_ei1_real_evaluator", 123, evaluation_interval=1, evaluator="real", games=3, depth=4, batch_size=4),
    _case("r4_ei2_real_evaluator_tau03", 124, rollouts=4, evaluation_interval=2, evaluator="real", tau=0.3, update_interval=1,
          alpha_update=0.5, gamma=0.5),
]
REAL_EVALUATOR = dict(n_games=4, scrambling_depths=[2, 4], max_time=None, max_states=60)
STUB_GAMES = 4

_NUM = dict(rollouts=3, games=16, depth=8, batch_size=50, evaluation_interval=0, update_interval=0, alpha_update=0.0, gamma=1.0,
            tau=1.0, reward_method="lapanfix", lr=1e-3, script=None, evaluator="stub", seed=0)
NUMERICS_CASES = [
    dict(_NUM, name="tau1"),
    dict(_NUM, name="tau03", tau=0.3, gamma=0.5, update_interval=1, alpha_update=0.5),
    dict(_NUM, name="reward0", reward_method="reward0"),
]


def summarize(state_dict):
    """float64[T, 2 + HEAD] per tensor of a state_dict, in its order: sum, sum of squares, the first HEAD values (zero padded)."""
    rows = []
    for t in state_dict.values():
        x = t.detach().cpu().double().reshape(-1).numpy()
        head = np.zeros(HEAD)
        head[:min(HEAD, len(x))] = x[:HEAD]
        rows.append(np.concatenate([[x.sum(), (x * x).sum()], head]))
    return np.array(rows)


class StubEvaluator:
    """Scripted results, no searches, no random numbers; remembers at which rollout it was called and the network it saw."""

    def __init__(self, script, rollout_of_call):
        self.script, self.rollout_of_call = list(script or []), rollout_of_call
        self.scrambling_depths = np.array([3])
        self.n_games = STUB_GAMES
        self.calls, self.nets = [], []

    def eval(self, agent):
        self.calls.append(self.rollout_of_call())
        self.nets.append(summarize(agent.net.state_dict()))
        solved = int(round(self.script[len(self.calls) - 1] * STUB_GAMES))
        results = np.array([[5] * solved + [-1] * (STUB_GAMES - solved)])
        return results, np.zeros_like(results), np.zeros(results.shape)


def run_reference(case, double=False, optim=torch.optim.Adam):
    """One Train.train of the reference for `case`; everything the tests compare, as a dict of arrays."""
    from librubiks import cube
    from librubiks.model import Model, ModelConfig
    from librubiks.solving.agents import MCTS, PolicySearch
    from librubiks.solving.evaluation import Evaluator
    from librubiks.train import Train

    torch.manual_seed(case["seed"])
    np.random.seed(case["seed"])
    net = Model.create(ModelConfig())
    rec = {"init": summarize(net.state_dict()), "alpha": [], "lr": [], "ohcols": [], "weights": [], "policy": [], "value": [],
           "gap": [], "eval_pos": [], "eval_key": []}

    if double:
        def as_double(module):
            """float64 module that takes the reference's float32 one-hot input and whose clones are float64 too
            (Model.clone rebuilds the module through Model.create, i.e. in fp32)."""
            module.double()
            plain = type(module).forward
            module.forward = types.MethodType(lambda self, x, policy=True, value=True: plain(self, x.double(), policy, value), module)

            def clone(self):
                twin = Model.create(self.config)
                as_double(twin)
                twin.load_state_dict({k: v.clone() for k, v in self.state_dict().items()})
                return twin
            module.clone = types.MethodType(clone, module)
            return module
        net = as_double(net)

    kept = {}

    def optim_fn(params, lr):
        kept["optimizer"] = optim(params, lr=lr)
        return kept["optimizer"]

    if case["evaluator"] == "real":
        evaluator = Evaluator(**REAL_EVALUATOR)
        plain_eval = evaluator.eval

        def recording_eval(agent):
            state = np.random.get_state()
            rec["eval_pos"].append(int(state[2]))
            rec["eval_key"].append(hashlib.sha256(state[1].tobytes()).hexdigest())
            evaluator_calls.append(len(rec["alpha"]) - 1)
            return plain_eval(agent)
        evaluator_calls = []
        evaluator.eval = recording_eval
        agent = MCTS(net, c=0.6, search_graph=True)
    else:
        evaluator = StubEvaluator(case["script"], lambda: len(rec["alpha"]) - 1)
        evaluator_calls = evaluator.calls
        agent = PolicySearch(None)

    train = Train(rollouts=case["rollouts"], batch_size=case["batch_size"], rollout_games=case["games"], rollout_depth=case["depth"],
                  optim_fn=optim_fn, alpha_update=case["alpha_update"], lr=case["lr"], gamma=case["gamma"],
                  update_interval=case["update_interval"], agent=agent, evaluator=evaluator,
                  evaluation_interval=case["evaluation_interval"], with_analysis=False, tau=case["tau"],
                  reward_method=case["reward_method"])
    plain_adi = train.ADI_traindata
    win = 0.0 if case["reward_method"] == "reward0" else 1.0

    def recording_adi(generator, alpha):
        oh, policy, value, weights = plain_adi(generator, alpha)
        assert next(generator.parameters()).dtype == (torch.float64 if double else torch.float32)   # clones included
        rec["alpha"].append(float(alpha))
        rec["lr"].append(float(kept["optimizer"].param_groups[0]["lr"]))
        cols = np.nonzero(oh.cpu().numpy())[1].reshape(len(oh), 20)
        rec["ohcols"].append(cols.astype(np.int16))
        rec["weights"].append(weights.numpy().copy())
        rec["policy"].append(policy.numpy().copy())
        rec["value"].append(value.numpy().copy())
        # best minus second best of value + reward over the 12 substates of every state, from the same generator
        states = (cols - 24 * np.arange(20)).astype(np.int8)
        substates = cube.multi_rotate(np.repeat(states, 12, axis=0), *cube.iter_actions(len(states)))
        rewards = np.where(cube.multi_is_solved(substates), win, -1.0)
        with torch.no_grad():
            values = generator(cube.as_oh(substates), policy=False, value=True).double().numpy().reshape(-1) + rewards
        top = np.sort(values.reshape(-1, 12), axis=1)
        rec["gap"].append(top[:, -1] - top[:, -2])
        assert not double or np.array_equal(values.reshape(-1, 12).argmax(1), rec["policy"][-1])
        return oh, policy, value, weights
    train.ADI_traindata = recording_adi

    net, best = train.train(net)
    out = {k: np.array(v) for k, v in rec.items() if k != "eval_key"}
    out["eval_key"] = np.array(rec["eval_key"])
    out["evaluation_rollouts"] = np.asarray(train.evaluation_rollouts, dtype=np.int64)
    out["eval_calls"] = np.array(evaluator_calls, dtype=np.int64)
    out["policy_losses"], out["value_losses"] = train.policy_losses.copy(), train.value_losses.copy()
    out["final"] = summarize(net.state_dict())
    out["final_tensors"] = [t.detach().cpu().double().reshape(-1).numpy() for t in net.state_dict().values()]
    out["draw"] = np.array(np.random.randint(0, 2 ** 31), dtype=np.int64)
    if case["evaluator"] == "stub":
        best_sum = summarize(best.state_dict())
        hits = [r for r, s in zip(evaluator.calls, evaluator.nets) if np.array_equal(s, best_sum)]
        if np.array_equal(best_sum, rec["init"]):
            hits.append(-1)
        assert len(hits) == 1, (case["name"], hits)
        out["best"] = np.array(hits[0], dtype=np.int64)
    return out


SCHEDULE_KEYS = ("init", "alpha", "lr", "ohcols", "weights", "evaluation_rollouts", "eval_calls", "draw")


def sgd(params, lr):
    return torch.optim.SGD(params, lr=lr)


def make_train():
    import librubiks  # noqa: F401  (the reference; fails early if it is not on the path)
    torch.set_num_threads(1)
    fx, meta = {}, {"schedule": {}, "numerics": {}, "gap": GAP, "max_share": MAX_SHARE, "head": HEAD,
                    "real_evaluator": REAL_EVALUATOR, "stub_games": STUB_GAMES}

    for case in SCHEDULE_CASES:
        out = run_reference(case)
        pre = f"s_{case['name']}_"
        for k in SCHEDULE_KEYS:
            fx[pre + k] = out[k]
        if case["evaluator"] == "real":
            fx[pre + "eval_pos"], fx[pre + "eval_key"] = out["eval_pos"], out["eval_key"]
        else:
            fx[pre + "best"] = out["best"]
        meta["schedule"][case["name"]] = case
        print(f"schedule {case['name']}: alpha {out['alpha'].tolist()} lr {out['lr'].tolist()} evaluations at "
              f"{out['eval_calls'].tolist()} of {out['evaluation_rollouts'].tolist()} best {out.get('best')} draw {out['draw']}")

    for case in NUMERICS_CASES:
        r32, r64 = run_reference(case, optim=sgd), run_reference(case, double=True, optim=sgd)
        pre = f"n_{case['name']}_"
        assert np.array_equal(r32["ohcols"], r64["ohcols"]) and np.array_equal(r32["init"], r64["init"])
        assert r32["value"].dtype == np.float32 and r64["value"].dtype == np.float64
        close = r64["gap"] <= GAP
        share = close.mean(axis=1)
        assert share.max() <= MAX_SHARE, (case["name"], share)
        assert np.array_equal(r32["policy"][~close], r64["policy"][~close]), case["name"]
        for k in ("init", "ohcols", "weights", "alpha", "lr", "draw"):
            fx[pre + k] = r32[k]
        for k in ("policy", "value", "policy_losses", "value_losses", "final"):
            fx[pre + k + "32"], fx[pre + k + "64"] = r32[k], r64[k]
        fx[pre + "gap64"] = r64["gap"]
        # e_ref: the reference's own fp32-vs-float64 distance, the largest over the case's rollouts
        e_ref = {"value": float(np.abs(r32["value"] - r64["value"]).max()),
                 "policy_losses": float(np.abs(r32["policy_losses"] - r64["policy_losses"]).max()),
                 "value_losses": float(np.abs(r32["value_losses"] - r64["value_losses"]).max())}
        # ... and per tensor of the final state_dict, for sum / sum of squares / leading values.  The two sums run over the
        # elements, and the signed sum of the reference's per-element differences cancels by chance (the BatchNorm bias of the
        # first layer: 1.6e-11 in the tau = 1 case, 1.4e-8 in the tau = 0.3 case, same tensor, same first rollout), so one
        # run's signed sum is no yardstick for another's.  Its scale is the root of the sum of the squared per-element
        # differences (the standard deviation of a sum of independent zero-mean terms): e_ref is the larger of the two.
        d = np.abs(r32["final"] - r64["final"])
        signed = np.stack([d[:, 0], d[:, 1], d[:, 2:].max(axis=1)], axis=1)
        rss = np.array([[np.sqrt(((a - b) ** 2).sum()), np.sqrt(((a * a - b * b) ** 2).sum()), 0.0]
                        for a, b in zip(r32["final_tensors"], r64["final_tensors"])])
        fx[pre + "e_ref_final_signed"], fx[pre + "e_ref_final_rss"] = signed, rss
        fx[pre + "e_ref_final"] = np.maximum(signed, rss)
        meta["numerics"][case["name"]] = dict(case, e_ref=e_ref, share_below_gap=share.tolist(), smallest_gap=float(r64["gap"].min()),
                                              policy_mismatches_below_gap=int((r32["policy"] != r64["policy"]).sum()))
        print(f"numerics {case['name']}: e_ref {e_ref} share below gap {share.tolist()} smallest gap {r64['gap'].min():.3e} "
              f"losses {r64['policy_losses'].tolist()} {r64['value_losses'].tolist()}")

    fx["meta_json"] = np.array(json.dumps(meta))
    fx["torch_version"], fx["numpy_version"] = np.array(torch.__version__), np.array(np.__version__)
    path = os.path.join(OUT, "train_golden.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print("train_golden.npz:", len(fx), "arrays,", size, "bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    make_train()
