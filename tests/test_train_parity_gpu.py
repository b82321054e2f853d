"""
`Train.train` against the reference's own runs, rollout by rollout (tests/golden/train_golden.npz, recorded from the imported
reference by tests/golden/make_golden_train.py).  The product's `Train` is instrumented from here exactly as the reference was
there (tests/train_parity.py): a recording wrapper around `ADI_traindata`, an `optim_fn` that keeps its optimizer, a stub
evaluator with scripted results.

Schedule cases: exact quantities -- alpha, learning rate, training states of every rollout, loss weights, the evaluation schedule,
the rollouts at which the evaluator ran, the chosen best net, the global NumPy stream after training.

Numerics cases (SGD, three rollouts, 16 games x depth 8, batches 50 / 50 / 28): compared with the reference's FLOAT64 run.
Tolerance of a quantity = 4 x e_ref + four fp32 ulps of its magnitude, where e_ref is the reference's own fp32-vs-float64
distance for that quantity, the largest over the case's rollouts, taken from the fixture.  The factor 4 allows for another
summation order in the GPU's GEMMs and reductions over three chained rollouts; nothing is calibrated on the product's output.

For a statistic that is a sum over a tensor's elements (sum, sum of squares) e_ref is the larger of the reference's signed
distance and the root of the sum of its squared per-element differences: the signed sum of zero-mean differences cancels by
chance and is no yardstick from one run to the next.  With the signed distance alone this test failed on three BatchNorm bias
tensors -- tau = 1, first layer: product 8.09e-9 (2.86e-8 on the split engine) against a signed e_ref of 1.6e-11, where the
reference's tau = 0.3 run has 1.4e-8 for the same tensor after the same first rollout; reward0, second layer: 1.26e-8
against 2.2e-9 -- while every other quantity stood as it stands now.

Measured on one MI355X, |product - float64| / e_ref (the same figures in two runs on two machines):

    case             value targets  policy losses  value losses  final sum  final sum sq.  final leading values
    tau1                     1.80           0.93          1.75       3.04           1.65                  1.88
    tau03                    1.59           1.01          1.52       1.72           2.01                  1.89
    reward0                  1.31           1.63          2.31       2.83           2.93                  2.12
    tau1 / F32_SPLIT         1.53           0.99          2.10       3.80           1.80                  2.09

(final ...: the largest ratio over the 32 tensors; the medians are 0.5 - 1.05.)  Above 2, hence reported: the value losses
of reward0 and of the split engine, and single tensors of the final summaries; the tensors with ratios above 3 have a four-ulp
floor larger than 2 x e_ref, and no tensor uses more than 0.68 of its tolerance (reward0, BatchNorm bias of the second
layer: 1.26e-8 of 1.86e-8).  Policy targets agree on every state in all four; no state of the fixture is a near-tie.
bf16 (reported only): policy targets agree on 98.4 / 99.2 / 100 % of the states, value targets within 6e-3, losses within 1.1 %.
"""
import numpy as np
import pytest
import torch

from train_parity import META, NUMERICS, SCHEDULE, fixture, run_product

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23


def _sgd(params, lr):
    return torch.optim.SGD(params, lr=lr)


@pytest.mark.parametrize("name", sorted(SCHEDULE))
def test_schedule_parity(name):
    case, ref = SCHEDULE[name], fixture("s", name)
    got = run_product(case)
    assert np.array_equal(got["init"], ref["init"]), "the seeded initial network differs: not a matter of the loop"
    assert len(got["alpha"]) == case["rollouts"]
    for r in range(case["rollouts"]):
        where = f"{name}: rollout {r}"
        print(f"{where}: alpha {got['alpha'][r]} / {ref['alpha'][r]}  lr {got['lr'][r]} / {ref['lr'][r]}  "
              f"states equal {np.array_equal(got['ohcols'][r], ref['ohcols'][r])}")
        assert float(got["alpha"][r]) == float(ref["alpha"][r]), where
        assert float(got["lr"][r]) == float(ref["lr"][r]), where
        assert np.array_equal(got["ohcols"][r], ref["ohcols"][r]), f"{where}: training states differ from the reference's"
        assert got["weights"].dtype == np.float32 and np.array_equal(got["weights"][r], ref["weights"][r]), where
    assert got["evaluation_rollouts"].tolist() == ref["evaluation_rollouts"].tolist()
    assert got["eval_calls"].tolist() == ref["eval_calls"].tolist()
    if case["evaluator"] == "stub":
        assert got["best"] == [int(ref["best"])], f"best net of rollout {got['best']}, the reference's: {int(ref['best'])}"
    else:   # the reference's Evaluator: where the global stream stands whenever an evaluation begins
        assert got["eval_pos"].tolist() == ref["eval_pos"].tolist()
        assert got["eval_key"].tolist() == ref["eval_key"].tolist()
    assert int(got["draw"]) == int(ref["draw"]), "the global NumPy stream after training"


def _tolerance(e_ref, magnitude):
    return 4 * e_ref + 4 * ULP32 * magnitude


def _check_numerics(name, got, label):
    """The assertions of a numerics case; returns {quantity: distance to the float64 run / e_ref}."""
    case, ref = NUMERICS[name], fixture("n", name)
    assert np.array_equal(got["init"], ref["init"]), "the seeded initial network differs: not a matter of the loop"
    assert np.array_equal(got["ohcols"], ref["ohcols"]), "training states"
    assert got["alpha"].tolist() == ref["alpha"].tolist() and got["lr"].tolist() == ref["lr"].tolist()
    assert int(got["draw"]) == int(ref["draw"])
    # policy targets: wherever the float64 run's best and second-best substate are further apart than the gap
    decided = ref["gap64"] > META["gap"]
    share = 1 - decided.mean(axis=1)
    assert share.max() <= META["max_share"], share
    agree = got["policy"] == ref["policy64"]
    print(f"{label}: policy targets agree on {agree.mean():.4f} of all states, excluded share per rollout {share.tolist()}")
    assert agree[decided].all(), f"{(~agree[decided]).sum()} policy targets differ outside the excluded near-ties"
    ratios, failures = {}, []

    def hold(quantity, distance, e_ref, magnitude):
        tol = _tolerance(e_ref, magnitude)
        ratios[quantity] = distance / e_ref if e_ref else (0.0 if distance == 0 else np.inf)
        print(f"{label}: {quantity}: |product - float64| = {distance:.3e}, e_ref = {e_ref:.3e}, ratio {ratios[quantity]:.2f}, "
              f"tolerance {tol:.3e}")
        if not distance <= tol:
            failures.append(f"{quantity}: {distance:.3e} > {tol:.3e} (e_ref {e_ref:.3e})")

    e = case["e_ref"]
    assert np.isfinite(got["value"]).all() and np.isfinite(got["policy_losses"]).all() and np.isfinite(got["value_losses"]).all()
    hold("value targets", np.abs(got["value"] - ref["value64"]).max(), e["value"], np.abs(ref["value64"]).max())
    for k in ("policy_losses", "value_losses"):
        hold(k, np.abs(got[k] - ref[k + "64"]).max(), e[k], np.abs(ref[k + "64"]).max())
    # final parameters and BatchNorm buffers, per tensor: sum, sum of squares, leading values
    f64, e_final = ref["final64"], ref["e_ref_final"]
    dist = np.abs(got["final"] - f64)
    dist = np.stack([dist[:, 0], dist[:, 1], dist[:, 2:].max(axis=1)], axis=1)
    mag = np.stack([np.abs(f64[:, 0]), np.abs(f64[:, 1]), np.abs(f64[:, 2:]).max(axis=1)], axis=1)
    tol = _tolerance(e_final, mag)
    for j, stat in enumerate(("sum", "sum of squares", "leading values")):
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(e_final[:, j] > 0, dist[:, j] / e_final[:, j], 0.0)
        worst = int(np.argmax(dist[:, j] / np.maximum(tol[:, j], 1e-300)))
        ratios[f"final {stat}"] = float(ratio.max())
        print(f"{label}: final {stat}: largest ratio to e_ref over the tensors {ratio.max():.2f}, median {np.median(ratio):.2f}; "
              f"closest to its tolerance: tensor {worst}, {dist[worst, j]:.3e} of {tol[worst, j]:.3e} (e_ref {e_final[worst, j]:.3e})")
        bad = np.nonzero(~(dist[:, j] <= tol[:, j]))[0]
        if len(bad):
            failures.append(f"final {stat}: tensors {bad.tolist()} beyond tolerance, e.g. {dist[bad[0], j]:.3e} > {tol[bad[0], j]:.3e}")
    assert not failures, f"{label}: " + "; ".join(failures)
    return ratios


@pytest.mark.parametrize("name", sorted(NUMERICS))
def test_numerics_parity(name):
    got = run_product(NUMERICS[name], optim=_sgd, record_generator=NUMERICS[name]["tau"] != 1)
    _check_numerics(name, got, name)
    if NUMERICS[name]["tau"] != 1:
        _check_generator(got["generator"], NUMERICS[name]["tau"], NUMERICS[name]["rollouts"])


def _check_generator(updates, tau, rollouts):
    """generator <- tau * net + (1 - tau) * generator after every `_update_gen_net`, against float64 arithmetic on the two
    inputs.  fp32 does two roundings of the products and one of the sum, and rounds tau itself: within four ulps of the
    addends' size.  Integer buffers (num_batches_tracked) are the truncated float64 value, exactly."""
    assert len(updates) == rollouts
    for r, (gen, net, out) in enumerate(updates):
        assert list(out) == list(net) == list(gen)
        for k in out:
            want = tau * net[k].double() + (1 - tau) * gen[k].double()
            if out[k].dtype.is_floating_point:
                assert out[k].dtype == torch.float32
                bound = 4 * ULP32 * (abs(tau) * net[k].double().abs() + abs(1 - tau) * gen[k].double().abs())
                worst = ((out[k].double() - want).abs() - bound).max().item()
                assert worst <= 0, f"rollout {r}, {k}: beyond four ulps by {worst:.3e}"
            else:
                assert torch.equal(out[k], want.to(out[k].dtype)), f"rollout {r}, {k}: {out[k].tolist()} != trunc({want.tolist()})"
        tracked = [int(out[k]) for k in out if k.endswith("num_batches_tracked")]
        print(f"generator after update {r}: num_batches_tracked {tracked}")


def test_numerics_parity_split_engine():
    """The tau = 1 case with the ADI value network on the f16x3 split engine: same assertions, same tolerance -- its targets
    feed back into training for three rollouts."""
    from librubiks.model import F32_SPLIT
    got = run_product(NUMERICS["tau1"], optim=_sgd, adi_net_dtype=F32_SPLIT)
    _check_numerics("tau1", got, "tau1 / F32_SPLIT")


def test_numerics_bf16_engine_reported():
    """bf16 ADI engine: the scrambles do not depend on the engine (exact); the rest is reported, and finite."""
    name = "tau1"
    ref, got = fixture("n", name), run_product(NUMERICS[name], optim=_sgd, adi_net_dtype=torch.bfloat16)
    assert np.array_equal(got["ohcols"], ref["ohcols"]) and int(got["draw"]) == int(ref["draw"])
    decided = ref["gap64"] > META["gap"]
    for r in range(NUMERICS[name]["rollouts"]):
        print(f"bf16 rollout {r}: policy targets agree on {(got['policy'][r] == ref['policy64'][r])[decided[r]].mean():.4f}, "
              f"value targets within {np.abs(got['value'][r] - ref['value64'][r]).max():.3e}, "
              f"policy loss {got['policy_losses'][r]:.6f} / {ref['policy_losses64'][r]:.6f}, "
              f"value loss {got['value_losses'][r]:.6f} / {ref['value_losses64'][r]:.6f}")
    for k in ("value", "policy_losses", "value_losses", "final"):
        assert np.isfinite(got[k]).all(), k
