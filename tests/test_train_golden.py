"""
tests/golden/train_golden.npz (the reference's training loop, recorded) held to what is already trusted, without a GPU, so that
a regenerated file cannot drift unseen: the oracle's scrambler, the closed form of the loss weights, the product's own
evaluation schedule, and the fixture's own near-tie accounting.
"""
import numpy as np
import pytest

from oracle import cube as oc
from oracle import train as ot
from train_parity import META, NUMERICS, SCHEDULE, _fx, fixture

CASES = [("s", n) for n in sorted(SCHEDULE)] + [("n", n) for n in sorted(NUMERICS)]


def _case(kind, name):
    return (SCHEDULE if kind == "s" else NUMERICS)[name], fixture(kind, name)


def test_case_coverage():
    """The configurations the schedule cases have to cover between them."""
    cs = list(SCHEDULE.values())
    assert {c["rollouts"] for c in cs} >= set(range(1, 8))
    assert {c["evaluation_interval"] for c in cs} >= {0, 1, 2, 3} and any(c["evaluation_interval"] > c["rollouts"] for c in cs)
    assert {c["update_interval"] for c in cs} >= {0, 1, 2, 3}
    assert {c["alpha_update"] for c in cs} >= {0, 0.3, 0.5, 1} and {c["gamma"] for c in cs} >= {1, 0.5} and {c["tau"] for c in cs} >= {1, 0.3}
    assert {c["reward_method"] for c in cs} == {"paper", "lapanfix", "schultzfix", "reward0"}
    sizes = [(c["games"] * c["depth"], c["batch_size"]) for c in cs]
    assert any(n % b == 0 for n, b in sizes) and any(n % b for n, b in sizes)
    assert all(n % b == 0 or n % b >= 2 for n, b in sizes), "BatchNorm needs two rows in the last batch"
    assert sum(c["evaluator"] == "real" for c in cs) == 2
    best = {n: int(fixture("s", n)["best"]) for n, c in SCHEDULE.items() if c["evaluator"] == "stub" and c["evaluation_interval"]}
    assert best["r5_ei9_all_zero"] == best["r2_ei1_all_zero"] == -1            # 0 % throughout: the initial clone stays
    assert best["r3_ei1_ties_only"] == 0 and best["r3_ei1_tie_then_better"] == 2   # a tie does not replace, an improvement does
    assert len(NUMERICS) == 3 and all(c["games"] * c["depth"] % c["batch_size"] >= 2 for c in NUMERICS.values())


@pytest.mark.parametrize("kind,name", CASES)
def test_first_rollout_states_are_the_oracles(kind, name):
    """Rollout 0 starts right after the seeding: the states are what the oracle's scrambler draws (any value function)."""
    case, fx = _case(kind, name)
    np.random.seed(case["seed"])
    states, _, _, w = ot.adi_traindata(lambda s: np.zeros(len(s), dtype=np.float32), case["games"], case["depth"],
                                       case["reward_method"], float(fx["alpha"][0]))
    assert np.array_equal(oc.oh_indices(states), fx["ohcols"][0])
    assert np.array_equal(w, fx["weights"][0])


@pytest.mark.parametrize("kind,name", CASES)
def test_loss_weights_closed_form(kind, name):
    case, fx = _case(kind, name)
    G, D = case["games"], case["depth"]
    assert fx["alpha"].shape == fx["lr"].shape == (case["rollouts"],) and fx["ohcols"].shape == (case["rollouts"], G * D, 20)
    weighted = np.tile(1 / np.arange(1, D + 1), G)
    ws, us = weighted.sum(), len(weighted)
    for r, alpha in enumerate(fx["alpha"]):
        want = ((1 - alpha) * weighted / ws + alpha * np.ones_like(weighted) / us) * (ws + us)
        assert fx["weights"].dtype == np.float32 and np.array_equal(fx["weights"][r], want.astype(np.float32)), (name, r)
    assert 0 <= fx["alpha"].min() and fx["alpha"].max() <= 1
    # lr <- gamma * lr, alpha += alpha_update, after every update_interval-th rollout but rollout 0
    steps = np.array([sum(1 for q in range(1, r) if case["update_interval"] and q % case["update_interval"] == 0)
                      for r in range(case["rollouts"])])
    assert np.allclose(fx["lr"], case["lr"] * case["gamma"] ** steps, rtol=1e-12)


@pytest.mark.parametrize("name", sorted(SCHEDULE))
def test_evaluation_rollouts_are_the_products(name):
    import torch
    from librubiks.train import Train
    case, fx = _case("s", name)
    tr = Train(rollouts=case["rollouts"], batch_size=case["batch_size"], rollout_games=case["games"], rollout_depth=case["depth"],
               optim_fn=torch.optim.Adam, alpha_update=case["alpha_update"], lr=case["lr"], gamma=case["gamma"],
               update_interval=case["update_interval"], agent=None, evaluator=None,
               evaluation_interval=case["evaluation_interval"], tau=case["tau"], reward_method=case["reward_method"])
    assert list(tr.evaluation_rollouts) == fx["evaluation_rollouts"].tolist()
    assert fx["eval_calls"].tolist() == fx["evaluation_rollouts"].tolist()
    if case["evaluator"] == "real":
        assert len(fx["eval_pos"]) == len(fx["eval_key"]) == len(fx["eval_calls"])


def test_get_batches_draws_like_a_shuffle():
    """`_get_batches` returns contiguous slices and moves the global NumPy stream as np.random.shuffle(np.arange(size)) does
    (the reference shuffles an index array it does not use: train.py:400-410)."""
    from librubiks.train import Train
    for size, bsize in ((6, 3), (12, 5), (128, 50), (48, 24), (7, 7)):
        np.random.seed(size)
        batches = Train._get_batches(size, bsize)
        after = np.random.get_state()
        np.random.seed(size)
        np.random.shuffle(np.arange(size))
        want = np.random.get_state()
        assert after[2] == want[2] and np.array_equal(after[1], want[1]), (size, bsize)
        assert np.array_equal(np.concatenate([np.arange(size)[b] for b in batches]), np.arange(size))
        assert all(b.stop - b.start == bsize for b in batches[:-1]) and 0 < batches[-1].stop - batches[-1].start <= bsize


@pytest.mark.parametrize("name", sorted(NUMERICS))
def test_numerics_near_ties_and_yardstick(name):
    case, fx = _case("n", name)
    close = fx["gap64"] <= META["gap"]
    share = close.mean(axis=1)
    assert share.max() <= META["max_share"] and np.allclose(share, case["share_below_gap"])
    assert np.array_equal(fx["policy32"][~close], fx["policy64"][~close])
    assert fx["value32"].dtype == np.float32 and fx["value64"].dtype == np.float64
    e = case["e_ref"]
    assert e["value"] == np.abs(fx["value32"] - fx["value64"]).max()
    for k in ("policy_losses", "value_losses"):
        assert e[k] == np.abs(fx[k + "32"] - fx[k + "64"]).max() and np.isfinite(fx[k + "64"]).all()
    d = np.abs(fx["final32"] - fx["final64"])
    # per tensor: the signed distance of the two runs' summaries, and for the two sums over the elements the root of the sum of
    # the squared per-element differences (make_golden_train.py says why); the yardstick is the larger
    assert np.array_equal(fx["e_ref_final_signed"], np.stack([d[:, 0], d[:, 1], d[:, 2:].max(axis=1)], axis=1))
    assert np.array_equal(fx["e_ref_final"], np.maximum(fx["e_ref_final_signed"], fx["e_ref_final_rss"]))
    rss = fx["e_ref_final_rss"]
    assert (rss[:, 2] == 0).all() and (rss[:, :2] >= 0).all()
    numel = 16 * 4096 * 480     # no tensor is larger: |sum of n terms| <= sqrt(n) * root sum of squares
    assert (fx["e_ref_final_signed"][:, :2] <= np.sqrt(numel) * rss[:, :2] * (1 + 1e-9) + 1e-300).all()
    assert not np.array_equal(fx["final64"], fx["init"])


def test_versions_recorded():
    assert str(_fx["torch_version"]) and str(_fx["numpy_version"])
