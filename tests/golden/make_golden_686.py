"""
Generates tests/golden/cube686_golden.npz by IMPORTING THE REFERENCE (peleiden/rl-rubiks) with its 6x8x6 representation switched on.

Run only where a checkout of the reference is at hand (the GPU tests never run this script; they read the committed file), from a
directory other than this repository's root so that the reference's `librubiks` is the one imported:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python <this repository>/tests/golden/make_golden_686.py <reference checkout>

The fixture is DATA: states, the reference's outputs on them, names and shapes of its networks' tensors and their outputs under
weights that come from a formula of this project's own (`formula_tensor`, repeated in tests/formula_weights.py -- the conv network
has 18 M parameters, so no weights travel).  It also prints the reference's CPU throughput of `_Cube686.multi_rotate`, the Python
loop the device kernel replaces (recorded in profiles/env686_probe.txt).
"""
import json
import os
import sys
import time
import warnings

import numpy as np

warnings.filterwarnings("ignore")
OUT = os.path.dirname(os.path.abspath(__file__))
N, MOVES, SEED = 1027, 30, 686
NET_STATES = 64


def formula_tensor(index: int, key: str, shape, seed: int = SEED) -> np.ndarray:
    """Tensor number `index` (state_dict order) of a network, from np.random.RandomState(seed + index): weights of two or more
    dimensions are N(0, 1) / sqrt(fan_in); one-dimensional `weight`s (BatchNorm scales) 1 + 0.1 N(0, 1); biases and running means
    0.1 N(0, 1); running variances uniform in [0.5, 1.5); `num_batches_tracked` stays 0."""
    rng = np.random.RandomState(seed + index)
    shape = tuple(shape)
    if key.endswith("num_batches_tracked"):
        return np.zeros(shape, dtype=np.int64)
    if key.endswith("running_var"):
        return (0.5 + rng.uniform(size=shape)).astype(np.float32)
    x = rng.standard_normal(shape)
    if len(shape) >= 2:
        return (x / np.sqrt(np.prod(shape[1:]))).astype(np.float32)
    if key.endswith("weight"):
        return (1.0 + 0.1 * x).astype(np.float32)
    return (0.1 * x).astype(np.float32)


def main():
    import torch
    from librubiks import cube
    from librubiks.model import Model, ModelConfig
    fx = {}

    # (1) the same random move lists in both representations; a few solved and one-move states in front
    rng = np.random.RandomState(SEED)
    faces, dirs = rng.randint(0, 6, (MOVES, N)), rng.randint(0, 2, (MOVES, N))
    depth = np.full(N, MOVES)
    depth[:4] = 0
    depth[4:28] = 1
    faces[0, 4:28], dirs[0, 4:28] = np.repeat(np.arange(6), 4), np.tile([1, 0], 12)   # every action twice
    pair = {}
    for is2024 in (True, False):
        cube.set_is2024(is2024)
        states = np.array([cube.get_solved()] * N)
        for d in range(MOVES):
            moved = cube.multi_rotate(states, faces[d], dirs[d])
            states = np.where((d < depth).reshape((N,) + (1,) * (states.ndim - 1)), moved, states)
        pair[is2024] = states
    fx["states2024"], fx["states686"] = pair[True].astype(np.int8), pair[False].astype(np.int8)
    assert fx["states686"].shape == (N, 6, 8, 6)

    # (2) as633 agrees between the representations (the isomorphism the bridge rests on), recorded for the tests
    cube.set_is2024(True)
    nets2024 = np.array([cube.as633(s) for s in pair[True]])
    cube.set_is2024(False)
    nets686 = np.array([cube.as633(s) for s in pair[False]])
    assert np.array_equal(nets2024, nets686)
    fx["as633"] = nets686.astype(np.int8)

    # (3) environment outputs on the 6x8x6 states
    s686 = pair[False]
    mf, md = rng.randint(0, 6, N), rng.randint(0, 2, N)
    assert set(np.unique(md)) == {0, 1}
    fx["mr_faces"], fx["mr_dirs"] = mf.astype(np.uint8), md.astype(np.uint8)
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        out = cube.multi_rotate(s686, mf, md)
    rate = reps * N / (time.perf_counter() - t0)
    print(f"reference _Cube686.multi_rotate on this CPU: {rate:,.0f} states/s ({N} states, {reps} repeats)")
    fx["mr_out"] = out.astype(np.int8)
    for i in range(32):
        assert np.array_equal(cube.rotate(s686[i], mf[i], md[i]), out[i])
    ex_idx = np.concatenate([np.arange(0, 32), np.arange(N - 32, N)])   # solved, one-move (children include the solved cube) and deep states
    fx["ex_idx"] = ex_idx
    fx["ex_children"] = cube.multi_rotate(np.repeat(s686[ex_idx], 12, axis=0), *cube.iter_actions(len(ex_idx))).astype(np.int8)
    fx["is_solved"] = cube.multi_is_solved(s686)
    assert fx["is_solved"][:4].all() and not fx["is_solved"][4:28].any()
    fx["ex_children_solved"] = cube.multi_is_solved(fx["ex_children"])
    assert fx["ex_children_solved"].sum() >= 24
    oh = cube.as_oh(s686)
    assert oh.shape == (N, 288) and oh.dtype == torch.float32
    fx["as_oh"] = oh.cpu().numpy()
    fx["as_oh_single"] = cube.as_oh(s686[5]).cpu().numpy()
    fx["as_correct"] = cube.as_correct(oh).cpu().numpy()
    assert fx["as_correct"].shape == (N, 6, 8) and fx["as_correct"].dtype == np.float32
    assert cube.get_oh_shape() == 288 and cube.shape() == (6, 8, 6)
    fx["solved"] = cube.get_solved()
    fx["repeat_state"] = cube.repeat_state(s686[40], 3)

    # (4) scrambles and sequence_scrambler after np.random.seed(0 / 42)
    for seed in (0, 42):
        for d in (10, 14):
            np.random.seed(seed)
            S, Fs, Ds = [], [], []
            for _ in range(8):
                s, f, dd = cube.scramble(d, True)
                S.append(s), Fs.append(f), Ds.append(dd)
            fx[f"scr_s{seed}_d{d}_states"], fx[f"scr_s{seed}_d{d}_faces"], fx[f"scr_s{seed}_d{d}_dirs"] = np.array(S), np.array(Fs), np.array(Ds)
        for ws in (True, False):
            np.random.seed(seed)
            s, soh = cube.sequence_scrambler(4, 10, ws)
            assert np.array_equal(soh.cpu().numpy(), s.reshape(len(s), 288).astype(np.float32))
            fx[f"seq_s{seed}_ws{int(ws)}_states"] = s.astype(np.int8)

    # (5) networks: names and shapes, and eval-mode fp32 outputs under the formula weights
    net_idx = np.concatenate([np.arange(0, 16), np.arange(N - 48, N)])
    fx["net_idx"] = net_idx
    x = cube.as_oh(s686[net_idx])
    meta = {}
    for arch in ("conv", "fc_small", "res_small"):
        net = Model.create(ModelConfig(architecture=arch, is2024=False))
        sd = net.state_dict()
        meta[arch] = [[k, list(t.shape)] for k, t in sd.items()]
        net.load_state_dict({k: torch.from_numpy(formula_tensor(i, k, t.shape)) for i, (k, t) in enumerate(sd.items())}, strict=True)
        net.eval()
        with torch.no_grad():
            p, v = net(x)
        assert p.shape == (NET_STATES, 12) and v.shape == (NET_STATES, 1) and p.dtype == torch.float32
        assert np.isfinite(p.numpy()).all() and float(p.std()) > 1e-3 and float(v.std()) > 1e-3, (arch, float(p.std()), float(v.std()))
        fx[f"{arch}_policy"], fx[f"{arch}_value"] = p.numpy(), v.numpy()
        print(arch, sum(t.numel() for t in sd.values()), "values in", len(sd), "tensors; policy std", float(p.std()), "value std", float(v.std()))
    fx["meta_json"] = np.array(json.dumps(meta))

    # (6) one ADI data-generation call (16 games x depth 8, lapanfix, alpha 0.5) after np.random.seed(3), under the formula weights:
    # as the reference runs it (fp32) and with the module in float64; their distance is the yardstick e_ref of the test
    # (tests/golden/make_golden_train.py does the same for the 20x24 training runs)
    import types
    from librubiks.solving.agents import PolicySearch
    from librubiks.train import Train
    adi = {}
    plain_as_correct = cube.as_correct
    for arch in ("conv", "fc_small"):
        runs = {}
        for double in (False, True):
            net = Model.create(ModelConfig(architecture=arch, is2024=False))
            net.load_state_dict({k: torch.from_numpy(formula_tensor(i, k, t.shape)) for i, (k, t) in enumerate(net.state_dict().items())})
            if double:
                net.double()
                plain = type(net).forward
                net.forward = types.MethodType(lambda self, x, policy=True, value=True, plain=plain: plain(self, x.double(), policy, value), net)
                cube.as_correct = lambda t: plain_as_correct(t).double()   # the conv net's +-1 input follows the module's dtype
            train = Train(rollouts=1, batch_size=50, rollout_games=16, rollout_depth=8, optim_fn=None, alpha_update=0.0, lr=1e-3, gamma=1.0,
                          update_interval=0, agent=PolicySearch(None), evaluator=None, evaluation_interval=0, with_analysis=False, tau=1.0,
                          reward_method="lapanfix")
            np.random.seed(3)
            with torch.no_grad():
                oh, policy, value, weights = train.ADI_traindata(net, 0.5)
                states = oh.cpu().numpy().reshape(-1, 6, 8, 6).astype(np.int8)
                substates = cube.multi_rotate(np.repeat(states, 12, axis=0), *cube.iter_actions(len(states)))
                rewards = np.where(cube.multi_is_solved(substates), 1.0, -1.0)
                values = net(cube.as_oh(substates), policy=False, value=True).double().numpy().reshape(-1) + rewards
            cube.as_correct = plain_as_correct
            top = np.sort(values.reshape(-1, 12), axis=1)
            runs[double] = {"states": states, "policy": policy.numpy().copy(), "value": value.double().numpy().copy(),
                            "weights": weights.numpy().copy(), "gap": top[:, -1] - top[:, -2]}
        r32, r64 = runs[False], runs[True]
        assert np.array_equal(r32["states"], r64["states"]) and r32["states"].shape == (128, 6, 8, 6)
        assert np.array_equal(values.reshape(-1, 12).argmax(1), r64["policy"])
        fx[f"adi_{arch}_states"], fx[f"adi_{arch}_weights"] = r32["states"], r32["weights"]
        fx[f"adi_{arch}_policy64"], fx[f"adi_{arch}_value64"], fx[f"adi_{arch}_gap64"] = r64["policy"], r64["value"], r64["gap"]
        fx[f"adi_{arch}_policy32"], fx[f"adi_{arch}_value32"] = r32["policy"], r32["value"].astype(np.float32)
        adi[arch] = {"e_ref_value": float(np.abs(r32["value"] - r64["value"]).max()), "smallest_gap": float(r64["gap"].min())}
        print("ADI", arch, adi[arch], "policy agreement fp32/float64", float((r32["policy"] == r64["policy"]).mean()))
    fx["adi_json"] = np.array(json.dumps(adi))

    path = os.path.join(OUT, "cube686_golden.npz")
    np.savez_compressed(path, **fx)
    print("cube686_golden.npz:", os.path.getsize(path), "bytes;", {k: v.shape for k, v in fx.items()})


if __name__ == "__main__":
    assert len(sys.argv) == 2 and os.path.isdir(os.path.join(sys.argv[1], "librubiks")), "usage: make_golden_686.py <reference checkout>"
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    main()
