"""
The search agents and the ADI data generation on 6x8x6 networks (`ModelConfig(is2024=False)`: the conv architecture and fc_small).

The searches keep their 20-byte states; only the network input changes -- `librubiks.cube.device.encode` picks
rc_as_oh686_from2024_* for an engine whose `encoding` is "686".  Every search here runs the SAME torch module along two routes:
through that encoder, and through `Via2024`, a wrapper that takes the 480-wide one-hot of the 20x24 encoder, re-encodes it to 288
in torch with the host bridge table and is served as an ordinary 20x24 `GenericNet`.  Both routes hand the module identical
inputs at identical batch shapes in one process, so the two `BatchResult`s are equal field for field, and every reported
solution, replayed, solves its scramble.  Weights come from the formula in tests/formula_weights.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402,F401
from formula_weights import fill  # noqa: E402


class Via2024(torch.nn.Module):
    """`inner` (a 6x8x6 network) behind the 20x24 one-hot: codes = argmax per cubie, stickers and colours from the bridge table."""

    def __init__(self, inner):
        super().__init__()
        from librubiks.cube import cube686
        self.inner = inner
        bridge = cube686.get_bridge_table().astype(np.int64)                       # [20, 24, 3, (sticker, colour)]
        index = np.where(bridge[..., 0] < 48, bridge[..., 0] * 6 + bridge[..., 1], 288)   # 288: a column that is cut off again
        self.register_buffer("index", torch.from_numpy(index.reshape(480, 3)))
        self.register_buffer("offset", torch.arange(20) * 24)

    def forward(self, x, policy=True, value=True):
        n = len(x)
        codes = x.reshape(n, 20, 24).argmax(2) + self.offset
        oh = torch.zeros((n, 289), dtype=torch.float32, device=x.device).scatter_(1, self.index[codes].reshape(n, 60), 1.0)
        return self.inner(oh[:, :288].contiguous(), policy=policy, value=value)


@pytest.fixture(scope="module", params=["conv", "fc_small"])
def nets(request):
    from librubiks.model import GenericNet, Model, ModelConfig, make_inference_net
    net = fill(Model.create(ModelConfig(architecture=request.param, is2024=False))).eval()
    via = Via2024(net).cuda().eval()
    a, b = make_inference_net(net), make_inference_net(via)
    assert isinstance(a, GenericNet) and (a.encoding, a.input_width) == ("686", 288)
    assert isinstance(b, GenericNet) and (b.encoding, b.input_width) == ("2024", 480)
    return net, via


@pytest.fixture(scope="module")
def scrambles():
    from librubiks import cube
    np.random.seed(686)
    cubes, _, _ = cube.scramble_batch(8, 6, True)
    return cubes.numpy()


def _same(a, b):
    for field in ("solved", "lengths", "nodes", "iterations", "status"):
        assert np.array_equal(getattr(a, field), getattr(b, field)), field
    assert [list(q) for q in a.queues] == [list(q) for q in b.queues]


def _replays(states, res):
    from librubiks import cube
    assert res.solved.dtype == bool
    for g in np.flatnonzero(res.solved):
        s = states[g]
        assert len(res.queues[g]) == res.lengths[g]
        for action in res.queues[g]:
            s = cube.rotate(s, *cube.action_space[action])
        assert cube.is_solved(s), f"game {g}: the reported solution does not solve its scramble"


def test_both_routes_feed_the_module_the_same_rows(nets, scrambles):
    from librubiks.cube import DeviceCubes, cube686
    from librubiks.cube.device import encode
    from librubiks.model import GenericNet
    net, via = nets
    cubes = DeviceCubes.from_numpy(scrambles)
    oh = encode(GenericNet(net), cubes)
    assert oh.shape == (8, 288) and np.array_equal(oh.cpu().numpy(), cube686.from2024(scrambles).reshape(8, 288))
    pa, va = GenericNet(net)(oh)
    pb, vb = GenericNet(via)(encode(GenericNet(via), cubes))
    assert torch.equal(pa, pb) and torch.equal(va, vb)


def test_mcts(nets, scrambles):
    from librubiks.solving.agents import MCTS
    res = [MCTS(n, c=0.6, search_graph=True).search_batch(scrambles, None, 2000) for n in nets]   # graph capture on (the default)
    _same(*res)
    _replays(scrambles, res[0])
    assert (res[0].nodes > 12).all() or res[0].solved.any()
    pooled = [MCTS(n, c=0.6, search_graph=True).search_batch(scrambles, None, 2000, slots=4) for n in nets]
    _same(*pooled)
    _replays(scrambles, pooled[0])


def test_astar(nets, scrambles):
    from librubiks.solving.agents import AStar
    res = [AStar(n, lambda_=0.2, expansions=10).search_batch(scrambles, None, 2000) for n in nets]
    _same(*res)
    _replays(scrambles, res[0])
    pooled = [AStar(n, lambda_=0.2, expansions=10).search_batch(scrambles, None, 2000, slots=4) for n in nets]
    _same(*pooled)
    _replays(scrambles, pooled[0])


def test_egvm_with_seeds(nets, scrambles):
    from librubiks.solving.agents import EGVM
    res = [EGVM(n, epsilon=0.375, workers=10, depth=6).search_batch(scrambles, None, 600, seeds=7) for n in nets]
    _same(*res)
    _replays(scrambles, res[0])


def test_value_search(nets, scrambles):
    from librubiks.solving.agents import ValueSearch
    res = [ValueSearch(n).search_batch(scrambles, None, 30) for n in nets]
    _same(*res)
    _replays(scrambles, res[0])


def test_adi_data_generation(nets):
    """One data-generation call at 16 games x depth 8 (lapanfix) after np.random.seed(3), as tests/golden/make_golden_686.py ran the
    reference's: the training states are the reference's, 288 wide; the targets are held to the reference's float64 run with the
    helper and tolerance of tests/test_train_parity_gpu.py (4 e_ref + 4 ulp of the magnitude, policy targets wherever the float64
    run's best two substates are further apart than the recorded gap); and they equal those of the same module served through the
    20x24 route bit for bit."""
    import json
    from formula_weights import golden
    from test_train_parity_gpu import _tolerance
    from train_parity import META
    from librubiks.solving.agents import PolicySearch
    from librubiks.train import Train
    net, via = nets
    arch = net.config.architecture
    g = golden()
    out = []
    for n in (net, via):
        train = Train(rollouts=1, batch_size=50, rollout_games=16, rollout_depth=8, optim_fn=None, alpha_update=0.0, lr=1e-3, gamma=1.0,
                      update_interval=0, agent=PolicySearch(None), evaluator=None, evaluation_interval=0, reward_method="lapanfix")
        np.random.seed(3)
        out.append(train.ADI_traindata(n, 0.5))
    oh, policy, value, weights = out[0]
    assert oh.shape == (128, 288) and oh.dtype == torch.float32
    assert np.array_equal(oh.cpu().numpy(), g[f"adi_{arch}_states"].reshape(128, 288))
    assert np.array_equal(weights.cpu().numpy(), g[f"adi_{arch}_weights"])
    decided = g[f"adi_{arch}_gap64"] > META["gap"]
    assert 1 - decided.mean() <= META["max_share"]
    assert (policy.cpu().numpy() == g[f"adi_{arch}_policy64"])[decided].all()
    value64 = g[f"adi_{arch}_value64"]
    e_ref = json.loads(str(g["adi_json"]))[arch]["e_ref_value"]
    distance, tol = np.abs(value.cpu().numpy().astype(np.float64) - value64).max(), _tolerance(e_ref, np.abs(value64).max())
    print(f"{arch}: value targets |product - float64| = {distance:.3e}, e_ref = {e_ref:.3e}, tolerance {tol:.3e}")
    assert distance <= tol
    assert out[1][0].shape == (128, 480)
    for a, b in zip(out[0][1:], out[1][1:]):     # policy targets, value targets, loss weights: the same module, the same rows
        assert torch.equal(a, b)


def test_saved_6x8x6_networks_load_into_the_agents(tmp_path, scrambles):
    """A checkpoint directory (model.pt + config.json with "is2024": false) loads through Model.load, and from_saved agents run on it."""
    from librubiks.model import ConvNet, Model, ModelConfig
    from librubiks.solving.agents import AStar, MCTS
    for arch in ("conv", "fc_small"):
        loc = str(tmp_path / arch)
        fill(Model.create(ModelConfig(architecture=arch, is2024=False))).save(loc)
        agent = MCTS.from_saved(loc, False, c=0.6, search_graph=True)
        assert agent.net.config.is2024 is False and isinstance(agent.net, ConvNet) == (arch == "conv")
        res = agent.search_batch(scrambles[:2], None, 200)
        _replays(scrambles[:2], res)
        res = AStar.from_saved(loc, False, lambda_=0.2, expansions=10).search_batch(scrambles[:2], None, 200)
        _replays(scrambles[:2], res)
