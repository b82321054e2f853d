"""
The 6x8x6 networks on the bf16 and f16x3 engines (`Folded(net)`): the conv-branch kernel rc_conv686_branch against the float64
torch expression of the same folded weights, its reproducibility per state, its range flag; the engines of fc_small / res_small /
conv against the float64 module and the reference's recorded outputs (tests/golden/cube686_golden.npz) with the tolerances
tests/test_net_gpu.py states (split: 1.25 x the fp32 module's own error + 1e-7 scale; fp32 chain 1e-4 scale; bf16 4e-2 scale,
scale = max(1, max |output|)); the bridge fold as exactly a 20x24 network; the search agents on the folded engines.
Weights come from the formula in tests/formula_weights.py.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402,F401
from formula_weights import fill, golden  # noqa: E402

TILE = 16   # states per workgroup of rc_conv686_branch (csrc/rubiks_conv686.hip, kCvStates)
FORMATS = (0, 1, 2)


# =================================================================================================
# The kernel
# =================================================================================================
@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def states(g):
    """353 of the golden pairs (20 codes) and the (353, 6, 8) correctness map of the same cubes, float64, on the host."""
    from librubiks.cube import cube686
    codes = np.ascontiguousarray(g["states2024"][:353])
    x = cube686.as_correct(torch.from_numpy(g["states686"][:353].reshape(-1, 288).astype(np.float64)))
    return codes, x


_branches = {}


def _branch(act: str, batchnorm: bool):
    """(folded float64 layers, activation module, packed weights, packed biases on the GPU) of a formula-filled ConvNet."""
    from librubiks.model import ConvNet, ModelConfig, _fold_conv, pack_conv686
    key = (act, batchnorm)
    if key not in _branches:
        fn = nn.ELU(alpha=float(act[3:] or 1.0)) if act.startswith("elu") else nn.ReLU()
        net = fill(ConvNet(ModelConfig(architecture="conv", is2024=False, batchnorm=batchnorm, activation_function=fn))).eval()
        with torch.no_grad():
            convs, last = _fold_conv(net.shared_conv_net)
        assert (last is not None) == batchnorm and [tuple(W.shape) for W, _ in convs] == [(32, 6, 3), (64, 32, 3), (128, 64, 3)]
        w, b = pack_conv686(convs)
        _branches[key] = (convs, fn, w.cuda(), b.cuda())
    return _branches[key]


def _launch(cubes, w, b, fmt, act, n=None, lo=0, pitch=1024, col0=0, flag=None, fill_value=None):
    """rc_conv686_branch on rows lo .. lo + n of `cubes`; returns the raw (n, pitch) buffer (format 2: (n, 2 pitch) halves)."""
    from librubiks import _hip
    n = cubes.n - lo if n is None else n
    dtype = (torch.float32, torch.bfloat16, torch.float16)[fmt]
    width = 2 * pitch if fmt == 2 else pitch
    out = torch.empty((n, width), dtype=dtype, device="cuda") if fill_value is None else torch.full((n, width), fill_value, dtype=dtype, device="cuda")
    code, alpha = (2, float(act[3:] or 1.0)) if act.startswith("elu") else ({"none": 0, "relu": 1}[act], 1.0)   # "elu0.37": ELU(alpha = 0.37)
    _hip.check(_hip.lib().rc_conv686_branch(cubes.soa.data_ptr() + lo, n, cubes.stride, w.data_ptr(), b.data_ptr(), out.data_ptr(), width, col0,
                                            fmt, code, alpha, None if flag is None else flag.data_ptr(), _hip.stream_ptr()), "rc_conv686_branch")
    return out


def _value(out, fmt, col0=0):
    """float64 (n, 1024) of a raw buffer: formats 0 / 1 as they are, format 2 reassembled hi + lo 2^-11."""
    if fmt != 2:
        return out[:, col0:col0 + 1024].double().cpu()
    half = out.shape[1] // 2
    return (out[:, col0:col0 + 1024].double() + out[:, half + col0:half + col0 + 1024].double() / 2048.0).cpu()


@pytest.mark.parametrize("batchnorm", (True, False))
@pytest.mark.parametrize("act", ("elu", "relu", "elu0.37"))
def test_kernel_against_the_float64_expression(act, batchnorm, states):
    from librubiks.cube import DeviceCubes
    from librubiks.model import _conv_branch_torch
    codes, x64 = states
    convs, fn, w, b = _branch(act, batchnorm)
    with torch.no_grad():
        y64 = _conv_branch_torch(x64, convs, fn)
        y32 = _conv_branch_torch(x64.float(), [(W.float(), c.float()) for W, c in convs], fn).double()
    e32, scale = float((y32 - y64).abs().max()), max(1.0, float(y64.abs().max()))
    batch64 = DeviceCubes.from_numpy(codes[:64])
    launches = [(DeviceCubes.from_numpy(codes[:n]), 0, n, 0) for n in (1, TILE - 1, TILE + 1, 353)] + [(batch64, 16, 37, 16)]
    for cubes, lo, n, first in launches:
        ref = y64[first:first + n]
        for fmt in FORMATS:
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            got = _value(_launch(cubes, w, b, fmt, act, n=n, lo=lo, flag=flag), fmt)
            err = (got - ref).abs()
            print(f"{act} bn={batchnorm} n={n} lo={lo} format {fmt}: max |err| {float(err.max()):.3e}, torch fp32 {e32:.3e}, |y| <= {scale:.2f}")
            bound = 1.25 * e32 + 1e-7 * scale
            if fmt == 1:
                assert bool((err <= bound + 2.0 ** -8 * ref.abs()).all())   # one bf16 rounding, a factor 2 of slack
            else:
                assert float(err.max()) <= bound
            assert int(flag.item()) == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_writes_its_block_and_nothing_else(fmt, states):
    from librubiks.cube import DeviceCubes
    codes, _ = states
    _, _, w, b = _branch("elu", True)
    cubes = DeviceCubes.from_numpy(codes[:TILE + 1])
    plain = _launch(cubes, w, b, fmt, "elu")
    sentinel = -7.0
    wide = _launch(cubes, w, b, fmt, "elu", pitch=3072, col0=2048, fill_value=sentinel)
    blocks = [(0, 1024)] if fmt != 2 else [(0, 1024), (1024, 2048)]
    mask = torch.ones_like(wide, dtype=torch.bool)
    for i, (lo, hi) in enumerate(blocks):
        at = 2048 + i * 3072
        assert torch.equal(wide[:, at:at + 1024], plain[:, lo:hi])
        mask[:, at:at + 1024] = False
    assert bool((wide[mask] == sentinel).all())


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_state_has_the_same_bits_in_every_launch(fmt, states):
    from librubiks.cube import DeviceCubes
    codes, _ = states
    _, _, w, b = _branch("elu", True)
    whole = _launch(DeviceCubes.from_numpy(codes), w, b, fmt, "elu")
    for r in (0, 20, 352):
        alone = _launch(DeviceCubes.from_numpy(codes[r:r + 1]), w, b, fmt, "elu")
        assert torch.equal(alone[0], whole[r]), r
    window = _launch(DeviceCubes.from_numpy(codes[:64]), w, b, fmt, "elu", n=37, lo=16)
    assert torch.equal(window, whole[16:53])


def test_range_flag(states):
    from librubiks.cube import DeviceCubes
    from librubiks.model import pack_conv686
    codes, _ = states
    convs, _, w, b = _branch("elu", True)
    cubes = DeviceCubes.from_numpy(codes[:TILE + 1])
    big, big_b = (t.cuda() for t in pack_conv686(convs[:2] + [(convs[2][0] * 1e6, convs[2][1])]))
    inf_b = b.clone()
    inf_b[-1] = float("inf")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for fmt, weights, biases, expect in ((2, w, b, 0), (1, w, b, 0), (2, big, big_b, 1),   # beyond +-65 504: the split format cannot hold it
                                         (1, big, big_b, 0),                                # ... bf16 can
                                         (1, w, inf_b, 1), (2, w, inf_b, 1), (0, w, inf_b, 0)):
        flag.zero_()
        _launch(cubes, weights, biases, fmt, "elu", flag=flag)
        assert int(flag.item()) == expect, (fmt, expect)


# =================================================================================================
# The engines
# =================================================================================================
ARCHS = ("fc_small", "res_small", "conv")
ROWS = (300, 5632, 11264)   # the row counts at which tests/test_net_gpu.py crosses the layer plans
_cases = {}


def _case(arch):
    """The formula-filled network on the GPU, and per batch: cubes, float64 module outputs, the fp32 module's own error."""
    from librubiks import cube
    from librubiks.cube import DeviceCubes
    from librubiks.model import Model, ModelConfig
    if arch not in _cases:
        net = fill(Model.create(ModelConfig(architecture=arch, is2024=False))).eval()
        ref64 = copy.deepcopy(net).double()
        g = golden()
        np.random.seed(686)
        batches = {"golden": DeviceCubes.from_numpy(np.ascontiguousarray(g["states2024"][g["net_idx"]]))}
        for n in ROWS:
            batches[n] = cube.scramble_batch(n, 25, True)[0]
        out = {}
        for name, cubes in batches.items():
            oh = cubes.as_oh686(torch.float32)
            with torch.no_grad():
                p64, v64 = ref64(oh.double())
                p32, v32 = net(oh)
            v64 = v64.reshape(-1)
            e_f32 = max(float((p32.double() - p64).abs().max()), float((v32.reshape(-1).double() - v64).abs().max()))
            out[name] = (cubes, p64, v64, e_f32, max(1.0, float(p64.abs().max()), float(v64.abs().max())))
        del ref64
        _cases[arch] = (net, out)
    return _cases[arch]


def _dtypes():
    from librubiks.model import F32_SPLIT
    return {"f32s": F32_SPLIT, "fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.mark.parametrize("which", ("f32s", "fp32", "bf16"))
@pytest.mark.parametrize("arch", ARCHS)
def test_engines_against_the_float64_module_and_the_reference(arch, which, g):
    from librubiks.model import Folded, GenericNet, InferenceNet, SplitF32Net, make_inference_net
    from librubiks.solving.agents import _evaluate, _values
    net, batches = _case(arch)
    eng = make_inference_net(Folded(net), _dtypes()[which])
    assert isinstance(eng, SplitF32Net if which == "f32s" else InferenceNet) and not isinstance(eng, GenericNet)
    assert (eng.encoding, eng.input_width) == ("686", 288)
    assert bool(eng.supports_cubes) == (which != "fp32")
    err = lambda a, b: float((a.double() - b).abs().max())   # noqa: E731
    for name, (cubes, p64, v64, e_f32, scale) in batches.items():
        p, v = _evaluate(eng, cubes)
        e = max(err(p, p64), err(v, v64))
        e_v = err(_values(eng, cubes), v64)
        bound = {"f32s": 1.25 * e_f32 + 1e-7 * scale, "fp32": 1e-4 * scale, "bf16": 4e-2 * scale}[which]
        print(f"{arch} {which} {name}: |out| <= {scale:.2f}; max |err| vs float64 {e:.3e} (value head alone {e_v:.3e}), fp32 module {e_f32:.3e}, bound {bound:.3e}")
        assert e <= bound and e_v <= bound
        if which == "f32s":
            assert not eng.overflowed()
        if name == "golden" and which != "bf16":
            np.testing.assert_allclose(p.cpu().numpy(), g[f"{arch}_policy"], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{arch}_value"].reshape(-1), rtol=1e-4, atol=1e-4)
        if name == 5632 and which != "fp32":
            # a window of the batch against the same rows of the full call: the layer plan follows the row count, the rows agree within
            # fp32 rounding (the rule of test_split_f32_engine_is_at_least_as_accurate_as_fp32) / within the bf16 tolerance
            win, full = eng.value_cubes(cubes, None, 1024, 512), eng.value_cubes(cubes)[1024:1536]
            tol = 2e-6 * max(1.0, float(full.abs().max())) if which == "f32s" else 4e-2 * scale
            assert float((win - full).abs().max()) <= tol


def test_one_hot_entry_points_of_the_conv_engines(g):
    """`eng(oh)` / `eng.value(oh)` on a 288-wide one-hot: the conv branch comes from the states the one-hot encodes (the bridge
    inverted in torch); the deterministic engine runs its fused input layer from them as well, bit for bit what forward_cubes gives,
    and a batch that is no cube state is refused with the *_cubes methods named."""
    from librubiks.model import F32_SPLIT, F32_SPLIT_DET, Folded, make_inference_net
    net, batches = _case("conv")
    cubes, p64, v64, e_f32, scale = batches["golden"]
    oh = cubes.as_oh686(torch.float32)
    for dt in (F32_SPLIT, F32_SPLIT_DET, torch.bfloat16):
        eng = make_inference_net(Folded(net), dt)
        p, v = eng(oh.to(eng.input_dtype))
        bound = 4e-2 * scale if dt == torch.bfloat16 else 1.25 * e_f32 + 1e-7 * scale
        assert float((p.double() - p64).abs().max()) <= bound and float((v.double() - v64).abs().max()) <= bound
        assert float((eng.value(oh.to(eng.input_dtype)).double() - v64).abs().max()) <= bound
        if dt == F32_SPLIT_DET:
            pc, vc = eng.forward_cubes(cubes)
            assert torch.equal(p, pc) and torch.equal(v, vc)
            alone = eng.forward_cubes(type(cubes).from_numpy(cubes.numpy()[5:6]))
            assert torch.equal(alone[0][0], pc[5]) and torch.equal(alone[1][0], vc[5])
            with pytest.raises(ValueError, match="_cubes"):
                eng(oh.roll(6, 1))


def test_the_fold_is_exactly_a_20x24_network():
    from librubiks import cube
    from librubiks.model import Model, ModelConfig, SplitF32Net, InferenceNet, _bridge_matrix
    net686, _ = _case("fc_small")
    twin = Model.create(ModelConfig(architecture="fc_small", is2024=True)).eval()
    sd = {k: v.clone() for k, v in net686.state_dict().items()}
    sd["shared_net.0.weight"] = (sd["shared_net.0.weight"].double() @ _bridge_matrix().cuda()).float()
    twin.load_state_dict(sd, strict=True)
    np.random.seed(3)
    cubes = cube.scramble_batch(300, 25, True)[0]
    a, b = SplitF32Net(net686), SplitF32Net(twin)
    assert a.gather_input and b.gather_input
    (pa, va), (pb, vb) = a.forward_cubes(cubes), b.forward_cubes(cubes)
    assert torch.equal(pa, pb) and torch.equal(va, vb)
    (pa, va), (pb, vb) = InferenceNet(net686).forward_cubes(cubes), InferenceNet(twin).forward_cubes(cubes)
    scale = max(1.0, float(pb.abs().max()), float(vb.abs().max()))
    assert float((pa - pb).abs().max()) <= 4e-2 * scale and float((va - vb).abs().max()) <= 4e-2 * scale


# =================================================================================================
# The agents
# =================================================================================================
@pytest.fixture(scope="module")
def scrambles():
    from librubiks import cube
    np.random.seed(686)
    cubes, _, _ = cube.scramble_batch(8, 6, True)
    return cubes.numpy()


def _replays(states, res):
    from librubiks import cube
    assert res.solved.dtype == bool
    for game in np.flatnonzero(res.solved):
        s = states[game]
        assert len(res.queues[game]) == res.lengths[game]
        for action in res.queues[game]:
            s = cube.rotate(s, *cube.action_space[action])
        assert cube.is_solved(s), f"game {game}: the reported solution does not solve its scramble"


def _on_the_fused_path(holder):
    from librubiks.model import GenericNet
    assert not isinstance(holder.engine, GenericNet) and holder.engine.supports_cubes and holder.engine.encoding == "686"
    assert holder._oh is None, "a one-hot buffer was allocated"
    assert getattr(holder, "_fused", True)


@pytest.mark.parametrize("which", ("f32s", "bf16"))
@pytest.mark.parametrize("arch", ("conv", "fc_small"))
def test_agents_search_on_the_folded_engines(arch, which, scrambles):
    from librubiks.model import Folded
    from librubiks.solving.agents import AStar, EGVM, MCTS, ValueSearch
    net, dt = Folded(_case(arch)[0]), _dtypes()[which]
    for slots in (None, 4):
        agent = MCTS(net, c=0.6, search_graph=True, net_dtype=dt)
        res = agent.search_batch(scrambles, None, 2000, slots=slots)
        _replays(scrambles, res)
        _on_the_fused_path(agent.forest)
        assert (res.nodes > 12).all() or res.solved.any()
        agent = AStar(net, lambda_=0.2, expansions=10, net_dtype=dt)
        _replays(scrambles, agent.search_batch(scrambles, None, 2000, slots=slots))
        _on_the_fused_path(agent.batch)
    agent = EGVM(net, epsilon=0.375, workers=10, depth=6, net_dtype=dt)
    _replays(scrambles, agent.search_batch(scrambles, None, 600, seeds=7))
    _on_the_fused_path(agent.batch)
    agent = ValueSearch(net, net_dtype=dt)
    _replays(scrambles, agent.search_batch(scrambles, None, 30))
    assert agent._engine.supports_cubes and agent._engine.encoding == "686"


@pytest.mark.parametrize("arch", ("conv", "fc_small"))
def test_deterministic_mcts_is_the_same_in_a_batch_on_four_slots_and_alone(arch, scrambles):
    from librubiks.model import F32_SPLIT_DET, Folded
    from librubiks.solving.agents import MCTS
    mk = lambda: MCTS(Folded(_case(arch)[0]), c=0.6, search_graph=True, deterministic=True)   # noqa: E731
    agent = mk()
    res = agent.search_batch(scrambles, None, 2000)
    assert agent.forest.engine.dtype == F32_SPLIT_DET and agent.forest._fused
    pooled = mk().search_batch(scrambles, None, 2000, slots=4)
    for name in ("nodes", "solved", "lengths", "iterations", "status"):
        assert np.array_equal(getattr(res, name), getattr(pooled, name)), name
    assert [list(q) for q in res.queues] == [list(q) for q in pooled.queues]
    alone = mk()
    for t in range(len(scrambles)):
        assert alone.search(scrambles[t], None, 2000) == bool(res.solved[t]) and len(alone) == res.nodes[t]
        assert list(alone.action_queue) == list(res.queues[t])


def test_conv_mcts_trees_equal_the_oracle_on_the_recorded_outputs(scrambles):
    """MCTS on the conv network's split engine, rebuilt node for node by the oracle on the network outputs the trees recorded."""
    from test_search_edge_gpu import _TableNet, _compare
    from librubiks.model import Folded
    from librubiks.solving.agents import MCTS
    from oracle import agents as oa
    agent = MCTS(Folded(_case("conv")[0]), c=0.6, search_graph=True)
    res = agent.search_batch(scrambles, None, 400, compact=False)
    assert agent.forest._fused and agent.forest.engine._conv is not None
    for t in range(len(scrambles)):
        tree = agent.forest.tree_arrays(t)
        n = tree["n"]
        table = {tree["states"][i].tobytes(): (tree["P"][i].astype(np.float32), np.float32(tree["V"][i])) for i in range(1, n + 1)}
        ref = oa.MCTS(_TableNet(table), c=0.6, search_graph=True)
        ok = ref.search(scrambles[t], 400)
        assert bool(res.solved[t]) == ok and res.nodes[t] == len(ref) == n and list(res.queues[t]) == list(ref.action_queue)
        _compare(tree, ref, n)
