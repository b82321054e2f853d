"""
The 6x8x6 networks on the folded engines, CPU side: the bridge fold of the input layer (a legal cube's 288-wide one-hot is a fixed
function of its 20 codes, so W1 becomes a 480-row table), `InferenceNet` in float64 on the CPU for fc_small / res_small / conv
(the conv branch as a torch expression of the folded weights) against the module in float64 and against what the reference's own
modules gave (tests/golden/cube686_golden.npz), the `Folded` handle's routing and fingerprint, and the new library entry point.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from formula_weights import fill, golden

ARCHS = ("fc_small", "res_small", "conv")


@pytest.fixture(scope="module")
def g():
    return golden()


def _cpu_net(arch, is2024=False, **kw):
    from librubiks.model import ConvNet, Model, ModelConfig
    config = ModelConfig(architecture=arch, is2024=is2024, **kw)
    return (ConvNet if arch == "conv" else Model)(config)   # not through create(): that moves the module to the GPU when there is one


def test_bridge_fold_of_the_input_layer_on_every_golden_pair(g):
    from librubiks.model import _fold_bridge
    W1 = fill(_cpu_net("fc_small")).shared_net[0].weight.detach().double()
    T = _fold_bridge(W1)
    assert T.shape == (W1.shape[0], 480) and T.dtype == torch.float64
    codes = torch.from_numpy(g["states2024"].astype(np.int64))
    oh = torch.from_numpy(g["states686"].reshape(-1, 288).astype(np.float64))
    assert len(codes) == 1027
    rows = T.t()[24 * torch.arange(20)[None, :] + codes]        # (n, 20, H): the rows a state's codes select
    ref = oh @ W1.t()
    err = float((rows.sum(1) - ref).abs().max()) / float(ref.abs().max())
    assert err <= 1e-12, err


@pytest.mark.parametrize("arch", ARCHS)
def test_cpu_engine_equals_the_float64_module_and_the_reference(arch, g):
    from librubiks.model import InferenceNet
    net = fill(_cpu_net(arch)).eval()
    eng = InferenceNet(net, dtype=torch.float64, device="cpu", first_layer_table="onehot")
    assert eng.encoding == "686" and eng.input_width == 288 and not eng.supports_cubes
    x = torch.from_numpy(g["states686"][g["net_idx"]].reshape(-1, 288).astype(np.float64))
    with torch.no_grad():
        p64, v64 = copy.deepcopy(net).double()(x)
    p, v = eng(x)                          # (the engine returns float32: the comparison pays one rounding of values of order 1)
    out = eng._run(eng.layers, x, x)       # ... so the 1e-10 bound is taken on the float64 result itself
    assert out.dtype == torch.float64
    assert float((out[:, :12] - p64).abs().max()) <= 1e-10 and float((out[:, 12:] - v64).abs().max()) <= 1e-10
    assert torch.equal(p, out[:, :12].float()) and torch.equal(v, out[:, 12].float())
    np.testing.assert_allclose(p.numpy(), g[f"{arch}_policy"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(v.numpy(), g[f"{arch}_value"].reshape(-1), rtol=1e-4, atol=1e-4)
    assert torch.equal(eng.value(x), v)


@pytest.mark.parametrize("batchnorm", (True, False))
def test_conv_fold_with_and_without_batchnorm(batchnorm, g):
    import torch.nn as nn
    from librubiks.model import InferenceNet
    net = fill(_cpu_net("conv", batchnorm=batchnorm, activation_function=nn.ReLU())).eval()
    eng = InferenceNet(net, dtype=torch.float64, device="cpu", first_layer_table="onehot")
    x = torch.from_numpy(g["states686"][g["net_idx"][:16]].reshape(-1, 288).astype(np.float64))
    with torch.no_grad():
        p64, v64 = copy.deepcopy(net).double()(x)
    out = eng._run(eng.layers, x, x)
    assert float((out[:, :12] - p64).abs().max()) <= 1e-10 and float((out[:, 12:] - v64).abs().max()) <= 1e-10


def test_codes_from_oh_inverts_the_bridge_and_refuses_what_is_no_cube(g):
    from librubiks.cube import cube686
    oh = torch.from_numpy(g["states686"].reshape(-1, 288).astype(np.float32))
    assert np.array_equal(cube686.codes_from_oh(oh).numpy(), g["states2024"])
    bad = oh[:4].clone()
    bad[1] = bad[1].roll(6)   # every sticker's colour moved on by one: no cubie has these colours
    with pytest.raises(ValueError, match="_cubes"):
        cube686.codes_from_oh(bad)


@pytest.mark.parametrize("arch", ("fc_small", "conv"))
def test_fingerprint_of_the_handle_follows_the_weights(arch):
    from librubiks.model import F32_SPLIT, Folded, net_fingerprint
    net = _cpu_net(arch)
    h = Folded(net)
    for dt in (F32_SPLIT, torch.bfloat16):
        fp = net_fingerprint(h, dt)
        assert fp == net_fingerprint(h, dt) == net_fingerprint(Folded(net), dt) and fp != net_fingerprint(h, torch.float32)
        p = next(net.parameters())
        # an in-place update as optimizers and load_state_dict make it (torch counts it in `_version`), and a swap of `.data` (a new
        # storage).  `p.data.add_(1)` itself is invisible to torch -- `.data` hands out a tensor with a version counter of its own --
        # for these networks exactly as for the 20x24 ones, whose fingerprint this is.
        with torch.no_grad():
            p.add_(1)
        fp2 = net_fingerprint(h, dt)
        assert fp2 != fp
        p.data = p.data + 1
        assert net_fingerprint(h, dt) != fp2
        fp2 = net_fingerprint(h, dt)
        opt = torch.optim.SGD(net.parameters(), lr=0.1)
        net.train()
        net(torch.zeros(4, 288))[0].sum().backward()
        opt.step()
        assert net_fingerprint(h, dt) != fp2
    assert net_fingerprint(net, torch.bfloat16) == (id(net), str(torch.bfloat16))   # the bare network: served live, as before


def test_routing_of_the_handle():
    from librubiks.model import F32_SPLIT, Folded, GenericNet, InferenceNet, make_inference_net, net_fingerprint
    m2024 = _cpu_net("fc_small", is2024=True)
    for dt in (torch.float32, torch.float64):
        assert type(make_inference_net(Folded(m2024), dt)) is type(make_inference_net(m2024, dt)) is InferenceNet
    assert net_fingerprint(Folded(m2024), F32_SPLIT) == net_fingerprint(m2024, F32_SPLIT)
    m686 = _cpu_net("fc_small")
    assert isinstance(make_inference_net(m686, torch.float32), GenericNet)
    eng = make_inference_net(Folded(m686), torch.float32)
    assert isinstance(eng, InferenceNet) and eng.encoding == "686" and eng.input_width == 288
    assert make_inference_net(eng) is eng
    with pytest.raises(ValueError, match="Linear"):
        Folded(torch.nn.Linear(288, 13))


def test_engines_name_what_they_cannot_fold():
    from librubiks.model import InferenceNet
    net = _cpu_net("conv")
    net.config.conv_channels = [16, 32, 64]
    with pytest.raises(ValueError, match="conv_channels"):
        InferenceNet(net, dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="Linear"):
        InferenceNet(torch.nn.Linear(480, 13), dtype=torch.float64, device="cpu")


def test_conv_branch_entry_point_is_exported_and_validates():
    from librubiks import _hip
    lib = _hip.load()
    assert hasattr(lib, "rc_conv686_branch") and "rc_conv686_branch" in _hip.SIGNATURES
    assert lib.rc_abi_version() == 10   # symbols were only added
    nw, nb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.rc_conv686_packed_floats(32, 64, 128, ctypes.byref(nw), ctypes.byref(nb)) == 0 and (nw.value, nb.value) == (31296, 224)
    assert lib.rc_conv686_packed_floats(16, 32, 64, ctypes.byref(nw), ctypes.byref(nb)) == -4
    assert lib.rc_conv686_packed_floats(32, 64, 128, None, None) == -1
    # argument validation happens on the host, in front of any launch: 16-byte aligned fake addresses are never dereferenced
    a = 1 << 20
    call = lambda soa=a, n=32, stride=32, w=a, b=a, out=a, pitch=3072, col0=2048, fmt=0, act=2, flag=None: \
        lib.rc_conv686_branch(soa, n, stride, w, b, out, pitch, col0, fmt, act, 1.0, flag, None)   # noqa: E731
    assert call(n=0) == 0
    assert call(soa=None) == -1 and call(w=None) == -1 and call(b=None) == -1 and call(out=None) == -1
    assert call(soa=a + 4) == -2 and call(out=a + 8) == -2 and call(stride=40) == -2 and call(col0=2052) == -2 and call(pitch=3076) == -2
    assert call(stride=16) == -3                     # stride < round_up(n, 16)
    assert call(pitch=3064) == -3                    # the 1 024 columns do not fit behind col0
    assert call(fmt=2, pitch=3072, col0=1024) == -3  # format 2: a row is [hi | lo], each half out_pitch / 2 wide
    assert call(fmt=3) == -4 and call(fmt=-1) == -4 and call(act=3) == -4
