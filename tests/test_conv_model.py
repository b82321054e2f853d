"""
The 6x8x6 networks on the CPU: `ModelConfig(is2024=False)` for fc_* / res_* and the reference's conv architecture
(librubiks/model.py:267-338).  Names and shapes of the state_dict are the reference's (so its checkpoints load with strict=True),
and under weights from a formula (tests/formula_weights.py) the eval-mode outputs match the ones the reference's own modules gave
(tests/golden/cube686_golden.npz).
"""
import json

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from formula_weights import fill, golden, golden_meta

ARCHS = ("conv", "fc_small", "res_small")


@pytest.fixture(scope="module")
def g():
    return golden()


def _cpu_net(arch):
    from librubiks.model import ConvNet, Model, ModelConfig
    config = ModelConfig(architecture=arch, is2024=False)
    net = (ConvNet if arch == "conv" else Model)(config)   # not through create(): that moves the module to the GPU when there is one
    return net


@pytest.mark.parametrize("arch", ARCHS)
def test_state_dict_names_and_shapes_are_the_references(arch):
    net = _cpu_net(arch)
    assert [[k, list(t.shape)] for k, t in net.state_dict().items()] == golden_meta()[arch]
    assert net.config.input_width == 288 and net.shared_net[0].in_features == 288


@pytest.mark.parametrize("arch", ARCHS)
def test_cpu_outputs_match_the_reference_under_formula_weights(arch, g):
    net = fill(_cpu_net(arch)).eval()
    x = torch.from_numpy(g["states686"][g["net_idx"]].reshape(-1, 288).astype(np.float32))
    with torch.no_grad():
        p, v = net(x)
        v_only = net(x, policy=False, value=True)
    assert p.shape == (64, 12) and v.shape == (64, 1) and torch.equal(v, v_only)
    # rtol = atol = 1e-4: the tolerance tests/test_model.py uses for an fp32 module against the reference's fp32 module
    np.testing.assert_allclose(p.numpy(), g[f"{arch}_policy"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(v.numpy(), g[f"{arch}_value"], rtol=1e-4, atol=1e-4)


def test_conv_forward_takes_gradients_through_the_linear_and_conv_weights(g):
    net = fill(_cpu_net("conv")).train()
    x = torch.from_numpy(g["states686"][g["net_idx"][:8]].reshape(-1, 288).astype(np.float32))
    p, v = net(x)
    (p.sum() + v.sum()).backward()
    for name in ("shared_net.0.weight", "shared_conv_net.1.weight", "cat_net.0.weight", "policy_net.0.weight"):
        grad = dict(net.named_parameters())[name].grad
        assert grad is not None and float(grad.abs().sum()) > 0, name


def test_as_correct_on_cpu_tensors_matches_the_reference(g):
    from librubiks.cube import cube686
    out = cube686.as_correct(torch.from_numpy(g["as_oh"]))
    assert out.dtype == torch.float32 and np.array_equal(out.numpy(), g["as_correct"])


@pytest.mark.parametrize("arch", ARCHS)
def test_save_and_load_round_trip(arch, tmp_path, monkeypatch):
    import librubiks
    import librubiks.model as lm
    monkeypatch.setattr(lm, "gpu", librubiks.cpu)   # `create` and `load` place the module on `gpu`: keep this test on the CPU
    net = fill(lm.Model.create(lm.ModelConfig(architecture=arch, is2024=False)))
    net.save(str(tmp_path))
    conf = json.load(open(tmp_path / "config.json"))
    assert conf["is2024"] is False and conf["architecture"] == arch
    twin = lm.Model.load(str(tmp_path))
    assert type(twin) is type(net) and twin.config.is2024 is False
    for (k, a), (k2, b) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert k == k2 and torch.equal(a, b)
    clone = net.clone()
    assert type(clone) is type(net) and all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), clone.state_dict().values()))


def test_conv_on_the_20x24_representation_is_refused_with_the_reason():
    from librubiks.model import ModelConfig
    with pytest.raises(ValueError, match="6x8x6"):
        ModelConfig(architecture="conv")
    with pytest.raises(ValueError, match="6x8x6"):
        ModelConfig(architecture="conv", is2024=True)
    assert ModelConfig(architecture="conv", is2024=False).conv_channels == [32, 64, 128]


def test_engines_route_6x8x6_networks_to_the_live_module():
    from librubiks.model import GenericNet, make_inference_net, net_fingerprint
    net = _cpu_net("fc_small")
    eng = make_inference_net(net)
    assert isinstance(eng, GenericNet) and eng.encoding == "686" and eng.input_width == 288 and eng.input_dtype == torch.float32
    assert net_fingerprint(net, torch.bfloat16) == (id(net), str(torch.bfloat16))
    plain = GenericNet(torch.nn.Linear(480, 13))
    assert plain.encoding == "2024" and plain.input_width == 480
