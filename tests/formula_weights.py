"""
Weights from a formula, shared by the 6x8x6 tests: the same function tests/golden/make_golden_686.py used to fill the reference's
networks before it recorded their outputs (the conv network has 18 M parameters, so no weights are committed).
"""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cube686_golden.npz")
SEED = 686


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


def fill(net: torch.nn.Module) -> torch.nn.Module:
    """Overwrites every parameter and buffer of `net` from the formula (strict load: the names are the module's own)."""
    sd = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(formula_tensor(i, k, t.shape)).to(t.device) for i, (k, t) in enumerate(sd.items())}, strict=True)
    return net


def golden():
    return np.load(GOLDEN)


def golden_meta() -> dict:
    return json.loads(str(golden()["meta_json"]))
