"""
CPU checks of what lets a grid over the exploration constant c be searched as one MCTS pool: the library exports the five
rc_mcts_*_each entry points and their ctypes signatures are registered (the scalar ones, the ABI version and rc_mcts_t's size are
what they were), argument errors are reported before anything is launched, `MCTS.search_batch` refuses a malformed per-game c
before anything touches the device, and `GridSearch` sees that a grid over c can go through the pool.
"""
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_RANGE = -1, -2, -4
NEW = ("rc_mcts_select_each", "rc_mcts_backup_select_each", "rc_mcts_backup_select_head_each", "rc_mcts_step_each",
       "rc_mcts_step_head_each")


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    from librubiks.solving import mcts_device  # noqa: F401  (registers the rc_mcts_* signatures)
    return _hip.load()


def _struct(B=4, C=100):
    """A well-formed rc_mcts_t whose pointers name no memory: every call below must fail its checks before it would use them."""
    from librubiks.solving import mcts_device as md
    s = md._McStruct()
    s.n_trees, s.capacity, s.hash_size, s.max_path = B, C, 256, 4096
    s.rows_per_tree, s.node_words, s.ring_k = md.ROWS, md.NODE_WORDS, md.RING_K
    s.path_block_log2, s.lds_levels, s.ring_levels, s.unc_list_cap = 12, 4096, 4096, 128
    s.child_stride, s.n_active = 64, B
    plain = [n for n, t in md._McStruct._fields_ if t is ctypes.c_void_p and n not in ("N", "W", "rec", "P", "nbr", "active", "mapped_rows", "path_rows")]
    for i, name in enumerate(plain):
        setattr(s, name, 0x100000 * (i + 1))
    n0 = 0x10000000   # the fields of the 256-byte node record, where the kernels' strides assume them
    s.N, s.W, s.rec, s.P, s.nbr = n0, n0 + 48, n0 + 96, n0 + 128, n0 + 176
    return s


def test_the_library_exports_the_five_entry_points_and_the_abi_stays(lib):
    from librubiks.solving import mcts_device as md
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.rc_abi_version() == 10
    assert lib.rc_mcts_struct_bytes() == ctypes.sizeof(md._McStruct) == 336


def test_the_ctypes_signatures_are_registered(lib):
    from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32, c_void_p
    from librubiks import _hip
    from librubiks.solving.mcts_device import _McStruct
    M = POINTER(_McStruct)
    scalar = {
        "rc_mcts_select": [M, c_double, c_uint32, c_void_p],
        "rc_mcts_backup_select": [M, c_void_p, c_void_p, c_double, c_uint32, c_void_p],
        "rc_mcts_backup_select_head": [M, c_void_p, c_size_t, c_int, c_double, c_uint32, c_void_p],
        "rc_mcts_step": [M, c_void_p, c_void_p, c_double, c_uint32, c_uint32, c_void_p],
        "rc_mcts_step_head": [M, c_void_p, c_size_t, c_int, c_double, c_uint32, c_uint32, c_void_p],
    }
    for name, args in scalar.items():
        assert _hip.SIGNATURES[name] == args, name                                                 # the scalar forms keep theirs
        each = [c_void_p if a is c_double else a for a in args]                                    # the twin: a pointer where c was
        assert _hip.SIGNATURES[name + "_each"] == each, name
        for n in (name, name + "_each"):
            assert list(getattr(lib, n).argtypes) == _hip.SIGNATURES[n] and getattr(lib, n).restype is ctypes.c_int


def test_the_entry_points_reject_bad_arguments_without_a_launch(lib):
    s, p, odd = _struct(), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x20004)
    m = ctypes.byref(s)
    calls = {   # name -> arguments with the struct and c_each left out: (before c_each, after c_each)
        "rc_mcts_select_each": ((), (0, None)),
        "rc_mcts_backup_select_each": ((p, p), (0, None)),
        "rc_mcts_backup_select_head_each": ((p, 16, 0), (0, None)),
        "rc_mcts_step_each": ((p, p), (0, 100, None)),
        "rc_mcts_step_head_each": ((p, 16, 0), (0, 100, None)),
    }
    for name, (pre, post) in calls.items():
        fn = getattr(lib, name)
        assert fn(None, *pre, p, *post) == RC_ERR_NULL, name
        assert fn(m, *pre, None, *post) == RC_ERR_NULL, name
        assert fn(m, *pre, odd, *post) == RC_ERR_ALIGN, name
        if pre:                                                  # the network outputs
            assert fn(m, None, *pre[1:], p, *post) == RC_ERR_NULL, name
    assert lib.rc_mcts_backup_select_each(m, p, None, p, 0, None) == RC_ERR_NULL
    assert lib.rc_mcts_backup_select_head_each(m, p, 12, 0, p, 0, None) == RC_ERR_RANGE      # ld < 13
    assert lib.rc_mcts_step_each(m, p, p, p, 0, 0, None) == RC_ERR_RANGE                    # max_states 0
    assert lib.rc_mcts_step_head_each(m, p, 16, 0, p, 0, 0, None) == RC_ERR_RANGE
    s.capacity = 5                                               # the struct's own checks come before a launch as well
    for name, (pre, post) in calls.items():
        assert getattr(lib, name)(m, *pre, p, *post) == RC_ERR_RANGE, name


G = 6
MALFORMED = {
    "wrong_length": (np.full(G + 1, 0.5), "shape"),
    "two_dimensional": (np.full((G, 1), 0.5), "shape"),
    "nan": (np.array([0.1, 0.2, np.nan, 0.1, 0.1, 0.1]), "game 2"),
    "inf": (np.array([0.1, 0.2, 0.1, 0.1, np.inf, 0.1]), "game 4"),
    "minus_inf_scalar": (-np.inf, "game 0"),
    "complex": (np.full(G, 0.5 + 1j), "real"),
    "strings": (np.array(["0.5"] * G), "real"),
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_a_malformed_per_game_c_raises_before_a_device_call(case, monkeypatch):
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving.agents import MCTS

    def no_device(*a, **k):
        raise AssertionError("the device was touched before c was checked")
    monkeypatch.setattr(DeviceCubes, "of", classmethod(no_device))
    monkeypatch.setattr(MCTS, "_forest_for", no_device)
    c, said = MALFORMED[case]
    agent = MCTS(None, c=0.6, search_graph=True)
    for call in (agent.search_batch, agent.start_batch):
        with pytest.raises(ValueError, match=said):
            call(np.zeros((G, 20), dtype=np.int8), None, 1000, c=c)


def test_a_well_formed_c_passes_the_check():
    from librubiks.solving.agents import MCTS
    agent = MCTS(None, c=0.6, search_graph=False)
    assert MCTS.sweep_parameters == ("c",)
    assert agent._per_game_c(G, None) is None
    assert agent._per_game_c(G, 0.6) is None and agent._per_game_c(G, np.float32(0.6)) is not None   # the agent's own c: the scalar path
    got = agent._per_game_c(G, 4)
    assert got.dtype == np.float64 and got.tolist() == [4.0] * G
    got = agent._per_game_c(G, [0.1, 0.6, 4, 100, 0.1, 0.6])
    assert got.dtype == np.float64 and got.tolist() == [0.1, 0.6, 4.0, 100.0, 0.1, 0.6]
    assert agent._per_game_c(G, np.full(G, 0.6)) is not None                                         # an array is never the scalar path


def test_grid_search_sees_that_a_grid_over_c_can_be_pooled():
    from librubiks.solving.agents import MCTS
    from librubiks.solving.evaluation import Evaluator
    from librubiks.solving.hyper_optim import GridSearch
    ev = Evaluator(6, [4], None, 200, slots=8)
    gs = GridSearch(None, {"c": (0.1, 100)})
    gs.objective_from_evaluator(ev, MCTS, {"net": None, "search_graph": True})
    assert gs.pooled_route_applies()
    assert gs.pooled_by_default()                                                                     # the measured choice for MCTS ...
    gs.agent_class = type("Tuned", (MCTS,), {})
    assert gs.pooled_by_default() and gs.pooled_route_applies()                                       # ... and for what derives from it
    gs = GridSearch(None, {"c": (0.1, 100), "nu": (1, 100)})                                          # not a sweepable parameter
    gs.objective_from_evaluator(ev, MCTS, {"net": None, "search_graph": True})
    assert not gs.pooled_route_applies()
    gs = GridSearch(None, {"c": (0.1, 100)})
    gs.objective_from_evaluator(Evaluator(6, [4], None, 200), MCTS, {"net": None, "search_graph": True})   # no slots
    assert not gs.pooled_route_applies()


def test_the_sweep_asks_for_the_batch_independent_form_of_the_split_engine():
    """A sweep promises the rows of one `eval` per setting; the default split engine's plan per row count does not keep that for
    MCTS, and it has a form that does."""
    import torch
    from librubiks.solving.agents import MCTS
    from librubiks.solving.evaluation import Evaluator
    from librubiks.solving.hyper_optim import GridSearch
    default = MCTS(None, c=0.6, search_graph=True)
    assert "deterministic=True" in default.sweep_refusal()
    assert MCTS(None, c=0.6, search_graph=True, deterministic=True).sweep_refusal() is None
    assert MCTS(None, c=0.6, search_graph=True, net_dtype=torch.float32).sweep_refusal() is None
    with pytest.raises(ValueError, match="deterministic=True"):        # (before a scramble is drawn or the device touched)
        Evaluator(6, [4], None, 200, slots=8).eval_sweep(default, {"c": np.array([0.5])})

    class Recording:
        max_states, slots, seen = 200, 8, []

        def eval(self, agent):
            self.seen.append(agent.c)
            return np.array([[1, -1]]), np.array([[5, 9]]), np.array([[0.1, 0.2]])

        def eval_sweep(self, agent, params):
            raise AssertionError("the automatic choice took a pool the agent refuses")
    ev = Recording()
    gs = GridSearch(None, {"c": (0.1, 100)})                            # pooled=None
    gs.objective_from_evaluator(ev, MCTS, {"net": None, "search_graph": True})
    assert gs.pooled_route_applies() and gs.optimize(3) == {"c": 0.1}
    assert ev.seen == np.linspace(0.1, 100, 3).tolist() and gs.score_history == [0.5] * 3
