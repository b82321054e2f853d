"""
CPU checks of the device entry points behind the lock-step rollout agents (rc_rollout_plant, rc_rollout_step_policy,
rc_rollout_step_value): the struct is the header's, argument errors are reported before anything is launched, so they need no
GPU, and the ABI version stays where callers built against it expect it (symbols were only added).
"""
import ctypes

import pytest

import conftest  # noqa: F401  (puts the package on sys.path)

RC_ERR_NULL, RC_ERR_ALIGN, RC_ERR_STRIDE, RC_ERR_RANGE = -1, -2, -3, -4
VALUE_ONLY = ("kids_soa", "kid_solved")


@pytest.fixture(scope="module")
def lib():
    from librubiks import _hip
    from librubiks.solving import rollout_device  # noqa: F401  (registers the rc_rollout_* signatures)
    return _hip.load()


def _struct(S=40, Q=8, **over):
    """A well-formed rc_rollout_t whose pointers name no memory: every call below must fail its checks before it would use them."""
    from librubiks.solving.rollout_device import _RoStruct
    s = _RoStruct()
    s.n_slots, s.queue_width, s.stride = S, Q, 256
    for i, (name, _) in enumerate(_RoStruct._fields_[3:]):
        setattr(s, name, 0x1000 * (i + 1))
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _bad_structs(children: bool):
    """(struct, code) for every way the batch description itself can be wrong."""
    from librubiks.solving.rollout_device import _RoStruct
    names = [name for name, _ in _RoStruct._fields_[3:] if children or name not in VALUE_ONLY]
    out = [(_struct(**{name: None}), RC_ERR_NULL) for name in names]
    out += [(_struct(S=0), RC_ERR_RANGE), (_struct(Q=0), RC_ERR_RANGE), (_struct(states_soa=0x1004), RC_ERR_ALIGN),
            (_struct(stride=264), RC_ERR_ALIGN), (_struct(S=300), RC_ERR_STRIDE)]        # 300 games need 304 bytes per plane
    if children:
        out += [(_struct(kids_soa=0x2008), RC_ERR_ALIGN), (_struct(kid_solved=0x3004), RC_ERR_ALIGN)]
    return out


def test_abi_version_stays_10_and_the_entry_points_exist(lib):
    from librubiks.solving.rollout_device import _RoStruct
    assert lib.rc_abi_version() == 10
    for name in ("rc_rollout_struct_bytes", "rc_rollout_plant", "rc_rollout_step_policy", "rc_rollout_step_value", "rc_rollout_seed",
                 "rc_rollout_draw"):
        assert hasattr(lib, name)
    assert lib.rc_rollout_struct_bytes() == ctypes.sizeof(_RoStruct) == 64


def test_step_policy_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    ok = lambda st=s, head=p, ld=13, bf=0, dec=p, uni=p, cap=30: lib.rc_rollout_step_policy(  # noqa: E731
        None if st is None else ctypes.byref(st), head, ld, bf, dec, uni, cap, None)
    assert ok(st=None) == RC_ERR_NULL
    assert ok(head=None, dec=None, uni=None) == RC_ERR_NULL                                 # nothing to take an action from
    assert ok(head=None, uni=p) == RC_ERR_NULL                                              # uniforms without a policy
    assert ok(head=ctypes.c_void_p(0x10002)) == RC_ERR_ALIGN                                # float rows
    assert ok(head=ctypes.c_void_p(0x10001), bf=1) == RC_ERR_ALIGN
    assert ok(uni=ctypes.c_void_p(0x10004)) == RC_ERR_ALIGN                                 # doubles
    assert ok(ld=12) == RC_ERR_RANGE                                                        # what the engines write has 13 columns
    assert ok(cap=0) == RC_ERR_RANGE
    for bad, code in _bad_structs(False):
        assert ok(st=bad) == code
    assert ok(st=_struct(kids_soa=None, kid_solved=None), cap=0) == RC_ERR_RANGE            # the policy step needs no children


def test_step_value_rejects_bad_arguments_without_a_launch(lib):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    assert lib.rc_rollout_step_value(None, p, 30, None) == RC_ERR_NULL
    assert lib.rc_rollout_step_value(ctypes.byref(s), None, 30, None) == RC_ERR_NULL
    assert lib.rc_rollout_step_value(ctypes.byref(s), ctypes.c_void_p(0x10002), 30, None) == RC_ERR_ALIGN
    assert lib.rc_rollout_step_value(ctypes.byref(s), p, 0, None) == RC_ERR_RANGE
    for bad, code in _bad_structs(True):
        assert lib.rc_rollout_step_value(ctypes.byref(bad), p, 30, None) == code


@pytest.mark.parametrize("children", [0, 1])
def test_plant_rejects_bad_arguments_without_a_launch(lib, children):
    s, p = _struct(), ctypes.c_void_p(0x10000)
    plant = lambda st=s, slots=p, n=1, roots=p, stride=16, first=0: lib.rc_rollout_plant(  # noqa: E731
        None if st is None else ctypes.byref(st), slots, n, roots, stride, first, children, None)
    assert plant(st=None) == RC_ERR_NULL
    assert plant(slots=None) == RC_ERR_NULL and plant(slots=None, n=0) == RC_ERR_NULL and plant(roots=None) == RC_ERR_NULL
    assert plant(roots=ctypes.c_void_p(0x10004)) == RC_ERR_ALIGN and plant(stride=24) == RC_ERR_ALIGN
    assert plant(n=41, stride=64) == RC_ERR_RANGE                                          # more slots than S
    assert plant(n=2, first=15) == RC_ERR_RANGE and plant(first=17) == RC_ERR_RANGE        # columns beyond the stride
    assert plant(first=2 ** 64 - 1) == RC_ERR_RANGE
    for bad, code in _bad_structs(bool(children)):
        assert plant(st=bad) == code
    assert plant(n=0) == 0                                                                  # nothing to plant: nothing is launched
