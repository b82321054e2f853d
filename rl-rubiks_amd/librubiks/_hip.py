"""
ctypes binding of librubiks_hip.so (include/rubiks_hip.h).  The library is built in-tree by
`make -C rl-rubiks_amd` (or __graft_entry__.build()) into rl-rubiks_amd/lib/.

Fails loudly: a missing library, a missing symbol or a missing GPU raise -- nothing falls back to
the CPU.
"""
import ctypes
import os
from ctypes import c_char_p, c_int, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# RUBIKS_HIP_LIB: another build of the same library (same-box A/B of kernel changes); it must export the same ABI
LIB_PATH = os.environ.get("RUBIKS_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "librubiks_hip.so")

P, SZ, I = c_void_p, c_size_t, c_int

# name -> argtypes (restype is always int unless listed in _RESTYPES); mirrors include/rubiks_hip.h
SIGNATURES = {
    "rc_abi_version": [],
    "rc_error_string": [I],
    "rc_init": [I],
    "rc_get_move_table": [P],
    "rc_get_solved": [P],
    "rc_aos_to_soa": [P, P, SZ, SZ, P],
    "rc_soa_to_aos": [P, P, SZ, SZ, P],
    "rc_multi_rotate_aos": [P, P, P, SZ, P],
    "rc_is_solved_aos": [P, P, SZ, P],
    "rc_as_oh_aos_f32": [P, P, SZ, P],
    "rc_multi_rotate": [P, P, P, SZ, SZ, SZ, P],
    "rc_expand12": [P, P, SZ, SZ, SZ, P],
    "rc_expand12_flags": [P, P, SZ, SZ, SZ, P, P, P],
    "rc_is_solved": [P, P, P, P, SZ, SZ, P],
    "rc_as_oh_f32": [P, P, SZ, SZ, P],
    "rc_as_oh_bf16": [P, P, SZ, SZ, P],
    "rc_apply_moves": [P, P, SZ, SZ, SZ, P],
    "rc_sequence_states": [P, P, SZ, SZ, I, SZ, P],
    "rc_act_bf16_inplace": [P, SZ, I, ctypes.c_float, P],
    "rc_oh_split_f16": [P, SZ, SZ, P, P],
    "rc_first_layer_split_f16": [P, SZ, SZ, P, P, P, P, SZ, I, ctypes.c_float, P],
    "rc_first_layer_split_flag_f16": [P, SZ, SZ, P, P, P, P, SZ, I, ctypes.c_float, P, P],
    "rc_first_layer_gather_f16": [P, SZ, SZ, P, P, P, SZ, I, ctypes.c_float, P, P],
    "rc_first_layer_gather_rows_f16": [P, SZ, SZ, P, P, P, SZ, I, ctypes.c_float, P, P, P, I, P],
    "rc_split_act_f16": [P, P, ctypes.c_float, SZ, SZ, P, I, ctypes.c_float, P, P, P],
    "rc_split_reduce_f16": [P, SZ, I, I, SZ, SZ, P, P, I, ctypes.c_float, P, P, P, P, P, P],
    "rc_split_reduce_rows_f16": [P, SZ, I, I, SZ, SZ, P, P, I, ctypes.c_float, P, P, P, P, P, P, P],
    "rc_split_layer_f16": [P, P],
    "rc_gemm_layer_bf16": [P, P],
    "rc_split_layer_corr_chunks": [SZ, I],
    "rc_split_layer_struct_bytes": [],
    "rc_split_gemm_f16": [P, P, P, SZ, SZ, SZ, I, ctypes.c_float, P, P, I, P],
    "rc_gemm_bias_act_bf16": [P, P, P, SZ, SZ, SZ, I, ctypes.c_float, P, I, P],
    "rc_split_gemm_partials_f16": [P, P, SZ, SZ, SZ, P, P],
    "rc_head_split_f32": [P, P, ctypes.c_float, SZ, SZ, P, I, ctypes.c_float, P, P, SZ, P, P],
    "rc_head_split_rows_f32": [P, P, ctypes.c_float, SZ, SZ, P, I, ctypes.c_float, P, P, SZ, P, P, P, P],
    "rc_head_bf16": [P, SZ, SZ, P, P, SZ, P, I, ctypes.c_float, P],
    "rc_adi_targets": [P, P, P, SZ, SZ, ctypes.c_float, I, P, P, P],
    "rc_first_layer_mfma_bf16": [P, SZ, SZ, P, P, P, SZ, I, ctypes.c_float, I, P],
    # the 6x8x6 representation (csrc/rubiks_env686.hip)
    "rc686_get_perm_table": [P],
    "rc686_get_bridge_table": [P],
    "rc686_aos_to_soa": [P, P, SZ, SZ, P],
    "rc686_soa_to_aos": [P, P, SZ, SZ, P],
    "rc686_multi_rotate": [P, P, P, SZ, SZ, SZ, P],
    "rc686_expand12": [P, P, SZ, SZ, SZ, P],
    "rc686_expand12_flags": [P, P, SZ, SZ, SZ, P, P, P],
    "rc686_is_solved": [P, P, SZ, SZ, P],
    "rc686_as_oh_f32": [P, P, SZ, SZ, P],
    "rc686_as_oh_bf16": [P, P, SZ, SZ, P],
    "rc686_as_correct_f32": [P, P, SZ, SZ, P],
    "rc686_apply_moves": [P, P, SZ, SZ, SZ, SZ, P],
    "rc686_multi_rotate_aos": [P, P, P, SZ, P],
    "rc686_is_solved_aos": [P, P, SZ, P],
    "rc686_as_oh_aos_f32": [P, P, SZ, P],
    "rc_2024_to_686": [P, P, SZ, SZ, SZ, P],
    "rc_as_oh686_from2024_f32": [P, P, SZ, SZ, P],
    "rc_as_oh686_from2024_bf16": [P, P, SZ, SZ, P],
    "rc_as_correct_from2024_f32": [P, P, SZ, SZ, P],
    "rc686_as_correct_oh_f32": [P, P, SZ, P],
    "rc686_as_correct_oh_bf16": [P, P, SZ, P],
    # the conv branch of the 6x8x6 ConvNet from the code planes (csrc/rubiks_conv686.hip)
    "rc_conv686_packed_floats": [I, I, I, P, P],
    "rc_conv686_branch": [P, SZ, SZ, P, P, P, SZ, SZ, I, I, ctypes.c_float, P, P],
    # pattern mining (csrc/rubiks_patterns.hip); no search module imports it, so it is declared here: the struct pointer as void*,
    # which librubiks/analysis/pattern_mining.py replaces by its typed mirror when it is imported
    "rc_patterns_struct_bytes": [],
    "rc_patterns_table_cells": [SZ],
    "rc_patterns_workspace_bytes": [SZ],
    "rc_patterns_hash": [ctypes.c_uint64],
    "rc_patterns_begin": [P, P],
    "rc_patterns_extend": [P, P],
    "rc_patterns_close": [P, P],
    "rc_patterns_level": [P, P],
    # the near-solved table (csrc/rubiks_near.hip); no search module imports librubiks/solving/near.py, so it is declared here.
    # rc_near_t / rc_near_tighten_t go by address (ctypes.byref of near.py's mirrors)
    "rc_near_struct_bytes": [],
    "rc_near_tighten_struct_bytes": [],
    "rc_near_scan_bytes": [ctypes.c_uint32],
    "rc_near_begin": [P, P],
    "rc_near_expand": [P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, P],
    "rc_near_depth": [P, P, SZ, SZ, P, P, P, P],
    "rc_near_solve": [P, P, SZ, SZ, P, ctypes.c_uint32, P, P, P],
    "rc_near_tighten_distances": [P, P, P],
    "rc_near_tighten_route": [P, P, P],
    "rc_near_tighten": [P, P, P],
    # ... and the search beyond it (csrc/rubiks_near_reach.hip); rc_near_reach_t by address as well
    "rc_near_reach_struct_bytes": [],
    "rc_near_reach_items": [ctypes.c_uint32, ctypes.c_uint32],
    "rc_near_reach_begin": [P, P, P],
    "rc_near_reach_level": [P, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, P],
    "rc_near_reach_finish": [P, P, P],
}
_RESTYPES = {"rc_error_string": c_char_p, "rc_split_layer_struct_bytes": c_size_t, "rc_patterns_struct_bytes": c_size_t,
             "rc_patterns_table_cells": c_size_t, "rc_patterns_workspace_bytes": c_size_t, "rc_patterns_hash": ctypes.c_uint64,
             "rc_near_struct_bytes": c_size_t, "rc_near_tighten_struct_bytes": c_size_t, "rc_near_scan_bytes": c_size_t,
             "rc_near_reach_struct_bytes": c_size_t, "rc_near_reach_items": ctypes.c_uint64}

_lib = None
_initialised_devices = set()


class RubiksHipError(RuntimeError):
    pass


def register(signatures: dict, restypes: dict = None):
    """Lets the search modules declare their own entry points next to where they are used."""
    SIGNATURES.update(signatures)
    if restypes:
        _RESTYPES.update(restypes)
    if _lib is not None:
        _bind(_lib, signatures)


def _bind(lib, signatures):
    for name, argtypes in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RubiksHipError(f"librubiks_hip.so does not export {name}; rebuild it (make -C rl-rubiks_amd)") from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)


def load() -> ctypes.CDLL:
    """Loads the shared library (no GPU needed for that) and binds every declared symbol."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RubiksHipError(f"{LIB_PATH} is missing: build it with `make -C rl-rubiks_amd` "
                                 "(there is no CPU fallback for the cube environment)")
        lib = ctypes.CDLL(LIB_PATH)
        _bind(lib, SIGNATURES)
        _lib = lib
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().rc_error_string(rc).decode()
        raise RubiksHipError(f"{what or 'librubiks_hip'} failed ({rc}): {msg}")


def lib() -> ctypes.CDLL:
    """The library, initialised for the current torch CUDA(HIP) device.  Raises without a GPU."""
    l = load()
    if not torch.cuda.is_available():
        raise RubiksHipError("no MI355X visible (torch.cuda.is_available() is False): the cube "
                             "environment has no CPU path")
    dev = torch.cuda.current_device()
    if dev not in _initialised_devices:
        check(l.rc_init(dev), "rc_init")
        _initialised_devices.add(dev)
    return l


def stream_ptr() -> int:
    """hipStream_t of torch's current stream, so kernels order with torch ops and capture into graphs."""
    return torch.cuda.current_stream().cuda_stream


def ptr(t: torch.Tensor) -> int:
    return t.data_ptr()
