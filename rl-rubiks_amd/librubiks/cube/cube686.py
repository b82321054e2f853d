"""
The reference's stateless cube API in its 6x8x6 representation (librubiks/cube/cube.py with `set_is2024(False)`: the
dispatchers at :41-234 over `_Cube686`, :311-388) on MI355X.

Same function names, shapes and dtypes as the reference gives under that flag: a state is int8 (6,8,6), the one-hot colour
of the 8 non-centre stickers of each face; batches are (n,6,8,6); `as_oh` is the 288-wide float32 one-hot on `librubiks.gpu`.
Inputs are never mutated.  The reference chooses the representation through a process-wide flag; here it is this namespace
(`from librubiks.cube import cube686`) and, for networks, `ModelConfig(is2024=False)` -- `cube.set_is2024(False)` stays
refused, so no caller's 20x24 code changes meaning behind its back.

Every function that computes states runs as a HIP kernel (csrc/rubiks_env686.hip) over 48 sticker planes (`DeviceCubes686`);
small calls go through pinned staging buffers in one launch.  The two representations describe the same cubes: `from2024` /
`to2024` convert on the host, `DeviceCubes.to686()` / `.as_oh686()` on the device, and the search agents keep their 20-byte
states whichever network they serve.
"""
import numpy as np
import torch

from librubiks import _hip, gpu
from librubiks.cube import cube as _c2024
from librubiks.cube.cube import (F, B, T, D, L, R, action_names, action_space, action_dim, dtype, _actions_of, _padded_actions,  # noqa: F401
                                 iter_actions, indices_to_actions, rev_action, rev_actions, SMALL_CALL)
from librubiks.cube.device import DeviceCubes686, OH_WIDTH_686

_SHAPE = (6, 8, 6)


###########################
# Tables, read back from the library (no GPU needed)
###########################
_tables = None


def get_perm_table() -> np.ndarray:
    """uint8[12, 48]: action a moves sticker perm[a, s] onto sticker s (sticker f*8+p)."""
    buf = np.empty(12 * 48, dtype=np.uint8)
    _hip.check(_hip.load().rc686_get_perm_table(buf.ctypes.data), "rc686_get_perm_table")
    return buf.reshape(12, 48)


def get_bridge_table() -> np.ndarray:
    """uint8[20, 24, 3, 2]: (sticker, colour) pair k of cubie i with code v; sticker 255 = no such pair."""
    buf = np.empty(20 * 24 * 3 * 2, dtype=np.uint8)
    _hip.check(_hip.load().rc686_get_bridge_table(buf.ctypes.data), "rc686_get_bridge_table")
    return buf.reshape(20, 24, 3, 2)


def _host_tables():
    """(stickers int[20,24,3], colours int[20,24,3], inverse uint8[20 positions, 216] -> cubie, orientation) for the converters."""
    global _tables
    if _tables is None:
        bridge = get_bridge_table().astype(np.int64)
        stickers, colours = bridge[..., 0], bridge[..., 1]
        # position q (corner q < 8: codes 3q..3q+2; edge q - 8: codes 2(q-8)..) shows the colour tuple of exactly one (cubie, orientation)
        pos_stickers = np.zeros((20, 3), dtype=np.int64)
        inverse = np.full((20, 216, 2), -1, dtype=np.int64)
        for q in range(20):
            corner = q < 8
            per, lo, hi, k = (3, 0, 8, 3) if corner else (2, 8, 20, 2)
            pos = q if corner else q - 8
            pos_stickers[q, :k] = stickers[lo, per * pos, :k]
            for i in range(lo, hi):
                for o in range(per):
                    c = colours[i, per * pos + o]
                    key = c[0] * 36 + c[1] * 6 + (c[2] if corner else 0)
                    inverse[q, key] = (i, o)
        _tables = stickers, colours, pos_stickers, inverse
    return _tables


def from2024(states: np.ndarray) -> np.ndarray:
    """(n,20) or (20,) codes -> the same cubes as (n,6,8,6) / (6,8,6) int8 one-hot, in NumPy (the bridge table on the host)."""
    states = np.asarray(states)
    single = states.ndim == 1
    s = states.reshape(-1, 20).astype(np.int64)
    stickers, colours, _, _ = _host_tables()
    n = len(s)
    col = np.zeros((n, 48), dtype=np.int64)
    rows = np.arange(n)
    for i in range(20):
        for k in range(3 if i < 8 else 2):
            col[rows, stickers[i, s[:, i], k]] = colours[i, s[:, i], k]
    out = (col[:, :, None] == np.arange(6)).astype(dtype).reshape(n, 6, 8, 6)
    return out[0] if single else out


def to2024(states686: np.ndarray) -> np.ndarray:
    """(n,6,8,6) or (6,8,6) one-hot -> (n,20) / (20,) int8 codes: the bridge inverted -- the colours a corner or edge position shows
    name the cubie sitting there and its orientation."""
    states686 = np.asarray(states686)
    single = states686.ndim == 3
    col = states686.reshape(-1, 48, 6).argmax(2).astype(np.int64)
    _, _, pos_stickers, inverse = _host_tables()
    out = np.zeros((len(col), 20), dtype=dtype)
    for q in range(20):
        corner = q < 8
        key = col[:, pos_stickers[q, 0]] * 36 + col[:, pos_stickers[q, 1]] * 6 + (col[:, pos_stickers[q, 2]] if corner else 0)
        who = inverse[q, key]
        assert (who[:, 0] >= 0).all(), "not a cube state: a position shows colours no cubie has"
        out[np.arange(len(col)), who[:, 0]] = (3 * q if corner else 2 * (q - 8)) + who[:, 1]
    return out[0] if single else out


_torch_tables = {}


def codes_from_oh(oh: torch.Tensor, check: bool = True) -> torch.Tensor:
    """(n,288) one-hot tensor -> (n,20) int8 codes on the same device: `to2024` in torch (the bridge inverted by table lookups, no
    host round trip; safe inside a graph capture with check=False).  check: raise ValueError unless every row is a cube state."""
    assert oh.dim() == 2 and oh.shape[1] == OH_WIDTH_686, f"expected (n,288), got {tuple(oh.shape)}"
    tabs = _torch_tables.get(oh.device)
    if tabs is None:
        _, _, pos_stickers, inverse = _host_tables()
        q = np.arange(20)
        tabs = _torch_tables[oh.device] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(oh.device) for a in (
            pos_stickers, inverse, (q < 8).astype(np.int64), np.where(q < 8, 3 * q, 2 * (q - 8)), q))
    pos_stickers, inverse, corner, base, q = tabs
    col = oh.reshape(len(oh), 48, 6).argmax(2)
    c = col[:, pos_stickers]                                          # (n, 20 positions, 3 stickers)
    who = inverse[q[None, :], c[..., 0] * 36 + c[..., 1] * 6 + c[..., 2] * corner]   # (n, 20, 2): cubie, orientation
    if check and not bool((who[..., 0].sort(1).values == q).all()):
        raise ValueError("not a batch of 6x8x6 one-hot cube states (a position shows colours no cubie has, or a cubie sits twice): "
                         "evaluate device states with the engine's forward_cubes / head_cubes / value_cubes instead")
    codes = torch.zeros((len(oh), 20), dtype=torch.int64, device=oh.device)
    codes.scatter_(1, who[..., 0].clamp_min(0), base[None, :] + who[..., 1])
    return codes.to(torch.int8)


###########################
# Staging for small calls
###########################
class _Staging:
    """Pinned host buffers for calls with a handful of states: one memcpy in, one launch, one synchronisation (see cube.py)."""

    def __init__(self):
        self.cap = 0

    def get(self, n: int):
        if n > self.cap:
            self.cap = max(256, 1 << int(np.ceil(np.log2(n))))
            self.states = torch.empty((self.cap, OH_WIDTH_686), dtype=torch.int8, pin_memory=True)
            self.out = torch.empty((self.cap, OH_WIDTH_686), dtype=torch.int8, pin_memory=True)
            self.actions = torch.empty(self.cap, dtype=torch.uint8, pin_memory=True)
            self.flags = torch.empty(self.cap, dtype=torch.uint8, pin_memory=True)
            self.np_states, self.np_out = self.states.numpy(), self.out.numpy()
            self.np_actions, self.np_flags = self.actions.numpy(), self.flags.numpy()
        return self


_staging = _Staging()
SMALL_CALL_686 = SMALL_CALL // 8   # rows are 288 bytes, not 20: the one-launch form gives way to the planes sooner


def _batch(states: np.ndarray) -> np.ndarray:
    states = np.asarray(states)
    assert states.ndim == 4 and states.shape[1:] == _SHAPE, f"expected (n,6,8,6) states, got {states.shape}"
    return states


################
# Rotate logic #   reference cube.py:41-52,330-361
################
def rotate(state: np.ndarray, face: int, direction: int) -> np.ndarray:
    return multi_rotate(np.asarray(state)[None], np.array([face]), np.array([direction]))[0]


def multi_rotate(states: np.ndarray, faces: np.ndarray, directions: np.ndarray) -> np.ndarray:
    """Performs action (faces[i], directions[i]) on states[i]."""
    states = _batch(states)
    n = len(states)
    if n == 0:
        _hip.lib()
        return np.empty((0,) + _SHAPE, dtype=dtype)
    assert len(faces) == n and len(directions) == n
    if n <= SMALL_CALL_686:
        lib, st = _hip.lib(), _staging.get(n)
        st.np_states[:n] = states.reshape(n, OH_WIDTH_686)
        st.np_actions[:n] = _actions_of(faces, directions)
        stream = torch.cuda.current_stream()
        _hip.check(lib.rc686_multi_rotate_aos(st.states.data_ptr(), st.actions.data_ptr(), st.out.data_ptr(), n, stream.cuda_stream),
                   "rc686_multi_rotate_aos")
        stream.synchronize()
        return st.np_out[:n].reshape((n,) + _SHAPE).copy()
    cubes = DeviceCubes686.from_numpy(states)
    return cubes.multi_rotate(_padded_actions(_actions_of(faces, directions), n)).numpy()


#################
# Solving logic #   reference cube.py:67-89
#################
_solved686 = None


def get_solved_instance() -> np.ndarray:
    """The module's own solved array -- read-only by convention, like the reference's."""
    global _solved686
    if _solved686 is None:
        _solved686 = np.zeros(_SHAPE, dtype=dtype)
        for i in range(6):
            _solved686[i, :, i] = 1
    return _solved686


def get_solved() -> np.ndarray:
    return get_solved_instance().copy()


def is_solved(state: np.ndarray) -> bool:
    return bool(multi_is_solved(np.asarray(state)[None])[0])


def multi_is_solved(states: np.ndarray) -> np.ndarray:
    states = _batch(states)
    n = len(states)
    if n == 0:
        _hip.lib()
        return np.zeros(0, dtype=bool)
    if n <= SMALL_CALL_686:
        lib, st = _hip.lib(), _staging.get(n)
        st.np_states[:n] = states.reshape(n, OH_WIDTH_686)
        stream = torch.cuda.current_stream()
        _hip.check(lib.rc686_is_solved_aos(st.states.data_ptr(), st.flags.data_ptr(), n, stream.cuda_stream), "rc686_is_solved_aos")
        stream.synchronize()
        return st.np_flags[:n].astype(bool)
    return DeviceCubes686.from_numpy(states).is_solved().cpu().numpy()


########################
# Representation logic #   reference cube.py:127-147,363-380
########################
def get_is2024() -> bool:
    return False


def shape():
    return _SHAPE


def get_oh_shape() -> int:
    return OH_WIDTH_686


def as_oh(states: np.ndarray) -> torch.Tensor:
    """n states -> (n,288) float32 one-hot on `librubiks.gpu`; a single state gives (1,288)."""
    states = np.asarray(states)
    if states.ndim == 3:
        states = states[None]
    states = _batch(states)
    n = len(states)
    if n == 0:
        _hip.lib()
        return torch.zeros((0, OH_WIDTH_686), device=gpu)
    if n <= SMALL_CALL_686:
        lib, st = _hip.lib(), _staging.get(n)
        st.np_states[:n] = states.reshape(n, OH_WIDTH_686)
        out = torch.empty((n, OH_WIDTH_686), dtype=torch.float32, device=gpu)
        stream = torch.cuda.current_stream()
        _hip.check(lib.rc686_as_oh_aos_f32(st.states.data_ptr(), out.data_ptr(), n, stream.cuda_stream), "rc686_as_oh_aos_f32")
        stream.synchronize()
        return out
    return DeviceCubes686.from_numpy(states).as_oh(torch.float32)


def as_correct(t: torch.Tensor) -> torch.Tensor:
    """(n,288) one-hot tensor as `as_oh` gives it -> (n,6,8) correctness form: +1 where a sticker has its face's colour, -1 elsewhere
    (reference cube.py:135-137,372-380).  A HIP kernel on device tensors (float32 / bfloat16, result in the same dtype); the same
    expression in torch on CPU tensors.  The comparison carries no gradient either way."""
    assert t.dim() == 2 and t.shape[1] == OH_WIDTH_686, f"expected (n,288), got {tuple(t.shape)}"
    if t.is_cuda and t.dtype in (torch.float32, torch.bfloat16):
        lib = _hip.lib()
        x = t.detach().contiguous()
        out = torch.empty((len(x), 6, 8), dtype=x.dtype, device=x.device)
        fn = lib.rc686_as_correct_oh_f32 if x.dtype == torch.float32 else lib.rc686_as_correct_oh_bf16
        _hip.check(fn(x.data_ptr(), out.data_ptr(), len(x), _hip.stream_ptr()), "rc686_as_correct_oh")
        return out
    solved = torch.from_numpy(get_solved_instance()).to(t.device)
    ok = (t.detach().reshape(len(t), 6, 8, 6) == solved).all(dim=3)
    return torch.where(ok, 1.0, -1.0).to(t.dtype if t.is_floating_point() else torch.float32)


def repeat_state(state: np.ndarray, n: int = action_dim) -> np.ndarray:
    return np.tile(state, [n, 1, 1, 1])


##################
# Scramble logic #   reference cube.py:206-234: the draws of the 20x24 functions, which are the reference's; the same cubes, converted on the device
##################
def scramble_batch(games: int, depth, force_not_solved: bool = False):
    """(DeviceCubes686, faces, dirs): `games` scrambles in the reference's np.random draw order (see cube.scramble_batch)."""
    cubes, faces, dirs = _c2024.scramble_batch(games, depth, force_not_solved)
    return cubes.to686(), faces, dirs


def scramble(depth: int, force_not_solved=False):
    """(state int8[6,8,6], faces, dirs) exactly as the reference returns them."""
    cubes, faces, dirs = scramble_batch(1, depth, force_not_solved)
    return cubes.numpy()[0], faces[0], dirs[0]


def sequence_scrambler_device(games: int, depth: int, with_solved: bool) -> DeviceCubes686:
    return _c2024.sequence_scrambler_device(games, depth, with_solved).to686()


def sequence_scrambler(games: int, depth: int, with_solved: bool):
    """(int8[games*depth, 6, 8, 6] game-major states, float32 one-hot[games*depth, 288] on gpu)."""
    cubes = _c2024.sequence_scrambler_device(games, depth, with_solved)
    return cubes.to686().numpy(), cubes.as_oh686(torch.float32)


############
# Printing #   reference cube.py:149-173,383-388 (host only)
############
_RING_CELL = np.array([0, 3, 6, 7, 8, 5, 2, 1])   # ring position -> 3*row + col (csrc/rubiks_tables686.h)
_RING_START = np.array([0, 6, 6, 4, 2, 4])        # sticker p of face f sits at ring position (p - start[f]) mod 8


def as633(state: np.ndarray) -> np.ndarray:
    """Sticker colours int[6,3,3], faces in order F, B, T, D, L, R."""
    colours = np.asarray(state).reshape(6, 8, 6).argmax(2)
    net = np.repeat(np.arange(6), 9).reshape(6, 9)
    for f in range(6):
        net[f, _RING_CELL] = colours[f, (np.arange(8) + _RING_START[f]) % 8]
    return net.reshape(6, 3, 3)


def as69(state: np.ndarray) -> np.ndarray:
    return as633(state).reshape((6, 9))


def stringify(state: np.ndarray) -> str:
    net = as633(state)
    canvas = np.full((9, 12), " ", dtype="<U1")
    for face, (br, bc) in {T: (0, 1), L: (1, 0), F: (1, 1), R: (1, 2), B: (1, 3), D: (2, 1)}.items():
        canvas[3 * br:3 * br + 3, 3 * bc:3 * bc + 3] = net[face].astype(str)
    return "\n".join(" ".join(row) for row in canvas)
