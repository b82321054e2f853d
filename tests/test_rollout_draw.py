"""
rc_rollout_draw against NumPy, on the CPU: a game's draws are its own np.random.RandomState's -- `randint(12)` bytes (mode 0) and
`random_sample` doubles (mode 1, the one number np.random.choice consumes), bit for bit, round after round across the generator's
624-word refill -- and the generator is left where NumPy leaves it.
"""
import numpy as np
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)

N_SEEDS, ROUNDS = 200, 5


@pytest.fixture(scope="module")
def rd():
    from librubiks.solving import rollout_device
    return rollout_device


def _streams(seeds):
    from librubiks.solving.egvm_device import GameStreams
    st = GameStreams(seeds)
    st.start(np.arange(len(seeds)))
    return st


def test_the_two_stream_facts_the_kernels_rest_on():
    """`randint(12, size=K)` is K scalar `np.random.randint(12)` calls, and `np.random.choice(n, p=p32)` is one random_sample
    looked up in the normalised double cumulative sum of p."""
    np.random.seed(5)
    many = np.random.randint(12, size=50)
    np.random.seed(5)
    assert many.tolist() == [int(np.random.randint(12)) for _ in range(50)]
    rs = np.random.RandomState(9)
    for i in range(200):
        p = rs.rand(12).astype(np.float32)
        p /= p.sum()
        p = (p / p.sum()).astype(np.float32)
        a, b = np.random.RandomState(i), np.random.RandomState(i)
        try:
            got = a.choice(12, p=p)
        except ValueError:      # (a float32 vector whose double sum misses 1 by more than choice's tolerance)
            continue
        cdf = p.astype(np.float64).cumsum()
        cdf /= cdf[-1]
        assert got == cdf.searchsorted(b.random_sample(), side="right")
        assert a.get_state()[2] == b.get_state()[2]


@pytest.mark.parametrize("steps", [1, 7, 64])
@pytest.mark.parametrize("mode", ["randint", "random_sample"])
def test_draws_equal_numpy(rd, steps, mode):
    seeds = np.arange(N_SEEDS, dtype=np.int64) * 7919 + 3
    st = _streams(seeds)
    ref = [np.random.RandomState(int(s)) for s in seeds]
    dtype = np.uint8 if mode == "randint" else np.float64
    games = np.arange(0, N_SEEDS, 2)                 # every other game plays; game g in column (3 g) % stride
    stride = 608
    slots = (3 * games) % stride
    assert len(set(slots.tolist())) == len(slots)
    idle = np.setdiff1d(np.arange(stride), slots)
    rounds = ROUNDS if mode == "random_sample" else 2 * ROUNDS   # (a byte takes one 32-bit output or more, a double two)
    for r in range(rounds):
        table = np.full((steps, stride), 77, dtype=dtype)
        rd.draw(st, games, slots, table)
        for g, c in zip(games, slots):
            want = ref[g].randint(12, size=steps) if mode == "randint" else ref[g].random_sample(steps)
            assert np.array_equal(table[:, c], want.astype(dtype)), (r, g)
        assert (table[:, idle] == 77).all()           # columns of games that are not listed are not touched
    for g in range(N_SEEDS):                          # key and pos as RandomState.get_state() has them; idle games never moved
        _, key, pos = (ref[g] if g in games else np.random.RandomState(int(seeds[g]))).get_state()[:3]
        assert np.array_equal(st.keys[g], key) and st.pos[g] == pos, g
    if steps == 64:                                   # every listed game went through the 624-word refill in mid-stream
        assert rounds * steps * (2 if mode == "random_sample" else 1) > 624


def test_seeding_equals_numpy(rd):
    """rc_rollout_seed leaves what np.random.RandomState(seed) starts with, for the listed games only."""
    from librubiks import _hip
    from librubiks.solving.egvm_device import GameStreams
    seeds = np.concatenate([[0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.random.RandomState(3).randint(0, 2 ** 31 - 1, N_SEEDS)]).astype(np.int64)
    st = GameStreams(seeds)
    listed = np.arange(0, len(seeds), 3)
    st.keys[:] = 7
    rd.start(st, listed)
    for g in range(len(seeds)):
        if g in listed:
            assert st.state(g)[2] == 624 and np.array_equal(st.keys[g], np.random.RandomState(int(seeds[g])).get_state()[1]), g
            assert np.random.RandomState(int(seeds[g])).randint(12, size=5).tolist() == _next_bytes(rd, st, g, 5)
        else:
            assert (st.keys[g] == 7).all()
    for bad in (-1, 2 ** 32):                         # NumPy: "Seed must be between 0 and 2**32 - 1"
        st = GameStreams(np.array([5, bad], dtype=np.int64))
        with pytest.raises(_hip.RubiksHipError):
            rd.start(st, [0, 1])
        assert not st.keys.any()
        rd.start(st, [0])


def _next_bytes(rd, st, g, n):
    table = np.zeros((n, 16), dtype=np.uint8)
    rd.draw(st, [g], [0], table)
    return table[:, 0].tolist()


def test_draw_rejects_bad_arguments(rd):
    from librubiks import _hip
    lib = _hip.load()
    st = _streams(np.arange(3))
    table = np.zeros((4, 16), dtype=np.float64)
    g = np.array([0, 2], dtype=np.int32)
    k, p, t = st.keys.ctypes.data, st.pos.ctypes.data, table.ctypes.data
    call = lambda **kw: lib.rc_rollout_draw(*[kw.get(n, d) for n, d in (("keys", k), ("pos", p), ("n_games", 3), ("games", g.ctypes.data),  # noqa: E731
                                                                        ("slots", g.ctypes.data), ("n", 2), ("mode", 1), ("steps", 4),
                                                                        ("table", t), ("stride", 16))])
    before = (st.keys.copy(), st.pos.copy())
    assert call(keys=None) == -1 and call(pos=None) == -1 and call(table=None) == -1 and call(games=None) == -1 and call(slots=None) == -1
    assert call(table=t + 4) == -2                                    # doubles
    assert call(mode=2) == -4 and call(mode=-1) == -4 and call(steps=0) == -4
    assert call(n_games=2) == -4                                      # game 2 does not exist
    assert call(stride=2) == -4                                       # slot 2 is beyond the row
    bad = np.array([0, -1], dtype=np.int32)
    assert call(games=bad.ctypes.data) == -4 and call(slots=bad.ctypes.data) == -4
    st.pos[2] = 625
    assert call() == -4
    st.pos[2] = before[1][2]
    assert np.array_equal(st.keys, before[0]) and np.array_equal(st.pos, before[1]) and not table.any()   # nothing was drawn
    assert call(n=0, games=None, slots=None) == 0
