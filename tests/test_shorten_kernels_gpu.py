"""
The rc_shorten_* kernels against tests/shorten_model.py after EVERY launch and on every array the header defines: keys, ids,
neighbour rows, claim and parent words, both frontiers, the outputs and the statuses, each array between guard bytes and
pre-filled so that what a launch must not write is seen to be still there.  Hash cells are compared through look-ups of every
position's state (their placement depends on the order of the inserts).  One ragged batch holds the model test's cases together
with unselected games, empty queues, a queue with a byte that is no action and a game whose search takes dozens of compaction
passes; a second batch has an output row one byte too short.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shorten_model as sm  # noqa: E402
from oracle import agents as oa  # noqa: E402

GUARD, FILL = 256, 0xA5
WORKSPACE = ("keys", "ids", "nbr", "claim", "frontier_a", "frontier_b", "hash", "out_queues", "out_lens", "status")
STEPS = {"rc_shorten_index": sm.index, "rc_shorten_neighbours": sm.neighbours, "rc_shorten_bfs": sm.bfs}


def _guarded(batch):
    """Moves every array a launch writes between GUARD bytes of FILL, itself filled with FILL."""
    bufs = {}
    for name in WORKSPACE:
        t = getattr(batch, name)
        nbytes = t.numel() * t.element_size()
        buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=t.device)
        inner = buf[GUARD:GUARD + nbytes].view(t.dtype).view(t.shape)
        setattr(batch, name, inner)
        setattr(batch.struct, name, inner.data_ptr())
        bufs[name] = (buf, nbytes)
    return bufs


def _guards_intact(bufs):
    for name, (buf, nbytes) in bufs.items():
        h = buf.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + nbytes:] == FILL).all(), f"{name}: bytes outside the array were written"


def _device_batch(model: sm.Batch):
    from librubiks.cube.device import DeviceCubes
    from librubiks.solving.shorten import ShortenBatch
    roots = DeviceCubes.from_numpy(model.roots)
    roots.soa[:, model.G:] = 0x7f                                  # the padding columns of the planes hold no state
    batch = ShortenBatch(roots, model.queues, model.lens, model.select, out_width=model.out_width)
    assert (batch.pos_off_h == model.pos_off).all() and (batch.hash_off_h == model.hash_off).all()
    assert (batch.P, batch.H, batch.max_len) == (model.P, model.H, model.max_len)
    return batch, _guarded(batch)


def _host(batch, name):
    a = getattr(batch, name).cpu().numpy()
    return a.view(np.uint32) if name == "keys" else a


def _compare(batch, model, names, step):
    for name in names:
        got, want = _host(batch, name), getattr(model, name)
        bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
        assert len(bad) == 0, f"after {step}: {name} differs in rows {bad[:8]} ({len(bad)} rows): {got[bad[0]]} != {want[bad[0]]}"


def _compare_tables(batch, model):
    cells, keys = batch.hash.cpu().numpy(), _host(batch, "keys")
    for g in range(model.G):
        if model.status[g] != sm.OK:
            continue
        L, p0 = model.game(g)
        h0, h1 = int(model.hash_off[g]), int(model.hash_off[g + 1])
        tab, gk = cells[h0:h1], keys[p0:p0 + L + 1]
        for p in range(L + 1):
            assert sm.lookup(tab, gk, gk[p]) == model.ids[p0 + p], f"game {g}, position {p}"
        assert np.count_nonzero(tab) == len(model.tables[g])          # one cell per state: equal states met in one


def _run_and_compare(model: sm.Batch):
    batch, bufs = _device_batch(model)
    for step, fn in STEPS.items():
        batch.step(step)
        torch.cuda.synchronize()
        fn(model)
        _compare(batch, model, WORKSPACE[:6] + WORKSPACE[7:], step)    # arrays no launch has written yet still hold FILL on both sides
        if step == "rc_shorten_index":
            _compare_tables(batch, model)
        _guards_intact(bufs)
    return batch


@pytest.fixture(scope="module")
def cases(standin_net):
    from test_egvm_batch_gpu import MAIN, inputs, oracle_games
    seed, n, depth_of, solved_at, eps, W, D, cap, _ = MAIN
    states, seeds = inputs(seed, n, depth_of, solved_at)
    games = oracle_games(oa.TorchNet(standin_net, device="cpu"), states, seeds, eps, W, D, cap)
    egvm = [(f"egvm {g}", states[g], games[g][2]) for g in range(n) if games[g][0]]
    assert len(egvm) == 29
    return sm.small_cases() + sm.ball_cases() + sm.walk_cases() + [sm.long_case()] + egvm


def test_every_launch_against_the_model(cases):
    names = [c[0] for c in cases]
    roots, queues, select = [c[1] for c in cases], [list(c[2]) for c in cases], [1] * len(cases)
    # ragged extras: games left alone (one of them with a byte that would be a bad action), empty queues, a bad action
    s = sm.scrambled(21)
    for name, q, sel in (("unselected", [0, 2, 4], 0), ("unselected bad", [0, 200, 4], 0), ("empty a", [], 1), ("bad action", [3, 5, 12, 7], 1),
                         ("empty b", [], 1), ("bad last byte", [3, 5, 7, 255], 1), ("byte behind the length", [3, 5], 1)):
        names.append(name), roots.append(s), queues.append(q), select.append(sel)
    order = np.random.RandomState(4).permutation(len(names))                      # long and short games next to each other
    names, roots, queues, select = ([x[i] for i in order] for x in (names, roots, queues, select))
    model = sm.Batch(roots, queues, select, fill=FILL)
    g_behind = names.index("byte behind the length")
    model.queues[g_behind, 2] = 99                                                 # not inside the length: not looked at
    batch = _run_and_compare(model)
    assert batch.G == len(names) and batch.roots.stride > batch.G

    at = {name: g for g, name in enumerate(names)}
    st, c = model.status, model.counts
    for name in ("unselected", "unselected bad"):
        assert st[at[name]] == sm.SKIPPED and c[at[name]] == {"skipped": 1}
    for name in ("bad action", "bad last byte"):
        assert st[at[name]] == sm.BAD_ACTION and c[at[name]] == {"bad_action": 1}
    for name in ("empty a", "empty b", "there and back", "one move four times", "empty"):
        assert st[at[name]] == sm.OK and c[at[name]]["target_is_root"] == 1 and model.out_lens[at[name]] == 0
    assert model.result(g_behind) == [3, 5] and c[g_behind]["same_length"] == 1
    assert model.result(at["commuting shortcut"]) == [sm.B] and model.result(at["two routes, FIFO decides"]) == [sm.F, sm.B]
    assert c[at["depth-2 ball"]]["nodes"] == 127 and c[at["depth-3 ball"]]["nodes"] == 1195
    g_long = at["depth-3 ball and one move beyond"]
    assert c[g_long]["levels"] == 4 and c[g_long]["passes"] == 1 + 1 + 6 + 51 and c[g_long]["visited_skipped"] > 1000 and model.out_lens[g_long] == 4
    for name in ("walk 1", "walk 2"):
        assert c[at[name]]["revisits"] > 500 and c[at[name]]["shorter"] == 1 and c[at[name]]["levels"] > 50
    shrunk = sorted((len(queues[at[n]]), int(model.out_lens[at[n]])) for n in names if n.startswith("egvm") and c[at[n]].get("shorter"))
    assert shrunk == sorted([(5, 3), (5, 1), (11, 1), (15, 1), (4, 2), (6, 2)])
    assert all(st[at[n]] == sm.OK for n in names if n.startswith("egvm"))


def test_an_output_row_one_byte_too_short():
    picked = [sm.small_cases()[5], sm.small_cases()[4], sm.walk_cases(300)[0]]
    roots, queues = [c[1] for c in picked], [list(c[2]) for c in picked]
    full = sm.shorten(roots, queues)
    longest = int(full.out_lens.max())
    assert longest >= 3
    model = sm.Batch(roots, queues, out_width=longest - 1, fill=FILL)
    _run_and_compare(model)
    g = int(full.out_lens.argmax())
    assert model.status[g] == sm.NO_ROOM and model.out_lens[g] == longest and (model.out_queues[g] == FILL).all()   # length reported, row unwritten
    assert model.counts[g]["no_room"] == 1 and [model.status[i] for i in range(3) if i != g] == [sm.OK, sm.OK]
