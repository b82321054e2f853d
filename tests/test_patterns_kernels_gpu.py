"""
The rc_patterns_* kernels against tests/patterns_model.py after EVERY launch and on every array the header defines: the lane
words, the node and seen tables, the output rows, the counters and the statuses, each array between guard bytes and pre-filled so
that what a launch must not write is seen to be still there.  Where a key lands depends on the order of the inserts, so node ids
are compared through what they name: a lane's node must hold the lane's own key (its parent's node of the level before and its
token), the count and the first occurrence the model has for that pattern, and the (node, sequence) key must be found by a
look-up.  One ragged batch holds the lengths around a wavefront, more starts than a workgroup, identical sequences, 200 equal
moves, all 12 actions and a byte that is no action; a second batch gets tables smaller than its keys.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import patterns_model as pm  # noqa: E402

GUARD, FILL = 256, 0xA5
ARRAYS = pm.Batch.ARRAYS


def _guarded(batch):
    """Moves every array a launch writes between GUARD bytes of FILL, itself filled with FILL."""
    bufs = {}
    for name in ARRAYS:
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


def _device_batch(model: pm.Batch):
    from librubiks.analysis.pattern_mining import PatternBatch
    batch = PatternBatch(model.acts, model.lens, model.min_count)
    assert (batch.pos_off_h == model.pos_off).all() and (batch.P, batch.cap, batch.n) == (model.P, model.cap, model.n)
    return batch, _guarded(batch)


def _snap(batch, model):
    """Every array on the host, in the model's (unsigned) types."""
    return {name: getattr(batch, name).cpu().numpy().view(getattr(model, name).dtype) for name in ARRAYS}


def _same(got, want, names, step):
    for name in names:
        bad = np.flatnonzero((got[name] != want[name]).reshape(len(want[name]), -1).any(axis=1))
        assert len(bad) == 0, f"after {step}: {name} differs in rows {bad[:8]} ({len(bad)} rows): {got[name][bad[0]]} != {want[name][bad[0]]}"


def _model_arrays(model):
    return {name: getattr(model, name) for name in ARRAYS}


def _launch(batch, model, name):
    s = batch.struct
    s.level, s.node_cells, s.seen_cells = model.level, model.node_cells, model.seen_cells
    batch.step(name)
    torch.cuda.synchronize()


def _begin(batch, model, bufs):
    _launch(batch, model, "rc_patterns_begin")
    model.begin()
    _same(_snap(batch, model), _model_arrays(model), ARRAYS, "rc_patterns_begin")   # the tables and rows still hold FILL on both sides
    _guards_intact(bufs)


def _extend(batch, model, bufs, no_room: bool = False):
    before = _snap(batch, model)
    _launch(batch, model, "rc_patterns_extend")
    model.extend()
    got, NC, SC = _snap(batch, model), model.node_cells, model.seen_cells
    _same(got, before, ("lane_seq", "out_rows"), "rc_patterns_extend")
    assert (got["counters"] == 0).all()
    for name, cells in (("node_keys", NC), ("node_count", NC), ("node_first", NC), ("seen_keys", SC)):   # cells this level does not use
        assert (got[name][cells:] == before[name][cells:]).all(), name
    free = got["node_keys"][:NC] == 0
    assert (got["node_count"][:NC][free] == 0).all() and (got["node_first"][:NC][free] == pm.FREE_FIRST).all()
    d_node, m_node = got["lane_node"], model.lane_node
    if no_room:   # which lanes find the tables full depends on the order of the inserts: the survivors must still be right
        assert (d_node[before["lane_node"] < 0] == -1).all() and (got["status"] == pm.NO_ROOM).any()
        assert set(np.flatnonzero(got["status"] != before["status"])) <= set(np.flatnonzero(got["status"] == pm.NO_ROOM))
    else:
        _same(got, _model_arrays(model), ("lane_state", "status"), "rc_patterns_extend")
        assert ((d_node < 0) == (m_node < 0)).all()
        assert np.count_nonzero(~free) == np.count_nonzero(model.node_keys[:NC]) == model.distinct[model.level]
        assert np.count_nonzero(got["seen_keys"][:SC]) == np.count_nonzero(model.seen_keys[:SC])
    live = np.flatnonzero(d_node >= 0)
    assert (d_node[live] < NC).all()
    keys = got["node_keys"][d_node[live]]
    tokens = np.array([model.tokens[p] for p in live], dtype=np.uint64)
    assert ((keys & np.uint64(0xFF)) == tokens + np.uint64(1)).all()
    assert ((keys >> np.uint64(8)) == (before["lane_node"][live] + 1).astype(np.uint64)).all()   # the parent: the lane's node of the level before
    if not no_room:
        assert (got["node_first"][d_node[live]] == model.node_first[m_node[live]]).all()
        assert (got["node_count"][d_node[live]] == model.node_count[m_node[live]]).all()
    for p in live:
        assert pm.lookup(got["seen_keys"], SC, (int(d_node[p]) + 1) << 32 | (int(got["lane_seq"][p]) + 1)) >= 0, f"lane {p}"
    _guards_intact(bufs)
    return got


def _close(batch, model, bufs, no_room: bool = False):
    before = _snap(batch, model)
    _launch(batch, model, "rc_patterns_close")
    got = _snap(batch, model)
    _same(got, before, ("lane_seq", "lane_state", "node_keys", "node_count", "node_first", "seen_keys", "status"), "rc_patterns_close")
    live_d, n_out, full = int(got["counters"][0]), int(got["counters"][1]), int(got["counters"][2])
    assert full == 0 and got["counters"][3] == 0 and (got["out_rows"][n_out:] == before["out_rows"][n_out:]).all()
    kept = got["lane_node"] >= 0
    assert live_d == np.count_nonzero(kept) and (got["lane_node"][kept] == before["lane_node"][kept]).all() and (got["lane_node"][~kept] == -1).all()
    rows = got["out_rows"][:n_out]
    if not no_room:
        model.close()
        assert live_d == model.live and (kept == (model.lane_node >= 0)).all()
        assert sorted(map(tuple, rows.tolist())) == sorted(map(tuple, model.rows.tolist()))
    _guards_intact(bufs)
    return rows


@pytest.mark.parametrize("support", [0, 1 / 12, 0.3, 1.0, 1.5])
def test_every_launch_against_the_model(support):
    acts, lens = pm.ragged_batch()
    assert sorted(lens.tolist()) == [0, 1, 2, 7, 9, 9, 17, 63, 64, 65, 200, 300] and acts[11, 3] == 12
    model = pm.Batch(acts, lens, pm.min_count(12, support), fill=FILL)
    batch, bufs = _device_batch(model)
    _begin(batch, model, bufs)
    assert model.status.tolist() == [pm.OK] * 11 + [pm.BAD_ACTION] and model.live == int(np.maximum(lens[:11] - 1, 0).sum()) > 256
    bad_lanes = slice(int(model.pos_off[11]), int(model.pos_off[12]))
    assert (model.lane_state[bad_lanes] == 0xA5A5A5A5).all() and (model.lane_node[bad_lanes] == -1).all()   # nothing else is written for it
    rows, want, levels = [], [], 0
    while model.live > 0:
        model.next_level()
        _extend(batch, model, bufs)
        rows += _close(batch, model, bufs).tolist()
        want += model.rows.tolist()
        levels += 1
    assert model.status.tolist() == [pm.OK] * 11 + [pm.BAD_ACTION]
    if support in (0, 1 / 12):   # min_count 0 and 1: every distinct pattern, once (tens of thousands: the rows were compared level by level)
        assert model.min_count == (0 if support == 0 else 1) and levels == 299
        assert len(rows) == sum(model.distinct.values()) > 10_000 and [1, 8, 0, 200] in rows   # AA..A of sequence 8, the 200 equal moves
    else:
        from librubiks.analysis.pattern_mining import result_of
        got = result_of(np.array(rows, dtype=np.uint32).reshape(-1, 4), acts, 12)
        assert list(got.items()) == list(pm.result_of(want, acts, 12).items())
        if support == 0.3:
            assert model.min_count == 4 and levels < 20 and len(got) == 27 and got["AA"] == 6 / 12   # (27: what the model finds on the CPU)
        else:
            assert model.min_count in (12, 13) and levels == 1 and got == {}


def test_tables_smaller_than_their_keys_end_no_room_inside_the_arrays():
    rng = np.random.RandomState(8)
    acts, lens = pm.padded([rng.randint(0, 12, 40).tolist() for _ in range(6)])
    model = pm.Batch(acts, lens, 0, fill=FILL)
    batch, bufs = _device_batch(model)
    _begin(batch, model, bufs)
    for _ in range(3):
        model.next_level()
        _extend(batch, model, bufs)
        _close(batch, model, bufs)
    ahead = copy.deepcopy(model)
    ahead.next_level()
    ahead.extend()
    nodes, pairs = ahead.distinct[5], np.count_nonzero(ahead.seen_keys[:ahead.seen_cells])
    assert ahead.live == 6 * 36 and 64 < nodes <= pairs <= ahead.live
    small = lambda keys: pm.table_cells(keys) // 4 if pm.table_cells(keys) // 2 >= keys else pm.table_cells(keys) // 2   # noqa: E731
    for which, node_cells, seen_cells in (("nodes", small(nodes), None), ("seen", None, small(pairs))):
        m = copy.deepcopy(model)
        b, bf = _device_batch(m)
        for name in ARRAYS:
            getattr(b, name).copy_(getattr(batch, name))
        m.next_level(node_cells, seen_cells)
        assert (node_cells or seen_cells) < (nodes if which == "nodes" else pairs)   # the largest power of two below the keys
        got = _extend(b, m, bf, no_room=True)
        table = got["node_keys"][:m.node_cells] if which == "nodes" else got["seen_keys"][:m.seen_cells]
        assert (table != 0).all() and (m.status == pm.NO_ROOM).any()                  # full, and the model saw it too
        assert np.count_nonzero(got["lane_node"] >= 0) < ahead.live
        _close(b, m, bf, no_room=True)
