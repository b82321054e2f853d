"""
Helpers shared by the MCTS GPU tests (a plain module, imported by the test modules and by their child processes): the node-for-node
comparison of a device tree with the oracle's, and `drive`, which steps a forest one iteration at a time in one form of the tree
kernel and can disturb what line following reads between two iterations (tests/test_store_edges_gpu.py).
"""
import ctypes

import numpy as np
import torch

from keys_model import check_hash_table  # noqa: F401  (the MCTS tests take it from here)

TREE_KEYS = ("states", "neighbors", "leaves", "N", "L", "V", "W", "P")
WRAP = 65536 - 48      # iteration number planted by `drive(what="wrap")`: 48 iterations before the 16-bit path number wraps


def compare_tree(tree: dict, ref: dict, n: int):
    assert tree["n"] == n
    assert np.array_equal(tree["states"][1:n + 1], ref["states"][1:n + 1])
    assert np.array_equal(tree["neighbors"][:n + 1], ref["neighbors"][:n + 1])
    assert np.array_equal(tree["leaves"][1:n + 1], ref["leaves"][1:n + 1])
    assert np.array_equal(tree["N"][:n + 1], ref["N"][:n + 1])
    assert np.array_equal(tree["L"][:n + 1], ref["L"][:n + 1])
    assert np.array_equal(tree["V"][1:n + 1], np.asarray(ref["V"][1:n + 1], dtype=np.float64))
    assert np.array_equal(tree["W"][1:n + 1], ref["W"][1:n + 1])
    assert np.allclose(tree["P"][1:n + 1], ref["P"][1:n + 1], rtol=0, atol=1e-6)


def oracle_arrays(ref) -> dict:
    """An oracle agent's tree as the dict `compare_tree` takes."""
    return {k: getattr(ref, k) for k in TREE_KEYS}


def standin_from_golden(npz):
    from standin_net import StandInNet
    return StandInNet(weights={k[4:]: npz[k] for k in npz.files if k.startswith("net_") and not k.startswith("net_probe")})


def _scramble_rings(f, rng, seq_sel: np.ndarray):
    """Permutes every tree's ring slots (whole lines with their lengths: each line stays a path the tree walked) and rewrites node
    tags so that they name lines, positions and ages that do not describe where the node was: a third of the nodes point at some
    place where they do sit on a line, a third at a random place of a random line, the rest keep their tags, which now name another
    line.  Everything stays in range: tags are 1 .. ring_k iterations old for the select that runs next, positions < ring_len."""
    from librubiks.solving import mcts_device as md
    K = md.RING_K
    rn, ra, rl = (x.cpu().numpy() for x in (f.ring_node, f.ring_act, f.ring_len))
    n_nodes = f.n_nodes.cpu().numpy()
    for t in range(f.B):
        perm = rng.permutation(K)
        rn[t], ra[t], rl[t] = rn[t][perm], ra[t][perm], rl[t][perm]
        occ = {}
        for s in range(K):
            for p in range(int(rl[t, s])):
                occ.setdefault(int(rn[t, s, p]), []).append((s, p))
        lines = [s for s in range(K) if rl[t, s] > 0]
        n, base = int(n_nodes[t]), t * (f.C + 1)
        tags = f.rec[base + 1:base + n + 1, 3].cpu().numpy().view(np.uint32).copy()
        for node in range(1, n + 1):
            r = rng.randint(3)
            if r == 0 and node in occ:
                s, p = occ[node][rng.randint(len(occ[node]))]
                a = int(ra[t, s, p])
            elif r == 1 and lines:
                s = lines[rng.randint(len(lines))]
                p, a = rng.randint(int(rl[t, s])), rng.randint(12)
            else:
                continue
            age = int((int(seq_sel[t]) - s) & (K - 1)) or K
            tags[node - 1] = ((((int(seq_sel[t]) - age) & 0xFFFF) << 16) | (p << 4) | a)
        f.rec[base + 1:base + n + 1, 3] = torch.from_numpy(tags.view(np.int32)).to(f.device)
    for name, x in (("ring_node", rn), ("ring_act", ra), ("ring_len", rl)):
        getattr(f, name).copy_(torch.from_numpy(x))


def drive(net, states: np.ndarray, c: float, form: str, s1: int, s2: int, what: str, seed: int = 0) -> dict:
    """A naive-search forest of len(states) trees (stand-in `net`), s1 iterations, then `what` ("wrap": every tree's iteration number
    becomes WRAP; "rings": `_scramble_rings`), then s2 more, one at a time.  form: "select0" = rc_mcts_expand -> network ->
    rc_mcts_backup -> rc_mcts_select (k_mcts_select<0>); "three_phase" = rc_mcts_expand -> network -> rc_mcts_backup_select
    (k_mcts_select<1>); "one_launch" = network -> rc_mcts_step (k_mcts_select<1, true, NT, LW>, LW as RUBIKS_LINE_WAVES / the
    forest's size choose).  Returns the trees, iteration counts and what line following did."""
    from librubiks import _hip
    from librubiks.cube import DeviceCubes
    from librubiks.model import GenericNet
    from librubiks.solving import mcts_device as md
    B = len(states)
    cap = 12 * (s1 + s2) + 64
    f = md.MCTSForest(B, cap, vmm=False)
    f.set_net(GenericNet(net), torch.float32)
    roots = DeviceCubes.from_numpy(np.asarray(states))
    one = form == "one_launch"
    if one:
        f.set_active(None)
        f.plant(None, roots, 0, cap)
    else:
        f.reset(roots)
    m = ctypes.byref(f.struct)

    def step():
        if form != "select0":
            return f.step(c, cap, use_graph=False)
        st = _hip.stream_ptr()
        _hip.check(f.lib.rc_mcts_expand(m, cap, st))
        f._evaluate_children()
        _hip.check(f.lib.rc_mcts_backup(m, f.probs.data_ptr(), f.values.data_ptr(), st))
        _hip.check(f.lib.rc_mcts_select(m, c, 0, st))

    # a tree's first iteration takes two steps in the three-phase forms; a one-launch plant expands the root itself
    for _ in range(s1 if one else s1 + 1):
        step()
    torch.cuda.synchronize()
    out = {"it_at": f.iterations.cpu().numpy().astype(np.int64)}
    seq_end = (WRAP + s2) & 0xFFFF
    if what == "wrap":
        rec = f.rec.cpu().numpy()
        n = f.n_nodes.cpu().numpy()
        tseq = [(rec[t * (f.C + 1) + 1:t * (f.C + 1) + n[t] + 1, 3].view(np.uint32) >> 16) for t in range(B)]
        # tags that a select after the wrap reads as 1 .. ring_k iterations old although they are 65 536 + that old
        out["aliasing"] = int(sum(((x >= 1) & (x < seq_end)).sum() for x in tseq))
        out["pre_max"] = int(max(int(x.max()) for x in tseq))
        f.iterations.fill_(WRAP)
    elif what == "rings":
        _scramble_rings(f, np.random.RandomState(seed), (out["it_at"] + (0 if one else 1)) & 0xFFFF)
    window_rounds, rounds = 0, 0
    for _ in range(s2):
        step()
        st, it, stats = (x.cpu().numpy() for x in (f.status, f.iterations, f.select_stats))
        run = st == md.RUNNING
        used = (it.astype(np.int64) - (1 if one else 0)) & 0xFFFF        # the path number the select of this step used
        lr = (stats[:, 7].astype(np.uint32) >> 16).astype(np.int64)
        rounds += int(lr[run].sum())
        if what == "wrap":
            win = run & (used >= 1) & (used <= out["pre_max"] + md.RING_K) & (used < WRAP)
            window_rounds += int(lr[win].sum())
    if one:
        f.close_pending(c)
    torch.cuda.synchronize()
    out.update(rounds=rounds, window_rounds=window_rounds, it_end=f.iterations.cpu().numpy().astype(np.int64),
               status=f.status.cpu().numpy(), trees=[f.tree_arrays(t) for t in range(B)])
    return out


def save_trees(path: str, out: dict):
    flat = {f"{t}_{k}": v for t, tree in enumerate(out["trees"]) for k, v in tree.items()}
    np.savez(path, it_at=out["it_at"], it_end=out["it_end"], status=out["status"], rounds=out["rounds"],
             window_rounds=out["window_rounds"], aliasing=out.get("aliasing", -1), **flat)


def load_trees(path: str) -> dict:
    z = np.load(path)
    B = len(z["status"])
    trees = [{k: (int(z[f"{t}_{k}"]) if k == "n" else z[f"{t}_{k}"]) for k in ("n",) + TREE_KEYS} for t in range(B)]
    return {"it_at": z["it_at"], "it_end": z["it_end"], "status": z["status"], "rounds": int(z["rounds"]),
            "window_rounds": int(z["window_rounds"]), "aliasing": int(z["aliasing"]), "trees": trees}
