"""
The scenarios of tests/astar_each_model.py on the models alone: the seeds are chosen here, on the CPU, so that every case the GPU
comparison (tests/test_astar_each_kernels_gpu.py) is meant to meet does occur -- the same assertions run there.
"""
import numpy as np

import conftest  # noqa: F401
import astar_each_model as em
import astar_model as am


def _run(scenario, seed):
    pool = em.EachPool()
    launches = []
    for launch in scenario(pool, seed):
        pool.apply(launch)
        launches.append(launch)
    return pool, launches


def test_the_seeded_scenario_reaches_its_cases():
    pool, launches = _run(em.seeded_scenario, em.SEED)
    count = pool.counters()
    assert not [k for k in em.WANTED if count[k] < 1], dict(count)
    assert (pool.Nmax, pool.B, 12 * pool.Nmax) == (22, 4, 264) and pool.H == am.min_hash_size(pool.C)
    assert pool.N[em.REPLANT["slot"]] == em.REPLANT["N"] and pool.lam[em.REPLANT["slot"]] == em.REPLANT["lam"]
    # the new tenant searched under its own values: it popped, and never more than its N
    after = [x for x in launches[[i for i, x in enumerate(launches) if x["op"] == "plant"][0]:] if x["op"] == "pop"]
    assert after and pool.models[em.REPLANT["slot"]].iterations[0] >= 2


def test_the_clamp_scenario_reaches_its_cases():
    pool, launches = _run(em.clamp_scenario, em.CLAMP_SEED)
    count = pool.counters()
    assert not [k for k in em.CLAMP_WANTED if count[k] < 1], dict(count)
    assert [int(x["expansions"][1]) for x in launches if x["op"] == "pop"][2] == pool.Nmax + 1
    assert [int(x["expansions"][2]) for x in launches if x["op"] == "pop"][3] == 0
    assert [int(x["expansions"][0]) for x in launches if x["op"] == "pop"][4] == -1


def test_a_pool_of_equal_settings_is_the_batch_model():
    """Four problems with one (lambda, N): the side-by-side single models hold what AStarModel(4, N, ...) holds."""
    rng = np.random.RandomState(7)
    roots = am.seeded_roots(rng, 4, 0.5)
    pool, whole = em.EachPool((5,) * 4, (0.2,) * 4, 255), am.AStarModel(4, 5, 255, am.min_hash_size(255))
    pool.apply({"op": "init", "roots": roots})
    whole.init(roots)
    for _ in range(4):
        pool.apply({"op": "pop", "max_states": am.U32_MAX, "expansions": pool.expansions()})
        whole.pop_expand(am.U32_MAX)
        off = pool.offsets()
        assert np.array_equal(off, am.offsets(whole))
        values = am.PALETTE[rng.randint(0, len(am.PALETTE), int(off[-1]))]
        pool.apply({"op": "push", "new_offset": off, "values": values, "lambda": pool.lambdas()})
        whole.push_relax(off, values, 0.2)
        for b, m in enumerate(pool.models):
            for name in em.NODE_ROWS + tuple(n for n, _ in em.STAGING) + am.SCALARS:
                assert np.array_equal(getattr(m, name)[0], getattr(whole, name)[b]), (b, name)
            assert sorted(m.heap[0]) == sorted(whole.heap[b])
