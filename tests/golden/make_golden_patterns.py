"""
find_generalized_patterns recorded from the IMPORTED REFERENCE (librubiks/analysis/pattern_mining.py; nothing of it is copied).
Run like make_golden.py, with the reference's checkout first on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg PYTHONPATH=<reference> python tests/golden/make_golden_patterns.py

40 random batches (1-7 sequences of 0-15 moves over 2, 3, 4 or 12 symbols, supports from 0 to 1.5) and six hand-made ones.  Per
record k: k_acts uint8 [n, w], k_lens, k_support, and the result in the reference's order: k_patterns (the strings joined by
newlines, as bytes), k_values (float64, as the reference divides) and k_counts.  Only arrays are written
(tests/golden/patterns_golden.npz).
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import patterns_model as pm  # noqa: E402


def record(fx, name, acts, lens, support, find):
    sequences = [pm.names_of(acts[s, :lens[s]]) for s in range(len(lens))]
    result = find(sequences, support)
    n = len(lens)
    fx[f"{name}_acts"], fx[f"{name}_lens"], fx[f"{name}_support"] = acts, lens, np.float64(support)
    fx[f"{name}_patterns"] = np.frombuffer("\n".join(result).encode(), dtype=np.uint8)
    fx[f"{name}_values"] = np.array(list(result.values()), dtype=np.float64)
    fx[f"{name}_counts"] = np.array([round(v * n) for v in result.values()], dtype=np.int64)
    return result


def main():
    from librubiks.analysis.pattern_mining import find_generalized_patterns as find
    fx = {}
    rng = np.random.RandomState(2024)
    for k in range(40):
        n = rng.randint(1, 8)
        symbols = (2, 3, 4, 12)[k % 4]
        seqs = [rng.randint(0, symbols, rng.randint(0, 16)).tolist() for _ in range(n)]
        support = [0, 0.3, 1 / 3, 0.5, 2 / n, 1.0, 1.5, float(rng.uniform(0, 1))][k % 8]
        record(fx, f"random{k:02d}", *pm.padded(seqs), support, find)
    a = pm.actions_of
    hand = {
        "renaming": ([a("RTr"), a("FLf"), a("Fff"), a("BBBb"), a("fFfF")], 0),
        "ties": ([a("FR"), a("RFRF"), a("ffLL"), a("LLff"), a("TdTd")], 0),
        "short_only": ([[], a("F"), a("r")], 0),
        "all_twelve": ([list(range(12)) + list(range(11, -1, -1))], 0),
    }
    for name, (seqs, support) in hand.items():
        record(fx, name, *pm.padded(seqs), support, find)
    acts, lens = pm.ragged_batch(with_bad_byte=False)
    for name, support in (("ragged_03", 0.3), ("ragged_05", 0.5)):
        r = record(fx, name, acts, lens, support, find)
        print(name, len(r), "patterns")
    assert find([], 0.5) == {}   # (an empty list has no arrays to record: tests state it)
    np.savez_compressed(os.path.join(OUT, "patterns_golden.npz"), **fx)
    print(len(fx) // 6, "records,", os.path.getsize(os.path.join(OUT, "patterns_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
