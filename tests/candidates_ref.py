"""The negative sampler's definition restated in numpy (tlsan_sample_negatives): what tests/test_candidates_cpu.py checks
on its own and tests/test_gpu_candidates.py holds the kernel to."""
import numpy as np


def splitmix64(z):
    """the standard SplitMix64 finaliser on uint64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, np.uint64) + np.uint64(0x9e3779b97f4a7c15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def reference_negatives(item_count, label, excluded, n, seed, row):
    """The sampler's definition: the first n distinct items of the draw sequence t = 0, 1, ... of global row `row` that
    are neither the label nor in `excluded`, among the first 64 n draws; -1 past the last one found."""
    with np.errstate(over="ignore"):
        h = splitmix64(np.array([(int(seed) ^ int(row)) & 0xFFFFFFFFFFFFFFFF], np.uint64))[0]
        t = np.arange(64 * n, dtype=np.uint64)
        key = splitmix64(h ^ t)
        items = ((key >> np.uint64(32)) * np.uint64(item_count)) >> np.uint64(32)
    out, seen = [], set(int(x) for x in excluded) | {int(label)}
    for it in items.astype(np.int64).tolist():
        if it not in seen:
            seen.add(it)
            out.append(it)
            if len(out) == n:
                break
    return np.array(out + [-1] * (n - len(out)), np.int32)
