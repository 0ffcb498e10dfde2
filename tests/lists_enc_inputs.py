"""Inputs of the many-lists encode tests, shared by tests/test_gpu_lists_enc.py
(GPU parity) and tests/test_lists_enc_cpu.py (the capacity bound): the shape
matrix in two shuffled orders, plain and delta-1, and the exception-kinds
lists.  Test infrastructure only."""
import numpy as np

import lists_ref as ref


def lists(lens, d1, rng, start0=None, outliers=False):
    if d1:
        return [ref.d1_values(n, 0 if start0 is None else int(start0[j]), rng, outliers) for j, n in enumerate(lens)]
    return [ref.plain_values(n, rng) for n in lens]


def matrix_inputs():
    """(order seed, d1) -> (lists, start0): the shape matrix's inputs ."""
    built = {}
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        lens = [ref.MATRIX[i] for i in rng.permutation(len(ref.MATRIX))]
        for d1 in (False, True):
            start0 = rng.integers(0, 1 << 32, size=len(lens), dtype=np.uint64).astype(np.uint32)
            built[(seed, d1)] = (lists(lens, d1, rng, start0), start0)
    return built


KIND_LENS = [256 * 70 + 130, 5, 256 * 3, 256 * 33 + 1, 0, 200, 256 * 18 + 255]


def kinds_inputs():
    rng = np.random.default_rng(10)
    start0 = rng.integers(0, 1 << 32, size=len(KIND_LENS), dtype=np.uint64).astype(np.uint32)
    return lists(KIND_LENS, True, rng, start0, outliers=True), start0
