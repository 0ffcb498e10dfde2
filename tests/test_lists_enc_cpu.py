"""CPU-only checks of the many-lists encode's host surface
(include/turbopfor_gpu.h tpf_p4nenc256v32_lists): the symbols are exported,
the bound and workspace-size functions are pure host functions, monotone in
each argument, the entry point reports TPF_ENODEV instead of falling back to a
CPU codec, and the bound holds for the oracle's composition of every input the
GPU parity test (tests/test_gpu_lists_enc.py) encodes and of the worst-case
lists."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lists_enc_inputs as inp
import lists_ref
import turbopfor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "turbopfor-cpp_amd", "lib", "libturbopfor_amd.so")
u64 = ctypes.c_uint64
STEPS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 4095, 4096, 4097, 10 ** 6, 0x7FFFFFFF]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "turbopfor-cpp_amd"), "-j8"])
    return turbopfor_amd.declare(ctypes.CDLL(LIB))


def test_symbols_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"tpf_p4nenc256v32_lists", "tpf_p4nenc256v32_lists_bound", "tpf_p4nenc256v32_lists_workspace_size"} <= exported


@pytest.mark.parametrize("name", ["tpf_p4nenc256v32_lists_bound", "tpf_p4nenc256v32_lists_workspace_size"])
def test_size_functions_are_pure_and_monotone(lib, name):
    f = getattr(lib, name)
    for a in STEPS:
        assert f(a, 1) > 0 and f(1, a) > 0
    for fixed in (1, 1000, 10 ** 6):
        for a, b in zip(STEPS, STEPS[1:]):
            assert f(a, fixed) <= f(b, fixed), ("first argument", a, b, fixed)
            assert f(fixed, a) <= f(fixed, b), ("second argument", a, b, fixed)
    assert f(1000, 10) == f(1000, 10)  # no state


def test_bound_is_monotone_across_a_block_boundary(lib):
    """The per-unit bounds themselves are not (one list of 255 values: a
    2,168-byte tail; of 256: an 1,800-byte block); the documented formula is."""
    f = lib.tpf_p4nenc256v32_lists_bound
    for nlists in (1, 2, 7):
        prev = 0
        for n in range(0, 256 * 9 + 3):
            assert f(n, nlists) >= prev, (n, nlists)
            prev = f(n, nlists)


def test_bound_formula(lib):
    """8 nvalues + 128 T - floor(248 max(0, nvalues - 255 T - 255) / 256) + 64,
    T = min(nlists, nvalues), as include/turbopfor_gpu.h states it; and it
    dominates the per-unit bounds of every partition tried."""
    f = lib.tpf_p4nenc256v32_lists_bound
    rng = np.random.default_rng(3)
    for nv, nl in [(0, 0), (0, 5), (1, 1), (255, 1), (256, 1), (257, 1), (10 ** 6, 3), (10 ** 6, 10 ** 6), (2560000000, 2500000)]:
        T = min(nl, nv)
        assert f(nv, nl) == 8 * nv + 128 * T - (248 * max(0, nv - 255 * T - 255)) // 256 + 64
    for _ in range(200):
        nl = int(rng.integers(1, 40))
        lens = rng.integers(0, 256 * 6, size=nl)
        per_unit = sum(1800 * (int(n) // 256) + (128 + 8 * (int(n) % 256) if n % 256 else 0) for n in lens)
        assert per_unit <= f(int(lens.sum()), nl)


def test_no_cpu_fallback_without_device(lib):
    if subprocess.run([sys.executable, "-c", "import torch,sys;sys.exit(0 if torch.cuda.is_available() else 1)"]).returncode == 0:
        pytest.skip("a HIP device is visible")
    rc = lib.tpf_p4nenc256v32_lists(None, u64(0), None, u64(1), 0, None, None, u64(0), None, u64(1), None, ctypes.c_size_t(0), None,
                                    None)
    assert rc == -3  # TPF_ENODEV
    assert b"no CPU fallback" in lib.tpf_last_error()


def _composed_len(lists, d1, start0):
    packed, offs, _, vals = lists_ref.compose(lists, d1, start0)
    assert int(offs[-1]) == len(packed)
    return len(packed), len(vals)


def test_bound_holds_for_the_gpu_test_inputs(lib):
    f = lib.tpf_p4nenc256v32_lists_bound
    cases = [(lists, d1, start0) for (_, d1), (lists, start0) in inp.matrix_inputs().items()]
    kl, ks = inp.kinds_inputs()
    cases.append((kl, True, ks))
    for lists, d1, start0 in cases:
        total, nvalues = _composed_len(lists, d1, start0)
        assert total <= f(nvalues, len(lists))


@pytest.mark.parametrize("n", [255, 256])
@pytest.mark.parametrize("d1", [False, True])
def test_bound_holds_for_the_worst_case_lists(lib, n, d1):
    """[0xFFFFFFFF, 0] * 128: every value (every delta too) needs 32 bits."""
    f = lib.tpf_p4nenc256v32_lists_bound
    worst = np.array([0xFFFFFFFF, 0] * 128, dtype=np.uint32)
    lists = [worst[:n].copy() for _ in range(40)]
    total, nvalues = _composed_len(lists, d1, np.zeros(len(lists), np.uint32))
    assert nvalues == 40 * n and total <= f(nvalues, len(lists))
    assert total <= f(nvalues, 10 ** 6)  # more lists allowed than used
