"""GPU checks of the wide Gram (csrc/als_cg.hip: als_gram_wide_kernel and als_gram_wide_fold_kernel, G = F^T F for D 65 .. 256)
through the harness entry goctr_selftest_als_gram_wide (csrc/selftest.hip), past the row counts and widths ALS's own tests reach:
row counts that are no multiple of 4 (a partial MFMA step with zero rows staged behind the last) or of 16 (a partial last chunk),
widths that are no multiple of 16, every count of rounds of 12 tile pairs, and the second batch of the byte-bounded parts scratch.

Integer factors in {-2 .. 2} make every partial sum exact in any order, so those cases ask for F^T F bit for bit; the float cases
are held within 16 x e0 of als_ref.gram in longdouble, e0 that function's own spread between float64 forwards, float64 backwards
and longdouble (test_gpu_als_cg.py's rule and margin).  The harness fills G's device buffer with 0xff bytes before every call: an
element left unwritten, or a sum that starts from what was there, is a NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_ref as A  # noqa: E402
from test_gpu_als_cg import RUNS, spread  # noqa: E402
from test_gpu_primitives import INT, LL, Harness, _p  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_D = [65, 72, 96, 100, 129, 192, 193, 255, 256]
EXACT_N = [1, 3, 4, 15, 17, 255, 256, 257, 1027]


@pytest.fixture(scope="module")
def H():
    return Harness()


@pytest.fixture(scope="module")
def ints():
    """(n, D) -> F [n, D] of integers in {-2 .. 2} as float64: 2^20 + 7 draws, made once and repeated as often as a case needs"""
    base = np.random.default_rng(23).integers(-2, 3, size=(1 << 20) + 7).astype(np.float64)
    return lambda n, D, skip=0: np.resize(base[skip:], n * D).reshape(n, D)


def gram_wide(H, F):
    F = np.ascontiguousarray(F, np.float64)
    n, D = F.shape
    out, parts = np.zeros((D, D), np.float64), LL(-1)
    H.call("als_gram_wide", _p(F), LL(n), INT(D), _p(out), C.byref(parts))
    return out, parts.value


def same_bits(G, F):
    want = F.T @ F                                                               # (integers below 2^53: exact in any order)
    return G.tobytes() == want.tobytes() and G.tobytes() == np.ascontiguousarray(G.T).tobytes()


@pytest.mark.parametrize("D", EXACT_D)
def test_integer_factors_give_the_gram_matrix_bit_for_bit(H, ints, D):
    for n in EXACT_N:
        F = ints(n, D)
        G, parts = gram_wide(H, F)
        assert same_bits(G, F) and parts >= 1, (n, D)


def test_the_second_batch_of_the_parts_scratch(H, ints):
    D = 256
    _, max_parts = gram_wide(H, ints(3, D))
    n = 256 * (max_parts + 1) + 3                                                # one tile past a full batch, and a ragged tile behind it
    assert max_parts >= 1 and n * D * 8 < 256 << 20                             # (33027 rows, 68 MB at the present 64 MB of scratch)
    F = ints(n, D)
    G, _ = gram_wide(H, F)
    assert same_bits(G, F)
    # the scratch the large call left behind serves smaller ones: one tile (a fold with init = 1 alone, behind a call whose last
    # fold had init = 0) and two tiles at another width
    for n2, D2 in ((17, 256), (300, 100)):
        F2 = ints(n2, D2, skip=1000)
        assert same_bits(gram_wide(H, F2)[0], F2), (n2, D2)


@pytest.mark.parametrize("D,n", [(100, 257), (190, 1027), (256, 515)])
def test_float_factors_within_the_restatements_own_spread(H, D, n):
    F = np.random.default_rng(D).standard_normal((n, D))
    runs = [(A.gram(F, order, dtype),) for order, dtype in RUNS]
    e0 = spread(runs)
    G, _ = gram_wide(H, F)
    err = A.rel_diff(G, runs[2][0])
    print(f"gram D{D} n{n}: e0 = {e0:.3e}, device / restatement {err:.3e}")
    assert 0 < e0 < 1e-11 and err <= 16 * e0 and G.tobytes() == np.ascontiguousarray(G.T).tobytes()
