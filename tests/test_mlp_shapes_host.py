"""CPU side of tests/test_gpu_mlp_shapes.py: the float64 MLP off the handful of shapes the other MLP tests use.

1. The reference is good enough for the tolerance it is used at.  For every case of mlp_ref.SHAPE_CASES and every hidden
   activation, mlp_ref.loss_grad_rows runs in float64 and in numpy's extended precision (np.longdouble arrays in, nothing else
   changed); the float64 gradient must lie within 1e-3 of the GPU suite's budget of the extended one,
   |g64 - gLD| <= 1e-3 (1e-9 |gLD| + 1e-13), the loss within 1e-12 relative, and the logistic / softmax head must stay inside
   [1e-6, 1 - 1e-6] (a saturated head makes the clamped log-loss a statement about the data).  What the GPU tests then measure
   at rtol 1e-9 / atol 1e-13 is the kernels.  The measured ratios are printed (pytest -s).
2. Each case reaches the branch it is listed for.  mlp_ref.plan restates the host's dispatch (csrc/mlp.hip, launch_nn64 /
   launch_tn64 in csrc/mlp_kernels.h, fused_ok / chain_ok in csrc/mlp_model.h); the assertions below spell out, per case, the
   tile counts, grids, K phases, wavefront groups and slab counts (at 256 compute units) the GPU module's docstring lists, so
   that a changed case cannot go empty silently.
3. The slab workspace bound: tn_slabs64's `most` (csrc/mlp.hip) is checked against every smaller batch by brute force."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as ref  # noqa: E402

ROWS = 77            # the GPU one-step test's rows: three 32-row slabs, the last with 13 rows
LD = np.longdouble


@pytest.mark.parametrize("hidden", ref.SHAPE_HIDDEN)
@pytest.mark.parametrize("name", sorted(ref.SHAPE_CASES))
def test_float64_reference_against_extended_precision(name, hidden):
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    head, units, _ = ref.SHAPE_CASES[name]
    theta = ref.case_theta(name, hidden)
    X, Y = ref.case_data(name, ROWS)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    a64, d64 = ref.blocks(units, ROWS)
    l64, g64 = ref.loss_grad_rows(units, hidden, head, ref.SHAPE_ALPHA, theta.copy(), X64, Y64, a64, d64)
    aLD, dLD = ref.blocks(units, ROWS, LD)
    lLD, gLD = ref.loss_grad_rows(units, hidden, head, ref.SHAPE_ALPHA, theta.astype(LD), X64.astype(LD), Y64.astype(LD), aLD, dLD)
    assert gLD.dtype == LD and aLD[-1].dtype == LD
    budget = 1e-9 * np.abs(gLD) + 1e-13
    ratio = float(np.max(np.abs(g64.astype(LD) - gLD) / budget))
    lrel = abs(l64 - lLD) / abs(lLD)
    H = a64[-1]
    print(f"case {name} {hidden:8s}: float64 vs longdouble gradient at {ratio:.2e} of the GPU budget, loss {float(lrel):.2e} relative; "
          f"head in [{H.min():.3e}, {H.max():.3e}]")
    assert np.all(np.isfinite(g64)) and np.isfinite(l64)
    assert ratio <= 1e-3
    assert lrel <= 1e-12
    if head != "identity":
        assert 1e-6 <= H.min() and H.max() <= 1 - 1e-6


def test_cases_reach_their_branches():
    P = {n: ref.plan(h, u) for n, (h, u, _) in ref.SHAPE_CASES.items()}
    # a - d: the fused forward / chain kernels, ng = up1 / 32 wavefront groups
    assert [P[n].fused and P[n].chain for n in "abcd"] == [True] * 4
    assert [P[n].ng for n in "abcd"] == [1, 2, 3, 4]
    assert P["a"].up == [32, 32, 16] and P["a"].units[1] == 31            # ones column = column 31, the wavefront's last
    assert P["b"].units[0] % 16 == 0 and P["b"].up == [32, 48, 16]        # tail chunk = ones column alone; half-filled 2nd wave
    assert P["c"].units[0] % 16 == 15 and P["c"].up == [48, 80, 16]
    assert P["d"].up == [384, 128, 16] and P["d"].nch == 24 == 4 * 6      # four turns of the six-slot ring
    assert P["d"].units[1] == 127                                         # full last wavefront, ones column in its last lane column
    assert 8 * P["d"].up[0] * 32 == 96 * 1024                             # mlp_fwd_kernel's LDS image
    t = P["d"].tn[0]
    assert (t.kernel, t.KT, t.NT, t.grid_y) == ("mlp_tn64_kernel", 24, 8, 8)
    # the largest fused shape is the largest: one more input or hidden unit leaves the fused path
    assert not ref.plan("logistic", [384, 127, 1]).fused and not ref.plan("logistic", [383, 128, 1]).fused
    # e - j: never the fused kernels
    assert not any(P[n].fused for n in "efghij")
    # e: a binary net on the per-layer kernels; last K phase one 16-row chunk; KT = 25 -> last k-block one tile
    assert P["e"].up == [400, 32, 16] and P["e"].fwd[0].phases == [128, 128, 128, 16]
    t = P["e"].tn[0]
    assert (t.kernel, t.KT, t.grid_y, t.kcnt[-1]) == ("mlp_tn64_kernel", 25, 9, [1])
    # f: NT = 9
    t = P["f"].tn[0]
    assert (t.kernel, t.NT, t.KT, t.WK, t.WN, t.grid_y, t.grid_z) == ("gemm_tn_kernel<double,3,2,16>", 9, 2, 1, 2, 1, 3)
    assert t.ncnt == [[2, 2], [2, 2], [1, 0]] and t.kcnt == [[2]]         # last n-block: one tile, wave column 1 idle
    for g in (P["f"].fwd[0], P["f"].bwd[1]):                              # the same grid under EpiMlpAct and EpiMlpDAct
        assert (g.NT, g.WN, g.ntw, g.grid_y, g.tiles) == (9, 2, 4, 2, [[4, 4], [1, 0]])
    assert P["f"].tn[1].kernel == "mlp_tn64_kernel" and P["f"].tn[1].KT == 9
    # g: the DIN widths
    assert P["g"].up == [112, 208, 96, 16]
    t = P["g"].tn[0]
    assert (t.kernel, t.KT, t.NT, t.WK, t.WN, t.grid_y, t.grid_z) == ("gemm_tn_kernel<double,3,2,16>", 7, 13, 2, 2, 2, 4)
    assert t.kcnt == [[3, 3], [1, 0]] and t.ncnt == [[2, 2]] * 3 + [[1, 0]]
    g = P["g"].fwd[0]
    assert (g.NT, g.ntw, g.grid_y, g.tiles) == (13, 4, 2, [[4, 4], [4, 1]])
    g = P["g"].fwd[1]
    assert (g.NT, g.ntw, g.grid_y, g.phases, g.tiles) == (6, 4, 1, [128, 80], [[4, 2]])    # ntw = 4 instantiation, 2 tiles in use
    assert P["g"].bwd[1].NT == 13 and P["g"].bwd[1].phases == [96]
    t = P["g"].tn[1]
    assert (t.kernel, t.KT, t.NT, t.kcnt[-1]) == ("mlp_tn64_kernel", 13, 6, [1])
    # h: 70 classes
    assert P["h"].units[-1] == 70 > 64 and P["h"].up == [32, 160, 80]
    t = P["h"].tn[0]
    assert (t.kernel, t.NT, t.grid_z, t.ncnt[-1]) == ("gemm_tn_kernel<double,3,2,16>", 10, 3, [2, 0])
    assert P["h"].tn[1].kernel == "mlp_tn64_kernel" and P["h"].tn[1].NT == 5
    # i: the output layer on gemm_tn with one k tile
    assert P["i"].up == [16, 16, 144]
    t = P["i"].tn[1]
    assert (t.kernel, t.KT, t.NT, t.WK, t.kcnt, t.grid_z) == ("gemm_tn_kernel<double,3,2,16>", 1, 9, 1, [[1]], 3)
    # j: eight layers
    assert P["j"].nl == 7 and len(P["j"].units) == 8 and P["j"].up == [16, 32, 16, 48, 16, 32, 16, 16]
    # every case: 77 rows are three 32-row slabs, the last with 13 rows, at 256 compute units
    for n, p in P.items():
        assert ref.slabs(p, ROWS)[:2] == (32, 3), n
    # the shapes of the A0-copy remainder loop: nch > 6 ng
    for units, ng, nch in (([100, 12, 1], 1, 7), ([200, 40, 1], 2, 13), ([300, 70, 1], 3, 19)):
        p = ref.plan("logistic", units)
        assert p.chain and (p.ng, p.nch) == (ng, nch) and nch > 6 * ng
    assert ref.plan("logistic", [281, 100, 1]).nch == 18 <= 6 * 4         # (the shape that path had been tested at)
    # many slabs: more than one 48-slab round of the plain sum, more than one 256-slab round of the cooperative one
    p = ref.plan("logistic", [20, 12, 1])
    assert ref.slabs(p, 2100)[1] == 66 == 48 + 18
    assert ref.cdiv(4128, 16) == 258 > 256 and ref.slabs(p, 4128)[1] == 129


@pytest.mark.parametrize("units,n_hi,n_lo,c_hi,c_lo", [([281, 100, 1], 1345, 1344, 40, 42), ([6, 4, 1], 8193, 8192, 241, 256)])
def test_slab_count_is_not_monotone_and_the_workspace_bound_holds(units, n_hi, n_lo, c_hi, c_lo):
    """what the workspace-reuse tests on the GPU rest on: at 256 compute units the smaller batch launches MORE slabs, and
    tn_slabs64's `most` (what ensure_ws allocates) covers every batch up to n"""
    p = ref.plan("logistic", units)
    assert ref.slabs(p, n_hi)[1] == c_hi and ref.slabs(p, n_lo)[1] == c_lo and c_lo > c_hi
    assert ref.slabs(p, n_hi)[2] >= c_lo
    for cus in (256, 304, 64, 7):
        q = ref.plan("logistic", units, cus)
        worst = 0
        for n in range(1, n_hi + 40):
            rows, count, most = ref.slabs(q, n)
            worst = max(worst, count)
            assert rows >= 32 and rows % 2 == 0 and worst <= most, (cus, n, worst, most)
