"""CPU checks of the bootstrap's definition (tests/boot_ref.py, the restatement the device is compared with) and of its host
surfaces: the Poisson table recomputed in decimal arithmetic, the weights' moments, the weighted AUC formula against the
unweighted reference over repeated rows, the paired weights, the wrappers' argument checks and the struct layouts."""
import ctypes as C
import decimal
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auc_ref  # noqa: E402
import boot_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_is_the_poisson_cdf_in_decimal():
    decimal.getcontext().prec = 60
    e1 = decimal.Decimal(-1).exp()
    cdf, fact, table = decimal.Decimal(0), decimal.Decimal(1), []
    for k in range(13):
        if k:
            fact *= k
        cdf += e1 / fact
        table.append(int((cdf * 2 ** 32).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    assert table == [int(t) for t in boot_ref.T]
    assert table[-1] == 2 ** 32 - 1                       # w <= 13: every later threshold would be 2^32
    # the header's literals are the same table
    txt = open(os.path.join(ROOT, "goctr_amd", "csrc", "metrics_boot.h")).read()
    lits = txt[txt.index("#define GOCTR_BOOT_T"):].split("{", 1)[1].split("}", 1)[0].replace("\\", "")
    assert [int(x.strip().rstrip("u"), 16) for x in lits.split(",")] == table


def test_weight_moments():
    """2^18 draws: mean and variance of Poisson(1) are 1; the standard error of the mean is sqrt(1 / N), of the variance
    sqrt((mu4 - sigma^4) / N) with mu4 = 4 for Poisson(1) (lambda + 3 lambda^2)"""
    N = 1 << 18
    w = np.concatenate([boot_ref.weights(7, b, np.arange(4096)) for b in range(64)]).astype(np.float64)
    assert w.size == N and w.max() <= 13
    assert abs(w.mean() - 1.0) <= 5 * (1.0 / N) ** 0.5
    assert abs(w.var() - 1.0) <= 5 * (3.0 / N) ** 0.5


def test_one_hash_serves_two_replicates():
    u = np.arange(1000)
    for seed in (0, 7, 2 ** 64 - 1):
        lo, hi = boot_ref.draws(seed, 5, u), boot_ref.draws(seed, 4, u)
        assert not np.array_equal(lo, hi)
        # the wraparound arithmetic in Python integers
        for c in (0, 999):
            z = (seed + 0x9E3779B97F4A7C15 * (((2 << 32) | c) + 1)) % 2 ** 64
            z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 % 2 ** 64
            z ^= z >> 27; z = z * 0x94D049BB133111EB % 2 ** 64
            z ^= z >> 31
            assert int(hi[c]) == z >> 32 and int(lo[c]) == z & 0xffffffff
    big = boot_ref.weights(3, 2, np.array([0, 2 ** 31 - 1]))
    assert big.shape == (2,)


@pytest.mark.parametrize("kind", ["distinct", "levels3", "equal"])
@pytest.mark.parametrize("width", [np.float32, np.float64])
def test_formula_equals_the_reference_over_repeated_rows(kind, width):
    """a replicate's (S, den, correct) = auc_ref.reference over the rows repeated w times"""
    rng = np.random.default_rng(11)
    for n in (1, 2, 7, 40):
        s = {"distinct": rng.random(n), "levels3": rng.integers(0, 3, n) / 3.0, "equal": np.full(n, 0.25)}[kind].astype(width)
        y = (rng.random(n) < 0.5).astype(width)
        cl = rng.integers(0, max(n // 3, 1), n)
        for cluster in (None, cl):
            r = boot_ref.reference(s, y, cluster=cluster, replicates=9, seed=n)
            W = boot_ref.weight_matrix(n, 9, np.arange(n) if cluster is None else cluster)
            for b in range(9):
                w = W[b]
                assert int(r["reps"]["n_w"][b]) == int(w.sum())
                if w.sum() == 0:
                    assert int(r["reps"]["s_a"][b]) == 0 and int(r["reps"]["correct_a"][b]) == 0
                    continue
                ref = auc_ref.reference(np.repeat(s, w), np.repeat(y, w))
                assert int(r["reps"]["pos_w"][b]) == ref.positives and int(r["reps"]["neg_w"][b]) == ref.negatives
                assert int(r["reps"]["correct_a"][b]) == ref.correct
                if ref.auc_den:
                    assert int(r["reps"]["s_a"][b]) == ref.auc_num
                    assert 2 * ref.positives * ref.negatives == ref.auc_den
                else:
                    assert int(r["reps"]["s_a"][b]) == 0
                # the boundary form the kernel sums
                assert boot_ref.boundary_S(s, y > 0.5, w) == int(r["reps"]["s_a"][b])


def test_paired_weights_are_shared():
    rng = np.random.default_rng(3)
    n = 300
    a, b = rng.random(n), rng.random(n)
    y = (rng.random(n) < 0.3).astype(np.float64)
    r = boot_ref.reference(a, y, score_b=b, replicates=12, seed=5)
    ra, rb = boot_ref.reference(a, y, replicates=12, seed=5), boot_ref.reference(b, y, replicates=12, seed=5)
    for f in ("n_w", "pos_w", "neg_w"):
        assert np.array_equal(ra["reps"][f], rb["reps"][f]) and np.array_equal(r["reps"][f], ra["reps"][f])
    assert np.array_equal(r["reps"]["s_a"], ra["reps"]["s_a"]) and np.array_equal(r["reps"]["s_b"], rb["reps"]["s_a"])
    assert r["ci"]["auc_b"] == rb["ci"]["auc_a"]
    same = boot_ref.reference(a, y, score_b=a, replicates=12, seed=5)
    assert same["head"]["ties"] == same["head"]["valid"] and same["ci"]["d_auc"]["lo"] == 0.0 == same["ci"]["d_auc"]["hi"]


def test_degenerate_replicates_of_the_reference():
    r = boot_ref.reference(np.array([0.1, 0.2, 0.3]), np.array([1.0, 0.0, 0.0]), replicates=64, seed=0)
    assert r["head"]["valid"] == 64 - 25
    rng = np.random.default_rng(0)
    y = np.zeros(64)
    y[:8] = 1.0
    assert boot_ref.reference(rng.random(64), y, replicates=64, seed=0)["head"]["valid"] == 64
    allpos = boot_ref.reference(rng.random(10), np.ones(10), replicates=5)
    assert allpos["head"]["valid"] == 0 and all(np.isnan(v) for v in allpos["ci"]["auc_a"].values())


def test_wrappers_reject_bad_arguments_without_a_device():
    from goctr_amd import metrics
    s, y = np.linspace(0.1, 0.9, 8), np.array([0, 1] * 4, np.float64)
    bad = [dict(replicates=0), dict(replicates=4097), dict(level=0.0), dict(level=1.0), dict(level=float("nan")),
           dict(chunk_rows=100), dict(chunk_rows=131072), dict(rep_tile=65), dict(rep_tile=-1), dict(seed=-1), dict(seed=2 ** 64)]
    for kw in bad:
        with pytest.raises(ValueError):
            metrics.bootstrap_metrics(s, y, **kw)
    with pytest.raises(ValueError):
        metrics.bootstrap_metrics(s, y[:7])
    with pytest.raises(ValueError):
        metrics.bootstrap_metrics(s, y, score_b=s[:5])
    with pytest.raises(ValueError):
        metrics.bootstrap_metrics(s, y, cluster=np.arange(7))
    with pytest.raises(ValueError):
        metrics.bootstrap_metrics(s, y, cluster=np.array([0, 1, 2, -1, 4, 5, 6, 7]))
    with pytest.raises(ValueError):
        metrics.bootstrap_metrics(s[:0], y[:0])
    with pytest.raises(ValueError):
        metrics.bootstrap_weights(np.arange(4), b0=4095, nb=2)
    with pytest.raises(ValueError):
        metrics.bootstrap_weights(np.arange(0))
    cfg = metrics.make_boot_cfg(replicates=33, seed=2 ** 64 - 1, level=0.9, chunk_rows=512, rep_tile=3)
    assert (cfg.replicates, cfg.seed, cfg.level, cfg.chunk_rows, cfg.rep_tile, cfg.reserved) == (33, 2 ** 64 - 1, 0.9, 512, 3, 0)


def test_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the four bootstrap structs through a compiled C probe, against the ctypes mirrors"""
    from goctr_amd import capi, metrics
    structs = {"goctr_boot_cfg": capi.BootCfg, "goctr_boot_ci": capi.BootCi, "goctr_boot_rep": capi.BootRep,
               "goctr_boot_metrics": capi.BootMetrics}
    lines, exp = [], []
    for cname, st in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        exp.append(C.sizeof(st))
        for f, _ in st._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            exp.append(getattr(st, f).offset)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == exp
    assert metrics.BOOT_REP_DTYPE.itemsize == C.sizeof(capi.BootRep)
    assert [metrics.BOOT_REP_DTYPE.fields[f][1] for f, _ in capi.BootRep._fields_] == [getattr(capi.BootRep, f).offset
                                                                                       for f, _ in capi.BootRep._fields_]


def test_defaults():
    from goctr_amd import capi
    c = capi.default_boot_cfg()
    assert (c.replicates, c.chunk_rows, c.rep_tile, c.reserved, c.seed, c.level) == (200, 0, 0, 0, 0, 0.95)
