"""GPU checks of the conjugate-gradient kernels (csrc/als_cg.hip) at every width class and on every path, beside
tests/test_gpu_als_cg.py, which holds the semantics at a few widths: every (C, G staged or not) class and both sides of every class
edge in a fit, the long-row kernel's rounds of four segments on both sides against the restatement, the early stop with r.r exactly
zero and clearly below 2^-100, the fold-in unstaged and at C = 3 and 4 with every request count of a workgroup, and the claim that
no byte of a row depends on its place.  The cases are tests/alscg_cases.py's (tests/test_alscg_cases_host.py holds them against the
restatement alone); the tolerance is test_gpu_als_cg.py's: 16 x e0 of the longdouble restatement, e0 its own spread."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import alscg_cases as S  # noqa: E402
import alscg_ref as G  # noqa: E402
import itemnbr_ref as N  # noqa: E402
from test_gpu_als_cg import ALPHA_LAMBDA, RUNS, SEED, handle, scenes, spread  # noqa: E402,F401
from test_gpu_itemcf import MODES, Cache  # noqa: E402

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [f"D{D}{'w' if w else ''}" for D, w in cases]


def _errs(h, runs):
    e = h.export()
    return e, dict(zip("XYl", (A.rel_diff(got, want) for got, want in zip((e["X"], e["Y"], np.array([h.loss()])), runs[2]))))


# 1. ------------------------------------------------------------------------------------------ fit parity at every width class
@pytest.mark.parametrize("D,weighted", S.FIT_CASES, ids=_ids(S.FIT_CASES))
def test_base_fit_at_every_width_class(scenes, D, weighted):
    runs = S.base_fit_runs(D, weighted)
    e0 = spread(runs)
    h = handle(scenes["base", weighted], D, "base", cg_steps=S.CG_STEPS).fit()
    e, errs = _errs(h, runs)
    print(f"base-D{D}{'-weighted' if weighted else ''} ({S.WIDTHS[D]}): e0 = {e0:.3e}, device / restatement: {errs}")
    assert h.solver()["cg_steps"] == S.CG_STEPS and h.info()["half_steps"] == 2 * S.N_ITERS
    assert e["X"][0].tobytes() == bytes(8 * D)                                   # the user without entries: exactly zero
    assert 0 < e0 < 1e-11 and all(err <= 16 * e0 for err in errs.values())


# 2. ----------------------------------------------------------------------------------------------------------- the scene long
@pytest.fixture(scope="module")
def long_graphs():
    """weighted -> the device's graph over the scene long"""
    from goctr_amd import recall as gl
    c = Cache(S.long_scene()[0])
    return {False: gl.WalkGraph(c.c, S.LONG_ITEMS), True: gl.WalkGraph(c.c, S.LONG_ITEMS, weights=S.LONG_RULE)}


def long_handle(graph, D, n_iters=S.LONG_ITERS, **kw):
    from goctr_amd import recall as gl
    alpha, lam = S.LONG_ALPHA_LAMBDA
    return gl.ALS(graph, D=D, n_iters=n_iters, alpha=alpha, lambda_=lam, seed=SEED, solver="cg", cg_steps=S.CG_STEPS, **kw)


@pytest.mark.parametrize("D,weighted", S.LONG_FIT_CASES, ids=_ids(S.LONG_FIT_CASES))
def test_long_rows_of_both_sides_equal_the_restatement(long_graphs, monkeypatch, D, weighted):
    _, g, w = S.long_scene()
    graph = long_graphs[weighted]
    assert (graph.n_users, graph.n_items, graph.n_edges) == (g["n_users"], g["n_items"], g["n_edges"])
    if weighted:
        gw = graph.weights()
        assert np.array_equal(gw["uw"], w["uw"]) and np.array_equal(gw["iw"], w["iw"])
    runs = S.long_fit_runs(D, weighted)
    e0 = spread(runs)
    monkeypatch.setenv("GOCTR_ALS_LONG_ROW", str(S.LONG_THR))                    # (read at create)
    h = long_handle(graph, D).fit()
    e, errs = _errs(h, runs)
    rows = {f"{side[0]}{row}": A.rel_diff(e["X" if side == "users" else "Y"][row], runs[2][side == "items"][row]) for side, row in S.LONG_ROWS}
    print(f"long-D{D}{'-weighted' if weighted else ''}: e0 = {e0:.3e}, device / restatement: {errs}, the named rows: {rows}")
    assert 0 < e0 < 1e-11 and all(err <= 16 * e0 for err in errs.values()) and np.isfinite(e["X"]).all() and np.isfinite(e["Y"]).all()
    assert all(e[k][row].any() for k, row in (("Y", 0), ("Y", 1), ("Y", 2), ("Y", 3), ("X", 1024)))
    if D == 160:                                                                 # the same bytes with every row in the row kernel
        monkeypatch.setenv("GOCTR_ALS_LONG_ROW", "4096")
        t = long_handle(graph, D).fit()
        et = t.export()
        assert all(e[k].tobytes() == et[k].tobytes() for k in e) and h.loss() == t.loss()


# 3. ----------------------------------------------------------------------------------------------------------- the early stop
def _held_to(got, outs, rest, what):
    e0 = spread([(out[rest],) for out in outs])
    err = A.rel_diff(got[rest], outs[2][rest])
    print(f"{what}: e0 = {e0:.3e}, device / restatement {err:.3e} over the {len(rest)} rows that run")
    assert 0 < e0 < 1e-11 and err <= 16 * e0 and np.isfinite(got).all()


@pytest.mark.parametrize("D", S.STOP_WIDTHS)
def test_a_row_with_no_residual_stops_without_a_division_row_form(D):
    from goctr_amd import recall as gl
    Y, outs, _ = S.stop_case(D)
    graph = gl.WalkGraph(Cache(S.stop_seqs()).c, K.N_ITEMS)
    alpha, lam = S.BASE_ALPHA_LAMBDA
    h = gl.ALS(graph, D=D, n_iters=1, alpha=alpha, lambda_=lam, seed=SEED, solver="cg", cg_steps=S.CG_STEPS)
    X = h.set_factors(X=np.zeros((S.STOP_USERS, D)), Y=Y).step("users").export()["X"]
    zero, tiny = list(S.STOP_KINDS["zero"]), list(S.STOP_KINDS["tiny"])
    assert not np.isnan(X[zero]).any() and (X[zero] == 0.0).all()                # r.r = 0 exactly: no 0 / 0
    assert X[tiny].tobytes() == bytes(8 * D * len(tiny))                         # r.r near 2^-110: the start bytes
    assert X[12].tobytes() == bytes(8 * D)                                       # no entries
    _held_to(X, outs, [u for u in range(13, S.STOP_USERS)], f"stop-D{D}")


@pytest.mark.parametrize("kind", ["zero", "tiny"])
def test_a_row_with_no_residual_stops_without_a_division_long_form(long_graphs, monkeypatch, kind):
    D = S.LONG_STOP_D
    X, outs, _ = S.long_stop_case(kind)
    monkeypatch.setenv("GOCTR_ALS_LONG_ROW", str(S.LONG_THR))
    h = long_handle(long_graphs[False], D)
    Y = h.set_factors(X=X, Y=np.zeros((S.LONG_ITEMS, D))).step("items").export()["Y"]
    # item 2 (257 holders: the long form, every wavefront leaves at s_done) and item 3 (256: the row kernel) keep their start
    assert not np.isnan(Y[[2, 3]]).any() and Y[[2, 3]].tobytes() == bytes(8 * D * 2)
    _held_to(Y, outs, [i for i in range(S.LONG_ITEMS) if i not in (2, 3)], f"long-stop-{kind}-D{D}")
    assert Y[0].any() and Y[1].any()


# 4. ------------------------------------------------------------------------------------------------------------------ fold-in
@pytest.mark.parametrize("D,weighted", S.FOLDIN_WIDTHS, ids=_ids(S.FOLDIN_WIDTHS))
def test_foldin_unstaged_and_wide(scenes, D, weighted):
    c, _, _, _, rule = scene = scenes["base", weighted]
    alpha, lam = ALPHA_LAMBDA["base"]
    h = handle(scene, D, "base").fit()
    Y = h.export()["Y"]
    v = h.item_vectors()
    q = v.export()["q"]
    users, ts = K.foldin_rows(c.seqs)
    rule = None if rule is None else dict(ts_ref_used=rule["ts_ref_used"], half_life=rule["half_life"], cap=rule["cap"])
    for H in S.FOLDIN_HISTORIES:
        runs = [G.foldin(Y, c.seqs, users, ts, H, alpha, lam, 10, rule, order, dtype) for order, dtype in RUNS]
        e0 = spread([(r["x"],) for r in runs])
        got = h.foldin(c.c, users, ts, H)
        err = A.rel_diff(got["x"], runs[2]["x"])
        print(f"foldin-D{D}{'-weighted' if weighted else ''} H{H}: e0 = {e0:.3e}, device / restatement {err:.3e}")
        assert e0 > 0 and err <= 16 * e0
        assert np.array_equal(got["n"], runs[2]["n"]) and np.array_equal(got["p"], N.quantise(got["x"])[0]) and got["n"][0] == 0
        rec = h.recall_users(v, c.c, users, ts, validate=True, history=H, n_cand=16, exclude="all")
        want = A.scan(rec["p"], q, c.seqs, users, ts, None, n_cand=16, exclude=MODES["all"])
        assert np.array_equal(rec["p"], got["p"]) and rec["x"].tobytes() == got["x"].tobytes() and (rec["count"] > 0).any()
        assert all(np.array_equal(rec[k], want[k]) for k in ("items", "w", "count"))
        # 1, 5 and 8 requests: a workgroup with one live wavefront, a second workgroup with one, two full ones.  The rows are the
        # first of the twelve, so the restatement's rows hold them too
        for k in S.FOLDIN_COUNTS:
            part = h.foldin(c.c, users[:k], ts[:k], H)
            assert part["x"].shape == (k, D) and A.rel_diff(part["x"], runs[2]["x"][:k]) <= 16 * e0
            assert np.array_equal(part["n"], runs[2]["n"][:k]) and np.array_equal(part["p"], N.quantise(part["x"])[0])
            assert part["x"].tobytes() == got["x"][:k].tobytes()
    # one request row at the places 0 .. 7 of a batch among different neighbours: the same bytes eight times
    row, others = (7, 20), [(u, t) for u, t in zip(users.tolist(), ts.tolist()) if u != 7]
    seen = set()
    for pos in range(8):
        rest = others[pos:] + others[:pos]
        batch = rest[:pos] + [row] + rest[pos:7]
        bu, bt = np.array([b[0] for b in batch], np.int32), np.array([b[1] for b in batch], np.int64)
        got = h.foldin(c.c, bu, bt, 50)
        assert bu[pos] == 7 and got["n"][pos] > 1 and got["x"][pos].any()
        seen.add((got["x"][pos].tobytes(), got["p"][pos].tobytes(), int(got["n"][pos])))
    assert len(seen) == 1


# 5. ---------------------------------------------------------------------------------- place and form at an unstaged width
def test_no_byte_depends_on_the_group_or_the_form_unstaged(monkeypatch):
    from goctr_amd import recall as gl
    D, n_items = 200, 320
    rng = np.random.default_rng(29)
    seqs = {u: ([int(i) for i in rng.integers(0, n_items, size=int(rng.integers(2, 31)))], None) for u in range(101)}
    seqs[3] = (list(range(10, 310)), None)                                       # 300 entries: the long form at threshold 256
    pairs = [(3, 3 + 17), (4, 4 + 40), (5, 5 + 95)]                              # the same row at another place of another group
    for src, dst in pairs:
        seqs[dst] = seqs[src]
    seqs = {u: (items, list(range(len(items), 0, -1))) for u, (items, _) in seqs.items()}
    graph = gl.WalkGraph(Cache(seqs).c, n_items)
    out = {}
    for thr in (256, 4096):
        monkeypatch.setenv("GOCTR_ALS_LONG_ROW", str(thr))                       # (read at create)
        out[thr] = gl.ALS(graph, D=D, seed=SEED, solver="cg").step("users").export()["X"]
    X = out[256]
    assert all(X[src].tobytes() == X[dst].tobytes() and X[src].any() for src, dst in pairs) and np.isfinite(X).all()
    assert X.tobytes() == out[4096].tobytes()
