"""The inputs of the GPU checks of the weighted graph and of ALS with per-edge confidence (tests/test_gpu_edgew.py,
tests/test_gpu_alsw.py), kept apart from them so that the CPU suite (tests/test_alsw_host.py) can run the same scenes, rules and seeds
through the restatements.  The scenes are als_cases' two:

  rule     scene  half_life  ts_ref  cap        what it exercises
  count    base   0          0       0          rho in {1 .. 5}: repeats only
  decay    base   7          0       0          60 distinct rho, the largest 2.0625
  capref   base   7          40      3 * 65536  entries newer than ts_ref; the cap reached
  dead     base   1          0       0          828 of the 1217 edges have r = 0
  fast     wide   2          0       2 * 65536  hubs of 600 / 256 / 257 holders with unequal weights"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import edgew_ref as E  # noqa: E402

N_ITEMS, N_ITERS, HISTORIES, foldin_rows = K.N_ITEMS, K.N_ITERS, K.HISTORIES, K.foldin_rows

# name: (scene, dict(half_life, ts_ref, cap))
RULES = {
    "count": ("base", dict(half_life=0, ts_ref=0, cap=0)),
    "decay": ("base", dict(half_life=7, ts_ref=0, cap=0)),
    "capref": ("base", dict(half_life=7, ts_ref=40, cap=3 * 65536)),
    "dead": ("base", dict(half_life=1, ts_ref=0, cap=0)),
    "fast": ("wide", dict(half_life=2, ts_ref=0, cap=2 * 65536)),
}
# the rule under which every edge has r = 65536: the weighted equations with the unweighted model's numbers
UNIT = dict(half_life=0, ts_ref=0, cap=65536)

# the fit cases: (als_cases' case, whose scene, D, alpha, lambda and seed they take; the rule)
FIT_CASES = {
    "base-D8/count": ("base-D8", "count"), "base-D8/decay": ("base-D8", "decay"), "base-D8/capref": ("base-D8", "capref"),
    "base-D8/dead": ("base-D8", "dead"), "base-D24/decay": ("base-D24", "decay"), "base-D6/dead": ("base-D6", "dead"),
    "base-D64/decay": ("base-D64", "decay"), "base-D64/capref": ("base-D64", "capref"),
    "wide-D8/fast": ("wide-D8", "fast"), "wide-D64/fast": ("wide-D64", "fast"),
}
_MEMO = {}


def weighted_scene(rule):
    """(seqs, walk_ref.graph, edgew_ref.weights, the rule's dict) of a rule name (or of UNIT over a scene: ("unit", scene))"""
    if rule not in _MEMO:
        sc, kw = (rule[1], UNIT) if isinstance(rule, tuple) else RULES[rule]
        seqs, g = K.scene(sc)
        _MEMO[rule] = (seqs, g, E.weights(g, seqs, **kw), kw)
    return _MEMO[rule]


def fit_case(name):
    """(seqs, g, w, rule dict, D, alpha, lambda, seed) of a fit case"""
    base, rule = FIT_CASES[name]
    sc, D, alpha, lam, seed = K.FIT_CASES[base]
    seqs, g, w, kw = weighted_scene(rule)
    assert RULES[rule][0] == sc
    return seqs, g, w, kw, D, alpha, lam, seed
