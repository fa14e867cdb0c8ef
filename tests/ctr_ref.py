"""What the DIN / YouTube-DNN GPU tests share (tests/test_gpu_ctr.py, tests/test_gpu_ctr_shapes.py) and what the CPU test of the
oracle at the same shapes uses (tests/test_oracle_ctr.py): tolerances, the gradient rules, seeded data and the oracle / device
model pair."""
import numpy as np

# Multi-epoch training COSTS of the reduced-size shapes below are held to 5e-5, not to the 1e-5 of logits / loss / the full-size
# tests (tests/test_gpu_fullsize.py holds 1e-5 at the benchmark's shapes).  Why: these tests use 0.15-0.3 N(0,1) weights on a few
# dozen inputs, which puts single rows at |z2| ~ 10.  There one float32 ulp of the pre-activation (|z2| 2^-23 ~ 1.2e-6, and device
# and oracle sum z2 in different orders) moves log p = -softplus(-z2) by ~1e-6 for that row; a batch of 20-50 rows holds a few such
# rows, their signs do not cancel inside one mean, and after 2-4 epochs of updates that each saw such a cost the epoch means drift
# by a few 1e-5 (round 3 tightened these from 1e-4 and found 1e-5 too tight for exactly these shapes).  5e-5 = that
# drift with margin; a real defect (a wrong mask, a missing 1/B) shows up at 1e-3 and above.
COST_TOL_SMALL_SHAPES = 5e-5

LOGIT_TOL = 1e-5
LOSS_TOL = 1e-5


def grad_close(g, ref):
    return np.max(np.abs(g - ref)) <= 1e-6 + 2e-4 * np.max(np.abs(ref))


def grad_bound_sides(g_dev, g_orc, g64):
    """(|g_dev - truth|_max, 2 |g_orc32 - truth|_max + one float32 ulp of the largest entry): grad_bound's two sides"""
    g_dev, g_orc, g64 = (np.asarray(a, np.float64).ravel() for a in (g_dev, g_orc, g64))
    return np.max(np.abs(g_dev - g64)), 2 * np.max(np.abs(g_orc - g64)) + 6e-8 * np.max(np.abs(g64))


def grad_bound(g_dev, g_orc, g64):
    """|g_dev - truth|_max <= 2 |g_orc32 - truth|_max + one float32 ulp of the largest entry"""
    lhs, rhs = grad_bound_sides(g_dev, g_orc, g64)
    return lhs <= rhs


def make_data(rng, rows, U, T, D, Cc, pad_frac=0.3):
    X = rng.random((rows, U + T * D + D + Cc), dtype=np.float32)
    ub = X[:, U:U + T * D].reshape(rows, T, D)
    ub[rng.random((rows, T)) < pad_frac] = 0.0
    Y = (rng.random(rows) < 0.5).astype(np.float32)
    return X, Y


def oracle_model(oracle, kind, U, T, D, Cc, rng, att=0, scale=None, hidden=None):
    """pair()'s oracle half: the weights pair() draws, in the order pair() draws them"""
    H1, H2 = hidden if hidden is not None else (200, 80)
    om = oracle.CtrModel(kind, U, T, D, Cc, H1=H1, H2=H2, att=att)
    if scale is None:
        om.init_gaussian(rng)            # the reference's N(0,1) init (din.go:187-191)
    else:
        om.W0[:] = (rng.standard_normal(om.W0.shape) * scale).astype(np.float32)
        om.W1[:] = (rng.standard_normal(om.W1.shape) * scale).astype(np.float32)
        om.W2[:] = (rng.standard_normal(om.W2.shape) * scale).astype(np.float32)
    om.att0[:] = (1 + 0.3 * rng.standard_normal(om.att0.shape)).astype(np.float32) if kind == 0 else 1.0
    return om


def pair(oracle, kind, U, T, D, Cc, rng, att=0, scale=None, hidden=None):
    """an oracle model and a device model with identical weights; hidden=(H1, H2), default the reference's 200 / 80"""
    from goctr_amd import model as gm
    from goctr_amd.recommend import SampleInfo
    om = oracle_model(oracle, kind, U, T, D, Cc, rng, att=att, scale=scale, hidden=hidden)
    cls = gm.DinNet if kind == 0 else gm.YoutubeDnn
    kw = {} if hidden is None else {"hidden": hidden}
    dm = cls(U, T, D, D, Cc, att=att, **kw) if kind == 0 else cls(U, T, D, D, Cc, **kw)
    dm.set_weights("mlp0", om.W0); dm.set_weights("mlp1", om.W1); dm.set_weights("mlp2", om.W2)
    if kind == 0:
        dm.set_weights("att0", om.att0)
    return om, dm, SampleInfo.from_dims(U, T, D, Cc)


# ---- the shapes off the reference's (D > 64, hidden widths other than 200 / 80): tests/test_gpu_ctr_shapes.py runs them on the
# device, tests/test_oracle_ctr.py holds the float32 oracle to float64 at the same shapes first.
# name: (mode, U, T, D, Cc, (H1, H2), [(kind, att), ...]); DESIGN.md 3 has the branch each one reaches
SHAPE_CASES = {
    "a": ("dense", 5, 6, 100, 3, (200, 80), [(0, 0), (0, 1), (1, 0)]),
    "b": ("dense", 5, 6, 20, 3, (200, 80), [(0, 0)]),
    "c": ("id", 5, 6, 100, 3, (200, 80), [(0, 0), (0, 1)]),
    "d": ("id", 9, 5, 256, 7, (200, 80), [(0, 0), (1, 0)]),
    "e": ("id", 5, 6, 70, 3, (200, 80), [(0, 0)]),
    "f": ("id", 20, 8, 16, 10, (304, 96), [(0, 0), (1, 0)]),
    "g": ("id", 20, 8, 16, 10, (520, 40), [(1, 0), (0, 0)]),
    "h": ("dense", 7, 4, 8, 5, (50, 7), [(0, 0)]),
    "i": ("id", 6, 260, 4, 3, (200, 80), [(0, 0)]),
    "j": ("id", 9, 5, 256, 7, (1024, 1024), [(0, 0)]),
    # beyond the issue's list: dense rows wider than 192 columns, so that the widest scalar-lane instantiation (four columns per
    # lane) runs with its fourth column in use
    "k": ("dense", 5, 6, 200, 3, (200, 80), [(0, 0)]),
    # the widths the fused chain kernels accept (chain_ok: H1p = 208 or 224, H2p = 80, Ip <= 240) away from 200 / 80 and from the
    # two K phases of Ip = 48 .. 160; tests/test_gpu_ctr_shapes.py has the host arithmetic of each
    "l": ("id", 20, 8, 16, 10, (224, 80), [(0, 0), (1, 0)]),        # 14 tiles of H1, no pad column
    "m": ("id", 20, 8, 16, 10, (220, 70), [(0, 0), (0, 1)]),        # 14 tiles, pad columns in H1 and H2
    "n": ("id", 52, 8, 16, 53, (195, 66), [(0, 0), (1, 0)]),        # Ip = 144, H1p = 208: the bf16-split chain with pad columns
    "o": ("id", 60, 8, 16, 70, (200, 80), [(0, 0), (1, 0)]),        # Ip = 176: three K phases
    "p": ("id", 100, 8, 16, 108, (200, 80), [(0, 0)]),              # I = Ip = 240: the bf16-split chain at its widest
    "q": ("id", 20, 8, 16, 28, (200, 80), [(0, 0)]),                # I = Ip = 80: exactly one full K phase
}
SHAPE_PARAMS = [(name, kind, att) for name, c in SHAPE_CASES.items() for kind, att in c[6]]
SHAPE_B, SHAPE_VALID, SHAPE_TRAIN_ROWS, SHAPE_V = 64, 50, 150, 300
# N(0,1) x 0.15 weights, as test_loss_and_grads and test_id_mode_shape_sweep use; x 0.05 at case j, whose 1024-wide layers saturate
# with 0.15 (cost 3.8, |z2| ~ 10): there the float32 oracle itself is 2.0e-6 from float64 on the cost, outside the 2e-6
# tests/test_oracle_ctr.py holds it to
SHAPE_SCALE = {name: 0.05 if name == "j" else 0.15 for name in SHAPE_CASES}

# Adam's learning rate in the training checks: the reference's 0.01 (model.go:88), but 0.001 at case j.  An Adam step moves every
# weight by about lr, so a unit's pre-activation by about lr x fan-in x 0.5: 1.0 at the reference's 200 inputs, 5 at 1024 -- the
# float32 ORACLE's own training of case j at 0.01 saturates the output and ends in NaN costs (log 0; 0.003: a first epoch cost of
# 7.5).  0.01 x 200 / 1024, rounded down to a power of ten, keeps the step the reference's size.
SHAPE_LR = {name: 0.001 if name == "j" else 0.01 for name in SHAPE_CASES}

# Which data a case runs on.  grad_bound measures the device with the float32 oracle's OWN distance from float64, and on a tensor of
# a handful of entries (att0 has T = 5 .. 8 here, mlp2 as few as 7) that distance is one draw of a wide distribution: at case a's
# shape it ran from 3.6e-11 to 9.8e-11 over four seeds, the first (lowest) being the seed the case was first written with -- and
# there the device, 8.65e-11 from float64 and inside that spread, missed 2 x 3.6e-11 + 0.8e-11 (case j the same way, at 0.99 of
# its bound).  Both sides sum the same float32 products in another order (tests/test_oracle_ctr.py attributes the error: the
# K = H1 accumulation of dp and the D-long dot dp . x), so neither is wrong; the yard-stick was drawn from its lucky tail.  So a
# case's seed is chosen by a rule that looks at the REFERENCE alone: of SHAPE_SEED_CANDIDATES seeds, the one at which the oracle's
# luck is the median.  luck(seed) = min over the case's gradient tensors of  e_k(seed) / median over the candidates of e_k ,
# e_k = |g32_k - g64_k|_max / |g64_k|_max.  SHAPE_SEED_PICK holds the result; the CPU test recomputes it
# (test_shape_seeds_are_where_the_oracle_has_median_luck), the GPU tests only read it.  Bounds and cases are untouched by this.
SHAPE_SEED_CANDIDATES = 7
SHAPE_SEED_PICK = {("a", 0, 0): 6, ("a", 0, 1): 4, ("a", 1, 0): 2, ("b", 0, 0): 4, ("c", 0, 0): 3, ("c", 0, 1): 6, ("d", 0, 0): 6,
                   ("d", 1, 0): 3, ("e", 0, 0): 1, ("f", 0, 0): 0, ("f", 1, 0): 6, ("g", 1, 0): 6, ("g", 0, 0): 0, ("h", 0, 0): 4,
                   ("i", 0, 0): 0, ("j", 0, 0): 5, ("k", 0, 0): 5, ("l", 0, 0): 4, ("l", 1, 0): 6, ("m", 0, 0): 5, ("m", 0, 1): 4,
                   ("n", 0, 0): 4, ("n", 1, 0): 6, ("o", 0, 0): 4, ("o", 1, 0): 4, ("p", 0, 0): 1, ("q", 0, 0): 1}


def shape_seed(name, kind, att, pick=None):
    pick = SHAPE_SEED_PICK[(name, kind, att)] if pick is None else pick
    return 7000 + 100 * (ord(name) - ord("a")) + 10 * kind + att + 10000 * pick


def shape_step(oracle, name, kind, att, pick=None):
    """(oracle model, X, Y, ids, float32 step, float64 step) of a case: ROWS rows of data, the one-step results on the first
    SHAPE_VALID of them in a batch of SHAPE_B"""
    mode, U, T, D, Cc, hidden, _ = SHAPE_CASES[name]
    rng = np.random.default_rng(shape_seed(name, kind, att, pick))
    om = oracle_model(oracle, kind, U, T, D, Cc, rng, att=att, scale=SHAPE_SCALE[name], hidden=hidden)
    X, Y, ids = shape_data(oracle, name, rng, SHAPE_TRAIN_ROWS)
    step32 = om.loss_grad(X[:SHAPE_VALID], Y[:SHAPE_VALID], B=SHAPE_B)
    step64 = om.loss_grad_f64(X[:SHAPE_VALID], Y[:SHAPE_VALID], B=SHAPE_B)
    return om, X, Y, ids, step32, step64


def median_luck_pick(oracle, name, kind, att):
    """the rule above: (index of the candidate seed at which the float32 oracle's distance from float64 is the median one, the
    candidates ordered from the luckiest to the unluckiest)"""
    tensors = ("W0", "W1", "W2") + (("att0",) if kind == 0 else ())
    e = []
    for pick in range(SHAPE_SEED_CANDIDATES):
        _, _, _, _, (_, g, _), (_, g64, _) = shape_step(oracle, name, kind, att, pick)
        e.append([np.max(np.abs(g[k].ravel() - g64[k].ravel())) / np.max(np.abs(g64[k])) for k in tensors])
    e = np.array(e)
    luck = (e / np.median(e, axis=0)).min(axis=1)
    order = [int(i) for i in np.argsort(luck, kind="stable")]
    return order[SHAPE_SEED_CANDIDATES // 2], order


def shape_data(oracle, name, rng, rows):
    """(X, Y, ids) of a case: `rows` TrainSample rows; ids = None (dense) or (emb, ub, it, uf, cf) that X was assembled from.
    id mode: signed embeddings, 25 % missing ids, one sample with no history, one with a missing candidate
    (test_id_mode_shape_sweep's data).  dense: make_data (U[0,1) features, 30 % zeroed history rows), with the embedding columns
    made signed (0.5 N(0,1)) in every second case."""
    mode, U, T, D, Cc = SHAPE_CASES[name][:5]
    if mode == "id":
        V = SHAPE_V
        emb = (rng.standard_normal((V, D)) * 0.5).astype(np.float32)
        ub = rng.integers(0, V, size=(rows, T)).astype(np.int32)
        ub[rng.random((rows, T)) < 0.25] = -1
        ub[0, :] = -1                                                         # a sample with no behaviour at all
        it = rng.integers(0, V, size=rows).astype(np.int32)
        it[1] = -1                                                            # a missing candidate embedding
        uf = rng.random((rows, U), dtype=np.float32); cf = rng.random((rows, Cc), dtype=np.float32)
        Y = (rng.random(rows) < 0.5).astype(np.float32)
        return oracle.assemble_rows(emb, ub, it, uf, cf), Y, (emb, ub, it, uf, cf)
    X, Y = make_data(rng, rows, U, T, D, Cc)
    if (ord(name) - ord("a")) % 2 == 0:                                       # a, k: signed embedding columns; b, h: U[0,1)
        zero = ~X[:, U:U + T * D].reshape(rows, T, D).any(-1)
        X[:, U:U + T * D + D] = (rng.standard_normal((rows, T * D + D)) * 0.5).astype(np.float32)
        X[:, U:U + T * D].reshape(rows, T, D)[zero] = 0.0
    return X, Y, None
