"""float64 numpy restatement of the reference's sklearn-port MLP (nn/neural_network/basemlp64.go) for all three output heads
and the learning-rate schedules -- what the softmax / identity heads and the schedules are checked against, since the C oracle
(oracle/orc_sklmlp.c) knows only the logistic head and the constant schedule.  Written from the Go semantics:

  forwardPass :259-274        act(A_i . W_i + b_i); hidden activation, then the output activation on the last block
  Activations64 :79-117       logistic, tanh(-z) (quirk Q9), relu, identity; softmax: exp of each column in column order
                              into a running sum, then the divide -- no max subtraction
  LossFunctions64 :151-195    square_loss sum e^2 / 2 / h.Rows; log_loss sum over y != 0 of -y log(clamp h) / h.Rows;
                              binary_log_loss; clamps Nextafter(0, 1) / Nextafter(1, 0)
  backprop :340-406           deltas[last] = h - y over y.Rows, then the hidden deltas with the activation derivative
                              (relu' tests a == 0, quirk Q12); computeLossGrad :322-330, matRowMean64 :213-226
  fitStochastic :729-857      short last batch (quirk Q11): only activations[0] has the short row count, the other blocks keep
                              the previous batch's rows beyond it; epoch loss sum(batch loss x rows) / rows; mlp.t += rows
  SGDOptimizer64 :988-1039    Nesterov momentum; invscaling rate lr_init / (t + 1)^power_t at each epoch's end;
                              adaptive: stop at rate <= 1e-6, else rate x 0.8
  AdamOptimizer64 :1041-1091  beta powers advanced once per PARAMETER (quirk Q7); adaptive scales LearningRateInit and
                              tests the last effective rate

Matrix products are numpy's (summation order differs from the reference's): compare at 1e-9-ish relative, never bit-exact.
Batch normalisation and weight decay are not restated (the new heads share that code with the logistic head).

The last part (SHAPE_CASES, plan) is the table of shapes of tests/test_mlp_shapes_host.py and tests/test_gpu_mlp_shapes.py and a
restatement of the host's launch arithmetic, so that the tests can say which kernel and grid a shape reaches."""
import math
import types

import numpy as np

HMIN, HMAX = np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)


def act(kind, z):
    if kind == "logistic":
        return 1 / (1 + np.exp(-z))
    if kind == "tanh":
        return np.tanh(-z)                       # Q9
    if kind == "relu":
        return np.where(z < 0, 0.0, z)
    if kind == "softmax":
        return softmax_rows(z)
    return z


def softmax_rows(z):
    """Activations64["softmax"]: per row, e_c = exp(z_c) and sum += e_c in column order, then e_c / sum"""
    e = np.exp(z)
    s = np.zeros(z.shape[0])
    for c in range(z.shape[1]):
        s = s + e[:, c]
    return e / s[:, None]


def deriv(kind, a, d):
    if kind == "logistic":
        return d * (a * (1 - a))
    if kind == "tanh":
        return d * (1 - a * a)
    if kind == "relu":
        return np.where(a == 0, 0.0, d)          # Q12
    return d


def loss_sum(out, y, h):
    """the numerator of LossFunctions64[name] over y's rows (the caller divides by h.Rows)"""
    if out == "identity":                        # square_loss
        e = h - y
        return float(np.sum(e * e)) / 2
    hc = np.clip(h, HMIN, HMAX)
    if out == "softmax":                         # log_loss: only terms with y != 0
        return float(np.sum(np.where(y != 0, -y * np.log(np.where(y != 0, hc, 1.0)), 0.0)))
    return float(np.sum(-y * np.log(hc) - (1 - y) * np.log1p(-hc)))     # binary_log_loss


def unpack(units, theta):
    bs, Ws, off = [], [], 0
    for i in range(len(units) - 1):
        fi, fo = units[i], units[i + 1]
        bs.append(theta[off:off + fo]); off += fo
        Ws.append(theta[off:off + fi * fo].reshape(fi, fo)); off += fi * fo
    return bs, Ws


def nparams(units):
    return sum((1 + units[i]) * units[i + 1] for i in range(len(units) - 1))


def blocks(units, B, dtype=np.float64):
    """fit's activation / delta blocks (basemlp64.go:529-545): B rows per layer, zero-filled"""
    return ([None] + [np.zeros((B, u), dtype) for u in units[1:]], [np.zeros((B, u), dtype) for u in units[1:]])


def forward(units, hidden, out, theta, X, acts=None):
    """forwardPass on len(X) rows, or -- with the caller's B-row blocks -- the short-batch form (only the first product has
    len(X) rows; rows beyond it keep the previous batch's values and are re-biased and re-activated like the others)"""
    bs, Ws = unpack(units, theta)
    L = len(units)
    ns = X.shape[0]
    if acts is None:
        acts = [None] + [np.zeros((ns, u)) for u in units[1:]]
    acts[0] = X
    for i in range(L - 1):
        kind = hidden if i + 1 != L - 1 else out
        z = acts[i + 1].copy()
        prod = acts[i] @ Ws[i]
        z[:prod.shape[0]] = prod
        acts[i + 1][:] = act(kind, z + bs[i])
    return acts


def loss_grad_rows(units, hidden, out, alpha, theta, X, Y, acts, deltas):
    """backprop (basemlp64.go:340-406) for a batch of ns = len(X) rows on B-row blocks (ns < B: the short last batch, Q11)"""
    ns, B = X.shape[0], acts[1].shape[0]
    L = len(units)
    bs, Ws = unpack(units, theta)
    forward(units, hidden, out, theta, X, acts)
    H = acts[L - 1]
    loss = loss_sum(out, Y, H[:ns]) / B                     # sum over y.Rows / h.Rows
    loss += (0.5 * alpha) * sum(float(np.sum(W * W)) for W in Ws) / ns
    last = L - 2
    deltas[last][:ns] = H[:ns] - Y                          # rows beyond ns keep their values
    gb, gW = [None] * (L - 1), [None] * (L - 1)
    for layer in range(last, -1, -1):
        a = acts[layer]
        gW[layer] = (a.T @ deltas[layer][:a.shape[0]]) * (1 / ns) + (alpha / ns) * Ws[layer]
        gb[layer] = deltas[layer].sum(axis=0) / B           # matRowMean64 over deltas.Rows = B
        if layer >= 1:
            deltas[layer - 1][:] = deriv(hidden, acts[layer], deltas[layer] @ Ws[layer].T)
    g = np.concatenate([np.concatenate([gb[i], gW[i].ravel()]) for i in range(L - 1)])
    return loss, g


def loss_grad(units, hidden, out, alpha, theta, X, Y):
    acts, deltas = blocks(units, X.shape[0])
    return loss_grad_rows(units, hidden, out, alpha, theta.copy(), np.asarray(X, np.float64), np.asarray(Y, np.float64),
                          acts, deltas)


class SGD:
    """SGDOptimizer64 (basemlp64.go:988-1039)"""

    def __init__(self, n, lr_init, schedule="constant", power_t=0.5, momentum=0.9, nesterov=True):
        self.LearningRateInit = self.LearningRate = lr_init
        self.LRSchedule, self.PowerT, self.Momentum, self.Nesterov = schedule, power_t, momentum, nesterov
        self.velocities = np.zeros(n)

    def updateParams(self, theta, g):
        upd = self.Momentum * self.velocities - self.LearningRate * g
        self.velocities = upd
        theta += (self.Momentum * upd - self.LearningRate * g) if self.Nesterov else upd

    def iterationEnds(self, t):
        if self.LRSchedule == "invscaling":
            self.LearningRate = self.LearningRateInit / math.pow(t + 1, self.PowerT)

    def triggerStopping(self):
        if self.LRSchedule != "adaptive" or self.LearningRate <= 1e-6:
            return True
        self.LearningRate *= 0.8
        return False


class Adam:
    """AdamOptimizer64 (basemlp64.go:1041-1091): the beta powers advance once per PARAMETER (Q7) -- the running products are
    np.cumprod of the same factors, in the same order"""

    def __init__(self, n, lr_init, schedule="constant", beta1=0.9, beta2=0.999, eps=1e-8):
        self.LearningRateInit = self.LearningRate = lr_init
        self.LRSchedule, self.Beta1, self.Beta2, self.Epsilon = schedule, beta1, beta2, eps
        self.ms, self.vs = np.zeros(n), np.zeros(n)
        self.beta1t = self.beta2t = 1.0
        self.t = 0

    def updateParams(self, theta, g):
        n = g.size
        self.t += 1
        self.ms = self.Beta1 * self.ms + (1 - self.Beta1) * g
        self.vs = self.Beta2 * self.vs + (1 - self.Beta2) * g * g
        b1t = np.cumprod(np.concatenate([[self.beta1t * self.Beta1], np.full(n - 1, self.Beta1)]))
        b2t = np.cumprod(np.concatenate([[self.beta2t * self.Beta2], np.full(n - 1, self.Beta2)]))
        self.beta1t, self.beta2t = b1t[-1], b2t[-1]
        lr = self.LearningRateInit * np.sqrt(1 - b2t) / (1. - b1t)
        self.LearningRate = float(lr[-1])
        theta += -lr * self.ms / (np.sqrt(self.vs) + self.Epsilon)

    def iterationEnds(self, t):
        pass

    def triggerStopping(self):
        if self.LRSchedule != "adaptive" or self.LearningRate <= 1e-6:
            return True
        self.LearningRateInit *= 0.8
        return False


def fit(units, hidden, out, alpha, theta, opt, X, Y, batch, max_iter, tol=1e-4, n_iter_no_change=10, perm=None):
    """fitStochastic (basemlp64.go:729-857) without early stopping: returns (loss curve, NIter); theta is updated in place"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64).reshape(len(X), -1)
    n = X.shape[0]
    batch = min(batch, n)
    acts, deltas = blocks(units, batch)
    best, no_improve, t = math.inf, 0, 0
    curve = []
    for it in range(max_iter):
        order = perm[it] if perm is not None else np.arange(n)
        acc = 0.0
        for s in range(0, n, batch):
            idx = order[s:s + batch]
            bl, g = loss_grad_rows(units, hidden, out, alpha, theta, X[idx], Y[idx], acts, deltas)
            acc += bl * len(idx)
            opt.updateParams(theta, g)
        loss = acc / n
        curve.append(loss)
        t += n
        if loss > best - tol:                    # updateNoImprovementCount :859-895
            no_improve += 1
        else:
            no_improve = 0
        if loss < best:
            best = loss
        opt.iterationEnds(float(t))
        if no_improve > n_iter_no_change:
            if opt.triggerStopping():
                break
            no_improve = 0
    return np.array(curve), len(curve)


# ---------------------------------------------------------------- shapes off the handful the other MLP tests use
# (tests/test_mlp_shapes_host.py, tests/test_gpu_mlp_shapes.py).  name -> (output head, layer units, what the shape reaches on the
# device; the arithmetic behind each note is plan() below and is asserted by the host test)
SHAPE_CASES = {
    "a": ("logistic", [20, 31, 1], "up1 = 32: one full wavefront of hidden columns, the ones column in its last lane column"),
    "b": ("logistic", [16, 40, 1], "F % 16 == 0: the tail chunk holds the ones column alone; up1 = 48: ng = 2, second wavefront half filled"),
    "c": ("logistic", [47, 70, 1], "F % 16 == 15; up1 = 80: ng = 3"),
    "d": ("logistic", [383, 127, 1], "the largest fused shape: up0 = 384 (24 chunks), up1 = 128 (ng = 4, all full), mlp_tn64_kernel at NT = 8"),
    "e": ("logistic", [384, 20, 1], "up0 = 400 > 384: a binary net on the per-layer kernels; K phases 128, 128, 128, 16; mlp_tn64_kernel with KT = 25"),
    "f": ("logistic", [20, 128, 1], "NT = 9: gemm_tn_kernel<double,3,2,16> with WK = 1, grid.z = 3; gemm_nn_kernel<double> with grid.y = 2"),
    "g": ("logistic", [100, 200, 80, 1], "the DIN widths: NT = 13, KT = 7 -> WK = 2, grid.y = 2, grid.z = 4; layer 1 in two K phases (128 + 80)"),
    "h": ("softmax", [30, 150, 70], "70 classes: two 64-column rounds of mlp_softmax_kernel; upL = 80; layer 0 on gemm_tn_kernel (NT = 10)"),
    "i": ("identity", [12, 9, 130], "the output layer on gemm_tn_kernel with KT = 1; upL = 144"),
    "j": ("logistic", [9, 17, 5, 33, 3, 16, 15, 1], "eight layers, goctr_mlp_create's limit: seven blocks in the reduce launch's layer lookup"),
}
SHAPE_HIDDEN = ("relu", "logistic", "tanh", "identity")
SHAPE_ALPHA = 1e-2


def _case_rng(name, stream):
    return np.random.default_rng([20, ord(name), stream])


def case_theta(name, hidden):
    """the case's parameters: initialize's one-sided draw (goctr_amd.mlp init_params, quirk Q8) halved, as tests/test_gpu_mlp.py does"""
    from goctr_amd import mlp as gmlp
    _, units, _ = SHAPE_CASES[name]
    return gmlp.MLPClassifier(units[1:-1], hidden).init_params(units, _case_rng(name, 0)) * 0.5


def case_data(name, rows, stream=1):
    """float32 rows and targets of a case.  The inputs are CENTRED ([-0.5, 0.5)): with [0, 1) inputs and one-sided weights the relu
    net of [383,127,1] saturates its logistic head, and the clamped log-loss then differs by 4e-5 relative between float64 and
    extended precision -- a property of the data, not of a kernel"""
    head, units, _ = SHAPE_CASES[name]
    rng = _case_rng(name, stream)
    X = (rng.random((rows, units[0])) - 0.5).astype(np.float32)
    return X, targets(rng, rows, units[-1], head)


def targets(rng, rows, no, head):
    if head == "softmax":
        return np.eye(no, dtype=np.float32)[rng.integers(0, no, rows)]
    if head == "identity":
        return rng.standard_normal((rows, no)).astype(np.float32)
    return (rng.random((rows, no)) < 0.5).astype(np.float32)


# ---- the host's dispatch, restated (csrc/mlp.hip: forward, backward, tn_slabs64; csrc/mlp_kernels.h: launch_nn64, launch_tn64;
# csrc/mlp_model.h: fused_ok, chain_ok; csrc/mfma_gemm.h: gemm_nn_phase_rows)
def up(u):
    """padded width of a layer: its units and the ones column, rounded up to 16"""
    return (u + 16) // 16 * 16


def cdiv(a, b):
    return -(-a // b)


def nn_launch(Kp, Np):
    """launch_nn64 -> gemm_nn_kernel<double, Epi, ntw>: C[M, Np] = A[M, Kp] . B[Kp, Np]"""
    NT = Np // 16
    WN = 2 if NT >= 2 else 1
    ntw = cdiv(NT, WN)
    ntw = 1 if ntw <= 1 else (2 if ntw <= 2 else 4)
    blk = WN * ntw                                           # tiles per column block
    grid_y = cdiv(NT, blk)
    kph = min(152 * 1024 // ((blk * 16 + 4) * 8) // 16 * 16, 8 * 16, Kp)      # rows of B per LDS phase
    return types.SimpleNamespace(
        NT=NT, WN=WN, ntw=ntw, grid_y=grid_y, phases=[min(kph, Kp - k0) for k0 in range(0, Kp, kph)],
        # tiles[y][wn]: 16-column tiles wavefront column wn of column block y stores
        tiles=[[max(0, min(ntw, min(blk, NT - y * blk) - wn * ntw)) for wn in range(WN)] for y in range(grid_y)])


def tn_launch(KT, NT):
    """launch_tn64: the weight-gradient product of a layer with KT x NT 16-wide tiles"""
    if NT <= 8:
        gy = cdiv(KT, 3)
        return types.SimpleNamespace(kernel="mlp_tn64_kernel", KT=KT, NT=NT, grid_y=gy, grid_z=1, workgroups=gy,
                                     kcnt=[[min(3, KT - 3 * y)] for y in range(gy)], ncnt=[[min(2, max(0, NT - 2 * w)) for w in range(4)]])
    WK, WN = (2 if KT >= 6 else 1), min(2, cdiv(NT, 2))
    gy, gz = cdiv(KT, WK * 3), cdiv(NT, WN * 2)
    return types.SimpleNamespace(
        kernel="gemm_tn_kernel<double,3,2,16>", KT=KT, NT=NT, WK=WK, WN=WN, grid_y=gy, grid_z=gz, workgroups=gy * gz,
        # kcnt[y][wk] / ncnt[z][wn]: tiles of A's / D's columns wavefront row wk / column wn of block y / z owns
        kcnt=[[max(0, min(3, min(WK * 3, KT - y * WK * 3) - wk * 3)) for wk in range(WK)] for y in range(gy)],
        ncnt=[[max(0, min(2, min(WN * 2, NT - z * WN * 2) - wn * 2)) for wn in range(WN)] for z in range(gz)])


def plan(head, units, cus=256):
    """what the host launches for a net: the fused / chain kernels or the per-layer GEMMs, and every GEMM's grid"""
    ups = [up(u) for u in units]
    nl = len(units) - 1
    fused = nl == 2 and units[2] == 1 and head == "logistic" and ups[1] <= 128 and ups[0] <= 16 * 24
    p = types.SimpleNamespace(units=list(units), up=ups, nl=nl, fused=fused, chain=fused,    # (chain_ok's two divisibility tests
                              ng=cdiv(ups[1], 32) if fused else 0, nch=ups[0] // 16,         # hold for every up[2] = 16)
                              tn=[tn_launch(ups[l] // 16, ups[l + 1] // 16) for l in range(nl)],
                              fwd=[nn_launch(ups[l], ups[l + 1]) for l in range(nl)],
                              bwd={l: nn_launch(ups[l + 1], ups[l]) for l in range(1, nl)})
    p.cap = max(1, cus // max(t.workgroups for t in p.tn))
    return p


def slabs(p, n):
    """tn_slabs64: (rows per slab, slabs over n rows, the most slabs any n' <= n has)"""
    rows = cdiv(n, p.cap)
    rows = 32 if rows < 32 else rows + rows % 2
    return rows, cdiv(n, rows), min(p.cap, cdiv(n, 32))
