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
Batch normalisation and weight decay are not restated (the new heads share that code with the logistic head)."""
import math

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


def blocks(units, B):
    """fit's activation / delta blocks (basemlp64.go:529-545): B rows per layer, zero-filled"""
    return ([None] + [np.zeros((B, u)) for u in units[1:]], [np.zeros((B, u)) for u in units[1:]])


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
