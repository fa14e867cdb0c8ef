"""Host mirror of the sklearn-port MLP used by go-ctr's "simple 2-layer MLP" path.

Reference: nn/neural_network/multilayer_perceptron.go:9-134 (MLPRegressor, MLPClassifier, their constructors, Fit,
Predict, Score), nn/neural_network/basemlp64.go (hyper-parameters :25-51, defaults :228-254, init :408-482, Fit :578-599,
validateHyperparameters :625-673, scores :1116-1155, LabelBinarizer64 :1283-1375) and the adapters model/mlp/mlp.go:15-65
(SimpleMlpFitWrap / SimpleMlpPredWrap).  Arithmetic is float64 on the device (include/goctr.h, goctr_mlp_*); this file
keeps the reference's names, defaults and error behaviour and owns what is host-side in the reference too: the init RNG
(Q8: one-sided U[0,bound)), the per-epoch shuffle, the label binarizer and the two score rules.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi
from .recommend import Fitter, PredictAbstract, TrainSample

_ACT = {"identity": 0, "logistic": 1, "tanh": 2, "relu": 3}
_SOLVER = {"sgd": 0, "adam": 1}
_OUT = {"logistic": 0, "softmax": 1, "identity": 2}                 # include/goctr.h GOCTR_OUT_*
_LR = {"constant": 0, "invscaling": 1, "adaptive": 2}               # include/goctr.h GOCTR_LR_*


class LabelBinarizer64:
    """LabelBinarizer64 (basemlp64.go:1283-1375) with NegLabel 0, PosLabel 1, as BaseMultilayerPerceptron64.Fit builds it:
    each column's distinct values sorted ascending, one-hot over them (so one column holding two labels becomes two)."""

    def __init__(self, NegLabel=0.0, PosLabel=1.0):
        self.NegLabel, self.PosLabel = NegLabel, PosLabel
        self.Classes = []

    def Fit(self, Y):
        Y = np.asarray(Y, np.float64).reshape(len(Y), -1)
        self.Classes = [np.unique(Y[:, j]) for j in range(Y.shape[1])]
        return self

    def Transform(self, Y):
        Y = np.asarray(Y, np.float64).reshape(len(Y), -1)
        out = np.full((Y.shape[0], sum(len(c) for c in self.Classes)), self.NegLabel, np.float64)
        base = 0
        for j, cls in enumerate(self.Classes):
            k = np.searchsorted(cls, Y[:, j])
            hit = (k < len(cls)) & (cls[np.minimum(k, len(cls) - 1)] == Y[:, j])
            out[np.nonzero(hit)[0], base + k[hit]] = self.PosLabel
            base += len(cls)
        return out

    def FitTransform(self, Y):
        return self.Fit(Y).Transform(Y)

    def InverseTransform(self, Yb):
        """per original column: the class at MaxIdx64 (the first maximum) of its block of columns"""
        Yb = np.asarray(Yb, np.float64)
        out = np.empty((Yb.shape[0], len(self.Classes)), np.float64)
        base = 0
        for j, cls in enumerate(self.Classes):
            out[:, j] = cls[np.argmax(Yb[:, base:base + len(cls)], axis=1)]
            base += len(cls)
        return out


def r2Score64(yTrue, yPred):
    """r2Score64 (basemlp64.go:1116-1141): mean over the columns of 1 - sum (pred - true)^2 / sum (true - mean)^2"""
    yTrue = np.asarray(yTrue, np.float64).reshape(len(yTrue), -1)
    yPred = np.asarray(yPred, np.float64).reshape(yTrue.shape)
    acc = 0.0
    for c in range(yTrue.shape[1]):
        t = yTrue[:, c]
        avg = 0.0
        for v in t:                       # the reference's running sums, in row order
            avg += v
        avg /= len(t)
        num = den = 0.0
        for a, b in zip(yPred[:, c], t):
            num += (a - b) * (a - b)
            den += (b - avg) * (b - avg)
        if den == 0:
            raise ValueError("yDen=0")
        acc += 1 - num / den
    return acc / yTrue.shape[1]


def AccuracyScore64(Y, H):
    """AccuracyScore64 (basemlp64.go:1143-1155): the share of rows whose every column is EXACTLY equal"""
    Y = np.asarray(Y, np.float64).reshape(len(Y), -1)
    H = np.asarray(H, np.float64).reshape(Y.shape)
    return float(np.count_nonzero(np.all(H == Y, axis=1))) / Y.shape[0]


class _BaseMLP:
    """BaseMultilayerPerceptron64's exported fields and what Fit / Predict share on the device.

    Not supported, and refused with ValueError by Fit: Solver "lbfgs" (no device path); WarmStart (every Fit starts from a fresh
    initialisation and a fresh optimizer); EarlyStopping -- read literally, the reference scores a classifier's validation rows
    by exact equality between probabilities and 0/1 labels and, with BestValidationScore starting at 0, can end by copying
    never-written zero parameters back (basemlp64.go:852, :879-881, :933-942); whether to reproduce that is a separate decision."""

    OutActivation = "logistic"

    def __init__(self, hiddenLayerSizes, activation="relu", solver="adam", Alpha=1e-4):
        # NewBaseMultilayerPerceptron64 defaults (basemlp64.go:228-254)
        self.HiddenLayerSizes = list(hiddenLayerSizes)
        self.Activation, self.Solver, self.Alpha = activation, solver, Alpha
        self.BatchSize = 200
        self.LearningRate = "constant"      # "invscaling" (SGD only, like the reference) | "adaptive"
        self.LearningRateInit = 0.001
        self.PowerT = 0.5
        self.MaxIter = 200
        self.Shuffle = True
        self.RandomState = None          # numpy Generator; None => time-seeded like basemlp64.go:446-448
        self.Tol = 1e-4
        self.Verbose = False
        self.Momentum, self.NesterovsMomentum = 0.9, True
        self.Beta1, self.Beta2, self.Epsilon = 0.9, 0.999, 1e-8
        self.NIterNoChange = 10
        self.BatchNormalize = False
        self.WeightDecay = 0.0
        self.WarmStart = False
        self.EarlyStopping = False
        self.ValidationFraction = 0.1
        # fitted state
        self.LossCurve = []
        self.NIter = 0
        self._h = None
        self._units = None

    # validateHyperparameters (basemlp64.go:625-673) panics; here: ValueError
    def _validate(self):
        if self.Activation not in _ACT:
            raise ValueError(f"The activation {self.Activation} is not supported.")
        if self.Solver not in _SOLVER:
            raise ValueError(f"The solver {self.Solver} is not supported (lbfgs has no device path).")
        if self.Alpha < 0 or self.LearningRateInit <= 0 or self.MaxIter <= 0:
            raise ValueError("invalid hyper-parameters")
        if any(s <= 0 for s in self.HiddenLayerSizes):
            raise ValueError(f"hiddenLayerSizes must be > 0, got {self.HiddenLayerSizes}.")
        if self.LearningRate not in _LR:
            raise ValueError(f"learning rate {self.LearningRate} is not supported.")
        if self.EarlyStopping:
            raise ValueError("EarlyStopping is not supported (see the class docstring)")
        if self.WarmStart:
            raise ValueError("WarmStart is not supported: every Fit starts from a fresh initialisation")

    def _cfg(self, units, batch):
        c = capi.MlpCfg()
        capi.load().goctr_mlp_cfg_default(C.byref(c))
        c.n_layers = len(units)
        for i, u in enumerate(units):
            c.units[i] = u
        c.activation, c.solver, c.alpha = _ACT[self.Activation], _SOLVER[self.Solver], self.Alpha
        c.lr_init, c.beta1, c.beta2, c.eps = self.LearningRateInit, self.Beta1, self.Beta2, self.Epsilon
        c.momentum, c.nesterov = self.Momentum, int(self.NesterovsMomentum)
        c.batch_normalize, c.weight_decay = int(self.BatchNormalize), self.WeightDecay
        c.batch, c.max_iter, c.n_iter_no_change, c.tol = batch, self.MaxIter, self.NIterNoChange, self.Tol
        c.out_activation, c.lr_schedule, c.power_t = _OUT[self.OutActivation], _LR[self.LearningRate], self.PowerT
        return c

    def init_params(self, units, rng):
        """initialize (basemlp64.go:432-475): packed [b_i | W_i], each = U[0,1) * sqrt(f/(fanIn+fanOut)),
        f = 2 for logistic else 6 -- one-sided on purpose (quirk Q8)."""
        theta = []
        for i in range(len(units) - 1):
            fi, fo = units[i], units[i + 1]
            bound = math.sqrt((2.0 if self.Activation == "logistic" else 6.0) / (fi + fo))
            theta.append(rng.random(fo + fi * fo) * bound)
        return np.concatenate(theta)

    def create(self, units, batch, theta):
        capi.init()
        self.close()
        self._units = list(units)
        self._h = C.c_void_p()
        cfg = self._cfg(units, batch)
        capi.check(capi.load().goctr_mlp_create(C.byref(cfg), C.byref(self._h)))
        self.set_params(theta)

    def set_params(self, theta):
        theta = np.ascontiguousarray(theta, np.float64)
        capi.check(capi.load().goctr_mlp_set_params(self._h, capi.ptr(theta, C.c_double), C.c_size_t(theta.size)))

    def get_params(self):
        n = capi.load().goctr_mlp_nparams(self._h)
        theta = np.empty(n, np.float64)
        capi.check(capi.load().goctr_mlp_get_params(self._h, capi.ptr(theta, C.c_double), C.c_size_t(n)))
        return theta

    def loss_grad(self, X, Y):
        X = np.ascontiguousarray(X, np.float64)
        Y = np.ascontiguousarray(Y, np.float64).reshape(X.shape[0], -1)
        g = np.empty(capi.load().goctr_mlp_nparams(self._h), np.float64)
        loss = C.c_double(0)
        capi.check(capi.load().goctr_mlp_loss_grad(self._h, capi.ptr(X, C.c_double), capi.ptr(Y, C.c_double),
                                                   C.c_int(X.shape[0]), C.byref(loss), capi.ptr(g, C.c_double)))
        return loss.value, g

    def _fit(self, X, Y, theta0=None, perm=None):
        """fit :484 -> fitStochastic :729 on the device with self.OutActivation's head.  X float32 rows (the adapter
        widens them, mlp.go:46-53).  Every row is trained: a sample count that is not a multiple of the batch
        ends each epoch with one short batch, computed the reference's way (quirk Q11, basemlp64.go:790-812 -- its hidden
        block and output deltas keep the previous batch's rows beyond the short batch; csrc/mlp_api.hip goctr_mlp_fit_resident)."""
        self._validate()
        X = capi.f32(X)
        Y = capi.f32(Y).reshape(X.shape[0], -1)
        rng = self.RandomState or np.random.default_rng()
        units = [X.shape[1], *self.HiddenLayerSizes, Y.shape[1]]
        batch = min(self.BatchSize if self.BatchSize > 0 else 200, X.shape[0])     # basemlp64.go:516-527
        rows = X.shape[0]
        theta = theta0 if theta0 is not None else self.init_params(units, rng)
        self.create(units, batch, theta)
        if perm is None and self.Shuffle:
            # the reference shuffles X,Y in place every epoch (cumulative); equivalent index form
            order = np.arange(rows)
            perms = []
            for _ in range(self.MaxIter):
                order = order[rng.permutation(rows)]
                perms.append(order.copy())
            perm = np.stack(perms).astype(np.int32)
        curve = np.zeros(self.MaxIter, np.float64)
        ran = C.c_int(0)
        pp = np.ascontiguousarray(perm, np.int32) if perm is not None else None
        capi.check(capi.load().goctr_mlp_fit(self._h, capi.ptr(X, C.c_float), capi.ptr(Y, C.c_float), C.c_int64(rows),
                                             capi.ptr(pp, C.c_int32), capi.ptr(curve, C.c_double), C.byref(ran)))
        self._resident_rows = rows
        return self._fitted(curve, ran.value)

    def _fitted(self, curve, ran):
        self.NIter = ran
        self.LossCurve = curve[:ran].tolist()
        if self.Verbose:
            for i, l in enumerate(self.LossCurve):
                print("Iteration %d, loss = %.8f" % (i + 1, l))
        return self

    def FitResident(self, perm=None):
        """fitStochastic over the rows a previous upload() left in HBM (goctr_mlp_fit_resident: what Fit runs after its
        upload).  perm: [MaxIter][rows] int32 row order per epoch, or None = the given order every epoch."""
        curve = np.zeros(self.MaxIter, np.float64)
        ran = C.c_int(0)
        pp = np.ascontiguousarray(perm, np.int32) if perm is not None else None
        capi.check(capi.load().goctr_mlp_fit_resident(self._h, capi.ptr(pp, C.c_int32), capi.ptr(curve, C.c_double), C.byref(ran)))
        return self._fitted(curve, ran.value)

    def EvaluateResident(self):
        """the resident rows (upload) scored by predictProbas in float64 against the resident Y, on the device
        (goctr_mlp_evaluate_resident): a metrics.BinaryMetrics.  Single-output heads only."""
        from .metrics import BinaryMetrics
        out = capi.BinaryMetrics()
        capi.check(capi.load().goctr_mlp_evaluate_resident(self._h, C.byref(out)))
        return BinaryMetrics.from_c(out)

    def EvaluateResidentCurve(self, bins=10, threshold=0.5, points=0):
        """EvaluateResident's scores through the curve pipeline (goctr_mlp_evaluate_resident_curve): a metrics.CurveMetrics.
        Single-output heads only."""
        from .metrics import CurveCall
        call = CurveCall(bins, threshold, points)
        capi.check(capi.load().goctr_mlp_evaluate_resident_curve(self._h, *call.args()))
        return call.result()

    def EvaluateResidentGrouped(self, group, k=10, pooled=False):
        """EvaluateResident's scores grouped by group [resident rows] (goctr_mlp_evaluate_resident_grouped): a
        metrics.GroupMetrics, or (BinaryMetrics, GroupMetrics) with pooled=True.  Single-output heads only."""
        from .metrics import BinaryMetrics, GroupMetrics
        out, allm = capi.GroupMetrics(), capi.BinaryMetrics()
        g = np.ascontiguousarray(group, np.int32).ravel()
        rows = getattr(self, "_resident_rows", None)
        if rows is None:
            raise ValueError("EvaluateResidentGrouped: upload() the rows first (the group column is matched against them)")
        if g.size != rows:
            raise ValueError(f"{rows} resident rows but {g.size} group ids")
        capi.check(capi.load().goctr_mlp_evaluate_resident_grouped(self._h, capi.ptr(g, C.c_int32), C.c_int(k),
                                                                   C.byref(allm) if pooled else None, C.byref(out)))
        gm = GroupMetrics.from_c(out)
        return (BinaryMetrics.from_c(allm), gm) if pooled else gm

    def EvaluateResidentBootstrap(self, other=None, cluster=None, reps=False, **cfg):
        """EvaluateResident's scores (and those of `other`, a second model holding as many resident rows: a paired comparison)
        through the bootstrap (goctr_mlp_evaluate_resident_bootstrap): a metrics.BootstrapMetrics against THIS model's resident Y.
        cluster: the resample unit of every resident row, or None (rows are drawn).  ``cfg``: replicates, seed, level, chunk_rows,
        rep_tile.  Single-output heads only."""
        from .metrics import BootCall, cluster_ids
        call = BootCall(reps, **cfg)
        g = None
        if cluster is not None:
            rows = getattr(self, "_resident_rows", None)
            if rows is None:
                raise ValueError("EvaluateResidentBootstrap: upload() the rows first (the cluster column is matched against them)")
            g = cluster_ids(cluster, rows)
        capi.check(capi.load().goctr_mlp_evaluate_resident_bootstrap(self._h, other._h if other is not None else None,
                                                                     capi.ptr(g, C.c_int32), *call.args()))
        return call.result()

    def EvaluateResidentRegression(self):
        """every column of the head over the resident rows against the resident Y, on the device
        (goctr_mlp_evaluate_resident_regression): a metrics.RegressionMetrics.  Any head."""
        from . import metrics
        out = capi.RegressionMetrics()
        cols = np.zeros(self._units[-1], metrics.REGRESSION_COL_DTYPE)
        capi.check(capi.load().goctr_mlp_evaluate_resident_regression(self._h, C.byref(out),
                                                                      cols.ctypes.data_as(C.POINTER(capi.RegressionCol))))
        return metrics._regression_result(out, cols)

    def EvaluateResidentMulticlass(self, top_k=1, beta=1.0, ovr=False):
        """the head's probabilities over the resident rows against the first maximum of each resident Y row, on the device
        (goctr_mlp_evaluate_resident_multiclass): a metrics.MulticlassMetrics.  Heads with two output units at least."""
        from .metrics import MulticlassCall
        call = MulticlassCall(self._units[-1], top_k, beta, ovr)
        capi.check(capi.load().goctr_mlp_evaluate_resident_multiclass(self._h, *call.args()))
        return call.result()

    def _predict64(self, X):
        """predictProbas (basemlp64.go:897-913) in float64: the head's values"""
        X = capi.f32(X)
        y = np.empty((X.shape[0], self._units[-1]), np.float64)
        capi.check(capi.load().goctr_mlp_predict64(self._h, capi.ptr(X, C.c_float), C.c_int64(X.shape[0]),
                                                   capi.ptr(y, C.c_double)))
        return y

    def _predict32(self, X):
        X = capi.f32(X)
        no = self._units[-1]
        y = np.empty((X.shape[0], no), np.float32)
        capi.check(capi.load().goctr_mlp_predict(self._h, capi.ptr(X, C.c_float), C.c_int64(X.shape[0]),
                                                 capi.ptr(y, C.c_float)))
        return y

    def upload(self, X, Y):
        X = capi.f32(X)
        Y = capi.f32(Y).reshape(X.shape[0], -1)
        capi.check(capi.load().goctr_mlp_upload(self._h, capi.ptr(X, C.c_float), capi.ptr(Y, C.c_float),
                                                C.c_int64(X.shape[0])))
        self._resident_rows = X.shape[0]

    def train_steps(self, n_steps, first_batch=0):
        capi.check(capi.load().goctr_mlp_train_steps(self._h, C.c_int64(first_batch), C.c_int(n_steps)))

    def close(self):
        if self._h:
            capi.load().goctr_mlp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MLPClassifier(_BaseMLP):
    """nn.MLPClassifier (multilayer_perceptron.go:74-134) with BaseMultilayerPerceptron64's exported fields.

    The output head follows the reference's Fit (basemlp64.go:578-599, :503-511, initialize :416-429): targets that are all
    0 / 1 are trained as they are -- one column: logistic + binary_log_loss; more than one column: softmax + log_loss, since
    the reference's rule is isMulticlass = y.Cols > 1 (so 0 / 1 one-hot or multi-label targets select softmax too).  Any
    other target values are label-binarized first (LabelBinarizer64) and Predict maps the softmax (or logistic) outputs back
    to class labels by arg-max."""

    def __init__(self, hiddenLayerSizes, activation="relu", solver="adam", Alpha=1e-4):
        super().__init__(hiddenLayerSizes, activation, solver, Alpha)
        self.lb = None

    def Fit(self, X, Y, theta0=None, perm=None):
        """Base64.Fit (basemlp64.go:578-599) -> fit :484 -> fitStochastic :729 (theta0 / perm: a given initialisation and
        row order per epoch, [MaxIter][rows] int32)"""
        Y = np.asarray(Y, np.float32).reshape(np.asarray(X).shape[0], -1)
        self.lb = None
        if not np.all((Y == 0) | (Y == 1)):
            self.lb = LabelBinarizer64(0, 1)
            Y = self.lb.FitTransform(Y).astype(np.float32)
        self.OutActivation = "softmax" if Y.shape[1] > 1 else "logistic"
        return self._fit(X, Y, theta0, perm)

    def Predict(self, X):
        """predict (basemlp64.go:915-929): class labels (float64, one column per original target column) when Fit
        label-binarized the targets, else predictProbas' probabilities, float32 like mlp.go:33-38"""
        if self.lb is not None:
            return self.lb.InverseTransform(self._predict64(X))
        return self._predict32(X)

    def Score(self, X, Y):
        """MLPClassifier.Score (multilayer_perceptron.go:126-134): AccuracyScore64 of Predict against Y.  Quirk kept: for 0 / 1
        targets Predict returns probabilities, never thresholded, so a row only counts when its probabilities equal its
        labels exactly (the reference compares the same way)."""
        Y = np.asarray(Y, np.float64).reshape(np.asarray(X).shape[0], -1)
        H = self.lb.InverseTransform(self._predict64(X)) if self.lb is not None else self._predict64(X)
        return AccuracyScore64(Y, H)

    def ScoreResident(self):
        """Score over the rows Fit left resident, without a download: the arg-max accuracy
        (goctr_mlp_evaluate_resident_multiclass) when Fit label-binarized ONE target column into two classes at least.  Otherwise
        ValueError: on 0 / 1 targets the reference's rule is exact equality between probabilities and labels, which has no meaning
        on this path -- use EvaluateResidentMulticlass (or EvaluateResident for the logistic head)."""
        if self.lb is None or len(self.lb.Classes) != 1 or self._units[-1] < 2:
            raise ValueError("ScoreResident needs one label-binarized target column; use EvaluateResidentMulticlass")
        return self.EvaluateResidentMulticlass().conf.accuracy


class MLPRegressor(_BaseMLP):
    """nn.MLPRegressor (multilayer_perceptron.go:9-71): identity output + square_loss, float64 predictions, Score = r2Score64.
    (The reference's fit picks the head from the target values, basemlp64.go:503-511, so a regressor handed only 0 / 1
    targets would train a logistic head; this one always trains the identity head MLPRegressor stands for.)"""

    OutActivation = "identity"

    def Fit(self, X, Y, theta0=None, perm=None):
        return self._fit(X, Y, theta0, perm)

    def Predict(self, X):
        return self._predict64(X)

    def Score(self, X, Y):
        return r2Score64(np.asarray(Y, np.float64).reshape(np.asarray(X).shape[0], -1), self.Predict(X))

    def ScoreResident(self):
        """r2Score64 over the rows Fit left resident, from the device's column sums (goctr_mlp_evaluate_resident_regression:
        r2_mlp_uniform); ValueError("yDen=0") when a column is constant, as r2Score64"""
        m = self.EvaluateResidentRegression()
        if m.constant_columns:
            raise ValueError("yDen=0")
        return m.r2_mlp_uniform


def NewMLPRegressor(hiddenLayerSizes, activation, solver, Alpha):
    """multilayer_perceptron.go:19-28"""
    return MLPRegressor(hiddenLayerSizes, activation, solver, Alpha)


def NewMLPClassifier(hiddenLayerSizes, activation, solver, Alpha):
    """multilayer_perceptron.go:81-90"""
    return MLPClassifier(hiddenLayerSizes, activation, solver, Alpha)


class SimpleMlpPredWrap(PredictAbstract):
    """model/mlp/mlp.go:11-39"""

    def __init__(self, pred: MLPClassifier):
        self.pred = pred

    def Predict(self, X):
        return self.pred.Predict(X)


class SimpleMlpFitWrap(Fitter):
    """model/mlp/mlp.go:41-65"""

    def __init__(self, Model: MLPClassifier):
        self.Model = Model

    def Fit(self, trainSample: TrainSample) -> PredictAbstract:
        X = np.asarray(trainSample.X, np.float32).reshape(trainSample.Rows, trainSample.XCols)
        self.Model.Fit(X, np.asarray(trainSample.Y, np.float32))
        return SimpleMlpPredWrap(self.Model)
