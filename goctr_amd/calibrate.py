"""Isotonic score calibration over the device calls of include/goctr.h ("isotonic score calibration on the device").

``IsotonicCalibrator`` holds a goctr_calibrator: the weighted least-squares non-decreasing fit of labels against scores, as a table
of blocks (lo, hi, value, num, den, rows, pos), and maps scores through it.  The fit, the apply kernel and the calibrated predict /
evaluate paths run on the device; float32 arrays take the float32 ABI, anything else the float64 one.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .metrics import CurveCall, _abi, _score_label

STEP, LINEAR = capi.CALIB_STEP, capi.CALIB_LINEAR

BLOCK_DTYPE = np.dtype([("lo", np.float64), ("hi", np.float64), ("value", np.float64), ("num", np.uint64), ("den", np.uint64),
                        ("rows", np.int64), ("pos", np.int64)])
assert BLOCK_DTYPE.itemsize == C.sizeof(capi.CalibBlock)


def calib_cfg(w_pos=1, w_neg=1, interp=LINEAR, tile=0, clip_eps=0.0) -> capi.CalibCfg:
    return capi.default_calib_cfg(w_pos=int(w_pos), w_neg=int(w_neg), interp=int(interp), tile=int(tile), clip_eps=float(clip_eps))


class IsotonicCalibrator:
    """A fitted (or loaded) isotonic calibrator.  Build one with ``fit`` (host arrays), ``fit_dataset`` (a CTR net's scores of a
    resident dataset), ``fit_mlp`` (an MLP's resident rows) or ``from_dict`` (a saved table); ``apply`` maps scores."""

    def __init__(self, handle, cfg: capi.CalibCfg):
        self._h = handle
        self.cfg = cfg

    # ---- construction
    @classmethod
    def _made(cls, call, cfg):
        h = C.c_void_p()
        capi.check(call(C.byref(cfg), C.byref(h)))
        return cls(h, cfg)

    @classmethod
    def fit(cls, score, y, **cfg) -> "IsotonicCalibrator":
        """goctr_calibrator_fit / _f64 over host arrays score [n], y [n] (positive iff y > 0.5); cfg: calib_cfg's fields"""
        fn, ty, dt = _abi(score, "calibrator_fit")
        s, t = _score_label(score, y, dt)
        return cls._made(lambda c, h: fn(capi.ptr(s, ty), capi.ptr(t, ty), s.size, c, h), calib_cfg(**cfg))

    @classmethod
    def fit_dataset(cls, net, ds, batch, emb=None, **cfg) -> "IsotonicCalibrator":
        """model.predict_dataset's scores, left on the device, against the dataset's resident labels"""
        L = capi.load()
        return cls._made(lambda c, h: L.goctr_calibrator_fit_dataset(net._h, emb._h if emb else None, ds._h, C.c_int(batch), c, h),
                         calib_cfg(**cfg))

    @classmethod
    def fit_mlp(cls, mlp, **cfg) -> "IsotonicCalibrator":
        """an MLP's resident rows (upload): its float64 scores against the resident Y"""
        L = capi.load()
        return cls._made(lambda c, h: L.goctr_mlp_calibrator_fit_resident(mlp._h, c, h), calib_cfg(**cfg))

    @classmethod
    def from_blocks(cls, blocks, **cfg) -> "IsotonicCalibrator":
        """goctr_calibrator_create over a BLOCK_DTYPE array (what ``blocks`` returns)"""
        b = np.ascontiguousarray(blocks, BLOCK_DTYPE)
        L = capi.load()
        return cls._made(lambda c, h: L.goctr_calibrator_create(b.ctypes.data_as(C.POINTER(capi.CalibBlock)), b.size, c, h),
                         calib_cfg(**cfg))

    # ---- the table
    def info(self) -> dict:
        o = capi.CalibInfo()
        capi.check(capi.load().goctr_calibrator_info(self._h, C.byref(o)))
        return {f: int(getattr(o, f)) for f, _ in capi.CalibInfo._fields_}

    def blocks(self) -> np.ndarray:
        """the block table as a BLOCK_DTYPE array, lowest block first"""
        b = np.zeros(self.info()["blocks"], BLOCK_DTYPE)
        capi.check(capi.load().goctr_calibrator_export(self._h, b.ctypes.data_as(C.POINTER(capi.CalibBlock)), b.size))
        return b

    def to_dict(self) -> dict:
        """plain lists (JSON-safe but for infinite knots, which json writes as Infinity) of the table and the apply settings;
        doubles as their hex strings so that a round trip returns the same bits"""
        b = self.blocks()
        d = {f: [float(x).hex() for x in b[f]] for f in ("lo", "hi", "value")}
        d.update({f: [int(x) for x in b[f]] for f in ("num", "den", "rows", "pos")})
        d["cfg"] = {"w_pos": self.cfg.w_pos, "w_neg": self.cfg.w_neg, "interp": self.cfg.interp, "clip_eps": float(self.cfg.clip_eps).hex()}
        return d

    @classmethod
    def from_dict(cls, d) -> "IsotonicCalibrator":
        b = np.zeros(len(d["lo"]), BLOCK_DTYPE)
        for f in ("lo", "hi", "value"):
            b[f] = [float.fromhex(x) for x in d[f]]
        for f in ("num", "den", "rows", "pos"):
            b[f] = d[f]
        c = d.get("cfg", {})
        return cls.from_blocks(b, w_pos=c.get("w_pos", 1), w_neg=c.get("w_neg", 1), interp=c.get("interp", LINEAR),
                               clip_eps=float.fromhex(c.get("clip_eps", "0x0p+0")))

    # ---- use
    def apply(self, score) -> np.ndarray:
        """the calibrated scores, in the input's shape (goctr_calibrator_apply for float32, else _f64)"""
        fn, ty, dt = _abi(score, "calibrator_apply")
        s = np.ascontiguousarray(score, dt)
        out = np.empty_like(s)
        capi.check(fn(self._h, capi.ptr(s.ravel(), ty), s.size, capi.ptr(out.reshape(-1), ty)))
        return out

    def predict_dataset(self, net, ds, batch, emb=None) -> np.ndarray:
        """model.predict_dataset's scores through the calibrator on the device (goctr_predict_dataset_calibrated)"""
        y = np.zeros(ds.rows, np.float32)
        capi.check(capi.load().goctr_predict_dataset_calibrated(net._h, emb._h if emb else None, ds._h, C.c_int(batch), self._h,
                                                                capi.ptr(y, C.c_float)))
        return y

    def evaluate_dataset_curve(self, net, ds, batch, emb=None, bins=10, threshold=0.5, points=0):
        """model.evaluate_dataset_curve over the calibrated scores (goctr_evaluate_dataset_curve_calibrated)"""
        call = CurveCall(bins, threshold, points)
        capi.check(capi.load().goctr_evaluate_dataset_curve_calibrated(net._h, emb._h if emb else None, ds._h, C.c_int(batch),
                                                                       self._h, *call.args()))
        return call.result()

    def evaluate_mlp_curve(self, mlp, bins=10, threshold=0.5, points=0):
        """MLP.EvaluateResidentCurve over the calibrated scores (goctr_mlp_evaluate_resident_curve_calibrated)"""
        call = CurveCall(bins, threshold, points)
        capi.check(capi.load().goctr_mlp_evaluate_resident_curve_calibrated(mlp._h, self._h, *call.args()))
        return call.result()

    def close(self):
        if self._h:
            capi.load().goctr_calibrator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
