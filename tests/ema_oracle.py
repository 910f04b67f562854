"""Host oracle of the weight average (csrc/ema.hip; include/fmri_hip.h fmri_ema_update): a helper, not a test.

    decay_at     the decay of step t in Python floats: double quotient, one cast to fp32
    update       one step in numpy fp32, op by op, in the kernel's order (no fused multiply-add)
    update_f64   the exact recurrence in float64, for the error bound
"""
import numpy as np


def decay_at(t: int, start: int, decay: float, warmup: bool) -> np.float32:
    d = np.float32(decay)
    if t < start:
        return np.float32(0.0)
    if not warmup:
        return d
    s = float(t) - float(start)
    w = np.float32((1.0 + s) / (10.0 + s))
    return w if w < d else d


def update(e: np.ndarray, w: np.ndarray, d) -> np.ndarray:
    """fp32: omd = 1 - d; e + omd * (w - e), every operation rounded to fp32."""
    e, w = np.asarray(e, dtype=np.float32), np.asarray(w, dtype=np.float32)
    omd = np.float32(1) - np.float32(d)
    with np.errstate(all="ignore"):
        diff = (w - e).astype(np.float32)
        prod = (omd * diff).astype(np.float32)
        return (e + prod).astype(np.float32)


def update_f64(e: np.ndarray, w: np.ndarray, d) -> np.ndarray:
    """The same step in float64 from float64 state.  The weight is the kernel's: omd = 1.0f - d is part of the formula
    (exact for d >= 0.5, one fp32 rounding below), everything behind it is exact to float64."""
    e, w = np.asarray(e, dtype=np.float64), np.asarray(w, dtype=np.float64)
    omd = float(np.float32(1) - np.float32(d))
    return e + omd * (w - e)
