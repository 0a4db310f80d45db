"""The scale rule of the FP8 K / V cache's calibration (include/ivg.h ivg_kv_calibration_finish), restated for tests/test_kv_scales_cpu.py
and tests/test_gpu_kv_scales.py.  No GPU import.

amax is the largest |x| a (layer, tensor, head) showed, a bf16 value.  With amax = m 2^e, m in [0.5, 1) (frexp):
    p = e - 9 if m <= 0.875 else e - 8          (448 = 0.875 * 2^9: 2^p is the smallest power of two s with amax / s <= 448)
    scale = 2^clamp(p + headroom, -126, 126),   amax = 0 -> 1.0
Integer arithmetic on the exponent, no logarithm: nothing rounds.  A NaN or Inf amax has no scale (ValueError here, IVG_ERR_INVALID there).
"""
import math

import numpy as np

E4M3_MAX = 448.0
HEADROOM_DEFAULT = 1


def scale_from_amax(amax, headroom=0):
    """float or array of non-negative finite fp32 values -> the scale(s), as Python float / float32 array of the same shape."""
    if isinstance(amax, (int, float)):
        a = float(np.float32(amax))
        if not (math.isfinite(a) and a >= 0.0):
            raise ValueError(f"amax must be finite and non-negative, not {amax!r}")
        if a == 0.0:
            return 1.0
        m, e = math.frexp(a)
        p = (e - 9 if m <= 0.875 else e - 8) + int(headroom)
        return 2.0 ** min(126, max(-126, p))
    arr = np.asarray(amax, dtype=np.float32)
    out = np.array([scale_from_amax(float(x), headroom) for x in arr.reshape(-1)], dtype=np.float32)
    return out.reshape(arr.shape)


def brute_force_scale(amax, headroom=0):
    """the same by search: the smallest 2^k, k in [-200, 200], with amax / 2^k <= 448, times 2^headroom, clamped (float64: the divisions
    by powers of two are exact)."""
    a = float(np.float32(amax))
    if a == 0.0:
        return 1.0
    k = next(k for k in range(-200, 201) if a / 2.0 ** k <= E4M3_MAX)
    return 2.0 ** min(126, max(-126, k + int(headroom)))
