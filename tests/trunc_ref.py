"""numpy restatement of truncated sampling (top_k / min_p) of the free-running decoder's pitch draw: include/ptvae_hip.h "Sampled decode",
csrc/philox.hpp pitch_keep_threshold().  The noise and `perturbed` are sample_ref's; everything here is fp32 as on the device.

  top_k:    class c is kept iff logit[c] >= v_k, the k-th largest of the row counted with multiplicity (ties with it all kept); k >= 130 or
            0 / None: no rule
  ln_min_p: class c is kept iff logit[c] >= fl(m + fl(T * ln_min_p)), m the row's maximum; any value > 0 (LN_MIN_P_OFF): no rule
  both:     the larger threshold.  No rule: the threshold is -inf.  A zero threshold is +0.0 (-0.0 == +0.0 in every comparison).
"""
import math

import numpy as np

import sample_ref as S

NP_ = 130
LN_MIN_P_OFF = np.float32(1.0)


def ln_min_p_of(min_p):
    """what the host stores: ln(min_p) in float64 rounded to fp32; None / 0 -> the off sentinel"""
    if min_p is None or min_p == 0:
        return LN_MIN_P_OFF
    return np.float32(math.log(float(min_p)))


def kth_largest(logits, k):
    """the k-th largest value of every row, by sorting: fp32 [...]"""
    a = np.asarray(logits, dtype=np.float32)
    return np.sort(a, axis=-1)[..., a.shape[-1] - k]


def kth_largest_bitwise(logits, k):
    """the same value by the device's method: a 32-round select on the order-preserving integer key, most significant bit first"""
    u = np.asarray(logits, dtype=np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0                                                     # -0.0 is +0.0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    sel = np.zeros(key.shape[:-1], dtype=np.uint32)
    for b in range(31, -1, -1):
        cand = sel | np.uint32(1 << b)
        sel = np.where((key >= cand[..., None]).sum(-1) >= k, cand, sel).astype(np.uint32)
    back = np.where(sel & np.uint32(0x80000000), sel & np.uint32(0x7FFFFFFF), ~sel).astype(np.uint32)
    return back.view(np.float32)


def threshold(logits, T, top_k, ln_min_p):
    """the row's keep threshold, fp32 [...]"""
    a = np.asarray(logits, dtype=np.float32)
    thr = np.full(a.shape[:-1], -np.inf, dtype=np.float32)
    if top_k and top_k < a.shape[-1]:
        thr = kth_largest(a, top_k)
    l = np.float32(ln_min_p)
    if l <= 0:
        with np.errstate(invalid='ignore'):
            thr = np.maximum(thr, (a.max(-1) + (np.float32(T) * l).astype(np.float32)).astype(np.float32))
    return (thr + np.float32(0.0)).astype(np.float32)


def keep_mask(logits, T, top_k, ln_min_p):
    """bool [..., 130]: the classes the draw runs over"""
    a = np.asarray(logits, dtype=np.float32)
    return a >= threshold(a, T, top_k, ln_min_p)[..., None]


def decide_pitch_trunc(logits, noise, T, top_k, ln_min_p):
    """first maximal index over the KEPT classes of logit + T * g"""
    x = S.perturbed(logits, noise, T)
    return np.argmax(np.where(keep_mask(logits, T, top_k, ln_min_p), x, np.float32(-np.inf)), axis=-1)


def band_classes(logits, T, ln_min_p, ulps=4):
    """bool [..., 130]: the classes within `ulps` ulp of the row's largest logit from the min_p threshold -- a device that fused
    m + T * ln_min_p into one rounding could keep or drop them differently.  (top_k compares emitted values exactly: no band.)"""
    a = np.asarray(logits, dtype=np.float32)
    if np.float32(ln_min_p) > 0:
        return np.zeros(a.shape, dtype=bool)
    m = a.max(-1)
    thr = m.astype(np.float64) + float(T) * float(np.float32(ln_min_p))
    band = ulps * np.spacing(np.abs(m)).astype(np.float64)
    return np.abs(a.astype(np.float64) - thr[..., None]) <= band[..., None]


def threshold_ambiguous(logits, T, ln_min_p, ulps=4):
    """bool [...]: rows with a class inside the band"""
    return band_classes(logits, T, ln_min_p, ulps).any(-1)
