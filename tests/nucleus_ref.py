"""numpy restatement of nucleus (top_p) truncation of the free-running decoder's pitch draw, beside top_k / min_p (tests/trunc_ref.py) and the
noise (tests/sample_ref.py): include/ptvae_hip.h "Sampled decode", csrc/philox.hpp pitch_keep_threshold().

The rule, exactly as on the device (T = T_pitch as fp32, q = top_p_q24 = round(top_p * 2^24) in [1, 2^24], 0 = off):
    m   = the row's largest logit
    x_c = fl(fl(logit_c - m) / T)                       two fp32 operations, each correctly rounded
    w_c = floor(exp(x_c) * 2^20)                        an integer in [0, 2^20]; the best class has exactly 2^20
    Z   = sum of w_c                                    < 2^28
    class c is kept iff  G_above(c) * 2^24 < Z * q      G_above(c) = sum of w over the classes with a logit strictly above logit_c
                                                        (-0.0 == +0.0); 64-bit integers
i.e. logit_c >= t, t the largest value with mass{logit >= t} * 2^24 >= Z * q -- the device finds it with the 32-round bitwise select of
top_k on the order-preserving key, the masses in place of the counts (nucleus_threshold_bitwise); nucleus_threshold_sorted is the
definition by sorting.  With top_k / min_p as well: the largest threshold.  T = 0: no nucleus rule.

The one thing numpy cannot restate is the device's exponential (__expf: v_exp_f32 of x * log2(e), both fp32); here exp is float64 of the
fp32 x.  E bounds |w_device - w_here| per class, in units of the integer mass (2^-20 of the best class's mass).  Derivation: w > 0 needs
|x| < 13.9; the fp32 product x * log2(e) and the rounded constant put a relative error <= |x| * 2^-24 * (1 + ...) on exp2, the hardware
exponential adds 1 ulp (2^-23 relative): with w <= 2^20 * exp(-|x|) that is < 0.2 units before the truncation, which can then flip the
integer: 1 unit.  E = 2 leaves a factor two.  A class c is IN THE BAND of its row iff
    | G_above(c) * 2^24 - Z * q |  <=  (n_above(c) + 130 * top_p) * E * 2^24
(n_above classes each off by <= E in G_above; 130 classes each off by <= E in Z, times q = top_p * 2^24): the device may keep or drop it.
The best class is never in the band (G_above = n_above = 0 and Z >= 2^20 > 130 E).  A decision is band-skippable iff the restated
decision differs between keeping and dropping the band classes of its row.
"""
import numpy as np

import sample_ref as S
import trunc_ref as TR

NP_ = 130
MASS_ONE = 1 << 20
Q_ONE = 1 << 24
E_UNITS = 2


def q24_of(top_p):
    """what the host stores: None / 1.0 -> 0 (off); else round(top_p * 2^24), never below 1"""
    if top_p is None or top_p == 1:
        return 0
    return min(max(int(np.floor(float(top_p) * Q_ONE + 0.5)), 1), Q_ONE)


def order_keys(logits):
    """the device's order-preserving uint32 key (-0.0 is +0.0)"""
    u = np.asarray(logits, dtype=np.float32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_values(key):
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32).view(np.float32)


def masses(logits, T):
    """int64 [..., 130]: the integer masses w_c"""
    a = np.asarray(logits, dtype=np.float32)
    with np.errstate(under='ignore'):
        x = ((a - a.max(-1, keepdims=True)).astype(np.float32) / np.float32(T)).astype(np.float32)
        return np.floor(np.exp(x.astype(np.float64)) * MASS_ONE).astype(np.int64)


def mass_above(logits, T):
    """(G_above int64 [..., 130], n_above int64 [..., 130], Z int64 [...]): mass and number of the classes strictly above each class"""
    a = np.asarray(logits, dtype=np.float32)
    w = masses(a, T)
    key = order_keys(a).astype(np.int64)
    order = np.argsort(-key, axis=-1, kind='stable')
    ks = np.take_along_axis(key, order, -1)
    ws = np.take_along_axis(w, order, -1)
    excl = np.cumsum(ws, -1) - ws                                                          # mass before each sorted place
    idx = np.broadcast_to(np.arange(a.shape[-1]), a.shape)
    new = np.concatenate([np.ones(a.shape[:-1] + (1,), dtype=bool), ks[..., 1:] != ks[..., :-1]], -1)
    start = np.maximum.accumulate(np.where(new, idx, 0), axis=-1)                          # first place of the tie group
    g_sorted = np.take_along_axis(excl, start, -1)
    G = np.empty_like(w)
    n = np.empty_like(w)
    np.put_along_axis(G, order, g_sorted, -1)
    np.put_along_axis(n, order, start.astype(np.int64), -1)
    return G, n, w.sum(-1)


def nucleus_mask_sorted(logits, T, q):
    """bool [..., 130] by the definition: kept iff the mass strictly above is < top_p * Z"""
    G, _, Z = mass_above(logits, T)
    return G * Q_ONE < (Z * int(q))[..., None]


def nucleus_threshold_sorted(logits, T, q):
    """fp32 [...]: the smallest kept logit of the definition"""
    a = np.asarray(logits, dtype=np.float32)
    thr = np.where(nucleus_mask_sorted(a, T, q), a, np.float32(np.inf)).min(-1)
    return (thr + np.float32(0.0)).astype(np.float32)


def nucleus_threshold_bitwise(logits, T, q):
    """the same value by the device's method: 32 rounds, most significant bit first; a round keeps the bit iff
    mass{key >= candidate} * 2^24 >= Z * q"""
    a = np.asarray(logits, dtype=np.float32)
    key = order_keys(a)
    w = masses(a, T)
    need = w.sum(-1) * int(q)
    sel = np.zeros(key.shape[:-1], dtype=np.uint32)
    for b in range(31, -1, -1):
        cand = sel | np.uint32(1 << b)
        g = np.where(key >= cand[..., None], w, 0).sum(-1)
        sel = np.where(g * Q_ONE >= need, cand, sel).astype(np.uint32)
    return (key_values(sel) + np.float32(0.0)).astype(np.float32)


def threshold(logits, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """the row's keep threshold under all three rules, fp32 [...]; -inf: no rule"""
    a = np.asarray(logits, dtype=np.float32)
    thr = TR.threshold(a, T, top_k, ln_min_p)
    if q and float(np.float32(T)) > 0:
        thr = np.maximum(thr, nucleus_threshold_bitwise(a, T, q))
    return (thr + np.float32(0.0)).astype(np.float32)


def keep_mask(logits, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """bool [..., 130]: the classes the draw runs over"""
    a = np.asarray(logits, dtype=np.float32)
    return a >= threshold(a, T, top_k, ln_min_p, q)[..., None]


def decide_pitch(logits, noise, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0, keep=None):
    """first maximal index over the kept classes of logit + T * g (keep: another mask than keep_mask's)"""
    x = S.perturbed(logits, noise, T)
    keep = keep_mask(logits, T, top_k, ln_min_p, q) if keep is None else keep
    return np.argmax(np.where(keep, x, np.float32(-np.inf)), axis=-1)


def band_classes(logits, T, q, E=E_UNITS):
    """bool [..., 130]: the classes the device may keep or drop differently under the nucleus rule (module docstring)"""
    a = np.asarray(logits, dtype=np.float32)
    if not q or float(np.float32(T)) <= 0:
        return np.zeros(a.shape, dtype=bool)
    G, n, Z = mass_above(a, T)
    top_p = int(q) / Q_ONE
    return np.abs(G * Q_ONE - (Z * int(q))[..., None]) <= (n + NP_ * top_p) * (E * Q_ONE)


def band_skippable(logits, noise, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0, E=E_UNITS):
    """bool [...]: decisions that differ between keeping and dropping the band classes of their row (the other rules as they are)"""
    a = np.asarray(logits, dtype=np.float32)
    band = band_classes(a, T, q, E)
    if not band.any():
        return np.zeros(a.shape[:-1], dtype=bool)
    other = TR.keep_mask(a, T, top_k, ln_min_p)
    nuc = nucleus_mask_sorted(a, T, q)
    with_band = decide_pitch(a, noise, T, keep=other & (nuc | band))
    without = decide_pitch(a, noise, T, keep=other & nuc & ~band)
    return with_band != without


def crafted_rows():
    """64 hand-made 130-wide rows, float32 [64, 130]: the rows of tests/test_gpu_truncated_sampling.py re-created (ties straddling a rank,
    all-equal rows, the best value at the lane-layout seams, values differing in the last bit, +-0.0, spreads 0.03 / 1 / 30 -- at the
    widest and at a low T most masses truncate to 0), the last eight replaced by rows made for the nucleus rule: one dominant class,
    two equal halves, a geometric ladder and its tied form"""
    g = np.random.default_rng(21)
    base = lambda sd=0.03: (g.standard_normal(130) * sd).astype(np.float32)
    rows = []
    for k in (2, 9, 16, 17, 129):                                  # duplicates straddling the k-th place (ranks k - 1 .. k + 2 equal)
        for shift in (0, 1):
            r = base()
            order = np.argsort(-r, kind='stable')
            lo, hi = max(k - 2 + shift, 0), min(k + 2 + shift, 130)
            r[order[lo:hi]] = r[order[lo]]
            rows.append(r)
    for v in (0.5, 0.0, -0.0, -3.0):                               # all-equal rows
        rows.append(np.full(130, v, dtype=np.float32))
    for col in (129, 0, 128, 16, 63, 64):                          # the best value in the last / first column (and at lane-layout seams)
        r = base()
        r[col] = 1.0
        rows.append(r)
        r = base(1.0)
        r[col] = r.max() + np.float32(0.25)
        rows.append(r)
    one = np.float32(1.0)                                          # values differing in the last bit
    for step in (1, 2, 3):
        r = np.array([one + np.float32(i % (step + 1)) * np.spacing(one) for i in range(130)], dtype=np.float32)
        rows.append(g.permutation(r))
        rows.append(-g.permutation(r))
    for n_neg in (0, 3, 60):                                       # +-0.0 among a few other values
        r = np.where(g.integers(0, 2, 130) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        r[g.choice(130, n_neg, replace=False)] = -np.abs(base(1.0))[:n_neg]
        rows.append(r)
        r2 = r.copy()
        r2[g.choice(130, 4, replace=False)] = np.abs(base(1.0))[:4]
        rows.append(r2)
    while len(rows) < 56:                                          # plain rows of several spreads, some quantised (many ties)
        r = base((0.03, 1.0, 30.0)[len(rows) % 3])
        rows.append(np.round(r * 8) / 8 if len(rows) % 2 else r)
    for col in (0, 77, 129):                                       # one dominant class: every other mass truncates to 0 at a low T
        r = base()
        r[col] = 40.0
        rows.append(r)
    r = np.full(130, -1.0, dtype=np.float32)                       # two equal halves: the boundary of top_p = 0.5 inside a tie group
    r[g.permutation(130)[:65]] = 1.0
    rows.append(r)
    ladder = (-0.5 * np.arange(130)).astype(np.float32)            # a geometric ladder (each class e^-0.5 of the one above at T = 1)
    rows.append(g.permutation(ladder))
    rows.append(g.permutation(np.round(ladder / 2) * 2).astype(np.float32))               # ... in tied pairs
    r = base(1.0)                                                  # a tie group of five straddling the 0.5 boundary
    order = np.argsort(-r, kind='stable')
    r[order[3:8]] = r[order[3]]
    rows.append(r)
    r = base(3.0)
    r[order[:2]] = r.max()                                         # two classes tied for best
    rows.append(r)
    a = np.stack(rows).astype(np.float32)
    assert a.shape == (64, 130)
    return a
