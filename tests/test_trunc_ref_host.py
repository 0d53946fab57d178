"""CPU: the numpy restatement of truncated sampling (tests/trunc_ref.py) against brute force -- the GPU tests compare the kernels with it, so
it is checked on its own first.  No GPU, no library."""
import numpy as np

import sample_ref as S
import trunc_ref as TR

KS = (1, 2, 8, 40, 129, 130, 1000)


def rows(n=400, seed=3, sd=0.03):
    """130-wide rows of an untrained model's spread, a third of them quantised so that ties (also at the k-th place) are common"""
    g = np.random.default_rng(seed)
    a = (g.standard_normal((n, 130)) * sd).astype(np.float32)
    a[::3] = np.round(a[::3] * 64) / 64
    return a


def brute_mask(row, k):
    """ties at the k-th value included, by Python's own float comparison"""
    vals = sorted((float(x) for x in row), reverse=True)
    if k >= len(vals):
        return np.ones(len(vals), dtype=bool)
    return np.array([float(x) >= vals[k - 1] for x in row])


def test_top_k_mask_agrees_with_a_brute_force_sort_ties_included():
    a = rows()
    tied = 0
    for k in KS:
        m = TR.keep_mask(a, 1.0, k, TR.LN_MIN_P_OFF)
        for i in range(0, a.shape[0], 7):
            want = brute_mask(a[i], k)
            assert np.array_equal(m[i], want), (k, i)
            tied += int(k < 130 and want.sum() > k)
        assert (m.sum(-1) >= min(k, 130)).all()
    assert tied > 0                                                                        # (the quantised rows did tie at the k-th place)


def test_the_bitwise_select_equals_the_sorted_kth_value():
    """the device's method (32 rounds on the order-preserving key) restated: the same value as the sort for every row and k"""
    a = np.concatenate([rows(2000, seed=5), -rows(50, seed=6), np.zeros((1, 130), np.float32),
                        np.where(np.arange(130) % 2, np.float32(-0.0), np.float32(0.0))[None].astype(np.float32)])
    for k in (1, 2, 8, 40, 129, 130):
        got, want = TR.kth_largest_bitwise(a, k), TR.kth_largest(a, k)
        assert np.array_equal(got, want), k                                                # (value equality: -0.0 == +0.0)
        assert not np.signbit(got[got == 0]).any()                                         # ... and the select's zero is +0.0


def test_min_p_mask_is_the_probability_rule():
    a = rows(200, seed=9, sd=1.5)
    for T in (0.5, 1.0, 2.0):
        for min_p in (1.0, 0.5, 0.05, 1e-6):
            l = TR.ln_min_p_of(min_p)
            m = TR.keep_mask(a, T, None, l)
            amb = TR.band_classes(a, T, l)
            p = np.exp((a.astype(np.float64) - a.max(-1, keepdims=True)) / T)             # p_c / p_max
            want = p >= min_p
            assert np.array_equal(m[~amb], want[~amb]), (T, min_p)
            assert (amb & (a < a.max(-1, keepdims=True))).mean() < 1e-3                   # (min_p = 1 puts the best class itself on the threshold)


def test_kept_set_grows_in_k_and_shrinks_in_min_p():
    a = rows()
    prev = np.zeros(a.shape, dtype=bool)
    for k in KS:
        m = TR.keep_mask(a, 1.0, k, TR.LN_MIN_P_OFF)
        assert (m | ~prev).all()
        prev = m
    assert prev.all()
    prev = np.ones(a.shape, dtype=bool)
    for min_p in (None, 0.0, 1e-6, 0.5, 0.9, 0.99, 1.0):
        m = TR.keep_mask(a, 0.05, None, TR.ln_min_p_of(min_p))
        assert (prev | ~m).all()
        prev = m
    # both rules: the intersection
    both = TR.keep_mask(a, 0.05, 8, TR.ln_min_p_of(0.5))
    assert np.array_equal(both, TR.keep_mask(a, 0.05, 8, TR.LN_MIN_P_OFF) & TR.keep_mask(a, 0.05, None, TR.ln_min_p_of(0.5)))


def test_top_k_130_without_min_p_is_the_plain_draw():
    a = rows(64)
    noise = S.pitch_noise(11, 4, np.arange(64), 3, 5)
    for k in (130, 1000):
        assert np.array_equal(TR.decide_pitch_trunc(a, noise, 1.0, k, TR.LN_MIN_P_OFF), S.decide_pitch(a, noise, 1.0))
    assert (TR.decide_pitch_trunc(a, noise, 1.0, 2, TR.LN_MIN_P_OFF) != S.decide_pitch(a, noise, 1.0)).any()
    # T = 0: the plain argmax under any truncation
    for k, mp in ((1, None), (8, 0.5), (None, 1.0)):
        assert np.array_equal(TR.decide_pitch_trunc(a, noise, 0.0, k, TR.ln_min_p_of(mp)), a.argmax(-1))


def test_the_best_class_is_always_kept_and_the_decision_is_a_kept_class():
    a = rows()
    noise = S.pitch_noise(1, 0, np.arange(a.shape[0]), 0, 0)
    best = a.argmax(-1)
    for k in (None,) + KS:
        for mp in (None, 1.0, 0.5, 1e-6):
            if k is None and mp is None:
                continue
            l = TR.ln_min_p_of(mp)
            m = TR.keep_mask(a, 0.7, k, l)
            assert m[np.arange(a.shape[0]), best].all()
            d = TR.decide_pitch_trunc(a, noise, 0.7, k, l)
            assert m[np.arange(a.shape[0]), d].all()
    only = TR.keep_mask(a, 0.7, None, TR.ln_min_p_of(1.0))                                # min_p = 1: the classes tied for best
    assert np.array_equal(only, a == a.max(-1, keepdims=True))


def test_signed_zeros_compare_equal_and_an_all_equal_row_keeps_everything():
    z = np.where(np.arange(130) % 2, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    z[5], z[6] = -1.0, -2.0
    for k in (1, 2, 64, 128):
        m = TR.keep_mask(z, 1.0, k, TR.LN_MIN_P_OFF)
        assert m.sum() == 128 and not m[5] and not m[6]                                    # 128 zeros of either sign tie at the k-th place
        assert TR.threshold(z, 1.0, k, TR.LN_MIN_P_OFF).view(np.uint32) == 0               # +0.0
    assert TR.keep_mask(z, 1.0, 129, TR.LN_MIN_P_OFF).sum() == 129
    assert TR.keep_mask(z, 1.0, None, TR.ln_min_p_of(1.0)).sum() == 128
    for v in (0.0, -0.0, 3.25, -7.5):
        e = np.full(130, v, dtype=np.float32)
        for k, mp in ((1, None), (17, None), (None, 1.0), (3, 0.5)):
            assert TR.keep_mask(e, 1.0, k, TR.ln_min_p_of(mp)).all()
