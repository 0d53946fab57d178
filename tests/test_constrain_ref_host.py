"""CPU: tests/constrain_ref.py (the numpy restatement of the constrained decode) against brute force on small rows -- the allowed set of
the mask and of `lo`, constraints-first thresholds, the kept set never empty, the constrained draw's frequencies against the renormalised
restricted softmax, the mask builder's rule and the running `lo`."""
import math

import numpy as np

import constrain_ref as CR
import nucleus_ref as NR
import sample_ref as S
import trunc_ref as TR

# upper 0.1 % points of chi-square, by degrees of freedom (tables): a fixed seed either passes or fails, the level says how surprising
# a failure of a correct rule would have been
CHI2_999 = {1: 10.83, 2: 13.82, 3: 16.27, 4: 18.47, 5: 20.52, 6: 22.46, 7: 24.32, 8: 26.12, 9: 27.88, 10: 29.59, 11: 31.26, 12: 32.91}


def some_masks(g, n):
    """n mask rows int32 [n, 4]: empty, full, single bits at the word seams, then random ones of several densities"""
    rows = [np.zeros(4, dtype=np.int32), CR.FULL_MASK.copy()]
    for p in (0, 15, 16, 31, 32, 63, 64, 127):
        bits = np.zeros(128, dtype=bool)
        bits[p] = True
        rows.append(CR.mask_from_bits(bits))
    while len(rows) < n:
        rows.append(CR.mask_from_bits(g.random(128) < (0.03, 0.3, 0.9)[len(rows) % 3]))
    return np.stack(rows[:n])


def test_mask_bits_round_trip_and_bit_order():
    g = np.random.default_rng(1)
    bits = g.random((7, 128)) < 0.4
    m = CR.mask_from_bits(bits)
    assert m.dtype == np.int32 and m.shape == (7, 4)
    assert np.array_equal(CR.mask_bits(m), bits)
    one = np.zeros(128, dtype=bool)
    one[37] = True                                                   # bit 37 & 31 = 5 of word 37 >> 5 = 1
    assert CR.mask_from_bits(one).tolist() == [0, 1 << 5, 0, 0]
    one[:] = False
    one[127] = True                                                  # the sign bit of the last word
    assert CR.mask_from_bits(one).tolist() == [0, 0, 0, -(1 << 31)]


def test_allowed_set_is_the_definition():
    g = np.random.default_rng(2)
    masks = some_masks(g, 24)
    for asc in (False, True):
        for lo in (-1, 0, 62, 63, 64, 126, 127):
            got = CR.allowed(masks, np.full(len(masks), lo), asc)
            for r in range(len(masks)):
                assert got[r].tolist() == CR.allowed_brute(masks[r], lo, asc), (asc, lo, r)
            nomask = CR.allowed(None, np.array([lo]), asc)
            assert nomask[0].tolist() == CR.allowed_brute(None, lo, asc)
    al = CR.allowed(masks, np.full(len(masks), 127), True)
    assert al[:, CR.EOS].all() and not al[:, :129].any()             # pitches exhausted: the step can only end
    assert CR.allowed(np.zeros((1, 4), dtype=np.int32))[0].tolist() == [False] * 128 + [True, True]   # the mask does not cover 128 / 129
    assert not CR.allowed(None, np.array([-1]), True)[0, CR.SOS]      # ascending: never <sos>
    assert CR.allowed(CR.FULL_MASK[None]).all()


def brute_threshold(row, al, T, k, l, q):
    sub = row[al]
    thr = np.float32(-np.inf)
    if k and k < 130 and k <= len(sub):
        thr = np.sort(sub)[len(sub) - k]
    if q and T > 0:
        thr = max(thr, NR.nucleus_threshold_sorted(sub[None], T, q)[0])
    if l <= 0:
        thr = max(thr, np.float32(sub.max() + np.float32(np.float32(T) * np.float32(l))))
    return np.float32(thr + np.float32(0.0))


def test_constraints_come_first_in_every_threshold():
    """the threshold of the constrained row is the threshold of the compacted row of allowed classes: the k best ALLOWED classes, the
    mass and maximum of the allowed classes; fewer than k allowed -> all of them"""
    g = np.random.default_rng(3)
    masks = some_masks(g, 32)
    T = 0.7
    for sd in (0.03, 1.0):
        a = (g.standard_normal((32, 130)) * sd).astype(np.float32)
        a[5] = 0.25                                                  # all equal
        a[6, a[6].argmax()] += 1                                     # (row 6 / 7: a clear best, disallowed or not by the mask below)
        for asc, lo in ((False, -1), (True, -1), (True, 63), (True, 127)):
            al = CR.allowed(masks, np.full(32, lo), asc)
            for k, mp, p in ((None, None, None), (1, None, None), (8, None, None), (129, None, None), (None, 0.5, None), (None, None, 0.9),
                             (8, None, 0.9), (3, 0.5, 0.5)):
                l, q = TR.ln_min_p_of(mp), NR.q24_of(p)
                thr = CR.threshold(a, al, T, k, l, q)
                keep = CR.keep_mask(a, al, T, k, l, q)
                for r in range(32):
                    want = brute_threshold(a[r], al[r], T, k, l, q)
                    assert thr[r].view(np.uint32) == want.view(np.uint32), (sd, asc, lo, k, mp, p, r, thr[r], want)
                    assert keep[r].tolist() == [bool(al[r, c]) and a[r, c] >= want for c in range(130)]
                assert keep.any(-1).all()                            # never empty
                best_allowed = np.where(al, a, -np.inf).argmax(-1)
                assert keep[np.arange(32), best_allowed].all()       # the best allowed class passes every rule
                assert not (keep & ~al).any()


def test_kept_set_never_empty_in_the_corners():
    a = np.zeros((3, 130), dtype=np.float32)
    a[1, :128] = 50.0                                                # every pitch far above <eos>
    a[2] = -np.arange(130, dtype=np.float32)
    empty = np.zeros((3, 4), dtype=np.int32)
    for asc, lo in ((False, -1), (True, 127), (True, 0)):
        for k, mp, p in ((None, None, None), (1, 1.0, 0.01), (129, None, None)):
            keep = CR.keep_mask(a, CR.allowed(empty, np.full(3, lo), asc), 1.0, k, TR.ln_min_p_of(mp), NR.q24_of(p))
            assert keep.any(-1).all() and keep[:, CR.EOS].any()
    al = CR.allowed(empty, np.full(3, 127), True)
    assert (CR.decide_pitch(a, np.zeros_like(a), al, 1.0) == CR.EOS).all()


def test_constrained_draw_is_the_renormalised_restricted_softmax():
    """chi-square of the decisions over 40,000 noise draws (sample_ref's Philox noise of 40,000 global samples) against
    softmax(logits / T) renormalised over the allowed-and-kept classes, at the 0.1 % level; no decision leaves that set"""
    N = 40000
    g = np.random.default_rng(5)
    row = (g.standard_normal(130) * 0.8).astype(np.float32)
    noise = S.pitch_noise(11, 4, np.arange(N), 3, 2)
    bits = np.zeros(128, dtype=bool)
    bits[[40, 43, 47, 52, 55, 59, 64, 67, 71, 76]] = True
    mask = CR.mask_from_bits(bits)
    for T, asc, lo, k, p in ((1.0, False, -1, None, None), (1.0, True, 47, None, None), (0.6, True, 43, 5, None), (1.0, False, -1, 8, 0.9)):
        al = CR.allowed(mask[None], np.array([lo]), asc)[0]
        l, q = TR.LN_MIN_P_OFF, NR.q24_of(p)
        keep = CR.keep_mask(row, al, T, k, l, q)
        dec = CR.decide_pitch(np.broadcast_to(row, (N, 130)), noise, np.broadcast_to(al, (N, 130)), T, k, l, q)
        cls = np.flatnonzero(keep)
        assert 2 <= len(cls) <= 13 and np.isin(dec, cls).all()
        pr = np.exp(row[cls].astype(np.float64) / T)
        pr /= pr.sum()
        obs = np.array([(dec == c).sum() for c in cls], dtype=np.float64)
        assert (N * pr).min() > 5
        chi2 = ((obs - N * pr) ** 2 / (N * pr)).sum()
        print('T %.1f ascending %s lo %d top_k %s top_p %s: %d classes, chi2 %.2f (0.1 %% point %.2f)'
              % (T, asc, lo, k, p, len(cls), chi2, CHI2_999[len(cls) - 1]))
        assert chi2 < CHI2_999[len(cls) - 1]


def test_temperature_zero_is_the_constrained_argmax():
    g = np.random.default_rng(6)
    a = (g.standard_normal((16, 130))).astype(np.float32)
    a[3, 7] = a[3, 90] = a[3].max() + 1                              # a tie: the first allowed maximal index
    masks = some_masks(g, 16)
    masks[3] = CR.mask_from_bits(np.arange(128) >= 8)
    al = CR.allowed(masks, np.full(16, 5), True)
    noise = S.pitch_noise(1, 2, np.arange(16), 0, 0)
    dec = CR.decide_pitch(a, noise, al, 0.0)
    for r in range(16):
        best, bi = -math.inf, None
        for c in range(130):
            if al[r, c] and a[r, c] > best:
                best, bi = a[r, c], c
        assert dec[r] == bi
    assert dec[3] == 90


def test_running_lo():
    p = np.array([[60, 64, 129, 10, 128, 70, 3], [129, 129, 5, 5, 4, 127, 0]])
    want = []
    for row in p:
        lo, out = -1, []
        for v in row:
            out.append(lo)
            if v < 128:
                lo = max(lo, int(v))
        want.append(out)
    assert CR.running_lo(p).tolist() == want


def test_mask_builder_rule():
    g = np.random.default_rng(7)
    B = 3
    c = np.zeros((B, 8, 36), dtype=np.float32)
    c[:, :, 12:24] = (g.random((B, 8, 12)) < 0.3) * g.choice([1.0, -2.0, 0.5], (B, 8, 12))   # any non-zero value counts
    c[:, :, :12] = 1.0                                                                      # root / bass parts are not read
    for kw in (dict(), dict(c=c), dict(pitch_classes=0b101010110101), dict(lo=36, hi=84), dict(c=c, pitch_classes=0b000010010001, lo=1, hi=126),
               dict(pitch_classes=0), dict(lo=127, hi=127)):
        m = CR.mask_build(B, **kw)
        assert m.shape == (B, 32, 4) and m.dtype == np.int32
        bits = CR.mask_bits(m)
        pcs, lo, hi = kw.get('pitch_classes', 0xFFF), kw.get('lo', 0), kw.get('hi', 127)
        for b in range(B):
            for t in range(32):
                for p in range(128):
                    ok = lo <= p <= hi and bool(pcs >> (p % 12) & 1)
                    if 'c' in kw:
                        ok = ok and c[b, t // 4, 12 + p % 12] != 0
                    assert bits[b, t, p] == ok, (kw.keys(), b, t, p)
    assert np.array_equal(CR.mask_build(2), np.broadcast_to(CR.FULL_MASK, (2, 32, 4)))
