"""CPU: the numpy restatement of nucleus (top_p) truncation (tests/nucleus_ref.py) against its own definition by sorting and against float64
masses, and the host side of the keyword (validation, block words) -- the GPU tests compare the kernels with the restatement, so it is
checked on its own first.  No GPU, no library."""
import math
import struct

import numpy as np
import pytest

import nucleus_ref as NR
import sample_ref as S
import trunc_ref as TR
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M

TS = (0.05, 0.7, 1.0, 4.0)
TOP_PS = (2.0 ** -24, 0.1, 0.5, 0.9, 1 - 2.0 ** -24)


def rows():
    """the crafted rows plus plain ones of spread 0.03 / 1 / 30, a third quantised (ties at the boundary are common)"""
    g = np.random.default_rng(8)
    out = [NR.crafted_rows()]
    for sd in (0.03, 1.0, 30.0):
        a = (g.standard_normal((150, 130)) * sd).astype(np.float32)
        a[::3] = (np.round(a[::3] / sd * 4) / 4 * sd).astype(np.float32)
        out.append(a)
    return np.concatenate(out)


def test_the_bitwise_select_equals_the_sort_definition():
    """every row, T and top_p: the threshold of the 32-round select on integer masses is the smallest kept logit of the definition (mass
    strictly above < top_p * Z), the masks are equal, the best class is kept, the select's zero is +0.0"""
    a = rows()
    seen_tail0 = seen_tie = 0
    for T in TS:
        w = NR.masses(a, T)
        assert (w.max(-1) == NR.MASS_ONE).all() and (w >= 0).all() and (w.sum(-1) < 1 << 28).all()
        seen_tail0 += int((w == 0).any(-1).sum())
        for p in TOP_PS:
            q = NR.q24_of(p)
            assert 1 <= q <= NR.Q_ONE
            tb, ts = NR.nucleus_threshold_bitwise(a, T, q), NR.nucleus_threshold_sorted(a, T, q)
            assert np.array_equal(tb.view(np.uint32), ts.view(np.uint32)), (T, p, np.argwhere(tb != ts)[:4])
            assert not np.signbit(tb[tb == 0]).any()
            keep = NR.keep_mask(a, T, q=q)
            assert np.array_equal(keep, NR.nucleus_mask_sorted(a, T, q)), (T, p)
            assert keep[np.arange(a.shape[0]), a.argmax(-1)].all()
            assert (np.take_along_axis(a, a.argmax(-1)[:, None], -1)[:, 0] >= tb).all()
            # a tie group is kept or dropped as a whole
            srt = np.sort(a, -1)
            n_keep = keep.sum(-1)
            inside = (n_keep < 130) & (n_keep > 1)
            seen_tie += int((srt[inside, 130 - n_keep[inside]] == srt[inside, 130 - n_keep[inside] + 1]).sum())
            assert (srt[n_keep < 130, 129 - n_keep[n_keep < 130]] < tb[n_keep < 130]).all()
    assert seen_tail0 > 0 and seen_tie > 0                                                 # (tails that truncate to 0, ties at the boundary: both occurred)


def test_hand_worked_rows():
    # two equal halves at T = 1: 65 classes of mass 2^20, 65 of floor(e^-2 * 2^20); top_p = 0.5 is reached inside the upper tie group
    a = NR.crafted_rows()[59]
    assert (a == 1).sum() == 65 and (a == -1).sum() == 65
    for p, n in ((2.0 ** -24, 65), (0.5, 65), (0.88, 65), (0.8809, 130), (1 - 2.0 ** -24, 130)):   # the upper half holds 1 / (1 + e^-2) = 0.88080
        assert NR.keep_mask(a, 1.0, q=NR.q24_of(p)).sum() == n, p
    # one dominant class at T = 0.05: every other mass is 0, only it is kept -- even at top_p = 1 - 2^-24
    d = NR.crafted_rows()[56]
    assert (NR.masses(d, 0.05) > 0).sum() == 1
    assert NR.keep_mask(d, 0.05, q=NR.q24_of(1 - 2.0 ** -24)).sum() == 1
    # all-equal rows and +-0.0: one tie group, everything kept
    for v in (0.5, 0.0, -0.0, -3.0):
        e = np.full(130, v, dtype=np.float32)
        for p in TOP_PS:
            assert NR.keep_mask(e, 0.7, q=NR.q24_of(p)).all()
    z = np.where(np.arange(130) % 2, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    z[5], z[6] = -1.0, 2.0
    assert NR.keep_mask(z, 1.0, q=NR.q24_of(0.1)).sum() == 129 and not NR.keep_mask(z, 1.0, q=NR.q24_of(0.1))[5]   # class 6 holds 7.389 / 136.8 < 0.1
    assert NR.keep_mask(z, 1.0, q=NR.q24_of(0.05)).sum() == 1
    assert NR.threshold(z, 1.0, q=NR.q24_of(0.1)).view(np.uint32) == 0                    # +0.0
    # the geometric ladder at T = 1: class r (rank from 0) has e^(-r / 2); the first n reach 1 - e^(-n / 2) of the total
    lad = NR.crafted_rows()[60]
    for p in (0.1, 0.5, 0.9):
        n = math.ceil(-2 * math.log(1 - p))
        assert NR.keep_mask(lad, 1.0, q=NR.q24_of(p)).sum() == n, (p, n)


def test_kept_mass_reaches_top_p_and_the_set_is_minimal():
    """in float64: the kept classes hold >= top_p of the softmax mass, and without their lowest tie group < top_p -- outside the band (a row
    with a band class, or whose float64 mass is within the band's width of top_p, may go either way)"""
    a = rows()
    n_band_rows = 0
    for T in TS:
        with np.errstate(under='ignore'):
            p64 = np.exp((a.astype(np.float64) - a.max(-1, keepdims=True)) / float(np.float32(T)))
        p64 /= p64.sum(-1, keepdims=True)
        for p in TOP_PS:
            q = NR.q24_of(p)
            keep = NR.keep_mask(a, T, q=q)
            band = NR.band_classes(a, T, q).any(-1)
            n_band_rows += int(band.sum())
            thr = NR.threshold(a, T, q=q)
            mass = np.where(keep, p64, 0).sum(-1)
            less = np.where(a > thr[:, None], p64, 0).sum(-1)                              # the kept set without its lowest tie group
            tol = (130 + 130 * p) * NR.E_UNITS * 2.0 ** -20                                # the band's width as a share of Z >= 2^20
            ok = ~band
            assert (mass[ok] >= q / NR.Q_ONE - tol).all(), (T, p)
            assert (less[ok] < q / NR.Q_ONE + tol).all(), (T, p)
            exact = ok & (np.abs(mass - q / NR.Q_ONE) > tol) & (np.abs(less - q / NR.Q_ONE) > tol)
            assert (mass[exact] >= q / NR.Q_ONE).all() and (less[exact] < q / NR.Q_ONE).all(), (T, p)
            if 0.05 < p < 0.95:                                                            # (the extreme top_p sit inside tol of 0 / 1 themselves)
                assert exact.mean() > 0.5, (T, p, exact.mean())
    print('rows with a band class over all settings: %d' % n_band_rows)


def test_the_kept_set_grows_with_top_p_and_rules_intersect():
    a = rows()
    for T in TS:
        prev = np.zeros(a.shape, dtype=bool)
        for p in TOP_PS:
            m = NR.keep_mask(a, T, q=NR.q24_of(p))
            assert (m | ~prev).all()
            prev = m
        both = NR.keep_mask(a, T, 9, TR.ln_min_p_of(0.5), NR.q24_of(0.5))
        assert np.array_equal(both, TR.keep_mask(a, T, 9, TR.ln_min_p_of(0.5)) & NR.keep_mask(a, T, q=NR.q24_of(0.5)))
        # without the word the restatement is trunc_ref's, bit for bit
        assert np.array_equal(NR.threshold(a, T, 9, TR.ln_min_p_of(0.5), 0).view(np.uint32), TR.threshold(a, T, 9, TR.ln_min_p_of(0.5)).view(np.uint32))
    # top_p = 2^-24: only the classes tied for best
    assert np.array_equal(NR.keep_mask(a, 0.7, q=1), a == a.max(-1, keepdims=True))


def test_decisions_and_the_band():
    a = rows()
    noise = S.pitch_noise(11, 4, np.arange(a.shape[0]), 3, 5)
    q = NR.q24_of(0.5)
    d = NR.decide_pitch(a, noise, 1.0, q=q)
    assert NR.keep_mask(a, 1.0, q=q)[np.arange(a.shape[0]), d].all()
    assert (d != S.decide_pitch(a, noise, 1.0)).any()
    # T = 0: no nucleus rule, the argmax
    assert np.array_equal(NR.decide_pitch(a, noise, 0.0, q=q), a.argmax(-1))
    assert np.isneginf(NR.threshold(a, 0.0, q=q)).all()
    # q = 0: the plain draw
    assert np.array_equal(NR.decide_pitch(a, noise, 1.0, q=0), S.decide_pitch(a, noise, 1.0))
    # the band: never the best class; a band-skippable decision has a band class in its row; E = 0 still flags exact boundaries only
    for T in TS:
        for p in TOP_PS:
            qq = NR.q24_of(p)
            band = NR.band_classes(a, T, qq)
            assert not band[np.arange(a.shape[0]), a.argmax(-1)].any()
            sk = NR.band_skippable(a, noise, T, q=qq)
            assert not (sk & ~band.any(-1)).any()
            assert (NR.band_classes(a, T, qq, E=0) <= band).all()


def parent_words(temperature, dur_temperature=None, seed=7, draw=0, sample_offset=0, top_k=None, min_p=None):
    """the block words as they were before the top_p word existed, restated"""
    tp = float(temperature)
    td = tp if dur_temperature is None else float(dur_temperature)
    words = [seed - (1 << 64) if seed >= (1 << 63) else seed, draw, sample_offset, struct.unpack('<q', struct.pack('<ff', tp, td))[0]]
    if top_k is not None or min_p is not None:
        k = 0 if top_k is None else min(top_k, 130)
        ln = 1.0 if not min_p else math.log(float(min_p))
        words += [struct.unpack('<q', struct.pack('<if', k, ln))[0], 0]
    return words


def test_block_words():
    for kw in (dict(), dict(top_k=8), dict(min_p=0.5), dict(top_k=1000, min_p=0.0), dict(top_k=3, min_p=1.0), dict(min_p=1e-6)):
        for extra in (dict(), dict(dur_temperature=0.7, seed=(1 << 64) - 3, draw=5, sample_offset=16)):
            assert FF_.sampling_words(1.0, **extra, **kw) == parent_words(1.0, **extra, **kw), (kw, extra)
            assert FF_.sampling_words(1.0, **extra, **kw, top_p=None) == parent_words(1.0, **extra, **kw)
    assert len(FF_.sampling_words(1.0)) == 4
    # top_p alone: six words, top_k = 0, ln_min_p = off, the value in the low half of word 5, the high half zero
    for p in TOP_PS + (1e-12, 1 - 2.0 ** -30, 0.25):
        w = FF_.sampling_words(0.7, top_p=p)
        assert len(w) == 6 and w[:4] == parent_words(0.7)
        assert struct.unpack('<if', struct.pack('<q', w[4])) == (0, 1.0)
        lo, hi = struct.unpack('<II', struct.pack('<q', w[5]))
        assert hi == 0 and lo == NR.q24_of(p) and 1 <= lo <= 1 << 24, p
    assert FF_.sampling_words(0.7, top_p=0.25)[5] == 1 << 22
    assert FF_.sampling_words(0.7, top_p=2.0 ** -24)[5] == 1 and FF_.sampling_words(0.7, top_p=1e-12)[5] == 1
    assert FF_.sampling_words(0.7, top_p=1 - 2.0 ** -24)[5] == (1 << 24) - 1
    # top_p = 1.0 alone: still six words, the word 0 (as min_p = 0.0)
    w = FF_.sampling_words(0.7, top_p=1.0)
    assert len(w) == 6 and w[5] == 0 and w == FF_.sampling_words(0.7, min_p=0.0)
    # with the other rules: their word unchanged
    w = FF_.sampling_words(0.7, top_k=8, min_p=0.5, top_p=0.9)
    assert w[:5] == parent_words(0.7, top_k=8, min_p=0.5)[:5] and w[5] == NR.q24_of(0.9)
    assert FF_.check_truncation(None, None, None) is None and FF_.check_truncation(8, None) == (8, 1.0, 0)
    assert FF_.check_truncation(None, None, 0.5) == (0, 1.0, 1 << 23)


def test_host_validation():
    bad = (True, False, 0, 0.0, -0.1, 1.5, 2, float('nan'), float('inf'), -float('inf'), '0.5', [0.5])
    for v in bad:
        for f in (lambda: FF_.check_truncation(None, None, v), lambda: FF_.check_truncation(8, 0.5, v),
                  lambda: FF_.check_sampling(1.0, top_p=v), lambda: FF_.sampling_words(1.0, top_p=v),
                  lambda: FF_.sampling_block('cpu', 1.0, top_p=v),                         # (the value is refused before the device is looked at)
                  lambda: M.DisentangleVAE._check_sampling(temperature=1.0, top_p=v)):
            with pytest.raises(ValueError):
                f()
    for v in (1, 1.0, 0.5, 2.0 ** -24, 1e-30):
        FF_.check_truncation(None, None, v)
        assert M.DisentangleVAE._check_sampling(temperature=1.0, top_p=v) is True
    with pytest.raises(ValueError):                                                        # top_p belongs to a sampled decode
        M.DisentangleVAE._check_sampling(top_p=0.5)
    assert M.DisentangleVAE._check_sampling() is False
