"""Host, no GPU: the properties of tests/dur_limits_ref.py itself -- the reference the duration-limit GPU tests are held to -- by brute force over
all 528 ranges, the five bits and every prefix; the header's macro against the reference's encoding; the reference builder."""
import os
import re

import numpy as np
import pytest

import dur_limits_ref as DR

RANGES = [(lo, hi) for lo in range(32) for hi in range(lo, 32)]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ptvae_hip.h')


def test_there_are_528_ranges_and_the_word_round_trips():
    assert len(RANGES) == 528
    words = set()
    for lo, hi in RANGES:
        w = DR.word(lo, hi)
        assert -2047 <= w <= -1024
        assert DR.unword(w) == (lo, hi)
        words.add(w)
    assert len(words) == 528
    for w in (-1, -2, -256, -257, -384, -1023, -2048, -5000, 0, 1, 129):
        assert DR.unword(w) is None
        assert DR.allowed(w, 2, 1) == (True, True)


def test_the_allowed_set_is_what_enumerating_the_completions_gives():
    """independent of dur_ref.allowed's own loop: from the set of values of the range"""
    n = 0
    for lo, hi in RANGES:
        w = DR.word(lo, hi)
        inside = set(range(lo, hi + 1))
        for d in range(5):
            for p in range(1 << d):
                for b in (0, 1):
                    comp = [v for v in range(32) if (v >> (4 - d)) == 2 * p + b]
                    assert len(comp) == 1 << (4 - d)
                    assert DR.allowed(w, d, p)[b] == bool(inside & set(comp)), (lo, hi, d, p, b)
                    # ... and the interval form the header states
                    q, s = 2 * p + b, 4 - d
                    assert DR.allowed(w, d, p)[b] == ((q << s) <= hi and (q << s) + (1 << s) - 1 >= lo)
                    n += 1
    assert n == 528 * 31 * 2
    assert len(DR.table()) == 528 * 31


def test_every_path_through_allowed_bits_ends_in_the_range_and_every_value_is_reachable():
    for lo, hi in RANGES:
        w = DR.word(lo, hi)
        ends = set()
        stack = [(0, 0)]
        while stack:
            d, p = stack.pop()
            if d == 5:
                ends.add(p)
                continue
            a = DR.allowed(w, d, p)
            assert a[0] or a[1], (lo, hi, d, p)                          # a prefix reached through allowed bits always goes on
            for b in (0, 1):
                if a[b]:
                    stack.append((d + 1, 2 * p + b))
        assert ends == set(range(lo, hi + 1)), (lo, hi)


def test_decide():
    for lo, hi in RANGES:
        w = DR.word(lo, hi)
        for model in range(32):                                          # the model's own preference, bit by bit
            p = 0
            for d in range(5):
                want = (model >> (4 - d)) & 1
                got = DR.decide(w, d, p, want)
                a = DR.allowed(w, d, p)
                assert a[got]
                if a[want]:
                    assert got == want                                   # the model's bit wherever it is allowed
                assert DR.determined(w, d, p) == (a[0] != a[1])
                p = 2 * p + got
            assert lo <= p <= hi
            if lo <= model <= hi:
                assert p == model
    # a forced word overrides, a plain free word and a prefix that left the range (neither allowed) leave the decision alone
    assert DR.decide(1, 0, 0, 0) == 1 and DR.decide(0, 4, 7, 1) == 0 and DR.determined(0, 1, 1)
    for w in (-1, -2, -300):
        assert DR.decide(w, 2, 3, 1) == 1 and DR.decide(w, 2, 3, 0) == 0 and not DR.determined(w, 2, 3)
    w = DR.word(0, 3)
    assert DR.allowed(w, 1, 1) == (False, False)
    assert DR.decide(w, 1, 1, 1) == 1 and DR.decide(w, 1, 1, 0) == 0 and not DR.determined(w, 1, 1)


def test_the_headers_macro_is_the_references_encoding():
    src = open(HEADER).read()
    m = re.search(r'#define\s+PTV_FORCE_DUR_RANGE\(lo,\s*hi\)\s+(.+)', src)
    assert m, 'PTV_FORCE_DUR_RANGE is not defined in include/ptvae_hip.h'
    body = m.group(1).strip()
    assert re.fullmatch(r'[-()\s\d|<lohi]+', body), body                  # integers, lo, hi, | << - and brackets: the same in C and Python
    for lo, hi in RANGES:
        assert eval(body, {'__builtins__': {}}, {'lo': lo, 'hi': hi}) == DR.word(lo, hi), (lo, hi)
    assert DR.BASE == -1024


def test_fits():
    assert DR.fit_row('segment') == list(range(32, 0, -1))
    assert DR.fit_row('bar') == list(range(16, 0, -1)) * 2
    assert DR.fit_row('beat') == [4, 3, 2, 1] * 8
    with pytest.raises(KeyError):
        DR.fit_row('phrase')


def test_builder():
    B = 3
    rng = np.random.default_rng(5)
    lo = rng.integers(0, 40, (B, 32)).astype(np.uint8)
    hi = rng.integers(0, 40, (1, 32)).astype(np.uint8)
    steps = (rng.random((B, 32)) < 0.7).astype(np.uint8)
    r = DR.build(lo, hi, steps, B)
    R = 32 * B
    assert (r['pitch'] == -1).all()
    for b in range(B):
        for t in range(32):
            H = min(max(int(hi[0, t]), 1), 32)
            F = max(int(lo[b, t]), 1)
            col = r['dur'][:, np.arange(15) * R + t * B + b]
            if not steps[b, t]:
                assert (col == -1).all() and r['yielded'][b, t] == 0 and not r['limited'][b, t].any()
                continue
            assert r['yielded'][b, t] == int(F > H)
            assert (col == DR.word(min(F, H) - 1, H - 1)).all() and r['limited'][b, t].all()
            assert (r['lo'][b, t], r['hi'][b, t]) == (min(F, H) - 1, H - 1)
    assert r['yielded'].sum() > 0
    # built INTO arrays: forced and foreign words survive, a decision with any forced bit keeps all five words
    src_p = rng.integers(-400, 130, (15, R)).astype(np.int32)
    src_d = np.full((5, 15 * R), -1, dtype=np.int32)
    pick = rng.random(15 * R)
    for d in range(5):
        src_d[d, pick < 0.3] = rng.integers(0, 2, int((pick < 0.3).sum()))
    src_d[2, (pick >= 0.3) & (pick < 0.4)] = 1                            # one forced bit among free ones
    src_d[:, (pick >= 0.4) & (pick < 0.5)] = -7                           # a foreign negative word: free, so it gets the range
    r2 = DR.build(lo, hi, steps, B, src_p, src_d)
    assert np.array_equal(r2['pitch'], src_p)
    for i in range(15 * R):
        n, rest = divmod(i, R)
        t, b = divmod(rest, B)
        if steps[b, t] and (src_d[:, i] < 0).all():
            assert (r2['dur'][:, i] == DR.word(r2['lo'][b, t], r2['hi'][b, t])).all() and r2['limited'][b, t, n]
        else:
            assert np.array_equal(r2['dur'][:, i], src_d[:, i]) and not r2['limited'][b, t, n]
    # a second build over the first replaces the range words of the selected steps
    r3 = DR.build(np.full((1, 32), 2, np.uint8), np.full((1, 32), 4, np.uint8), np.ones((1, 32), np.uint8), B, r['pitch'], r['dur'])
    assert (r3['dur'] == DR.word(1, 3)).all()
    assert DR.value([1, 0, 1, 1, 0]) == 22
