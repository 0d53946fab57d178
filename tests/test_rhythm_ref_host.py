"""Host, no GPU: the properties of tests/rhythm_ref.py itself -- the reference the kept-rhythm GPU tests are held to."""
import numpy as np

import constrain_ref as CR
import keep_ref as K
import rhythm_ref as RR

EOS = 129


def blank():
    s = np.full((16, 6), 2, dtype=np.int64)
    s[:, 0] = 130
    s[0, 0] = 128
    return s


def step_of(pitches, eos=True):
    s = blank()
    for i, p in enumerate(pitches, 1):
        s[i] = (p, i & 1, 1, 0, (i >> 1) & 1, 2 if i == 3 else 1)
    if eos and len(pitches) < 15:
        s[len(pitches) + 1, 0] = EOS
    return s


def grid():
    """x [2, 32, 16, 6]: step 0 empty, 1 three notes, 2 fifteen notes without <eos>, 3 fourteen notes, 4 an unforcible pitch before the <eos>,
    5 notes but no <eos> at all (pads behind them), the rest two notes"""
    x = np.stack([np.stack([step_of([60, 64]) for _ in range(32)]) for _ in range(2)])
    for b in range(2):
        x[b, 0] = step_of([])
        x[b, 1] = step_of([50, 55, 59])
        x[b, 2] = step_of(list(range(40, 55)))
        x[b, 3] = step_of(list(range(40, 54)))
        x[b, 4] = step_of([50, 131, 128, 70])
        x[b, 5] = step_of([48, 52], eos=False)
    return x


def test_a_whole_step_is_keep_ref():
    x = grid()
    rng = np.random.default_rng(0)
    sel = rng.random((2, 32)) < 0.5
    sel[:, :6] = True
    want = K.build(x, sel.astype(np.uint8))
    for durations in (True, False):
        got = RR.build(x, sel.astype(np.uint8), durations)
        for k in ('pitch', 'dur', 'err', 'forced_pitch', 'forced_dur'):
            assert np.array_equal(got[k], want[k]), k
        assert not got['not_eos'].any() and (got['K'] == -1).all()
        assert np.array_equal(got['kept_n'], want['forced_pitch'].sum(-1))
    assert want['err'].all()


def test_rhythm_steps():
    x = grid()
    mode = np.full((1, 32), 3, dtype=np.uint8)
    r = RR.build(x, mode)
    B = 2
    col = lambda t, b: r['pitch'][:, t * B + b]
    for b in range(B):
        assert list(col(0, b)) == [EOS] + [-1] * 14                          # K = 0: a rest, <eos> forced at n = 0
        assert list(col(1, b)) == [-2] * 3 + [EOS] + [-1] * 11
        assert list(col(2, b)) == [-2] * 15                                  # K = 15: no <eos> is forced
        assert list(col(3, b)) == [-2] * 14 + [EOS]
        assert list(col(4, b)) == [-2] * 4 + [EOS] + [-1] * 10               # unforcible pitches still count as note positions
        assert list(col(5, b)) == [-2] * 15                                  # no <eos> in the step: 15, whatever the slots hold
    assert list(r['K'][0, :6]) == [0, 3, 15, 14, 4, 15] and np.array_equal(r['kept_n'], r['K'])
    assert list(r['err']) == [1, 1]
    x2 = x.copy()
    x2[:, 4] = x2[:, 1]
    x2[:, 5] = x2[:, 1]
    assert not RR.build(x2, mode)['err'].any()
    # the duration words: x's bits where 0 / 1 for n < K, -1 at the forced <eos> and behind it
    R = 32 * B
    d = r['dur'].reshape(5, 15, R)
    assert list(d[:, 0, 1 * B]) == list(x[0, 1, 1, 1:]) and d[4, 2, 1 * B] == -1 and x[0, 1, 3, 5] == 2
    assert (d[:, 3:, 1 * B] == -1).all() and (d[:, :, 0] == -1).all()
    assert np.array_equal(r['forced_dur'], d.transpose(2, 1, 0).reshape(32, B, 15, 5).transpose(1, 0, 2, 3) >= 0)
    free = RR.build(x, mode, durations=False)
    assert (free['dur'] == -1).all() and np.array_equal(free['pitch'], r['pitch'])
    # maps
    assert np.array_equal(r['not_eos'], (r['pitch'] == -2).T.reshape(32, B, 15).transpose(1, 0, 2))
    assert np.array_equal(r['forced_pitch'], (r['pitch'] >= 0).T.reshape(32, B, 15).transpose(1, 0, 2))


def test_modes_mix_and_illegal_bytes():
    x = grid()
    mode = np.zeros((2, 32), dtype=np.uint8)
    mode[0, 1] = 3; mode[0, 2] = 1; mode[1, 3] = 2; mode[1, 7] = 9; mode[1, 1] = 3
    r = RR.build(x, mode)
    assert list(r['err']) == [0, 2]
    assert (r['pitch'][:, 3 * 2 + 1] == -1).all() and (r['pitch'][:, 7 * 2 + 1] == -1).all()
    assert r['kept_n'][0, 1] == 3 and r['kept_n'][0, 2] == 15 and r['kept_n'][1, 3] == 0
    one = RR.build(x, mode[:1])
    assert np.array_equal(one['pitch'].reshape(15, 32, 2)[:, :, 1], one['pitch'].reshape(15, 32, 2)[:, :, 0])


def rows():
    g = np.random.default_rng(4)
    a = (g.standard_normal((6, 130)) * 0.5).astype(np.float32)
    a[:, EOS] = 4.0                                                          # <eos> is the best logit of every row
    a[:, 70] = 3.0
    a[:, 20] = 2.0
    return a


def test_removal_precedes_top_k():
    a = rows()
    noise = np.zeros((6, 130), dtype=np.float32)
    al = CR.allowed(None, None, False, (6,))
    words = np.array([-2, -1, -2, 5, -3, -7])
    got = RR.decide_pitch(a, noise, al, words, 1.0, top_k=1)
    assert list(got) == [70, EOS, 70, 5, EOS, EOS]                           # other negative words are free: <eos> stays and wins
    keep = RR.keep_mask(a, al, words, 1.0, top_k=1)
    assert keep[0].sum() == 1 and keep[0, 70] and keep[1].sum() == 1 and keep[1, EOS]
    assert list(RR.decide_pitch(a, noise, al, words, 0.0)) == [70, EOS, 70, 5, EOS, EOS]   # without a temperature: the argmax over the set
    # the mask forbids 70: the best ALLOWED pitch
    bits = np.ones((6, 128), dtype=bool)
    bits[:, 70] = False
    al = CR.allowed(CR.mask_from_bits(bits), None, False)
    assert list(RR.decide_pitch(a, noise, al, words, 1.0, top_k=1)) == [20, EOS, 20, 5, EOS, EOS]


def test_empty_intersection_leaves_eos():
    a = rows()
    noise = np.zeros((6, 130), dtype=np.float32)
    bits = np.zeros((6, 128), dtype=bool)
    bits[:, 20] = True
    lo = np.array([19, 20, 127, -1, 20, 20])
    al = CR.allowed(CR.mask_from_bits(bits), lo, True)
    words = np.full(6, -2)
    red = RR.allowed(al, words)
    assert list(RR.fallback(al, words)) == [False, True, True, False, True, True]
    assert list(RR.decide_pitch(a, noise, al, words, 1.0, top_k=8)) == [20, EOS, EOS, 20, EOS, EOS]
    assert red.any(-1).all() and np.array_equal(red[:, EOS], RR.fallback(al, words))
    # <sos> counts as another class only where it is allowed: never under `ascending`
    al2 = CR.allowed(CR.mask_from_bits(np.zeros((1, 128), dtype=bool)), np.array([-1]), False)
    assert RR.allowed(al2, np.array([-2]))[0].nonzero()[0].tolist() == [128]
    al3 = CR.allowed(CR.mask_from_bits(np.zeros((1, 128), dtype=bool)), np.array([-1]), True)
    assert RR.allowed(al3, np.array([-2]))[0].nonzero()[0].tolist() == [EOS]


def test_other_words_change_nothing():
    a = rows()
    g = np.random.default_rng(9)
    noise = g.gumbel(size=(6, 130)).astype(np.float32)
    lo = np.array([-1, 3, 60, 100, 126, 127])
    al = CR.allowed(None, lo, True)
    for w in (-1, -3, -100):
        words = np.full(6, w)
        assert np.array_equal(RR.allowed(al, words), al)
        assert np.array_equal(RR.decide_pitch(a, noise, al, words, 1.0, 8), CR.decide_pitch(a, noise, al, 1.0, 8))
        assert np.array_equal(RR.threshold(a, al, words, 1.0, 8).view(np.uint32), CR.threshold(a, al, 1.0, 8).view(np.uint32))
