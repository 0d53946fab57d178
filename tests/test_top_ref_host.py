"""Host, no GPU: the properties of tests/top_ref.py itself -- the reference the kept-top-voice GPU tests are held to -- the induction that
makes the feature safe (every lane non-empty, whatever is drawn), and the ValueErrors of the Python surface, which precede any launch."""
import itertools

import numpy as np
import pytest
import torch

import constrain_ref as CR
import keep_ref as K
import top_ref as TP
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M

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


STEPS = {0: [], 1: [60], 2: [50, 64], 3: list(range(40, 70, 2)), 4: [48, 52], 5: [50, 55, 131, 70], 6: [50, 131, 60, 70], 7: [50, 60, 55, 70],
         8: [40, 50, 60, 70]}


def grid():
    """x [2, 32, 16, 6]: step 0 K = 0, 1 K = 1, 2 K = 2, 3 K = 15 (no <eos>), 4 two notes and no <eos> at all (K = 15: pads count), 5 a
    non-note in the suffix's way, 6 a non-note under the suffix, 7 a step that does not ascend, the rest four notes"""
    x = np.stack([np.stack([step_of(STEPS[8]) for _ in range(32)]) for _ in range(2)])
    for b in range(2):
        for t in range(8):
            x[b, t] = step_of(STEPS[t], eos=t != 4)
    return x


def col(r, t, b, B=2):
    return list(r['pitch'][:, t * B + b])


def test_top_steps_by_hand():
    x = grid()
    mode = np.full((1, 32), 4, dtype=np.uint8)
    r = TP.build(x, mode)                                                   # both limits None: the very top note
    B_ = TP.below
    for b in range(2):
        assert col(r, 0, b) == [EOS] + [-1] * 14                            # K = 0: a rest
        assert col(r, 1, b) == [60, EOS] + [-1] * 13                        # K = 1: the note is the top
        assert col(r, 2, b) == [B_(64), 64, EOS] + [-1] * 12
        assert col(r, 3, b) == [B_(p) for p in range(42, 70, 2)] + [68]     # K = 15: no <eos> forced
        assert col(r, 4, b) == [B_(52)] + [B_(128)] * 14                    # no <eos>: 15 slots, the top one is <pad>: nothing kept
        assert col(r, 5, b) == [B_(55), B_(128), B_(70), 70, EOS] + [-1] * 10
        assert col(r, 6, b) == [B_(128), B_(60), B_(70), 70, EOS] + [-1] * 10
        assert col(r, 7, b) == [B_(60), B_(55), B_(70), 70, EOS] + [-1] * 10
        assert col(r, 8, b) == [B_(50), B_(60), B_(70), 70, EOS] + [-1] * 10
    assert list(r['K'][0, :9]) == [0, 1, 2, 15, 15, 4, 4, 4, 4]
    assert list(r['h'][0, :9]) == [0, 1, 1, 1, 0, 1, 1, 1, 1] and np.array_equal(r['kept_n'], r['h'])
    assert list(r['err']) == [1, 1]
    for bad in (4, 5, 6, 7):
        x2 = x.copy()
        for t in (4, 5, 6, 7):
            if t != bad:
                x2[:, t] = x2[:, 8]
        assert list(TP.build(x2, mode)['err']) == [1, 1], bad
    x2 = x.copy()
    for t in (4, 5, 6, 7):
        x2[:, t] = x2[:, 8]
    assert not TP.build(x2, mode)['err'].any()
    # the suffix stops at a non-note, whatever the limits say; a non-note under it changes nothing above it
    r15 = TP.build(x, mode, highest=15)
    assert r15['h'][0, 5] == 1 and r15['h'][0, 6] == 2 and r15['h'][0, 8] == 4 and r15['h'][0, 3] == 15 and r15['h'][0, 4] == 0
    assert col(r15, 8, 0) == [40, 50, 60, 70, EOS] + [-1] * 10 and col(r15, 3, 0) == list(range(40, 70, 2))
    assert col(r15, 6, 0) == [B_(128), B_(60), 60, 70, EOS] + [-1] * 10
    # highest = 0: nothing is kept, the count is
    r0 = TP.build(x, mode, highest=0)
    assert (r0['h'][:, :9] == 0).all() and col(r0, 8, 1) == [B_(50), B_(60), B_(70), B_(128), EOS] + [-1] * 10
    # above cuts the suffix: to 0 (71), to the notes >= 55
    ra = TP.build(x, mode, above=71)
    assert (ra['h'] == 0).all() and np.array_equal(ra['pitch'], r0['pitch'])
    rb = TP.build(x, mode, above=55)
    assert rb['h'][0, 8] == 2 and col(rb, 8, 0) == [B_(50), B_(60), 60, 70, EOS] + [-1] * 10
    rc = TP.build(x, mode, above=55, highest=1)
    assert rc['h'][0, 8] == 1
    # per (row, step) limits
    hi = np.zeros((2, 32), dtype=np.int32); hi[1, 8] = 3
    rd = TP.build(x, mode, highest=hi)
    assert rd['h'][0, 8] == 0 and rd['h'][1, 8] == 3


def test_room_ceilings():
    x = grid()
    mode = np.full((1, 32), 4, dtype=np.uint8)
    B_ = TP.below
    r = TP.build(x, mode, lanes=False)
    assert col(r, 8, 0) == [B_(68), B_(69), B_(70), 70, EOS] + [-1] * 10
    assert col(r, 2, 0) == [B_(64), 64, EOS] + [-1] * 12
    r0 = TP.build(x, mode, highest=0, lanes=False)
    assert col(r0, 8, 0) == [B_(125), B_(126), B_(127), B_(128), EOS] + [-1] * 10
    assert col(r0, 4, 0) == [B_(114 + n) for n in range(15)]
    # a ceiling is clamped into 1..128
    x2 = x.copy()
    x2[:, 8] = step_of([5, 4, 3, 2])
    r2 = TP.build(x2, mode, lanes=False)
    assert col(r2, 8, 0) == [B_(1), B_(1), B_(2), 2, EOS] + [-1] * 10 and r2['err'][0] == 1
    assert (TP.build(x2, mode)['ceil'][0, 8, :3] == [4, 3, 2]).all()


def test_duration_words():
    x = grid()
    mode = np.full((1, 32), 4, dtype=np.uint8)
    B, R = 2, 64
    full = TP.build(x, mode, above=55)['dur'].reshape(5, 15, R)
    kept = TP.build(x, mode, above=55, durations='kept')['dur'].reshape(5, 15, R)
    none = TP.build(x, mode, above=55, durations=False)['dur']
    assert (none == -1).all()
    c = 8 * B                                                                # step 8, b = 0: K = 4, J = 2
    for n in range(4):
        want = [int(v) if v in (0, 1) else -1 for v in x[0, 8, n + 1, 1:]]
        assert list(full[:, n, c]) == want
        assert list(kept[:, n, c]) == (want if n >= 2 else [-1] * 5)
    assert (full[:, 4:, c] == -1).all() and full[4, 2, c] == -1 and x[0, 8, 3, 5] == 2
    r = TP.build(x, mode, above=55)
    assert np.array_equal(r['forced_dur'], full.transpose(2, 1, 0).reshape(32, B, 15, 5).transpose(1, 0, 2, 3) >= 0)
    assert np.array_equal(r['forced_pitch'], (r['pitch'] >= 0).T.reshape(32, B, 15).transpose(1, 0, 2))
    assert np.array_equal(r['ceil'] > 0, (r['pitch'] <= -257).T.reshape(32, B, 15).transpose(1, 0, 2))


def test_a_whole_step_is_keep_ref_and_modes_mix():
    x = grid()
    rng = np.random.default_rng(0)
    sel = rng.random((2, 32)) < 0.5
    sel[:, :9] = True
    want = K.build(x, sel.astype(np.uint8))
    for lanes in (True, False):
        got = TP.build(x, sel.astype(np.uint8), highest=2, durations='kept', lanes=lanes)
        for k in ('pitch', 'dur', 'err', 'forced_pitch', 'forced_dur'):
            assert np.array_equal(got[k], want[k]), k
        assert (got['K'] == -1).all() and not got['ceil'].any()
        assert np.array_equal(got['kept_n'], want['forced_pitch'].sum(-1))
    mode = np.zeros((2, 32), dtype=np.uint8)
    mode[0, 8] = 4; mode[0, 2] = 1; mode[1, 3] = 2; mode[1, 9] = 3; mode[1, 8] = 4
    r = TP.build(x, mode)
    assert list(r['err']) == [0, 2]
    assert (r['pitch'][:, 3 * 2 + 1] == -1).all() and (r['pitch'][:, 9 * 2 + 1] == -1).all()
    assert r['kept_n'][0, 8] == 1 and r['kept_n'][0, 2] == 3 and r['kept_n'][1, 3] == 0
    one = TP.build(x, mode[:1])
    assert np.array_equal(one['pitch'].reshape(15, 32, 2)[:, :, 1], one['pitch'].reshape(15, 32, 2)[:, :, 0])


def notes_of(step):
    out = []
    for s in range(1, 16):
        if step[s, 0] == EOS:
            break
        out.append(tuple(step[s]))
    return out


def test_split_reassembles():
    x = grid()
    mode = np.full((2, 32), 4, dtype=np.uint8)
    mode[0, 10] = 1; mode[1, 11] = 0
    voice, rest, kept_n = TP.split(x, mode, above=55, highest=3)
    for b in range(2):
        for t in range(32):
            assert (voice[b, t, 0] == x[b, t, 0]).all() and (rest[b, t, 0] == x[b, t, 0]).all()
            if mode[b, t] == 4:
                assert rest_plus_voice(rest[b, t], voice[b, t]) == notes_of(x[b, t]), (b, t)
                assert len(notes_of(voice[b, t])) == kept_n[b, t]
            elif mode[b, t] == 1:
                assert (voice[b, t] == x[b, t]).all() and notes_of(rest[b, t]) == []
            else:
                assert (rest[b, t] == x[b, t]).all() and notes_of(voice[b, t]) == []
            for g in (voice, rest):                                          # a valid step: notes, <eos>, <pad> (15 notes: no <eos>)
                n = len(notes_of(g[b, t]))
                if mode[b, t] == 4:
                    assert n == 15 or (g[b, t, n + 1, 0] == EOS and (g[b, t, n + 2:, 0] == 130).all())
    assert len(notes_of(voice[0, 8])) == 2 and [p[0] for p in notes_of(rest[0, 8])] == [40, 50]


def rest_plus_voice(rest, voice):
    return notes_of(rest) + notes_of(voice)


# ---- the allowed rule ------------------------------------------------------------------------------------------------------------------
def test_allowed_rule_by_hand():
    bits = np.zeros(128, dtype=bool)
    bits[[20, 40, 60]] = True
    nz = lambda a: list(np.nonzero(a)[0])
    # inside the mask: the mask's notes of the lane
    al, rel, emp = TP.allowed_row(bits, 10, True, TP.below(50))
    assert nz(al) == [20, 40] and not rel and not emp
    al, rel, emp = TP.allowed_row(bits, 20, True, TP.below(50))
    assert nz(al) == [40] and not rel and not emp
    # the mask empties the lane: it yields, the lane is the set
    al, rel, emp = TP.allowed_row(bits, 20, True, TP.below(40))
    assert nz(al) == list(range(21, 40)) and rel and not emp
    # the lane is empty: <eos> alone
    for lo, u in ((39, 40), (60, 40), (127, 128)):
        al, rel, emp = TP.allowed_row(bits, lo, True, TP.below(u))
        assert nz(al) == [EOS] and emp and not rel
    # without `ascending` lo is not read; <sos> is never in
    al, rel, emp = TP.allowed_row(bits, 100, False, TP.below(41))
    assert nz(al) == [20, 40] and not rel
    al, rel, emp = TP.allowed_row(None, 100, False, TP.below(128))
    assert nz(al) == list(range(128))
    # the other words keep their meaning
    assert nz(TP.allowed_row(bits, 20, True, -1)[0]) == [40, 60, EOS]
    assert nz(TP.allowed_row(bits, 20, True, -2)[0]) == [40, 60]
    assert nz(TP.allowed_row(bits, 60, True, -2)[0]) == [EOS]
    assert nz(TP.allowed_row(bits, 20, False, -256)[0]) == [20, 40, 60, 128, EOS]     # u = 0 and u = 129 are no ceilings
    assert nz(TP.allowed_row(bits, 20, False, -385)[0]) == [20, 40, 60, 128, EOS]
    assert nz(TP.allowed_row(bits, 20, True, 5)[0]) == [40, 60, EOS]
    # the vector form agrees with constrain_ref / rhythm_ref on the words that are no ceilings
    g = np.random.default_rng(3)
    mb = g.random((40, 128)) < 0.1
    lo = g.integers(-1, 128, 40)
    words = g.choice([-1, -2, 7, -3, -256, -400], 40)
    import rhythm_ref as RR
    for asc in (False, True):
        al, rel, emp = TP.allowed(CR.mask_from_bits(mb), lo, asc, words)
        assert np.array_equal(al, RR.allowed(CR.allowed(CR.mask_from_bits(mb), lo, asc), words)) and not rel.any() and not emp.any()


def test_the_array_form_is_the_loop_form():
    g = np.random.default_rng(8)
    N = 600
    mb = g.random((N, 128)) < g.choice([0.0, 0.02, 0.1, 0.5], (N, 1))
    mask = CR.mask_from_bits(mb)
    lo = g.integers(-1, 128, N)
    u = np.where(g.random(N) < 0.5, np.clip(lo + g.integers(-2, 12, N), 1, 128), g.integers(1, 129, N))
    words = np.where(g.random(N) < 0.7, TP.below(u), g.choice([-1, -2, 7, -256, -385, 129], N))
    seen = np.zeros(2, dtype=np.int64)
    for asc in (False, True):
        for m in (mask, None):
            want = TP.allowed(m, lo, asc, words)
            got = TP.allowed_grid(m, lo, asc, words)
            for a, b in zip(want, got):
                assert np.array_equal(a, b)
            seen += [want[1].sum(), want[2].sum()]
    assert (seen > 20).all(), seen
    got = TP.allowed_grid(mask.reshape(20, 30, 4), lo.reshape(20, 30), True, words.reshape(20, 30))
    assert np.array_equal(got[0].reshape(N, 130), TP.allowed(mask, lo, True, words)[0])


def test_eos_never_wins_under_a_ceiling():
    g = np.random.default_rng(4)
    a = (g.standard_normal((4, 130)) * 0.5).astype(np.float32)
    a[:, EOS] = 4.0
    a[:, 128] = 3.5
    a[:, 70] = 3.0
    a[:, 20] = 2.0
    noise = np.zeros((4, 130), dtype=np.float32)
    words = np.array([TP.below(128), TP.below(70), -1, TP.below(10)])
    al, rel, emp = TP.allowed(None, np.array([-1, -1, -1, 9]), True, words)
    assert list(TP.decide_pitch(a, noise, al, words, 1.0, top_k=1)) == [70, 20, EOS, EOS] and list(emp) == [False, False, False, True]
    assert TP.keep_mask(a, al, 1.0, top_k=1)[0].sum() == 1                   # top_k counts the allowed classes: the rule precedes it


# ---- the induction, by brute force ----------------------------------------------------------------------------------------------------
def draws_never_stall(pitches, h, lanes, top):
    """every sequence of allowed draws under the ceilings of one step, over the toy range 0..top-1: each lane non-empty -> True"""
    K = len(pitches)
    colv = [128] + list(pitches) + [EOS] + [130] * (14 - K)
    J = K - h
    if lanes:
        us = [colv[n + 2] if n + 1 < K else top for n in range(J)]
    else:
        us = [(colv[J + 1] if J < K else top) - (J - 1 - n) for n in range(J)]

    def go(n, lo):
        if n == J:
            return True
        lane = [c for c in range(top) if lo < c < us[n]]
        if not lane:
            return False
        return all(go(n + 1, c) for c in lane)
    return go(0, -1)


def test_induction_brute_force():
    top = 12
    checked = 0
    for K_ in range(0, 6):
        for pitches in itertools.combinations(range(top), K_):
            for h in range(0, K_ + 1):
                for lanes in (True, False):
                    assert draws_never_stall(pitches, h, lanes, top), (pitches, h, lanes)
                    checked += 1
    assert checked == 2 * sum((k + 1) * len(list(itertools.combinations(range(top), k))) for k in range(6))
    # the toy's ceilings are top_ref's with 128 in place of `top`: same formulas on a real step
    for lanes in (True, False):
        for h in range(4):
            colv = np.array([128, 3, 5, 9, EOS] + [130] * 11)
            us = TP.ceilings(colv, 3, h, lanes)
            toy = [colv[n + 2] if n + 1 < 3 else 128 for n in range(3 - h)] if lanes else \
                [(colv[3 - h + 1] if h else 128) - (3 - h - 1 - n) for n in range(3 - h)]
            assert us == [int(v) for v in toy]
    # and a step that does not ascend can stall: the premise is needed
    assert not draws_never_stall((5, 0), 1, True, top) and not draws_never_stall((4, 6, 1), 1, False, top)


# ---- the surface: every ValueError precedes any launch, so it is raised without a GPU -----------------------------------------------------
def test_value_errors_before_any_launch():
    x = torch.zeros(2, 32, 16, 6, dtype=torch.int64)
    for fn in (FF_.build_keep_top, FF_.split_top):
        for kw in (dict(above=129), dict(above=-1), dict(above=True), dict(above=60.0), dict(highest=16), dict(highest=-1),
                   dict(highest='1')):
            with pytest.raises(ValueError, match='above|highest'):
                fn(x, range(32), **kw)
        with pytest.raises(ValueError, match='top_steps'):
            fn(x, None)
        with pytest.raises(ValueError, match='0..31'):
            fn(x, [32])
        with pytest.raises(ValueError, match='0..31'):
            fn(x, range(4), whole_steps=[-1])
        with pytest.raises(ValueError, match='device tensor'):
            fn(x, range(32))                                                 # a host grid
        with pytest.raises(ValueError, match='device tensor'):
            fn('x', range(32))
    for d in (None, 'all', 1, 'KEPT'):
        with pytest.raises(ValueError, match='durations'):
            FF_.build_keep_top(x, range(32), durations=d)
    with pytest.raises(ValueError, match='lanes'):
        FF_.build_keep_top(x, range(32), lanes=1)
    assert FF_.FORCE_BELOW_BASE == -256 and issubclass(FF_.TopKeep, FF_.Keep) and FF_.TopKeep._fields == FF_.Keep._fields


def test_request_refuses_descending_top_keep():
    kp = FF_.TopKeep(None, None, None, 1)
    with pytest.raises(ValueError, match='ascending'):
        M.DisentangleVAE._request(object(), 1, keep=kp, ascending=False)
