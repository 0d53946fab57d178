"""CPU: tests/keep_voice_ref.py (the numpy restatement of the kept-voices rule) against steps worked out by hand, the whole-step mode
against tests/keep_ref.py, and the host-side validation of functional_free.build_keep_voice / split_voice that needs no GPU."""
import numpy as np
import pytest

import keep_ref as K
import keep_voice_ref as V
from test_gpu_keep_decode import spliced_steps
from test_keep_ref_host import blank, note


def step_of(*notes, eos=True):
    """a step [16, 6] holding the given (pitch, bits) notes from slot 1 on, then <eos>"""
    x = blank(1)
    x[0, 0, 1, 0] = 130
    for s, (p, bits) in enumerate(notes, 1):
        note(x, 0, 0, s, p, bits)
    if eos:
        x[0, 0, len(notes) + 1, 0] = 129
    return x[0, 0]


ONES, ZEROS = (1, 1, 1, 1, 1), (0, 0, 0, 0, 0)
SP = spliced_steps()
# (name, step, below, lowest) -> K, bit 0 of err: worked out by hand from the rule
CASES = [
    ('empty', SP['empty'], 60, None, 0, 0),
    ('14 notes: 41 44 .. 59 lie under 60', SP['14 notes'], 60, None, 7, 0),
    ('14 notes, lowest 3', SP['14 notes'], 60, 3, 3, 0),
    ('14 notes, no limit but lowest 15', SP['14 notes'], 128, 15, 14, 0),
    ('15 notes: 35 .. 55, then a pitch EQUAL to below', SP['15 notes'], 60, None, 5, 0),
    ('15 notes, below 61', SP['15 notes'], 61, None, 6, 0),
    ('15 notes without <eos>, all kept', SP['15 notes'], 128, None, 15, 0),
    ('pad before eos: 60 >= below stops first', SP['pad before eos'], 60, None, 0, 0),
    ('pad before eos: the pad is met', SP['pad before eos'], 61, None, 1, 1),
    ('pad before eos: lowest 1 stops before the pad is looked at', SP['pad before eos'], None, 1, 1, 0),
    ('pitch 131 in slot 1', SP['pitch 131'], 60, None, 0, 1),
    ('pitch 131, lowest 0: nothing is looked at', SP['pitch 131'], 60, 0, 0, 0),
    ('pitch -1 behind a kept note', SP['pitch -1'], 60, None, 1, 1),
    ('pitch -1 behind a note that is not kept', SP['pitch -1'], 50, None, 0, 0),
    ('<sos> inside the voice', step_of((40, ONES), (128, ZEROS), (50, ONES)), 60, None, 1, 1),
    ('lowest larger than the step', step_of((40, ONES), (45, ZEROS)), None, 9, 2, 0),
    ('descending: the first note is >= below', step_of((70, ONES), (50, ONES), (40, ONES)), 60, None, 0, 0),
    ('not ascending: the prefix ends at the first note >= below', step_of((50, ONES), (70, ONES), (40, ONES)), 60, None, 1, 0),
    ('below 0 keeps nothing', SP['14 notes'], 0, None, 0, 0),
    ('limits beyond their range are clamped', SP['14 notes'], 1000, 99, 14, 0),
    ('negative lowest is 0', SP['14 notes'], 60, -4, 0, 0),
]


def case_batch():
    """one case per sample, in time step 3; the other steps are empty and free"""
    B = len(CASES)
    x = blank(B)
    mode = np.zeros((B, 32), dtype=np.uint8)
    below = np.full((B, 32), 128, dtype=np.int32)
    lowest = np.full((B, 32), 15, dtype=np.int32)
    for b, (_, step, bl, lw, _, _) in enumerate(CASES):
        x[b, 3] = step
        mode[b, 3] = 2
        below[b, 3] = 128 if bl is None else bl
        lowest[b, 3] = 15 if lw is None else lw
    return x, mode, below, lowest


def test_prefix_lengths_by_hand():
    x, mode, below, lowest = case_batch()
    r = V.build(x, mode, below, lowest)
    for b, (name, _, _, _, k, e) in enumerate(CASES):
        assert r['K'][b, 3] == k and r['kept_n'][b, 3] == k, name
        assert r['err'][b] == e, name
        assert r['forced_pitch'][b, 3, :k].all() and not r['forced_pitch'][b, 3, k:].any(), name
    assert r['K'].sum() == sum(c[4] for c in CASES) and r['kept_n'].sum() == r['K'].sum()


def test_force_words_of_one_voice_step_by_hand():
    B = 2
    x = blank(B)
    note(x, 1, 3, 1, 48, (0, 1, 0, 1, 1))
    note(x, 1, 3, 2, 55, (1, 1, 2, 1, 1))                         # a duration bit that is neither 0 nor 1 stays free
    note(x, 1, 3, 3, 64, (0, 0, 0, 0, 0))                         # >= below: the right hand
    x[1, 3, 4, 0] = 129
    mode = np.zeros((B, 32), dtype=np.uint8)
    mode[1, 3] = 2
    R, M, row = 32 * B, 480 * B, 3 * B + 1
    want_p = np.full((15, R), -1, dtype=np.int32)
    want_p[0, row], want_p[1, row] = 48, 55                       # the <eos> of a voice step is never forced: row 2 stays -1
    want_d = np.full((5, M), -1, dtype=np.int32)
    for d, v in enumerate((0, 1, 0, 1, 1)):
        want_d[d, 0 * R + row] = v
    for d, v in enumerate((1, 1, -1, 1, 1)):
        want_d[d, 1 * R + row] = v
    r = V.build(x, mode, 60)
    assert np.array_equal(r['pitch'], want_p) and np.array_equal(r['dur'], want_d)
    assert list(r['err']) == [0, 0] and r['kept_n'].sum() == 2 and r['kept_n'][1, 3] == 2
    assert r['forced_dur'].sum() == 9
    r = V.build(x, mode, 60, durations=False)                     # "durations stay free": every duration word of a voice step is -1
    assert np.array_equal(r['pitch'], want_p) and (r['dur'] == -1).all() and not r['forced_dur'].any()
    r = V.build(x, mode, None, 1)                                 # the bass note alone
    assert r['pitch'][0, row] == 48 and (r['pitch'] >= 0).sum() == 1
    r = V.build(x, mode, 128, 15)                                 # the whole voicing -- and still no <eos>
    assert list(r['pitch'][:4, row]) == [48, 55, 64, -1] and r['kept_n'][1, 3] == 3


def test_modes():
    """mode 1 is keep_ref's rule element for element and ignores durations; a byte that is none of 0 / 1 / 2 leaves the step free and sets
    bit 1; rows = 1 serves every sample"""
    B = 3
    x = blank(B)
    for b in range(B):
        for t, name in enumerate(SP):
            x[b, t + b] = SP[name]
    steps = (np.arange(32) % 3 != 1).astype(np.uint8).reshape(1, 32)
    want = K.build(x, steps)
    for durations in (True, False):
        r = V.build(x, steps, 60, 2, durations)
        for k in ('pitch', 'dur', 'err', 'forced_pitch', 'forced_dur'):
            assert np.array_equal(r[k], want[k]), k
        assert np.array_equal(r['kept_n'], want['forced_pitch'].sum(-1))
    assert want['err'].any() and want['forced_dur'].any()
    mode = np.zeros((B, 32), dtype=np.uint8)
    mode[1, 1] = 7
    mode[2, 2] = 2
    r = V.build(x, mode, 60)
    assert list(r['err']) == [0, 2, 0] and (r['pitch'][:, [t * B + 1 for t in range(32)]] == -1).all()
    mode[2, 2 + 4] = 3                                            # row 2 holds 'pitch 131' at t = 6
    mode[2, 2 + 5] = 2                                            # ... and 'pitch -1' at t = 7: 50 kept, -1 met
    r = V.build(x, mode, 60)
    assert list(r['err']) == [0, 2, 3]
    a, b_ = V.build(x, steps * 2, 60), V.build(x, np.broadcast_to(steps * 2, (B, 32)).copy(), np.full((B, 32), 60))
    for k in a:
        assert np.array_equal(a[k], b_[k]), k


def test_split_by_hand():
    x, mode, below, lowest = case_batch()
    voice, rest = V.split(x, mode, below, lowest)
    names = [c[0] for c in CASES]
    b = names.index('14 notes, lowest 3')
    s = SP['14 notes']
    assert np.array_equal(voice[b, 3, :4], s[:4]) and list(voice[b, 3, 4]) == [129, 2, 2, 2, 2, 2]
    assert (voice[b, 3, 5:, 0] == 130).all() and (voice[b, 3, 5:, 1:] == 2).all()
    assert np.array_equal(rest[b, 3, 0], s[0]) and np.array_equal(rest[b, 3, 1:13], s[4:16]) and rest[b, 3, 12, 0] == 129
    assert (rest[b, 3, 13:, 0] == 130).all()
    b = names.index('15 notes without <eos>, all kept')
    assert np.array_equal(voice[b, 3], SP['15 notes']) and list(rest[b, 3, :3, 0]) == [128, 129, 130]
    b = names.index('15 notes, below 61')                          # x holds no <eos>: one follows the nine moved notes
    assert np.array_equal(rest[b, 3, 1:10], SP['15 notes'][7:16]) and list(rest[b, 3, 10:12, 0]) == [129, 130]
    b = names.index('descending: the first note is >= below')
    assert list(voice[b, 3, :3, 0]) == [128, 129, 130] and np.array_equal(rest[b, 3], x[b, 3])
    b = names.index('pitch -1 behind a kept note')                 # the unforcible slot leads the rest
    assert list(voice[b, 3, :3, 0]) == [128, 50, 129] and list(rest[b, 3, :4, 0]) == [128, -1, 129, 130]
    # a free step: the reverse of a whole step
    assert np.array_equal(rest[0, 5], x[0, 5]) and list(voice[0, 5, :3, 0]) == [128, 129, 130]
    mode1 = np.ones((1, 32), dtype=np.uint8)
    voice, rest = V.split(x, mode1)
    assert np.array_equal(voice, x) and (rest[:, :, 1, 0] == 129).all() and (rest[:, :, 2:, 0] == 130).all() and (rest[..., 1:] == 2).all()


def test_the_voice_is_no_corner_of_the_synthetic_batch():
    """synth_batch(32, 5) split at pitch 60: of its 1024 steps 330 keep a proper, non-empty prefix, 57 all of their notes, 107 none, 530
    are empty -- and every step is ascending, so the prefix IS the left hand"""
    from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch
    x = synth_batch(32, 5)[0]
    r = V.build(x, np.full((1, 32), 2, dtype=np.uint8), 60)
    L = K.build(x, range(32))['L'] - 1                             # notes of the step (every step of synth_batch holds its <eos>)
    assert (x[np.arange(32)[:, None], np.arange(32)[None], L + 1, 0] == 129).all()
    Kk = r['K']
    assert ((Kk > 0) & (Kk < L)).sum() == 330 and ((Kk == L) & (L > 0)).sum() == 57 and ((Kk == 0) & (L > 0)).sum() == 107
    assert (L == 0).sum() == 530 and r['err'].sum() == 0
    for b in range(32):
        for t in range(32):
            p = x[b, t, 1:L[b, t] + 1, 0]
            assert (np.diff(p) > 0).all() and (p[:Kk[b, t]] < 60).all() and (p[Kk[b, t]:] >= 60).all()


def test_host_validation_and_symbols():
    """the ValueErrors of build_keep_voice / split_voice that need no device, each raised before x is looked at; the header declares
    both entry points"""
    import torch
    from polyphonic_chord_texture_disentanglement_amd import _lib
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    from polyphonic_chord_texture_disentanglement_amd import model as M
    assert {'ptv_keep_voice_force_build', 'ptv_grid_split_voice'} <= set(_lib.exported_symbols())
    assert len(_lib._SIGNATURES['ptv_keep_voice_force_build'][1]) == 14 and len(_lib._SIGNATURES['ptv_grid_split_voice'][1]) == 13
    x = torch.zeros(2, 32, 16, 6, dtype=torch.int64)
    for fn in (FF_.build_keep_voice, FF_.split_voice):
        with pytest.raises(ValueError, match='below .* or lowest'):
            fn(x, range(4))
        for bad in (129, -1, True, 1.5, '60', [60]):
            with pytest.raises(ValueError, match='below must be'):
                fn(x, range(4), below=bad)
        for bad in (16, -1, False, 2.0):
            with pytest.raises(ValueError, match='lowest must be'):
                fn(x, range(4), lowest=bad)
        for bad in ([32], [-1], [1.0], 5):
            with pytest.raises(ValueError, match='time step|steps must be'):
                fn(x, bad, below=60)
            with pytest.raises(ValueError, match='time step|steps must be'):
                fn(x, range(4), below=60, whole_steps=bad)
        with pytest.raises(ValueError, match='voice_steps'):
            fn(x, None, below=60)
        with pytest.raises(ValueError, match='x must be a device tensor'):
            fn(x, range(4), below=60, lowest=1, whole_steps=slice(8, 16))
        with pytest.raises(ValueError, match='x must be a device tensor'):
            fn(x, range(4), below=128)                                                       # 128 / 15: the ends of the ranges are values
        with pytest.raises(ValueError, match='x must be a device tensor'):
            fn(x, range(4), lowest=15)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='durations'):
            FF_.build_keep_voice(x, range(4), below=60, durations=bad)
    assert M.DisentangleVAE.keep_voice.__doc__ and M.DisentangleVAE.split_voice.__doc__
