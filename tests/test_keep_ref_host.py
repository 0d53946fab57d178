"""CPU: tests/keep_ref.py (the numpy restatement of the kept-steps rule) against cases written out by hand, and the host-side validation
of DisentangleVAE.keep / the keep= keyword that needs no GPU."""
import numpy as np
import pytest

import keep_ref as K


def blank(B):
    """a grid of empty steps: <sos> in slot 0, <eos> in slot 1, <pad> behind, duration pad 2"""
    x = np.full((B, 32, 16, 6), 2, dtype=np.int64)
    x[..., 0] = 130
    x[:, :, 0, 0] = 128
    x[:, :, 1, 0] = 129
    return x


def note(x, b, t, s, p, bits):
    x[b, t, s, 0] = p
    x[b, t, s, 1:] = bits


def test_one_kept_step_by_hand():
    B = 2
    x = blank(B)
    note(x, 1, 3, 1, 60, (0, 1, 0, 1, 1))
    note(x, 1, 3, 2, 64, (1, 1, 1, 1, 1))
    x[1, 3, 3, 0] = 129                                           # <eos> in slot 3: L = 3, its duration bits are the pad 2
    note(x, 1, 3, 4, 72, (0, 0, 0, 0, 0))                         # behind the <eos>: not kept
    steps = np.zeros((B, 32), dtype=np.uint8)
    steps[1, 3] = 1
    r = K.build(x, steps)
    R, M = 32 * B, 480 * B
    row = 3 * B + 1
    want_p = np.full((15, R), -1, dtype=np.int32)
    want_p[0, row], want_p[1, row], want_p[2, row] = 60, 64, 129
    want_d = np.full((5, M), -1, dtype=np.int32)
    for d, v in enumerate((0, 1, 0, 1, 1)):
        want_d[d, 0 * R + row] = v
    for d in range(5):
        want_d[d, 1 * R + row] = 1
    assert np.array_equal(r['pitch'], want_p)
    assert np.array_equal(r['dur'], want_d)
    assert np.array_equal(r['err'], [0, 0])
    assert r['L'][1, 3] == 3 and r['L'].sum() == 3
    assert r['forced_pitch'].sum() == 3 and r['forced_pitch'][1, 3, :3].all()
    assert r['forced_dur'].sum() == 10 and r['forced_dur'][1, 3, :2].all() and not r['forced_dur'][1, 3, 2].any()


def test_lengths_of_the_edge_steps():
    x = blank(1)
    # t = 0: empty step (<eos> in slot 1); t = 1: 14 notes, <eos> in slot 15; t = 2: 15 notes, no <eos>
    for s in range(1, 15):
        note(x, 0, 1, s, 40 + s, (1, 0, 0, 0, 0))
    x[0, 1, 15, 0] = 129
    for s in range(1, 16):
        note(x, 0, 2, s, 40 + s, (0, 0, 0, 0, 1))
    r = K.build(x, range(3))
    assert list(r['L'][0, :4]) == [1, 15, 15, 0]
    assert r['pitch'][0, 0] == 129 and (r['pitch'][1:, 0] == -1).all()
    assert list(r['pitch'][:, 1]) == [41 + n for n in range(14)] + [129]
    assert list(r['pitch'][:, 2]) == [41 + n for n in range(15)]
    assert (r['pitch'][:, 3:] == -1).all()
    assert r['forced_dur'][0, 0].sum() == 0                       # the <eos> row carries pad bits: free
    assert r['forced_dur'][0, 1, :14].all() and not r['forced_dur'][0, 1, 14].any()
    assert r['forced_dur'][0, 2].all()
    assert r['err'][0] == 0


def test_unforcible_pitches_set_err_and_stay_free():
    x = blank(4)
    note(x, 0, 5, 1, 60, (0, 0, 0, 0, 0)); x[0, 5, 2, 0] = 130; x[0, 5, 3, 0] = 129        # <pad> before the <eos>
    note(x, 1, 5, 1, 131, (0, 0, 0, 0, 0)); x[1, 5, 2, 0] = 129                              # pitch 131
    note(x, 2, 5, 1, -1, (1, 1, 0, 0, 0)); x[2, 5, 2, 0] = 129                               # pitch -1
    note(x, 3, 5, 1, 60, (0, 0, 0, 0, 0)); x[3, 5, 2, 0] = 129; x[3, 5, 3, 0] = 131          # a bad pitch BEHIND the <eos>: not looked at
    r = K.build(x, [5])
    assert list(r['err']) == [1, 1, 1, 0]
    B = 4
    assert list(r['pitch'][:3, 5 * B + 0]) == [60, -1, 129]
    assert list(r['pitch'][:2, 5 * B + 1]) == [-1, 129]
    assert list(r['pitch'][:2, 5 * B + 2]) == [-1, 129]
    assert [r['dur'][d, 0 * 32 * B + 5 * B + 2] for d in range(5)] == [1, 1, 0, 0, 0]        # the bits of a note whose pitch is free are still kept
    assert not r['forced_pitch'][0, 5, 1] and r['forced_pitch'][0, 5, 2]
    # without the step nothing is wrong with the sample
    assert K.build(x, [4])['err'].sum() == 0


def test_step_selections():
    assert K.steps_matrix(range(16), 3)[:, :16].all() and not K.steps_matrix(range(16), 3)[:, 16:].any()
    assert np.array_equal(K.steps_matrix(slice(0, 32, 2), 2)[1], np.arange(32) % 2 == 0)
    one = (np.arange(32) % 4 < 2).astype(np.uint8).reshape(1, 32)
    assert np.array_equal(K.steps_matrix(one, 5), np.broadcast_to(one != 0, (5, 32)))
    x = blank(5)
    a, b = K.build(x, one), K.build(x, np.broadcast_to(one, (5, 32)).copy())
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a['forced_pitch'].sum() == 5 * 16                       # one forced <eos> per kept step


def test_host_step_rows_and_keep_validation():
    """functional_free.keep_steps_row / check_keep / DisentangleVAE._check_sampling: the ValueErrors that need no device"""
    import torch
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    from polyphonic_chord_texture_disentanglement_amd import model as M
    assert FF_.keep_steps_row(range(16)) == bytes([1] * 16 + [0] * 16)
    assert FF_.keep_steps_row(slice(30, None)) == bytes([0] * 30 + [1, 1])
    assert FF_.keep_steps_row([]) == bytes(32)
    for bad in ([32], [-1], [1.0], [True], 5, 'ab'):
        with pytest.raises(ValueError):
            FF_.keep_steps_row(bad)
    with pytest.raises(ValueError):
        FF_.build_keep(torch.zeros(2, 32, 16, 6, dtype=torch.int64), range(4))               # a CPU tensor
    with pytest.raises(ValueError):
        FF_.check_keep(object())
    with pytest.raises(ValueError):
        M.DisentangleVAE._check_sampling(keep={'pitch': None, 'dur': None})
    assert M.DisentangleVAE._check_sampling(keep=None) is False
