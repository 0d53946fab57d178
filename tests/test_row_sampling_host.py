"""CPU: the host side of per-row sampling (functional_free.row_sampling_words and the ten-word block): the row table is bit-equal to the
words the scalar block holds for the same values, scalars broadcast, every bad value raises and names its row, the sample ids, and the
word count that names the row-wise kind.  Nothing here touches a GPU."""
import itertools
import struct

import numpy as np
import pytest
import torch

from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M

TS = (0, 0.5, 1, 1.7)
TOP_KS = (None, 1, 8, 130, 500)
MIN_PS = (None, 0, 1e-3, 0.2, 1)
TOP_PS = (None, 1e-9, 0.5, 0.9, 1)


def scalar_words(T, td, k, mp, pp):
    """words 3 to 5 of the scalar block as five int32: (T_pitch, T_dur, top_k, ln_min_p, top_p_q24); ascending=False makes the block carry
    its truncation words whatever the rule"""
    w = FF_.sampling_words(T, td, top_k=k, min_p=mp, top_p=pp, ascending=False)
    assert len(w) == 8
    return np.frombuffer(struct.pack('<qq', w[3], w[4]) + struct.pack('<q', w[5])[:4], dtype=np.int32)


def test_1_table_is_bit_equal_to_the_scalar_block():
    grid = list(itertools.product(TS, TOP_KS, MIN_PS, TOP_PS))
    n = len(grid)
    assert n == 500
    cols = [list(c) for c in zip(*grid)]
    tds = [None if i % 3 else 0.25 * (i % 7) for i in range(n)]
    tab = FF_.row_sampling_words(n, cols[0], tds, cols[1], cols[2], cols[3])
    assert isinstance(tab, np.ndarray) and tab.dtype == np.int32 and tab.shape == (n, 8) and tab.flags['C_CONTIGUOUS']
    for r, (T, k, mp, pp) in enumerate(grid):
        assert np.array_equal(tab[r, :5], scalar_words(T, tds[r], k, mp, pp)), (r, T, tds[r], k, mp, pp)
    assert not tab[:, 5].any()
    assert np.array_equal(tab.view(np.int64)[:, 3], np.arange(n))
    # numpy arrays in place of lists: the same table
    tab2 = FF_.row_sampling_words(n, np.array(cols[0], dtype=np.float64), tds, cols[1], cols[2], cols[3])
    assert np.array_equal(tab, tab2)


def test_2_scalars_broadcast_and_ids():
    tab = FF_.row_sampling_words(5, 0.8, top_k=6, top_p=0.5, sample_offset=40)
    want = scalar_words(0.8, None, 6, None, 0.5)
    assert all(np.array_equal(tab[r, :5], want) for r in range(5))
    assert tab.view(np.int64)[:, 3].tolist() == [40, 41, 42, 43, 44]
    mixed = FF_.row_sampling_words(3, [0.0, 1.0, 2.0], 0.5, top_k=[None, 3, None])
    assert mixed.view(np.float32)[:, 0].tolist() == [0.0, 1.0, 2.0] and mixed.view(np.float32)[:, 1].tolist() == [0.5] * 3
    assert mixed[:, 2].tolist() == [0, 3, 0]
    ids = [7, (1 << 47) - 1, 0]
    assert FF_.row_sampling_words(3, 1.0, sample_id=ids).view(np.int64)[:, 3].tolist() == ids
    assert FF_.row_sampling_words(3, 1.0, sample_id=np.array(ids)).view(np.int64)[:, 3].tolist() == ids
    assert FF_.row_sampling_words(2, None).view(np.float32)[:, :2].tolist() == [[0.0, 0.0]] * 2          # no temperature: the argmax


@pytest.mark.parametrize('kw, text', [
    (dict(temperature=[1.0, -1.0, 1.0]), 'row 1: temperature must be a finite float >= 0'),
    (dict(temperature=[1.0, 1.0, float('nan')]), 'row 2: temperature must be'),
    (dict(temperature=1.0, dur_temperature=[0.5, 0.5, float('inf')]), 'row 2: dur_temperature must be'),
    (dict(temperature=1.0, top_k=[1, 0, 1]), 'row 1: top_k must be an integer >= 1'),
    (dict(temperature=1.0, top_k=[1, 2, 2.0]), 'row 2: top_k must be'),
    (dict(temperature=1.0, min_p=[0.1, 0.2, 1.5]), 'row 2: min_p must be a finite float in [0, 1]'),
    (dict(temperature=1.0, top_p=[0.0, 0.2, 0.5]), 'row 0: top_p must be a finite float in (0, 1]'),
    (dict(temperature=1.0, top_p=[0.5, True, 0.5]), 'row 1: top_p must be'),
    (dict(temperature=1.0, sample_id=[0, -1, 2]), 'row 1: sample_id must be an integer in [0, 2^47)'),
    (dict(temperature=1.0, sample_id=[0, 1, 1 << 47]), 'row 2: sample_id must be'),
    (dict(temperature=1.0, sample_id=[0, 1, 2.0]), 'row 2: sample_id must be'),
])
def test_3_every_bad_value_names_its_row(kw, text):
    with pytest.raises(ValueError) as got:
        FF_.row_sampling_words(3, **kw)
    assert str(got.value).startswith(text), str(got.value)
    # ... and the rest of the text is the scalar validator's own
    if 'sample_id' not in kw:
        bad = {k: (v[int(text[4])] if isinstance(v, list) else v) for k, v in kw.items()}
        with pytest.raises(ValueError) as direct:
            FF_.check_sampling(bad.get('temperature'), bad.get('dur_temperature'), top_k=bad.get('top_k'), min_p=bad.get('min_p'),
                               top_p=bad.get('top_p'))
        assert str(got.value) == 'row %s: %s' % (text[4], direct.value)


def test_4_shapes_and_offsets_are_checked():
    for kw in (dict(temperature=[1.0, 1.0]), dict(temperature=1.0, top_k=[1, 2, 3, 4]), dict(temperature=np.ones((3, 1))),
               dict(temperature=torch.ones(3)), dict(temperature='1.0'), dict(temperature=1.0, sample_id=[1, 2]),
               dict(temperature=1.0, sample_offset=-1), dict(temperature=1.0, sample_offset=1 << 47)):
        with pytest.raises(ValueError):
            FF_.row_sampling_words(3, **kw)
    for batch in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            FF_.row_sampling_words(batch, 1.0)


def test_5_the_ten_word_block_is_the_row_wise_kind():
    k = FF_.block_kind(torch.zeros(10, dtype=torch.int64))
    assert k is FF_.ROWWISE and k.kind == 4 and k.nbytes == 80 and k.words == 10 and k.cons == 1 and k.trunc == 1 and k.rows == 1
    assert k.bits == FF_.SAMPLE_BIT | FF_.TRUNC_BIT | FF_.CONS_BIT | FF_.ROWS_BIT and FF_.ROWS_BIT == 0x4000000
    assert (k.note_token, k.dur_gru, k.dur_token) == ('ptv_note_token_sample_rows', 'ptv_dur_gru_fwd_sample_rows',
                                                      'ptv_dur_out_token_sample_rows')
    assert [FF_.block_kind(torch.zeros(w, dtype=torch.int64)).rows for w in (4, 6, 8)] == [0, 0, 0] and FF_.ARGMAX.rows == 0
    for name in (k.note_token, k.dur_gru, k.dur_token, 'ptv_debug_pitch_constrain_rows'):
        from polyphonic_chord_texture_disentanglement_amd import _lib
        assert name in _lib.exported_symbols()
    assert FF_.note_loop_word(0, 0, None, 0, k) == k.bits
    assert 'rows' in M.DECODE_KEYS and 'rows' in M.DECODE_KEYS[:-2]


def test_6_rows_is_validated_before_anything_runs():
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    with pytest.raises(ValueError, match='rows must be what DisentangleVAE.row_sampling'):
        m._request(3, rows=np.zeros((3, 8), dtype=np.int32))
    with pytest.raises(RuntimeError, match='device memory'):
        m.row_sampling(3, 1.0)                                           # (the model is on the CPU; the values were fine)
    with pytest.raises(ValueError, match='row 2: top_k'):
        m.row_sampling(3, 1.0, top_k=[1, 2, 0])
    assert m._sample_draws == 0
