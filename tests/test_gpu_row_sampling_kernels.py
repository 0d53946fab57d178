"""GPU: the keep rule with per-row parameters (ptv_debug_pitch_constrain_rows: pitch_constrain() + pitch_keep_threshold() with a row table,
csrc/philox.hpp SampleBlockR) against its numpy restatement evaluated row by row and against the scalar entry run once per parameter
group.  Row r takes group r % 6, so in the 16-lanes-per-row layout every wave holds four different rules -- the branches of
pitch_keep_threshold() diverge between the rows of a wave -- and every 16-row panel holds all six.  The crafted rows, their masks and
the band treatment are those of tests/test_gpu_constrained_decode.py::test_1_allowed_rule_on_crafted_rows."""
import numpy as np
import pytest
import torch

import constrain_ref as CR
import nucleus_ref as NR
import test_gpu_constrained_decode as TC
import trunc_ref as TR
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = TC.DEV
# the six parameter groups of the row-wise tests (keywords of row_sampling_words / sampling_block); row r takes group r % 6
GROUPS = (dict(temperature=1.0), dict(temperature=0.0), dict(temperature=1.0, top_k=4), dict(temperature=1.0, top_p=0.85),
          dict(temperature=1.0, min_p=0.2), dict(temperature=1.0, top_k=8, top_p=0.9, min_p=0.05))
N_RANDOM = 35            # 64 crafted rows + 35 random ones = 99: no multiple of 4 (rows per block, layout 1) nor of 16 (layout 0)


def group_columns(n):
    """the five rule arguments of row_sampling_words for n rows, row r of group r % 6"""
    return {k: [GROUPS[r % 6].get(k) for r in range(n)] for k in ('temperature', 'top_k', 'min_p', 'top_p')}


def rows_of(shift):
    """(logits [99, 130], masks [99, 4], lo [99]): the crafted rows of a shift, then random rows of the model's and of a wide spread"""
    a, masks, lo = TC.crafted(shift)
    g = np.random.default_rng(40 + shift)
    ra = (g.standard_normal((N_RANDOM, 130)) * g.choice([0.03, 1.0, 6.0], (N_RANDOM, 1))).astype(np.float32)
    rm = CR.mask_from_bits(g.random((N_RANDOM, 128)) < g.choice([0.1, 0.5, 1.0], (N_RANDOM, 1)))
    rl = g.integers(-1, 128, N_RANDOM).astype(np.int32)
    return np.concatenate([a, ra]), np.concatenate([masks, rm]), np.concatenate([lo, rl])


def run_rows(table, logits, dm, dlo, words, n, layout, asc):
    blk = FF_.sampling_block(DEV, 0.7, ascending=asc)                    # (only its flags are read: the temperature here is a decoy)
    keep = torch.full((n, 130), 7, device=DEV, dtype=torch.uint8)
    thr = torch.full((n,), 123.0, device=DEV)
    call('ptv_debug_pitch_constrain_rows', ptr(blk), ptr(table), ptr(logits), ptr(dm), ptr(dlo), None if words is None else ptr(words), n,
         layout, ptr(keep), ptr(thr), stream_ptr())
    torch.cuda.synchronize()
    return keep.cpu().numpy(), thr.cpu().numpy()


@pytest.mark.parametrize('shift', (0, 1, 2))
def test_1_rows_rule_equals_the_restatement_row_by_row(shift):
    """kept sets and thresholds of the mixed table equal constrain_ref.keep_mask / threshold evaluated with each row's own parameters,
    with the band treatment of the scalar test; both layouts bit-equal; the 99-row and the 64-row call agree on their common rows"""
    a, masks, lo = rows_of(shift)
    n = a.shape[0]
    assert n == 99
    logits, dm, dlo = torch.from_numpy(a).to(DEV), torch.from_numpy(masks).to(DEV), torch.from_numpy(lo).to(DEV)
    table = torch.from_numpy(FF_.row_sampling_words(n, **group_columns(n))).to(DEV)
    for asc in (False, True):
        al = CR.allowed(masks, lo, asc)
        con = CR.constrained(a, al)
        got = [run_rows(table, logits, dm, dlo, None, n, layout, asc) for layout in (0, 1)]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), (shift, asc)
        short = run_rows(table, logits, dm, dlo, None, 64, 0, asc)
        assert np.array_equal(short[0], got[0][0][:64]) and np.array_equal(short[1].view(np.uint32), got[0][1][:64].view(np.uint32))
        mask = got[0][0]
        assert set(np.unique(mask)) <= {0, 1}
        mask = mask.astype(bool)
        for gi, kw in enumerate(GROUPS):
            r = np.arange(gi, n, 6)
            T = kw['temperature']
            k, l, q = TC.rule(kw)
            want = CR.keep_mask(a[r], al[r], T, k, l, q)
            want_thr = CR.threshold(a[r], al[r], T, k, l, q)
            band = (NR.band_classes(con[r], T, q) | TR.band_classes(con[r], T, l)) & al[r]
            clean = ~band.any(-1)
            what = (shift, asc, gi)
            assert not (mask[r] & ~al[r]).any(), what
            assert np.array_equal(mask[r][~band], want[~band]), (what, np.argwhere((mask[r] != want) & ~band)[:4])
            assert np.array_equal(got[0][1][r][clean].view(np.uint32), want_thr[clean].view(np.uint32)), what
            assert mask[r].any(-1).all() and mask[r][np.arange(len(r)), con[r].argmax(-1)].all(), what


@pytest.mark.parametrize('shift', (0, 2))
def test_2_each_row_equals_the_scalar_entry_of_its_group(shift):
    """bit for bit: row r of the mixed call is row r of ptv_debug_pitch_constrain_words run with group r % 6 as the scalar block --
    keep map and threshold, both layouts, with force words (free, PTV_FORCE_NOT_EOS, PTV_FORCE_BELOW(u)) dealt over the rows; and a
    table with one group in every row is the scalar call on all rows"""
    a, masks, lo = rows_of(shift)
    n = a.shape[0]
    g = np.random.default_rng(7 + shift)
    w = g.choice(np.array([-1, -1, FF_.FORCE_NOT_EOS, FF_.FORCE_BELOW_BASE - 1, FF_.FORCE_BELOW_BASE - 60, FF_.FORCE_BELOW_BASE - 128, 5],
                          dtype=np.int32), n).astype(np.int32)
    logits, dm, dlo, words = (torch.from_numpy(x).to(DEV) for x in (a, masks, lo, w))
    table = torch.from_numpy(FF_.row_sampling_words(n, **group_columns(n))).to(DEV)
    for asc in (False, True):
        for layout in (0, 1):
            mixed = run_rows(table, logits, dm, dlo, words, n, layout, asc)
            for gi, kw in enumerate(GROUPS):
                blk = FF_.sampling_block(DEV, ascending=asc, **kw)
                keep = torch.full((n, 130), 7, device=DEV, dtype=torch.uint8)
                thr = torch.full((n,), 123.0, device=DEV)
                call('ptv_debug_pitch_constrain_words', ptr(blk), ptr(logits), ptr(dm), ptr(dlo), ptr(words), n, layout, ptr(keep), ptr(thr),
                     stream_ptr())
                torch.cuda.synchronize()
                r = np.arange(gi, n, 6)
                assert np.array_equal(mixed[0][r], keep.cpu().numpy()[r]), (shift, asc, layout, gi)
                assert np.array_equal(mixed[1][r].view(np.uint32), thr.cpu().numpy()[r].view(np.uint32)), (shift, asc, layout, gi)
                if layout == 0 and gi in (2, 5):
                    uni = torch.from_numpy(FF_.row_sampling_words(n, **kw)).to(DEV)
                    one = run_rows(uni, logits, dm, dlo, words, n, layout, asc)
                    assert np.array_equal(one[0], keep.cpu().numpy()) and np.array_equal(one[1].view(np.uint32), thr.cpu().numpy().view(np.uint32))


def test_3_bad_arguments_are_refused_before_any_launch():
    d = torch.zeros(256, device=DEV)
    di = torch.zeros(256, device=DEV, dtype=torch.int32)
    st = stream_ptr()
    f = lib().ptv_debug_pitch_constrain_rows
    assert f(None, ptr(di), ptr(d), ptr(di), ptr(di), None, 1, 0, ptr(d), ptr(d), st) == -1
    assert f(ptr(d), None, ptr(d), ptr(di), ptr(di), None, 1, 0, ptr(d), ptr(d), st) == -1
    assert f(ptr(d), ptr(di[1:]), ptr(d), ptr(di), ptr(di), None, 1, 0, ptr(d), ptr(d), st) == -1     # a table that is not 16-byte aligned
    assert f(ptr(d), ptr(di), ptr(d), ptr(di), ptr(di), None, 0, 0, ptr(d), ptr(d), st) == -1
    assert f(ptr(d), ptr(di), ptr(d), ptr(di), ptr(di), None, 1, 2, ptr(d), ptr(d), st) == -1
