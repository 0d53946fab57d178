"""GPU: the kernels of the kept top voice (include/ptvae_hip.h "Kept top voice") against tests/top_ref.py: ptv_keep_top_force_build element for
element at B = 1, 3 and 65 (one full wave plus one row; 32 * 65 rows are no multiple of 256) with every limit form and flag value;
ptv_grid_split_top; the allowed rule with PTV_FORCE_BELOW words through ptv_debug_pitch_constrain_words in both lane layouts."""
import functools

import numpy as np
import pytest
import torch

import constrain_ref as CR
import nucleus_ref as NR
import test_gpu_constrained_decode as CD
import test_gpu_keep_decode as KD
import test_gpu_keep_rhythm_kernels as RK
import test_gpu_keep_voice_kernels as VK
import top_ref as TP
import trunc_ref as TR
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = KD.DEV
SENT = -77                                                         # no kernel writes it: force words are >= -384 and != -77, counts and bits >= 0
EOS = 129
ROWS = RK.ROWS
dev = RK.dev


@functools.lru_cache(maxsize=None)
def inputs(B):
    """(x [B, 32, 16, 6], mode uint8 [B, 32] of 0 / 1 / 4 and the illegal 2 / 7, above, highest int32 [B, 32]): the grid of the kept-rhythm
    kernel tests (the crafted grid tiled, its first row with every hand-made step) -- its mode bytes with 4 in place of 3 --, and, in row
    0, a step that does not ascend at t = 9; limits drawn per (row, step), out-of-range values among them (they clamp)"""
    x, mode = RK.inputs(B)
    x, mode = x.copy(), np.where(mode == 3, 4, mode).astype(np.uint8)
    x[0, 9, 1:4, 0] = (60, 50, 70)
    x[0, 9, 4, 0] = EOS
    mode[0, 9] = 4
    rng = np.random.default_rng(300 + B)
    above = rng.choice(np.array([0, 48, 60, 72, 128, -5, 200], dtype=np.int32), size=(B, 32))
    highest = rng.choice(np.array([0, 1, 2, 3, 15, -1, 40], dtype=np.int32), size=(B, 32))
    for a in (x, mode, above, highest):
        a.setflags(write=False)
    return x, mode, above, highest


def limit_forms(above, highest):
    """(above, highest) as the entry takes them: both NULL, one NULL, one row, B rows"""
    return ((None, None), (np.ascontiguousarray(above[:1]), None), (None, np.ascontiguousarray(highest[:1])), (above, highest),
            (np.ascontiguousarray(above[:1]), highest))


def rows_of(a):
    return 1 if a is None else a.shape[0]


def gpu_build(x, mode, above, highest, flags):
    B = x.shape[0]
    xd, md, ad, hd = dev(x), dev(mode), dev(above), dev(highest)
    out = dict(pitch=torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV),
               dur=torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV),
               kept_n=torch.full((B, 32), SENT, dtype=torch.int32, device=DEV), err=torch.full((B,), SENT, dtype=torch.int32, device=DEV))
    call('ptv_keep_top_force_build', ptr(xd), ptr(md), mode.shape[0], ptr(ad), rows_of(above), ptr(hd), rows_of(highest), flags, B,
         ptr(out['pitch']), ptr(out['dur']), ptr(out['kept_n']), ptr(out['err']), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('B', (1, 3, 65))
def test_1_builder_matches_the_reference(B):
    """B rows and one row of mode bytes, every limit form, the four flag values: the four arrays equal top_ref in every element (the
    sentinel is gone everywhere); rests, 15-note steps, non-notes, a step that does not ascend, both err bits, whole steps, suffixes of
    0, 1 and more notes and both kinds of word took part"""
    x, mode, above, highest = inputs(B)
    seen = np.zeros(9, dtype=np.int64)
    for m in (mode, np.ascontiguousarray(mode[:1])):
        for ab, hi in limit_forms(above, highest):
            for flags in range(4):
                want = TP.build(x, m, ab, hi, durations='kept' if flags & 1 else True, lanes=not flags & 2)
                got = gpu_build(x, m, ab, hi, flags)
                for k in ('pitch', 'dur', 'kept_n', 'err'):
                    assert np.array_equal(got[k], want[k]), (B, m.shape[0], rows_of(ab), rows_of(hi), flags, k,
                                                             np.argwhere(got[k] != want[k])[:4])
            seen += [(want['K'] == 0).sum(), (want['K'] == 15).sum(), (want['err'] & 1).sum(), (want['err'] & 2).sum(), (m == 1).sum(),
                     (want['pitch'] <= -257).sum(), (want['h'] == 0).sum(), (want['h'] == 1).sum(), (want['h'] > 1).sum()]
    assert seen.all(), seen
    if B == 3:                                                     # the same grid under every byte: 2 and 3 are the siblings' legal ones
        every = VK.sibling_bytes(B)
        for m in (every, np.ascontiguousarray(every[:1])):
            for flags in range(4):
                want = TP.build(x, m, above, highest, durations='kept' if flags & 1 else True, lanes=not flags & 2)
                got = gpu_build(x, m, above, highest, flags)
                for k in ('pitch', 'dur', 'kept_n', 'err'):
                    assert np.array_equal(got[k], want[k]), (m.shape[0], flags, k, np.argwhere(got[k] != want[k])[:4])
                VK.assert_foreign_free(got, m, (2, 3), B)
            assert (want['err'] & 2).all() and (want['pitch'] <= -257).any() and (want['h'] > 0).any()
    lanes, room = (TP.build(x, mode, above, highest, lanes=l)['pitch'] for l in (True, False))
    assert (lanes != room).any() and np.array_equal(lanes >= -1, room >= -1)
    first = TP.build(x, mode)
    assert first['err'][0] == 3 and list(first['pitch'][:5, 9 * B]) == [TP.below(50), TP.below(70), 70, EOS, -1]


def test_2_whole_and_free_steps_are_ptv_keep_force_build():
    """a call whose mode bytes are 0 / 1 only is bit-equal to ptv_keep_force_build on the same selection in all three arrays, whatever the
    flags and limits, and kept_n counts its forced pitch words"""
    for B in (3, 65):
        x, mode, above, highest = inputs(B)
        for steps in ((mode == 1).astype(np.uint8), np.ascontiguousarray((mode[:1] == 4).astype(np.uint8))):
            xd, sd = dev(x), dev(steps)
            pitch = torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV)
            dur = torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV)
            err = torch.full((B,), SENT, dtype=torch.int32, device=DEV)
            call('ptv_keep_force_build', ptr(xd), ptr(sd), steps.shape[0], B, ptr(pitch), ptr(dur), ptr(err), stream_ptr())
            torch.cuda.synchronize()
            for flags, (ab, hi) in zip(range(4), limit_forms(above, highest)):
                got = gpu_build(x, steps, ab, hi, flags)
                assert np.array_equal(got['pitch'], pitch.cpu().numpy()) and np.array_equal(got['dur'], dur.cpu().numpy())
                assert np.array_equal(got['err'], err.cpu().numpy())
                assert np.array_equal(got['kept_n'], (got['pitch'] >= 0).sum(0).reshape(32, B).T)
            assert (pitch >= 0).any() and (dur >= 0).any()
    assert int(err.sum()) > 0


def test_3_bad_arguments():
    """PTV_ERR_ARG before any launch: a NULL pointer (but the limits), B < 1, a row count outside {1, B}, flags outside 0..3 -- and nothing
    is written, by the builder or by the split"""
    B = 3
    x, mode, above, highest = inputs(B)
    xd, md, ad, hd = dev(x), dev(mode), dev(above), dev(highest)
    i32 = lambda *s: torch.full(s, SENT, dtype=torch.int32, device=DEV)
    outs = [i32(15, 32 * B), i32(5, 480 * B), i32(B, 32), i32(B)]
    st = stream_ptr()
    good = [ptr(xd), ptr(md), B, ptr(ad), B, ptr(hd), B, 0, B] + [ptr(o) for o in outs]
    fn = lib().ptv_keep_top_force_build
    for i, v in ((0, None), (1, None), (2, 2), (2, 0), (4, 2), (4, 0), (6, 4), (6, -1), (7, 4), (7, -1), (8, 0), (8, -3), (9, None),
                 (10, None), (11, None), (12, None)):
        args = list(good)
        args[i] = v
        assert fn(*args, st) == -1, (i, v)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs)
    assert fn(*good, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), TP.build(x, mode, above, highest)['pitch'])
    grids = [torch.full((B, 32, 16, 6), SENT, dtype=torch.int64, device=DEV) for _ in range(2)]
    outs = grids + [i32(B, 32), i32(B)]
    good = [ptr(xd), ptr(md), B, ptr(ad), B, ptr(hd), B, B] + [ptr(o) for o in outs]
    fn = lib().ptv_grid_split_top
    for i, v in ((0, None), (1, None), (2, 2), (4, 0), (6, 7), (7, 0), (8, None), (9, None), (10, None), (11, None)):
        args = list(good)
        args[i] = v
        assert fn(*args, st) == -1, (i, v)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs)


def notes_of(step):
    out = []
    for s in range(1, 16):
        if step[s, 0] == EOS:
            break
        out.append(tuple(step[s]))
    return out


@pytest.mark.parametrize('B', (3, 65))
def test_4_split(B):
    """ptv_grid_split_top equals top_ref.split in every element of both grids (sentinel-filled), for every limit form; both are valid
    grids -- notes, an <eos> unless there are 15, <pad> -- and at a top step rest's notes followed by voice's are x's; kept_n and err are
    the builder's"""
    x, mode, above, highest = inputs(B)
    xd = dev(x)
    every = VK.sibling_bytes(B)                                    # first, under every byte: 2 and 3 are the siblings' legal ones  
    for m in (every, np.ascontiguousarray(every[:1])) * (B == 3) + (mode, np.ascontiguousarray(mode[:1])):
        for ab, hi in limit_forms(above, highest):
            voice = torch.full((B, 32, 16, 6), SENT, dtype=torch.int64, device=DEV)
            rest = torch.full((B, 32, 16, 6), SENT, dtype=torch.int64, device=DEV)
            kept_n = torch.full((B, 32), SENT, dtype=torch.int32, device=DEV)
            err = torch.full((B,), SENT, dtype=torch.int32, device=DEV)
            md, ad, hd = dev(m), dev(ab), dev(hi)                    # (held until the launch has run)
            call('ptv_grid_split_top', ptr(xd), ptr(md), m.shape[0], ptr(ad), rows_of(ab), ptr(hd), rows_of(hi), B, ptr(voice), ptr(rest),
                 ptr(kept_n), ptr(err), stream_ptr())
            torch.cuda.synchronize()
            wv, wr, wk = TP.split(x, m, ab, hi)
            ref = TP.build(x, m, ab, hi)
            v, r = voice.cpu().numpy(), rest.cpu().numpy()
            assert np.array_equal(v, wv) and np.array_equal(r, wr), (m.shape[0], rows_of(ab), rows_of(hi))
            assert np.array_equal(kept_n.cpu().numpy(), wk) and np.array_equal(err.cpu().numpy(), ref['err'])
            foreign = np.isin(np.broadcast_to(m, (B, 32)), (2, 3))         # a free step: all of it in rest, none kept, bit 1 of err
            assert np.array_equal(r[foreign], x[foreign]) and (v[foreign][:, 1, 0] == EOS).all() and (wk[foreign] == 0).all()
            assert (ref['err'][foreign.any(1)] & 2).all()
    mm = np.broadcast_to(m, (B, 32))
    n_top = 0
    for b in range(min(B, 8)):
        for t in range(32):
            for g in (v, r):
                n = len(notes_of(g[b, t]))
                if mm[b, t] == 4:
                    assert n == 15 or (g[b, t, n + 1, 0] == EOS and (g[b, t, n + 2:, 0] == 130).all() and (g[b, t, n + 1:, 1:] == 2).all())
            if mm[b, t] == 4:
                assert notes_of(r[b, t]) + notes_of(v[b, t]) == notes_of(x[b, t]), (b, t)
                assert len(notes_of(v[b, t])) == ref['h'][b, t]
                n_top += 1
    assert n_top > 20


# ================================================================================================ the allowed rule
@functools.lru_cache(maxsize=None)
def rule_rows():
    """the 37 crafted rows of the kept-rhythm kernel tests (masks, lo, <eos> the maximum of every fourth row) with words that cycle through:
    a ceiling inside the mask (one over the highest mask pitch above lo; 128 without one), a ceiling whose lane the mask empties (the first
    mask pitch above lo + 1; 128 without one), a ceiling at lo + 1 (under `ascending` the lane is empty: <eos> stays), -2, -1, a forced 5"""
    a, masks, lo, _ = RK.rule_rows()
    bits = CR.mask_bits(masks)
    words = np.zeros(ROWS, dtype=np.int32)
    for r in range(ROWS):
        over = [p for p in range(128) if bits[r, p] and p > lo[r]]
        kind = r % 6
        if kind == 0:
            words[r] = TP.below(over[-1] + 1 if over else 128)
        elif kind == 1:
            gap = [p for p in over if p > lo[r] + 1]
            words[r] = TP.below(gap[0] if gap else 128)
        elif kind == 2:
            words[r] = TP.below(min(max(int(lo[r]) + 1, 1), 128))
        else:
            words[r] = (-2, -1, 5)[kind - 3]
    words.setflags(write=False)
    return a, masks, lo, words


def test_5_allowed_rule_with_ceilings():
    """ptv_debug_pitch_constrain_words on 37 rows in both layouts, ascending off / on, no rule / top_k 1 / top_k 8 / top_p 0.9 / min_p 0.5 at
    T = 0.7, held to top_ref as the kept-rhythm test holds it to rhythm_ref: layouts bit-equal; the keep map equal outside the classes of
    the nucleus / min_p bands, the threshold bit-equal on rows without a band class; never empty; no <eos> and no <sos> on a ceiling row
    unless its lane is empty, and then <eos> alone.  Counted by the reference: relaxed rows, empty lanes, rows whose best allowed logit
    was <eos> and lost it.  With every word -1 the bytes of the entry without words"""
    T = 0.7
    a, masks, lo, words = rule_rows()
    da, dm, dlo, dw = dev(a), dev(masks), dev(lo), dev(words)
    free = dev(np.full(ROWS, -1, dtype=np.int32))
    ceil = words <= -257
    n_rel = n_emp = n_eos_best = 0
    for asc in (False, True):
        al0 = CR.allowed(masks, lo, asc)
        al, rel, emp = TP.allowed(masks, lo, asc, words)
        n_rel += int(rel.sum())
        n_emp += int(emp.sum())
        n_eos_best += int(((CR.constrained(a, al0).argmax(-1) == EOS) & ceil & ~emp).sum())
        assert np.array_equal(al[words >= -1], al0[words >= -1]) and al.any(-1).all()
        assert not al[ceil & ~emp][:, 128:].any() and (al[emp].sum(-1) == 1).all() and al[emp][:, EOS].all()
        assert (rel & ~(al & al0).any(-1)).sum() == rel.sum()                  # a relaxed row holds nothing the mask allows
        con = CR.constrained(a, al)
        for kw in (dict(), dict(top_k=1), dict(top_k=8), dict(top_p=0.9), dict(min_p=0.5)):
            blk = FF_.sampling_block(DEV, T, ascending=asc, **kw)
            got = [RK.constrain_words(blk, da, dm, dlo, dw, layout) for layout in (0, 1)]
            what = (asc, kw)
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), what
            k, l, q = CD.rule(kw)
            want = TP.keep_mask(a, al, T, k, l, q)
            want_thr = CR.threshold(a, al, T, k, l, q)
            band = (NR.band_classes(con, T, q) | TR.band_classes(con, T, l)) & al
            clean = ~band.any(-1)
            mask = got[0][0]
            assert set(np.unique(mask)) <= {0, 1}
            mask = mask.astype(bool)
            assert not (mask & ~al).any(), (what, np.argwhere(mask & ~al)[:4])
            assert np.array_equal(mask[~band], want[~band]), (what, np.argwhere((mask != want) & ~band)[:4])
            assert np.array_equal(got[0][1][clean].view(np.uint32), want_thr[clean].view(np.uint32)), what
            assert mask.any(-1).all() and mask[np.arange(ROWS), con.argmax(-1)].all(), what
            assert np.array_equal(mask[ceil][:, EOS], emp[ceil]) and not mask[ceil][:, 128].any(), what
            if not kw:
                assert np.array_equal(mask, al), what
            for layout in (0, 1):
                old = RK.constrain_words(blk, da, dm, dlo, None, layout)
                new = RK.constrain_words(blk, da, dm, dlo, free, layout)
                assert old[0].tobytes() == new[0].tobytes() and old[1].tobytes() == new[1].tobytes(), what
    print('relaxed rows %d, empty lanes %d, <eos> best and excluded %d' % (n_rel, n_emp, n_eos_best))
    assert n_rel >= 2 and n_emp >= 2 and n_eos_best >= 2, (n_rel, n_emp, n_eos_best)
