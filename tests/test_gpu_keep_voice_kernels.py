"""GPU: ptv_keep_voice_force_build and ptv_grid_split_voice (csrc/keep.hip; include/ptvae_hip.h "Kept voices") element for element
against tests/keep_voice_ref.py, at B = 1, 3 and 67 (R = 2144: a partial last block and a partial last wave), for every combination of one
row / B rows / NULL of mode, below and lowest and both flag values; the whole-step mode against ptv_keep_force_build bit for bit; the
argument checks; what the two split grids are to each other and to x; functional_free.build_keep_voice / split_voice on top."""
import functools
import itertools

import numpy as np
import pytest
import torch

import keep_ref as K
import keep_voice_ref as V
import test_gpu_keep_decode as KD
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = KD.DEV
SENT = -77                                                         # no kernel writes it: force words are >= -1, counts and bits >= 0
ORDER = [1, 5, 6, 7, 4, 2, 3, 9, 10, 0, 8] + list(range(11, 32))   # row 1 holds all six hand-made steps, 5 / 6 / 7 the unforcible ones


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(B):
    """(x [B, 32, 16, 6], mode uint8 [B, 32] of 0 / 1 / 2 / 7, below int32 [B, 32], lowest int32 [B, 32]): the crafted grid of
    test_gpu_keep_decode tiled; limits inside and beyond their ranges; the hand-made steps of the first row are voice steps"""
    x = np.ascontiguousarray(KD.crafted()[0][[ORDER[i % 32] for i in range(B)]])
    rng = np.random.default_rng(100 + B)
    mode = rng.choice(np.array([0, 1, 2, 7], dtype=np.uint8), size=(B, 32), p=[0.2, 0.2, 0.5, 0.1])
    mode[0, :6] = 2
    below = rng.integers(36, 90, (B, 32)).astype(np.int32)
    far = rng.random((B, 32)) < 0.15
    below[far] = rng.choice([-5, 0, 61, 128, 140, 1 << 30], size=int(far.sum()))
    below[0, :6] = 61                                              # 'pad before eos' meets its pad, 'pitch -1' its -1
    lowest = rng.integers(0, 7, (B, 32)).astype(np.int32)
    far = rng.random((B, 32)) < 0.3
    lowest[far] = rng.choice([-2, 15, 20, -(1 << 31)], size=int(far.sum()))
    lowest[0, :6] = 15
    for a in (x, mode, below, lowest):
        a.setflags(write=False)
    return x, mode, below, lowest


def sibling_bytes(B):
    """mode uint8 [B, 32] that cycles through every byte 0..7 and 255 -- the legal bytes of the sibling entry points among them -- each
    row from another start, so that a row and a column meet every byte"""
    cycle = np.array(list(range(8)) + [255], dtype=np.uint8)
    return cycle[(np.arange(32)[None, :] + 3 * np.arange(B)[:, None]) % 9]


def assert_foreign_free(got, mode, foreign, B):
    """every step whose byte is one of `foreign` -- a sibling's legal byte -- came out free (all 15 + 75 words -1, kept_n 0), with bit 1
    of its sample's err"""
    mm = np.broadcast_to(mode, (B, 32))
    hit = np.isin(mm, foreign)
    assert all((mm == f).any() for f in foreign)
    cols = hit.T.reshape(-1)                                       # r = t * B + b
    assert (got['pitch'][:, cols] == -1).all() and (got['dur'].reshape(5, 15, 32 * B)[:, :, cols] == -1).all()
    assert (got['kept_n'][hit] == 0).all() and (got['err'][hit.any(1)] & 2).all()


def variants(a, with_null=True):
    """an argument as B rows, as its first row alone and (limits) as NULL"""
    return [a, np.ascontiguousarray(a[:1])] + ([None] if with_null else [])


def rows_of(a):
    return 1 if a is None else a.shape[0]


def gpu_build(x, mode, below, lowest, flags):
    B = x.shape[0]
    xd, md, bd, ld = dev(x), dev(mode), dev(below), dev(lowest)
    out = dict(pitch=torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV),
               dur=torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV),
               kept_n=torch.full((B, 32), SENT, dtype=torch.int32, device=DEV), err=torch.full((B,), SENT, dtype=torch.int32, device=DEV))
    call('ptv_keep_voice_force_build', ptr(xd), ptr(md), rows_of(mode), ptr(bd), rows_of(below), ptr(ld), rows_of(lowest), flags, B,
         ptr(out['pitch']), ptr(out['dur']), ptr(out['kept_n']), ptr(out['err']), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def gpu_split(x, mode, below, lowest):
    B = x.shape[0]
    xd, md, bd, ld = dev(x), dev(mode), dev(below), dev(lowest)
    out = dict(voice=torch.full((B, 32, 16, 6), SENT, dtype=torch.int64, device=DEV),
               rest=torch.full((B, 32, 16, 6), SENT, dtype=torch.int64, device=DEV),
               kept_n=torch.full((B, 32), SENT, dtype=torch.int32, device=DEV), err=torch.full((B,), SENT, dtype=torch.int32, device=DEV))
    call('ptv_grid_split_voice', ptr(xd), ptr(md), rows_of(mode), ptr(bd), rows_of(below), ptr(ld), rows_of(lowest), B, ptr(out['voice']),
         ptr(out['rest']), ptr(out['kept_n']), ptr(out['err']), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('B', (1, 3, 67))
def test_1_builder_and_split_match_the_reference(B):
    """every combination of B rows / one row for mode, B rows / one row / NULL for below and lowest, both flag values: the four arrays of
    the builder and the two grids, kept_n and err of the split equal keep_voice_ref in every element (so the sentinel is gone everywhere)"""
    x, mode, below, lowest = inputs(B)
    seen = np.zeros(4, dtype=np.int64)
    for m, bl, lw in itertools.product(variants(mode, False), variants(below), variants(lowest)):
        what = (B, rows_of(m), None if bl is None else rows_of(bl), None if lw is None else rows_of(lw))
        sp = gpu_split(x, m, bl, lw)
        voice, rest = V.split(x, m, bl, lw)
        assert np.array_equal(sp['voice'], voice) and np.array_equal(sp['rest'], rest), what
        for flags in (0, 1):
            want = V.build(x, m, bl, lw, durations=not flags)
            got = gpu_build(x, m, bl, lw, flags)
            for k in ('pitch', 'dur', 'kept_n', 'err'):
                assert np.array_equal(got[k], want[k]), what + (flags, k)
            if not flags:
                assert np.array_equal(sp['kept_n'], want['kept_n']) and np.array_equal(sp['err'], want['err']), what
        seen += [(want['K'] > 0).sum(), (want['err'] & 1).sum(), (want['err'] & 2).sum() // 2, (m == 1).sum()]
    assert seen.all()                                              # kept notes, both err bits and whole steps took part
    if B == 3:                                                     # the same grid under every byte: 3 and 4 are the siblings' legal ones
        for m in variants(sibling_bytes(B), False):
            sp = gpu_split(x, m, below, lowest)
            voice, rest = V.split(x, m, below, lowest)
            assert np.array_equal(sp['voice'], voice) and np.array_equal(sp['rest'], rest), rows_of(m)
            for flags in (0, 1):
                want = V.build(x, m, below, lowest, durations=not flags)
                got = gpu_build(x, m, below, lowest, flags)
                for k in ('pitch', 'dur', 'kept_n', 'err'):
                    assert np.array_equal(got[k], want[k]), (rows_of(m), flags, k)
                assert_foreign_free(got, m, (3, 4), B)
            assert np.array_equal(sp['kept_n'], want['kept_n']) and np.array_equal(sp['err'], want['err']), rows_of(m)
            assert (want['err'] & 2).all() and (want['K'][np.broadcast_to(m, (B, 32)) == 2] > 0).any()


def test_2_whole_and_free_steps_are_ptv_keep_force_build():
    """a call whose mode bytes are 0 / 1 only is bit-equal to ptv_keep_force_build on the same selection in all three arrays, whatever
    the limits and the flag"""
    for B in (3, 67):
        x, mode, below, lowest = inputs(B)
        for steps in ((mode == 1).astype(np.uint8), np.ascontiguousarray((mode[:1] == 2).astype(np.uint8))):
            xd, sd = dev(x), dev(steps)
            pitch = torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV)
            dur = torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV)
            err = torch.full((B,), SENT, dtype=torch.int32, device=DEV)
            call('ptv_keep_force_build', ptr(xd), ptr(sd), steps.shape[0], B, ptr(pitch), ptr(dur), ptr(err), stream_ptr())
            torch.cuda.synchronize()
            for flags, bl, lw in ((0, None, None), (1, below, lowest)):
                got = gpu_build(x, steps, bl, lw, flags)
                assert np.array_equal(got['pitch'], pitch.cpu().numpy()) and np.array_equal(got['dur'], dur.cpu().numpy())
                assert np.array_equal(got['err'], err.cpu().numpy())
                assert np.array_equal(got['kept_n'], (got['pitch'] >= 0).sum(0).reshape(32, B).T)
            assert (pitch >= 0).any() and (dur >= 0).any()
    assert int(err.sum()) > 0


def test_3_bad_arguments():
    """PTV_ERR_ARG before any launch: a NULL required pointer, B < 1, a row count outside {1, B}, flags outside 0..1 -- and nothing is
    written; NULL limits with a row count of 1 or B are fine"""
    B = 3
    x, mode, below, lowest = inputs(B)
    xd, md, bd, ld = dev(x), dev(mode), dev(below), dev(lowest)
    i32 = lambda *s: torch.full(s, SENT, dtype=torch.int32, device=DEV)
    outs = [i32(15, 32 * B), i32(5, 480 * B), i32(B, 32), i32(B)]
    grids = [torch.full((B, 32, 16, 6), SENT, dtype=torch.int64, device=DEV) for _ in range(2)]
    st = stream_ptr()
    sel = [ptr(xd), ptr(md), B, ptr(bd), B, ptr(ld), B]
    good_b = sel + [0, B] + [ptr(o) for o in outs]
    good_s = sel + [B] + [ptr(g) for g in grids] + [ptr(o) for o in outs[2:]]
    bad_sel = [(0, None), (1, None), (2, 2), (2, 0), (2, 4), (4, 2), (4, 0), (4, -1), (6, 2), (6, 0), (6, 64)]
    for good, fn, more in ((good_b, lib().ptv_keep_voice_force_build, [(7, 2), (7, -1), (7, 3), (8, 0), (8, -3), (9, None), (10, None),
                                                                         (11, None), (12, None)]),
                           (good_s, lib().ptv_grid_split_voice, [(7, 0), (7, -1), (8, None), (9, None), (10, None), (11, None)])):
        for i, v in bad_sel + more:
            args = list(good)
            args[i] = v
            assert fn(*args, st) == -1, (fn.__name__, i, v)
        for i in (3, 5):                                           # a NULL limit still names a row count
            args = list(good)
            args[i], args[i + 1] = None, 2
            assert fn(*args, st) == -1, (fn.__name__, i)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs + grids)
    for rows in (1, B):
        args = list(good_b)
        args[3], args[4], args[5], args[6] = None, rows, None, rows
        assert lib().ptv_keep_voice_force_build(*args, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), V.build(x, mode)['pitch'])


def notes_of(step):
    """the rows of the slots 1.. of a step [16, 6] before its first <eos> (all 15 without one)"""
    return step[1:K.step_len(step[:, 0]) if (step[1:, 0] == 129).any() else 16]


@pytest.mark.parametrize('B', (3, 67))
def test_4_the_two_grids_of_a_split(B):
    """voice, kept WHOLE by ptv_keep_force_build's rule, gives the voice keep's force words except the <eos> decisions (a voice or free
    step ends in an <eos> the voice keep does not force); the notes of voice followed by the notes of rest are the notes of x, per step"""
    x, mode, below, lowest = inputs(B)
    mode = np.where(mode == 7, 0, mode).astype(np.uint8)
    sp = gpu_split(x, mode, below, lowest)
    want = V.build(x, mode, below, lowest)
    whole = K.build(sp['voice'], np.ones((1, 32), dtype=np.uint8))
    assert np.array_equal(whole['dur'], want['dur'])
    diff = np.argwhere(whole['pitch'] != want['pitch'])
    eos_rows = set()
    for n, r in diff:
        t, b = divmod(int(r), B)
        assert mode[b, t] != 1 and whole['pitch'][n, r] == 129 and want['pitch'][n, r] == -1 and n == want['K'][b, t], (n, b, t)
        eos_rows.add((b, t))
    assert eos_rows == {(b, t) for b in range(B) for t in range(32) if mode[b, t] != 1 and want['K'][b, t] < 15}
    for b in range(B):
        for t in range(32):
            both = np.concatenate([notes_of(sp['voice'][b, t]), notes_of(sp['rest'][b, t])])
            assert np.array_equal(both, notes_of(x[b, t])), (b, t)
            assert len(notes_of(sp['voice'][b, t])) == (want['K'][b, t] if mode[b, t] == 2 else len(notes_of(x[b, t])) * (mode[b, t] == 1))
    assert (sp['voice'][:, :, 0] == x[:, :, 0]).all() and (sp['rest'][:, :, 0] == x[:, :, 0]).all()


def test_5_build_keep_voice_and_split_voice():
    """the Python surface on the device: host and device selections, host and device limits, a step in both selections is a whole step,
    return_counts, durations=False; the ValueErrors that need a device tensor; nothing but the documented Keep comes back"""
    B = 3
    x, _, below, lowest = inputs(B)
    xd = dev(x)
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    vsel = ((t_ + b_) % 4 < 2).astype(np.uint8)
    wsel = (t_ % 8 == 1).astype(np.uint8)
    mode = np.where(wsel != 0, 1, 2 * vsel).astype(np.uint8)
    cases = [(dict(voice_steps=dev(vsel), whole_steps=dev(wsel).bool(), below=60), (mode, 60, None, True)),
             (dict(voice_steps=dev(vsel[:1]).bool(), below=dev(below), lowest=dev(lowest[:1]), durations=False),
              (2 * vsel[:1], below, lowest[:1], False)),
             (dict(voice_steps=range(32), whole_steps=[1, 9, 17, 25], lowest=1), (np.where(wsel[:1] != 0, 1, 2).astype(np.uint8), None, 1, True)),
             (dict(voice_steps=slice(0, 16), whole_steps=dev(wsel[:1]), below=128, lowest=15),
              (np.where(wsel[:1] != 0, 1, 2 * (t_[:1] < 16)).astype(np.uint8), 128, 15, True))]
    for kw, (m, bl, lw, durations) in cases:
        want = V.build(x, m, bl, lw, durations)
        kp, kept_n = FF_.build_keep_voice(xd, return_counts=True, **kw)
        torch.cuda.synchronize()
        assert isinstance(kp, FF_.Keep) and kp.batch == B
        FF_.check_keep(kp, B)
        for got, k in ((kp.pitch, 'pitch'), (kp.dur, 'dur'), (kp.err, 'err'), (kept_n, 'kept_n')):
            assert np.array_equal(got.cpu().numpy(), want[k]), (sorted(kw), k)
        assert isinstance(FF_.build_keep_voice(xd, **kw), FF_.Keep)
        kw.pop('durations', None)
        voice, rest, kn, err = FF_.split_voice(xd, **kw)
        torch.cuda.synchronize()
        wv, wr = V.split(x, m, bl, lw)
        assert np.array_equal(voice.cpu().numpy(), wv) and np.array_equal(rest.cpu().numpy(), wr)
        assert np.array_equal(kn.cpu().numpy(), V.build(x, m, bl, lw)['kept_n']) and np.array_equal(err.cpu().numpy(), want['err'])
    good = dict(voice_steps=dev(vsel), below=60)
    for bad in (dict(voice_steps=dev(vsel).cpu()), dict(voice_steps=dev(vsel).int()), dict(voice_steps=dev(vsel[:2])),
                dict(voice_steps=dev(vsel[:, :31])), dict(whole_steps=dev(wsel[0])), dict(below=dev(below).long()), dict(below=dev(below).cpu()),
                dict(below=dev(below[:2])), dict(lowest=dev(lowest[0])), dict(lowest=dev(lowest).float())):
        with pytest.raises(ValueError):
            FF_.build_keep_voice(xd, **dict(good, **bad))
    for bad_x in (xd.int(), xd[:, :, :15], xd[0]):
        with pytest.raises(ValueError):
            FF_.build_keep_voice(bad_x, range(4), below=60)
