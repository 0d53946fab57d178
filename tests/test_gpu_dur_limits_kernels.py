"""GPU: the kernels of the duration limits (include/ptvae_hip.h "Duration limits") against tests/dur_limits_ref.py:
ptv_dur_range_force_build element for element at B = 1, 3 and 65 with one row and B rows of floors / ceilings / selections, every fit
through DisentangleVAE.dur_limits, a floor above its ceiling with its count, built into a whole-step keep, a rhythm keep and a top keep
(forced and foreign words survive bit for bit); the rule itself through ptv_debug_dur_range on the whole brute-force table."""
import functools

import numpy as np
import pytest
import torch

import dur_limits_ref as DR
import test_gpu_keep_decode as KD
import test_gpu_truncated_sampling as TT
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = KD.DEV
SENT = -77                                                         # no kernel writes it: it is no range word, counts are 0 / 1


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def gpu_build(lo, hi, steps, B, src=None):
    out = dict(pitch=torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV),
               dur=torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV),
               yielded=torch.full((B, 32), SENT, dtype=torch.int32, device=DEV))
    l, h, s = dev(lo), dev(hi), dev(steps)
    sp, sd = (None, None) if src is None else (dev(src[0]), dev(src[1]))
    call('ptv_dur_range_force_build', ptr(l), lo.shape[0], ptr(h), hi.shape[0], ptr(s), steps.shape[0], ptr(sp), ptr(sd), B, ptr(out['pitch']),
         ptr(out['dur']), ptr(out['yielded']), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def limits(B):
    """floors / ceilings as bytes 0..40 (0 and > 32 are clamped), a selection of about three steps in four; in every batch some floor lies
    above its ceiling at a selected step"""
    rng = np.random.default_rng(300 + B)
    lo = rng.integers(0, 41, (B, 32)).astype(np.uint8)
    hi = rng.integers(0, 41, (B, 32)).astype(np.uint8)
    steps = (rng.random((B, 32)) < 0.75).astype(np.uint8)
    lo[0, 3], hi[0, 3], steps[0, 3] = 9, 4, 1
    lo[0, 4], hi[0, 4], steps[0, 4] = 9, 4, 0                        # ... and at a step that is not selected: not counted
    for a in (lo, hi, steps):
        a.setflags(write=False)
    return lo, hi, steps


@pytest.mark.parametrize('B', (1, 3, 65))
def test_1_builder_matches_the_reference(B):
    lo, hi, steps = limits(B)
    n_yield = 0
    for rl in (1, B):
        for rh in (1, B):
            for rs in (1, B):
                a, b, c = (np.ascontiguousarray(v[:r]) for v, r in ((lo, rl), (hi, rh), (steps, rs)))
                want = DR.build(a, b, c, B)
                got = gpu_build(a, b, c, B)
                for k in ('pitch', 'dur', 'yielded'):
                    assert np.array_equal(got[k], want[k]), (k, rl, rh, rs)
                assert (got['pitch'] == -1).all()
                n_yield += int(want['yielded'].sum())
    want = DR.build(lo, hi, steps, B)
    assert want['yielded'][0, 3] == 1 and want['yielded'][0, 4] == 0
    assert want['dur'][0, 3 * B] == DR.word(3, 3)                     # the ceiling won: 4..4
    assert n_yield > 0 and want['limited'].any()


def test_2_arguments():
    lo, hi, steps = limits(3)
    l, h, s = dev(lo), dev(hi), dev(steps)
    p, d, y = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (15 * 96, 5 * 1440, 96))
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    f = lib().ptv_dur_range_force_build
    ok = (ptr(l), 3, ptr(h), 3, ptr(s), 3, None, None, 3, ptr(p), ptr(d), ptr(y), stream_ptr())
    assert f(*ok) == 0
    for i, v in ((0, None), (2, None), (4, None), (9, None), (10, None), (11, None), (1, 2), (3, 2), (5, 2), (8, 0), (6, ptr(p)), (7, ptr(d))):
        bad = list(ok)
        bad[i] = v
        assert f(*bad) != 0, i
    bad = list(ok)
    bad[6], bad[7] = ptr(p), ptr(d)                                   # the outputs as their own source
    assert f(*bad) != 0
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def model():
    return TT.model()


def keeps(B):
    """(name, keep) built from the crafted grid: a whole-step keep, a rhythm keep, a top keep -- forced pitches, forced duration bits,
    -2 and -256 - u words among their arrays"""
    m = model()
    x = dev(np.ascontiguousarray(KD.crafted()[0][[i % 32 for i in range(B)]]))
    sel = [t for t in range(32) if t % 3 != 2]
    return (('whole', m.keep(x, sel)), ('rhythm', m.keep_rhythm(x, sel, durations=False, whole_steps=[0, 1])),
            ('rhythm-dur', m.keep_rhythm(x, sel)), ('top', m.keep_top(x, sel, durations='kept')))


@pytest.mark.parametrize('B', (3, 65))
def test_3_built_into_a_keep(B):
    m = model()
    lo, hi, steps = limits(B)
    for name, keep in keeps(B):
        sp, sd = keep.pitch.cpu().numpy(), keep.dur.cpu().numpy()
        want = DR.build(lo, hi, steps, B, sp, sd)
        got = gpu_build(lo, hi, steps, B, (sp, sd))
        for k in ('pitch', 'dur', 'yielded'):
            assert np.array_equal(got[k], want[k]), (name, k)
        forced = sd >= 0
        assert forced.any() or name == 'rhythm'
        assert np.array_equal(got['dur'][forced], sd[forced]) and np.array_equal(got['pitch'], sp)
        # through the model: the same arrays, the keep stays what it is
        out, y = m.dur_limits(min_dur=dev(lo), max_dur=dev(hi), steps=dev(steps), keep=keep, return_counts=True)
        assert np.array_equal(out.pitch.cpu().numpy(), want['pitch']) and np.array_equal(out.dur.cpu().numpy(), want['dur'])
        assert np.array_equal(y.cpu().numpy(), want['yielded']) and out.err is keep.err and out.batch == B
        assert isinstance(out, FF_.DurKeep) and isinstance(out, type(keep))
        assert isinstance(out, FF_.RhythmKeep) == isinstance(keep, FF_.RhythmKeep)
        assert isinstance(out, FF_.TopKeep) == isinstance(keep, FF_.TopKeep)
        again = m.dur_limits(min_dur=2, max_dur=3, keep=out)            # built into a DurKeep: the same type, the range words replaced
        assert type(again) is type(out)
        free = (want['dur'] < 0).all(0)
        assert (again.dur.cpu().numpy()[:, free] == DR.word(1, 2)).all()
        assert np.array_equal(again.dur.cpu().numpy()[:, ~free], want['dur'][:, ~free])


@pytest.mark.parametrize('fit', ('segment', 'bar', 'beat'))
def test_4_every_fit(fit):
    m = model()
    B = 3
    ones = np.ones((1, 32), dtype=np.uint8)
    row = np.array([DR.fit_row(fit)], dtype=np.uint8)
    want = DR.build(ones, row, ones, B)
    got = m.dur_limits(fit=fit, batch=B)
    assert type(got) is FF_.DurKeep and got.batch == B and not got.err.any().item()
    assert np.array_equal(got.dur.cpu().numpy(), want['dur']) and (got.pitch == -1).all().item()
    # combined: the smallest ceiling, then the floor, which yields
    mx = np.full((1, 32), 5, dtype=np.uint8)
    want = DR.build(np.full((1, 32), 3, np.uint8), np.minimum(row, mx), np.array([[t % 2 for t in range(32)]], np.uint8), B)
    got, y = m.dur_limits(min_dur=3, max_dur=5, fit=fit, steps=range(1, 32, 2), batch=B, return_counts=True)
    assert np.array_equal(got.dur.cpu().numpy(), want['dur']) and np.array_equal(y.cpu().numpy(), want['yielded'])
    assert want['yielded'].sum() == B * sum(1 for t in range(1, 32, 2) if row[0, t] < 3) > 0
    # tensors [32] and [B, 32]
    lo_t = torch.arange(32, device=DEV) % 7
    hi_t = (torch.arange(B * 32, device=DEV).view(B, 32) * 5) % 36
    want = DR.build(lo_t.cpu().numpy()[None].astype(np.uint8), np.minimum(hi_t.cpu().numpy(), row).astype(np.uint8), ones, B)
    got = m.dur_limits(min_dur=lo_t, max_dur=hi_t.to(torch.int32), fit=fit)
    assert got.batch == B and np.array_equal(got.dur.cpu().numpy(), want['dur'])


def test_5_the_rule_on_the_whole_table():
    tab = DR.table()
    extra = [(w, d, p) for w in (-1, -2, -300, -1023, -2048, 0, 1, DR.BASE - (9 | 4 << 5)) for d in range(5) for p in range(1 << d)]
    rows = tab + extra
    a = np.array(rows, dtype=np.int32)
    w, d, p = (dev(np.ascontiguousarray(a[:, i])) for i in range(3))
    out = torch.full((len(rows),), 0x55, dtype=torch.uint8, device=DEV)
    call('ptv_debug_dur_range', ptr(w), ptr(d), ptr(p), len(rows), ptr(out), stream_ptr())
    got = out.cpu().numpy()
    n_det = n_both = 0
    for i, (ww, dd, pp) in enumerate(rows):
        a0, a1 = DR.allowed(ww, dd, pp)
        want = int(a0) | int(a1) << 1
        if ww < 0:
            want |= DR.decide(ww, dd, pp, 0) << 2 | DR.decide(ww, dd, pp, 1) << 3
            assert got[i] == want, (ww, dd, pp, got[i], want)
        else:                                                        # a forced word: the rule leaves it to forced(), which comes after
            assert got[i] == 3 | 0 << 2 | 1 << 3
        n_det += a0 != a1
        n_both += a0 and a1
    assert len(tab) == 528 * 31 and n_det > 1000 and n_both > 1000
    # a d or prefix outside the rule's domain is refused per row, not evaluated
    bad = dev(np.array([[DR.word(0, 31), 5, 0], [DR.word(0, 31), -1, 0], [DR.word(0, 31), 2, 4], [DR.word(0, 31), 2, -1]], dtype=np.int32))
    cols = [bad[:, i].contiguous() for i in range(3)]
    out = torch.zeros(4, dtype=torch.uint8, device=DEV)
    call('ptv_debug_dur_range', ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), 4, ptr(out), stream_ptr())
    assert (out == 0xff).all().item()
