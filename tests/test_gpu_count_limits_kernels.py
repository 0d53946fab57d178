"""GPU: the builder of the note-count limits (include/ptvae_hip.h "Note-count limits") against tests/count_limits_ref.py:
ptv_note_count_force_build element for element at B = 1, 5 and 32 with one row and B rows of floors / ceilings / selections, with and
without the room flag, floors above their ceilings, ceilings 0 and 15, bytes above 15 (clamped); built into a whole, voice, rhythm and top
keep and into a dur_limits keep (foreign words survive bit for bit, owned steps are copied); count_limits and dur_limits in either order
give identical arrays; every PTV_ERR_ARG case writes nothing."""
import functools

import numpy as np
import pytest
import torch

import count_limits_ref as CL
import test_gpu_keep_decode as KD
import test_gpu_truncated_sampling as TT
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = KD.DEV
SENT = -77                                                         # no kernel writes it: it is no force word, yielded is 0..15
EOS = 129


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def gpu_build(lo, hi, steps, B, src=None, room=False):
    out = dict(pitch=torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV),
               dur=torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV),
               yielded=torch.full((B, 32), SENT, dtype=torch.int32, device=DEV))
    l, h, s = dev(lo), dev(hi), dev(steps)
    sp, sd = (None, None) if src is None else (dev(src[0]), dev(src[1]))
    call('ptv_note_count_force_build', ptr(l), lo.shape[0], ptr(h), hi.shape[0], ptr(s), steps.shape[0], ptr(sp), ptr(sd), 1 if room else 0,
         B, ptr(out['pitch']), ptr(out['dur']), ptr(out['yielded']), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def limits(B):
    """floors / ceilings as bytes 0..19 (above 15: clamped), some 255, a selection of about three steps in four; in every batch a floor
    above its ceiling, a rest (H = 0) and no ceiling (H = 15) at selected steps"""
    rng = np.random.default_rng(700 + B)
    lo = rng.integers(0, 20, (B, 32)).astype(np.uint8)
    hi = rng.integers(0, 20, (B, 32)).astype(np.uint8)
    steps = (rng.random((B, 32)) < 0.75).astype(np.uint8)
    lo[0, 3], hi[0, 3], steps[0, 3] = 9, 4, 1
    lo[0, 4], hi[0, 4], steps[0, 4] = 9, 4, 0                        # ... and at a step that is not selected: not reported
    lo[0, 5], hi[0, 5], steps[0, 5] = 2, 0, 1
    lo[0, 6], hi[0, 6], steps[0, 6] = 3, 15, 1
    lo[0, 7], hi[0, 7], steps[0, 7] = 255, 255, 1
    for a in (lo, hi, steps):
        a.setflags(write=False)
    return lo, hi, steps


@pytest.mark.parametrize('B', (1, 5, 32))
def test_1_builder_matches_the_reference(B):
    lo, hi, steps = limits(B)
    for room in (False, True):
        for rl in (1, B):
            for rh in (1, B):
                for rs in (1, B):
                    a, b, c = (np.ascontiguousarray(v[:r]) for v, r in ((lo, rl), (hi, rh), (steps, rs)))
                    want = CL.build(a, b, c, B, room=room)
                    got = gpu_build(a, b, c, B, room=room)
                    for k in ('pitch', 'dur', 'yielded'):
                        assert np.array_equal(got[k], want[k]), (k, room, rl, rh, rs)
                    assert (got['dur'] == -1).all()
        want = CL.build(lo, hi, steps, B, room=room)
        w = CL.words_of(want['pitch'])[0]
        assert want['yielded'][0, 3] == 1 and want['yielded'][0, 4] == 0 and (w[4] == -1).all()
        assert w[3, 4] == EOS and (w[3, 5:] == -1).all()                                                     # the ceiling won: 4 notes
        assert w[3, :4].tolist() == ([CL.below(125 + n) for n in range(4)] if room else [-2] * 4)
        assert w[5, 0] == EOS and (w[5, 1:] == -1).all()                                                     # a rest
        assert EOS not in w[6] and (w[6, 3:] == -1).all() and (w[6, :3] < -1).all()                          # no ceiling
        assert (w[7] < -1).all() and want['yielded'][0, 7] == 0                                              # 255: fifteen notes
        if room:
            assert w[7].tolist() == [CL.below(114 + n) for n in range(15)]


def test_2_arguments():
    lo, hi, steps = limits(5)
    l, h, s = dev(lo), dev(hi), dev(steps)
    p, d, y = (torch.full((n,), SENT, dtype=torch.int32, device=DEV) for n in (15 * 160, 5 * 2400, 160))
    sp, sd = torch.full((15 * 160,), -1, dtype=torch.int32, device=DEV), torch.full((5 * 2400,), -1, dtype=torch.int32, device=DEV)
    f = lib().ptv_note_count_force_build
    ok = [ptr(l), 5, ptr(h), 5, ptr(s), 5, ptr(sp), ptr(sd), 1, 5, ptr(p), ptr(d), ptr(y), stream_ptr()]
    cases = [(0, None), (2, None), (4, None), (10, None), (11, None), (12, None), (1, 2), (3, 4), (5, 0), (9, 0), (9, -3), (8, 2), (8, -1),
             (6, None), (7, None), (6, ptr(p)), (7, ptr(d))]
    for i, v in cases:
        bad = list(ok)
        bad[i] = v
        assert f(*bad) != 0, i
    bad = list(ok)
    bad[6], bad[7] = ptr(p), ptr(d)                                   # the outputs as their own source
    assert f(*bad) != 0
    torch.cuda.synchronize()
    for o in (p, d, y):
        assert (o == SENT).all().item()                               # a refused call wrote nothing
    assert f(*ok) == 0
    ok[6] = ok[7] = None
    assert f(*ok) == 0
    torch.cuda.synchronize()
    assert not (p == SENT).any().item() and not (d == SENT).any().item() and not (y == SENT).any().item()


@functools.lru_cache(maxsize=None)
def model():
    return TT.model()


def keeps(B):
    """(name, keep) built from the crafted grid: forced pitches, forced duration bits, -2 and -256 - u words, range words"""
    m = model()
    x = dev(np.ascontiguousarray(KD.crafted()[0][[i % 32 for i in range(B)]]))
    sel = [t for t in range(32) if t % 3 != 2]
    return (('whole', m.keep(x, sel)), ('voice', m.keep_voice(x, sel, lowest=2)), ('voice-below', m.keep_voice(x, sel, below=60, durations=False)),
            ('rhythm', m.keep_rhythm(x, sel, durations=False, whole_steps=[0, 1])), ('top', m.keep_top(x, sel, durations='kept')),
            ('dur', m.dur_limits(min_dur=2, fit='bar', batch=B)), ('voice-dur', m.dur_limits(max_dur=4, keep=m.keep_voice(x, sel, lowest=3))))


@pytest.mark.parametrize('B', (5, 32))
def test_3_built_into_a_keep(B):
    m = model()
    lo, hi, steps = limits(B)
    seen = 0
    for name, keep in keeps(B):
        sp, sd = keep.pitch.cpu().numpy(), keep.dur.cpu().numpy()
        for room in (False, True):
            want = CL.build(lo, hi, steps, B, sp, sd, room=room)
            got = gpu_build(lo, hi, steps, B, (sp, sd), room=room)
            for k in ('pitch', 'dur', 'yielded'):
                assert np.array_equal(got[k], want[k]), (name, room, k)
            foreign = sp != -1
            assert np.array_equal(got['pitch'][foreign], sp[foreign]) and np.array_equal(got['dur'], sd)
            own = np.repeat(want['owned'].T.reshape(1, 32 * B), 15, 0)          # [15, 32 B] in the arrays' (t, b) order
            assert np.array_equal(got['pitch'][own], sp[own])
            assert ((want['yielded'] & 2) != 0).tolist() == want['owned'].tolist()
            seen |= int(np.bitwise_or.reduce(want['yielded'].ravel()))
            if name in ('whole', 'rhythm', 'top'):
                assert want['owned'].any()
            if name.startswith('voice'):
                assert (want['J'] > 0).any() and not want['owned'].any()
            # through the model: the same arrays, the demands are the union
            out, y = m.count_limits(min_count=dev(lo), max_count=dev(hi), steps=dev(steps), room=room, keep=keep, return_counts=True)
            assert np.array_equal(out.pitch.cpu().numpy(), want['pitch']) and np.array_equal(out.dur.cpu().numpy(), want['dur'])
            assert np.array_equal(y.cpu().numpy(), want['yielded']) and out.err is keep.err and out.batch == B
            assert isinstance(out, FF_.CountKeep) and isinstance(out, type(keep)) and out.needs_constrained
            assert out.needs_ascending == (room or keep.needs_ascending)
            cap = m.count_limits(max_count=dev(hi), steps=dev(steps), keep=keep)        # no floor: it stays what it is
            assert type(cap) is type(keep)
            assert np.array_equal(cap.pitch.cpu().numpy(), CL.build(np.zeros((1, 32), np.uint8), hi, steps, B, sp, sd)['pitch'])
    assert seen & 1 and seen & 2 and seen & 4


def test_4_room_over_a_kept_voice_raises_bit_3():
    """a forced prefix that ends so high that the semitones above it cannot hold the floor: bit 3; one that leaves room: not"""
    B = 5
    sp = np.full((15, 32 * B), -1, dtype=np.int32)
    sd = np.full((5, 480 * B), -1, dtype=np.int32)
    sp[0, :] = 60
    sp[1, 0::2] = 126                                                  # (t, b) rows 0, 2, 4, ...: the voice ends on 126
    sp[1, 1::2] = 70
    lo, hi, steps = (np.full((1, 32), v, dtype=np.uint8) for v in (5, 8, 1))
    want = CL.build(lo, hi, steps, B, sp, sd, room=True)
    got = gpu_build(lo, hi, steps, B, (sp, sd), room=True)
    for k in ('pitch', 'dur', 'yielded'):
        assert np.array_equal(got[k], want[k]), k
    y = got['yielded'].T.reshape(-1)                                   # in (t, b) order
    assert (y[0::2] == 8).all() and (y[1::2] == 0).all()
    assert not (gpu_build(lo, hi, steps, B, (sp, sd), room=False)['yielded']).any()


def test_5_count_and_dur_limits_in_either_order():
    m = model()
    B = 5
    lo, hi, steps = limits(B)
    x = dev(np.ascontiguousarray(KD.crafted()[0][:B]))
    for base in (None, m.keep_voice(x, range(0, 32, 2), lowest=2), m.keep_rhythm(x, range(8))):
        for room in (False, True):
            ckw = dict(min_count=dev(lo), max_count=dev(hi), steps=dev(steps), room=room)
            dkw = dict(min_dur=2, max_dur=6, steps=range(4, 32))
            if base is None:
                a = m.dur_limits(keep=m.count_limits(**ckw), **dkw)
                b = m.count_limits(keep=m.dur_limits(batch=B, **dkw), **ckw)
            else:
                a = m.dur_limits(keep=m.count_limits(keep=base, **ckw), **dkw)
                b = m.count_limits(keep=m.dur_limits(keep=base, **dkw), **ckw)
            assert torch.equal(a.pitch, b.pitch) and torch.equal(a.dur, b.dur)
            assert (a.dur < -1000).any().item() and (a.pitch < -1).any().item()
            for k in (a, b):
                assert isinstance(k, FF_.CountKeep) and isinstance(k, FF_.DurKeep) and k.needs_constrained
                assert k.needs_ascending == room and (base is None or isinstance(k, type(base)))
