"""CPU: tests/count_limits_ref.py, the restatement of the note-count limits (include/ptvae_hip.h "Note-count limits"), held to a brute-force
statement of the rule for every (F, H, J) with owned and not-owned sources; the room guarantee by replay -- for every L an adversarial
and a random ascending chooser under the allowed rule of top_ref / constrain_ref always reaches L notes, with and without a one-pitch-class
mask --; and the argument surface of build_count_limits as far as it runs without a device (every ValueError comes before any launch,
the composed result types)."""
import numpy as np
import pytest
import torch

import count_limits_ref as CL
import top_ref as TR_
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_

EOS = 129


def brute_word(w, n, F, H, room):
    """word n of a selected step by the definition, one element at a time; w: the source words; F, H clamped"""
    owned = any(v == EOS or v < -1 for v in w)
    if owned or w[n] != -1:
        return w[n]
    forced = [i for i in range(15) if w[i] >= 0]
    J = forced[-1] + 1 if forced else 0
    L, E = min(F, H), max(H, J)
    if n < L:
        return -256 - (128 - (L - 1 - n)) if room else -2
    return EOS if n == E else -1


def sources(J, rng):
    """not-owned sources with a forced prefix of J decisions (one of them with a free gap inside), and owned ones"""
    pre = sorted(rng.choice(128, J, replace=False).tolist())
    plain = pre + [-1] * (15 - J)
    free = [plain]
    if J >= 3:
        gap = list(plain)
        gap[1] = -1                                                    # a decision the keep could not force: still -1, still replaced
        free.append(gap)
    owned = []
    if J < 15:
        owned.append(pre + [EOS] + [-1] * (14 - J))                       # a whole step
        owned.append([-2] * J + [EOS] + [-1] * (14 - J))                  # a rhythm step
        owned.append([-256 - 100] * J + [-1] * (15 - J) if J else [-1] * 14 + [-7])   # BELOW words / a foreign negative word
    else:
        owned.append([-2] * 15)
    return free, owned


def test_reference_against_brute_force():
    rng = np.random.default_rng(11)
    n_checked = 0
    for room in (False, True):
        for F in range(16):
            for H in range(16):
                for J in range(16):
                    free, owned = sources(J, rng)
                    for w in free + owned:
                        new, y, L, H2, E, J2, own = CL.step(w, F, H, room)
                        is_owned = any(w is o for o in owned)
                        assert own == is_owned and H2 == H and L == min(F, H)
                        assert new == [brute_word(w, n, F, H, room) for n in range(15)], (w, F, H, room)
                        if is_owned:
                            assert y == 2 and new == list(w)
                            continue
                        jj = max([i + 1 for i in range(15) if w[i] >= 0], default=0)
                        assert J2 == jj == J and E == max(H, J)
                        assert y & 2 == 0 and bool(y & 1) == (F > H) and bool(y & 4) == (J > H)
                        p = w[J - 1] if J else None
                        assert bool(y & 8) == bool(room and 0 < J < L and p + 1 >= 128 - (L - 1 - J))
                        # what the words mean: exactly one forced <eos> at E (none at 15), nothing but -1 words replaced
                        assert all(new[n] == w[n] for n in range(15) if w[n] != -1)
                        assert [n for n in range(15) if new[n] == EOS] == ([E] if E <= 14 and w[E] == -1 else [])
                        n_checked += 1
    assert n_checked > 2 * 16 * 16 * 16


def test_builder_rows_clamping_and_selection():
    B = 5
    rng = np.random.default_rng(3)
    lo = rng.integers(0, 20, (B, 32)).astype(np.uint8)
    hi = rng.integers(0, 20, (1, 32)).astype(np.uint8)
    lo[0, 0], hi[0, 0] = 255, 200                                         # clamped to 15 / 15: no ceiling, fifteen floor words
    steps = (rng.random((B, 32)) < 0.7).astype(np.uint8)
    steps[:, 0] = 1
    for room in (False, True):
        r = CL.build(lo, hi, steps, B, room=room)
        words = CL.words_of(r['pitch'])
        assert (r['dur'] == -1).all()
        for b in range(B):
            for t in range(32):
                if not steps[b, t]:
                    assert (words[b, t] == -1).all() and r['yielded'][b, t] == 0 and r['L'][b, t] == -1
                    continue
                F, H = min(int(lo[b, t]), 15), min(int(hi[0, t]), 15)
                assert words[b, t].tolist() == [brute_word([-1] * 15, n, F, H, room) for n in range(15)]
                assert r['yielded'][b, t] == int(F > H) and (r['L'][b, t], r['H'][b, t], r['E'][b, t], r['J'][b, t]) == (min(F, H), H, H, 0)
        assert (words[0, 0] != -1).all() and EOS not in words[0, 0] and r['yielded'].sum() > 0
    # built into arrays: the duration words and every foreign pitch word survive
    R = 32 * B
    src_p = np.full((15, R), -1, dtype=np.int32)
    src_p[:3, ::2] = rng.integers(0, 128, (3, (R + 1) // 2))
    src_p[3, ::4] = EOS
    src_d = rng.integers(-1100, 2, (5, 15 * R)).astype(np.int32)
    r = CL.build(lo, hi, steps, B, src_p, src_d, room=True)
    assert np.array_equal(r['dur'], src_d) and np.array_equal(r['pitch'][src_p != -1], src_p[src_p != -1])
    assert r['owned'].any() and (r['yielded'][r['owned']] == 2).all() and (r['yielded'] & 4).any()


def choose(al, kind, rng):
    notes = [c for c in range(128) if al[c]]
    if not notes:
        assert al[EOS]
        return EOS
    if kind == 'highest':                                                 # the adversary: climb as fast as the rule lets it
        return notes[-1]
    if kind == 'eos-first' and al[EOS]:                                   # end the step as soon as the rule lets it
        return EOS
    return int(rng.choice(notes + ([EOS] if al[EOS] else [])))


@pytest.mark.parametrize('masked', (False, True))
def test_room_guarantee(masked):
    """room=True under `ascending`: whatever an ascending chooser picks inside the allowed set, the step reaches L notes and holds at
    most H; with a mask of one pitch class the mask yields where it must, never the count.  Without room the adversary falls short."""
    rng = np.random.default_rng(29)
    mask_row = [(p % 12) == 7 for p in range(128)] if masked else None
    short_without_room = 0
    for L in range(16):
        for H in sorted({L, min(L + 2, 15), 15}):
            for room in (True, False):
                words, y = CL.step([-1] * 15, L, H, room)[:2]
                assert y == 0
                for kind in ('highest', 'eos-first', 'random', 'random', 'random'):
                    lo, count = -1, 0
                    for n in range(15):
                        if words[n] == EOS:
                            break
                        al, relaxed, empty = TR_.allowed_row(mask_row, lo, True, words[n])
                        c = choose(al, kind, rng)
                        if c == EOS:
                            break
                        assert c > lo
                        lo, count = c, count + 1
                        if room and n < L:
                            assert not empty and c <= 128 - L + n
                    assert count <= H
                    if room:
                        assert count >= L, (L, H, kind, masked, count)
                    elif count < L:
                        short_without_room += 1
    assert short_without_room > 0


def test_surface_without_a_device():
    f = FF_.build_count_limits
    for bad in (dict(device='cpu', max_count=3, batch=2), dict(max_count=16), dict(min_count=-1), dict(min_count=True), dict(max_count=2.0),
                dict(max_count='4'), dict(min_count=torch.zeros(32, dtype=torch.int32)), dict(max_count=3, batch=0), dict(max_count=3, batch=True),
                dict(max_count=3, batch=2.5), dict(max_count=3, room=1), dict(max_count=3, room=None), dict(max_count=3, steps=[32]),
                dict(max_count=3, steps=7), dict(max_count=3, onsets=[-1]), dict(max_count=3, rests=[0.5]), dict(max_count=3, keep=(1, 2, 3, 4)),
                dict(steps=range(4)), dict(batch=4), dict(max_count=3, steps=torch.ones(1, 32, dtype=torch.bool)),
                dict(rests=torch.ones(2, 32, dtype=torch.uint8)), dict(max_count=3), dict(onsets=[0, 4], rests=[2])):
        kw = dict(dict(device='cuda'), **bad)
        if 'batch' not in kw and bad not in (dict(max_count=3), dict(onsets=[0, 4], rests=[2])):
            kw['batch'] = 2
        with pytest.raises(ValueError):
            f(**kw)


def test_result_types_compose():
    T = FF_._limits_keep_type
    mk = lambda cls: cls(None, None, None, 1)
    # what existed stays exactly what it was
    assert T(None, FF_.DurKeep) is FF_.DurKeep and T(mk(FF_.Keep), FF_.DurKeep) is FF_.DurKeep
    assert T(mk(FF_.RhythmKeep), FF_.DurKeep) is FF_.RhythmDurKeep and T(mk(FF_.TopKeep), FF_.DurKeep) is FF_.TopDurKeep
    for cls in (FF_.DurKeep, FF_.RhythmDurKeep, FF_.TopDurKeep):
        assert T(mk(cls), FF_.DurKeep) is cls
    # a ceiling-only count limit adds nothing
    for cls in (FF_.Keep, FF_.RhythmKeep, FF_.TopKeep, FF_.DurKeep, FF_.CountKeep):
        assert T(mk(cls), None) is cls
    assert T(None, None) is FF_.Keep
    # a floor
    assert T(None, FF_.CountKeep) is FF_.CountKeep and FF_.CountKeep.needs_constrained and not FF_.CountKeep.needs_ascending
    room = T(None, FF_.CountKeep, True)
    assert issubclass(room, FF_.CountKeep) and room.needs_constrained and room.needs_ascending and room is T(None, FF_.CountKeep, True)
    # unions, in either order
    for have, asc in ((FF_.RhythmKeep, False), (FF_.TopKeep, True), (FF_.DurKeep, False), (FF_.TopDurKeep, True), (FF_.RhythmDurKeep, False)):
        for r in (False, True):
            c = T(mk(have), FF_.CountKeep, r)
            assert issubclass(c, have) and issubclass(c, FF_.CountKeep) and c.needs_constrained and c.needs_ascending == (asc or r)
            assert c._fields == FF_.Keep._fields and T(mk(c), FF_.CountKeep, r) is c and T(mk(c), None) is c
            d = T(mk(c), FF_.DurKeep)
            assert issubclass(d, FF_.DurKeep) and issubclass(d, FF_.CountKeep) and d.needs_ascending == (asc or r)
    a = T(mk(T(None, FF_.CountKeep, True)), FF_.DurKeep)
    b = T(mk(FF_.DurKeep), FF_.CountKeep, True)
    assert a.needs_ascending and b.needs_ascending and a.needs_constrained and b.needs_constrained
    k = b(1, 2, 3, 4)
    assert isinstance(k, FF_.Keep) and type(k)(*k) == k and k.batch == 4
