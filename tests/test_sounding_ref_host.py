"""CPU: tests/sounding_ref.py, the numpy restatement of the sounding state (include/ptvae_hip.h "Sounding state"), against a brute-force
definition on an explicit [32, 128] "which onset sounds here" roll; the count words against count_limits_ref.build fed F' and H'."""
import numpy as np

import count_limits_ref as CL
import sounding_ref as SR

B = 6


def brute_held(grid_row, s1):
    """the pitches that sound at step s1 from onsets at steps < s1: every accepted onset, in step and slot order, first silences its
    key from its step on and then holds it down for its duration"""
    roll = [[None] * 128 for _ in range(32)]
    for s in range(s1):
        notes = []
        for j in range(1, 16):
            p = int(grid_row[s, j, 0])
            if p == 129:
                break
            if 0 <= p <= 127:
                d = 1 + int(''.join(str(int(v) & 1) for v in grid_row[s, j, 1:6]), 2)
                notes.append((j, p, d))
        for j, p, d in notes:
            for t in range(s, 32):
                roll[t][p] = None
            for t in range(s, min(s + d, 32)):
                roll[t][p] = (s, j)
    return [p for p in range(128) if roll[s1][p] is not None]


def tables(seed):
    rng = np.random.default_rng(seed)
    K = rng.integers(0, 9, (B, 32)).astype(np.uint8)
    F = rng.integers(0, 6, (B, 32)).astype(np.uint8)
    steps = (rng.random((B, 32)) < 0.7).astype(np.uint8)
    mask = rng.integers(-2 ** 31, 2 ** 31, (B, 32, 4)).astype(np.int32)
    force = np.full((15, 32 * B), -1, dtype=np.int32)
    for r in range(32 * B):
        kind = rng.integers(0, 5)
        if kind == 1:                                            # a forced prefix
            for n in range(int(rng.integers(1, 6))):
                force[n, r] = 40 + 2 * n
        elif kind == 2:                                          # an owned step: a forced <eos>
            force[int(rng.integers(0, 15)), r] = 129
        elif kind == 3:                                          # an owned step: a word of the constrained kind
            force[0, r] = -2
    K[0, 0], F[0, 0], steps[0, 0] = 2, 5, 1                      # nothing is held at step 0: a floor over its ceiling
    force[:, 0] = -1
    return K, F, steps, mask, force


def test_grids_hold_what_the_parse_has_rules_for():
    x = SR.random_grids(B, 1)
    slots = x[:, :, 1:, 0]
    assert (slots == 128).any() and (slots == 130).any()
    first_eos = np.where((slots == 129).any(2), (slots == 129).argmax(2), 15)
    assert (first_eos == 0).any() and (first_eos == 15).any()                      # rests and 15-note steps with no <eos>
    twice = overhang = False
    for b in range(B):
        for s in range(32):
            notes = SR.accepted(x[b, s], s)
            ps = [p for p, _ in notes]
            twice |= len(set(ps)) < len(ps)
            for j in range(1, 16):
                if x[b, s, j, 0] == 129:
                    break
                if 0 <= x[b, s, j, 0] <= 127:
                    overhang |= 1 + int(''.join(str(int(v) & 1) for v in x[b, s, j, 1:6]), 2) > 32 - s
            assert all(1 <= d <= 32 - s for _, d in notes)
    assert twice and overhang
    assert SR.accepted(x[0, 0], 0) == [(0, 32), (127, 1), (0, 3)]


def test_held_set_is_the_brute_force_roll():
    x = SR.random_grids(B, 2)
    got = SR.run(x, B)
    assert (got['held'][:, 0] == 0).all() and (got['held'] > 0).any()
    for b in range(B):
        rem = [0] * 128
        for s1 in range(32):
            if s1 > 0:
                rem = SR.advance(rem, SR.accepted(x[b, s1 - 1], s1 - 1))
            want = brute_held(x[b], s1)
            assert [p for p in range(128) if rem[p] > 0] == want, (b, s1)
            assert got['held'][b, s1] == len(want)
    # the later onset wins, shorter or not: pitch 0 of row 0 struck with 32 and then with 3 in one step is free again at step 3
    assert 0 in brute_held(x[0], 1) and 0 in brute_held(x[0], 2)
    if not any(p == 0 for s in (1, 2) for p, _ in SR.accepted(x[0, s], s)):
        assert 0 not in brute_held(x[0], 3)


def test_effective_arrays_follow_the_definition():
    x = SR.random_grids(B, 3)
    K, F, steps, mask, force = tables(4)
    for no_restrike in (False, True):
        got = SR.run(x, B, no_restrike, K, F, steps, mask, force)
        Hp, Fp = np.zeros((B, 32), np.uint8), np.zeros((B, 32), np.uint8)
        for b in range(B):
            for s in range(32):
                H = brute_held(x[b], s)
                h = len(H)
                Hp[b, s] = 15 if K[b, s] == 0 else min(max(int(K[b, s]) - h, 0), 15)
                Fp[b, s] = min(max(int(F[b, s]) - h, 0), 15)
                assert (got['Hc'][b, s], got['Fc'][b, s]) == (Hp[b, s], Fp[b, s])
                for p in range(128):
                    base = (int(mask[b, s, p >> 5]) >> (p & 31)) & 1
                    bit = (int(got['mask_eff'][b, s, p >> 5]) >> (p & 31)) & 1
                    assert bit == (0 if (no_restrike and steps[b, s] and p in H) else base), (b, s, p)
        # the count words: ptv_note_count_force_build's rule fed F' and H'
        want = CL.build(Fp, Hp, steps, B, force, None, room=False)
        assert np.array_equal(got['force_eff'], want['pitch'])
        assert want['owned'].any() and (want['J'] > want['H']).any() and (want['yielded'] & 1).any()
        unsel = np.repeat((steps == 0).T.reshape(1, 32 * B), 15, 0)
        assert np.array_equal(got['force_eff'][unsel], force[unsel])
    # nothing selected, or no rule: the base arrays
    none = SR.run(x, B, True, K, F, np.zeros((1, 32), np.uint8), mask, force)
    assert np.array_equal(none['mask_eff'], mask) and np.array_equal(none['force_eff'], force)
    off = SR.run(x, B, False, None, None, None, mask[:1], force)
    assert np.array_equal(off['mask_eff'], np.repeat(mask[:1], B, 0)) and np.array_equal(off['force_eff'], force)
    assert np.array_equal(off['held'], none['held'])


def test_onsets_plus_held_stay_under_the_cap():
    """by construction: a step the keep does not own with J <= H' ends after at most H' = K - h notes"""
    x = SR.random_grids(B, 5)
    K = np.full((1, 32), 4, np.uint8)
    got = SR.run(x, B, K=K)
    words = CL.words_of(got['force_eff'])
    for b in range(B):
        for s in range(32):
            h = int(got['held'][b, s])
            E = min(max(4 - h, 0), 15)
            assert words[b, s, E] == 129 and (np.delete(words[b, s], E) == -1).all()
    partial = SR.run(x, B, K=K, upto=7)
    assert np.array_equal(partial['force_eff'][:, :8 * B], got['force_eff'][:, :8 * B]) and (partial['force_eff'][:, 8 * B:] == -1).all()
    assert np.array_equal(partial['held'][:, :8], got['held'][:, :8]) and (partial['held'][:, 8:] == 0).all()
