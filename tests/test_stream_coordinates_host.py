"""CPU: the 64-bit coordinates of the sampling noise (seed, draw, sample index g; csrc/philox.hpp sample_words) in the restatement
tests/sample_ref.py / tests/chord_sample_ref.py and in the host words of functional_free, at the limits of their ranges -- what
tests/test_gpu_stream_coordinates.py then holds the device to.  The counter is injective at the field limits, each upper half reaches
every output word, the type of g does not matter, a set of recorded noise values pins the restatement, and the block and the row table
hold the values they were given.  Nothing here touches a GPU."""
import itertools

import numpy as np

import chord_sample_ref as CS
import sample_ref as S
from test_gpu_stream_coordinates import DRAW_HI, OFF_CARRY, OFF_TOP, SEED_HI
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_

GS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 47 - 1, 2 ** 48 - 1)
DRAWS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1)


def test_1_the_counter_is_injective_at_the_field_limits():
    """g x t x n x kind x sub x draw at both ends of every field: 384 calls, 384 different counters; bit 31 of word 3 is always set (the eps
    streams of ptv_philox_normal keep it clear), and every word fits 32 bits"""
    seen = {}
    for draw in DRAWS:
        for kind in (0, 1):
            for g, t, n, sub in itertools.product(GS, (0, 31), (0, 15), (0, 47)):
                c = S.counter(draw, g, t, n, kind, sub)
                assert c.shape == (4,) and c.dtype == np.uint64 and (c < 2 ** 32).all()
                assert int(c[3]) >> 31 == 1
                key = tuple(int(x) for x in c)
                assert key not in seen, ((draw, g, t, n, kind, sub), seen[key])
                seen[key] = (draw, g, t, n, kind, sub)
    assert len(seen) == len(GS) * 2 * 2 * 2 * 2 * len(DRAWS) == 384
    # the fields lie where csrc/philox.hpp says
    c = S.counter(DRAW_HI, 2 ** 47 - 1, 31, 14, 1, 2)
    assert [int(x) for x in c] == [0xFFFFFFFF, (0x7FFF << 16) | (31 << 11) | (14 << 7) | (1 << 6) | 2, 5, 0x80000000 | (2 ** 30 + 1)]
    # ... and words() is Philox of exactly this counter under the key (seed lo, seed hi)
    from oracle.rng_oracle import philox4x32_10
    key = np.array([SEED_HI & 0xFFFFFFFF, SEED_HI >> 32], dtype=np.uint64)
    assert np.array_equal(S.words(SEED_HI, DRAW_HI, 2 ** 47 - 1, 31, 14, 1, 2), philox4x32_10(c, key))


def test_2_each_upper_half_changes_every_word():
    base = dict(seed=11, draw=4, g=5)
    w0 = S.words(base['seed'], base['draw'], base['g'], 31, 14, 0, 47)
    for name in ('seed', 'draw', 'g'):
        for start in (base, dict(seed=SEED_HI - 2 ** 32, draw=DRAW_HI - 2 ** 32, g=OFF_CARRY)):
            kw = dict(start)
            a = S.words(kw['seed'], kw['draw'], kw['g'], 31, 14, 0, 47)
            kw[name] += 2 ** 32
            b = S.words(kw['seed'], kw['draw'], kw['g'], 31, 14, 0, 47)
            assert (a != b).all(), (name, start)
    assert w0.dtype == np.uint32 and w0.shape == (4,)
    # the noise functions see the change too: all three kinds
    for name in ('seed', 'draw', 'g'):
        kw = dict(base)
        kw[name] += 2 ** 32
        assert (S.pitch_noise(kw['seed'], kw['draw'], kw['g'], 31, 14) != S.pitch_noise(11, 4, 5, 31, 14)).mean() > 0.99
        assert (S.dur_noise(kw['seed'], kw['draw'], kw['g'], 31, 14) != S.dur_noise(11, 4, 5, 31, 14)).all()
        assert (CS.noise(kw['seed'], kw['draw'], kw['g'], 7) != CS.noise(11, 4, 5, 7)).mean() > 0.95


def test_3_the_type_of_g_does_not_matter():
    for g in (0, 2 ** 32 - 1, 2 ** 32, OFF_CARRY + 16, 2 ** 47 - 1, 2 ** 47 + 30, 2 ** 48 - 1):
        want = S.words(SEED_HI, DRAW_HI, g, 31, 14, 1, 2)
        for cast in (np.int64, np.uint64):
            assert np.array_equal(S.words(SEED_HI, DRAW_HI, cast(g), 31, 14, 1, 2), want), (g, cast)
            assert np.array_equal(S.words(SEED_HI, DRAW_HI, np.array([g], dtype=cast), 31, 14, 1, 2)[0], want), (g, cast)
            assert np.array_equal(S.pitch_noise(SEED_HI, DRAW_HI, cast(g), 31, 14), S.pitch_noise(SEED_HI, DRAW_HI, g, 31, 14))
            assert np.array_equal(S.dur_noise(SEED_HI, DRAW_HI, cast(g), 31, 14), S.dur_noise(SEED_HI, DRAW_HI, g, 31, 14))
            assert np.array_equal(CS.noise(SEED_HI, DRAW_HI, cast(g), 7), CS.noise(SEED_HI, DRAW_HI, g, 7))
    # a batch that crosses 2^32 is its rows one by one
    g = OFF_CARRY + np.arange(32)
    p, d = S.decode_noise(SEED_HI, DRAW_HI, g)
    for b in (0, 15, 16, 31):
        assert np.array_equal(p[b, 31, 14], S.pitch_noise(SEED_HI, DRAW_HI, int(g[b]), 31, 14))
        assert np.array_equal(d[b, 31, 14], S.dur_noise(SEED_HI, DRAW_HI, int(g[b]), 31, 14))


# Recorded from the restatement as it stood in the parent of the commit that added this file (tests/sample_ref.py,
# tests/chord_sample_ref.py over oracle/rng_oracle.py), at (SEED_HI, DRAW_HI): per g the raw words of the call (t, n, kind, sub) =
# (31, 14, 0, 47) and the fp32 bit patterns of pitch noise columns 0 and 129 and duration noise [bit 0, class 0] and [bit 4, class 1] at
# (t, n) = (31, 14), and of chord noise [lane 0, word 0] and [lane 11, word 3] at t = 7.  The device is compared with the restatement
# (tests/test_gpu_stream_coordinates.py); these constants keep the restatement from drifting together with it.
RECORDED = {
    OFF_CARRY + 15: ((0xa54b54e4, 0xcc9069f6, 0xbc335729, 0x8c483f59), (0x3f383396, 0x3d5330cf), (0x3fd4881d, 0x4043e6a7), (0xbeb86059, 0x3f9e64fc)),
    OFF_CARRY + 16: ((0x2cb0a7c4, 0x8cdc2759, 0x0ddbcc91, 0x55d45bb5), (0xbdd85d87, 0x3fa0336c), (0x3ff849e2, 0x3e8070bf), (0x405b30f5, 0x4040e95c)),
    2 ** 47 - 1: ((0x9fb989c2, 0x2ab3d7df, 0x22f4c29f, 0x3c795ee8), (0xbe9ad91a, 0x400f44eb), (0x3fe3adf2, 0x3db3fdfd), (0x3f7ae582, 0xbf2446dc)),
}


def test_4_recorded_noise_values():
    assert OFF_CARRY + 15 == 2 ** 32 - 1 and OFF_CARRY + 16 == 2 ** 32
    for g, (raw, pitch, dur, chord) in RECORDED.items():
        assert tuple(int(x) for x in S.words(SEED_HI, DRAW_HI, g, 31, 14, 0, 47)) == raw, hex(g)
        p = S.pitch_noise(SEED_HI, DRAW_HI, g, 31, 14)
        d = S.dur_noise(SEED_HI, DRAW_HI, g, 31, 14)
        c = CS.noise(SEED_HI, DRAW_HI, g, 7)
        assert p.dtype == d.dtype == c.dtype == np.float32 and p.shape == (130,) and d.shape == (5, 2) and c.shape == (12, 4)
        assert tuple(int(x) for x in p.view(np.uint32)[[0, 129]]) == pitch, hex(g)
        assert (int(d.view(np.uint32)[0, 0]), int(d.view(np.uint32)[4, 1])) == dur, hex(g)
        assert (int(c.view(np.uint32)[0, 0]), int(c.view(np.uint32)[11, 3])) == chord, hex(g)


def test_5_host_words_at_the_limits():
    w = FF_.sampling_words(1.0, 0.7, SEED_HI, DRAW_HI, OFF_TOP)
    assert len(w) == 4 and w[:3] == [SEED_HI - 2 ** 64, DRAW_HI, OFF_TOP]
    assert w[0] < 0 and np.array([w[0]], dtype=np.int64).view(np.uint64)[0] == SEED_HI
    assert np.array(w[:3], dtype=np.int64).view(np.uint64).tolist() == [SEED_HI, DRAW_HI, OFF_TOP]       # what the device block holds
    assert np.array([w[3]], dtype=np.int64).view(np.float32).tolist() == [1.0, np.float32(0.7)]
    for seed in (2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1):
        assert np.array([FF_.sampling_words(1.0, seed=seed)[0]], dtype=np.int64).view(np.uint64)[0] == seed
    assert FF_.sampling_words(1.0, draw=2 ** 63 - 1, sample_offset=2 ** 47 - 1)[1:3] == [2 ** 63 - 1, 2 ** 47 - 1]
    ids = [2 ** 32 - 100 + 7 * b for b in range(32)]
    assert ids[14] < 2 ** 32 <= ids[15]
    tab = FF_.row_sampling_words(32, 1.0, sample_id=ids)
    assert tab.view(np.int64)[:, 3].tolist() == ids
    assert tab[:, 6].view(np.uint32).tolist() == [i & 0xFFFFFFFF for i in ids] and tab[:, 7].tolist() == [i >> 32 for i in ids]
    # default ids: sample_offset + row with the carry, up to the largest legal id
    assert FF_.row_sampling_words(32, 1.0, sample_offset=OFF_CARRY).view(np.int64)[:, 3].tolist() == [OFF_CARRY + b for b in range(32)]
    assert FF_.row_sampling_words(32, 1.0, sample_offset=OFF_TOP).view(np.int64)[:, 3].tolist()[-1] == 2 ** 47 - 1
