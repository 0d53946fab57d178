"""CPU: the numpy restatement of the row-independent chord decode (tests/chord_sample_ref.py) on hand-made cases -- the noise slot, ties to the
lowest index, the keep rule with its invalid blocks, T = 0 and forced decisions giving logq = 0, the two log-probabilities against the
textbook formula, the fold -- and the host-side validation of the chord keywords (no GPU, no launch)."""
import numpy as np
import pytest
import torch

import chord_sample_ref as CS
import sample_ref as S
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M


def onehot(i):
    v = np.zeros(12, np.float32)
    v[i] = 1
    return v


def chord(r, bits, b):
    return np.concatenate([onehot(r), np.asarray(bits, np.float32), onehot(b)])


def test_noise_is_the_n15_slot_of_the_decoders_domain():
    nz = CS.noise(11, 4, np.array([0, 5, 1 << 33]), 6)
    assert nz.shape == (3, 12, 4) and nz.dtype == np.float32
    for i, g in enumerate((0, 5, 1 << 33)):
        for j in (0, 7, 11):
            w = S.words(11, 4, g, 6, 15, 0, j)
            assert np.array_equal(nz[i, j], S.gumbel_from_word(w))
    full = CS.decode_noise(11, 4, [3, 4])
    assert full.shape == (2, 8, 12, 4) and np.array_equal(full[1, 6], CS.noise(11, 4, 4, 6))
    # no note decision shares a word with it: the pitch words of n = 0..14 at the same (g, t) are other Philox calls
    pitch = S.pitch_noise(11, 4, 5, 6, np.arange(15))
    assert not np.isin(nz[1].ravel(), pitch.ravel()).any()
    r, b, c = CS.split(nz)
    assert np.array_equal(r, nz[..., 0]) and np.array_equal(b, nz[..., 1]) and np.array_equal(c, nz[..., 2:])


def test_ties_go_to_the_lowest_index_at_temperature_zero():
    root = np.array([[1, 3, 3, 0, 3, 0, 0, 0, 0, 0, 0, 0], [2] * 12], np.float32)
    bass = np.array([[0] * 11 + [5], [-1, -1, 4, 4, -1, -1, -1, -1, -1, -1, -1, 4]], np.float32)
    chroma = np.zeros((2, 12, 2), np.float32)
    chroma[0, 3] = (1, 2)
    chroma[0, 4] = (2, 2)                                    # a tied pair is class 0
    chroma[1, 0] = (-3, -2.5)
    nz = CS.noise(1, 0, [0, 1], 0)
    for noise, T in ((None, 0.0), (nz, 0.0)):                # without a block and with T = 0 the noise does not enter
        d = CS.decide(root, chroma, bass, noise, T, T)
        assert d['root'].tolist() == [1, 0] and d['bass'].tolist() == [11, 2]
        assert d['bits'][0].tolist() == [0, 0, 0, 1] + [0] * 8 and d['bits'][1].tolist() == [1] + [0] * 11
        assert not d['forced'].any() and not d['err'].any()
    c, c14 = CS.tokens(d['root'], d['bits'], d['bass'])
    assert c.shape == (2, 36) and c14.shape == (2, 14)
    assert np.array_equal(c[0], chord(1, d['bits'][0], 11)) and c14[0].tolist() == [1] + d['bits'][0].tolist() + [11]


def test_sampled_decisions_follow_the_perturbed_logits():
    rng = np.random.RandomState(3)
    root, bass, chroma = rng.normal(0, 1, (40, 12)), rng.normal(0, 1, (40, 12)), rng.normal(0, 1, (40, 12, 2))
    nz = CS.noise(5, 2, np.arange(40), 3)
    d = CS.decide(root, chroma, bass, nz, 1.0, 0.5)
    r32, b32, c32 = (a.astype(np.float32) for a in (root, bass, chroma))
    assert np.array_equal(d['root'], np.argmax(r32 + np.float32(1.0) * nz[..., 0], -1))
    assert np.array_equal(d['bass'], np.argmax(b32 + np.float32(1.0) * nz[..., 1], -1))
    x = c32 + np.float32(0.5) * nz[..., 2:]
    assert np.array_equal(d['bits'], (x[..., 1] > x[..., 0]).astype(np.int64))
    assert (d['root'] != np.argmax(r32, -1)).any()           # the noise matters
    d0 = CS.decide(root, chroma, bass, nz, 1.0, 0.0)         # chroma at T = 0 is its argmax
    assert np.array_equal(d0['bits'], (c32[..., 1] > c32[..., 0]).astype(np.int64)) and np.array_equal(d0['root'], d['root'])


def test_keep_forces_and_invalid_blocks_stay_free():
    rng = np.random.RandomState(4)
    root, bass, chroma = rng.normal(0, 1, (5, 12)), rng.normal(0, 1, (5, 12)), rng.normal(0, 1, (5, 12, 2))
    bits = [1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0]
    keep = np.stack([chord(9, bits, 4)] * 5)
    keep[1, 0:12] = 0                                        # root block all zero
    keep[2, 24:36] = 0
    keep[2, [25, 30]] = 1                                    # bass block with two ones
    keep[3, 9] = -2.5                                        # any non-zero entry counts
    keep[3, 12:24] = [0.5, 0, 0, 0, -1, 0, 0, 3, 0, 0, 0, 0]
    keep[4] = np.nan                                         # not kept: never looked at
    kept = np.array([True, True, True, True, False])
    free = CS.decide(root, chroma, bass, None, 0, 0)
    d = CS.decide(root, chroma, bass, None, 0, 0, keep, kept)
    assert d['root'].tolist() == [9, free['root'][1], 9, 9, free['root'][4]]
    assert d['bass'].tolist() == [4, 4, free['bass'][2], 4, free['bass'][4]]
    assert all(d['bits'][i].tolist() == bits for i in range(4)) and np.array_equal(d['bits'][4], free['bits'][4])
    assert d['forced'].tolist() == [[1, 12, 1], [0, 12, 1], [1, 12, 0], [1, 12, 1], [0, 0, 0]]
    assert d['err'].tolist() == [0, 1, 1, 0, 0]
    fr, fbits, fb, err = CS.forced(keep, kept)
    assert fr.tolist() == [9, -1, 9, 9, -1] and fb.tolist() == [4, 4, -1, 4, -1] and err.tolist() == [0, 1, 1, 0, 0]
    # a forced decision ignores logits and noise
    nz = CS.noise(1, 1, np.arange(5), 2)
    dn = CS.decide(root * 50, chroma * 50, bass * 50, nz, 2.0, 2.0, keep, kept)
    assert dn['root'][[0, 2, 3]].tolist() == [9, 9, 9] and dn['bass'][[0, 1, 3]].tolist() == [4, 4, 4]
    assert all(dn['bits'][i].tolist() == bits for i in range(4))
    # a one-row step pattern serves every row
    d1 = CS.decide(root[:4], chroma[:4], bass[:4], None, 0, 0, keep[:4], np.array([True]))
    assert np.array_equal(d1['forced'], d['forced'][:4])


def textbook(v, d):
    v = np.asarray(v, np.float64)
    return np.take_along_axis(v - np.log(np.exp(v).sum(-1, keepdims=True)), np.asarray(d)[..., None], -1)[..., 0]


def test_logp_and_logq_are_the_log_softmax_at_the_decided_class():
    rng = np.random.RandomState(5)
    root, bass, chroma = (rng.normal(0, 2, s).astype(np.float32) for s in ((30, 12), (30, 12), (30, 12, 2)))
    nz = CS.noise(2, 0, np.arange(30), 1)
    Tc, Th = 1.3, 0.7
    d = CS.decide(root, chroma, bass, nz, Tc, Th)
    lp, lq, sp, sq = CS.logprob(root, chroma, bass, d, Tc, Th)
    assert lp.shape == lq.shape == sp.shape == sq.shape == (30, 3)
    np.testing.assert_allclose(lp[:, 0], textbook(root, d['root']), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lp[:, 2], textbook(bass, d['bass']), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lp[:, 1], textbook(chroma, d['bits']).sum(-1), rtol=0, atol=1e-12)
    t32 = lambda T: np.float64(np.float32(T))
    np.testing.assert_allclose(lq[:, 0], textbook(root.astype(np.float64) / t32(Tc), d['root']), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lq[:, 2], textbook(bass.astype(np.float64) / t32(Tc), d['bass']), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lq[:, 1], textbook(chroma.astype(np.float64) / t32(Th), d['bits']).sum(-1), rtol=0, atol=1e-12)
    assert (lp <= 0).all() and (lq <= 0).all() and (sp > 0).all()
    # the fp32 evaluation in the kernel's term order stays within fp32 rounding of it
    f_lp, f_lq, _, _ = CS.logprob(root, chroma, bass, d, Tc, Th, dtype=np.float32)
    assert f_lp.dtype == np.float32 and f_lq.dtype == np.float32
    assert np.abs(f_lp - lp).max() < 2e-5 and np.abs(f_lq - lq).max() < 2e-5
    # the rotation tree of the kernel's 16-lane sum, spelled out for one row
    e = np.concatenate([np.exp(root[0] - root[0].max()).astype(np.float32), np.zeros(4, np.float32)])
    for r in (8, 4, 2, 1):
        e = e + np.roll(e, r)
    want = np.float32(root[0][d['root'][0]] - root[0].max()) - np.log(e[0]).astype(np.float32)
    assert f_lp[0, 0] == want and np.all(e == e[0])


def test_logq_is_zero_at_temperature_zero_and_for_forced_decisions():
    rng = np.random.RandomState(6)
    root, bass, chroma = (rng.normal(0, 2, s).astype(np.float32) for s in ((6, 12), (6, 12), (6, 12, 2)))
    nz = CS.noise(2, 0, np.arange(6), 0)
    d = CS.decide(root, chroma, bass, nz, 1.0, 0.0)
    lp, lq, _, sq = CS.logprob(root, chroma, bass, d, 1.0, 0.0)
    assert (lq[:, 1] == 0).all() and (sq[:, 1] == 0).all() and (lq[:, [0, 2]] < 0).all() and (lp < 0).all()
    _, lq0, _, _ = CS.logprob(root, chroma, bass, d, 1.0, 0.5, sampled=False)                # no block: the argmax is certain
    assert (lq0 == 0).all()
    keep = np.stack([chord(2, [1] * 12, 7)] * 6)
    keep[1, 0:12] = 0                                        # its root stays free: it keeps its logq
    kept = np.array([True, True, False, False, False, False])
    dk = CS.decide(root, chroma, bass, nz, 1.0, 0.5, keep, kept)
    lpk, lqk, _, _ = CS.logprob(root, chroma, bass, dk, 1.0, 0.5)
    assert (lqk[0] == 0).all() and lqk[1, 0] < 0 and lqk[1, 1] == 0 and lqk[1, 2] == 0 and (lqk[2:] < 0).all()
    assert np.isfinite(lpk).all() and (lpk < 0).all()       # logp is computed for forced decisions too
    np.testing.assert_allclose(lpk[0, 0], textbook(root[0], 2), rtol=0, atol=1e-12)


def test_fold_is_the_sequential_fp32_sum():
    rng = np.random.RandomState(7)
    sp, sq = rng.normal(-3, 2, (4, 8, 3)).astype(np.float32), rng.normal(-1, 2, (4, 8, 3)).astype(np.float32)
    sf = rng.randint(0, 13, (4, 8, 3)).astype(np.int32)
    se = np.zeros((4, 8), np.int32)
    se[2, 5] = 1
    lp, lq, f, e = CS.fold(sp, sq, sf, se)
    for b in range(4):
        for h in range(3):
            s = np.float32(0)
            for t in range(8):
                s = np.float32(s + sp[b, t, h])
            assert lp[b, h] == s
    assert lp.dtype == lq.dtype == np.float32 and np.array_equal(f, sf.sum(1)) and e.tolist() == [0, 0, 1, 0]


# ---------------------------------------------------------------------------------------------------------------- host-side validation
def test_chord_keep_steps_row():
    assert FF_.chord_keep_steps_row(range(4)) == b'\x01\x01\x01\x01\x00\x00\x00\x00'
    assert FF_.chord_keep_steps_row(slice(6, None)) == b'\x00' * 6 + b'\x01\x01'
    assert FF_.chord_keep_steps_row([]) == b'\x00' * 8
    for bad in ([8], [-1], [True], [1.0], 3):
        with pytest.raises(ValueError):
            FF_.chord_keep_steps_row(bad)


def test_check_chord_sampling():
    assert FF_.check_chord_sampling() is False
    assert FF_.check_chord_sampling(0.0) is True and FF_.check_chord_sampling(1.0, 0.5, 3, 4, 16) is True
    for kw in (dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature=float('inf')), dict(temperature=True),
               dict(temperature=1.0, chroma_temperature=-0.5), dict(temperature=1.0, chroma_temperature=float('inf')),
               dict(chroma_temperature=0.5), dict(seed=3), dict(draw=0), dict(sample_offset=16), dict(temperature=1.0, seed=-1),
               dict(temperature=1.0, draw=1 << 63), dict(temperature=1.0, sample_offset=1.5)):
        with pytest.raises(ValueError):
            FF_.check_chord_sampling(**kw)
    with pytest.raises(ValueError, match='chroma_temperature'):
        FF_.check_chord_sampling(1.0, -2.0)


def test_model_refuses_bad_chord_keywords_before_anything_else():
    """every ValueError of the chord keywords, on a CPU model with CPU latents: raised before any device is needed, the draw counter and
    the training flag untouched"""
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    m._sample_draws = 5
    m.train()
    z = torch.zeros(2, 256)
    bad = (dict(chord_temperature=-1.0), dict(chord_temperature=float('nan')), dict(chroma_temperature=0.5),
           dict(chord_temperature=1.0, chroma_temperature=-1.0), dict(keep_chords=object()),
           dict(chord_temperature=1.0, seed=-3), dict(chord_temperature=1.0, draw=1 << 63))
    for kw in bad:
        for f in (lambda: m.decode_to_inputs(z, z, **kw), lambda: m.decode_logprob(z, z, **kw), lambda: m.reencode(z, z, **kw),
                  lambda: m.decode_chords(z, **kw)):
            with pytest.raises(ValueError):
                f()
    for kw in (dict(seed=3), dict(draw=1), dict(sample_offset=16)):                          # no temperature at all
        with pytest.raises(ValueError):
            m.decode_chords(z, **kw)
        with pytest.raises(ValueError):
            m.decode_to_inputs(z, z, keep_chords=None, **kw)
    with pytest.raises(ValueError):
        m.decode_to_inputs(z, z, temperature=-1.0, chord_temperature=1.0)                    # the note decode's own refusals stay
    assert m._sample_draws == 5 and m.training
    creq = m._chord_request(2, chord_temperature=1.0, seed=9)
    assert isinstance(creq, M.ChordRequest) and creq.sampled and creq.chroma_temperature is None and creq.seed == 9 and creq.draw is None
    assert m._chord_request(2) is None
    assert m._chord_request(2, note_sampled=True, seed=4) is None
    # seed / draw / sample_offset without a CHORD temperature are the note decode's when that one samples
    assert m._chord_request(2, chroma_temperature=None, keep_chords=None, seed=4, note_sampled=True) is None
    with pytest.raises(RuntimeError):                                                        # valid keywords reach the device check
        m.decode_chords(z, chord_temperature=1.0)
    assert m._sample_draws == 5
