"""CPU: the numpy restatement of the chord grammar (tests/chord_grammar_ref.py) against a brute-force conditional of the model's bit-product
distribution, its identity with chord_sample_ref, the frequencies of its draws, and the host side of the feature: the words
DisentangleVAE.chord_grammar builds and every ValueError of the grammar keywords (no GPU, no launch)."""
import numpy as np
import pytest
import torch

import chord_grammar_ref as CG
import chord_sample_ref as CS
import sample_ref as S
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M

TRIADS = [0x091, 0x089, 0x049, 0x111]
SEVENTHS = TRIADS + [0x891, 0x491, 0x489, 0x449, 0x249, 0x889]
C_MAJOR = 0xab5
SKIP_CAP = 0.005


def logits(B, seed, scale=2.0):
    rng = np.random.RandomState(seed)
    return (rng.normal(0, scale, (B, 12)).astype(np.float32), rng.normal(0, scale, (B, 12, 2)).astype(np.float32),
            rng.normal(0, scale, (B, 12)).astype(np.float32))


def word(roots=0xfff, pcs=0xfff, flags=0):
    return roots | (pcs << 12) | flags


def brute_force(chroma, T, allowed_sets):
    """all 4096 bit patterns weighted by the product of the per-bit softmaxes at T, restricted to the given absolute sets, renormalised"""
    e = np.asarray(chroma, np.float64) / T
    p1 = 1.0 / (1.0 + np.exp(e[:, 0] - e[:, 1]))
    pats = np.arange(4096)
    bits = (pats[:, None] >> np.arange(12)) & 1
    w = np.where(bits == 1, p1, 1 - p1).prod(-1)
    assert abs(w.sum() - 1) < 1e-12
    sel = np.array([w[a] for a in allowed_sets])
    return sel / sel.sum()


@pytest.mark.parametrize('vocab', [TRIADS, SEVENTHS, [0x001, 0xfff, 0x091]])
def test_template_distribution_is_the_brute_force_conditional(vocab):
    _, chroma, _ = logits(6, 1)
    cases = [(0, 0xfff), (7, 0xfff), (0, C_MAJOR), (2, C_MAJOR), (11, C_MAJOR), (4, 0x001)]     # the last: nothing fits -> all (yield)
    for b, (r, mask) in enumerate(cases):
        for T in (1.0, 0.6):
            p = CG.template_distribution(chroma[b], word(pcs=mask, flags=CG.VOCAB), vocab, r, T)
            A = [int(CG.rot12(v, r)) for v in vocab]
            fits = [a & ~(mask | 1 << r) == 0 for a in A]
            if not any(fits):
                fits = [True] * len(A)
                assert CG.sets(word(pcs=mask, flags=CG.VOCAB), vocab, np.int64(r))['tmpl_yield']
            want = np.zeros(len(A))
            want[fits] = brute_force(chroma[b], float(np.float32(T)), [a for a, f in zip(A, fits) if f])
            np.testing.assert_allclose(p, want, rtol=0, atol=1e-12)
            assert (p[~np.array(fits)] == 0).all() and abs(p.sum() - 1) < 1e-12
    # C major, root D (2): of the triads only D minor fits the scale
    st = CG.sets(word(pcs=C_MAJOR, flags=CG.VOCAB), TRIADS, np.int64(2))
    assert st['tmpl'].tolist() == [False, True, False, False]


@pytest.mark.parametrize('sampled', [True, False])
def test_identity_rule_is_the_plain_decode(sampled):
    B = 40
    root, chroma, bass = logits(B, 2)
    nz = CS.noise(3, 1, np.arange(B), 4) if sampled else None
    keep_c, _ = CS.tokens(np.arange(B) % 12, (np.arange(B)[:, None] >> np.arange(12)) & 1, (np.arange(B) * 5) % 12)
    keep_c[3, 0:12] = 0
    kept = np.arange(B) % 3 == 0
    for kc, kp in ((None, None), (keep_c, kept)):
        want = CS.decide(root, chroma, bass, nz, 1.0, 0.7, kc, kp)
        got = CG.decide(root, chroma, bass, nz, None if nz is None else np.zeros((B, 0), np.float32), 1.0, 0.7, CG.IDENTITY, [], kc, kp)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert (got['template'] == -1).all()
        for dtype in (np.float64, np.float32):
            a = CS.logprob(root, chroma, bass, want, 1.0, 0.7, sampled, dtype)
            b = CG.logprob(root, chroma, bass, got, 1.0, 0.7, CG.IDENTITY, [], sampled, dtype)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        # a vocabulary that the word does not switch on changes nothing either
        got2 = CG.decide(root, chroma, bass, nz, None if nz is None else CG.vocab_noise(3, 1, np.arange(B), 4, 4), 1.0, 0.7, CG.IDENTITY, TRIADS, kc, kp)
        assert all(np.array_equal(got2[k], got[k]) for k in got)


def test_vocab_noise_uses_the_unused_subs():
    vz = CG.vocab_noise(11, 4, np.array([0, 5, 1 << 33]), 6, 64)
    assert vz.shape == (3, 64) and vz.dtype == np.float32
    for i, g in enumerate((0, 5, 1 << 33)):
        for v in (0, 15, 16, 17, 63):
            assert vz[i, v] == S.gumbel_from_word(S.words(11, 4, g, 6, 15, 0, 16 + (v & 15)))[v >> 4]
    assert np.array_equal(CG.vocab_noise(11, 4, 5, 6, 17), vz[1, :17])
    assert not np.isin(vz[1], CS.noise(11, 4, 5, 6).ravel()).any()


def test_rules_yields_and_obeys():
    B = 64
    root, chroma, bass = logits(B, 5)
    nz, vz = CS.noise(1, 0, np.arange(B), 2), CG.vocab_noise(1, 0, np.arange(B), 2, len(SEVENTHS))
    rule = np.array([word(C_MAJOR, C_MAJOR, CG.VOCAB | CG.ROOT_IN_CHORD | CG.BASS_IN_CHORD), word(0x004, 0xfff, CG.ROOT_IN_CHORD),
                     word(0xfff, 0x0f0, CG.BASS_IN_CHORD), word(0, 0xfff), word(0xfff, 0x001, CG.VOCAB), word(0xfff, 0, CG.BASS_IN_CHORD),
                     CG.IDENTITY, word(0x010, 0x010, 0)])[np.arange(B) % 8]
    d = CG.decide(root, chroma, bass, nz, vz, 1.0, 0.8, rule, SEVENTHS)
    c, _ = CS.tokens(d['root'], d['bits'], d['bass'])
    assert CG.obeys(c, rule, SEVENTHS).all()
    k = np.arange(B) % 8
    assert (d['err'][k == 3] == CG.ERR_ROOT_MASK).all() and (d['err'][k == 5] == CG.ERR_NO_BASS).all() and not d['err'][(k == 0) | (k == 6)].any()
    assert (d['root'][k == 1] == 2).all() and (d['bits'][k == 1][:, 2] == 1).all() and not d['bits'][k == 5].any()
    assert set(np.unique(d['err'][k == 4])) <= {0, CG.ERR_NO_TEMPLATE} and (d['err'][k == 4] == CG.ERR_NO_TEMPLATE).any()
    assert (d['bits'][k == 7].sum(-1) <= 1).all() and (d['root'][k == 7] == 4).all()
    assert (d['template'][(k == 0) | (k == 4)] >= 0).all() and (d['template'][(k != 0) & (k != 4)] == -1).all()
    # a chord off its rule is seen
    bad = c.copy()
    bad[0, 12:24] = 1
    assert not CG.obeys(bad, rule, SEVENTHS)[0] and CG.obeys(bad, rule, SEVENTHS)[1:].all()
    # logq: exactly 0 for a one-element set and for forced bits, and the allowed-set softmax otherwise
    lp, lq, _, _ = CG.logprob(root, chroma, bass, d, 1.0, 0.8, rule, SEVENTHS)
    plain = CS.logprob(root, chroma, bass, d, 1.0, 0.8)[0]
    assert np.array_equal(lp, plain)
    assert (lq[k == 1, 0] == 0).all() and (lq[k == 7, 0] == 0).all() and (lq[k == 5, 1] == 0).all() and (lq <= 0).all()
    f32 = CG.logprob(root, chroma, bass, d, 1.0, 0.8, rule, SEVENTHS, dtype=np.float32)
    assert np.abs(f32[1] - lq).max() < 2e-5 and (f32[1][k == 1, 0] == 0).all()
    b = int(np.nonzero(k == 0)[0][0])
    p = CG.template_distribution(chroma[b], rule[b], SEVENTHS, d['root'][b], 0.8)
    np.testing.assert_allclose(lq[b, 1], np.log(p[d['template'][b]]), rtol=0, atol=1e-12)


def test_draw_frequencies_follow_the_distribution():
    """N = 8000 draws (the samples g = 0..N-1 of seed 21, draw 0, chord step 3) of one row's chroma from the sevenths on root 0 at T = 0.9,
    once without a mask (ten allowed templates) and once in C major (two: C and Cmaj7).  Criterion: every template's frequency lies within
    4 standard deviations sqrt(p (1 - p) / N) of its conditional probability -- a false alarm over the 12 frequencies has probability
    below 1e-3 -- and a disallowed template is never drawn.  The device then only has to equal the restatement."""
    N, T, r = 8000, 0.9, 0
    _, chroma, _ = logits(1, 7, scale=1.0)
    root = np.zeros((N, 12), np.float32)
    root[:, r] = 50
    ch = np.broadcast_to(chroma, (N, 12, 2))
    nz, vz = CS.noise(21, 0, np.arange(N), 3), CG.vocab_noise(21, 0, np.arange(N), 3, len(SEVENTHS))
    for w, allowed in ((word(0xfff, 0xfff, CG.VOCAB), 10), (word(C_MAJOR, C_MAJOR, CG.VOCAB), 2)):
        d = CG.decide(root, ch, root, nz, vz, 0.0, T, w, SEVENTHS)
        p = CG.template_distribution(chroma[0], w, SEVENTHS, r, T)
        freq = np.bincount(d['template'], minlength=len(SEVENTHS)) / N
        sd = np.sqrt(p * (1 - p) / N)
        print('template p    ', np.round(p, 4), '\nfrequency     ', np.round(freq, 4), '\ndeviation     ', np.round(freq - p, 4), '\n4 sd          ',
              np.round(4 * sd, 4))
        assert (d['root'] == r).all() and (p > 0).sum() == allowed and (freq[p == 0] == 0).all()
        assert (np.abs(freq - p) <= 4 * sd).all()


def test_skippable_counts_of_the_gpu_cases_stay_under_the_cap():
    """the restatement's own count of skippable decisions for the seeds, shapes and temperatures of tests/test_gpu_chord_grammar_kernels.py's
    sampled cases: at most SKIP_CAP of a case's decisions"""
    import chord_grammar_cases as GC
    for Tc, Th in GC.TEMPERATURES:
        case = GC.sampled_case(Tc, Th)
        d = CG.decide(*case['logits'], case['nz'], case['vz'], Tc, Th, case['rule'], case['vocab'])
        skip = CG.skippable(*case['logits'], case['nz'], case['vz'], Tc, Th, case['rule'], case['vocab'], d)
        n = sum(s.size for s in skip)
        k = sum(int(s.sum()) for s in skip)
        print('T = (%g, %g): %d of %d decisions skippable' % (Tc, Th, k, n))
        assert k <= SKIP_CAP * n
        c, _ = CS.tokens(d['root'], d['bits'], d['bass'])
        assert CG.obeys(c, case['rule'], case['vocab']).all()


# ---------------------------------------------------------------------------------------------------------------- the builder
def cpu_model():
    return M.DisentangleVAE.init_model(torch.device('cpu'))


def test_builder_words():
    m = cpu_model()
    g = m.chord_grammar(key=0)
    assert isinstance(g, FF_.ChordGrammar) and g.rule.dtype == torch.int32 and tuple(g.rule.shape) == (1, 8) and g.batch == 1
    assert (g.rule == (C_MAJOR | C_MAJOR << 12)).all() and g.vocab.numel() == 0 and g.vocab.dtype == torch.int32
    assert (m.chord_grammar(key=9, scale='minor').rule == (C_MAJOR | C_MAJOR << 12)).all()            # A minor is C major's set
    assert (m.chord_grammar(key=0, scale='harmonic_minor').rule & 0xfff == 0x9ad).all()
    assert (m.chord_grammar(key=2).rule & 0xfff == 0xad6).all()                                       # D major
    assert (m.chord_grammar(key=0, scale=[0, 2, 4, 5, 7, 9, 11]).rule == m.chord_grammar(key=0).rule).all()
    assert (m.chord_grammar(key=0, scale=0x001).rule == (1 | 1 << 12)).all()
    # roots relative to the key; absolute without one
    g = m.chord_grammar(key=7, roots=[0, 5, 7])
    assert (g.rule & 0xfff == (1 << 7 | 1 << 0 | 1 << 2)).all() and ((g.rule >> 12) & 0xfff == int(CG.rot12(C_MAJOR, 7))).all()
    g = m.chord_grammar(roots=[0, 5, 7])
    assert (g.rule == (0x0a1 | 0xfff << 12)).all()
    g = m.chord_grammar(pitch_classes=0x0f0, root_in_chord=True, bass_in_chord=True)
    assert (g.rule == (0xfff | 0x0f0 << 12 | CG.ROOT_IN_CHORD | CG.BASS_IN_CHORD)).all()
    assert ((m.chord_grammar(key=0, pitch_classes=[0, 1, 2]).rule >> 12) & 0xfff == 0x005).all()
    # identity
    assert (m.chord_grammar().rule == CG.IDENTITY).all() and FF_.CHORD_RULE_IDENTITY == CG.IDENTITY
    # vocabularies
    g = m.chord_grammar(qualities='triads')
    assert g.vocab.tolist() == TRIADS and (g.rule == (CG.IDENTITY | CG.VOCAB | CG.ROOT_IN_CHORD)).all()
    assert m.chord_grammar(qualities='sevenths').vocab.tolist() == SEVENTHS
    assert m.chord_grammar(qualities=[(0, 4, 7), 0x089, [0, 7]]).vocab.tolist() == [0x091, 0x089, 0x081]
    assert (FF_.CHORD_RULE_VOCAB, FF_.CHORD_RULE_ROOT_IN_CHORD, FF_.CHORD_RULE_BASS_IN_CHORD) == (CG.VOCAB, CG.ROOT_IN_CHORD, CG.BASS_IN_CHORD)
    # steps
    g = m.chord_grammar(key=0, steps=range(4, 8))
    assert (g.rule[:, :4] == CG.IDENTITY).all() and (g.rule[:, 4:] == (C_MAJOR | C_MAJOR << 12)).all()
    g = m.chord_grammar(key=0, steps=slice(0, 2), batch=3)
    assert tuple(g.rule.shape) == (3, 8) and g.batch == 3 and (g.rule[:, 2:] == CG.IDENTITY).all() and (g.rule[:, :2] != CG.IDENTITY).all()
    st = torch.zeros(2, 8, dtype=torch.bool)
    st[1, 3] = True
    g = m.chord_grammar(key=0, qualities='triads', steps=st)
    assert tuple(g.rule.shape) == (2, 8) and (g.rule != CG.IDENTITY).sum() == 1 and g.rule[1, 3] == (C_MAJOR | C_MAJOR << 12 | CG.VOCAB | CG.ROOT_IN_CHORD)
    # a key per row, and per row and step
    keys = torch.tensor([0, 2, 11, 7])
    g = m.chord_grammar(key=keys, bass_in_chord=True)
    assert tuple(g.rule.shape) == (4, 8) and g.batch == 4
    for b, k in enumerate(keys.tolist()):
        s = int(CG.rot12(C_MAJOR, k))
        assert (g.rule[b] == (s | s << 12 | CG.BASS_IN_CHORD)).all()
    ks = (torch.arange(3)[:, None] + torch.arange(8)[None, :]) % 12
    g = m.chord_grammar(key=ks.to(torch.int32), scale='minor')
    want = CG.rot12(0x5ad, ks.numpy())
    assert np.array_equal(g.rule.numpy() & 0xfff, want) and np.array_equal((g.rule.numpy() >> 12) & 0xfff, want)
    FF_.check_chord_grammar(g, 3)
    FF_.check_chord_grammar(m.chord_grammar(key=0), 3)


def test_builder_refusals():
    m = cpu_model()
    bad = (dict(key=12), dict(key=-1), dict(key=True), dict(key=1.0), dict(key=torch.zeros(3)), dict(key=torch.zeros(3, 7, dtype=torch.int64)),
           dict(key=torch.zeros(2, 8, 1, dtype=torch.int64)), dict(key=0, scale='dorian'), dict(key=0, scale=0x1000), dict(key=0, scale=[12]),
           dict(key=0, scale=1.5), dict(roots=[True]), dict(roots=-1), dict(pitch_classes=0x1000), dict(pitch_classes=[0.5]),
           dict(qualities='ninths'), dict(qualities=[]), dict(qualities=[0x090]), dict(qualities=[(4, 7)]), dict(qualities=[0x091, (0, 4, 7)]),
           dict(qualities=[0x1001]), dict(qualities=[1 | (v << 1) for v in range(65)]), dict(qualities=7), dict(qualities='triads', root_in_chord=False),
           dict(root_in_chord=1), dict(bass_in_chord=None), dict(steps=[8]), dict(steps=3), dict(steps=torch.ones(2, 7, dtype=torch.bool)),
           dict(steps=torch.ones(2, 8)), dict(key=torch.zeros(3, dtype=torch.int64), steps=torch.ones(2, 8, dtype=torch.bool)),
           dict(batch=0), dict(batch=True), dict(key=torch.zeros(3, dtype=torch.int64), batch=4))
    for kw in bad:
        with pytest.raises(ValueError):
            m.chord_grammar(**kw)
    g = m.chord_grammar(key=0, batch=3)
    for broken in (object(), FF_.ChordGrammar(g.rule.long(), g.vocab, 3), FF_.ChordGrammar(g.rule, g.vocab.float(), 3),
                   FF_.ChordGrammar(g.rule, g.vocab, 2), FF_.ChordGrammar(g.rule[:, :7], g.vocab, 3),
                   FF_.ChordGrammar(g.rule, torch.zeros(65, dtype=torch.int32), 3)):
        with pytest.raises(ValueError):
            FF_.check_chord_grammar(broken)
    with pytest.raises(ValueError):
        FF_.check_chord_grammar(g, 4)
    FF_.check_chord_grammar(None, 4)


def test_model_refuses_bad_grammar_keywords_before_anything_else():
    """every ValueError of grammar= / chord_grammar= on the four entry points, on a CPU model with CPU latents: raised before any device is
    needed, the draw counter and the training flag untouched"""
    m = cpu_model()
    m._sample_draws = 5
    m.train()
    z = torch.zeros(2, 256)
    g3 = m.chord_grammar(key=0, batch=3)
    g1 = m.chord_grammar(key=0, qualities='triads')
    for bad in (object(), g3, FF_.ChordGrammar(g1.rule.long(), g1.vocab, 1), 'major'):
        for f in (lambda: m.decode_to_inputs(z, z, chord_grammar=bad), lambda: m.decode_logprob(z, z, chord_grammar=bad),
                  lambda: m.reencode(z, z, chord_grammar=bad), lambda: m.decode_chords(z, grammar=bad)):
            with pytest.raises(ValueError):
                f()
    # a grammar alone is no sampled decode: seed / draw / sample_offset without a temperature stay refused
    for kw in (dict(seed=3), dict(draw=1), dict(sample_offset=16)):
        with pytest.raises(ValueError):
            m.decode_chords(z, grammar=g1, **kw)
        with pytest.raises(ValueError):
            m.decode_to_inputs(z, z, chord_grammar=g1, **kw)
    with pytest.raises(ValueError):
        m.decode_chords(z, grammar=g1, chroma_temperature=0.5)
    with pytest.raises(ValueError):
        m.chd_decoder.decode_chords(z, grammar=g3)
    assert m._sample_draws == 5 and m.training
    # the request: None without a chord keyword, the grammar as its last field with one
    assert m._chord_request(2) is None and m._chord_request(2, note_sampled=True, seed=4) is None
    creq = m._chord_request(2, grammar=g1)
    assert isinstance(creq, M.ChordRequest) and not creq.sampled and creq.grammar is g1 and creq.keep is None
    assert m._chord_request(2, 1.0, None, None, 9).grammar is None                            # the positional call of the existing test
    assert M.ChordRequest(True, 1.0, None, 1, 2, 3, None).grammar is None and M.ChordRequest._fields[-1] == 'grammar'
    with pytest.raises(RuntimeError):                                                        # valid keywords reach the device check
        m.decode_chords(z, grammar=g1)
    assert m._sample_draws == 5
