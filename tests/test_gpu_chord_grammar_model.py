"""GPU: the chord grammar at the model level (RnnDecoder.decode_chords(grammar=), DisentangleVAE.chord_grammar / decode_chords /
decode_to_inputs / decode_logprob / reencode; INTEGRATION.md "Chord grammar") on the full model with full_params() and z_chd =
torch.randn(24, 256) under torch.manual_seed(12).

ptv_chord_decode_grammar equals a Python sequencing of its launches bit for bit; under the identity rule it is the plain decode bit for bit;
every chord decoded under a rule satisfies it (tests/chord_grammar_ref.obeys, no tolerance); a shard decodes like the whole batch; kept
steps override the rule; the output path passes the grammar through and is what it was without one."""
import numpy as np
import pytest
import torch

import chord_grammar_ref as CG
import test_gpu_chord_decode_kernels as KT
import test_gpu_chord_decode_model as MT
from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = KT.DEV
SEED, DRAW = KT.SEED, KT.DRAW
B = 24
host, model, with_precision = MT.host, MT.model, MT.with_precision


def latents():
    torch.manual_seed(12)
    return torch.randn(B, 256).to(DEV)


def keys():
    return (torch.arange(B, device=DEV) * 7) % 12


def decode(m, z, Tc=None, Th=None, offset=0, keep=None, grammar=None):
    return m.chd_decoder.decode_chords(z, temperature=Tc, chroma_temperature=Th, seed=SEED, draw=DRAW, sample_offset=offset, keep=keep,
                                       grammar=grammar, return_logprob=True)


def same_logprob(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def sequenced(P, z, prec, blk, keep, grammar):
    """the launches of ptv_chord_decode_grammar, sequenced from Python through the same entry points -> the composite's outputs by name"""
    dev = z.device
    n, H, I, T = z.shape[0], P['gru.weight_hh_l0'].shape[1], 36, 8
    e = lambda *s: torch.empty(*s, device=dev)
    i = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
    hall = e(T + 1, n, H)
    F_.gemm(z, P['z2dec_hid.weight'], hall[0], bias=P['z2dec_hid.bias'], prec=prec)
    z_in = F_.gemm(z, P['z2dec_in.weight'], bias=P['z2dec_in.bias'], prec=prec)
    w_ih = P['gru.weight_ih_l0']
    zg = F_.gemm(z_in, w_ih[:, I:], bias=P['gru.bias_ih_l0'], prec=prec)
    tok, gi = e(n, I), e(n, 3 * H)
    F_.copy2d(tok, P['init_input'].view(1, -1), lds=0)
    root, chroma, bass = e(T, n, 12), e(T, n, 24), e(T, n, 12)
    c, c14, sp, sq, sf, se = e(n, T, 36), e(n, T, 14), e(n, T, 3), e(n, T, 3), i(n, T, 3), i(n, T)
    nv = grammar.vocab.shape[0]
    for t in range(T):
        F_.gemm(tok, w_ih[:, :I], gi, prec=prec)
        FF_.gru_step(prec, hall[t], gi, 3 * H, P['gru.weight_hh_l0'], P['gru.bias_hh_l0'], hall[t + 1], gi2=zg)
        F_.gemm(hall[t + 1], P['root_out.weight'], root[t], bias=P['root_out.bias'], prec=prec)
        F_.gemm(hall[t + 1], P['chroma_out.weight'], chroma[t], bias=P['chroma_out.bias'], prec=prec)
        F_.gemm(hall[t + 1], P['bass_out.weight'], bass[t], bias=P['bass_out.bias'], prec=prec)
        call('ptv_chord_decide_grammar', ptr(root[t]), ptr(chroma[t]), ptr(bass[t]), n, t, ptr(blk), ptr(keep.c) if keep else None,
             ptr(keep.steps) if keep else None, keep.steps.shape[0] if keep else 0, ptr(grammar.rule), grammar.rule.shape[0],
             ptr(grammar.vocab) if nv else None, nv, ptr(tok) if t + 1 < T else None, ptr(c), ptr(c14), ptr(sp), ptr(sq), ptr(sf), ptr(se),
             stream_ptr())
    lp, lq, f, er = e(n, 3), e(n, 3), i(n, 3), i(n)
    call('ptv_chord_logprob_fold', ptr(sp), ptr(sq), ptr(sf), ptr(se), n, ptr(lp), ptr(lq), ptr(f), ptr(er), stream_ptr())
    return dict(c=c, chord14=c14, root=root, chroma=chroma, bass=bass, logp=lp, logq=lq, forced=f, err=er, step_logp=sp, step_logq=sq,
                step_forced=sf)


def mixed_grammar(m, n):
    """a key per row; the vocabulary on the odd steps only, so both chroma paths run in one decode"""
    k = (torch.arange(n, device=DEV) * 5) % 12
    g = m.chord_grammar(key=k, qualities='sevenths', bass_in_chord=True)
    odd = torch.arange(8, device=DEV) % 2 == 1
    rule = torch.where(odd[None, :], g.rule, g.rule & ~FF_.CHORD_RULE_VOCAB)
    return FF_.ChordGrammar(rule.contiguous(), g.vocab, n)


@pytest.mark.parametrize('n', [3, 24])
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_composite_equals_the_python_sequencing(prec, n):
    m = with_precision(prec)
    try:
        g = torch.Generator().manual_seed(5)
        z = torch.randn(n, 256, generator=g).to(DEV)
        P = dict(zip(F_.CHD_PARAM_NAMES, m.chd_decoder._params()))
        pc = F_.prec_code(prec)
        steps = (torch.arange(n, device=DEV)[:, None] + torch.arange(8, device=DEV)[None, :]) % 3 == 0
        with torch.no_grad():
            first = FF_.chord_decode(z, P, pc)
            keep = FF_.build_chord_keep(first.c, steps)
            for blk, kp, gr in ((None, None, mixed_grammar(m, n)), (KT.block(1.0, 0.7, 9), None, mixed_grammar(m, n)),
                                (KT.block(0.8, 0.0, 9), keep, mixed_grammar(m, n)), (KT.block(1.0, 0.7, 9), None, m.chord_grammar(key=4))):
                calls, plain_calls = FF_._CDG.get('calls', 0), FF_._CDS.get('calls', 0)
                got = FF_.chord_decode(z, P, pc, blk, kp, gr)
                assert FF_._CDG['calls'] == calls + 1 and FF_._CDS.get('calls', 0) == plain_calls      # the grammar composite really ran
                want = sequenced(P, z, pc, blk, kp, gr)
                flat = dict(got._asdict(), **got.logprob._asdict())
                for k, v in want.items():
                    assert torch.equal(flat[k], v), (k, blk is not None, kp is not None)
                if kp is not None:
                    assert torch.equal(got.c[steps], first.c[steps]) and host(got.logprob.forced).sum() > 0
    finally:
        m.set_precision('fp32')


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_identity_rule_is_the_plain_decode(prec):
    m, z = with_precision(prec), latents()
    try:
        ident = m.chord_grammar()
        assert (host(ident.rule) == CG.IDENTITY).all() and ident.vocab.numel() == 0
        other = decode(m, z, 1.0, 0.5)[0]
        keep = m.keep_chords(other, range(2, 5))
        for Tc, Th, kp in ((None, None, None), (1.0, 0.5, None), (1.0, 0.0, keep), (None, None, keep)):
            c, c14, lp = decode(m, z, Tc, Th, keep=kp)
            raw = [a.clone() for a in m.chd_decoder.last_chord_logits]
            for gr in (ident, m.chord_grammar(batch=B), FF_.ChordGrammar(ident.rule, m.chord_grammar(qualities='triads').vocab, 1)):
                c2, c142, lp2 = decode(m, z, Tc, Th, keep=kp, grammar=gr)
                assert torch.equal(c2, c) and torch.equal(c142, c14) and same_logprob(lp2, lp)
                assert all(torch.equal(a, b) for a, b in zip(m.chd_decoder.last_chord_logits, raw))
    finally:
        m.set_precision('fp32')


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('Tc,Th', [(None, None), (1.0, 0.7)])
def test_decoded_chords_obey_the_rule_and_shards_agree(prec, Tc, Th):
    m, z = with_precision(prec), latents()
    try:
        gr = m.chord_grammar(key=keys(), qualities='triads', bass_in_chord=True)
        c, c14, lp = decode(m, z, Tc, Th, grammar=gr)
        logits = [a.clone() for a in m.chd_decoder.last_chord_logits]
        rule, vocab = host(gr.rule), host(gr.vocab)
        assert CG.obeys(host(c), rule, vocab).all() and not host(lp.err).any() and not host(lp.forced).any()
        plain = decode(m, z, Tc, Th)[0]
        off = ~CG.obeys(host(plain), rule, vocab)
        print('%s T = %s: %d of %d chords of the plain decode are off the rule' % (prec, Tc, off.sum(), off.size))
        assert off.any()                                     # the rule changes something
        bits = host(c)[..., 12:24]
        assert (bits.sum(-1) == 3).all()                     # triads
        if Tc is None:
            assert (host(lp.logq) == 0).all()
        else:
            assert (host(lp.logq) <= 0).all() and (host(lp.logq)[:, 0] < 0).all()
        # the two halves, decoded separately at their sample offsets with their rows of the rule, are the whole decode: the same logits
        # (the products over 12 and over 24 rows round alike on an MI355X: 12 of 12 rows in every case), the same chords, the same figures
        h = B // 2
        for lo in (0, h):
            sub = FF_.ChordGrammar(gr.rule[lo:lo + h].contiguous(), gr.vocab, h)
            c_s, c14_s, lp_s = decode(m, z[lo:lo + h].contiguous(), Tc, Th, offset=lo, grammar=sub)
            same = np.array([all(torch.equal(a[:, i], b[:, lo + i]) for a, b in zip(m.chd_decoder.last_chord_logits, logits)) for i in range(h)])
            print('%s rows %d..%d: %d of %d rows have the whole decode\'s logits' % (prec, lo, lo + h - 1, same.sum(), h))
            assert same.all()
            sel = torch.from_numpy(same).to(DEV)
            assert torch.equal(c_s[sel], c[lo:lo + h][sel]) and torch.equal(c14_s[sel], c14[lo:lo + h][sel])
            assert all(torch.equal(a[sel], b[lo:lo + h][sel]) for a, b in zip(lp_s, lp))
            assert CG.obeys(host(c_s), rule[lo:lo + h], vocab).all()
            # ... and the first step, whose logits depend on z alone, decides alike wherever its logits agree
            first = np.array([all(torch.equal(a[0, i], b[0, lo + i]) for a, b in zip(m.chd_decoder.last_chord_logits, logits)) for i in range(h)])
            print('%s rows %d..%d: %d of %d rows have the whole decode\'s first logits' % (prec, lo, lo + h - 1, first.sum(), h))
            assert torch.equal(c_s[:, 0][torch.from_numpy(first).to(DEV)], c[lo:lo + h, 0][torch.from_numpy(first).to(DEV)])
    finally:
        m.set_precision('fp32')


def test_kept_first_bar_and_a_grammar_on_the_second():
    m, z = with_precision('bf16'), latents()
    try:
        other = decode(m, z, 1.0, 0.5)[0]
        keep = m.keep_chords(other, range(4))
        whole = m.chord_grammar(key=keys(), qualities='triads', bass_in_chord=True)
        second = m.chord_grammar(key=keys(), qualities='triads', bass_in_chord=True, steps=range(4, 8))
        assert (host(second.rule)[:, :4] == CG.IDENTITY).all() and np.array_equal(host(second.rule)[:, 4:], host(whole.rule)[:, 4:])
        got = [decode(m, z, 1.0, 0.7, keep=keep, grammar=gr) for gr in (whole, second)]
        for c, c14, lp in got:                               # a kept step overrides its rule word: both grammars decode alike
            assert torch.equal(c[:, :4], other[:, :4]) and (host(lp.forced) == np.array([4, 48, 4])).all() and not host(lp.err).any()
            assert CG.obeys(host(c)[:, 4:], host(whole.rule)[:, 4:], host(whole.vocab)).all()
            assert (host(lp.step_logq)[:, :4] == 0).all() and (host(lp.step_logq)[:, 4:] <= 0).all()
        assert torch.equal(got[0][0], got[1][0]) and same_logprob(got[0][2], got[1][2])
        assert not CG.obeys(host(other)[:, :4], host(whole.rule)[:, :4], host(whole.vocab)).all()      # the kept bar itself is off the rule
        # without the keep the second grammar leaves the first bar to the plain rule
        c, _, lp = decode(m, z, 1.0, 0.7, grammar=second)
        assert torch.equal(c[:, :4], decode(m, z, 1.0, 0.7)[0][:, :4]) and CG.obeys(host(c)[:, 4:], host(whole.rule)[:, 4:], host(whole.vocab)).all()
    finally:
        m.set_precision('fp32')


def test_surface():
    m = with_precision('bf16')
    try:
        g = torch.Generator().manual_seed(6)
        z = torch.randn(4, 512, generator=g).to(DEV)
        zc, zr = z[:, :256].contiguous(), z[:, 256:].contiguous()
        m.use_philox(SEED, 32)
        m._sample_draws = 3
        gr = m.chord_grammar(key=torch.tensor([0, 7, 2, 9], device=DEV), qualities='sevenths', bass_in_chord=True)
        rule, vocab = host(gr.rule), host(gr.vocab)
        # without the keyword (and with chord_grammar=None): today's call -- decode_tokens' chords, no chord-decode launch, the counter stays
        launches = (dict(FF_._CDS), dict(FF_._CDG))
        plain = m.decode_to_inputs(zc, zr)
        none = m.decode_to_inputs(zc, zr, chord_grammar=None)
        assert len(plain) == 6 and torch.equal(plain[2], m.chd_decoder.decode_tokens(zc)[0]) and m._sample_draws == 3
        assert all(torch.equal(a, b) for a, b in zip(plain, none)) and (dict(FF_._CDS), dict(FF_._CDG)) == launches
        assert len(m.decode_logprob(zc, zr)) == 7
        d0 = m.reencode(zc, zr)
        assert torch.equal(d0[0].mean, m.inference_encode(plain[0], plain[2])[0].mean)
        # a grammar alone selects the row-independent decode, as its argmax: no draw is spent
        out = m.decode_to_inputs(zc, zr, chord_grammar=gr)
        assert len(out) == 6 and m._sample_draws == 3 and FF_._CDG['calls'] == launches[1].get('calls', 0) + 1
        want = m.chd_decoder.decode_chords(zc, grammar=gr)[0]
        assert torch.equal(out[2], want) and CG.obeys(host(out[2]), rule, vocab).all()
        for a, b in zip(out[:2] + out[3:], plain[:2] + plain[3:]):                          # the note decode is untouched
            assert torch.equal(a, b)
        c, c14, lp = m.decode_chords(zc, grammar=gr, return_logprob=True)
        assert torch.equal(c, want) and m._sample_draws == 3 and (host(lp.logq) == 0).all() and not host(lp.err).any()
        full = m.decode_logprob(zc, zr, chord_grammar=gr)
        assert len(full) == 8 and isinstance(full[7], FF_.ChordLogprob) and same_logprob(full[7], lp) and torch.equal(full[2], want)
        d1, _ = m.reencode(zc, zr, chord_grammar=gr)
        assert torch.equal(d1.mean, m.inference_encode(plain[0], want)[0].mean) and not torch.equal(d1.mean, d0[0].mean)
        # sampled under the grammar: one call, one draw, the model's seed and offset
        s = m.decode_to_inputs(zc, zr, chord_temperature=1.0, chroma_temperature=0.7, chord_grammar=gr)
        assert m._sample_draws == 4
        want = m.chd_decoder.decode_chords(zc, temperature=1.0, chroma_temperature=0.7, seed=SEED, draw=3, sample_offset=32, grammar=gr)[0]
        assert torch.equal(s[2], want) and CG.obeys(host(want), rule, vocab).all()
        cs, _ = m.decode_chords(zc, chord_temperature=1.0, chroma_temperature=0.7, draw=3, grammar=gr)
        assert torch.equal(cs, want) and m._sample_draws == 4
        # the decoded chords are chords: pitch_mask takes them, and a step's mask holds exactly the chord's tones
        mask = m.pitch_mask(c=want)
        assert mask.dtype == torch.int32 and tuple(mask.shape) == (4, 32, 4)
        mk = host(mask).view(np.uint32)
        tones = np.array([[[(mk[b, t, p >> 5] >> (p & 31)) & 1 for p in range(128)] for t in range(32)] for b in range(4)])
        assert np.array_equal(tones, np.repeat(host(want)[:, :, 12:24], 4, axis=1)[:, :, np.arange(128) % 12].astype(np.int64))
        assert (tones.reshape(4, 32, -1).sum(-1) > 0).all()
        # refusals: a ValueError, no launch, no counter change
        launches = (dict(FF_._CDS), dict(FF_._CDG))
        for bad in (object(), m.chord_grammar(key=0, batch=3), FF_.ChordGrammar(gr.rule.cpu(), gr.vocab.cpu(), 4)):
            for f in (lambda: m.decode_to_inputs(zc, zr, chord_grammar=bad), lambda: m.decode_chords(zc, grammar=bad),
                      lambda: m.reencode(zc, zr, chord_grammar=bad)):
                with pytest.raises(ValueError):
                    f()
        for kw in (dict(seed=1), dict(draw=1), dict(sample_offset=1)):
            with pytest.raises(ValueError):
                m.decode_to_inputs(zc, zr, chord_grammar=gr, **kw)
            with pytest.raises(ValueError):
                m.decode_chords(zc, grammar=gr, **kw)
        assert m._sample_draws == 4 and (dict(FF_._CDS), dict(FF_._CDG)) == launches
    finally:
        m._philox = None
        m._sample_draws = 0
        m.set_precision('fp32')
