"""GPU: the row-independent chord decode at the model level (RnnDecoder.decode_chords, DisentangleVAE.decode_chords / keep_chords /
decode_to_inputs / decode_logprob / reencode; INTEGRATION.md "Chord decode") on the full model with full_params() and z_chd =
torch.randn(64, 256) under torch.manual_seed(11).

Every decision must follow from the decode's own emitted logits and the restated noise (tests/chord_sample_ref.py) but for the decisions
sample_ref.skippable() allows, at most SKIP_CAP of a case; an fp64 restatement of this model and these z skips 0 of the 7,168 decisions of
both temperature pairs, and all 64 rows differ from the argmax decode.  The emitted logits are those of the project's own teacher-forced
chord decoder and of the oracle fed the decoded chords (atol 1e-4, the bar of test_full_config_vs_reference_golden); a replay through
keep_chords reproduces the decode bit for bit; the one-call composite equals the Python sequencing of its launches bit for bit."""
import functools

import numpy as np
import pytest
import torch

import chord_sample_ref as CS
import test_gpu_chord_decode_kernels as KT
from helpers import full_params
from oracle.ptvae_oracle import Oracle
from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M
from polyphonic_chord_texture_disentanglement_amd._lib import call, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = KT.DEV
SEED, DRAW = KT.SEED, KT.DRAW
B = 64
LOGIT_ATOL = 1e-4
GAP = 2e-4                                                   # twice the logit bar: a decision closer than this may differ between two paths
MAX_SKIPPED_ROWS = 12                                        # the fp64 restatement has 6 such rows: 1, 7, 21, 23, 33, 62; an MI355X: 22, 26, 51


@functools.lru_cache(maxsize=None)
def model():
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV)
    m.eval()
    return m


def with_precision(prec):
    return model().set_precision(prec)


@functools.lru_cache(maxsize=None)
def latents():
    torch.manual_seed(11)
    return torch.randn(B, 256).to(DEV)


@functools.lru_cache(maxsize=None)
def noise(lo, hi):
    nz = CS.decode_noise(SEED, DRAW, np.arange(lo, hi))
    nz.setflags(write=False)
    return nz


def host(t):
    return t.cpu().numpy()


def emitted(m):
    """the step-major logits of the last decode_chords in batch-major API shapes: root [B,8,12], chroma [B,8,12,2], bass [B,8,12]"""
    root, chroma, bass = (host(a) for a in m.chd_decoder.last_chord_logits)
    n = root.shape[1]
    return root.transpose(1, 0, 2), chroma.reshape(8, n, 12, 2).transpose(1, 0, 2, 3), bass.transpose(1, 0, 2)


def decisions(chord14):
    c14 = host(chord14)
    return dict(root=c14[..., 0].astype(np.int64), bits=c14[..., 1:13].astype(np.int64), bass=c14[..., 13].astype(np.int64))


def decode(m, z, Tc=None, Th=None, offset=0, draw=DRAW, keep=None):
    """one decode -> (c, chord14, ChordLogprob, logits, decisions); the token forms are checked against each other"""
    c, c14, lp = m.chd_decoder.decode_chords(z, temperature=Tc, chroma_temperature=Th, seed=SEED, draw=draw, sample_offset=offset,
                                             keep=keep, return_logprob=True)
    d = decisions(c14)
    want_c, want_c14 = CS.tokens(d['root'], d['bits'], d['bass'])
    assert np.array_equal(host(c), want_c) and np.array_equal(host(c14), want_c14)
    return c, c14, lp, emitted(m), d


def explained(logits, d, nz, Tc, Th, what, steps=slice(None)):
    root, chroma, bass = (a[:, steps] for a in logits)
    nz = nz[:, steps]
    want = CS.decide(root, chroma, bass, nz, Tc, Th)
    KT.explained({k: v[:, steps] for k, v in d.items()}, want, CS.skippable(root, chroma, bass, nz, Tc, Th), what)


def logprob_matches(lp, logits, d, Tc, Th, family):
    """ChordLogprob against the restatement at the decode's own logits and decisions, step by step; the fold bit for bit"""
    sp, sq, sf = host(lp.step_logp), host(lp.step_logq), host(lp.step_forced)
    for t in (0, 7):
        r = dict(root=d['root'][:, t], bits=d['bits'][:, t], bass=d['bass'][:, t], step_forced=sf[:, t], step_logp=sp[:, t], step_logq=sq[:, t])
        KT.check_logprob('%s t=%d' % (family, t), logits[0][:, t], logits[1][:, t], logits[2][:, t], r, Tc or 0.0, Th or 0.0, Tc is not None)
    f_lp, f_lq, f_f, f_e = CS.fold(sp, sq, sf, np.zeros(sp.shape[:2], np.int32))
    assert host(lp.logp).tobytes() == f_lp.tobytes() and host(lp.logq).tobytes() == f_lq.tobytes()
    assert np.array_equal(host(lp.forced), f_f)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('Tc,Th', [(1.0, 1.0), (1.0, 0.5)])
def test_every_decision_is_explained(prec, Tc, Th):
    m, z = with_precision(prec), latents()
    try:
        c, c14, lp, logits, d = decode(m, z, Tc, Th)
        explained(logits, d, noise(0, B), Tc, Th, '%s T = (%g, %g)' % (prec, Tc, Th))
        logprob_matches(lp, logits, d, Tc, Th, '%s T=(%g,%g)' % (prec, Tc, Th))
        assert not host(lp.err).any() and not host(lp.forced).any()
        plain = decode(m, z)
        assert (host(plain[0]) != host(c)).reshape(B, -1).any(1).all()                       # all 64 rows differ from the argmax decode
        assert (host(plain[2].logq) == 0).all()
        # a shard decodes like the whole batch: z[16:32] at sample_offset 16 draws the noise of global samples 16..31
        _, _, _, s_logits, s_d = decode(m, z[16:32].contiguous(), Tc, Th, offset=16)
        explained(s_logits, s_d, noise(16, 32), Tc, Th, '%s shard' % prec)
        same = np.array([all(np.array_equal(a[i, 0], b[16 + i, 0]) for a, b in zip(s_logits, logits)) for i in range(16)])
        print('%s: the first step\'s logits of the shard equal the full batch\'s on %d of 16 rows' % (prec, same.sum()))
        for k in s_d:
            assert np.array_equal(s_d[k][same, 0], d[k][16:32][same, 0]), k
    finally:
        m.set_precision('fp32')


def test_the_trajectory_is_the_models():
    """fp32: the emitted logits against the teacher-forced chord decoder, and against the oracle, both fed the decoded chords"""
    m, z = with_precision('fp32'), latents()
    c, _, _, logits, _ = decode(m, z, 1.0, 0.5)
    with torch.no_grad():
        tf = m.chd_decoder(z, False, 1., c=c, coins=[True] * 8)
    for name, a, b in zip(('root', 'chroma', 'bass'), logits, tf):
        err = np.abs(a - host(b.contiguous())).max()
        print('teacher-forced %s: max |dlogit| %.3e' % (name, err))
        assert err <= LOGIT_ATOL, (name, err)
    with torch.no_grad():
        ref = Oracle(full_params()).chd_decoder(z.cpu(), False, 1.0, c.cpu(), coin=lambda: 0.0)
    for name, a, b in zip(('root', 'chroma', 'bass'), logits, ref):
        err = np.abs(a - b.numpy()).max()
        print('oracle %s: max |dlogit| %.3e' % (name, err))
        assert err <= LOGIT_ATOL, (name, err)


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_replay_through_keep_chords_is_bit_identical(prec):
    m, z = with_precision(prec), latents()
    try:
        c, c14, lp, _, _ = decode(m, z, 1.0, 0.5)
        raw = [a.clone() for a in m.chd_decoder.last_chord_logits]
        keep = model().keep_chords(c, range(8))
        c2, c142, lp2 = m.chd_decoder.decode_chords(z, keep=keep, return_logprob=True)
        assert torch.equal(c2, c) and torch.equal(c142, c14)
        assert all(torch.equal(a, b) for a, b in zip(m.chd_decoder.last_chord_logits, raw))
        assert (host(lp2.forced) == np.array([8, 96, 8])).all() and (host(lp2.logq) == 0).all() and not host(lp2.err).any()
        assert torch.equal(lp2.logp, lp.logp) and torch.equal(lp2.step_logp, lp.step_logp)
        assert (host(lp2.step_forced) == np.array([1, 12, 1])).all()
    finally:
        m.set_precision('fp32')


def test_partial_keep_redraws_the_rest():
    m, z = with_precision('bf16'), latents()
    try:
        other = decode(m, z, 1.0, 0.5, draw=DRAW + 1)[0]
        steps = torch.zeros(1, 8, dtype=torch.bool, device=DEV)
        steps[0, :4] = True
        for keep in (model().keep_chords(other, range(4)), model().keep_chords(other, steps), model().keep_chords(other, steps.expand(B, 8))):
            c, _, lp, logits, d = decode(m, z, 1.0, 0.5, keep=keep)
            assert torch.equal(c[:, :4], other[:, :4]) and not torch.equal(c[:, 4:], other[:, 4:])
            explained(logits, d, noise(0, B), 1.0, 0.5, 'after a kept first bar', steps=slice(4, 8))
            assert not host(lp.err).any() and (host(lp.forced) == np.array([4, 48, 4])).all()
            assert (host(lp.step_logq)[:, :4] == 0).all() and (host(lp.step_logq)[:, 4:] <= 0).all() and (host(lp.logq) < 0).all()
        bad = other.clone()
        bad[5, 2, 0:12] = 0                                  # a root block without an entry: that decision stays free, the row reports it
        _, _, lp, _, _ = decode(m, z, 1.0, 0.5, keep=model().keep_chords(bad, range(4)))
        e = host(lp.err)
        assert e[5] == 1 and e.sum() == 1 and host(lp.forced)[5].tolist() == [3, 48, 4]
    finally:
        m.set_precision('fp32')


def decisive_gap(logits):
    """per row the smallest gap between the two best classes over its 112 decisions"""
    root, chroma, bass = (a.astype(np.float64) for a in logits)
    top = lambda v: np.sort(v, -1)[..., -1] - np.sort(v, -1)[..., -2]
    return np.minimum(np.minimum(top(root).min(1), top(bass).min(1)), np.abs(chroma[..., 1] - chroma[..., 0]).reshape(len(root), -1).min(1))


def test_one_row_batches_agree_with_decode_tokens():
    """at B = 1 the union over the batch is the row's own token: decode_chords(z)[b] is decode_tokens(z[b:b+1]), but for rows with a
    decision closer than GAP in the new path's own logits (a product over 64 rows and one over 1 row round differently)"""
    m, z = with_precision('fp32'), latents()
    c, c14, _, logits, _ = decode(m, z)
    skip = decisive_gap(logits) < GAP
    print('rows with a decisive gap below %g: %s' % (GAP, np.nonzero(skip)[0].tolist()))
    assert skip.sum() <= MAX_SKIPPED_ROWS
    for b in range(B):
        c1, c141 = m.chd_decoder.decode_tokens(z[b:b + 1])
        if not skip[b]:
            assert torch.equal(c1[0], c[b]) and torch.equal(c141[0], c14[b]), b
    cu, _ = m.chd_decoder.decode_tokens(z)
    differ = (host(cu) != host(c)).reshape(B, -1).any(1)
    print('decode_tokens(z) at B = 64 (the union over the batch) differs from decode_chords(z) on %d of 64 rows' % differ.sum())
    assert differ.any()                                      # the batch dependence the new path removes (on an MI355X: 64 of 64 rows)


def sequenced(P, z, prec, blk, keep):
    """the launches of ptv_chord_decode, sequenced from Python through the same entry points -> the composite's outputs by name"""
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
    for t in range(T):
        F_.gemm(tok, w_ih[:, :I], gi, prec=prec)
        FF_.gru_step(prec, hall[t], gi, 3 * H, P['gru.weight_hh_l0'], P['gru.bias_hh_l0'], hall[t + 1], gi2=zg)
        F_.gemm(hall[t + 1], P['root_out.weight'], root[t], bias=P['root_out.bias'], prec=prec)
        F_.gemm(hall[t + 1], P['chroma_out.weight'], chroma[t], bias=P['chroma_out.bias'], prec=prec)
        F_.gemm(hall[t + 1], P['bass_out.weight'], bass[t], bias=P['bass_out.bias'], prec=prec)
        call('ptv_chord_decide', ptr(root[t]), ptr(chroma[t]), ptr(bass[t]), n, t, ptr(blk), ptr(keep.c) if keep else None,
             ptr(keep.steps) if keep else None, keep.steps.shape[0] if keep else 0, ptr(tok) if t + 1 < T else None, ptr(c), ptr(c14), ptr(sp),
             ptr(sq), ptr(sf), ptr(se), stream_ptr())
    lp, lq, f, er = e(n, 3), e(n, 3), i(n, 3), i(n)
    call('ptv_chord_logprob_fold', ptr(sp), ptr(sq), ptr(sf), ptr(se), n, ptr(lp), ptr(lq), ptr(f), ptr(er), stream_ptr())
    return dict(c=c, chord14=c14, root=root, chroma=chroma, bass=bass, logp=lp, logq=lq, forced=f, err=er, step_logp=sp, step_logq=sq,
                step_forced=sf)


@pytest.mark.parametrize('n', [3, 70])
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
            for blk, kp in ((None, None), (KT.block(1.0, 0.7, 9), None), (KT.block(0.8, 0.0, 9), keep)):
                calls = FF_._CDS.get('calls', 0)
                got = FF_.chord_decode(z, P, pc, blk, kp)
                assert FF_._CDS['calls'] == calls + 1                                       # the composite really ran
                want = sequenced(P, z, pc, blk, kp)
                flat = dict(got._asdict(), **got.logprob._asdict())
                for k, v in want.items():
                    assert torch.equal(flat[k], v), (k, blk is not None, kp is not None)
                if kp is not None:
                    assert torch.equal(got.c[steps], first.c[steps]) and host(got.logprob.forced).sum() > 0
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
        # without the keywords: today's call -- the chords are decode_tokens', the counter stays
        plain = m.decode_to_inputs(zc, zr)
        assert len(plain) == 6 and torch.equal(plain[2], m.chd_decoder.decode_tokens(zc)[0]) and m._sample_draws == 3
        assert len(m.decode_logprob(zc, zr)) == 7
        # with them: c is decode_chords' with the same seed, draw and offset; one call, one draw
        out = m.decode_to_inputs(zc, zr, chord_temperature=1.0, chroma_temperature=0.5)
        assert len(out) == 6 and m._sample_draws == 4
        want = m.chd_decoder.decode_chords(zc, temperature=1.0, chroma_temperature=0.5, seed=SEED, draw=3, sample_offset=32)[0]
        assert torch.equal(out[2], want) and not torch.equal(out[2], plain[2])
        for a, b in zip(out[:2] + out[3:], plain[:2] + plain[3:]):                          # the note decode is untouched
            assert torch.equal(a, b)
        both = m.decode_to_inputs(zc, zr, temperature=1.0, chord_temperature=1.0, return_logprob=True)      # both decoders sample: one draw
        assert len(both) == 8 and m._sample_draws == 5 and isinstance(both[7], FF_.ChordLogprob)
        assert torch.equal(both[2], m.chd_decoder.decode_chords(zc, temperature=1.0, seed=SEED, draw=4, sample_offset=32)[0])
        assert torch.equal(both[1], m.decode_to_inputs(zc, zr, temperature=1.0, draw=4)[1]) and m._sample_draws == 5
        named = m.decode_logprob(zc, zr, chord_temperature=0.7, seed=5, draw=9, sample_offset=2)
        assert len(named) == 8 and m._sample_draws == 5
        again = m.decode_logprob(zc, zr, chord_temperature=0.7, seed=5, draw=9, sample_offset=2)
        assert all(torch.equal(a, b) for a, b in zip(named[7], again[7])) and torch.equal(named[2], again[2])   # the same bits
        assert torch.equal(named[2], m.decode_chords(zc, chord_temperature=0.7, seed=5, draw=9, sample_offset=2)[0])
        # the model's own decode_chords: seed / offset from use_philox, the counter advances once per sampled call
        c, c14 = m.decode_chords(zc, chord_temperature=1.0)
        assert m._sample_draws == 6 and torch.equal(c, m.chd_decoder.decode_chords(zc, temperature=1.0, seed=SEED, draw=5, sample_offset=32)[0])
        c0, _, lp0 = m.decode_chords(zc, return_logprob=True)
        assert m._sample_draws == 6 and (host(lp0.logq) == 0).all() and c14.shape == (4, 8, 14)
        # kept chords through the output path and through reencode
        keep = m.keep_chords(c, range(4))
        kept = m.decode_to_inputs(zc, zr, keep_chords=keep, return_logprob=True)
        assert m._sample_draws == 6 and torch.equal(kept[2][:, :4], c[:, :4]) and (host(kept[7].forced) == np.array([4, 48, 4])).all()
        d1, _ = m.reencode(zc, zr, chord_temperature=1.0, draw=5)
        d2 = m.inference_encode(m.decode_to_inputs(zc, zr)[0], c)[0]
        assert torch.equal(d1.mean, d2.mean) and not torch.equal(d1.mean, m.reencode(zc, zr)[0].mean)
        # refusals: a ValueError, no launch, no counter change
        launches = dict(FF_._CDS)
        steps = torch.ones(3, 8, dtype=torch.uint8, device=DEV)
        for kw in (dict(chord_temperature=-1.0), dict(chord_temperature=float('inf')), dict(chroma_temperature=0.5),
                   dict(keep_chords=m.keep_chords(c[:3].contiguous(), range(2))), dict(keep_chords=FF_.ChordKeep(c, steps, 4))):
            for f in (lambda: m.decode_to_inputs(zc, zr, **kw), lambda: m.decode_chords(zc, **kw), lambda: m.reencode(zc, zr, **kw)):
                with pytest.raises(ValueError):
                    f()
        for kw in (dict(seed=1), dict(draw=1), dict(sample_offset=1)):
            with pytest.raises(ValueError):
                m.decode_to_inputs(zc, zr, keep_chords=keep, **kw)
            with pytest.raises(ValueError):
                m.decode_chords(zc, **kw)
        for bad in ((c, torch.ones(4, 7, dtype=torch.uint8, device=DEV)), (c, steps), (c.cpu(), range(2)), (c.double(), range(2)), (c, [8])):
            with pytest.raises(ValueError):
                m.keep_chords(*bad)
        assert m._sample_draws == 6 and dict(FF_._CDS) == launches
    finally:
        m._philox = None
        m._sample_draws = 0
        m.set_precision('fp32')
