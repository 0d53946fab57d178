"""GPU: kept rhythm in the free-running decode (DisentangleVAE.keep_rhythm, keep=; INTEGRATION.md "Kept rhythm") against tests/rhythm_ref.py on
every selectable note-loop path: the rhythm comes out, the free decisions are the documented draw, promotion to the constrained kind alone
changes nothing, the fixed point, the log-probability pass, graph replay, best-of-n, causality and the surface.  B = 32; the model, latents,
paths and noise are those of tests/test_gpu_truncated_sampling.py, the grid with its hand-made steps and the constrained setting (chord mask
+ ascending + top_k = 8 + top_p = 0.9) those of tests/test_gpu_keep_decode.py.  The keep: rhythm steps at (t + b) % 4 < 2, row 1 whole.
Under `ascending` a decode of this untrained model climbs fast: a draw lands anywhere among the allowed pitches above lo, so about five
notes exhaust the range whatever the mask (on test_gpu_keep_decode's grid as it is, 99 of the 496 rhythm steps ended in the fallback under
the chord mask, and between 73 and 128 under seven other masks, a plain 40..100 range among them).  So that the fallback happens at least
once and at no more than 5 % of the rhythm steps, as test 1 asserts on the emitted logits, the mask stays the chord mask and the RHYTHM is
thinned instead: a step of 3 .. 13 notes keeps its first two (the hand-made steps with a pitch that is no note stay as they are; the 14- and
15-note steps of rows 9 and 10 and the rhythm steps whose chord has no tone at all are the fallbacks that are certain)."""
import functools

import numpy as np
import pytest
import torch

import logprob_ref as LR
import rhythm_ref as RR
import sample_ref as S
import test_gpu_constrained_decode as CD
import test_gpu_decode_logprob_kernels as LK
import test_gpu_keep_decode as KD
import test_gpu_keep_rhythm_kernels as RK
import test_gpu_truncated_sampling as TT
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
B = 32
SKIP_CAP = 0.005
SETTINGS = ('argmax', 'sampled', 'cons')
FALLBACK_MAX = 0.05
EOS = 129
dev = KD.dev


@functools.lru_cache(maxsize=None)
def crafted():
    """(x [32, 32, 16, 6], rhythm selection, whole selection uint8 [32, 32], mode, {durations: rhythm_ref.build})"""
    x = KD.crafted()[0].copy()
    for b in range(B):
        for t in range(32):
            K = RR.note_count(x[b, t, :, 0])
            p = x[b, t, 1:K + 1, 0]
            if 3 <= K <= 13 and ((p >= 0) & (p < 128)).all():
                x[b, t, 3] = (EOS, 2, 2, 2, 2, 2)
                x[b, t, 4:] = (130, 2, 2, 2, 2, 2)
    x.setflags(write=False)
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    rsel = ((t_ + b_) % 4 < 2).astype(np.uint8)
    wsel = np.zeros((B, 32), dtype=np.uint8)
    wsel[1] = 1
    mode = np.where(wsel != 0, 1, 3 * rsel).astype(np.uint8)
    refs = {d: RR.build(x, mode, d) for d in (True, False)}
    for a in (rsel, wsel, mode) + tuple(refs[True].values()) + tuple(refs[False].values()):
        a.setflags(write=False)
    return x, rsel, wsel, mode, refs


MASK_HI = 127                                                      # the top of the constrained setting's pitch range (see the docstring)


@functools.lru_cache(maxsize=None)
def mask_pair():
    """(device int32 [32, 32, 4], the same as numpy): the chord tones of synth_batch's c up to pitch MASK_HI (DisentangleVAE.pitch_mask)"""
    c = torch.from_numpy(synth_batch(B, 5)[1]).to(DEV)
    mask = TT.model().pitch_mask(c=c, hi=MASK_HI)
    torch.cuda.synchronize()
    m = mask.cpu().numpy()
    m.setflags(write=False)
    return mask, m


def cons_block(offset=0, rows=slice(None)):
    return TT.block(offset, pitch_mask=mask_pair()[0][rows].contiguous(), **KD.CONS)


def keep_of(x, rsel, wsel=None, **kw):
    out = TT.model().keep_rhythm(dev(x), dev(rsel), whole_steps=None if wsel is None else dev(wsel), **kw)
    torch.cuda.synchronize()
    return out


def halves(z):
    return z[:, :256].contiguous(), z[:, 256:].contiguous()


def blocks():
    """the three settings as blocks of the constrained kind, which a RhythmKeep needs one level under the model: the constrained argmax,
    plain sampling with the vacuous constraint, the constrained truncated setting"""
    return {'argmax': TT.block(0, 0.0, 0.0, ascending=False), 'sampled': TT.block(0, ascending=False), 'cons': cons_block()}


def setting_kw(name):
    return dict(KD.CONS, pitch_mask=mask_pair()[0]) if name == 'cons' else {}


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: the crafted rhythm keep with and without its durations under the three settings"""
    attrs, prec = PATHS[path]
    x, rsel, wsel, _, _ = crafted()
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            for d in (True, False):
                kp = keep_of(x, rsel, wsel, durations=d)
                for name, blk in blocks().items():
                    out[name, d] = KD.kdecode(m, z, blk, kp)
    finally:
        m.set_precision('bf16')
    return out


def words_of(ref):
    """the pitch force words of a reference as [B, 32, 15]"""
    n = ref['pitch'].shape[1] // 32
    return ref['pitch'].reshape(15, 32, n).transpose(2, 1, 0)


def notes_len(xh):
    """int [B, 32]: the decisions of each step of a decoded grid [B, 32, 15, 6] before its first <eos>"""
    eos = xh[..., 0] == EOS
    return np.where(eos.any(-1), eos.argmax(-1), 15)


def fallbacks(xh, ref, kw, mask_np):
    """bool [B, 32, 15]: rhythm_ref's verdict, on the decode's own mask rows and running lo, that a -2 decision had nothing but <eos>"""
    return RR.fallback(CD.allowed_of(xh, kw, mask_np), words_of(ref))


def expected_len(xh, ref, kw, mask_np):
    """int [B, 32]: K of a rhythm step -- or the note step of its first fallback, which ends it early"""
    fall = fallbacks(xh, ref, kw, mask_np)
    return np.where(fall.any(-1), fall.argmax(-1), ref['K']), fall


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', list(PATHS))
def test_1_the_rhythm_comes_out(path):
    """at a rhythm step the decoded step has K notes -- but where rhythm_ref, on the emitted logits' own mask rows and lo, says the fallback
    ended it early -- and with durations=True x's bits; without a mask and `ascending` there is no fallback at all, under the chord mask
    with `ascending` at least one and at most 5 % of the rhythm steps; the pitches differ from x somewhere; whole steps equal x"""
    x, _, _, mode, refs = crafted()
    r = runs(path)
    _, mask_np = mask_pair()
    rh = mode == 3
    assert rh.sum() > 400
    for d in (True, False):
        ref = refs[d]
        fp, fd, ne = ref['forced_pitch'], ref['forced_dur'], ref['not_eos']
        for name in SETTINGS:
            xh = r[name, d][2]
            want, fall = expected_len(xh, ref, setting_kw(name), mask_np)
            short = fall.any(-1) & rh
            print('%s %s durations=%s: %d rhythm steps, %d ended early by the fallback (share %.4f)'
                  % (path, name, d, rh.sum(), short.sum(), short.sum() / rh.sum()))
            assert np.array_equal(notes_len(xh)[rh], want[rh]), (path, name, d, np.argwhere((notes_len(xh) != want) & rh)[:4])
            if name == 'cons':
                assert 1 <= short.sum() <= FALLBACK_MAX * rh.sum(), (path, d, short.sum())
            else:
                assert not fall.any() and np.array_equal(notes_len(xh)[rh], ref['K'][rh])
            assert np.array_equal(xh[..., 1:][fd], x[:, :, 1:, 1:][fd]), (path, name, d)
            assert np.array_equal(xh[..., 0][fp], np.where(rh[..., None], EOS, x[:, :, 1:, 0])[fp]), (path, name, d)
            assert (xh[..., 0][ne] != x[:, :, 1:, 0][ne]).any()
            whole = (mode == 1)[..., None]
            assert np.array_equal(xh[..., 0][fp & whole], x[:, :, 1:, 0][fp & whole]) and (fp & whole).sum() > 50
    assert refs[True]['forced_dur'][rh].sum() > 1500 and not refs[False]['forced_dur'][rh].any() and refs[False]['forced_dur'][1].any()
    bits = refs[True]['forced_dur'] & ~refs[False]['forced_dur']
    assert (r['sampled', False][2][..., 1:][bits] != x[:, :, 1:, 1:][bits]).any()          # durations=False: the bits are drawn


def explained_free(po, do, xh, pn, dn, kw, mask_np, ref, what):
    """test_gpu_keep_decode.explained_free with rhythm_ref's not_eos map: every free pitch decision is rhythm_ref.decide_pitch on the emitted
    logits -- over the allowed set without <eos> where the word is -2 --, every free duration decision sample_ref.decide_dur; skipped:
    decisions sample_ref.skippable, at most SKIP_CAP of the free ones"""
    k, l, q = CD.rule(kw)
    al = CD.allowed_of(xh, kw, mask_np)
    words = words_of(ref)
    want_p = RR.decide_pitch(po, pn, al, words, KD.T_PITCH, k, l, q)
    skip_p = RR.skippable(po, pn, al, words, KD.T_PITCH, k, l, q)
    want_d = S.decide_dur(do, dn, KD.T_DUR)
    skip_d = S.skippable(do, dn, KD.T_DUR, S.NOISE_TOL)
    free_p, free_d = ~ref['forced_pitch'], ~ref['forced_dur']
    bad_p = (xh[..., 0] != want_p) & ~skip_p & free_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d & free_d
    share_p, share_d = skip_p[free_p].mean(), skip_d[free_d].mean()
    print('%s: free pitch decisions %d of %d (%d of them not <eos>), skipped %d (share %.5f); free duration decisions %d of %d, skipped %d '
          '(share %.5f)' % (what, free_p.sum(), free_p.size, ref['not_eos'].sum(), skip_p[free_p].sum(), share_p, free_d.sum(), free_d.size,
                            skip_d[free_d].sum(), share_d))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert share_p <= SKIP_CAP and share_d <= SKIP_CAP
    assert np.take_along_axis(RR.allowed(al, words), xh[..., :1], -1)[..., 0][free_p].all()    # a free decision is a class of the reduced set


@pytest.mark.parametrize('path', list(PATHS))
def test_2_free_decisions_are_the_documented_draw(path):
    _, _, _, _, refs = crafted()
    r = runs(path)
    pn, dn = TT.noise(0, B)
    _, mask_np = mask_pair()
    for d in (True, False):
        for name in ('cons', 'sampled'):
            po, do, xh = r[name, d]
            explained_free(po, do, xh, pn, dn, setting_kw(name), mask_np, refs[d], '%s %s rhythm keep, durations=%s' % (path, name, d))


def last_logits(m):
    last = m.decoder._last_decode
    return last.pitch.clone(), last.dur.clone(), None if last.sampling is None else last.sampling.numel()


@pytest.mark.parametrize('path', ('default', 'bf16-step-loop'))
def test_3_promotion_alone_changes_nothing(path):
    """a rhythm keep with no step selected sends the decode as the constrained kind (an eight-word block with flags 0 and no mask) and
    gives the grid and the logits of the same decode without a keep, bit for bit -- under argmax and under plain sampling"""
    attrs, prec = PATHS[path]
    x = crafted()[0]
    m = TT.model()
    m.set_precision(prec)
    zc, zr = halves(TT.latents())
    try:
        with TT.patched(attrs):
            kp = m.keep_rhythm(dev(x), [])
            assert isinstance(kp, FF_.RhythmKeep) and int((kp.pitch != -1).sum()) == 0 and int((kp.dur != -1).sum()) == 0
            for kw, words in ((dict(), None), (dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW), 4)):
                a = m.inference_decode(zc, zr, **kw)
                la = last_logits(m)
                b = m.inference_decode(zc, zr, keep=kp, **kw)
                lb = last_logits(m)
                assert la[2] == words and lb[2] == 8
                assert np.array_equal(a, b) and torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1]), (path, kw)
    finally:
        m.set_precision('bf16')


@pytest.mark.parametrize('path', ('default', 'cluster4', 'split', 'bf16-step-loop'))
def test_4_fixed_point(path):
    """the output of a rhythm-keep decode, kept WHOLE (DisentangleVAE.keep) and decoded with the same block: the same grid, bit-equal logits
    -- under plain sampling everywhere.  Under the constrained setting everywhere but behind the <eos> of a step the fallback ended: there
    the rhythm keep still forced x's duration bits on the decisions up to K, which the whole keep of the shorter step leaves free; those
    slots lie behind the step's end, and no later time step differs"""
    attrs, prec = PATHS[path]
    x, rsel, wsel, _, refs = crafted()
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            for name in ('sampled', 'cons'):
                a = KD.kdecode(m, z, blocks()[name], keep_of(x, rsel, wsel))
                own = m.decoder.last_xhat.clone()
                kp = m.keep(own, range(32))
                assert type(kp) is FF_.Keep and int(kp.err.sum()) == 0
                out[name] = (a, KD.kdecode(m, z, blocks()[name], kp))
    finally:
        m.set_precision('bf16')
    for u, v, what in zip(*out['sampled'], ('pitch logits', 'duration logits', 'grid')):
        assert np.array_equal(u, v), (path, 'sampled', what)
    a, b = out['cons']
    _, fall = expected_len(a[2], refs[True], setting_kw('cons'), mask_pair()[1])
    behind = np.arange(15)[None, None, :] > notes_len(a[2])[..., None]                     # the slots behind the first <eos>
    same = ~(fall.any(-1)[..., None] & behind)
    assert fall.any() and not same.all()
    for u, v, what in zip(a, b, ('pitch logits', 'duration logits', 'grid')):
        assert np.array_equal(u[same], v[same]), (path, 'cons', what)


def test_5_decode_logprob():
    """the log-probability pass after a constrained sampled rhythm-keep decode of the first 8 rows (the fp64 restatement walks every decision
    in Python): counts, err and the four sums against logprob_ref over the support the device reports with the keep's words
    (ptv_debug_pitch_constrain_words), at the tolerance of tests/test_gpu_decode_logprob_kernels.py; the -2 decisions count as free, the
    forced <eos> as forced; err 0.  With temperature=None and a rhythm keep logq is exactly 0"""
    x, rsel, wsel, mode, refs = crafted()
    n = 8
    m = TT.model()
    zc, zr = halves(TT.latents()[:n])
    mask = mask_pair()[0][:n].contiguous()
    kp, kept_n = m.keep_rhythm(dev(x[:n]), dev(rsel[:n]), whole_steps=dev(wsel[:n]), return_counts=True)
    ref = RR.build(x[:n], mode[:n])
    assert np.array_equal(kept_n.cpu().numpy(), ref['kept_n']) and np.array_equal(kp.pitch.cpu().numpy(), ref['pitch'])
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW, **KD.CONS)
    lp = m.decode_logprob(zc, zr, keep=kp, pitch_mask=mask, **kw)[6]
    torch.cuda.synchronize()
    last = m.decoder._last_decode
    assert last.sampling.numel() == 8
    pitch = LK.host(last.pitch.permute(2, 1, 0, 3))
    dur = LK.host(last.dur.view(15, 32, n, 5, 2).permute(2, 1, 0, 3, 4))
    xg = LK.host(last.xhat)
    finite = np.where(LR.counted(xg)[0][..., None], pitch, np.float32(0))
    kept = RK.kept_with_words(kw, xg, finite, LK.host(mask), ref['pitch'])
    r_lp, r_cn, r_er, scale = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, ref['pitch'], ref['dur'])
    f_lp = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, ref['pitch'], ref['dur'], dtype=np.float32)[0]
    got, cn = LK.host(lp.step_logp), LK.host(lp.step_counts)
    assert np.array_equal(cn, r_cn) and np.array_equal(LK.host(lp.err), r_er) and not r_er[np.arange(n) != 1].any()
    for col, fam in enumerate(('logp pitch', 'logp dur', 'logq pitch', 'logq dur')):
        LK.check('rhythm keep %s' % fam, got[..., col], r_lp[..., col], f_lp[..., col], scale[..., col])
    s, c = LR.fold(got, cn, np.float32)
    assert torch.cat([lp.logp, lp.logq], 1).cpu().numpy().tobytes() == s.tobytes() and np.array_equal(LK.host(lp.counts), c)
    # the counts: at a rhythm step that came out whole, K free decisions and the forced <eos>
    rh = mode[:n] == 3
    length = notes_len(xg[:, :, 1:])
    full = rh & (length == ref['K']) & (ref['K'] < 15)
    assert full.sum() > 60 and (cn[..., 2][full] == 1).all() and np.array_equal(cn[..., 0][full], ref['K'][full] + 1)
    assert (got[..., 2][full & (ref['K'] > 0)] < 0).any() and not got[..., 2][rh & (ref['K'] == 0)].any()
    lp0 = m.decode_logprob(zc, zr, keep=kp)[6]
    assert m.decoder._last_decode.sampling.numel() == 8
    assert not LK.host(lp0.logq).any() and not LK.host(lp0.step_logp)[..., 2:].any() and (LK.host(lp0.logp)[:, 0] < 0).all()
    assert not LK.host(lp0.err)[np.arange(n) != 1].any()


def test_6_graph_replay():
    """captured with one rhythm keep, replayed with another (other steps, durations=False) and with a whole keep: ONE capture of the
    (constrained kind, a keep) graph serves them all, each replay equal to its eager decode"""
    x, rsel, wsel, _, _ = crafted()
    m = TT.model()
    zc, zr = halves(TT.latents()[:16])
    xd = dev(x[:16])
    keeps = [m.keep_rhythm(xd, dev(rsel[:16]), whole_steps=dev(wsel[:16])), m.keep_rhythm(xd, range(8, 32), durations=False),
             m.keep(xd, dev(rsel[:16]))]
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=9, draw=5, ascending=False)        # (the whole keep asks for the kind itself)
    eager = [m.inference_decode(zc, zr, keep=k, **kw) for k in keeps]
    assert all((eager[i] != eager[j]).any() for i in range(3) for j in range(i))
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[0], **kw), eager[0])
        held = len(m.decoder._graphs)
        assert m.decoder.graph_captures == before + 1
        for i in (1, 2, 0, 1):
            assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[i], **kw), eager[i]), i
        assert m.decoder.graph_captures == before + 1 and len(m.decoder._graphs) == held
        kw.pop('ascending')                                                                    # the promotion picks the same graph
        assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[1], **kw), eager[1])
        assert m.decoder.graph_captures == before + 1 and len(m.decoder._graphs) == held
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_decode_best_of():
    """decode_best_of(n = 3) with a rhythm keep of B rows and no constraint of its own (the tiled request promotes too): the candidates are
    the rows of a plain decode of the batch tiled three times with the keep built from the tiled grid, EVERY candidate has the rhythm,
    and the winner is the first candidate with the largest logp"""
    x, rsel, wsel, mode, refs = crafted()
    m = TT.model()
    zc, zr = halves(TT.latents())
    n = 3
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=6, top_k=8)
    xd, rd, wd = dev(x), dev(rsel), dev(wsel)
    keep = m.keep_rhythm(xd, rd, whole_steps=wd)
    tiled = m.keep_rhythm(xd.repeat(n, 1, 1, 1), rd.repeat(n, 1), whole_steps=wd.repeat(n, 1))
    plain = m.decode_logprob(zc.repeat(n, 1), zr.repeat(n, 1), keep=tiled, **kw)
    cand = m.decoder.last_xhat[:, :, 1:].cpu().numpy()             # [3 B, 32, 15, 6]: every candidate's decided grid
    out = m.decode_best_of(zc, zr, n, keep=keep, **kw)
    torch.cuda.synchronize()
    assert m.decoder._last_decode.sampling.numel() == 8
    rh = np.tile(mode == 3, (n, 1))
    K = np.tile(refs[True]['K'], (n, 1))
    assert np.array_equal(notes_len(cand)[rh], K[rh])
    fd = np.tile(refs[True]['forced_dur'], (n, 1, 1, 1))
    assert np.array_equal(cand[..., 1:][fd], np.tile(x[:, :, 1:, 1:], (n, 1, 1, 1))[fd])
    assert (cand[:B] != cand[B:2 * B]).any() and (cand[B:2 * B] != cand[2 * B:]).any()
    lp = plain[6]
    score = lp.logp.sum(1).cpu().numpy()
    want, _ = LR.best_of(score.reshape(n, B))
    best = out[6].cpu().numpy()
    assert np.array_equal(best, want) and len(set(best.tolist())) > 1
    rows = torch.from_numpy(want.astype(np.int64) * B + np.arange(B)).to(DEV)
    assert torch.equal(out[1], plain[1][rows]) and torch.equal(out[0], plain[0][rows])
    assert torch.equal(out[7], torch.cat([lp.logp, lp.logq], 1)[rows])


def test_8_causality():
    """changing row 5's keep -- its grid, its selection, its durations -- changes no other row's grid or logits"""
    x, rsel, wsel, _, _ = crafted()
    m = TT.model()
    z = TT.latents()
    x2, r2 = x.copy(), rsel.copy()
    x2[5] = synth_batch(B, 9)[0][5]
    r2[5] = 1 - rsel[5]
    a = KD.kdecode(m, z, cons_block(), keep_of(x, rsel, wsel))
    b = KD.kdecode(m, z, cons_block(), keep_of(x2, r2, wsel))
    others = np.arange(B) != 5
    assert (a[2][5] != b[2][5]).any()
    for u, v in zip(a, b):
        assert np.array_equal(u[others], v[others])


def test_9_surface():
    x, rsel, wsel, _, refs = crafted()
    m = TT.model()
    Bs = 4
    zc, zr = halves(TT.latents()[:Bs])
    xd = dev(x[:Bs])
    rd, wd = dev(rsel[:Bs]), dev(wsel[:Bs])
    # ---- DisentangleVAE.keep_rhythm: every bad argument is a ValueError before any launch
    for bad_x in (xd.cpu(), xd.int(), xd[:, :, :15], xd[0]):
        with pytest.raises(ValueError):
            m.keep_rhythm(bad_x, range(4))
    for bad in (dict(steps=rd.cpu()), dict(steps=rd.int()), dict(steps=dev(rsel[:3])), dict(steps=rd[:, :31]), dict(steps=rd[0]),
                dict(steps=[32]), dict(steps=[-1]), dict(steps=[0.5]), dict(steps=7), dict(steps=None), dict(whole_steps=wd[0]),
                dict(whole_steps=wd.cpu()), dict(whole_steps=[40]), dict(durations=1), dict(durations=None)):
        with pytest.raises(ValueError):
            m.keep_rhythm(xd, **dict(dict(steps=rd), **bad))
    # ---- what comes back: a RhythmKeep that passes for a Keep; host and device selections; a step in both is a whole step
    kp, kept_n = m.keep_rhythm(xd, rd, whole_steps=wd, return_counts=True)
    torch.cuda.synchronize()
    assert isinstance(kp, FF_.RhythmKeep) and isinstance(kp, FF_.Keep) and kp.batch == Bs and kp._fields == FF_.Keep._fields
    FF_.check_keep(kp, Bs)
    want = RR.build(x[:Bs], np.where(wsel[:Bs] != 0, 1, 3 * rsel[:Bs]).astype(np.uint8))
    for got, k in ((kp.pitch, 'pitch'), (kp.dur, 'dur'), (kp.err, 'err'), (kept_n, 'kept_n')):
        assert np.array_equal(got.cpu().numpy(), want[k]), k
    host = m.keep_rhythm(xd, range(32), whole_steps=slice(0, 4), durations=False)
    want = RR.build(x[:Bs], np.array([[1] * 4 + [3] * 28], dtype=np.uint8), durations=False)
    assert np.array_equal(host.pitch.cpu().numpy(), want['pitch']) and np.array_equal(host.dur.cpu().numpy(), want['dur'])
    assert type(m.keep_rhythm(xd, rd.bool())) is FF_.RhythmKeep
    # ---- one level down: a RhythmKeep beside anything but a constrained block is refused before any launch
    dec_z = torch.cat([zc, zr], -1)
    m.decoder._last_decode = None
    for blk in (None, TT.block(0), TT.block(0, top_k=8)):
        with pytest.raises(ValueError):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=blk, keep=kp)
    assert m.decoder._last_decode is None
    with torch.no_grad():
        m.decoder(dec_z, True, None, None, 0., 0., sampling=TT.block(0, ascending=False), keep=kp)
    # ---- like any keep: a wrong batch, together with force_trace -- before anything is encoded or launched
    draws = m._sample_draws
    other = m.keep_rhythm(dev(x[:8]), range(4))
    trace = TT.trace_of(np.zeros((Bs, 32, 15, 6), dtype=np.int64))
    _, c_np, pr_np = synth_batch(Bs, 5)
    c, pr = dev(c_np), dev(pr_np)
    for bad, ft in ((other, None), (kp, trace)):
        m.decoder.force_trace = ft
        try:
            for fn in (lambda: m.inference_decode(zc, zr, temperature=1.0, keep=bad), lambda: m.decode_to_inputs(zc, zr, keep=bad),
                       lambda: m.swap(pr, pr, c, c, True, True, temperature=1.0, keep=bad),
                       lambda: m.decode_best_of(zc, zr, 2, temperature=1.0, keep=bad)):
                with pytest.raises(ValueError):
                    fn()
        finally:
            m.decoder.force_trace = None
    assert m._sample_draws == draws
    # ---- every entry point takes it: the rhythm of the kept steps comes out of decode_to_inputs, swap and reencode's decode
    K = want_k = RR.build(x[:Bs], np.where(wsel[:Bs] != 0, 1, 3 * rsel[:Bs]).astype(np.uint8))['K']
    rh = K >= 0
    m.decode_to_inputs(zc, zr, temperature=1.0, keep=kp)
    assert np.array_equal(notes_len(m.decoder.last_xhat[:, :, 1:].cpu().numpy())[rh], want_k[rh])
    est = m.swap(pr, pr, c, c, True, True, keep=kp)
    assert np.array_equal(notes_len(est)[rh], want_k[rh]) and m._sample_draws == draws + 1
    m.reencode(zc, zr, temperature=0.8, keep=kp)
    assert np.array_equal(notes_len(m.decoder.last_xhat[:, :, 1:].cpu().numpy())[rh], want_k[rh])
