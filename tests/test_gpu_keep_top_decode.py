"""GPU: kept top voice in the free-running decode (DisentangleVAE.keep_top, keep=; INTEGRATION.md "Kept top voice") against tests/top_ref.py on
every selectable note-loop path: the note count, the kept notes and the <eos> come out exactly, the free decisions are the documented draw
under their ceilings, an empty TopKeep is the `ascending` decode, the fixed point, the log-probability pass, graph replay, best-of-n,
causality and the surface.  B = 32; the model, latents, paths and noise are those of tests/test_gpu_truncated_sampling.py, the grid with its
hand-made steps and the constrained setting (chord mask + ascending + top_k = 8 + top_p = 0.9) those of tests/test_gpu_keep_decode.py, the
chord mask that of tests/test_gpu_keep_rhythm_decode.py.  The keep: top steps at (t + b) % 4 < 2 with at most two notes kept, row 1 whole.

The relaxation (a ceiling decision whose lane holds no tone of the mask: the mask yields) has to happen at least twice under the chord
mask.  The grid is taken as it is: from the reference alone, before any decode, 5 top steps with a free decision lie on a chord
without a single tone (40 of the 1024 steps have such a chord; certain_relaxations() below counts the 5 and test 1 asserts at least 2);
there every free decision is relaxed whatever the logits are, so no step had to be given a one-tone chord.  One of the 5 lies in the
first eight rows, which the log-probability test decodes.

The guarantee -- K notes, the kept ones in their slots -- is stated for steps whose notes ascend strictly (err bit 0 clear).  The grid's
hand-made steps with a pitch that is no note (rows 5, 6, 7; row 1 is whole) raise that bit; they are decoded and explained like the others
but left out of the exact count, as the rule leaves them out ("the lane may be empty and the rule's last resort applies").

The fixed point (test 4) is asserted bit for bit under the room ceiling, where the ceilings depend on the kept pitch and the count alone,
so the second decode has the first one's force words.  Under lanes the ceilings of the second decode are the FIRST DECODE's own next
notes, not x's: the lane of a decision differs, another class can win the same noise, and the outputs need not be equal -- there the test
asserts what the feature promises (count, kept notes, interleaving with the new neighbours) and prints how many steps differ."""
import functools

import numpy as np
import pytest
import torch

import constrain_ref as CR
import logprob_ref as LR
import sample_ref as S
import test_gpu_constrained_decode as CD
import test_gpu_decode_logprob_kernels as LK
import test_gpu_keep_decode as KD
import test_gpu_keep_rhythm_decode as RD
import test_gpu_keep_rhythm_kernels as RK
import test_gpu_truncated_sampling as TT
import top_ref as TP
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
B = 32
SKIP_CAP = 0.005
SETTINGS = ('argmax', 'sampled', 'cons')
CONFIGS = ((True, True), (True, 'kept'), (False, True), (False, 'kept'))       # (lanes, durations)
HIGHEST = 2
EOS = 129
dev = KD.dev
halves = RD.halves
notes_len = RD.notes_len
words_of = RD.words_of
mask_pair = RD.mask_pair


@functools.lru_cache(maxsize=None)
def crafted():
    """(x [32, 32, 16, 6] -- test_gpu_keep_decode's grid as it is --, top selection, whole selection uint8 [32, 32], mode,
    {(lanes, durations): top_ref.build}, good bool [32, 32]: the top steps whose notes ascend strictly)"""
    x = KD.crafted()[0]
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    tsel = ((t_ + b_) % 4 < 2).astype(np.uint8)
    wsel = np.zeros((B, 32), dtype=np.uint8)
    wsel[1] = 1
    mode = np.where(wsel != 0, 1, 4 * tsel).astype(np.uint8)
    refs = {c: TP.build(x, mode, None, HIGHEST, durations=c[1], lanes=c[0]) for c in CONFIGS}
    good = np.zeros((B, 32), dtype=bool)
    for b in range(B):
        for t in range(32):
            good[b, t] = mode[b, t] == 4 and not TP.step_err(x[b, t, :, 0], int(refs[CONFIGS[0]]['K'][b, t]))
    for a in (tsel, wsel, mode, good) + tuple(v for r in refs.values() for v in r.values()):
        a.setflags(write=False)
    return x, tsel, wsel, mode, refs, good


def certain_relaxations(mask_np):
    """from the reference alone: the good top steps with a free decision whose chord has no tone at all -- every ceiling decision there is
    relaxed whatever the logits"""
    _, _, _, _, refs, good = crafted()
    r = refs[CONFIGS[0]]
    empty = ~CR.mask_bits(mask_np).any(-1)
    return int((good & (r['K'] - r['h'] > 0) & empty).sum())


def keep_of(x, tsel, wsel=None, lanes=True, durations=True, **kw):
    out = TT.model().keep_top(dev(x), dev(tsel), highest=HIGHEST, whole_steps=None if wsel is None else dev(wsel), lanes=lanes,
                              durations=durations, **kw)
    torch.cuda.synchronize()
    return out


def blocks():
    """the three settings as blocks of the constrained kind with the ascending flag, which a TopKeep needs one level under the model"""
    return {'argmax': TT.block(0, 0.0, 0.0, ascending=True), 'sampled': TT.block(0, ascending=True), 'cons': RD.cons_block()}


def setting_kw(name):
    return dict(KD.CONS, pitch_mask=mask_pair()[0]) if name == 'cons' else dict(ascending=True)


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: the crafted top keep in its four configurations under the three settings"""
    attrs, prec = PATHS[path]
    x, tsel, wsel, _, _, _ = crafted()
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            for c in CONFIGS:
                kp = keep_of(x, tsel, wsel, *c)
                for name, blk in blocks().items():
                    out[name, c] = KD.kdecode(m, z, blk, kp)
    finally:
        m.set_precision('bf16')
    return out


def allowed_of(xh, kw, mask_np, ref):
    """(al bool [B, 32, 15, 130], relaxed, empty_lane bool [B, 32, 15]) of a decode: top_ref's allowed rule on the mask rows of its samples,
    the running lo of its own decisions and the keep's words"""
    lo = CR.running_lo(xh[..., 0])
    mk = None if kw.get('pitch_mask') is None else np.broadcast_to(mask_np[:, :, None, :], xh.shape[:3] + (4,))
    return TP.allowed_grid(mk, lo, bool(kw.get('ascending')), words_of(ref))


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', list(PATHS))
def test_1_the_top_comes_out(path):
    """at every top step whose notes ascend, on every path, setting and configuration -- exactly, with no cap: the decoded step has K notes,
    the kept notes sit in their slots with their duration bits, the <eos> sits at K; the decisions ascend strictly and each ceiling
    decision lies under its ceiling (lanes: decision n < x's pitch n + 1).  Under the chord mask the relaxation, recomputed by top_ref
    from the decode's own lo and the mask, happened at least twice; no lane of a good step was empty.  Whole steps equal x"""
    x, _, _, mode, refs, good = crafted()
    r = runs(path)
    _, mask_np = mask_pair()
    top = mode == 4
    assert top.sum() > 400 and good.sum() > 400 and certain_relaxations(mask_np) >= 2
    xp = x[:, :, 1:, 0]
    for c in CONFIGS:
        ref = refs[c]
        fp, fd, ce, K, h = ref['forced_pitch'], ref['forced_dur'], ref['ceil'], ref['K'], ref['h']
        words = words_of(ref)
        for name in SETTINGS:
            xh = r[name, c][2]
            what = (path, name, c)
            assert np.array_equal(notes_len(xh)[good], K[good]), (what, np.argwhere((notes_len(xh) != K) & good)[:4])
            g3 = good[..., None]
            assert np.array_equal(xh[..., 0][fp & g3], words[fp & g3]), what
            n = np.arange(15)[None, None, :]
            kept = g3 & (n >= (K - h)[..., None]) & (n < K[..., None])
            assert np.array_equal(xh[..., 0][kept], xp[kept]) and kept.sum() > 400, what
            at_k = g3 & (n == K[..., None])
            assert (xh[..., 0][at_k] == EOS).all() and at_k.sum() > 300, what
            assert np.array_equal(xh[..., 1:][fd], x[:, :, 1:, 1:][fd]), what
            free = g3 & (ce > 0)
            assert free.sum() > 300 and (xh[..., 0][free] < ce[free]).all(), what
            if c[0]:
                nxt = np.concatenate([xp[..., 1:], np.full((B, 32, 1), 128)], -1)
                assert (xh[..., 0][free] < np.minimum(nxt, 128)[free]).all(), what
            live = g3 & (n < K[..., None])
            asc = np.concatenate([np.ones((B, 32, 1), dtype=bool), xh[..., 1:, 0] > xh[..., :-1, 0]], -1)
            assert asc[live].all(), what
            al, rel, emp = allowed_of(xh, setting_kw(name), mask_np, ref)
            assert not emp[g3 & np.ones(15, dtype=bool)].any(), what
            assert np.take_along_axis(al, xh[..., :1], -1)[..., 0][free].all(), what
            print('%s %s lanes=%s durations=%s: %d good top steps, %d ceiling decisions, %d relaxed'
                  % (path, name, c[0], c[1], good.sum(), free.sum(), (rel & free).sum()))
            if name == 'cons':
                assert (rel & free).sum() >= 2, what
            else:
                assert not rel.any(), what
            whole = (mode == 1)[..., None]
            assert np.array_equal(xh[..., 0][fp & whole], xp[fp & whole]) and (fp & whole).sum() > 50
            assert (xh[..., 0][free] != xp[free]).any()
    full, part = refs[True, True]['forced_dur'], refs[True, 'kept']['forced_dur']
    assert full[top].sum() > 1500 and part[top].sum() > 500 and (full & ~part)[top].sum() > 500 and not (part & ~full).any()
    bits = full & ~part
    assert (r['sampled', (True, 'kept')][2][..., 1:][bits] != x[:, :, 1:, 1:][bits]).any()    # durations='kept': the bits below are drawn


def explained_free(po, do, xh, pn, dn, kw, mask_np, ref, what):
    """test_gpu_keep_decode.explained_free with top_ref's allowed rule: every free pitch decision is top_ref.decide_pitch on the emitted
    logits -- over the lane, within the mask unless that leaves nothing, where the word is a ceiling --, every free duration decision
    sample_ref.decide_dur; skipped: decisions sample_ref.skippable, at most SKIP_CAP of the free ones"""
    k, l, q = CD.rule(kw)
    al, rel, emp = allowed_of(xh, kw, mask_np, ref)
    words = words_of(ref)
    want_p = TP.decide_pitch(po, pn, al, words, KD.T_PITCH, k, l, q)
    skip_p = CR.skippable(po, pn, al, KD.T_PITCH, k, l, q)
    want_d = S.decide_dur(do, dn, KD.T_DUR)
    skip_d = S.skippable(do, dn, KD.T_DUR, S.NOISE_TOL)
    free_p, free_d = ~ref['forced_pitch'], ~ref['forced_dur']
    bad_p = (xh[..., 0] != want_p) & ~skip_p & free_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d & free_d
    share_p, share_d = skip_p[free_p].mean(), skip_d[free_d].mean()
    print('%s: free pitch decisions %d of %d (%d under a ceiling, %d relaxed, %d with an empty lane), skipped %d (share %.5f); free '
          'duration decisions %d of %d, skipped %d (share %.5f)'
          % (what, free_p.sum(), free_p.size, (ref['ceil'] > 0).sum(), rel.sum(), emp.sum(), skip_p[free_p].sum(), share_p, free_d.sum(),
             free_d.size, skip_d[free_d].sum(), share_d))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert share_p <= SKIP_CAP and share_d <= SKIP_CAP
    assert np.take_along_axis(al, xh[..., :1], -1)[..., 0][free_p].all()                   # a free decision is a class of the allowed set


@pytest.mark.parametrize('path', list(PATHS))
def test_2_free_decisions_are_the_documented_draw(path):
    _, _, _, _, refs, _ = crafted()
    r = runs(path)
    pn, dn = TT.noise(0, B)
    _, mask_np = mask_pair()
    for c in (CONFIGS[0], CONFIGS[3]):
        for name in ('cons', 'sampled'):
            po, do, xh = r[name, c]
            explained_free(po, do, xh, pn, dn, setting_kw(name), mask_np, refs[c], '%s %s top keep, lanes=%s durations=%s' % ((path, name) + c))


@pytest.mark.parametrize('path', ('default', 'bf16-step-loop'))
def test_3_an_empty_top_keep_is_the_ascending_decode(path):
    """a top keep with no step selected sends the decode as the constrained kind with the ascending flag and gives the grid and the logits of
    the same request with ascending=True and no keep, bit for bit -- under argmax and under plain sampling"""
    attrs, prec = PATHS[path]
    x = crafted()[0]
    m = TT.model()
    m.set_precision(prec)
    zc, zr = halves(TT.latents())
    try:
        with TT.patched(attrs):
            kp = m.keep_top(dev(x), [])
            assert isinstance(kp, FF_.TopKeep) and int((kp.pitch != -1).sum()) == 0 and int((kp.dur != -1).sum()) == 0
            for kw in (dict(), dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW)):
                a = m.inference_decode(zc, zr, ascending=True, **kw)
                la = RD.last_logits(m)
                b = m.inference_decode(zc, zr, keep=kp, **kw)
                lb = RD.last_logits(m)
                assert la[2] == 8 and lb[2] == 8 and m.decoder._last_decode.sampling.ascending
                assert np.array_equal(a, b) and torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1]), (path, kw)
                free = m.inference_decode(zc, zr, **kw)
                assert (free != a).any()                            # (the flag does something: the plain decode differs)
    finally:
        m.set_precision('bf16')


@pytest.mark.parametrize('path', ('default', 'cluster4', 'split', 'bf16-step-loop'))
def test_4_fixed_point(path):
    """the output of a top-keep decode, kept again by keep_top with the same arguments and decoded with the same block and noise.  Room
    ceilings: the same force words, so the same grid and bit-equal logits under all three settings.  Lanes: the ceilings are now the first
    decode's own notes (see the module docstring): the count, the kept notes and the interleaving hold; the differing steps are printed"""
    attrs, prec = PATHS[path]
    x, tsel, wsel, mode, refs, good = crafted()
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            for lanes in (False, True):
                for name in SETTINGS:
                    k1 = keep_of(x, tsel, wsel, lanes)
                    a = KD.kdecode(m, z, blocks()[name], k1)
                    own = m.decoder.last_xhat.clone()
                    k2 = keep_of(own.cpu().numpy(), tsel, wsel, lanes)
                    if not lanes:
                        sel = torch.from_numpy(np.repeat(good.T.reshape(1, -1), 15, 0)).to(DEV)
                        assert torch.equal(k1.pitch[sel], k2.pitch[sel])
                    out[lanes, name] = (a, KD.kdecode(m, z, blocks()[name], k2), own[:, :, :, 0].cpu().numpy())
    finally:
        m.set_precision('bf16')
    ok = good | (mode == 0)                                                                # (row 1, whole, holds unforcible pitches)
    first_bad = np.where((~ok).any(1), (~ok).argmax(1), 32)                                # per row: nothing before its first err step differs
    before = np.arange(32)[None, :] < first_bad[:, None]
    assert before.sum() > 800
    for name in SETTINGS:
        a, b, _ = out[False, name]
        for u, v, what in zip(a, b, ('pitch logits', 'duration logits', 'grid')):
            assert np.array_equal(u[before], v[before]), (path, name, what)
        a, b, own = out[True, name]
        K, h = refs[True, True]['K'], refs[True, True]['h']
        assert np.array_equal(notes_len(b[2])[good], K[good])
        n = np.arange(15)[None, None, :]
        kept = good[..., None] & (n >= (K - h)[..., None]) & (n <= K[..., None])
        assert np.array_equal(b[2][..., 0][kept], a[2][..., 0][kept])
        free = good[..., None] & (n < (K - h)[..., None])
        nxt = np.concatenate([own[:, :, 2:], np.full((B, 32, 1), 128)], -1)
        assert (b[2][..., 0][free] < np.minimum(nxt, 128)[free]).all()
        print('%s %s lanes: %d of %d good top steps differ in the second decode'
              % (path, name, ((a[2][..., 0] != b[2][..., 0]).any(-1) & good).sum(), good.sum()))


def test_5_decode_logprob():
    """the log-probability pass after a constrained sampled top-keep decode of the first 8 rows (the fp64 restatement walks every decision
    in Python): counts, err and the four sums against logprob_ref over the support the device reports with the keep's words
    (ptv_debug_pitch_constrain_words), relaxed or not, at the tolerance of tests/test_gpu_decode_logprob_kernels.py, which
    tests/test_gpu_keep_rhythm_decode.py uses for the same quantity; the ceiling decisions count as free, the kept notes and the <eos> as
    forced; err 0.  With temperature=None and a top keep logq is exactly 0"""
    x, tsel, wsel, mode, refs, good = crafted()
    n = 8
    m = TT.model()
    zc, zr = halves(TT.latents()[:n])
    mask = mask_pair()[0][:n].contiguous()
    kp, kept_n = m.keep_top(dev(x[:n]), dev(tsel[:n]), highest=HIGHEST, whole_steps=dev(wsel[:n]), return_counts=True)
    ref = TP.build(x[:n], mode[:n], None, HIGHEST)
    assert np.array_equal(kept_n.cpu().numpy(), ref['kept_n']) and np.array_equal(kp.pitch.cpu().numpy(), ref['pitch'])
    assert np.array_equal(kp.dur.cpu().numpy(), ref['dur']) and np.array_equal(kp.err.cpu().numpy(), ref['err'])
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
    # the device's support is top_ref's allowed rule where no truncation band decides: every kept class is allowed, relaxed rows included
    al, rel, emp = allowed_of(xg[:, :, 1:], dict(kw, pitch_mask=mask), LK.host(mask), ref)
    live = LR.counted(xg)[0]
    assert not (kept & ~al)[live].any() and (rel & live).sum() >= 1
    r_lp, r_cn, r_er, scale = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, ref['pitch'], ref['dur'])
    f_lp = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, ref['pitch'], ref['dur'], dtype=np.float32)[0]
    got, cn = LK.host(lp.step_logp), LK.host(lp.step_counts)
    assert np.array_equal(cn, r_cn) and np.array_equal(LK.host(lp.err), r_er) and not r_er[np.arange(n) != 1].any()
    for col, fam in enumerate(('logp pitch', 'logp dur', 'logq pitch', 'logq dur')):
        LK.check('top keep %s' % fam, got[..., col], r_lp[..., col], f_lp[..., col], scale[..., col])
    s, c = LR.fold(got, cn, np.float32)
    assert torch.cat([lp.logp, lp.logq], 1).cpu().numpy().tobytes() == s.tobytes() and np.array_equal(LK.host(lp.counts), c)
    # the counts at a good top step: K + 1 pitch decisions (K = 15: 15), of them h kept notes and the <eos> forced, J ceiling decisions free
    g = good[:n]
    K, h = ref['K'], ref['h']
    assert g.sum() > 100
    assert np.array_equal(cn[..., 0][g], np.minimum(K + 1, 15)[g]) and np.array_equal(cn[..., 2][g], (h + (K < 15))[g])
    assert np.array_equal(cn[..., 3][g], ref['forced_dur'].sum((2, 3))[g])
    assert (got[..., 2][g & (K - h > 0)] < 0).any() and not got[..., 2][g & (K - h == 0)].any()
    lp0 = m.decode_logprob(zc, zr, keep=kp)[6]
    assert m.decoder._last_decode.sampling.numel() == 8 and m.decoder._last_decode.sampling.ascending
    assert not LK.host(lp0.logq).any() and not LK.host(lp0.step_logp)[..., 2:].any() and (LK.host(lp0.logp)[:, 0] < 0).all()
    assert not LK.host(lp0.err)[np.arange(n) != 1].any()


def test_6_graph_replay():
    """captured by a WHOLE-step keep under a constrained block; a top keep, another top keep (other steps, room ceilings, durations=False)
    and the whole keep again replay from that capture -- graph_captures does not grow -- each equal to its eager decode"""
    x, tsel, wsel, _, _, _ = crafted()
    m = TT.model()
    zc, zr = halves(TT.latents()[:16])
    xd = dev(x[:16])
    keeps = [m.keep(xd, dev(tsel[:16])), m.keep_top(xd, dev(tsel[:16]), highest=HIGHEST, whole_steps=dev(wsel[:16])),
             m.keep_top(xd, range(8, 32), above=60, durations=False, lanes=False)]
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=9, draw=5, ascending=True)         # (the whole keep asks for the kind itself)
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
        assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[2], **kw), eager[2])
        assert m.decoder.graph_captures == before + 1 and len(m.decoder._graphs) == held
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_decode_best_of():
    """decode_best_of(n = 2) with a top keep of B rows and no constraint of its own (the tiled request keeps the type, so it promotes
    too): the candidates are the rows of a plain decode of the batch tiled twice with the keep built from the tiled grid, bit for bit;
    every candidate has the count and the kept notes; the winner is the first candidate with the largest logp"""
    x, tsel, wsel, mode, refs, good = crafted()
    m = TT.model()
    zc, zr = halves(TT.latents())
    n = 2
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=6, top_k=8)
    xd, td, wd = dev(x), dev(tsel), dev(wsel)
    keep = m.keep_top(xd, td, highest=HIGHEST, whole_steps=wd)
    tiled = m.keep_top(xd.repeat(n, 1, 1, 1), td.repeat(n, 1), highest=HIGHEST, whole_steps=wd.repeat(n, 1))
    plain = m.decode_logprob(zc.repeat(n, 1), zr.repeat(n, 1), keep=tiled, **kw)
    cand = m.decoder.last_xhat[:, :, 1:].cpu().numpy()             # [2 B, 32, 15, 6]: every candidate's decided grid
    out = m.decode_best_of(zc, zr, n, keep=keep, **kw)
    torch.cuda.synchronize()
    assert m.decoder._last_decode.sampling.numel() == 8 and m.decoder._last_decode.sampling.ascending
    g = np.tile(good, (n, 1))
    ref = refs[True, True]
    K, h = np.tile(ref['K'], (n, 1)), np.tile(ref['h'], (n, 1))
    assert np.array_equal(notes_len(cand)[g], K[g])
    nn = np.arange(15)[None, None, :]
    kept = g[..., None] & (nn >= (K - h)[..., None]) & (nn < K[..., None])
    assert np.array_equal(cand[..., 0][kept], np.tile(x[:, :, 1:, 0], (n, 1, 1))[kept])
    assert (cand[:B] != cand[B:]).any()
    lp = plain[6]
    score = lp.logp.sum(1).cpu().numpy()
    want, _ = LR.best_of(score.reshape(n, B))
    best = out[6].cpu().numpy()
    assert np.array_equal(best, want) and len(set(best.tolist())) > 1
    rows = torch.from_numpy(want.astype(np.int64) * B + np.arange(B)).to(DEV)
    assert torch.equal(out[1], plain[1][rows]) and torch.equal(out[0], plain[0][rows])
    assert torch.equal(out[7], torch.cat([lp.logp, lp.logq], 1)[rows])


def test_8_causality():
    """the time steps before the first top step are those of the decode without the keep under ascending=True, grid and logits, bit for bit;
    and changing row 5's keep changes no other row"""
    x, tsel, wsel, _, _, _ = crafted()
    m = TT.model()
    z = TT.latents()
    late = tsel.copy()
    late[:, :9] = 0
    a = KD.kdecode(m, z, RD.cons_block(), keep_of(x, late))
    free = KD.kdecode(m, z, RD.cons_block())
    first = np.where(late.any(1), late.argmax(1), 32)
    before = np.arange(32)[None, :] < first[:, None]
    assert before.sum() >= 9 * B and (a[2] != free[2]).any()
    for u, v in zip(a, free):
        assert np.array_equal(u[before], v[before])
    x2, t2 = x.copy(), tsel.copy()
    x2[5] = synth_batch(B, 9)[0][5]
    t2[5] = 1 - tsel[5]
    a = KD.kdecode(m, z, RD.cons_block(), keep_of(x, tsel, wsel))
    b = KD.kdecode(m, z, RD.cons_block(), keep_of(x2, t2, wsel))
    others = np.arange(B) != 5
    assert (a[2][5] != b[2][5]).any()
    for u, v in zip(a, b):
        assert np.array_equal(u[others], v[others])


def test_9_surface():
    x, tsel, wsel, mode, refs, good = crafted()
    m = TT.model()
    Bs = 4
    zc, zr = halves(TT.latents()[:Bs])
    xd = dev(x[:Bs])
    td, wd = dev(tsel[:Bs]), dev(wsel[:Bs])
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    # ---- DisentangleVAE.keep_top / split_top: every bad argument is a ValueError before any launch
    for fn in (m.keep_top, m.split_top):
        for bad_x in (xd.cpu(), xd.int(), xd[:, :, :15], xd[0]):
            with pytest.raises(ValueError):
                fn(bad_x, range(4))
        for bad in (dict(top_steps=td.cpu()), dict(top_steps=td.int()), dict(top_steps=dev(tsel[:3])), dict(top_steps=td[:, :31]),
                    dict(top_steps=td[0]), dict(top_steps=[32]), dict(top_steps=[-1]), dict(top_steps=[0.5]), dict(top_steps=7),
                    dict(top_steps=None), dict(whole_steps=wd[0]), dict(whole_steps=wd.cpu()), dict(whole_steps=[40]), dict(above=129),
                    dict(above=-1), dict(above=60.0), dict(highest=16), dict(highest=True), dict(above=i32([[60] * 32]).cpu()),
                    dict(above=i32([[60] * 32]).long()), dict(highest=i32([[1] * 32] * 3)), dict(highest=i32([1] * 32))):
            with pytest.raises(ValueError):
                fn(xd, **dict(dict(top_steps=td), **bad))
    for bad in (dict(durations=1), dict(durations=None), dict(durations='all'), dict(lanes=0), dict(lanes=None)):
        with pytest.raises(ValueError):
            m.keep_top(xd, td, **bad)
    # ---- what comes back: a TopKeep that passes for a Keep; host and device selections and limits; durations=False frees the top steps
    kp, kept_n = m.keep_top(xd, td, highest=HIGHEST, whole_steps=wd, return_counts=True)
    torch.cuda.synchronize()
    assert isinstance(kp, FF_.TopKeep) and isinstance(kp, FF_.Keep) and kp.batch == Bs and kp._fields == FF_.Keep._fields
    FF_.check_keep(kp, Bs)
    want = TP.build(x[:Bs], mode[:Bs], None, HIGHEST)
    for got, k in ((kp.pitch, 'pitch'), (kp.dur, 'dur'), (kp.err, 'err'), (kept_n, 'kept_n')):
        assert np.array_equal(got.cpu().numpy(), want[k]), k
    hi = np.tile(np.arange(32, dtype=np.int32) % 4, (Bs, 1))
    for d in (True, 'kept', False):
        for lanes in (True, False):
            host = m.keep_top(xd, range(32), above=55, highest=i32(hi), whole_steps=slice(0, 4), durations=d, lanes=lanes)
            want = TP.build(x[:Bs], np.array([[1] * 4 + [4] * 28], dtype=np.uint8), 55, hi, durations=d, lanes=lanes)
            assert np.array_equal(host.pitch.cpu().numpy(), want['pitch']) and np.array_equal(host.dur.cpu().numpy(), want['dur']), (d, lanes)
            FF_.check_keep(host, Bs)
    assert type(m.keep_top(xd, td.bool())) is FF_.TopKeep
    top_only = TP.build(x[:Bs], np.full((1, 32), 4, dtype=np.uint8))
    assert np.array_equal(m.keep_top(xd, slice(None)).pitch.cpu().numpy(), top_only['pitch']) and (top_only['h'] <= 1).all()
    # ---- split_top: the same selection as two grids
    xt, xr, kn, er = m.split_top(xd, td, highest=HIGHEST, whole_steps=wd)
    wv, wr, wk = TP.split(x[:Bs], mode[:Bs], None, HIGHEST)
    assert np.array_equal(xt.cpu().numpy(), wv) and np.array_equal(xr.cpu().numpy(), wr) and np.array_equal(kn.cpu().numpy(), wk)
    assert np.array_equal(er.cpu().numpy(), kp.err.cpu().numpy())
    # ---- the request: ascending=False beside a TopKeep is refused before anything is launched or the draw counter moves
    draws = m._sample_draws
    m.decoder._last_decode = None
    for fn in (lambda: m.inference_decode(zc, zr, temperature=1.0, keep=kp, ascending=False),
               lambda: m.decode_to_inputs(zc, zr, keep=kp, ascending=False),
               lambda: m.decode_logprob(zc, zr, temperature=1.0, keep=kp, ascending=False),
               lambda: m.decode_best_of(zc, zr, 2, temperature=1.0, keep=kp, ascending=False)):
        with pytest.raises(ValueError, match='ascending'):
            fn()
    # ---- one level down: a TopKeep beside anything but a constrained block with the ascending flag is refused before any launch
    dec_z = torch.cat([zc, zr], -1)
    for blk in (None, TT.block(0), TT.block(0, top_k=8), TT.block(0, ascending=False),
                TT.block(0, pitch_mask=mask_pair()[0][:Bs].contiguous())):
        with pytest.raises(ValueError):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=blk, keep=kp)
    assert m.decoder._last_decode is None and m._sample_draws == draws
    with torch.no_grad():
        m.decoder(dec_z, True, None, None, 0., 0., sampling=TT.block(0, ascending=True), keep=kp)
    # ---- like any keep: a wrong batch, together with force_trace -- before anything is encoded or launched
    other = m.keep_top(dev(x[:8]), range(4))
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
    # ---- every entry point takes it: the count of the top steps comes out of decode_to_inputs, swap and reencode's decode, and with the
    # documented usage line (a chord mask of another chord)
    g = good[:Bs]
    want_k = TP.build(x[:Bs], mode[:Bs], None, HIGHEST)['K']
    m.decode_to_inputs(zc, zr, temperature=1.0, keep=kp)
    assert np.array_equal(notes_len(m.decoder.last_xhat[:, :, 1:].cpu().numpy())[g], want_k[g])
    est = m.swap(pr, pr, c, c, True, True, keep=kp)
    assert np.array_equal(notes_len(est)[g], want_k[g]) and m._sample_draws == draws + 1
    m.reencode(zc, zr, temperature=0.8, keep=kp)
    assert np.array_equal(notes_len(m.decoder.last_xhat[:, :, 1:].cpu().numpy())[g], want_k[g])
    c_new = dev(synth_batch(Bs, 11)[1])
    m.decode_to_inputs(zc, zr, keep=kp, temperature=1.0, pitch_mask=m.pitch_mask(c=c_new))
    xh = m.decoder.last_xhat[:, :, 1:].cpu().numpy()
    assert np.array_equal(notes_len(xh)[g], want_k[g])
