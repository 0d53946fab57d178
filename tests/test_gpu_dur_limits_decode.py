"""GPU: duration limits in the free-running decode (DisentangleVAE.dur_limits, keep=; INTEGRATION.md "Duration limits") against
tests/dur_limits_ref.py on every selectable note-loop path: every note of a limited step has its duration in range, each duration bit
is the documented decision on the emitted logits, promotion alone changes nothing, lo == hi is a forced keep, the fixed point, the
log-probability pass, graph replay, best-of-n, causality, the unclipped piano-roll and the surface.  B = 32; the model, latents, paths and
noise are those of tests/test_gpu_truncated_sampling.py, the three settings (constrained argmax, plain sampling sent as the constrained
kind, chord mask + ascending + top_k + top_p) those of tests/test_gpu_keep_rhythm_decode.py.  The limits: fit='bar' with min_dur=2 at the
steps (t + b) % 4 < 3; row ONE has max_dur=1 (its floor yields: every bit is determined), row FREE has no step selected."""
import functools

import numpy as np
import pytest
import torch

import dur_limits_ref as DR
import logprob_ref as LR
import sample_ref as S
import test_gpu_decode_logprob_kernels as LK
import test_gpu_keep_decode as KD
import test_gpu_keep_rhythm_decode as RD
import test_gpu_keep_rhythm_kernels as RK
import test_gpu_truncated_sampling as TT
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
B = 32
SKIP_CAP = 0.005
SETTINGS = ('argmax', 'sampled', 'cons')
ONE, FREE = 2, 3
EOS = 129
dev = KD.dev


@functools.lru_cache(maxsize=None)
def limits():
    """(min_dur, max_dur uint8 [32, 32], steps uint8 [32, 32], dur_limits_ref.build of them under fit='bar')"""
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    steps = ((t_ + b_) % 4 < 3).astype(np.uint8)
    steps[FREE] = 0
    lo = np.full((B, 32), 2, dtype=np.uint8)
    hi = np.full((B, 32), 32, dtype=np.uint8)
    hi[ONE] = 1
    ref = DR.build(lo, np.minimum(hi, np.array([DR.fit_row('bar')], dtype=np.uint8)), steps, B)
    for a in (lo, hi, steps) + tuple(ref.values()):
        a.setflags(write=False)
    return lo, hi, steps, ref


def limits_keep(rows=slice(None), **kw):
    lo, hi, steps, _ = limits()
    out = TT.model().dur_limits(min_dur=dev(lo[rows]), max_dur=dev(hi[rows]), fit='bar', steps=dev(steps[rows]), **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: under the three settings with the limits and, same block, without a keep"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            kp = limits_keep()
            for name, blk in RD.blocks().items():
                out[name] = KD.kdecode(m, z, blk, kp)
                out[name, 'plain'] = KD.kdecode(m, z, blk, None)
    finally:
        m.set_precision('bf16')
    return out


def values(xh):
    """int [B, 32, 15]: the 5-bit value of every decision's duration bits (D - 1)"""
    bits = xh[..., 1:]
    return ((bits[..., 0] * 2 + bits[..., 1]) * 2 + bits[..., 2]) * 4 + bits[..., 3] * 2 + bits[..., 4]


def notes_of(xh):
    """bool [B, 32, 15]: the decisions that are notes of the decoded step (before its first <eos>, a pitch < 128)"""
    return (np.arange(15)[None, None, :] < RD.notes_len(xh)[..., None]) & (xh[..., 0] < 128)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', list(PATHS))
def test_1_every_duration_is_in_range(path):
    """at a limited step EVERY decision's five bits -- the notes among them -- have a value in [lo, hi]; row ONE holds only D = 1; the
    row without a selected step equals the decode without a keep, logits and grid, bit for bit"""
    _, _, steps, ref = limits()
    r = runs(path)
    sel = steps != 0
    lo, hi = ref['lo'][..., None], ref['hi'][..., None]
    for name in SETTINGS:
        po, do, xh = r[name]
        v = values(xh)
        assert set(np.unique(xh[..., 1:]).tolist()) <= {0, 1}
        inside = (v >= lo) & (v <= hi)
        assert inside[sel].all(), (path, name, np.argwhere(~inside & sel[..., None])[:4])
        nt = notes_of(xh)
        assert nt[sel].sum() > 200 and (v[ONE][sel[ONE]] == 0).all()
        assert (v + 1 <= 16 - np.arange(32)[None, :, None] % 16)[sel].all()                  # nothing over the bar line
        for u, w, what in zip(r[name], r[name, 'plain'], ('pitch logits', 'duration logits', 'grid')):
            assert np.array_equal(u[FREE], w[FREE]), (path, name, what)
        assert (xh != r[name, 'plain'][2]).any()


@functools.lru_cache(maxsize=None)
def rule_tables():
    """dur_limits_ref.allowed of every (lo, hi, d, p) as two bool arrays [32, 32, 5, 16] (lo > hi: both allowed, the plain free word)"""
    a0 = np.ones((32, 32, 5, 16), dtype=bool)
    a1 = np.ones((32, 32, 5, 16), dtype=bool)
    for w, d, p in DR.table():
        lo, hi = DR.unword(w)
        a0[lo, hi, d, p], a1[lo, hi, d, p] = DR.allowed(w, d, p)
    return a0, a1


def explained(do, xh, dn, T, ref, what):
    """every duration bit is the documented decision: with the prefix the decode itself took, a bit the range determines is the allowed
    value (never left out); any other bit is sample_ref.decide_dur on the emitted logits and the restated noise, but for near-ties
    (sample_ref.skippable), whose share is asserted -> (determined bits, bits with both values allowed)"""
    a0, a1 = rule_tables()
    bits = xh[..., 1:]
    pre = np.zeros(bits.shape, dtype=np.int64)
    for d in range(1, 5):
        pre[..., d] = 2 * pre[..., d - 1] + bits[..., d - 1]
    lim = ref['limited']
    lo = np.where(lim, ref['lo'][..., None], 1)[..., None]              # (lo > hi: the tables' free entry)
    hi = np.where(lim, ref['hi'][..., None], 0)[..., None]
    d_ix = np.arange(5)[None, None, None, :]
    al0, al1 = a0[lo, hi, d_ix, pre], a1[lo, hi, d_ix, pre]
    det = al0 != al1
    both = al0 & al1 & lim[..., None]
    assert (al0 | al1).all()                                             # the decode never left its range
    want = np.where(det, al1.astype(np.int64), S.decide_dur(do, dn, T))
    skip = S.skippable(do, dn, T, S.NOISE_TOL) & ~det
    bad = (bits != want) & ~skip
    print('%s: %d determined bits, %d limited bits with both values allowed, %d free; left out as near-ties %d of %d (share %.5f)'
          % (what, det.sum(), both.sum(), (~lim[..., None] & ~det).sum(), skip.sum(), (~det).sum(), skip.sum() / max((~det).sum(), 1)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4])
    assert skip.sum() <= SKIP_CAP * (~det).sum()
    return int(det.sum()), int(both.sum())


@pytest.mark.parametrize('path', list(PATHS))
def test_2_every_bit_is_the_documented_decision(path):
    _, _, steps, ref = limits()
    r = runs(path)
    _, dn = TT.noise(0, B)
    sel = steps != 0
    for name in SETTINGS:
        _, do, xh = r[name]
        det, both = explained(do, xh, dn, 0.0 if name == 'argmax' else KD.T_DUR, ref, '%s %s' % (path, name))
        assert det >= 1 and both >= 1, (path, name, det, both)
        plain = r[name, 'plain'][2]
        over = notes_of(plain) & (values(plain) + 1 > 16 - np.arange(32)[None, :, None] % 16) & sel[..., None]
        print('%s %s: %d notes of the same decode without limits hang over the bar line at a limited step' % (path, name, over.sum()))
        assert over.sum() >= 1, (path, name)


@pytest.mark.parametrize('path', ('default', 'bf16-step-loop'))
def test_3_promotion_alone_changes_nothing(path):
    """limits with no step selected, or with the whole range 1..32 at every step, send the decode as the constrained kind and give the grid
    and the logits of the same decode without a keep, bit for bit -- under argmax and under plain sampling"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    zc, zr = RD.halves(TT.latents())
    try:
        with TT.patched(attrs):
            none = m.dur_limits(min_dur=4, max_dur=6, steps=[], batch=B)
            whole = m.dur_limits(min_dur=1, max_dur=32, batch=B)
            assert type(none) is FF_.DurKeep and int((none.dur != -1).sum()) == 0
            assert int((whole.dur != DR.word(0, 31)).sum()) == 0 and int((whole.pitch != -1).sum()) == 0
            for kw, words in ((dict(), None), (dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW), 4)):
                a = m.inference_decode(zc, zr, **kw)
                la = RD.last_logits(m)
                assert la[2] == words
                for kp in (none, whole):
                    b = m.inference_decode(zc, zr, keep=kp, **kw)
                    lb = RD.last_logits(m)
                    assert lb[2] == 8
                    assert np.array_equal(a, b) and torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1]), (path, kw)
    finally:
        m.set_precision('bf16')


@pytest.mark.parametrize('path', ('default', 'cluster4', 'split', 'bf16-step-loop'))
def test_4_identities(path):
    """lo == hi is a keep that forces those five bits: the same grid, bit-equal logits.  The output of a limited decode, kept WHOLE
    (DisentangleVAE.keep) and decoded with the same block, comes back: the same grid and bit-equal logits at every decision up to each
    step's <eos> (the whole keep forces nothing behind it, where the limits still acted; no later time step reads those slots)"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    rng = np.random.default_rng(17)
    D = rng.integers(1, 33, (B, 32)).astype(np.uint8)
    forced = np.zeros((5, 15, 32, B), dtype=np.int32)
    for d in range(5):
        forced[d] = ((D.T.astype(np.int32) - 1) >> (4 - d) & 1)[None]
    out = {}
    try:
        with TT.patched(attrs):
            blocks = RD.blocks()
            same = m.dur_limits(min_dur=dev(D), max_dur=dev(D))
            bits = FF_.Keep(torch.full((15, 32 * B), -1, dtype=torch.int32, device=DEV), dev(forced.reshape(5, 480 * B)),
                            torch.zeros(B, dtype=torch.int32, device=DEV), B)
            for name in ('sampled', 'cons'):
                out['eq', name] = (KD.kdecode(m, z, blocks[name], same), KD.kdecode(m, z, blocks[name], bits))
                a = KD.kdecode(m, z, blocks[name], limits_keep())
                kp = m.keep(m.decoder.last_xhat.clone(), range(32))
                assert type(kp) is FF_.Keep and int(kp.err.sum()) == 0
                out['fix', name] = (a, KD.kdecode(m, z, blocks[name], kp))
    finally:
        m.set_precision('bf16')
    for name in ('sampled', 'cons'):
        a, b = out['eq', name]
        assert np.array_equal(values(a[2]), np.broadcast_to((D.astype(np.int64) - 1)[..., None], (B, 32, 15)))
        for u, v, what in zip(a, b, ('pitch logits', 'duration logits', 'grid')):
            assert np.array_equal(u, v), (path, name, 'lo == hi', what)
        a, b = out['fix', name]
        upto = np.arange(15)[None, None, :] <= RD.notes_len(a[2])[..., None]
        assert not upto.all()
        for u, v, what in zip(a, b, ('pitch logits', 'duration logits', 'grid')):
            assert np.array_equal(u[upto], v[upto]), (path, name, 'fixed point', what)


def test_5_decode_logprob():
    """the log-probability pass after a constrained sampled decode of the first 8 rows under the limits against the fp64 walk of
    logprob_ref over the same support: a bit the range determines counts with the forced decisions (log p as ever, log q 0), a bit with
    both values allowed is free; counts exact, sums at the tolerance of tests/test_gpu_decode_logprob_kernels.py; err 0"""
    n = 8
    _, _, steps, ref = limits()
    m = TT.model()
    zc, zr = RD.halves(TT.latents()[:n])
    mask = RD.mask_pair()[0][:n].contiguous()
    kp = limits_keep(slice(0, n))
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW, **KD.CONS)
    lp = m.decode_logprob(zc, zr, keep=kp, pitch_mask=mask, **kw)[6]
    torch.cuda.synchronize()
    last = m.decoder._last_decode
    assert last.sampling.numel() == 8
    pitch = LK.host(last.pitch.permute(2, 1, 0, 3))
    dur = LK.host(last.dur.view(15, 32, n, 5, 2).permute(2, 1, 0, 3, 4))
    xg = LK.host(last.xhat)
    finite = np.where(LR.counted(xg)[0][..., None], pitch, np.float32(0))
    free_p = np.full((15, 32 * n), -1, dtype=np.int32)
    kept = RK.kept_with_words(kw, xg, finite, LK.host(mask), free_p)
    # the force words the walk sees: a determined bit is its value, every other bit free
    words = LK.host(kp.dur)
    eff = np.full((5, 480 * n), -1, dtype=np.int32)
    n_det = 0
    for b in range(n):
        for t in range(32):
            for s in range(15):
                i = s * 32 * n + t * n + b
                p = 0
                for d in range(5):
                    bit = int(xg[b, t, s + 1, 1 + d])
                    if bit not in (0, 1):
                        break
                    if DR.determined(int(words[d, i]), d, p):
                        assert DR.decide(int(words[d, i]), d, p, bit) == bit
                        eff[d, i] = bit
                        n_det += 1
                    p = 2 * p + bit
    r_lp, r_cn, r_er, scale = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, free_p, eff)
    f_lp = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, free_p, eff, dtype=np.float32)[0]
    got, cn = LK.host(lp.step_logp), LK.host(lp.step_counts)
    assert np.array_equal(cn, r_cn) and np.array_equal(LK.host(lp.err), r_er) and not r_er.any()
    assert n_det > 500 and 0 < cn[..., 3].sum() < cn[..., 1].sum() and cn[..., 2].sum() == 0
    s1 = steps[ONE] != 0                                                 # row ONE: every bit of a limited step is determined
    assert cn[FREE, :, 3].sum() == 0 and np.array_equal(cn[ONE, s1, 3], cn[ONE, s1, 1]) and not got[ONE, s1, 3].any()
    assert cn[ONE, s1, 1].sum() > 0 and cn[ONE, ~s1, 3].sum() == 0
    for col, fam in enumerate(('logp pitch', 'logp dur', 'logq pitch', 'logq dur')):
        LK.check('duration limits %s' % fam, got[..., col], r_lp[..., col], f_lp[..., col], scale[..., col])
    s, c = LR.fold(got, cn, np.float32)
    assert torch.cat([lp.logp, lp.logq], 1).cpu().numpy().tobytes() == s.tobytes() and np.array_equal(LK.host(lp.counts), c)


def test_6_graph_replay():
    """captured with the limits, replayed with a rhythm keep and a whole keep: ONE capture of the (constrained kind, a keep) graph serves
    them all, each replay equal to its eager decode"""
    x, rsel, wsel, _, _ = RD.crafted()
    m = TT.model()
    zc, zr = RD.halves(TT.latents()[:16])
    xd = dev(x[:16])
    keeps = [limits_keep(slice(0, 16)), m.keep_rhythm(xd, dev(rsel[:16]), whole_steps=dev(wsel[:16])), m.keep(xd, dev(rsel[:16])),
             m.dur_limits(max_dur=4, fit='beat', keep=m.keep_rhythm(xd, range(8, 32), durations=False))]
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=9, draw=5, ascending=False)
    eager = [m.inference_decode(zc, zr, keep=k, **kw) for k in keeps]
    assert all((eager[i] != eager[j]).any() for i in range(4) for j in range(i))
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[0], **kw), eager[0])
        held = len(m.decoder._graphs)
        assert m.decoder.graph_captures == before + 1
        for i in (1, 2, 3, 0):
            assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[i], **kw), eager[i]), i
        assert m.decoder.graph_captures == before + 1 and len(m.decoder._graphs) == held
        kw.pop('ascending')                                                                    # the promotion picks the same graph
        assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[0], **kw), eager[0])
        assert m.decoder.graph_captures == before + 1 and len(m.decoder._graphs) == held
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_decode_best_of():
    """decode_best_of(n = 2) with the limits of B rows: the candidates are the rows of a plain decode of the batch tiled twice with the
    tiled keep, EVERY candidate is in range, and the winner is the first candidate with the largest logp"""
    lo, hi, steps, ref = limits()
    m = TT.model()
    zc, zr = RD.halves(TT.latents())
    n = 2
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=6, top_k=8)
    keep = limits_keep()
    tiled = m.dur_limits(min_dur=dev(np.tile(lo, (n, 1))), max_dur=dev(np.tile(hi, (n, 1))), fit='bar', steps=dev(np.tile(steps, (n, 1))))
    plain = m.decode_logprob(zc.repeat(n, 1), zr.repeat(n, 1), keep=tiled, **kw)
    cand = m.decoder.last_xhat[:, :, 1:].cpu().numpy()
    out = m.decode_best_of(zc, zr, n, keep=keep, **kw)
    torch.cuda.synchronize()
    assert m.decoder._last_decode.sampling.numel() == 8
    sel = np.tile(steps != 0, (n, 1))
    v = values(cand)
    assert ((v >= np.tile(ref['lo'], (n, 1))[..., None]) & (v <= np.tile(ref['hi'], (n, 1))[..., None]))[sel].all()
    assert (cand[:B] != cand[B:]).any()
    lp = plain[6]
    want, _ = LR.best_of(lp.logp.sum(1).cpu().numpy().reshape(n, B))
    best = out[6].cpu().numpy()
    assert np.array_equal(best, want) and len(set(best.tolist())) > 1
    rows = torch.from_numpy(want.astype(np.int64) * B + np.arange(B)).to(DEV)
    assert torch.equal(out[1], plain[1][rows]) and torch.equal(out[0], plain[0][rows])
    assert torch.equal(out[7], torch.cat([lp.logp, lp.logq], 1)[rows])


def test_8_causality_and_the_unclipped_piano_roll():
    """limits at the steps >= 16 leave the steps < 16 as they are without a keep, logits and grid bit for bit.  Under fit='segment' the
    piano-roll of decode_to_inputs holds every note's full duration D: nothing was clipped at the end of the segment"""
    m = TT.model()
    z = TT.latents()
    blk = RD.blocks()['cons']
    a = KD.kdecode(m, z, blk, m.dur_limits(min_dur=3, fit='bar', steps=range(16, 32), batch=B))
    b = KD.kdecode(m, z, blk, None)
    assert (a[2][:, 16:] != b[2][:, 16:]).any()
    for u, v in zip(a, b):
        assert np.array_equal(u[:, :16], v[:, :16])
    zc, zr = RD.halves(z)
    kw = dict(temperature=1.0, dur_temperature=1.0, seed=TT.SEED, draw=TT.DRAW, ascending=True)
    clipped = 0
    for keep in (None, m.dur_limits(fit='segment', batch=B)):
        pr = m.decode_to_inputs(zc, zr, keep=keep, **kw)[0].cpu().numpy()
        xh = m.decoder.last_xhat[:, :, 1:].cpu().numpy()
        nt, D = notes_of(xh) & (np.arange(15) < 10), values(xh) + 1      # (the output path reads max_notes = 10 notes of a step)
        room = 32 - np.arange(32)[None, :, None]
        bi, ti, ni = np.nonzero(nt)
        held = pr[bi, ti, xh[bi, ti, ni, 0]]
        assert nt.sum() > 1000 and np.array_equal(held, np.minimum(D, room)[nt])
        if keep is None:
            clipped = int((D > room)[nt].sum())
            assert clipped >= 1                                          # without the limits the output path cuts notes silently
        else:
            assert (D <= room)[nt].all() and np.array_equal(held, D[nt])


def test_9_surface():
    lo, hi, steps, ref = limits()
    m = TT.model()
    Bs = 4
    zc, zr = RD.halves(TT.latents()[:Bs])
    t32 = torch.full((Bs, 32), 3, dtype=torch.int32, device=DEV)
    sel = dev(steps[:Bs])
    # ---- every bad argument is a ValueError before any launch
    for bad in (dict(min_dur=0), dict(min_dur=33), dict(max_dur=0), dict(max_dur=33), dict(min_dur=True), dict(max_dur=False),
                dict(min_dur=2.0), dict(max_dur='4'), dict(min_dur=t32.cpu()), dict(max_dur=t32.cpu()), dict(min_dur=t32.float()),
                dict(max_dur=t32.bool()), dict(min_dur=t32[:, :31]), dict(max_dur=t32[0, :16]), dict(min_dur=t32[:3].contiguous(), max_dur=t32),
                dict(max_dur=t32.view(Bs, 32, 1)), dict(fit='phrase'), dict(fit=16), dict(fit=True), dict(steps=sel.cpu()),
                dict(steps=sel.int()), dict(steps=sel[:, :31]), dict(steps=sel[0]), dict(steps=[32]), dict(steps=[-1]), dict(steps=7),
                dict(batch=0), dict(batch=True), dict(batch=2.0), dict(batch=Bs + 1, min_dur=t32), dict(keep=(1, 2, 3, 4)),
                dict(keep=m.dur_limits(batch=Bs + 1), min_dur=t32)):
        with pytest.raises(ValueError):
            m.dur_limits(**dict(dict(batch=Bs) if 'batch' not in bad else {}, **bad))
    with pytest.raises(ValueError):
        m.dur_limits(min_dur=2)                                          # nothing tells the batch
    # ---- what comes back: a DurKeep that passes for a Keep
    kp, y = m.dur_limits(min_dur=dev(lo[:Bs]), max_dur=dev(hi[:Bs]), fit='bar', steps=sel, return_counts=True)
    torch.cuda.synchronize()
    assert type(kp) is FF_.DurKeep and isinstance(kp, FF_.Keep) and kp.batch == Bs and kp._fields == FF_.Keep._fields
    FF_.check_keep(kp, Bs)
    want = DR.build(lo[:Bs], np.minimum(hi[:Bs], np.array([DR.fit_row('bar')], np.uint8)), steps[:Bs], Bs)
    assert np.array_equal(kp.dur.cpu().numpy(), want['dur']) and np.array_equal(y.cpu().numpy(), want['yielded'])
    assert want['yielded'][ONE].sum() == (steps[ONE] != 0).sum() and want['yielded'].sum() > want['yielded'][ONE].sum()
    assert type(m.dur_limits(steps=sel.bool(), max_dur=torch.full((32,), 4, dtype=torch.int64, device=DEV))) is FF_.DurKeep
    # ---- one level down: a DurKeep beside anything but a constrained block is refused before any launch
    dec_z = torch.cat([zc, zr], -1)
    m.decoder._last_decode = None
    for blk in (None, TT.block(0), TT.block(0, top_k=8)):
        with pytest.raises(ValueError):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=blk, keep=kp)
    assert m.decoder._last_decode is None
    with torch.no_grad():
        m.decoder(dec_z, True, None, None, 0., 0., sampling=TT.block(0, ascending=False), keep=kp)
    # ---- built into a top keep it stays one: ascending=False is still refused, a wrong batch too, before the draw counter moves
    x = RD.crafted()[0]
    top = m.dur_limits(max_dur=4, keep=m.keep_top(dev(x[:Bs]), range(8)))
    assert isinstance(top, FF_.TopKeep) and isinstance(top, FF_.DurKeep)
    draws = m._sample_draws
    with pytest.raises(ValueError):
        m.inference_decode(zc, zr, temperature=1.0, ascending=False, keep=top)
    with pytest.raises(ValueError):
        m.inference_decode(zc, zr, temperature=1.0, keep=m.dur_limits(max_dur=4, batch=8))
    assert m._sample_draws == draws
    # ---- every entry point takes it
    in_range = lambda g: bool(((values(g) >= want['lo'][..., None]) & (values(g) <= want['hi'][..., None]))[steps[:Bs] != 0].all())
    m.decode_to_inputs(zc, zr, temperature=1.0, keep=kp)
    assert in_range(m.decoder.last_xhat[:, :, 1:].cpu().numpy())
    assert in_range(m.inference_decode(zc, zr, keep=kp))
    m.reencode(zc, zr, temperature=0.8, keep=kp)
    assert in_range(m.decoder.last_xhat[:, :, 1:].cpu().numpy())
    m.inference_decode(zc, zr, temperature=1.0, keep=top)
    assert m.decoder._last_decode.sampling.ascending
