"""GPU: note-count limits in the free-running decode (DisentangleVAE.count_limits, keep=; INTEGRATION.md "Note-count limits") against
tests/count_limits_ref.py on every selectable note-loop path: the count of every selected step is at most H always, at least L always
under room=True and, without it, everywhere but where the replayed allowed set held only <eos>; rests and onset patterns; a row without
a selected step is the decode without a keep bit for bit; a ceiling-only keep runs as the plain argmax / sampled kind and equals the
unlimited decode up to the first step it cuts; every decision is the documented one by replay on the emitted logits; the
log-probability pass, best-of-n, graph replay, rows=, the yield bits and the surface.  B = 32; the model, latents, paths and noise are
those of tests/test_gpu_truncated_sampling.py, the settings those of tests/test_gpu_keep_rhythm_decode.py (room=False) and
tests/test_gpu_keep_top_decode.py (room=True: the same blocks with the ascending flag).
The limits: steps (t + b) % 4 < 3; floor 2 + t % 2, ceiling 4; row OVER has floor 6 over ceiling 3, row OPEN no ceiling (15) and
floor 3, the rows >= 16 rest at t % 8 == 7; row FREE has no step selected."""
import functools

import numpy as np
import pytest
import torch

import constrain_ref as CR
import count_limits_ref as CL
import logprob_ref as LR
import rhythm_ref as RR
import sample_ref as S
import test_gpu_constrained_decode as CD
import test_gpu_decode_logprob_kernels as LK
import test_gpu_keep_decode as KD
import test_gpu_keep_rhythm_decode as RD
import test_gpu_keep_rhythm_kernels as RK
import test_gpu_keep_top_decode as TD
import test_gpu_truncated_sampling as TT
import top_ref as TP
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
B = 32
SKIP_CAP = 0.005
SETTINGS = ('argmax', 'sampled', 'cons')
FREE, OVER, OPEN = 3, 5, 6
EOS = 129
dev = KD.dev
notes_len = RD.notes_len


@functools.lru_cache(maxsize=None)
def limits():
    """(lo, hi, steps uint8 [32, 32], {room: count_limits_ref.build})"""
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    steps = ((t_ + b_) % 4 < 3).astype(np.uint8)
    steps[FREE] = 0
    lo = (2 + t_ % 2).astype(np.uint8)
    hi = np.full((B, 32), 4, dtype=np.uint8)
    lo[OVER], hi[OVER] = 6, 3
    lo[OPEN], hi[OPEN] = 3, 15
    hi[16:, 7::8] = 0
    refs = {room: CL.build(lo, hi, steps, B, room=room) for room in (False, True)}
    for a in (lo, hi, steps) + tuple(refs[False].values()) + tuple(refs[True].values()):
        a.setflags(write=False)
    return lo, hi, steps, refs


def limits_keep(room, rows=slice(None), **kw):
    lo, hi, steps, _ = limits()
    out = TT.model().count_limits(min_count=dev(lo[rows]), max_count=dev(hi[rows]), steps=dev(steps[rows]), room=room, **kw)
    torch.cuda.synchronize()
    return out


def cap_keep(rows=slice(None)):
    _, hi, steps, _ = limits()
    out = TT.model().count_limits(max_count=dev(hi[rows]), steps=dev(steps[rows]))
    torch.cuda.synchronize()
    return out


def blocks(room):
    return TD.blocks() if room else RD.blocks()


def setting_kw(name, room):
    return TD.setting_kw(name) if room else RD.setting_kw(name)


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: with the limits and, same block, without a keep under the three settings, room off and on;
    the ceiling-only keep and no keep as the plain argmax kind (no block) and the plain sampled kind (a four-word block)"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            for room in (False, True):
                kp = limits_keep(room)
                for name, blk in blocks(room).items():
                    out[name, room] = KD.kdecode(m, z, blk, kp)
                    out[name, room, 'plain'] = KD.kdecode(m, z, blk, None)
            cap = cap_keep()
            assert type(cap) is FF_.Keep
            for name, blk in (('argmax', None), ('sampled', TT.block(0))):
                out['cap', name] = KD.kdecode(m, z, blk, cap)
                out['cap', name, 'plain'] = KD.kdecode(m, z, blk, None)
    finally:
        m.set_precision('bf16')
    return out


def words_of(ref):
    return CL.words_of(ref['pitch'])


def allowed_of(xh, kw, mask_np, words):
    """(al bool [B, 32, 15, 130], relaxed, empty_lane) of a decode: the allowed rule of top_ref (constrain_ref's mask and `ascending`,
    rhythm_ref's -2, the BELOW lane) on the mask rows of its samples, the running lo of its own decisions and the keep's words"""
    lo = CR.running_lo(xh[..., 0])
    mk = None if kw.get('pitch_mask') is None else np.broadcast_to(mask_np[:, :, None, :], xh.shape[:3] + (4,))
    return TP.allowed_grid(mk, lo, bool(kw.get('ascending')), words)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', list(PATHS))
def test_1_counts(path):
    lo, hi, steps, refs = limits()
    r = runs(path)
    _, mask_np = RD.mask_pair()
    sel = steps != 0
    n_short = 0
    for room in (False, True):
        ref = refs[room]
        L, H = ref['L'], ref['H']
        words = words_of(ref)
        for name in SETTINGS:
            po, do, xh = r[name, room]
            cnt = notes_len(xh)
            what = (path, name, room)
            assert (cnt <= H)[sel].all(), (what, np.argwhere((cnt > H) & sel)[:4])
            assert (cnt[16:, 7::8][sel[16:, 7::8]] == 0).all()                                    # the rests
            al, rel, emp = allowed_of(xh, setting_kw(name, room), mask_np, words)
            short = (cnt < L) & sel
            if room:
                assert not short.any(), (what, np.argwhere(short)[:4])
                assert not emp.any()
                asc = np.concatenate([np.ones((B, 32, 1), dtype=bool), xh[..., 1:, 0] > xh[..., :-1, 0]], -1)
                live = np.arange(15)[None, None, :] < cnt[..., None]
                assert asc[live].all(), what
            else:
                # a step that fell short ended on a floor decision whose allowed set, replayed, held nothing but <eos>
                fall = RR.fallback(CD.allowed_of(xh, setting_kw(name, room), mask_np), words)
                at = np.take_along_axis(fall, np.minimum(cnt, 14)[..., None], -1)[..., 0]
                assert at[short].all(), (what, np.argwhere(short & ~at)[:4])
                if name != 'cons':
                    assert not short.any() and not fall.any(), what
                n_short += int(short.sum())
            print('%s %s room=%s: %d selected steps, %d short of the floor, %d relaxed decisions; counts %s'
                  % (path, name, room, sel.sum(), short.sum(), rel.sum(), np.bincount(cnt[sel], minlength=16).tolist()))
            assert (cnt[OVER][sel[OVER]] == 3).all() or name == 'cons'                            # floor 6 yields to ceiling 3
            assert (cnt[OPEN][sel[OPEN]] >= 3).all() or (name == 'cons' and not room)
            plain = r[name, room, 'plain']
            for u, w, tag in zip(r[name, room], plain, ('pitch logits', 'duration logits', 'grid')):
                assert np.array_equal(u[FREE], w[FREE]), (what, tag)
            pc = notes_len(plain[2])
            print('%s %s room=%s: without the limits %d selected steps hold more than H notes, %d fewer than L'
                  % (path, name, room, ((pc > H) & sel).sum(), ((pc < L) & sel).sum()))
            assert (xh != plain[2]).any()
    print('%s: %d steps fell short without room under the chord mask with ascending' % (path, n_short))
    assert n_short >= 1                                                  # the caveat is real: room=False can fall short, room=True never did


@pytest.mark.parametrize('path', list(PATHS))
def test_2_ceiling_only_runs_as_the_plain_kind(path):
    """a max_count-only keep is a plain Keep of forced <eos> words: it runs through the argmax and the plain sampled kernels, and equals
    the unlimited decode at every step before the first one whose unlimited count exceeds H -- and there in its first H decisions"""
    _, hi, steps, refs = limits()
    r = runs(path)
    sel = steps != 0
    H = refs[False]['H']
    for name in ('argmax', 'sampled'):
        a, b = r['cap', name], r['cap', name, 'plain']
        cut = (notes_len(b[2]) > H) & sel
        first = np.where(cut.any(1), cut.argmax(1), 32)
        before = np.arange(32)[None, :] < first[:, None]
        assert cut.any() and before.sum() > B and (a[2] != b[2]).any()
        for u, v, tag in zip(a, b, ('pitch logits', 'duration logits', 'grid')):
            assert np.array_equal(u[before], v[before]), (path, name, tag)
        rows = np.nonzero(first < 32)[0]
        for i in rows:
            h = H[i, first[i]]
            assert np.array_equal(a[2][i, first[i], :h], b[2][i, first[i], :h]) and a[2][i, first[i], h, 0] == EOS
        assert (notes_len(a[2]) <= np.where(sel, H, 15)).all()


@pytest.mark.parametrize('path', ('default', 'python-sequenced', 'bf16-step-loop'))
def test_2b_a_forced_eos_behind_a_free_eos_is_inert(path):
    """ceilings two notes above what the unlimited decode holds at every step: every forced <eos> lies behind the step's own free <eos>,
    and the decode is the unlimited one, logits and grid, bit for bit up to every step's <eos>.  This untrained model all but never decides <eos> by itself, so
    the blocks that are asserted to hold such steps are the ascending ones, whose steps end when the pitches run out (the <eos> there
    is a free decision, word -1); the plain argmax and sampled kinds run too, with what they have"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    try:
        with TT.patched(attrs):
            for blk, many in ((None, False), (TT.block(0), False), (TT.block(0, 0.0, 0.0, ascending=True), True),
                              (TT.block(0, ascending=True), True), (RD.cons_block(), True)):
                plain = KD.kdecode(m, z, blk, None)
                hi = np.minimum(notes_len(plain[2]) + 2, 15).astype(np.uint8)
                kp = m.count_limits(max_count=dev(hi))
                assert type(kp) is FF_.Keep and int((kp.pitch == EOS).sum()) == int((hi < 15).sum())
                assert (hi < 15).sum() > 100 or not many
                # every decision up to and including each step's <eos>, at every time step: behind it the forced word is what the grid
                # shows, no later step reads those slots, and the later steps being equal is the inertness
                upto = np.arange(15)[None, None, :] <= notes_len(plain[2])[..., None]
                for u, v, tag in zip(KD.kdecode(m, z, blk, kp), plain, ('pitch logits', 'duration logits', 'grid')):
                    assert np.array_equal(u[upto], v[upto]), (path, tag)
    finally:
        m.set_precision('bf16')


def explained_free(po, do, xh, pn, dn, kw, mask_np, ref, what):
    """every free pitch decision is top_ref.decide_pitch on the emitted logits over the allowed set of the keep's word, every duration
    decision sample_ref.decide_dur; left out: decisions sample_ref.skippable, at most SKIP_CAP of the free ones, asserted"""
    k, l, q = CD.rule(kw)
    words = words_of(ref)
    al, rel, emp = allowed_of(xh, kw, mask_np, words)
    want_p = TP.decide_pitch(po, pn, al, words, KD.T_PITCH, k, l, q)
    skip_p = CR.skippable(po, pn, al, KD.T_PITCH, k, l, q)
    want_d = S.decide_dur(do, dn, KD.T_DUR)
    skip_d = S.skippable(do, dn, KD.T_DUR, S.NOISE_TOL)
    free_p = words < 0
    bad_p = (xh[..., 0] != want_p) & ~skip_p & free_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d
    share_p, share_d = skip_p[free_p].mean(), skip_d.mean()
    print('%s: free pitch decisions %d of %d (%d floor words, %d relaxed), left out %d (share %.5f); duration decisions %d, left out %d '
          '(share %.5f)' % (what, free_p.sum(), free_p.size, (words < -1).sum(), rel.sum(), skip_p[free_p].sum(), share_p, skip_d.size,
                            skip_d.sum(), share_d))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert share_p <= SKIP_CAP and share_d <= SKIP_CAP
    assert np.take_along_axis(al, xh[..., :1], -1)[..., 0][free_p].all()
    forced = words >= 0
    assert (xh[..., 0][forced] == EOS).all() and forced.sum() > 500                               # the ceilings and rests came out


@pytest.mark.parametrize('path', list(PATHS))
def test_3_every_decision_is_the_documented_one(path):
    refs = limits()[3]
    r = runs(path)
    pn, dn = TT.noise(0, B)
    _, mask_np = RD.mask_pair()
    for room in (False, True):
        for name in ('cons', 'sampled'):
            po, do, xh = r[name, room]
            explained_free(po, do, xh, pn, dn, setting_kw(name, room), mask_np, refs[room], '%s %s room=%s' % (path, name, room))


@pytest.mark.parametrize('path', ('default', 'bf16-step-loop'))
def test_4_onsets_and_rests(path):
    """count_limits(onsets=pattern, rests=~pattern): notes exactly on the pattern -- plain sampled (nothing can fall short), and under
    the chord mask with ascending and room=True (the mask yields, the count does not); through the model, which promotes the decode"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    zc, zr = RD.halves(TT.latents())
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    pat = ((t_ * (1 + b_ % 3) + b_) % 4 == 0)
    try:
        with TT.patched(attrs):
            for room, kw in ((False, dict()), (True, dict(pitch_mask=RD.mask_pair()[0], **KD.CONS)), (False, dict(temperature=None))):
                kp, y = m.count_limits(onsets=dev(pat), rests=dev(~pat), room=room, return_counts=True)
                assert isinstance(kp, FF_.CountKeep) and kp.needs_ascending == room and not y.any().item()
                kw = dict(dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW), **kw)
                if kw['temperature'] is None:
                    kw = {}
                est = m.inference_decode(zc, zr, keep=kp, **kw)
                assert m.decoder._last_decode.sampling.numel() == 8
                cnt = notes_len(est)
                assert np.array_equal(cnt > 0, pat), (path, room, np.argwhere((cnt > 0) != pat)[:4])
            host = m.count_limits(onsets=range(0, 32, 4), rests=[t for t in range(32) if t % 4], batch=B)
            cnt = notes_len(m.inference_decode(zc, zr, keep=host, temperature=1.0))
            assert np.array_equal(cnt > 0, np.broadcast_to(np.arange(32) % 4 == 0, (B, 32)))
    finally:
        m.set_precision('bf16')


def test_5_decode_logprob():
    """the log-probability pass after a constrained sampled decode of the first 8 rows under the limits, room off and on, against the
    fp64 walk of logprob_ref over the support the device reports with the keep's words: a forced <eos> is certain (it counts with the
    forced decisions, log q 0), a floor decision is free under its reduced support; counts and err exact, sums at the tolerance of
    tests/test_gpu_decode_logprob_kernels.py; err 0"""
    n = 8
    _, _, steps, refs = limits()
    m = TT.model()
    zc, zr = RD.halves(TT.latents()[:n])
    mask = RD.mask_pair()[0][:n].contiguous()
    free_d = np.full((5, 480 * n), -1, dtype=np.int32)
    for room in (False, True):
        kp = limits_keep(room, slice(0, n))
        fp = LK.host(kp.pitch)
        lo, hi, st, _ = limits()
        assert np.array_equal(fp, CL.build(lo[:n], hi[:n], st[:n], n, room=room)['pitch'])
        kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW, **KD.CONS)
        lp = m.decode_logprob(zc, zr, keep=kp, pitch_mask=mask, **kw)[6]
        torch.cuda.synchronize()
        last = m.decoder._last_decode
        assert last.sampling.numel() == 8
        pitch = LK.host(last.pitch.permute(2, 1, 0, 3))
        dur = LK.host(last.dur.view(15, 32, n, 5, 2).permute(2, 1, 0, 3, 4))
        xg = LK.host(last.xhat)
        finite = np.where(LR.counted(xg)[0][..., None], pitch, np.float32(0))
        kept = RK.kept_with_words(kw, xg, finite, LK.host(mask), fp)
        words = CL.words_of(fp)
        al, rel, emp = allowed_of(xg[:, :, 1:], dict(kw, pitch_mask=mask), LK.host(mask), words)
        live = LR.counted(xg)[0]
        assert not (kept & ~al)[live].any()
        floor = live & (words < -1)
        assert floor.sum() > 100 and not kept[..., EOS][floor & al[..., :128].any(-1)].any()      # the reduced support: no <eos> in it
        r_lp, r_cn, r_er, scale = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, fp, free_d)
        f_lp = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, fp, free_d, dtype=np.float32)[0]
        got, cn = LK.host(lp.step_logp), LK.host(lp.step_counts)
        assert np.array_equal(cn, r_cn) and np.array_equal(LK.host(lp.err), r_er) and not r_er.any()
        for col, fam in enumerate(('logp pitch', 'logp dur', 'logq pitch', 'logq dur')):
            LK.check('count limits room=%s %s' % (room, fam), got[..., col], r_lp[..., col], f_lp[..., col], scale[..., col])
        s, c = LR.fold(got, cn, np.float32)
        assert torch.cat([lp.logp, lp.logq], 1).cpu().numpy().tobytes() == s.tobytes() and np.array_equal(LK.host(lp.counts), c)
        # a step that reached its ceiling: count + 1 pitch decisions, exactly one of them forced (the <eos>)
        cnt = notes_len(xg[:, :, 1:])
        H = refs[room]['H'][:n]
        full = (steps[:n] != 0) & (cnt == H) & (H < 15)
        assert full.sum() >= 1 and (cn[..., 2][full] == 1).all() and np.array_equal(cn[..., 0][full], H[full] + 1)
        assert (cn[..., 2][steps[:n] == 0] == 0).all() and cn[FREE, :, 2].sum() == 0
    # a rest is certain: one forced decision, log q exactly 0
    kp0 = m.count_limits(rests=range(32), batch=n)
    lp0 = m.decode_logprob(zc, zr, keep=kp0, temperature=1.0, seed=TT.SEED, draw=TT.DRAW)[6]
    c0 = LK.host(lp0.step_counts)
    assert (c0[..., 0] == 1).all() and (c0[..., 2] == 1).all() and not LK.host(lp0.step_logp)[..., 2:].any()
    assert not LK.host(lp0.err).any() and (LK.host(lp0.step_logp)[..., 0] < 0).all()


def test_6_graph_replay():
    """one captured graph of the (constrained kind, a keep) decode serves two different limit tables, a rhythm keep and limits built
    into it, each replay equal to its eager decode"""
    x, rsel, wsel, _, _ = RD.crafted()
    m = TT.model()
    zc, zr = RD.halves(TT.latents()[:16])
    xd = dev(x[:16])
    keeps = [limits_keep(False, slice(0, 16)), m.count_limits(min_count=1, max_count=2, steps=range(8, 32), batch=16),
             m.keep_rhythm(xd, dev(rsel[:16])), m.count_limits(min_count=3, max_count=5, keep=m.keep_voice(xd, range(0, 32, 2), lowest=1))]
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
        assert np.array_equal(m.inference_decode(zc, zr, keep=keeps[1], **kw), eager[1])
        assert m.decoder.graph_captures == before + 1 and len(m.decoder._graphs) == held
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_decode_best_of():
    """decode_best_of(n = 2) with the limits of B rows (room=True, so the tiled keep must keep its type): the candidates are the rows of
    a plain decode of the batch tiled twice with the tiled limits, EVERY candidate obeys them, the winner is the first largest logp"""
    lo, hi, steps, refs = limits()
    m = TT.model()
    zc, zr = RD.halves(TT.latents())
    n = 2
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=6, top_k=8)
    keep = limits_keep(True)
    tiled = m.count_limits(min_count=dev(np.tile(lo, (n, 1))), max_count=dev(np.tile(hi, (n, 1))), steps=dev(np.tile(steps, (n, 1))), room=True)
    plain = m.decode_logprob(zc.repeat(n, 1), zr.repeat(n, 1), keep=tiled, **kw)
    cand = m.decoder.last_xhat[:, :, 1:].cpu().numpy()
    out = m.decode_best_of(zc, zr, n, keep=keep, **kw)
    torch.cuda.synchronize()
    assert m.decoder._last_decode.sampling.numel() == 8 and m.decoder._last_decode.sampling.ascending
    sel = np.tile(steps != 0, (n, 1))
    cnt = notes_len(cand)
    assert (cnt <= np.tile(refs[True]['H'], (n, 1)))[sel].all() and (cnt >= np.tile(refs[True]['L'], (n, 1)))[sel].all()
    assert (cand[:B] != cand[B:]).any()
    lp = plain[6]
    want, _ = LR.best_of(lp.logp.sum(1).cpu().numpy().reshape(n, B))
    best = out[6].cpu().numpy()
    assert np.array_equal(best, want) and len(set(best.tolist())) > 1
    rows = torch.from_numpy(want.astype(np.int64) * B + np.arange(B)).to(DEV)
    assert torch.equal(out[1], plain[1][rows]) and torch.equal(out[0], plain[0][rows])
    assert torch.equal(out[7], torch.cat([lp.logp, lp.logq], 1)[rows])


def test_8_rows():
    """rows=: a row of a row-wise decode with the limits is bit-equal to the scalar decode of the whole batch with that row's rule"""
    lo, hi, steps, refs = limits()
    m = TT.model()
    Bs = 8
    zc, zr = RD.halves(TT.latents()[:Bs])
    kp = limits_keep(False, slice(0, Bs))
    temps = [1.0, 0.6] * (Bs // 2)
    ks = [None, 8] * (Bs // 2)
    rows = m.row_sampling(Bs, temps, 0.7, top_k=ks)
    got = m.inference_decode(zc, zr, keep=kp, rows=rows, seed=TT.SEED, draw=TT.DRAW)
    sel = steps[:Bs] != 0
    assert (notes_len(got) <= refs[False]['H'][:Bs])[sel].all() and (notes_len(got) >= refs[False]['L'][:Bs])[sel].all()
    for i in (0, 1):
        want = m.inference_decode(zc, zr, keep=kp, temperature=temps[i], dur_temperature=0.7, top_k=ks[i], seed=TT.SEED, draw=TT.DRAW)
        assert np.array_equal(got[i::2], want[i::2]), i
    assert (got[0::2] != m.inference_decode(zc, zr, keep=kp, temperature=0.6, dur_temperature=0.7, top_k=8, seed=TT.SEED, draw=TT.DRAW)[0::2]).any()


def test_9_yield_bits():
    """yielded bits 1, 2, 4 and 8, each on an input built to raise it, and what the decode does there"""
    m = TT.model()
    x = RD.crafted()[0]
    xd = dev(x)
    zc, zr = RD.halves(TT.latents())
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW)
    # bit 0 (1): the floor lies over the ceiling -- the ceiling wins, exactly H notes
    kp, y = m.count_limits(min_count=7, max_count=2, batch=B, return_counts=True)
    assert (y == 1).all().item()
    assert (notes_len(m.inference_decode(zc, zr, keep=kp, **kw)) == 2).all()
    # bit 1 (2): a rhythm keep owns its steps -- they come out with the rhythm's count, the other steps with the limits'
    K = np.array([[RR.note_count(x[b, t, :, 0]) for t in range(32)] for b in range(B)])
    rk = m.keep_rhythm(xd, range(0, 32, 2), durations=False)
    kp, y = m.count_limits(min_count=1, max_count=1, keep=rk, return_counts=True)
    yn = y.cpu().numpy()
    assert (yn[:, 0::2] == 2).all() and (yn[:, 1::2] == 0).all() and isinstance(kp, FF_.RhythmKeep) and isinstance(kp, FF_.CountKeep)
    assert torch.equal(kp.pitch.view(15, 32, B)[:, 0::2], rk.pitch.view(15, 32, B)[:, 0::2])
    cnt = notes_len(m.inference_decode(zc, zr, keep=kp, **kw))
    assert np.array_equal(cnt[:, 0::2], K[:, 0::2]) and (cnt[:, 1::2] == 1).all()
    # bit 2 (4): a kept voice longer than the ceiling -- the <eos> follows the voice
    xf = KD.crafted()[0]                                                # (the grid before the rhythm tests thinned it: steps of three notes and more)
    vk, kept_n = m.keep_voice(dev(xf), range(32), lowest=3, return_counts=True)
    kn = kept_n.cpu().numpy()
    kp, y = m.count_limits(max_count=2, keep=vk, return_counts=True)
    yn = y.cpu().numpy()
    assert type(kp) is FF_.Keep
    ref = CL.build(np.zeros((1, 32), np.uint8), np.full((1, 32), 2, np.uint8), np.ones((1, 32), np.uint8), B, vk.pitch.cpu().numpy(), vk.dur.cpu().numpy())
    assert np.array_equal(yn, ref['yielded']) and np.array_equal((yn & 4) != 0, ref['J'] > 2) and (yn == 4).sum() > 50
    est = m.inference_decode(zc, zr, keep=kp, **kw)
    assert m.decoder._last_decode.sampling.numel() == 4                                          # no promotion: the plain sampled kind
    cnt = notes_len(est)
    long = yn == 4
    assert np.array_equal(cnt[long], ref['J'][long]) and (cnt[~long] <= 2).all()
    assert np.array_equal(est[..., 0][long][:, :3], xf[:, :, 1:4, 0][long]) and (kn[long] == 3).all()
    # bit 3 (8): room over a voice that ends on the top of the range -- reported; over one that leaves room the floor is reached
    hand = x.copy()
    hand[:, :, 1, 0] = 60
    hand[:, :, 2, 0] = np.where(np.arange(B)[:, None] % 2 == 0, 126, 70)
    hand[:, :, 3] = (EOS, 2, 2, 2, 2, 2)
    vk = m.keep_voice(dev(hand), range(32), lowest=2)
    kp, y = m.count_limits(min_count=5, max_count=8, room=True, keep=vk, return_counts=True)
    yn = y.cpu().numpy()
    assert (yn[0::2] == 8).all() and (yn[1::2] == 0).all() and kp.needs_ascending
    est = m.inference_decode(zc, zr, keep=kp, **kw)
    cnt = notes_len(est)
    assert ((cnt[1::2] >= 5) & (cnt[1::2] <= 8)).all()
    assert (est[0::2, :, 1, 0] == 126).all() and (cnt[0::2] == 2).all()              # no note is left under the first ceiling: the step ends short


def test_10_surface():
    lo, hi, steps, refs = limits()
    m = TT.model()
    Bs = 4
    zc, zr = RD.halves(TT.latents()[:Bs])
    t32 = torch.full((Bs, 32), 3, dtype=torch.int32, device=DEV)
    sel = dev(steps[:Bs])
    # ---- every bad argument is a ValueError before any launch
    for bad in (dict(min_count=-1), dict(min_count=16), dict(max_count=-1), dict(max_count=16), dict(min_count=True), dict(max_count=False),
                dict(min_count=2.0), dict(max_count='4'), dict(min_count=t32.cpu()), dict(max_count=t32.cpu()), dict(min_count=t32.float()),
                dict(max_count=t32.bool()), dict(min_count=t32[:, :31]), dict(max_count=t32[0, :16]), dict(min_count=t32[:3].contiguous(), max_count=t32),
                dict(max_count=t32.view(Bs, 32, 1)), dict(max_count=3, room=1), dict(max_count=3, room='yes'), dict(max_count=3, steps=sel.cpu()),
                dict(max_count=3, steps=sel.int()), dict(max_count=3, steps=sel[:, :31]), dict(max_count=3, steps=sel[0]), dict(max_count=3, steps=[32]),
                dict(max_count=3, onsets=[-1]), dict(max_count=3, rests=7), dict(onsets=sel.cpu()), dict(rests=sel.int()), dict(onsets=sel[:3].contiguous(), rests=sel),
                dict(max_count=3, batch=0), dict(max_count=3, batch=True), dict(max_count=3, batch=2.0), dict(batch=Bs + 1, min_count=t32),
                dict(max_count=3, keep=(1, 2, 3, 4)), dict(keep=m.count_limits(max_count=3, batch=Bs + 1), min_count=t32), dict(), dict(steps=range(8))):
        with pytest.raises(ValueError):
            m.count_limits(**dict(dict(batch=Bs) if 'batch' not in bad else {}, **bad))
    with pytest.raises(ValueError):
        m.count_limits(min_count=2)                                      # nothing tells the batch
    # ---- what comes back
    kp, y = m.count_limits(min_count=dev(lo[:Bs]), max_count=dev(hi[:Bs]), steps=sel, return_counts=True)
    torch.cuda.synchronize()
    assert type(kp) is FF_.CountKeep and isinstance(kp, FF_.Keep) and kp.batch == Bs and kp._fields == FF_.Keep._fields
    assert kp.needs_constrained and not kp.needs_ascending and not kp.err.any().item()
    FF_.check_keep(kp, Bs)
    want = CL.build(lo[:Bs], hi[:Bs], steps[:Bs], Bs)
    assert np.array_equal(kp.pitch.cpu().numpy(), want['pitch']) and np.array_equal(y.cpu().numpy(), want['yielded']) and (kp.dur == -1).all().item()
    room = m.count_limits(min_count=2, batch=Bs, room=True)
    assert isinstance(room, FF_.CountKeep) and room.needs_ascending and room.needs_constrained
    assert type(m.count_limits(max_count=torch.full((32,), 4, dtype=torch.int64, device=DEV), batch=Bs)) is FF_.Keep
    assert type(m.count_limits(rests=sel.bool())) is FF_.Keep and type(m.count_limits(max_count=2, room=True, batch=Bs)) is FF_.Keep
    assert type(m.count_limits(onsets=[0], batch=Bs)) is FF_.CountKeep
    dk = m.dur_limits(max_dur=4, batch=Bs)
    assert type(m.count_limits(max_count=3, keep=dk)) is FF_.DurKeep
    both = m.count_limits(min_count=1, keep=dk)
    assert isinstance(both, FF_.DurKeep) and isinstance(both, FF_.CountKeep) and not both.needs_ascending
    assert type(m.dur_limits(max_dur=4, keep=kp)) is type(m.dur_limits(min_dur=2, keep=kp)) and isinstance(m.dur_limits(max_dur=4, keep=kp), FF_.CountKeep)
    assert m.dur_limits(max_dur=4, keep=room).needs_ascending
    # ---- one level down: a CountKeep beside anything but a constrained block is refused before any launch; a ceiling-only keep goes anywhere
    dec_z = torch.cat([zc, zr], -1)
    m.decoder._last_decode = None
    for blk in (None, TT.block(0), TT.block(0, top_k=8)):
        with pytest.raises(ValueError):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=blk, keep=kp)
    for blk in (TT.block(0, ascending=False),):
        with pytest.raises(ValueError):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=blk, keep=room)
    assert m.decoder._last_decode is None
    cap = m.count_limits(max_count=3, batch=Bs)
    with torch.no_grad():
        for blk in (None, TT.block(0), TT.block(0, top_k=8), TT.block(0, ascending=False)):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=blk, keep=cap)
            assert (notes_len(m.decoder.last_xhat[:, :, 1:].cpu().numpy()) <= 3).all()
        m.decoder(dec_z, True, None, None, 0., 0., sampling=TT.block(0, ascending=False), keep=kp)
    # ---- a TopKeep + limits still forces ascending; a wrong batch is refused before the draw counter moves
    x = RD.crafted()[0]
    top = m.count_limits(min_count=2, max_count=6, keep=m.keep_top(dev(x[:Bs]), range(8)))
    assert isinstance(top, FF_.TopKeep) and isinstance(top, FF_.CountKeep) and top.needs_ascending
    capped_top = m.count_limits(max_count=6, keep=m.keep_top(dev(x[:Bs]), range(8)))
    assert type(capped_top) is FF_.TopKeep
    draws = m._sample_draws
    for k in (top, capped_top, room):
        with pytest.raises(ValueError):
            m.inference_decode(zc, zr, temperature=1.0, ascending=False, keep=k)
    with pytest.raises(ValueError):
        m.inference_decode(zc, zr, temperature=1.0, keep=m.count_limits(max_count=4, batch=8))
    assert m._sample_draws == draws
    # ---- every entry point takes it
    ok = lambda g: bool(((notes_len(g) <= want['H']) & (notes_len(g) >= want['L']))[steps[:Bs] != 0].all())
    m.decode_to_inputs(zc, zr, temperature=1.0, keep=kp)
    assert ok(m.decoder.last_xhat[:, :, 1:].cpu().numpy())
    assert ok(m.inference_decode(zc, zr, keep=kp))
    m.reencode(zc, zr, temperature=0.8, keep=kp)
    assert ok(m.decoder.last_xhat[:, :, 1:].cpu().numpy())
    m.inference_decode(zc, zr, temperature=1.0, keep=top)
    assert m.decoder._last_decode.sampling.ascending
    m.inference_decode(zc, zr, temperature=1.0, keep=room)
    assert m.decoder._last_decode.sampling.ascending and m.decoder._last_decode.sampling.numel() == 8
