"""GPU: the sounding-aware free-running decode (DisentangleVAE.sounding, sounding=; INTEGRATION.md "Sounding state") on every selectable
note-loop path: the decode with sounding= is bit-equal to the decode with the STATIC pitch_mask=mask_eff and keep=Keep(force_pitch_eff, ...)
it reports; what it reports is tests/sounding_ref.py applied to its own grid; no held pitch is struck again, held + onsets stay under
the cap, the floor is reached wherever the replayed allowed set held more than <eos>; the same decode without sounding= breaks each of
these; a kept first step holds its keys down for as long as it says; identities, row independence, composite = Python sequencing,
graph replay, decode_logprob and best-of-n.  B = 32; the model, latents, paths and blocks are those of
tests/test_gpu_truncated_sampling.py and tests/test_gpu_keep_decode.py.
The rules: steps (t + b) % 4 < 3; max_sounding 4 and min_sounding 1; row CAP2 has the cap 2, row FLOOR no cap and the floor 15, row
BOTH the cap 12 over the floor 10, the rows >= 16 the cap 6 at even steps; row FREE has no step selected, row CAP2 every step.  Step 0
is selected in every row but FREE and has, but in the rows CAP2 and BOTH, the floor 15 and no cap: nothing is held there whatever was
decoded, so that is where a decode WITHOUT sounding= can be seen to miss a floor (from step 1 on a plain decode of this untrained model
holds far more keys down than any floor asks)."""
import functools

import numpy as np
import pytest
import torch

import logprob_ref as LR
import rhythm_ref as RR
import sounding_ref as SR
import test_gpu_constrained_decode as CD
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
FREE, CAP2, FLOOR, BOTH = 3, 5, 6, 7
EOS = 129
SETTINGS = ('argmax', 'sampled', 'cons')
BLK = {'argmax': dict(tp=0.0, td=0.0, ascending=False), 'sampled': dict(ascending=False), 'cons': dict(KD.CONS)}
dev = KD.dev
notes_len = RD.notes_len


@functools.lru_cache(maxsize=None)
def tables():
    """(K, F, steps) uint8 [32, 32]"""
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    steps = ((t_ + b_) % 4 < 3).astype(np.uint8)
    steps[FREE] = 0
    steps[CAP2] = 1                                                    # every step of this row is selected: never more than 2 keys down
    K = np.full((B, 32), 4, dtype=np.uint8)
    F = np.ones((B, 32), dtype=np.uint8)
    K[CAP2] = 2
    K[FLOOR], F[FLOOR] = 0, 15
    K[BOTH], F[BOTH] = 12, 10
    K[16:, 0::2] = 6
    steps[:, 0] = 1
    steps[FREE, 0] = 0
    first = [b for b in range(B) if b not in (CAP2, BOTH)]
    K[first, 0], F[first, 0] = 0, 15
    for a in (K, F, steps):
        a.setflags(write=False)
    return K, F, steps


def sounding_of(rows=slice(None), no_restrike=True):
    K, F, steps = tables()
    return TT.model().sounding(no_restrike=no_restrike, max_sounding=dev(K[rows]), min_sounding=dev(F[rows]), steps=dev(steps[rows]))


def base_mask(name, rows=slice(None)):
    return RD.mask_pair()[0][rows].contiguous() if name == 'cons' else None


def block(name, mask=None, offset=0, **kw):
    return TT.block(offset, **dict(BLK[name], **kw), **({} if mask is None else dict(pitch_mask=mask)))


def sdecode(m, z, blk, snd=None, keep=None):
    """one decode one level under the model -> dict(po, do, x (the whole grid [B, 32, 16, 6]), xh (its 15 note slots), and with sounding=
    mask_eff, force_eff, held as numpy plus the device tensors mask_t / force_t)"""
    with torch.no_grad():
        po, do = m.decoder(z, True, None, None, 0., 0., sampling=blk, keep=keep, sounding=snd)
    torch.cuda.synchronize()
    x = m.decoder.last_xhat.cpu().numpy()
    out = dict(po=po.contiguous().cpu().numpy(), do=do.contiguous().cpu().numpy(), x=x, xh=x[:, :, 1:])
    if snd is not None:
        mt, ft, held = m.decoder.last_sounding
        out.update(mask_t=mt, force_t=ft, mask_eff=None if mt is None else mt.cpu().numpy(), force_eff=None if ft is None else ft.cpu().numpy(),
                   held=held.cpu().numpy())
    else:
        assert m.decoder.last_sounding is None
    return out


def static_keep(force_t, dur=None):
    n = force_t.shape[1] // 32
    dur = torch.full((5, 480 * n), -1, dtype=torch.int32, device=DEV) if dur is None else dur
    return FF_.CountKeep(force_t, dur, torch.zeros(n, dtype=torch.int32, device=DEV), n)


def same(a, b, what):
    for k, tag in (('po', 'pitch logits'), ('do', 'duration logits'), ('x', 'grid')):
        assert np.array_equal(a[k], b[k]), (what, tag)


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: per setting with sounding=, again with the static arrays it reported, and without either"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            snd = sounding_of()
            for name in SETTINGS:
                a = out[name] = sdecode(m, z, block(name, base_mask(name)), snd)
                out[name, 'static'] = sdecode(m, z, block(name, a['mask_t']), None, static_keep(a['force_t']))
                out[name, 'plain'] = sdecode(m, z, block(name, base_mask(name)))
    finally:
        m.set_precision('bf16')
    return out


def reference(r, name, **kw):
    K, F, steps = tables()
    mb = RD.mask_pair()[1] if name == 'cons' else None
    return SR.run(r['x'], r['x'].shape[0], True, K, F, steps, mb, None, **kw)


def invariants(xh_full, ref, name, mask_eff):
    """(restruck, over, short, unexplained) bool [B, 32] of a grid against the reference walk of ITS OWN notes: a selected step strikes a
    held pitch / holds more onsets than H' = K - h / holds fewer than L = min(F', H'), and among the short ones those whose replayed
    allowed set at the deciding <eos> held more than <eos>"""
    K, F, steps = tables()
    sel = steps != 0
    xh = xh_full[:, :, 1:]
    cnt = notes_len(xh)
    restruck = np.zeros((B, 32), dtype=bool)
    for b in range(B):
        rem = [0] * 128
        for s in range(32):
            if s > 0:
                rem = SR.advance(rem, SR.accepted(xh_full[b, s - 1], s - 1))
            restruck[b, s] = sel[b, s] and any(rem[p] > 0 for p, _ in SR.accepted(xh_full[b, s], s))
    Hc, Fc = ref['Hc'], ref['Fc']
    over = sel & (cnt > Hc)
    L = np.minimum(Fc, Hc)
    short = sel & (cnt < L)
    words = np.where(np.arange(15)[None, None, :] < L[..., None], -2, -1)
    kw = dict(BLK[name], pitch_mask=True)
    fall = RR.fallback(CD.allowed_of(xh, kw, mask_eff), words)
    at = np.take_along_axis(fall, np.minimum(cnt, 14)[..., None], -1)[..., 0]
    return restruck, over, short, short & ~at


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', list(PATHS))
def test_1_equivalence_and_reference(path):
    """sounding= is the static decode under what it reports, bit for bit, and what it reports is the reference on the emitted grid"""
    r = runs(path)
    for name in SETTINGS:
        a = r[name]
        same(a, r[name, 'static'], (path, name))
        ref = reference(a, name)
        for k in ('mask_eff', 'force_eff', 'held'):
            assert np.array_equal(a[k], ref[k]), (path, name, k)
        assert (a['x'] != r[name, 'plain']['x']).any() and (a['held'] > 0).any() and (a['force_eff'] == EOS).any()
        assert (a['force_eff'] == -2).any()
        for u, v in ((a, r[name, 'plain']),):                                   # a row without a selected step is the plain decode
            for k in ('po', 'do', 'x'):
                assert np.array_equal(u[k][FREE], v[k][FREE]), (path, name, k)


@pytest.mark.parametrize('path', list(PATHS))
def test_2_invariants_and_vacuity(path):
    r = runs(path)
    K, F, steps = tables()
    broke = np.zeros(3, dtype=int)
    for name in SETTINGS:
        a = r[name]
        ref = reference(a, name)
        restruck, over, short, bad = invariants(a['x'], ref, name, a['mask_eff'])
        print('%s %s: %d selected steps; held max %d; %d steps short of the floor, every one explained by an allowed set of <eos> alone'
              % (path, name, (steps != 0).sum(), a['held'].max(), short.sum()))
        assert not restruck.any(), (path, name, np.argwhere(restruck)[:4])
        assert not over.any(), (path, name, np.argwhere(over)[:4])
        assert not bad.any(), (path, name, np.argwhere(bad)[:4])
        # held + onsets <= K wherever the cap still has room for what is held (an unselected step decides freely and can leave more
        # than K keys down; H' = clamp(K - h, 0, 15) then makes the following selected steps rests)
        sounding_now = a['held'] + notes_len(a['xh'])
        room = (steps != 0) & (K > 0) & (a['held'] <= K)
        # what `room` must hold whatever is decoded: all 32 steps of row CAP2 (every step selected, so by induction never more than
        # K = 2 keys down) and step 0 of every other selected row with a cap (nothing is held there)
        least = 32 + int(((steps[:, 0] != 0) & (K[:, 0] > 0)).sum()) - 1
        print('%s %s: held + onsets <= K asked at %d steps (at least %d by construction)' % (path, name, room.sum(), least))
        assert room[CAP2].all() and room.sum() >= least and (sounding_now <= K)[room].all(), (path, name)
        assert (sounding_now[CAP2] <= 2).all() and (a['held'][CAP2] <= 2).all()
        # the same decode without sounding=: its own walk, the base mask
        p = r[name, 'plain']
        pref = reference(p, name)
        mb = RD.mask_pair()[1] if name == 'cons' else np.full((B, 32, 4), -1, np.int32)
        pr, po_, ps, pb = invariants(p['x'], pref, name, mb)
        print('%s %s without sounding=: %d steps strike a held pitch, %d exceed the cap, %d miss a floor they could have reached'
              % (path, name, pr.sum(), po_.sum(), pb.sum()))
        if name != 'argmax':
            broke += (pr.any(), po_.any(), pb.any())
        if name == 'sampled':
            assert pr.any() and po_.any()
    # the vacuity guard: the sampled decodes without sounding= break every invariant somewhere.  A held pitch struck again and the cap
    # exceeded: under plain sampling itself.  A floor missed although more than <eos> was allowed: somewhere among the two sampled
    # settings -- it takes an <eos> the model decided unforced, which this untrained model does at a decision in a hundred, and a step
    # at which less is held than the floor asks, which in a plain decode is step 0
    assert broke.all(), (path, broke)


@pytest.mark.parametrize('path', list(PATHS))
def test_3_bite_a_kept_first_step_holds_its_keys(path):
    """step 0 kept whole from a crafted grid holding (40, 32), (60, 8), (64, 1): whatever the weights decide, 40 is never struck again, 60
    not before step 8, 64 is free at once, something always sounds, and under max_sounding = 3 no step holds more than 3 - held onsets"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    x = np.full((B, 32, 16, 6), 2, dtype=np.int64)
    x[..., 0] = 130
    x[:, :, 0, 0] = 128
    x[:, :, 1, 0] = EOS
    note = lambda p, d: (p,) + tuple(((d - 1) >> k) & 1 for k in (4, 3, 2, 1, 0))
    x[:, 0, 1], x[:, 0, 2], x[:, 0, 3], x[:, 0, 4, 0] = note(40, 32), note(60, 8), note(64, 1), EOS
    try:
        with TT.patched(attrs):
            kp = m.keep(dev(x), [0])
            snd = m.sounding(no_restrike=True, max_sounding=3, batch=B)
            a = sdecode(m, z, block('sampled'), snd, kp)
            plain = sdecode(m, z, block('sampled'), None, kp)
    finally:
        m.set_precision('bf16')
    assert np.array_equal(a['x'][:, 0, :4], x[:, 0, :4]) and (a['x'][:, 0, 4, 0] == EOS).all()            # (an <eos> slot carries the decided bits)
    assert np.array_equal(plain['x'][:, 0], a['x'][:, 0])
    ref = SR.run(a['x'], B, True, np.full((1, 32), 3, np.uint8), None, None, None, kp.pitch.cpu().numpy())
    for k in ('mask_eff', 'force_eff', 'held'):
        assert np.array_equal(a[k], ref[k]), (path, k)
    bit = lambda p: (a['mask_eff'][:, :, p >> 5] >> (p & 31)) & 1                       # [B, 32]
    assert (bit(40)[:, 1:] == 0).all() and (bit(60)[:, 1:8] == 0).all() and (bit(60)[:, 8] == 1).all() and (bit(64)[:, 1] == 1).all()
    assert (bit(40)[:, 0] == 1).all() and (a['held'][:, 1:] >= 1).all() and (a['held'][:, 1] == 2).all()
    cnt = notes_len(a['xh'])
    assert (cnt[:, 1:] <= 3 - a['held'][:, 1:]).all() and (a['held'] <= 3).all()
    struck = lambda g, p: (g[:, 1:, 1:, 0] == p).any()
    assert not struck(a['x'], 40) and not (a['x'][:, 1:8, 1:, 0] == 60).any()
    pc = notes_len(plain['xh'])
    assert (pc[:, 1:] > 3).any() and (struck(plain['x'], 40) or (plain['x'][:, 1:8, 1:, 0] == 60).any())      # ... which the plain decode does


@pytest.mark.parametrize('path', ('default', 'python-sequenced', 'bf16-step-loop'))
def test_4_identities(path):
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    try:
        with TT.patched(attrs):
            cap = m.sounding(max_sounding=127, batch=B)
            assert not cap.needs_constrained and cap.needs_force
            for blk in (None, TT.block(0), TT.block(0, top_k=8), block('cons', base_mask('cons'))):      # a ceiling alone runs in every kind
                a = sdecode(m, z, blk, cap)
                same(a, sdecode(m, z, blk), (path, 'max_sounding=127'))
                assert a['mask_eff'] is None and (a['force_eff'] == -1).all() and (a['held'][:, 1:] > 0).any()
            off = m.sounding(no_restrike=True, steps=[], batch=B)
            for name in SETTINGS:
                a = sdecode(m, z, block(name, base_mask(name)), off)
                same(a, sdecode(m, z, block(name, base_mask(name))), (path, name, 'no step selected'))
                assert a['force_eff'] is None and (a['held'][:, 1:] > 0).any()
    finally:
        m.set_precision('bf16')


@pytest.mark.parametrize('path', ('default', 'python-sequenced', 'bf16-step-loop'))
def test_5_rows_are_independent(path):
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    whole = runs(path)
    try:
        with TT.patched(attrs):
            for name in ('sampled', 'cons'):
                part = sdecode(m, z[16:].contiguous(), block(name, base_mask(name, slice(16, 32)), offset=16), sounding_of().sliced(16, 32))
                for k in ('po', 'do', 'x', 'mask_eff', 'held'):
                    assert np.array_equal(part[k], whole[name][k][16:]), (path, name, k)
                assert np.array_equal(part['force_eff'].reshape(15, 32, 16), whole[name]['force_eff'].reshape(15, 32, B)[:, :, 16:])
    finally:
        m.set_precision('bf16')


def test_6_paths_agree():
    """the composite is the Python sequencing bit for bit; graph replay is the eager decode; one capture serves two Soundings"""
    a, b = runs('default'), runs('python-sequenced')
    for name in SETTINGS:
        same(a[name], b[name], name)
        for k in ('mask_eff', 'force_eff', 'held'):
            assert np.array_equal(a[name][k], b[name][k]), (name, k)
    m = TT.model()
    zc, zr = RD.halves(TT.latents()[:16])
    K, F, steps = tables()
    snds = [sounding_of(slice(0, 16)), m.sounding(no_restrike=True, max_sounding=3, batch=16),
            m.sounding(max_sounding=dev(K[:16]), min_sounding=2, steps=range(4, 32))]
    kp = m.keep(dev(KD.crafted()[0][:16]), [0, 1])
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=9, draw=5, ascending=False)
    cases = [(s, None) for s in snds] + [(snds[1], kp)]
    eager, reports = [], []
    for s, k in cases:
        eager.append(m.inference_decode(zc, zr, sounding=s, keep=k, **kw))
        reports.append([None if t is None else t.cpu().numpy() for t in m.decoder.last_sounding])
    assert all((eager[i] != eager[j]).any() for i in range(4) for j in range(i))
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        for i in (0, 1, 2, 3, 0):
            s, k = cases[i]
            assert np.array_equal(m.inference_decode(zc, zr, sounding=s, keep=k, **kw), eager[i]), i
            mt, ft, held = m.decoder.last_sounding
            assert np.array_equal(held.cpu().numpy(), reports[i][2])
            if reports[i][1] is not None:
                assert np.array_equal(ft.cpu().numpy(), reports[i][1])
            if reports[i][0] is not None:
                assert np.array_equal(mt.cpu().numpy(), reports[i][0])
            lp = m.decoder.decode_logprob()
            assert not lp.err.any().item()
            assert m.decoder.graph_captures == before + 1, i                        # one capture serves every Sounding, with a keep or without
        plain_keys = len(m.decoder._graphs)
        m.inference_decode(zc, zr, **kw)                                            # a decode without sounding: its own key, as before
        assert m.decoder.graph_captures == before + 2 and len(m.decoder._graphs) == plain_keys + 1
        assert m.decoder.last_sounding is None
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_decode_logprob():
    """err == 0 and the sums are logprob_ref's fp64 walk under the EFFECTIVE mask and words, at the tolerance of
    tests/test_gpu_decode_logprob_kernels.py; a forced <eos> written by the cap counts as a forced decision"""
    n = 8
    m = TT.model()
    zc, zr = RD.halves(TT.latents()[:n])
    mask = RD.mask_pair()[0][:n].contiguous()
    free_d = np.full((5, 480 * n), -1, dtype=np.int32)
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW, **KD.CONS)
    lp = m.decode_logprob(zc, zr, sounding=sounding_of(slice(0, n)), pitch_mask=mask, **kw)[6]
    torch.cuda.synchronize()
    last = m.decoder._last_decode
    mt, ft, held = m.decoder.last_sounding
    assert last.sampling.numel() == 8 and last.sampling.pitch_mask is mt and last.force['pitch'] is ft
    fp, me = LK.host(ft), LK.host(mt)
    pitch = LK.host(last.pitch.permute(2, 1, 0, 3))
    dur = LK.host(last.dur.view(15, 32, n, 5, 2).permute(2, 1, 0, 3, 4))
    xg = LK.host(last.xhat)
    K, F, steps = tables()
    ref = SR.run(xg, n, True, K[:n], F[:n], steps[:n], LK.host(mask), None)
    assert np.array_equal(fp, ref['force_eff']) and np.array_equal(me, ref['mask_eff'])
    finite = np.where(LR.counted(xg)[0][..., None], pitch, np.float32(0))
    kept = RK.kept_with_words(kw, xg, finite, me, fp)
    r_lp, r_cn, r_er, scale = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, fp, free_d)
    f_lp = LR.logprob(pitch, dur, xg, kept, 1.0, 0.7, fp, free_d, dtype=np.float32)[0]
    got, cn = LK.host(lp.step_logp), LK.host(lp.step_counts)
    assert not LK.host(lp.err).any() and not r_er.any() and np.array_equal(cn, r_cn)
    for col, fam in enumerate(('logp pitch', 'logp dur', 'logq pitch', 'logq dur')):
        LK.check('sounding %s' % fam, got[..., col], r_lp[..., col], f_lp[..., col], scale[..., col])
    cnt = notes_len(xg[:, :, 1:])
    full = (steps[:n] != 0) & (cnt == ref['Hc']) & (ref['Hc'] < 15)                 # a step that reached its cap: its <eos> is forced
    assert full.sum() >= 1 and (cn[..., 2][full] == 1).all() and np.array_equal(cn[..., 0][full], ref['Hc'][full] + 1)
    assert cn[FREE, :, 2].sum() == 0


def test_8_decode_best_of():
    """decode_best_of(n = 2): the candidates are the rows of a plain decode of the batch tiled twice with the tiled Sounding"""
    m = TT.model()
    zc, zr = RD.halves(TT.latents())
    n = 2
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=6, top_k=8)
    snd = sounding_of()
    plain = m.decode_logprob(zc.repeat(n, 1), zr.repeat(n, 1), sounding=snd.tiled(n), **kw)
    cand = m.decoder.last_xhat.cpu().numpy()
    held = m.decoder.last_sounding[2].cpu().numpy()
    K, F, steps = (np.tile(a, (n, 1)) for a in tables())
    ref = SR.run(cand, n * B, True, K, F, steps)
    assert np.array_equal(held, ref['held']) and (notes_len(cand[:, :, 1:]) <= ref['Hc'])[steps != 0].all()
    assert (cand[:B] != cand[B:]).any()
    out = m.decode_best_of(zc, zr, n, sounding=snd, **kw)
    torch.cuda.synchronize()
    assert m.decoder._last_decode.sampling.numel() == 8 and np.array_equal(m.decoder.last_xhat.cpu().numpy(), cand)
    lp = plain[6]
    want, _ = LR.best_of(lp.logp.sum(1).cpu().numpy().reshape(n, B))
    best = out[6].cpu().numpy()
    assert np.array_equal(best, want) and len(set(best.tolist())) > 1
    rows = torch.from_numpy(want.astype(np.int64) * B + np.arange(B)).to(DEV)
    assert torch.equal(out[1], plain[1][rows]) and torch.equal(out[0], plain[0][rows])
    assert torch.equal(out[7], torch.cat([lp.logp, lp.logq], 1)[rows])


def test_9_surface_on_the_device():
    m = TT.model()
    Bs = 4
    zc, zr = RD.halves(TT.latents()[:Bs])
    dec_z = torch.cat([zc, zr], -1)
    t32 = torch.full((Bs, 32), 3, dtype=torch.int32, device=DEV)
    for bad in (dict(max_sounding=t32.float()), dict(max_sounding=t32[:, :31]), dict(min_sounding=t32[:3].contiguous(), max_sounding=t32),
                dict(max_sounding=3, steps=t32), dict(max_sounding=t32, batch=Bs + 1)):
        with pytest.raises(ValueError):
            m.sounding(**bad)
    snd = m.sounding(no_restrike=True, max_sounding=t32, min_sounding=torch.ones(32, dtype=torch.int64, device=DEV))
    assert snd.batch == Bs and snd.max_sounding.shape == (Bs, 32) and snd.min_sounding.shape == (1, 32) and snd.steps.shape == (1, 32)
    FF_.check_sounding(snd, Bs, torch.device(DEV))
    # one level down: no_restrike or a floor beside anything but a constrained block is refused before any launch; so is force_trace
    m.decoder._last_decode = None
    for blk in (None, TT.block(0), TT.block(0, top_k=8)):
        with pytest.raises(ValueError):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=blk, sounding=snd)
    m.decoder.force_trace = {'pitch': None, 'dur': None}
    try:
        with pytest.raises(ValueError):
            m.decoder(dec_z, True, None, None, 0., 0., sampling=TT.block(0, ascending=False), sounding=snd)
        with pytest.raises(ValueError):
            m.inference_decode(zc, zr, sounding=snd)
    finally:
        m.decoder.force_trace = None
    with pytest.raises(ValueError):
        m.inference_decode(zc, zr, sounding=m.sounding(max_sounding=3, batch=Bs + 1))
    assert m.decoder._last_decode is None
    # through the model: promoted to the constrained kind; a ceiling alone is not; rows= takes it
    m.inference_decode(zc, zr, sounding=snd)
    assert m.decoder._last_decode.sampling.numel() == 8 and not m.decoder._last_decode.sampling.ascending
    cap = m.sounding(max_sounding=3, batch=Bs)
    est = m.inference_decode(zc, zr, sounding=cap, temperature=1.0)
    assert m.decoder._last_decode.sampling.numel() == 4 and m.decoder.last_sounding[0] is None
    assert (notes_len(est) + m.decoder.last_sounding[2].cpu().numpy() <= 3).all()
    est = m.inference_decode(zc, zr, sounding=cap)
    assert m.decoder._last_decode.sampling is None and (notes_len(est) + m.decoder.last_sounding[2].cpu().numpy() <= 3).all()
    est = m.inference_decode(zc, zr, sounding=cap, rows=m.row_sampling(Bs, [1.0, 0.5, 0.8, 1.2]), seed=3, draw=1)
    assert m.decoder._last_decode.sampling.numel() == 10 and (notes_len(est) + m.decoder.last_sounding[2].cpu().numpy() <= 3).all()
    m.decode_to_inputs(zc, zr, temperature=1.0, sounding=snd)
    m.reencode(zc, zr, temperature=0.8, sounding=snd)
    assert m.decoder.last_sounding is not None
    m.inference_decode(zc, zr, temperature=1.0)
    assert m.decoder.last_sounding is None
