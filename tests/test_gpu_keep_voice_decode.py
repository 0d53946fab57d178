"""GPU: kept voices in the free-running decode (DisentangleVAE.keep_voice / split_voice, keep=; INTEGRATION.md "Kept voices") against
tests/keep_voice_ref.py on every selectable note-loop path: the voice comes out as given, the free decisions are the documented draw, the
fixed point, ascending and a pitch range above the voice, the log-probability pass, graph replay, best-of-n and causality.  B = 32; the
model, latents, paths and noise are those of tests/test_gpu_truncated_sampling.py, the grid with its hand-made steps, the chord mask and
the constrained setting those of tests/test_gpu_keep_decode.py.  The keep: voice steps at (t + b) % 4 < 2 with below = 60, row 1 whole."""
import functools

import numpy as np
import pytest
import torch

import keep_voice_ref as V
import test_gpu_constrained_decode as CD
import test_gpu_keep_decode as KD
import test_gpu_truncated_sampling as TT
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
B = 32
BELOW = 60
SETTINGS = ('argmax', 'sampled', 'cons')
dev = KD.dev


@functools.lru_cache(maxsize=None)
def crafted():
    """(x [32, 32, 16, 6], voice selection, whole selection uint8 [32, 32], mode, {durations: keep_voice_ref.build})"""
    x = KD.crafted()[0]
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    vsel = ((t_ + b_) % 4 < 2).astype(np.uint8)
    wsel = np.zeros((B, 32), dtype=np.uint8)
    wsel[1] = 1
    mode = np.where(wsel != 0, 1, 2 * vsel).astype(np.uint8)
    refs = {d: V.build(x, mode, BELOW, None, d) for d in (True, False)}
    for a in (vsel, wsel, mode) + tuple(refs[True].values()) + tuple(refs[False].values()):
        a.setflags(write=False)
    return x, vsel, wsel, mode, refs


def keep_of(x, vsel, wsel=None, **kw):
    out = TT.model().keep_voice(dev(x), dev(vsel), whole_steps=None if wsel is None else dev(wsel), **kw)
    torch.cuda.synchronize()
    return out


def halves(z):
    return z[:, :256].contiguous(), z[:, 256:].contiguous()


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: the crafted voice keep with and without its durations, each under argmax, plain sampling and the
    constrained truncated setting (chord mask + ascending + top_k = 8 + top_p = 0.9)"""
    attrs, prec = PATHS[path]
    x, vsel, wsel, _, _ = crafted()
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            for d in (True, False):
                kp = keep_of(x, vsel, wsel, below=BELOW, durations=d)
                out['argmax', d] = KD.kdecode(m, z, None, kp)
                out['sampled', d] = KD.kdecode(m, z, TT.block(0), kp)
                out['cons', d] = KD.kdecode(m, z, KD.cons_block(), kp)
    finally:
        m.set_precision('bf16')
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', list(PATHS))
def test_1_the_kept_voice_comes_out_as_given(path):
    """where keep_voice_ref says forced, the decoded grid equals x -- pitches and bits; with durations=False pitches only (row 1, kept
    whole, keeps its bits), and the bits of the voice are then drawn: some differ from x"""
    x, _, _, mode, refs = crafted()
    r = runs(path)
    for d in (True, False):
        fp, fd = refs[d]['forced_pitch'], refs[d]['forced_dur']
        assert fp.sum() > 400 and np.array_equal(fp, refs[True]['forced_pitch'])
        for name in SETTINGS:
            xh = r[name, d][2]
            assert np.array_equal(xh[..., 0][fp], x[:, :, 1:, 0][fp]), (path, name, d)
            assert np.array_equal(xh[..., 1:][fd], x[:, :, 1:, 1:][fd]), (path, name, d)
    assert not refs[False]['forced_dur'][mode != 1].any() and refs[False]['forced_dur'][1].any()
    voice_bits = refs[True]['forced_dur'] & ~refs[False]['forced_dur']
    assert voice_bits.sum() > 1500
    assert (r['sampled', False][2][..., 1:][voice_bits] != x[:, :, 1:, 1:][voice_bits]).any()
    assert (r['sampled', True][2] != r['argmax', True][2]).any() and (r['cons', True][2] != r['sampled', True][2]).any()


@pytest.mark.parametrize('path', list(PATHS))
def test_2_free_decisions_are_the_documented_draw(path):
    """test_gpu_keep_decode.explained_free with keep_voice_ref's maps, on the constrained and on the plain sampled decode, with and without
    the voice's durations: every free decision is constrain_ref.decide_pitch / sample_ref.decide_dur on the emitted logits and the restated
    noise (lo of `ascending` runs over the kept voice); the skipped near-ties (printed) are at most SKIP_CAP = 0.005 of the free decisions"""
    _, _, _, _, refs = crafted()
    r = runs(path)
    pn, dn = TT.noise(0, B)
    mask, mask_np = CD.chord_mask()
    for d in (True, False):
        po, do, xh = r['cons', d]
        KD.explained_free(po, do, xh, pn, dn, dict(KD.CONS, pitch_mask=mask), mask_np, refs[d], '%s constrained voice keep, durations=%s' % (path, d))
        po, do, xh = r['sampled', d]
        KD.explained_free(po, do, xh, pn, dn, {}, mask_np, refs[d], '%s sampled voice keep, durations=%s' % (path, d))


@pytest.mark.parametrize('path', ('default', 'cluster4', 'split', 'bf16-step-loop'))
def test_3_fixed_point(path):
    """the model's own argmax decode, kept as voice with below = 128 and lowest = 15 at every step (all its notes, never the <eos>), decodes
    to the same grid and bit-equal logits; so does its own sampled `ascending` decode under the same seed and draw"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    try:
        with TT.patched(attrs):
            for block in (None, TT.block(0, ascending=True)):       # (`ascending` never draws <sos>, which no voice can hold)
                a = TT.decode(m, z, block)
                own = m.decoder.last_xhat.clone()
                kp, kept_n = m.keep_voice(own, range(32), below=128, lowest=15, return_counts=True)
                b = KD.kdecode(m, z, block, kp)
                p = own[:, :, 1:, 0]
                stop = p > 127                                      # the voice ends at <eos> -- or at a decided <sos>, which sets err
                notes = torch.where(stop.any(-1), stop.int().argmax(-1), 15)
                first = torch.gather(p, 2, notes.clamp(max=14).unsqueeze(-1))[..., 0]
                print('%s %s: %d kept notes' % (path, 'argmax' if block is None else 'sampled', int(kept_n.sum())))
                assert torch.equal(kept_n.long(), notes) and int((kp.pitch > 127).sum()) == 0
                assert torch.equal(kp.err != 0, (stop.any(-1) & (first != 129)).any(1)) and (block is None or int(kp.err.sum()) == 0)
                assert block is None or int(kept_n.sum()) > 300
                for u, v, what in zip(a, b, ('pitch logits', 'duration logits', 'grid')):
                    assert np.array_equal(u, v), (path, block is None, what)
    finally:
        m.set_precision('bf16')


def notes_len(xh):
    """int [B, 32]: the notes of each step of a decoded grid [B, 32, 15, 6] -- the decisions before its first <eos>"""
    eos = xh[..., 0] == 129
    return np.where(eos.any(-1), eos.argmax(-1), 15)


def redrawn(xh, K):
    """bool [B, 32, 15]: the note decisions of a decoded grid behind the first K of their step and before the step's first <eos>"""
    n = np.arange(15)
    return (n >= K[..., None]) & (n < notes_len(xh)[..., None])


def test_4_ascending_and_a_range_above_the_voice():
    """sampled with `ascending`: every note behind the voice is above its highest kept pitch (and the step strictly ascending); with
    pitch_mask(lo=60) on top every re-drawn note of a voice or free step is >= 60 -- the mask never checks the forced voice below it,
    which still comes out"""
    x, vsel, wsel, mode, refs = crafted()
    ref = refs[True]
    m = TT.model()
    z = TT.latents()
    kp = keep_of(x, vsel, wsel, below=BELOW)
    fp, Kk = ref['forced_pitch'], ref['K']
    top = np.where(fp, x[:, :, 1:, 0], -1).max(-1)                  # highest kept pitch of the step, -1 without one
    voice = (mode == 2) & (Kk > 0)
    for block, lo in ((TT.block(0, ascending=True), None), (TT.block(0, ascending=True, pitch_mask=m.pitch_mask(lo=60)), 60)):
        xh = KD.kdecode(m, z, block, kp)[2]
        assert np.array_equal(xh[..., 0][fp], x[:, :, 1:, 0][fp])
        assert (xh[..., 0][fp & (mode == 2)[..., None]] < BELOW).all()
        new = redrawn(xh, np.where(mode == 1, 15, Kk)) & (mode != 1)[..., None]
        above = new & voice[..., None]
        assert above.sum() > 20 and new.sum() > above.sum()
        assert (xh[..., 0] > top[..., None])[above].all()
        length = notes_len(xh)
        for b in range(B):
            for t in range(32):
                if mode[b, t] != 1:
                    p = xh[b, t, :length[b, t], 0]
                    assert (np.diff(p) > 0).all() and (p < 128).all(), (b, t)
        if lo is not None:
            assert (xh[..., 0][new] >= lo).all()


def test_5_decode_logprob():
    """the log-probability pass after a sampled voice-keep decode: counts[:, 2] is the number of forced pitch decisions that lie before the
    decoded step's end -- kept_n.sum(1) exactly for every row but row 1, whose whole steps hold unforcible pitches (a free decision in the
    middle of a kept step may end it early); counts[:, 3] likewise the reference's forced bits; err == 0; a step whose counted decisions
    are all forced has logq exactly 0"""
    x, vsel, wsel, mode, refs = crafted()
    ref = refs[True]
    m = TT.model()
    zc, zr = halves(TT.latents())
    kp, kept_n = m.keep_voice(dev(x), dev(vsel), below=BELOW, whole_steps=dev(wsel), return_counts=True)
    out = m.decode_logprob(zc, zr, keep=kp, temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW)
    lp = out[6]
    torch.cuda.synchronize()
    xh = m.decoder.last_xhat[:, :, 1:].cpu().numpy()               # (the decided grid; out[1] is the output path's, cut to max_notes)
    counts, step_counts, step_logp = lp.counts.cpu().numpy(), lp.step_counts.cpu().numpy(), lp.step_logp.cpu().numpy()
    kept_n = kept_n.cpu().numpy()
    assert np.array_equal(kept_n, ref['kept_n'])
    eos = xh[..., 0] == 129
    L = np.where(eos.any(-1), eos.argmax(-1) + 1, 15)
    counted = np.arange(15) < L[..., None]
    want_p = (ref['forced_pitch'] & counted).sum((1, 2))
    want_d = (ref['forced_dur'] & (counted & (xh[..., 0] < 128))[..., None]).sum((1, 2, 3))
    print('forced pitch decisions per row', counts[:, 2], 'kept_n', kept_n.sum(1))
    assert np.array_equal(counts[:, 2], want_p) and np.array_equal(counts[:, 3], want_d)
    rows = np.arange(B) != 1
    assert np.array_equal(counts[rows, 2], kept_n.sum(1)[rows]) and counts[:, 2].sum() > 300
    assert np.array_equal(counts[rows, 3], ref['forced_dur'].sum((1, 2, 3))[rows])
    assert not lp.err.cpu().numpy().any()
    full = (step_counts[..., 2] == step_counts[..., 0]) & (step_counts[..., 3] == step_counts[..., 1])
    assert full[1].sum() > 16 and not full[mode == 2].any()        # the <eos> of a voice step is a free decision
    assert not step_logp[full][:, 2:].any() and (step_logp[~full][:, 2] < 0).any()
    partial = (mode == 2) & (ref['K'] > 0)
    assert np.array_equal(step_counts[..., 2][partial], ref['K'][partial]) and (step_counts[..., 0][partial] > ref['K'][partial]).all()


def test_6_graph_replay():
    """a whole-step keep and then a voice keep through inference_decode are served by ONE captured graph, the decoder holds no more
    graphs after the second than after the first, and both are bit-equal to the eager decode"""
    x, vsel, wsel, _, _ = crafted()
    m = TT.model()
    zc, zr = halves(TT.latents()[:16])
    xd = dev(x[:16])
    keeps = [m.keep(xd, dev(vsel[:16])), m.keep_voice(xd, dev(vsel[:16]), below=BELOW, whole_steps=dev(wsel[:16])),
             m.keep_voice(xd, range(32), lowest=1, durations=False)]
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=9, draw=5)
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
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_decode_best_of():
    """decode_best_of(n = 2) with a voice keep of B rows: the winners' grids and sums are rows of a plain decode of the batch tiled twice
    with the keep built from the tiled grid"""
    x, vsel, wsel, _, _ = crafted()
    m = TT.model()
    zc, zr = halves(TT.latents())
    n = 2
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=6, top_k=8, ascending=True)
    xd, vd, wd = dev(x), dev(vsel), dev(wsel)
    keep = m.keep_voice(xd, vd, below=BELOW, whole_steps=wd)
    tiled = m.keep_voice(xd.repeat(n, 1, 1, 1), vd.repeat(n, 1), below=BELOW, whole_steps=wd.repeat(n, 1))
    plain = m.decode_logprob(zc.repeat(n, 1), zr.repeat(n, 1), keep=tiled, **kw)
    out = m.decode_best_of(zc, zr, n, keep=keep, **kw)
    torch.cuda.synchronize()
    best = out[6].cpu().numpy()
    assert len(set(best.tolist())) == 2                             # not always candidate 0
    rows = torch.from_numpy(best.astype(np.int64) * B + np.arange(B)).to(DEV)
    assert torch.equal(out[1], plain[1][rows]) and torch.equal(out[0], plain[0][rows])
    assert torch.equal(out[7], torch.cat([plain[6].logp, plain[6].logq], 1)[rows])
    fp = crafted()[4][True]['forced_pitch'] & (crafted()[3] == 2)[..., None]     # (the grid of the output path: `ascending` steps come back as decided)
    assert np.array_equal(out[1][:, :, 1:, 0].cpu().numpy()[fp], x[:, :, 1:, 0][fp])
    assert (plain[1][:B] != plain[1][B:]).any()


def test_8_causality():
    """two keeps that differ only from step 16 on -- grid, selection and limit -- decode bit-equal for t < 16"""
    x, vsel, wsel, _, _ = crafted()
    m = TT.model()
    z = TT.latents()
    x2, v2 = x.copy(), vsel.copy()
    x2[:, 16:] = synth_batch(B, 9)[0][:, 16:]
    v2[:, 16:] = 1 - vsel[:, 16:]
    below = np.full((B, 32), BELOW, dtype=np.int32)
    below2 = below.copy()
    below2[:, 16:] = 72
    a = KD.kdecode(m, z, KD.cons_block(), keep_of(x, vsel, wsel, below=dev(below)))
    b = KD.kdecode(m, z, KD.cons_block(), keep_of(x2, v2, wsel, below=dev(below2)))
    assert (a[2][:, 16:] != b[2][:, 16:]).any()
    for u, v in zip(a, b):
        assert np.array_equal(u[:, :16], v[:, :16])
