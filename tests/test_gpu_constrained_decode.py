"""GPU: the constrained free-running decode (pitch masks, ascending notes) against its numpy restatement (tests/constrain_ref.py over
sample_ref / trunc_ref / nucleus_ref): the shared allowed rule on crafted rows in both lane layouts, every decision of every selectable
note-loop path explained by the restated rule on the emitted logits, the hard invariants of the PianoTree grammar, the constrained
trajectory a trajectory of the argmax model, vacuous constraints bit-identical to the unconstrained decodes, graph replay and the
Python / C surface.  The paths, the model, the latents and the noise are those of tests/test_gpu_truncated_sampling.py."""
import functools

import numpy as np
import pytest
import torch

import constrain_ref as CR
import nucleus_ref as NR
import sample_ref as S
import test_gpu_truncated_sampling as TT
import trunc_ref as TR
from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
T_PITCH, T_DUR = TT.T_PITCH, TT.T_DUR
SKIP_CAP = 0.005
SETTINGS = ('mask', 'ascending', 'both')
B = 32


@functools.lru_cache(maxsize=None)
def chord_mask():
    """(device int32 [32, 32, 4], the same as numpy): the chord tones of synth_batch's c, built by DisentangleVAE.pitch_mask"""
    c = torch.from_numpy(synth_batch(B, 5)[1]).to(DEV)
    mask = TT.model().pitch_mask(c=c)
    torch.cuda.synchronize()
    m = mask.cpu().numpy()
    m.setflags(write=False)
    return mask, m


def setting(name, rows=slice(None)):
    """keywords of sampling_block for a setting, the mask cut to `rows`"""
    mask = chord_mask()[0][rows].contiguous()
    return {'mask': dict(pitch_mask=mask), 'ascending': dict(ascending=True),
            'both': dict(pitch_mask=mask, ascending=True, top_k=8, top_p=0.9)}[name]


def rule(kw):
    return kw.get('top_k'), TR.ln_min_p_of(kw.get('min_p')), NR.q24_of(kw.get('top_p'))


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: per setting the constrained B = 32 decode at T = 1.0 and z[16:] / mask[16:] at sample_offset 16;
    the argmax and the plain sampled decode; the vacuous constraints; the decisions of 'both' forced through the ARGMAX kernels"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    full = torch.full((B, 32, 4), -1, dtype=torch.int32, device=DEV)
    out = {}
    try:
        with TT.patched(attrs):
            for s in SETTINGS:
                out[s] = TT.decode(m, z, TT.block(0, **setting(s)))
                out[s + '/half'] = TT.decode(m, z[16:].contiguous(), TT.block(16, **setting(s, slice(16, None))))
            out['plain'] = TT.decode(m, z)
            out['sampled'] = TT.decode(m, z, TT.block(0))
            out['vacuous'] = TT.decode(m, z, TT.block(0, pitch_mask=full, ascending=False))
            out['vacuous/row1'] = TT.decode(m, z, TT.block(0, pitch_mask=full[:1].contiguous()))
            out['vacuous/argmax'] = TT.decode(m, z, TT.block(0, 0.0, 0.0, pitch_mask=full, ascending=False))
            out['forced'] = TT.decode(m, z, None, TT.trace_of(out['both'][2]))
    finally:
        m.set_precision('bf16')
    return out


def allowed_of(xh, kw, mask_np):
    """bool [B, 32, 15, 130] of a decode: the mask rows of its samples and the running lo of its own decisions"""
    lo = CR.running_lo(xh[..., 0])
    mk = None if kw.get('pitch_mask') is None else np.broadcast_to(mask_np[:, :, None, :], xh.shape[:3] + (4,))
    return CR.allowed(mk, lo, bool(kw.get('ascending')))


def explained(po, do, xh, pn, dn, kw, mask_np, what):
    """every pitch decision is constrain_ref.decide_pitch on the emitted logits (but for decisions sample_ref.skippable among the
    allowed-and-kept classes and rows in the min_p band); the durations stay sample_ref's -> share of allowed-and-kept classes"""
    k, l, q = rule(kw)
    al = allowed_of(xh, kw, mask_np)
    keep = CR.keep_mask(po, al, T_PITCH, k, l, q)
    want_p = CR.decide_pitch(po, pn, al, T_PITCH, k, l, q)
    amb = (TR.threshold_ambiguous(CR.constrained(po, al), T_PITCH, l) if kw.get('min_p') not in (None, 1.0)
           else np.zeros(po.shape[:-1], dtype=bool))
    skip_p = CR.skippable(po, pn, al, T_PITCH, k, l, q) | amb
    nuc = NR.band_skippable(CR.constrained(po, al), pn, T_PITCH, k, l, q)                  # (reported only: not a reason to skip here)
    want_d = S.decide_dur(do, dn, T_DUR)
    skip_d = S.skippable(do, dn, T_DUR, S.NOISE_TOL)
    bad_p = (xh[..., 0] != want_p) & ~skip_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d
    print('%s: allowed share %.4f, allowed-and-kept %.4f; pitch skipped %d of %d (min_p band %d; mismatching among the skipped: %d; nucleus '
          'band-skippable, not skipped: %d), duration skipped %d of %d'
          % (what, al.mean(), keep.mean(), skip_p.sum(), skip_p.size, amb.sum(), ((xh[..., 0] != want_p) & skip_p).sum(), nuc.sum(),
             skip_d.sum(), skip_d.size))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert skip_p.mean() <= SKIP_CAP and skip_d.mean() <= SKIP_CAP
    assert np.take_along_axis(al, xh[..., :1], -1).all()                                   # a decision is an allowed class, skipped or not
    return keep.mean()


# ---------------------------------------------------------------------------------------------------------------------------------
MASK_BITS = (None, 'full', 0, 15, 16, 31, 32, 63, 64, 127)
LOS = (-1, 0, 62, 63, 64, 126, 127)


def crafted(shift):
    """64 rows (nucleus_ref's crafted ones), a mask and a lo for each: the 70 pairs of MASK_BITS x LOS dealt over the rows, another deal
    per shift; shift 2 ends with rows whose best logit the mask forbids and rows whose allowed values are all equal"""
    a = NR.crafted_rows().copy()
    masks = np.zeros((64, 4), dtype=np.int32)
    lo = np.zeros(64, dtype=np.int32)
    for r in range(64):
        i = (r + 64 * shift) % 70
        mb = MASK_BITS[i % 10]
        lo[r] = LOS[i // 10]
        if mb == 'full':
            masks[r] = -1
        elif mb is not None:
            bits = np.zeros(128, dtype=bool)
            bits[mb] = True
            masks[r] = CR.mask_from_bits(bits)
    if shift == 2:
        g = np.random.default_rng(3)
        for r in range(48, 56):                                                            # the best logit is a pitch the mask forbids
            a[r] = (g.standard_normal(130) * 0.5).astype(np.float32)
            best = int(g.integers(0, 128))
            a[r, best] = 3.0
            bits = np.ones(128, dtype=bool)
            bits[best] = False
            masks[r] = CR.mask_from_bits(bits)
            lo[r] = (-1, 20)[r % 2]
        for r in range(56, 64):                                                            # all allowed values equal (the others are not)
            a[r] = (g.standard_normal(130) * 0.5).astype(np.float32)
            bits = g.random(128) < 0.1
            masks[r] = CR.mask_from_bits(bits)
            lo[r] = (-1, 40)[r % 2]
            al = CR.allowed(masks[r][None])[0]                                              # (with `ascending` a subset of these)
            a[r, al] = np.float32(0.125)
    return a, masks, lo


def test_1_allowed_rule_on_crafted_rows():
    """ptv_debug_pitch_constrain runs the decoder's own pitch_constrain() + pitch_keep_threshold() on 64 crafted rows in both lane layouts:
    masks empty / full / single bits at 0, 15, 16, 31, 32, 63, 64, 127 crossed with lo in {-1, 0, 62, 63, 64, 126, 127}, rows whose best
    logit is disallowed, rows whose allowed values are all equal; each with ascending off / on and top_k in {off, 1, 8, 129}, top_p 0.9,
    min_p 0.5 at T = 0.7.  Keep map and threshold bit-equal between the layouts; the keep map equal to constrain_ref outside the classes
    of the nucleus / min_p bands of the existing rules, the threshold bit-equal on rows without a band class; never empty"""
    T = 0.7
    n_band = 0
    for shift in (0, 1, 2):
        a, masks, lo = crafted(shift)
        logits, dm, dlo = torch.from_numpy(a).to(DEV), torch.from_numpy(masks).to(DEV), torch.from_numpy(lo).to(DEV)
        for asc in (False, True):
            al = CR.allowed(masks, lo, asc)
            con = CR.constrained(a, al)
            for kw in (dict(), dict(top_k=1), dict(top_k=8), dict(top_k=129), dict(top_p=0.9), dict(min_p=0.5)):
                blk = FF_.sampling_block(DEV, T, ascending=asc, **kw)
                assert blk.numel() == 8
                got = []
                for layout in (0, 1):
                    keep = torch.full((64, 130), 7, device=DEV, dtype=torch.uint8)
                    thr = torch.full((64,), 123.0, device=DEV)
                    call('ptv_debug_pitch_constrain', ptr(blk), ptr(logits), ptr(dm), ptr(dlo), 64, layout, ptr(keep), ptr(thr), stream_ptr())
                    torch.cuda.synchronize()
                    got.append((keep.cpu().numpy(), thr.cpu().numpy()))
                what = (shift, asc, kw)
                assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), what
                k, l, q = rule(kw)
                want = CR.keep_mask(a, al, T, k, l, q)
                want_thr = CR.threshold(a, al, T, k, l, q)
                band = (NR.band_classes(con, T, q) | TR.band_classes(con, T, l)) & al
                n_band += int(band.sum())
                clean = ~band.any(-1)
                mask = got[0][0]
                assert set(np.unique(mask)) <= {0, 1}
                mask = mask.astype(bool)
                assert not (mask & ~al).any(), what                                          # a disallowed class is never kept, band or not
                assert np.array_equal(mask[~band], want[~band]), (what, np.argwhere((mask != want) & ~band)[:4])
                assert np.array_equal(got[0][1][clean].view(np.uint32), want_thr[clean].view(np.uint32)), what
                assert mask.any(-1).all() and mask[np.arange(64), con.argmax(-1)].all(), what   # never empty: the best allowed class is kept
    print('classes inside a band of the existing rules over all settings: %d' % n_band)


@pytest.mark.parametrize('path', list(PATHS))
def test_2_every_decision_is_explained(path):
    """Constrained decodes at T_pitch = 1.0, T_dur = 0.7 under the chord-tone mask of synth_batch's c, `ascending`, and both with top_k = 8,
    top_p = 0.9: every pitch decision of the B = 32 decode and of z[16:] / mask[16:] at sample_offset = 16 is constrain_ref.decide_pitch
    on the emitted logits, the sample's mask words and the running lo of the emitted decisions; the durations stay sample_ref's.
    Skipped: decisions sample_ref.skippable among the allowed-and-kept classes (and rows in the min_p band: none of these settings has
    one), at most 0.5 %.
    The reference's own share, constrain_ref on 200,000 synthetic 130-wide rows of the model's spread (sd 0.03) with sample_ref's noise
    at T = 1: chord-tone mask (37.4 pitches allowed on average) 1 of 200,000 skippable (5e-6); ascending with lo uniform in -1..98: 0;
    both with top_k = 8, top_p = 0.9: 1 (5e-6) -- three orders of magnitude under the cap.
    Nucleus band-skippable decisions (nucleus_ref's band of the device exponential) on those rows under 'both': 0 -- top_k = 8 is the
    binding rule on rows this flat, so the band is no reason to skip here and is only counted.  The on-card counts are printed."""
    r = runs(path)
    pn, dn = TT.noise(0, 32)
    mask_np = chord_mask()[1]
    for s in SETTINGS:
        kw = setting(s)
        po, do, xh = r[s]
        explained(po, do, xh, pn, dn, kw, mask_np, '%s %s B = 32' % (path, s))
        po2, do2, xh2 = r[s + '/half']
        explained(po2, do2, xh2, pn[16:], dn[16:], kw, mask_np[16:], '%s %s z[16:] at offset 16' % (path, s))
        assert (xh[..., 0] != r['sampled'][2][..., 0]).any(), s                              # the constraint bites
        if np.array_equal(po[16:, 0, 0], po2[:, 0, 0]):                                    # the sample index and the mask row travel with the sample
            assert np.array_equal(xh[16:, 0, 0, 0], xh2[:, 0, 0, 0])


@pytest.mark.parametrize('path', list(PATHS))
def test_3_hard_invariants(path):
    """no skips: every pitch before the first <eos> of a step lies in the mask; under `ascending` the pitches of a step are strictly
    increasing (over all 15 note steps, <eos> rows between them or not) and never <sos>"""
    r = runs(path)
    bits = CR.mask_bits(chord_mask()[1])                                                   # [B, 32, 128]
    for s in SETTINGS:
        for key, rows in ((s, slice(None)), (s + '/half', slice(16, None))):
            p = r[key][2][..., 0]                                                          # [b, 32, 15]
            before = np.cumsum(p == CR.EOS, -1) == 0
            if s != 'ascending':
                ok = np.take_along_axis(bits[rows], np.minimum(p, 127), -1) | (p >= 128)
                assert ok[before].all(), (path, key, np.argwhere(before & ~ok)[:4])
                assert ok.all(), (path, key)                                               # (and after it: the rule does not end with the step)
            if s != 'mask':
                assert (p != CR.SOS).all(), (path, key)
                lo = CR.running_lo(p)
                assert ((p > lo) | (p == CR.EOS)).all(), (path, key, np.argwhere((p <= lo) & (p != CR.EOS))[:4])
                assert before.any(-1).mean() > 0.5                                         # (steps do hold notes: the check is not vacuous)


def test_3b_output_path_merges_nothing():
    """decode_to_inputs(..., ascending=True, max_notes=15): no bad-pitch bit in err and every note of the list is a cell of the piano-roll"""
    m = TT.model()
    z = TT.latents()
    zc, zr = z[:, :256].contiguous(), z[:, 256:].contiguous()
    for kw in (dict(temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW), dict()):   # sampled, and the constrained argmax
        pr_mat, x, c, notes, count, err = m.decode_to_inputs(zc, zr, max_notes=15, ascending=True, **kw)
        torch.cuda.synchronize()
        assert int((err & 1).sum()) == 0
        assert torch.equal((pr_mat != 0).sum((1, 2)).int(), count.int())
        assert int(count.sum()) > 0
    # ... which the plain sampled decode of the same seed does not give: that is what the constraint is for
    pr_mat, x, c, notes, count, err = m.decode_to_inputs(zc, zr, max_notes=15, temperature=1.0, dur_temperature=0.7, seed=TT.SEED, draw=TT.DRAW)
    print('plain sampled decode: %d samples with a bad pitch, %d notes merged away'
          % (int((err & 1).ne(0).sum()), int((count.int() - (pr_mat != 0).sum((1, 2)).int()).sum())))


@pytest.mark.parametrize('path', list(PATHS))
def test_4_the_constrained_trajectory_is_a_trajectory_of_the_model(path):
    """the constrained decisions forced through the argmax kernels (force_trace): the same logits and the same grid, bit for bit"""
    r = runs(path)
    for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
        assert np.array_equal(r['both'][k], r['forced'][k]), (path, name)


def test_4b_note_loop_kernels_agree_on_one_time_step():
    """ptv_free_note_loop itself, B = 20 (a full panel and a clamped partial one), sampling + constraint bits, a random mask of B rows and
    `ascending` with top_k = 8: resident heads, streamed heads (bit 21), 2 / 4 / 8 members per panel and the 8-wave kernel give the same
    logits, decisions and tokens bit for bit, the decisions are the restated rule, and the one-row form of a mask equals its expanded form"""
    dev = torch.device(DEV)
    m = TT.model()
    P = dict(m.decoder.named_parameters())
    Bn = 20
    R, Mr = 32 * Bn, 15 * 32 * Bn
    panels = (Bn + 15) // 16
    pk = FF_._free_packs(P, 1024)
    with torch.no_grad():
        tab0, tab = FF_.dur_tabs(P, dev)
    wl = FF_.note_loop_weights(P, pk, tab0, tab)
    g = torch.Generator(device=dev).manual_seed(5)
    GC = torch.randn(Bn, 1536, device=dev, generator=g) * 0.6
    HN0 = torch.randn(R, 512, device=dev, generator=g) * 0.5
    TOK0 = torch.randn(R, 128, device=dev, generator=g) * 0.5
    rng = np.random.default_rng(12)
    mask_np = CR.mask_from_bits(rng.random((Bn, 32, 128)) < 0.4)
    mask = torch.from_numpy(mask_np).to(DEV)
    t = 3
    one_np = np.ascontiguousarray(mask_np[7:8])
    one = torch.from_numpy(one_np).to(DEV)
    kw = dict(ascending=True, top_k=8)
    blocks = {'rows': TT.block(1000, pitch_mask=mask, **kw), 'one': TT.block(1000, pitch_mask=one, **kw),
              'one-expanded': TT.block(1000, pitch_mask=one.expand(Bn, 32, 4).contiguous(), **kw)}
    assert all(b.numel() == 8 for b in blocks.values())
    variants = [('resident', 0x10000, 'rows'), ('streamed', 0x10000 | 0x200000, 'rows'), ('two', 0x10000 | (2 << 18), 'rows'),
                ('four', 0x10000 | (4 << 18), 'rows'), ('eight', 0x10000 | 0x400000, 'rows'), ('8-wave', 0x20000, 'rows'),
                ('resident/one', 0x10000, 'one'), ('resident/one-expanded', 0x10000, 'one-expanded'), ('8-wave/one', 0x20000, 'one')]
    res = {}
    for name, bits, which in variants:
        HN = torch.zeros(16, R, 512, device=dev); HN[0] = HN0
        pitch = torch.zeros(Mr, 136, device=dev)
        dur = torch.zeros(Mr, 10, device=dev)
        idx = torch.zeros(5, Mr, device=dev, dtype=torch.int32)
        TOK = torch.zeros(15, R, 128, device=dev); TOK[0] = TOK0
        PRED = torch.zeros(16, R, 128, device=dev)
        xhat = torch.zeros(Bn, 32, 16, 6, device=dev, dtype=torch.long)
        plen = torch.zeros(R, device=dev, dtype=torch.int32)
        clustered = name in ('two', 'four', 'eight')
        xch = torch.zeros(panels * 2 * 16 * 512 * 2, device=dev, dtype=torch.bfloat16) if clustered else None
        cnt = torch.zeros(panels + 1, device=dev, dtype=torch.int32) if clustered else None
        io = FF_.note_loop_io(GC=GC, HN=HN, PITCH=pitch, DUR=dur, IDX=idx, TOK=TOK, PRED=PRED, XHAT=xhat, PLEN=plen, XCH=xch, CNT=cnt,
                              BLOCK=blocks[which])
        call('ptv_free_note_loop', wl, io, 136, Bn, t, 0, bits | FF_.SAMPLE_BIT | FF_.TRUNC_BIT | FF_.CONS_BIT, stream_ptr())
        torch.cuda.synchronize()
        if clustered:
            assert int(cnt[-1]) == 0
        rows = slice(t * Bn, (t + 1) * Bn)
        res[name] = (pitch.view(15, R, 136)[:, rows, :130].cpu().numpy(), dur.view(15, R, 10)[:, rows].cpu().numpy(),
                     xhat[:, t, 1:].cpu().numpy(), PRED[:, rows].cpu().numpy())
    for name, got in res.items():
        ref = res['resident/one'] if '/one' in name or name == '8-wave/one' else res['resident']
        for a_, b_, what in zip(ref, got, ('pitch', 'dur', 'xhat', 'PRED')):
            assert np.array_equal(a_, b_), (name, what)
    gi = np.arange(1000, 1000 + Bn).reshape(Bn, 1)
    pn = S.pitch_noise(TT.SEED, TT.DRAW, gi, t, np.arange(15).reshape(1, 15))
    for name, mk in (('resident', mask_np[:, t]), ('resident/one', np.broadcast_to(one_np[:, t], (Bn, 4)))):
        po, do, xh, _ = res[name]                                                          # [15, Bn, 130], [15, Bn, 10], [Bn, 15, 6]
        po = po.transpose(1, 0, 2)
        al = CR.allowed(np.broadcast_to(mk[:, None, :], (Bn, 15, 4)), CR.running_lo(xh[..., 0]), True)
        want = CR.decide_pitch(po, pn, al, T_PITCH, 8)
        skip = CR.skippable(po, pn, al, T_PITCH, 8)
        assert not ((xh[..., 0] != want) & ~skip).any() and skip.mean() <= SKIP_CAP, name
        assert np.take_along_axis(al, xh[..., :1], -1).all()
    assert (res['resident'][2] != res['resident/one'][2]).any()


@pytest.mark.parametrize('path', list(PATHS))
def test_5_vacuous_constraints(path):
    """a full mask with ascending=False through the constrained kernels is the same decode without the keywords, bit for bit (also as a
    one-row mask); at temperature 0 it is the argmax decode"""
    r = runs(path)
    for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
        assert np.array_equal(r['vacuous'][k], r['sampled'][k]), (path, name)
        assert np.array_equal(r['vacuous/row1'][k], r['sampled'][k]), (path, name)
        assert np.array_equal(r['vacuous/argmax'][k], r['plain'][k]), (path, name)


def test_5b_temperature_none_is_the_constrained_argmax():
    """temperature=None with a constraint: a T = 0 block through the constrained kernels -- the first maximal ALLOWED index of every
    emitted row, the draw counter untouched, bit-identical to the argmax decode when the constraint is vacuous"""
    m = TT.model()
    z = TT.latents()
    zc, zr = z[:, :256].contiguous(), z[:, 256:].contiguous()
    mask, mask_np = chord_mask()
    full = torch.full((1, 32, 4), -1, dtype=torch.int32, device=DEV)
    draws = m._sample_draws
    plain = m.inference_decode(zc, zr)
    assert np.array_equal(m.inference_decode(zc, zr, pitch_mask=full, ascending=False), plain)
    got = m.inference_decode(zc, zr, pitch_mask=mask, ascending=True)
    assert m._sample_draws == draws
    po, do, xh = TT.decode(m, z, FF_.sampling_block(DEV, 0.0, 0.0, pitch_mask=mask, ascending=True))
    assert np.array_equal(got, xh)
    al = allowed_of(xh, dict(pitch_mask=mask, ascending=True), mask_np)
    assert np.array_equal(xh[..., 0], np.where(al, po, np.float32(-np.inf)).argmax(-1))
    assert (got != plain).any()
    for kw in (dict(seed=3), dict(draw=1), dict(sample_offset=4), dict(top_k=3)):
        with pytest.raises(ValueError):
            m.inference_decode(zc, zr, ascending=True, **kw)


def test_6_graph_replay():
    """replay equals eager; two different masks and both values of `ascending` (and other seeds / draws) are served by ONE capture"""
    m = TT.model()
    zc, zr = TT.latents()[:16, :256].contiguous(), TT.latents()[:16, 256:].contiguous()
    mask_a = chord_mask()[0][:16].contiguous()
    mask_b = m.pitch_mask(pitch_classes=(0, 2, 4, 5, 7, 9, 11), lo=36, hi=96)               # one row: C major in a range
    assert mask_b.shape == (1, 32, 4)
    sets = [dict(pitch_mask=mask_a, ascending=True, draw=5), dict(pitch_mask=mask_b, ascending=False, draw=6),
            dict(pitch_mask=mask_b, ascending=True, top_k=8, top_p=0.9, draw=7), dict(ascending=True, draw=8)]
    eager = [m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, **kw) for kw in sets]
    assert all((eager[i] != eager[j]).any() for i in range(4) for j in range(i))
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        for i in (0, 1, 2, 3, 0, 1):
            assert np.array_equal(m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, **sets[i]), eager[i]), i
        assert m.decoder.graph_captures == before + 1
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_surface():
    m = TT.model()
    Bs = 4
    zc, zr = TT.latents()[:Bs, :256].contiguous(), TT.latents()[:Bs, 256:].contiguous()
    good = torch.full((Bs, 32, 4), -1, dtype=torch.int32, device=DEV)
    # rejected inputs: ValueError before any launch (CPU latents would be refused later: nothing got that far)
    bad = (dict(pitch_mask=good.cpu()), dict(pitch_mask=good.long()), dict(pitch_mask=good.float()), dict(pitch_mask=good[:, :, :3]),
           dict(pitch_mask=good[:, :16]), dict(pitch_mask=good.view(Bs * 32, 4)), dict(pitch_mask=torch.cat([good, good])[:Bs + 1]),
           dict(pitch_mask=good.cpu().numpy()), dict(ascending=1), dict(ascending='yes'), dict(ascending=None, pitch_mask=good[:2]))
    for kw in bad:
        for t in (dict(), dict(temperature=1.0)):
            with pytest.raises(ValueError):
                m.inference_decode(zc.cpu(), zr.cpu(), **kw, **t)
            with pytest.raises(ValueError):
                m.decode_to_inputs(zc.cpu(), zr.cpu(), **kw, **t)
    xs, cs, prs = (torch.from_numpy(a).to(DEV) for a in synth_batch(Bs, 5))
    for kw in (dict(pitch_mask=good.cpu()), dict(pitch_mask=good[:3].contiguous()), dict(ascending=0)):
        for fn in (lambda: m.inference(prs.cpu(), cs.cpu(), False, **kw), lambda: m.swap(prs.cpu(), prs.cpu(), cs.cpu(), cs.cpu(), True, True, **kw),
                   lambda: m.posterior_sample(prs.cpu(), cs.cpu(), **kw), lambda: m.prior_sample(prs.cpu(), cs.cpu(), **kw),
                   lambda: m.reencode(zc.cpu(), zr.cpu(), **kw)):
            with pytest.raises(ValueError):                                                # (CPU inputs: nothing was encoded)
                fn()
    with pytest.raises(ValueError):                                                        # interp: the rows are the flattened [bs * int_count] batch
        m.interp(prs[:2].cpu(), cs[:2].cpu(), prs[2:].cpu(), cs[2:].cpu(), int_count=3, pitch_mask=good[:2].contiguous())
    # the block: its word count selects the kernels
    assert FF_.sampling_block(DEV, 1.0, ascending=False).numel() == 8 and FF_.sampling_block(DEV, 1.0, top_k=3, pitch_mask=good).numel() == 8
    blk = FF_.sampling_block(DEV, 1.0, pitch_mask=good[:1].contiguous(), ascending=True)
    w = blk.cpu().tolist()
    assert w[6] == (FF_.CONS_ASCENDING | FF_.CONS_MASK_ROW1) and w[7] == blk.pitch_mask.data_ptr()
    assert FF_.sampling_block(DEV, 1.0, top_k=3).cpu().tolist() == FF_.sampling_block(DEV, 1.0, top_k=3, ascending=False).cpu().tolist()[:6]
    # the keywords reach the other entry points
    kw = dict(temperature=1.0, seed=3, draw=0)
    mask = m.pitch_mask(c=cs)
    assert mask.shape == (Bs, 32, 4) and mask.dtype == torch.int32
    cons = dict(pitch_mask=mask, ascending=True)
    assert (m.inference_decode(zc, zr, **kw) != m.inference_decode(zc, zr, **kw, **cons)).any()
    assert not torch.equal(m.decode_to_inputs(zc, zr, **kw)[1], m.decode_to_inputs(zc, zr, **kw, **cons)[1])
    assert torch.is_tensor(m.reencode(zc, zr, **kw, **cons)[0].mean)
    m.use_philox(seed=7, sample_offset=0)
    a0 = m.posterior_sample(prs, cs, temperature=1.0, draw=0)
    m.use_philox(seed=7, sample_offset=0)
    a1 = m.posterior_sample(prs, cs, temperature=1.0, draw=0, **cons)
    assert a0.shape == a1.shape and (a0 != a1).any()
    s1 = m.swap(prs, prs.flip(0), cs, cs.flip(0), True, False, temperature=1.0, draw=0, **cons)
    p1 = m.prior_sample(prs, cs, temperature=1.0, draw=0, **cons)
    bits = CR.mask_bits(mask.cpu().numpy())
    for got in (a1, s1, p1):
        p = got[..., 0]
        assert (np.take_along_axis(bits, np.minimum(p, 127), -1) | (p == CR.EOS)).all() and (p != CR.SOS).all()
    one = m.pitch_mask(pitch_classes=[0, 4, 7])
    i0 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0)
    i1 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0, pitch_mask=one, ascending=True)
    i6 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0,
                  pitch_mask=one.expand(6, 32, 4).contiguous(), ascending=True)
    assert i0.shape == i1.shape == (2, 3, 32, 15, 6) and (i0 != i1).any() and np.array_equal(i1, i6)
    pi = i1[..., 0]
    assert np.isin(pi[pi < 128] % 12, (0, 4, 7)).all()
    m._philox = None
    # training and a constrained block do not combine
    blk = TT.block(0, ascending=True)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1).requires_grad_(True), False, None, None, 0.5, 0.5, sampling=blk)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1), False, None, None, 0., 0., sampling=blk)
    with pytest.raises(ValueError):                                                        # eight words that no sampling_block() made
        m.decoder(torch.cat([zc, zr], -1), True, None, None, 0., 0., sampling=torch.zeros(8, device=DEV, dtype=torch.int64))
    with pytest.raises(ValueError):                                                        # a mask of another batch
        m.decoder(torch.cat([zc, zr], -1), True, None, None, 0., 0., sampling=TT.block(0, pitch_mask=torch.cat([good, good])))
    # ... at the C level: PTV_ERR_ARG before any launch (no pointer is followed)
    dummy = torch.zeros(64, device=DEV)
    wl = F_._parr([dummy] * 16)
    io = F_._parr([dummy] * 22)
    st = stream_ptr()
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, FF_.CONS_BIT, st) == -1                      # the bit without the sampling bit
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, FF_.CONS_BIT | FF_.TRUNC_BIT, st) == -1
    for train in (1, 2):
        assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, train | FF_.SAMPLE_BIT | FF_.CONS_BIT, st) == -1
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 1, FF_.SAMPLE_BIT | FF_.CONS_BIT, st) == -1     # a teacher-forcing coin
    io[21] = None
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, FF_.SAMPLE_BIT | FF_.CONS_BIT, st) == -1     # the bits without a block
    d, di = ptr(dummy), ptr(torch.zeros(64, device=DEV, dtype=torch.int32))
    dl = ptr(torch.zeros(64, device=DEV, dtype=torch.long))
    assert lib().ptv_note_token_sample_cons(d, 136, di, 4, d, d, 128, d, 128, dl, 3072, di, 1, 0, None, 4, None, 0, st) == -1   # no block
    assert lib().ptv_note_token_sample_cons(d, 136, di, 4, d, d, 128, d, 128, dl, 3072, di, 16, 0, None, 4, d, 0, st) == -1     # n past 15
    assert lib().ptv_note_token_sample_cons(d, 136, di, 4, d, d, 128, d, 128, dl, 3072, di, 1, 0, None, 4, d, 32, st) == -1     # t past 31
    assert lib().ptv_debug_pitch_constrain(None, d, di, di, 1, 0, d, d, st) == -1
    assert lib().ptv_debug_pitch_constrain(d, d, None, di, 1, 0, d, d, st) == -1
    assert lib().ptv_debug_pitch_constrain(d, d, di, di, 1, 2, d, d, st) == -1                          # no such layout
    for args in ((None, 1, 0, 127, 0xfff, None), (di, 0, 0, 127, 0xfff, None), (di, 1, -1, 127, 0xfff, None), (di, 1, 0, 128, 0xfff, None),
                 (di, 1, 60, 59, 0xfff, None), (di, 1, 0, 127, 0x1000, None), (di, 1, 0, 127, -1, None)):
        assert lib().ptv_pitch_mask_build(*args, st) == -1
    for kw in (dict(lo=-1), dict(hi=128), dict(lo=5, hi=4), dict(pitch_classes=[12]), dict(pitch_classes=0x1000), dict(c=cs.cpu()),
               dict(c=cs[:, :, :24]), dict(c=cs.double()), dict(batch=0), dict(c=cs, batch=Bs + 1), dict(lo=True)):
        with pytest.raises(ValueError):
            m.pitch_mask(**kw)


def test_8_mask_builder_matches_numpy():
    """ptv_pitch_mask_build (DisentangleVAE.pitch_mask) against constrain_ref.mask_build, bit for bit: every constraint alone and all ANDed,
    an odd batch, more than one block of the kernel"""
    m = TT.model()
    g = np.random.default_rng(9)
    for Bn in (1, 3, 37):
        c = np.zeros((Bn, 8, 36), dtype=np.float32)
        c[:, :, 12:24] = (g.random((Bn, 8, 12)) < 0.3) * g.choice([1.0, -2.0, 0.5], (Bn, 8, 12))
        c[:, :, :12] = 1.0
        dc = torch.from_numpy(c).to(DEV)
        for kw in (dict(), dict(c=c), dict(pitch_classes=0b101010110101), dict(lo=36, hi=84), dict(c=c, pitch_classes=0b000010010001, lo=1, hi=126),
                   dict(pitch_classes=0), dict(lo=127, hi=127), dict(lo=0, hi=0), dict(lo=31, hi=32)):
            dk = dict(kw, c=dc) if 'c' in kw else dict(kw, batch=Bn)
            got = m.pitch_mask(**dk)
            torch.cuda.synchronize()
            assert got.dtype == torch.int32 and tuple(got.shape) == (Bn, 32, 4)
            assert np.array_equal(got.cpu().numpy(), CR.mask_build(Bn, **kw)), (Bn, list(kw))
    assert np.array_equal(m.pitch_mask(pitch_classes=[0, 4, 7]).cpu().numpy(), CR.mask_build(1, pitch_classes=0b10010001))
