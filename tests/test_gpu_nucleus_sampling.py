"""GPU: nucleus (top_p) truncation of the free-running decoder's pitch draw against its numpy restatement (tests/nucleus_ref.py over
tests/trunc_ref.py and tests/sample_ref.py): the shared threshold function on crafted rows in both lane layouts, every decision of every
selectable note-loop path explained by the restated rule on the emitted logits, the nucleus trajectory a trajectory of the argmax model,
the kernel variants bit-equal, the degenerate settings, graph replay and the Python / C surface."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import nucleus_ref as NR
import sample_ref as S
import trunc_ref as TR
from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED, DRAW = 11, 4
T_DUR = 0.7
SKIP_CAP = 0.005
P_MIN, P_MAX = 2.0 ** -24, 1 - 2.0 ** -24

# the note-loop paths that can be selected (tests/test_gpu_sampling.py): module attributes of functional_free + the decoder precision
PATHS = {
    'default': ({}, 'bf16'),
    'cluster0': (dict(NOTE_LOOP_CLUSTER=0, NOTE_CLUSTER8=False), 'bf16'),
    'cluster2': (dict(NOTE_LOOP_CLUSTER=2, NOTE_CLUSTER8=False), 'bf16'),
    'cluster4': (dict(NOTE_LOOP_CLUSTER=4, NOTE_CLUSTER8=False), 'bf16'),
    'split': (dict(NOTE_LOOP_SPLIT=True), 'bf16'),
    'python-sequenced': (dict(FREE_COMPOSITE=False), 'bf16'),
    'fp32': ({}, 'fp32'),
    'bf16-step-loop': (dict(FREE_PERSIST=False), 'bf16'),
}
SETTINGS = ('half', 'sharp', 'with_k')          # top_p = 0.5 at T = 1; top_p = 0.9 at T = 0.05; the second with a derived top_k


@contextlib.contextmanager
def patched(attrs):
    old = {k: getattr(FF_, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(FF_, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(FF_, k, v)


@functools.lru_cache(maxsize=None)
def model():
    torch.manual_seed(1234)
    m = M.DisentangleVAE.init_model(torch.device(DEV)).to(DEV)
    m.eval()
    return m.set_precision('bf16')


@functools.lru_cache(maxsize=None)
def latents(B=32):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, 512, generator=g).to(DEV)


@functools.lru_cache(maxsize=None)
def noise(lo, hi):
    """restated noise of the global samples [lo, hi): computed once, shared, never modified"""
    p, d = S.decode_noise(SEED, DRAW, np.arange(lo, hi))
    p.setflags(write=False)
    d.setflags(write=False)
    return p, d


def decode(m, z, block=None, force=None):
    """one free-running decode -> (pitch logits [B,32,15,130], duration logits [B,32,15,5,2], xhat [B,32,15,6]) as numpy"""
    m.decoder.force_trace = force
    try:
        with torch.no_grad():
            po, do = m.decoder(z, True, None, None, 0., 0., sampling=block)
    finally:
        m.decoder.force_trace = None
    torch.cuda.synchronize()
    return po.contiguous().cpu().numpy(), do.contiguous().cpu().numpy(), m.decoder.last_xhat[:, :, 1:].cpu().numpy()


def block(offset=0, tp=1.0, td=T_DUR, seed=SEED, draw=DRAW, **trunc):
    return FF_.sampling_block(DEV, tp, td, seed=seed, draw=draw, sample_offset=offset, **trunc)


def trace_of(xh):
    """decisions [B,32,15,6] -> the force_trace layout of PtvaeDecoder"""
    B = xh.shape[0]
    x = torch.from_numpy(xh.astype(np.int32))
    return {'pitch': x[..., 0].permute(2, 1, 0).reshape(15, 32 * B).contiguous().to(DEV),
            'dur': x[..., 1:].permute(3, 2, 1, 0).reshape(5, 15 * 32 * B).contiguous().to(DEV)}


@functools.lru_cache(maxsize=None)
def derived_top_k():
    """a top_k that competes with top_p = 0.9 at T = 0.05 on this model's logits: the median over the rows of a plain argmax decode of the
    number of classes that nucleus rule keeps"""
    po = decode(model(), latents())[0].reshape(-1, 130)
    k = int(np.median(NR.keep_mask(po, 0.05, q=NR.q24_of(0.9)).sum(-1)))
    assert 1 < k < 130
    return k


def setting(name):
    """(T_pitch, keywords)"""
    return {'half': (1.0, dict(top_p=0.5)), 'sharp': (0.05, dict(top_p=0.9)),
            'with_k': (0.05, dict(top_p=0.9, top_k=derived_top_k()))}[name]


def rule(kw):
    """(top_k, ln_min_p, top_p_q24) of nucleus_ref for the keywords of a block"""
    return kw.get('top_k'), TR.ln_min_p_of(kw.get('min_p')), NR.q24_of(kw.get('top_p'))


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: per setting the nucleus B = 32 decode and z[16:32] at offset 16; the argmax decode and the plain
    sampled decodes at both temperatures; the decisions of the 'with_k' decode forced through the ARGMAX kernels"""
    attrs, prec = PATHS[path]
    derived_top_k()
    m = model()
    m.set_precision(prec)
    z = latents()
    out = {}
    try:
        with patched(attrs):
            for s in SETTINGS:
                T, kw = setting(s)
                out[s] = decode(m, z, block(0, T, **kw))
                out[s + '/half'] = decode(m, z[16:].contiguous(), block(16, T, **kw))
            out['plain'] = decode(m, z)
            out['sampled/1.0'] = decode(m, z, block(0, 1.0))
            out['sampled/0.05'] = decode(m, z, block(0, 0.05))
            out['forced'] = decode(m, z, None, trace_of(out['with_k'][2]))
    finally:
        m.set_precision('bf16')
    return out


def explained(po, do, xh, pn, dn, T, kw, what):
    """every pitch decision is the restated rule (all three rules) on the emitted logits -- but for decisions inside the tolerance of the
    device's logarithm among the KEPT classes, decisions that differ between keeping and dropping the nucleus band classes of their row,
    and rows with a class in the 4-ulp min_p band; the durations stay sample_ref's -> (kept share, thresholds of the single rules)"""
    k, l, q = rule(kw)
    keep = NR.keep_mask(po, T, k, l, q)
    want_p = NR.decide_pitch(po, pn, T, keep=keep)
    band = NR.band_classes(po, T, q)
    skip_band = NR.band_skippable(po, pn, T, k, l, q)
    amb = TR.threshold_ambiguous(po, T, l) if kw.get('min_p') not in (None, 1.0) else np.zeros(po.shape[:-1], dtype=bool)
    skip_noise = S.skippable(np.where(keep, po, np.float32(-1e30)), pn, T, S.NOISE_TOL)
    skip_p = skip_noise | skip_band | amb
    want_d = S.decide_dur(do, dn, T_DUR)
    skip_d = S.skippable(do, dn, T_DUR, S.NOISE_TOL)
    bad_p = (xh[..., 0] != want_p) & ~skip_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d
    print('%s: kept share %.4f; rows with a band class %d, band classes %d; pitch skipped %d of %d (noise %d, band-skippable %d, min_p band %d; '
          'mismatching among the skipped: %d), duration skipped %d of %d'
          % (what, keep.mean(), band.any(-1).sum(), band.sum(), skip_p.sum(), skip_p.size, skip_noise.sum(), skip_band.sum(), amb.sum(),
             ((xh[..., 0] != want_p) & skip_p).sum(), skip_d.sum(), skip_d.size))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert skip_p.mean() <= SKIP_CAP and skip_d.mean() <= SKIP_CAP
    took_keep = np.take_along_axis(keep, xh[..., :1], -1)[..., 0]
    took_band = np.take_along_axis(band, xh[..., :1], -1)[..., 0]
    assert (took_keep | took_band | amb).all()                                             # a decision is a kept class
    if q:                                                                                  # ... and in float64 on the emitted logits: the softmax
        with np.errstate(under='ignore'):                                                  # mass strictly above the decision is below top_p
            p64 = np.exp((po.astype(np.float64) - po.max(-1, keepdims=True)) / float(np.float32(T)))
        p64 /= p64.sum(-1, keepdims=True)
        took = np.take_along_axis(po, xh[..., :1], -1)
        above = np.where(po > took, p64, 0).sum(-1)
        tol = (130 + 130 * q / NR.Q_ONE) * (NR.E_UNITS + 1) * 2.0 ** -20                   # the band's width as a share of Z >= 2^20, and
        assert (above < q / NR.Q_ONE + tol).all(), (what, float(above.max()))               # one more unit per class for the truncation
    return keep.mean()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_1_threshold_function_on_crafted_rows():
    """ptv_debug_pitch_keep runs the decoder's own pitch_keep_threshold() on the 64 crafted rows of nucleus_ref in both lane layouts (16
    lanes x 9 strided columns; 64 lanes x columns lane + 64 i), top_p in {off, 2^-24, 0.1, 0.5, 0.9, 1 - 2^-24} x top_k in {off, 9, 130} x
    min_p in {off, 0.5} at T = 0.7 and T = 0.05: the layouts bit-equal to each other in mask and threshold (no band: the sums are
    integers), the mask equal to nucleus_ref outside the band classes (E = 2 units of 2^-20; and the 4-ulp min_p band), the threshold
    bit-equal on rows without a band class, the best class kept"""
    a = NR.crafted_rows()
    logits = torch.from_numpy(a).to(DEV)
    n_band = n_band_rows = n_in_band_diff = n_set = 0
    for T in (0.7, 0.05):
        for p in (None, P_MIN, 0.1, 0.5, 0.9, P_MAX):
            for k in (None, 9, 130):
                for mp in (None, 0.5):
                    if p is None and k is None and mp is None:
                        continue
                    blk = FF_.sampling_block(DEV, T, top_k=k, min_p=mp, top_p=p)
                    assert blk.numel() == 6
                    got = []
                    for layout in (0, 1):
                        keep = torch.full((64, 130), 7, device=DEV, dtype=torch.uint8)
                        thr = torch.full((64,), 123.0, device=DEV)
                        call('ptv_debug_pitch_keep', ptr(blk), ptr(logits), 64, layout, ptr(keep), ptr(thr), stream_ptr())
                        torch.cuda.synchronize()
                        got.append((keep.cpu().numpy(), thr.cpu().numpy()))
                    what = (T, p, k, mp)
                    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), what
                    l, q = TR.ln_min_p_of(mp), NR.q24_of(p)
                    want_thr = NR.threshold(a, T, k, l, q)
                    want = NR.keep_mask(a, T, k, l, q)
                    band = NR.band_classes(a, T, q)
                    if mp is not None:
                        band = band | TR.band_classes(a, T, l)
                    clean = ~band.any(-1)
                    n_set += 1
                    n_band += int(band.sum())
                    n_band_rows += int((~clean).sum())
                    mask = got[0][0].astype(bool)
                    n_in_band_diff += int((mask != want)[band].sum())
                    assert set(np.unique(got[0][0])) <= {0, 1}
                    assert np.array_equal(mask[~band], want[~band]), (what, np.argwhere((mask != want) & ~band)[:4])
                    assert np.array_equal(got[0][1][clean].view(np.uint32), want_thr[clean].view(np.uint32)), \
                        (what, np.argwhere(clean & (got[0][1] != want_thr))[:4])
                    assert mask[np.arange(64), a.argmax(-1)].all(), what
    print('%d settings x 64 rows: %d band classes in %d rows; masks differing from the restatement inside the band: %d'
          % (n_set, n_band, n_band_rows, n_in_band_diff))


@pytest.mark.parametrize('path', list(PATHS))
def test_2_every_decision_is_explained(path):
    """Nucleus decodes at T_dur = 0.7 under 'half' (top_p = 0.5 at T_pitch = 1), 'sharp' (top_p = 0.9 at T_pitch = 0.05: the init model's
    rows have spread ~0.03, the low T makes the masses uneven) and 'with_k' ('sharp' plus top_k = the median kept count of 'sharp' on the
    model's own logits): every pitch decision of the B = 32 decode and of z[16:32] at sample_offset = 16 is nucleus_ref.decide_pitch on
    the emitted logits and sample_ref's noise; the duration decisions stay sample_ref's.  Skipped: decisions sample_ref.skippable among
    the kept classes plus band-skippable ones (the restated decision differs between keeping and dropping the band classes of the row,
    E = 2), together at most 0.5 %.
    Band-skippable share recomputed with nucleus_ref on 100,000 synthetic 130-wide rows with sample_ref's noise (rows with any band class
    in brackets): spread 0.03 / top_p 0.5 / T = 1: 0 (0); spread 0.03 / top_p 0.9 / T = 0.05: 2e-5 (0.60 %); spread 1 / top_p 0.9 / T = 1:
    5e-5 (1.45 %); spread 3 / top_p 0.9 / T = 1: 2.0e-4 (1.75 %); spread 1 / top_p 0.5 / T = 1: 2e-5 (0.17 %) -- the refinement (the
    band class must win the draw) brings every case far below the cap, rows-with-a-band-class alone would not.
    Each decision is also checked in float64 on the emitted logits (the softmax mass strictly above it is below top_p, within the band's
    width); the kept share is about one half under 'half' (0.45 .. 0.55) and strictly between 0.1 and 0.95 under 'sharp'; under
    'with_k' each of the two rules is the binding one (its threshold strictly the larger) on at least 10 % of the rows."""
    r = runs(path)
    pn, dn = noise(0, 32)
    for s in SETTINGS:
        T, kw = setting(s)
        po, do, xh = r[s]
        share = explained(po, do, xh, pn, dn, T, kw, '%s %s B = 32' % (path, s))
        po2, do2, xh2 = r[s + '/half']
        explained(po2, do2, xh2, pn[16:], dn[16:], T, kw, '%s %s z[16:32] at offset 16' % (path, s))
        if s == 'half':
            assert 0.45 < share < 0.55, share
        elif s == 'sharp':
            assert 0.10 < share < 0.95, share
        else:
            k, l, q = rule(kw)
            t_k, t_p = NR.threshold(po, T, k, l, 0), NR.threshold(po, T, None, l, q)
            print('%s with_k: top_k = %d binds on %.3f of the rows, top_p on %.3f' % (path, k, (t_k > t_p).mean(), (t_p > t_k).mean()))
            assert (t_k > t_p).mean() >= 0.10 and (t_p > t_k).mean() >= 0.10
        if np.array_equal(po[16:, 0, 0], po2[:, 0, 0]):                                    # the sample index is global
            assert np.array_equal(xh[16:, 0, 0, 0], xh2[:, 0, 0, 0])


@pytest.mark.parametrize('path', list(PATHS))
def test_3_the_nucleus_trajectory_is_a_trajectory_of_the_model(path):
    """the nucleus-sampled decisions forced through the argmax kernels (force_trace): the same logits and the same grid, bit for bit;
    and the grid is not the plain-sampled grid of the same seed, draw and temperature"""
    r = runs(path)
    for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
        assert np.array_equal(r['with_k'][k], r['forced'][k]), (path, name)
    for s in SETTINGS:
        assert (r[s][2] != r['sampled/%s' % setting(s)[0]][2]).any(), s


@pytest.mark.parametrize('path', [p for p in PATHS if p not in ('default', 'fp32', 'bf16-step-loop')])
def test_4_variants_agree(path):
    """two paths whose argmax decodes of the same z are bit-equal give bit-equal nucleus decodes"""
    a, b = runs('default'), runs(path)
    for k in range(3):
        assert np.array_equal(a['plain'][k], b['plain'][k]), (path, 'the argmax decodes differ: nothing to compare', k)
    for s in SETTINGS:
        for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
            assert np.array_equal(a[s][k], b[s][k]), (path, s, name)
            assert np.array_equal(a[s + '/half'][k], b[s + '/half'][k]), (path, s, name)


def test_4b_note_loop_kernels_agree_on_one_time_step():
    """ptv_free_note_loop itself, B = 20 (a full panel and a clamped partial one), sampling + truncation bits, top_p = 0.5 with top_k = 40:
    resident heads, streamed heads (bit 21), 2 / 4 / 8 members per panel and the 8-wave kernel give the same logits, decisions and tokens
    bit for bit, the error word is 0, and the decisions are the restated rule"""
    dev = torch.device(DEV)
    m = model()
    P = dict(m.decoder.named_parameters())
    B = 20
    R, Mr = 32 * B, 15 * 32 * B
    panels = (B + 15) // 16
    pk = FF_._free_packs(P, 1024)
    with torch.no_grad():
        tab0, tab = FF_.dur_tabs(P, dev)
    wl = FF_.note_loop_weights(P, pk, tab0, tab)
    g = torch.Generator(device=dev).manual_seed(5)
    GC = torch.randn(B, 1536, device=dev, generator=g) * 0.6
    HN0 = torch.randn(R, 512, device=dev, generator=g) * 0.5
    TOK0 = torch.randn(R, 128, device=dev, generator=g) * 0.5
    T = 0.05
    kw = dict(top_p=0.5, top_k=40)
    blk = block(1000, T, **kw)
    assert blk.numel() == 6
    t = 3
    res = {}
    for name, bits in (('resident', 0x10000), ('streamed', 0x10000 | 0x200000), ('two', 0x10000 | (2 << 18)), ('four', 0x10000 | (4 << 18)),
                       ('eight', 0x10000 | 0x400000), ('8-wave', 0x20000)):
        HN = torch.zeros(16, R, 512, device=dev); HN[0] = HN0
        pitch = torch.zeros(Mr, 136, device=dev)
        dur = torch.zeros(Mr, 10, device=dev)
        idx = torch.zeros(5, Mr, device=dev, dtype=torch.int32)
        TOK = torch.zeros(15, R, 128, device=dev); TOK[0] = TOK0
        PRED = torch.zeros(16, R, 128, device=dev)
        xhat = torch.zeros(B, 32, 16, 6, device=dev, dtype=torch.long)
        plen = torch.zeros(R, device=dev, dtype=torch.int32)
        clustered = name in ('two', 'four', 'eight')
        xch = torch.zeros(panels * 2 * 16 * 512 * 2, device=dev, dtype=torch.bfloat16) if clustered else None
        cnt = torch.zeros(panels + 1, device=dev, dtype=torch.int32) if clustered else None
        io = FF_.note_loop_io(GC=GC, HN=HN, PITCH=pitch, DUR=dur, IDX=idx, TOK=TOK, PRED=PRED, XHAT=xhat, PLEN=plen, XCH=xch, CNT=cnt, BLOCK=blk)
        call('ptv_free_note_loop', wl, io, 136, B, t, 0, bits | FF_.SAMPLE_BIT | FF_.TRUNC_BIT, stream_ptr())
        torch.cuda.synchronize()
        if clustered:
            assert int(cnt[-1]) == 0
        rows = slice(t * B, (t + 1) * B)
        res[name] = (pitch.view(15, R, 136)[:, rows, :130].cpu().numpy(), dur.view(15, R, 10)[:, rows].cpu().numpy(),
                     xhat[:, t, 1:].cpu().numpy(), PRED[:, rows].cpu().numpy())
    for name, got in res.items():
        for a_, b_, what in zip(res['resident'], got, ('pitch', 'dur', 'xhat', 'PRED')):
            assert np.array_equal(a_, b_), (name, what)
    po, do, xh, _ = res['resident']                                                        # [15, B, 130], [15, B, 10], [B, 15, 6]
    gi = np.arange(1000, 1000 + B).reshape(B, 1)
    pn = S.pitch_noise(SEED, DRAW, gi, t, np.arange(15).reshape(1, 15))
    dn = S.dur_noise(SEED, DRAW, gi, t, np.arange(15).reshape(1, 15))
    # (300 decisions: one skipped decision is 0.33 % of them, two would pass the cap)
    explained(po.transpose(1, 0, 2), do.transpose(1, 0, 2).reshape(B, 15, 5, 2), xh, pn, dn, T, kw, 'note loop, one time step')


def test_5_degenerate_settings():
    m = model()
    z = latents()[:20].contiguous()
    plain = decode(m, z)
    # top_p = 1.0 alone, through the truncated instantiation: the plain sampled decode
    sampled = decode(m, z, block(0))
    blk = block(0, top_p=1.0)
    assert blk.numel() == 6
    for a, b in zip(sampled, decode(m, z, blk)):
        assert np.array_equal(a, b)
    # temperature = 0 with any top_p: the argmax decode
    for kw in (dict(top_p=0.5), dict(top_p=P_MIN), dict(top_p=0.9, top_k=3), dict(top_p=0.1, min_p=0.5)):
        for a, b in zip(plain, decode(m, z, block(0, 0.0, 0.0, **kw))):
            assert np.array_equal(a, b), kw
    # ... and T_pitch = 0 beside a sampled duration: the pitch decisions are the argmax of their rows
    po, do, xh = decode(m, z, block(0, 0.0, 0.7, top_p=0.5))
    assert np.array_equal(xh[..., 0], po.argmax(-1))
    # top_p = 2^-24 behaves as top_k = 1: the decision's logit is the row's largest
    for T in (1.0, 0.05):
        po, do, xh = decode(m, z, block(0, T, top_p=P_MIN))
        assert np.array_equal(np.take_along_axis(po, xh[..., :1], -1)[..., 0], po.max(-1)), T
    k1 = decode(m, z, block(0, 1.0, top_k=1))
    for a, b in zip(k1, decode(m, z, block(0, 1.0, top_p=P_MIN))):
        assert np.array_equal(a, b)
    # top_p = 0.5 bites
    assert (decode(m, z, block(0, top_p=0.5))[2][..., 0] != sampled[2][..., 0]).any()


def test_6_graph_replay():
    """one capture serves every top_p / top_k / draw: the values live in the device block"""
    m = model()
    zc, zr = latents()[:16, :256].contiguous(), latents()[:16, 256:].contiguous()
    sets = [dict(top_p=0.5, top_k=None, draw=5), dict(top_p=0.9, top_k=20, draw=6), dict(top_p=0.1, top_k=None, draw=7)]
    eager = [m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, **kw) for kw in sets]
    assert (eager[0] != eager[1]).any() and (eager[1] != eager[2]).any()
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        for i in (0, 1, 2, 0):
            assert np.array_equal(m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, **sets[i]), eager[i]), i
        assert m.decoder.graph_captures == before + 1
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7_surface():
    m = model()
    B = 4
    zc, zr = latents()[:B, :256].contiguous(), latents()[:B, 256:].contiguous()
    xs, cs, prs = (torch.from_numpy(a) for a in synth_batch(B, 5))
    # bad values: ValueError before any launch, at every entry point, whatever device the inputs are on (CPU tensors would be refused
    # later: nothing got that far)
    for kw in (dict(top_p=0.5), dict(temperature=1.0, top_p=0), dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=-0.5),
               dict(temperature=1.0, top_p=1.5), dict(temperature=1.0, top_p=True), dict(temperature=1.0, top_p=float('nan')),
               dict(temperature=1.0, top_p=float('inf')), dict(temperature=1.0, top_k=8, min_p=0.5, top_p=2)):
        for f in (lambda: m.inference_decode(zc.cpu(), zr.cpu(), **kw), lambda: m.decode_to_inputs(zc.cpu(), zr.cpu(), **kw),
                  lambda: m.reencode(zc.cpu(), zr.cpu(), **kw), lambda: m.inference(prs, cs, False, **kw),
                  lambda: m.swap(prs, prs, cs, cs, True, True, **kw), lambda: m.posterior_sample(prs, cs, **kw),
                  lambda: m.posterior_sample(prs, cs, scale=2.0, **kw), lambda: m.prior_sample(prs, cs, **kw),
                  lambda: m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, **kw)):
            with pytest.raises(ValueError):
                f()
    assert FF_.sampling_block(DEV, 1.0).numel() == 4 and FF_.sampling_block(DEV, 1.0, top_p=0.5).numel() == 6
    assert FF_.sampling_block(DEV, 1.0, top_p=1.0).numel() == 6
    assert FF_.sampling_block(DEV, 1.0, top_p=0.5).cpu().tolist()[4:] == FF_.sampling_words(1.0, top_p=0.5)[4:]
    # the keyword reaches the other entry points: under the same seed and draw the grids differ from the plain-sampled ones
    kw = dict(temperature=1.0, seed=3, draw=0)
    tr = dict(top_p=0.1)
    assert (m.inference_decode(zc, zr, **kw) != m.inference_decode(zc, zr, **kw, **tr)).any()
    assert not torch.equal(m.decode_to_inputs(zc, zr, **kw)[1], m.decode_to_inputs(zc, zr, **kw, **tr)[1])
    cs, prs = cs.to(DEV), prs.to(DEV)
    m.use_philox(seed=7, sample_offset=0)
    a0 = m.posterior_sample(prs, cs, temperature=1.0, draw=0)
    m.use_philox(seed=7, sample_offset=0)
    a1 = m.posterior_sample(prs, cs, temperature=1.0, draw=0, **tr)
    assert a0.shape == a1.shape and (a0 != a1).any()
    i0 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0)
    i1 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0, **tr)
    assert i0.shape == i1.shape == (2, 3, 32, 15, 6) and (i0 != i1).any()
    m._philox = None
    # training and a nucleus block do not combine
    blk = block(0, top_p=0.5)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1).requires_grad_(True), False, None, None, 0.5, 0.5, sampling=blk)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1), False, None, None, 0., 0., sampling=blk)
    # ... at the C level the argument errors are what they were: PTV_ERR_ARG before any launch (no pointer is followed)
    dummy = torch.zeros(64, device=DEV)
    wl = F_._parr([dummy] * 16)
    io = F_._parr([dummy] * 22)
    st = stream_ptr()
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, FF_.TRUNC_BIT, st) == -1                     # the truncation bit without the sampling bit
    for train in (1, 2):
        assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, train | FF_.SAMPLE_BIT | FF_.TRUNC_BIT, st) == -1
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 1, FF_.SAMPLE_BIT | FF_.TRUNC_BIT, st) == -1    # a teacher-forcing coin
    io[21] = None
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, FF_.SAMPLE_BIT | FF_.TRUNC_BIT, st) == -1    # the bits without a block
    assert lib().ptv_debug_pitch_keep(None, ptr(dummy), 1, 0, ptr(dummy), ptr(dummy), st) == -1
    assert lib().ptv_debug_pitch_keep(ptr(dummy), ptr(dummy), 1, 2, ptr(dummy), ptr(dummy), st) == -1   # no such layout
