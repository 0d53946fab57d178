"""GPU: truncated sampling (top_k / min_p) of the free-running decoder's pitch draw against its numpy restatement (tests/trunc_ref.py over
tests/sample_ref.py): the shared threshold function on crafted rows in both lane layouts, every decision of every selectable note-loop
path explained by the restated rule on the emitted logits, the truncated trajectory a trajectory of the argmax model, the kernel variants
bit-equal, the degenerate settings, graph replay and the Python / C surface."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

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
T_PITCH, T_DUR = 1.0, 0.7
SKIP_CAP = 0.005

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
SETTINGS = ('top_k', 'min_p', 'both')


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


def block(offset=0, tp=T_PITCH, td=T_DUR, seed=SEED, draw=DRAW, **trunc):
    return FF_.sampling_block(DEV, tp, td, seed=seed, draw=draw, sample_offset=offset, **trunc)


def trace_of(xh):
    """decisions [B,32,15,6] -> the force_trace layout of PtvaeDecoder"""
    B = xh.shape[0]
    x = torch.from_numpy(xh.astype(np.int32))
    return {'pitch': x[..., 0].permute(2, 1, 0).reshape(15, 32 * B).contiguous().to(DEV),
            'dur': x[..., 1:].permute(3, 2, 1, 0).reshape(5, 15 * 32 * B).contiguous().to(DEV)}


@functools.lru_cache(maxsize=None)
def derived_min_p():
    """a min_p that bites on this model's logits: the median over the rows of a plain argmax decode of m - (65th largest logit), as a
    probability ratio at T_PITCH -- about half the classes of a typical row pass"""
    po = decode(model(), latents())[0].reshape(-1, 130)
    gap = np.median(po.max(-1).astype(np.float64) - np.sort(po, -1)[:, 130 - 65].astype(np.float64))
    assert gap > 0
    return float(math.exp(-gap / T_PITCH))


def setting(name):
    return {'top_k': dict(top_k=8), 'min_p': dict(min_p=derived_min_p()), 'both': dict(top_k=8, min_p=derived_min_p())}[name]


def rule(kw):
    """(top_k, ln_min_p) of trunc_ref for the keywords of a block"""
    return kw.get('top_k'), TR.ln_min_p_of(kw.get('min_p'))


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: per setting the truncated B = 32 decode and z[16:32] at offset 16; the argmax and the plain
    sampled decode; the decisions of the 'both' decode forced through the ARGMAX kernels"""
    attrs, prec = PATHS[path]
    derived_min_p()
    m = model()
    m.set_precision(prec)
    z = latents()
    out = {}
    try:
        with patched(attrs):
            for s in SETTINGS:
                out[s] = decode(m, z, block(0, **setting(s)))
                out[s + '/half'] = decode(m, z[16:].contiguous(), block(16, **setting(s)))
            out['plain'] = decode(m, z)
            out['sampled'] = decode(m, z, block(0))
            out['forced'] = decode(m, z, None, trace_of(out['both'][2]))
    finally:
        m.set_precision('bf16')
    return out


def explained(po, do, xh, pn, dn, kw, what, T=T_PITCH):
    """every pitch decision is the restated truncated rule on the emitted logits (but for decisions inside the tolerance of the device's
    logarithm among the KEPT classes, and rows with a class in the 4-ulp min_p band); the durations stay sample_ref's -> kept share"""
    k, l = rule(kw)
    keep = TR.keep_mask(po, T, k, l)
    want_p = TR.decide_pitch_trunc(po, pn, T, k, l)
    amb = TR.threshold_ambiguous(po, T, l) if kw.get('min_p') not in (None, 1.0) else np.zeros(po.shape[:-1], dtype=bool)
    skip_p = S.skippable(np.where(keep, po, np.float32(-1e30)), pn, T, S.NOISE_TOL) | amb
    want_d = S.decide_dur(do, dn, T_DUR)
    skip_d = S.skippable(do, dn, T_DUR, S.NOISE_TOL)
    bad_p = (xh[..., 0] != want_p) & ~skip_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d
    print('%s: kept share %.4f; pitch skipped %d of %d (%d of them rows in the min_p band; mismatching among the skipped: %d), duration '
          'skipped %d of %d' % (what, keep.mean(), skip_p.sum(), skip_p.size, amb.sum(), ((xh[..., 0] != want_p) & skip_p).sum(),
                                skip_d.sum(), skip_d.size))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert skip_p.mean() <= SKIP_CAP and skip_d.mean() <= SKIP_CAP
    assert (np.take_along_axis(keep, xh[..., :1], -1)[..., 0] | amb).all()                # a decision is a kept class
    return keep.mean()


# ---------------------------------------------------------------------------------------------------------------------------------
def crafted_rows():
    """64 hand-made 130-wide rows"""
    g = np.random.default_rng(21)
    base = lambda sd=0.03: (g.standard_normal(130) * sd).astype(np.float32)
    rows = []
    for k in (2, 9, 16, 17, 129):                                  # duplicates straddling the k-th place (ranks k - 1 .. k + 2 equal)
        for shift in (0, 1):
            r = base()
            order = np.argsort(-r, kind='stable')
            lo, hi = max(k - 2 + shift, 0), min(k + 2 + shift, 130)
            r[order[lo:hi]] = r[order[lo]]
            rows.append(r)
    for v in (0.5, 0.0, -0.0, -3.0):                               # all-equal rows
        rows.append(np.full(130, v, dtype=np.float32))
    for col in (129, 0, 128, 16, 63, 64):                          # the best value in the last / first column (and at lane-layout seams)
        r = base()
        r[col] = 1.0
        rows.append(r)
        r = base(1.0)
        r[col] = r.max() + np.float32(0.25)
        rows.append(r)
    one = np.float32(1.0)                                          # values differing in the last bit
    for step in (1, 2, 3):
        r = np.array([one + np.float32(i % (step + 1)) * np.spacing(one) for i in range(130)], dtype=np.float32)
        rows.append(g.permutation(r))
        rows.append(-g.permutation(r))
    for n_neg in (0, 3, 60):                                       # +-0.0 among a few other values
        r = np.where(g.integers(0, 2, 130) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        r[g.choice(130, n_neg, replace=False)] = -np.abs(base(1.0))[:n_neg]
        rows.append(r)
        r2 = r.copy()
        r2[g.choice(130, 4, replace=False)] = np.abs(base(1.0))[:4]
        rows.append(r2)
    while len(rows) < 64:                                          # plain rows of several spreads, some quantised (many ties)
        r = base((0.03, 1.0, 30.0)[len(rows) % 3])
        rows.append(np.round(r * 8) / 8 if len(rows) % 2 else r)
    a = np.stack(rows[:64]).astype(np.float32)
    assert a.shape == (64, 130)
    return a


def test_1_threshold_function_on_crafted_rows():
    """ptv_debug_pitch_keep runs the decoder's own pitch_keep_threshold() on 64 crafted rows in both lane layouts (16 lanes x 9 strided
    columns; 64 lanes x columns lane + 64 i), k in {off, 1, 2, 9, 16, 17, 129, 130, 1000} x min_p in {off, 1.0, 0.5, 1e-6} at T = 0.7:
    mask and threshold bit-equal to trunc_ref (the mask outside the classes of the 4-ulp min_p band), and the layouts bit-equal to each other"""
    a = crafted_rows()
    T = 0.7
    logits = torch.from_numpy(a).to(DEV)
    n_band = 0
    for k in (None, 1, 2, 9, 16, 17, 129, 130, 1000):
        for mp in (None, 1.0, 0.5, 1e-6):
            if k is None and mp is None:
                continue
            blk = FF_.sampling_block(DEV, T, top_k=k, min_p=mp)
            assert blk.numel() == 6
            got = []
            for layout in (0, 1):
                keep = torch.full((64, 130), 7, device=DEV, dtype=torch.uint8)
                thr = torch.full((64,), 123.0, device=DEV)
                call('ptv_debug_pitch_keep', ptr(blk), ptr(logits), 64, layout, ptr(keep), ptr(thr), stream_ptr())
                torch.cuda.synchronize()
                got.append((keep.cpu().numpy(), thr.cpu().numpy()))
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), (k, mp)
            l = TR.ln_min_p_of(mp)
            want_thr = TR.threshold(a, T, k, l)
            want = TR.keep_mask(a, T, k, l)
            band = TR.band_classes(a, T, l) if mp not in (None, 1.0) else np.zeros(a.shape, dtype=bool)   # (min_p = 1: T * 0, nothing is rounded)
            n_band += int(band.sum())
            assert np.array_equal(got[0][1].view(np.uint32), want_thr.view(np.uint32)), (k, mp, np.argwhere(got[0][1] != want_thr)[:4])
            assert set(np.unique(got[0][0])) <= {0, 1}
            assert np.array_equal(got[0][0].astype(bool)[~band], want[~band]), (k, mp)
            assert got[0][0].astype(bool)[np.arange(64), a.argmax(-1)].all()
    print('classes inside the 4-ulp min_p band over all settings: %d' % n_band)


@pytest.mark.parametrize('path', list(PATHS))
def test_2_every_decision_is_explained(path):
    """Truncated decodes at T_pitch = 1.0, T_dur = 0.7 under top_k = 8, a min_p derived from the model's own logits (derived_min_p) and both:
    every pitch decision of the B = 32 decode and of z[16:32] at sample_offset = 16 is trunc_ref.decide_pitch_trunc on the emitted logits
    and sample_ref's noise; the duration decisions stay sample_ref's.  Skipped: decisions sample_ref.skippable among the kept classes and
    rows threshold_ambiguous, together at most 0.5 %.
    Kept share: under min_p alone it must lie strictly between 10 % and 90 % (the rule bites, and not on everything).  top_k = 8 keeps
    8 / 130 = 6.2 % of a row by definition (more only through ties), so under 'top_k' and 'both' the share is asserted against that
    figure instead: at most 8 / 130 plus ties, at least 1 / 130.
    Share of rows in the 4-ulp band, recomputed with trunc_ref on 200,000 synthetic 130-wide rows of this model's spread (sd 0.03): 8.5e-5
    of the rows at the min_p derived the same way from those rows (0.9265: kept share 0.483), 5.5e-5 at min_p = 0.9, 5.0e-5 at 0.97 -- two
    orders of magnitude below the cap.  The on-card count is printed.  The device does not fuse m + T * ln_min_p (the library is built
    with -ffp-contract=off), so a row in the band is not expected to differ either."""
    r = runs(path)
    pn, dn = noise(0, 32)
    for s in SETTINGS:
        kw = setting(s)
        po, do, xh = r[s]
        share = explained(po, do, xh, pn, dn, kw, '%s %s B = 32' % (path, s))
        po2, do2, xh2 = r[s + '/half']
        explained(po2, do2, xh2, pn[16:], dn[16:], kw, '%s %s z[16:32] at offset 16' % (path, s))
        if s == 'min_p':
            assert 0.10 < share < 0.90, share
        else:
            assert 1 / 130 <= share <= 8 / 130 + 0.01, share
        if np.array_equal(po[16:, 0, 0], po2[:, 0, 0]):                                    # the sample index is global
            assert np.array_equal(xh[16:, 0, 0, 0], xh2[:, 0, 0, 0])


@pytest.mark.parametrize('path', list(PATHS))
def test_3_the_truncated_trajectory_is_a_trajectory_of_the_model(path):
    """the truncated-sampled decisions forced through the argmax kernels (force_trace): the same logits and the same grid, bit for bit;
    and the grid is not the plain-sampled grid of the same seed and draw"""
    r = runs(path)
    for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
        assert np.array_equal(r['both'][k], r['forced'][k]), (path, name)
    for s in SETTINGS:
        assert (r[s][2] != r['sampled'][2]).any(), s


@pytest.mark.parametrize('path', [p for p in PATHS if p not in ('default', 'fp32', 'bf16-step-loop')])
def test_4_variants_agree(path):
    """two paths whose argmax decodes of the same z are bit-equal give bit-equal truncated decodes"""
    a, b = runs('default'), runs(path)
    for k in range(3):
        assert np.array_equal(a['plain'][k], b['plain'][k]), (path, 'the argmax decodes differ: nothing to compare', k)
    for s in SETTINGS:
        for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
            assert np.array_equal(a[s][k], b[s][k]), (path, s, name)
            assert np.array_equal(a[s + '/half'][k], b[s + '/half'][k]), (path, s, name)


def test_4b_note_loop_kernels_agree_on_one_time_step():
    """ptv_free_note_loop itself, B = 20 (a full panel and a clamped partial one), sampling + truncation bits, top_k = 8 and a min_p: resident
    heads, streamed heads (bit 21), 2 / 4 / 8 members per panel and the 8-wave kernel give the same logits, decisions and tokens bit for
    bit, and the decisions are the restated rule"""
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
    kw = dict(top_k=8, min_p=0.97)
    blk = block(1000, **kw)
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
    explained(po.transpose(1, 0, 2), do.transpose(1, 0, 2).reshape(B, 15, 5, 2), xh, pn, dn, kw, 'note loop, one time step')


def test_5_degenerate_settings():
    m = model()
    z = latents()[:20].contiguous()
    plain = decode(m, z)
    # top_k = 130 without min_p, through the truncated instantiation: the plain sampled decode
    sampled = decode(m, z, block(0))
    blk = block(0, top_k=130)
    assert blk.numel() == 6
    for a, b in zip(sampled, decode(m, z, blk)):
        assert np.array_equal(a, b)
    for a, b in zip(sampled, decode(m, z, block(0, top_k=1000, min_p=0.0))):
        assert np.array_equal(a, b)
    # min_p = 1.0: only the classes tied for best
    po, do, xh = decode(m, z, block(0, min_p=1.0))
    assert np.array_equal(np.take_along_axis(po, xh[..., :1], -1)[..., 0], po.max(-1))
    # temperature = 0 with any truncation: the argmax decode
    for kw in (dict(top_k=3), dict(min_p=0.5), dict(top_k=1, min_p=1.0)):
        for a, b in zip(plain, decode(m, z, block(0, 0.0, 0.0, **kw))):
            assert np.array_equal(a, b), kw
    # top_k = 2: every decision among the two best classes of its emitted row
    po, do, xh = decode(m, z, block(0, top_k=2))
    second = np.sort(po, -1)[..., 128]
    assert (np.take_along_axis(po, xh[..., :1], -1)[..., 0] >= second).all()
    assert (xh[..., 0] != plain[2][..., 0]).any()
    # top_k = 1 (T_dur = 0: the duration bits are their argmax): the argmax decode, per sample, up to and including the first row whose two
    # best emitted logits are exactly equal -- there the draw chooses among the tied classes while the argmax takes the lowest
    po, do, xh = decode(m, z, block(0, 1.0, 0.0, top_k=1))
    B = z.shape[0]
    srt = np.sort(po.reshape(B, 480, 130), -1)
    tied = srt[..., 129] == srt[..., 128]
    n_tied = 0
    for b in range(B):
        f = int(np.argmax(tied[b])) if tied[b].any() else 480
        n_tied += int(f < 480)
        e = min(f + 1, 480)
        assert np.array_equal(po.reshape(B, 480, 130)[b, :e], plain[0].reshape(B, 480, 130)[b, :e]), b
        assert np.array_equal(xh.reshape(B, 480, 6)[b, :f], plain[2].reshape(B, 480, 6)[b, :f]), b
        if f < 480:
            assert po.reshape(B, 480, 130)[b, f, xh.reshape(B, 480, 6)[b, f, 0]] == srt[b, f, 129]
    print('top_k = 1: %d of %d samples had a row whose two best logits are exactly equal' % (n_tied, B))


def test_6_graph_replay():
    """one capture serves every top_k / min_p / draw: the values live in the device block"""
    m = model()
    zc, zr = latents()[:16, :256].contiguous(), latents()[:16, 256:].contiguous()
    sets = [dict(top_k=8, min_p=None, draw=5), dict(top_k=3, min_p=0.97, draw=6), dict(top_k=None, min_p=0.9, draw=7)]
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
    # bad values: ValueError before any launch (CPU tensors would be refused later: nothing got that far)
    for kw in (dict(top_k=8), dict(min_p=0.5), dict(temperature=1.0, top_k=0), dict(temperature=1.0, top_k=-3), dict(temperature=1.0, top_k=True),
               dict(temperature=1.0, top_k=2.0), dict(temperature=1.0, min_p=1.5), dict(temperature=1.0, min_p=-0.1),
               dict(temperature=1.0, min_p=float('nan')), dict(temperature=1.0, min_p=float('inf')), dict(temperature=1.0, min_p=True)):
        with pytest.raises(ValueError):
            m.inference_decode(zc.cpu(), zr.cpu(), **kw)
        with pytest.raises(ValueError):
            m.decode_to_inputs(zc.cpu(), zr.cpu(), **kw)
    assert FF_.sampling_block(DEV, 1.0).numel() == 4 and FF_.sampling_block(DEV, 1.0, top_k=8).numel() == 6
    assert FF_.sampling_block(DEV, 1.0, min_p=0.0).numel() == 6
    # the keywords reach the other entry points: under the same seed and draw the grids differ from the plain-sampled ones
    kw = dict(temperature=1.0, seed=3, draw=0)
    tr = dict(top_k=2, min_p=0.5)
    assert (m.inference_decode(zc, zr, **kw) != m.inference_decode(zc, zr, **kw, **tr)).any()
    assert not torch.equal(m.decode_to_inputs(zc, zr, **kw)[1], m.decode_to_inputs(zc, zr, **kw, **tr)[1])
    xs, cs, prs = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, 5))
    m.use_philox(seed=7, sample_offset=0)
    a0 = m.posterior_sample(prs, cs, temperature=1.0, draw=0)
    m.use_philox(seed=7, sample_offset=0)
    a1 = m.posterior_sample(prs, cs, temperature=1.0, draw=0, **tr)
    assert a0.shape == a1.shape and (a0 != a1).any()
    i0 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0)
    i1 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0, **tr)
    assert i0.shape == i1.shape == (2, 3, 32, 15, 6) and (i0 != i1).any()
    m._philox = None
    # training and a truncated block do not combine
    blk = block(0, top_k=8)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1).requires_grad_(True), False, None, None, 0.5, 0.5, sampling=blk)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1), False, None, None, 0., 0., sampling=blk)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1), True, None, None, 0., 0., sampling=torch.zeros(5, device=DEV, dtype=torch.int64))   # not a block
    # ... at the C level: PTV_ERR_ARG before any launch (no pointer is followed)
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
