"""GPU: the sampled free-running decode (seeded temperature sampling of pitch and duration) against its numpy restatement
(tests/sample_ref.py), on every note-loop path that can be selected: every decision is the restated rule applied to the emitted logits and
the keyed noise, the sampled trajectory is a trajectory of the argmax model, the kernel variants agree bit for bit, and the Python surface
(graph replay, keywords, refusals) does what INTEGRATION.md says."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import sample_ref as S
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

# the note-loop paths that can be selected today: module attributes of functional_free (restored afterwards) + the decoder precision
PATHS = {
    'default': ({}, 'bf16'),                                                      # eight-member cluster at these sizes
    'cluster0': (dict(NOTE_LOOP_CLUSTER=0, NOTE_CLUSTER8=False), 'bf16'),         # one workgroup per panel, resident heads
    'cluster2': (dict(NOTE_LOOP_CLUSTER=2, NOTE_CLUSTER8=False), 'bf16'),
    'cluster4': (dict(NOTE_LOOP_CLUSTER=4, NOTE_CLUSTER8=False), 'bf16'),
    'split': (dict(NOTE_LOOP_SPLIT=True), 'bf16'),                                # the 8-wave producer / head kernel
    'python-sequenced': (dict(FREE_COMPOSITE=False), 'bf16'),
    'fp32': ({}, 'fp32'),                                                         # the step loop
    'bf16-step-loop': (dict(FREE_PERSIST=False), 'bf16'),                         # the step loop with the fused duration GRU (other geometries' path)
}


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


def block(offset=0, tp=T_PITCH, td=T_DUR, seed=SEED, draw=DRAW):
    return FF_.sampling_block(DEV, tp, td, seed=seed, draw=draw, sample_offset=offset)


def trace_of(xh):
    """decisions [B,32,15,6] -> the force_trace layout of PtvaeDecoder"""
    B = xh.shape[0]
    x = torch.from_numpy(xh.astype(np.int32))
    return {'pitch': x[..., 0].permute(2, 1, 0).reshape(15, 32 * B).contiguous().to(DEV),
            'dur': x[..., 1:].permute(3, 2, 1, 0).reshape(5, 15 * 32 * B).contiguous().to(DEV)}


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: sampled B = 32, sampled z[16:32] at offset 16, argmax B = 32, the sampled decisions forced
    through the ARGMAX kernels"""
    attrs, prec = PATHS[path]
    m = model()
    m.set_precision(prec)
    z = latents()
    try:
        with patched(attrs):
            full = decode(m, z, block(0))
            half = decode(m, z[16:].contiguous(), block(16))
            plain = decode(m, z)
            forced = decode(m, z, None, trace_of(full[2]))
    finally:
        m.set_precision('bf16')
    return dict(full=full, half=half, plain=plain, forced=forced)


def explained(po, do, xh, pn, dn, what):
    """every decision equals the restated rule on the emitted logits, but for decisions inside the tolerance of the device's logarithm"""
    want_p = S.decide_pitch(po, pn, T_PITCH)
    skip_p = S.skippable(po, pn, T_PITCH, S.NOISE_TOL)
    want_d = S.decide_dur(do, dn, T_DUR)
    skip_d = S.skippable(do, dn, T_DUR, S.NOISE_TOL)
    bad_p = (xh[..., 0] != want_p) & ~skip_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d
    print('%s: pitch skipped %d of %d (mismatching inside the tolerance: %d), duration skipped %d of %d (%d)'
          % (what, skip_p.sum(), skip_p.size, ((xh[..., 0] != want_p) & skip_p).sum(), skip_d.sum(), skip_d.size,
             ((xh[..., 1:] != want_d) & skip_d).sum()))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert skip_p.mean() <= SKIP_CAP and skip_d.mean() <= SKIP_CAP


# ---------------------------------------------------------------------------------------------------------------------------------
def test_1_noise_equals_the_restatement():
    """ptv_debug_sample_noise (the decoder's own device functions) against sample_ref for B = 20, two (t, n), offsets 0 and 1000.  The device
    takes the two logarithms in fp32: |g_dev - g_ref| <= NOISE_TOL = 4 * the measured maximum (tests/sample_ref.py), itself below 1e-4"""
    worst = 0.0
    for off in (0, 1000):
        blk = block(off)
        for t, n in ((0, 0), (31, 14)):
            op = torch.empty(20, 130, device=DEV)
            od = torch.empty(20, 5, 2, device=DEV)
            call('ptv_debug_sample_noise', ptr(blk), 20, t, n, ptr(op), ptr(od), stream_ptr())
            torch.cuda.synchronize()
            g = np.arange(off, off + 20)
            dp = np.abs(op.cpu().numpy().astype(np.float64) - S.pitch_noise(SEED, DRAW, g, t, n)).max()
            dd = np.abs(od.cpu().numpy().astype(np.float64) - S.dur_noise(SEED, DRAW, g, t, n)).max()
            worst = max(worst, dp, dd)
    print('delta = max |g_dev - g_ref| = %.3e' % worst)
    assert S.NOISE_DELTA is not None and S.NOISE_DELTA <= 1e-4
    assert worst <= S.NOISE_TOL


@pytest.mark.parametrize('path', list(PATHS))
def test_2_every_decision_is_explained(path):
    """A sampled decode at T_pitch = 1.0, T_dur = 0.7: every pitch and duration decision in last_xhat / last_dur_idx is the restated rule
    applied to the emitted logits and sample_ref's noise; the same noise of global samples 16..31 explains the second half of the B = 32
    decode and the decode of z[16:32] at sample_offset = 16.
    A decision whose two best perturbed values are closer than T * NOISE_TOL + 4 ulp of the larger logit may go either way; at most 0.5 %
    of the pitch and 0.5 % of the duration decisions may be such.  The share computed on the CPU beforehand, with the restated rule and
    NOISE_TOL = 4e-6 on the logits of the reference's own decode (tests/golden/full_infer_b4.npz): 0 of its 9,600 duration decisions under
    this seed and draw, 1 of 480,000 under 50 other draws (2e-6); 3 of 300,000 pitch decisions (1e-5: three 130-wide rows of its sampled
    pitch logits under 100,000 sample indices each) -- of the order of the tolerance, 500 times below the cap.  On the card: 0 of 15,360
    pitch and 0 of 76,800 duration decisions skipped on every path."""
    r = runs(path)
    po, do, xh = r['full']
    pn, dn = noise(0, 32)
    explained(po, do, xh, pn, dn, path + ' B = 32')
    idx = model().decoder.last_dur_idx
    assert idx is not None
    po2, do2, xh2 = r['half']
    explained(po2, do2, xh2, pn[16:], dn[16:], path + ' z[16:32] at offset 16')
    explained(po[16:], do[16:], xh[16:], *noise(16, 32), path + ' second half')
    # the sample index is global: wherever both decodes computed the same logits up to a step, they took the same decisions there
    same_t0 = np.array_equal(po[16:, 0, 0], po2[:, 0, 0])
    if same_t0:
        assert np.array_equal(xh[16:, 0, 0, 0], xh2[:, 0, 0, 0])


def test_2b_last_dur_idx_holds_the_duration_decisions():
    m = model()
    decode(m, latents()[:20].contiguous(), block(0))
    B = 20
    idx = m.decoder.last_dur_idx.cpu().numpy().reshape(5, 15, 32, B)                      # [d, n, t, b]
    xh = m.decoder.last_xhat[:, :, 1:, 1:].cpu().numpy()                                  # [b, t, n, d]
    assert np.array_equal(idx.transpose(3, 2, 1, 0), xh)


@pytest.mark.parametrize('path', list(PATHS))
def test_3_the_sampled_trajectory_is_a_trajectory_of_the_model(path):
    """the sampled decisions forced through the argmax kernels (force_trace): the same logits and the same grid, bit for bit"""
    r = runs(path)
    for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
        assert np.array_equal(r['full'][k], r['forced'][k]), (path, name)
    assert (r['full'][2] != r['plain'][2]).any()                                          # ... and it is not the argmax trajectory


@pytest.mark.parametrize('path', [p for p in PATHS if p not in ('default', 'fp32', 'bf16-step-loop')])
def test_4_variants_agree(path):
    """two paths whose argmax decodes of the same z are bit-equal give bit-equal sampled decodes"""
    a, b = runs('default'), runs(path)
    for k in range(3):
        assert np.array_equal(a['plain'][k], b['plain'][k]), (path, 'the argmax decodes differ: nothing to compare', k)
    for k, name in enumerate(('pitch logits', 'duration logits', 'xhat')):
        assert np.array_equal(a['full'][k], b['full'][k]), (path, name)
        assert np.array_equal(a['half'][k], b['half'][k]), (path, name)


def test_4b_note_loop_kernels_agree_on_one_time_step():
    """ptv_free_note_loop itself, B = 20 (a full panel and a clamped partial one), sampling bit set: resident heads, streamed heads
    (bit 21), 2 / 4 / 8 members per panel and the 8-wave kernel give the same logits, decisions and tokens bit for bit, and the decisions
    are the restated rule"""
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
    blk = block(1000)
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
        # (cluster launches need every earlier time step's arrivals: t = 0 first would be the protocol; one step tagged t is self-consistent)
        io = FF_.note_loop_io(GC=GC, HN=HN, PITCH=pitch, DUR=dur, IDX=idx, TOK=TOK, PRED=PRED, XHAT=xhat, PLEN=plen, XCH=xch, CNT=cnt, BLOCK=blk)
        call('ptv_free_note_loop', wl, io, 136, B, t, 0, bits | FF_.SAMPLE_BIT, stream_ptr())
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
    explained(po.transpose(1, 0, 2), do.transpose(1, 0, 2).reshape(B, 15, 5, 2), xh, pn, dn, 'note loop, one time step')


def test_5_reproducibility():
    m = model()
    zc, zr = latents()[:16, :256].contiguous(), latents()[:16, 256:].contiguous()
    a = m.inference_decode(zc, zr, temperature=1.0, seed=3, draw=5)
    assert np.array_equal(a, m.inference_decode(zc, zr, temperature=1.0, seed=3, draw=5))
    assert (a != m.inference_decode(zc, zr, temperature=1.0, seed=3, draw=6)).any()
    assert (a != m.inference_decode(zc, zr, temperature=1.0, seed=4, draw=5)).any()
    first = m.inference_decode(zc, zr, temperature=1.0, seed=3)
    second = m.inference_decode(zc, zr, temperature=1.0, seed=3)
    assert (first != second).any()                                                        # draw=None: the model's counter advanced


def test_6_degenerate_cases(monkeypatch):
    m = model()
    z = latents()[:20].contiguous()
    zc, zr = z[:, :256].contiguous(), z[:, 256:].contiguous()
    plain = decode(m, z)
    zero = decode(m, z, block(0, 0.0, 0.0))
    for a, b in zip(plain, zero):
        assert np.array_equal(a, b)
    assert np.array_equal(m.inference_decode(zc, zr), m.inference_decode(zc, zr, temperature=0.0, dur_temperature=0.0))
    for a, b in zip(m.decode_to_inputs(zc, zr), m.decode_to_inputs(zc, zr, temperature=0, dur_temperature=0)):
        assert torch.equal(a, b)
    # temperature=None: DecoderStepFn receives what it received before -- no sampling block, so the present instantiations run
    seen = []
    orig = FF_.DecoderStepFn.apply

    def spy(*args):
        seen.append(args)
        return orig(*args)
    monkeypatch.setattr(FF_.DecoderStepFn, 'apply', staticmethod(spy))
    m.inference_decode(zc, zr)
    m.inference_decode(zc, zr, temperature=1.0, seed=3, draw=0)
    monkeypatch.undo()
    n_plain = 7 + len(FF_.FREE_PARAM_NAMES)
    assert len(seen) == 2 and len(seen[0]) == n_plain and len(seen[1]) == n_plain + 1
    assert not any(torch.is_tensor(a) and a.dtype == torch.int64 for a in seen[0])
    assert seen[1][-1].dtype == torch.int64 and seen[1][-1].numel() == 4
    # T_pitch = 1, T_dur = 0: the duration decisions are the plain argmax of their emitted logits
    po, do, xh = decode(m, z, block(0, 1.0, 0.0))
    assert np.array_equal(xh[..., 1:], (do[..., 1] > do[..., 0]).astype(np.int64))
    assert (xh[..., 0] != plain[2][..., 0]).any()


def test_7_graph_replay():
    m = model()
    zc, zr = latents()[:16, :256].contiguous(), latents()[:16, 256:].contiguous()
    eager = {d: m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, draw=d) for d in (5, 6)}
    assert (eager[5] != eager[6]).any()
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        for d in (5, 6, 5):
            assert np.array_equal(m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, draw=d), eager[d]), d
        assert m.decoder.graph_captures == before + 1
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_8_surface():
    m = model()
    B = 4
    zc, zr = latents()[:B, :256].contiguous(), latents()[:B, 256:].contiguous()
    kw = dict(temperature=1.0, seed=3, draw=0)
    est = m.inference_decode(zc, zr, **kw)
    pr_mat, x, c, notes, count, err = m.decode_to_inputs(zc, zr, **kw)
    # the same arguments decode the same grid ...
    assert np.array_equal(m.decoder.last_xhat[:, :, 1:].cpu().numpy(), est)
    # ... and decode_to_inputs' x is, as for the argmax decode, the CANONICAL grid of what was read from it (grid_to_pr_and_notes_batch's
    # x_clean: a step ends at its first <eos>, holds at most max_notes notes, the rest is <pad>) -- not the raw grid est_x
    pr2, notes2, count2, x2, err2 = m.decoder.grid_to_pr_and_notes_batch(torch.from_numpy(est).to(DEV))
    assert torch.equal(pr_mat, pr2) and torch.equal(count, count2) and torch.equal(x, x2) and torch.equal(err, err2)
    valid = torch.arange(notes.shape[1], device=DEV)[None, :] < count[:, None]              # (notes beyond count are not written)
    assert bool(valid.any()) and torch.equal(notes[valid], notes2[valid])
    plain = m.decode_to_inputs(zc, zr)
    assert not torch.equal(plain[1], x)                                                     # (it is not the argmax decode)
    xs, cs, prs = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, 5))
    m.use_philox(seed=7, sample_offset=0)
    a0 = m.posterior_sample(prs, cs)
    m.use_philox(seed=7, sample_offset=0)
    a1 = m.posterior_sample(prs, cs, temperature=1.0, draw=0)
    assert a0.shape == a1.shape and (a0 != a1).any()
    i0 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3)
    i1 = m.interp(prs[:2], cs[:2], prs[2:], cs[2:], interp_chd=True, int_count=3, temperature=1.0, draw=0)
    assert i0.shape == i1.shape == (2, 3, 32, 15, 6) and (i0 != i1).any()
    m._philox = None
    # training and sampling do not combine
    blk = block(0)
    with pytest.raises(ValueError):                         # (refused before x / lengths are looked at)
        m.decoder(torch.cat([zc, zr], -1).requires_grad_(True), False, None, None, 0.5, 0.5, sampling=blk)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1), False, None, None, 0., 0., sampling=blk)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1), True, None, None, 0., 0., sampling=torch.zeros(4, device=DEV))      # not a block
    # ... at the C level: the sampling bit with train & 3 != 0 is PTV_ERR_ARG before any launch (no pointer is followed)
    dummy = torch.zeros(64, device=DEV)
    wl = F_._parr([dummy] * 16)
    io = F_._parr([dummy] * 22)
    for train in (1, 2):
        assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, train | FF_.SAMPLE_BIT, stream_ptr()) == -1
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 1, FF_.SAMPLE_BIT, stream_ptr()) == -1            # a teacher-forcing coin
    io[21] = None
    assert lib().ptv_free_note_loop(wl, io, 136, 16, 0, 0, FF_.SAMPLE_BIT, stream_ptr()) == -1            # the bit without a block
