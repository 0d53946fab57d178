"""GPU: kept time steps in the free-running decode (keep=, DisentangleVAE.keep, ptv_keep_force_build; INTEGRATION.md "Kept steps") against
tests/keep_ref.py: the builder element for element, the kept steps coming out as given on every selectable note-loop path, the keep decode
a trajectory of the model, its free decisions the documented draw, the fixed point, causality and slicing, every note-loop kernel on one
time step, graph replay and the Python surface.  The paths, the model, the latents and the noise are those of
tests/test_gpu_truncated_sampling.py, the chord mask that of tests/test_gpu_constrained_decode.py."""
import functools

import numpy as np
import pytest
import torch

import constrain_ref as CR
import keep_ref as K
import sample_ref as S
import test_gpu_constrained_decode as CD
import test_gpu_truncated_sampling as TT
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
T_PITCH, T_DUR = TT.T_PITCH, TT.T_DUR
SKIP_CAP = 0.005
B = 32
CONS = dict(top_k=8, top_p=0.9, ascending=True)                    # + the chord mask: the setting of tests 3 and 4
BAD_ROWS = (1, 5, 6, 7)                                            # samples whose KEPT steps hold an unforcible pitch


def spliced_steps():
    """hand-made steps [16, 6] by name"""
    def blank():
        s = np.full((16, 6), 2, dtype=np.int64)
        s[:, 0] = 130
        s[0, 0] = 128
        return s
    out = {}
    s = blank(); s[1, 0] = 129; out['empty'] = s
    s = blank()
    for i in range(1, 15):
        s[i] = (38 + 3 * i, i & 1, 1, 0, (i >> 1) & 1, 1)
    s[15, 0] = 129
    out['14 notes'] = s
    s = blank()
    for i in range(1, 16):
        s[i] = (30 + 5 * i, 0, i & 1, 1, 0, (i >> 2) & 1)
    out['15 notes'] = s
    s = blank(); s[1] = (60, 0, 0, 1, 1, 0); s[3] = (67, 1, 0, 0, 0, 0); s[4, 0] = 129; out['pad before eos'] = s      # slot 2 stays <pad>
    s = blank(); s[1] = (131, 0, 1, 0, 1, 0); s[2] = (72, 0, 0, 0, 0, 1); s[3, 0] = 129; out['pitch 131'] = s
    s = blank(); s[1] = (50, 1, 1, 1, 1, 1); s[2] = (-1, 0, 0, 0, 1, 1); s[3, 0] = 129; out['pitch -1'] = s
    return out


@functools.lru_cache(maxsize=None)
def crafted():
    """(x int64 [32, 32, 16, 6], steps uint8 [32, 32], keep_ref.build of them): synth_batch(32, 5)'s grid with the hand-made steps spliced in
    -- all six into row 1 (which keeps everything), the unforcible ones also into kept steps of rows 5, 6, 7 and into a step row 4 does NOT keep;
    row 0 keeps nothing, row 2 only t = 0, row 3 only t = 31, the others (t + b) % 4 < 2"""
    x = synth_batch(B, 5)[0].copy()
    sp = spliced_steps()
    for t, name in enumerate(sp):
        x[1, t] = sp[name]
    x[2, 0] = sp['14 notes']
    x[3, 31] = sp['15 notes']
    x[5, 3] = sp['pitch 131']          # (3 + 5) % 4 = 0: kept
    x[6, 2] = sp['pitch -1']           # (2 + 6) % 4 = 0: kept
    x[7, 1] = sp['pad before eos']     # (1 + 7) % 4 = 0: kept
    x[4, 2] = sp['pitch 131']          # (2 + 4) % 4 = 2: not kept
    x[9, 3] = sp['empty']; x[9, 4] = sp['15 notes']; x[10, 2] = sp['14 notes']
    t_, b_ = np.meshgrid(np.arange(32), np.arange(B))
    steps = ((t_ + b_) % 4 < 2).astype(np.uint8)
    steps[0] = 0
    steps[1] = 1
    steps[2] = 0; steps[2, 0] = 1
    steps[3] = 0; steps[3, 31] = 1
    ref = K.build(x, steps)
    for a in (x, steps) + tuple(ref.values()):
        a.setflags(write=False)
    return x, steps, ref


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # (a copy: the cached arrays are read-only)


def keep_of(x, steps):
    kp = TT.model().keep(dev(x), dev(steps) if isinstance(steps, np.ndarray) else steps)
    torch.cuda.synchronize()
    return kp


def kdecode(m, z, block=None, keep=None):
    """one free-running decode with kept steps -> (pitch logits [B,32,15,130], duration logits [B,32,15,5,2], xhat [B,32,15,6]) as numpy"""
    with torch.no_grad():
        po, do = m.decoder(z, True, None, None, 0., 0., sampling=block, keep=keep)
    torch.cuda.synchronize()
    return po.contiguous().cpu().numpy(), do.contiguous().cpu().numpy(), m.decoder.last_xhat[:, :, 1:].cpu().numpy()


def cons_block(offset=0, rows=slice(None), **kw):
    return TT.block(offset, pitch_mask=CD.chord_mask()[0][rows].contiguous(), **CONS, **kw)


@functools.lru_cache(maxsize=None)
def runs(path):
    """the decodes of one path, run once: the crafted keep under argmax, plain sampling and the constrained truncated setting; the whole
    grid of the last one forced through the ARGMAX kernels with the all-forced force_trace"""
    attrs, prec = PATHS[path]
    x, steps, _ = crafted()
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    out = {}
    try:
        with TT.patched(attrs):
            kp = keep_of(x, steps)
            out['argmax'] = kdecode(m, z, None, kp)
            out['sampled'] = kdecode(m, z, TT.block(0), kp)
            out['cons'] = kdecode(m, z, cons_block(), kp)
            out['forced'] = TT.decode(m, z, None, TT.trace_of(out['cons'][2]))
    finally:
        m.set_precision('bf16')
    return out


def explained_free(po, do, xh, pn, dn, kw, mask_np, ref, what):
    """test_gpu_constrained_decode.explained restricted to the FREE decisions of a keep decode (keep_ref's maps): every free pitch decision
    is constrain_ref.decide_pitch on the emitted logits (lo runs over the forced pitches too), every free duration decision
    sample_ref.decide_dur; skipped: decisions sample_ref.skippable, at most SKIP_CAP of the free ones"""
    k, l, q = CD.rule(kw)
    al = CD.allowed_of(xh, kw, mask_np)
    want_p = CR.decide_pitch(po, pn, al, T_PITCH, k, l, q)
    skip_p = CR.skippable(po, pn, al, T_PITCH, k, l, q)
    want_d = S.decide_dur(do, dn, T_DUR)
    skip_d = S.skippable(do, dn, T_DUR, S.NOISE_TOL)
    free_p, free_d = ~ref['forced_pitch'], ~ref['forced_dur']
    bad_p = (xh[..., 0] != want_p) & ~skip_p & free_p
    bad_d = (xh[..., 1:] != want_d) & ~skip_d & free_d
    share_p, share_d = skip_p[free_p].mean(), skip_d[free_d].mean()
    print('%s: free pitch decisions %d of %d, skipped %d (share %.5f); free duration decisions %d of %d, skipped %d (share %.5f)'
          % (what, free_p.sum(), free_p.size, skip_p[free_p].sum(), share_p, free_d.sum(), free_d.size, skip_d[free_d].sum(), share_d))
    assert not bad_p.any(), (what, 'pitch', int(bad_p.sum()), np.argwhere(bad_p)[:4])
    assert not bad_d.any(), (what, 'duration', int(bad_d.sum()), np.argwhere(bad_d)[:4])
    assert share_p <= SKIP_CAP and share_d <= SKIP_CAP
    assert np.take_along_axis(al, xh[..., :1], -1)[..., 0][free_p].all()                   # a free decision is an allowed class


# ---------------------------------------------------------------------------------------------------------------------------------
def test_1_builder_matches_keep_ref():
    """ptv_keep_force_build on B = 3 rows of the crafted grid (everything kept with all six hand-made steps; the (t + b) % 4 pattern with
    pitch 131; only t = 0), [B, 32] and [1, 32] steps and a [B, 32] array of the bytes 0, 1, 2, 3, 4, 7 and 255: pitch, dur and err equal keep_ref in every element; bad arguments are PTV_ERR_ARG"""
    x, steps, _ = crafted()
    x3, s3 = np.ascontiguousarray(x[[1, 5, 2]]), np.ascontiguousarray(steps[[1, 5, 2]])
    other = np.array([0, 1, 2, 3, 4, 7, 255], dtype=np.uint8)     # any non-zero byte is a kept step here: err never gets bit 1
    other = other[(np.arange(32)[None, :] + np.arange(3)[:, None]) % 7]
    for st in (s3, np.ascontiguousarray(steps[5:6]), other):
        want = K.build(x3, st)
        assert not (want['err'] & 2).any()
        xd, sd = dev(x3), dev(st)
        pitch = torch.full((15, 96), 77, dtype=torch.int32, device=DEV)
        dur = torch.full((5, 1440), 77, dtype=torch.int32, device=DEV)
        err = torch.full((3,), 77, dtype=torch.int32, device=DEV)
        call('ptv_keep_force_build', ptr(xd), ptr(sd), st.shape[0], 3, ptr(pitch), ptr(dur), ptr(err), stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(pitch.cpu().numpy(), want['pitch'])
        assert np.array_equal(dur.cpu().numpy(), want['dur'])
        assert np.array_equal(err.cpu().numpy(), want['err'])
        assert want['err'].any() and (want['pitch'] >= 0).any() and (want['dur'] >= 0).any()
        kp = TT.model().keep(xd, sd)
        torch.cuda.synchronize()
        assert kp.batch == 3 and np.array_equal(kp.pitch.cpu().numpy(), want['pitch']) and np.array_equal(kp.dur.cpu().numpy(), want['dur'])
        assert np.array_equal(kp.err.cpu().numpy(), want['err'])
    st_ = stream_ptr()
    good = [ptr(xd), ptr(sd), 1, 3, ptr(pitch), ptr(dur), ptr(err)]
    for i, v in ((3, 0), (3, -2), (2, 2), (2, 0), (2, 4), (0, None), (1, None), (4, None), (5, None), (6, None)):
        args = list(good)
        args[i] = v
        assert lib().ptv_keep_force_build(*args, st_) == -1, (i, v)


@pytest.mark.parametrize('path', list(PATHS))
def test_2_kept_steps_come_out_as_given(path):
    """argmax, plain sampled and constrained keep decodes: where keep_ref says forced, the decoded grid equals x; the length of a kept step
    whose pitches are all forcible (first <eos> slot of the decoded step, 15 without one) is its L"""
    x, steps, ref = crafted()
    r = runs(path)
    whole = ref['forced_pitch'].sum(-1) == ref['L']                 # kept steps without an unforcible pitch (and every step not kept: 0 == 0)
    for name in ('argmax', 'sampled', 'cons'):
        xh = r[name][2]
        fp, fd = ref['forced_pitch'], ref['forced_dur']
        assert np.array_equal(xh[..., 0][fp], x[:, :, 1:, 0][fp]), (path, name)
        assert np.array_equal(xh[..., 1:][fd], x[:, :, 1:, 1:][fd]), (path, name)
        eos = xh[..., 0] == 129
        length = np.where(eos.any(-1), eos.argmax(-1) + 1, 15)
        sel = (steps != 0) & whole
        assert sel.sum() > 300 and np.array_equal(length[sel], ref['L'][sel]), (path, name)
    assert (r['sampled'][2] != r['argmax'][2]).any() and (r['cons'][2] != r['sampled'][2]).any()


@pytest.mark.parametrize('path', list(PATHS))
def test_3_the_keep_decode_is_a_trajectory_of_the_model(path):
    """the whole grid of the constrained sampled keep decode forced through the argmax kernels (all-forced force_trace): pitch and
    duration logits bit-equal -- the kept notes were fed back through the token and the re-summarisation exactly as decisions are"""
    r = runs(path)
    for a, b, what in zip(r['cons'], r['forced'], ('pitch logits', 'duration logits', 'grid')):
        assert np.array_equal(a, b), (path, what)


@pytest.mark.parametrize('path', list(PATHS))
def test_4_free_decisions_are_the_documented_draw(path):
    """the free decisions of the constrained and of the plain sampled keep decode are constrain_ref.decide_pitch / sample_ref.decide_dur on
    the emitted logits and the restated noise; the skipped share (printed) is at most 0.005 of the free decisions"""
    _, _, ref = crafted()
    r = runs(path)
    pn, dn = TT.noise(0, B)
    mask, mask_np = CD.chord_mask()
    po, do, xh = r['cons']
    explained_free(po, do, xh, pn, dn, dict(CONS, pitch_mask=mask), mask_np, ref, '%s constrained keep' % path)
    po, do, xh = r['sampled']
    explained_free(po, do, xh, pn, dn, {}, mask_np, ref, '%s sampled keep' % path)


@pytest.mark.parametrize('path', ('default', 'cluster4', 'split', 'bf16-step-loop'))
def test_5_fixed_point(path):
    """a keep built from a plain sampled decode's OWN grid, same seed and draw: logits and grid bit-equal to that decode everywhere"""
    attrs, prec = PATHS[path]
    _, steps, _ = crafted()
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    try:
        with TT.patched(attrs):
            a = TT.decode(m, z, TT.block(0))
            own = m.decoder.last_xhat.clone()                       # [B, 32, 16, 6], slot 0 = <sos>
            assert (own[:, :, 0, 0] == 128).all()
            kp = m.keep(own, dev(steps))
            b = kdecode(m, z, TT.block(0), kp)
            assert int(kp.err.sum()) == 0 and int((kp.pitch >= 0).sum()) > 1000
    finally:
        m.set_precision('bf16')
    for u, v, what in zip(a, b, ('pitch logits', 'duration logits', 'grid')):
        assert np.array_equal(u, v), (path, what)


def test_6_causality_and_slicing():
    """two keeps that differ only at steps >= 12 decode bit-equal for t < 12; z[16:] with a keep of x[16:] at sample_offset 16 equals rows
    16.. of the whole decode"""
    x, steps, _ = crafted()
    m = TT.model()
    z = TT.latents()
    x2, s2 = x.copy(), steps.copy()
    x2[:, 12:] = synth_batch(B, 9)[0][:, 12:]
    s2[:, 12:] = 1 - steps[:, 12:]
    a = kdecode(m, z, cons_block(), keep_of(x, steps))
    b = kdecode(m, z, cons_block(), keep_of(x2, s2))
    assert (a[2][:, 12:] != b[2][:, 12:]).any()
    for u, v in zip(a, b):
        assert np.array_equal(u[:, :12], v[:, :12])
    h = kdecode(m, z[16:].contiguous(), cons_block(16, slice(16, None)), keep_of(x[16:], steps[16:]))
    for u, v in zip(a, h):
        assert np.array_equal(u[16:], v)


def test_7_note_loop_kernels_agree_on_one_time_step():
    """ptv_free_note_loop itself, B = 20 (a full panel and a clamped partial one), sampling + truncation, force arrays mixing forced and
    free rows and bits: resident heads, streamed heads (bit 21), 2 / 4 / 8 members per panel and the 8-wave kernel bit-equal, the forced
    entries come out as given, and all-negative arrays are bit-equal to NULL pointers"""
    d_ = torch.device(DEV)
    m = TT.model()
    P = dict(m.decoder.named_parameters())
    Bn = 20
    R, Mr = 32 * Bn, 15 * 32 * Bn
    panels = (Bn + 15) // 16
    pk = FF_._free_packs(P, 1024)
    with torch.no_grad():
        tab0, tab = FF_.dur_tabs(P, d_)
    wl = FF_.note_loop_weights(P, pk, tab0, tab)
    g = torch.Generator(device=d_).manual_seed(5)
    GC = torch.randn(Bn, 1536, device=d_, generator=g) * 0.6
    HN0 = torch.randn(R, 512, device=d_, generator=g) * 0.5
    TOK0 = torch.randn(R, 128, device=d_, generator=g) * 0.5
    blk = TT.block(1000, top_k=8, min_p=0.97)
    t = 3
    rng = np.random.default_rng(3)
    fp = np.where(rng.random((15, R)) < 0.5, rng.integers(0, 130, (15, R)), -1).astype(np.int32)
    fd = np.where(rng.random((5, Mr)) < 0.5, rng.integers(0, 2, (5, Mr)), -1).astype(np.int32)
    fp[:, t * Bn + 2] = -1; fd.reshape(5, 15, R)[:, :, t * Bn + 2] = -1                     # a row all free
    fp[:, t * Bn + 17] = 60; fd.reshape(5, 15, R)[:, :, t * Bn + 17] = 1                    # a row all forced, in the partial panel
    forces = {'mixed': (dev(fp), dev(fd)), 'none': (None, None),
              'negative': (torch.full((15, R), -1, dtype=torch.int32, device=d_), torch.full((5, Mr), -5, dtype=torch.int32, device=d_)),
              'pitch only': (dev(fp), None)}
    res = {}
    for name, bits in (('resident', 0x10000), ('streamed', 0x10000 | 0x200000), ('two', 0x10000 | (2 << 18)), ('four', 0x10000 | (4 << 18)),
                       ('eight', 0x10000 | 0x400000), ('8-wave', 0x20000)):
        for fname, (fpd, fdd) in forces.items():
            HN = torch.zeros(16, R, 512, device=d_); HN[0] = HN0
            pitch = torch.zeros(Mr, 136, device=d_)
            dur = torch.zeros(Mr, 10, device=d_)
            idx = torch.zeros(5, Mr, device=d_, dtype=torch.int32)
            TOK = torch.zeros(15, R, 128, device=d_); TOK[0] = TOK0
            PRED = torch.zeros(16, R, 128, device=d_)
            xhat = torch.zeros(Bn, 32, 16, 6, device=d_, dtype=torch.long)
            plen = torch.zeros(R, device=d_, dtype=torch.int32)
            clustered = name in ('two', 'four', 'eight')
            xch = torch.zeros(panels * 2 * 16 * 512 * 2, device=d_, dtype=torch.bfloat16) if clustered else None
            cnt = torch.zeros(panels + 1, device=d_, dtype=torch.int32) if clustered else None
            io = FF_.note_loop_io(GC=GC, HN=HN, PITCH=pitch, DUR=dur, IDX=idx, TOK=TOK, PRED=PRED, XHAT=xhat, PLEN=plen, FORCE_PITCH=fpd,
                                  FORCE_DUR=fdd, XCH=xch, CNT=cnt, BLOCK=blk)
            call('ptv_free_note_loop', wl, io, 136, Bn, t, 0, bits | FF_.SAMPLE_BIT | FF_.TRUNC_BIT, stream_ptr())
            torch.cuda.synchronize()
            if clustered:
                assert int(cnt[-1]) == 0
            rows = slice(t * Bn, (t + 1) * Bn)
            res[name, fname] = (pitch.view(15, R, 136)[:, rows, :130].cpu().numpy(), dur.view(15, R, 10)[:, rows].cpu().numpy(),
                                xhat[:, t, 1:].cpu().numpy(), PRED[:, rows].cpu().numpy(), idx.view(5, 15, R)[:, :, rows].cpu().numpy(),
                                plen[rows].cpu().numpy())
    for (name, fname), got in res.items():
        for a_, b_, what in zip(res['resident', fname], got, ('pitch', 'dur', 'xhat', 'PRED', 'idx', 'plen')):
            assert np.array_equal(a_, b_), (name, fname, what)
        for a_, b_, what in zip(res[name, 'none'], res[name, 'negative'], ('pitch', 'dur', 'xhat', 'PRED', 'idx', 'plen')):
            assert np.array_equal(a_, b_), (name, 'all-negative arrays against NULL pointers', what)
    xh = res['resident', 'mixed'][2]                                                        # [B, 15, 6]
    fpt = fp[:, t * Bn:(t + 1) * Bn].T                                                      # [B, 15]
    fdt = fd.reshape(5, 15, R)[:, :, t * Bn:(t + 1) * Bn].transpose(2, 1, 0)                # [B, 15, 5]
    assert np.array_equal(xh[..., 0][fpt >= 0], fpt[fpt >= 0]) and np.array_equal(xh[..., 1:][fdt >= 0], fdt[fdt >= 0])
    free = res['resident', 'none'][2]
    assert np.array_equal(xh[2], free[2])                                                   # the all-free row of the first note step's inputs ...
    assert (xh[..., 0][fpt < 0] != free[..., 0][fpt < 0]).any()                             # ... while forced notes changed what follows them
    assert np.array_equal(res['resident', 'pitch only'][2][..., 0][fpt >= 0], fpt[fpt >= 0])


def test_8_graph_replay():
    """replay equals eager; three different keeps and two draws are served by ONE capture; a decode without a keep afterwards is replayed
    from a graph of its own"""
    x, steps, _ = crafted()
    m = TT.model()
    zc, zr = TT.latents()[:16, :256].contiguous(), TT.latents()[:16, 256:].contiguous()
    keeps = [keep_of(x[:16], steps[:16]), keep_of(x[16:], steps[16:]), m.keep(dev(x[:16]), range(16))]
    sets = [dict(keep=keeps[0], draw=5), dict(keep=keeps[1], draw=6), dict(keep=keeps[2], draw=5), dict(keep=keeps[0], draw=6)]
    kw = dict(temperature=1.0, dur_temperature=0.7, seed=9)
    eager = [m.inference_decode(zc, zr, **kw, **s) for s in sets]
    plain = m.inference_decode(zc, zr, **kw, draw=5)
    assert all((eager[i] != eager[j]).any() for i in range(4) for j in range(i))
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        for i in (0, 1, 2, 3, 0, 2):
            assert np.array_equal(m.inference_decode(zc, zr, **kw, **sets[i]), eager[i]), i
        assert m.decoder.graph_captures == before + 1
        assert np.array_equal(m.inference_decode(zc, zr, **kw, draw=5), plain)
        assert m.decoder.graph_captures == before + 2
        assert np.array_equal(m.inference_decode(zc, zr, **kw, **sets[1]), eager[1])
        assert np.array_equal(m.inference_decode(zc, zr, **kw, draw=5), plain)
        assert m.decoder.graph_captures == before + 2
        assert sorted(len(k) for k in m.decoder._graphs) == [5, 6]                          # the key without a keep is what it was
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_9_surface():
    x, steps, ref = crafted()
    m = TT.model()
    Bs = 4
    zc, zr = TT.latents()[:Bs, :256].contiguous(), TT.latents()[:Bs, 256:].contiguous()
    _, c_np, pr_np = synth_batch(Bs, 5)
    c, pr = dev(c_np), dev(pr_np)
    xd = dev(x[:Bs])
    good = m.keep(xd, dev(steps[:Bs]))
    other = m.keep(dev(x[:8]), range(4))
    # ---- DisentangleVAE.keep
    for bad_x in (xd.cpu(), xd.int(), xd[:, :, :15], xd[0]):
        with pytest.raises(ValueError):
            m.keep(bad_x, range(4))
    for bad_s in (dev(steps[:Bs]).cpu(), dev(steps[:3]), dev(steps[:Bs, :31]), dev(steps[:Bs]).int(), dev(steps[0]), [32], [-1], [0.5], 7):
        with pytest.raises(ValueError):
            m.keep(xd, bad_s)
    assert m.keep(xd, slice(0, 16)).pitch.shape == (15, 32 * Bs) and m.keep(xd, dev(steps[:1]).bool()).batch == Bs
    # ---- the keyword: a wrong batch, not a Keep, together with force_trace -- before anything is encoded or launched
    draws = m._sample_draws
    trace = TT.trace_of(np.zeros((Bs, 32, 15, 6), dtype=np.int64))
    for bad, ft in ((other, None), ({'pitch': good.pitch, 'dur': good.dur}, None), (good, trace)):
        m.decoder.force_trace = ft
        try:
            for fn in (lambda: m.inference_decode(zc, zr, temperature=1.0, keep=bad),
                       lambda: m.decode_to_inputs(zc, zr, temperature=1.0, keep=bad),
                       lambda: m.swap(pr, pr, c, c, True, True, temperature=1.0, keep=bad),
                       lambda: m.inference_decode(zc, zr, keep=bad)):
                with pytest.raises(ValueError):
                    fn()
        finally:
            m.decoder.force_trace = None
    assert m._sample_draws == draws
    with pytest.raises(ValueError):                                                        # inference only, one level down
        m.decoder(torch.cat([zc, zr], -1), False, None, None, 0., 0., keep=good)
    with pytest.raises(ValueError):
        m.decoder(torch.cat([zc, zr], -1), True, None, None, 0., 0., keep=other)
    # ---- without a temperature: the argmax decode with kept steps, the draw counter stays
    est = m.inference_decode(zc, zr, keep=good)
    assert m._sample_draws == draws
    fp = ref['forced_pitch'][:Bs]
    assert np.array_equal(est[..., 0][fp], x[:Bs, :, 1:, 0][fp])
    assert np.array_equal(m.swap(pr, pr, c, c, True, True, keep=good)[..., 0][fp], x[:Bs, :, 1:, 0][fp])
    # ---- chained on the device: decode -> keep the first bar -> decode again
    pr0, x0, _, _, _, _ = m.decode_to_inputs(zc, zr, temperature=1.0, dur_temperature=0.7, seed=3, draw=1)
    kp = m.keep(x0, range(16))
    pr1, x1, _, _, _, _ = m.decode_to_inputs(zc, zr, temperature=1.0, dur_temperature=0.7, seed=3, draw=2, keep=kp)
    torch.cuda.synchronize()
    assert int(kp.err.sum()) == 0
    assert torch.equal(pr1[:, :16], pr0[:, :16]) and not torch.equal(pr1[:, 16:], pr0[:, 16:])
    # ---- err reports the crafted bad pitches and nothing else
    err = keep_of(x, steps).err.cpu().numpy()
    assert np.array_equal(err, ref['err']) and sorted(np.nonzero(err)[0]) == list(BAD_ROWS)
