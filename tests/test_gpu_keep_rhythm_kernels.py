"""GPU: the kernels of the kept rhythm (include/ptvae_hip.h "Kept rhythm") against tests/rhythm_ref.py: ptv_keep_rhythm_force_build element
for element at B = 1, 3 and 67; the allowed rule with PTV_FORCE_NOT_EOS words through ptv_debug_pitch_constrain_words in both lane layouts;
every selectable kernel of ptv_free_note_loop on one time step with force arrays that mix forced, free and -2 words;
ptv_note_token_sample_cons with -2 words; ptv_decode_logprob with -2 words against the fp64 restatement."""
import functools

import numpy as np
import pytest
import torch

import constrain_ref as CR
import kernel_ops as KO
import logprob_ref as LR
import nucleus_ref as NR
import rhythm_ref as RR
import sample_ref as S
import test_gpu_constrained_decode as CD
import test_gpu_decode_logprob_kernels as LK
import test_gpu_keep_decode as KD
import test_gpu_keep_voice_kernels as VK
import test_gpu_truncated_sampling as TT
import trunc_ref as TR
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = KD.DEV
SENT = -77                                                         # no kernel writes it: force words are >= -2, counts and bits >= 0
ORDER = [1, 5, 6, 7, 4, 2, 3, 9, 10, 0, 8] + list(range(11, 32))   # row 1 of the crafted grid holds its six hand-made steps
EOS = 129


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(B):
    """(x [B, 32, 16, 6], mode uint8 [B, 32] of 0 / 1 / 3 and the illegal 2 / 7): test_gpu_keep_decode's crafted grid tiled, its first row with
    two more hand-made steps: t = 6 holds an <sos> before its <eos>, t = 7 notes whose duration words are 2; the hand-made steps of the
    first row -- the empty step, 14 and 15 notes, <pad> / 131 / -1 before the <eos> among them -- are rhythm steps"""
    x = np.ascontiguousarray(KD.crafted()[0][[ORDER[i % 32] for i in range(B)]])
    s = np.full((16, 6), 2, dtype=np.int64)
    s[:, 0] = 130
    s[0, 0] = 128
    s[1] = (40, 0, 1, 0, 1, 0); s[2, 0] = 128; s[3] = (77, 1, 1, 0, 0, 0); s[4, 0] = EOS
    x[0, 6] = s
    s = s.copy()
    s[1] = (40, 2, 1, 2, 1, 0); s[2] = (52, 0, 2, 2, 2, 2); s[3] = (77, 1, 1, 0, 0, 2); s[4, 0] = EOS
    x[0, 7] = s
    rng = np.random.default_rng(200 + B)
    mode = rng.choice(np.array([0, 1, 3, 2, 7], dtype=np.uint8), size=(B, 32), p=[0.2, 0.25, 0.45, 0.05, 0.05])
    mode[0, :8] = 3
    mode[0, 8] = 7                                                 # one illegal byte whatever the draw
    for a in (x, mode):
        a.setflags(write=False)
    return x, mode


def gpu_build(x, mode, flags):
    B = x.shape[0]
    xd, md = dev(x), dev(mode)
    out = dict(pitch=torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV),
               dur=torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV),
               kept_n=torch.full((B, 32), SENT, dtype=torch.int32, device=DEV), err=torch.full((B,), SENT, dtype=torch.int32, device=DEV))
    call('ptv_keep_rhythm_force_build', ptr(xd), ptr(md), mode.shape[0], flags, B, ptr(out['pitch']), ptr(out['dur']), ptr(out['kept_n']),
         ptr(out['err']), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('B', (1, 3, 67))
def test_1_builder_matches_the_reference(B):
    """B rows and one row of mode bytes, both flag values: the four arrays equal rhythm_ref in every element (the sentinel is gone
    everywhere); rests, 15-note steps, unforcible pitches, both err bits and whole steps took part"""
    x, mode = inputs(B)
    seen = np.zeros(6, dtype=np.int64)
    for m in (mode, np.ascontiguousarray(mode[:1])):
        for flags in (0, 1):
            want = RR.build(x, m, durations=not flags)
            got = gpu_build(x, m, flags)
            for k in ('pitch', 'dur', 'kept_n', 'err'):
                assert np.array_equal(got[k], want[k]), (B, m.shape[0], flags, k, np.argwhere(got[k] != want[k])[:4])
        seen += [(want['K'] == 0).sum(), (want['K'] == 15).sum(), (want['err'] & 1).sum(), (want['err'] & 2).sum(), (m == 1).sum(),
                 (want['pitch'] == -2).sum()]
    assert seen.all(), seen
    if B == 3:                                                     # the same grid under every byte: 2 and 4 are the siblings' legal ones
        every = VK.sibling_bytes(B)
        for m in (every, np.ascontiguousarray(every[:1])):
            for flags in (0, 1):
                want = RR.build(x, m, durations=not flags)
                got = gpu_build(x, m, flags)
                for k in ('pitch', 'dur', 'kept_n', 'err'):
                    assert np.array_equal(got[k], want[k]), (m.shape[0], flags, k, np.argwhere(got[k] != want[k])[:4])
                VK.assert_foreign_free(got, m, (2, 4), B)
            assert (want['err'] & 2).all() and (want['pitch'] == -2).any()
    if B > 1:
        first = RR.build(x, mode)
        assert first['err'][0] == 3
        col = first['pitch'][:, 6 * B]
        assert list(col[:5]) == [-2, -2, -2, EOS, -1]              # the <sos> before the <eos> is a note position
        d = first['dur'].reshape(5, 15, 32 * B)[:, :, 7 * B]
        assert list(d[:, 0]) == [-1, 1, -1, 1, 0] and list(d[:, 1]) == [0, -1, -1, -1, -1] and (d[:, 3:] == -1).all()


def test_2_whole_and_free_steps_are_ptv_keep_force_build():
    """a call whose mode bytes are 0 / 1 only is bit-equal to ptv_keep_force_build on the same selection in all three arrays, whatever the
    flag, and kept_n counts its forced pitch words"""
    for B in (3, 67):
        x, mode = inputs(B)
        for steps in ((mode == 1).astype(np.uint8), np.ascontiguousarray((mode[:1] == 3).astype(np.uint8))):
            xd, sd = dev(x), dev(steps)
            pitch = torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV)
            dur = torch.full((5, 480 * B), SENT, dtype=torch.int32, device=DEV)
            err = torch.full((B,), SENT, dtype=torch.int32, device=DEV)
            call('ptv_keep_force_build', ptr(xd), ptr(sd), steps.shape[0], B, ptr(pitch), ptr(dur), ptr(err), stream_ptr())
            torch.cuda.synchronize()
            for flags in (0, 1):
                got = gpu_build(x, steps, flags)
                assert np.array_equal(got['pitch'], pitch.cpu().numpy()) and np.array_equal(got['dur'], dur.cpu().numpy())
                assert np.array_equal(got['err'], err.cpu().numpy())
                assert np.array_equal(got['kept_n'], (got['pitch'] >= 0).sum(0).reshape(32, B).T)
            assert (pitch >= 0).any() and (dur >= 0).any()
    assert int(err.sum()) > 0


def test_3_bad_arguments():
    """PTV_ERR_ARG before any launch: a NULL pointer, B < 1, a row count outside {1, B}, flags outside 0..1 -- and nothing is written"""
    B = 3
    x, mode = inputs(B)
    xd, md = dev(x), dev(mode)
    i32 = lambda *s: torch.full(s, SENT, dtype=torch.int32, device=DEV)
    outs = [i32(15, 32 * B), i32(5, 480 * B), i32(B, 32), i32(B)]
    st = stream_ptr()
    good = [ptr(xd), ptr(md), B, 0, B] + [ptr(o) for o in outs]
    fn = lib().ptv_keep_rhythm_force_build
    for i, v in ((0, None), (1, None), (2, 2), (2, 0), (2, 4), (3, 2), (3, -1), (3, 3), (4, 0), (4, -3), (5, None), (6, None), (7, None),
                 (8, None)):
        args = list(good)
        args[i] = v
        assert fn(*args, st) == -1, (i, v)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs)
    assert fn(*good, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), RR.build(x, mode)['pitch'])


# ================================================================================================ the allowed rule
ROWS = 37                                                          # 16 lanes per row: a partial wave in layout 0; a wave per row in layout 1


@functools.lru_cache(maxsize=None)
def rule_rows():
    """37 of test_gpu_constrained_decode's crafted rows (21 of the mask x lo deal, empty masks among them, then the 16 whose best logit the mask
    forbids or whose allowed values are all equal), <eos> made the maximum of every fourth row; words -2 / -1 / 5 in turn"""
    a, masks, lo = CD.crafted(2)
    pick = list(range(21)) + list(range(48, 64))
    a, masks, lo = a[pick].copy(), masks[pick].copy(), lo[pick].copy()
    a[::4, EOS] = a[::4].max(-1) + np.float32(1.0)
    words = np.array([(-2, -1, 5)[r % 3] for r in range(ROWS)], dtype=np.int32)
    words[-1] = -2
    for v in (a, masks, lo, words):
        v.setflags(write=False)
    return a, masks, lo, words


def constrain_words(blk, a, masks, lo, words, layout):
    keep = torch.full((ROWS, 130), 7, device=DEV, dtype=torch.uint8)
    thr = torch.full((ROWS,), 123.0, device=DEV)
    if words is None:
        call('ptv_debug_pitch_constrain', ptr(blk), ptr(a), ptr(masks), ptr(lo), ROWS, layout, ptr(keep), ptr(thr), stream_ptr())
    else:
        call('ptv_debug_pitch_constrain_words', ptr(blk), ptr(a), ptr(masks), ptr(lo), ptr(words), ROWS, layout, ptr(keep), ptr(thr),
             stream_ptr())
    torch.cuda.synchronize()
    return keep.cpu().numpy(), thr.cpu().numpy()


def test_4_allowed_rule_with_words():
    """ptv_debug_pitch_constrain_words on 37 rows in both layouts, ascending off / on, no rule / top_k 1 / top_k 8 / top_p 0.9 / min_p 0.5 at
    T = 0.7, held to rhythm_ref as test_gpu_constrained_decode holds the entry without words to constrain_ref: layouts bit-equal; the keep map
    equal outside the classes of the nucleus / min_p bands, the threshold bit-equal on rows without a band class; never empty; <eos> kept
    on a -2 row iff the reference says fallback.  With every word -1 the bytes of the entry without words"""
    T = 0.7
    a, masks, lo, words = rule_rows()
    da, dm, dlo, dw = dev(a), dev(masks), dev(lo), dev(words)
    free = dev(np.full(ROWS, -1, dtype=np.int32))
    n_fall = n_eos_best = 0
    for asc in (False, True):
        al0 = CR.allowed(masks, lo, asc)
        al = RR.allowed(al0, words)
        fall = RR.fallback(al0, words)
        n_fall += int(fall.sum())
        n_eos_best += int(((CR.constrained(a, al0).argmax(-1) == EOS) & (words == -2) & ~fall).sum())
        assert np.array_equal(al[words != -2], al0[words != -2]) and al.any(-1).all()
        con = CR.constrained(a, al)
        for kw in (dict(), dict(top_k=1), dict(top_k=8), dict(top_p=0.9), dict(min_p=0.5)):
            blk = FF_.sampling_block(DEV, T, ascending=asc, **kw)
            got = [constrain_words(blk, da, dm, dlo, dw, layout) for layout in (0, 1)]
            what = (asc, kw)
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), what
            k, l, q = CD.rule(kw)
            want = RR.keep_mask(a, al0, words, T, k, l, q)
            want_thr = RR.threshold(a, al0, words, T, k, l, q)
            band = (NR.band_classes(con, T, q) | TR.band_classes(con, T, l)) & al
            clean = ~band.any(-1)
            mask = got[0][0]
            assert set(np.unique(mask)) <= {0, 1}
            mask = mask.astype(bool)
            assert not (mask & ~al).any(), what
            assert np.array_equal(mask[~band], want[~band]), (what, np.argwhere((mask != want) & ~band)[:4])
            assert np.array_equal(got[0][1][clean].view(np.uint32), want_thr[clean].view(np.uint32)), what
            assert mask.any(-1).all() and mask[np.arange(ROWS), con.argmax(-1)].all(), what
            assert np.array_equal(mask[words == -2][:, EOS], fall[words == -2]), what
            for layout in (0, 1):
                old = constrain_words(blk, da, dm, dlo, None, layout)
                new = constrain_words(blk, da, dm, dlo, free, layout)
                assert old[0].tobytes() == new[0].tobytes() and old[1].tobytes() == new[1].tobytes(), what
    assert n_fall >= 2 and n_eos_best >= 2, (n_fall, n_eos_best)
    st = stream_ptr()
    keep, thr = torch.zeros(ROWS, 130, dtype=torch.uint8, device=DEV), torch.zeros(ROWS, device=DEV)
    assert lib().ptv_debug_pitch_constrain_words(ptr(blk), ptr(da), ptr(dm), ptr(dlo), None, ROWS, 0, ptr(keep), ptr(thr), st) == -1


# ================================================================================================ ptv_free_note_loop
def test_5_note_loop_kernels_agree_on_one_time_step():
    """ptv_free_note_loop itself, B = 20 (a full panel and a clamped partial one), the 64-byte block with sampling + top_k = 8 + top_p = 0.9
    + a random mask + `ascending`, force arrays mixing forced, free and -2 words (row 19's differ from row 3's, row 5 is all -2): resident
    heads, streamed heads (bit 21), 2 / 4 / 8 members per panel and the 8-wave kernel give the same logits, decisions and tokens bit for
    bit, and the decisions are rhythm_ref's on the emitted logits -- the fallback among them"""
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
    rng = np.random.default_rng(12)
    bits = rng.random((Bn, 32, 128)) < 0.4
    bits[7, 3] = False
    bits[7, 3, [30, 40, 50, 60, 70]] = True                        # row 7 has five pitches for its fifteen -2 words: the fallback
    mask_np = CR.mask_from_bits(bits)
    kw = dict(ascending=True, top_k=8, top_p=0.9)
    blk = TT.block(1000, pitch_mask=dev(mask_np), **kw)
    assert blk.numel() == 8
    t = 3
    u = rng.random((15, R))
    fp = np.where(u < 0.2, rng.integers(0, 130, (15, R)), np.where(u < 0.7, -2, -1)).astype(np.int32)
    fd = np.where(rng.random((5, Mr)) < 0.5, rng.integers(0, 2, (5, Mr)), -1).astype(np.int32)
    fp[:, t * Bn + 5] = -2
    fp[:, t * Bn + 7] = -2
    fp[:, t * Bn + 2] = -1
    fp[:, t * Bn + 19] = np.where(fp[:, t * Bn + 3] == -2, -1, -2)
    res = {}
    for name, bits in (('resident', 0x10000), ('streamed', 0x10000 | 0x200000), ('two', 0x10000 | (2 << 18)), ('four', 0x10000 | (4 << 18)),
                       ('eight', 0x10000 | 0x400000), ('8-wave', 0x20000)):
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
        io = FF_.note_loop_io(GC=GC, HN=HN, PITCH=pitch, DUR=dur, IDX=idx, TOK=TOK, PRED=PRED, XHAT=xhat, PLEN=plen, FORCE_PITCH=dev(fp),
                              FORCE_DUR=dev(fd), XCH=xch, CNT=cnt, BLOCK=blk)
        call('ptv_free_note_loop', wl, io, 136, Bn, t, 0, bits | FF_.SAMPLE_BIT | FF_.TRUNC_BIT | FF_.CONS_BIT, stream_ptr())
        torch.cuda.synchronize()
        if clustered:
            assert int(cnt[-1]) == 0
        rows = slice(t * Bn, (t + 1) * Bn)
        res[name] = (pitch.view(15, R, 136)[:, rows, :130].cpu().numpy(), dur.view(15, R, 10)[:, rows].cpu().numpy(),
                     xhat[:, t, 1:].cpu().numpy(), PRED[:, rows].cpu().numpy(), idx.view(5, 15, R)[:, :, rows].cpu().numpy(),
                     plen[rows].cpu().numpy())
    for name, got in res.items():
        for a_, b_, what in zip(res['resident'], got, ('pitch', 'dur', 'xhat', 'PRED', 'idx', 'plen')):
            assert np.array_equal(a_, b_), (name, what)
    po, _, xh = res['resident'][:3]
    po = po.transpose(1, 0, 2)                                     # [Bn, 15, 130]
    words = fp[:, t * Bn:(t + 1) * Bn].T                           # [Bn, 15]
    fdt = fd.reshape(5, 15, R)[:, :, t * Bn:(t + 1) * Bn].transpose(2, 1, 0)
    gi = np.arange(1000, 1000 + Bn).reshape(Bn, 1)
    pn = S.pitch_noise(TT.SEED, TT.DRAW, gi, t, np.arange(15).reshape(1, 15))
    al0 = CR.allowed(np.broadcast_to(mask_np[:, t][:, None, :], (Bn, 15, 4)), CR.running_lo(xh[..., 0]), True)
    k, l, q = CD.rule(kw)
    want = RR.decide_pitch(po, pn, al0, words, TT.T_PITCH, k, l, q)
    skip = RR.skippable(po, pn, al0, words, TT.T_PITCH, k, l, q) & (words < 0)
    fall = RR.fallback(al0, words)
    assert not ((xh[..., 0] != want) & ~skip).any(), np.argwhere((xh[..., 0] != want) & ~skip)[:4]
    assert skip[words < 0].mean() <= KD.SKIP_CAP
    assert np.array_equal(xh[..., 0][words >= 0], words[words >= 0]) and np.array_equal(xh[..., 1:][fdt >= 0], fdt[fdt >= 0])
    ne = words == -2
    assert ne.sum() > 100 and fall.sum() >= 1 and (xh[..., 0][fall] == EOS).all() and (xh[..., 0][ne & ~fall] != EOS).all()
    assert np.take_along_axis(RR.allowed(al0, words), xh[..., :1], -1)[..., 0][words < 0].all()
    assert (xh[..., 0][words == -1] == EOS).any()                  # a plainly free decision may still end its step


# ================================================================================================ ptv_note_token_sample_cons
@pytest.mark.parametrize('M', (5, 67))
@pytest.mark.parametrize('n', (1, 4))
def test_6_note_token_with_words(M, n):
    """the step loop's token kernel under mask + `ascending` + top_k = 8, words -2 / -1 / forced in turn, slots 1 .. n - 1 of the grid
    filled: the decision is rhythm_ref's on the same logits; rows whose mask and lo leave no pitch fall back to <eos>"""
    rng = np.random.default_rng(31 * M + n)
    t, E = 5, 128
    logits = (rng.standard_normal((M, 130)) * 2).astype(np.float32)
    logits[::3, EOS] = 9.0                                         # <eos> the maximum of every third row
    bits = rng.random((M, 32, 128)) < 0.3
    bits[3::5] = False                                             # rows whose mask allows no pitch: the fallback (rows 3, 23, 43, 63 hold -2)
    mask_np = CR.mask_from_bits(bits)
    grid = np.full((M, 32, 16, 6), 2, dtype=np.int64)
    grid[..., 0] = 130
    grid[:, :, 0, 0] = 128
    before = np.sort(rng.integers(20, 100, (M, 3)), -1)
    grid[:, t, 1:n, 0] = before[:, :n - 1]
    grid[2::7, t, 1:n, 0] = 127                                    # (n > 1) lo = 127: nothing above it
    words = np.array([(-2, -1, 64, -2)[r % 4] for r in range(M)], dtype=np.int32)
    kw = dict(ascending=True, top_k=8)
    blk = TT.block(300, pitch_mask=dev(mask_np), **kw)
    W = (rng.standard_normal((E, 135)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(E) * 0.3).astype(np.float32)
    dbits = rng.integers(0, 2, (5, M)).astype(np.int32)
    pbuf = np.zeros((M, 136), dtype=np.float32)
    pbuf[:, :130] = logits
    xd = dev(grid)
    pred = torch.zeros(M, E, device=DEV)
    plen = torch.zeros(M, dtype=torch.int32, device=DEV)
    KO.leaf('ptv_note_token_sample_cons', dev(pbuf), 136, dev(dbits), M, dev(W), dev(bias), E, pred, E, xd[0, t, n], 3072, plen, n, 0,
            dev(words), M, blk, t)
    torch.cuda.synchronize()
    out = xd.cpu().numpy()
    lo = CR.running_lo(out[:, t, 1:, 0])[:, n - 1]
    al0 = CR.allowed(mask_np[:, t], lo, True)
    pn = S.pitch_noise(TT.SEED, TT.DRAW, np.arange(300, 300 + M), t, n - 1)
    k, l, q = CD.rule(kw)
    want = RR.decide_pitch(logits, pn, al0, words, TT.T_PITCH, k, l, q)
    skip = RR.skippable(logits, pn, al0, words, TT.T_PITCH, k, l, q) & (words < 0)
    fall = RR.fallback(al0, words)
    got = out[:, t, n, 0]
    assert not ((got != want) & ~skip).any(), np.argwhere((got != want) & ~skip)[:4]
    assert skip.sum() <= 1                                         # (near-ties of the device's logarithm: 0.005 * 67 rows is under one)
    assert fall.sum() >= 1 and (got[fall] == EOS).all() and (got[(words == -2) & ~fall] != EOS).all()
    assert (got[words == 64] == 64).all() and np.array_equal(out[:, t, n, 1:], dbits.T)
    other = np.ones((M, 32, 16), dtype=bool)
    other[:, t, n] = False
    assert np.array_equal(out[..., 0][other], grid[..., 0][other])


# ================================================================================================ ptv_decode_logprob
def kept_with_words(kw, x, pitch, m, fp):
    """the kept set of every row from the device, as test_gpu_decode_logprob_kernels.device_kept_kw but through
    ptv_debug_pitch_constrain_words with the force word of every row (fp: [15, 32 B])"""
    B = x.shape[0]
    rows = B * 480
    full = FF_.sampling_block(DEV, kw['temperature'], kw.get('dur_temperature'), seed=3, top_k=kw.get('top_k'), min_p=kw.get('min_p'),
                              top_p=kw.get('top_p'), ascending=bool(kw.get('ascending')))
    mw = np.broadcast_to(np.asarray(m)[:, :, None, :], (B, 32, 15, 4))
    w = np.asarray(fp).reshape(15, 32, B).transpose(2, 1, 0).astype(np.int32)
    keep = torch.zeros(rows * 130, dtype=torch.uint8, device=DEV)
    thr = torch.zeros(rows, device=DEV)
    KO.leaf('ptv_debug_pitch_constrain_words', full, LK.dev(pitch.reshape(rows, 130)), LK.dev(mw.reshape(rows, 4)),
            LK.dev(LR.running_lo(x).astype(np.int32).reshape(rows)), LK.dev(w.reshape(rows)), rows, 1, keep, thr)
    return LK.host(keep).reshape(B, 32, 15, 130).astype(bool)


def test_7_decode_logprob_with_words():
    """ptv_decode_logprob at B = 3 under the 64-byte block of the log-probability kernel tests, the force arrays rhythm_ref builds from the
    decoded grid itself (every step a rhythm step): both logit layouts give the same bits; counts and err exact -- the -2 decisions free,
    the forced <eos> forced, err 0 --; the four sums within the tolerance of those tests against the fp64 restatement over the reduced
    support; logq differs from the run without words.  An <eos> decided under a -2 word with an allowed pitch beside it sets bit 0 of err"""
    name = '64'
    x, pitch, dur, mask, pp, dp = LK.case(3)
    B = 3
    ref = RR.build(x, np.full((1, 32), 3, dtype=np.uint8))
    force = (ref['pitch'], ref['dur'])
    assert not ref['err'].any()
    _, _, m, kw = LK.make_block(name, mask)
    kept = kept_with_words(kw, x, pitch, m, ref['pitch'])
    plain = LK.device_kept(name, x, pitch, mask)
    ne = ref['not_eos']
    assert not kept[ne][:, EOS].any() and np.array_equal(kept[~ne], plain[~ne])
    got = LK.run(x, pp, dp, name, mask, LK.LAYOUTS[0], force)
    for layout in (LK.LAYOUTS[1], LK.LAYOUTS[3]):
        again = LK.run(x, pp, dp, name, mask, layout, force)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), layout
    lp, cn, er = got
    (r_lp, r_cn, r_er, scale), (f_lp, _, _, _) = LK.reference(x, pp, dp, name, mask, kept, force)
    assert np.array_equal(cn, r_cn) and np.array_equal(er, r_er) and not er.any()
    K = ref['K']
    assert np.array_equal(cn[..., 2], (K < 15).astype(np.int32)) and np.array_equal(cn[..., 0], np.minimum(K + 1, 15))
    assert np.array_equal(cn[..., 3], ref['forced_dur'].sum((2, 3)))
    for col, fam in enumerate(('logp pitch', 'logp dur', 'logq pitch', 'logq dur')):
        LK.check('%s [rhythm words]' % fam, lp[..., col], r_lp[..., col], f_lp[..., col], scale[..., col])
    free = LK.run(x, pp, dp, name, mask, LK.LAYOUTS[0])
    assert lp[..., 0].tobytes() == free[0][..., 0].tobytes() and (lp[..., 2] != free[0][..., 2]).any()
    # ---- an <eos> where the word says -2 and a pitch was allowed
    b, t = 2, 6
    k = int(K[b, t])
    assert 0 < k < 15 and x[b, t, k + 1, 0] == EOS and LR.kept_sets(pitch, x, 0.0, mask=m, ascending=True)[b, t, k, :128].any()
    fp2 = ref['pitch'].copy()
    fp2[k, t * B + b] = -2
    lp2, cn2, er2 = LK.run(x, pp, dp, name, mask, LK.LAYOUTS[0], (fp2, ref['dur']))
    assert er2.tolist() == [0, 0, 1] and cn2[b, t, 2] == 0 and np.array_equal(np.delete(cn2[..., 2].ravel(), b * 32 + t),
                                                                              np.delete(cn[..., 2].ravel(), b * 32 + t))
    assert lp2[b, t, 2] == lp[b, t, 2]                             # nothing is added for it
