"""GPU: the sampled decodes over the whole accepted range of their 64-bit noise coordinates -- seed in [0, 2^64), draw in [0, 2^63), sample
index g = sample_offset + row (or a row's sample_id) in [0, 2^47) -- against the numpy restatements tests/sample_ref.py and
tests/chord_sample_ref.py, which are Python-int / uint64 arithmetic over oracle/rng_oracle.py and pinned by
tests/test_stream_coordinates_host.py.  Every other GPU test of the sampling keeps seed <= 11, draw <= 9 and g <= about 1,220, so the
upper halves of all three (counter word 1 bits 16.., counter word 3, key word 1), a seed the host stores as a negative int64, the upper
word of a row's sample_id and the carry of sample_offset + row over 2^32 are zero or absent on the device there.  A call site that
truncated one of them would stay self-consistent (shard against whole, composite against Python sequencing) and only draw another row's
noise: here every decode kind runs on every selectable note-loop path with all three coordinates high and a batch that straddles 2^32,
and each decision must follow from the emitted logits and the restated noise of ITS g.

The checks, tolerances and caps are the neighbours' own (imported, not copied): sample_ref.NOISE_TOL bounds the device's two fp32
logarithms of u and does not depend on the coordinates -- a wrong counter word changes the noise by O(1); a decision is skipped only inside
sample_ref.skippable's band (T * 4e-6 + 4 ulp), and at most SKIP_CAP = 0.005 of a case may be.  On synthetic logits (sd 0.03, 1, 6) under
exactly this noise the restatement's own skippable share was at most 7e-5 (pitch) and 2e-5 (duration).  The model, latents and paths are
those of tests/test_gpu_truncated_sampling.py."""
import functools

import numpy as np
import pytest
import torch

import chord_sample_ref as CS
import dur_limits_ref as DR
import keep_ref as K
import nucleus_ref as NR
import sample_ref as S
import test_gpu_chord_decode_kernels as KT
import test_gpu_chord_decode_model as CM
import test_gpu_constrained_decode as TC
import test_gpu_dur_limits_decode as DL
import test_gpu_keep_decode as KD
import test_gpu_nucleus_sampling as TN
import test_gpu_row_sampling_decode as RS
import test_gpu_sampling as TS
import test_gpu_truncated_sampling as TT
from test_gpu_row_sampling_kernels import GROUPS
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = TT.DEV
PATHS = TT.PATHS
SKIP_CAP = TC.SKIP_CAP
B = 32

SEED_HI = 0x9E3779B97F4A7C15              # >= 2^63 (a negative int64 word on the host), both halves non-zero
DRAW_HI = 2 ** 62 + 2 ** 32 + 5           # both halves non-zero
OFF_CARRY = 2 ** 32 - 16                  # B = 32: rows 0..15 below 2^32, rows 16..31 at or above it
OFF_TOP = 2 ** 47 - 32                    # B = 32: the last row is the largest legal id, 2^47 - 1
OFF_PAST = 2 ** 47 - 1                    # a legal offset whose later rows have g in [2^47, 2^48): the counter's 16-bit field holds them
FAR = 2 ** 32                             # OFF_CARRY + FAR: the same low words, other high words
TWO_PATHS = ('default', 'bf16-step-loop')
KINDS = ('sampled', 'truncated', 'constrained', 'rows')
TRUNC = dict(top_k=8, top_p=0.9)
NAMES = ('pitch logits', 'duration logits', 'xhat')


def row_ids(n=B, shift=0):
    """scattered ids that straddle 2^32 near row 15"""
    return [2 ** 32 - 100 + 7 * b + shift for b in range(n)]


@functools.lru_cache(maxsize=None)
def noise(ids):
    """restated noise at (SEED_HI, DRAW_HI) of the samples `ids` (a tuple, or an int: the 32 samples from there): computed once, shared,
    never modified"""
    g = np.arange(ids, ids + B) if isinstance(ids, int) else np.array(ids, dtype=np.int64)
    p, d = S.decode_noise(SEED_HI, DRAW_HI, g)
    p.setflags(write=False)
    d.setflags(write=False)
    return p, d


def hi_block(offset, rows=slice(None), **kw):
    if 'pitch_mask' in kw:
        kw['pitch_mask'] = TC.chord_mask()[0][rows].contiguous()
    return TT.block(offset, seed=SEED_HI, draw=DRAW_HI, **kw)


def rows_block(n=B, ids=None, offset=0, cons=None):
    """the 80-byte block over a table of the six GROUPS dealt by row % 6"""
    tab = FF_.RowSampling(torch.from_numpy(RS.table_words(n, ids=ids, offset=offset)).to(DEV), n, offset)
    return FF_.sampling_block(DEV, seed=SEED_HI, draw=DRAW_HI, rows=tab, **(cons or {}))


def block_of(kind, offset, rows=slice(None)):
    """the block of a decode kind whose row 0 is sample `offset` (row-wise: the scattered ids shifted by offset - OFF_CARRY)"""
    if kind == 'sampled':
        blk, words = hi_block(offset), 4
    elif kind == 'truncated':
        blk, words = hi_block(offset, **TRUNC), 6
    elif kind == 'constrained':
        blk, words = hi_block(offset, rows, ascending=True, pitch_mask=True), 8
    elif kind == 'rows':
        blk, words = rows_block(B, row_ids(shift=offset - OFF_CARRY), cons=RS.masked()), 10
    else:                                                                                  # 'rows/default': default ids, no constraint
        blk, words = rows_block(B, offset=offset), 10
    assert blk.numel() == words and blk.dtype == torch.int64                               # 32, 48, 64 and 80 bytes
    return blk


@functools.lru_cache(maxsize=None)
def run(path, kind, offset=OFF_CARRY, keep=None, half=False):
    """one decode of a path, run once and shared: kind at `offset`; keep: None, 'steps' (the first 16 steps of synth_batch's grid kept)
    or 'limits' (dur_limits(min_dur=2, max_dur=8), which needs the 64-byte kind: the sampled block with the vacuous constraint);
    half: z[16:] (and mask[16:])"""
    attrs, prec = PATHS[path]
    m = TT.model()
    m.set_precision(prec)
    z = TT.latents()
    try:
        with TT.patched(attrs):
            if keep == 'steps':
                kp = m.keep(torch.from_numpy(synth_batch(B, 5)[0]).to(DEV), range(16))
                return KD.kdecode(m, z, block_of(kind, offset), kp)
            if keep == 'limits':
                return KD.kdecode(m, z, hi_block(offset, ascending=False), m.dur_limits(min_dur=2, max_dur=8, batch=B))
            if half:
                return TT.decode(m, z[16:].contiguous(), block_of(kind, offset, slice(16, None)))
            return TT.decode(m, z, block_of(kind, offset))
    finally:
        m.set_precision('bf16')


def rows_explained(po, do, xh, ids, cons, mask_np, what):
    """the check of tests/test_gpu_row_sampling_decode.py::test_2_every_decision_is_explained: every decision of a row follows from the
    emitted logits by the restated rule with THAT row's parameters and the noise at THAT row's id; the T = 0 rows are the constrained
    argmax, exactly"""
    pn, dn = noise(tuple(ids))
    for g in range(6):
        rows = np.arange(g, len(ids), 6)
        T, td, kw = RS.scalars(g)
        if T == 0:
            al = TC.allowed_of(xh[rows], cons, mask_np[rows])
            assert np.array_equal(xh[rows][..., 0], np.where(al, po[rows], np.float32(-np.inf)).argmax(-1)), what
            assert np.array_equal(xh[rows][..., 1:], (do[rows][..., 1] > do[rows][..., 0]).astype(np.int64)), what
            continue
        assert (T, td) == (TC.T_PITCH, TC.T_DUR)                                            # (explained() judges with these)
        TC.explained(po[rows], do[rows], xh[rows], pn[rows], dn[rows], dict(kw, **cons), mask_np[rows], '%s group %d' % (what, g))


def explained(kind, out, offset, what, rows=slice(None)):
    """the neighbours' check of a decode kind at (SEED_HI, DRAW_HI) and the samples offset + b"""
    po, do, xh = out
    mask_np = TC.chord_mask()[1]
    if kind == 'rows':
        return rows_explained(po, do, xh, row_ids(shift=offset - OFF_CARRY), dict(pitch_mask=True, ascending=True), mask_np, what)
    pn, dn = (a[rows] for a in noise(offset))
    if kind == 'sampled':
        TS.explained(po, do, xh, pn, dn, what)
    elif kind == 'truncated':
        # every rule restated (top_k and the nucleus): tests/test_gpu_nucleus_sampling.py's check; where the nucleus keeps all of a row's
        # eight best classes -- every row of this flat-logit model -- the rule is top_k = 8 alone and the truncated module's check says so
        TN.explained(po, do, xh, pn, dn, TT.T_PITCH, TRUNC, what)
        k, l, q = TN.rule(TRUNC)
        if np.array_equal(NR.keep_mask(po, TT.T_PITCH, k, l, q), NR.keep_mask(po, TT.T_PITCH, k, l, NR.q24_of(None))):
            TT.explained(po, do, xh, pn, dn, dict(top_k=TRUNC['top_k']), what + ' (top_k alone)')
    else:
        TC.explained(po, do, xh, pn, dn, dict(pitch_mask=True, ascending=True), mask_np[16:] if po.shape[0] == 16 else mask_np, what)


# ---------------------------------------------------------------------------------------------------------------------------------
BASE = (11, 4, 0)
SEEDS = (2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, SEED_HI)
DRAWS = (2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, DRAW_HI)
OFFSETS = (2 ** 32 - 10, 2 ** 32, 2 ** 40 + 3, 2 ** 47 - 20, OFF_PAST)
FIELDS = ([BASE] + [(s, BASE[1], BASE[2]) for s in SEEDS] + [(BASE[0], d, BASE[2]) for d in DRAWS] + [(BASE[0], BASE[1], o) for o in OFFSETS]
          + [(SEED_HI, DRAW_HI, OFF_CARRY), (SEED_HI, DRAW_HI, OFF_PAST), (2 ** 64 - 1, 2 ** 63 - 1, 2 ** 47 - 20)])


def test_1_noise_one_field_at_a_time():
    """ptv_debug_sample_noise and ptv_debug_chord_noise (the decoders' own device functions), 20 rows: from (seed, draw, offset) =
    (11, 4, 0) each coordinate alone through its 32-bit and 64-bit edges, then all three high; (t, n) in {(0, 0), (31, 14)} for the note
    noise, t in {0, 7} for the chord noise.  |device - restatement| <= sample_ref.NOISE_TOL, the bound of the small-coordinate tests:
    it covers the device's fp32 logarithms and knows nothing of the coordinates"""
    n = 20
    worst, seen = 0.0, set()
    for seed, draw, off in FIELDS:
        blk = FF_.sampling_block(DEV, 1.0, 0.7, seed=seed, draw=draw, sample_offset=off)
        g = off + np.arange(n)
        for t, nn in ((0, 0), (31, 14)):
            op = torch.full((n + 2, 130), 777.0, device=DEV)
            od = torch.full((n + 2, 5, 2), 777.0, device=DEV)
            call('ptv_debug_sample_noise', ptr(blk), n, t, nn, ptr(op), ptr(od), stream_ptr())
            torch.cuda.synchronize()
            gp, gd = op.cpu().numpy(), od.cpu().numpy()
            assert (gp[n:] == 777.0).all() and (gd[n:] == 777.0).all()
            dp = np.abs(gp[:n].astype(np.float64) - S.pitch_noise(seed, draw, g, t, nn)).max()
            dd = np.abs(gd[:n].astype(np.float64) - S.dur_noise(seed, draw, g, t, nn)).max()
            assert dp <= S.NOISE_TOL and dd <= S.NOISE_TOL, ((seed, draw, off), (t, nn), dp, dd)
            worst = max(worst, dp, dd)
            seen.add(gp[:n].tobytes())
        for t in (0, 7):
            out = torch.full((n + KT.GUARD, 12, 4), float(KT.SENT_F), device=DEV)
            assert lib().ptv_debug_chord_noise(ptr(blk), n, t, ptr(out), stream_ptr()) == 0
            got = KT.host(out)
            assert (got[n:] == KT.SENT_F).all()
            dc = np.abs(got[:n].astype(np.float64) - CS.noise(seed, draw, g, t)).max()
            assert dc <= S.NOISE_TOL, ((seed, draw, off), t, dc)
            worst = max(worst, dc)
    assert len(seen) == 2 * len(FIELDS)                                                     # no two settings drew the same noise
    print('worst |device noise - restatement| over %d settings: %.3e (NOISE_TOL %.1e)' % (len(FIELDS), worst, S.NOISE_TOL))


@pytest.mark.parametrize('offset', [2 ** 32 - 256, 2 ** 47 - 512])
def test_2_chord_decisions(offset):
    """ptv_chord_decide on 512 rows whose sample indices cross 2^32 at row 256, or end at the largest legal id"""
    n, t = 512, 7
    root, chroma, bass = KT.logits(n, 2)
    nz = CS.noise(SEED_HI, DRAW_HI, offset + np.arange(n), t)
    want = CS.decide(root, chroma, bass, nz, 1.0, 0.7)
    blk = FF_.sampling_block(DEV, 1.0, 0.7, seed=SEED_HI, draw=DRAW_HI, sample_offset=offset)
    r = KT.decide(root, chroma, bass, t, blk)
    KT.explained(r, want, CS.skippable(root, chroma, bass, nz, 1.0, 0.7), 'chord decisions from sample 0x%x' % offset)
    assert (r['root'] != np.argmax(root, -1)).mean() > 0.2                                  # the noise is there
    low = CS.decide(root, chroma, bass, CS.noise(SEED_HI, DRAW_HI, (offset + np.arange(n)) & 0xFFFFFFFF, t), 1.0, 0.7)
    assert (r['root'] != low['root']).mean() > 0.2                                          # ... and it is not the noise of g lo alone


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('path', list(PATHS))
def test_3_every_decode_kind_on_every_path_across_the_carry(path, kind):
    """B = 32 at (SEED_HI, DRAW_HI) and sample_offset = OFF_CARRY (row-wise: the six GROUPS dealt by b % 6 under the chord mask and
    `ascending`, sample_id = 2^32 - 100 + 7 b): every decision is the neighbours' restated rule under the noise of its own g.  So is
    the same decode with 2^32 added to every g -- the same low words --, and it differs in the rows below the carry and in the rows above
    it: a device that ignored the high word of g would make the two equal"""
    out = run(path, kind)
    explained(kind, out, OFF_CARRY, '%s %s' % (path, kind))
    far = run(path, kind, OFF_CARRY + FAR)
    explained(kind, far, OFF_CARRY + FAR, '%s %s + 2^32' % (path, kind))
    sampled_rows = np.array([b for b in range(B) if kind != 'rows' or GROUPS[b % 6]['temperature'] > 0])
    for part in (sampled_rows[sampled_rows < 16], sampled_rows[sampled_rows >= 16]):
        assert (out[2][part] != far[2][part]).any(), (path, kind, part[0])


@pytest.mark.parametrize('kind', ('sampled', 'constrained'))
@pytest.mark.parametrize('path', TWO_PATHS)
def test_4_shards_across_the_carry(path, kind):
    """z[16:] at sample_offset = 2^32 is rows 16..31 of the OFF_CARRY decode, bit for bit"""
    whole, half = run(path, kind), run(path, kind, 2 ** 32, half=True)
    for a_, b_, what in zip(whole, half, NAMES):
        assert b_.shape[0] == 16 and np.array_equal(a_[16:], b_), (path, kind, what)
    explained(kind, half, OFF_CARRY, '%s %s z[16:] at 2^32' % (path, kind), rows=slice(16, None))


@pytest.mark.parametrize('path', TWO_PATHS)
def test_5_top_of_the_range(path):
    """the sampled decode and the row-wise decode with default ids at OFF_TOP (the last row is sample 2^47 - 1), and the sampled decode
    at OFF_PAST, whose rows 1..31 have g in [2^47, 2^47 + 30]: the stated stream, g = sample_offset + b"""
    explained('sampled', run(path, 'sampled', OFF_TOP), OFF_TOP, '%s sampled at 2^47 - 32' % path)
    explained('sampled', run(path, 'sampled', OFF_PAST), OFF_PAST, '%s sampled at 2^47 - 1' % path)
    po, do, xh = run(path, 'rows/default', OFF_TOP)
    rows_explained(po, do, xh, [OFF_TOP + b for b in range(B)], {}, TC.chord_mask()[1], '%s rows at 2^47 - 32' % path)
    assert (xh != run(path, 'sampled', OFF_TOP)[2]).any()


@pytest.mark.parametrize('path', TWO_PATHS)
def test_6_forced_variants_of_the_loops(path):
    """the FORCE = 1 instantiations at (SEED_HI, DRAW_HI, OFF_CARRY): the first 16 steps of synth_batch's grid kept under the sampled and
    under the constrained block, and dur_limits(min_dur=2, max_dur=8) under the 64-byte block its words need.  The kept steps come out
    as given, the free decisions are explained by the same noise (tests/test_gpu_keep_decode.py::explained_free), every duration bit of
    the limited decode is the documented decision (tests/test_gpu_dur_limits_decode.py::explained) and its pitches are sample_ref's"""
    x = synth_batch(B, 5)[0]
    ref = K.build(x, range(16))
    fp, fd = ref['forced_pitch'], ref['forced_dur']
    assert fp[:, :16].any() and not fp[:, 16:].any()
    pn, dn = noise(OFF_CARRY)
    mask, mask_np = TC.chord_mask()
    for kind, kw in (('sampled', {}), ('constrained', dict(pitch_mask=mask, ascending=True))):
        po, do, xh = run(path, kind, keep='steps')
        assert np.array_equal(xh[..., 0][fp], x[:, :, 1:, 0][fp]) and np.array_equal(xh[..., 1:][fd], x[:, :, 1:, 1:][fd]), (path, kind)
        KD.explained_free(po, do, xh, pn, dn, kw, mask_np, ref, '%s %s keep' % (path, kind))
        assert (xh[:, 16:] != run(path, kind)[2][:, 16:]).any()                             # the kept bar reaches the free one
    po, do, xh = run(path, 'sampled', keep='limits')
    lim = DR.build(np.full((B, 32), 2, np.uint8), np.full((B, 32), 8, np.uint8), np.ones((B, 32), np.uint8), B)
    det, both = DL.explained(do, xh, dn, TT.T_DUR, lim, '%s limits' % path)
    assert det >= 1 and both >= 1
    v = DL.values(xh)
    assert ((v >= 1) & (v <= 7)).all() and not ((DL.values(run(path, 'sampled')[2]) >= 1) & (DL.values(run(path, 'sampled')[2]) <= 7)).all()
    want = S.decide_pitch(po, pn, TT.T_PITCH)
    skip = S.skippable(po, pn, TT.T_PITCH, S.NOISE_TOL)
    print('%s limits: pitch skipped %d of %d' % (path, skip.sum(), skip.size))
    assert not ((xh[..., 0] != want) & ~skip).any() and skip.mean() <= SKIP_CAP


# ---------------------------------------------------------------------------------------------------------------------------------
HI_KW = dict(temperature=1.0, dur_temperature=0.7, seed=SEED_HI, draw=DRAW_HI)


def test_7a_inference_decode_and_graph_replay():
    m = TT.model()
    zc, zr = TT.latents()[:, :256].contiguous(), TT.latents()[:, 256:].contiguous()
    want = run('default', 'sampled')
    got = m.inference_decode(zc, zr, sample_offset=OFF_CARRY, **HI_KW)
    assert np.array_equal(got, want[2])
    assert m.decoder._last_decode.sampling.cpu().numpy().view(np.uint64)[:3].tolist() == [SEED_HI, DRAW_HI, OFF_CARRY]
    small = m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, draw=5)
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        assert np.array_equal(m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, draw=5), small)
        assert np.array_equal(m.inference_decode(zc, zr, sample_offset=OFF_CARRY, **HI_KW), want[2])
        assert np.array_equal(m.inference_decode(zc, zr, temperature=1.0, dur_temperature=0.7, seed=9, draw=5), small)
        assert m.decoder.graph_captures == before + 1
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()


def test_7b_best_of_tiles_ids_and_offsets_across_the_carry():
    m = TT.model()
    n = 16
    zc, zr = TT.latents()[:n, :256].contiguous(), TT.latents()[:n, 256:].contiguous()
    ids = [2 ** 32 - 8 + b for b in range(n)]
    tab = FF_.RowSampling(torch.from_numpy(RS.table_words(n, ids=ids)).to(DEV), n)
    t2 = tab.tiled(2)
    torch.cuda.synchronize()
    tiled = [ids[b] + n * k for k in range(2) for b in range(n)]
    assert t2.batch == 2 * n and t2.table.cpu().numpy().view(np.int64)[:, 3].tolist() == tiled
    assert np.array_equal(t2.table.cpu().numpy()[:, :6], np.concatenate([tab.table.cpu().numpy()[:, :6]] * 2))
    assert tab.table.cpu().numpy().view(np.int64)[:, 3].tolist() == ids                     # (the original is untouched)
    m.decode_best_of(zc, zr, 2, rows=tab, seed=SEED_HI, draw=DRAW_HI)
    torch.cuda.synchronize()
    cand = m.decoder.last_xhat[:, :, 1:].cpu().numpy()
    words = np.concatenate([RS.table_words(n, ids=tiled[:n]), RS.table_words(n, ids=tiled[n:])])      # (row 16 k + b keeps the group of b)
    assert np.array_equal(t2.table.cpu().numpy(), words)
    plain = m.inference_decode(zc.repeat(2, 1), zr.repeat(2, 1), rows=FF_.RowSampling(torch.from_numpy(words).to(DEV), 2 * n),
                               seed=SEED_HI, draw=DRAW_HI)
    assert cand.shape[0] == 2 * n and np.array_equal(cand, plain)
    assert (cand[:n] != cand[n:]).any()
    # the scalar keywords: candidate k of row b is sample sample_offset + 16 k + b -- the carry falls inside the second tile
    off = 2 ** 32 - 24
    m.decode_best_of(zc, zr, 2, sample_offset=off, **HI_KW)
    torch.cuda.synchronize()
    cand = m.decoder.last_xhat[:, :, 1:].cpu().numpy()
    plain = m.inference_decode(zc.repeat(2, 1), zr.repeat(2, 1), sample_offset=off, **HI_KW)
    assert np.array_equal(cand, plain)
    assert (cand[:n] != cand[n:]).any()


def test_7c_decode_chords():
    """DisentangleVAE.decode_chords at samples 2^32 - 8 .. 2^32 + 23: every decision from the emitted logits and chord_sample_ref's noise
    (tests/test_gpu_chord_decode_model.py::explained, as there at offset 32)"""
    m = TT.model()
    zc = TT.latents()[:, :256].contiguous()
    off = 2 ** 32 - 8
    c, c14 = m.decode_chords(zc, chord_temperature=1.0, chroma_temperature=0.7, seed=SEED_HI, draw=DRAW_HI, sample_offset=off)
    torch.cuda.synchronize()
    d = CM.decisions(c14)
    want_c, want_c14 = CS.tokens(d['root'], d['bits'], d['bass'])
    assert np.array_equal(CM.host(c), want_c) and np.array_equal(CM.host(c14), want_c14)
    nz = CS.decode_noise(SEED_HI, DRAW_HI, off + np.arange(B))
    CM.explained(CM.emitted(m), d, nz, 1.0, 0.7, 'decode_chords from sample 2^32 - 8')
    low = m.decode_chords(zc, chord_temperature=1.0, chroma_temperature=0.7, seed=SEED_HI, draw=DRAW_HI, sample_offset=off + FAR)[1]
    assert (CM.host(low)[:8] != CM.host(c14)[:8]).any() and (CM.host(low)[8:] != CM.host(c14)[8:]).any()
