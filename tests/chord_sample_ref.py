"""numpy restatement of the row-independent chord decode's decisions (csrc/chord_decode.hip) -- oracle side only, never
imported by the product.

A decision of chord step t of global sample g is the first maximal index of logit + T * gumbel(word); the words are one Philox call of
the decoder's domain (tests/sample_ref.py) at the note step nothing else uses:
    sample_ref.words(seed, draw, g, t, n = 15, kind = 0, sub = j), j = 0..11
    word 0: root class j    word 1: bass class j    word 2 / 3: class 0 / 1 of chroma bit j
Root and bass take T_chord, the chroma bits T_chroma; bit j is 1 iff e1 + T g1 > e0 + T g0.  A kept step forces the decisions from
keep_c[b, t]: root / bass = the index of the single non-zero entry of [0:12] / [24:36] (a block without exactly one non-zero entry forces
nothing and sets the error bit), chroma bit k = keep_c[b, t, 12 + k] != 0.
logp = log softmax(logits)[decided], logq = log softmax(logits / T)[decided] (0 where T = 0 and for a forced decision); the chroma figure is
the sum over the 12 bits in ascending order.  The formulas take a dtype: float64 is the reference, float32 follows the kernel's term order
(the 16-lane rotation tree of its sums, its sequential chroma sum)."""
import numpy as np

import sample_ref as S

NOISE_N = 15
STEPS = 8


def noise(seed, draw, g, t):
    """g, t broadcastable -> float32 [..., 12, 4]: lane j's four Gumbel values in word order"""
    g, t = np.broadcast_arrays(np.asarray(g, dtype=np.int64), np.asarray(t, dtype=np.int64))
    w = S.words(seed, draw, g[..., None], t[..., None], NOISE_N, 0, np.arange(12))          # [..., 12, 4]
    return S.gumbel_from_word(w)


def decode_noise(seed, draw, g):
    """the noise of a whole chord decode of the samples g [B] -> float32 [B, 8, 12, 4]"""
    return noise(seed, draw, np.asarray(g, dtype=np.int64).reshape(-1, 1), np.arange(STEPS).reshape(1, STEPS))


def split(nz):
    """[..., 12, 4] -> (root [..., 12], bass [..., 12], chroma [..., 12, 2])"""
    return nz[..., 0], nz[..., 1], nz[..., 2:4]


def forced(keep_c, kept):
    """keep_c [..., 36] (entries of rows that are not kept are never looked at), kept bool [...] -> (root int [...], bits int [..., 12],
    bass int [...], err int [...]): -1 = the head stays free; bits are meaningful where kept"""
    kept = np.asarray(kept, bool)
    kc = np.where(kept[..., None], np.asarray(keep_c, np.float32), np.float32(0))
    nz = kc != 0
    out = []
    for lo in (0, 24):
        blk = nz[..., lo:lo + 12]
        one = kept & (blk.sum(-1) == 1)
        out.append(np.where(one, blk.argmax(-1), -1))
    err = (kept & ((out[0] < 0) | (out[1] < 0))).astype(np.int32)
    return out[0], nz[..., 12:24].astype(np.int64), out[1], err


def decide(root, chroma, bass, nz, Tc, Th, keep_c=None, kept=None):
    """root / bass [..., 12], chroma [..., 12, 2] logits, nz [..., 12, 4] noise (None: the argmax) -> dict(root, bits, bass: the decisions,
    forced int32 [..., 3], err int32 [...])"""
    root, chroma, bass = (np.asarray(a, np.float32) for a in (root, chroma, bass))
    if nz is None:
        nz, Tc, Th = np.zeros(root.shape + (4,), np.float32), 0.0, 0.0
    nr, nb, nc = split(nz)
    dr = np.argmax(S.perturbed(root, nr, Tc), -1)
    db = np.argmax(S.perturbed(bass, nb, Tc), -1)
    bits = S.decide_dur(chroma, nc, Th)
    shape = root.shape[:-1]
    frc, err = np.zeros(shape + (3,), np.int32), np.zeros(shape, np.int32)
    if keep_c is not None:
        kept = np.broadcast_to(np.asarray(kept, bool), shape)
        fr, fbits, fb, err = forced(keep_c, kept)
        dr, db = np.where(fr >= 0, fr, dr), np.where(fb >= 0, fb, db)
        bits = np.where(kept[..., None], fbits, bits)
        frc = np.stack([fr >= 0, 12 * kept, fb >= 0], -1).astype(np.int32)
    return dict(root=dr, bits=bits, bass=db, forced=frc, err=err)


def skippable(root, chroma, bass, nz, Tc, Th):
    """decisions the device may take either way (sample_ref.skippable): (root [...], bits [..., 12], bass [...]) bools"""
    nr, nb, nc = split(nz)
    return (S.skippable(root, nr, Tc, S.NOISE_TOL), S.skippable(chroma, nc, Th, S.NOISE_TOL), S.skippable(bass, nb, Tc, S.NOISE_TOL))


def tokens(dr, bits, db):
    """decisions -> (c [..., 36] f32 = root one-hot | bits | bass one-hot, chord14 [..., 14] f32 = root index | bits | bass index)"""
    eye = np.eye(12, dtype=np.float32)
    bits = np.asarray(bits, np.float32)
    c = np.concatenate([eye[dr], bits, eye[db]], -1)
    c14 = np.concatenate([np.asarray(dr, np.float32)[..., None], bits, np.asarray(db, np.float32)[..., None]], -1)
    return c, c14


def _tree16(x):
    """the kernel's sum over a row of 16 lanes: x += rotate(x, 8), 4, 2, 1 -- in the dtype of x"""
    for r in (8, 4, 2, 1):
        x = x + np.roll(x, r, -1)
    return x[..., 0]


def _logsoftmax12(v, d, dtype):
    """log softmax of v [..., 12] at class d [...]: v[d] - m - log(sum exp(v - m)), the sum as the kernel forms it; and the |terms|"""
    v = np.asarray(v, dtype)
    pad = np.concatenate([v, np.full(v.shape[:-1] + (4,), -np.inf, dtype)], -1)
    m = v.max(-1)
    with np.errstate(invalid='ignore'):
        s = _tree16(np.exp(pad - m[..., None]).astype(dtype))
    vd = np.take_along_axis(v, np.asarray(d)[..., None], -1)[..., 0]
    ls = np.log(s).astype(dtype)
    return ((vd - m).astype(dtype) - ls).astype(dtype), np.abs(vd) + np.abs(m) + np.abs(ls)


def _logsoftmax2(e, bit, dtype):
    """the same for pairs e [..., 2] at class bit [...]"""
    e = np.asarray(e, dtype)
    m = e.max(-1)
    ls = np.log((np.exp(e[..., 0] - m).astype(dtype) + np.exp(e[..., 1] - m).astype(dtype)).astype(dtype)).astype(dtype)
    ed = np.where(np.asarray(bit) != 0, e[..., 1], e[..., 0])
    return ((ed - m).astype(dtype) - ls).astype(dtype), np.abs(ed) + np.abs(m) + np.abs(ls)


def _seq_sum(x, dtype):
    """sequential sum over the last axis in ascending order"""
    s = np.zeros(x.shape[:-1], dtype)
    for k in range(x.shape[-1]):
        s = (s + x[..., k]).astype(dtype)
    return s


def logprob(root, chroma, bass, dec, Tc, Th, sampled=True, dtype=np.float64):
    """logits and decide()'s result -> (logp [..., 3], logq [..., 3], scale_p [..., 3], scale_q [..., 3]) in `dtype`, heads (root, chroma,
    bass); the divisions by T happen in `dtype` on the fp32 logits, as on the device; scale = the sum of the |terms| of an element"""
    root, chroma, bass = (np.asarray(a, np.float32).astype(dtype) for a in (root, chroma, bass))
    dr, bits, db, frc = dec['root'], dec['bits'], dec['bass'], dec['forced']
    Tc_, Th_ = dtype(np.float32(Tc)), dtype(np.float32(Th))
    lpr, spr = _logsoftmax12(root, dr, dtype)
    lpb, spb = _logsoftmax12(bass, db, dtype)
    lpc1, spc1 = _logsoftmax2(chroma, bits, dtype)
    lp = np.stack([lpr, _seq_sum(lpc1, dtype), lpb], -1)
    sp = np.stack([spr, spc1.sum(-1), spb], -1)
    lq, sq = np.zeros(lp.shape, dtype), np.zeros(lp.shape, np.float64)
    if sampled and Tc > 0:
        for col, (v, d) in ((0, (root, dr)), (2, (bass, db))):
            q, s = _logsoftmax12((v / Tc_).astype(dtype), d, dtype)
            free = frc[..., col] == 0
            lq[..., col], sq[..., col] = np.where(free, q, 0), np.where(free, s, 0)
    if sampled and Th > 0:
        q1, s1 = _logsoftmax2((chroma / Th_).astype(dtype), bits, dtype)
        free = (frc[..., 1] == 0)[..., None]
        lq[..., 1], sq[..., 1] = _seq_sum(np.where(free, q1, 0).astype(dtype), dtype), np.where(free, s1, 0).sum(-1)
    return lp, lq, sp, sq


def fold(step_logp, step_logq, step_forced, step_err):
    """[B, 8, 3] x 3 and [B, 8] -> (logp, logq f32 [B, 3], forced int32 [B, 3], err int32 [B]): the sequential fp32 sum over t ascending, the
    OR of the error words"""
    lp, lq = (_seq_sum(np.moveaxis(np.asarray(a, np.float32), 1, -1), np.float32) for a in (step_logp, step_logq))
    return lp, lq, np.asarray(step_forced, np.int32).sum(1, dtype=np.int32), np.bitwise_or.reduce(np.asarray(step_err, np.int32), 1)
