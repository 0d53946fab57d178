"""numpy restatement of the chord grammar (csrc/chord_decode.hip: chord_decide_grammar_kernel; include/ptvae_hip.h "Chord grammar") --
oracle side only, never imported by the product.  Built on chord_sample_ref.py / sample_ref.py.

A rule word per (row, step): bits 0..11 the allowed roots, bits 12..23 the allowed pitch classes of the chroma, bit 24 VOCAB, bit 25
ROOT_IN_CHORD, bit 26 BASS_IN_CHORD; a vocabulary of V <= 64 root-relative 12-bit templates.  The order of a step's decisions:
    kept step   chord_sample_ref's forced decisions; the rule is not consulted (the word is the identity)
    root        first maximum over the allowed roots (none allowed: all, error 2)
    chroma      without VOCAB: bit p free iff mask bit p, else 0; ROOT_IN_CHORD: bit r is 1
                with VOCAB (and V > 0): template v is A_v = rot12(vocab[v], r), allowed iff A_v <= mask | {r} (none: all, error 4);
                score s_v = sum_p (p in A_v ? e1[p] : e0[p]) (fp32, p ascending from 0); first maximum of s_v + T_chroma * g_v,
                g_v = word v >> 4 of sample_ref.words(seed, draw, g, t, n = 15, kind = 0, sub = 16 + (v & 15))
    bass        BASS_IN_CHORD: interval i allowed iff bit (r + i) % 12 of the decided chroma (no bit at all: all, error 8)
logp is chord_sample_ref's (the model's own softmaxes); logq is the log softmax at T over the ALLOWED set: forced bits add 0, the
vocabulary figure is s_v / T - log sum_{allowed u} exp(s_u / T), a lane adding its templates j, j + 16, j + 32, j + 48 in that order and
the 16 lanes through the kernel's rotation tree."""
import numpy as np

import chord_sample_ref as CS
import sample_ref as S

IDENTITY = 0x00ffffff
VOCAB, ROOT_IN_CHORD, BASS_IN_CHORD = 1 << 24, 1 << 25, 1 << 26
ERR_KEEP, ERR_ROOT_MASK, ERR_NO_TEMPLATE, ERR_NO_BASS = 1, 2, 4, 8
MAX_VOCAB = 64
J12 = np.arange(12)


def rot12(x, r):
    """the 12-bit set x moved up by r (mod 12): interval i -> pitch class (r + i) % 12"""
    x, r = np.asarray(x, np.int64), np.asarray(r, np.int64)
    return ((x << r) | (x >> (12 - r))) & 0xfff


def unrot12(x, r):
    """pitch class p -> interval (p - r) % 12"""
    x, r = np.asarray(x, np.int64), np.asarray(r, np.int64)
    return ((x >> r) | (x << (12 - r))) & 0xfff


def bitset(bits):
    """[..., 12] of 0 / 1 -> the integer set"""
    return (np.asarray(bits, np.int64) << J12).sum(-1)


def members(x):
    """integer sets [...] -> bool [..., 12]"""
    return ((np.asarray(x, np.int64)[..., None] >> J12) & 1).astype(bool)


def vocab_noise(seed, draw, g, t, V):
    """g, t broadcastable -> float32 [..., V]: the Gumbel value of every template"""
    g, t = np.broadcast_arrays(np.asarray(g, dtype=np.int64), np.asarray(t, dtype=np.int64))
    v = np.arange(V)
    w = S.words(seed, draw, g[..., None], t[..., None], CS.NOISE_N, 0, 16 + (v & 15))      # [..., V, 4]
    w = np.take_along_axis(w, np.broadcast_to((v >> 4)[:, None], w.shape[:-1] + (1,)), -1)[..., 0]
    return S.gumbel_from_word(w)


def _seq(terms, dtype):
    """sequential sum over the last axis, ascending, from 0, in dtype"""
    s = np.zeros(terms.shape[:-1], dtype)
    for k in range(terms.shape[-1]):
        s = (s + terms[..., k].astype(dtype)).astype(dtype)
    return s


def scores(chroma, A, dtype=np.float32):
    """chroma [..., 12, 2] logits, A int [..., V] absolute sets -> (s [..., V] in dtype, magnitude [..., V] = the sum of the 12 |terms|)"""
    e = np.asarray(chroma, np.float32)
    terms = np.where(members(A), e[..., None, :, 1], e[..., None, :, 0])                     # [..., V, 12]
    return _seq(terms, dtype), np.abs(terms.astype(np.float64)).sum(-1)


def sets(rule, vocab, dr, bits=None, kept=None):
    """the allowed sets of rows with rule words `rule` [...] once the root dr [...] (and, for the bass, the chroma bits [..., 12]) are decided:
    dict(word, root bool [..., 12], root_yield, bit_free [..., 12], bit_one [..., 12], use_vocab [...], A int [..., V], tmpl bool [..., V],
    tmpl_yield, bass bool [..., 12], bass_yield)"""
    word = np.asarray(rule, np.int64) & 0xffffffff
    dr = np.asarray(dr, np.int64)
    word = np.broadcast_to(word, dr.shape).copy()
    if kept is not None:
        word[np.broadcast_to(np.asarray(kept, bool), dr.shape)] = IDENTITY
    vocab = np.asarray(vocab, np.int64).reshape(-1) & 0xfff
    V = len(vocab)
    rmask, cmask = word & 0xfff, (word >> 12) & 0xfff
    root_yield = rmask == 0
    out = dict(word=word, root=members(np.where(root_yield, 0xfff, rmask)), root_yield=root_yield)
    root_in = (word & ROOT_IN_CHORD) != 0
    out['bit_one'] = root_in[..., None] & (J12 == dr[..., None])
    out['bit_free'] = members(cmask) & ~out['bit_one']
    out['use_vocab'] = ((word & VOCAB) != 0) & (V > 0)
    A = rot12(vocab, dr[..., None])
    fits = (A & ~(cmask | (1 << dr))[..., None]) == 0
    none = ~fits.any(-1)
    out.update(A=A, tmpl=fits | none[..., None], tmpl_yield=out['use_vocab'] & none)
    if bits is not None:
        b12 = bitset(bits)
        bass_in = (word & BASS_IN_CHORD) != 0
        out['bass_yield'] = bass_in & (b12 == 0)
        out['bass'] = members(np.where(bass_in & (b12 != 0), unrot12(b12, dr), 0xfff))
    return out


def _first_max(logits, noise, T, allowed):
    x = S.perturbed(logits, noise, T)
    return np.argmax(np.where(allowed, x, -np.inf), -1)


def decide(root, chroma, bass, nz, vnz, Tc, Th, rule, vocab, keep_c=None, kept=None):
    """root / bass [..., 12], chroma [..., 12, 2] logits, nz [..., 12, 4] and vnz [..., V] noise (both None: the argmax), rule int [...]
    -> dict(root, bits, bass, template (-1: not from the vocabulary), forced int32 [..., 3], err int32 [...])"""
    root, chroma, bass = (np.asarray(a, np.float32) for a in (root, chroma, bass))
    vocab = np.asarray(vocab, np.int64).reshape(-1)
    shape = root.shape[:-1]
    if nz is None:
        nz, vnz, Tc, Th = np.zeros(shape + (12, 4), np.float32), np.zeros(shape + (len(vocab),), np.float32), 0.0, 0.0
    nr, nb, nc = CS.split(nz)
    kept_ = np.zeros(shape, bool) if keep_c is None else np.broadcast_to(np.asarray(kept, bool), shape)
    fr, fbits, fb, err = CS.forced(np.zeros(shape + (36,), np.float32) if keep_c is None else keep_c, kept_)
    err = err.astype(np.int32)
    # root
    st = sets(rule, vocab, np.zeros(shape, np.int64), kept=kept_)
    dr = np.where(fr >= 0, fr, _first_max(root, nr, Tc, st['root']))
    err = err | np.where(st['root_yield'], ERR_ROOT_MASK, 0).astype(np.int32)
    # chroma
    st = sets(rule, vocab, dr, kept=kept_)
    mbits = np.where(st['bit_one'], 1, np.where(st['bit_free'], S.decide_dur(chroma, nc, Th), 0))
    template = np.full(shape, -1, np.int64)
    bits = mbits
    if len(vocab):
        s, _ = scores(chroma, st['A'])
        dv = _first_max(s, vnz, Th, st['tmpl'])
        vbits = members(np.take_along_axis(st['A'], dv[..., None], -1)[..., 0]).astype(np.int64)
        bits = np.where(st['use_vocab'][..., None], vbits, mbits)
        template = np.where(st['use_vocab'], dv, -1)
        err = err | np.where(st['tmpl_yield'], ERR_NO_TEMPLATE, 0).astype(np.int32)
    bits = np.where(kept_[..., None], fbits, bits)
    # bass
    st = sets(rule, vocab, dr, bits, kept_)
    db = np.where(fb >= 0, fb, _first_max(bass, nb, Tc, st['bass']))
    err = err | np.where(st['bass_yield'], ERR_NO_BASS, 0).astype(np.int32)
    frc = np.stack([fr >= 0, 12 * kept_, fb >= 0], -1).astype(np.int32)
    return dict(root=dr, bits=bits, bass=db, template=template, forced=frc, err=err)


def template_of(bits, A):
    """the index of the template whose set is the decided chroma (templates are distinct, so there is at most one); -1: none"""
    hit = A == bitset(bits)[..., None]
    return np.where(hit.any(-1), hit.argmax(-1), -1)


def _gap(x, mag, best_only=False):
    """x float64 [..., n] perturbed values (-inf where disallowed), mag [..., n] -> (gap of the two best, a magnitude): the larger magnitude
    of the two (sample_ref.top2_gap's convention, the 12-class heads), or with best_only the magnitude of the larger value alone"""
    if x.shape[-1] < 2:                                      # one candidate: never close to another
        x = np.concatenate([np.full(x.shape, -np.inf), x], -1)
        mag = np.concatenate([np.zeros(x.shape[:-1] + (1,)), np.broadcast_to(mag, x.shape[:-1] + (1,))], -1)
    idx = np.argsort(x, -1)[..., -2:]
    top = np.take_along_axis(x, idx, -1)
    m = np.take_along_axis(np.broadcast_to(mag, x.shape), idx, -1)
    two = np.isfinite(top[..., 0])
    with np.errstate(invalid='ignore'):
        gap = np.where(two, top[..., 1] - top[..., 0], np.inf)
    return gap, np.where(two & (not best_only), m.max(-1), m[..., 1])


def _skip(logits, noise, T, allowed, mag=None):
    lg = np.asarray(logits, np.float64)
    x = np.where(allowed, lg + float(T) * np.asarray(noise, np.float64), -np.inf)
    gap, m = _gap(x, np.abs(lg) if mag is None else mag, best_only=mag is not None)
    return gap < T * S.NOISE_TOL + 4 * np.spacing(m.astype(np.float32)).astype(np.float64)


def skippable(root, chroma, bass, nz, vnz, Tc, Th, rule, vocab, dec):
    """decisions the device may take either way, judged with the allowed sets of `dec` (a decide() result): (root [...], chroma [..., 12],
    bass [...]) bools.  Root and bass follow sample_ref.skippable (4 ulp of the larger |logit| of the two best).  A vocabulary step marks
    all 12 bits when its template decision is skippable: the two best perturbed scores are closer than T * NOISE_TOL plus 4 ulp of the
    LARGER score's own 12-term magnitude (the sum of the |terms| of the best score, not of the runner-up).  Forced decisions are never
    skippable."""
    nr, nb, nc = CS.split(nz)
    kept = dec['forced'][..., 1] != 0
    st = sets(rule, vocab, dec['root'], dec['bits'], kept)
    sr = _skip(root, nr, Tc, st['root']) & (dec['forced'][..., 0] == 0)
    sb = _skip(bass, nb, Tc, st['bass']) & (dec['forced'][..., 2] == 0)
    sc = S.skippable(chroma, nc, Th, S.NOISE_TOL) & st['bit_free'] & ~kept[..., None]
    if len(np.asarray(vocab).reshape(-1)):
        s, mag = scores(chroma, st['A'])
        sv = _skip(s, vnz, Th, st['tmpl'], mag)
        sc = np.where(st['use_vocab'][..., None], (sv & ~kept)[..., None], sc)
    return sr, sc, sb


def _masked_logsoftmax12(a, d, allowed, dtype):
    """log softmax over the allowed classes of a [..., 12] at class d: the kernel's 16-lane sum; and the |terms|"""
    a = np.where(allowed, np.asarray(a, dtype), dtype(-np.inf))
    pad = np.concatenate([a, np.full(a.shape[:-1] + (4,), -np.inf, dtype)], -1)
    m = a.max(-1)
    s = CS._tree16(np.exp(pad - m[..., None]).astype(dtype))
    ad = np.take_along_axis(a, np.asarray(d)[..., None], -1)[..., 0]
    ls = np.log(s).astype(dtype)
    return ((ad - m).astype(dtype) - ls).astype(dtype), np.abs(ad) + np.abs(m) + np.abs(ls)


def template_logq(chroma, A, allowed, dv, T, dtype):
    """log of softmax(s / T) over the allowed templates at template dv, in the kernel's term order; and the |terms| (the 12-term magnitudes
    of the decided and of the best score over T, and the logarithm)"""
    s, mag = scores(chroma, A, dtype)
    T_ = dtype(np.float32(T))
    a = np.where(allowed, (s / T_).astype(dtype), dtype(-np.inf))
    m = a.max(-1)
    V = a.shape[-1]
    e = np.where(allowed, np.exp(a - m[..., None]).astype(dtype), dtype(0))
    e = np.concatenate([e, np.zeros(e.shape[:-1] + (MAX_VOCAB - V,), dtype)], -1).reshape(e.shape[:-1] + (4, 16))
    part = _seq(np.moveaxis(e, -2, -1), dtype)                                               # lane j: k = 0..3 ascending
    ls = np.log(CS._tree16(part)).astype(dtype)
    ad = np.take_along_axis(a, dv[..., None], -1)[..., 0]
    mag_d = np.take_along_axis(mag, dv[..., None], -1)[..., 0]
    mag_m = np.take_along_axis(mag, a.argmax(-1)[..., None], -1)[..., 0]
    return ((ad - m).astype(dtype) - ls).astype(dtype), (mag_d + mag_m) / float(np.float32(T)) + np.abs(ls)


def logprob(root, chroma, bass, dec, Tc, Th, rule, vocab, sampled=True, dtype=np.float64):
    """chord_sample_ref.logprob under the grammar, at the decisions of `dec` (root, bits, bass, forced) -> (logp, logq, scale_p, scale_q)
    [..., 3]: logp is the plain decode's, logq is taken over the allowed sets"""
    lp, _, sp, _ = CS.logprob(root, chroma, bass, dec, Tc, Th, sampled, dtype)
    root, chroma, bass = (np.asarray(a, np.float32).astype(dtype) for a in (root, chroma, bass))
    frc = dec['forced']
    kept = frc[..., 1] != 0
    st = sets(rule, vocab, dec['root'], dec['bits'], kept)
    lq, sq = np.zeros(lp.shape, dtype), np.zeros(lp.shape, np.float64)
    Tc_, Th_ = dtype(np.float32(Tc)), dtype(np.float32(Th))
    if sampled and Tc > 0:
        for col, v, d, al in ((0, root, dec['root'], st['root']), (2, bass, dec['bass'], st['bass'])):
            q, s = _masked_logsoftmax12((v / Tc_).astype(dtype), d, al, dtype)
            free = frc[..., col] == 0
            lq[..., col], sq[..., col] = np.where(free, q, 0), np.where(free, s, 0)
    if sampled and Th > 0:
        q1, s1 = CS._logsoftmax2((chroma / Th_).astype(dtype), dec['bits'], dtype)
        free = st['bit_free'] & ~kept[..., None]
        qc, sc = _seq(np.where(free, q1, 0).astype(dtype), dtype), np.where(free, s1, 0).sum(-1)
        if len(np.asarray(vocab).reshape(-1)):
            dv = template_of(dec['bits'], st['A'])
            on = st['use_vocab'] & ~kept
            assert (dv[on] >= 0).all(), 'a vocabulary step decided a chroma that is no template'
            qv, sv = template_logq(chroma, st['A'], st['tmpl'], np.maximum(dv, 0), Th, dtype)
            qc, sc = np.where(on, qv, qc), np.where(on, sv, sc)
        lq[..., 1], sq[..., 1] = qc, sc
    return lp, lq, sp, sq


def template_distribution(chroma, rule_word, vocab, r, T):
    """float64 probabilities [V] of the templates at one row: softmax(s / T) over the allowed ones, 0 elsewhere"""
    st = sets(np.asarray(rule_word), vocab, np.asarray(r))
    s, _ = scores(np.asarray(chroma, np.float32), st['A'], np.float64)
    a = np.where(st['tmpl'], s / float(np.float32(T)), -np.inf)
    p = np.exp(a - a.max())
    return p / p.sum()


def obeys(c, rule, vocab):
    """c [..., 36] decoded chords, rule int [...] -> bool [...]: the chord satisfies its rule word (yields included: where no root / no
    template / no chord tone could be allowed the fallback set is what must hold)"""
    c = np.asarray(c)
    ok = (c[..., 0:12] != 0).sum(-1) == 1
    ok &= (c[..., 24:36] != 0).sum(-1) == 1
    dr, db = (c[..., 0:12] != 0).argmax(-1), (c[..., 24:36] != 0).argmax(-1)
    bits = (c[..., 12:24] != 0).astype(np.int64)
    st = sets(rule, vocab, dr, bits)
    ok &= np.take_along_axis(st['root'], dr[..., None], -1)[..., 0]
    plain = ((bits == 0) | st['bit_free'] | st['bit_one']).all(-1) & ((bits != 0) | ~st['bit_one']).all(-1)
    dv = template_of(bits, st['A'])
    in_vocab = (dv >= 0) & np.take_along_axis(st['tmpl'], np.maximum(dv, 0)[..., None], -1)[..., 0] if st['A'].shape[-1] else False
    ok &= np.where(st['use_vocab'], in_vocab, plain)
    ok &= np.take_along_axis(st['bass'], db[..., None], -1)[..., 0]
    return ok
