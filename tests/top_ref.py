"""numpy restatement of the kept-top-voice rule of the free-running decode (include/ptvae_hip.h "Kept top voice", INTEGRATION.md "Kept top
voice").

The builder: x int64 [B, 32, 16, 6] as in keep_ref, mode uint8 [rows, 32], rows 1 or B, per (b, t): 0 = free; 1 = the whole step is kept
(keep_ref's rule); 4 = the top of the step is kept: K = the notes before the first <eos> (15 without one); the kept notes are the last h:
from slot K downwards, stop at h == highest, at a pitch outside 0..127, at the first pitch < above (both limits None: highest = 1).  J = K - h.
Pitch words n < J are BELOW(u_n) = -256 - u_n, u_n clamped into 1..128: lanes -- the pitch of the next note of x (128 behind the last);
room -- the lowest kept pitch (128 without one) less (J - 1 - n).  Words J..K-1 are x's pitches, word K (K < 15) is 129.  Duration words: x's
bits where 0 / 1 for n < K (durations True), for J <= n < K ('kept'), nowhere (False).  Bit 0 of err[b]: a slot 1..K of a top step holds no
note, or a pitch not above the slot before it.  Any other mode byte: free, bit 1 of err[b].
The allowed rule with a ceiling word: lane = notes c < u (ascending: also c > lo); allowed = lane & mask, else lane, else {<eos>}.
The decision: constrain_ref.decide_pitch over that set.
Written with plain loops on purpose: it shares no code and no vectorised trick with the kernels or the tests' own bookkeeping."""
import numpy as np

import constrain_ref as CR
import keep_ref
import rhythm_ref as RR
import trunc_ref as TR

EOS = 129
BELOW_BASE = -256


def below(u):
    return BELOW_BASE - u


def ceiling_of(word):
    """the ceiling u of a BELOW word, None for every other word"""
    u = BELOW_BASE - int(word)
    return u if 1 <= u <= 128 else None


def limit_matrix(v, B, default):
    """a limit (None, an int, or an array [rows, 32], rows 1 or B) -> int [B, 32]"""
    out = np.zeros((B, 32), dtype=np.int64)
    if v is None:
        out[:] = default
        return out
    a = np.asarray(v)
    if a.ndim == 0:
        out[:] = int(a)
        return out
    assert a.ndim == 2 and a.shape[1] == 32 and a.shape[0] in (1, B), a.shape
    for b in range(B):
        for t in range(32):
            out[b, t] = int(a[0 if a.shape[0] == 1 else b, t])
    return out


def suffix_len(col, K, above, highest):
    """h of one top step from its pitch column [16]: the kept notes are slots K - h + 1 .. K"""
    above = min(max(int(above), 0), 128)
    highest = min(max(int(highest), 0), 15)
    h = 0
    for s in range(K, 0, -1):
        if h == highest:
            break
        p = int(col[s])
        if p < 0 or p > 127:
            break
        if p < above:
            break
        h += 1
    return h


def step_err(col, K):
    e = 0
    for s in range(1, K + 1):
        p = int(col[s])
        if p < 0 or p > 127:
            e = 1
        if s >= 2 and p <= int(col[s - 1]):
            e = 1
    return e


def clamp_u(u):
    return 1 if u < 1 else (128 if u > 128 else int(u))


def ceilings(col, K, h, lanes):
    """the J = K - h ceilings of one top step"""
    J = K - h
    out = []
    for n in range(J):
        if lanes:
            u = int(col[n + 2]) if n + 1 < K else 128
        else:
            u = (int(col[J + 1]) if J < K else 128) - (J - 1 - n)
        out.append(clamp_u(u))
    return out


def build(x, mode, above=None, highest=None, durations=True, lanes=True):
    """-> dict(pitch int32 [15, 32 B], dur int32 [5, 480 B], kept_n int32 [B, 32], err int32 [B], forced_pitch bool [B, 32, 15] (words >= 0),
    forced_dur bool [B, 32, 15, 5], ceil int [B, 32, 15] (the ceiling of a BELOW word, 0 elsewhere), K, h int [B, 32] (-1 off the top steps))"""
    assert durations in (True, False, 'kept')
    x = np.asarray(x)
    B = x.shape[0]
    assert x.shape == (B, 32, 16, 6)
    mode = RR.mode_matrix(mode, B)
    both_none = above is None and highest is None
    ab = limit_matrix(above, B, 0)
    hi = limit_matrix(highest, B, 1 if both_none else 15)
    R, M = 32 * B, 15 * 32 * B
    pitch = np.full((15, R), -1, dtype=np.int32)
    dur = np.full((5, M), -1, dtype=np.int32)
    kept_n = np.zeros((B, 32), dtype=np.int32)
    err = np.zeros(B, dtype=np.int32)
    fp = np.zeros((B, 32, 15), dtype=bool)
    fd = np.zeros((B, 32, 15, 5), dtype=bool)
    ce = np.zeros((B, 32, 15), dtype=np.int64)
    Ks = np.full((B, 32), -1, dtype=np.int64)
    hs = np.full((B, 32), -1, dtype=np.int64)
    for b in range(B):
        for t in range(32):
            m = int(mode[b, t])
            if m == 0:
                continue
            if m not in (1, 4):
                err[b] |= 2
                continue
            col = x[b, t, :, 0]
            if m == 1:
                L = keep_ref.step_len(col)
                for n in range(L):
                    p = int(col[n + 1])
                    if 0 <= p <= 129:
                        pitch[n, t * B + b] = p
                        fp[b, t, n] = True
                        kept_n[b, t] += 1
                    else:
                        err[b] |= 1
                d0, d1 = 0, L
            else:
                K = RR.note_count(col)
                h = suffix_len(col, K, ab[b, t], hi[b, t])
                J = K - h
                Ks[b, t], hs[b, t], kept_n[b, t] = K, h, h
                err[b] |= step_err(col, K)
                for n, u in enumerate(ceilings(col, K, h, lanes)):
                    pitch[n, t * B + b] = below(u)
                    ce[b, t, n] = u
                for n in range(J, K):
                    pitch[n, t * B + b] = int(col[n + 1])
                    fp[b, t, n] = True
                if K < 15:
                    pitch[K, t * B + b] = EOS
                    fp[b, t, K] = True
                d0, d1 = (0, K) if durations is True else ((J, K) if durations == 'kept' else (0, 0))
            for n in range(d0, d1):
                for d in range(5):
                    v = int(x[b, t, n + 1, 1 + d])
                    if v in (0, 1):
                        dur[d, n * R + t * B + b] = v
                        fd[b, t, n, d] = True
    return dict(pitch=pitch, dur=dur, kept_n=kept_n, err=err, forced_pitch=fp, forced_dur=fd, ceil=ce, K=Ks, h=hs)


def put_notes(dst, src, s0, cnt):
    for j in range(1, cnt + 1):
        dst[j] = src[s0 + j - 1]
    if cnt < 15:
        dst[cnt + 1] = (EOS, 2, 2, 2, 2, 2)
    for j in range(cnt + 2, 16):
        dst[j] = (130, 2, 2, 2, 2, 2)


def split(x, mode, above=None, highest=None):
    """-> (voice, rest int64 [B, 32, 16, 6], kept_n int32 [B, 32]): a top step's kept notes / the notes under them, each followed by
    <eos> and <pad>; a whole step goes to voice, a free step to rest, the other grid gets the empty step; slot 0 is x's"""
    x = np.asarray(x)
    B = x.shape[0]
    r = build(x, mode, above, highest)
    modem = RR.mode_matrix(mode, B)
    voice, rest = np.zeros_like(x), np.zeros_like(x)
    for b in range(B):
        for t in range(32):
            voice[b, t, 0] = x[b, t, 0]
            rest[b, t, 0] = x[b, t, 0]
            m = int(modem[b, t])
            if m == 4:
                K, h = int(r['K'][b, t]), int(r['h'][b, t])
                put_notes(voice[b, t], x[b, t], K - h + 1, h)
                put_notes(rest[b, t], x[b, t], 1, K - h)
            else:
                whole, empty = (voice, rest) if m == 1 else (rest, voice)
                whole[b, t, 1:] = x[b, t, 1:]
                put_notes(empty[b, t], x[b, t], 1, 0)
    return voice, rest, r['kept_n']


# ---- the allowed rule with a force word ---------------------------------------------------------------------------------------------
def allowed_row(mask_row, lo, ascending, word):
    """ONE row, one class at a time: (list of 130 bools, relaxed, empty_lane).  mask_row: 128 bools or None"""
    u = ceiling_of(word)
    if u is None:
        base = [True] * 130
        for c in range(130):
            if mask_row is not None and c < 128:
                base[c] = bool(mask_row[c])
            if ascending:
                base[c] = base[c] and (c == EOS or (c < 128 and c > lo))
        if int(word) == RR.NOT_EOS and any(base[c] for c in range(130) if c != EOS):
            base[EOS] = False
        return base, False, False
    lane = [c < 128 and c < u and (not ascending or c > lo) for c in range(130)]
    inter = [lane[c] and (mask_row is None or bool(mask_row[c])) for c in range(128)] + [False, False]
    if any(inter):
        return inter, False, False
    if any(lane):
        return lane, True, False
    return [c == EOS for c in range(130)], False, True


def allowed(mask, lo, ascending, words):
    """mask: int32 [N, 4] or None; lo int [N]; words int [N] -> (al bool [N, 130], relaxed bool [N], empty_lane bool [N])"""
    words = np.asarray(words)
    N = words.shape[0]
    bits = None if mask is None else CR.mask_bits(np.broadcast_to(np.asarray(mask), (N, 4)))
    lo = np.broadcast_to(np.asarray(-1 if lo is None else lo), (N,))
    al = np.zeros((N, 130), dtype=bool)
    rel = np.zeros(N, dtype=bool)
    emp = np.zeros(N, dtype=bool)
    for i in range(N):
        al[i], rel[i], emp[i] = allowed_row(None if bits is None else bits[i], int(lo[i]), ascending, int(words[i]))
    return al, rel, emp


def allowed_grid(mask, lo, ascending, words):
    """allowed() for a whole decode at once (array operations: the loops above take minutes on 15360 decisions; tests/test_top_ref_host.py
    holds this form to them).  mask: int32 [..., 4] or None; lo, words: int [...] -> (al bool [..., 130], relaxed, empty_lane bool [...])"""
    words = np.asarray(words).astype(np.int64)
    shape = words.shape
    lo = np.broadcast_to(np.asarray(-1 if lo is None else lo, dtype=np.int64), shape)
    if mask is not None:
        mask = np.broadcast_to(np.asarray(mask), shape + (4,))
    base = RR.allowed(CR.allowed(mask, lo, ascending, shape), words)
    u = BELOW_BASE - words
    ceil = (u >= 1) & (u <= 128)
    c = np.arange(130)
    lo_ = lo if ascending else np.full(shape, -1, dtype=np.int64)
    lane = (c < 128) & (c < u[..., None]) & (c > lo_[..., None])
    inter = lane.copy()
    if mask is not None:
        inter[..., :128] &= CR.mask_bits(mask)
    has_i, has_l = inter.any(-1), lane.any(-1)
    under = np.where(has_i[..., None], inter, np.where(has_l[..., None], lane, c == EOS))
    return np.where(ceil[..., None], under, base), ceil & ~has_i & has_l, ceil & ~has_l


def keep_mask(logits, al, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    return CR.keep_mask(logits, al, T, top_k, ln_min_p, q)


def decide_pitch(logits, noise, al, words, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """the decision of a row: a word >= 0 is the decision; else constrain_ref.decide_pitch over the allowed set of allowed()"""
    words = np.asarray(words)
    free = CR.decide_pitch(logits, noise, al, T, top_k, ln_min_p, q)
    return np.where(words >= 0, words, free)
