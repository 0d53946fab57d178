"""numpy restatement of the kept-rhythm rule of the free-running decode (include/ptvae_hip.h "Kept rhythm", INTEGRATION.md "Kept rhythm").

The builder: x int64 [B, 32, 16, 6] as in keep_ref, mode uint8 [rows, 32], rows 1 or B, per (b, t): 0 = free; 1 = the whole step is kept
(keep_ref's rule); 3 = the rhythm is kept: L = the first slot 1..15 holding <eos>, else 15; K = L - 1 notes, or 15 where the step holds no
<eos>.  Pitch words n < K are NOT_EOS (-2: free, but not <eos>), word K (K < 15) is 129; duration words of n < K are x's bits where they are
0 / 1 unless durations is False; everything else -1.  A slot 1..K whose pitch is outside 0..127 sets bit 0 of err[b] and still counts.  Any
other byte: free, bit 1 of err[b].
The decision: constrain_ref.decide_pitch over the allowed set from which <eos> has been taken iff the word is -2 and another class is allowed.
Written with plain loops on purpose: it shares no code and no vectorised trick with the kernels or the tests' own bookkeeping."""
import numpy as np

import constrain_ref as CR
import keep_ref
import trunc_ref as TR

EOS = 129
NOT_EOS = -2


def mode_matrix(mode, B):
    a = np.asarray(mode)
    assert a.ndim == 2 and a.shape[1] == 32 and a.shape[0] in (1, B), a.shape
    out = np.zeros((B, 32), dtype=np.int64)
    for b in range(B):
        for t in range(32):
            out[b, t] = int(a[0 if a.shape[0] == 1 else b, t])
    return out


def note_count(col):
    """K of one rhythm step from its pitch column [16]"""
    for s in range(1, 16):
        if col[s] == EOS:
            return s - 1
    return 15


def build(x, mode, durations=True):
    """-> dict(pitch int32 [15, 32 B], dur int32 [5, 480 B], kept_n int32 [B, 32], err int32 [B], forced_pitch bool [B, 32, 15] (words >= 0),
    forced_dur bool [B, 32, 15, 5], not_eos bool [B, 32, 15] (words -2), K int [B, 32]: the notes of a rhythm step, -1 elsewhere)"""
    x = np.asarray(x)
    B = x.shape[0]
    assert x.shape == (B, 32, 16, 6)
    mode = mode_matrix(mode, B)
    R, M = 32 * B, 15 * 32 * B
    pitch = np.full((15, R), -1, dtype=np.int32)
    dur = np.full((5, M), -1, dtype=np.int32)
    kept_n = np.zeros((B, 32), dtype=np.int32)
    err = np.zeros(B, dtype=np.int32)
    fp = np.zeros((B, 32, 15), dtype=bool)
    fd = np.zeros((B, 32, 15, 5), dtype=bool)
    ne = np.zeros((B, 32, 15), dtype=bool)
    Ks = np.full((B, 32), -1, dtype=np.int64)
    for b in range(B):
        for t in range(32):
            m = int(mode[b, t])
            if m == 0:
                continue
            if m not in (1, 3):
                err[b] |= 2
                continue
            if m == 1:
                L = keep_ref.step_len(x[b, t, :, 0])
                for n in range(L):
                    p = int(x[b, t, n + 1, 0])
                    if 0 <= p <= 129:
                        pitch[n, t * B + b] = p
                        fp[b, t, n] = True
                        kept_n[b, t] += 1
                    else:
                        err[b] |= 1
                nd = L
            else:
                K = note_count(x[b, t, :, 0])
                Ks[b, t] = K
                kept_n[b, t] = K
                for n in range(K):
                    pitch[n, t * B + b] = NOT_EOS
                    ne[b, t, n] = True
                    p = int(x[b, t, n + 1, 0])
                    if p < 0 or p > 127:
                        err[b] |= 1
                if K < 15:
                    pitch[K, t * B + b] = EOS
                    fp[b, t, K] = True
                nd = K if durations else 0
            for n in range(nd):
                for d in range(5):
                    v = int(x[b, t, n + 1, 1 + d])
                    if v in (0, 1):
                        dur[d, n * R + t * B + b] = v
                        fd[b, t, n, d] = True
    return dict(pitch=pitch, dur=dur, kept_n=kept_n, err=err, forced_pitch=fp, forced_dur=fd, not_eos=ne, K=Ks)


def allowed(al, words):
    """al bool [..., 130] (constrain_ref.allowed), words int [...] -> al with <eos> cleared where the word is NOT_EOS and another class is
    allowed (the fallback: <eos> stays where it is the only one)"""
    al = np.array(al, dtype=bool, copy=True)
    words = np.broadcast_to(np.asarray(words), al.shape[:-1])
    others = al.copy()
    others[..., EOS] = False
    drop = (words == NOT_EOS) & others.any(-1)
    al[..., EOS] &= ~drop
    return al


def fallback(al, words):
    """bool [...]: the word is NOT_EOS but nothing except <eos> is allowed -- the decision is <eos> and the step ends short"""
    al = np.asarray(al, dtype=bool)
    others = al.copy()
    others[..., EOS] = False
    return (np.broadcast_to(np.asarray(words), al.shape[:-1]) == NOT_EOS) & ~others.any(-1)


def keep_mask(logits, al, words, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    return CR.keep_mask(logits, allowed(al, words), T, top_k, ln_min_p, q)


def threshold(logits, al, words, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    return CR.threshold(logits, allowed(al, words), T, top_k, ln_min_p, q)


def decide_pitch(logits, noise, al, words, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """the decision of a row: a word >= 0 is the decision; else constrain_ref.decide_pitch over the reduced allowed set"""
    words = np.broadcast_to(np.asarray(words), np.shape(logits)[:-1])
    free = CR.decide_pitch(logits, noise, allowed(al, words), T, top_k, ln_min_p, q)
    return np.where(words >= 0, words, free)


def skippable(logits, noise, al, words, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    return CR.skippable(logits, noise, allowed(al, words), T, top_k, ln_min_p, q)
