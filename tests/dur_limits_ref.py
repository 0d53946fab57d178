"""numpy restatement of the duration limits of the free-running decode (include/ptvae_hip.h "Duration limits", INTEGRATION.md "Duration
limits").

A note's duration is D = v + 1, v the value of its five duration bits, bit 0 the most significant.  A range word of force_dur,
word(lo, hi) = -1024 - (lo | hi << 5) with 0 <= lo <= hi <= 31, leaves the decision free and keeps v in [lo, hi]: bit d may take value b
after the prefix p (the value of bits 0..d-1) iff some v with those d + 1 leading bits lies in [lo, hi].  One value allowed: that is the
decision; both or neither: the bit is decided as without the word.  A word >= 0 overrides.
The builder: lo / hi bytes [rows, 32] in durations 1..32 (rows 1 or B, each its own), steps bytes [rows, 32]; per (b, t) H = hi clamped into
1..32, F = max(lo, 1), L = min(F, H) (the ceiling wins; yielded = the step is selected and F > H); at a selected step every decision whose
five source words are all negative gets word(L - 1, H - 1) in all five planes; every other word is the source's (-1 without a source).
Written with plain loops on purpose: it shares no code and no vectorised trick with the kernels or the tests' own bookkeeping."""
import numpy as np

BASE = -1024


def word(lo, hi):
    assert 0 <= lo <= hi <= 31
    return BASE - (lo | (hi << 5))


def unword(w):
    """(lo, hi) of a range word, None for any other word"""
    r = BASE - int(w)
    if r < 0 or r > 1023 or (r & 31) > (r >> 5):
        return None
    return r & 31, r >> 5


def completions(d, p, b):
    """every 5-bit value whose bits 0..d-1 have the value p and whose bit d is b"""
    lead = (2 * p + b) << (4 - d)
    return [lead + rest for rest in range(1 << (4 - d))]


def allowed(w, d, p):
    """(value 0 allowed, value 1 allowed); a word that is no range word allows both"""
    r = unword(w)
    if r is None:
        return True, True
    lo, hi = r
    return tuple(any(lo <= v <= hi for v in completions(d, p, b)) for b in (0, 1))


def decide(w, d, p, decided):
    """the decision of bit d: a word >= 0; else the one allowed value; else `decided` (the first maximum of logit + T g)"""
    if w >= 0:
        return int(w)
    a0, a1 = allowed(w, d, p)
    if a0 != a1:
        return 1 if a1 else 0
    return int(decided)


def determined(w, d, p):
    """the word decides the bit whatever the model prefers (a forced bit, or exactly one allowed value)"""
    if w >= 0:
        return True
    a0, a1 = allowed(w, d, p)
    return a0 != a1


def table():
    """the whole brute-force table: every range, bit and prefix -> list of (word, d, p)"""
    out = []
    for lo in range(32):
        for hi in range(lo, 32):
            for d in range(5):
                for p in range(1 << d):
                    out.append((word(lo, hi), d, p))
    return out


FITS = {'segment': lambda t: 32 - t, 'bar': lambda t: 16 - t % 16, 'beat': lambda t: 4 - t % 4}


def fit_row(fit):
    return [FITS[fit](t) for t in range(32)]


def rows_matrix(a, B):
    a = np.asarray(a)
    assert a.ndim == 2 and a.shape[1] == 32 and a.shape[0] in (1, B), a.shape
    out = np.zeros((B, 32), dtype=np.int64)
    for b in range(B):
        for t in range(32):
            out[b, t] = int(a[0 if a.shape[0] == 1 else b, t])
    return out


def build(lo, hi, steps, B, src_pitch=None, src_dur=None):
    """-> dict(pitch int32 [15, 32 B], dur int32 [5, 480 B], yielded int32 [B, 32], lo / hi int [B, 32]: the range in bit values 0..31 that
    acts at a selected step, -1 elsewhere, limited bool [B, 32, 15]: the decisions that got the word)"""
    lo, hi, steps = rows_matrix(lo, B), rows_matrix(hi, B), rows_matrix(steps, B)
    R, M = 32 * B, 15 * 32 * B
    pitch = np.full((15, R), -1, dtype=np.int32) if src_pitch is None else np.array(src_pitch, dtype=np.int32, copy=True)
    dur = np.full((5, M), -1, dtype=np.int32) if src_dur is None else np.array(src_dur, dtype=np.int32, copy=True)
    assert pitch.shape == (15, R) and dur.shape == (5, M)
    yielded = np.zeros((B, 32), dtype=np.int32)
    lo_v = np.full((B, 32), -1, dtype=np.int64)
    hi_v = np.full((B, 32), -1, dtype=np.int64)
    limited = np.zeros((B, 32, 15), dtype=bool)
    for b in range(B):
        for t in range(32):
            if not steps[b, t]:
                continue
            H = min(max(int(hi[b, t]), 1), 32)
            F = max(int(lo[b, t]), 1)
            L = min(F, H)
            if F > H:
                yielded[b, t] = 1
            lo_v[b, t], hi_v[b, t] = L - 1, H - 1
            for n in range(15):
                i = n * R + t * B + b
                if all(dur[d, i] < 0 for d in range(5)):
                    for d in range(5):
                        dur[d, i] = word(L - 1, H - 1)
                    limited[b, t, n] = True
    return dict(pitch=pitch, dur=dur, yielded=yielded, lo=lo_v, hi=hi_v, limited=limited)


def value(bits):
    v = 0
    for x in bits:
        v = 2 * v + int(x)
    return v
