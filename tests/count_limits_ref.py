"""numpy restatement of the note-count limits of the free-running decode (include/ptvae_hip.h "Note-count limits", INTEGRATION.md
"Note-count limits").

The builder: lo / hi bytes [rows, 32] in note counts (rows 1 or B, each its own), steps bytes [rows, 32]; the arrays of a keep to build
into, or none (every word -1).  Per selected (b, t): F = lo, H = hi, each clamped into 0..15, L = min(F, H) (the ceiling wins); w[n] the
15 source pitch words.  An OWNED step -- some w[n] is 129 or a negative word other than -1 -- is copied, yielded bit 1.  Otherwise J = 1 +
the index of the last w[n] >= 0 (0 with none), E = max(H, J); only words equal to -1 are replaced: n < L gets NOT_EOS (-2), or with room
BELOW(128 - (L - 1 - n)) = -256 - that ceiling; w[E] = 129 if E <= 14.  yielded: bit 0 F > H, bit 2 J > H, bit 3 room and 0 < J < L and the
prefix's last pitch p in 0..127 has p + 1 >= 128 - (L - 1 - J).  Unselected: copied, yielded 0.  Duration words are the source's.
Written with plain loops on purpose: it shares no code and no vectorised trick with the kernel or the tests' own bookkeeping."""
import numpy as np

EOS = 129
NOT_EOS = -2
BELOW_BASE = -256


def below(u):
    assert 1 <= u <= 128
    return BELOW_BASE - u


def ceiling_of(w):
    """u of a BELOW word, None for any other word"""
    u = BELOW_BASE - int(w)
    return u if 1 <= u <= 128 else None


def rows_matrix(a, B):
    a = np.asarray(a)
    assert a.ndim == 2 and a.shape[1] == 32 and a.shape[0] in (1, B), a.shape
    out = np.zeros((B, 32), dtype=np.int64)
    for b in range(B):
        for t in range(32):
            out[b, t] = int(a[0 if a.shape[0] == 1 else b, t])
    return out


def step(w, F, H, room):
    """one selected step: w the 15 source words -> (the 15 new words, yielded, L, H, E, J, owned) with F, H already clamped"""
    w = [int(v) for v in w]
    assert len(w) == 15 and 0 <= F <= 15 and 0 <= H <= 15
    L = F if F < H else H
    owned = False
    for v in w:
        if v == EOS or (v < 0 and v != -1):
            owned = True
    J = 0
    for n in range(15):
        if w[n] >= 0:
            J = n + 1
    E = H if H > J else J
    if owned:
        return list(w), 2, L, H, E, J, True
    out = list(w)
    for n in range(L):
        if w[n] == -1:
            out[n] = below(128 - (L - 1 - n)) if room else NOT_EOS
    if E <= 14 and w[E] == -1:
        out[E] = EOS
    y = 0
    if F > H:
        y |= 1
    if J > H:
        y |= 4
    if room and 0 < J < L:
        p = w[J - 1]
        if 0 <= p <= 127 and p + 1 >= 128 - (L - 1 - J):
            y |= 8
    return out, y, L, H, E, J, False


def build(lo, hi, steps, B, src_pitch=None, src_dur=None, room=False):
    """-> dict(pitch int32 [15, 32 B], dur int32 [5, 480 B], yielded int32 [B, 32], L / H / E / J int [B, 32] (-1 at an unselected step),
    owned bool [B, 32], selected bool [B, 32])"""
    lo, hi, steps = rows_matrix(lo, B), rows_matrix(hi, B), rows_matrix(steps, B)
    R, M = 32 * B, 15 * 32 * B
    pitch = np.full((15, R), -1, dtype=np.int32) if src_pitch is None else np.array(src_pitch, dtype=np.int32, copy=True)
    dur = np.full((5, M), -1, dtype=np.int32) if src_dur is None else np.array(src_dur, dtype=np.int32, copy=True)
    assert pitch.shape == (15, R) and dur.shape == (5, M)
    yielded = np.zeros((B, 32), dtype=np.int32)
    per = {k: np.full((B, 32), -1, dtype=np.int64) for k in 'LHEJ'}
    owned = np.zeros((B, 32), dtype=bool)
    selected = np.zeros((B, 32), dtype=bool)
    for b in range(B):
        for t in range(32):
            if not steps[b, t]:
                continue
            selected[b, t] = True
            F = min(max(int(lo[b, t]), 0), 15)
            H = min(max(int(hi[b, t]), 0), 15)
            r = t * B + b
            new, y, L, H, E, J, own = step([pitch[n, r] for n in range(15)], F, H, room)
            for n in range(15):
                pitch[n, r] = new[n]
            yielded[b, t] = y
            per['L'][b, t], per['H'][b, t], per['E'][b, t], per['J'][b, t] = L, H, E, J
            owned[b, t] = own
    return dict(pitch=pitch, dur=dur, yielded=yielded, L=per['L'], H=per['H'], E=per['E'], J=per['J'], owned=owned, selected=selected)


def words_of(pitch):
    """the pitch words [15, 32 B] as [B, 32, 15]"""
    n = pitch.shape[1] // 32
    return pitch.reshape(15, 32, n).transpose(2, 1, 0)
