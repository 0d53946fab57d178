"""numpy restatement of the constrained free-running decode (pitch masks, ascending notes) over the noise (tests/sample_ref.py) and the
truncation rules (tests/trunc_ref.py, tests/nucleus_ref.py): include/ptvae_hip.h "Constrained decode", csrc/philox.hpp pitch_constrain().

For row b, time step t, note step n a class c in 0..129 is ALLOWED iff it passes every constraint that is on:
    pitch_mask  int32 [B, 32, 4]: bit p & 31 of word p >> 5 of [b, t] set = grid pitch p (0..127) allowed; 128 / 129 are not covered
    ascending   c < 128 is allowed iff c > lo, lo the largest pitch < 128 already decided in this time step (-1 at n = 0); 128 never
    <eos> (129) is always allowed
Constraints come first: a disallowed class enters the truncation rules as -inf (top_k counts the k best allowed classes, the nucleus
mass, Z and min_p's maximum are those of the allowed classes), and the decision is the first maximal index of logit + T * g over the
classes that are allowed and kept.  Everything is integer or the fp32 of the modules underneath: nothing new is rounded here.
"""
import numpy as np

import nucleus_ref as NR
import sample_ref as S
import trunc_ref as TR

NP_ = 130
SOS, EOS = 128, 129
FULL_MASK = np.full(4, -1, dtype=np.int32)


def mask_bits(mask):
    """int32 [..., 4] -> bool [..., 128]: the verdict of the mask on the grid pitches"""
    w = np.asarray(mask, dtype=np.int32).view(np.uint32)
    p = np.arange(128)
    return ((w[..., p >> 5] >> (p & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def mask_from_bits(bits):
    """bool [..., 128] -> int32 [..., 4]"""
    b = np.asarray(bits, dtype=bool).reshape(np.shape(bits)[:-1] + (4, 32)).astype(np.uint64)
    w = (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return w.view(np.int32)


def allowed(mask=None, lo=None, ascending=False, shape=()):
    """bool [..., 130].  mask: int32 [..., 4] or None (no mask); lo: int [...] (read under `ascending` only)"""
    if mask is not None:
        shape = np.shape(mask)[:-1]
    elif lo is not None:
        shape = np.shape(lo)
    al = np.ones(tuple(shape) + (NP_,), dtype=bool)
    if mask is not None:
        al[..., :128] = mask_bits(mask)
    if ascending:
        c = np.arange(NP_)
        lo = np.broadcast_to(np.asarray(lo, dtype=np.int64), shape)
        al &= (c == EOS) | ((c < 128) & (c > lo[..., None]))
    return al


def allowed_brute(mask_row, lo, ascending):
    """the definition, one class at a time: list of 130 bools for ONE row (mask_row: four ints or None)"""
    out = []
    for c in range(NP_):
        ok = True
        if mask_row is not None and c < 128:
            ok = ok and bool((int(mask_row[c >> 5]) & 0xFFFFFFFF) >> (c & 31) & 1)
        if ascending:
            ok = ok and (c == EOS or (c < 128 and c > lo))
        if c == EOS:
            assert ok
        out.append(ok)
    return out


def running_lo(pitch):
    """decisions int [..., N] along the note axis -> lo [..., N]: the largest pitch < 128 among the decisions BEFORE each note step, -1 if none"""
    p = np.asarray(pitch, dtype=np.int64)
    v = np.where(p < 128, p, -1)
    run = np.maximum.accumulate(v, axis=-1)
    return np.concatenate([np.full(p.shape[:-1] + (1,), -1, dtype=np.int64), run[..., :-1]], -1)


def constrained(logits, al):
    """the row as the truncation rules see it: disallowed classes at -inf"""
    return np.where(al, np.asarray(logits, dtype=np.float32), np.float32(-np.inf)).astype(np.float32)


def threshold(logits, al, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """fp32 [...]: the keep threshold of the allowed classes (-inf: no rule, or fewer than top_k allowed)"""
    with np.errstate(invalid='ignore'):
        return NR.threshold(constrained(logits, al), T, top_k, ln_min_p, q)


def keep_mask(logits, al, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """bool [..., 130]: allowed and kept -- the classes the draw runs over"""
    a = np.asarray(logits, dtype=np.float32)
    return al & (a >= threshold(a, al, T, top_k, ln_min_p, q)[..., None])


def decide_pitch(logits, noise, al, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """first maximal index over the allowed-and-kept classes of logit + T * g"""
    x = S.perturbed(logits, noise, T)
    return np.argmax(np.where(keep_mask(logits, al, T, top_k, ln_min_p, q), x, np.float32(-np.inf)), axis=-1)


def skippable(logits, noise, al, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0):
    """sample_ref.skippable among the allowed-and-kept classes"""
    keep = keep_mask(logits, al, T, top_k, ln_min_p, q)
    return S.skippable(np.where(keep, np.asarray(logits, dtype=np.float32), np.float32(-1e30)), noise, T, S.NOISE_TOL)


def mask_build(B=1, c=None, pitch_classes=0xFFF, lo=0, hi=127):
    """ptv_pitch_mask_build: int32 [B, 32, 4]; pitch p at step t passes iff lo <= p <= hi, bit p % 12 of pitch_classes is set and, with
    c (f32 [B, 8, 36]), c[b, t // 4, 12 + p % 12] != 0"""
    if c is not None:
        B = np.shape(c)[0]
    p = np.arange(128)
    ok = (p >= lo) & (p <= hi) & (((int(pitch_classes) >> (p % 12)) & 1) == 1)
    bits = np.broadcast_to(ok, (B, 32, 128)).copy()
    if c is not None:
        chroma = np.asarray(c)[:, np.arange(32) // 4, 12:24] != 0                          # [B, 32, 12]
        bits &= chroma[:, :, p % 12]
    return mask_from_bits(bits)
