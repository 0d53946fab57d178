"""numpy restatement of the kept-voices rule of the free-running decode (include/ptvae_hip.h "Kept voices", INTEGRATION.md "Kept voices").

x int64 [B, 32, 16, 6] as in keep_ref.  mode uint8 [rows, 32], rows 1 or B, per (b, t): 0 = free; 1 = the whole step is kept (keep_ref's
rule, <eos> included); 2 = the voice is kept: over the slots s = 1..15 with K = 0, in this order -- K == lowest: stop; p == 129: stop; p
outside 0..127: bit 0 of err[b], stop; p >= below: stop; else K += 1.  Pitch decisions n < K are forced to the slot's pitch, their duration
bits where they are 0 / 1 unless durations is False; the <eos> of a voice step is never forced.  Any other byte: free, bit 1 of err[b].
below / lowest: int [rows, 32] (each with its own rows in {1, B}) or a plain int or None (no limit), clamped to 0..128 / 0..15.
Written with plain loops on purpose: it shares no code and no vectorised trick with the kernels or the tests' own bookkeeping."""
import numpy as np

EOS, PAD = 129, 130


def per_step(a, B, none, lo, hi):
    """a limit or mode argument -> int array [B, 32], clamped to lo..hi"""
    if a is None:
        return np.full((B, 32), none, dtype=np.int64)
    a = np.asarray(a)
    if a.ndim == 0:
        a = np.full((1, 32), int(a))
    assert a.ndim == 2 and a.shape[1] == 32 and a.shape[0] in (1, B), a.shape
    out = np.zeros((B, 32), dtype=np.int64)
    for b in range(B):
        for t in range(32):
            out[b, t] = min(max(int(a[0 if a.shape[0] == 1 else b, t]), lo), hi)
    return out


def prefix_len(col, below, lowest):
    """(K, bad) of one voice step from its pitch column [16]"""
    K = 0
    for s in range(1, 16):
        if K == lowest:
            break
        p = int(col[s])
        if p == EOS:
            break
        if p < 0 or p > 127:
            return K, True
        if p >= below:
            break
        K += 1
    return K, False


def whole_len(col):
    for s in range(1, 16):
        if col[s] == EOS:
            return s
    return 15


def build(x, mode, below=None, lowest=None, durations=True):
    """-> dict(pitch int32 [15, 32 B], dur int32 [5, 480 B], kept_n int32 [B, 32], err int32 [B], forced_pitch bool [B, 32, 15],
    forced_dur bool [B, 32, 15, 5], K int [B, 32]: the kept prefix of a voice step, the L of a whole step, 0 of a free one)"""
    x = np.asarray(x)
    B = x.shape[0]
    assert x.shape == (B, 32, 16, 6)
    mode = per_step(mode, B, 0, 0, 255)
    below = per_step(below, B, 128, 0, 128)
    lowest = per_step(lowest, B, 15, 0, 15)
    R, M = 32 * B, 15 * 32 * B
    pitch = np.full((15, R), -1, dtype=np.int32)
    dur = np.full((5, M), -1, dtype=np.int32)
    kept_n = np.zeros((B, 32), dtype=np.int32)
    err = np.zeros(B, dtype=np.int32)
    fp = np.zeros((B, 32, 15), dtype=bool)
    fd = np.zeros((B, 32, 15, 5), dtype=bool)
    Ks = np.zeros((B, 32), dtype=np.int64)
    for b in range(B):
        for t in range(32):
            m = int(mode[b, t])
            if m == 0:
                continue
            if m not in (1, 2):
                err[b] |= 2
                continue
            if m == 1:
                K = whole_len(x[b, t, :, 0])
                bits = True
            else:
                K, bad = prefix_len(x[b, t, :, 0], int(below[b, t]), int(lowest[b, t]))
                if bad:
                    err[b] |= 1
                bits = bool(durations)
            Ks[b, t] = K
            for n in range(K):
                p = int(x[b, t, n + 1, 0])
                if 0 <= p <= 129:
                    pitch[n, t * B + b] = p
                    fp[b, t, n] = True
                    kept_n[b, t] += 1
                else:
                    assert m == 1
                    err[b] |= 1
                if not bits:
                    continue
                for d in range(5):
                    v = int(x[b, t, n + 1, 1 + d])
                    if v in (0, 1):
                        dur[d, n * R + t * B + b] = v
                        fd[b, t, n, d] = True
    return dict(pitch=pitch, dur=dur, kept_n=kept_n, err=err, forced_pitch=fp, forced_dur=fd, K=Ks)


def token(p):
    return np.array([p, 2, 2, 2, 2, 2], dtype=np.int64)


def empty_step(sos_slot):
    s = np.empty((16, 6), dtype=np.int64)
    s[0] = sos_slot
    s[1] = token(EOS)
    for j in range(2, 16):
        s[j] = token(PAD)
    return s


def split(x, mode, below=None, lowest=None):
    """-> (voice, rest) int64 [B, 32, 16, 6]: slot 0 as in x; a voice step: voice = the K kept slots, then <eos> (none when K = 15), rest =
    the slots K + 1 .. of x moved down to slot 1 up to and including the first <eos> (none in x: all of them and, while a slot is left, an
    <eos>); mode 1: voice = the step, rest = the empty step; anything else: the reverse.  Unused slots are <pad> with bits 2."""
    x = np.asarray(x)
    B = x.shape[0]
    mode = per_step(mode, B, 0, 0, 255)
    below = per_step(below, B, 128, 0, 128)
    lowest = per_step(lowest, B, 15, 0, 15)
    voice, rest = np.zeros_like(x), np.zeros_like(x)
    for b in range(B):
        for t in range(32):
            xs = x[b, t]
            m = int(mode[b, t])
            if m == 1:
                voice[b, t], rest[b, t] = xs, empty_step(xs[0])
            elif m != 2:
                voice[b, t], rest[b, t] = empty_step(xs[0]), xs
            else:
                K, _ = prefix_len(xs[:, 0], int(below[b, t]), int(lowest[b, t]))
                v = [xs[0]] + [xs[s] for s in range(1, K + 1)]
                if K < 15:
                    v.append(token(EOS))
                r = [xs[0]]
                ended = False
                for s in range(K + 1, 16):
                    r.append(xs[s])
                    if xs[s, 0] == EOS:
                        ended = True
                        break
                if not ended and len(r) < 16:
                    r.append(token(EOS))
                for lst, out in ((v, voice), (r, rest)):
                    while len(lst) < 16:
                        lst.append(token(PAD))
                    out[b, t] = np.stack(lst)
    return voice, rest
