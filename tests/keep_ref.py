"""numpy restatement of the kept-steps rule of the free-running decode (include/ptvae_hip.h "Kept steps", INTEGRATION.md "Kept steps").

A keep is a grid x int64 [B, 32, 16, 6] (slot 0 <sos>, pitches 0..127, <eos> 129, <pad> 130; duration bits 0 / 1, 2 = pad) and a step
selection steps [B, 32] or [1, 32].  For a kept (b, t): L = the first slot s in 1..15 with x[b, t, s, 0] == 129, else 15; for the note
steps n < L (slot n + 1) the pitch decision is forced to x[b, t, n + 1, 0] where that lies in 0..129 (else it stays free and bit 0 of
err[b] is set) and duration decision d to x[b, t, n + 1, 1 + d] where that is 0 or 1 (else free); note steps n >= L and steps not kept
are free.  Force arrays: pitch int32 [15, 32 B] (row t * B + b), dur int32 [5, 480 B] (row n * 32 B + t * B + b), -1 = free.
Written with plain loops on purpose: it shares no code and no vectorised trick with the kernel or the tests' own bookkeeping."""
import numpy as np

EOS = 129


def steps_matrix(steps, B):
    """bool [B, 32] of a selection: a [B, 32] / [1, 32] array, an iterable of step indices or a slice"""
    if isinstance(steps, slice):
        steps = range(*steps.indices(32))
    if isinstance(steps, np.ndarray) and steps.ndim == 2:
        assert steps.shape[1] == 32 and steps.shape[0] in (1, B)
        return np.broadcast_to(steps != 0, (B, 32)).copy()
    row = np.zeros(32, dtype=bool)
    for t in steps:
        assert 0 <= int(t) < 32
        row[int(t)] = True
    return np.broadcast_to(row, (B, 32)).copy()


def step_len(col):
    """L of one kept step from its pitch column [16]"""
    for s in range(1, 16):
        if col[s] == EOS:
            return s
    return 15


def build(x, steps):
    """-> dict(pitch int32 [15, 32 B], dur int32 [5, 480 B], err int32 [B], forced_pitch bool [B, 32, 15], forced_dur bool [B, 32, 15, 5],
    L int [B, 32] (0 where the step is not kept))"""
    x = np.asarray(x)
    B = x.shape[0]
    assert x.shape == (B, 32, 16, 6)
    st = steps_matrix(steps, B)
    R, M = 32 * B, 15 * 32 * B
    pitch = np.full((15, R), -1, dtype=np.int32)
    dur = np.full((5, M), -1, dtype=np.int32)
    err = np.zeros(B, dtype=np.int32)
    fp = np.zeros((B, 32, 15), dtype=bool)
    fd = np.zeros((B, 32, 15, 5), dtype=bool)
    Ls = np.zeros((B, 32), dtype=np.int64)
    for b in range(B):
        for t in range(32):
            if not st[b, t]:
                continue
            L = step_len(x[b, t, :, 0])
            Ls[b, t] = L
            for n in range(L):
                p = int(x[b, t, n + 1, 0])
                if 0 <= p <= 129:
                    pitch[n, t * B + b] = p
                    fp[b, t, n] = True
                else:
                    err[b] |= 1
                for d in range(5):
                    v = int(x[b, t, n + 1, 1 + d])
                    if v in (0, 1):
                        dur[d, n * R + t * B + b] = v
                        fd[b, t, n, d] = True
    return dict(pitch=pitch, dur=dur, err=err, forced_pitch=fp, forced_dur=fd, L=Ls)
