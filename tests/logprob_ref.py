"""numpy restatement of the log-probabilities of a free-running decode (csrc/decode_score.hip; include/ptvae_hip.h "Log-probabilities of a
free-running decode"): which decisions of a decided grid count, and for each the model's own log-probability (logp) and the
log-probability under the distribution the decode drew from (logq).

The kept set of a pitch row is an INPUT here (bool [B, 32, 15, 130]: allowed and kept): kept_sets() computes it from the restatements of
the decoder's rules (tests/constrain_ref.py over tests/nucleus_ref.py / tests/trunc_ref.py), or the device reports it
(ptv_debug_pitch_constrain) -- the arithmetic below is then judged apart from the select.

Shapes are the API's: x int64 [B, 32, 16, 6] (slot 0 <sos>), pitch [B, 32, 15, 130], dur [B, 32, 15, 5, 2]; force_pitch int [15, 32 B] /
force_dur int [5, 480 B] are step-major (row t*B + b of plane n; row n*32B + t*B + b of plane d), >= 0 = forced.
logprob(..., dtype=np.float64) is the reference, dtype=np.float32 the same formulas with every operation rounded to fp32 in the
kernel's order of the terms (ascending n; a note's pitch term, then its bits ascending): the measure of what fp32 can be asked to give."""
import numpy as np

import constrain_ref as CR
import trunc_ref as TR

NP_ = 130
EOS = 129


def step_len(col):
    """pitches of the 16 slots of one time step -> L: the first slot in 1..15 holding <eos>, else 15 (ptv_keep_force_build's rule)"""
    for s in range(1, 16):
        if int(col[s]) == EOS:
            return s
    return 15


def counted(x):
    """-> (pc bool [B, 32, 15], bc bool [B, 32, 15, 5], err int32 [B]): the pitch decisions and duration bits that count.  n < L; a pitch
    outside 0..129 names no class: skipped, bit 0 of err; bits count for the counted notes with pitch < 128 and a value of 0 or 1"""
    x = np.asarray(x)
    B = x.shape[0]
    pc, bc, err = np.zeros((B, 32, 15), bool), np.zeros((B, 32, 15, 5), bool), np.zeros(B, np.int32)
    for b in range(B):
        for t in range(32):
            L = step_len(x[b, t, :, 0])
            for n in range(L):
                p = int(x[b, t, n + 1, 0])
                if not 0 <= p < NP_:
                    err[b] |= 1
                    continue
                pc[b, t, n] = True
                if p < 128:
                    for d in range(5):
                        bc[b, t, n, d] = int(x[b, t, n + 1, 1 + d]) in (0, 1)
    return pc, bc, err


def running_lo(x):
    """[B, 32, 15]: the largest pitch in 0..127 decided BEFORE each note step of the time step, -1 if none (pitch_lo_next)"""
    p = np.asarray(x)[:, :, 1:, 0]
    return CR.running_lo(np.where((p >= 0) & (p < 128), p, 128))


def kept_sets(pitch, x, T, top_k=None, ln_min_p=TR.LN_MIN_P_OFF, q=0, mask=None, ascending=False):
    """bool [B, 32, 15, 130]: the classes the decode drew from at every note step, by the restated rules.  mask: int32 [B, 32, 4] / [1, 32, 4]"""
    pitch = np.asarray(pitch, np.float32)
    B = pitch.shape[0]
    m = None if mask is None else np.broadcast_to(np.asarray(mask, np.int32)[:, :, None, :], (B, 32, 15, 4))
    al = CR.allowed(m, running_lo(x), ascending, shape=(B, 32, 15))
    if T <= 0:
        return al
    return CR.keep_mask(pitch, al, np.float32(T), top_k, ln_min_p, q)


def _lse(v, dt):
    """(max, log sum exp(v - max)) of a 1-d array in dtype dt"""
    m = v.max()
    return m, dt(np.log(np.exp((v - m).astype(dt)).astype(dt).sum(dtype=dt)))


def logp_row(v, d, dt=np.float64):
    """log softmax(v)[d] over every class of the 1-d row v"""
    v = np.asarray(v).astype(dt)
    m, ls = _lse(v, dt)
    return dt(dt(v[d] - m) - ls)


def logq_row(v, kept, T, d, dt=np.float64):
    """log softmax((v - m) / T)[d] over the kept classes (bool mask) of the row, m their maximum; d must be kept"""
    v, k = np.asarray(v).astype(dt), np.asarray(kept, bool)
    assert k[d]
    mk = v[k].max()
    a = ((v[k] - mk).astype(dt) / dt(T)).astype(dt)
    return dt(dt(dt(v[d] - mk) / dt(T)) - dt(np.log(np.exp(a).astype(dt).sum(dtype=dt))))


def logprob(pitch, dur, x, kept=None, Tp=0.0, Td=0.0, force_pitch=None, force_dur=None, dtype=np.float64):
    """-> (step_logp [B, 32, 4] = (logp pitch, logp dur, logq pitch, logq dur), step_counts int32 [B, 32, 4] = (pitch_n, dur_n,
    forced_pitch_n, forced_dur_n), err int32 [B], scale float64 [B, 32, 4] = the sum of the |terms| of every element).
    kept None: every class (no constraint, no truncation).  Tp / Td = 0 (or an argmax decode): logq = 0.  Uncounted rows and bits are
    never read: they may hold NaN."""
    dt = dtype
    x = np.asarray(x)
    B = x.shape[0]
    R = 32 * B
    pitch, dur = np.asarray(pitch, np.float32).astype(dt), np.asarray(dur, np.float32).astype(dt)
    Tp_, Td_ = dt(np.float32(Tp)), dt(np.float32(Td))
    pc, bc, err = counted(x)
    lp = np.zeros((B, 32, 4), dt)
    scale = np.zeros((B, 32, 4))
    cn = np.zeros((B, 32, 4), np.int32)

    def add(b, t, col, term):
        lp[b, t, col] = dt(lp[b, t, col] + term)
        scale[b, t, col] += abs(float(term))

    with np.errstate(invalid='ignore', divide='ignore'):
        for b in range(B):
            for t in range(32):
                for n in range(15):
                    if not pc[b, t, n]:
                        continue
                    r = t * B + b
                    d_ = int(x[b, t, n + 1, 0])
                    v = pitch[b, t, n]
                    add(b, t, 0, logp_row(v, d_, dt))
                    cn[b, t, 0] += 1
                    forced = force_pitch is not None and int(force_pitch[n][r]) >= 0
                    if forced:
                        cn[b, t, 2] += 1
                    elif Tp_ > 0:
                        k = np.ones(NP_, bool) if kept is None else np.asarray(kept[b, t, n], bool)
                        if not k[d_]:
                            err[b] |= 1
                            add(b, t, 2, dt(0))
                        else:
                            add(b, t, 2, logq_row(v, k, Tp_, d_, dt))
                    for d in range(5):
                        if not bc[b, t, n, d]:
                            continue
                        c = int(x[b, t, n + 1, 1 + d])
                        pair = dur[b, t, n, d]
                        add(b, t, 1, logp_row(pair, c, dt))
                        cn[b, t, 1] += 1
                        if force_dur is not None and int(force_dur[d][n * R + r]) >= 0:
                            cn[b, t, 3] += 1
                        elif Td_ > 0:
                            add(b, t, 3, logp_row((pair / Td_).astype(dt), c, dt))
    return lp, cn, err, scale


def fold(step_logp, step_counts, dtype=np.float64):
    """the sums over t = 0..31 in ascending order -> ([B, 4], int [B, 4])"""
    s = np.zeros((step_logp.shape[0], 4), dtype)
    for t in range(32):
        s = (s + np.asarray(step_logp)[:, t].astype(dtype)).astype(dtype)
    return s, np.asarray(step_counts, np.int64).sum(1)


def best_of(score):
    """score [n, B] -> (best int32 [B], err int32 [B]): the first maximal k, a NaN never wins; all NaN: k = 0 and err = 2"""
    score = np.asarray(score)
    n, B = score.shape
    best, err = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        kb = -1
        for k in range(n):
            s = score[k, b]
            if s != s:
                continue
            if kb < 0 or s > score[kb, b]:
                kb = k
        best[b], err[b] = max(kb, 0), 2 if kb < 0 else 0
    return best, err
