"""Plain fp64 references (numpy, CPU) of the per-sample score kernels of csrc/score.hip, written from the definitions of
include/ptvae_hip.h ("Per-sample scores") -- the oracle side of tests/test_gpu_score_kernels.py / test_gpu_score_model.py, itself guarded
by tests/test_score_ref_host.py.  Logits come in API shapes (batch-major); every function widens to float64, integer outputs are int64.
Ignored rows and bits are EXCLUDED by indexing, never multiplied by zero: a NaN in one cannot reach a result."""
import numpy as np

F8 = np.float64
COUNT_NAMES = ('pitch_n', 'pitch_hit', 'dur_n', 'dur_hit', 'note_n', 'note_hit')


def _nll_rows(logits, targets):
    """logits [rows, C] (all rows live), targets [rows] -> (-log softmax(logits)[target], first arg-max)"""
    logits = np.asarray(logits, F8)
    m = logits.max(axis=-1, keepdims=True)
    with np.errstate(divide='ignore'):
        ls = logits - m - np.log(np.exp(logits - m).sum(axis=-1, keepdims=True))
    return -ls[np.arange(logits.shape[0]), targets], logits.argmax(axis=-1)           # (numpy's argmax: the first maximum)


def recon_step_scores(pitch, dur, x):
    """pitch [B,32,15,130], dur [B,32,15,5,2], x int [B,32,16,6] -> step_scores f64 [B,32,2] = (pitch NLL sum, duration NLL sum),
    step_counts int64 [B,32,6] = COUNT_NAMES.  Pitch target 130 / duration-bit target 2 = ignored; arg-max ties go to the lowest index;
    note_hit = pitch target < 128, pitch hit and all five bits hit (an ignored bit is not a hit)."""
    x = np.asarray(x, np.int64)
    B = x.shape[0]
    pt, dt = x[:, :, 1:, 0], x[:, :, 1:, 1:]                                          # [B,32,15], [B,32,15,5]
    scores, counts = np.zeros((B, 32, 2), F8), np.zeros((B, 32, 6), np.int64)
    p_hit = np.zeros(pt.shape, bool)
    live = np.nonzero(pt != 130)
    if live[0].size:
        nll, am = _nll_rows(np.asarray(pitch)[live], pt[live])
        np.add.at(scores[:, :, 0], live[:2], nll)
        p_hit[live] = am == pt[live]
    d_hit = np.zeros(dt.shape, bool)
    dlive = np.nonzero(dt != 2)
    if dlive[0].size:
        nll, am = _nll_rows(np.asarray(dur)[dlive], dt[dlive])
        np.add.at(scores[:, :, 1], dlive[:2], nll)
        d_hit[dlive] = am == dt[dlive]
    note = pt < 128
    counts[..., 0], counts[..., 1] = (pt != 130).sum(-1), p_hit.sum(-1)
    counts[..., 2], counts[..., 3] = (dt != 2).sum((-1, -2)), d_hit.sum((-1, -2))
    counts[..., 4], counts[..., 5] = note.sum(-1), (note & p_hit & d_hit.all(-1)).sum(-1)
    return scores, counts


def score_fold(step_scores, step_counts):
    """-> scores [B,2], counts [B,6]: the sums over the 32 time steps"""
    return np.asarray(step_scores, F8).sum(1), np.asarray(step_counts, np.int64).sum(1)


def kl_rows(mu, sd):
    """mu, sd [B,Z] -> [B]: sum_z (-log sd + (sd^2 + mu^2)/2 - 1/2)"""
    mu, sd = np.asarray(mu, F8), np.asarray(sd, F8)
    return (-np.log(sd) + (sd * sd + mu * mu) * 0.5 - 0.5).sum(-1)


def chord_targets(c):
    """c [B,8,36] -> root [B,8] (first maximum of c[..., :12]), chroma [B,8,12] (int of c[..., 12:24]), bass [B,8] (of c[..., 24:])"""
    c = np.asarray(c, F8)
    return c[..., :12].argmax(-1), c[..., 12:24].astype(np.int64), c[..., 24:].argmax(-1)


def chord_step_scores(root, chroma, bass, c):
    """root / bass [B,8,12], chroma [B,8,12,2], c [B,8,36] -> scores f64 [B,3] = root / chroma / bass NLL sums over the 8 steps,
    counts int64 [B,3] = root hits of 8, chroma-bit hits of 96, bass hits of 8"""
    B = np.asarray(c).shape[0]
    rt, ct, bt = chord_targets(c)
    scores, counts = np.zeros((B, 3), F8), np.zeros((B, 3), np.int64)
    for j, (lg, tg, C) in enumerate(((root, rt, 12), (chroma, ct, 2), (bass, bt, 12))):
        nll, am = _nll_rows(np.asarray(lg).reshape(-1, C), tg.reshape(-1))
        scores[:, j] = nll.reshape(B, -1).sum(-1)
        counts[:, j] = (am == tg.reshape(-1)).reshape(B, -1).sum(-1)
    return scores, counts


def roll_match(est_pr, ref_pr):
    """two [B,32,128] rolls -> int64 [B,4] = cells > 0 in est, cells > 0 in ref, cells > 0 in both, cells > 0 in both and equal"""
    e, r = np.asarray(est_pr, F8), np.asarray(ref_pr, F8)
    be, br = e > 0, r > 0
    return np.stack([be.sum((1, 2)), br.sum((1, 2)), (be & br).sum((1, 2)), (be & br & (e == r)).sum((1, 2))], -1).astype(np.int64)


def _div(a, b):
    return float(a) / float(b) if b else 0.0


def report(counts, chord_counts, roll, nll_sum):
    """per-sample counts [B,6], chord_counts [B,3], roll-match counts [B,4], the sum of pitch_nll + dur_nll -> the report's pooled ratios
    (total hits over total targets; a zero denominator gives 0.0)"""
    c, h, r = (np.asarray(a, np.int64).sum(0) for a in (counts, chord_counts, roll))
    steps = 8 * np.asarray(chord_counts).shape[0]
    return dict(pitch_acc=_div(c[1], c[0]), dur_acc=_div(c[3], c[2]), note_acc=_div(c[5], c[4]), root_acc=_div(h[0], steps),
                chroma_acc=_div(h[1], 12 * steps), bass_acc=_div(h[2], steps), onset_precision=_div(r[2], r[0]),
                onset_recall=_div(r[2], r[1]), onset_f1=_div(2 * r[2], r[0] + r[1]), exact_f1=_div(2 * r[3], r[0] + r[1]),
                nll_per_note=_div(nll_sum, c[4]))
