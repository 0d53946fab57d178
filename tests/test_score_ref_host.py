"""CPU: the fp64 references of tests/score_ref.py against torch's own cross-entropy, and the identity that ties the per-sample sums to
the batch means the reference model reported (tests/golden/reduced_tf1.npz: its logits, posteriors and `losses`)."""
import numpy as np
import torch

import score_ref as S
from helpers import load_npz


def _grid(rng, B, pad=0.5):
    x = np.concatenate([rng.randint(0, 130, (B, 32, 16, 1)), rng.randint(0, 2, (B, 32, 16, 5))], -1).astype(np.int64)
    x[rng.rand(B, 32, 16) < pad] = [130, 2, 2, 2, 2, 2]
    x[:, :, :, 1:][rng.rand(B, 32, 16, 5) < 0.1] = 2                                   # single ignored bits on live rows too
    return x


def test_step_scores_equal_torch_cross_entropy_fp64():
    rng = np.random.RandomState(3)
    B = 3
    x = _grid(rng, B)
    pitch = rng.normal(0, 3, (B, 32, 15, 130))
    dur = rng.normal(0, 3, (B, 32, 15, 5, 2))
    pitch[x[:, :, 1:, 0] == 130] = np.nan                                              # ignored rows / bits: excluded, not multiplied by zero
    dur[x[:, :, 1:, 1:] == 2] = np.nan
    scores, counts = S.recon_step_scores(pitch, dur, x)
    assert np.isfinite(scores).all()
    ce = torch.nn.functional.cross_entropy
    pt, dt = torch.from_numpy(x[:, :, 1:, 0]), torch.from_numpy(x[:, :, 1:, 1:])
    nan0 = lambda a: torch.from_numpy(np.nan_to_num(a, nan=0.0))
    pn = ce(nan0(pitch).reshape(-1, 130), pt.reshape(-1), ignore_index=130, reduction='none').reshape(B, 32, 15)
    dn = ce(nan0(dur).reshape(-1, 2), dt.reshape(-1), ignore_index=2, reduction='none').reshape(B, 32, 75)
    np.testing.assert_allclose(scores[..., 0], pn.sum(-1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(scores[..., 1], dn.sum(-1).numpy(), rtol=1e-12, atol=1e-12)
    # the counts, once more from torch's arg-max
    p_hit = (nan0(pitch).argmax(-1) == pt) & (pt != 130)
    d_hit = (nan0(dur).argmax(-1) == dt) & (dt != 2)
    note = pt < 128
    want = torch.stack([(pt != 130).sum(-1), p_hit.sum(-1), (dt != 2).sum((-1, -2)), d_hit.sum((-1, -2)), note.sum(-1),
                        (note & p_hit & d_hit.all(-1)).sum(-1)], -1).numpy()
    assert np.array_equal(counts, want)
    fs, fc = S.score_fold(scores, counts)
    assert np.array_equal(fc, want.sum(1)) and np.allclose(fs, scores.sum(1), rtol=0, atol=0)


def test_ties_go_to_the_lowest_index():
    x = np.full((1, 32, 16, 6), 2, np.int64)
    x[..., 0] = 130
    x[0, 0, 1] = [5, 0, 1, 0, 1, 2]
    x[0, 0, 2] = [5, 1, 1, 1, 1, 1]
    pitch, dur = np.zeros((1, 32, 15, 130)), np.zeros((1, 32, 15, 5, 2))
    pitch[0, 0, 0, [3, 5]] = 2.0                                                       # target 5 tied with the LOWER class 3: a miss
    pitch[0, 0, 1, [5, 9]] = 2.0                                                       # ... with the HIGHER class 9: a hit
    dur[0, 0, 1, :, 1] = 1.0                                                           # row 2: class 1 wins all five bits
    _, counts = S.recon_step_scores(pitch, dur, x)                                     # row 1: all pairs tied -> class 0
    assert counts[0, 0].tolist() == [2, 1, 9, 2 + 5, 2, 1] and not counts[0, 1:].any()


def test_chord_scores_equal_torch_cross_entropy_fp64():
    rng = np.random.RandomState(5)
    B = 4
    c = np.zeros((B, 8, 36), np.float32)
    c[..., :12], c[..., 24:] = rng.normal(0, 1, (B, 8, 12)), rng.normal(0, 1, (B, 8, 12))
    c[..., 12:24] = rng.randint(0, 2, (B, 8, 12))
    c[0, 0, :12] = 0.0                                                                 # a twelve-way tie: root 0
    root, chroma, bass = rng.normal(0, 2, (B, 8, 12)), rng.normal(0, 2, (B, 8, 12, 2)), rng.normal(0, 2, (B, 8, 12))
    scores, counts = S.chord_step_scores(root, chroma, bass, c)
    ce = torch.nn.functional.cross_entropy
    rt, ct, bt = (torch.from_numpy(np.ascontiguousarray(t)) for t in S.chord_targets(c))
    assert rt[0, 0] == 0
    for j, (lg, tg, C) in enumerate(((root, rt, 12), (chroma, ct, 2), (bass, bt, 12))):
        l = torch.from_numpy(lg).reshape(-1, C)
        nll = ce(l, tg.reshape(-1), reduction='none').reshape(B, -1).sum(-1).numpy()
        np.testing.assert_allclose(scores[:, j], nll, rtol=1e-12, atol=1e-12)
        assert np.array_equal(counts[:, j], (l.argmax(-1) == tg.reshape(-1)).reshape(B, -1).sum(-1).numpy())


def test_roll_match_and_report():
    est, ref = np.zeros((2, 32, 128), np.float32), np.zeros((2, 32, 128), np.float32)
    est[0, 0, 60], ref[0, 0, 60] = 4, 4                                                # equal
    est[0, 1, 62], ref[0, 1, 62] = 2, 3                                                # same cell, other duration
    est[0, 2, 64], ref[0, 3, 64] = 1, 1                                                # disjoint
    ref[1, 5, 5] = 7                                                                   # an empty estimate
    r = S.roll_match(est, ref)
    assert r.tolist() == [[3, 3, 2, 1], [0, 1, 0, 0]]
    rep = S.report(np.array([[10, 5, 50, 40, 8, 2]] * 2), np.array([[8, 90, 4]] * 2), r, 32.0)
    assert rep['pitch_acc'] == 0.5 and rep['dur_acc'] == 0.8 and rep['note_acc'] == 0.25 and rep['root_acc'] == 1.0
    assert rep['chroma_acc'] == 180 / 192 and rep['bass_acc'] == 0.5 and rep['nll_per_note'] == 2.0
    assert rep['onset_precision'] == 2 / 3 and rep['onset_recall'] == 0.5 and rep['onset_f1'] == 4 / 7 and rep['exact_f1'] == 2 / 7
    empty = S.report(np.zeros((1, 6)), np.zeros((1, 3)), np.zeros((1, 4)), 0.0)
    assert empty['pitch_acc'] == empty['onset_f1'] == empty['nll_per_note'] == 0.0     # zero denominators


def test_per_sample_sums_pool_to_the_reference_models_batch_means():
    """sum of the per-sample sums over the number of targets = the means the reference's loss_function returned on the same tensors
    (atol 1e-5: the bound tests/test_gpu_model.py holds the fp32 path to on this fixture)"""
    g = load_npz('reduced_tf1.npz')
    losses = g['losses']
    step_scores, step_counts = S.recon_step_scores(g['pitch_outs'], g['dur_outs'], g['x'])
    scores, counts = S.score_fold(step_scores, step_counts)
    assert counts[:, 0].sum() > 0 and counts[:, 2].sum() > 0
    assert abs(scores[:, 0].sum() / counts[:, 0].sum() - losses[2]) <= 1e-5
    assert abs(scores[:, 1].sum() / counts[:, 2].sum() - losses[3]) <= 1e-5
    B, Z = g['mu_chd'].shape
    assert abs(S.kl_rows(g['mu_chd'], g['std_chd']).sum() / (B * Z) - losses[5]) <= 1e-5
    assert abs(S.kl_rows(g['mu_rhy'], g['std_rhy']).sum() / (B * Z) - losses[6]) <= 1e-5
    chord, _ = S.chord_step_scores(g['recon_root'], g['recon_chroma'], g['recon_bass'], g['c'])
    assert abs(chord[:, 0].sum() / (B * 8) - losses[8]) <= 1e-5
    assert abs(chord[:, 1].sum() / (B * 96) - losses[9]) <= 1e-5
    assert abs(chord[:, 2].sum() / (B * 8) - losses[10]) <= 1e-5
