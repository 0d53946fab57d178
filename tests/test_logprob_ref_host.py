"""CPU: the float64 restatement of the decode log-probabilities (tests/logprob_ref.py) against a brute-force loop over single classes,
the normalisation of logq over a row's kept set, the counting rule on crafted grids, and the host-side validation of decode_best_of."""
import math

import numpy as np
import pytest

import constrain_ref as CR
import logprob_ref as LR
import nucleus_ref as NR

PAD = 130


def crafted_grid():
    """[2, 32, 16, 6]: everything <pad> except step (0, 0): <eos> at slot 1; (0, 1): 15 notes, no <eos>; (0, 2): two notes, <sos> at slot
    3, a note, <eos>, then junk after it; (0, 3): a pitch outside 0..129 before the <eos>; (0, 4): a note with a bit that is no class;
    sample 1: every step <eos> at slot 1"""
    x = np.full((2, 32, 16, 6), 2, np.int64)
    x[..., 0] = PAD
    x[0, :, 1, 0] = 129
    x[0, 1, 1:, 0], x[0, 1, 1:, 1:] = np.arange(15) * 8 + 3, 1
    x[0, 2, 1:6, 0] = [60, 64, 128, 67, 129]
    x[0, 2, 1:6, 1:] = 0
    x[0, 2, 6:9, 0], x[0, 2, 6:9, 1:] = [70, 129, 71], 1
    x[0, 3, 1:4, 0], x[0, 3, 1:4, 1:] = [50, 131, 129], 0
    x[0, 4, 1:3, 0] = [40, 129]
    x[0, 4, 1, 1:] = [0, 1, 2, 1, 0]
    x[1, :, 1, 0] = 129
    return x


def test_the_counting_rule_on_crafted_grids():
    x = crafted_grid()
    pc, bc, err = LR.counted(x)
    assert LR.step_len(x[0, 0, :, 0]) == 1 and LR.step_len(x[0, 1, :, 0]) == 15 and LR.step_len(x[0, 2, :, 0]) == 5
    assert pc[0, 0].tolist() == [True] + [False] * 14 and not bc[0, 0].any()                  # <eos> at slot 1: one decision, no bit
    assert pc[0, 1].all() and bc[0, 1].all()                                                  # no <eos>: 15 pitches, 75 bits
    assert pc[0, 2].tolist() == [True] * 5 + [False] * 10                                     # up to the FIRST <eos>; what follows is dead
    assert bc[0, 2].all(-1).tolist() == [True, True, False, True, False] + [False] * 10       # <sos> mid-step counts, its bits do not
    assert pc[0, 3].tolist() == [True, False, True] + [False] * 12 and err.tolist() == [1, 0]  # a pitch that names no class
    assert bc[0, 4, 0].tolist() == [True, True, False, True, True]
    assert pc[1].sum() == 32 and not bc[1].any()
    lo = LR.running_lo(x)
    assert lo[0, 1].tolist() == [-1] + (np.arange(14) * 8 + 3).tolist()
    assert lo[0, 2, :6].tolist() == [-1, 60, 64, 64, 67, 67]                                   # <sos> / <eos> do not move lo
    rng = np.random.RandomState(3)
    pitch, dur = rng.normal(0, 3, (2, 32, 15, 130)), rng.normal(0, 3, (2, 32, 15, 5, 2))
    pitch[~pc], dur[~bc] = np.nan, np.nan                                                    # what does not count is never read
    lp, cn, e2, scale = LR.logprob(pitch, dur, x, Tp=0.7, Td=1.3)
    assert np.isfinite(lp).all() and e2.tolist() == [1, 0]
    assert np.array_equal(cn[..., 0], pc.sum(-1)) and np.array_equal(cn[..., 1], bc.sum((-1, -2))) and not cn[..., 2:].any()
    assert cn[0, 1].tolist() == [15, 75, 0, 0] and cn[0, 2].tolist() == [5, 15, 0, 0]


def brute(pitch, dur, x, kept, Tp, Td, fp, fd):
    """one class at a time with math.exp / math.log: the definition"""
    B = x.shape[0]
    out, cn = np.zeros((B, 32, 4)), np.zeros((B, 32, 4), np.int64)
    for b in range(B):
        for t in range(32):
            L = next((s for s in range(1, 16) if x[b, t, s, 0] == 129), 15)
            for n in range(L):
                d = int(x[b, t, n + 1, 0])
                if not 0 <= d <= 129:
                    continue
                v = [float(np.float32(a)) for a in pitch[b, t, n]]
                z = sum(math.exp(a - max(v)) for a in v)
                out[b, t, 0] += v[d] - max(v) - math.log(z)
                cn[b, t, 0] += 1
                if fp is not None and fp[n][t * B + b] >= 0:
                    cn[b, t, 2] += 1
                elif Tp > 0 and kept[b, t, n, d]:
                    ks = [c for c in range(130) if kept[b, t, n, c]]
                    mk = max(v[c] for c in ks)
                    out[b, t, 2] += (v[d] - mk) / Tp - math.log(sum(math.exp((v[c] - mk) / Tp) for c in ks))
                if d >= 128:
                    continue
                for i in range(5):
                    c = int(x[b, t, n + 1, 1 + i])
                    if c not in (0, 1):
                        continue
                    l = [float(np.float32(a)) for a in dur[b, t, n, i]]
                    out[b, t, 1] += l[c] - max(l) - math.log(sum(math.exp(a - max(l)) for a in l))
                    cn[b, t, 1] += 1
                    if fd is not None and fd[i][n * 32 * B + t * B + b] >= 0:
                        cn[b, t, 3] += 1
                    elif Td > 0:
                        a = [q / Td for q in l]
                        out[b, t, 3] += a[c] - max(a) - math.log(sum(math.exp(q - max(a)) for q in a))
    return out, cn


def sampled_case(seed=5, B=2):
    """a grid DRAWN from the kept sets (ascending, one-row mask, top_k, top_p), so that every free decision lies inside them"""
    rng = np.random.RandomState(seed)
    pitch = rng.normal(0, 3, (B, 32, 15, 130)).astype(np.float32)
    dur = rng.normal(0, 2, (B, 32, 15, 5, 2)).astype(np.float32)
    mask = CR.mask_build(1, pitch_classes=0b101010110101, lo=30, hi=100)
    T, k, q = 0.8, 8, NR.q24_of(0.9)
    x = np.full((B, 32, 16, 6), 2, np.int64)
    x[..., 0] = PAD
    x[:, :, 0, 0] = 128
    kept = np.zeros((B, 32, 15, 130), bool)
    for b in range(B):
        for t in range(32):
            lo = -1
            for n in range(15):
                al = CR.allowed(mask[0, t], lo, True)
                kp = CR.keep_mask(pitch[b, t, n], al, np.float32(T), k, q=q)
                kept[b, t, n] = kp
                ks = np.nonzero(kp)[0]
                d = 129 if kp[129] and (n == 14 or rng.rand() < 0.25) else int(ks[rng.randint(len(ks))])
                x[b, t, n + 1, 0] = d
                if d == 129:
                    break
                x[b, t, n + 1, 1:] = rng.randint(0, 2, 5)
                lo = max(lo, d)
    return pitch, dur, x, kept, mask, T, k, q


def test_reference_against_the_brute_force_loop():
    pitch, dur, x, kept, mask, T, k, q = sampled_case()
    B = x.shape[0]
    assert np.array_equal(kept[LR.counted(x)[0]], LR.kept_sets(pitch, x, T, k, q=q, mask=mask, ascending=True)[LR.counted(x)[0]])
    rng = np.random.RandomState(9)
    fp = np.where(rng.rand(15, 32 * B) < 0.3, 1, -1)
    fd = np.where(rng.rand(5, 480 * B) < 0.3, 0, -1)
    for fp_, fd_, Tp, Td in ((None, None, T, 1.4), (fp, fd, T, 1.4), (None, None, 0.0, 0.0), (fp, None, T, 0.0)):
        lp, cn, err, _ = LR.logprob(pitch, dur, x, kept, Tp, Td, fp_, fd_)
        want, wcn = brute(pitch, dur, x, kept, float(np.float32(Tp)), float(np.float32(Td)), fp_, fd_)
        assert not err.any() and np.array_equal(cn, wcn)
        assert np.abs(lp - want).max() < 1e-10
        if Tp == 0:
            assert not lp[..., 2:].any()
        f32 = LR.logprob(pitch, dur, x, kept, Tp, Td, fp_, fd_, dtype=np.float32)
        assert f32[0].dtype == np.float32 and np.array_equal(f32[1], cn)
        assert 0 < np.abs(f32[0] - lp).max() < 1e-3                                            # fp32 rounds, and only rounds
    assert (lp[..., 2] >= lp[..., 0]).any()                                                  # (truncation concentrates mass: no assertion of order)
    s, c = LR.fold(lp, cn)
    assert np.allclose(s, lp.sum(1), rtol=0, atol=1e-9) and np.array_equal(c, cn.sum(1))


def test_a_decision_outside_the_kept_set_is_reported_not_scored():
    pitch, dur, x, kept, *_ = sampled_case(6, 1)
    b, t = 0, 7
    d = int(x[b, t, 1, 0])
    kept[b, t, 0, d] = False
    lp, cn, err, _ = LR.logprob(pitch, dur, x, kept, 0.8, 0.8)
    assert err.tolist() == [1]
    kept[b, t, 0, d] = True
    lp2, cn2, err2, _ = LR.logprob(pitch, dur, x, kept, 0.8, 0.8)
    assert err2.tolist() == [0] and np.array_equal(cn, cn2) and np.array_equal(lp[..., :2], lp2[..., :2])
    assert lp[b, t, 2] != lp2[b, t, 2] and np.array_equal(np.delete(lp[b, :, 2], t), np.delete(lp2[b, :, 2], t))


def test_exp_logq_sums_to_one_over_the_kept_set():
    pitch, dur, x, kept, mask, T, k, q = sampled_case(8, 1)
    rows = 0
    for t in range(0, 32, 5):
        for n in range(15):
            kp = kept[0, t, n]
            if not kp.any():
                continue
            rows += 1
            tot = sum(math.exp(LR.logq_row(pitch[0, t, n], kp, T, int(c))) for c in np.nonzero(kp)[0])
            assert abs(tot - 1.0) < 1e-12, (t, n, tot)
            tot = sum(math.exp(LR.logp_row(pitch[0, t, n], c)) for c in range(130))
            assert abs(tot - 1.0) < 1e-12
    assert rows > 10


def test_best_of_reference():
    nan = np.nan
    best, err = LR.best_of(np.array([[1.0, nan, nan, -np.inf], [1.0, 2.0, nan, nan], [0.5, 2.0, nan, -np.inf]]))
    assert best.tolist() == [0, 1, 0, 0] and err.tolist() == [0, 0, 2, 0]


@pytest.mark.parametrize('kw', [dict(n=0), dict(n=-1), dict(n=2.0), dict(n=True), dict(n=2, rank_by='p'), dict(n=2, temperature=None),
                                dict(n=2, length_normalize=1)])
def test_decode_best_of_refuses_bad_arguments_before_any_launch(kw):
    """the validation is a static function of the arguments (no model, no device), and decode_best_of runs it first: on a model with
    host tensors anything that went further would fail otherwise than by this ValueError"""
    import torch
    from polyphonic_chord_texture_disentanglement_amd.model import DisentangleVAE
    kw = dict(dict(temperature=1.0), **kw)
    with pytest.raises(ValueError):
        DisentangleVAE._check_best_of(**kw)
    m = DisentangleVAE.init_model(device='cpu')
    z = torch.zeros(2, 256)
    with pytest.raises(ValueError):
        m.decode_best_of(z, z, kw.pop('n'), **kw)


def test_decode_best_of_accepts_good_arguments():
    from polyphonic_chord_texture_disentanglement_amd.model import DisentangleVAE
    DisentangleVAE._check_best_of(1, temperature=1.0)
    DisentangleVAE._check_best_of(4, 'logq', True, temperature=0.5, top_k=3)
    DisentangleVAE._check_best_of(2, dur_temperature=0.5)
