"""The per-sample score kernels of csrc/score.hip, one entry point at a time, against the plain fp64 references of tests/score_ref.py:
ptv_recon_step_scores in both row orders, with unpadded (130) and padded (136) rows and a misaligned base (the 16-byte and the 4-byte
load paths), ptv_score_fold, ptv_kl_rows, ptv_chord_step_scores and ptv_roll_match.

Every case builds fp32 inputs on the CPU from a seeded generator and gives the same values to the kernel and, widened, to the
reference.  Integer outputs and the bit-identity assertions are exact.  Floating-point outputs have no pre-chosen tolerance (the rule of
tests/test_gpu_leaf_kernels.py): the same formula is evaluated in fp32 on the CPU (torch), that evaluation's error against the fp64
reference is measured, and the kernel's error may be at most 4x that, with a floor of 8 fp32 ulps of the case's scale (check() below).
The bound never sees the kernel's output.  Each check prints `SCORE_RATIO family kernel-error/bound` (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import kernel_ops as K
import score_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = np.float32(np.nan)
SENT_F, SENT_I = np.float32(777.0), -7
RATIOS = {}
PAD = 130
WALK = (0, 1, 63, 64, 127, 128, 129, PAD)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def check(family, got, ref, f32, scale):
    """|got - ref| <= max(4 * max|f32 - ref|, 8 ulp_fp32(scale)); scale: a scalar, or one figure per output element"""
    got, ref, f32 = (np.asarray(a, np.float64) for a in (got, ref, f32))
    assert got.shape == ref.shape == f32.shape, (got.shape, ref.shape, f32.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all() and np.isfinite(f32).all()
    err32 = np.abs(f32 - ref).max()
    bound = np.maximum(4.0 * err32, 8.0 * np.spacing(np.abs(np.asarray(scale, np.float64)).astype(np.float32)).astype(np.float64))
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = float(np.where(err == 0, 0.0, err / bound).max())
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print('SCORE_RATIO %s %.3f (kernel err %.3e, fp32 err %.3e)' % (family, ratio, err.max(), err32))
    assert (err <= bound).all(), '%s: kernel error %.3e over the bound %.3e (fp32 evaluation: %.3e)' % (
        family, err.max(), float(np.min(bound)), err32)


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('SCORE_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


# ================================================================================================ ptv_recon_step_scores
def step_case(seed, B):
    """x int64 [B,32,16,6], pitch f32 [B,32,15,130], dur f32 [B,32,15,5,2] (API shapes; ignored rows / bits hold finite values here).
    Row r = (b*32 + t)*15 + n takes value pattern r % 8 and pitch target WALK[(r // 8) % 8], so every target meets every pattern:
    0 plain N(0, 3); 1 / 2 shifted by +-3e4; 3 the target tied for the maximum with a LOWER class (a miss); 4 tied with a HIGHER class (a
    hit; its duration bits favour their targets); 5 all classes equal; 6 -inf on some non-target classes; 7 plain, its duration pairs
    tied.  Sample 1 (if any) is all <pad>; step (0, 3) holds 14 notes and <eos>: all 15 rows live."""
    rng = np.random.RandomState(seed)
    rows = B * 480
    r = np.arange(rows)
    k = r % 8
    pt = np.array(WALK)[(r // 8) % 8]
    dt = rng.randint(0, 2, (rows, 5))
    dt[pt >= 128] = 2                                                  # <sos> / <eos> / <pad> rows carry no duration
    dt[rng.rand(rows, 5) < 0.08] = 2                                   # single ignored bits on live rows
    x = np.full((B, 32, 16, 6), 2, np.int64)
    x[..., 0] = PAD
    x[:, :, 1:, 0], x[:, :, 1:, 1:] = pt.reshape(B, 32, 15), dt.reshape(B, 32, 15, 5)
    x[0, 3, 1:15, 0], x[0, 3, 1:15, 1:] = np.arange(14) * 9 + 2, rng.randint(0, 2, (14, 5))
    x[0, 3, 15] = [129, 2, 2, 2, 2, 2]
    if B > 1:
        x[1, :, :, 0], x[1, :, :, 1:] = PAD, 2
    pt = x[:, :, 1:, 0].reshape(rows)
    pitch = rng.normal(0, 3, (rows, 130)).astype(np.float32)
    dur = rng.normal(0, 3, (rows, 5, 2)).astype(np.float32)
    pitch[k == 1] += np.float32(3e4)
    pitch[k == 2] -= np.float32(3e4)
    dur[k == 1] += np.float32(3e4)
    dur[k == 2] -= np.float32(3e4)
    top = pitch.max(1) + np.float32(1)
    lo = np.nonzero((k == 3) & (pt > 0) & (pt < PAD))[0]
    pitch[lo, pt[lo]] = top[lo]
    pitch[lo, pt[lo] // 2] = top[lo]                                   # (a class below the target)
    hi = np.nonzero((k == 4) & (pt < 129))[0]
    pitch[hi, pt[hi]] = top[hi]
    pitch[hi, pt[hi] + 1 + (128 - pt[hi]) // 2] = top[hi]              # (a class above it)
    pitch[k == 5] = np.float32(1.5)
    cut = (np.arange(130)[None, :] % 3 == 1) & (np.arange(130)[None, :] != pt[:, None]) & (k == 6)[:, None]
    pitch[cut] = -np.inf
    dur[k == 7, :, 1] = dur[k == 7, :, 0]
    dtv = x[:, :, 1:, 1:].reshape(rows, 5)
    for d in range(5):                                                 # the pitch-hit rows mostly hit their bits too: whole-note hits occur
        sel = np.nonzero((k == 4) & (dtv[:, d] != 2))[0]
        dur[sel, d, dtv[sel, d]] += np.float32(20)
    return x, pitch.reshape(B, 32, 15, 130), dur.reshape(B, 32, 15, 5, 2)


def poisoned(x, pitch, dur):
    """NaN over every ignored row and bit"""
    pitch, dur = pitch.copy(), dur.copy()
    pitch[x[:, :, 1:, 0] == PAD] = NAN
    dur[x[:, :, 1:, 1:] == 2] = NAN
    return pitch, dur


def device_logits(pitch, dur, step_major, ld, off):
    """the kernel's view: rows in the asked order, pitch rows of stride ld with NaN padding, base pointer `off` floats into the allocation"""
    if step_major:
        pitch, dur = pitch.transpose(2, 1, 0, 3), dur.transpose(2, 1, 0, 3, 4)
    rows = pitch.size // 130
    buf = np.full(off + rows * ld, NAN, np.float32)
    buf[off:].reshape(rows, ld)[:, :130] = pitch.reshape(rows, 130)
    return dev(buf)[off:], dev(dur.reshape(-1))


def run_steps(x, pitch, dur, step_major, ld, off=0):
    B = x.shape[0]
    p, d = device_logits(pitch, dur, step_major, ld, off)
    ss = torch.full(((B + 1) * 64,), float(SENT_F), device=DEV)
    sc = torch.full(((B + 1) * 192,), SENT_I, dtype=torch.int32, device=DEV)
    K.leaf('ptv_recon_step_scores', p, ld, d, dev(x), B, step_major, ss, sc)
    ss, sc = host(ss), host(sc)
    assert (ss[B * 64:] == SENT_F).all() and (sc[B * 192:] == SENT_I).all()             # nothing written past the outputs
    return ss[:B * 64].reshape(B, 32, 2), sc[:B * 192].reshape(B, 32, 6)


def steps_f32(x, pitch, dur):
    """the same formula in fp32 (torch, CPU): -log_softmax[target] of the live rows / bits, added per step in fp32"""
    B = x.shape[0]
    out = np.zeros((B, 32, 2), np.float32)
    for col, (lg, tg, ign) in enumerate(((pitch, x[:, :, 1:, 0], PAD), (dur, x[:, :, 1:, 1:], 2))):
        live = np.nonzero(tg != ign)
        ls = torch.log_softmax(torch.from_numpy(np.ascontiguousarray(lg[live])), -1)
        nll = -ls[torch.arange(ls.shape[0]), torch.from_numpy(tg[live])].numpy()
        np.add.at(out[:, :, col], live[:2], nll)
    return out


def step_scale(x, pitch, dur):
    """per output element: the sum of the |nll| it adds"""
    sc = np.zeros((x.shape[0], 32, 2))
    for col, (lg, tg, ign) in enumerate(((pitch, x[:, :, 1:, 0], PAD), (dur, x[:, :, 1:, 1:], 2))):
        live = np.nonzero(tg != ign)
        nll, _ = S._nll_rows(lg[live], tg[live])
        np.add.at(sc[:, :, col], live[:2], np.abs(nll))
    return sc


STEP_CASES = [(B, sm, ld, 0) for B in (1, 2, 3, 5) for sm in (0, 1) for ld in (130, 136)] + [(65, 1, 136, 0), (3, 0, 136, 1), (3, 1, 136, 1)]


@pytest.mark.parametrize('B,step_major,ld,off', STEP_CASES)
def test_step_scores_against_fp64_with_nan_over_everything_ignored(B, step_major, ld, off):
    """both row orders, the 16-byte path (ld 136, aligned) and the 4-byte path (ld 130, or the base one float off); B = 65: the step-major
    row stride crosses a wave.  Ignored rows and bits hold NaN: the outputs are finite and bit-identical to the run without the poison."""
    x, pitch, dur = step_case(50 + B, B)
    assert (x[0, 3, 1:, 0] != PAD).all() and (B == 1 or (x[1, :, 1:, 0] == PAD).all())
    pp, dp = poisoned(x, pitch, dur)
    ss, sc = run_steps(x, pp, dp, step_major, ld, off)
    ss0, sc0 = run_steps(x, pitch, dur, step_major, ld, off)
    assert np.isfinite(ss).all()
    assert ss.tobytes() == ss0.tobytes() and sc.tobytes() == sc0.tobytes()
    ref_s, ref_c = S.recon_step_scores(pp, dp, x)
    assert np.array_equal(sc, ref_c)                                                   # integers: exact
    assert sc[0, 3, 0] == 15 and sc[0, 3, 4] == 14
    if B > 1:
        assert not sc[1].any() and not ss[1].any() and not np.signbit(ss[1]).any()     # a sample of <pad>: zeros
    hit, n = sc[..., 1].sum(), sc[..., 0].sum()
    assert 0 < hit < n                                                                 # both tie directions occur: hits and misses
    assert 0 < sc[..., 5].sum() < sc[..., 4].sum()                                     # ... and whole-note hits and misses
    check('step scores %s' % ('vec' if ld % 4 == 0 and off % 4 == 0 else 'scalar'), ss, ref_s, steps_f32(x, pitch, dur),
          step_scale(x, pitch, dur))


def test_tie_rows_hit_and_miss_as_the_lowest_index_rule_says():
    x, pitch, dur = step_case(7, 2)
    _, sc = run_steps(x, pitch, dur, 1, 136)
    pt = x[:, :, 1:, 0].reshape(-1)
    am = pitch.reshape(-1, 130).astype(np.float64).argmax(-1)
    k = np.arange(pt.size) % 8
    lo, hi = (k == 3) & (pt > 0) & (pt < PAD), (k == 4) & (pt < 129)
    assert lo.sum() > 10 and hi.sum() > 10
    assert (am[lo] < pt[lo]).all() and (am[hi] == pt[hi]).all()                        # the first tie is a miss, the second a hit
    eq = (k == 5) & (pt < PAD)
    assert (am[eq] == 0).all()                                                         # all classes equal: class 0
    assert np.array_equal(sc, S.recon_step_scores(pitch, dur, x)[1])


@pytest.mark.parametrize('B', [3, 5])
def test_step_scores_do_not_depend_on_the_layout(B):
    x, pitch, dur = step_case(90 + B, B)
    pitch, dur = poisoned(x, pitch, dur)
    outs = [run_steps(x, pitch, dur, sm, ld, off) for sm, ld, off in ((1, 136, 0), (0, 136, 0), (1, 130, 0), (0, 130, 0), (1, 136, 1), (1, 132, 0))]
    for ss, sc in outs[1:]:
        assert ss.tobytes() == outs[0][0].tobytes() and sc.tobytes() == outs[0][1].tobytes()


# ================================================================================================ ptv_score_fold
@pytest.mark.parametrize('B', [1, 3, 65])
def test_score_fold_is_the_sequential_fp32_sum(B):
    x, pitch, dur = step_case(20 + B, B)
    p, d = device_logits(pitch, dur, 1, 136, 0)
    ss = torch.empty(B, 32, 2, device=DEV)
    sc = torch.empty(B, 32, 6, dtype=torch.int32, device=DEV)
    K.leaf('ptv_recon_step_scores', p, 136, d, dev(x), B, 1, ss, sc)
    outs = []
    for _ in range(2):
        fs = torch.full(((B + 1) * 2,), float(SENT_F), device=DEV)
        fc = torch.full(((B + 1) * 6,), SENT_I, dtype=torch.int32, device=DEV)
        K.leaf('ptv_score_fold', ss, sc, B, fs, fc)
        outs.append((host(fs), host(fc)))
    (fs, fc), (fs2, fc2) = outs
    assert fs.tobytes() == fs2.tobytes() and fc.tobytes() == fc2.tobytes()             # a second call: the same bits
    assert (fs[B * 2:] == SENT_F).all() and (fc[B * 6:] == SENT_I).all()
    hs, hc = host(ss), host(sc)
    acc = np.zeros((B, 2), np.float32)
    for t in range(32):
        acc = acc + hs[:, t]                                                           # fp32, t ascending
    assert fs[:B * 2].tobytes() == acc.tobytes()
    assert np.array_equal(fc[:B * 6].reshape(B, 6), hc.astype(np.int64).sum(1))
    assert np.array_equal(fc[:B * 6].reshape(B, 6), S.recon_step_scores(pitch, dur, x)[1].sum(1))


# ================================================================================================ ptv_kl_rows
def kl_case(Z, B=5):
    rng = np.random.RandomState(300 + Z)
    mu = rng.normal(0, 2, (B, Z)).astype(np.float32)
    sd = np.exp(rng.uniform(np.log(1e-3), np.log(30.0), (B, Z))).astype(np.float32)
    sd[0, 0], sd[-1, -1] = np.float32(1e-3), np.float32(30.0)
    return mu, sd


@pytest.mark.parametrize('Z', [1, 16, 63, 64, 65, 256])
def test_kl_rows(Z):
    mu, sd = kl_case(Z)
    B = mu.shape[0]
    out = torch.full((B + 1,), float(SENT_F), device=DEV)
    K.leaf('ptv_kl_rows', dev(mu), dev(sd), B, Z, out)
    got = host(out)
    assert got[B] == SENT_F
    tm, ts = torch.from_numpy(mu), torch.from_numpy(sd)
    f32 = (-torch.log(ts) + (ts * ts + tm * tm) * 0.5 - 0.5).sum(-1).numpy()
    m8, s8 = mu.astype(np.float64), sd.astype(np.float64)
    scale = np.abs(-np.log(s8) + (s8 * s8 + m8 * m8) * 0.5 - 0.5).sum(-1) + 0.5 * Z
    check('kl rows', got[:B], S.kl_rows(mu, sd), f32, scale)
    # the order of a row's sum depends on Z only: the row alone gives the same bits as the row in the batch
    dm, ds = dev(mu), dev(sd)
    for b in range(B):
        one = torch.full((2,), float(SENT_F), device=DEV)
        K.leaf('ptv_kl_rows', dm[b], ds[b], 1, Z, one)
        assert host(one)[0].tobytes() == got[b].tobytes() and host(one)[1] == SENT_F


# ================================================================================================ ptv_chord_step_scores
def chord_case(B):
    rng = np.random.RandomState(400 + B)
    c = np.zeros((B, 8, 36), np.float32)
    bt = np.arange(B * 8).reshape(B, 8)
    c[np.arange(B)[:, None], np.arange(8)[None, :], bt % 12] = 1
    c[np.arange(B)[:, None], np.arange(8)[None, :], 24 + (11 - bt % 12)] = 1
    c[:, :, 12:24] = rng.randint(0, 2, (B, 8, 12))
    c[0, 2, :12] = 0                                                                   # an all-zero one-hot: the first maximum, index 0
    c[0, 3, :12], c[0, 3, 24:] = 0.5, rng.normal(0, 1, 12)                             # a twelve-way tie; free-valued scores
    c[0, 4, [3, 9]], c[0, 4, [24 + 5, 24 + 7]] = 2.0, 3.0                              # two-way ties
    root = rng.normal(0, 3, (B, 8, 12)).astype(np.float32)
    chroma = rng.normal(0, 3, (B, 8, 12, 2)).astype(np.float32)
    bass = rng.normal(0, 3, (B, 8, 12)).astype(np.float32)
    rt, _, bs = S.chord_targets(c)
    root[0, 0] = 1.25                                                                  # all classes equal: arg-max 0
    root[0, 1] += np.float32(3e4)
    top = root[0, 5].max() + 1
    root[0, 5, rt[0, 5]] = root[0, 5, (rt[0, 5] + 1) % 12] = top                       # the target tied with a neighbour
    top = bass[0, 6].max() + 1
    bass[0, 6, bs[0, 6]] = bass[0, 6, (bs[0, 6] + 11) % 12] = top
    bass[0, 7, (bs[0, 7] + 3) % 12] = -np.inf
    chroma[0, 0, :, 1] = chroma[0, 0, :, 0]                                            # tied pairs: class 0
    chroma[0, 1] -= np.float32(3e4)
    return c, root, chroma, bass


@pytest.mark.parametrize('step_major', [0, 1])
@pytest.mark.parametrize('B', [1, 3])
def test_chord_step_scores(B, step_major):
    c, root, chroma, bass = chord_case(B)
    order = (lambda a: a.swapaxes(0, 1)) if step_major else (lambda a: a)
    sc = torch.full(((B + 1) * 3,), float(SENT_F), device=DEV)
    cn = torch.full(((B + 1) * 3,), SENT_I, dtype=torch.int32, device=DEV)
    K.leaf('ptv_chord_step_scores', dev(order(root)), dev(order(chroma)), dev(order(bass)), dev(c), B, step_major, sc, cn)
    sc, cn = host(sc), host(cn)
    assert (sc[B * 3:] == SENT_F).all() and (cn[B * 3:] == SENT_I).all()
    ref_s, ref_c = S.chord_step_scores(root, chroma, bass, c)
    assert np.array_equal(cn[:B * 3].reshape(B, 3), ref_c)
    rt, ct, bs = S.chord_targets(c)
    f32, scale = np.zeros((B, 3), np.float32), np.zeros((B, 3))
    for j, (lg, tg, C) in enumerate(((root, rt, 12), (chroma, ct, 2), (bass, bs, 12))):
        ls = torch.log_softmax(torch.from_numpy(lg).reshape(-1, C), -1)
        nll = -ls[torch.arange(ls.shape[0]), torch.from_numpy(np.ascontiguousarray(tg)).reshape(-1)].reshape(B, -1)
        f32[:, j] = nll.sum(-1).numpy()
        scale[:, j] = np.abs(S._nll_rows(lg.reshape(-1, C), tg.reshape(-1))[0]).reshape(B, -1).sum(-1)
    check('chord scores', sc[:B * 3].reshape(B, 3), ref_s, f32, scale)


# ================================================================================================ ptv_roll_match
@pytest.mark.parametrize('B', [1, 3])
def test_roll_match(B):
    rng = np.random.RandomState(500 + B)
    est, ref = np.zeros((B, 32, 128), np.float32), np.zeros((B, 32, 128), np.float32)
    cells = rng.rand(32, 128) < 0.05
    est[0][cells] = ref[0][cells] = rng.randint(1, 33, int(cells.sum()))                # equal cells
    diff = rng.rand(32, 128) < 0.02
    est[0][diff & cells] += 1                                                          # equal positions, other values
    if B > 1:
        est[1][cells], ref[1][np.roll(cells, 1, 1) & ~cells] = 3, 3                    # disjoint cells
        ref[2][cells] = 5                                                              # an empty estimate
    out = torch.full(((B + 1) * 4,), SENT_I, dtype=torch.int32, device=DEV)
    K.leaf('ptv_roll_match', dev(est), dev(ref), B, out)
    got = host(out)
    assert (got[B * 4:] == SENT_I).all()
    want = S.roll_match(est, ref)
    assert np.array_equal(got[:B * 4].reshape(B, 4), want)
    assert want[0, 2] == cells.sum() and 0 < want[0, 3] < want[0, 2]
    if B > 1:
        assert want[1, 2] == 0 and want[1, 0] > 0 and want[1, 1] > 0 and want[2].tolist() == [0, int(cells.sum()), 0, 0]
        K.leaf('ptv_roll_match', dev(ref), dev(est), B, out)                           # ... and the empty roll on the other side
        assert np.array_equal(host(out)[:B * 4].reshape(B, 4), want[:, [1, 0, 2, 3]])


# ================================================================================================ argument errors
def test_null_pointers_and_empty_batches_are_refused_and_write_nothing():
    B = 2
    f = lambda n: torch.full((n,), float(SENT_F), device=DEV)
    i = lambda n: torch.full((n,), SENT_I, dtype=torch.int32, device=DEV)
    x = torch.full((B * 32 * 16 * 6,), 1, dtype=torch.int64, device=DEV)
    calls = {
        'ptv_recon_step_scores': ([f(B * 480 * 136), 136, f(B * 4800), x, B, 1, f(B * 64), i(B * 192)], (0, 2, 3, 6, 7), 4),
        'ptv_score_fold': ([f(B * 64), i(B * 192), B, f(B * 2), i(B * 6)], (0, 1, 3, 4), 2),
        'ptv_kl_rows': ([f(B * 16), f(B * 16), B, 16, f(B)], (0, 1, 4), 2),
        'ptv_chord_step_scores': ([f(B * 96), f(B * 192), f(B * 96), f(B * 288), B, 1, f(B * 3), i(B * 3)], (0, 1, 2, 3, 6, 7), 4),
        'ptv_roll_match': ([f(B * 4096), f(B * 4096), B, i(B * 4)], (0, 1, 3), 2),
    }
    for name, (args, ptrs, b_at) in calls.items():
        outs = [a for a in args if torch.is_tensor(a)]
        for p in ptrs:
            bad = list(args)
            bad[p] = None
            assert K.leaf_rc(name, *bad) == -1, (name, p)
        for b in (0, -3):
            bad = list(args)
            bad[b_at] = b
            assert K.leaf_rc(name, *bad) == -1, (name, b)
        torch.cuda.synchronize()
        for t in outs:
            if t.dtype == torch.int32:
                assert (host(t) == SENT_I).all(), name
            elif t.dtype == torch.float32:
                assert (host(t) == SENT_F).all(), name
    assert K.leaf_rc('ptv_recon_step_scores', f(64), 129, f(64), x, B, 1, f(B * 64), i(B * 192)) == -1      # rows shorter than the 130 classes
