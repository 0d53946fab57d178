"""GPU: the kernels of csrc/chord_decode.hip on synthetic logits, no model: ptv_debug_chord_noise, ptv_chord_decide (argmax with planted
ties, sampled decisions, partial DPP groups / waves / workgroups, kept chords with invalid blocks, the two log-probabilities) and
ptv_chord_logprob_fold, against the numpy restatement tests/chord_sample_ref.py.

Decisions are exact but for those sample_ref.skippable() allows (the device's fp32 logarithm moves the noise by up to NOISE_TOL), at most
SKIP_CAP of a case.  Integer outputs are exact.  logp / logq follow the rule of tests/test_gpu_decode_logprob_kernels.py and bring no number
of their own: |got - ref| <= max(4 * max|f32 - ref|, 8 ulp_fp32(scale)), ref the float64 restatement, f32 the same formulas in fp32 in
the kernel's term order, scale the sum of the |terms| of the element; both are evaluated at the decisions the device took, and the bound
never sees the kernel's output."""
import numpy as np
import pytest
import torch

import chord_sample_ref as CS
import sample_ref as S
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED, DRAW = 11, 4
SKIP_CAP = 0.005                                             # the cap of tests/test_gpu_sampling.py
SENT_F, SENT_I = np.float32(777.0), -7
GUARD = 2                                                    # rows behind the batch that must stay untouched


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def block(Tc, Th, offset=0):
    return FF_.sampling_block(DEV, Tc, Th, seed=SEED, draw=DRAW, sample_offset=offset)


def logits(B, seed, scale=2.0):
    rng = np.random.RandomState(seed)
    return (rng.normal(0, scale, (B, 12)).astype(np.float32), rng.normal(0, scale, (B, 12, 2)).astype(np.float32),
            rng.normal(0, scale, (B, 12)).astype(np.float32))


def decide(root, chroma, bass, t, blk=None, keep_c=None, keep_steps=None, want_tok=True, expect=0):
    """one ptv_chord_decide launch on sentinel-filled outputs with GUARD rows behind the batch -> dict of numpy arrays (or the status)"""
    B = root.shape[0]
    R = B + GUARD
    f = lambda *s: torch.full(s, float(SENT_F), device=DEV, dtype=torch.float32)
    i = lambda *s: torch.full(s, SENT_I, device=DEV, dtype=torch.int32)
    o = dict(tok=f(R, 36), c=f(R, 8, 36), chord14=f(R, 8, 14), step_logp=f(R, 8, 3), step_logq=f(R, 8, 3), step_forced=i(R, 8, 3),
             step_err=i(R, 8))
    d_in = [dev(root), dev(chroma.reshape(B, 24)), dev(bass)]
    kc = None if keep_c is None else dev(np.asarray(keep_c, np.float32))
    ks = None if keep_steps is None else dev(np.asarray(keep_steps, np.uint8))
    rc = lib().ptv_chord_decide(ptr(d_in[0]), ptr(d_in[1]), ptr(d_in[2]), B, t, ptr(blk), ptr(kc), ptr(ks), 0 if ks is None else ks.shape[0],
                                ptr(o['tok']) if want_tok else None, ptr(o['c']), ptr(o['chord14']), ptr(o['step_logp']), ptr(o['step_logq']),
                                ptr(o['step_forced']), ptr(o['step_err']), stream_ptr())
    assert rc == expect, rc
    torch.cuda.synchronize()
    out = {k: host(v) for k, v in o.items()}
    if rc != 0:                                              # refused: nothing is written
        assert all((v == (SENT_I if v.dtype == np.int32 else SENT_F)).all() for v in out.values())
        return rc
    # nothing but row t of the B rows is written
    for k, v in out.items():
        sent = SENT_I if v.dtype == np.int32 else SENT_F
        assert (v[B:] == sent).all(), k
        if k != 'tok':
            other = np.delete(v[:B], t, axis=1)
            assert (other == sent).all(), k
    if not want_tok:
        assert (out['tok'] == SENT_F).all()
    r = {k: (v[:B] if k == 'tok' else v[:B, t]) for k, v in out.items()}
    # the three token forms say the same thing
    c14 = r['chord14']
    dr, bits, db = c14[:, 0].astype(np.int64), c14[:, 1:13].astype(np.int64), c14[:, 13].astype(np.int64)
    c, again = CS.tokens(dr, bits, db)
    assert np.array_equal(again, c14) and np.array_equal(r['c'], c)
    if want_tok:
        assert np.array_equal(r['tok'], c)
    r.update(root=dr, bits=bits, bass=db)
    return r


def explained(got, ref, skip, what, cap=True):
    """every decision equals the restated one or is skippable; at most SKIP_CAP of the case's decisions are skippable"""
    bad = [(got[k] != ref[k]) & ~s for k, s in zip(('root', 'bits', 'bass'), skip)]
    n = sum(s.size for s in skip)
    k = sum(int(s.sum()) for s in skip)
    print('%s: skipped %d of %d decisions (mismatching inside the tolerance: %d)'
          % (what, k, n, sum(int(((got[key] != ref[key]) & s).sum()) for key, s in zip(('root', 'bits', 'bass'), skip))))
    for name, b in zip(('root', 'bits', 'bass'), bad):
        assert not b.any(), (what, name, int(b.sum()), np.argwhere(b)[:4])
    if cap:
        assert k <= SKIP_CAP * n, (what, k, n)


def check(family, got, ref, f32, scale):
    """|got - ref| <= max(4 * max|f32 - ref|, 8 ulp_fp32(scale)), scale one figure per output element"""
    got, ref, f32 = (np.asarray(a, np.float64) for a in (got, ref, f32))
    assert got.shape == ref.shape == f32.shape, (got.shape, ref.shape, f32.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all() and np.isfinite(f32).all()
    err32 = np.abs(f32 - ref).max()
    bound = np.maximum(4.0 * err32, 8.0 * np.spacing(np.abs(np.asarray(scale, np.float64)).astype(np.float32)).astype(np.float64))
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = float(np.where(err == 0, 0.0, err / bound).max())
    print('CHORD_LOGPROB_RATIO %s %.3f (kernel err %.3e, fp32 err %.3e)' % (family, ratio, err.max(), err32))
    assert (err <= bound).all(), '%s: kernel error %.3e over the bound (fp32 evaluation: %.3e)' % (family, err.max(), err32)


def check_logprob(family, root, chroma, bass, r, Tc, Th, sampled):
    """the device's step_logp / step_logq against the restatement AT THE DEVICE'S decisions"""
    dec = dict(root=r['root'], bits=r['bits'], bass=r['bass'], forced=r['step_forced'])
    lp, lq, sp, sq = CS.logprob(root, chroma, bass, dec, Tc, Th, sampled)
    f_lp, f_lq, _, _ = CS.logprob(root, chroma, bass, dec, Tc, Th, sampled, dtype=np.float32)
    for h, head in enumerate(('root', 'chroma', 'bass')):
        check('%s logp %s' % (family, head), r['step_logp'][:, h], lp[:, h], f_lp[:, h], sp[:, h])
        zero = sq[:, h] == 0                                 # T = 0, no block, forced: exactly 0
        assert (r['step_logq'][zero, h] == 0).all() and (lq[zero, h] == 0).all()
        if (~zero).any():
            check('%s logq %s' % (family, head), r['step_logq'][~zero, h], lq[~zero, h], f_lq[~zero, h], sq[~zero, h])


# ---------------------------------------------------------------------------------------------------------------------------------
def test_noise_equals_the_restatement():
    """ptv_debug_chord_noise (the device function ptv_chord_decide calls) for 20 rows, two steps, offsets 0 and 1000"""
    worst = 0.0
    for offset in (0, 1000):
        for t in (2, 7):
            out = torch.full((20 + GUARD, 12, 4), float(SENT_F), device=DEV)
            assert lib().ptv_debug_chord_noise(ptr(block(1.0, 0.7, offset)), 20, t, ptr(out), stream_ptr()) == 0
            got = host(out)
            assert (got[20:] == SENT_F).all()
            ref = CS.noise(SEED, DRAW, offset + np.arange(20), t)
            worst = max(worst, float(np.abs(got[:20].astype(np.float64) - ref).max()))
            assert np.abs(got[:20].astype(np.float64) - ref).max() <= S.NOISE_TOL
    print('chord noise: max |device - restatement| = %.3e (NOISE_TOL %.1e)' % (worst, S.NOISE_TOL))
    out = torch.zeros(4, 12, 4, device=DEV)
    for bad in ((None, 4, 0, out), (block(1.0, 1.0), 0, 0, out), (block(1.0, 1.0), 4, 8, out), (block(1.0, 1.0), 4, 0, None)):
        assert lib().ptv_debug_chord_noise(ptr(bad[0]), bad[1], bad[2], ptr(bad[3]), stream_ptr()) == -1


@pytest.mark.parametrize('blk', [None, (0.0, 0.0)])
def test_argmax_with_planted_ties_is_exact(blk):
    """integer-valued logits, ties planted in every head: the decisions are the restated first maxima, exactly; logq = 0"""
    B = 70
    rng = np.random.RandomState(1)
    root, chroma, bass = (rng.randint(-3, 4, s).astype(np.float32) for s in ((B, 12), (B, 12, 2), (B, 12)))
    root[0] = 2                                              # all tied: class 0
    bass[1] = -1
    bass[1, [4, 9]] = 3                                      # two maxima: the first
    root[2, [11]] = 9
    root[3, [0, 11]] = 9
    chroma[4] = 1                                            # tied pairs: class 0
    want = CS.decide(root, chroma, bass, None, 0, 0)
    assert ((chroma[..., 0] == chroma[..., 1]).sum() > 60) and (np.sort(root, -1)[:, -1] == np.sort(root, -1)[:, -2]).sum() > 10
    r = decide(root, chroma, bass, 3, None if blk is None else block(*blk, offset=1000))
    for k in ('root', 'bits', 'bass'):
        assert np.array_equal(r[k], want[k]), k
    assert r['root'][:4].tolist() == [0, int(want['root'][1]), 11, 0] and r['bass'][1] == 4 and not r['bits'][4].any()
    assert not r['step_forced'].any() and not r['step_err'].any() and (r['step_logq'] == 0).all()
    check_logprob('argmax', root, chroma, bass, r, 0.0, 0.0, blk is not None)


@pytest.mark.parametrize('Tc,Th', [(1.0, 0.7), (1.0, 0.0)])
def test_sampled_decisions_follow_the_restated_rule(Tc, Th):
    B, t, offset = 512, 5, 1000
    root, chroma, bass = logits(B, 2)
    nz = CS.noise(SEED, DRAW, offset + np.arange(B), t)
    want = CS.decide(root, chroma, bass, nz, Tc, Th)
    r = decide(root, chroma, bass, t, block(Tc, Th, offset))
    explained(r, want, CS.skippable(root, chroma, bass, nz, Tc, Th), 'T = (%g, %g)' % (Tc, Th))
    assert (r['root'] != np.argmax(root, -1)).mean() > 0.2   # the noise is there
    if Th == 0:
        assert np.array_equal(r['bits'], (chroma[..., 1] > chroma[..., 0]).astype(np.int64)) and (r['step_logq'][:, 1] == 0).all()
    assert not r['step_forced'].any() and not r['step_err'].any()


@pytest.mark.parametrize('t', [0, 7])
@pytest.mark.parametrize('B', [1, 3, 17, 70])
def test_shapes(B, t):
    """a partial DPP group's wave (B = 1, 3), a row count that is no multiple of the four samples of a wave (17), two workgroups with the
    last partly filled (70); with and without the token output (the last step has none)"""
    root, chroma, bass = logits(B, 10 + B)
    nz = CS.noise(SEED, DRAW, 40 + np.arange(B), t)
    want = CS.decide(root, chroma, bass, nz, 1.0, 0.7)
    skip = CS.skippable(root, chroma, bass, nz, 1.0, 0.7)
    r = decide(root, chroma, bass, t, block(1.0, 0.7, 40))
    explained(r, want, skip, 'B = %d, t = %d' % (B, t), cap=False)          # (too few decisions for a share; the cap is the test above)
    r2 = decide(root, chroma, bass, t, block(1.0, 0.7, 40), want_tok=False)
    assert all(np.array_equal(r[k], r2[k]) for k in r if k != 'tok')
    plain = decide(root, chroma, bass, t)
    ref = CS.decide(root, chroma, bass, None, 0, 0)
    assert all(np.array_equal(plain[k], ref[k]) for k in ('root', 'bits', 'bass'))
    check_logprob('shapes B=%d t=%d' % (B, t), root, chroma, bass, r, 1.0, 0.7, True)


def keep_case(B, seed):
    """keep_c [B, 8, 36] of valid chords with planted invalid blocks; row 1: root block all zero, row 2: bass block with two ones, row 3: both
    invalid, row 4: odd non-zero values"""
    rng = np.random.RandomState(seed)
    kr, kb, kbits = rng.randint(0, 12, (B, 8)), rng.randint(0, 12, (B, 8)), rng.randint(0, 2, (B, 8, 12))
    keep_c, _ = CS.tokens(kr, kbits, kb)
    keep_c = keep_c.copy()
    keep_c[1, :, 0:12] = 0
    keep_c[2, :, 24:36] = 0
    keep_c[2, :, [25, 30]] = 1
    keep_c[3, :, 0:12] = 1
    keep_c[3, :, 24:36] = 0
    keep_c[4][keep_c[4] != 0] = -2.5
    return keep_c


@pytest.mark.parametrize('rows', ['per-row', 'one-row'])
def test_kept_chords(rows):
    B, Tc, Th = 17, 1.0, 0.7
    root, chroma, bass = logits(B, 21, scale=40.0)           # decisive logits: a forced decision must ignore them
    keep_c = keep_case(B, 22)
    if rows == 'per-row':
        steps = ((np.arange(B)[:, None] + np.arange(8)[None, :]) % 3 != 0).astype(np.uint8)
    else:
        steps = np.array([[1, 0, 1, 1, 0, 0, 1, 0]], np.uint8)
    kept_all = np.broadcast_to(steps.astype(bool), (B, 8))
    poisoned = keep_c.copy()
    poisoned[~kept_all] = np.nan                             # a step that is not kept is never read
    for t in (0, 1, 6):
        kept = kept_all[:, t]
        nz = CS.noise(SEED, DRAW, np.arange(B), t)
        want = CS.decide(root, chroma, bass, nz, Tc, Th, keep_c[:, t], kept)
        r = decide(root, chroma, bass, t, block(Tc, Th), poisoned, steps)
        assert np.array_equal(r['step_forced'], want['forced']) and np.array_equal(r['step_err'], want['err'])
        skip = CS.skippable(root, chroma, bass, nz, Tc, Th)
        free = want['forced'] == 0
        skip = (skip[0] & free[:, 0], skip[1] & free[:, 1:2], skip[2] & free[:, 2])   # a forced decision is never skipped
        explained(r, want, skip, '%s t = %d' % (rows, t), cap=False)
        if kept[0]:
            assert r['step_forced'][0].tolist() == [1, 12, 1] and r['step_err'][0] == 0
        for b, (f, e) in ((1, ([0, 12, 1], 1)), (2, ([1, 12, 0], 1)), (3, ([0, 12, 0], 1)), (4, ([1, 12, 1], 0))):
            assert r['step_forced'][b].tolist() == (f if kept[b] else [0, 0, 0]) and r['step_err'][b] == (e if kept[b] else 0)
        if kept[4]:
            assert np.array_equal(r['c'][4], (keep_c[4, t] != 0).astype(np.float32))
        # forced decisions do not see logits or noise: other logits, another draw, the same forced part
        r2 = decide(-root, -chroma, -bass, t, FF_.sampling_block(DEV, 3.0, 3.0, seed=5, draw=9), poisoned, steps)
        fr, fb = want['forced'][:, 0] == 1, want['forced'][:, 2] == 1
        assert np.array_equal(r2['root'][fr], r['root'][fr]) and np.array_equal(r2['bass'][fb], r['bass'][fb])
        assert np.array_equal(r2['bits'][kept], r['bits'][kept]) and np.array_equal(r2['step_forced'], r['step_forced'])
        check_logprob('keep %s t=%d' % (rows, t), root / 20, chroma / 20, bass / 20,
                      decide(root / 20, chroma / 20, bass / 20, t, block(Tc, Th), poisoned, steps), Tc, Th, True)
    # without a block: the kept argmax
    r = decide(root, chroma, bass, 2, None, poisoned, steps)
    want = CS.decide(root, chroma, bass, None, 0, 0, keep_c[:, 2], kept_all[:, 2])
    assert all(np.array_equal(r[k], want[k]) for k in ('root', 'bits', 'bass')) and np.array_equal(r['step_forced'], want['forced'])


@pytest.mark.parametrize('Tc,Th,sampled', [(1.3, 0.7, True), (1.0, 0.0, True), (0.0, 0.5, True), (0.0, 0.0, False)])
def test_logp_and_logq(Tc, Th, sampled):
    """plain rows, rows shifted by +-300 (the softmax must subtract the maximum), all-equal rows and rows with one dominant class"""
    B, t = 70, 4
    root, chroma, bass = logits(B, 31, scale=3.0)
    k = np.arange(B) % 5
    for a in (root, chroma, bass):
        a[k == 1] += np.float32(300)
        a[k == 2] -= np.float32(300)
        a[k == 3] = np.float32(1.5)
    root[k == 4, 7] += np.float32(60)
    chroma[k == 4, :, 1] += np.float32(60)
    r = decide(root, chroma, bass, t, block(Tc, Th, 7) if sampled else None)
    check_logprob('T=(%g,%g)%s' % (Tc, Th, '' if sampled else ' no block'), root, chroma, bass, r, Tc, Th, sampled)
    assert (r['step_logp'] <= 0).all() and (r['step_logq'] <= 0).all()


def test_fold_is_the_sequential_sum_bit_for_bit():
    B = 70
    rng = np.random.RandomState(41)
    sp, sq = rng.normal(-5, 30, (B, 8, 3)).astype(np.float32), rng.normal(-2, 1e-3, (B, 8, 3)).astype(np.float32)
    sf = rng.randint(0, 13, (B, 8, 3)).astype(np.int32)
    se = (rng.rand(B, 8) < 0.1).astype(np.int32) * rng.randint(1, 4, (B, 8)).astype(np.int32)
    lp, lq = (torch.full((B + GUARD, 3), float(SENT_F), device=DEV) for _ in range(2))
    f, e = torch.full((B + GUARD, 3), SENT_I, device=DEV, dtype=torch.int32), torch.full((B + GUARD,), SENT_I, device=DEV, dtype=torch.int32)
    args = [dev(sp), dev(sq), dev(sf), dev(se)]
    assert lib().ptv_chord_logprob_fold(*(ptr(a) for a in args), B, ptr(lp), ptr(lq), ptr(f), ptr(e), stream_ptr()) == 0
    r_lp, r_lq, r_f, r_e = CS.fold(sp, sq, sf, se)
    assert host(lp)[:B].tobytes() == r_lp.tobytes() and host(lq)[:B].tobytes() == r_lq.tobytes()
    assert np.array_equal(host(f)[:B], r_f) and np.array_equal(host(e)[:B], r_e) and r_e.any()
    assert (host(lp)[B:] == SENT_F).all() and (host(lq)[B:] == SENT_F).all() and (host(f)[B:] == SENT_I).all() and (host(e)[B:] == SENT_I).all()
    assert lib().ptv_chord_logprob_fold(*(ptr(a) for a in args), 0, ptr(lp), ptr(lq), ptr(f), ptr(e), stream_ptr()) == -1
    assert lib().ptv_chord_logprob_fold(None, *(ptr(a) for a in args[1:]), B, ptr(lp), ptr(lq), ptr(f), ptr(e), stream_ptr()) == -1


def test_bad_arguments_are_refused_before_any_launch():
    root, chroma, bass = logits(5, 51)
    keep_c = keep_case(5, 52)
    steps5, steps2 = np.ones((5, 8), np.uint8), np.ones((2, 8), np.uint8)
    assert decide(root, chroma, bass, 8, expect=-1) == -1
    assert decide(root, chroma, bass, -1, expect=-1) == -1
    assert decide(root, chroma, bass, 0, None, keep_c, None, expect=-1) == -1              # a keep without its steps
    assert decide(root, chroma, bass, 0, None, keep_c, steps2, expect=-1) == -1            # two step rows for five samples
    assert decide(root[:0], chroma[:0], bass[:0], 0, expect=-1) == -1                      # B = 0
    assert isinstance(decide(root, chroma, bass, 0, None, keep_c, steps5), dict)
    assert isinstance(decide(root, chroma, bass, 0, None, None, steps5), dict)             # steps without a keep: no keep
