"""CPU guard of tests/gemm_ref.py, the oracle of tests/test_gpu_gemm_kernels.py: the float64 product against torch's float64 matmul and
exp, the bf16 rounding against torch's `.to(torch.bfloat16)`, the column-blocked layout against its index formula, the dead rows
against the sentence of include/ptvae_hip.h -- and, over the WHOLE parameter list of the GPU file, the precondition that makes its
bit-for-bit comparison legitimate: operands of integers whose every partial sum, bias and C0 included, stays below 2^23 in
magnitude (so any order of fp32 additions is exact, alpha = 0.5 included), and a result that fp32 (and, where C is bf16, its one RNE
rounding) represents as the reference computes it.  The same walk asserts that every case is on the kernel configuration it was
written for (plan(), the host mirror of gemm_dispatch)."""
import numpy as np
import pytest
import torch

import gemm_ref as R
import test_gpu_gemm_kernels as G

F4, F8 = np.float32, np.float64
LAYS = [(0, 0), (0, 1), (1, 1), (1, 0)]


def _real(rng, M, N, K, ta, tb):
    a = rng.standard_normal((K, M) if ta else (M, K)).astype(F4)
    b = rng.standard_normal((K, N) if tb else (N, K)).astype(F4)
    return a, b, rng.standard_normal(N).astype(F4), rng.standard_normal((M, N)).astype(F4)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.parametrize('ta,tb', LAYS)
@pytest.mark.parametrize('act', [0, 1])
def test_product_is_torchs_float64_product(ta, tb, act):
    rng = np.random.RandomState(3 + 2 * ta + tb)
    a, b, bias, c0 = _real(rng, 13, 9, 21, ta, tb)
    b *= F4(0.2)
    ta_, tb_ = _t(a).double(), _t(b).double()
    la = ta_.t() if ta else ta_
    lb = tb_ if tb else tb_.t()
    for use_bias in (False, True):
        for acc in (False, True):
            for alpha in R.ALPHAS:
                v = alpha * (la @ lb)
                if use_bias:
                    v = v + _t(bias).double()
                if act:
                    v = torch.exp(v)
                if acc:
                    v = v + _t(c0).double()
                got = R.product(a, b, ta, tb, bias if use_bias else None, alpha, act, c0 if acc else None, acc)
                assert got.dtype == F8 and np.allclose(got, v.numpy(), rtol=1e-13, atol=1e-13)


def test_bf16_round_is_torchs_rne_conversion():
    rng = np.random.RandomState(5)
    a = (rng.standard_normal(20000) * np.exp2(rng.uniform(-20, 20, 20000))).astype(F4)
    u = a.view(np.uint32)
    u[:5000] = (u[:5000] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)               # exact ties, both parities of the lower neighbour
    assert set(((u[:5000] >> 16) & 1).tolist()) == {0, 1}
    want = _t(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(R.bf16_round(a).view(np.uint32), want.view(np.uint32))
    assert R.is_bf16(want) and not R.is_bf16(a)
    t = G.tie_matrix(np.random.RandomState(1), 40, 30)
    assert np.array_equal(R.bf16_round(t), _t(t).to(torch.bfloat16).float().numpy())


@pytest.mark.parametrize('ta,tb', LAYS)
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_kp_product_is_torchs_float32_product_of_the_rounded_operands(ta, tb, prec):
    rng = np.random.RandomState(11 + 2 * ta + tb)
    a, b, bias, c0 = _real(rng, 13, 12, 40, ta, tb)
    b *= F4(0.15)
    rnd = (lambda x: x.to(torch.bfloat16).float()) if prec == 'bf16' else (lambda x: x)
    la = rnd(_t(a).t() if ta else _t(a))
    lb = rnd(_t(b) if tb else _t(b).t())
    for cbf in ((False, True) if prec == 'bf16' else (False,)):
        for act in (0, 1):
            for acc in (False, True):
                v = torch.tensor(0.5) * (la @ lb) + _t(bias)
                if act:
                    v = torch.exp(v)
                c0_ = R.bf16_round(c0) if cbf else c0
                if acc:
                    v = v + _t(c0_)
                if cbf:
                    v = v.to(torch.bfloat16).float()
                got = R.kp_product(a, b, ta, tb, bias, 0.5, act, c0_ if acc else None, acc, prec, cbf)
                assert got.dtype == F4
                # (two BLAS may add in different orders: a few fp32 ulps, or one bf16 ulp where a rounding flips)
                tol = 2.0 ** -7 if cbf else 1e-5
                assert np.allclose(got, v.numpy(), rtol=tol, atol=tol)
                ref = R.product(rnd(_t(a)).numpy(), rnd(_t(b)).numpy(), ta, tb, bias, 0.5, act, c0_ if acc else None, acc)
                assert np.abs(got - ref).max() <= (2.0 ** -7 if cbf else 2e-5) * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize('w', [16, 32])
def test_blocked_layout_round_trip_and_index_formula(w):
    M, N = 7, 3 * w
    c = np.arange(M * N, dtype=F4).reshape(M, N)
    b = R.to_blocked(c, w)
    assert b.shape == (N // w, M, w) and np.array_equal(R.from_blocked(b, w), c)
    flat = b.ravel()
    for m in range(M):
        for n in range(N):
            assert flat[((n // w) * M + m) * w + n % w] == c[m, n]                  # include/ptvae_hip.h, dtypes bits 3 / 4


def test_dead_rows_and_what_the_header_promises_for_them():
    assert not R.dead_rows(10).any()
    assert np.array_equal(np.flatnonzero(R.dead_rows(300, 1, 96)), np.arange(192, 300))
    assert R.dead_rows(300, -1, 96).all() and not R.dead_rows(300, 3, 96).any()
    d = R.dead_rows(8 * 256 - 40, None, 0, (0, 128, 256), 256, 3)
    for r in range(d.size):
        assert d[r] == ((r % 256) >= (0, 128, 256)[(r // 256) % 3])
    both = R.dead_rows(2008, 3, 256, (0, 128, 256), 256, 3)
    assert np.array_equal(both, d | (np.arange(2008) >= 1024))
    # the promise = the formula with a zero row of A
    rng = np.random.RandomState(2)
    a, b, bias, c0 = _real(rng, 12, 5, 6, 0, 0)
    dead = R.dead_rows(12, 1, 4)
    a[dead] = 0
    for use_bias in (False, True):
        for act in (0, 1):
            for acc in (False, True):
                bs = bias if use_bias else None
                full = R.product(a, b, 0, 0, bs, 0.5, act, c0, acc)
                assert np.array_equal(R.expected_with_dead(full, dead, bs, act, c0, acc), full)
    out = R.expected_with_dead(np.ones((12, 5)), dead, None, 0, c0, True)
    assert np.array_equal(out[dead], c0[dead].astype(F8))                           # unchanged
    assert (R.expected_with_dead(np.ones((12, 5)), dead)[dead] == 0).all()         # zero


def _all_exact_cases():
    for name, cs in G.GROUPS.items():
        for c in cs:
            yield name, c


def test_int_case_refuses_what_fp32_cannot_hold():
    rng = np.random.RandomState(0)
    with pytest.raises(AssertionError):
        R.int_case(rng, 4, 4, 2 ** 20, alpha=-2.0)                                  # 16 * 2^20 * 2 = 2^25
    assert R.exact_ok(np.full((2, 3), 4, F4), np.full((2, 3), -4, F4), 0, 0, np.full(2, 4, F4), -2.0, np.full((2, 2), 4, F4))[0] == 104.0


@pytest.mark.parametrize('group', list(G.GROUPS))
def test_every_exact_case_of_the_gpu_file_is_exact_in_fp32(group):
    for c in G.GROUPS[group]:
        G.check_plan(c)
        d = G.build_int(c)                                                          # (int_case asserts the bound)
        ta, tb = G.LAYOUTS[c['lay']]
        top, ok = R.exact_ok(d['A'], d['B'], ta, tb, d['bias'], c['alpha'], d['C0'])
        assert ok and top < 2.0 ** 23, (G.case_id(c), top)
        for k in ('A', 'B', 'bias', 'C0'):
            if d[k] is not None:
                assert d[k].dtype == F4 and np.array_equal(d[k], np.rint(d[k])) and np.abs(d[k]).max(initial=0) <= 4 and R.is_bf16(d[k])
        want = G.expected(c, d)
        assert np.array_equal(want.astype(F4).astype(F8), want), G.case_id(c)       # the float64 result is an fp32 number
        assert np.array_equal(2.0 * want, np.rint(2.0 * want))                      # (an integer or, with alpha = 0.5, a half)
        dead = G.dead_of(c)
        if dead is not None:
            assert (d['A'][dead] == 0).all() and c['lay'] in ('NT', 'NN')


def test_k_list_is_derived_from_the_constants_of_the_sources():
    """every 2*PF*BK hand-over of every kernel configuration minus 1, exact and plus 1; a K tile and a 16-byte chunk on both sides; one K
    beyond every threshold"""
    ks = set(G.k_list())
    assert G.k_list() == sorted(ks) and min(ks) == 1
    for prec, bk in G.BK.items():
        assert bk % G.CH[prec] == 0 and {bk - 1, bk, bk + 1} <= ks
        assert any(k % G.CH[prec] and k < G.CH[prec] for k in ks) and any(k % G.CH[prec] and G.CH[prec] < k < bk for k in ks)
        for pf in (1, G.PF_SMALL, G.PF_NT, G.PF_TN):
            t = 2 * pf * bk
            assert {t - 1, t, t + 1} <= ks, (prec, pf)
    assert max(ks) > 2 * max(1, G.PF_SMALL, G.PF_NT, G.PF_TN) * max(G.BK.values()) + max(G.BK.values())
    assert G.WGRAD_K > max(ks)                                   # (the TN bf16 groups of the K list stay on the generic kernel)


def test_the_gpu_parameter_list_covers_what_it_says():
    cs = [c for _, c in _all_exact_cases()]
    assert len(cs) > 1500
    assert {c['K'] for c in cs if (c['M'], c['N']) == (70, 66)} >= set(G.k_list())
    assert {(c['prec'], c['src'], c['lay']) for c in cs} == {(p, s, l) for p in G.PRECS for s in G.SRCS[p] for l in G.LAYOUTS}
    assert {G.plan(c).get('tile') for c in cs} == {64, 128, None} and any(G.plan(c)['wgrad'] for c in cs)
    assert {G.plan(c)['pf'] for c in cs if not G.plan(c)['wgrad'] and G.plan(c)['tile'] == 128} == {1, G.PF_NT, G.PF_TN}
    sp = [G.plan(c) for c in cs if c['splitk'] > 1]
    assert any(p['last'] < p['kper'] for p in sp) and any(p['splits'] < c['splitk'] for p, c in zip(sp, [c for c in cs if c['splitk'] > 1]))
    assert all(0 < p['last'] <= p['kper'] for p in sp)                              # no split is empty
    assert any(G.plan(c)['splits'] > 1 for c in cs if c['splitk'] == 0 and not G.plan(c)['wgrad'])     # the automatic split
    for c in G.REAL.values():
        G.check_plan(c)
