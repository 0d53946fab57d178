"""The weight-gradient family one call at a time -- ptv_wgrad / ptv_wgrad_cat / ptv_wgrad_batch (csrc/wgrad.hip) -- against the float64
reference of tests/wgrad_ref.py.  Every dispatch branch of the host side has a named case in wgrad_ref.CASES whose plan
tests/test_wgrad_ref_host.py pins through ptv_debug_wgrad_plan; here each case asserts the same plan on its REAL pointers before it runs,
so a failure names the path that broke.

A. exact (test_exact_*): operands, C0 and b0 of integers in [-4, 4], alpha in {1, 0.5, -2}.  Every fp32 partial sum is exact in any order
   (gemm_ref.exact_ok, asserted per case), so ordered AND atomic mode must give the float64 result bit for bit: every CASES entry over the
   four dtype combinations, accumulate, colsum_a, the LDS-DMA kernel; k_top / k_rev limits at every edge with NaN in B's dead rows;
   K segments of both period signs; ptv_wgrad_cat; fp32 sources at exact bf16 ties; one nine-job list through the four batch modes and
   as single calls, in both reduction modes.
B. real-valued (test_real_*): randn operands, one case per map, a tail, segments, the two-source form.  Only the additions round (a
   bf16 x bf16 product is exact in fp32), so per element
       |C - ref| <= (K_live + total_slabs + 4) * 2^-23 * (|alpha| * |A|^T |B| + |C0|)
   (2^-23: twice the unit roundoff, an accumulator that truncates still passes), the same form for the column sums; ordered mode gives
   the same bits twice.  Prints `WGRAD_RATIO family ratio` (pytest -s; table in profiles/LOG.md).
C. refusals leave C and colsum_a untouched.

C is a [M + 3, N + 5] array and colsum_a an [M + 7] array pre-filled with a sentinel that must survive bit for bit outside [M, N] / [M];
the padding columns of the operands hold NaN; without accumulate C starts as NaN.  Every switch a test sets is put back in a finally, and
ptv_ordered_fallbacks must not move over the module."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import wgrad_ref as W
from gemm_ref import ALPHAS
from polyphonic_chord_texture_disentanglement_amd import _lib
from polyphonic_chord_texture_disentanglement_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
F4, F8 = np.float32, np.float64
SENT = np.float32(768.0)
SENT_BITS = int(np.array(SENT).view(np.int32))
PTV_ERR_ARG = -1
RATIOS = {}
# what the finally blocks put back: the library's switches at load, from the variables csrc/wgrad.hip reads then (the ABI has no getters)
MODE0 = 0 if os.environ.get('PTV_WGRAD_ORDERED', '')[:1] == '0' else 1
DMA0 = 1 if int(os.environ.get('PTV_WGRAD_DMA', '0') or 0) else 0
BATCH0 = int(os.environ.get('PTV_WGRAD_BATCH', '3') or 3)


class switches:
    """with switches(ordered=, dma=, batch=): the three process-wide switches of the family, restored on the way out"""

    def __init__(self, ordered=1, dma=0, batch=3):
        self.v = (ordered, dma, batch)

    def __enter__(self):
        _lib.call('ptv_wgrad_mode', self.v[0])
        _lib.call('ptv_wgrad_dma', self.v[1])
        _lib.call('ptv_wgrad_batch_mode', self.v[2])

    def __exit__(self, *exc):
        try:
            torch.cuda.synchronize()
        finally:
            lib().ptv_wgrad_mode(MODE0)
            lib().ptv_wgrad_dma(DMA0)
            lib().ptv_wgrad_batch_mode(BATCH0)
        return False


@pytest.fixture(scope='module', autouse=True)
def no_ordered_fallbacks():
    """no ordered reduction of this module may have fallen back to atomics (no workspace); and the ratio table of the real-valued tests"""
    fb = lib().ptv_ordered_fallbacks(0)
    yield
    assert lib().ptv_ordered_fallbacks(0) == fb, 'an ordered weight-gradient reduction fell back to atomics'
    for k in sorted(RATIOS):
        print('WGRAD_RATIO_MAX %s %.2e' % (k, RATIOS[k]))


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


# ================================================================================================ operands on the device
def dev_operand(X, ld, off, bf):
    """host [K, W] float32 -> the view from column `off` on of a [K + 1, ld] device array that holds X in its first K rows and W columns and NaN
    everywhere else (the view is never empty, whatever K and W: an empty tensor has no address; the calls pass K and W themselves)"""
    Kd, Wd = X.shape
    assert off + Wd <= ld and off < ld
    full = np.full((Kd + 1, ld), np.nan, F4)
    full[:Kd, off:off + Wd] = X
    t = torch.from_numpy(full).to(DEV)
    if bf:
        t = t.to(BF)
    return t[:, off:]


class Problem:
    """one product: host operands (A [K, M], B [K, N], float32; an fp32 source may hold what bf16 cannot: the kernel rounds it), its live rows,
    C0 / b0, and the device arrays with their sentinels"""

    def __init__(self, M, N, K, A, B, dtypes, lda, ldb, offa=0, offb=0, alpha=1.0, accumulate=1, colsum=True, C0=None, b0=None, live=None,
                 slabs=0, k_top=None, k_unit=0, k_rev=0, seg=None):
        self.M, self.N, self.K, self.dtypes, self.alpha, self.accumulate, self.slabs = M, N, K, dtypes, alpha, accumulate, slabs
        self.live = np.ones(K, bool) if live is None else live
        self.A, self.B = np.array(A, F4), np.array(B, F4)
        assert not self.A[~self.live].any(), 'the dead rows of A are zero by contract'
        Bn = self.B.copy()
        Bn[~self.live] = np.nan                                                   # "may never have been written"
        self.C0 = np.zeros((M, N), F4) if C0 is None else np.array(C0, F4)
        self.b0 = np.zeros(M, F4) if b0 is None else np.array(b0, F4)
        self.Ad = dev_operand(self.A, lda, offa, dtypes & 1)
        self.Bd = dev_operand(Bn, ldb, offb, dtypes & 2)
        self.k_top = None if k_top is None else torch.tensor([k_top], dtype=torch.int32, device=DEV)
        self.k_unit, self.k_rev = k_unit, k_rev
        self.seg = seg
        self.seg_n = None if seg is None else torch.tensor(list(seg[1]), dtype=torch.int32, device=DEV)
        self.colsum = colsum
        self.reset()

    def reset(self):
        M, N = self.M, self.N
        c = np.full((M + 3, N + 5), SENT, F4)
        c[:M, :N] = self.C0 if self.accumulate else np.nan
        self.Cfull = torch.from_numpy(c).to(DEV)
        s = np.full(M + 7, SENT, F4)
        s[:M] = self.b0
        self.sfull = torch.from_numpy(s).to(DEV)

    # ---- the job
    def job(self):
        j = dict(M=self.M, N=self.N, K=self.K, A=self.Ad, B=self.Bd, C=self.Cfull, alpha=self.alpha,
                 accumulate=self.accumulate, slabs=self.slabs, colsum_a=self.sfull if self.colsum else None, k_top=self.k_top,
                 k_unit=self.k_unit, k_rev=self.k_rev)
        if self.seg is not None:
            j.update(seg_n=self.seg_n, seg_unit=self.seg[0], seg_period=self.seg[2])
        return j

    def single(self):
        """ptv_wgrad (K segments exist only in ptv_wgrad_job: a batch of one)"""
        if self.seg is not None:
            return _lib.wgrad_batch([self.job()])
        _lib.call('ptv_wgrad', self.M, self.N, self.K, ptr(self.Ad), self.Ad.stride(0), ptr(self.Bd), self.Bd.stride(0), ptr(self.Cfull),
                  self.Cfull.stride(0), self.alpha, self.accumulate, self.dtypes, self.slabs, ptr(self.sfull) if self.colsum else None,
                  ptr(self.k_top), self.k_unit, self.k_rev, stream_ptr())

    def plan(self):
        arr = job_array([self.job()])
        out = (ctypes.c_int * 10)()
        assert lib().ptv_debug_wgrad_plan(arr, out) == 0
        return dict(zip(W.PLAN_FIELDS, list(out)))

    # ---- the reference
    def want(self):
        return W.product(self.A, self.B, self.live, self.alpha, self.C0, self.accumulate)

    def want_sum(self):
        return W.colsum(self.A, self.live, self.b0)

    def assert_exact_ok(self):
        top, ok = W.exact_ok(self.A[self.live], self.B[self.live], 1, 1, None, self.alpha, self.C0 if self.accumulate and self.C0.size else None)
        assert ok and float(np.abs(self.A).sum(0).max(initial=0)) + float(np.abs(self.b0).max(initial=0)) < 2.0 ** 23, top

    # ---- what came out
    def result(self):
        """(C [M, N], colsum [M]) on the host, after checking that nothing outside them moved"""
        torch.cuda.synchronize()
        M, N = self.M, self.N
        c, s = self.Cfull.cpu().numpy(), self.sfull.cpu().numpy()
        cb, sb = c.view(np.int32), s.view(np.int32)
        assert (cb[:, N:] == SENT_BITS).all(), 'the pad columns of C moved'
        assert (cb[M:, :] == SENT_BITS).all(), 'the rows of C after M moved'
        assert (sb[M:] == SENT_BITS).all(), 'colsum_a moved after M'
        if not self.colsum:
            assert np.array_equal(s[:M].view(np.int32), self.b0.view(np.int32)), 'colsum_a moved although the call passed none'
        return c[:M, :N].copy(), s[:M].copy()

    def check_exact(self, what=''):
        c, s = self.result()
        want, ws = self.want(), self.want_sum()
        assert np.isfinite(c).all(), 'C is not finite (a dead row of B was read?) ' + what
        assert torch.equal(torch.from_numpy(c), torch.from_numpy(want.astype(F4))) and np.array_equal(want.astype(F4).astype(F8), want), \
            'C differs from the exact reference in %d of %d elements, max |d| %g %s' % ((c != want).sum(), c.size, np.abs(c - want).max(initial=0), what)
        if self.colsum:
            assert torch.equal(torch.from_numpy(s), torch.from_numpy(ws.astype(F4))), \
                'colsum_a differs from the exact reference in %d of %d elements %s' % ((s != ws).sum(), s.size, what)


def job_array(jobs):
    """dicts with the fields of ptv_wgrad_job -> the ctypes array _lib.wgrad_batch would build (for calls whose status is the point)"""
    arr = (_lib.WgradJob * max(1, len(jobs)))()
    for q, j in zip(arr, jobs):
        A, B, C = j['A'], j['B'], j['C']
        q.M, q.N, q.K = j['M'], j['N'], j['K']
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), C.stride(0)
        q.alpha, q.accumulate, q.slabs = j.get('alpha', 1.0), j.get('accumulate', 1), j.get('slabs', 0)
        q.dtypes = (1 if A.dtype == BF else 0) | (2 if B.dtype == BF else 0)
        q.colsum_a, q.k_top = ptr(j.get('colsum_a')), ptr(j.get('k_top'))
        q.k_unit, q.k_rev = j.get('k_unit', 0), j.get('k_rev', 0)
        q.seg_n, q.seg_unit, q.seg_period = ptr(j.get('seg_n')), j.get('seg_unit', 0), j.get('seg_period', 0)
    return arr


def ints(rng, *shape):
    return rng.randint(-4, 5, shape).astype(F4)


def case_problem(name, dtypes, alpha=1.0, accumulate=1, colsum=True, real=False, k_top=None, k_unit=0, k_rev=0, period_sign=1, seg_full=False,
                 key=()):
    """a CASES entry as a Problem: integer operands (exact) or randn ones (real: rounded to bf16 where the device dtype is bf16); the rows
    the limits / segments declare dead are zero in A"""
    c = W.CASES[name]
    M, N, K = c['M'], c['N'], c['K']
    rng = np.random.RandomState(seed_of(name, dtypes, key))
    seg = None
    if c['seg']:
        unit, n, period = c['seg']
        seg = (unit, tuple(unit for _ in n) if seg_full else n, period * period_sign)
    live = W.live_rows(K, k_top, k_unit, k_rev, *((c['seg'][1], c['seg'][0], c['seg'][2] * period_sign) if c['seg'] else (None, 0, 0)))
    if real:
        A, B = rng.standard_normal((K, M)).astype(F4), rng.standard_normal((K, N)).astype(F4)
        A = W.bf16_round(A) if dtypes & 1 else A
        B = W.bf16_round(B) if dtypes & 2 else B
        C0, b0 = rng.standard_normal((M, N)).astype(F4), rng.standard_normal(M).astype(F4)
    else:
        A, B, C0, b0 = ints(rng, K, M), ints(rng, K, N), ints(rng, M, N), ints(rng, M)
    A[~live] = 0
    return Problem(M, N, K, A, B, dtypes, c['lda'], c['ldb'], c['offa'], c['offb'], alpha, accumulate, colsum, C0, b0, live, c['slabs'],
                   k_top, k_unit, k_rev, seg)


def assert_plan(name, p):
    got = p.plan()
    assert got == W.CASES[name]['expect'], 'case %s left the branch it is named after: plan %r' % (name, got)
    return got


# ================================================================================================ A. exact: every case of the census
def _grid():
    out = []
    for name in W.CASES:
        h = seed_of(name)
        for dtypes in range(4):
            i = dtypes ^ (h & 3)
            for ordered in (1, 0):
                out.append(pytest.param(name, dtypes, i & 1, (i >> 1) & 1, ALPHAS[(dtypes + h) % 3], ordered, 0,
                                        id='%s-dt%d-%s' % (name, dtypes, 'ord' if ordered else 'atom')))
        if W.CASES[name]['expect']['kfast'] > 0:                                 # the LDS-DMA kernel: bf16 x bf16, the unguarded launch
            for ordered in (1, 0):
                out.append(pytest.param(name, 3, ordered, 1, ALPHAS[h % 3], ordered, 1, id='%s-dma-%s' % (name, 'ord' if ordered else 'atom')))
    return out


@pytest.mark.parametrize('name,dtypes,acc,colsum,alpha,ordered,dma', _grid())
def test_exact_every_case_equals_the_integer_reference(name, dtypes, acc, colsum, alpha, ordered, dma):
    p = case_problem(name, dtypes, alpha, acc, bool(colsum))
    p.assert_exact_ok()
    assert_plan(name, p)
    with switches(ordered=ordered, dma=dma):
        p.single()
        p.check_exact()
        if p.seg is not None:                                                     # the other period sign: the units in reversed order
            q = case_problem(name, dtypes, alpha, acc, bool(colsum), period_sign=-1)
            q.single()
            q.check_exact('(negative period)')


# ================================================================================================ limits
LIMIT_CASES = ('map0_explicit3', 'map1_beyond_k', 'map2_over_map1', 'tail32', 'tail22', 'tail_multi', 'tail_only', 'unaligned_3', 'one_slab')


def limit_values(name):
    """k_top over units of 32 rows: nothing, the first unit, a slab boundary, inside a slab, the last unit, beyond it -- and the two on either
    side of the guarded tail's first row (behind a fast launch the tail is at most 32 rows and a limit is a multiple of 32: a limit "inside
    the tail" can only be its first row -- the tail dead, or with k_rev the tail alone alive -- or beyond it; the all-guarded launch of
    unaligned operands also gets limits strictly inside its slabs)"""
    c = W.CASES[name]
    e = c['expect']
    units = W.cdiv(c['K'], 32)
    kper = (e['kper_fast'] or e['kper_tail']) // 32
    v = {-1, 0, kper - 1, kper, units - 1, units + 3}
    if 0 < e['kfast'] < c['K']:
        v |= {e['kfast'] // 32 - 1, e['kfast'] // 32}
    if e['kfast'] == 0 and e['nslab_tail'] > 1:
        v |= {kper + 1, 2 * kper}                                                  # inside the all-guarded launch's second and third slab
    return sorted(x for x in v if x >= -1)


@pytest.mark.parametrize('rev', [0, 1])
@pytest.mark.parametrize('name', LIMIT_CASES)
def test_exact_limits_at_every_edge_with_nan_in_the_dead_rows_of_b(name, rev):
    c = W.CASES[name]
    units = W.cdiv(c['K'], 32)
    for n, kt in enumerate(limit_values(name)):
        for ordered in (1, 0):
            dtypes, acc = (n + 2 * rev + ordered) & 3, (n + ordered) & 1
            p = case_problem(name, dtypes, ALPHAS[n % 3], acc, True, k_top=kt, k_unit=32, k_rev=units if rev else 0, key=('lim', kt, rev))
            p.assert_exact_ok()
            assert_plan(name, p)
            what = '(k_top %d of %d units, k_rev %d, %s, dtypes %d, accumulate %d)' % (kt, units, p.k_rev, 'ordered' if ordered else 'atomic', dtypes, acc)
            if kt == -1 or kt >= units - 1:
                assert p.live.sum() == (0 if kt == -1 else c['K']), what
            with switches(ordered=ordered):
                p.single()
                p.check_exact(what)
                if kt == -1:
                    cgot, sgot = p.result()
                    assert np.array_equal(cgot, p.C0 if acc else np.zeros_like(p.C0)) and np.array_equal(sgot, p.b0), what


# ================================================================================================ K segments
@pytest.mark.parametrize('sign', [1, -1])
@pytest.mark.parametrize('name', W.SEG_CASES)
def test_exact_segments_with_a_limit_on_top_and_against_full_segments(name, sign):
    c = W.CASES[name]
    unit = c['seg'][0]
    units = c['K'] // unit
    for n, (kt, rev) in enumerate(((None, 0), (units // 2, 0), (units // 2 - 1, units), (0, 0))):
        for ordered in (1, 0):
            dtypes = (n + ordered + (sign > 0)) & 3
            kw = dict(k_top=kt, k_unit=unit if kt is not None else 0, k_rev=rev, period_sign=sign, key=('seg', kt, rev))
            p = case_problem(name, dtypes, ALPHAS[n % 3], n & 1, True, **kw)
            p.assert_exact_ok()
            assert_plan(name, p)
            what = '(k_top %r k_rev %d period sign %d %s)' % (kt, rev, sign, 'ordered' if ordered else 'atomic')
            with switches(ordered=ordered):
                p.single()
                p.check_exact(what)


@pytest.mark.parametrize('name', W.SEG_CASES)
def test_real_full_segments_give_the_bits_of_the_clipped_call(name):
    """the header: "against the same product without segments the result is bit-identical when the skipped rows of A are zero" -- the same
    job with seg_n = seg_unit everywhere and finite numbers in B's skipped rows"""
    for sign in (1, -1):
        p = case_problem(name, 3, 0.5, 1, True, real=True, period_sign=sign)
        q = case_problem(name, 3, 0.5, 1, True, real=True, period_sign=sign, seg_full=True)
        assert np.array_equal(p.A, q.A) and np.array_equal(p.B, q.B) and p.seg[1] != q.seg[1]
        q.live = np.ones(q.K, bool)
        q.Bd = dev_operand(q.B, W.CASES[name]['ldb'], W.CASES[name]['offb'], True)      # finite everywhere
        with switches(ordered=1):
            p.single()
            q.single()
            (c1, s1), (c2, s2) = p.result(), q.result()
        assert np.array_equal(c1.view(np.int32), c2.view(np.int32)) and np.array_equal(s1.view(np.int32), s2.view(np.int32)), sign


# ================================================================================================ ptv_wgrad_cat
def cat_problem(M1, M2, N, K, dtypes, real, key):
    rng = np.random.RandomState(seed_of('cat', M1, M2, N, K, dtypes, key))
    M = M1 + M2
    if real:
        A, B = rng.standard_normal((K, M)).astype(F4), rng.standard_normal((K, N)).astype(F4)
        A = W.bf16_round(A) if dtypes & 1 else A
        B = W.bf16_round(B) if dtypes & 2 else B
        C0, b0 = rng.standard_normal((M, N)).astype(F4), rng.standard_normal(M).astype(F4)
    else:
        A, B, C0, b0 = ints(rng, K, M), ints(rng, K, N), ints(rng, M, N), ints(rng, M)
    p = Problem(M, N, K, A, B, dtypes, W.ceil8(M), W.ceil8(N) + 8, alpha=0.5, C0=C0, b0=b0)
    p.A1d = dev_operand(A[:, :M1], M1 + 8, 0, dtypes & 1)                        # lda1 != lda2
    p.A2d = dev_operand(A[:, M1:], W.ceil8(M2) + 24, 0, dtypes & 1)
    assert p.A1d.stride(0) != p.A2d.stride(0)
    return p


def run_cat(p, M1, M2, slabs=0):
    _lib.call('ptv_wgrad_cat', M1, ptr(p.A1d), p.A1d.stride(0), M2, ptr(p.A2d), p.A2d.stride(0), p.N, p.K, ptr(p.Bd), p.Bd.stride(0),
              ptr(p.Cfull), p.Cfull.stride(0), p.alpha, p.accumulate, p.dtypes, slabs, ptr(p.sfull), None, 0, 0, stream_ptr())


def run_cat_as_two(p, M1, M2, slabs=0):
    for A_, lo, hi in ((p.A1d, 0, M1), (p.A2d, M1, M1 + M2)):
        _lib.call('ptv_wgrad', hi - lo, p.N, p.K, ptr(A_), A_.stride(0), ptr(p.Bd), p.Bd.stride(0), ptr(p.Cfull[lo:hi]), p.Cfull.stride(0), p.alpha,
                  p.accumulate, p.dtypes, slabs, ptr(p.sfull[lo:hi]), None, 0, 0, stream_ptr())


@pytest.mark.parametrize('K', [1024, 1000])
@pytest.mark.parametrize('M2', [72, 128])
@pytest.mark.parametrize('M1', [128, 256])
def test_exact_two_source_product_equals_the_reference_and_the_two_calls(M1, M2, K):
    """the split lies on a tile-row boundary of C by contract (M1 a multiple of 128); M2 = 72 leaves the second source's last tile row partly
    outside it, K = 1000 sends its last 8 rows through the guarded launch"""
    for dtypes in (3, 0, 1, 2):
        for ordered in (1, 0):
            p = cat_problem(M1, M2, 136, K, dtypes, False, ())
            p.assert_exact_ok()
            with switches(ordered=ordered):
                run_cat(p, M1, M2)
                p.check_exact('(cat, dtypes %d)' % dtypes)
                c1, s1 = p.result()
                p.reset()
                run_cat_as_two(p, M1, M2)
                p.check_exact('(the two calls, dtypes %d)' % dtypes)
                c2, s2 = p.result()
            assert np.array_equal(c1, c2) and np.array_equal(s1, s2)


# ================================================================================================ fp32 sources at exact bf16 ties
def tie_values(rng, K, Wd):
    """[K, Wd] float32 of values exactly half way between two bf16 numbers, both parities of the lower neighbour (257 -> 256, 259 -> 260),
    both signs, one power-of-two scale per column: the sums down a column stay on one grid"""
    base = rng.choice(np.array([257.0, 259.0, 261.0, 263.0, 385.0, 387.0, 509.0, 511.0], F8), (K, Wd))
    sign = rng.choice(np.array([-1.0, 1.0]), (K, Wd))
    scale = np.exp2(rng.randint(-10, 3, Wd)).astype(F8)
    v = (base * sign * scale[None, :]).astype(F4)
    u = v.view(np.uint32)
    assert ((u & np.uint32(0xFFFF)) == np.uint32(0x8000)).all() and set(((u >> 16) & 1).ravel().tolist()) == {0, 1}
    return v, scale


@pytest.mark.parametrize('which', ['a', 'b', 'ab'])
@pytest.mark.parametrize('name', ['one_slab', 'tail22', 'unaligned_3', 'map1_explicit8'])
def test_exact_fp32_sources_round_to_nearest_even_at_ties(name, which):
    c = W.CASES[name]
    M, N, K = c['M'], c['N'], c['K']
    rng = np.random.RandomState(seed_of('tie', name, which))
    A, sa = tie_values(rng, K, M) if 'a' in which else (ints(rng, K, M), np.ones(M))
    B, sb = tie_values(rng, K, N) if 'b' in which else (ints(rng, K, N), np.ones(N))
    dtypes = {'a': 2, 'b': 1, 'ab': 0}[which]                                    # the tie side is an fp32 source, the other one bf16
    Ar, Br = W.bf16_round(A), W.bf16_round(B)
    assert (Ar != A).all() if 'a' in which else np.array_equal(Ar, A)
    # exactness: every partial sum is an integer multiple of its column's grid and below 2^24 grid steps
    grid = (4.0 * sa if 'a' in which else sa)[:, None] * (4.0 * sb if 'b' in which else sb)[None, :]
    assert (W.abs_product(Ar, Br) / grid).max() < 2.0 ** 24 and (np.abs(Ar.astype(F8)).sum(0) / (4.0 * sa if 'a' in which else sa)).max() < 2.0 ** 24
    for ordered in (1, 0):
        p = Problem(M, N, K, A, B, dtypes, c['lda'], c['ldb'], c['offa'], c['offb'], 1.0, 0, True, slabs=c['slabs'])
        p.A, p.B = Ar, Br                                                         # the reference sees what RNE makes of the sources
        assert_plan(name, p)
        with switches(ordered=ordered):
            p.single()
            p.check_exact('(ties in %s, %s)' % (which, 'ordered' if ordered else 'atomic'))


# ================================================================================================ the batch
BIG = dict(M=256, N=512, K=4096, slabs=24)                                       # 8 tiles x 22 slabs = 176 blocks: launched alone in mode 3


def batch_problems(key):
    """nine jobs = two tables of the batched launch: mixed dtypes, a fast + tail product with a one-slab fast part and one with four slabs,
    a product of more than 160 blocks, a single slab, K segments, a limit, K = 0 without accumulate (must zero C), M = 0"""
    ps = [case_problem('tail32', 3, 1.0, 1, True, key=key),
          None,
          case_problem('tail_multi', 2, 0.5, 0, True, key=key),
          None,
          case_problem('one_slab', 1, -2.0, 1, True, key=key),
          case_problem('seg_map1_9to16', 3, 1.0, 0, True, key=key),
          None,
          case_problem('map0_explicit3', 0, 0.5, 1, True, k_top=11, k_unit=32, key=key),
          case_problem('map2_auto', 3, -2.0, 1, False, key=key)]
    rng = np.random.RandomState(seed_of('batch', key))
    b = BIG
    ps[1] = Problem(b['M'], b['N'], b['K'], ints(rng, b['K'], b['M']), ints(rng, b['K'], b['N']), 3, b['M'], b['N'], alpha=1.0, accumulate=1,
                    C0=ints(rng, b['M'], b['N']), b0=ints(rng, b['M']), slabs=b['slabs'])
    ps[3] = Problem(128, 136, 0, np.zeros((0, 128), F4), np.zeros((0, 136), F4), 3, 128, 136, accumulate=0, b0=ints(rng, 128))
    ps[6] = Problem(0, 128, 64, np.zeros((64, 0), F4), ints(rng, 64, 128), 3, 8, 128)
    return ps


@pytest.mark.parametrize('ordered', [1, 0], ids=['ord', 'atom'])
@pytest.mark.parametrize('route', ['single', 'mode0', 'mode1', 'mode2', 'mode3'])
def test_exact_batch_every_route_gives_the_reference(route, ordered):
    """one job list under ptv_wgrad_batch_mode 0-3 and as single calls.  Atomic mode with mode 1 (and mode 3: these products are small) puts
    the one-slab guarded tail of `tail32` into the SAME launch as its fast part, both without a workspace: the tail may add into C with a
    plain read-modify-write only if it is the product's sole writer (wgrad_store)."""
    ps = batch_problems(('b',))
    for p in ps:
        p.assert_exact_ok()
    pl = ps[1].plan()
    assert pl['tiles_m'] * pl['tiles_n'] * pl['total_slabs'] > 160 and pl['map_fast'] == 2
    t32 = ps[0].plan()
    assert (t32['nslab_fast'], t32['nslab_tail']) == (1, 1) and ps[2].plan()['nslab_fast'] == 4
    with switches(ordered=ordered, batch=int(route[-1]) if route != 'single' else 3):
        if route == 'single':
            for p in ps:
                p.single()
        else:
            _lib.wgrad_batch([p.job() for p in ps])
        for n, p in enumerate(ps):
            p.check_exact('(job %d, %s, %s)' % (n, route, 'ordered' if ordered else 'atomic'))
    c3, s3 = ps[3].result()
    assert (c3 == 0).all() and np.array_equal(s3, ps[3].b0)                       # K = 0 without accumulate: C zeroed, no sums added


def test_batch_refuses_more_than_64_jobs_and_takes_none():
    p = case_problem('one_slab', 3)
    before = p.Cfull.clone(), p.sfull.clone()
    arr = job_array([p.job()] * 65)
    assert lib().ptv_wgrad_batch(arr, 65, stream_ptr()) == PTV_ERR_ARG
    assert lib().ptv_wgrad_batch(arr, -1, stream_ptr()) == PTV_ERR_ARG
    assert lib().ptv_wgrad_batch(None, 1, stream_ptr()) == PTV_ERR_ARG
    assert lib().ptv_wgrad_batch(arr, 0, stream_ptr()) == 0 and lib().ptv_wgrad_batch(None, 0, stream_ptr()) == 0
    _lib.wgrad_batch([])
    torch.cuda.synchronize()
    assert torch.equal(p.Cfull.view(torch.int32), before[0].view(torch.int32)) and torch.equal(p.sfull.view(torch.int32), before[1].view(torch.int32))


# ================================================================================================ B. real-valued
REAL_CASES = ('map0_explicit3', 'map1_beyond_k', 'map2_auto', 'map1_deep_k', 'tail_multi', 'unaligned_auto', 'seg_unit384', 'seg_tail_live')
U = 2.0 ** -23


def check_bound(p, c, s, total_slabs, family):
    """|C - ref| <= (K_live + total_slabs + 4) * 2^-23 * (|alpha| |A|^T |B| + |C0|), evaluated in float64; the same form for the sums.
    Derivation: bf16 x bf16 products are exact in fp32; a sum of K_live of them in any order and any grouping into slabs carries at most
    K_live - 1 roundings of relative size 2^-24 each on partial sums bounded by |A|^T |B|; adding the slabs costs total_slabs - 1 more, alpha
    and the add into C one each (to first order; the factor 2 between 2^-24 and 2^-23 and the + 4 cover the higher orders)."""
    Ar = W.bf16_round(p.A).astype(F8)
    Br = W.bf16_round(np.nan_to_num(p.B)).astype(F8)
    ref = W.product(Ar, Br, p.live, p.alpha, p.C0, p.accumulate)
    n = int(p.live.sum()) + total_slabs + 4
    bound = n * U * (abs(p.alpha) * W.abs_product(Ar, Br, p.live) + (np.abs(p.C0.astype(F8)) if p.accumulate else 0.0))
    err = np.abs(c.astype(F8) - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max(initial=0))
    rs = 0.0
    if p.colsum:
        refs = W.colsum(Ar, p.live, p.b0)
        bs = n * U * (np.abs(Ar[p.live]).sum(0) + np.abs(p.b0.astype(F8)))
        rs = float((np.abs(s.astype(F8) - refs) / np.maximum(bs, 1e-300)).max(initial=0))
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    RATIOS[family + '/colsum'] = max(RATIOS.get(family + '/colsum', 0.0), rs)
    print('WGRAD_RATIO %s C %.2e colsum %.2e' % (family, ratio, rs))
    assert np.isfinite(c).all() and ratio <= 1.0 and rs <= 1.0, (family, ratio, rs)


@pytest.mark.parametrize('dtypes', [3, 0, 1, 2])
@pytest.mark.parametrize('name', REAL_CASES)
def test_real_within_the_derived_bound_and_the_same_bits_twice(name, dtypes):
    p = case_problem(name, dtypes, 0.5, 1, True, real=True)
    total = assert_plan(name, p)['total_slabs']
    with switches(ordered=1):
        p.single()
        c1, s1 = p.result()
        check_bound(p, c1, s1, total, name + '/ordered')
        p.reset()
        p.single()
        c2, s2 = p.result()
    assert np.array_equal(c1.view(np.int32), c2.view(np.int32)) and np.array_equal(s1.view(np.int32), s2.view(np.int32)), \
        'two ordered calls gave different bits'
    p.reset()
    with switches(ordered=0):
        p.single()
        c3, s3 = p.result()
        check_bound(p, c3, s3, total, name + '/atomic')
    if dtypes == 3 and W.CASES[name]['expect']['kfast'] > 0:
        p.reset()
        with switches(ordered=1, dma=1):
            p.single()
            c4, s4 = p.result()
            check_bound(p, c4, s4, total, name + '/dma')


@pytest.mark.parametrize('dtypes', [3, 0])
def test_real_two_source_product_within_the_bound_and_equal_to_the_two_calls(dtypes):
    M1, M2, N, K = 256, 72, 136, 2000
    p = cat_problem(M1, M2, N, K, dtypes, True, ())
    q = Problem(M1 + M2, N, K, p.A, p.B, dtypes, W.ceil8(M1 + M2), W.ceil8(N) + 8, slabs=4)   # (explicit slabs: the two single calls plan alike)
    total = q.plan()['total_slabs']                                               # (the one-array job of the same shape: the same plan)
    with switches(ordered=1):
        run_cat(p, M1, M2, 4)
        c1, s1 = p.result()
        check_bound(p, c1, s1, total, 'cat/ordered')
        p.reset()
        run_cat(p, M1, M2, 4)
        c2, s2 = p.result()
        p.reset()
        run_cat_as_two(p, M1, M2, 4)
        c3, s3 = p.result()
    assert np.array_equal(c1.view(np.int32), c2.view(np.int32)) and np.array_equal(s1.view(np.int32), s2.view(np.int32))
    assert np.array_equal(c1.view(np.int32), c3.view(np.int32)) and np.array_equal(s1.view(np.int32), s3.view(np.int32))
    p.reset()
    with switches(ordered=0):
        run_cat(p, M1, M2, 4)
        c4, s4 = p.result()
        check_bound(p, c4, s4, total, 'cat/atomic')


def test_real_batch_modes_give_the_bits_of_the_single_calls():
    """"same bits in every mode": the job list of the exact test with real numbers, ordered reduction"""
    def real_list():
        ps = [case_problem(n, dt, al, acc, cs, real=True, key=('rb',), **kw) for n, dt, al, acc, cs, kw in (
            ('tail32', 3, 1.0, 1, True, {}), ('tail_multi', 2, 0.5, 0, True, {}), ('one_slab', 1, -2.0, 1, True, {}),
            ('seg_map1_9to16', 3, 1.0, 0, True, {}), ('map0_explicit3', 0, 0.5, 1, True, dict(k_top=11, k_unit=32)),
            ('map2_auto', 3, -2.0, 1, False, {}), ('narrow_200x135', 0, 1.0, 1, True, {}), ('seg_tail_live', 3, 1.0, 1, True, {}),
            ('map2_over_map1', 3, 1.0, 1, True, {}))]
        return ps
    outs = {}
    for route in ('single', 0, 1, 2, 3):
        ps = real_list()
        with switches(ordered=1, batch=route if route != 'single' else 3):
            if route == 'single':
                for p in ps:
                    p.single()
            else:
                _lib.wgrad_batch([p.job() for p in ps])
            outs[route] = [p.result() for p in ps]
    for route in (0, 1, 2, 3):
        for n, ((c, s), (c0, s0)) in enumerate(zip(outs[route], outs['single'])):
            assert np.array_equal(c.view(np.int32), c0.view(np.int32)) and np.array_equal(s.view(np.int32), s0.view(np.int32)), (route, n)


# ================================================================================================ C. refusals
def _untouched(p, before):
    torch.cuda.synchronize()
    return torch.equal(p.Cfull.view(torch.int32), before[0].view(torch.int32)) and torch.equal(p.sfull.view(torch.int32), before[1].view(torch.int32))


def test_refusals_return_err_arg_and_leave_the_outputs_untouched():
    p = case_problem('map0_explicit3', 3)
    s = case_problem('seg_map0', 3)
    kt = torch.tensor([1], dtype=torch.int32, device=DEV)
    for q in (p, s):
        q.before = q.Cfull.clone(), q.sfull.clone()

    def single(**over):
        a = dict(M=p.M, N=p.N, K=p.K, A=ptr(p.Ad), B=ptr(p.Bd), C=ptr(p.Cfull), k_top=None, k_unit=0)
        a.update(over)
        return lib().ptv_wgrad(a['M'], a['N'], a['K'], a['A'], p.Ad.stride(0), a['B'], p.Bd.stride(0), a['C'], p.Cfull.stride(0), 1.0, 1, 3, 0,
                               ptr(p.sfull), a['k_top'], a['k_unit'], 0, stream_ptr())

    def batch(q, **over):
        arr = job_array([q.job()])
        for k, v in over.items():
            setattr(arr[0], k, v)
        return lib().ptv_wgrad_batch(arr, 1, stream_ptr())

    assert single(k_top=ptr(kt), k_unit=48) == PTV_ERR_ARG                       # k_unit no multiple of 32 with k_top set
    assert single(k_top=ptr(kt), k_unit=0) == PTV_ERR_ARG
    for nul in ('A', 'B', 'C'):
        assert single(**{nul: None}) == PTV_ERR_ARG                                # a null operand
        assert batch(p, **{nul: None}) == PTV_ERR_ARG
    for neg in ('M', 'N', 'K'):
        assert single(**{neg: -1}) == PTV_ERR_ARG                                  # negative sizes
        assert batch(p, **{neg: -1}) == PTV_ERR_ARG
    assert batch(p, k_top=ptr(kt), k_unit=48) == PTV_ERR_ARG
    assert _untouched(p, p.before)
    assert batch(s, seg_period=0) == PTV_ERR_ARG                                 # a seg job without a period
    assert batch(s, seg_unit=64) == PTV_ERR_ARG                                  # unsupported units
    assert batch(s, seg_unit=128 * 129, K=2 * 128 * 129) == PTV_ERR_ARG           # 258 slabs of 128 rows (refused on the host, nothing is read)
    assert batch(s, seg_unit=384) == PTV_ERR_ARG
    assert _untouched(s, s.before)
    # a refused job refuses the whole call: nothing of the good job in front of it runs
    arr = job_array([p.job(), s.job()])
    arr[1].seg_period = 0
    assert lib().ptv_wgrad_batch(arr, 2, stream_ptr()) == PTV_ERR_ARG
    assert _untouched(p, p.before) and _untouched(s, s.before)
    # ptv_wgrad_cat: M1 no multiple of 128, a null second source
    c = cat_problem(128, 72, 136, 256, 3, False, ())
    c.before = c.Cfull.clone(), c.sfull.clone()

    def cat(M1, A2):
        return lib().ptv_wgrad_cat(M1, ptr(c.A1d), c.A1d.stride(0), 200 - M1, A2, c.A2d.stride(0), c.N, c.K, ptr(c.Bd), c.Bd.stride(0), ptr(c.Cfull),
                                   c.Cfull.stride(0), 1.0, 1, 3, 0, ptr(c.sfull), None, 0, 0, stream_ptr())
    assert cat(120, ptr(c.A2d)) == PTV_ERR_ARG and cat(128, None) == PTV_ERR_ARG and cat(0, ptr(c.A2d)) == PTV_ERR_ARG and cat(200, ptr(c.A2d)) == PTV_ERR_ARG
    assert _untouched(c, c.before)
    try:
        assert lib().ptv_wgrad_batch_mode(4) == PTV_ERR_ARG and lib().ptv_wgrad_batch_mode(-1) == PTV_ERR_ARG
    finally:
        lib().ptv_wgrad_batch_mode(BATCH0)
