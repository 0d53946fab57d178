"""ptv_gemm_mtop_seg_map (csrc/gemm.hip): the plain product with a row map on C -- product row m is stored at, and with accumulate read
from, C row (m / c_unit) * c_unit + c_rows[m % c_unit].

Operands, bias and C0 are the small integers of tests/gemm_ref.py (every fp32 partial sum exact), and the comparison is np.array_equal:
the mapped call must give what the unmapped call (ptv_gemm_mtop_seg on the same operands, C0 gathered through the map) gives, scattered
through the map by numpy -- and that unmapped result is itself held to the float64 product.  Both tiles (64 x 64 with partial tiles,
128 x 128 on 192 blocks), one and several units, store and accumulate, fp32 / bf16 sources and C, a bias, m_top / seg_n limits whose dead
tiles write through the map.  A stored C starts as NaN inside [M, N] (a row nobody wrote shows) and as a sentinel around it (padding
columns and guard rows must survive).  Refusals leave C untouched."""
import numpy as np
import pytest
import torch

import gemm_ref as R
import kernel_ops as K_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
F4 = np.float32
SENT = np.float32(768.0)                         # (exact in bf16)
G = 2                                            # guard rows before and after C
ERR_ARG = -1

# (M, N, K, c_unit, limits): limits = None or dict(m_top, m_unit, seg_n, seg_unit, seg_period)
SHAPES = {
    'tile64_1unit': (70, 66, 40, 70, [dict(m_top=0, m_unit=16)]),                           # rows from 16 on are zero: the partial tile 64 .. 69 is dead
    'tile64_3units': (210, 66, 40, 70, [dict(m_top=1, m_unit=70), dict(m_top=0, m_unit=64)]),      # dead row tiles from row 192 / 64 on
    'tile128_1unit': (12288, 130, 96, 12288, [dict(m_top=1, m_unit=4096, seg_n=(4096, 1024, 0), seg_unit=4096, seg_period=3),
                                              dict(seg_n=(2048, 128), seg_unit=1024 * 6, seg_period=2)]),
    'tile128_3units': (12288, 130, 96, 4096, [dict(m_top=1, m_unit=4096, seg_n=(4096, 1024, 0), seg_unit=4096, seg_period=3),
                                              dict(seg_n=(384,), seg_unit=512, seg_period=1)]),
}
# (precision, bf16 sources)
SOURCES = (('fp32', ''), ('bf16', ''), ('bf16', 'AB'), ('bf16', 'B'), ('bf16', 'A'))


def call_product(entry, prec, src, tb, A, B, Cbuf, M, N, K, bias, alpha, acc, cbf, splitk, lim, c_rows=None, c_unit=0, ta=0, extra_dtypes=0):
    """one call on device tensors; Cbuf is the whole guarded buffer [(M + 2G), ldc]"""
    ldc = Cbuf.shape[1]
    lim = lim or {}
    top = None if lim.get('m_top') is None else torch.tensor([lim['m_top']], dtype=torch.int32, device=DEV)
    seg = None if lim.get('seg_n') is None else torch.tensor(list(lim['seg_n']), dtype=torch.int32, device=DEV)
    dtypes = (1 if 'A' in src else 0) | (2 if 'B' in src else 0) | (4 if cbf else 0) | extra_dtypes
    args = [1 if prec == 'bf16' else 0, ta, tb, M, N, K, A, A.shape[1], B, B.shape[1], Cbuf[G:], ldc, bias, float(alpha), int(acc), 0, splitk, dtypes,
            top, lim.get('m_unit', 0), seg, lim.get('seg_unit', 0), lim.get('seg_period', 0)]
    if entry == 'ptv_gemm_mtop_seg_map':
        args += [c_rows, c_unit]
    rc = K_.leaf_rc(entry, *args)
    torch.cuda.synchronize()
    return rc


def c_buffer(M, N, body, cbf):
    """[(M + 2G), ldc] of the sentinel with `body` ([M, N] array or a scalar) inside"""
    ldc = (N + 4) // 4 * 4
    buf = np.full((M + 2 * G, ldc), SENT, F4)
    buf[G:G + M, :N] = body
    t = torch.from_numpy(buf)
    return (t.to(BF) if cbf else t).to(DEV)


def split_buffer(buf, M, N):
    """-> (the [M, N] body, True if everything around it still holds the sentinel)"""
    out = buf.float().cpu().numpy()
    body = out[G:G + M, :N].copy()
    out[G:G + M, :N] = SENT
    return body, bool((out == SENT).all())


def row_map(rng, M, c_unit):
    """-> (c_rows [c_unit] int32, the C row of every product row [M])"""
    p = rng.permutation(c_unit).astype(np.int32)
    m = np.arange(M)
    return p, (m // c_unit) * c_unit + p[m % c_unit]


def operands(rng, M, N, K, tb, src, lim):
    iv = lambda *s: rng.randint(-4, 5, s).astype(F4)
    A, B = iv(M, K), (iv(K, N) if tb else iv(N, K))
    if lim:
        A[R.dead_rows(M, lim.get('m_top'), lim.get('m_unit', 0), lim.get('seg_n'), lim.get('seg_unit', 0), lim.get('seg_period', 0))] = 0
    At, Bt = torch.from_numpy(A), torch.from_numpy(B)
    return A, B, (At.to(BF) if 'A' in src else At).to(DEV), (Bt.to(BF) if 'B' in src else Bt).to(DEV)


def run_pair(rng, M, N, K, c_unit, prec, src, tb, acc, cbf, with_bias, alpha, lim, splitk=0):
    """the mapped call against the unmapped call scattered by numpy, and the unmapped call against float64"""
    tag = 'M %d N %d K %d unit %d %s src=%r tb %d acc %d cbf %d bias %d alpha %g lim %r' % (M, N, K, c_unit, prec, src, tb, acc, cbf, with_bias, alpha, lim)
    A, B, Ad, Bd = operands(rng, M, N, K, tb, src, lim)
    bias = rng.randint(-4, 5, N).astype(F4) if with_bias else None
    bias_d = None if bias is None else torch.from_numpy(bias).to(DEV)
    c_rows, crow = row_map(rng, M, c_unit)
    c_rows_d = torch.from_numpy(c_rows).to(DEV)
    C0 = rng.randint(-4, 5, (M, N)).astype(F4) if acc else None             # what C holds before the MAPPED call
    top, ok = R.exact_ok(A, B, 0, tb, bias, alpha, C0)
    assert ok, tag
    # unmapped: product row m accumulates onto what the mapped call finds in ITS row, C0[crow[m]]
    plain = c_buffer(M, N, C0[crow] if acc else np.nan, cbf)
    assert call_product('ptv_gemm_mtop_seg', prec, src, tb, Ad, Bd, plain, M, N, K, bias_d, alpha, acc, cbf, splitk, lim) == 0, tag
    U, clean = split_buffer(plain, M, N)
    assert clean, tag
    want64 = R.product(A, B, 0, tb, bias, alpha, 0, None if C0 is None else C0[crow], acc)     # (the dead rows of A are zero: no special case)
    want64 = want64.astype(F4)
    assert np.array_equal(U, R.bf16_round(want64) if cbf else want64), tag
    mapped = c_buffer(M, N, C0 if acc else np.nan, cbf)
    rc = call_product('ptv_gemm_mtop_seg_map', prec, src, tb, Ad, Bd, mapped, M, N, K, bias_d, alpha, acc, cbf, splitk, lim, c_rows_d, c_unit)
    assert rc == 0, tag
    got, clean = split_buffer(mapped, M, N)
    assert clean, tag + ': written outside C[M, N]'
    want = np.empty_like(U)
    want[crow] = U
    assert not np.isnan(got).any(), tag + ': %d rows were never written' % int(np.isnan(got).any(axis=1).sum())
    assert np.array_equal(got, want), tag


@pytest.mark.parametrize('shape', list(SHAPES))
def test_mapped_product_equals_the_scattered_unmapped_product(shape):
    M, N, K, c_unit, limits = SHAPES[shape]
    rng = np.random.RandomState(len(shape) * 131 + M)
    for prec, src in SOURCES:
        for cbf in ((0,) if prec == 'fp32' else (0, 1)):                     # (a bf16 C belongs to the bf16 precision)
            for acc in (0, 1):
                # plain, with a bias (and another alpha), and with every row limit of the shape (dead tiles: zeros / the bias through the
                # map when storing, nothing when accumulating without a bias)
                run_pair(rng, M, N, K, c_unit, prec, src, 0, acc, cbf, False, 1.0, None)
                run_pair(rng, M, N, K, c_unit, prec, src, 1, acc, cbf, True, -2.0, None)
                for lim in limits:
                    run_pair(rng, M, N, K, c_unit, prec, src, 0, acc, cbf, False, 1.0, lim)
                run_pair(rng, M, N, K, c_unit, prec, src, 0, acc, cbf, True, 1.0, limits[0])


def test_identity_map_and_a_depth_the_unmapped_product_would_split():
    """c_rows = 0 .. c_unit - 1 is the unmapped product; where splitk = 0 splits K (K = 640 on eight 64 x 64 tiles: partials in a workspace,
    the ordered reduction stores through the map) the mapped result is still the scattered unmapped one, under the atomic fallback too;
    splitk = 1 / -1 are taken"""
    rng = np.random.RandomState(77)
    M, N, K, c_unit = 210, 66, 640, 70
    import os
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    mode0 = 0 if os.environ.get('PTV_WGRAD_ORDERED', '')[:1] == '0' else 1    # the library's reduction mode at load (it has a setter, no getter)
    try:
        for ordered in (1, 0):
            assert lib().ptv_ordered_reductions(ordered) == 0
            for splitk in (0, 1, -1):
                for prec, src in (('fp32', ''), ('bf16', 'AB')):
                    run_pair(rng, M, N, K, c_unit, prec, src, 0, 0, 0, True, 1.0, None, splitk=splitk)
                    run_pair(rng, M, N, K, c_unit, prec, src, 0, 1, 0, False, 0.5, None, splitk=splitk)
    finally:
        assert lib().ptv_ordered_reductions(mode0) == 0
    A, B, Ad, Bd = operands(rng, M, N, 40, 0, '', None)
    ident = torch.arange(c_unit, dtype=torch.int32, device=DEV)
    a, b = c_buffer(M, N, np.nan, 0), c_buffer(M, N, np.nan, 0)
    assert call_product('ptv_gemm_mtop_seg', 'fp32', '', 0, Ad, Bd, a, M, N, 40, None, 1.0, 0, 0, 0, None) == 0
    assert call_product('ptv_gemm_mtop_seg_map', 'fp32', '', 0, Ad, Bd, b, M, N, 40, None, 1.0, 0, 0, 0, None, ident, c_unit) == 0
    assert torch.equal(a, b)


def test_refusals_leave_c_untouched():
    rng = np.random.RandomState(3)
    M, N, K, c_unit = 128, 64, 64, 64
    A, B, Ad, Bd = operands(rng, M, N, K, 0, '', None)
    At = Ad.t().contiguous()                                                  # [K, M] for transA
    c_rows = torch.from_numpy(row_map(rng, M, c_unit)[0]).to(DEV)
    buf = c_buffer(M, N, SENT, 0)
    E = 'ptv_gemm_mtop_seg_map'
    base = dict(entry=E, prec='bf16', src='', tb=0, A=Ad, B=Bd, Cbuf=buf, M=M, N=N, K=K, bias=None, alpha=1.0, acc=0, cbf=0, splitk=0, lim=None,
                c_rows=c_rows, c_unit=c_unit)
    cases = {
        'column-blocked C by 32': dict(extra_dtypes=8), 'column-blocked C by 16': dict(extra_dtypes=16), 'splitk 2': dict(splitk=2),
        'transA': dict(ta=1, A=At), 'c_unit 0': dict(c_unit=0), 'c_unit -1': dict(c_unit=-1), 'M no multiple of c_unit': dict(c_unit=48),
    }
    for name, over in cases.items():
        assert call_product(**dict(base, **over)) == ERR_ARG, name
        assert bool((buf == SENT).all()), name + ': C was written'
    assert call_product(**base) == 0                                          # (the base case itself is taken)
    assert not bool((buf[G:G + M, :N] == SENT).all())
