"""Plain references (numpy, CPU) of the dense-product family -- ptv_gemm / ptv_gemm_mtop / ptv_gemm_mtop_seg, csrc/gemm.hip on
csrc/gemm_core.hpp -- written from the formula of include/ptvae_hip.h ("Dense product"): the oracle side of
tests/test_gpu_gemm_kernels.py, itself held to torch's float64 operators by tests/test_gemm_ref_host.py.

    C[m, n] = act(alpha * sum_k A(m, k) B(n, k) + bias[n])  (+ C[m, n] when accumulate)

Operands are given AS STORED: A is [M, K] (transA = 0) or [K, M] (transA = 1), B is [N, K] (transB = 0, the nn.Linear weight layout)
or [K, N] (transB = 1).  product() is float64 throughout.  kp_product() is no reference: it evaluates the same formula in float32 with
the operands rounded to bf16 where the kernel rounds them (bf16 precision: both operands while they are staged; a bf16 C: the stored
result, and the C that is read back under accumulate), and its error against product() is the yardstick of the real-valued tests.
int_case() builds the operands of the exact tests: small integers, for which every fp32 partial sum in any order is exact."""
import numpy as np

F8, F4 = np.float64, np.float32
ALPHAS = (1.0, 0.5, -2.0)


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even) -> fp32; finite inputs"""
    u = np.ascontiguousarray(a, dtype=F4).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(F4)


def is_bf16(a):
    return np.array_equal(bf16_round(a), np.asarray(a, F4))


def _act(v, act):
    assert act in (0, 1)
    return np.exp(v) if act == 1 else v


def product(A, B, ta=0, tb=0, bias=None, alpha=1.0, act=0, C0=None, accumulate=0):
    A, B = np.asarray(A, F8), np.asarray(B, F8)
    a = A.T if ta else A                                     # [M, K]
    b = B if tb else B.T                                     # [K, N]
    assert a.shape[1] == b.shape[0], (a.shape, b.shape)
    v = F8(alpha) * (a @ b) if a.shape[1] else np.zeros((a.shape[0], b.shape[1]), F8)
    if bias is not None:
        v = v + np.asarray(bias, F8)[None, :]
    v = _act(v, act)
    return v + np.asarray(C0, F8) if accumulate else v


def kp_product(A, B, ta=0, tb=0, bias=None, alpha=1.0, act=0, C0=None, accumulate=0, prec='fp32', c_bf16=False):
    A, B = np.asarray(A, F4), np.asarray(B, F4)
    if prec == 'bf16':
        A, B = bf16_round(A), bf16_round(B)
    a = A.T if ta else A
    b = B if tb else B.T
    v = (F4(alpha) * (a @ b).astype(F4)).astype(F4)
    if bias is not None:
        v = (v + np.asarray(bias, F4)[None, :]).astype(F4)
    if act == 1:
        v = np.exp(v).astype(F4)
    if accumulate:
        c0 = np.asarray(C0, F4)
        v = (v + (bf16_round(c0) if c_bf16 else c0)).astype(F4)
    return bf16_round(v) if c_bf16 else v


# ---- column-blocked C (dtypes bits 8 / 16): element (m, n) at ((n / w) * M + m) * w + n % w
def to_blocked(C, w):
    M, N = C.shape
    assert N % w == 0
    return np.ascontiguousarray(C.reshape(M, N // w, w).transpose(1, 0, 2))       # [N/w][M][w]


def from_blocked(Cb, w):
    nb, M, w_ = Cb.shape
    assert w_ == w
    return np.ascontiguousarray(Cb.transpose(1, 0, 2).reshape(M, nb * w))


# ---- dead rows (ptv_gemm_mtop / ptv_gemm_mtop_seg)
def dead_rows(M, m_top=None, m_unit=0, seg_n=None, seg_unit=0, seg_period=0):
    """bool [M]: the rows of A the header declares zero -- from (m_top + 1) * m_unit on, and inside every unit of seg_unit rows the ones
    from seg_n[unit % seg_period] on"""
    r = np.arange(M, dtype=np.int64)
    dead = np.zeros(M, bool)
    if m_top is not None:
        dead |= r >= (int(m_top) + 1) * int(m_unit)
    if seg_n is not None:
        dead |= (r % seg_unit) >= np.asarray(seg_n, np.int64)[(r // seg_unit) % seg_period]
    return dead


def expected_with_dead(full, dead, bias=None, act=0, C0=None, accumulate=0):
    """`full` = product() of the same call without limits; the dead rows get what the header promises for a zero row of A:
    act(bias) (zero without bias and act; plus C, i.e. C unchanged without bias, under accumulate)"""
    out = np.array(full, F8, copy=True)
    N = out.shape[1]
    row = _act(np.zeros(N, F8) if bias is None else np.asarray(bias, F8), act)
    out[dead] = row[None, :] + (np.asarray(C0, F8)[dead] if accumulate else 0.0)
    return out


# ---- exact operands
def exact_ok(A, B, ta, tb, bias, alpha, C0):
    """the largest magnitude any partial sum of the case can reach, bias and C0 included, and whether it is below 2^24 (2^23 for the
    half-integers of alpha = 0.5): then every fp32 addition of the kernel, in any order, is exact"""
    a = np.abs(np.asarray(A, F8).T if ta else np.asarray(A, F8))
    b = np.abs(np.asarray(B, F8) if tb else np.asarray(B, F8).T)
    s = float((a @ b).max()) if a.shape[1] and a.size and b.size else 0.0
    top = max(1.0, abs(alpha)) * s + (float(np.abs(bias).max()) if bias is not None else 0.0) + (float(np.abs(C0).max()) if C0 is not None else 0.0)
    return top, top < 2.0 ** 23


def int_case(rng, M, N, K, ta=0, tb=0, bias=False, alpha=1.0, accumulate=False):
    """operands, bias and C0 of integers in [-4, 4] (exact in bf16), alpha one of ALPHAS -> dict(A, B, bias, C0) of float32 arrays in the
    stored layouts"""
    assert alpha in ALPHAS
    iv = lambda *s: rng.randint(-4, 5, s).astype(F4)
    c = dict(A=iv(K, M) if ta else iv(M, K), B=iv(K, N) if tb else iv(N, K), bias=iv(N) if bias else None,
             C0=iv(M, N) if accumulate else None)
    top, ok = exact_ok(c['A'], c['B'], ta, tb, c['bias'], alpha, c['C0'])
    assert ok, 'max |alpha * sum| + |bias| + |C0| = %g is not below 2^23' % top
    return c
