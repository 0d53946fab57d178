"""Plain fp64 reference (numpy, CPU) of the bi-GRU autograd node functional.BiGruFinalFn -- _bigru_forward / _bigru_backward and the four
composites ptv_bigru_final_fwd / _bwd, ptv_bigru_rows_fwd / _bwd behind it: the oracle side of tests/test_gpu_bigru_node.py, itself held
to torch's float64 nn.GRU(bidirectional=True) over pack_padded_sequence and autograd by tests/test_bigru_ref_host.py.

A thin layer over the references of the kernels under the node -- gru_ref (the cell and its BPTT), rowgru_ref / pgru_ref (the row and the
persistent kernels' configuration of it), gemm_ref (the input products and dX) and wgrad_ref (the weight-gradient products and bias sums)
-- written from include/ptvae_hip.h ("GRU recurrence", "Dense product", "Weight-gradient product") and the node's docstrings:

    gi_d[t]  = x[t] . W_ih_d^T + b_ih_d                                  d = 0: t = 0 .. len-1,  d = 1: t = len-1 .. 0,  h_d = 0 before
    out      = [h_0 after its last live step | h_1 after its last live step]              a row of length 0: zeros in both halves
    dW_ih_d  = sum over (t, m) of dgi_d[t, m]^T x[t, m]            db_ih_d = column sums of dgi_d           (dgi indexed by TIME)
    dW_hh_d  = sum over (s, m) of dgh_d[s, m]^T h_d before step s  db_hh_d = column sums of dgh_d           (dgh, h by PROCESSING STEP)
    dx       = dgi_0 . W_ih_0 + dgi_1 . W_ih_1                          exactly zero at (t, m) with t >= len[m]

Everything is in NATURAL row order: the length sort (perm), the per-step live-row counts (seg), the `top` clip of the products, k_rev and
the negative seg_period of the reversed direction, the two streams and the accumulate-into-dx_acc link are the node's way of computing
these sums and change none of them.  w8 = (w_ih, w_hh, b_ih, b_hh) x 2 directions, the node's parameter order.

kp_forward / kp_backward evaluate the same chain in float32 with the roundings of one branch of the node.  They are no reference: their
error against forward / backward is the yardstick the node's error is held to (bound_of of tests/test_gpu_dur_kernels.py).  The
roundings, read in functional.py, csrc/composite.hip, csrc/notes_persist.hip, csrc/gru_persist.hip, csrc/gru.hip, csrc/gemm_core.hpp
and csrc/wgrad.hip:

  'rows'     (H = I = 128; rowgru_ref.kp_*)   x and W_ih rounded to bf16 as MFMA operands of the fused input product, gi itself stays in
             fp32 registers; W_hh bf16; the recurrent operand is the bf16 state shadow; gates saved as bf16; the BPTT reads the fp32
             states and the bf16 gates, its recurrent operand is the bf16 dgh; dgi and dgh stored as bf16.
  'persist'  (gemm_ref.kp_product + pgru_ref.kp_*)   the input product on bf16(x) x bf16(W_ih) + b_ih with gi STORED as bf16 (dtypes bit
             C16 of the composite, out_dtype of the Python sequencing; WIH_F32: the fp32 weight is rounded while it is staged -- the
             same values); then as 'rows'.
  'step' bf16 (gemm_ref.kp_product + gru_ref.kp_*, bf16=True)   the same roundings as 'persist' through ptv_gru_seq_fwd / _bwd.
  'step' fp32 (bf16=False)   fp32 throughout, nothing rounded.
  every bf16 branch: dW_ih = bf16 dgi x bf16(x) (wgrad.hip: "fp32 sources are rounded to bf16 on the way into LDS"; below K = 512 the dense
             product does the same while it stages), dW_hh = bf16 dgh x the bf16 state shadow, the bias sums over the bf16 dgi / dgh,
             dX = bf16 dgi x the transposed bf16 weight shadow (without an optimiser: the fp32 weight rounded while staged), all with
             fp32 accumulation; the second direction's dX is added to the first's in fp32.
  x_bf16:    a bf16 input is read as it is (X_BF16); autograd hands its gradient back in the input's dtype, so dx is rounded to bf16.

ROWS_CASES, STEP_FP32_CASES and persist_cases(M, H) -- at the (M, H) the device supports -- are the case tables the GPU test runs,
here so that the host test can assert what they reach (its single cases -- under 512 rows, split-K, the crossing -- are built with
case() in the GPU file); inputs() are the seeded CPU generators:
weights U(+-1/sqrt(H)), rounded to bf16 for the bf16 branches (the optimiser's shadows round them anyway; this keeps the kernel-precision
model from being dominated by that), x = 0.7 N(0, 1), dout = 0.3 N(0, 1)."""
import functools
import zlib

import numpy as np

import gemm_ref as GM
import gru_ref as G
import pgru_ref as PG
import rowgru_ref as RR
import wgrad_ref as WG
from gemm_ref import bf16_round

F8, F4 = np.float64, np.float32
PANEL, BLOCK = RR.PANEL, RR.BLOCK
NAMES = tuple('%s_%d' % (n, d) for d in range(2) for n in ('w_ih', 'w_hh', 'b_ih', 'b_hh'))


# ================================================================================================ fp64
def trace(x, lengths, w8, dout=None):
    """the chain of both directions in float64 -> per direction a dict: gi [T, M, 3H] by time, states [T + 1, M, H] (slot 0 = zeros, slot
    s + 1 after processing step s), gates [T, 4, M, H] by step and, with dout [M, 2H], dgi [T, M, 3H] by TIME, dgh [T, M, 3H] by STEP"""
    x = np.asarray(x, F8)
    T, M, I = x.shape
    out = []
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = (np.asarray(a, F8) for a in w8[4 * d: 4 * d + 4])
        H = w_hh.shape[1]
        gi = GM.product(x.reshape(T * M, I), w_ih, bias=b_ih).reshape(T, M, 3 * H)
        hs, gates = G.gru_forward(gi, None, w_hh, b_hh, np.zeros((M, H), F8), lengths, bool(d), None)
        tr = dict(gi=gi, states=np.concatenate([np.zeros((1, M, H), F8), hs]), gates=gates, w_ih=w_ih, w_hh=w_hh)
        if dout is not None:
            last = np.asarray(dout, F8)[:, d * H:(d + 1) * H]
            tr['dgi'], tr['dgh'] = G.gru_backward(tr['states'][:T], gates, w_hh, None, last, None, None, bool(d))[:2]
        out.append(tr)
    return out


def out_of(tr):
    """[M, 2H]: direction 0's final state in the first half, direction 1's in the second"""
    return np.concatenate([tr[0]['states'][-1], tr[1]['states'][-1]], axis=1)


def grads_of(x, tr, d):
    """direction d's (dW_ih, dW_hh, db_ih, db_hh) and its share of dx [T, M, I]"""
    x = np.asarray(x, F8)
    T, M, I = x.shape
    t = tr[d]
    H3 = t['dgi'].shape[2]
    dgi2, dgh2 = t['dgi'].reshape(T * M, H3), t['dgh'].reshape(T * M, H3)
    g = [WG.product(dgi2, x.reshape(T * M, I)), WG.product(dgh2, t['states'][:T].reshape(T * M, -1)), WG.colsum(dgi2), WG.colsum(dgh2)]
    return g, GM.product(dgi2, t['w_ih'], tb=1).reshape(T, M, I)


def forward(x, lengths, w8):
    """x [T, M, I], lengths [M] or None (every row has length T) -> out [M, 2H], float64"""
    return out_of(trace(x, lengths, w8))


def backward(x, lengths, w8, dout):
    """-> dx [T, M, I] and the eight gradients in the node's order, float64"""
    tr = trace(x, lengths, w8, dout)
    (g0, dx0), (g1, dx1) = grads_of(x, tr, 0), grads_of(x, tr, 1)
    return dx0 + dx1, g0 + g1


# ================================================================================================ the node's own precision
BRANCHES = ('rows', 'persist', 'step')


def _kp_trace(x, lengths, w8, dout, branch, bf16):
    assert branch in BRANCHES and (bf16 or branch == 'step')
    x = np.asarray(x, F4)
    T, M, I = x.shape
    prec = 'bf16' if bf16 else 'fp32'
    out = []
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = (np.asarray(a, F4) for a in w8[4 * d: 4 * d + 4])
        H = w_hh.shape[1]
        h0 = np.zeros((M, H), F4)
        last = None if dout is None else np.ascontiguousarray(np.asarray(dout, F4)[:, d * H:(d + 1) * H])
        if branch == 'rows':
            states, gates, s16 = RR.kp_forward(H, x, w_ih, w_hh, b_hh, h0, b_ih=b_ih, lengths=lengths, reverse=bool(d))
            bptt = lambda: RR.kp_backward(H, states[:T], gates, w_hh, None, last, bool(d))[:2]
        else:
            gi = GM.kp_product(x.reshape(T * M, I), w_ih, bias=b_ih, prec=prec, c_bf16=bf16).reshape(T, M, 3 * H)
            if branch == 'persist':
                states, gates, s16 = PG.kp_forward(gi, None, w_hh, b_hh, h0, lengths, bool(d))
                bptt = lambda: PG.kp_backward(states[:T], gates, w_hh, None, last, bool(d))[:2]
            else:
                hs, gates, h16 = G.kp_forward(gi, None, w_hh, b_hh, h0, lengths, bool(d), None, bf16=bf16, gates_bf16=bf16)
                states, s16 = np.concatenate([h0[None], hs]), np.concatenate([h0[None], h16])
                bptt = lambda: G.kp_backward(states[:T], gates, w_hh, None, last, None, None, bool(d), bf16=bf16, dg_bf16=bf16)[:2]
        tr = dict(states=states, operand=(s16 if bf16 else states), w_ih=w_ih)
        if dout is not None:
            tr['dgi'], tr['dgh'] = bptt()
        out.append(tr)
    return out


def kp_forward(x, lengths, w8, branch, bf16=True):
    return np.concatenate([t['states'][-1] for t in _kp_trace(x, lengths, w8, None, branch, bf16)], axis=1)


def kp_chain(x, lengths, w8, dout, branch, bf16=True, x_bf16=False):
    """-> out, dx and the eight gradients of one kernel-precision evaluation (float32)"""
    x = np.asarray(x, F4)
    T, M, I = x.shape
    prec = 'bf16' if bf16 else 'fp32'
    tr = _kp_trace(x, lengths, w8, dout, branch, bf16)
    grads, dx = [], None
    for d in range(2):
        t = tr[d]
        H3 = t['dgi'].shape[2]
        dgi2, dgh2 = t['dgi'].reshape(T * M, H3), t['dgh'].reshape(T * M, H3)
        grads += [GM.kp_product(dgi2, x.reshape(T * M, I), ta=1, tb=1, prec=prec),
                  GM.kp_product(dgh2, t['operand'][:T].reshape(T * M, -1), ta=1, tb=1, prec=prec),
                  dgi2.sum(axis=0, dtype=F4), dgh2.sum(axis=0, dtype=F4)]
        dx = GM.kp_product(dgi2, t['w_ih'], tb=1, prec=prec, C0=dx, accumulate=int(d))
    dx = dx.reshape(T, M, I)
    return np.concatenate([t['states'][-1] for t in tr], axis=1), (bf16_round(dx) if x_bf16 else dx), grads


def kp_backward(x, lengths, w8, dout, branch, bf16=True, x_bf16=False):
    return kp_chain(x, lengths, w8, dout, branch, bf16, x_bf16)[1:]


# ================================================================================================ the cases of the GPU test
def case(branch, M, T, lens, H=128, I=128, bf16=True, x_bf16=False, reaches=''):
    return dict(branch=branch, M=M, T=T, H=H, I=I, lens=lens, bf16=bf16, x_bf16=x_bf16, reaches=reaches)


ROWS_CASES = (
    case('rows', 4096, 3, 'random', reaches='sorted panels with seg; a row of length 0 and a full-length row'),
    case('rows', 4096, 3, None, reaches='the dense path'),
    case('rows', 4100, 3, 'random', reaches='M % 32 != 0: no top, no seg'),
    case('rows', 4224, 3, 'random', reaches='33 blocks, 66 panels'),
    case('rows', 4096, 16, 'short6', reaches='launch-wide dead steps: top clips all three products in both directions'),
    case('rows', 4096, 16, 'zero', reaches='every result exactly zero'),
)
STEP_FP32_CASES = (
    case('step', 8, 3, 'random', H=16, I=16, bf16=False),
    case('step', 8, 3, None, H=16, I=16, bf16=False),
    case('step', 5, 1, 'random', H=16, I=12, bf16=False),
)
SHORT_MAX = 6


PERSIST_GRID = tuple((lens, I, xb) for lens in ('random', None) for I in (64, 36) for xb in (False, True))


def persist_cases(M, H):
    """the persist family at the device's smallest supported (M, H), T = 3: with and without lengths, I = 64 (bf16 W_ih shadow) / 36 (none:
    WIH_F32), fp32 / bf16 x (X_BF16)"""
    return tuple(case('persist', M, 3, lens, H=H, I=I, x_bf16=xb) for lens, I, xb in PERSIST_GRID)


def case_id(c):
    return '%s-M%d-T%d-H%d-I%d-%s%s%s' % (c['branch'], c['M'], c['T'], c['H'], c['I'], c['lens'] or 'dense', '' if c['bf16'] else '-fp32',
                                          '-xbf16' if c['x_bf16'] else '')


def lengths_of(M, T, kind, rng):
    """'random': uniform 0 .. T, row 0 of length 0 and row 1 (when there is one) of length T; 'short6': uniform 0 .. 6 < T the same way,
    the longest row 6; 'zero': all 0; None: no lengths"""
    if kind is None:
        return None
    if kind == 'zero':
        return np.zeros(M, np.int32)
    top = {'random': T, 'short6': SHORT_MAX}[kind]
    assert top <= T
    ln = rng.randint(0, top + 1, size=M).astype(np.int32)
    ln[0] = 0
    if M > 1:
        ln[1] = top
    return ln


@functools.lru_cache(maxsize=None)
def _inputs(key):
    branch, M, T, H, I, lens, bf16, x_bf16 = key
    rng = np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)
    k = 1.0 / np.sqrt(H)
    w8 = [rng.uniform(-k, k, size=s).astype(F4) for _ in range(2) for s in ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,))]
    if bf16:
        w8 = [bf16_round(w) for w in w8]
    x = (0.7 * rng.standard_normal((T, M, I))).astype(F4)
    if x_bf16:
        x = bf16_round(x)
    dout = (0.3 * rng.standard_normal((M, 2 * H))).astype(F4)
    res = dict(x=x, w8=tuple(w8), dout=dout, lengths=lengths_of(M, T, lens, rng))
    for a in [x, dout] + w8 + ([] if res['lengths'] is None else [res['lengths']]):
        a.setflags(write=False)
    return res


def inputs(c):
    """the seeded operands of a case: x [T, M, I], w8, dout [M, 2H] float32, lengths int32 or None (read-only, shared)"""
    return _inputs(tuple(c[k] for k in ('branch', 'M', 'T', 'H', 'I', 'lens', 'bf16', 'x_bf16')))


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = dict(zip(('branch', 'M', 'T', 'H', 'I', 'lens', 'bf16', 'x_bf16'), key))
    ins = inputs(c)
    tr = trace(ins['x'], ins['lengths'], ins['w8'], ins['dout'])
    (g0, dx0), (g1, dx1) = grads_of(ins['x'], tr, 0), grads_of(ins['x'], tr, 1)
    kout, kdx, kg = kp_chain(ins['x'], ins['lengths'], ins['w8'], ins['dout'], c['branch'], c['bf16'], c['x_bf16'])
    return dict(out=out_of(tr), dx=dx0 + dx1, grads=g0 + g1, kp_out=kout, kp_dx=kdx, kp_grads=kg)


def reference(c):
    """the fp64 results and their kernel-precision evaluation of a case, computed once per process: out, dx, grads, kp_out, kp_dx, kp_grads"""
    return _reference(tuple(c[k] for k in ('branch', 'M', 'T', 'H', 'I', 'lens', 'bf16', 'x_bf16')))
