"""The fused per-note heads (csrc/heads.hip: ptv_heads_fwd / _top / _rows, ptv_heads_bwd / _rows) and the MFMA-fragment weight packs
(csrc/freerun.hip: ptv_pack_mfma_b_size / _b / _b2 / _multi) one call at a time against tests/heads_ref.py, through the C ABI as it is
declared (kernel_ops.leaf_rc).

A. packs: every element of every pack bit for bit -- plain and pair-interleaved tiles, a transposed source, a k-block sub-range of a
   wider buffer whose other k-blocks keep their sentinel, zero fill beyond N and K, bf16 ties of both parities, NaN in the source's row
   padding, one case per kernel beyond its grid cap; functional.heads_packs / notes_packs; the refusals.
B. heads, exact-integer: operands, biases and upstream gradients of integers in [-4, 4].  Every fp32 partial sum is exact in any order
   (heads_ref.exact_ok, asserted for every case on the CPU by tests/test_heads_ref_host.py) and the kernel's bf16 roundings apply to exactly
   known values, so every output is predicted BIT FOR BIT -- with the library's packs and with the reference's packs uploaded (a pack fault
   and a kernel fault are told apart).  Which rows are computed, zero or untouched under m_top / row_len / blocked comes from
   heads_ref.dead_fwd / dead_bwd, made from the header text and the arguments alone; hn and dhd0 hold NaN in every row that is not
   computed.
C. heads, real-valued: kernel error at most 4x the error of the kernel-precision CPU evaluation (heads_ref.kp_*) against float64, floor
   8 fp32 ulps of the scale; the bound never sees the kernel's output.  Prints `HEADS_RATIO family ratio` (pytest -s; profiles/LOG.md).
D. refusals: status -1, every output keeps its sentinel.

Every output has guard rows (elements) before and after and padding columns, pre-filled with a sentinel that is exact in bf16."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import heads_ref as R
import kernel_ops as K_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
F4, F8 = np.float32, np.float64
SENT = np.float32(768.0)                                               # (exact in bf16)
SENT16 = np.uint16(0x4440)
G = 2                                                                  # guard rows before and after a row-major output
GE = 64                                                                # guard elements around a flat output
RATIOS = {}
C_, Z_, U_ = R.COMPUTED, R.ZERO, R.UNTOUCHED

# ================================================================================================ the parameter lists
PACK_N = (1, 16, 17, 64, 130)
PACK_K = (1, 31, 32, 33, 130, 512)
SHAPE_M = (1, 15, 16, 17, 127, 128, 129, 300)
LDPS = (132, 136, 144)
TOPS = (-1, 0, 1, 3, 7)
FWD_LIMITS = [dict(M=512, m_unit=128, m_top=t) for t in TOPS]
# m_unit = 96, *m_top = 0 on M = 300: rows 96 .. 127 are the dead rows of a partly live block; m_unit = 16: the limit inside block 0 (0),
# on the block boundary (7), inside block 1 (10), beyond M (30), and none live (-1)
BWD_LIMITS = FWD_LIMITS + [dict(M=300, m_unit=96, m_top=0)] + [dict(M=300, m_unit=16, m_top=t) for t in (-1, 0, 7, 10, 30)]
ROW_LENS = {'3|1': [3] * 128 + [1] * 128, 'inside': [4] * 64 + [2] * 64 + [2] * 128}
ROWS_CASES = [dict(M=M, m_unit=256, m_top=t, row_len=k) for M in (1024, 1000) for t in (2, 3) for k in ROW_LENS]
REAL_MS = (300, 1024)
RM = 130                                                               # the refusals' M
INT_MS = sorted(set(SHAPE_M) | {c['M'] for c in BWD_LIMITS + ROWS_CASES} | {RM})


def lim_id(c):
    return ' '.join('%s=%s' % kv for kv in c.items())


@functools.lru_cache(maxsize=None)
def weights():
    c = R.int_case(np.random.RandomState(130512), 1)
    return {k: c[k] for k in ('w_p', 'w_dh', 'b_p', 'b_dh')}


@functools.lru_cache(maxsize=None)
def case_of(M):
    """the integer case of M rows (one set of weights for all of them); heads_ref.int_case asserts exact_ok"""
    c = R.int_case(np.random.RandomState(7 + M), M)
    c.update(weights())
    R.exact_ok(c)
    return c


@functools.lru_cache(maxsize=None)
def exact_of(M):
    """every output of the integer case, predicted exactly: the kernel-precision formulas in float64 on integers"""
    c = case_of(M)
    pitch, hd0, hd16 = R.kp_fwd(c['hn'], c['w_p'], c['w_dh'], c['b_p'], c['b_dh'], dt=F8)
    dpp, dn, dy = R.kp_bwd(c['dp'], c['dhd0'], c['w_p'], c['w_dh'], dt=F8)
    out = dict(pitch=pitch, hd0=hd0, hd16=hd16, dp=dpp, dnsum=dn, dy16=dy)
    for k, v in out.items():
        assert np.array_equal(v.astype(F4).astype(F8), v), k
    return {k: v.astype(F4) for k, v in out.items()}


# ================================================================================================ device plumbing
def lib():
    from polyphonic_chord_texture_disentanglement_amd._lib import lib as l
    return l()


def dev(x, bf=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t.to(BF) if bf else t).to(DEV)


def dev_bits(u16):
    """uint16 bit patterns -> a bf16 device tensor of those bits (flat)"""
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16).ravel()).view(BF).to(DEV)


def host_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def filled(shape, bf=False):
    return torch.full(shape, float(SENT), dtype=BF if bf else torch.float32, device=DEV)


def shifted(t, n):
    """a copy of t that starts n ELEMENTS after an aligned allocation (with room behind it)"""
    buf = torch.zeros(t.numel() + n + 64, dtype=t.dtype, device=t.device)
    buf[n:n + t.numel()] = t.reshape(-1)
    return buf[n:]


def ints(v):
    return None if v is None else torch.tensor(np.atleast_1d(np.asarray(v)), dtype=torch.int32, device=DEV)


def first_diff(got, want):
    ne = np.argwhere(np.asarray(got) != np.asarray(want))
    return '%d of %d elements differ, first at %s: got %r, want %r; index ranges %s' % (
        len(ne), np.asarray(got).size, tuple(ne[0]), np.asarray(got)[tuple(ne[0])], np.asarray(want)[tuple(ne[0])],
        [(int(ne[:, i].min()), int(ne[:, i].max())) for i in range(ne.shape[1])])


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), '%s: %s' % (what, first_diff(got, want))


# ================================================================================================ A. packs
def pack_src(rng, N, K, trans):
    """the stored source with NaN in its row padding: [N][K + 3], or transposed [K][N + 5]"""
    rows, cols = (K, N) if trans else (N, K)
    buf = np.full((rows, cols + (5 if trans else 3)), np.nan, F4)
    buf[:, :cols] = R.tie_values(rng, (rows, cols))
    return buf


def multi_jobs(rows):
    from polyphonic_chord_texture_disentanglement_amd._lib import ptr
    flat = [int(ptr(v)) if isinstance(v, torch.Tensor) else int(v) for r in rows for v in r]
    return (ctypes.c_long * max(1, len(flat)))(*flat)


def run_pack(entry, Wt, ld, N, K, pairs, trans, NT, kb0, KBtot, n_el=None):
    """-> (status, the whole output buffer as bits, guards included); Wt: the source on the device"""
    n_el = NT * KBtot * 512 if n_el is None else n_el
    out = filled((GE + n_el + GE,), bf=True)
    view = out[GE:]
    if entry == 'ptv_pack_mfma_b':
        rc = K_.leaf_rc(entry, Wt, ld, N, K, view, pairs)
    elif entry == 'ptv_pack_mfma_b2':
        rc = K_.leaf_rc(entry, Wt, ld, N, K, view, pairs, trans, NT, kb0, KBtot)
    else:
        rc = K_.leaf_rc(entry, multi_jobs([(Wt, ld, N, K, view, pairs, trans, NT, kb0, KBtot)]), 1)
    torch.cuda.synchronize()
    return rc, host_bits(out)


def want_pack(src, N, K, pairs, trans, NT, kb0, KBtot):
    n_el = NT * KBtot * 512
    w = np.full(GE + n_el + GE, SENT16, np.uint16)
    w[GE:GE + n_el] = R.pack(src, N, K, pairs, trans, NT, kb0, KBtot, out=np.full(n_el, SENT16, np.uint16)).ravel()
    return w


def check_pack(entry, src, Wt, N, K, pairs, trans, NT, kb0, KBtot):
    rc, got = run_pack(entry, Wt, src.shape[1], N, K, pairs, trans, NT, kb0, KBtot)
    assert rc == 0, (entry, N, K, pairs, trans, NT, kb0, KBtot)
    same(got, want_pack(src, N, K, pairs, trans, NT, kb0, KBtot), '%s N=%d K=%d pairs=%d trans=%d NT=%d kb0=%d KBtot=%d' % (
        entry, N, K, pairs, trans, NT, kb0, KBtot))
    return got


@pytest.mark.parametrize('K', PACK_K)
@pytest.mark.parametrize('N', PACK_N)
def test_pack_grid(N, K):
    """the three kernels on every (N, K): natural tiles and one spare tile, both orientations, kb0 = 0 and a sub-range of a wider buffer,
    pairs where N % 32 == 0; ptv_pack_mfma_b == _b2(trans = 0, kb0 = 0) == a one-job _multi"""
    rng = np.random.RandomState(1000 * N + K)
    NT, KB = R.cdiv(N, 16), R.cdiv(K, 32)
    assert lib().ptv_pack_mfma_b_size(N, K) == NT * KB * 512
    for trans in (0, 1):
        src = pack_src(rng, N, K, trans)
        Wt = dev(src)
        for pairs in ((0, 1) if N % 32 == 0 else (0,)):
            got = {}
            for entry in ('ptv_pack_mfma_b2', 'ptv_pack_mfma_multi') + (() if trans else ('ptv_pack_mfma_b',)):
                got[entry] = check_pack(entry, src, Wt, N, K, pairs, trans, NT, 0, KB)
                if entry != 'ptv_pack_mfma_b':
                    check_pack(entry, src, Wt, N, K, pairs, trans, NT + 2, 2, KB + 3)
            for g in got.values():
                same(g, got['ptv_pack_mfma_b2'], 'the entry points among themselves')


@pytest.mark.parametrize('entry', ['ptv_pack_mfma_b2', 'ptv_pack_mfma_multi'])
def test_pack_pairs_with_a_ragged_n(entry):
    """pair-interleaved tiles with N = 48 in NT = 4: the rows 48 .. 63 of the second pair are zeros"""
    rng = np.random.RandomState(48)
    for trans in (0, 1):
        for K, kb0, KBtot in ((33, 0, 2), (130, 1, 7)):
            src = pack_src(rng, 48, K, trans)
            check_pack(entry, src, dev(src), 48, K, 1, trans, 4, kb0, KBtot)


def test_pack_multi_eight_jobs_mix_all_flags():
    rng = np.random.RandomState(8)
    #        N    K  pairs trans NT kb0 KBtot
    jobs = [(130, 512, 0, 0, 9, 0, 16), (64, 130, 0, 0, 4, 0, 5), (130, 64, 0, 1, 9, 0, 2), (512, 130, 1, 1, 32, 0, 7),
            (48, 33, 1, 0, 4, 3, 6), (1, 1, 0, 1, 1, 0, 1), (17, 31, 0, 1, 3, 2, 4), (64, 33, 1, 0, 4, 0, 2)]
    srcs = [pack_src(rng, N, K, trans) for N, K, pairs, trans, NT, kb0, KBtot in jobs]
    Wts = [dev(s) for s in srcs]
    outs = [filled((GE + NT * KBtot * 512 + GE,), bf=True) for N, K, pairs, trans, NT, kb0, KBtot in jobs]
    rows = [(Wts[i], srcs[i].shape[1], j[0], j[1], outs[i][GE:]) + j[2:] for i, j in enumerate(jobs)]
    assert K_.leaf_rc('ptv_pack_mfma_multi', multi_jobs(rows), 8) == 0
    torch.cuda.synchronize()
    for i, (N, K, pairs, trans, NT, kb0, KBtot) in enumerate(jobs):
        same(host_bits(outs[i]), want_pack(srcs[i], N, K, pairs, trans, NT, kb0, KBtot), 'job %d' % i)


@pytest.mark.parametrize('entry,N,K', [('ptv_pack_mfma_b', 1536, 3072), ('ptv_pack_mfma_b2', 1536, 3072), ('ptv_pack_mfma_multi', 1536, 768)])
def test_pack_beyond_the_grid_cap(entry, N, K):
    """more fragments than the capped grid has threads: the grid-stride loop takes a second trip"""
    cap = 512 if entry == 'ptv_pack_mfma_multi' else 2048
    NT, KB = N // 16, K // 32
    assert NT * KB * 64 > cap * 256
    rng = np.random.RandomState(K)
    src = np.full((N, K + 3), np.nan, F4)
    src[:, :K] = (rng.randint(-256, 257, (N, K)) * 0.03125).astype(F4)              # (multiples of 2^-5: bf16 ties and non-ties)
    check_pack(entry, src, dev(src), N, K, 1 if entry != 'ptv_pack_mfma_b2' else 0, 0, NT, 0, KB)


def test_library_packs_equal_the_reference_packs():
    """functional.heads_packs (six jobs, wcat by two of them) and functional.notes_packs (H = 512 plain, H = 128 pair-interleaved)"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    rng = np.random.RandomState(6)
    w_p, w_dh = R.tie_values(rng, (R.NP, R.HN)), R.tie_values(rng, (R.HD, R.HN + R.NP))
    tp, td = dev(w_p), dev(w_dh)
    got, want = F_.heads_packs(tp, td), R.heads_packs(w_p, w_dh)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want)
    for k in want:
        same(host_bits(got[k]), want[k].ravel(), 'heads_packs %s' % k)
    same(want['wcat'], R.pack(np.concatenate([np.pad(w_p.T, ((0, 0), (0, 30))), w_dh[:, :R.HN].T], axis=1), 512, 224, 1, 0, 32, 0, 7),
         'wcat is the pair-interleaved pack of [W_p^T (-> 160) | W_dh[:, :512]^T]')
    for H, Ht, E in ((512, 1024, 128), (128, 256, 128)):
        w_ih, w_hh = R.tie_values(rng, (3 * H, Ht + E)), R.tie_values(rng, (3 * H, H))
        ti, th = dev(w_ih), dev(w_hh)
        got, want = F_.notes_packs(ti, th, Ht), R.notes_packs(w_ih, w_hh, Ht)
        torch.cuda.synchronize()
        assert sorted(got) == sorted(want)
        for k in want:
            same(host_bits(got[k]), want[k].ravel(), 'notes_packs H=%d %s' % (H, k))


#                     entry                 N   K  ld pairs trans NT kb0 KBtot
PACK_REFUSALS = {
    'b2 NT * 16 < N': ('ptv_pack_mfma_b2', 17, 33, 36, 0, 0, 1, 0, 2), 'multi NT * 16 < N': ('ptv_pack_mfma_multi', 17, 33, 36, 0, 0, 1, 0, 2),
    'b2 odd NT with pairs': ('ptv_pack_mfma_b2', 48, 33, 36, 1, 0, 3, 0, 2), 'multi odd NT with pairs': ('ptv_pack_mfma_multi', 48, 33, 36, 1, 0, 3, 0, 2),
    'b2 kb0 + KB > KBtot': ('ptv_pack_mfma_b2', 17, 33, 36, 0, 0, 2, 1, 2), 'multi kb0 + KB > KBtot': ('ptv_pack_mfma_multi', 17, 33, 36, 0, 0, 2, 1, 2),
    'b2 kb0 < 0': ('ptv_pack_mfma_b2', 17, 33, 36, 0, 0, 2, -1, 2),
    'b2 ld < K': ('ptv_pack_mfma_b2', 17, 33, 32, 0, 0, 2, 0, 2), 'multi ld < K': ('ptv_pack_mfma_multi', 17, 33, 32, 0, 0, 2, 0, 2),
    'b2 trans ld < N': ('ptv_pack_mfma_b2', 17, 33, 16, 0, 1, 2, 0, 2), 'multi trans ld < N': ('ptv_pack_mfma_multi', 17, 33, 16, 0, 1, 2, 0, 2),
    'b ld < K': ('ptv_pack_mfma_b', 32, 33, 32, 0, 0, 2, 0, 2), 'b N % 32 with pairs': ('ptv_pack_mfma_b', 48, 33, 36, 1, 0, 3, 0, 2),
    'b N = 0': ('ptv_pack_mfma_b', 0, 33, 36, 0, 0, 2, 0, 2), 'b2 K = 0': ('ptv_pack_mfma_b2', 17, 0, 36, 0, 0, 2, 0, 2),
}


@pytest.mark.parametrize('what', list(PACK_REFUSALS))
def test_pack_refusals_leave_out_alone(what):
    entry, N, K, ld, pairs, trans, NT, kb0, KBtot = PACK_REFUSALS[what]
    Wt = dev(np.ones((64, 64), F4))
    rc, got = run_pack(entry, Wt, ld, N, K, pairs, trans, NT, kb0, KBtot, n_el=8 * 8 * 512)
    assert rc == -1
    assert (got == SENT16).all()


def test_pack_refusals_of_the_job_count_and_null_pointers():
    Wt = dev(np.ones((64, 64), F4))
    out = filled((GE + 9 * 2048 + GE,), bf=True)
    row = lambda i: (Wt, 64, 17, 33, out[GE + 2048 * i:], 0, 0, 2, 0, 2)
    assert K_.leaf_rc('ptv_pack_mfma_multi', multi_jobs([row(i) for i in range(9)]), 0) == -1
    assert K_.leaf_rc('ptv_pack_mfma_multi', multi_jobs([row(i) for i in range(9)]), 9) == -1
    assert K_.leaf_rc('ptv_pack_mfma_multi', None, 1) == -1
    assert K_.leaf_rc('ptv_pack_mfma_multi', multi_jobs([row(0), (0,) + row(1)[1:]]), 2) == -1          # (a bad second job: nothing of the first runs)
    assert K_.leaf_rc('ptv_pack_mfma_multi', multi_jobs([row(0), row(1)[:4] + (0,) + row(1)[5:]]), 2) == -1
    assert K_.leaf_rc('ptv_pack_mfma_b', None, 64, 17, 33, out[GE:], 0) == -1
    assert K_.leaf_rc('ptv_pack_mfma_b', Wt, 64, 17, 33, None, 0) == -1
    assert K_.leaf_rc('ptv_pack_mfma_b2', None, 64, 17, 33, out[GE:], 0, 0, 2, 0, 2) == -1
    assert K_.leaf_rc('ptv_pack_mfma_b2', Wt, 64, 17, 33, None, 0, 0, 2, 0, 2) == -1
    torch.cuda.synchronize()
    assert (host_bits(out) == SENT16).all()


# ================================================================================================ B. heads: the runners
_PK = {}


def packs(kind, w_p, w_dh):
    """'lib': functional.heads_packs of the device weights; 'ref': heads_ref.heads_packs, uploaded"""
    key = (kind, w_p.tobytes()[:64], float(np.asarray(w_p, F8).sum()), float(np.asarray(w_dh, F8).sum()))
    if key not in _PK:
        if kind == 'lib':
            from polyphonic_chord_texture_disentanglement_amd import functional as F_
            tp, td = dev(w_p), dev(w_dh)
            _PK[key] = (dict(F_.heads_packs(tp, td)), tp, td)
        elif kind == 'poisoned':
            _PK[key] = ({k: dev_bits(v) for k, v in R.poisoned_heads_packs(w_p, w_dh).items()},)
        else:
            _PK[key] = ({k: dev_bits(v) for k, v in R.heads_packs(w_p, w_dh).items()},)
    return _PK[key][0]


FWD_ARGS = 'hn16 wp wdh wdp b_p b_dh pitch ldp hd0 hd16 M m_top m_unit row_len'.split()
BWD_ARGS = {'ptv_heads_bwd': 'dp ldp dhd0 wdpT wcat dnsum16 blocked dy16 m_top m_unit M'.split(),
            'ptv_heads_bwd_rows': 'dp ldp dhd0 wdpT wcat dnsum16 blocked dy16 m_top m_unit row_len M'.split()}
FWD_N = {'ptv_heads_fwd': 11, 'ptv_heads_fwd_top': 13, 'ptv_heads_fwd_rows': 14}


def run_fwd(c, pk, M, entry=None, ldp=136, hd16=True, m_top=None, m_unit=0, row_len=None, over=None):
    """-> (status, outputs on the host with their guard rows, prediction); hn holds NaN in every row the prediction does not compute"""
    pred = R.dead_fwd(M, m_top, m_unit, row_len)
    hn = np.array(c['hn'], F4, copy=True)
    hn[pred['pitch'] != C_] = np.nan
    o = dict(pitch=filled((G + M + G, ldp)), hd0=filled((G + M + G, R.HD)), hd16=filled((G + M + G, R.HD), bf=True))
    a = dict(hn16=dev(hn, bf=True), wp=pk['wp'], wdh=pk['wdh'], wdp=pk['wdp'], b_p=dev(c['b_p']), b_dh=dev(c['b_dh']), pitch=o['pitch'][G:],
             ldp=ldp, hd0=o['hd0'][G:], hd16=o['hd16'][G:] if hd16 else None, M=M, m_top=ints(m_top), m_unit=m_unit, row_len=ints(row_len))
    a.update(over(a) if callable(over) else (over or {}))
    if entry is None:
        entry = 'ptv_heads_fwd_rows' if row_len is not None else ('ptv_heads_fwd_top' if m_top is not None else 'ptv_heads_fwd')
    rc = K_.leaf_rc(entry, *[a[k] for k in FWD_ARGS[:FWD_N[entry]]])
    torch.cuda.synchronize()
    return rc, {k: v.float().cpu().numpy() for k, v in o.items()}, pred


def check_rows(what, body, pred, want, ncol, pad_zero_ok=False):
    """body [M][ld]: rows predicted COMPUTED hold want[:, :ncol] and the sentinel in their padding; ZERO rows zeros (their padding zeros
    or the sentinel where the header leaves it open); UNTOUCHED rows the sentinel"""
    comp, zero, unt = pred == C_, pred == Z_, pred == U_
    if comp.any():
        same(body[comp][:, :ncol], want[comp][:, :ncol], '%s, computed rows' % what)
    assert (body[comp][:, ncol:] == SENT).all(), '%s: padding of a computed row written' % what
    assert (body[zero][:, :ncol] == 0).all(), '%s: a row that must be zero is not (first: row %d)' % (
        what, np.flatnonzero(zero)[(body[zero][:, :ncol] != 0).any(1)][0])
    pz = body[zero][:, ncol:]
    assert ((pz == SENT) | (pz == 0)).all() if pad_zero_ok else (pz == SENT).all(), '%s: padding of a zero row' % what
    assert (body[unt] == SENT).all(), '%s: a row that must stay untouched was written (first: row %d)' % (
        what, np.flatnonzero(unt)[(body[unt] != SENT).any(1)][0] if unt.any() else -1)


def guards_ok(what, full, M):
    assert (full[:G] == SENT).all() and (full[G + M:] == SENT).all(), '%s: a guard row was written' % what


def check_fwd(tag, out, pred, want, M, hd16=True):
    for k in ('pitch', 'hd0', 'hd16'):
        guards_ok('%s %s' % (tag, k), out[k], M)
    check_rows(tag + ' pitch', out['pitch'][G:G + M], pred['pitch'], want['pitch'], R.NP, pad_zero_ok=True)
    check_rows(tag + ' hd0', out['hd0'][G:G + M], pred['hd0'], want['hd0'], R.HD)
    if hd16:
        check_rows(tag + ' hd16', out['hd16'][G:G + M], pred['hd16'], want['hd16'], R.HD)
    else:
        assert (out['hd16'] == SENT).all()


def run_bwd(c, pk, M, entry=None, ldp=136, dy16=True, blocked=0, m_top=None, m_unit=0, row_len=None, over=None):
    """-> (status, outputs on the host, prediction).  dp: the upstream gradient in the rows that are computed, the sentinel elsewhere and
    in the padding; dhd0: NaN in every row that is not computed"""
    pred = R.dead_bwd(M, m_top, m_unit, row_len, blocked)
    live = pred['dp'] == C_
    dp0 = np.full((G + M + G, ldp), SENT, F4)
    dp0[G:G + M][live, :R.NP] = c['dp'][live]
    dh = np.array(c['dhd0'], F4, copy=True)
    dh[~live] = np.nan
    o = dict(dp=dev(dp0), dnsum=filled((GE + M * R.HN + GE,), bf=True), dy16=filled((G + M + G, 200), bf=True))
    a = dict(dp=o['dp'][G:], ldp=ldp, dhd0=dev(dh), wdpT=pk['wdpT'], wcat=pk['wcat'], dnsum16=o['dnsum'][GE:], blocked=blocked,
             dy16=o['dy16'][G:] if dy16 else None, m_top=ints(m_top), m_unit=m_unit, row_len=ints(row_len), M=M)
    a.update(over(a) if callable(over) else (over or {}))
    if entry is None:
        entry = 'ptv_heads_bwd_rows' if row_len is not None else 'ptv_heads_bwd'
    rc = K_.leaf_rc(entry, *[a[k] for k in BWD_ARGS[entry]])
    torch.cuda.synchronize()
    return rc, {k: v.float().cpu().numpy() for k, v in o.items()}, pred


def check_bwd(tag, out, pred, want, M, blocked=0, dy16=True):
    guards_ok(tag + ' dp', out['dp'], M)
    guards_ok(tag + ' dy16', out['dy16'], M)
    dn = out['dnsum']
    assert (dn[:GE] == SENT).all() and (dn[GE + M * R.HN:] == SENT).all(), '%s dnsum: a guard element was written' % tag
    dn = dn[GE:GE + M * R.HN]
    dn = R.unblocked32(dn.reshape(16, M, 32)) if blocked & 1 else dn.reshape(M, R.HN)
    check_rows(tag + ' dp', out['dp'][G:G + M], pred['dp'], want['dp'], R.NP)
    check_rows(tag + ' dnsum', dn, pred['dnsum'], want['dnsum'], R.HN)
    if dy16:
        check_rows(tag + ' dy16', out['dy16'][G:G + M], pred['dy16'], want['dy16'], 200)
    else:
        assert (out['dy16'] == SENT).all()


def all_sentinels(out):
    return all((v == SENT).all() for v in out.values())


# ================================================================================================ B. heads: the exact cases
@pytest.mark.parametrize('pk', ['lib', 'ref'])
@pytest.mark.parametrize('M', SHAPE_M)
def test_heads_exact_shapes(M, pk):
    """every M on either side of the 16-row MFMA tile, the 32-row wave and the 128-row block; ldp 132 / 136 / 144; hd16 and dy16 given and
    NULL; dnsum row-major and column-blocked; all three forward and both backward entry points"""
    c, want = case_of(M), exact_of(M)
    p = packs(pk, c['w_p'], c['w_dh'])
    for i, ldp in enumerate(LDPS):
        for h16 in (True, False):
            entry = ('ptv_heads_fwd', 'ptv_heads_fwd_top', 'ptv_heads_fwd_rows')[(i + h16) % 3]
            rc, out, pred = run_fwd(c, p, M, entry=entry, ldp=ldp, hd16=h16)
            assert rc == 0
            check_fwd('fwd M=%d ldp=%d hd16=%d' % (M, ldp, h16), out, pred, want, M, h16)
            for blocked in (0, 1):
                entry = ('ptv_heads_bwd', 'ptv_heads_bwd_rows')[(i + blocked) % 2]
                rc, out, pred = run_bwd(c, p, M, entry=entry, ldp=ldp, dy16=h16, blocked=blocked)
                assert rc == 0
                check_bwd('bwd M=%d ldp=%d dy16=%d blocked=%d' % (M, ldp, h16, blocked), out, pred, want, M, blocked, h16)


@pytest.mark.parametrize('lim', FWD_LIMITS, ids=lim_id)
def test_heads_fwd_launch_wide_limit(lim):
    """max(*m_top, 0) + 1 units of m_unit rows are computed, the others keep the sentinel (their hn rows hold NaN)"""
    M = lim['M']
    c, want = case_of(M), exact_of(M)
    for pk in ('lib', 'ref'):
        rc, out, pred = run_fwd(c, packs(pk, c['w_p'], c['w_dh']), M, m_top=lim['m_top'], m_unit=lim['m_unit'])
        assert rc == 0
        assert (pred['pitch'] == C_).sum() == min(M, (max(lim['m_top'], 0) + 1) * lim['m_unit'])
        check_fwd('fwd ' + lim_id(lim), out, pred, want, M)


@pytest.mark.parametrize('blocked', [0, 1, 2, 3])
@pytest.mark.parametrize('lim', BWD_LIMITS, ids=lim_id)
def test_heads_bwd_launch_wide_limit(lim, blocked):
    """rows from (*m_top + 1) * m_unit on: dp untouched; dnsum zeros, in whole dead blocks under bit 1 of `blocked` untouched; dy16 zeros
    beside the live rows of a partly live block and untouched in whole dead blocks"""
    M = lim['M']
    c, want = case_of(M), exact_of(M)
    for pk in ('lib', 'ref'):
        rc, out, pred = run_bwd(c, packs(pk, c['w_p'], c['w_dh']), M, blocked=blocked, m_top=lim['m_top'], m_unit=lim['m_unit'])
        assert rc == 0
        check_bwd('bwd blocked=%d %s' % (blocked, lim_id(lim)), out, pred, want, M, blocked)


@pytest.mark.parametrize('lim', ROWS_CASES, ids=lim_id)
def test_heads_row_len(lim):
    """length-sorted rows: a block whose first row has row_len <= n gets zero logits (hd0 / hd16 untouched) forward and zero dy16 rows
    (dnsum, dp untouched) backward; every other block under the limit is computed in full"""
    M, rl = lim['M'], ROW_LENS[lim['row_len']]
    c, want = case_of(M), exact_of(M)
    for pk in ('lib', 'ref'):
        p = packs(pk, c['w_p'], c['w_dh'])
        rc, out, pred = run_fwd(c, p, M, m_top=lim['m_top'], m_unit=lim['m_unit'], row_len=rl)
        assert rc == 0
        assert {C_, Z_, U_} <= set(pred['pitch'].tolist()) or lim['m_top'] == 3
        check_fwd('fwd ' + lim_id(lim), out, pred, want, M)
        for blocked in (0, 3):
            rc, out, pred = run_bwd(c, p, M, blocked=blocked, m_top=lim['m_top'], m_unit=lim['m_unit'], row_len=rl)
            assert rc == 0
            check_bwd('bwd blocked=%d %s' % (blocked, lim_id(lim)), out, pred, want, M, blocked)


@pytest.mark.parametrize('M', [129, 300])
def test_heads_zero_the_operand_columns_130_to_159_themselves(M):
    """packs that hold ones where clean packs hold zeros -- the rows of wp / wdpT that produce columns 130 .. 143 of the logits / of dP', the
    k 130 .. 159 of wdp / wcat that multiply them: the kernels' own zero fill of those operand columns keeps every output what it was
    (and the padding of pitch / dp rows and columns 130 .. 135 of dy16 what they must be)"""
    c, want = case_of(M), exact_of(M)
    p = packs('poisoned', c['w_p'], c['w_dh'])
    clean = R.heads_packs(c['w_p'], c['w_dh'])
    assert all((host_bits(p[k]) != clean[k].ravel()).any() for k in ('wp', 'wdp', 'wdpT', 'wcat'))
    rc, out, pred = run_fwd(c, p, M)
    assert rc == 0
    check_fwd('fwd, poisoned pack padding', out, pred, want, M)
    for blocked in (0, 1):
        rc, out, pred = run_bwd(c, p, M, blocked=blocked)
        assert rc == 0
        check_bwd('bwd, poisoned pack padding', out, pred, want, M, blocked)


# ================================================================================================ C. real-valued
def bound_of(ref, kp, scale=None):
    """max(4 * max|kp - ref|, 8 ulp_fp32(scale)); scale: default the array's largest magnitude"""
    ref, kp = np.asarray(ref, F8), np.asarray(kp, F8)
    assert ref.shape == kp.shape and np.isfinite(ref).all() and np.isfinite(kp).all()
    scale = np.abs(ref).max() if scale is None else scale
    errk = np.abs(kp - ref).max()
    return max(4.0 * errk, 8.0 * float(np.spacing(F4(scale)))), errk


def check(family, got, ref, kp):
    got, ref = np.asarray(got, F8), np.asarray(ref, F8)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound, errk = bound_of(ref, kp)
    assert np.isfinite(got).all(), '%s: non-finite output' % family
    err = np.abs(got - ref).max()
    ratio = float(err / bound)
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print('HEADS_RATIO %s %.3f (kernel err %.3e, kernel-precision CPU err %.3e)' % (family, ratio, err, errk))
    assert err <= bound, '%s: kernel error %.3e over the bound %.3e (kernel-precision CPU evaluation: %.3e)' % (family, err, bound, errk)


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('HEADS_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


@pytest.mark.parametrize('M', REAL_MS)
def test_heads_real_valued(M):
    c = R.real_case(np.random.RandomState(M), M)
    p = packs('lib', c['w_p'], c['w_dh'])
    pitch, hd0 = R.fwd(c['hn'], c['w_p'], c['w_dh'], c['b_p'], c['b_dh'])
    kp = R.kp_fwd(c['hn'], c['w_p'], c['w_dh'], c['b_p'], c['b_dh'])
    rc, out, pred = run_fwd(c, p, M)
    assert rc == 0
    body = lambda k: out[k][G:G + M]
    check('pitch', body('pitch')[:, :R.NP], pitch, kp[0])
    check('hd0', body('hd0'), hd0, kp[1])
    check('hd16', body('hd16'), hd0, kp[2])
    same(body('hd16'), R.bf16_round(body('hd0')), 'hd16 is the RNE rounding of the hd0 the kernel stored')
    dpp, dn = R.bwd(c['dp'], c['dhd0'], c['w_p'], c['w_dh'])
    kb = R.kp_bwd(c['dp'], c['dhd0'], c['w_p'], c['w_dh'])
    for blocked in (0, 1):
        rc, out, pred = run_bwd(c, p, M, blocked=blocked)
        assert rc == 0
        dns = out['dnsum'][GE:GE + M * R.HN]
        dns = R.unblocked32(dns.reshape(16, M, 32)) if blocked else dns.reshape(M, R.HN)
        check('dp', body('dp')[:, :R.NP], dpp, kb[0])
        check('dnsum', dns, dn, kb[1])
        check('dy16[:, :130]', body('dy16')[:, :R.NP], dpp, kb[2][:, :R.NP])
        same(body('dy16')[:, :R.NP], R.bf16_round(body('dp')[:, :R.NP]), 'dy16 is the RNE rounding of the dp the kernel stored')
        same(body('dy16')[:, R.NP:], kb[2][:, R.NP:], 'dy16: six zeros and the RNE rounding of dhd0')
        assert (body('dp')[:, R.NP:] == SENT).all()


# ================================================================================================ D. refusals
def _flat_off(key, n):
    """the output `key` starting n elements later (still inside its allocation: the guard rows follow)"""
    return lambda a: {key: a[key].reshape(-1)[n:]}


def _copy_off(key, n):
    return lambda a: {key: shifted(a[key], n)}


FWD_REFUSALS = {
    'hn16 NULL': dict(over=dict(hn16=None)), 'wp NULL': dict(over=dict(wp=None)), 'wdh NULL': dict(over=dict(wdh=None)),
    'wdp NULL': dict(over=dict(wdp=None)), 'b_p NULL': dict(over=dict(b_p=None)), 'b_dh NULL': dict(over=dict(b_dh=None)),
    'pitch NULL': dict(over=dict(pitch=None)), 'hd0 NULL': dict(over=dict(hd0=None)),
    'M = 0': dict(over=dict(M=0)), 'M < 0': dict(over=dict(M=-1)), 'ldp = 129': dict(over=dict(ldp=129)), 'ldp = 134': dict(over=dict(ldp=134)),
    'row_len without m_top': dict(entry='ptv_heads_fwd_rows', over=lambda a: dict(row_len=ints([1] * 128), m_unit=128)),
    'm_unit = 0 with m_top': dict(m_top=0, m_unit=128, over=dict(m_unit=0)), 'm_unit = 96 with m_top': dict(m_top=0, m_unit=128, over=dict(m_unit=96)),
    'm_unit < 0 with m_top': dict(m_top=0, m_unit=128, over=dict(m_unit=-128)),
    'pitch off by 4 bytes': dict(over=_flat_off('pitch', 1)), 'hn16 off by 4 bytes': dict(over=_copy_off('hn16', 2)),
    # the alignment checks of the float4 / bf16x8 / bf16x4 accesses
    'b_dh off by 4 bytes': dict(over=_copy_off('b_dh', 1)), 'b_dh off by 8 bytes': dict(over=_copy_off('b_dh', 2)),
    'hd0 off by 4 bytes': dict(over=_flat_off('hd0', 1)), 'hd0 off by 8 bytes': dict(over=_flat_off('hd0', 2)),
    'hd16 off by 2 bytes': dict(over=_flat_off('hd16', 1)), 'hd16 off by 4 bytes': dict(over=_flat_off('hd16', 2)),
    'wp off by 8 bytes': dict(over=_copy_off('wp', 4)), 'wdh off by 8 bytes': dict(over=_copy_off('wdh', 4)),
    'wdp off by 2 bytes': dict(over=_copy_off('wdp', 1)),
}
BWD_REFUSALS = {
    'dp NULL': dict(over=dict(dp=None)), 'dhd0 NULL': dict(over=dict(dhd0=None)), 'wdpT NULL': dict(over=dict(wdpT=None)),
    'wcat NULL': dict(over=dict(wcat=None)), 'dnsum16 NULL': dict(over=dict(dnsum16=None)),
    'M = 0': dict(over=dict(M=0)), 'M < 0': dict(over=dict(M=-1)), 'ldp = 129': dict(over=dict(ldp=129)), 'ldp = 134': dict(over=dict(ldp=134)),
    'row_len without m_top': dict(entry='ptv_heads_bwd_rows', over=lambda a: dict(row_len=ints([1] * 128), m_unit=128)),
    'm_unit = 96 with row_len': dict(m_top=0, m_unit=128, row_len=[1] * 128, over=dict(m_unit=96)),
    'm_unit = 0 with m_top': dict(m_top=0, m_unit=16, over=dict(m_unit=0)), 'm_unit < 0 with m_top': dict(m_top=0, m_unit=16, over=dict(m_unit=-16)),
    'dp off by 4 bytes': dict(over=_flat_off('dp', 1)),
    # the alignment checks
    'dhd0 off by 4 bytes': dict(over=_copy_off('dhd0', 1)), 'dhd0 off by 8 bytes': dict(over=_copy_off('dhd0', 2)),
    'dnsum16 off by 2 bytes': dict(over=_flat_off('dnsum16', 1)), 'dnsum16 off by 8 bytes': dict(over=_flat_off('dnsum16', 4)),
    'dy16 off by 4 bytes': dict(over=_flat_off('dy16', 2)), 'dy16 off by 8 bytes': dict(over=_flat_off('dy16', 4)),
    'wdpT off by 8 bytes': dict(over=_copy_off('wdpT', 4)), 'wcat off by 2 bytes': dict(over=_copy_off('wcat', 1)),
}


@pytest.mark.parametrize('what', list(FWD_REFUSALS))
def test_heads_fwd_refusals_leave_the_outputs_alone(what):
    kw = dict(FWD_REFUSALS[what])
    c = case_of(RM)
    rc, out, pred = run_fwd(c, packs('lib', c['w_p'], c['w_dh']), RM, **kw)
    assert rc == -1
    assert all_sentinels(out)


@pytest.mark.parametrize('what', list(BWD_REFUSALS))
def test_heads_bwd_refusals_leave_the_outputs_alone(what):
    kw = dict(BWD_REFUSALS[what])
    c = case_of(RM)
    rc, out, pred = run_bwd(c, packs('lib', c['w_p'], c['w_dh']), RM, **kw)
    assert rc == -1
    want = np.full_like(out['dp'], SENT)
    live = pred['dp'] == C_
    want[G:G + RM][live, :R.NP] = c['dp'][live]
    same(out['dp'], want, 'dp')
    assert (out['dnsum'] == SENT).all() and (out['dy16'] == SENT).all()


def test_aligned_offsets_are_accepted():
    """the checks refuse no pointer the kernels can use: every operand 16 bytes (hd16: 8 bytes) into its allocation"""
    M = 17
    c, want = case_of(M), exact_of(M)
    p = packs('lib', c['w_p'], c['w_dh'])
    over = lambda a: dict(b_dh=shifted(a['b_dh'], 4), wp=shifted(a['wp'], 8), wdh=shifted(a['wdh'], 8), wdp=shifted(a['wdp'], 8),
                          hn16=shifted(a['hn16'], 8))
    rc, out, pred = run_fwd(c, p, M, over=over)
    assert rc == 0
    check_fwd('fwd shifted operands', out, pred, want, M)
    h8 = filled((4 + M * R.HD + 64,), bf=True)
    rc, out, pred = run_fwd(c, p, M, over=dict(hd16=h8[4:]))
    assert rc == 0
    same(h8.float().cpu().numpy()[4:4 + M * R.HD].reshape(M, R.HD), want['hd16'], 'hd16 8 bytes into its allocation')
    over = lambda a: dict(dhd0=shifted(a['dhd0'], 4), wdpT=shifted(a['wdpT'], 8), wcat=shifted(a['wcat'], 8))
    rc, out, pred = run_bwd(c, p, M, over=over)
    assert rc == 0
    check_bwd('bwd shifted operands', out, pred, want, M)
