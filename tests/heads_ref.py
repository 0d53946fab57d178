"""Plain references (numpy, CPU) of the fused per-note heads -- ptv_heads_fwd / _top / _rows, ptv_heads_bwd / _rows, csrc/heads.hip -- and of
the MFMA-fragment weight packs -- ptv_pack_mfma_b / _b2 / _multi, csrc/freerun.hip -- written from include/ptvae_hip.h ("The per-note heads
fused", the ptv_pack_mfma_b paragraph), not from the kernels: the oracle side of tests/test_gpu_heads_kernels.py, itself held to torch's
float64 operators and autograd by tests/test_heads_ref_host.py.

    fwd:  pitch = hn W_p^T + b_p;                      hd0 = hn W_dh[:, :512]^T + pitch W_dh[:, 512:]^T + b_dh
    bwd:  dP' = dP + dHD0 W_dh[:, 512:]  (in place);    dNSUM = dP' W_p + dHD0 W_dh[:, :512]
    pack: [nt][kb0 + kb][lane][e] = bf16(W(n, k)),  k = 32 kb + 8 (lane / 16) + e,  c = lane % 16,
          n = 16 nt + c  (plain)  or  32 (nt / 2) + 8 (c / 4) + 4 (nt % 2) + c % 4  (pair-interleaved);  zero for n >= N or k >= K

fwd() / bwd() are float64 throughout.  kp_fwd() / kp_bwd() are no references: they evaluate the same formulas in float32 with bf16 RNE
roundings where the kernel comments name them (the weights, hn, the logits as operand of the second product, dhd0, dP' as operand, the
stored dNSUM, hd16, dy16), and their error against fwd() / bwd() is the yardstick of the real-valued tests.  Evaluated in float64
(dt = F8) on the small integers of int_case(), for which every fp32 partial sum in any order is exact (exact_ok), they PREDICT every
output bit for bit."""
import numpy as np

from gemm_ref import bf16_round

F8, F4 = np.float64, np.float32
HN, NP, HD = 512, 130, 64                                    # the init_model() geometry the kernels are built for
COMPUTED, ZERO, UNTOUCHED = 0, 1, 2


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ bf16 as bits
def bf16_bits(a):
    """fp32 -> the bits (uint16) of the nearest bf16, ties to even"""
    return (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


def bits_f32(u):
    return (np.asarray(u, np.uint16).astype(np.uint32) << 16).view(F4)


def tie_values(rng, shape):
    """normal-range reals over 2^+-4, a quarter of them exactly half way between two bf16 neighbours, both parities of the lower one"""
    a = (rng.standard_normal(shape) * np.exp2(rng.uniform(-4, 4, shape))).astype(F4)
    u = a.view(np.uint32)
    m = rng.rand(*shape) < 0.25
    m.flat[:2] = True
    u[m] = (u[m] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    f = np.flatnonzero(m)[:2]
    u.flat[f[0]] &= np.uint32(0xFFFEFFFF)                     # (both parities also in a 1 x 1 ... tiny matrix)
    if f.size > 1:
        u.flat[f[1]] |= np.uint32(0x00010000)
    assert np.isfinite(a).all()
    return a


# ================================================================================================ packs
def pack_rows(NT, pairs):
    """[NT][16]: the row n of W that column c of tile nt holds"""
    nt, c = np.arange(NT)[:, None], np.arange(16)[None, :]
    return 32 * (nt // 2) + 8 * (c // 4) + 4 * (nt % 2) + c % 4 if pairs else 16 * nt + c


def pack(W, N, K, pairs, trans, NT, kb0, KBtot, out=None):
    """W as stored ([>= N][>= K], or [>= K][>= N] with trans; anything beyond N and K is never looked at) -> uint16 [NT][KBtot][64][8]"""
    KB = cdiv(K, 32)
    assert N > 0 and K > 0 and NT * 16 >= N and not (pairs and NT % 2) and 0 <= kb0 and kb0 + KB <= KBtot
    W = np.asarray(W, F4)
    full = np.zeros((NT * 16, KB * 32), F4)
    full[:N, :K] = (W.T if trans else W)[:N, :K]
    lane, e = np.arange(64)[:, None], np.arange(8)[None, :]
    n = pack_rows(NT, pairs)[:, None, lane % 16]                                   # [NT][1][64][8]
    k = (32 * np.arange(KB)[:, None, None] + 8 * (lane // 16) + e)[None]           # [1][KB][64][8]
    out = np.zeros((NT, KBtot, 64, 8), np.uint16) if out is None else np.array(out, np.uint16, copy=True).reshape(NT, KBtot, 64, 8)
    out[:, kb0:kb0 + KB] = bf16_bits(full[n, k])
    return out


def unpack(P, pairs, kb0=0, KB=None):
    """the inverse walk: uint16 [NT][KBtot][64][8] -> fp32 [16 NT][32 KB], the matrix the k-blocks [kb0, kb0 + KB) hold"""
    P = np.asarray(P, np.uint16)
    NT, KBtot = P.shape[:2]
    KB = KBtot - kb0 if KB is None else KB
    W = np.full((NT * 16, KB * 32), np.nan, F4)
    rows = pack_rows(NT, pairs)
    for nt in range(NT):
        for kb in range(KB):
            for lane in range(64):
                W[rows[nt, lane % 16], 32 * kb + 8 * (lane // 16):32 * kb + 8 * (lane // 16) + 8] = bits_f32(P[nt, kb0 + kb, lane])
    return W


def heads_packs(w_p, w_dh):
    """the six packs of functional.heads_packs (wcat by two jobs into one buffer): dict of uint16 [NT][KBtot][64][8]"""
    w_p, w_dh = np.asarray(w_p, F4), np.asarray(w_dh, F4)
    assert w_p.shape == (NP, HN) and w_dh.shape == (HD, HN + NP)
    w_dp = w_dh[:, HN:]
    wcat = pack(w_p, HN, NP, 1, 1, HN // 16, 0, 7)                                 # k-blocks 0-4: W_p^T, 130 columns zero-padded to 160
    wcat = pack(w_dh, HN, HD, 1, 1, HN // 16, 5, 7, out=wcat)                      # k-blocks 5-6: W_dh[:, :512]^T
    return dict(wp=pack(w_p, NP, HN, 0, 0, 9, 0, HN // 32), wdh=pack(w_dh, HD, HN, 0, 0, HD // 16, 0, HN // 32),
                wdp=pack(w_dp, HD, NP, 0, 0, HD // 16, 0, 5), wdpT=pack(w_dp, NP, HD, 0, 1, 9, 0, HD // 32), wcat=wcat)


def poisoned_heads_packs(w_p, w_dh, v=1.0):
    """heads_packs with `v` instead of zeros where a pack meets columns 130 .. 159 of the logits / of dP' as an operand -- rows 130 .. 143 of
    wp and wdpT (the outputs that become those columns), k 130 .. 159 of wdp and wcat (what multiplies them).  The header: the kernels zero
    those operand columns themselves, so every output is what the clean packs give"""
    w_p, w_dh = np.asarray(w_p, F4), np.asarray(w_dh, F4)
    w_dp = w_dh[:, HN:]
    fill = lambda a, rows, cols: np.concatenate([np.concatenate([a, np.full((a.shape[0], cols), v, F4)], axis=1),
                                                 np.full((rows, a.shape[1] + cols), v, F4)], axis=0)
    cat = np.concatenate([fill(w_p.T, 0, 30), w_dh[:, :HN].T], axis=1)             # [512][160 | 64]
    return dict(wp=pack(fill(w_p, 14, 0), NP + 14, HN, 0, 0, 9, 0, HN // 32), wdh=pack(w_dh, HD, HN, 0, 0, HD // 16, 0, HN // 32),
                wdp=pack(fill(w_dp, 0, 30), HD, NP + 30, 0, 0, HD // 16, 0, 5), wdpT=pack(fill(w_dp.T, 14, 0), NP + 14, HD, 0, 0, 9, 0, HD // 32),
                wcat=pack(cat, HN, 224, 1, 0, HN // 16, 0, 7))


def notes_packs(w_ih, w_hh, Ht):
    """the three packs of functional.notes_packs"""
    w_ih, w_hh = np.asarray(w_ih, F4), np.asarray(w_hh, F4)
    H3, H = w_hh.shape
    w_x = w_ih[:, Ht:]
    E = w_x.shape[1]
    pf = 0 if H == 512 else 1
    return dict(wg_h=pack(w_hh, H3, H, pf, 0, H3 // 16, 0, cdiv(H, 32)), wg_t=pack(w_x, H3, E, pf, 0, H3 // 16, 0, cdiv(E, 32)),
                wt=pack(w_hh, H, H3, 1, 1, H // 16, 0, cdiv(H3, 32)))


# ================================================================================================ the heads
def fwd(hn, w_p, w_dh, b_p, b_dh):
    hn, w_p, w_dh = np.asarray(hn, F8), np.asarray(w_p, F8), np.asarray(w_dh, F8)
    pitch = hn @ w_p.T + np.asarray(b_p, F8)
    hd0 = hn @ w_dh[:, :HN].T + pitch @ w_dh[:, HN:].T + np.asarray(b_dh, F8)
    return pitch, hd0


def bwd(dp, dhd0, w_p, w_dh):
    dp, dhd0, w_p, w_dh = np.asarray(dp, F8), np.asarray(dhd0, F8), np.asarray(w_p, F8), np.asarray(w_dh, F8)
    dpp = dp + dhd0 @ w_dh[:, HN:]
    return dpp, dpp @ w_p + dhd0 @ w_dh[:, :HN]


def _r(x, dt):
    """the bf16 rounding of a value the kernel holds in fp32 (dt = F8: the value must be one fp32 holds, as exact_ok guarantees)"""
    x4 = np.asarray(x, F4)
    assert dt is F4 or np.array_equal(x4.astype(F8), np.asarray(x, F8))
    return bf16_round(x4).astype(dt)


def kp_fwd(hn, w_p, w_dh, b_p, b_dh, dt=F4):
    """-> pitch, hd0, hd16 (as values)"""
    h, wp, wd = _r(hn, dt), _r(w_p, dt), _r(w_dh, dt)
    pitch = ((h @ wp.T).astype(dt) + np.asarray(b_p, dt)).astype(dt)
    hd0 = ((h @ wd[:, :HN].T).astype(dt) + (_r(pitch, dt) @ wd[:, HN:].T).astype(dt) + np.asarray(b_dh, dt)).astype(dt)
    return pitch, hd0, _r(hd0, dt)


def kp_bwd(dp, dhd0, w_p, w_dh, dt=F4):
    """-> dP', dNSUM (bf16 values), dy16 [M][200] (bf16 values) = [dP' (130) | 0 (6) | dhd0 (64)]"""
    wp, wd, dh = _r(w_p, dt), _r(w_dh, dt), _r(dhd0, dt)
    dpp = (np.asarray(dp, dt) + (dh @ wd[:, HN:]).astype(dt)).astype(dt)
    d16 = _r(dpp, dt)
    dn = _r(((d16 @ wp).astype(dt) + (dh @ wd[:, :HN]).astype(dt)).astype(dt), dt)
    return dpp, dn, np.concatenate([d16, np.zeros((d16.shape[0], 6), dt), dh], axis=1)


# ================================================================================================ which rows are written
def _block_first_dead(M, m_unit, row_len):
    """bool [M]: the row's 128-row block starts at a row with no target at its note step (row_len[r] <= n)"""
    rb = np.arange(M, dtype=np.int64) // 128 * 128
    if row_len is None:
        return np.zeros(M, bool)
    return np.asarray(row_len, np.int64)[rb % m_unit] <= rb // m_unit


def dead_fwd(M, m_top=None, m_unit=0, row_len=None):
    """per row, COMPUTED / ZERO / UNTOUCHED for pitch[:, :130], hd0, hd16.  The launch-wide limit: rows from (max(*m_top, 0) + 1) * m_unit
    on stay unwritten; row_len: blocks whose first row has no target get zero logits, hd0 / hd16 unwritten"""
    r = np.arange(M, dtype=np.int64)
    assert m_top is None or (m_unit > 0 and m_unit % 128 == 0)
    beyond = np.zeros(M, bool) if m_top is None else r >= (max(int(m_top), 0) + 1) * m_unit
    skip = _block_first_dead(M, m_unit, row_len) & ~beyond
    hd = np.where(beyond | skip, UNTOUCHED, COMPUTED)
    return dict(pitch=np.where(beyond, UNTOUCHED, np.where(skip, ZERO, COMPUTED)), hd0=hd, hd16=hd.copy())


def dead_bwd(M, m_top=None, m_unit=0, row_len=None, blocked=0):
    """per row, COMPUTED / ZERO / UNTOUCHED for dp, dnsum, dy16.  Rows from (*m_top + 1) * m_unit on are zero: dp stays, dnsum is zeros --
    in a WHOLE dead 128-row block left unwritten under bit 1 of `blocked` --, dy16 holds the live rows (zeros beside them in a partly
    live block, nothing in a whole dead one); row_len: blocks under the limit whose first row has no target get zero dy16 rows and
    nothing else"""
    r = np.arange(M, dtype=np.int64)
    live = M if m_top is None else min(M, max((int(m_top) + 1) * m_unit, 0))
    dead = r >= live
    whole = r // 128 * 128 >= live
    skip = _block_first_dead(M, m_unit, row_len) & ~whole
    dnsum = np.where(skip, UNTOUCHED, np.where(whole & bool(blocked & 2), UNTOUCHED, np.where(dead, ZERO, COMPUTED)))
    return dict(dp=np.where(dead | skip, UNTOUCHED, COMPUTED), dnsum=dnsum,
                dy16=np.where(skip, ZERO, np.where(whole, UNTOUCHED, np.where(dead, ZERO, COMPUTED))))


# ================================================================================================ layouts
def blocked32(x):
    """[M][512] -> [16][M][32]: element (m, u) at ((u / 32) * M + m) * 32 + u % 32"""
    M, N = x.shape
    assert N % 32 == 0
    return np.ascontiguousarray(x.reshape(M, N // 32, 32).transpose(1, 0, 2))


def unblocked32(xb):
    nb, M, w = xb.shape
    assert w == 32
    return np.ascontiguousarray(xb.transpose(1, 0, 2).reshape(M, nb * 32))


# ================================================================================================ exact operands
def exact_ok(c):
    """the largest magnitude any partial sum of the case can reach -- forward: |hn| |W_p|^T + |b_p|, then |hn| |W_dh[:, :512]|^T +
    |bf16(pitch)| |W_dh[:, 512:]|^T + |b_dh| with the logits of largest magnitude the first sum allows; backward alike with the rounded
    dP' -- asserted below 2^23: then every fp32 addition of the kernels, in any order, is exact"""
    a = lambda k: np.abs(np.asarray(c[k], F8))
    wp, wd = a('w_p'), a('w_dh')
    p = a('hn') @ wp.T + a('b_p')                                                  # bounds every partial sum of the logits
    p16 = p * (1 + 2.0 ** -8)                                                      # ... and their rounding (at most half a bf16 ulp up)
    h = a('hn') @ wd[:, :HN].T + p16 @ wd[:, HN:].T + a('b_dh')
    d = a('dp') + a('dhd0') @ wd[:, HN:]
    d16 = d * (1 + 2.0 ** -8)
    n = d16 @ wp + a('dhd0') @ wd[:, :HN]
    top_f, top_b = float(max(p.max(), h.max())), float(max(d.max(), n.max()))
    assert max(top_f, top_b) < 2.0 ** 23, 'largest partial sum: forward %g, backward %g, not below 2^23' % (top_f, top_b)
    return top_f, top_b


def int_case(rng, M):
    """operands, biases and upstream gradients of integers in [-4, 4] (exact in bf16): dict(hn, w_p, w_dh, b_p, b_dh, dp, dhd0), fp32"""
    iv = lambda *s: rng.randint(-4, 5, s).astype(F4)
    c = dict(hn=iv(M, HN), w_p=iv(NP, HN), w_dh=iv(HD, HN + NP), b_p=iv(NP), b_dh=iv(HD), dp=iv(M, NP), dhd0=iv(M, HD))
    exact_ok(c)
    return c


def real_case(rng, M):
    """Gaussian operands, weights of 1 / sqrt(fan-in); hn is a bf16 tensor in the library: bf16 numbers"""
    g = lambda *s: rng.standard_normal(s)
    return dict(hn=bf16_round((0.5 * g(M, HN)).astype(F4)), w_p=(g(NP, HN) / np.sqrt(HN)).astype(F4),
                w_dh=(g(HD, HN + NP) / np.sqrt(HN + NP)).astype(F4), b_p=(0.1 * g(NP)).astype(F4), b_dh=(0.1 * g(HD)).astype(F4),
                dp=(0.1 * g(M, NP)).astype(F4), dhd0=(0.1 * g(M, HD)).astype(F4))
