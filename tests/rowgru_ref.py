"""Plain fp64 references (numpy, CPU) of the row-partitioned persistent GRUs -- csrc/notes_persist.hip (row_gru_fwd_kernel<128, true>,
row_gru_bwd_kernel<128, true>, the 4-wave row_gru_bwd_kernel<512, false>) and csrc/notes_roles.hip (the 8-wave notes_fwd_kernel /
notes_bwd_kernel) behind ptv_notes_gru_persist_{fwd,bwd}{,_top,_rows} and ptv_row_gru_persist_{fwd,bwd}{,_perm}: the oracle side of
tests/test_gpu_rowgru_kernels.py, itself held to torch's float64 nn.GRU and autograd by tests/test_rowgru_ref_host.py.

A thin layer over tests/gru_ref.py: the cell (gru_forward / gru_backward) and its kernel-precision evaluation (kp_forward / kp_backward)
are that file's.  This one adds what the row kernels fuse and promise around the cell:

  * the input side.  H = 128: gi[t] = x[t] . W_x^T + b_ih.  H = 512: gi[t] = gc + emb[t] . W_tok^T (gc = the hoisted part, b_ih folded).
    kp_*: tokens and weights rounded to bf16, gc held as bf16, the state operand bf16, saved gates bf16; BPTT: the dgh operand bf16, dgi
    and dgh stored as bf16 (H = 512: the previous state read from the bf16 copy HN16 -- the caller passes that as `hprev`).
  * the layouts, written from include/ptvae_hip.h and checked against the sources: gc column-blocked by 16 ([3H/16][R][16]); ext, the
    [T*R][H] matrix, column-blocked by 32 ([H/32][T*R][32]); the saved gate planes unit-blocked by 16 (H = 512, notes_roles.hip blk16)
    or by 32 (H = 128, notes_persist.hip gate_off); dgh of H = 512 holds the n third only.
  * perm: x, lengths, out, dh_last and dgi are indexed by row perm[p]; HN, HN16, gates and dgh by panel position p.  The references
    below work in NATURAL row order (rows are independent) and to_pos / to_nat move between the two.
  * a three-valued expectation for every output slot: LIVE (compared with the reference), ZERO (exact zero bits), UNWRITTEN (keeps the
    caller's bits), and EITHER (zero or untouched, nothing else) where the header says rows "may stay unwritten" (T bit 16 / bit 24).
    A class is uniform over the H units of a (slot, row), so the class arrays are [slots, R].

Behaviour of the sources that the expectations model (read there, not in the header, before this file was written):
  * the H = 512 forward runs step 0 even when *live_top < 0: Tg = min(T, max(*live_top, 0) + 1).
  * deadness under row_len is per 128-row BLOCK: a 64-row panel takes row_len[r0 & ~127], the length of its block's first row.
  * the launch-wide dead-time limit of H = 128 (time indices at or beyond the longest row of the launch) exists only when R % 32 == 0;
    the forward needs ptv_zero_skip on for it (and for the panel limit), the BPTT needs top_step given (its panel limit needs only lengths).
  * H = 128 with lengths: a panel's steps beyond its longest row copy the state (HN and HN16 slot n + 1), gates unwritten; the BPTT
    writes zero rows there.  The reversed direction's launch-wide dead PREFIX leaves slots 1 .. n - 1 unwritten and materialises slot n
    in front of the first live step n.
  * ptv_zero_skip(0): the H = 512 BPTT ignores bound and row_len and computes every step (exact zeros, of either sign, where nothing arrives).
  * top_step is atomicMax'ed into the caller's value.  H = 512: the last step with a non-zero ext row (-0.0 counts as zero) in any panel,
    searched downward from min(T - 1, *bound) and, under row_len, not above row_len[block] - 1.  H = 128 (lengths given): the largest
    min(length, T) - 1 that is >= 0."""
import numpy as np

import gru_ref as G
from gemm_ref import bf16_round, from_blocked, to_blocked

F8, F4 = np.float64, np.float32
E, PANEL, BLOCK = 128, 64, 128
LIVE, ZERO, UNWRITTEN, EITHER = 1, 2, 3, 4


def cdiv(a, b):
    return -(-a // b)


def panels(R):
    return [(a, min(R, a + PANEL)) for a in range(0, R, PANEL)]


# ================================================================================================ layouts
def gate_block(H):
    return {128: 32, 512: 16}[H]


def gc_blocked(gc):
    """[R, 3H] -> [3H/16][R][16]"""
    return to_blocked(np.asarray(gc), 16)


def ext_blocked(ext):
    """[T, R, H] -> the [T*R][H] matrix column-blocked by 32: [H/32][T*R][32]"""
    T, R, H = ext.shape
    return to_blocked(np.asarray(ext).reshape(T * R, H), 32)


def ext_unblocked(blk, T):
    return from_blocked(blk, 32).reshape(T, blk.shape[1] // T, -1)


def gates_blocked(gates, H):
    """[T, 4, R, H] -> [T][4][H/w][R][w], w = gate_block(H)"""
    w = gate_block(H)
    return np.stack([np.stack([to_blocked(p, w) for p in step]) for step in np.asarray(gates)])


def gates_unblocked(blk, H):
    w = gate_block(H)
    return np.stack([np.stack([from_blocked(p, w) for p in step]) for step in blk])


def dgh_stored(dgh, H):
    """the [T, R, 3H] gradient of the hidden-side pre-activations as the BPTT stores it: whole (H = 128) or its n third (H = 512)"""
    return dgh if H == 128 else dgh[:, :, 2 * H:]


def to_pos(a, perm, axis):
    """natural row order -> panel positions: position p holds row perm[p]"""
    return a if perm is None else np.take(a, np.asarray(perm), axis=axis)


def to_nat(a, perm, axis):
    if perm is None:
        return a
    inv = np.empty(len(perm), np.int64)
    inv[np.asarray(perm)] = np.arange(len(perm))
    return np.take(a, inv, axis=axis)


def by_length(lengths):
    """ptv_rows_by_length: descending length, ties in row order"""
    return np.argsort(-np.asarray(lengths, np.int64), kind='stable').astype(np.int32)


# ================================================================================================ the fused input side
def gi_of(H, x, w_x, b_ih=None, gc=None):
    """x [T, R, 128] fed tokens, w_x [3H, 128]; H = 128: b_ih [3H]; H = 512: gc [R, 3H] -> gi [T, R, 3H] by TIME, float64"""
    x, w_x = np.asarray(x, F8), np.asarray(w_x, F8)
    assert (b_ih is None) == (H == 512) and (gc is None) == (H == 128)
    return x @ w_x.T + (np.asarray(b_ih, F8) if H == 128 else np.asarray(gc, F8)[None])


def kp_gi_of(H, x, w_x, b_ih=None, gc=None):
    p = (bf16_round(x) @ bf16_round(w_x).T).astype(F4)
    return (p + (np.asarray(b_ih, F4) if H == 128 else bf16_round(gc)[None])).astype(F4)


def forward(H, x, w_x, w_hh, b_hh, h0, b_ih=None, gc=None, lengths=None, reverse=False):
    """-> states [T + 1, R, H] (slot 0 = h0, slot s + 1 = the state after processing step s), gates [T, 4, R, H] by processing step;
    natural row order, float64"""
    hs, gates = G.gru_forward(gi_of(H, x, w_x, b_ih, gc), None, w_hh, b_hh, h0, lengths, reverse, None)
    return np.concatenate([np.asarray(h0, F8)[None], hs]), gates


def kp_forward(H, x, w_x, w_hh, b_hh, h0, b_ih=None, gc=None, lengths=None, reverse=False):
    """the same at the kernels' precision -> states fp32, gates (bf16 values), states16"""
    hs, gates, _ = G.kp_forward(kp_gi_of(H, x, w_x, b_ih, gc), None, w_hh, b_hh, h0, lengths, reverse, None, bf16=True, gates_bf16=True)
    st = np.concatenate([np.asarray(h0, F4)[None], hs])
    return st, gates, bf16_round(st)


def backward(H, hprev, gates, w_hh, ext=None, dh_last=None, reverse=False):
    """hprev [T, R, H] = the stored states 0 .. T-1 (H = 128: fp32 HN; H = 512: the bf16 copy HN16), gates [T, 4, R, H] as stored, ext
    [T, R, H] by processing step -> dgi [T, R, 3H] by TIME, dgh as stored by processing step, dh0; float64"""
    dgi, dgh, dh0, _ = G.gru_backward(hprev, gates, w_hh, ext, dh_last, None, None, reverse)
    return dgi, dgh_stored(dgh, H), dh0


def kp_backward(H, hprev, gates, w_hh, ext=None, dh_last=None, reverse=False):
    dgi, dgh, dh0, _ = G.kp_backward(hprev, gates, w_hh, ext, dh_last, None, None, reverse, bf16=True, dg_bf16=True)
    return dgi, dgh_stored(dgh, H), dh0


# ================================================================================================ the test inputs' row lists
def lengths_of(R, T, kind):
    """H = 128 lengths in natural row order.
    'mixed': the first panel holds every length T, T-1, .., 0 (a row of length 0 from R = T + 1 on, the row of length T first); the rows
             from 64 on are no longer than T // 2, so every later panel has late steps that are dead for all of its rows.
    'short': 0 .. T - 2 in turn (all 0 up to T = 2): no row reaches the times T - 2 and T - 1, which are then dead for the whole launch
             (R % 32 == 0) -- the last two processing steps forward, a dead PREFIX of two in the reversed direction."""
    i = np.arange(R)
    if kind == 'mixed':
        return np.where(i < PANEL, (T - i) % (T + 1), i % (T // 2 + 1)).astype(np.int32)
    assert kind == 'short'
    return (i % max(T - 1, 1)).astype(np.int32)


def row_len_of(R, T, dead=0):
    """H = 512 live steps per position, descending: T, T-1, T-2, T-3 in runs of 32 over the first 128-row block, `dead` (default 0: a block
    that is dead under row_len) from row 128 on"""
    i = np.arange(R)
    rl = np.where(i < BLOCK, np.maximum(T - i // 32, 0), min(dead, max(T - 3, 0))).astype(np.int32)
    assert (np.diff(rl) <= 0).all()
    return rl


# ================================================================================================ expectations
def _plen(lens, a, b, T):
    return min(max(int(lens[a:b].max()), 0), T)


def expect_fwd128(R, T, lengths=None, perm=None, reverse=False, skip=True):
    """-> HN [T+1, R] (slot 0: the caller's, UNWRITTEN), HN16 [T+1, R], gates [T, R] by position, final [R] = the slot `out` copies"""
    lens = None if lengths is None else to_pos(np.asarray(lengths), perm, 0)
    HN, HN16, gates = (np.full(s, UNWRITTEN, np.uint8) for s in ((T + 1, R), (T + 1, R), (T, R)))
    HN16[0] = LIVE
    final = np.zeros(R, np.int64)
    limits = lens is not None and skip
    gmax = min(max(int(lens.max()), 0), T) if limits and R % 32 == 0 else T
    for a, b in panels(R):
        pmax = _plen(lens, a, b, T) if limits else T
        slot = 0
        for n in range(T):
            tt = G.time_of(n, T, reverse)
            if tt >= gmax:
                continue
            if slot != n:
                HN[n, a:b] = HN16[n, a:b] = LIVE
            HN[n + 1, a:b] = HN16[n + 1, a:b] = LIVE
            if tt < pmax:
                gates[n, a:b] = LIVE
            slot = n + 1
        final[a:b] = slot
    return dict(HN=HN, HN16=HN16, gates=gates, final=final)


def expect_bwd128(R, T, lengths=None, perm=None, reverse=False, top_given=False, top_init=-1):
    """-> dgi [T, R] by (time, natural row), dgh [T, R] by (step, position), top = the expected top_step"""
    lens = None if lengths is None else to_pos(np.asarray(lengths), perm, 0)
    dgi, dgh = np.full((T, R), UNWRITTEN, np.uint8), np.full((T, R), UNWRITTEN, np.uint8)
    nat = np.arange(R) if perm is None else np.asarray(perm)
    gmax = min(max(int(lens.max()), 0), T) if lens is not None and top_given and R % 32 == 0 else T
    top = top_init
    for a, b in panels(R):
        pmax = _plen(lens, a, b, T) if lens is not None else T
        if lens is not None and pmax > 0:
            top = max(top, pmax - 1)
        for s in range(T):
            tt = G.time_of(s, T, reverse)
            if tt >= gmax:
                continue
            dgh[s, a:b] = dgi[tt, nat[a:b]] = LIVE if tt < pmax else ZERO
    return dict(dgi=dgi, dgh=dgh, top=top if top_given else None)


def expect_fwd512(R, T, live_top=None, row_len=None, nofill=False):
    """-> HN16 [T+1, R], gates [T, R], steps [R] = the steps each row's panel runs"""
    HN16, gates = np.full((T + 1, R), UNWRITTEN, np.uint8), np.full((T, R), UNWRITTEN, np.uint8)
    steps = np.zeros(R, np.int64)
    Tg = T if live_top is None else min(T, max(int(live_top), 0) + 1)
    for a, b in panels(R):
        Tp = Tg if row_len is None else min(Tg, max(int(row_len[a & ~(BLOCK - 1)]), 0))
        HN16[:Tp + 1, a:b] = LIVE
        gates[:Tp, a:b] = LIVE
        HN16[Tp + 1:Tg + 1, a:b] = EITHER if nofill else ZERO
        steps[a:b] = Tp
    return dict(HN16=HN16, gates=gates, steps=steps)


def expect_bwd512(R, T, ext, skip=True, bound=None, row_len=None, nofill=False, top_given=False, top_init=-1):
    """ext [T, R, H] as the caller holds it (it may hold anything where the contract says it is not read) -> dgi, dgh [T, R], top, and
    last [R] = the last step computed for the row's panel (-1: none): what arrives after it is zero for the reference"""
    dgi = np.full((T, R), UNWRITTEN, np.uint8)
    last = np.zeros(R, np.int64)
    top = top_init
    if not skip:
        dgi[:] = LIVE
        last[:] = T - 1
        return dict(dgi=dgi, dgh=dgi.copy(), top=max(top, T - 1) if top_given else None, last=last)
    s0 = T - 1 if bound is None else min(T - 1, max(int(bound), -1))
    for a, b in panels(R):
        s_panel = s0 if bound is None or row_len is None else min(s0, int(row_len[a & ~(BLOCK - 1)]) - 1)
        s = s0
        while s >= 0:
            if s <= s_panel and (np.asarray(ext[s, a:b]) != 0).any():         # (-0.0 == 0; NaN != 0, as the kernel's bit test has it)
                break
            dgi[s, a:b] = EITHER if nofill and s > s_panel else ZERO
            s -= 1
        dgi[:s + 1, a:b] = LIVE
        last[a:b] = s
        if s >= 0:
            top = max(top, s)
    return dict(dgi=dgi, dgh=dgi.copy(), top=top if top_given else None, last=last)


def ext_as_read(ext, last):
    """the arriving gradient the BPTT works with: zero after each row's last computed step"""
    out = np.array(ext, F4, copy=True)
    for s in range(out.shape[0]):
        out[s, last < s] = 0.0
    return out
