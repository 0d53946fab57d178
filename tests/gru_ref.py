"""Plain fp64 references (numpy, CPU) of the per-step GRU cell kernels of csrc/gru.hip -- ptv_gru_seq_fwd, ptv_gru_step_fwd and
ptv_gru_seq_bwd -- written from the formulas of that file's header and of include/ptvae_hip.h ("GRU recurrence"): the oracle side of
tests/test_gpu_gru_kernels.py, itself held to torch's float64 nn.GRU and autograd by tests/test_gru_ref_host.py.

    r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   hn = W_hn h + b_hn   n = tanh(gi_n + r hn)   h' = (1 - z) n + z h

Processing step s consumes time t = s, or T-1-s when reversed.  Row m is live at time t iff t < lengths[m]; a dead row keeps its state
and saves the gates (0, 1, 0, hn).  gi_idx redirects the gi row (a token table), never the gi2 row.

The second half (kp_*) evaluates the same formulas in float32, in the order the kernels write them, with bf16 rounding where the chosen
configuration rounds.  It is no reference: its error against the fp64 functions is the yardstick the kernels' error is held to.
plan_fwd / plan_bwd mirror the host dispatch (which kernel variant, which tile) from constants parsed out of the sources."""
import os
import re

import numpy as np

from gemm_ref import bf16_round, is_bf16  # noqa: F401  (bf16_round is held to torch by test_gemm_ref_host.py)

F8, F4 = np.float64, np.float32


def _f8(a):
    return None if a is None else np.asarray(a, dtype=F8)


def _f4(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=F4))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def live_mask(lengths, t, M):
    return np.ones(M, bool) if lengths is None else t < np.asarray(lengths)


def time_of(s, T, reverse):
    return T - 1 - s if reverse else s


def gru_forward(gi, gi2, w_hh, b_hh, h0, lengths, reverse, gi_idx, h0_operand=None):
    """gi [T, R, 3H] (R = M, or the table's rows under gi_idx), gi2 [T, M, 3H] or None, h0 [M, H] -> h [T, M, H] (state after step s),
    gates [T, 4, M, H] = (r, z, n, hn) by processing step.  h0_operand: what the recurrent product of step 0 sees in place of h0"""
    gi, gi2, w_hh, b_hh, h0, h0_operand = (_f8(a) for a in (gi, gi2, w_hh, b_hh, h0, h0_operand))
    T = gi.shape[0]
    M, H = h0.shape
    hs, gates = np.zeros((T, M, H), F8), np.zeros((T, 4, M, H), F8)
    h = h0
    for s in range(T):
        t = time_of(s, T, reverse)
        x = gi[t] if gi_idx is None else gi[t][np.asarray(gi_idx)]
        if gi2 is not None:
            x = x + gi2[t]
        gh = (h0_operand if s == 0 and h0_operand is not None else h) @ w_hh.T + b_hh
        r = _sigmoid(x[:, :H] + gh[:, :H])
        z = _sigmoid(x[:, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        n = np.tanh(x[:, 2 * H:] + r * hn)
        dead = ~live_mask(lengths, t, M)
        r[dead], z[dead], n[dead] = 0.0, 1.0, 0.0
        h = (1.0 - z) * n + z * h
        hs[s], gates[s] = h, (r, z, n, hn)
    return hs, gates


def gru_backward(hprev, gates, w_hh, dh_ext, dh_last, lr_a, lr_b, reverse):
    """one BPTT from given states hprev [T, M, H] (the state BEFORE step s) and gates [T, 4, M, H]; dh_ext [T, M, H] and lr_a [T, M, k]
    by processing step (or None), dh_last [M, H] added at step T-1 only, lr_b [k, H] -> dgi [T, M, 3H] by TIME (dr, dz, dn: gradients of
    the three pre-activations), dgh [T, M, 3H] by processing step (dr, dz, dn r: dn r is the gradient of hn), dh0 [M, H] and the last
    dhz = dh x z, that of step 0"""
    hprev, gates, w_hh, dh_ext, dh_last, lr_a, lr_b = (_f8(a) for a in (hprev, gates, w_hh, dh_ext, dh_last, lr_a, lr_b))
    T, M, H = hprev.shape
    dgi, dgh = np.zeros((T, M, 3 * H), F8), np.zeros((T, M, 3 * H), F8)
    carry = np.zeros((M, H), F8)                                    # dgh_{s+1} . W_hh + dhz_{s+1}
    dhz = carry
    for s in range(T - 1, -1, -1):
        r, z, n, hn = gates[s]
        dh = carry.copy()
        if dh_ext is not None:
            dh += dh_ext[s]
        if dh_last is not None and s == T - 1:
            dh += dh_last
        if lr_a is not None:
            dh += lr_a[s] @ lr_b
        dn = dh * (1.0 - z) * (1.0 - n * n)
        dz = dh * (hprev[s] - n) * z * (1.0 - z)
        dr = dn * hn * r * (1.0 - r)
        dgi[time_of(s, T, reverse)] = np.concatenate([dr, dz, dn], axis=1)
        dgh[s] = np.concatenate([dr, dz, dn * r], axis=1)
        dhz = dh * z
        carry = dgh[s] @ w_hh + dhz
    return dgi, dgh, carry, dhz


# ================================================================================================ the kernels' own precision
def _sigmoid4(x):
    return (F4(1) / (F4(1) + np.exp(-x, dtype=F4))).astype(F4)


def _rnd(a, on):
    return bf16_round(a) if on else _f4(a)


def kp_forward(gi, gi2, w_hh, b_hh, h0, lengths, reverse, gi_idx, h0_operand=None, bf16=False, gates_bf16=False):
    """gru_forward in float32: (gi + gi2) + acc + b, hn = acc + b, no contraction.  bf16: the state operand of the product and W_hh are
    rounded to bf16 (staged fp32 or the bf16 shadow: the same values); gates_bf16: the stored gates.  -> h, gates, h16 = bf16(h)"""
    gi, gi2, w_hh, b_hh, h0, h0_operand = (_f4(a) for a in (gi, gi2, w_hh, b_hh, h0, h0_operand))
    T = gi.shape[0]
    M, H = h0.shape
    w = _rnd(w_hh, bf16)
    hs, gates = np.zeros((T, M, H), F4), np.zeros((T, 4, M, H), F4)
    h = h0
    for s in range(T):
        t = time_of(s, T, reverse)
        x = gi[t] if gi_idx is None else gi[t][np.asarray(gi_idx)]
        if gi2 is not None:
            x = x + gi2[t]
        op = h0_operand if s == 0 and h0_operand is not None else h
        acc = (_rnd(op, bf16) @ w.T).astype(F4)
        r = _sigmoid4(x[:, :H] + acc[:, :H] + b_hh[:H])
        z = _sigmoid4(x[:, H:2 * H] + acc[:, H:2 * H] + b_hh[H:2 * H])
        hn = acc[:, 2 * H:] + b_hh[2 * H:]
        n = np.tanh(x[:, 2 * H:] + r * hn).astype(F4)
        dead = ~live_mask(lengths, t, M)
        r[dead], z[dead], n[dead] = 0.0, 1.0, 0.0
        h = ((F4(1) - z) * n + z * h).astype(F4)
        hs[s], gates[s] = h, (r, z, n, hn)
    return hs, _rnd(gates, gates_bf16), bf16_round(hs)


def kp_backward(hprev, gates, w_hh, dh_ext, dh_last, lr_a, lr_b, reverse, bf16=False, dg_bf16=False):
    """gru_backward in float32.  bf16: the dgh read back by the next step's product (and by the dh0 product) and W_hh are rounded to bf16;
    dg_bf16: dgi / dgh are stored in bf16.  -> dgi, dgh, dh0, dhz as stored"""
    hprev, gates, w_hh, dh_ext, dh_last, lr_a, lr_b = (_f4(a) for a in (hprev, gates, w_hh, dh_ext, dh_last, lr_a, lr_b))
    T, M, H = hprev.shape
    w = _rnd(w_hh, bf16)
    dgi, dgh = np.zeros((T, M, 3 * H), F4), np.zeros((T, M, 3 * H), F4)
    av, dhz = np.zeros((M, H), F4), np.zeros((M, H), F4)
    for s in range(T - 1, -1, -1):
        r, z, n, hn = gates[s]
        dh = (av + dhz).astype(F4)
        if dh_ext is not None:
            dh = dh + dh_ext[s]
        if dh_last is not None and s == T - 1:
            dh = dh + dh_last
        if lr_a is not None:
            for k in range(lr_b.shape[0]):
                dh = dh + lr_a[s][:, k:k + 1] * lr_b[k][None, :]
        dn = dh * (F4(1) - z) * (F4(1) - n * n)
        dz = dh * (hprev[s] - n) * z * (F4(1) - z)
        dr = dn * hn * r * (F4(1) - r)
        dgi[time_of(s, T, reverse)] = _rnd(np.concatenate([dr, dz, dn], axis=1), dg_bf16)
        dgh[s] = _rnd(np.concatenate([dr, dz, dn * r], axis=1), dg_bf16)
        dhz = (dh * z).astype(F4)
        av = (_rnd(dgh[s], bf16) @ w).astype(F4)
    return dgi, dgh, (av + dhz).astype(F4), dhz


# ================================================================================================ host mirrors of the dispatch
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, 'polyphonic_chord_texture_disentanglement_amd', 'csrc')
_GRU = open(os.path.join(_CSRC, 'gru.hip')).read()
_CORE = open(os.path.join(_CSRC, 'gemm_core.hpp')).read()


def _ints(pattern, text):
    m = re.search(pattern, text, re.S)
    assert m, 'csrc no longer holds %r: plan_fwd / plan_bwd must be edited together with the dispatch' % pattern
    return [int(g) for g in m.groups()]


BK = {'bf16': _ints(r'struct BF16 \{.*?int BK = (\d+)', _CORE)[0], 'fp32': _ints(r'struct F32 \{.*?int BK = (\d+)', _CORE)[0]}
assert 'kbeg + 2 * PF * CT::BK <= kend' in _CORE and 'if (fullA && fullB && kbeg' in _CORE
FWD_BIG_BLOCKS, = _ints(r'launch_fwd_step\(.*?cdiv\(g\.M, 64\) \* cdiv\(g\.N, 64\);\s*if \(blocks_big >= (\d+)\) \{', _GRU)
BWD_BIG_BLOCKS, BWD_BIG_MIN_N, BWD_MID_BLOCKS = _ints(
    r'launch_bwd_step\(.*?if \(blocks_big >= (\d+) && g\.N > (\d+)\) \{.*?else if \(blocks_mid >= (\d+)\) \{', _GRU)
_pf = _ints(r'EpiGruFwdT<MODE>, SA, SB, \(BM \* BJ <= 64 \* 32 \? (\d+) : (\d+)\)>', _GRU)
PF_FWD = {'64x32': _pf[0], '64x64': _pf[1]}
_pf = _ints(r'EpiGruBwdT<FAST>, SA, SB, \(BM \* BN <= 64 \* 32 \? (\d+) : \(BM \* BN <= 64 \* 64 \? (\d+) : (\d+)\)\)>', _GRU)
PF_BWD = {'64x32': _pf[0], '64x64': _pf[1], '128x128': _pf[2]}
# the lines plan_* copy by hand: when one of them changes the import fails here
for _line in (
        'const bool fast = a16 && w16 && ep.hout16 && (ep.flags & PTV_GRU_GI_BF16) && (!ep.gates || (ep.flags & PTV_GRU_GATES_BF16)) &&',
        '(!ep.gi2 || (ep.flags & PTV_GRU_GI2_BF16)) && !ep.gi_idx && g.M >= 1 && ep.H >= 4;',
        'if (fast && ep.gi2) launch_fwd_step<BF16, true, true, 2>(g, ep, s);',
        'else if (fast) launch_fwd_step<BF16, true, true, 1>(g, ep, s);',
        'else if (a16 && w16) launch_fwd_step<BF16, true, true, 0>(g, ep, s);',
        'else if (a16) launch_fwd_step<BF16, true, false, 0>(g, ep, s);',
        'else launch_fwd_step<BF16, false, false, 0>(g, ep, s);',
        '} else launch_fwd_step<F32, false, false, 0>(g, ep, s);',
        'const bool fast = dbf && w16 && (flags & PTV_GRU_GATES_BF16) && (!lr_a || lr_k <= 2);',
        'if (fast) launch_bwd_step<BF16, true, true, true>(g, ep, s);',
        'else if (dbf && w16) launch_bwd_step<BF16, true, true, false>(g, ep, s);',
        'else if (dbf) launch_bwd_step<BF16, true, false, false>(g, ep, s);',
        'else launch_bwd_step<BF16, false, false, false>(g, ep, s);',
        '} else launch_bwd_step<F32, false, false, false>(g, ep, s);',
        'const long blocks_big = (long)cdiv(g.M, 128) * cdiv(g.N, 128);',
        'const long blocks_mid = (long)cdiv(g.M, 64) * cdiv(g.N, 64);'):
    assert _line in _GRU, 'csrc/gru.hip no longer holds %r' % _line

FWD_VARIANTS = ('F32', 'B0', 'B-a', 'B-aw', 'FAST1', 'FAST2')
BWD_VARIANTS = ('F32', 'B0', 'B-d', 'B-dw', 'FAST')
FWD_TILES = ('64x32', '64x64')
BWD_TILES = ('64x32', '64x64', '128x128')


def cdiv(a, b):
    return -(-a // b)


def plan_fwd(M, H, cfg):
    """launch_fwd_any + launch_fwd_step.  cfg: prec 'fp32' / 'bf16'; hall16, w16, gi_idx: bool; gi: 'f' / 'b'; gates: None / 'f' / 'b';
    gi2: None / 'f' / 'b'; hout16 (ptv_gru_step_fwd: its own pointer; default = hall16) -> (variant, tile)"""
    a16, w16 = bool(cfg.get('hall16')), bool(cfg.get('w16'))
    fast = (a16 and w16 and bool(cfg.get('hout16', a16)) and cfg.get('gi', 'f') == 'b' and cfg.get('gates') in (None, 'b') and cfg.get('gi2') in (None, 'b')
            and not cfg.get('gi_idx') and M >= 1 and H >= 4)
    if cfg['prec'] == 'bf16':
        variant = ('FAST2' if cfg.get('gi2') else 'FAST1') if fast else 'B-aw' if a16 and w16 else 'B-a' if a16 else 'B0'
    else:
        variant = 'F32'
    return variant, '64x64' if cdiv(M, 64) * cdiv(H, 64) >= FWD_BIG_BLOCKS else '64x32'


def plan_bwd(M, H, cfg):
    """the `fast` expression of ptv_gru_seq_bwd + launch_bwd_step.  cfg: prec; dg16, w16, gates16: bool; lr_k: 0 = no low-rank addend"""
    dbf, w16 = bool(cfg.get('dg16')), bool(cfg.get('w16'))
    fast = dbf and w16 and bool(cfg.get('gates16')) and cfg.get('lr_k', 0) <= 2
    if cfg['prec'] == 'bf16':
        variant = 'FAST' if fast else 'B-dw' if dbf and w16 else 'B-d' if dbf else 'B0'
    else:
        variant = 'F32'
    if cdiv(M, 128) * cdiv(H, 128) >= BWD_BIG_BLOCKS and H > BWD_BIG_MIN_N:
        return variant, '128x128'
    return variant, '64x64' if cdiv(M, 64) * cdiv(H, 64) >= BWD_MID_BLOCKS else '64x32'


def handover(direction, tile, prec):
    """the K from which a full tile runs the branch-free pipeline of gemm_body: 2 * PF * BK"""
    return 2 * (PF_FWD if direction == 'fwd' else PF_BWD)[tile] * BK[prec]


def handover_H(direction, tile, prec):
    """(largest H below, smallest H at) the hand-over of the 64x32 tile, H a multiple of 8 (bf16) or 4 (fp32), and one more above:
    K = H forward, K = 3H backward"""
    step = 8 if prec == 'bf16' else 4
    k = handover(direction, tile, prec)
    per = 1 if direction == 'fwd' else 3
    at = cdiv(cdiv(k, per), step) * step
    return at - step, at, at + step
