"""Plain fp64 references (numpy, CPU), host mirrors and the case tables of the persistent, weight-stationary GRUs of csrc/gru_persist.hip --
pgru_fwd_kernel, pgru_bwd_kernel and the split-K team pgru_bwd_sk_kernel behind ptv_gru_persist_{fwd,bwd,bwd_splitk}: the oracle side of
tests/test_gpu_pgru_kernels.py, itself held to torch's float64 nn.GRU and autograd by tests/test_pgru_ref_host.py.

A thin layer over tests/gru_ref.py: the cell (gru_forward / gru_backward) and its kernel-precision evaluation (kp_forward / kp_backward)
are that file's.  The persistent configuration is bf16=True (the state operand -- at step 0 bf16(h0) --, the dgh operand and W rounded
to bf16), gates_bf16=True, dg_bf16=True.  This file adds
  * blocked / unblocked: one slot of the exchange tensor `xch`, [k/8][row][8] (include/ptvae_hip.h; K = H forward, 3H backward);
  * plan / splitk_ok / ku_plain / ku_splitk / block_map_branch / empty_groups / part_elems: the host dispatch of gru_persist.hip as a
    function of the CU count the grids are sized from (the device's minus ptv_gru_persist_cu_reserve), from constants parsed out of the
    source; the lines copied by hand are asserted present at import;
  * CASES, the case table of the GPU test (here so that the host test can assert what it reaches), and the input generators."""
import os
import re
import zlib

import numpy as np

import gru_ref as G
from gemm_ref import bf16_round, from_blocked, to_blocked

F8, F4 = np.float64, np.float32


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ the exchange layout
def blocked(a):
    """[M, K] -> one xch slot [K/8][M][8]: element (row, k) at ((k / 8) * M + row) * 8 + k % 8"""
    return to_blocked(np.asarray(a), 8)


def unblocked(x, M, K):
    return from_blocked(np.asarray(x).reshape(K // 8, M, 8), 8)


# ================================================================================================ the cell, in the persistent configuration
def forward(gi, gi2, w_hh, b_hh, h0, lengths, reverse):
    """gi [T, M, 3H] by time, gi2 [T or 1, M, 3H] or None -> states [T + 1, M, H] (slot 0 = h0), gates [T, 4, M, H] by step; float64"""
    gi2 = None if gi2 is None else np.broadcast_to(gi2, gi.shape)
    hs, gates = G.gru_forward(gi, gi2, w_hh, b_hh, h0, lengths, reverse, None)
    return np.concatenate([np.asarray(h0, F8)[None], hs]), gates


def kp_forward(gi, gi2, w_hh, b_hh, h0, lengths, reverse):
    """the same at the kernels' precision -> states fp32, gates (bf16 values), states16 (bf16 values)"""
    gi2 = None if gi2 is None else np.broadcast_to(gi2, gi.shape)
    hs, gates, _ = G.kp_forward(gi, gi2, w_hh, b_hh, h0, lengths, reverse, None, bf16=True, gates_bf16=True)
    st = np.concatenate([np.asarray(h0, F4)[None], hs])
    return st, gates, bf16_round(st)


def backward(hprev, gates, w_hh, ext, last, reverse):
    """hprev [T, M, H] the stored states 0 .. T-1, gates [T, 4, M, H] as stored, ext [T, M, H] by step or None, last [M, H] or None ->
    dgi [T, M, 3H] by TIME, dgh [T, M, 3H] by step, dh0 [M, H]; float64"""
    return G.gru_backward(hprev, gates, w_hh, ext, last, None, None, reverse)[:3]


def kp_backward(hprev, gates, w_hh, ext, last, reverse):
    return G.kp_backward(hprev, gates, w_hh, ext, last, None, None, reverse, bf16=True, dg_bf16=True)[:3]


# ================================================================================================ host mirrors of the dispatch
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(_ROOT, 'polyphonic_chord_texture_disentanglement_amd', 'csrc', 'gru_persist.hip')).read()


def _ints(pattern):
    m = re.search(pattern, _SRC, re.S)
    assert m, 'csrc/gru_persist.hip no longer holds %r: tests/pgru_ref.py must be edited together with the dispatch' % pattern
    return [int(g) for g in m.groups()]


PU, = _ints(r'constexpr int PU = (\d+);')
PMAXC, = _ints(r'constexpr int PMAXC = (\d+);')
PMAXG, = _ints(r'constexpr int PMAXG = (\d+);')
PMAXT, = _ints(r'constexpr int PMAXT = (\d+);')
H_MIN, H_MAX, H_MASK = _ints(r'static int plan\(.*?H < (\d+) \|\| H > (\d+) \|\| \(H & (\d+)\)\) return PTV_ERR_UNSUPPORTED;')
PANEL, RG_ROWS_MAX = _ints(r'while \(rg > 1 && \(M \+ rg - 1\) / rg < (\d+) && \(M \+ rg / 2 - 1\) / \(rg / 2\) <= (\d+)\) rg /= 2;')
FM_MAX_PLAIN, = _ints(r'int& FM, int fm_max = (\d+)\)')
FM_MAX_SK, = _ints(r'PTV_TRY\(plan\(NC, M, H, RG, rows_wg, FM, (\d+)\)\);')
K8_MOD, = _ints(r'const bool k8 = \(\(KK\) % (\d+)\) == 0;')
SK_MOD, = _ints(r'\(3 \* H / S\) % (\d+) == 0;')
SYNC_WORDS = 16 * (1 + PMAXG + PMAXT)
# the lines the mirrors copy by hand: when one of them changes the import fails here
for _line in (
        'if (NC < 1 || NC > PMAXC || M <= 0 ||',
        'const int ncu = num_cu() - g_cu_reserve;',
        'int rg = ncu / (NC * UG);',
        'if (rg < 1) return PTV_ERR_UNSUPPORTED;',
        'int p2 = 1; while (p2 * 2 <= rg) p2 *= 2;',
        'int fm = ((M + rg - 1) / rg + 63) / 64;',
        'if (fm == 3) fm = 4;',
        'if (fm > 4 && fm <= 8) fm = 8;',
        'if (fm > fm_max) return PTV_ERR_UNSUPPORTED;',
        'if (NC * rg > PMAXG) return PTV_ERR_UNSUPPORTED;',
        'RG = rg; rows_wg = fm * 64; FM = fm;',
        'static bool splitk_ok(int H, int S) { return (S == 2 || S == 4) && (H / PU) % S == 0 &&',
        'if (NC * RG * (H / PU / S) > PMAXT) return PTV_ERR_UNSUPPORTED;',
        'if (FM == 1) { if (k8) hipLaunchKernelGGL((K<1, 8, LP_>), grid, block, 0, s, a); else hipLaunchKernelGGL((K<1, 4, LP_>), grid, block, 0, s, a); }',
        'else if (FM == 2) hipLaunchKernelGGL((K<2, 4, LP_>), grid, block, 0, s, a);',
        'else hipLaunchKernelGGL((K<4, 2, LP_>), grid, block, 0, s, a);',
        'if (g_load_policy == 0) PTV_PG_LAUNCH(pgru_fwd_kernel, 0, H);',
        'if (g_load_policy == 0) PTV_PG_LAUNCH(pgru_bwd_kernel, 0, 3 * H);',
        'if (FM == 1) hipLaunchKernelGGL((pgru_bwd_sk_kernel<1, 3, S_>), grid, block, 0, s, a);',
        'else if (FM == 2) hipLaunchKernelGGL((pgru_bwd_sk_kernel<2, 3, S_>), grid, block, 0, s, a);',
        'else if (FM == 4) hipLaunchKernelGGL((pgru_bwd_sk_kernel<4, 3, S_>), grid, block, 0, s, a);',
        'else hipLaunchKernelGGL((pgru_bwd_sk_kernel<8, 1, S_>), grid, block, 0, s, a);',
        'if (G <= 8 && (8 % G) == 0 && (nW & 7) == 0) {',
        'block_map(a.NC * a.RG, a.UG, grp, ug);',
        'block_map(a.NC * a.RG, a.UG, grp, idx);',
        'const int row0 = rg * a.rows_wg + wave * (FM * 16);',
        'return 2L * RG * rows * H * S;'):
    assert _line in _SRC, 'csrc/gru_persist.hip no longer holds %r' % _line

PLAIN_INSTANCES = ((1, 8), (1, 4), (2, 4), (4, 2))                      # (FM, KU) of pgru_fwd_kernel / pgru_bwd_kernel
SK_INSTANCES = tuple((fm, s) for fm in (1, 2, 4, 8) for s in (2, 4))   # (FM, S) of pgru_bwd_sk_kernel


def plan(ncu, NC, M, H, fm_max=FM_MAX_PLAIN):
    """plan() of gru_persist.hip for grids sized from `ncu` CUs -> dict(RG, rows, FM) or None (PTV_ERR_UNSUPPORTED)"""
    if NC < 1 or NC > PMAXC or M <= 0 or H < H_MIN or H > H_MAX or (H & H_MASK):
        return None
    UG = H // PU
    rg = ncu // (NC * UG)
    if rg < 1:
        return None
    p2 = 1
    while p2 * 2 <= rg:
        p2 *= 2
    rg = p2
    while rg > 1 and cdiv(M, rg) < PANEL and cdiv(M, rg // 2) <= RG_ROWS_MAX:
        rg //= 2
    fm = cdiv(cdiv(M, rg), 64)
    if fm == 3:
        fm = 4
    if 4 < fm <= 8:
        fm = 8
    if fm > fm_max or NC * rg > PMAXG:
        return None
    return dict(RG=rg, rows=fm * 64, FM=fm)


def splitk_ok(H, S):
    return S in (2, 4) and (H // PU) % S == 0 and (3 * H // S) % SK_MOD == 0


def plan_splitk(ncu, NC, M, H, S):
    if not splitk_ok(H, S):
        return None
    p = plan(ncu, NC, M, H, FM_MAX_SK)
    if p is None or NC * p['RG'] * (H // PU // S) > PMAXT:
        return None
    return p


def part_elems(ncu, NC, M, H, S):
    p = plan_splitk(ncu, NC, M, H, S)
    return 0 if p is None else 2 * p['RG'] * p['rows'] * H * S


def ku_plain(FM, K):
    """PTV_PG_LAUNCH: K = H forward, 3H backward"""
    return {1: 8 if K % K8_MOD == 0 else 4, 2: 4, 4: 2}[FM]


def ku_splitk(FM):
    return 1 if FM == 8 else 3


def block_map_branch(NC, RG, H):
    G, nW = NC * RG, NC * RG * (H // PU)
    return 'xcd' if G <= 8 and 8 % G == 0 and nW % 8 == 0 else 'plain'


def empty_groups(p, M):
    """row groups of one chain none of whose rows exists"""
    return sum(1 for g in range(p['RG']) if g * p['rows'] >= M)


def reached(ncu, case):
    """what a case runs on a device whose grids are sized from ncu - reserve CUs -> dict of instantiation names, or absent keys"""
    n = ncu - case['reserve']
    NC, M, H = case['NC'], case['M'], case['H']
    out = {}
    p = plan(n, NC, M, H)
    if p is not None:
        out['plain'] = p
        out['fwd'] = (p['FM'], ku_plain(p['FM'], H))
        out['bwd'] = (p['FM'], ku_plain(p['FM'], 3 * H))
    for S in (2, 4):
        q = plan_splitk(n, NC, M, H, S)
        if q is not None:
            out['S%d' % S] = q
    return out


# ================================================================================================ the case table
def _case(M, H, T, NC=1, reserve=0, lengths=False, gi2=None, gi_pad=False, no_gates=False, ext='f', ext_pad=False, last='dense', dh0='all'):
    assert gi2 in (None, 'bcast', 'step') and ext in (None, 'f', 'b') and last in (None, 'dense', 'pad') and dh0 in ('all', 'none', 'mixed')
    return dict(M=M, H=H, T=T, NC=NC, reserve=reserve, lengths=lengths, gi2=gi2, gi_pad=gi_pad, no_gates=no_gates, ext=ext, ext_pad=ext_pad,
                last=last, dh0=dh0)


# The smallest shapes that reach each variant at 256 CUs (tests/test_pgru_ref_host.py asserts which).  Options vary across the table.
CASES = [
    # FM = 1, KU = 4 (H = 256: K = 256 forward, 768 backward, neither a multiple of 512)
    _case(1, 256, 1, dh0='all', ext=None),
    _case(40, 256, 2, lengths=True, gi2='bcast', ext='b', dh0='none'),
    _case(64, 256, 5, gi_pad=True, ext_pad=True, last='pad'),
    _case(40, 256, 32, lengths=True, last=None),
    # FM = 1, KU = 8
    _case(48, 512, 5, NC=2, gi2='step', dh0='mixed', no_gates=True),
    # FM = 1, RG = 16: the plain block_map branch
    _case(1024, 256, 2, lengths=True, ext='b', ext_pad=True),
    # FM = 2
    _case(100, 256, 5, lengths=True, gi2='step', last='pad'),
    _case(96, 768, 2, gi_pad=True, ext=None),
    _case(72, 1024, 2, gi2='bcast', dh0='none'),
    # FM = 2, RG = 2, the last group ragged
    _case(130, 256, 5, lengths=True, ext='b'),
    # FM = 2, empty row groups
    _case(257, 256, 2, lengths=True, no_gates=True),
    _case(520, 256, 1, last='pad', dh0='all'),
    # NC = 3: the plain block_map branch
    _case(40, 256, 5, NC=3, lengths=True, dh0='mixed', gi2='bcast'),
    _case(70, 256, 2, NC=3, dh0='mixed', ext='b', last=None),
    _case(300, 256, 2, NC=3, lengths=True, dh0='mixed', ext_pad=True),
    # NC = 4
    _case(33, 256, 5, NC=4, lengths=True, dh0='mixed', gi_pad=True),
    # FM = 4 (16 CUs left)
    _case(130, 256, 2, reserve=240, lengths=True, gi2='step'),
    _case(200, 256, 5, reserve=240, dh0='none', ext='b', last='pad'),
    # FM = 8: the split-K kernel only; the plain forward and BPTT refuse
    _case(300, 256, 2, reserve=240, lengths=True),
    _case(300, 256, 5, NC=2, reserve=224, dh0='mixed', ext=None),
]
# both parities of the two-slot partial ring are reused from T = 6 on: one more T on the split-K side of four shapes
SK_T6 = [_case(40, 256, 6, lengths=True), _case(130, 256, 6, ext='b', dh0='none'), _case(200, 256, 6, reserve=240, last='pad'),
         _case(300, 256, 6, reserve=240, dh0='all', gi2='bcast')]
ALL_CASES = CASES + SK_T6
# load policies 0 / 1 / 2 give identical bits: one FM = 1 case, one RG > 1 case, one NC = 3 case (indices into CASES)
POLICY_CASES = (2, 9, 12)
# one chain alone and as chain 0 of an NC = 3 launch; reserve 0 against reserve 240 (another FM / RG for the same rows)
ALONE_VS_NC3 = (_case(40, 256, 5, lengths=True, gi2='bcast'), CASES[12])
RESERVE_PAIR = (_case(130, 256, 5, lengths=True, ext='b'), _case(130, 256, 5, reserve=240, lengths=True, ext='b'))


def case_id(c):
    head = 'NC%d M%d H%d T%d' % (c['NC'], c['M'], c['H'], c['T'])
    return head + ''.join(' %s' % k if v is True else ' %s=%s' % (k, v) for k, v in sorted(c.items())
                          if k not in ('NC', 'M', 'H', 'T') and v not in (False, None, 0))


def key_of(c):
    return tuple(sorted(c.items()))


def lengths_of(M, T, rows_wg, RG, chain):
    """0 .. T + 2 in turn (0, T and values above T are all there from M = T + 3 on), rotated per chain; with more than one row group
    every row of group 1 is dead"""
    ln = ((T + 2 - np.arange(M) - chain) % (T + 3)).astype(np.int32)
    if RG > 1:
        ln[rows_wg:2 * rows_wg] = 0
    return ln


def chain_inputs(c, ch, with_dh0=None):
    """seeded inputs of chain `ch` of a case (the data of a chain depend on (M, H, T, its index and the options), not on NC or the plan,
    except the dead row group of `lengths`, placed from the plan at 256 CUs)"""
    M, H, T = c['M'], c['H'], c['T']
    seed = zlib.crc32(repr((M, H, T, ch, c['lengths'], c['gi2'], c['ext'], c['last'])).encode()) & 0x7FFFFFFF
    rng = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(H)
    w = bf16_round(rng.uniform(-k, k, (3 * H, H)))
    b = rng.uniform(-k, k, 3 * H).astype(F4)
    gi = bf16_round(rng.normal(0, 1, (T, M, 3 * H)))
    gi2 = None if c['gi2'] is None else bf16_round(rng.normal(0, 0.5, (1 if c['gi2'] == 'bcast' else T, M, 3 * H)))
    h0 = rng.normal(0, 0.5, (M, H)).astype(F4)
    if T == 1:
        h0 = bf16_round(h0)                                                  # the product is exact: the check is sharp
    ext = None if c['ext'] is None else rng.normal(0, 1, (T, M, H)).astype(F4)
    if c['ext'] == 'b':
        ext = bf16_round(ext)
    last = None if c['last'] is None else rng.normal(0, 1, (M, H)).astype(F4)
    lengths = None
    if c['lengths']:
        p = plan(256 - c['reserve'], c['NC'], M, H, FM_MAX_SK)
        lengths = lengths_of(M, T, p['rows'], p['RG'], ch)
    has_dh0 = {'all': True, 'none': False, 'mixed': ch % 2 == 0}[c['dh0']] if with_dh0 is None else with_dh0
    return dict(w=w, b=b, gi=gi, gi2=gi2, h0=h0, ext=ext, last=last, lengths=lengths, reverse=ch % 2 == 1, has_dh0=has_dh0)


def chain_reference(ins):
    """fp64 reference and kernel-precision evaluation of one chain.  The BPTT runs on the REFERENCE's states and gates rounded to their
    storage types (fp32 / bf16), never on a kernel's output"""
    a = (ins['gi'], ins['gi2'], ins['w'], ins['b'], ins['h0'], ins['lengths'], ins['reverse'])
    st, gates = forward(*a)
    kst, kgates, kst16 = kp_forward(*a)
    hall_in = st.astype(F4)
    gates_in = bf16_round(gates.astype(F4))
    bw = (hall_in[:-1], gates_in, ins['w'], ins['ext'], ins['last'], ins['reverse'])
    return dict(st=st, gates=gates, kst=kst, kgates=kgates, kst16=kst16, hall_in=hall_in, gates_in=gates_in, bwd=backward(*bw),
                kbwd=kp_backward(*bw))
