"""The persistent, weight-stationary GRUs of csrc/gru_persist.hip one launch at a time -- pgru_fwd_kernel, pgru_bwd_kernel and the split-K
team pgru_bwd_sk_kernel, every instantiation -- against the plain fp64 references of tests/pgru_ref.py, through the C ABI as it is
declared: ptv_gru_persist_fwd / _bwd / _bwd_splitk with host pointer and stride arrays built here, _supported / _splitk_supported /
_part_elems, _load_policy and _cu_reserve.

Launch discipline: every launch is on the current stream with freshly zeroed sync words and torch.cuda.synchronize() before and after
it, so no two persistent launches are ever in flight; word 0 of `sync` (a bounded spin gave up) is asserted zero after every launch.
The process-wide load policy and CU reserve are set inside try / finally that restores 0 and 0 (the reserve through functional.py's
wrapper, which also clears its cached support answers).  The timing hook load_policy >= 100 is never touched.

Inputs are built on the CPU from seeded generators (pgru_ref.chain_inputs): W_hh, gi, gi2 and bf16 dh_ext are bf16-representable; the
BPTT gets the REFERENCE's states and gates rounded to their storage types, never a kernel's forward output; with T = 1 h0 is
bf16-representable too, so the product is exact.  Chains of one launch differ in weights, direction (odd chains reversed) and in
whether they get dh0.  Every output is pre-filled with a sentinel and carries pad rows (a pad tail after xch and part) that must keep
it; inputs are compared byte for byte after the call and hall slot 0 stays as written.

Floating-point outputs have no pre-chosen tolerance: bound_of of test_gpu_dur_kernels.py -- the kernel error may be at most 4x the
error of the kernel-precision CPU evaluation (gru_ref.kp_*) against fp64, floor 8 fp32 ulps of the plane's scale -- taken per step
plane; the bound never sees the kernel's output.  Each check prints `PGRU_RATIO family ratio`, the module `PGRU_RATIO_MAX family`
(pytest -s; table in profiles/LOG.md).  S = 2, S = 4 and the plain BPTT differ in summation order: each is held to the reference, never
to another.  Bit for bit: hall16 = RNE(hall), slot 0 = RNE(h0); a dead row copies its state, saves gates (0, 1, 0), has zero gate
gradients and passes dh on; the r / z planes of dgi (by time) and dgh (by step) are the same bits; xch = blocked(hall16[s]) after the
forward and blocked(dgh[step]) after the BPTT; load policies 0 / 1 / 2; one chain alone and inside an NC = 3 launch, and with reserve 0
and 240 (another FM and RG); a split-K launch issued twice.

tests/test_pgru_ref_host.py asserts, without a GPU, what the case table reaches at 256 CUs.  On a device with another CU count the plan
differs: a case the device's plan refuses asserts the refusal and skips."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import pgru_ref as P
from gru_ref import time_of
from test_gpu_dur_kernels import bound_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = np.float32(np.nan)
SENT = 768.0                                                           # (exact in bf16)
BF = torch.bfloat16
RATIOS = {}
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
PAD = 64                                                               # elements behind xch and part


def L():
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    return lib()


def stream():
    from polyphonic_chord_texture_disentanglement_amd._lib import stream_ptr
    return stream_ptr()


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def bits(t):
    """a device tensor's bits on the host"""
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu().numpy().copy()


def val(t):
    return t.float().cpu().numpy()


def filled(shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def is_sent(t):
    return bool((t == SENT).all().item())


def parr(xs):
    """host array of device pointers: tensors, None (NULL) or raw addresses"""
    return (ctypes.c_void_p * len(xs))(*[x.data_ptr() if isinstance(x, torch.Tensor) else x for x in xs])


def larr(vs):
    return (ctypes.c_long * len(vs))(*[int(v) for v in vs])


def iarr(vs):
    return (ctypes.c_int * len(vs))(*[int(v) for v in vs])


def check(family, got, ref, kp):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return
    bound, errk = bound_of(ref, kp)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), '%s: non-finite output' % family
    ratio = float(np.where(err == 0, 0.0, err / bound).max())
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print('PGRU_RATIO %s %.3f (kernel err %.3e, kernel-precision CPU err %.3e)' % (family, ratio, err.max(), errk))
    at = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), '%s: kernel error %.3e over the bound %.3e at %s (kernel-precision CPU evaluation: %.3e)' % (
        family, err[at], float(np.min(bound)), at, errk)


def check_planes(family, got, ref, kp):
    for s in range(got.shape[0]):
        check(family, got[s], ref[s], kp[s])


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('PGRU_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


@contextlib.contextmanager
def cu_reserve(n):
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    try:
        F_.set_persist_cu_reserve(n)
        yield
    finally:
        F_.set_persist_cu_reserve(0)


@contextlib.contextmanager
def load_policy(lp):
    assert 0 <= lp <= 2                                                 # (>= 100 is the timing hook: results invalid)
    try:
        assert L().ptv_gru_persist_load_policy(lp) == OK
        yield
    finally:
        assert L().ptv_gru_persist_load_policy(0) == OK


def launch(name, args, sync):
    """one persistent launch, alone on the device -> status code; the error word of `sync` must stay zero"""
    torch.cuda.synchronize()
    rc = getattr(L(), name)(*args, sync if isinstance(sync, int) or sync is None else sync.data_ptr(), stream())
    torch.cuda.synchronize()
    if isinstance(sync, torch.Tensor):
        assert int(sync[0].item()) == 0, '%s: a bounded spin gave up (error word of sync)' % name
    return rc


def new_sync():
    return torch.zeros(P.SYNC_WORDS, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=64)
def _reference(key, ch):
    ins = P.chain_inputs(dict(key), ch)
    return ins, P.chain_reference(ins)


def chains_of(c):
    """[(inputs, reference)] of the case's chains (read only, shared between the tests)"""
    return [_reference(P.key_of(c), ch) for ch in range(c['NC'])]


# ================================================================================================ forward
FWD_ARGS = ('NC', 'M', 'H', 'T', 'gi', 'gi_step', 'gi_ld', 'gi2', 'gi2_step', 'gi2_ld', 'w', 'b', 'hall', 'hall16', 'gates', 'lengths',
            'reverse', 'xch')
FWD_INPUTS = ('gi', 'gi2', 'w', 'b', 'lengths')
FWD_OUTPUTS = ('hall16', 'gates', 'xch')


def fwd_setup(c, chains):
    M, H, T = c['M'], c['H'], c['T']
    gi_ld, gi_rows = (3 * H + 8, M + 2) if c['gi_pad'] else (3 * H, M)
    t = {k: [] for k in FWD_INPUTS + FWD_OUTPUTS + ('hall',)}
    for ins, _ in chains:
        g = np.full((T, gi_rows, gi_ld), NAN, np.float32)
        g[:, :M, :3 * H] = ins['gi']
        t['gi'].append(dev(g, BF))
        t['gi2'].append(dev(ins['gi2'], BF))
        t['w'].append(dev(ins['w'], BF))
        t['b'].append(dev(ins['b']))
        t['lengths'].append(dev(ins['lengths']))
        hall = filled(((T + 1) * M + 2, H))
        hall[:M] = dev(ins['h0'])
        t['hall'].append(hall)
        t['hall16'].append(filled(((T + 1) * M + 2, H), BF))
        t['gates'].append(None if c['no_gates'] else filled((T * 4 * M + 2, H), BF))
        t['xch'].append(filled(((T + 1) * M * H + PAD,), BF))
    NC = len(chains)
    a = dict(NC=NC, M=M, H=H, T=T, gi=parr(t['gi']), gi_step=larr([gi_rows * gi_ld] * NC), gi_ld=larr([gi_ld] * NC),
             gi2=None if c['gi2'] is None else parr(t['gi2']), gi2_step=larr([0 if c['gi2'] != 'step' else M * 3 * H] * NC),
             gi2_ld=larr([3 * H] * NC), w=parr(t['w']), b=parr(t['b']), hall=parr(t['hall']), hall16=parr(t['hall16']),
             gates=None if c['no_gates'] else parr(t['gates']), lengths=None if not c['lengths'] else parr(t['lengths']),
             reverse=iarr([ins['reverse'] for ins, _ in chains]), xch=parr(t['xch']))
    return a, t


def untouched_fwd(c, t, chains):
    """nothing was written: every output holds the sentinel, hall holds h0 and the sentinel"""
    M = c['M']
    for i, (ins, _) in enumerate(chains):
        assert all(is_sent(t[k][i]) for k in FWD_OUTPUTS if t[k][i] is not None)
        assert is_sent(t['hall'][i][M:]) and np.array_equal(bits(t['hall'][i][:M]), ins['h0'].view(np.int32))


def run_fwd(c, chains, reserve=None):
    """-> per chain dict of host arrays (bits) after the checks every launch gets, or None when the device's plan refuses the shape"""
    M, H, T = c['M'], c['H'], c['T']
    reserve = c['reserve'] if reserve is None else reserve
    a, t = fwd_setup(c, chains)
    before = {k: [None if x is None else bits(x) for x in t[k]] for k in FWD_INPUTS}
    sync = new_sync()
    with cu_reserve(reserve):
        plan = P.plan(ncu() - reserve, len(chains), M, H)
        assert L().ptv_gru_persist_supported(len(chains), M, H) == int(plan is not None)
        rc = launch('ptv_gru_persist_fwd', [a[k] for k in FWD_ARGS], sync)
    if plan is None:
        assert rc == ERR_UNSUPPORTED and not sync.any().item()
        untouched_fwd(c, t, chains)
        return None
    assert rc == OK
    out = []
    for i, (ins, _) in enumerate(chains):
        for k in FWD_INPUTS:
            assert before[k][i] is None or np.array_equal(before[k][i], bits(t[k][i])), 'input %s was written' % k
        n = (T + 1) * M
        assert is_sent(t['hall'][i][n:]) and is_sent(t['hall16'][i][n:]) and is_sent(t['xch'][i][n * H:]), 'pad rows written'
        assert t['gates'][i] is None or is_sent(t['gates'][i][T * 4 * M:])
        hall = t['hall'][i][:n].view(T + 1, M, H)
        assert np.array_equal(bits(hall[0]), ins['h0'].view(np.int32)), 'hall slot 0 was written'
        out.append(dict(hall=hall.cpu().numpy(), hall16_bits=bits(t['hall16'][i][:n]).reshape(T + 1, M, H),
                        hall16=val(t['hall16'][i][:n]).reshape(T + 1, M, H), rne=bits(hall.to(BF)),
                        gates=None if t['gates'][i] is None else val(t['gates'][i][:T * 4 * M]).reshape(T, 4, M, H),
                        xch=bits(t['xch'][i][:n * H]).reshape(T + 1, H // 8, M, 8)))
    return out


def verify_fwd(c, out, chains):
    M, H, T = c['M'], c['H'], c['T']
    for o, (ins, ref) in zip(out, chains):
        check_planes('fwd h', o['hall'][1:], ref['st'][1:], ref['kst'][1:])
        check_planes('fwd h16', o['hall16'][1:], ref['st'][1:], ref['kst16'][1:])
        assert np.array_equal(o['hall16_bits'], o['rne']), 'hall16 is not the RNE rounding of hall (slot 0: of h0)'
        for s in range(T + 1):
            assert np.array_equal(o['xch'][s], P.blocked(o['hall16_bits'][s])), 'xch slot %d is not blocked(hall16[%d])' % (s, s)
        if o['gates'] is not None:
            for g, name in enumerate('rzn'):
                check_planes('fwd gate ' + name, o['gates'][:, g], ref['gates'][:, g], ref['kgates'][:, g])
            check_planes('fwd gate hn', o['gates'][:, 3], ref['gates'][:, 3], ref['kgates'][:, 3])
        if ins['lengths'] is not None:
            for s in range(T):
                dead = time_of(s, T, ins['reverse']) >= ins['lengths']
                assert np.array_equal(o['hall'][s + 1][dead].view(np.int32), o['hall'][s][dead].view(np.int32)), 'a dead row moved'
                if o['gates'] is not None:
                    g = o['gates'][s][:, dead]
                    assert (g[0] == 0).all() and (g[1] == 1).all() and (g[2] == 0).all(), 'a dead row saves gates other than (0, 1, 0)'


@pytest.mark.parametrize('c', P.CASES, ids=P.case_id)
def test_forward(c):
    chains = chains_of(c)
    out = run_fwd(c, chains)
    if out is None:
        if P.plan(256 - c['reserve'], c['NC'], c['M'], c['H']) is None:
            return                                                      # FM = 8: the plain forward refuses, as asserted
        pytest.skip('the plan of this device (%d CUs) refuses the shape' % ncu())
    verify_fwd(c, out, chains)


# ================================================================================================ BPTT
BWD_ARGS = ('NC', 'M', 'H', 'T', 'hall', 'gates', 'w_t', 'ext', 'ext_step', 'ext_ld', 'ext_bf16', 'last', 'last_ld', 'dgi', 'dgh', 'dh0',
            'reverse', 'xch')
BWD_INPUTS = ('hall', 'gates', 'w_t', 'ext', 'last')
BWD_OUTPUTS = ('dgi', 'dgh', 'dh0', 'xch', 'part')
KIND = {0: 'plain', 2: 'S=2', 4: 'S=4'}


def bwd_setup(c, chains, S, part_elems=0):
    M, H, T = c['M'], c['H'], c['T']
    ext_ld, ext_rows = (H + 8, M + 2) if c['ext_pad'] else (H, M)
    last_ld = H + 8 if c['last'] == 'pad' else H
    t = {k: [] for k in BWD_INPUTS + BWD_OUTPUTS}
    for ins, ref in chains:
        t['hall'].append(dev(ref['hall_in']))
        t['gates'].append(dev(ref['gates_in'], BF))
        t['w_t'].append(dev(np.ascontiguousarray(ins['w'].T), BF))
        if ins['ext'] is None:
            t['ext'].append(None)
        else:
            e = np.full((T, ext_rows, ext_ld), NAN, np.float32)
            e[:, :M, :H] = ins['ext']
            t['ext'].append(dev(e, BF if c['ext'] == 'b' else None))
        if ins['last'] is None:
            t['last'].append(None)
        else:
            q = np.full((M, last_ld), NAN, np.float32)
            q[:, :H] = ins['last']
            t['last'].append(dev(q))
        t['dgi'].append(filled((T * M + 2, 3 * H), BF))
        t['dgh'].append(filled((T * M + 2, 3 * H), BF))
        t['dh0'].append(filled((M + 2, H)) if ins['has_dh0'] else None)
        t['xch'].append(filled((T * M * 3 * H + PAD,), BF))
        t['part'].append(filled((part_elems + PAD,)) if S else None)
    NC = len(chains)
    a = dict(S=S, NC=NC, M=M, H=H, T=T, hall=parr(t['hall']), gates=parr(t['gates']), w_t=parr(t['w_t']),
             ext=None if c['ext'] is None else parr(t['ext']), ext_step=larr([ext_rows * ext_ld] * NC), ext_ld=larr([ext_ld] * NC),
             ext_bf16=iarr([c['ext'] == 'b'] * NC), last=None if c['last'] is None else parr(t['last']), last_ld=larr([last_ld] * NC),
             dgi=parr(t['dgi']), dgh=parr(t['dgh']), dh0=None if all(x is None for x in t['dh0']) else parr(t['dh0']),
             reverse=iarr([ins['reverse'] for ins, _ in chains]), xch=parr(t['xch']), part=parr(t['part']))
    return a, t


def bwd_call(a, S, sync):
    if S:
        return launch('ptv_gru_persist_bwd_splitk', [a[k] for k in ('S',) + BWD_ARGS + ('part',)], sync)
    return launch('ptv_gru_persist_bwd', [a[k] for k in BWD_ARGS], sync)


def untouched_bwd(t):
    for k in BWD_OUTPUTS:
        assert all(is_sent(x) for x in t[k] if x is not None), '%s was written by a refused call' % k


def run_bwd(c, chains, S, reserve=None):
    M, H, T, NC = c['M'], c['H'], c['T'], len(chains)
    reserve = c['reserve'] if reserve is None else reserve
    sync = new_sync()
    with cu_reserve(reserve):
        n = ncu() - reserve
        plan = P.plan_splitk(n, NC, M, H, S) if S else P.plan(n, NC, M, H)
        if S:
            assert L().ptv_gru_persist_splitk_supported(NC, M, H, S) == int(plan is not None)
            part_elems = L().ptv_gru_persist_part_elems(NC, M, H, S)
            assert part_elems == P.part_elems(n, NC, M, H, S)
        else:
            assert L().ptv_gru_persist_supported(NC, M, H) == int(plan is not None)
            part_elems = 0
        a, t = bwd_setup(c, chains, S, part_elems)
        before = {k: [None if x is None else bits(x) for x in t[k]] for k in BWD_INPUTS}
        rc = bwd_call(a, S, sync)
    if plan is None:
        assert rc == ERR_UNSUPPORTED and not sync.any().item()
        untouched_bwd(t)
        return None
    assert rc == OK
    out = []
    for i, (ins, _) in enumerate(chains):
        for k in BWD_INPUTS:
            assert before[k][i] is None or np.array_equal(before[k][i], bits(t[k][i])), 'input %s was written' % k
        assert is_sent(t['dgi'][i][T * M:]) and is_sent(t['dgh'][i][T * M:]) and is_sent(t['xch'][i][T * M * 3 * H:]), 'pad rows written'
        assert t['dh0'][i] is None or is_sent(t['dh0'][i][M:])
        assert t['part'][i] is None or is_sent(t['part'][i][part_elems:]), 'the tail behind part was written'
        out.append(dict(dgi=val(t['dgi'][i][:T * M]).reshape(T, M, 3 * H), dgh=val(t['dgh'][i][:T * M]).reshape(T, M, 3 * H),
                        dgh_bits=bits(t['dgh'][i][:T * M]).reshape(T, M, 3 * H), dgi_bits=bits(t['dgi'][i][:T * M]).reshape(T, M, 3 * H),
                        dh0=None if t['dh0'][i] is None else t['dh0'][i][:M].cpu().numpy(),
                        xch=bits(t['xch'][i][:T * M * 3 * H]).reshape(T, 3 * H // 8, M, 8)))
    return out


def dh_passed_on(ins, rows):
    """dh0 of rows that are dead at every step: the arriving gradients added in the kernel's order, fp32, nothing else"""
    T = ins['gi'].shape[0]
    d = np.zeros((int(rows.sum()), ins['h0'].shape[1]), np.float32)
    for s in range(T - 1, -1, -1):
        e = np.zeros_like(d) if ins['ext'] is None else ins['ext'][s][rows].astype(np.float32)
        if s == T - 1 and ins['last'] is not None:
            e = e + ins['last'][rows]
        d = (np.float32(0) + d) + e
    return d


def verify_bwd(c, out, chains, S):
    M, H, T = c['M'], c['H'], c['T']
    fam = 'bptt %s ' % KIND[S]
    for o, (ins, ref) in zip(out, chains):
        dgi, dgh, dh0 = ref['bwd']
        kgi, kgh, kh0 = ref['kbwd']
        check_planes(fam + 'dgi', o['dgi'], dgi, kgi)
        check_planes(fam + 'dgh', o['dgh'], dgh, kgh)
        assert (o['dh0'] is not None) == ins['has_dh0']
        if o['dh0'] is not None:
            check(fam + 'dh0', o['dh0'], dh0, kh0)
        for s in range(T):
            t = time_of(s, T, ins['reverse'])
            assert np.array_equal(o['dgi_bits'][t][:, :2 * H], o['dgh_bits'][s][:, :2 * H]), 'r / z planes of dgi[t] and dgh[step] differ'
            assert np.array_equal(o['xch'][s], P.blocked(o['dgh_bits'][s])), 'xch slot %d is not blocked(dgh[%d])' % (s, s)
            if ins['lengths'] is not None:
                dead = t >= ins['lengths']
                assert (o['dgi'][t][dead] == 0).all() and (o['dgh'][s][dead] == 0).all(), 'a dead row has gate gradients'
        if ins['lengths'] is not None and o['dh0'] is not None:
            never = ins['lengths'] <= 0
            assert np.array_equal(o['dh0'][never].view(np.int32), dh_passed_on(ins, never).view(np.int32)), 'a dead row does not pass dh on'


BWD_CASES = [(c, S) for c in P.CASES for S in (0, 2, 4)] + [(c, S) for c in P.SK_T6 for S in (2, 4)]


@pytest.mark.parametrize('c,S', BWD_CASES, ids=lambda x: P.case_id(x) if isinstance(x, dict) else KIND[x])
def test_bptt(c, S):
    chains = chains_of(c)
    out = run_bwd(c, chains, S)
    if out is None:
        if S == 0 and P.plan(256 - c['reserve'], c['NC'], c['M'], c['H']) is None:
            return                                                      # FM = 8: the plain BPTT refuses, as asserted
        pytest.skip('the plan of this device (%d CUs) refuses the shape' % ncu())
    verify_bwd(c, out, chains, S)


# ================================================================================================ bit for bit between launches
def same(a, b, what):
    assert a is not None and b is not None, 'the plan of this device refuses one side of %s' % what
    for x, y in zip(a, b):
        for k in x:
            if x[k] is not None and k not in ('hall16', 'dgi', 'dgh'):
                xa, ya = np.ascontiguousarray(x[k]), np.ascontiguousarray(y[k])
                assert np.array_equal(xa.view(np.int32 if xa.dtype == np.float32 else xa.dtype),
                                      ya.view(np.int32 if ya.dtype == np.float32 else ya.dtype)), '%s: %s differs' % (what, k)


def need(c, S=None):
    n = ncu() - c['reserve']
    ok = P.plan(n, c['NC'], c['M'], c['H']) if S is None or S == 0 else P.plan_splitk(n, c['NC'], c['M'], c['H'], S)
    if ok is None:
        pytest.skip('the plan of this device (%d CUs) refuses the shape' % ncu())


@pytest.mark.parametrize('c', [P.CASES[i] for i in P.POLICY_CASES], ids=P.case_id)
def test_load_policies_give_identical_bits(c):
    """only the cache path of the exchanged operand differs between sc1 loads, nt loads and plain loads behind one acquire"""
    need(c)
    chains = chains_of(c)
    fwd, bwd = [], []
    for lp in (0, 1, 2):
        with load_policy(lp):
            fwd.append(run_fwd(c, chains))
            bwd.append(run_bwd(c, chains, 0))
    verify_fwd(c, fwd[0], chains), verify_bwd(c, bwd[0], chains, 0)
    for lp in (1, 2):
        same(fwd[0], fwd[lp], 'forward, load policy 0 / %d' % lp), same(bwd[0], bwd[lp], 'BPTT, load policy 0 / %d' % lp)


@pytest.mark.parametrize('S', [None, 0, 2, 4], ids=['fwd', 'plain', 'S=2', 'S=4'])
def test_one_chain_alone_and_inside_three(S):
    """every variant walks K ascending in 32-wide blocks: a chain's bits do not depend on what else the launch holds"""
    alone, three = P.ALONE_VS_NC3
    need(alone, S), need(three, S)
    run = (lambda c: run_fwd(c, chains_of(c))) if S is None else (lambda c: run_bwd(c, chains_of(c), S))
    same(run(alone), run(three)[:1], 'alone / chain 0 of NC = 3')


@pytest.mark.parametrize('S', [None, 0, 2, 4], ids=['fwd', 'plain', 'S=2', 'S=4'])
def test_one_chain_under_two_plans(S):
    """reserve 0 (RG = 2, FM = 2 at 256 CUs) against reserve 240 (RG = 1, FM = 4): the same rows, the same bits"""
    a, b = P.RESERVE_PAIR
    need(a, S), need(b, S)
    chains = chains_of(a)
    run = (lambda r: run_fwd(a, chains, reserve=r)) if S is None else (lambda r: run_bwd(a, chains, S, reserve=r))
    same(run(a['reserve']), run(b['reserve']), 'reserve 0 / 240')


@pytest.mark.parametrize('S', [2, 4])
def test_splitk_twice_is_bit_identical(S):
    """the header's "bit-reproducible": the team adds its partial tiles in source order, whatever the arrival order"""
    c = P.SK_T6[1]
    need(c, S)
    chains = chains_of(c)
    same(run_bwd(c, chains, S), run_bwd(c, chains, S), 'split-K S = %d issued twice' % S)


# ================================================================================================ host surface
def test_support_answers_agree_with_the_plan_mirror():
    for reserve in (0, 224, 240):
        with cu_reserve(reserve):
            n = ncu() - reserve
            for NC in (0, 1, 2, 3, 4, 5):
                for H in (128, 256, 384, 512, 768, 1024, 1280):
                    for M in (0, 1, 63, 64, 65, 130, 256, 257, 300, 512, 513, 520, 1024, 1025, 2049, 4097):
                        want = P.plan(n, NC, M, H)
                        assert L().ptv_gru_persist_supported(NC, M, H) == int(want is not None), (reserve, NC, M, H)
                        for S in (0, 1, 2, 3, 4, 8):
                            q = P.plan_splitk(n, NC, M, H, S)
                            assert L().ptv_gru_persist_splitk_supported(NC, M, H, S) == int(q is not None), (reserve, NC, M, H, S)
                            assert L().ptv_gru_persist_part_elems(NC, M, H, S) == P.part_elems(n, NC, M, H, S), (reserve, NC, M, H, S)


def test_process_wide_switches_refuse_what_the_header_says():
    try:
        assert L().ptv_gru_persist_load_policy(3) == ERR_ARG and L().ptv_gru_persist_load_policy(-1) == ERR_ARG
        assert L().ptv_gru_persist_cu_reserve(256) == ERR_ARG and L().ptv_gru_persist_cu_reserve(-1) == ERR_ARG
        c = P.CASES[1]
        assert L().ptv_gru_persist_supported(1, c['M'], c['H']) == int(P.plan(ncu(), 1, c['M'], c['H']) is not None)   # (nothing was set)
    finally:
        with cu_reserve(0), load_policy(0):
            pass


BASE = P._case(40, 256, 2, gi2='step', ext_pad=True, last='pad')
OFF = 2                                                                 # bytes: breaks 4-, 8- and 16-byte alignment alike


def shifted(ts, by=OFF):
    return parr([t.data_ptr() + by for t in ts])


FWD_REFUSALS = [
    ('T=0', dict(T=0), ERR_ARG), ('NC=0', dict(NC=0), ERR_UNSUPPORTED), ('NC=5', dict(NC=5), ERR_UNSUPPORTED),
    ('H=128', dict(H=128), ERR_UNSUPPORTED), ('H=384', dict(H=384), ERR_UNSUPPORTED), ('H=1280', dict(H=1280), ERR_UNSUPPORTED),
    ('M=0', dict(M=0), ERR_UNSUPPORTED),
] + [('NULL table ' + k, {k: None}, ERR_ARG) for k in ('gi', 'gi_step', 'gi_ld', 'w', 'b', 'hall', 'hall16', 'reverse', 'xch')] + [
    ('NULL entry ' + k, {k: 'null'}, ERR_ARG) for k in ('gi', 'w', 'b', 'hall', 'hall16', 'xch')] + [
    ('gi_ld % 4', dict(gi_ld=larr([3 * 256 + 2])), ERR_ARG), ('gi_step % 4', dict(gi_step=larr([40 * 768 + 2])), ERR_ARG),
    ('gi2_ld % 4', dict(gi2_ld=larr([3 * 256 + 2])), ERR_ARG), ('gi2_step % 4', dict(gi2_step=larr([40 * 768 + 1])), ERR_ARG),
    ('gi2 strides NULL', dict(gi2_ld=None), ERR_ARG), ('sync NULL', dict(sync=None), ERR_ARG), ('sync misaligned', dict(sync='shift'), ERR_ARG),
] + [('misaligned ' + k, {k: 'shift'}, ERR_ARG) for k in ('gi', 'gi2', 'w', 'b', 'hall', 'hall16', 'gates', 'lengths', 'xch')]


def apply(a, t, over, sync):
    a = dict(a)
    s = sync
    for k, v in over.items():
        if k == 'sync':
            s = None if v is None else sync.data_ptr() + OFF
        elif isinstance(v, str) and v == 'null':
            a[k] = parr([None])
        elif isinstance(v, str) and v == 'shift':
            a[k] = shifted(t[k])
        else:
            a[k] = v
    return a, s


@pytest.mark.parametrize('name,over,want', FWD_REFUSALS, ids=[r[0] for r in FWD_REFUSALS])
def test_forward_refusals(name, over, want):
    need(BASE)
    c = dict(BASE, lengths=True)
    chains = chains_of(c)
    a, t = fwd_setup(c, chains)
    sync = new_sync()
    a, s = apply(a, t, over, sync)
    assert launch('ptv_gru_persist_fwd', [a[k] for k in FWD_ARGS], s) == want
    untouched_fwd(c, t, chains)
    assert not sync.any().item()


BWD_REFUSALS = [
    ('T=0', dict(T=0), ERR_ARG), ('NC=0', dict(NC=0), ERR_UNSUPPORTED), ('NC=5', dict(NC=5), ERR_UNSUPPORTED),
    ('H=128', dict(H=128), ERR_UNSUPPORTED), ('H=384', dict(H=384), ERR_UNSUPPORTED), ('H=1280', dict(H=1280), ERR_UNSUPPORTED),
    ('M=0', dict(M=0), ERR_UNSUPPORTED),
] + [('NULL table ' + k, {k: None}, ERR_ARG) for k in ('hall', 'gates', 'w_t', 'dgi', 'dgh', 'reverse', 'xch')] + [
    ('NULL entry ' + k, {k: 'null'}, ERR_ARG) for k in ('hall', 'gates', 'w_t', 'dgi', 'dgh', 'xch')] + [
    ('ext_ld % 4', dict(ext_ld=larr([256 + 2])), ERR_ARG), ('ext_step % 4', dict(ext_step=larr([42 * 264 + 2])), ERR_ARG),
    ('last_ld % 4', dict(last_ld=larr([256 + 6])), ERR_ARG), ('ext strides NULL', dict(ext_ld=None), ERR_ARG),
    ('last_ld NULL', dict(last_ld=None), ERR_ARG), ('sync NULL', dict(sync=None), ERR_ARG), ('sync misaligned', dict(sync='shift'), ERR_ARG),
] + [('misaligned ' + k, {k: 'shift'}, ERR_ARG) for k in ('hall', 'gates', 'w_t', 'ext', 'last', 'dgi', 'dgh', 'dh0', 'xch')]
SK_REFUSALS = [('S=3', dict(S=3), ERR_UNSUPPORTED), ('S=8', dict(S=8), ERR_UNSUPPORTED), ('NULL table part', dict(part=None), ERR_ARG),
               ('NULL entry part', dict(part='null'), ERR_ARG), ('misaligned part', dict(part='shift'), ERR_ARG)]


BPTT_REFUSALS = [r + (S,) for S in (0, 2) for r in BWD_REFUSALS] + [r + (2,) for r in SK_REFUSALS]


@pytest.mark.parametrize('name,over,want,S', BPTT_REFUSALS, ids=['%s-%s' % (r[0], KIND[r[3]]) for r in BPTT_REFUSALS])
def test_bptt_refusals(name, over, want, S):
    need(BASE, S)
    chains = chains_of(BASE)
    a, t = bwd_setup(BASE, chains, S, L().ptv_gru_persist_part_elems(1, BASE['M'], BASE['H'], S) if S else 0)
    sync = new_sync()
    a, s = apply(a, t, over, sync)
    assert bwd_call(a, S, s) == want
    untouched_bwd(t)
    assert not sync.any().item()


def test_misaligned_bf16_dh_ext_is_refused():
    """bf16 dh_ext is read 8 bytes at a time (fp32: 16): an address that is 8- but not 16-byte aligned passes as bf16 only"""
    need(BASE)
    for kind, by, want in (('b', 4, ERR_ARG), ('f', 8, ERR_ARG)):
        c = dict(BASE, ext=kind)
        chains = chains_of(c)
        a, t = bwd_setup(c, chains, 0)
        sync = new_sync()
        a['ext'] = shifted(t['ext'], by)
        assert bwd_call(a, 0, sync) == want
        untouched_bwd(t)
        assert not sync.any().item()
