"""functional.BiGruFinalFn -- the bi-GRU autograd node, _bigru_forward / _bigru_backward and the composites ptv_bigru_final_fwd / _bwd and
ptv_bigru_rows_fwd / _bwd behind it -- against the plain fp64 reference of tests/bigru_ref.py, branch by branch.  The kernels under the
node have isolated tests of their own; this file holds what the node owns: the input products, the length sort (perm) and the per-step
live-row counts (seg), the `top` clip of the three products, the reversed direction's k_rev and negative seg_period, which half of `out`
a direction writes, the accumulate-into-dx_acc link, the persist-to-step fallback of the backward, the two-stream fork and join.

Every case runs BiGruFinalFn.apply(x, lengths, prec, *w) and out.backward(dout) on seeded CPU inputs (bigru_ref.inputs), asserts the
branch the forward recorded (out.grad_fn.saved_state.branch) and the call counters of the four composites (F_._BRF, _BRB, _BGF, _BGB: a
quiet fall-back cannot pass as the branch under test), and compares out, dx and the eight parameter gradients with the reference: dx
per time plane at that plane's own scale, every other array at its own.  No tolerance is chosen by hand: the node's error may be at most
4x the error of the kernel-precision CPU evaluation of the same branch (bigru_ref.kp_chain), with a floor of 8 fp32 ulps of the scale
(bound_of of tests/test_gpu_dur_kernels.py); the bound never sees the node's output.  Each check prints `BIGRU_RATIO family ratio`, the
module `BIGRU_RATIO_MAX family` (pytest -s; table in profiles/LOG.md).  Bit for bit: out of a row of length 0 and dx at t >= len are
zero bits; with every length 0 so are out, dx and all eight gradients; everything is finite.  Every buffer the node takes from F_._empty
arrives NaN-filled, so a read of a slot nobody wrote poisons the result.

tests/test_bigru_ref_host.py holds the reference to torch's float64 packed bi-GRU, asserts without a GPU that this bound rejects seven
wrong variants of the reference at these very inputs, and that the case list reaches what it claims.

The persist shape is chosen the way test_bigru_node_records_the_branch_it_ran_... chooses it: the smallest listed (M, H) of
test_gru_persistent_kernels_vs_oracle_and_step_kernels that two chains fit and whose 3 M reaches the backward composite's 512 rows.  The
case below 512 rows keeps that (M, H) when 2 M < 512; when M is too large for any T >= 2 it takes the smallest listed shape the device
supports with 3 M < 512, at T = 3."""
import functools

import numpy as np
import pytest
import torch

import bigru_ref as BR
from test_gpu_dur_kernels import bound_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
RATIOS = {}
KINDS = ('w_ih', 'w_hh', 'b_ih', 'b_hh') * 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host(t):
    return None if t is None else t.detach().float().cpu().numpy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def check(family, got, ref, kp):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), '%s: non-finite output' % family
    bound, errk = bound_of(ref, kp)
    err = np.abs(got - ref)
    ratio = float(np.where(err == 0, 0.0, err / bound).max())
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print('BIGRU_RATIO %s %.3f (node err %.3e, kernel-precision CPU err %.3e)' % (family, ratio, err.max(), errk))
    at = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), '%s: node error %.3e over the bound %.3e at %s (kernel-precision CPU evaluation: %.3e)' % (
        family, err[at], float(bound), at, errk)


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('BIGRU_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


@pytest.fixture
def F_(monkeypatch):
    """the functional module with every _empty buffer NaN-filled; afterwards its switches as they were, ZERO_SKIP handed back to the library"""
    from polyphonic_chord_texture_disentanglement_amd import functional as Fm
    plain_empty = Fm._empty

    def nan_empty(*shape, dev, dtype=torch.float32):
        t = plain_empty(*shape, dev=dev, dtype=dtype)
        return t.fill_(float('nan')) if t.dtype.is_floating_point else t

    monkeypatch.setattr(Fm, '_empty', nan_empty)
    switches = {k: getattr(Fm, k) for k in ('SORT_ROWS', 'ZERO_SKIP', 'BIGRU_BWD_COMPOSITE', 'PERSIST')}       # (the tests assign them)
    yield Fm
    monkeypatch.undo()
    for k, v in switches.items():
        setattr(Fm, k, v)
    Fm.zero_skip_sync()
    torch.cuda.synchronize()


def counts(F_):
    return [t.get('calls', 0) for t in (F_._BRF, F_._BRB, F_._BGF, F_._BGB)]


def expected_counts(c, branch, comp, opt, need_dx, fallback=False):
    """[BRF, BRB, BGF, BGB] of one forward + backward.  The forward composites run whenever they are switched on; the backward composites
    need 512 rows of K, for dx the optimiser's transposed bf16 weight shadows, and (persist) the branch still standing at the backward"""
    big = c['T'] * c['M'] >= 512
    if branch == 'rows':
        return [int(comp), int(comp and big and (opt or not need_dx)), 0, 0]
    if branch == 'persist':
        return [0, 0, int(comp), int(comp and big and not fallback)]
    return [0, 0, 0, 0]


def operands(c, opt=True, need_dx=True):
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    ins = BR.inputs(c)
    w = [torch.nn.Parameter(dev(a)) for a in ins['w8']]
    o = FusedClipAdam(w, lr=1e-3) if opt else None              # (the bf16 weight shadows the persistent kernels and the composites read)
    if o is not None:
        o.zero_grad()
    x = dev(ins['x'], BF if c['x_bf16'] else None).requires_grad_(need_dx)
    lengths = None if ins['lengths'] is None else dev(ins['lengths'])
    return w, o, x, lengths, dev(ins['dout'])


def run_node(F_, c, branch, *, comp=True, opt=True, need_dx=True, before_backward=None, fallback=False, state_check=None):
    """one forward + backward of the node -> host copies of out, dx (or None) and the eight gradients"""
    F_.BIGRU_BWD_COMPOSITE = comp                                # (the F_ fixture puts every switch back)
    w, o, x, lengths, dout = operands(c, opt, need_dx)
    n0 = counts(F_)
    out = F_.BiGruFinalFn.apply(x, lengths, 1 if c['bf16'] else 0, *w)
    state = out.grad_fn.saved_state
    assert state.branch == branch, 'the forward ran on %r, not on %r' % (state.branch, branch)
    if state_check is not None:
        state_check(state)
    if before_backward is not None:
        before_backward()
    out.backward(dout)
    torch.cuda.synchronize()
    F_.persist_check()
    got = [a - b for a, b in zip(counts(F_), n0)]
    assert got == expected_counts(c, branch, comp, opt, need_dx, fallback), 'composite calls [BRF, BRB, BGF, BGB] = %s' % got
    assert (x.grad is None) == (not need_dx)
    return dict(out=host(out), dx=host(x.grad), grads=[host(p.grad) for p in w], raw=[p.grad.clone() for p in w])


def compare(label, c, res, dx_prefill=None):
    ref, ins = BR.reference(c), BR.inputs(c)
    lens, T = ins['lengths'], c['T']
    print('BIGRU_CASE %s %s' % (label, BR.case_id(c)))
    check(label + '.out', res['out'], ref['out'], ref['kp_out'])
    if lens is not None:
        assert not bits(res['out'][lens == 0]).any(), 'out of a row of length 0 is not zero bits'
    if res['dx'] is not None:
        for t in range(T):
            want, kp = ref['dx'][t], ref['kp_dx'][t]
            if dx_prefill is not None:
                want, kp = dx_prefill[t].astype(np.float64) + want, (dx_prefill[t] + kp).astype(np.float32)
            check(label + '.dx', res['dx'][t], want, kp)
            if lens is not None:
                dead = lens <= t
                keep = 0 if dx_prefill is None else bits(dx_prefill[t][dead])
                assert (bits(res['dx'][t][dead]) == keep).all(), 'dx at t = %d >= len: not the bits it must keep' % t
    for kind, g, r, k in zip(KINDS, res['grads'], ref['grads'], ref['kp_grads']):
        check(label + '.' + kind, g, r, k)
    if lens is not None and lens.max() == 0:
        for a in [res['out'], res['dx']] + res['grads']:
            assert a is not None and not bits(a).any(), 'every length is 0: a result is not zero bits'


# ================================================================================================ rows
def rows_state(F_, c, sort=True, zero_skip=True):
    """what the rows forward must record: the lengths it skips by, the sorted order, the K segments (where ptv_wgrad_seg_supported says so)"""
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    M, T = c['M'], c['T']
    has_len = c['lens'] is not None
    want_perm = has_len and zero_skip and sort
    seg_ok = bool(lib().ptv_wgrad_seg_supported(T * M, M)) if M % 128 == 0 else False
    want_seg = want_perm and F_.WGRAD_SEG and M % 128 == 0 and seg_ok
    print('BIGRU_SEG M=%d T=%d ptv_wgrad_seg_supported=%s seg=%s' % (M, T, seg_ok, want_seg))

    def state_check(state):
        assert (state.lengths is not None) == (has_len and zero_skip)
        assert (state.perm is not None) == want_perm and (state.seg is not None) == want_seg
    return state_check


ROWS_RUNS = [(i, True, True, True) for i in range(len(BR.ROWS_CASES))]             # (case, composite, SORT_ROWS, ZERO_SKIP)
ROWS_RUNS += [(i, False, True, True) for i in (0, 4)] + [(i, True, False, True) for i in (0, 4)] + [(0, True, True, False)]


@pytest.mark.parametrize('i,comp,sort,zero_skip', ROWS_RUNS,
                         ids=['%s-%s%s%s' % (BR.case_id(BR.ROWS_CASES[i]), 'composite' if comp else 'python', '' if sort else '-unsorted',
                                             '' if zs else '-dense-steps') for i, comp, sort, zs in ROWS_RUNS])
def test_rows_branch_against_the_fp64_reference(i, comp, sort, zero_skip, F_):
    c = BR.ROWS_CASES[i]
    F_.SORT_ROWS, F_.ZERO_SKIP = sort, zero_skip
    if i == 0 and sort and zero_skip:
        assert F_.WGRAD_SEG and c['M'] % 128 == 0                  # the sorted case runs with K segments or not at all
    res = run_node(F_, c, 'rows', comp=comp, state_check=rows_state(F_, c, sort, zero_skip))
    compare('rows', c, res)


def test_rows_branch_without_an_optimiser(F_):
    """no bf16 weight shadows: the forward composite packs its own weights and runs; the backward composite needs the transposed
    shadow for dx and declines, the Python sequencing takes the fp32 weight through the dense product"""
    c = BR.ROWS_CASES[0]
    compare('rows', c, run_node(F_, c, 'rows', opt=False, state_check=rows_state(F_, c)))


# ================================================================================================ persist, step, crossing
@functools.lru_cache(maxsize=None)
def persist_shapes():
    """-> ((M, H) of the persist cases, (M, H) of the case under 512 rows at T = 3 or 2), None where the device fits none.  `main` is the
    expression of test_bigru_node_records_the_branch_it_ran_... (tests/test_gpu_kernels.py), which computes it inside its body: a change
    of the rule there belongs here too"""
    from polyphonic_chord_texture_disentanglement_amd import functional as Fm
    import test_gpu_kernels as TK
    marks = TK.test_gru_persistent_kernels_vs_oracle_and_step_kernels.pytestmark
    listed = next(m.args[1] for m in marks if m.args[0].startswith('NC,M,H'))
    fit = [s for s in sorted({(c[1], c[2]) for c in listed}, key=lambda s: s[0] * s[1]) if Fm.persist_supported(2, *s)]
    if not fit:
        return None, None
    main = next((s for s in fit if 3 * s[0] >= 512), (max(fit[0][0], -(-512 // 3)), fit[0][1]))
    if not Fm.persist_supported(2, *main):
        return None, None
    small = main if 2 * main[0] < 512 else next((s for s in fit if 3 * s[0] < 512), None)
    return main, small


def persist_case(lens, I, x_bf16, small=False, T=3):
    main, sm = persist_shapes()
    shape = sm if small else main
    if shape is None:
        pytest.skip('persist_supported(2, M, H) accepts no listed shape %s on this device' % ('under 512 rows' if small else ''))
    if small and 3 * shape[0] >= 512:
        T = 2
    if not small:                                                # (the table the host test checks: bigru_ref.persist_cases)
        return next(c for c in BR.persist_cases(*shape) if (c['lens'], c['I'], c['x_bf16']) == (lens, I, x_bf16))
    return BR.case('persist', shape[0], T, lens, H=shape[1], I=I, x_bf16=x_bf16)


@pytest.mark.parametrize('lens,I,x_bf16', BR.PERSIST_GRID,
                         ids=['%s-I%d-x-%s' % ('lengths' if l else 'dense', i, 'bf16' if b else 'fp32') for l, i, b in BR.PERSIST_GRID])
def test_persist_branch_against_the_fp64_reference(lens, I, x_bf16, F_):
    c = persist_case(lens, I, x_bf16)
    assert c['T'] * c['M'] >= 512
    compare('persist', c, run_node(F_, c, 'persist'))


def test_persist_branch_under_512_rows_runs_the_python_sequenced_backward(F_):
    c = persist_case('random', 64, False, small=True)
    assert c['T'] * c['M'] < 512 and c['T'] >= 2
    compare('persist-python-bwd', c, run_node(F_, c, 'persist'))


def test_persist_branch_split_k_bptt_at_the_chord_encoder_width(F_):
    M, H = 512, 1024
    if not F_.persist_supported(2, M, H):
        pytest.skip('persist_supported(2, 512, 1024) refuses on this device')
    if F_.persist_splitk(2, M, H) != 2:
        pytest.skip('persist_splitk(2, 512, 1024) = %d on this device, not 2' % F_.persist_splitk(2, M, H))
    c = BR.case('persist', M, 2, 'random', H=H, I=36)
    compare('persist-splitk', c, run_node(F_, c, 'persist'))


@pytest.mark.parametrize('i', range(len(BR.STEP_FP32_CASES)), ids=[BR.case_id(c) for c in BR.STEP_FP32_CASES])
def test_step_branch_fp32_against_the_fp64_reference(i, F_):
    c = BR.STEP_FP32_CASES[i]
    compare('step-fp32', c, run_node(F_, c, 'step'))


def test_step_branch_bf16_at_the_persist_shape(F_):
    c = dict(persist_case('random', 64, False), branch='step')
    F_.PERSIST = '0'
    compare('step-bf16', c, run_node(F_, c, 'step'))


def test_persist_forward_then_per_step_backward(F_):
    """the persistent kernels' states and gates are in the common layout: with the persistent kernels switched off after the forward,
    the per-step BPTT reads them (_bigru_backward's branch = 'step' fallback) and meets the same bound"""
    c = persist_case('random', 64, False)

    def off():
        F_.PERSIST = '0'
    compare('persist-to-step', c, run_node(F_, c, 'persist', before_backward=off, fallback=True))


# ================================================================================================ dx_acc, need_dx = False
def prefill_of(T, M, I):
    """bf16-exact, never zero: k / 16 with k in -16 .. 16 without 0"""
    k = (np.arange(T * M, dtype=np.int64)[:, None] * 5 + np.arange(I, dtype=np.int64)[None, :] * 3) % 32 - 16
    return (np.where(k >= 0, k + 1, k) / 16.0).astype(np.float32)


@pytest.mark.parametrize('which', ['rows-composite', 'rows-python', 'persist'])
def test_dx_acc_receives_both_directions_and_keeps_its_dead_times(which, F_):
    """_bigru_backward(..., need_dx, dx_acc): the decoder node's gradient of the same tensor is already in dx_acc; both directions'
    dX products accumulate into it and it is what comes back"""
    branch = which.split('-')[0]
    c = BR.ROWS_CASES[0] if branch == 'rows' else persist_case('random', 64, False)
    comp = which != 'rows-python'
    F_.BIGRU_BWD_COMPOSITE = comp
    T, M, I = c['T'], c['M'], c['I']
    w, o, x, lengths, dout = operands(c, need_dx=False)
    pre = prefill_of(T, M, I)
    assert BR.GM.is_bf16(pre) and pre.all()
    dx_acc = dev(pre)
    out, state = F_._bigru_forward(1, x, lengths, w)
    assert state.branch == branch
    n0 = counts(F_)
    grads, dx = F_._bigru_backward(1, x, w, state, dout, True, dx_acc)
    torch.cuda.synchronize()
    F_.persist_check()
    assert [a - b for a, b in zip(counts(F_), n0)] == [0, int(comp and branch == 'rows'), 0, int(comp and branch == 'persist')]
    assert dx.data_ptr() == dx_acc.data_ptr() and tuple(dx.shape) == (T, M, I)
    res = dict(out=host(out), dx=host(dx_acc).reshape(T, M, I), grads=[host(g) for g in grads])
    compare(which.replace('-composite', '') + '.dx_acc', c, res, dx_prefill=pre.reshape(T, M, I))


@pytest.mark.parametrize('which', ['rows', 'persist', 'step-fp32'])
def test_without_an_input_gradient_the_parameter_gradients_keep_their_bits(which, F_):
    branch = which.split('-')[0]
    c = {'rows': lambda: BR.ROWS_CASES[0], 'persist': lambda: persist_case('random', 64, False), 'step': lambda: BR.STEP_FP32_CASES[0]}[branch]()
    with_dx = run_node(F_, c, branch)
    without = run_node(F_, c, branch, need_dx=False)
    assert without['dx'] is None
    for a, b in zip(with_dx['raw'], without['raw']):
        assert torch.equal(a, b)
    assert np.array_equal(bits(with_dx['out']), bits(without['out']))
