"""The row-partitioned persistent GRUs one call at a time -- csrc/notes_persist.hip (row_gru_fwd_kernel<128, true>,
row_gru_bwd_kernel<128, true>, the 4-wave row_gru_bwd_kernel<512, false>) and csrc/notes_roles.hip (the 8-wave notes_fwd_kernel and
notes_bwd_kernel) behind ptv_notes_gru_persist_{fwd,bwd}{,_top,_rows}, ptv_row_gru_persist_{fwd,bwd}{,_perm} and both values of
ptv_notes_bwd_variant -- against the plain fp64 references of tests/rowgru_ref.py, through the C ABI as it is declared
(kernel_ops.leaf_rc).  Every variant is held to the reference on its own, never to another variant or to the per-step kernels.

Inputs are built on the CPU from seeded generators; weights, gc, ext and the fed tokens of the H = 512 cases are bf16-representable.
The backward gets the fp64 REFERENCE's states and gates, rounded to their storage types and written by this file in the blocked layouts
(rowgru_ref.gates_blocked / ext_blocked / gc_blocked), never a kernel's forward output; one chained forward -> backward case per kernel
pair is held end to end to the unrounded fp64 chain.  Every output is pre-filled with the sentinel 768.0 and carries 2 pad rows that
must keep it; input regions the contract says are not read hold NaN; after the call every input is byte-identical.

Every output slot has one of the classes of rowgru_ref (LIVE / ZERO / UNWRITTEN / EITHER), predicted from the call's arguments alone.
LIVE slots have no pre-chosen tolerance: the kernel's error against the fp64 reference may be at most 4x the error of the
kernel-precision CPU evaluation (rowgru_ref.kp_*), with a floor of 8 fp32 ulps of the scale (bound_of of test_gpu_dur_kernels.py) --
taken PER STEP PLANE, so the small early-step gradients are checked at their own size.  The bound never sees the kernel's output.
Each check prints `ROWGRU_RATIO family ratio`, the module `ROWGRU_RATIO_MAX family` (pytest -s; table in profiles/LOG.md).  Bit for
bit: HN16 is the RNE rounding of HN (H = 128) and of h0 in slot 0; a masked row copies its state; a row of length 0 never leaves h0 and
its `out` row has h0's bits; out[perm[p]] has the bits of the last written HN slot of position p; ZERO / UNWRITTEN slots; top_step.

Shapes: R in {1, 63, 64, 65, 96, 130, 200}, T in {1, 2, 5} (16 / 15 once), and per kernel R = 2176 (34 panels) with the ragged sibling
2182 at T = 2, where every panel-dependent rotation of the four kernels takes at least two values:
    row_gru_fwd_kernel<128>   prot = (panel >> 3) & (NPASS - 1), NPASS = H / 128 = 1: always 0
                              krot = (((panel >> 5) & 7) * 2) & (KBH - 1), KBH = H / 32 = 4: 0 for panels 0-31, 2 from panel 32
    notes_fwd_kernel          rot = (blockIdx.x >> 3) & (MPS - 1), MPS = 8: a new value every 8 panels (0 .. 4 over 34 panels)
    row_gru_bwd_kernel<H>     none (tile and k order are fixed)
    notes_bwd_kernel          none
tests/test_rowgru_ref_host.py asserts, without a GPU, that the row lists used here exercise every prediction class."""
import contextlib
import functools
import zlib

import numpy as np
import pytest
import torch

import kernel_ops as K
import rowgru_ref as RR
from rowgru_ref import EITHER, LIVE, UNWRITTEN, ZERO
from test_gpu_dur_kernels import bound_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = np.float32(np.nan)
SENT = np.float32(768.0)                                               # (exact in bf16)
BF = torch.bfloat16
RATIOS = {}
E = RR.E
BIT16, BIT24 = 1 << 16, 1 << 24


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.float().cpu().numpy() if t.dtype == BF else t.cpu().numpy()


def raw(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32).cpu().numpy().tobytes()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def out_buf(shape, dtype=torch.float32):
    """sentinel-filled output of `shape` with 2 pad rows behind it -> (view, whole buffer)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * shape[-1],), float(SENT), dtype=dtype, device=DEV)
    return whole[:n].view(*shape), whole


def pads_kept(whole, shape):
    return bool((whole[int(np.prod(shape)):] == float(SENT)).all())


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
    print('ROWGRU_RATIO %s %.3f (kernel err %.3e, kernel-precision CPU err %.3e)' % (family, ratio, err.max(), errk))
    at = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), '%s: kernel error %.3e over the bound %.3e at %s (kernel-precision CPU evaluation: %.3e)' % (
        family, err[at], float(np.min(bound)), at, errk)


def check_slots(family, got, ref, kp, cls):
    """got / ref / kp [S, R, W], cls [S, R]: the LIVE rows of every step plane against the reference at the plane's own scale; ZERO rows
    are zero bits, UNWRITTEN rows the sentinel's, EITHER rows one of the two"""
    got = np.asarray(got, np.float32)
    gb, sb = bits(got), bits(SENT)
    for c, ok, what in ((ZERO, gb == 0, 'exact zeros'), (UNWRITTEN, gb == sb, 'untouched'), (EITHER, (gb == 0) | (gb == sb), 'zeros or untouched')):
        bad = (cls == c)[:, :, None] & ~ok
        assert not bad.any(), '%s: slot (step, row, unit) %s should be %s, holds %r' % (family, np.argwhere(bad)[0], what, got[tuple(np.argwhere(bad)[0])])
    for s in range(cls.shape[0]):
        live = cls[s] == LIVE
        if live.any():
            check(family, got[s][live], ref[s][live], kp[s][live])


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('ROWGRU_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


@contextlib.contextmanager
def zero_skip(on):
    """ptv_zero_skip(on) for the block; afterwards what the package last handed to the library (default 1)"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    lib().ptv_zero_skip(int(on))
    try:
        yield
    finally:
        lib().ptv_zero_skip(int(F_._ZERO_SKIP_SET[0]) if F_._ZERO_SKIP_SET else 1)


@contextlib.contextmanager
def bwd_variant(eight):
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    lib().ptv_notes_bwd_variant(int(eight))
    try:
        yield
    finally:
        lib().ptv_notes_bwd_variant(1)


def C(**kw):
    return tuple(sorted(kw.items()))


def cid(key):
    c = dict(key)
    head = 'R%d T%d' % (c.pop('R'), c.pop('T'))
    return head + ''.join(' %s' % k if v is True else ' %s=%s' % (k, v) for k, v in sorted(c.items()) if v is not False and v is not None)


def seed_of(key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def pack(w, pairs):
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    return F_.pack_mfma_b(dev(w), pairs=pairs)


def int_dev(v):
    return None if v is None else torch.tensor(np.atleast_1d(v), dtype=torch.int32, device=DEV)


# ================================================================================================ H = 128: the note-summary GRU
H1 = 128
# lens: None / 'mixed' / 'short' (rowgru_ref.lengths_of); perm: None / 'id' / 'len'; wide: out and dh_last are halves of [R, 2H] rows
CASES128 = [
    C(R=1, T=1, sharp=True),
    C(R=63, T=2, lens='mixed', reverse=True, perm='id', wide=True),
    C(R=64, T=5, lens='short'),                                          # R % 32 == 0: the last time index is dead for the launch
    C(R=64, T=5, lens='short', reverse=True, perm='len', wide=True),     # ... and a dead PREFIX of the reversed direction
    C(R=65, T=1, lens='mixed', perm='len'),
    C(R=96, T=1, lens='short'),                                          # every row empty: nothing runs
    C(R=96, T=2, lens='short', reverse=True, wide=True),
    C(R=96, T=5, lens='mixed', perm='len'),
    C(R=130, T=1, lens='mixed'),                                         # panels 1 and 2 hold empty rows only
    C(R=130, T=5, lens='mixed', reverse=True, wide=True),
    C(R=130, T=2, reverse=True, perm='id'),
    C(R=200, T=5, lens='mixed', perm='len', wide=True),
    C(R=200, T=16, lens='mixed', reverse=True, perm='len'),
    C(R=2176, T=2, lens='mixed', perm='len', wide=True),
    C(R=2182, T=2, reverse=True),
]
SKIP128 = [c for c in CASES128 if dict(c).get('lens') and dict(c)['T'] == 5 and dict(c)['R'] in (64, 96)]


def perm_of(c, lengths):
    kind = c.get('perm')
    if kind is None:
        return None
    return np.arange(c['R'], dtype=np.int32) if kind == 'id' else RR.by_length(lengths)


@functools.lru_cache(maxsize=16)
def case128(key):
    """inputs (natural row order), fp64 reference and kernel-precision evaluation of one H = 128 case, forward and BPTT (read only)"""
    c = dict(key)
    R, T, H = c['R'], c['T'], H1
    rng = np.random.RandomState(seed_of(key))
    k = 1.0 / np.sqrt(H)
    U = lambda *s: RR.bf16_round(rng.uniform(-k, k, s))
    sharp = lambda a: RR.bf16_round(a) if c.get('sharp') else a.astype(np.float32)
    d = dict(w_x=U(3 * H, E), w_hh=U(3 * H, H), b_ih=rng.uniform(-k, k, 3 * H).astype(np.float32), b_hh=rng.uniform(-k, k, 3 * H).astype(np.float32),
             x=sharp(rng.randn(T, R, E) * 0.7), h0=sharp(rng.randn(R, H) * 0.5), dl=(rng.randn(R, 2 * H) * 0.3).astype(np.float32))
    d['lengths'] = RR.lengths_of(R, T, c['lens']) if c.get('lens') else None
    d['perm'] = perm_of(c, d['lengths'])
    rev = bool(c.get('reverse'))
    d['dh_last'] = d['dl'][:, H:] if rev else d['dl'][:, :H]
    args = (H, d['x'], d['w_x'], d['w_hh'], d['b_hh'], d['h0'])
    kw = dict(b_ih=d['b_ih'], lengths=d['lengths'], reverse=rev)
    d['st'], d['gates'] = RR.forward(*args, **kw)
    d['kst'], d['kgates'], _ = RR.kp_forward(*args, **kw)
    # the BPTT's operands: the reference's states and gates as stored (fp32 / bf16)
    d['st32'], d['g16'] = d['st'].astype(np.float32), RR.bf16_round(d['gates'])
    d['dgi'], d['dgh'], d['dh0'] = RR.backward(H, d['st32'][:T], d['g16'], d['w_hh'], None, d['dh_last'], rev)
    d['kdgi'], d['kdgh'], d['kdh0'] = RR.kp_backward(H, d['st32'][:T], d['g16'], d['w_hh'], None, d['dh_last'], rev)
    # end to end: nothing rounded in between
    d['e2e'] = RR.backward(H, d['st'][:T], d['gates'], d['w_hh'], None, d['dh_last'], rev)
    d['ke2e'] = RR.kp_backward(H, d['kst'][:T], d['kgates'], d['w_hh'], None, d['dh_last'], rev)
    return d


def run_fwd128(c, d, skip=True):
    """one forward call -> the outputs on the host, checked for sentinels / classes / bit identities; LIVE slots are returned unchecked"""
    R, T, H = c['R'], c['T'], H1
    perm, rev, wide = d['perm'], bool(c.get('reverse')), bool(c.get('wide'))
    ex = RR.expect_fwd128(R, T, d['lengths'], perm, rev, skip)
    x = d['x'].copy()
    if d['lengths'] is not None and skip and R % 32 == 0:               # time indices that are dead for the whole launch are not read
        x[min(max(int(d['lengths'].max()), 0), T):] = NAN
    ins = dict(wh=pack(d['w_hh'], True), wx=pack(d['w_x'], True), b_hh=dev(d['b_hh']), b_ih=dev(d['b_ih']), x=dev(x),
               lengths=dev(d['lengths']), perm=dev(perm))
    HN, HNw = out_buf((T + 1, R, H))
    HN[0] = dev(RR.to_pos(d['h0'], perm, 0))
    HN16, HN16w = out_buf((T + 1, R, H), BF)
    gates, gatesw = out_buf((T, 4, H // 32, R, 32), BF)
    ld = 2 * H if wide else H
    out, outw = out_buf((R, ld))
    o = out[:, H:] if wide and rev else out[:, :H]
    before = {k: raw(v) for k, v in ins.items() if v is not None}
    a = ('ptv_row_gru_persist_fwd_perm' if perm is not None else 'ptv_row_gru_persist_fwd', H, ins['wh'], ins['wx'], ins['b_hh'], ins['b_ih'], None, ins['x'],
         R * E, ins['lengths']) + ((ins['perm'],) if perm is not None else ()) + (HN, HN16, gates, o, ld, R, T, int(rev))
    with zero_skip(skip):
        assert K.leaf_rc(*a) == 0
        torch.cuda.synchronize()
    assert all(raw(v) == before[k] for k, v in ins.items() if v is not None), 'an input was written'
    assert pads_kept(HNw, (T + 1, R, H)) and pads_kept(HN16w, (T + 1, R, H)) and pads_kept(gatesw, (T, 4, R, H)) and pads_kept(outw, (R, ld))
    g = dict(HN=host(HN), HN16=host(HN16), gates=RR.gates_unblocked(host(gates), H), out=host(out), ex=ex)
    h0p = RR.to_pos(d['h0'], perm, 0)
    assert np.array_equal(bits(g['HN'][0]), bits(h0p)), 'slot 0 of HN is the caller\'s'
    assert np.array_equal(bits(g['HN16'][0]), bits(RR.bf16_round(h0p))), 'HN16 slot 0 = RNE(h0)'
    # ---- bit identities over the written slots
    lens = np.full(R, T + 1) if d['lengths'] is None else RR.to_pos(d['lengths'], perm, 0)
    written = ex['HN'] == LIVE
    written[0] = True
    for s in range(T + 1):
        w = written[s]
        assert np.array_equal(bits(g['HN16'][s][w]), bits(RR.bf16_round(g['HN'][s][w]))), 'HN16 slot %d is not RNE(HN)' % s
        assert (bits(g['HN'][s][~w]) == bits(SENT)).all() and (bits(g['HN16'][s][~w & (ex['HN16'][s] != LIVE)]) == bits(SENT)).all(), 'slot %d' % s
    for p in range(R):                                                  # between two written slots with only masked steps: the same bits
        prev = 0
        for s in range(1, T + 1):
            if written[s, p]:
                if all(RR.G.time_of(n, T, rev) >= lens[p] for n in range(prev, s)):
                    assert np.array_equal(bits(g['HN'][s, p]), bits(g['HN'][prev, p])), 'row at position %d: masked steps %d..%d changed the state' % (p, prev, s)
                prev = s
    nat = np.arange(R) if perm is None else perm
    col = slice(H, 2 * H) if wide and rev else slice(0, H)
    assert np.array_equal(bits(g['out'][nat, col]), bits(g['HN'][ex['final'], np.arange(R)])), 'out[perm[p]] = the last written slot of position p'
    if wide:
        assert (bits(g['out'][:, slice(0, H) if rev else slice(H, 2 * H)]) == bits(SENT)).all(), 'the other half of the out rows'
    return g


def assert_fwd128(c, d, g):
    R, T, H = c['R'], c['T'], H1
    perm, ex = d['perm'], g['ex']
    P = lambda a, ax=1: RR.to_pos(a, perm, ax)
    cls = ex['HN'].copy()
    cls[0] = 0                                                           # (asserted bit for bit above)
    check_slots('fwd128 HN', g['HN'], P(d['st']), P(d['kst']), cls)
    check_slots('fwd128 HN16', g['HN16'], P(d['st']), RR.bf16_round(P(d['kst'])), np.where(cls == 0, 0, ex['HN16']).astype(np.uint8))
    for q, nm in enumerate(('r', 'z', 'n', 'hn')):
        check_slots('fwd128 gate %s' % nm, g['gates'][:, q], P(d['gates'][:, q]), P(d['kgates'][:, q]), ex['gates'])
    if d['lengths'] is not None:                                         # a masked row of a computed step saves the gates (0, 1, 0)
        lens = P(d['lengths'], 0)
        for n in range(T):
            m = (ex['gates'][n] == LIVE) & (RR.G.time_of(n, T, bool(c.get('reverse'))) >= lens)
            assert (g['gates'][n, 0][m] == 0).all() and (g['gates'][n, 1][m] == 1).all() and (g['gates'][n, 2][m] == 0).all()


@pytest.mark.parametrize('key', CASES128, ids=cid)
def test_row_gru_h128_forward(key):
    """ptv_row_gru_persist_fwd / _fwd_perm, H = 128: states, bf16 states, gate planes (unit-blocked by 32) and final state against
    the fp64 reference; with T = 1 and bf16-representable state and tokens (the `sharp` case) the products are exact and the fp32 state
    is checked at fp32 sharpness"""
    c, d = dict(key), case128(key)
    assert_fwd128(c, d, run_fwd128(c, d))


@pytest.mark.parametrize('key', SKIP128, ids=cid)
def test_row_gru_h128_forward_zero_skip_off(key):
    """ptv_zero_skip(0): no panel or launch-wide limit, every slot is computed -- held to the reference by itself, and bit-identical
    to the skipping run wherever that one writes (skipping only leaves out copies of the state)"""
    c, d = dict(key), case128(key)
    g0 = run_fwd128(c, d, skip=False)
    assert_fwd128(c, d, g0)
    g1 = run_fwd128(c, d, skip=True)
    assert (g0['ex']['HN'][1:] == LIVE).all() and (g0['ex']['gates'] == LIVE).all() and (g1['ex']['gates'] != LIVE).any()
    for nm in ('HN', 'HN16', 'gates'):
        w = g1['ex'][nm] == LIVE
        a, b = (g0[nm], g1[nm]) if nm != 'gates' else (g0[nm].transpose(0, 2, 1, 3), g1[nm].transpose(0, 2, 1, 3))
        assert np.array_equal(bits(a[w]), bits(b[w])), nm
    assert np.array_equal(bits(g0['out']), bits(g1['out']))


def run_bwd128(c, d, i, hn=None, gates=None, refs=None, family='bwd128'):
    """one BPTT call on the reference's stored states and gates (or, chained, a forward kernel's: hn / gates as tensors)"""
    R, T, H = c['R'], c['T'], H1
    perm, rev, wide = d['perm'], bool(c.get('reverse')), bool(c.get('wide'))
    top_given, want_dh0 = i % 2 == 0, perm is None
    top_init = T + 5 if i % 4 == 0 else -1
    ex = RR.expect_bwd128(R, T, d['lengths'], perm, rev, top_given, top_init)
    if hn is None:
        fx = RR.expect_fwd128(R, T, d['lengths'], perm, rev, True)      # what the forward leaves unwritten the BPTT must not read
        st = RR.to_pos(d['st32'], perm, 1).copy()
        st[1:][fx['HN'][1:] != LIVE] = NAN
        g16 = RR.to_pos(d['g16'], perm, 2).copy()
        g16.transpose(0, 2, 1, 3)[fx['gates'] != LIVE] = NAN
        hn, gates = dev(st), dev(RR.gates_blocked(g16, H), BF)
    dl = d['dl'] if wide else np.ascontiguousarray(d['dh_last'])
    ins = dict(wt=pack(d['w_hh'].T, True), hn=hn, gates=gates, dl=dev(dl), lengths=dev(d['lengths']), perm=dev(perm))
    dlv = ins['dl'][:, H:] if wide and rev else ins['dl']
    dgi, dgiw = out_buf((T, R, 3 * H), BF)
    dgh, dghw = out_buf((T, R, 3 * H), BF)
    dh0, dh0w = out_buf((R, H))
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    scratch = torch.zeros(lib().ptv_row_gru_persist_scratch_elems(H, R), dtype=BF, device=DEV)
    top = int_dev(top_init) if top_given else None
    before = {k: raw(v) for k, v in ins.items() if v is not None}
    a = ('ptv_row_gru_persist_bwd_perm' if perm is not None else 'ptv_row_gru_persist_bwd', H, ins['wt'], hn, gates, None, dlv, 2 * H if wide else H,
         ins['lengths']) + ((ins['perm'],) if perm is not None else ()) + (dgi, dgh, dh0 if want_dh0 else None, scratch, R, T, int(rev), top)
    with zero_skip(1):
        assert K.leaf_rc(*a) == 0
        torch.cuda.synchronize()
    assert all(raw(v) == before[k] for k, v in ins.items() if v is not None), 'an input was written'
    assert pads_kept(dgiw, (T, R, 3 * H)) and pads_kept(dghw, (T, R, 3 * H)) and pads_kept(dh0w, (R, H))
    rdgi, rdgh, rdh0, kdgi, kdgh, kdh0 = refs or (d['dgi'], d['dgh'], d['dh0'], d['kdgi'], d['kdgh'], d['kdh0'])
    check_slots(family + ' dgi', host(dgi), rdgi, kdgi, ex['dgi'])
    check_slots(family + ' dgh', host(dgh), RR.to_pos(rdgh, perm, 1), RR.to_pos(kdgh, perm, 1), ex['dgh'])
    if want_dh0:
        check(family + ' dh0', host(dh0), rdh0, kdh0)
        if d['lengths'] is not None:                                     # an empty row's final state IS h0
            e = d['lengths'] <= 0
            assert np.array_equal(bits(host(dh0)[e]), bits(d['dh_last'][e])), 'dh0 of a row of length 0 is its dh_last'
    else:
        assert (bits(host(dh0)) == bits(SENT)).all()
    if top_given:
        assert int(top.item()) == ex['top'], 'top_step %d, expected %d' % (int(top.item()), ex['top'])


@pytest.mark.parametrize('i,key', list(enumerate(CASES128)), ids=lambda v: cid(v) if isinstance(v, tuple) else str(v))
def test_row_gru_h128_bptt(i, key):
    """ptv_row_gru_persist_bwd / _bwd_perm, H = 128, on the reference's states (fp32) and gates (bf16, unit-blocked by 32, NaN where the
    forward leaves them unwritten): dgi by (time, row perm[p]), dgh by (step, position), dh0 (no perm), top_step given (initial -1 or
    T + 5) or NULL, dh_last with last_ld = H or 2H"""
    c = dict(key)
    run_bwd128(c, case128(key), i)


def test_row_gru_h128_forward_then_bptt_end_to_end():
    """the chained pair: the BPTT on the forward kernel's own HN and gates, against the fp64 chain with nothing rounded in between"""
    key = C(R=130, T=5, lens='mixed', reverse=True, wide=True)
    c, d = dict(key), case128(key)
    T, R, H = c['T'], c['R'], H1
    g = run_fwd128(c, d)
    gates = dev(RR.gates_blocked(g['gates'], H), BF)
    run_bwd128(c, d, 1, hn=dev(g['HN']), gates=gates, refs=d['e2e'] + d['ke2e'], family='chain128')


# ================================================================================================ H = 512: the notes GRU
H5 = 512
# entry: 'plain' / 'top' / 'rows'; live_top; rl: row_len given (rowgru_ref.row_len_of); nofill: T bit 24 (forward) / bit 16 (BPTT)
FWD512 = [
    C(R=1, T=1, sharp=True),
    C(R=63, T=2, entry='top', live_top=-1),
    C(R=64, T=5, entry='top', live_top=0),
    C(R=65, T=5, entry='top', live_top=3),
    C(R=96, T=2, entry='top', live_top=1),
    C(R=96, T=5, entry='top', live_top=8),
    C(R=130, T=5, entry='rows', live_top=3, rl=True),
    C(R=130, T=2, entry='rows', rl=True, nofill=True),
    C(R=200, T=5, entry='rows', live_top=8, rl=True, nofill=True),
    C(R=200, T=1, entry='rows', live_top=0, rl=True),
    C(R=200, T=15),
    C(R=2176, T=2),
    C(R=2182, T=2, entry='top', live_top=1),
]
# ext: 'dense' / ('zero', k) / ('negzero', k): nothing arrives from step k on, nor at rows 64.. of step k - 1
BWD512 = [
    C(R=1, T=1, dh0=True),
    C(R=63, T=2, ext=('zero', 1), top=-1),
    C(R=64, T=5, entry='top', bound=3, dh0=True, top=-1),
    C(R=65, T=5, entry='top', bound=9, ext=('negzero', 2), top=10),
    C(R=96, T=2, entry='top', bound=-1, dh0=True, top=-1),
    C(R=130, T=5, entry='rows', bound=3, rl=True, top=-1, dh0=True),
    C(R=130, T=2, entry='rows', bound=1, rl=True, nofill=True, top=-1),
    C(R=200, T=5, entry='rows', bound=4, rl=True, nofill=True, ext=('zero', 3), top=10),
    C(R=200, T=1, entry='rows', bound=0, rl=True, top=-1, dh0=True),
    C(R=200, T=15, ext=('zero', 7), dh0=True, top=-1),
    C(R=2176, T=2, dh0=True),
    C(R=2182, T=2, entry='top', bound=1, top=-1),
]
SKIP512 = [C(R=63, T=2, ext=('zero', 1), top=-1), C(R=200, T=5, ext=('negzero', 3), top=-1, dh0=True)]


@functools.lru_cache(maxsize=8)
def base512(R, T, sharp):
    """inputs and the dense forward (reference and kernel precision) of one (R, T)"""
    H = H5
    rng = np.random.RandomState(seed_of(('base512', R, T, sharp)))
    k = 1.0 / np.sqrt(H)
    U = lambda *s: RR.bf16_round(rng.uniform(-k, k, s))
    d = dict(w_tok=U(3 * H, E), w_hh=U(3 * H, H), b_hh=rng.uniform(-k, k, 3 * H).astype(np.float32), gc=RR.bf16_round(rng.randn(R, 3 * H) * 0.5),
             emb=RR.bf16_round(rng.randn(T, R, E) * 0.5), h0=(rng.randn(R, H) * 0.5).astype(np.float32), ext=RR.bf16_round(rng.randn(T, R, H) * 0.1))
    if sharp:
        d['h0'] = RR.bf16_round(d['h0'])
    args = (H, d['emb'], d['w_tok'], d['w_hh'], d['b_hh'], d['h0'])
    d['st'], d['gates'] = RR.forward(*args, gc=d['gc'])
    d['kst'], d['kgates'], d['kst16'] = RR.kp_forward(*args, gc=d['gc'])
    return d


def run_fwd512(c, d):
    R, T, H = c['R'], c['T'], H5
    entry, lt, nofill = c.get('entry', 'plain'), c.get('live_top'), bool(c.get('nofill'))
    rl = RR.row_len_of(R, T) if c.get('rl') else None
    ex = RR.expect_fwd512(R, T, lt, rl, nofill)
    emb = d['emb'].copy()
    for s in range(1, T):                                                # (step 0's tokens are staged by every panel)
        emb[s, ex['steps'] <= s] = NAN
    ins = dict(wh=pack(d['w_hh'], False), wt=pack(d['w_tok'], False), b_hh=dev(d['b_hh']), gc=dev(RR.gc_blocked(d['gc']), BF), emb=dev(emb), h0=dev(d['h0']),
               lt=int_dev(lt), rl=dev(rl))
    HN16, HN16w = out_buf((T + 1, R, H), BF)
    gates, gatesw = out_buf((T, 4, H // 16, R, 16), BF)
    before = {k: raw(v) for k, v in ins.items() if v is not None}
    a = (ins['wh'], ins['wt'], ins['b_hh'], ins['gc'], ins['emb'], ins['h0'], HN16, gates, R, T | (BIT24 if nofill else 0))
    if entry == 'plain':
        rc = K.leaf_rc('ptv_notes_gru_persist_fwd', *a)
    elif entry == 'top':
        rc = K.leaf_rc('ptv_notes_gru_persist_fwd_top', *a, ins['lt'])
    else:
        rc = K.leaf_rc('ptv_notes_gru_persist_fwd_rows', *a, ins['lt'], ins['rl'])
    assert rc == 0
    torch.cuda.synchronize()
    assert all(raw(v) == before[k] for k, v in ins.items() if v is not None), 'an input was written'
    assert pads_kept(HN16w, (T + 1, R, H)) and pads_kept(gatesw, (T, 4, R, H))
    g = dict(HN16=host(HN16), gates=RR.gates_unblocked(host(gates), H), ex=ex, HN16_t=HN16, gates_t=gates)
    assert np.array_equal(bits(g['HN16'][0]), bits(RR.bf16_round(d['h0']))), 'HN16 slot 0 = RNE(h0)'
    return g


@pytest.mark.parametrize('key', FWD512, ids=cid)
def test_notes_gru_forward(key):
    """ptv_notes_gru_persist_fwd / _fwd_top (live_top in {-1, 0, T-2, T-1, T+3}) / _fwd_rows (with and without T bit 24): every bf16
    state and the gate planes (unit-blocked by 16) against the fp64 reference; slots beyond the limits zero / untouched as predicted"""
    c = dict(key)
    d = base512(c['R'], c['T'], bool(c.get('sharp')))
    g = run_fwd512(c, d)
    check_slots('fwd512 HN16', g['HN16'], d['st'], d['kst16'], g['ex']['HN16'])
    for q, nm in enumerate(('r', 'z', 'n', 'hn')):
        check_slots('fwd512 gate %s' % nm, g['gates'][:, q], d['gates'][:, q], d['kgates'][:, q], g['ex']['gates'])


def ext_of(c, d):
    """the arriving gradient of a BPTT case as the caller holds it: zero (or -0.0) where the case says nothing arrives"""
    ext = d['ext'].copy()
    kind = c.get('ext', 'dense')
    if kind != 'dense':
        z = np.float32(-0.0 if kind[0] == 'negzero' else 0.0)
        ext[kind[1]:] = z
        if kind[1] > 0:
            ext[kind[1] - 1, 64:] = z
    return ext


@functools.lru_cache(maxsize=8)
def bwd512_case(key, skip=True):
    c = dict(key)
    R, T, H = c['R'], c['T'], H5
    d = base512(R, T, False)
    rl = RR.row_len_of(R, T) if c.get('rl') else None
    ext = ext_of(c, d)
    top_given = 'top' in c
    ex = RR.expect_bwd512(R, T, ext, skip, c.get('bound'), rl, bool(c.get('nofill')), top_given, c.get('top', -1))
    if skip:                                                             # what is not read holds NaN
        for s in range(T):
            dead = ex['last'] < s
            if c.get('bound') is not None and s > c['bound']:
                ext[s] = NAN
            elif rl is not None:
                blockdead = np.repeat([rl[a & ~127] - 1 < s for a, _ in RR.panels(R)], 64)[:R]
                ext[s, blockdead & dead] = NAN
    ext_eff = RR.ext_as_read(np.nan_to_num(ext, nan=0.0), ex['last'])
    st16, g16 = RR.bf16_round(d['st']), RR.bf16_round(d['gates'])
    o = dict(d=d, ex=ex, rl=rl, ext=ext, st16=st16, g16=g16)
    o['ref'] = RR.backward(H, st16[:T], g16, d['w_hh'], ext_eff)
    o['kp'] = RR.kp_backward(H, st16[:T], g16, d['w_hh'], ext_eff)
    return o


def run_bwd512(c, o, eight, skip=True, hn16=None, gates=None, refs=None, family=None):
    R, T, H = c['R'], c['T'], H5
    d, ex, rl = o['d'], o['ex'], o['rl']
    entry, nofill, top_given = c.get('entry', 'plain'), bool(c.get('nofill')), 'top' in c
    family = family or ('bwd512 %d-wave' % (8 if eight else 4))
    if hn16 is None:
        st16, g16 = o['st16'].copy(), o['g16'].copy()
        if skip:
            for s in range(T):
                st16[s][ex['last'] < s] = NAN                           # (slot s is the previous state of step s)
                g16[s][:, ex['last'] < s] = NAN
            st16[T] = NAN                                                # the final state is nobody's previous state
        hn16, gates = dev(st16, BF), dev(RR.gates_blocked(g16, H), BF)
    ins = dict(wt=pack(d['w_hh'].T, True), hn16=hn16, gates=gates, ext=dev(RR.ext_blocked(o['ext']), BF), bound=int_dev(c.get('bound')), rl=dev(rl))
    dgi, dgiw = out_buf((T, R, 3 * H), BF)
    dgh, dghw = out_buf((T, R, H), BF)
    dh0, dh0w = out_buf((R, H))
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    scratch = torch.zeros(lib().ptv_notes_gru_persist_scratch_elems(R), dtype=BF, device=DEV)
    top = int_dev(c['top']) if top_given else None
    before = {k: raw(v) for k, v in ins.items() if v is not None}
    a = (ins['wt'], hn16, gates, ins['ext'], dgi, dgh, dh0 if c.get('dh0') else None, scratch, R, T | (BIT16 if nofill else 0))
    with zero_skip(skip), bwd_variant(eight):
        if entry == 'plain':
            rc = K.leaf_rc('ptv_notes_gru_persist_bwd', *a, top)
        elif entry == 'top':
            rc = K.leaf_rc('ptv_notes_gru_persist_bwd_top', *a, ins['bound'], top)
        else:
            rc = K.leaf_rc('ptv_notes_gru_persist_bwd_rows', *a, ins['bound'], ins['rl'], top)
        assert rc == 0
        torch.cuda.synchronize()
    assert all(raw(v) == before[k] for k, v in ins.items() if v is not None), 'an input was written'
    assert pads_kept(dgiw, (T, R, 3 * H)) and pads_kept(dghw, (T, R, H)) and pads_kept(dh0w, (R, H))
    (rdgi, rdgh, rdh0), (kdgi, kdgh, kdh0) = refs or (o['ref'], o['kp'])
    g = dict(dgi=host(dgi), dgh=host(dgh), dh0=host(dh0))
    check_slots(family + ' dgi', g['dgi'], rdgi, kdgi, ex['dgi'])
    check_slots(family + ' dgh', g['dgh'], rdgh, kdgh, ex['dgh'])
    if c.get('dh0'):
        check(family + ' dh0', g['dh0'], rdh0, kdh0)
    else:
        assert (bits(g['dh0']) == bits(SENT)).all()
    if top_given:
        assert int(top.item()) == ex['top'], 'top_step %d, expected %d' % (int(top.item()), ex['top'])
    return g


@pytest.mark.parametrize('eight', [1, 0], ids=['8-wave', '4-wave'])
@pytest.mark.parametrize('key', BWD512, ids=cid)
def test_notes_gru_bptt(key, eight):
    """ptv_notes_gru_persist_bwd / _bwd_top / _bwd_rows (with and without T bit 16) under both values of ptv_notes_bwd_variant, on the
    reference's bf16 states and gates (unit-blocked by 16) and an arriving gradient column-blocked by 32: dgi, the n third of dgh, dh0
    given / NULL, top_step from initial -1 and T + 5; ext zero or -0.0 from a step on; NaN wherever the contract says nothing is read"""
    c = dict(key)
    run_bwd512(c, bwd512_case(key), eight)


@pytest.mark.parametrize('eight', [1, 0], ids=['8-wave', '4-wave'])
@pytest.mark.parametrize('key', SKIP512, ids=cid)
def test_notes_gru_bptt_zero_skip_off(key, eight):
    """ptv_zero_skip(0) computes every step: held to the reference by itself, and bit-identical to the skipping run on that run's LIVE
    slots (skipping only removes exact-zero work)"""
    c = dict(key)
    g0 = run_bwd512(c, bwd512_case(key, False), eight, skip=False)
    o1 = bwd512_case(key, True)
    g1 = run_bwd512(c, o1, eight)
    assert (o1['ex']['dgi'] != LIVE).any()
    for nm in ('dgi', 'dgh'):
        w = o1['ex'][nm] == LIVE
        assert np.array_equal(bits(g0[nm][w]), bits(g1[nm][w])), nm
    if c.get('dh0'):
        assert np.array_equal(bits(g0['dh0']), bits(g1['dh0']))


@pytest.mark.parametrize('eight', [1, 0], ids=['8-wave', '4-wave'])
def test_notes_gru_forward_then_bptt_end_to_end(eight):
    """the chained pair: the BPTT on the forward kernel's own HN16 and gate planes, against the fp64 chain with nothing rounded in
    between (the kernel-precision chain rounds where the kernels store)"""
    key = C(R=130, T=5, dh0=True)
    c = dict(key)
    d = base512(130, 5, False)
    g = run_fwd512(dict(R=130, T=5), d)
    o = dict(bwd512_case(key))
    T, H = 5, H5
    refs = (RR.backward(H, d['st'][:T], d['gates'], d['w_hh'], o['ext']), RR.kp_backward(H, d['kst16'][:T], d['kgates'], d['w_hh'], o['ext']))
    run_bwd512(c, o, eight, hn16=g['HN16_t'], gates=g['gates_t'], refs=refs, family='chain512 %d-wave' % (8 if eight else 4))


# ================================================================================================ refusals
def small128():
    """a valid H = 128 forward / BPTT argument set on small sentinel-filled buffers (R = 65, T = 2)"""
    R, T, H = 65, 2, H1
    f = lambda *s: torch.zeros(*s, device=DEV)
    outs = dict(HN=out_buf((T + 1, R, H))[0], HN16=out_buf((T + 1, R, H), BF)[0], gates=out_buf((T, 4, R, H), BF)[0], out=out_buf((R, 2 * H))[0],
                dgi=out_buf((T, R, 3 * H), BF)[0], dgh=out_buf((T, R, 3 * H), BF)[0], dh0=out_buf((R, H))[0])
    ins = dict(wh=f(3 * H * H // 2).to(BF), wx=f(3 * H * E // 2).to(BF), b=f(3 * H), x=f(T, R, E + 4), lengths=torch.ones(R, dtype=torch.int32, device=DEV),
               perm=torch.arange(R, dtype=torch.int32, device=DEV), dl=f(R, 2 * H), scratch=f(2 * 2 * 3 * H * 64).to(BF), gc=f(R, 3 * H).to(BF),
               top=int_dev(-1))
    return R, T, H, ins, outs


def refused(outs, rc):
    assert rc != 0
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == float(SENT)).all()), 'a refused call wrote %s' % k


def test_row_gru_h128_refusals():
    """every documented PTV_ERR_ARG / PTV_ERR_UNSUPPORTED condition of ptv_row_gru_persist_{fwd,bwd}{,_perm} (each check sits ahead of
    every launch in the source): a non-zero status and untouched outputs"""
    R, T, H, i, o = small128()

    def fwd(**kw):
        a = dict(H=H, wh=i['wh'], wx=i['wx'], b_hh=i['b'], b_ih=i['b'], gc=None, x=i['x'], x_step=R * (E + 4), lengths=i['lengths'], perm=i['perm'],
                 HN=o['HN'], HN16=o['HN16'], gates=o['gates'], out=o['out'], out_ld=2 * H, R=R, T=T, reverse=0)
        a.update(kw)
        name = 'ptv_row_gru_persist_fwd_perm' if a['perm'] is not None else 'ptv_row_gru_persist_fwd'
        mid = (a['perm'],) if name.endswith('perm') else ()
        return K.leaf_rc(name, a['H'], a['wh'], a['wx'], a['b_hh'], a['b_ih'], a['gc'], a['x'], a['x_step'], a['lengths'], *mid, a['HN'], a['HN16'], a['gates'],
                         a['out'], a['out_ld'], a['R'], a['T'], a['reverse'])

    def bwd(**kw):
        a = dict(H=H, wt=i['wh'], HN=o['HN'], gates=o['gates'], ext=None, dl=i['dl'], last_ld=2 * H, lengths=i['lengths'], perm=None, dgi=o['dgi'], dgh=o['dgh'],
                 dh0=None, scratch=i['scratch'], R=R, T=T, reverse=0, top=i['top'])
        a.update(kw)
        name = 'ptv_row_gru_persist_bwd_perm' if a['perm'] is not None else 'ptv_row_gru_persist_bwd'
        mid = (a['perm'],) if name.endswith('perm') else ()
        return K.leaf_rc(name, a['H'], a['wt'], a['HN'], a['gates'], a['ext'], a['dl'], a['last_ld'], a['lengths'], *mid, a['dgi'], a['dgh'], a['dh0'],
                         a['scratch'], a['R'], a['T'], a['reverse'], a['top'])

    x1 = i['x'].view(-1)[1:]                                             # 4 bytes off a 16-byte boundary
    bad_fwd = [dict(wh=None), dict(wx=None), dict(b_hh=None), dict(x=None), dict(HN=None), dict(HN16=None), dict(b_ih=None), dict(gc=i['gc']),
               dict(H=64), dict(H=256), dict(R=0), dict(T=0), dict(T=0x100), dict(T=T | 0x100), dict(T=T | BIT24), dict(out_ld=2 * H + 2),
               dict(x_step=R * (E + 4) + 2), dict(x=x1), dict(HN=o['HN'].view(-1)[1:]), dict(out=o['out'].view(-1)[1:]), dict(R=1 << 31),
               dict(perm=None, wh=None), dict(perm=None, T=T | 0x800), dict(perm=None, H=512)]
    for kw in bad_fwd:
        refused(o, fwd(**kw))
    bad_bwd = [dict(wt=None), dict(HN=None), dict(gates=None), dict(dgi=None), dict(dgh=None), dict(scratch=None), dict(H=100), dict(R=0), dict(T=0),
               dict(T=0x100), dict(T=T | 0x100), dict(T=T | BIT16), dict(last_ld=2 * H + 1), dict(ext=i['gc']), dict(perm=i['perm'], dh0=o['dh0']),
               dict(HN=o['HN'].view(-1)[1:]), dict(R=1 << 31), dict(perm=i['perm'], wt=None), dict(perm=i['perm'], T=0)]
    for kw in bad_bwd:
        refused(o, bwd(**kw))


def test_notes_gru_refusals():
    """the same for the H = 512 entry points, under both BPTT variants: NULL operands, a step count of 0 (T = 0 and T = flags only), the
    H = 512 instance of ptv_row_gru_persist_fwd given b_ih / lengths / perm / reverse / out, the BPTT given lengths / dh_last / reverse,
    bound without top_step, row_len without bound, and R above each kernel's 32-bit addressing limit (refused on small buffers)"""
    R, T, H = 65, 2, H5
    f = lambda *s: torch.zeros(*s, device=DEV)
    o = dict(HN16=out_buf((T + 1, R, H), BF)[0], gates=out_buf((T, 4, R, H), BF)[0], dgi=out_buf((T, R, 3 * H), BF)[0], dgh=out_buf((T, R, H), BF)[0],
             dh0=out_buf((R, H))[0], out=out_buf((R, H))[0])
    i = dict(wh=f(3 * H * H // 2).to(BF), wt=f(3 * H * E // 2).to(BF), b=f(3 * H), gc=f(R, 3 * H).to(BF), emb=f(T, R, E), h0=f(R, H), ext=f(T, R, H).to(BF),
             scratch=f(2 * 2 * 3 * H * 64).to(BF), n=int_dev(1), rl=torch.full((R,), T, dtype=torch.int32, device=DEV), top=int_dev(-1))

    def fwd(entry='rows', **kw):
        a = dict(wh=i['wh'], wt=i['wt'], b=i['b'], gc=i['gc'], emb=i['emb'], h0=i['h0'], HN16=o['HN16'], gates=o['gates'], R=R, T=T, lt=i['n'], rl=i['rl'])
        a.update(kw)
        tail = {'plain': (), 'top': (a['lt'],), 'rows': (a['lt'], a['rl'])}[entry]
        return K.leaf_rc('ptv_notes_gru_persist_fwd' + {'plain': '', 'top': '_top', 'rows': '_rows'}[entry], a['wh'], a['wt'], a['b'], a['gc'], a['emb'], a['h0'],
                         a['HN16'], a['gates'], a['R'], a['T'], *tail)

    def bwd(entry='rows', **kw):
        a = dict(wt=i['wh'], HN16=o['HN16'], gates=o['gates'], ext=i['ext'], dgi=o['dgi'], dgh=o['dgh'], dh0=o['dh0'], scratch=i['scratch'], R=R, T=T,
                 bound=i['n'], rl=i['rl'], top=i['top'])
        a.update(kw)
        tail = {'plain': (a['top'],), 'top': (a['bound'], a['top']), 'rows': (a['bound'], a['rl'], a['top'])}[entry]
        return K.leaf_rc('ptv_notes_gru_persist_bwd' + {'plain': '', 'top': '_top', 'rows': '_rows'}[entry], a['wt'], a['HN16'], a['gates'], a['ext'], a['dgi'],
                         a['dgh'], a['dh0'], a['scratch'], a['R'], a['T'], *tail)

    for entry in ('plain', 'top', 'rows'):
        for kw in (dict(wh=None), dict(wt=None), dict(b=None), dict(gc=None), dict(emb=None), dict(h0=None), dict(HN16=None), dict(R=0), dict(T=0),
                   dict(T=0x800), dict(T=BIT24), dict(R=1048576)):
            refused(o, fwd(entry, **kw))
    # the H = 512 instance behind the generic entry point
    g = lambda **kw: K.leaf_rc('ptv_row_gru_persist_fwd_perm', 512, i['wh'], i['wt'], i['b'], kw.get('b_ih'), kw.get('gc', i['gc']), i['emb'], kw.get('x_step', R * E),
                               kw.get('lengths'), kw.get('perm'), i['h0'], o['HN16'], o['gates'], kw.get('out'), H, R, T, kw.get('reverse', 0))
    for kw in (dict(b_ih=i['b']), dict(lengths=i['rl']), dict(perm=i['rl']), dict(reverse=1), dict(out=o['out']), dict(gc=None), dict(x_step=R * E + 4)):
        refused(o, g(**kw))
    for eight in (1, 0):
        with bwd_variant(eight):
            for entry in ('plain', 'top', 'rows'):
                for kw in (dict(wt=None), dict(HN16=None), dict(gates=None), dict(ext=None), dict(dgi=None), dict(dgh=None), dict(scratch=None), dict(R=0),
                           dict(T=0), dict(T=0x400), dict(T=BIT16)):
                    refused(o, bwd(entry, **kw))
            refused(o, bwd('top', top=None))                             # bound without top_step
            refused(o, bwd('rows', top=None))
            refused(o, bwd('rows', bound=None))                          # row_len without bound
            refused(o, bwd('rows', R=1 << 31))
            b = lambda **kw: K.leaf_rc('ptv_row_gru_persist_bwd_perm', 512, i['wh'], o['HN16'], o['gates'], kw.get('ext', i['ext']), kw.get('dl'), H, kw.get('lengths'),
                                       kw.get('perm'), o['dgi'], o['dgh'], o['dh0'], i['scratch'], R, kw.get('T', T), kw.get('reverse', 0), i['top'])
            for kw in (dict(ext=None), dict(dl=i['h0']), dict(lengths=i['rl']), dict(perm=i['rl']), dict(reverse=1), dict(T=0x100)):
                refused(o, b(**kw))
    # the 8-wave BPTT's limits: R * 3072 bytes within one descriptor, and the 32-bit offset into ext
    for kw in (dict(R=699051), dict(R=16453, T=255), dict(R=280791, T=15)):
        refused(o, bwd('plain', **kw))
