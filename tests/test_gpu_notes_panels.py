"""The two panel heights of the notes GRU kernels (csrc/notes_roles.hip: notes_fwd_kernel<15, 0, ROWS> and notes_bwd_kernel<0, ROWS>,
ROWS = 64 / 32) behind ptv_notes_gru_persist_{fwd,bwd}{,_top,_rows}: forward T bits 25-26, BPTT T bits 17-18 (0 = 64 rows, 1 = 32 rows,
2 = the library's rule).

(i) forced 32 against forced 64 on identical inputs: rows are independent and every row's products accumulate over k in one fixed order,
so every element both variants compute is BYTE-equal -- HN16, the four gate planes, dgi, dgh, dh0, top_step.  Deadness is per 128-row
block at both heights, so the forward writes, zero-fills and leaves untouched exactly the same slots: whole buffers compare as bytes.
The BPTT's last-gradient scan is per panel: a 32-row panel may write zero rows where the 64-row panel around it computes -- those slots
must be zero as numbers (either sign) -- and what one variant leaves untouched (the sentinel) the other leaves untouched.
(ii) forced 32 against the fp64 reference by the method of test_gpu_rowgru_kernels.py (its builders, bounds and slot classes, with
rowgru_ref's panel height set to 32 for the predictions): error at most 4x the kernel-precision CPU evaluation, floor 8 ulps, per step
plane; NaN wherever the 32-row contract says nothing is read; inputs unchanged; pad rows keep the sentinel.
(iii) one train step of the model at B = 4 with the composites' "library's rule" answering 64, then 32 (the rule's own answer there):
losses and every parameter gradient byte-equal.

ext ('zero32', k): nothing arrives from step k on, nor at step k - 1 for the second 32 rows of every 64-row span -- the two 32-row
panels of a span disagree about their last live step."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import kernel_ops as K
import rowgru_ref as RR
import test_gpu_rowgru_kernels as TK
from rowgru_ref import LIVE, ZERO
from test_gpu_rowgru_kernels import BF, BIT16, BIT24, C, DEV, H5, NAN, SENT, bits, cid, dev, host, int_dev, out_buf, pack, pads_kept, raw

pytestmark = pytest.mark.gpu
FWD_ROWS = {64: 0, 32: 1 << 25}
BWD_ROWS = {64: 0, 32: 1 << 17}


@contextlib.contextmanager
def panel_height(n):
    """rowgru_ref's predictions (panels()) for panels of n rows"""
    old = RR.PANEL
    RR.PANEL = n
    try:
        yield
    finally:
        RR.PANEL = old


# ================================================================================================ forward
FWD = [
    C(R=1, T=1, sharp=True),
    C(R=31, T=2, entry='top', live_top=-1),
    C(R=32, T=5, entry='top', live_top=0),
    C(R=33, T=5, entry='top', live_top=3),
    C(R=64, T=1),
    C(R=64, T=5, entry='rows', live_top=4, rl=True),
    C(R=65, T=2, entry='rows', live_top=1, rl=True, nofill=True),
    C(R=96, T=5, entry='top', live_top=8),
    C(R=130, T=5, entry='rows', live_top=3, rl=True),
    C(R=130, T=2, entry='rows', live_top=1, rl=True, nofill=True),
    C(R=200, T=5, entry='rows', live_top=4, rl=True, nofill=True),
    C(R=200, T=1, entry='rows', live_top=0, rl=True),
    C(R=200, T=15),
    C(R=2176, T=2),
    C(R=2182, T=2, entry='top', live_top=1),
]


def run_fwd(c, d, rows):
    """one forward call at panel height `rows` on sentinel-filled outputs; inputs the contract says are not read hold NaN"""
    R, T, H = c['R'], c['T'], H5
    entry, lt, nofill = c.get('entry', 'plain'), c.get('live_top'), bool(c.get('nofill'))
    rl = RR.row_len_of(R, T) if c.get('rl') else None
    ex = RR.expect_fwd512(R, T, lt, rl, nofill)                          # (deadness is per 128-row block: the same at both heights)
    emb = d['emb'].copy()
    for s in range(1, T):
        emb[s, ex['steps'] <= s] = NAN
    ins = dict(wh=pack(d['w_hh'], False), wt=pack(d['w_tok'], False), b_hh=dev(d['b_hh']), gc=dev(RR.gc_blocked(d['gc']), BF), emb=dev(emb), h0=dev(d['h0']),
               lt=int_dev(lt), rl=dev(rl))
    HN16, HN16w = out_buf((T + 1, R, H), BF)
    gates, gatesw = out_buf((T, 4, H // 16, R, 16), BF)
    before = {k: raw(v) for k, v in ins.items() if v is not None}
    a = (ins['wh'], ins['wt'], ins['b_hh'], ins['gc'], ins['emb'], ins['h0'], HN16, gates, R, T | (BIT24 if nofill else 0) | FWD_ROWS[rows])
    tail = {'plain': (), 'top': (ins['lt'],), 'rows': (ins['lt'], ins['rl'])}[entry]
    rc = K.leaf_rc('ptv_notes_gru_persist_fwd' + {'plain': '', 'top': '_top', 'rows': '_rows'}[entry], *a, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(raw(v) == before[k] for k, v in ins.items() if v is not None), 'an input was written'
    assert pads_kept(HN16w, (T + 1, R, H)) and pads_kept(gatesw, (T, 4, R, H))
    return dict(HN16=host(HN16), gates=RR.gates_unblocked(host(gates), H), ex=ex, raw=(raw(HN16), raw(gates)))


@functools.lru_cache(maxsize=32)
def fwd_runs(key):
    c = dict(key)
    d = TK.base512(c['R'], c['T'], bool(c.get('sharp')))
    return d, run_fwd(c, d, 64), run_fwd(c, d, 32)


@pytest.mark.parametrize('key', FWD, ids=cid)
def test_forward_32_rows_equals_64_rows(key):
    """HN16 and the gate planes, sentinel-filled: the two heights leave the same bytes in every slot -- computed, zero-filled, untouched"""
    _, g64, g32 = fwd_runs(key)
    assert g64['raw'][0] == g32['raw'][0], 'HN16'
    assert g64['raw'][1] == g32['raw'][1], 'gate planes'


@pytest.mark.parametrize('key', FWD, ids=cid)
def test_forward_32_rows_against_fp64(key):
    d, _, g = fwd_runs(key)
    assert np.array_equal(bits(g['HN16'][0]), bits(RR.bf16_round(d['h0']))), 'HN16 slot 0 = RNE(h0)'
    TK.check_slots('fwd512/32 HN16', g['HN16'], d['st'], d['kst16'], g['ex']['HN16'])
    for q, nm in enumerate(('r', 'z', 'n', 'hn')):
        TK.check_slots('fwd512/32 gate %s' % nm, g['gates'][:, q], d['gates'][:, q], d['kgates'][:, q], g['ex']['gates'])


# ================================================================================================ BPTT
BWD = [
    C(R=1, T=1, dh0=True),
    C(R=31, T=2, ext=('zero32', 1), top=-1),
    C(R=32, T=5, entry='top', bound=3, dh0=True, top=-1),
    C(R=33, T=5, entry='top', bound=9, ext=('zero32', 2), top=10),
    C(R=64, T=2, ext=('zero32', 2), dh0=True, top=-1),
    C(R=64, T=5, ext=('zero32', 3), split=True),
    C(R=65, T=1, entry='top', bound=0, top=-1),
    C(R=96, T=2, entry='top', bound=-1, dh0=True, top=-1),
    C(R=96, T=5, ext=('zero32', 4), dh0=True, top=-1, split=True),
    C(R=130, T=5, entry='rows', bound=3, rl=True, top=-1, dh0=True),
    C(R=130, T=2, entry='rows', bound=1, rl=True, nofill=True, top=-1),
    C(R=200, T=5, entry='rows', bound=4, rl=True, nofill=True, ext=('zero32', 3), top=10),
    C(R=200, T=5, entry='rows', bound=4, rl=True, ext=('zero32', 3), top=-1, dh0=True),
    C(R=200, T=1, entry='rows', bound=0, rl=True, top=-1, dh0=True),
    C(R=200, T=15, ext=('zero32', 7), dh0=True, top=-1, split=True),
    C(R=2176, T=2, dh0=True),
    C(R=2182, T=2, entry='top', bound=1, ext=('zero32', 2), top=-1),
]


def ext_of(c, d):
    ext = d['ext'].copy()
    kind = c.get('ext', 'dense')
    if kind != 'dense':
        k = kind[1]
        ext[k:] = 0.0
        if k > 0:
            ext[k - 1, (np.arange(c['R']) % 64) >= 32] = 0.0
    return ext


def bwd_case(c, d, rows):
    """what a BPTT at panel height `rows` writes (rowgru_ref.expect_bwd512 with that height), the inputs with NaN wherever that kernel does
    not read, and the fp64 / kernel-precision references"""
    R, T, H = c['R'], c['T'], H5
    rl = RR.row_len_of(R, T) if c.get('rl') else None
    ext = ext_of(c, d)
    with panel_height(rows):
        ex = RR.expect_bwd512(R, T, ext, True, c.get('bound'), rl, bool(c.get('nofill')), 'top' in c, c.get('top', -1))
    st16, g16 = RR.bf16_round(d['st']).copy(), RR.bf16_round(d['gates']).copy()
    ext_eff = RR.ext_as_read(ext, ex['last'])
    o = dict(ex=ex, rl=rl, ref=RR.backward(H, st16[:T], g16, d['w_hh'], ext_eff), kp=RR.kp_backward(H, st16[:T], g16, d['w_hh'], ext_eff))
    for s in range(T):
        dead = ex['last'] < s
        if c.get('bound') is not None and s > c['bound']:
            ext[s] = NAN
        elif rl is not None:
            ext[s, (rl[np.arange(R) & ~127] - 1 < s) & dead] = NAN
        st16[s][dead] = NAN                                              # (slot s is the previous state of step s)
        g16[s][:, dead] = NAN
    st16[T] = NAN                                                        # the final state is nobody's previous state
    o.update(ext=ext, st16=st16, g16=g16)
    return o


def run_bwd(c, d, o, rows):
    """one BPTT call at panel height `rows` on the inputs of case `o`, sentinel-filled outputs"""
    R, T, H = c['R'], c['T'], H5
    entry, nofill, top_given = c.get('entry', 'plain'), bool(c.get('nofill')), 'top' in c
    ins = dict(wt=pack(d['w_hh'].T, True), hn16=dev(o['st16'], BF), gates=dev(RR.gates_blocked(o['g16'], H), BF), ext=dev(RR.ext_blocked(o['ext']), BF),
               bound=int_dev(c.get('bound')), rl=dev(o['rl']))
    dgi, dgiw = out_buf((T, R, 3 * H), BF)
    dgh, dghw = out_buf((T, R, H), BF)
    dh0, dh0w = out_buf((R, H))
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    scratch = torch.full((lib().ptv_notes_gru_persist_scratch_elems(R),), float(SENT), dtype=BF, device=DEV)
    top = int_dev(c['top']) if top_given else None
    before = {k: raw(v) for k, v in ins.items() if v is not None}
    a = (ins['wt'], ins['hn16'], ins['gates'], ins['ext'], dgi, dgh, dh0 if c.get('dh0') else None, scratch, R, T | (BIT16 if nofill else 0) | BWD_ROWS[rows])
    tail = {'plain': (top,), 'top': (ins['bound'], top), 'rows': (ins['bound'], ins['rl'], top)}[entry]
    with TK.zero_skip(True), TK.bwd_variant(1):
        rc = K.leaf_rc('ptv_notes_gru_persist_bwd' + {'plain': '', 'top': '_top', 'rows': '_rows'}[entry], *a, *tail)
        assert rc == 0
        torch.cuda.synchronize()
    assert all(raw(v) == before[k] for k, v in ins.items() if v is not None), 'an input was written'
    assert pads_kept(dgiw, (T, R, 3 * H)) and pads_kept(dghw, (T, R, H)) and pads_kept(dh0w, (R, H))
    if rows == 32:
        assert bool((scratch == float(SENT)).all()), 'the 32-row BPTT wrote the scratch ring'
    return dict(dgi=host(dgi), dgh=host(dgh), dh0=host(dh0), top=int(top.item()) if top_given else None)


@functools.lru_cache(maxsize=32)
def bwd_runs(key):
    """-> the 64-row case, both heights on ITS inputs (NaN where the 64-row kernel does not read: the 32-row kernel reads a subset), and
    the 32-row case with its own run"""
    c = dict(key)
    d = TK.base512(c['R'], c['T'], False)
    o64, o32 = bwd_case(c, d, 64), bwd_case(c, d, 32)
    return c, o64, run_bwd(c, d, o64, 64), run_bwd(c, d, o64, 32), o32, run_bwd(c, d, o32, 32)


@pytest.mark.parametrize('key', BWD, ids=cid)
def test_bptt_32_rows_equals_64_rows(key):
    c, o64, g64, g32, o32, _ = bwd_runs(key)
    sent = bits(SENT)
    for nm in ('dgi', 'dgh'):
        b64, b32 = bits(g64[nm]), bits(g32[nm])
        both = ((o64['ex'][nm] == LIVE) & (o32['ex'][nm] == LIVE))[:, :, None]
        assert ((b64 == sent) == (b32 == sent)).all(), '%s: a slot one height leaves untouched, the other writes' % nm
        assert (b64 == b32)[np.broadcast_to(both, b64.shape)].all(), '%s: computed by both heights, different bytes' % nm
        # computed by one (as zeros of either sign), zero-filled by the other; zero-filled / untouched by both
        assert ((b64 == b32) | ((g64[nm] == 0) & (g32[nm] == 0)))[np.broadcast_to(~both, b64.shape)].all(), '%s: zero-filled by one height, not zero in the other' % nm
    assert np.array_equal(bits(g64['dh0']), bits(g32['dh0'])), 'dh0'
    assert g64['top'] == g32['top']
    if c.get('split'):
        assert ((o64['ex']['dgi'] == LIVE) & (o32['ex']['dgi'] == ZERO)).any(), 'the case does not split a 64-row span'


@pytest.mark.parametrize('key', BWD, ids=cid)
def test_bptt_32_rows_against_fp64(key):
    c, _, _, _, o, g = bwd_runs(key)
    (rdgi, rdgh, rdh0), (kdgi, kdgh, kdh0) = o['ref'], o['kp']
    TK.check_slots('bwd512/32 dgi', g['dgi'], rdgi, kdgi, o['ex']['dgi'])
    TK.check_slots('bwd512/32 dgh', g['dgh'], rdgh, kdgh, o['ex']['dgh'])
    if c.get('dh0'):
        TK.check('bwd512/32 dh0', g['dh0'], rdh0, kdh0)
    else:
        assert (bits(g['dh0']) == bits(SENT)).all()
    if 'top' in c:
        assert g['top'] == o['ex']['top'], 'top_step %d, expected %d' % (g['top'], o['ex']['top'])


def test_unknown_height_and_timing_variants_are_refused():
    """bits = 3 is PTV_ERR_ARG; the timing variants (debug bits 8-10, ring depth) exist at 64 rows only"""
    R, T, H = 33, 2, H5
    f = lambda *s: torch.zeros(*s, device=DEV)
    o = dict(HN16=out_buf((T + 1, R, H), BF)[0], gates=out_buf((T, 4, R, H), BF)[0], dgi=out_buf((T, R, 3 * H), BF)[0], dgh=out_buf((T, R, H), BF)[0])
    i = dict(wh=f(3 * H * H // 2).to(BF), wt=f(3 * H * TK.E // 2).to(BF), b=f(3 * H), gc=f(R, 3 * H).to(BF), emb=f(T, R, TK.E), h0=f(R, H), ext=f(T, R, H).to(BF),
             scratch=f(2 * 2 * 3 * H * 64).to(BF))
    fwd = lambda Tw: K.leaf_rc('ptv_notes_gru_persist_fwd', i['wh'], i['wt'], i['b'], i['gc'], i['emb'], i['h0'], o['HN16'], o['gates'], R, Tw)
    bwd = lambda Tw: K.leaf_rc('ptv_notes_gru_persist_bwd', i['wh'], o['HN16'], o['gates'], i['ext'], o['dgi'], o['dgh'], None, i['scratch'], R, Tw, None)
    for rc in (fwd(T | (3 << 25)), fwd(T | (1 << 25) | (1 << 8)), fwd(T | (1 << 25) | (12 << 16)), bwd(T | (3 << 17)), bwd(T | (1 << 17) | (2 << 8))):
        TK.refused(o, rc)


# ================================================================================================ the model
def test_train_step_is_the_same_at_both_heights():
    """loss() + backward() at B = 4 in bf16 through the composites, which pass "the library's rule": answered 64 (debug override), then by
    the rule itself -- 32 rows there (R = 128: 2 panels of 64 rows).  Losses and every parameter gradient byte-equal"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch
    from test_gpu_dead_steps import _model, _step
    assert F_.DEC_COMPOSITE
    x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(4, 99))
    m = _model()
    opt = FusedClipAdam(m.parameters(), lr=1e-3)                 # (the backward composite reads the optimiser's transposed weight shadows)
    res = {}
    try:
        for rows in (64, 0):
            assert lib().ptv_debug_notes_panel_rule(rows) == 0
            res[rows] = _step(m, x, c, pr, 5)
    finally:
        lib().ptv_debug_notes_panel_rule(0)
    del opt
    (l64, g64), (l32, g32) = res[64], res[0]
    for a, b in zip(l64, l32):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (a, b)
    for k in g64:
        assert torch.isfinite(g32[k]).all(), k
        assert torch.equal(g64[k].view(torch.int32), g32[k].view(torch.int32)), (k, (g64[k] - g32[k]).abs().max())
