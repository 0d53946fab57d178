"""The per-step GRU cell kernels of csrc/gru.hip one call at a time -- ptv_gru_seq_fwd, ptv_gru_step_fwd, ptv_gru_seq_bwd, every
dispatch variant (forward F32 / B0 / B-a / B-aw / FAST1 / FAST2, backward F32 / B0 / B-d / B-dw / FAST) on every tile -- against the
plain fp64 references of tests/gru_ref.py, through the C ABI as it is declared (kernel_ops.leaf_rc).

Inputs are built on the CPU from seeded generators and given, the same values, to the kernel and (widened) to the reference.  W_hh is
bf16-representable in bf16 precision, gi / gi2 / dh_ext where they are stored as bf16; the backward gets the REFERENCE's gates and states
rounded to their storage type, never a kernel's forward output.  With T = 1 in bf16 precision the initial state is bf16-representable
too: the product is then exact and the check of the FAST cells is as sharp as that of the fp32 ones.  Every output buffer is pre-filled
with a sentinel and carries 2 pad rows (per plane where the entry point lets planes be strided) that must keep it.

Floating-point outputs have no pre-chosen tolerance: the same formulas are evaluated on the CPU in fp32 with bf16 rounding where the
configuration rounds (gru_ref.kp_*), that evaluation's error against the fp64 reference is measured, and the kernel's error may be at
most 4x that, with a floor of 8 fp32 ulps of the array's scale (check(), the rule of test_gpu_dur_kernels.py).  The bound never sees
the kernel's output.  Each check prints `GRU_RATIO family kernel-error/bound` (pytest -s; table in profiles/LOG.md).  What the design
relies on bit for bit is asserted bit for bit: a masked row copies its state, saves the gates (0, 1, 0), has zero gate gradients and
passes dh on; hall16 is the RNE rounding of hall; the r / z planes of dgi and dgh are the same bits; inputs are not written.

tests/test_gru_ref_host.py asserts, without a GPU, that plan_fwd / plan_bwd put every case below on the variant and tile it names."""
import functools
import zlib

import numpy as np
import pytest
import torch

import gru_ref as R
import kernel_ops as K
from test_gpu_dur_kernels import bound_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = np.float32(np.nan)
SENT = np.float32(768.0)                                               # (exact in bf16)
BF = torch.bfloat16
RATIOS = {}
GATES_BF16, GI_BF16, GI2_BF16, DG_BF16, W_BF16, SKIP_CAST0, EXT_BF16 = 1, 2, 4, 8, 16, 32, 64          # include/ptvae_hip.h
PREC = {'fp32': 0, 'bf16': 1}


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


def check(family, got, ref, kp, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return
    bound, errk = bound_of(ref, kp, scale)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), '%s: non-finite output' % family
    ratio = float(np.where(err == 0, 0.0, err / bound).max())
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print('GRU_RATIO %s %.3f (kernel err %.3e, kernel-precision CPU err %.3e)' % (family, ratio, err.max(), errk))
    assert (err <= bound).all(), '%s: kernel error %.3e over the bound %.3e (kernel-precision CPU evaluation: %.3e)' % (
        family, err.max(), float(np.min(bound)), errk)


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('GRU_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


def C(**kw):
    return tuple(sorted(kw.items()))


def cid(key):
    c = dict(key)
    head = '%s M%d H%d T%d' % (c.pop('cfg'), c.pop('M'), c.pop('H'), c.pop('T'))
    return head + ''.join(' %s' % k if v is True else ' %s=%s' % (k, v) for k, v in sorted(c.items()) if v not in (False, None))


def seed_of(key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


# ================================================================================================ the case lists
# forward configurations -> plan_fwd variant.  gi / gates / gi2: 'f' fp32, 'b' bf16, None absent
FWD_CFG = {
    'F32': dict(prec='fp32', gi='f', gates='f'),
    'F32 gi2': dict(prec='fp32', gi='f', gates='f', gi2='f'),
    'F32 idx': dict(prec='fp32', gi='f', gates=None, gi_idx=True),
    'B0': dict(prec='bf16', gi='f', gates='f'),
    'B0 gi2 idx': dict(prec='bf16', gi='f', gates='f', gi2='f', gi_idx=True),
    'B-a': dict(prec='bf16', hall16=True, gi='f', gates='f'),
    'B-a bf16 store': dict(prec='bf16', hall16=True, gi='b', gates='b', gi2='b'),
    'B-aw gi32': dict(prec='bf16', hall16=True, w16=True, gi='f', gates='b'),
    'B-aw gates32': dict(prec='bf16', hall16=True, w16=True, gi='b', gates='f'),
    'B-aw idx': dict(prec='bf16', hall16=True, w16=True, gi='b', gates='b', gi_idx=True),
    'B-aw gi2 fp32': dict(prec='bf16', hall16=True, w16=True, gi='b', gates='b', gi2='f'),
    'FAST1': dict(prec='bf16', hall16=True, w16=True, gi='b', gates='b'),
    'FAST1 no gates': dict(prec='bf16', hall16=True, w16=True, gi='b', gates=None),
    'FAST2': dict(prec='bf16', hall16=True, w16=True, gi='b', gates='b', gi2='b'),
    'FAST2 no gates': dict(prec='bf16', hall16=True, w16=True, gi='b', gates=None, gi2='b'),
}
FWD_VARIANT_OF = {k: 'F32' if k.startswith('F32') else k.split()[0] for k in FWD_CFG}
# backward configurations -> plan_bwd variant.  ext: None / 'f' / 'b' (EXT_BF16)
BWD_CFG = {
    'F32': dict(prec='fp32'),
    'F32 lr1': dict(prec='fp32', lr_k=1),
    'F32 lr3': dict(prec='fp32', lr_k=3),
    'B0': dict(prec='bf16'),
    'B0 ext16 lr2': dict(prec='bf16', ext='b', lr_k=2, gates16=True),
    'B-d': dict(prec='bf16', dg16=True),
    'B-d gates16': dict(prec='bf16', dg16=True, gates16=True, lr_k=1),
    'B-dw gates32': dict(prec='bf16', dg16=True, w16=True),
    'B-dw lr3': dict(prec='bf16', dg16=True, w16=True, gates16=True, lr_k=3),
    'FAST': dict(prec='bf16', dg16=True, w16=True, gates16=True),
    'FAST lr1': dict(prec='bf16', dg16=True, w16=True, gates16=True, lr_k=1),
    'FAST lr2': dict(prec='bf16', dg16=True, w16=True, gates16=True, lr_k=2),
    'FAST ext16': dict(prec='bf16', dg16=True, w16=True, gates16=True, ext='b'),
    'FAST ext16 lr2': dict(prec='bf16', dg16=True, w16=True, gates16=True, ext='b', lr_k=2),
}
BWD_VARIANT_OF = {k: k.split()[0] for k in BWD_CFG}
SMALL_M = (1, 15, 16, 17, 64, 70)                                      # 70: one full 64-row tile and a ragged one in the same launch
H_ANY, H_FP32_ONLY = (8, 24, 64, 72, 128), (4, 20, 36)                 # H_FP32_ONLY: no bf16 shadow (they need H % 8 == 0)


def fp32_storage(cfg, direction):
    return not (cfg.get('hall16') or cfg.get('w16')) if direction == 'fwd' else not cfg.get('dg16')


def small_cases(direction):
    """the cross product of configurations, M, H and T, thinned: every configuration visits every H of its list, the three hand-over
    values of its precision (on M = 64 and 70: only a full tile takes the pipeline) and, rotating, every M and T"""
    out = []
    for ci, (name, cfg) in enumerate((FWD_CFG if direction == 'fwd' else BWD_CFG).items()):
        hs = [(h, None) for h in H_ANY + (H_FP32_ONLY if fp32_storage(cfg, direction) else ())]
        below, at, above = R.handover_H(direction, '64x32', cfg['prec'])
        hs += [(below, 70), (at, 64), (at, 70), (above, 70)]
        for i, (H, M) in enumerate(hs):
            j = i + ci
            T = (1, 2, 3)[j % 3]
            kw = dict(cfg=name, M=SMALL_M[j % 6] if M is None else M, H=H, T=T, reverse=T == 3 and j % 2 == 0, lengths=j % 2 == 1 or j % 5 == 0)
            if direction == 'fwd':
                kw.update(gi_pad=j % 3 == 1, gi2_bcast=bool(cfg.get('gi2')) and j % 2 == 0)
            else:
                no_ext = cfg.get('ext') is None and j % 4 == 2
                kw.update(ext_pad=j % 3 == 1, last=('dense' if no_ext else None, 'dense', 'pad')[j % 3], no_dh0=j % 4 == 3, no_ext=no_ext,
                          integer=j % 3 == 0)
            out.append(C(**kw))
    return out


# one launch (two for the backward: T = 2) per tile that only a big M reaches, the FAST and the F32 variant; all with ragged M.  The
# (24520, 32), (12230, 32) and (24520, 72) shapes put a K below the hand-over of their tile's pipeline depth on that tile
FWD_TILE_SHAPES = {'64x64': ((3040, 512), (24520, 64), (24520, 32))}
BWD_TILE_SHAPES = {'128x128': ((6100, 512), (24520, 72)), '64x64': ((1500, 512), (12230, 64), (12230, 32))}


def tile_cases(direction):
    out = []
    for tile, shapes in (FWD_TILE_SHAPES if direction == 'fwd' else BWD_TILE_SHAPES).items():
        for M, H in shapes:
            for name in (('FAST2', 'F32 gi2') if direction == 'fwd' else ('FAST lr2', 'F32 lr1')):
                if direction == 'fwd':
                    out.append((tile, C(cfg=name, M=M, H=H, T=1, lengths=True, gi2_bcast=False)))
                else:
                    out.append((tile, C(cfg=name, M=M, H=H, T=2, lengths=True, last='dense')))
    return out


FWD_SMALL, BWD_SMALL = small_cases('fwd'), small_cases('bwd')
FWD_TILES, BWD_TILES = tile_cases('fwd'), tile_cases('bwd')


# ================================================================================================ forward
def lengths_of(M, T):
    """T, T-1, .., 0, T, ..: 0 and T are both there from M = T + 1 on"""
    return ((T - np.arange(M)) % (T + 1)).astype(np.int32)


@functools.lru_cache(maxsize=8)
def fwd_case(key):
    """inputs, fp64 reference and kernel-precision evaluation of one forward case (read only)"""
    c = dict(key)
    cfg = FWD_CFG[c['cfg']]
    M, H, T = c['M'], c['H'], c['T']
    rng = np.random.RandomState(seed_of(key))
    bf = cfg['prec'] == 'bf16'
    k = 1.0 / np.sqrt(H)
    rnd = lambda a, on: R.bf16_round(a) if on else a.astype(np.float32)
    w = rnd(rng.uniform(-k, k, (3 * H, H)), bf)
    b = rng.uniform(-k, k, 3 * H).astype(np.float32)
    rows = 3 if cfg.get('gi_idx') else M
    gi = rnd(rng.normal(0, 1, (T, rows, 3 * H)), cfg['gi'] == 'b')
    gi2 = None
    if cfg.get('gi2'):
        gi2 = rnd(rng.normal(0, 0.5, (1 if c.get('gi2_bcast') else T, M, 3 * H)), cfg['gi2'] == 'b')
    h0 = rnd(rng.normal(0, 0.5, (M, H)), bf and T == 1 and not c.get('probe'))
    op = R.bf16_round(h0 + rng.normal(0, 0.25, (M, H)).astype(np.float32)) if c.get('probe') else None
    lengths = lengths_of(M, T) if c.get('lengths') else None
    idx = ((2 * np.arange(M) + 1) % 3).astype(np.int32) if cfg.get('gi_idx') else None
    gi2_t = None if gi2 is None else np.broadcast_to(gi2, (T, M, 3 * H))
    a = (gi, gi2_t, w, b, h0, lengths, bool(c.get('reverse')), idx, op)
    ref = R.gru_forward(*a)
    kp = R.kp_forward(*a, bf16=bf, gates_bf16=cfg.get('gates') == 'b')
    return dict(w=w, b=b, gi=gi, gi2=gi2, h0=h0, op=op, lengths=lengths, idx=idx, ref=ref, kp=kp)


def padded(a, ld, dtype):
    """[.., n] -> device [.., ld] with NaN in the padding columns"""
    buf = np.full(a.shape[:-1] + (ld,), NAN, np.float32)
    buf[..., :a.shape[-1]] = a
    return dev(buf, dtype)


def fwd_flags(cfg):
    return (GATES_BF16 * (cfg.get('gates') == 'b') | GI_BF16 * (cfg['gi'] == 'b') | GI2_BF16 * (cfg.get('gi2') == 'b') |
            W_BF16 * bool(cfg.get('w16')))


def seq_fwd_setup(key):
    """device buffers and the ABI argument list of one ptv_gru_seq_fwd call -> (args: dict in call order, tensors, ins)"""
    c = dict(key)
    cfg = FWD_CFG[c['cfg']]
    M, H, T = c['M'], c['H'], c['T']
    ins = fwd_case(key)
    gi_ld = 3 * H + (8 if c.get('gi_pad') else 0)
    t = dict(gi=padded(ins['gi'], gi_ld, BF if cfg['gi'] == 'b' else None), w=dev(ins['w'], BF if cfg.get('w16') else None), b=dev(ins['b']),
             gi2=dev(ins['gi2'], BF if cfg.get('gi2') == 'b' else None), lengths=dev(ins['lengths']), idx=dev(ins['idx']))
    t['hall'] = torch.full(((T + 1) * M + 2, H), float(SENT), device=DEV)
    t['hall'][:M] = dev(ins['h0'])
    flags = fwd_flags(cfg)
    if cfg.get('hall16'):
        t['hall16'] = torch.full(((T + 1) * M + 2, H), float(SENT), dtype=BF, device=DEV)
        if c.get('probe'):
            t['hall16'][:M] = dev(ins['op'], BF)
            flags |= SKIP_CAST0
    if cfg.get('gates'):
        t['gates'] = torch.full((T * 4 * M + 2, H), float(SENT), dtype=BF if cfg['gates'] == 'b' else torch.float32, device=DEV)
    rows = ins['gi'].shape[1]
    args = dict(prec=PREC[cfg['prec']], M=M, H=H, T=T, gi=t['gi'], gi_step=rows * gi_ld, gi_ld=gi_ld, gi2=t['gi2'],
                gi2_step=0 if (t['gi2'] is None or c.get('gi2_bcast')) else M * 3 * H, gi2_ld=3 * H, w=t['w'], b=t['b'], hall=t['hall'],
                hall16=t.get('hall16'), gates=t.get('gates'), lengths=t['lengths'], reverse=int(bool(c.get('reverse'))), idx=t['idx'], flags=flags)
    return args, t, ins


INPUTS = ('gi', 'gi2', 'w', 'b', 'lengths', 'idx', 'hprev', 'hprev16', 'ext', 'last', 'lr_a', 'lr_b', 'gates_in', 'hall_in')


def call(entry, args, t, expect_rc=0, **override):
    """one call of the C entry point; inputs must come back unwritten"""
    a = dict(args)
    a.update(override)
    before = {k: raw(t[k]) for k in INPUTS if t.get(k) is not None}
    rc = K.leaf_rc(entry, *a.values())
    torch.cuda.synchronize()
    assert (rc == 0) == (expect_rc == 0), (entry, rc, override)
    for k, v in before.items():
        assert raw(t[k]) == v, 'input %s was written' % k
    return rc


def dead_steps(lengths, M, T, reverse):
    """bool [T, M]: row m is masked at processing step s"""
    return np.stack([~R.live_mask(lengths, R.time_of(s, T, reverse), M) for s in range(T)])


def check_seq_fwd(key, t, ins):
    c = dict(key)
    cfg = FWD_CFG[c['cfg']]
    M, H, T = c['M'], c['H'], c['T']
    tag = 'fwd ' + FWD_VARIANT_OF[c['cfg']]
    (h_ref, g_ref), (h_kp, g_kp, h16_kp) = ins['ref'], ins['kp']
    hall = host(t['hall'])
    assert (hall[(T + 1) * M:] == SENT).all()
    hall = hall[:(T + 1) * M].reshape(T + 1, M, H)
    assert bits(hall[0]).tobytes() == bits(ins['h0']).tobytes()
    check(tag + ' h', hall[1:], h_ref, h_kp)
    dead = dead_steps(ins['lengths'], M, T, bool(c.get('reverse')))
    for s in range(T):                                                               # a masked row copies its state bit for bit
        assert np.array_equal(bits(hall[s + 1][dead[s]]), bits(hall[s][dead[s]]))
    if 'hall16' in t:
        h16 = host(t['hall16'])
        assert (h16[(T + 1) * M:] == SENT).all()
        h16 = h16[:(T + 1) * M].reshape(T + 1, M, H)
        assert np.array_equal(bits(h16[1:]), bits(R.bf16_round(hall[1:])))           # the shadow is the RNE rounding of the fp32 state
        assert np.array_equal(bits(h16[0]), bits(ins['op'] if c.get('probe') else R.bf16_round(hall[0])))
        check(tag + ' h16', h16[1:], h_ref, h16_kp)
    if 'gates' in t:
        g = host(t['gates'])
        assert (g[T * 4 * M:] == SENT).all()
        g = g[:T * 4 * M].reshape(T, 4, M, H)
        assert (cfg['gates'] == 'b') == R.is_bf16(g) or not np.abs(g).max() > 0
        for s in range(T):                                                           # masked: exactly (0, 1, 0)
            assert (bits(g[s, 0][dead[s]]) == 0).all() and (g[s, 1][dead[s]] == 1).all() and (bits(g[s, 2][dead[s]]) == 0).all()
        for p, pn in enumerate('r z n hn'.split()):
            check('%s %s %s' % (tag, pn, 'bf16' if cfg['gates'] == 'b' else 'fp32'), g[:, p], g_ref[:, p], g_kp[:, p])


@pytest.mark.parametrize('key', FWD_SMALL, ids=cid)
def test_seq_fwd_small(key):
    args, t, ins = seq_fwd_setup(key)
    call('ptv_gru_seq_fwd', args, t)
    check_seq_fwd(key, t, ins)


@pytest.mark.parametrize('tile,key', FWD_TILES, ids=lambda v: cid(v) if isinstance(v, tuple) else v)
def test_seq_fwd_tiles(tile, key):
    c = dict(key)
    assert R.plan_fwd(c['M'], c['H'], FWD_CFG[c['cfg']])[1] == tile
    args, t, ins = seq_fwd_setup(key)
    call('ptv_gru_seq_fwd', args, t)
    check_seq_fwd(key, t, ins)


PROBES = [C(cfg=n, M=M, H=H, T=T, probe=True, lengths=True) for n, M, H, T in
          (('FAST1', 17, 24, 2), ('FAST2', 70, 72, 1), ('B-aw gates32', 16, 8, 3), ('B-a', 70, 64, 2))]


@pytest.mark.parametrize('key', PROBES, ids=cid)
def test_seq_fwd_skip_cast0_product_sees_the_callers_slot_0(key):
    """SKIP_CAST0 with a slot 0 that is NOT the rounding of hall[0]: the product of step 0 sees hall16[0], the blend z h sees hall[0],
    and slot 0 of the shadow is left as the caller wrote it"""
    args, t, ins = seq_fwd_setup(key)
    d = np.abs(ins['op'] - R.bf16_round(ins['h0']))
    assert d.max() > 0.1
    call('ptv_gru_seq_fwd', args, t)
    check_seq_fwd(key, t, ins)


# ---- ptv_gru_step_fwd
STEP_COMBOS = {'fp32': ('F32', False, False), 'B0': ('B0', False, False), 'B0 +hout16': ('B0', False, True), 'B-a': ('B-a', True, False),
               'B-a +hout16': ('B-a', True, True), 'B-aw': ('B-aw gates32', True, True), 'B-aw no hout16': ('B-aw gi32', True, False),
               'FAST1': ('FAST1', True, True), 'FAST2': ('FAST2', True, True), 'FAST1 no hout16 (generic)': ('FAST1', True, False),
               'F32 gi2': ('F32 gi2', False, False), 'F32 idx': ('F32 idx', False, False), 'B0 gi2 idx': ('B0 gi2 idx', False, True)}
STEP_CASES = [(k, p) for k, v in STEP_COMBOS.items() for p in (False, True) if v[1] or not p]          # probe: only where there is an hprev16


@pytest.mark.parametrize('M,H', [(17, 24), (70, 72)])
@pytest.mark.parametrize('combo,probe', STEP_CASES, ids=lambda v: v if isinstance(v, str) else 'probe' if v else 'plain')
def test_step_fwd(combo, probe, M, H):
    """explicit strides: ld_hprev = H + 4 (NaN padding), ld_hout = H + 8 and gates_plane = (M + 2) H (sentinel padding), t = 1 against
    lengths 2, 1, 0, ..; every hprev16 / hout16 combination the entry point takes.  probe: an hprev16 that is not the rounding of hprev"""
    name, a16, o16 = STEP_COMBOS[combo]
    cfg = FWD_CFG[name]
    key = C(cfg=name, M=M, H=H, T=1, probe=probe, step=True)
    rng = np.random.RandomState(seed_of(key))
    base = fwd_case(C(cfg=name, M=M, H=H, T=1, probe=probe, gi2_bcast=False))
    h0 = base['h0'] if probe else (base['h0'] + rng.normal(0, 1e-3, (M, H))).astype(np.float32)          # (not bf16-representable)
    op = base['op']
    lengths, tt = lengths_of(M, 2), 1
    # one step at time tt is a T = 1 chain whose row m is live iff tt < lengths[m]
    a = (base['gi'], base['gi2'], base['w'], base['b'], h0, (lengths > tt).astype(np.int32), False, base['idx'], op)
    bf = cfg['prec'] == 'bf16'
    (h_ref, g_ref), (h_kp, g_kp, h16_kp) = R.gru_forward(*a), R.kp_forward(*a, bf16=bf, gates_bf16=cfg.get('gates') == 'b')
    ld_p, ld_o, plane = H + 4, H + 8, (M + 2) * H
    t = dict(gi=dev(base['gi'][0], BF if cfg['gi'] == 'b' else None), gi2=None if base['gi2'] is None else dev(base['gi2'][0], BF if cfg['gi2'] == 'b' else None),
             w=dev(base['w'], BF if cfg.get('w16') else None), b=dev(base['b']), lengths=dev(lengths), idx=dev(base['idx']),
             hprev=padded(h0, ld_p, None), hprev16=dev(op if probe else R.bf16_round(h0), BF) if a16 else None)
    t['hout'] = torch.full((M + 2, ld_o), float(SENT), device=DEV)
    if o16:
        t['hout16'] = torch.full((M + 2, H), float(SENT), dtype=BF, device=DEV)
    if cfg.get('gates'):
        t['gates'] = torch.full((4, M + 2, H), float(SENT), dtype=BF if cfg['gates'] == 'b' else torch.float32, device=DEV)
    args = dict(prec=PREC[cfg['prec']], M=M, H=H, hprev=t['hprev'], ld_hprev=ld_p, hprev16=t['hprev16'], hout16=t.get('hout16'), gi=t['gi'],
                gi_ld=3 * H, gi2=t['gi2'], gi2_ld=3 * H, w=t['w'], b=t['b'], hout=t['hout'], ld_hout=ld_o, gates=t.get('gates'), plane=plane,
                lengths=t['lengths'], t=tt, idx=t['idx'], flags=fwd_flags(cfg))
    call('ptv_gru_step_fwd', args, t)
    variant = R.plan_fwd(M, H, dict(cfg, hall16=a16, hout16=o16))[0]
    assert variant == (FWD_VARIANT_OF[name] if a16 == o16 or not name.startswith('FAST') else 'B-aw')
    tag = 'step ' + variant
    hout = host(t['hout'])
    assert (hout[M:] == SENT).all() and (hout[:, H:] == SENT).all()
    hout = hout[:M, :H]
    check(tag + ' h', hout, h_ref[0], h_kp[0])
    dead = ~(tt < lengths)
    assert dead.any() and not dead.all()
    assert np.array_equal(bits(hout[dead]), bits(h0[dead]))
    if o16:
        h16 = host(t['hout16'])
        assert (h16[M:] == SENT).all() and np.array_equal(bits(h16[:M]), bits(R.bf16_round(hout)))
    if 'gates' in t:
        g = host(t['gates'])
        assert (g[:, M:] == SENT).all()
        g = g[:, :M]
        assert (bits(g[0][dead]) == 0).all() and (g[1][dead] == 1).all() and (bits(g[2][dead]) == 0).all()
        for p, pn in enumerate('r z n hn'.split()):
            check('%s %s %s' % (tag, pn, 'bf16' if cfg['gates'] == 'b' else 'fp32'), g[p], g_ref[0, p], g_kp[0, p])


# ================================================================================================ backward
@functools.lru_cache(maxsize=8)
def bwd_case(key):
    """operands of one BPTT: the fp64 REFERENCE's states and gates of a random chain rounded to their storage types (no kernel's forward
    output), external gradients, the fp64 reference backward and the kernel-precision evaluation"""
    c = dict(key)
    cfg = BWD_CFG[c['cfg']]
    M, H, T = c['M'], c['H'], c['T']
    rng = np.random.RandomState(seed_of(key))
    bf = cfg['prec'] == 'bf16'
    k = 1.0 / np.sqrt(H)
    rnd = lambda a, on: R.bf16_round(a) if on else np.asarray(a, np.float32)
    w = rnd(rng.uniform(-k, k, (3 * H, H)), bf)
    b = rng.uniform(-k, k, 3 * H)
    h0 = rng.normal(0, 0.5, (M, H)).astype(np.float32)
    lengths = lengths_of(M, T) if c.get('lengths') else None
    reverse = bool(c.get('reverse'))
    hs, gates = R.gru_forward(rng.normal(0, 1, (T, M, 3 * H)), None, w, b, h0, lengths, reverse, None)
    hprev = np.concatenate([h0[None], hs[:-1].astype(np.float32)])
    gates = rnd(gates, cfg.get('gates16'))
    integer = bool(c.get('integer'))
    grad = (lambda *s: rng.randint(-3, 4, s).astype(np.float32)) if integer else (lambda *s: rng.normal(0, 0.5, s).astype(np.float32))
    ext = None if c.get('no_ext') else rnd(grad(T, M, H), cfg.get('ext') == 'b')
    last = grad(M, H) if c.get('last') else None
    lr_k = cfg.get('lr_k', 0)
    lr_a, lr_b = (grad(T, M, lr_k), grad(lr_k, H)) if lr_k else (None, None)
    a = (hprev, gates, w, ext, last, lr_a, lr_b, reverse)
    return dict(w=w, hprev=hprev, gates=gates, ext=ext, last=last, lr_a=lr_a, lr_b=lr_b, lengths=lengths, ref=R.gru_backward(*a),
                kp=R.kp_backward(*a, bf16=bf, dg_bf16=bool(cfg.get('dg16'))))


def bwd_flags(cfg):
    return (GATES_BF16 * bool(cfg.get('gates16')) | DG_BF16 * bool(cfg.get('dg16')) | W_BF16 * bool(cfg.get('w16')) |
            EXT_BF16 * (cfg.get('ext') == 'b'))


def seq_bwd_setup(key):
    c = dict(key)
    cfg = BWD_CFG[c['cfg']]
    M, H, T = c['M'], c['H'], c['T']
    ins = bwd_case(key)
    dgt = BF if cfg.get('dg16') else torch.float32
    ext_ld = H + (8 if c.get('ext_pad') else 0)
    last_ld = H + (4 if c.get('last') == 'pad' else 0)
    lr_k = cfg.get('lr_k', 0)
    lda = lr_k + 1
    hall = np.concatenate([ins['hprev'], np.full((1, M, H), NAN, np.float32)])       # (slot T is not read)
    t = dict(hall_in=dev(hall), gates_in=dev(ins['gates'], BF if cfg.get('gates16') else None),
             w=dev(np.ascontiguousarray(ins['w'].T), BF) if cfg.get('w16') else dev(ins['w']),
             ext=None if ins['ext'] is None else padded(ins['ext'], ext_ld, BF if cfg.get('ext') == 'b' else None),
             last=None if ins['last'] is None else padded(ins['last'], last_ld, None),
             lr_a=None if not lr_k else padded(ins['lr_a'], lda, None), lr_b=dev(ins['lr_b']))
    t['dgi'] = torch.full((T * M + 2, 3 * H), float(SENT), dtype=dgt, device=DEV)
    t['dgh'] = torch.full((T * M + 2, 3 * H), float(SENT), dtype=dgt, device=DEV)
    t['dhz'] = torch.full((2 * M + 2, H), float(SENT), device=DEV)
    if not c.get('no_dh0'):
        t['dh0'] = torch.full((M + 2, H), float(SENT), device=DEV)
    args = dict(prec=PREC[cfg['prec']], M=M, H=H, T=T, hall=t['hall_in'], gates=t['gates_in'], w=t['w'], ext=t['ext'], ext_step=M * ext_ld,
                ext_ld=ext_ld, last=t['last'], last_ld=last_ld, lr_a=t['lr_a'], lr_step=M * lda, lr_lda=lda, lr_k=lr_k, lr_b=t['lr_b'],
                dgi=t['dgi'], dgh=t['dgh'], dhz=t['dhz'], dh0=t.get('dh0'), reverse=int(bool(c.get('reverse'))), flags=bwd_flags(cfg))
    return args, t, ins


def check_seq_bwd(key, t, ins):
    c = dict(key)
    cfg = BWD_CFG[c['cfg']]
    M, H, T = c['M'], c['H'], c['T']
    reverse = bool(c.get('reverse'))
    tag = 'bwd ' + BWD_VARIANT_OF[c['cfg']]
    (dgi_ref, dgh_ref, dh0_ref, dhz_ref), (dgi_kp, dgh_kp, dh0_kp, dhz_kp) = ins['ref'], ins['kp']
    dgi, dgh, dhz = host(t['dgi']), host(t['dgh']), host(t['dhz'])
    assert (dgi[T * M:] == SENT).all() and (dgh[T * M:] == SENT).all() and (dhz[2 * M:] == SENT).all()
    dgi, dgh, dhz = dgi[:T * M].reshape(T, M, 3 * H), dgh[:T * M].reshape(T, M, 3 * H), dhz[:2 * M].reshape(2, M, H)
    if T == 1:
        assert (dhz[1] == SENT).all()                                                # only slot step & 1 is written
    st = 'bf16' if cfg.get('dg16') else 'fp32'
    assert bool(cfg.get('dg16')) == (R.is_bf16(dgi) and R.is_bf16(dgh)) or not np.abs(dgi).max() > 0
    check('%s dgi %s' % (tag, st), dgi, dgi_ref, dgi_kp)
    check('%s dgh %s' % (tag, st), dgh, dgh_ref, dgh_kp)
    check(tag + ' dhz', dhz[0], dhz_ref, dhz_kp)
    for s in range(T):                                                               # the r and z planes of dgi and dgh are the same bits
        assert np.array_equal(bits(dgi[R.time_of(s, T, reverse)][:, :2 * H]), bits(dgh[s][:, :2 * H]))
    dead = dead_steps(ins['lengths'], M, T, reverse)
    for s in range(T):                                                               # masked: no gate gradient at all
        assert not dgh[s][dead[s]].any() and not dgi[R.time_of(s, T, reverse)][dead[s]].any()
    never = dead.all(0)
    if 'dh0' in t:
        dh0 = host(t['dh0'])
        assert (dh0[M:] == SENT).all()
        dh0 = dh0[:M]
        check(tag + ' dh0', dh0, dh0_ref, dh0_kp)
        assert np.array_equal(dh0[dead[0]], dhz[0][dead[0]])             # masked at step 0: z = 1, dhz = dh, no product term
        if c.get('integer') and never.any():                                         # never live: dh0 is the exact sum of what arrived
            assert np.array_equal(dh0[never], dh0_ref[never].astype(np.float32)) and (dh0_ref[never] == np.round(dh0_ref[never])).all()
    if c.get('integer') and never.any():
        assert np.array_equal(dhz[0][never], dhz_ref[never].astype(np.float32))      # a masked row's dhz is its dh


@pytest.mark.parametrize('key', BWD_SMALL, ids=cid)
def test_seq_bwd_small(key):
    args, t, ins = seq_bwd_setup(key)
    call('ptv_gru_seq_bwd', args, t)
    check_seq_bwd(key, t, ins)


@pytest.mark.parametrize('tile,key', BWD_TILES, ids=lambda v: cid(v) if isinstance(v, tuple) else v)
def test_seq_bwd_tiles(tile, key):
    c = dict(key)
    assert R.plan_bwd(c['M'], c['H'], BWD_CFG[c['cfg']])[1] == tile
    args, t, ins = seq_bwd_setup(key)
    call('ptv_gru_seq_bwd', args, t)
    check_seq_bwd(key, t, ins)


# ================================================================================================ refusals
def untouched(t, names):
    return all((host(t[n]) == SENT).all() for n in names if n in t)


def test_seq_fwd_refusals():
    """arguments ptv_gru_seq_fwd rejects before any launch (the slot-0 cast included): non-zero status, every output keeps its sentinel"""
    f32, fast, b0 = C(cfg='F32 gi2', M=17, H=16, T=2, gi2_bcast=False), C(cfg='FAST2', M=17, H=16, T=2, gi2_bcast=False), C(cfg='B0', M=17, H=16, T=2)
    cases = [(f32, dict(H=6)), (f32, dict(H=18)), (fast, dict(H=12)), (fast, dict(hall16=None)),                       # H % 4, H % 8 with a shadow, W_BF16 alone
             (fast, dict(prec=0)), (b0, dict(flags=W_BF16)), (f32, dict(flags=W_BF16)),
             (f32, dict(gi_ld=50)), (f32, dict(gi_step=17 * 48 + 2)), (f32, dict(gi2_ld=50)), (f32, dict(gi2_step=17 * 48 + 2)),
             (f32, dict(gi=None)), (f32, dict(w=None)), (f32, dict(b=None)), (f32, dict(hall=None)),
             (f32, dict(M=0)), (f32, dict(H=0)), (f32, dict(T=0)), (f32, dict(M=-1)), (f32, dict(H=-4)), (f32, dict(T=-1))]
    for key, bad in cases:
        args, t, ins = seq_fwd_setup(key)
        call('ptv_gru_seq_fwd', args, t, expect_rc=-1, **bad)
        assert untouched(t, ('gates', 'hall16')) and (host(t['hall'])[17:] == SENT).all(), bad


def test_step_fwd_refusals():
    M, H = 17, 16
    for name, bads in (('F32 gi2', [dict(H=6), dict(gi_ld=50), dict(ld_hprev=18), dict(ld_hout=18), dict(gi2_ld=50), dict(plane=17 * 16 + 2),
                                    dict(hprev=None), dict(gi=None), dict(w=None), dict(b=None), dict(hout=None), dict(M=0), dict(H=0),
                                    dict(M=-1), dict(flags=W_BF16), dict(hout16='o16'), dict(hprev16='p16')]),
                       ('FAST2', [dict(H=12), dict(hprev16=None), dict(prec=0)]), ('B0', [dict(flags=W_BF16), dict(H=12, hout16='o16')])):
        cfg = FWD_CFG[name]
        base = fwd_case(C(cfg=name, M=M, H=H, T=1, gi2_bcast=False))
        for bad in bads:
            t = dict(gi=dev(base['gi'][0], BF if cfg['gi'] == 'b' else None), gi2=None if base['gi2'] is None else dev(base['gi2'][0], BF if cfg['gi2'] == 'b' else None),
                     w=dev(base['w'], BF if cfg.get('w16') else None), b=dev(base['b']), hprev=dev(base['h0']),
                     p16=dev(R.bf16_round(base['h0']), BF), o16=torch.full((M, H), float(SENT), dtype=BF, device=DEV),
                     hout=torch.full((M, H), float(SENT), device=DEV), gates=torch.full((4, M, H), float(SENT), dtype=BF if cfg['gates'] == 'b' else torch.float32, device=DEV))
            a16 = bool(cfg.get('hall16'))
            args = dict(prec=PREC[cfg['prec']], M=M, H=H, hprev=t['hprev'], ld_hprev=H, hprev16=t['p16'] if a16 else None, hout16=t['o16'] if a16 else None,
                        gi=t['gi'], gi_ld=3 * H, gi2=t['gi2'], gi2_ld=3 * H, w=t['w'], b=t['b'], hout=t['hout'], ld_hout=H, gates=t['gates'], plane=M * H,
                        lengths=None, t=0, idx=None, flags=fwd_flags(cfg))
            call('ptv_gru_step_fwd', args, t, expect_rc=-1, **{k: t[v] if isinstance(v, str) else v for k, v in bad.items()})
            assert untouched(t, ('hout', 'o16', 'gates')), (name, bad)


def test_seq_bwd_refusals():
    """... and ptv_gru_seq_bwd, the two low-rank guards included: lr_a without lr_b, lr_a with a rank <= 0"""
    f32 = C(cfg='F32 lr1', M=17, H=16, T=2, last='dense')
    fast = C(cfg='FAST ext16 lr2', M=17, H=16, T=2, last='dense')
    b0 = C(cfg='B0', M=17, H=16, T=2, last='dense')
    cases = [(f32, dict(H=6)), (fast, dict(H=12)), (fast, dict(flags=GATES_BF16 | W_BF16)), (fast, dict(prec=0)),
             (f32, dict(flags=EXT_BF16)), (f32, dict(flags=DG_BF16)), (b0, dict(flags=W_BF16)),
             (f32, dict(ext_ld=18)), (f32, dict(ext_step=17 * 16 + 2)), (f32, dict(last_ld=18)),
             (f32, dict(hall=None)), (f32, dict(gates=None)), (f32, dict(w=None)), (f32, dict(dgi=None)), (f32, dict(dgh=None)), (f32, dict(dhz=None)),
             (f32, dict(M=0)), (f32, dict(H=0)), (f32, dict(T=0)), (f32, dict(M=-1)), (f32, dict(T=-2)),
             (f32, dict(lr_b=None)), (fast, dict(lr_b=None)), (f32, dict(lr_k=0)), (fast, dict(lr_k=0)), (fast, dict(lr_k=-1))]
    for key, bad in cases:
        args, t, ins = seq_bwd_setup(key)
        call('ptv_gru_seq_bwd', args, t, expect_rc=-1, **bad)
        assert untouched(t, ('dgi', 'dgh', 'dhz', 'dh0')), bad
