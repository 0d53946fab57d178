"""The 5-step duration decoder one kernel at a time against the plain fp64 references of tests/dur_ref.py: csrc/dur.hip
(ptv_dur_gru_fwd / _top / _rows), csrc/dur_bwd.hip (ptv_dur_gru_bwd in its four template variants -- saved gates or recompute, bf16 or
fp32 states -- and ptv_dur_bwd_finalize) and ptv_dur_out_token / ptv_dur_out_wgrad of csrc/misc.hip, at the small shapes where they can
go wrong: below one 16-row wave tile, ragged 64-row backward tiles, fewer / as many / more blocks than tiles, tiles without gradient,
padded strides, the live-row limits, and one size per grid cap that forces a second grid-stride trip.  The B = 512 regimes (1024 and
256 blocks) stay with test_gpu_kernels.py::test_fused_duration_kernels_at_the_b512_grid_caps.

Inputs are built on the CPU from seeded generators and given, the same values, to the kernel and (widened) to the reference; W_hh is
bf16-representable, and so are the gates and bf16 states fed to the saved-gates backward.  Every output buffer is pre-filled with a
sentinel.  Integer outputs and the stated equalities are exact.  Floating-point outputs have no pre-chosen tolerance: the same formulas
are evaluated on the CPU in fp32 with bf16 rounding where the kernels round (dur_ref.kp_*), that evaluation's error against the fp64
reference is measured, and the kernel's error may be at most 4x that, with a floor of 8 fp32 ulps of the array's scale (check()).  The
bound never sees the kernel's output.  Each check prints `DUR_RATIO family kernel-error/bound` (pytest -s; table in profiles/LOG.md)."""
import functools

import numpy as np
import pytest
import torch

import dur_ref as R
import kernel_ops as K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 64
NAN = np.float32(np.nan)
SENT = np.float32(768.0)                                               # (exact in bf16)
ISENT = -7
BF = torch.bfloat16
RATIOS = {}


def lib():
    from polyphonic_chord_texture_disentanglement_amd._lib import lib as _l
    return _l()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.float().cpu().numpy() if t.dtype == BF else t.cpu().numpy()


def bound_of(ref, kp, scale=None):
    """max(4 * max|kp - ref|, 8 ulp_fp32(scale)); scale: a scalar or one figure per element, default the array's largest magnitude"""
    ref, kp = np.asarray(ref, np.float64), np.asarray(kp, np.float64)
    assert ref.shape == kp.shape and np.isfinite(ref).all() and np.isfinite(kp).all()
    scale = np.abs(ref).max() if scale is None else scale
    errk = np.abs(kp - ref).max()
    return np.maximum(4.0 * errk, 8.0 * np.spacing(np.abs(np.asarray(scale, np.float64)).astype(np.float32)).astype(np.float64)), errk


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
    print('DUR_RATIO %s %.3f (kernel err %.3e, kernel-precision CPU err %.3e)' % (family, ratio, err.max(), errk))
    assert (err <= bound).all(), '%s: kernel error %.3e over the bound %.3e (kernel-precision CPU evaluation: %.3e)' % (
        family, err.max(), float(np.min(bound)), errk)


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('DUR_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


# ================================================================================================ inputs
@functools.lru_cache(maxsize=None)
def weights(seed=1, I=5, out_gain=1.0):
    rng = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(H)
    u = lambda *s: rng.uniform(-k, k, s).astype(np.float32)
    W = dict(w_hh=R.bf16_round(u(3 * H, H)), b_hh=u(3 * H), w_ih=u(3 * H, I), b_ih=u(3 * H), w_out=u(2, H) * np.float32(out_gain),
             b_out=u(2), sos=rng.uniform(0, 1, I).astype(np.float32))
    tab0, tab = R.gate_tables(W['w_ih'], W['b_ih'], W['sos'])
    W['tab0'], W['tab'] = tab0.astype(np.float32), tab.astype(np.float32)           # the kernels and the reference see these fp32 tables
    return W


def wdev(W):
    return {k: dev(v) for k, v in W.items()}


def tokens(rng, M):
    """[5, M] forced tokens; both values in every step's row where M allows it (with <sos>: all three token classes)"""
    t = rng.randint(0, 2, (5, M)).astype(np.int32)
    t[:, 0] = [0, 1, 0, 1, 1]
    if M > 1:
        t[:, 1] = [1, 0, 1, 0, 0]
    return t


@functools.lru_cache(maxsize=None)
def fwd_case(M, seed=0):
    """inputs, fp64 reference and kernel-precision evaluation of one forced-token forward, shared by the tests of that M (read only)"""
    rng = np.random.RandomState(1000 + 7 * M + seed)
    W = weights()
    h0 = rng.normal(0, 0.5, (M, H)).astype(np.float32)
    force = tokens(rng, M)
    a = (h0, W['w_hh'], W['b_hh'], W['tab0'], W['tab'], W['w_out'], W['b_out'], force)
    return h0, force, R.dur_forward(*a), R.kp_forward(*a)


# ================================================================================================ forward
def run_fwd(entry, M, W, h0, force, hall=True, hall16=False, gates=None, ld_h0=H, ld_out=10, idx_stride=None, force_stride=None,
            extra=(), pad_rows=2, expect_rc=0, Hd=H, bad=None):
    """one forward launch into sentinel-filled buffers whose planes have M + pad_rows rows -> host arrays"""
    Mp = M + pad_rows
    idx_stride = M if idx_stride is None else idx_stride
    force_stride = M if force_stride is None else force_stride
    hb = np.full((M, ld_h0), NAN, np.float32)
    hb[:, :H] = h0
    t = dict(dur=torch.full((Mp, ld_out), float(SENT), device=DEV), idx=torch.full((5, idx_stride), ISENT, dtype=torch.int32, device=DEV))
    if hall:
        t['hall'] = torch.full((5, Mp, H), float(SENT), device=DEV)
    if hall16:
        t['hall16'] = torch.full((5, Mp, H), float(SENT), dtype=BF, device=DEV)
    if gates:
        t['gates'] = torch.full((5, 4, Mp, H), float(SENT), dtype=BF if gates == 'bf16' else torch.float32, device=DEV)
    fb = None
    if force is not None:
        fbuf = np.zeros((5, force_stride), np.int32)
        fbuf[:, :M] = force
        fb = dev(fbuf)
    wd = wdev(W)
    s = dict(plane_h=Mp * H, plane_g=Mp * H, step_g=4 * Mp * H, ld_h0=ld_h0)
    s.update(bad or {})
    rc = K.leaf_rc(entry, Hd, M, dev(hb), s['ld_h0'], wd['w_hh'], wd['b_hh'], wd['tab0'], wd['tab'], wd['w_out'], wd['b_out'],
                   t.get('hall'), s['plane_h'], t.get('hall16'), t.get('gates'), s['plane_g'], s['step_g'], int(gates == 'bf16'),
                   t['dur'], ld_out, t['idx'], idx_stride, fb, force_stride, *extra)
    torch.cuda.synchronize()
    assert (rc == 0) == (expect_rc == 0), (entry, rc)
    return {k: host(v) for k, v in t.items()}


def rows_first(out):
    """every output with its row axis first: {name: [rows, ...]}"""
    v = {'dur': out['dur'], 'idx': out['idx'].T}
    for k in ('hall', 'hall16'):
        if k in out:
            v[k] = out[k].transpose(1, 0, 2)
    if 'gates' in out:
        v['gates'] = out['gates'].transpose(2, 0, 1, 3)
    return v


def untouched(name, a):
    return bool((a == (ISENT if name == 'idx' else SENT)).all())


def check_fwd(out, M, ref, kp, force, tag='', rows=None, ref_rows=None, gates=None):
    """every output of a forward launch against the reference on `rows` (default all M; ref / kp hold ref_rows), guards untouched"""
    rows = np.arange(M) if rows is None else rows
    rr = rows if ref_rows is None else ref_rows
    for name, a in rows_first(out).items():
        assert untouched(name, a[M:]), name                                          # the rows after M
    assert untouched('dur', out['dur'][:, 10:])                                      # the padding columns of est_dur
    assert np.array_equal(out['idx'][:, :M][:, rows], np.asarray(force)[:, rows])
    check('fwd est' + tag, out['dur'][rows, :10], ref['est_dur'][rr], kp['est_dur'][rr])
    if 'hall' in out:
        check('fwd h' + tag, out['hall'][:, rows], ref['h'][:, rr], kp['h'][:, rr])
    if 'hall16' in out:
        check('fwd h bf16' + tag, out['hall16'][:, rows], ref['h'][:, rr], R.bf16_round(kp['h'][:, rr]))
    if 'gates' in out:
        bf = gates == 'bf16'
        assert bf == R.is_bf16(out['gates'][:, :, :M][:, :, rows])
        for p, pn in enumerate('r z n hn'.split()):
            k = kp['gates'][:, p][:, rr]
            check('fwd %s %s%s' % (pn, 'bf16' if bf else 'fp32', tag), out['gates'][:, p][:, rows], ref['gates'][:, p][:, rr],
                  R.bf16_round(k) if bf else k)


FWD_COMBOS = {'hall': (True, False, None), 'hall16': (False, True, None), 'both+bf16': (True, True, 'bf16'),
              'hall+fp32': (True, False, 'fp32'), 'hall16+bf16': (False, True, 'bf16')}


@pytest.mark.parametrize('combo', list(FWD_COMBOS))
@pytest.mark.parametrize('M', [1, 15, 16, 17, 63, 64, 65, 130])
def test_fwd_forced_tokens(M, combo):
    """ptv_dur_gru_fwd around the 16-row wave tile and the 64-row block; every combination of fp32 / bf16 states and no / bf16 / fp32 gates"""
    h0, force, ref, kp = fwd_case(M)
    assert M == 1 or {0, 1} == set(force.reshape(-1).tolist())
    hall, hall16, gates = FWD_COMBOS[combo]
    out = run_fwd('ptv_dur_gru_fwd', M, weights(), h0, force, hall, hall16, gates)
    check_fwd(out, M, ref, kp, force, gates=gates)


@pytest.mark.parametrize('M', [17, 130])
def test_fwd_padded_strides(M):
    """ld_h0 = 72 (NaN in the padding), ld_out = 12, idx_stride = M + 3, force_stride = M + 5"""
    h0, force, ref, kp = fwd_case(M)
    out = run_fwd('ptv_dur_gru_fwd', M, weights(), h0, force, True, True, 'bf16', ld_h0=72, ld_out=12, idx_stride=M + 3, force_stride=M + 5)
    check_fwd(out, M, ref, kp, force, gates='bf16')
    assert out['dur'].shape[1] == 12 and out['idx'].shape[1] == M + 3


FREE_M, FREE_GAIN = 330, 4.0


@functools.lru_cache(maxsize=None)
def free_case():
    """free-running tokens.  A decision of the reference is CERTAIN when its margin |est1 - est0| and that of every earlier decision of
    its row exceed twice the est_dur bound: the kernel then saw the same tokens and must decide the same way"""
    rng = np.random.RandomState(77)
    W = weights(out_gain=FREE_GAIN)
    h0 = rng.normal(0, 0.5, (FREE_M, H)).astype(np.float32)
    a = (h0, W['w_hh'], W['b_hh'], W['tab0'], W['tab'], W['w_out'], W['b_out'])
    ref = R.dur_forward(*a)
    kp = R.kp_forward(*a, ref['idx'])
    bound, _ = bound_of(ref['est_dur'], kp['est_dur'])
    e = ref['est_dur'].reshape(FREE_M, 5, 2)
    certain = np.logical_and.accumulate(np.abs(e[:, :, 1] - e[:, :, 0]) > 2 * float(bound), axis=1).T          # [5, M]
    return W, h0, ref, kp, certain


def test_fwd_free_running_tokens():
    W, h0, ref, kp, certain = free_case()
    uncertain = 1.0 - certain.mean()
    print('DUR_FREE uncertain decisions: %d of %d (%.2f %%)' % ((~certain).sum(), certain.size, 100 * uncertain))
    assert uncertain < 0.05                                                          # (the reference alone: no kernel output in it)
    assert {0, 1} == set(ref['idx'][certain].tolist())
    out = run_fwd('ptv_dur_gru_fwd', FREE_M, W, h0, None, True, False, None)
    est = out['dur'][:FREE_M, :10].reshape(FREE_M, 5, 2)
    idx = out['idx'][:, :FREE_M]
    assert np.array_equal(idx, (est[:, :, 1] > est[:, :, 0]).T.astype(np.int32))     # the kernel's own argmax rule, exactly
    assert np.array_equal(idx[certain], ref['idx'][certain])
    rows = np.nonzero(certain.all(0))[0]                                             # rows that took the reference's path throughout
    check_fwd(out, FREE_M, ref, kp, ref['idx'], ' free', rows=rows)


def test_fwd_argmax_tie_gives_token_0():
    """a zero output layer with equal biases: est0 == est1 in every row and step, and the first maximum wins"""
    W = dict(weights())
    W['w_out'], W['b_out'] = np.zeros((2, H), np.float32), np.full(2, 0.3, np.float32)
    h0 = fwd_case(17)[0]
    out = run_fwd('ptv_dur_gru_fwd', 17, W, h0, None)
    assert (out['dur'][:17, :10] == np.float32(0.3)).all() and not out['idx'][:, :17].any()


def same_rows(a, b, live, M):
    """outputs a equal b bit for bit on the live rows and hold the sentinel on every other one"""
    va, vb = rows_first(a), rows_first(b)
    for name in va:
        x, y = va[name], vb[name]
        assert x[:M][live].tobytes() == y[:M][live].tobytes(), name
        assert untouched(name, x[:M][~live]) and untouched(name, x[M:]), name


@pytest.mark.parametrize('top', [-1, 0, 3, 100])
def test_fwd_top_live_row_limit(top):
    M, unit = 130, 16
    h0, force, ref, kp = fwd_case(M)
    full = run_fwd('ptv_dur_gru_fwd', M, weights(), h0, force, True, True, 'bf16')
    out = run_fwd('ptv_dur_gru_fwd_top', M, weights(), h0, force, True, True, 'bf16', extra=(dev(np.array([top], np.int32)), unit))
    n_live = min(M, (max(top, 0) + 1) * unit)
    live = np.arange(M) < n_live
    same_rows(out, full, live, M)
    rows = np.nonzero(live)[0]
    check_fwd(out, M, ref, kp, force, rows=rows, ref_rows=rows, gates='bf16')
    none = run_fwd('ptv_dur_gru_fwd_top', M, weights(), h0, force, True, True, 'bf16', extra=(None, 0))           # no limit: all rows
    same_rows(none, full, np.ones(M, bool), M)


@pytest.mark.parametrize('firsts', [(2,), (4,), (0,), (3, 1)])
def test_fwd_rows_dead_blocks(firsts):
    """row_len [m_unit] descending: the 128-row block that starts at row j of note step s is passed over when row_len[j] <= s"""
    steps, unit = 4, 128 * len(firsts)                                               # firsts: row_len of the first row of each 128-row block
    M = steps * unit
    h0, force, ref, kp = fwd_case(M)
    row_len = np.concatenate([np.maximum(0, f - np.arange(128) // 50) for f in firsts]).astype(np.int32)
    assert (np.diff(row_len) <= 0).all() and row_len.size == unit
    live = np.zeros(M, bool)
    for rb in range(0, M, 128):
        live[rb:rb + 128] = row_len[rb % unit] > rb // unit
    full = run_fwd('ptv_dur_gru_fwd', M, weights(), h0, force, False, True, None)
    out = run_fwd('ptv_dur_gru_fwd_rows', M, weights(), h0, force, False, True, None,
                  extra=(dev(np.array([steps - 1], np.int32)), unit, dev(row_len)))
    same_rows(out, full, live, M)
    rows = np.nonzero(live)[0]
    if rows.size:
        check_fwd(out, M, ref, kp, force, rows=rows, ref_rows=rows)


def test_fwd_argument_refusals():
    """what ptv_dur_gru_fwd_rows refuses returns non-zero and launches nothing: every output keeps its sentinel"""
    M = 256
    h0, force, _, _ = fwd_case(M)
    top, rl = dev(np.array([1], np.int32)), dev(np.full(128, 2, np.int32))
    cases = [dict(extra=(top, 24, None)), dict(extra=(top, 0, None)),                 # m_unit no multiple of 16 / not positive
             dict(extra=(None, 128, rl)),                                            # row_len without m_top
             dict(extra=(top, 64, rl)), dict(extra=(top, 144, rl)),                   # m_unit & 127 with row_len
             dict(extra=(None, 0, None), Hd=32), dict(extra=(None, 0, None), Hd=128),          # H != 64
             dict(extra=(None, 0, None), ld_h0=68, bad=dict(ld_h0=66)),               # misaligned strides (a 68-column buffer announced as 66)
             dict(extra=(None, 0, None), bad=dict(plane_h=(M + 2) * H + 4)),
             dict(extra=(None, 0, None), bad=dict(plane_g=(M + 2) * H + 4)), dict(extra=(None, 0, None), bad=dict(step_g=4 * (M + 2) * H + 4))]
    for kw in cases:
        out = run_fwd('ptv_dur_gru_fwd_rows', M, weights(), h0, force, True, True, 'bf16', expect_rc=-1, **kw)
        for name, a in rows_first(out).items():
            assert untouched(name, a), (kw, name)


def test_fwd_second_grid_stride_trip():
    """M = 64 x cap + 21 rows with cap = 3 x CU count blocks of 64 rows: the first 64 rows, the last 64 of the first trip and the 21 of the second"""
    cap = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    M = 64 * cap + 21
    rng = np.random.RandomState(5)
    W = weights()
    h0 = rng.normal(0, 0.5, (M, H)).astype(np.float32)
    force = rng.randint(0, 2, (5, M)).astype(np.int32)
    rows = np.concatenate([np.arange(64), np.arange(64 * cap - 64, M)])             # (wrap-around and last rows: one span of 85)
    a = (h0[rows], W['w_hh'], W['b_hh'], W['tab0'], W['tab'], W['w_out'], W['b_out'], force[:, rows])
    ref, kp = R.dur_forward(*a), R.kp_forward(*a)
    out = run_fwd('ptv_dur_gru_fwd', M, W, h0, force, False, True, None)
    check_fwd(out, M, ref, kp, force, ' 2nd trip', rows=rows, ref_rows=np.arange(rows.size))
    assert np.array_equal(out['idx'][:, :M], force)
    assert not (out['dur'][:M, :10] == SENT).any() and not (out['hall16'][:, :M] == SENT).all(-1).any()          # every row was written


# ================================================================================================ backward
VARIANTS = [('saved', 1), ('saved', 0), ('recompute', 1), ('recompute', 0)]          # (gates, h_bf16): dur_gru_bwd_kernel<HB, RC>


@functools.lru_cache(maxsize=None)
def bwd_case(M, mode, h_bf16, seed=0):
    """synthetic operands of one backward (they come from no forward pass: a backward error cannot hide behind a forward one), the
    fp64 reference and the kernel-precision evaluation.  saved: r, z in (0, 1), n in (-1, 1), hn free, bf16-representable"""
    rng = np.random.RandomState(2000 + 11 * M + seed)
    W = weights()
    states = rng.normal(0, 0.5, (5, M, H)).astype(np.float32)
    if h_bf16:
        states = R.bf16_round(states)
    ddur = rng.normal(0, 0.1, (M, 10)).astype(np.float32)
    idx = tokens(rng, M)
    gates = None
    if mode == 'saved':
        g = np.stack([rng.uniform(0.02, 0.98, (5, M, H)), rng.uniform(0.02, 0.98, (5, M, H)), rng.uniform(-0.98, 0.98, (5, M, H)),
                      rng.normal(0, 0.7, (5, M, H))], axis=1)
        gates = R.bf16_round(g.astype(np.float32))
        assert R.is_bf16(gates) and (gates[:, :2] > 0).all() and (gates[:, :2] < 1).all() and (np.abs(gates[:, 2]) < 1).all()
    return W, states, gates, ddur, idx


def bwd_ref(W, states, gates, ddur, idx):
    if gates is None:
        ref = R.dur_backward_recompute(states, ddur, idx, W['w_hh'], W['b_hh'], W['tab0'], W['tab'], W['w_out'])
    else:
        ref = R.dur_backward(gates, states, ddur, idx, W['w_hh'], W['w_out'])
    return ref, R.kp_backward(gates, states, ddur, idx, W['w_hh'], W['w_out'], W['b_hh'], W['tab0'], W['tab'])


TABLES = ('b_hh', 'tab0', 'tab')


def run_bwd(M, W, states, gates, ddur, idx, h_bf16, nblocks, pad=0, expect_rc=0, bad=None, null=(), keep=False):
    """one ptv_dur_gru_bwd launch -> dh0 [M, 64], part [nblocks, 256, 80]; pad: rows / columns / elements of NaN (index: 0) padding in
    every stride.  null: the recompute tables passed as NULL.  keep: the device partials too"""
    Mp, ld_dd, idx_stride = M + pad, 10 + 2 * pad, M + 3 * pad
    hb = np.full((5, Mp, H), NAN, np.float32)
    hb[:, :M] = states
    hall = dev(hb, BF if h_bf16 else None)
    gt = None
    if gates is not None:
        gb = np.full((5, 4, Mp, H), NAN, np.float32)
        gb[:, :, :M] = gates
        gt = dev(gb, BF)
    db = np.full((M, ld_dd), NAN, np.float32)
    db[:, :10] = ddur
    ib = np.zeros((5, idx_stride), np.int32)
    ib[:, :M] = idx
    psz = lib().ptv_dur_gru_bwd_part_size()
    assert psz == 256 * 80
    dh0 = torch.full((M + 1, H), float(SENT), device=DEV)
    part = torch.full((nblocks + 1, psz), float(SENT), device=DEV)
    wd = wdev(W)
    s = dict(plane_g=Mp * H, step_g=4 * Mp * H, plane_h=Mp * H, ld_dd=ld_dd, H=H)
    s.update(bad or {})
    rcw = [None if k in null else wd[k] for k in TABLES]
    rc = K.leaf_rc('ptv_dur_gru_bwd', s['H'], M, gt, s['plane_g'], s['step_g'], hall, s['plane_h'], int(h_bf16), dev(db), s['ld_dd'],
                   wd['w_hh'], wd['w_out'], dev(ib), idx_stride, dh0, part, nblocks, *rcw)
    torch.cuda.synchronize()
    assert (rc == 0) == (expect_rc == 0), rc
    d, p = host(dh0), host(part)
    if expect_rc:
        assert (d == SENT).all() and (p == SENT).all()                               # refused: nothing ran
        return None
    assert (d[M] == SENT).all() and (p[nblocks] == SENT).all()                       # guard row, guard partial
    out = d[:M], p[:nblocks].reshape(nblocks, 256, 80)
    return out + (part[:nblocks],) if keep else out


def check_bwd(tag, dh0, part, M, ref, kp, nblocks):
    (dh0_ref, S_ref), (dh0_kp, S_kp) = ref, kp
    assert not (part == SENT).any() and np.isfinite(part).all()                      # every block wrote its whole partial
    tiles = (M + 63) // 64
    assert not part[tiles:].any()                                                    # a block that owned no tile: zeros
    assert all(part[b].any() for b in range(min(tiles, nblocks)))
    S = part.astype(np.float64).sum(0)
    assert not S[:, 67:].any()
    check('bwd dh0 ' + tag, dh0, dh0_ref, dh0_kp)
    check('bwd S.h ' + tag, S[:, :64], S_ref[:, :64], S_kp[:, :64])
    check('bwd S.class ' + tag, S[:, 64:67], S_ref[:, 64:67], S_kp[:, 64:67])


def vtag(mode, h_bf16):
    return '%s %s' % (mode, 'bf16' if h_bf16 else 'fp32')


@pytest.mark.parametrize('mode,h_bf16', VARIANTS)
@pytest.mark.parametrize('M', [1, 17, 64, 65, 130, 327])
def test_bwd_shapes(M, mode, h_bf16):
    """below a tile, a whole tile, ragged tiles; as many blocks as functional.dur_bwd_fused launches; odd M with NaN-padded strides"""
    W, states, gates, ddur, idx = bwd_case(M, mode, h_bf16)
    nblocks = min(256, (M + 63) // 64)
    dh0, part = run_bwd(M, W, states, gates, ddur, idx, h_bf16, nblocks, pad=M % 2, null=TABLES if mode == 'saved' else ())            # saved gates: the tables may be NULL
    check_bwd(vtag(mode, h_bf16), dh0, part, M, *bwd_ref(W, states, gates, ddur, idx), nblocks)


@pytest.mark.parametrize('mode,h_bf16', VARIANTS)
@pytest.mark.parametrize('nblocks', [1, 2, 6, 8])
def test_bwd_blocks_below_equal_and_above_the_tile_count(nblocks, mode, h_bf16):
    M = 327                                                                          # 6 tiles, the last with 7 rows
    W, states, gates, ddur, idx = bwd_case(M, mode, h_bf16)
    dh0, part = run_bwd(M, W, states, gates, ddur, idx, h_bf16, nblocks, pad=1)
    check_bwd(vtag(mode, h_bf16), dh0, part, M, *bwd_ref(W, states, gates, ddur, idx), nblocks)


@pytest.mark.parametrize('mode,h_bf16', VARIANTS)
def test_bwd_tiles_without_gradient(mode, h_bf16):
    """tile 1: no gradient at all (A); tile 2: one live row (B).  Skipping on and off give equal results; with skipping on, tile 1's
    gates and states may hold anything -- what the decoder's dead-step limit relies on (its rows per step are a multiple of 128)"""
    M = 256
    W, states, gates, ddur, idx = bwd_case(M, mode, h_bf16)
    ddur = ddur.copy()
    ddur[64:192] = 0
    ddur[150] = bwd_case(M, mode, h_bf16)[3][150]
    ref, kp = bwd_ref(W, states, gates, ddur, idx)
    res = {}
    try:
        for skip in (1, 0):
            assert lib().ptv_zero_skip(skip) == 0
            res[skip] = run_bwd(M, W, states, gates, ddur, idx, h_bf16, 4)
        lib().ptv_zero_skip(1)
        st, gt = states.copy(), None if gates is None else gates.copy()
        st[:, 64:128] = NAN
        if gt is not None:
            gt[:, :, 64:128] = NAN
        poisoned = run_bwd(M, W, st, gt, ddur, idx, h_bf16, 4)
    finally:
        lib().ptv_zero_skip(1)
    for skip in (1, 0):
        dh0, part = res[skip]
        assert not dh0[64:128].any() and not part[1].any()                            # tile A: exactly zero
        assert dh0[150].any() and not dh0[128:150].any() and not dh0[151:192].any() and part[2].any()
        S = part.astype(np.float64).sum(0)
        check('bwd dh0 ' + vtag(mode, h_bf16), dh0, ref[0], kp[0])
        check('bwd S.h ' + vtag(mode, h_bf16), S[:, :64], ref[1][:, :64], kp[1][:, :64])
        check('bwd S.class ' + vtag(mode, h_bf16), S[:, 64:67], ref[1][:, 64:67], kp[1][:, 64:67])
    assert (res[1][0] == res[0][0]).all() and (res[1][1].astype(np.float64).sum(0) == res[0][1].astype(np.float64).sum(0)).all()
    assert np.isfinite(poisoned[0]).all() and np.isfinite(poisoned[1]).all()
    assert (poisoned[0] == res[1][0]).all() and (poisoned[1] == res[1][1]).all()


@pytest.mark.parametrize('mode,h_bf16', VARIANTS)
def test_bwd_rows_of_a_ragged_tile_contribute_nothing(mode, h_bf16):
    """M = 65 against M = 128 whose rows 65..127 receive no gradient: the same partials, the same dh0 on the first 65 rows"""
    W, states, gates, ddur, idx = bwd_case(128, mode, h_bf16)
    ddur = ddur.copy()
    ddur[65:] = 0
    big = run_bwd(128, W, states, gates, ddur, idx, h_bf16, 2)
    small = run_bwd(65, W, states[:, :65], None if gates is None else gates[:, :, :65], ddur[:65], idx[:, :65], h_bf16, 2, pad=1)
    assert (small[1].astype(np.float64).sum(0) == big[1].astype(np.float64).sum(0)).all()
    assert (small[0] == big[0][:65]).all() and not big[0][65:].any()
    ref, kp = bwd_ref(W, states[:, :65], None if gates is None else gates[:, :, :65], ddur[:65], idx[:, :65])
    check_bwd(vtag(mode, h_bf16), *small, 65, ref, kp, 2)


def test_bwd_argument_refusals():
    M = 130
    for mode, h_bf16 in VARIANTS:
        W, states, gates, ddur, idx = bwd_case(M, mode, h_bf16)
        a = (M, W, states, gates, ddur, idx, h_bf16, 3)
        if mode == 'recompute':                                                      # the tables are required
            for null in (('b_hh',), ('tab0',), ('tab',), TABLES):
                run_bwd(*a, pad=1, expect_rc=-1, null=null)
        run_bwd(*a, pad=1, expect_rc=-1, bad=dict(ld_dd=13))
        for k in ('plane_g', 'step_g', 'plane_h'):                                   # (within the padded buffers all the same)
            run_bwd(*a, pad=1, expect_rc=-1, bad={k: (M + 1) * H * (4 if k == 'step_g' else 1) + 2})
        run_bwd(*a, pad=1, expect_rc=-1, bad=dict(H=32))


# ================================================================================================ parameter gradients
def grad_start(rng, I):
    return [rng.normal(0, 1, s).astype(np.float32) for s in ((3 * H, H), (3 * H,), (3 * H,), (3 * H, I), (I,))]


GRAD_NAMES = ('dW_hh', 'db_hh', 'db_ih', 'dW_ih', 'd sos')


def run_finalize(S_dev, start, w_ih, sos, expect_rc=0, I=None):
    bufs = [dev(np.concatenate([s.reshape(-1), [SENT]]).astype(np.float32)) for s in start]
    rc = K.leaf_rc('ptv_dur_bwd_finalize', S_dev, *bufs, dev(w_ih), dev(sos), sos.size if I is None else I)
    torch.cuda.synchronize()
    assert (rc == 0) == (expect_rc == 0), rc
    got = [host(b) for b in bufs]
    assert all(g[-1] == SENT for g in got)
    return [g[:-1].reshape(s.shape) for g, s in zip(got, start)]


def check_finalize(tag, got, S_ref, S_kp, start, w_ih, sos):
    ref = [s.astype(np.float64) + i for s, i in zip(start, R.dur_finalize(S_ref, w_ih, sos))]
    kp = R.kp_finalize(S_kp, w_ih, sos, start)
    t0 = np.concatenate([S_ref[:128], S_ref[192:]])[:, 64].astype(np.float64)
    scales = [None, None, None, None, np.abs(start[4]).astype(np.float64) + np.abs(t0[:, None] * w_ih.astype(np.float64)).sum(0)]
    for name, g, r, k, sc in zip(GRAD_NAMES, got, ref, kp, scales):
        check('%s %s' % (tag, name), g, r, k, sc)


@pytest.mark.parametrize('mode,h_bf16', VARIANTS)
@pytest.mark.parametrize('M', [130, 327])
def test_parameter_gradient_chain(M, mode, h_bf16):
    """kernel partials -> colsum (as functional.dur_bwd_fused calls it) -> ptv_dur_bwd_finalize, into non-zero gradient buffers"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    W, states, gates, ddur, idx = bwd_case(M, mode, h_bf16)
    nblk = min(256, (M + 63) // 64)
    _, _, part = run_bwd(M, W, states, gates, ddur, idx, h_bf16, nblk, keep=True)
    S = F_.colsum(torch.zeros(1, part.shape[1], device=DEV), part)
    start = grad_start(np.random.RandomState(M), 5)
    got = run_finalize(S, start, W['w_ih'], W['sos'])
    (_, S_ref), (_, S_kp) = bwd_ref(W, states, gates, ddur, idx)
    check_finalize('chain ' + vtag(mode, h_bf16), got, S_ref, S_kp, start, W['w_ih'], W['sos'])


@pytest.mark.parametrize('I', [2, 5, 8])
def test_finalize_alone(I):
    """ptv_dur_bwd_finalize on a random S: every row and column of S distinct, so a wrong row or class column shows"""
    rng = np.random.RandomState(30 + I)
    S = rng.normal(0, 1, (256, 80)).astype(np.float32)
    S[:, 67:] = 0
    w_ih, sos = rng.normal(0, 1, (3 * H, I)).astype(np.float32), rng.uniform(0, 1, I).astype(np.float32)
    start = grad_start(rng, I)
    got = run_finalize(dev(S), start, w_ih, sos)
    check_finalize('finalize', got, S.astype(np.float64), S, start, w_ih, sos)


def test_finalize_refuses_input_widths_outside_2_to_8():
    rng = np.random.RandomState(3)
    S = dev(rng.normal(0, 1, (256, 80)).astype(np.float32))
    for I in (1, 9, 0):
        w_ih, sos = np.ones((3 * H, 9), np.float32), np.ones(9, np.float32)
        start = grad_start(rng, 9)
        got = run_finalize(S, start, w_ih, sos, expect_rc=-1, I=I)
        assert all(g.tobytes() == s.tobytes() for g, s in zip(got, start))


# ================================================================================================ output layer
@pytest.mark.parametrize('Hh', [64, 20])
@pytest.mark.parametrize('rows', [1, 15, 16, 17, 130])
def test_out_token(rows, Hh):
    """ptv_dur_out_token at any H, writing est_dur_d at column 2 d of ld_out = 10; idx absent, free-running and forced"""
    rng = np.random.RandomState(rows + Hh)
    h = rng.normal(0, 1, (rows, Hh)).astype(np.float32)
    h[rows // 2] = 0                                                                 # est = b_out
    w, b = rng.normal(0, 0.3, (2, Hh)).astype(np.float32), np.array([0.25, 0.25], np.float32)          # ... an exact tie: token 0
    est_ref, idx_ref = R.dur_out_token(h, w, b)
    kp = R.kp_out_token(h, w, b)
    scale = np.abs(b).astype(np.float64) + np.abs(h.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    bound, _ = bound_of(est_ref, kp, scale)
    force = rng.randint(0, 2, rows).astype(np.int32)
    for d, mode in enumerate(('null', 'free', 'forced', 'free', 'forced')):
        dur = torch.full(((rows + 1) * 10,), float(SENT), device=DEV)
        idx = torch.full((rows + 1,), ISENT, dtype=torch.int32, device=DEV)
        K.leaf('ptv_dur_out_token', dev(h), Hh, dev(w), dev(b), dur[2 * d:], 10, None if mode == 'null' else idx,
               dev(force) if mode == 'forced' else None, rows)
        torch.cuda.synchronize()
        out, got_idx = host(dur).reshape(rows + 1, 10), host(idx)
        mask = np.zeros((rows + 1, 10), bool)
        mask[:rows, 2 * d:2 * d + 2] = True
        assert (out[~mask] == SENT).all() and got_idx[rows] == ISENT
        est = out[:rows, 2 * d:2 * d + 2]
        check('out_token H%d' % Hh, est, est_ref, kp, scale)
        if mode == 'null':
            assert (got_idx == ISENT).all()
        elif mode == 'forced':
            assert np.array_equal(got_idx[:rows], force)
        else:
            assert np.array_equal(got_idx[:rows], (est[:, 1] > est[:, 0]).astype(np.int32))          # its own rule, exactly
            sure = np.abs(est_ref[:, 1] - est_ref[:, 0]) > 2 * bound.max(1)
            assert np.array_equal(got_idx[:rows][sure], idx_ref[sure]) and got_idx[rows // 2] == 0


@pytest.mark.parametrize('rows', [1, 31, 32, 33, 130, 32 * 256 + 5])           # the last: over the ordered reduction's 256-block cap
def test_out_wgrad(rows):
    rng = np.random.RandomState(rows)
    ddur = rng.normal(0, 0.1, (rows, 10)).astype(np.float32)
    dead = np.repeat(rng.rand(rows, 5) < 0.5, 2, axis=1)
    if rows > 1:
        ddur[dead] = 0                                                               # ignored targets: both gradients of a step zero
    ddur[rows // 2, 0] = 0                                                           # one of the two zero: the step is live
    hpl = R.bf16_round(rng.normal(0, 0.5, (5, rows, H)).astype(np.float32))
    ld_dd = 12
    db = np.full((rows, ld_dd), NAN, np.float32)
    db[:, :10] = ddur
    hb = np.full((6, rows, H), NAN, np.float32)                                      # plane 0 (h_0) is not read
    hb[1:] = hpl
    for d in range(5):
        hb[d + 1][(ddur[:, 2 * d:2 * d + 2] == 0).all(1)] = NAN                      # "its state is not read"
    start = rng.normal(0, 1, (2, H)).astype(np.float32)
    ref = start.astype(np.float64) + R.dur_out_wgrad(ddur, hpl)
    kp = R.kp_out_wgrad(ddur, hpl, start)
    scale = np.abs(start).astype(np.float64) + R.dur_out_wgrad(np.abs(ddur), np.abs(hpl))
    L = lib()
    dd, hd = dev(db), dev(hb, BF)

    def run():
        gw = dev(np.concatenate([start.reshape(-1), [SENT]]).astype(np.float32))
        K.leaf('ptv_dur_out_wgrad', dd, ld_dd, hd, rows * H, gw, rows, H)
        torch.cuda.synchronize()
        out = host(gw)
        assert out[-1] == SENT
        return out[:-1].reshape(2, H)
    try:
        assert L.ptv_ordered_reductions(1) == 0
        fb = L.ptv_ordered_fallbacks(0)
        a, b = run(), run()
        assert L.ptv_ordered_fallbacks(0) == fb                                      # the ordered path had its workspace
        assert a.tobytes() == b.tobytes()                                            # ... and adds in a fixed order
        check('out_wgrad ordered', a, ref, kp, scale)
        assert L.ptv_ordered_reductions(0) == 0
        check('out_wgrad atomics', run(), ref, kp, scale)
    finally:
        L.ptv_ordered_reductions(1)
    for bad in (dict(ld=11), dict(H=32), dict(plane=rows * H + 4)):
        gw = dev(start)
        assert K.leaf_rc('ptv_dur_out_wgrad', dd, bad.get('ld', ld_dd), hd, bad.get('plane', rows * H), gw, rows, bad.get('H', H)) != 0
        torch.cuda.synchronize()
        assert host(gw).tobytes() == start.tobytes()
