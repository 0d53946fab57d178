"""CPU guard of tests/wgrad_ref.py, the oracle of tests/test_gpu_wgrad_kernels.py: live_rows against a brute-force loop over rows written
from the sentences of include/ptvae_hip.h, product / colsum against torch's float64 operators -- and the CENSUS: every entry of
wgrad_ref.CASES goes through ptv_debug_wgrad_plan (host only: the job's pointers are made-up addresses, looked at for alignment) and must
report exactly the plan it was written for, in all four operand dtype combinations; the tags a case claims are re-derived from the reported
plan; and their union must cover every branch of plan_job that the GPU module is there to run."""
import ctypes

import numpy as np
import pytest
import torch

import wgrad_ref as W
from gemm_ref import ALPHAS
from polyphonic_chord_texture_disentanglement_amd import _lib

F4, F8 = np.float32, np.float64
PTV_ERR_ARG = -1
BASE_A, BASE_B, BASE_C = 0x7000000, 0x9000000, 0xB000000          # made-up, 16-byte aligned; never dereferenced


def fake_job(c, dtypes, **over):
    """ptv_wgrad_job of a CASES entry with made-up addresses: dtypes bit 0 / 1 = A / B bf16"""
    q = _lib.WgradJob()
    q.M, q.N, q.K, q.slabs = c['M'], c['N'], c['K'], c['slabs']
    q.A = BASE_A + c['offa'] * (2 if dtypes & 1 else 4)
    q.B = BASE_B + c['offb'] * (2 if dtypes & 2 else 4)
    q.C, q.ldc, q.lda, q.ldb = BASE_C, c['N'] + 5, c['lda'], c['ldb']
    q.alpha, q.accumulate, q.dtypes = 1.0, 1, dtypes
    if c['seg']:
        q.seg_n, q.seg_unit, q.seg_period = BASE_C + 0x100000, c['seg'][0], c['seg'][2]
    for k, v in over.items():
        setattr(q, k, v)
    return q


def probe(q):
    out = (ctypes.c_int * 10)(*([-7] * 10))
    rc = _lib.lib().ptv_debug_wgrad_plan(ctypes.byref(q), out)
    return rc, dict(zip(W.PLAN_FIELDS, list(out)))


# ------------------------------------------------------------------------------------------------ live_rows
def _brute(K, k_top, k_unit, k_rev, seg_n, seg_unit, seg_period):
    live = []
    for row in range(K):
        ok = True
        if k_top is not None:
            if k_rev > 0:
                ok = ok and not (row < (k_rev - k_top - 1) * k_unit)              # "the zero part is the rows BEFORE ..."
            else:
                ok = ok and not (row >= (k_top + 1) * k_unit)                     # "the rows from (*k_top + 1) * k_unit on are zero"
        if seg_n is not None:
            q = row // seg_unit
            if seg_period > 0:
                n = seg_n[q % seg_period]
            else:
                n = seg_n[abs(seg_period) - 1 - q % abs(seg_period)]
            ok = ok and (row - q * seg_unit) < n                                  # "only the first seg_n[...] rows hold anything"
        live.append(ok)
    return np.array(live, bool)


@pytest.mark.parametrize('period', [3, -3, 1, -1, 5])
def test_live_rows_is_the_brute_force_loop(period):
    unit, K = 64, 64 * 7 + 20
    seg = [64, 32, 0, 40, 8][:abs(period)]
    for k_top in (None, -1, 0, 2, 6, 7, 11):
        for k_rev in (0, 8, 5):
            for s in (None, seg):
                a = (K, k_top, 96, k_rev, s, unit, period)
                assert np.array_equal(W.live_rows(*a), _brute(*a)), a
    assert W.live_rows(10).all() and W.live_rows(0).shape == (0,)
    assert not W.live_rows(300, -1, 96).any() and W.live_rows(300, 3, 96).all()
    assert np.array_equal(np.flatnonzero(W.live_rows(300, 1, 96)), np.arange(192))
    assert np.array_equal(np.flatnonzero(W.live_rows(320, 1, 32, 10)), np.arange(256, 320))      # reversed: the LAST two units
    assert not W.live_rows(320, -1, 32, 10).any() and W.live_rows(320, 9, 32, 10).all()
    # a negative period reads seg_n backwards: unit 0 takes the last count
    assert np.array_equal(W.live_rows(8, None, 0, 0, [1, 3], 4, -2), np.array([1, 1, 1, 0, 1, 0, 0, 0], bool))
    assert np.array_equal(W.live_rows(8, None, 0, 0, [1, 3], 4, 2), np.array([1, 0, 0, 0, 1, 1, 1, 0], bool))


def test_product_and_colsum_are_torchs_float64_operators():
    rng = np.random.RandomState(4)
    A, B = rng.standard_normal((37, 13)).astype(F4), rng.standard_normal((37, 9)).astype(F4)
    C0, b0 = rng.standard_normal((13, 9)).astype(F4), rng.standard_normal(13).astype(F4)
    live = W.live_rows(37, 1, 8)
    Bn = B.copy()
    Bn[~live] = np.nan
    tA, tB = torch.from_numpy(A).double(), torch.from_numpy(B).double()
    for alpha in ALPHAS:
        for acc in (0, 1):
            want = alpha * (tA.t() @ tB) + (torch.from_numpy(C0).double() if acc else 0)
            got = W.product(A, B, None, alpha, C0, acc)
            assert got.dtype == F8 and np.allclose(got, want.numpy(), rtol=1e-13, atol=1e-13)
            wl = alpha * (tA[:16].t() @ tB[:16]) + (torch.from_numpy(C0).double() if acc else 0)
            gl = W.product(A, Bn, live, alpha, C0, acc)
            assert np.isfinite(gl).all() and np.allclose(gl, wl.numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(W.colsum(A, None, b0), (tA.sum(0) + torch.from_numpy(b0).double()).numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(W.colsum(A, live), tA[:16].sum(0).numpy(), rtol=1e-13, atol=1e-13)
    none = np.zeros(37, bool)
    assert (W.product(A, Bn, none) == 0).all() and np.array_equal(W.product(A, Bn, none, 1.0, C0, 1), C0.astype(F8))
    assert np.array_equal(W.colsum(A, none, b0), b0.astype(F8))
    assert np.allclose(W.abs_product(A, Bn, live), (tA[:16].abs().t() @ tB[:16].abs()).numpy(), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ the census
@pytest.mark.parametrize('name', list(W.CASES))
def test_every_case_reports_the_plan_it_was_written_for(name):
    c = W.CASES[name]
    for dtypes in (3, 2, 1, 0):
        rc, got = probe(fake_job(c, dtypes))
        assert rc == 0 and got == c['expect'], (name, dtypes, got, c['expect'])
    assert set(c['reaches']) <= W.tags_of(c, got), (name, c['reaches'], W.tags_of(c, got))
    # what the plan means in rows: the slabs of a part cover its rows, and only map 1 may carry slabs beyond them
    e, K = c['expect'], c['K']
    for w, kn in (('fast', e['kfast']), ('tail', K - e['kfast'])):
        ns, kper, mp = e['nslab_' + w], e['kper_' + w], e['map_' + w]
        if kn == 0:
            assert (ns, kper, mp) == (0, 0, 0)
            continue
        assert ns * kper >= kn and kper % 32 == 0 and (mp == 1 or (ns - 1) * kper < kn)
        if mp == 1:
            assert ns % 8 == 0
        if mp == 2:
            assert (e['tiles_m'] * e['tiles_n']) % 8 == 0
        if c['seg']:
            assert c['seg'][0] % kper == 0 and kper >= 128                         # a slab never straddles a unit
    if c['seg']:
        unit, n, period = c['seg']
        assert K % unit == 0 and K // unit > abs(period) - (1 if 'seg_tail' in c['reaches'] else 0) and all(v % 32 == 0 and 0 <= v <= unit for v in n) and len(n) == abs(period)
        assert _lib.lib().ptv_wgrad_seg_supported(K, unit) == 1
        assert any(v % 128 for v in n)                                             # multiples of 32 that are no multiple of 128


def test_the_cases_cover_every_branch_of_the_plan():
    seen = {}
    for name, c in W.CASES.items():
        rc, got = probe(fake_job(c, 3))
        assert rc == 0
        for t in W.tags_of(c, got) & set(c['reaches']):
            seen.setdefault(t, []).append(name)
    missing = [t for t in W.CENSUS if t not in seen]
    assert not missing, 'no case of wgrad_ref.CASES reaches: %s' % ', '.join(missing)
    assert set(W.CENSUS) >= {'map0', 'map1', 'map2', 'seg_map0', 'seg_map1', 'seg_map2', 'fast_only', 'tail_only', 'fast_tail',
                             'single_slab', 'map1_beyond_k', 'seg_map1_padded', 'maxs', 'deep', 'explicit'}
    # the two tail-meets-segment cases differ in exactly what the tail finds: 32 live rows of unit 3, or none
    for nm, live in (('seg_tail_live', 32), ('seg_tail_dead', 0)):
        c = W.CASES[nm]
        kf = c['expect']['kfast']
        assert int(W.live_rows(c['K'], None, 0, 0, c['seg'][1], c['seg'][0], c['seg'][2])[kf:].sum()) == live
    # a unit of three slabs: one full, one clipped to 32 rows, one dead
    c = W.CASES['seg_unit384']
    lv = W.live_rows(c['K'], None, 0, 0, c['seg'][1], c['seg'][0], c['seg'][2])[:384].reshape(3, 128).sum(1)
    assert lv.tolist() == [128, 32, 0]


def test_the_probe_launches_nothing_and_plans_only_what_would_run():
    c = W.CASES['tail32']
    for over in (dict(M=0), dict(N=0), dict(K=0)):
        rc, got = probe(fake_job(c, 3, **over))
        assert rc == 0 and set(got.values()) == {0}
    assert _lib.lib().ptv_debug_wgrad_plan(None, (ctypes.c_int * 10)()) == PTV_ERR_ARG
    assert _lib.lib().ptv_debug_wgrad_plan(ctypes.byref(fake_job(c, 3)), None) == PTV_ERR_ARG
    # fp32 rows of 4 elements are aligned where bf16 rows are not: the plan follows the dtype
    q = dict(W.CASES['one_slab'], lda=132, ldb=132)
    assert probe(fake_job(q, 0))[1]['kfast'] == 96 and probe(fake_job(q, 3))[1]['kfast'] == 0


@pytest.mark.parametrize('over', [dict(M=-1), dict(N=-1), dict(K=-1), dict(A=None), dict(B=None), dict(C=None),
                                  dict(k_top=BASE_C, k_unit=48), dict(k_top=BASE_C, k_unit=0), dict(k_top=BASE_C, k_unit=-32)])
def test_the_probe_refuses_what_the_product_refuses(over):
    rc, got = probe(fake_job(W.CASES['map0_explicit3'], 3, **over))
    assert rc == PTV_ERR_ARG and set(got.values()) == {-7}


def test_the_probe_refuses_unsupported_segments():
    c = W.CASES['seg_map0']
    assert probe(fake_job(c, 3, seg_period=0))[0] == PTV_ERR_ARG
    assert probe(fake_job(c, 3, seg_unit=64))[0] == PTV_ERR_ARG
    assert probe(fake_job(dict(c, K=2 * 128 * 129), 3, seg_unit=128 * 129))[0] == PTV_ERR_ARG
    assert probe(fake_job(c, 3, seg_unit=384))[0] == PTV_ERR_ARG                    # 512 rows are no whole number of 384-row units
    assert probe(fake_job(c, 3, seg_period=-2))[0] == 0


def seg_rule(K, unit):
    """ptv_wgrad_seg_supported as include/ptvae_hip.h words it"""
    if K <= 0 or unit < 128 or unit % 128 or K % unit:
        return 0
    p = 128
    while unit % (2 * p) == 0:
        p *= 2
    return 1 if W.cdiv(K, p) <= 248 else 0


def test_seg_supported_follows_its_documented_rule():
    f = _lib.lib().ptv_wgrad_seg_supported
    for unit in (0, 64, 96, 128, 192, 256, 384, 512, 640, 1024, 16384, 128 * 129, 3 * 4096):
        for units in (0, 1, 2, 3, 15, 16, 31, 62, 82, 83, 124, 125, 248, 249, 496, 497):
            K = unit * units
            assert f(K, unit) == seg_rule(K, unit), (K, unit)
            if unit:
                assert f(K + 32, unit) == seg_rule(K + 32, unit)
    assert f(248 * 128, 128) == 1 and f(249 * 128, 128) == 0                        # 248 and 249 slabs' worth
    assert f(3 * 83 * 128, 384) == 0 and f(3 * 82 * 128, 384) == 1                  # the slab stays 128 rows in a 384-row unit
    assert f(15 * 16384, 16384) == 1 and f(2 * 128 * 129, 128 * 129) == 0 and f(-128, 128) == 0
