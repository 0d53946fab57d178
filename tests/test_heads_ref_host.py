"""CPU guard of tests/heads_ref.py, the oracle of tests/test_gpu_heads_kernels.py: the float64 formulas of the per-note heads against torch's
float64 linear layers and autograd, the kernel-precision evaluation against torch's bf16 conversions, the pack layout against the
sentences of include/ptvae_hip.h (a transposed source, un-packing, the columns a lane of a pair of tiles owns), the dead-row predictors
against a per-row evaluation of the header's sentences -- and, over the GPU file's own parameter lists (imported, not copied), the
precondition that makes its bit-for-bit comparison legitimate: every partial sum of every integer case below 2^23."""
import numpy as np
import pytest
import torch

import heads_ref as R
import test_gpu_heads_kernels as G

F4, F8 = np.float32, np.float64


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def test_fwd_and_bwd_are_torchs_float64_linears_and_autograd():
    c = R.real_case(np.random.RandomState(1), 37)
    hn = _t(c['hn']).double().requires_grad_()
    w_p, w_dh, b_p, b_dh = (_t(c[k]).double() for k in ('w_p', 'w_dh', 'b_p', 'b_dh'))
    pitch = torch.nn.functional.linear(hn, w_p, b_p)
    pitch.retain_grad()
    hd0 = torch.nn.functional.linear(torch.cat([hn, pitch], dim=1), w_dh, b_dh)
    got = R.fwd(c['hn'], c['w_p'], c['w_dh'], c['b_p'], c['b_dh'])
    assert got[0].dtype == F8 and got[1].dtype == F8
    assert np.allclose(got[0], pitch.detach().numpy(), rtol=1e-13, atol=1e-13) and np.allclose(got[1], hd0.detach().numpy(), rtol=1e-13, atol=1e-13)
    ((pitch * _t(c['dp']).double()).sum() + (hd0 * _t(c['dhd0']).double()).sum()).backward()
    dpp, dn = R.bwd(c['dp'], c['dhd0'], c['w_p'], c['w_dh'])
    assert np.allclose(dpp, pitch.grad.numpy(), rtol=1e-13, atol=1e-13) and np.allclose(dn, hn.grad.numpy(), rtol=1e-13, atol=1e-13)


def test_kp_is_the_float32_evaluation_with_torchs_bf16_roundings():
    c = R.real_case(np.random.RandomState(2), 37)
    r = lambda x: _t(np.asarray(x, F4)).to(torch.bfloat16).float()
    hn, w_p, w_dh = r(c['hn']), r(c['w_p']), r(c['w_dh'])
    pitch = hn @ w_p.t() + _t(c['b_p'])
    hd0 = hn @ w_dh[:, :512].t() + r(pitch.numpy()) @ w_dh[:, 512:].t() + _t(c['b_dh'])
    got = R.kp_fwd(c['hn'], c['w_p'], c['w_dh'], c['b_p'], c['b_dh'])
    assert all(g.dtype == F4 for g in got)
    assert np.allclose(got[0], pitch.numpy(), rtol=0, atol=2e-6) and np.allclose(got[1], hd0.numpy(), rtol=0, atol=2e-5)
    assert np.array_equal(got[2], r(got[1]).numpy())
    dh = r(c['dhd0'])
    dpp = _t(c['dp']) + dh @ w_dh[:, 512:]
    dpk, dn, dy = R.kp_bwd(c['dp'], c['dhd0'], c['w_p'], c['w_dh'])
    assert np.allclose(dpk, dpp.numpy(), rtol=0, atol=1e-6)
    assert np.allclose(dn, (r(dpk) @ w_p + dh @ w_dh[:, :512]).numpy(), rtol=2.0 ** -7, atol=1e-6) and R.bf16_round(dn).tolist() == dn.tolist()
    assert dy.shape == (37, 200) and np.array_equal(dy[:, :130], r(dpk).numpy()) and (dy[:, 130:136] == 0).all() and np.array_equal(dy[:, 136:], dh.numpy())
    # on integers, in float64, the same functions are exact: they equal the float64 formulas wherever no rounding bites
    ci = G.case_of(17)
    p8, h8, _ = R.kp_fwd(ci['hn'], ci['w_p'], ci['w_dh'], ci['b_p'], ci['b_dh'], dt=F8)
    pf, _ = R.fwd(ci['hn'], ci['w_p'], ci['w_dh'], ci['b_p'], ci['b_dh'])
    assert np.array_equal(p8, pf)
    assert np.array_equal(h8, ci['hn'].astype(F8) @ ci['w_dh'][:, :512].T.astype(F8) + R.bf16_round(pf.astype(F4)).astype(F8) @ ci['w_dh'][:, 512:].T.astype(F8) + ci['b_dh'])
    assert (np.abs(pf) > 256).any() and (R.bf16_round(pf.astype(F4)) != pf).any(), 'no logit of the integer case is rounded'


def test_bf16_bits_and_tie_values():
    a = R.tie_values(np.random.RandomState(3), (40, 30))
    want = _t(a).to(torch.bfloat16)
    assert np.array_equal(R.bf16_bits(a).view(np.int16), want.view(torch.int16).numpy())
    assert np.array_equal(R.bits_f32(R.bf16_bits(a)), want.float().numpy())
    u = a.view(np.uint32)
    ties = (u & 0xFFFF) == 0x8000
    assert ties.sum() > 100 and set(((u[ties] >> 16) & 1).tolist()) == {0, 1}
    one = R.tie_values(np.random.RandomState(4), (1, 1))
    assert one.shape == (1, 1) and np.isfinite(one).all()


@pytest.mark.parametrize('N,K,pairs,NT,kb0,KBtot', [(17, 33, 0, 2, 0, 2), (130, 64, 0, 9, 0, 2), (64, 130, 1, 4, 0, 5), (48, 33, 1, 4, 1, 4), (1, 1, 0, 3, 2, 3)])
def test_pack_transposed_source_and_unpack(N, K, pairs, NT, kb0, KBtot):
    rng = np.random.RandomState(N + K)
    W = R.tie_values(rng, (N, K))
    stored = np.full((N, K + 3), np.nan, F4)
    stored[:, :K] = W
    stored_t = np.full((K, N + 5), np.nan, F4)
    stored_t[:, :N] = W.T
    sent = np.full((NT, KBtot, 64, 8), 0x4440, np.uint16)
    P = R.pack(stored, N, K, pairs, 0, NT, kb0, KBtot, out=sent)
    assert P.dtype == np.uint16 and P.shape == (NT, KBtot, 64, 8) and (sent == 0x4440).all()
    assert np.array_equal(P, R.pack(stored_t, N, K, pairs, 1, NT, kb0, KBtot, out=sent))
    KB = R.cdiv(K, 32)
    keep = np.ones(KBtot, bool)
    keep[kb0:kb0 + KB] = False
    assert (P[:, keep] == 0x4440).all()                                            # k-blocks outside the sub-range keep what `out` held
    U = R.unpack(P, pairs, kb0, KB)
    want = np.zeros((NT * 16, KB * 32), F4)
    want[:N, :K] = R.bf16_round(W)
    assert np.array_equal(U.view(np.uint32), want.view(np.uint32))                 # the RNE-rounded matrix, zero padded
    assert np.array_equal(R.pack(stored, N, K, pairs, 0, NT, 0, KB), P[:, kb0:kb0 + KB])


def test_pairs_layout_gives_a_lane_eight_consecutive_columns():
    """the header: lane (row, quad) of the MFMA C layout owns the 8 consecutive output columns 32t + 8*quad .. +7 across the pair's two
    accumulators.  C layout of a 16 x 16 tile: lane (row, quad) holds the tile's columns 4 quad .. 4 quad + 3; the tile's column c is the
    row of W that the B fragment holds at c"""
    rows = R.pack_rows(8, 1)
    for t in range(4):
        for quad in range(4):
            own = list(rows[2 * t, 4 * quad:4 * quad + 4]) + list(rows[2 * t + 1, 4 * quad:4 * quad + 4])
            assert own == list(range(32 * t + 8 * quad, 32 * t + 8 * quad + 8))
    assert sorted(rows.ravel().tolist()) == list(range(128))
    assert np.array_equal(R.pack_rows(3, 0), np.arange(48).reshape(3, 16))
    # ... and in the packed bits: W(n, k) = (2 n + 1) 2^(k - 16), exact in bf16 and different for every (n, k)
    W = ((2.0 * np.arange(64)[:, None] + 1.0) * np.exp2(np.arange(32)[None, :] - 16.0)).astype(F4)
    assert np.array_equal(R.bf16_round(W), W) and np.unique(W).size == W.size
    P = R.bits_f32(R.pack(W, 64, 32, 1, 0, 4, 0, 1))
    for nt in range(4):
        for lane in range(64):
            c, q = lane % 16, lane // 16
            n = 32 * (nt // 2) + 8 * (c // 4) + 4 * (nt % 2) + c % 4
            assert np.array_equal(P[nt, 0, lane], W[n, 8 * q:8 * q + 8])


def test_heads_packs_shapes_and_wcat():
    rng = np.random.RandomState(5)
    w_p, w_dh = R.tie_values(rng, (130, 512)), R.tie_values(rng, (64, 642))
    pk = R.heads_packs(w_p, w_dh)
    assert {k: v.shape[:2] for k, v in pk.items()} == dict(wp=(9, 16), wdh=(4, 16), wdp=(4, 5), wdpT=(9, 2), wcat=(32, 7))
    cat = np.concatenate([np.pad(w_p.T, ((0, 0), (0, 30))), w_dh[:, :512].T], axis=1)              # [512][224]
    assert np.array_equal(pk['wcat'], R.pack(cat, 512, 224, 1, 0, 32, 0, 7))
    assert np.array_equal(R.unpack(pk['wdpT'], 0)[:130, :64], R.bf16_round(w_dh[:, 512:].T))
    assert np.array_equal(R.unpack(pk['wp'], 0)[:130], R.bf16_round(w_p)) and (R.unpack(pk['wp'], 0)[130:] == 0).all()


def test_blocked32_is_its_index_formula():
    x = np.arange(5 * 512, dtype=F4).reshape(5, 512)
    b = R.blocked32(x)
    assert b.shape == (16, 5, 32)
    for m, u in ((0, 0), (4, 511), (3, 33), (2, 64)):
        assert b.ravel()[((u // 32) * 5 + m) * 32 + u % 32] == x[m, u]
    assert np.array_equal(R.unblocked32(b), x)


@pytest.mark.parametrize('M', G.INT_MS)
def test_exact_ok_holds_for_every_integer_case_of_the_gpu_file(M):
    c = G.case_of(M)
    for k in ('hn', 'w_p', 'w_dh', 'b_p', 'b_dh', 'dp', 'dhd0'):
        assert np.array_equal(c[k], np.rint(c[k])) and np.abs(c[k]).max() <= 4 and np.array_equal(R.bf16_round(c[k]), c[k])
    top_f, top_b = R.exact_ok(c)
    assert 0 < top_b < top_f < 2.0 ** 23
    # the worst case by hand: 512 * 16 + 4 = 8196 per logit, (8196 * 4 * 130 + 512 * 16 + 4) forward: [-4, 4] fits whatever is drawn
    worst = dict(hn=np.full((1, 512), 4, F4), w_p=np.full((130, 512), 4, F4), w_dh=np.full((64, 642), 4, F4), b_p=np.full(130, 4, F4),
                 b_dh=np.full(64, 4, F4), dp=np.full((1, 130), 4, F4), dhd0=np.full((1, 64), 4, F4))
    wf, wb = R.exact_ok(worst)
    assert top_f <= wf and top_b <= wb and 4.2e6 < wf < 4.4e6 and 5e5 < wb < 6e5
    every = set(G.SHAPE_M) | {c_['M'] for c_ in G.FWD_LIMITS + G.BWD_LIMITS + G.ROWS_CASES} | {G.RM}
    assert every == set(G.INT_MS)
    G.exact_of(M)                                                                  # (asserts that fp32 holds every predicted output)


# ---- the dead-row predictors against the header's sentences, row by row
def _brute_fwd(M, m_top, m_unit, row_len):
    out = {k: [] for k in ('pitch', 'hd0', 'hd16')}
    for row in range(M):
        first = row - row % 128                                                    # the first row of the 128-row block
        if m_top is not None and row >= (max(m_top, 0) + 1) * m_unit:             # "later rows of pitch / hd0 / hd16 stay unwritten"
            p = h = R.UNTOUCHED
        elif row_len is not None and row_len[first % m_unit] <= first // m_unit:   # "blocks whose first row has no target at their note step"
            p, h = R.ZERO, R.UNTOUCHED                                             # "logits are written as zeros, hd0 / hd16 stay unwritten"
        else:
            p = h = R.COMPUTED
        out['pitch'].append(p)
        out['hd0'].append(h)
        out['hd16'].append(h)
    return out


def _brute_bwd(M, m_top, m_unit, row_len, blocked):
    out = {k: [] for k in ('dp', 'dnsum', 'dy16')}
    live = M if m_top is None else min(M, max(0, (m_top + 1) * m_unit))
    for row in range(M):
        first = row - row % 128
        if first >= live:                                                          # a whole block of rows "known to be zero"
            d, n, y = R.UNTOUCHED, (R.UNTOUCHED if blocked & 2 else R.ZERO), R.UNTOUCHED
        elif row_len is not None and row_len[first % m_unit] <= first // m_unit:   # "their dy16 rows are zeros, their dnsum rows unwritten"
            d, n, y = R.UNTOUCHED, R.UNTOUCHED, R.ZERO
        elif row >= live:                                                          # the dead rows of a partly live block
            d, n, y = R.UNTOUCHED, R.ZERO, R.ZERO
        else:
            d = n = y = R.COMPUTED
        out['dp'].append(d)
        out['dnsum'].append(n)
        out['dy16'].append(y)
    return out


def test_dead_row_predictors_agree_with_the_header_row_by_row():
    seen = set()
    for lim in G.FWD_LIMITS + G.ROWS_CASES + [dict(M=300, m_unit=0, m_top=None)]:
        rl = G.ROW_LENS[lim['row_len']] if 'row_len' in lim else None
        got, want = R.dead_fwd(lim['M'], lim['m_top'], lim['m_unit'], rl), _brute_fwd(lim['M'], lim['m_top'], lim['m_unit'], rl)
        for k in want:
            assert got[k].tolist() == want[k], (lim, k)
            seen |= {('fwd', k, v) for v in want[k]}
    for lim in G.BWD_LIMITS + G.ROWS_CASES + [dict(M=300, m_unit=0, m_top=None)]:
        rl = G.ROW_LENS[lim['row_len']] if 'row_len' in lim else None
        for blocked in (0, 1, 2, 3):
            got, want = R.dead_bwd(lim['M'], lim['m_top'], lim['m_unit'], rl, blocked), _brute_bwd(lim['M'], lim['m_top'], lim['m_unit'], rl, blocked)
            for k in want:
                assert got[k].tolist() == want[k], (lim, blocked, k)
                seen |= {('bwd', k, v) for v in want[k]}
    # the limit cases reach every state of every output that the header names
    assert seen == ({('fwd', 'pitch', v) for v in (0, 1, 2)} | {('fwd', k, v) for k in ('hd0', 'hd16') for v in (0, 2)} |
                    {('bwd', 'dp', v) for v in (0, 2)} | {('bwd', k, v) for k in ('dnsum', 'dy16') for v in (0, 1, 2)})
    # the partly live block of m_unit = 96, *m_top = 0 on M = 300, spelled out
    p = R.dead_bwd(300, 0, 96, None, 2)
    assert p['dnsum'][:96].tolist() == [0] * 96 and p['dnsum'][96:128].tolist() == [1] * 32 and (p['dnsum'][128:] == 2).all()
    assert p['dy16'][96:128].tolist() == [1] * 32 and (p['dy16'][128:] == 2).all() and (p['dp'][96:] == 2).all()
