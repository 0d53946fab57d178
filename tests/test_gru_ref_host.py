"""Guards tests/gru_ref.py, the fp64 references of the step-GRU kernel tests: the forward against torch.nn.GRU in float64 (and, with
lengths, an explicit torch.where loop), the backward against float64 autograd, the kernel-precision evaluations against the references
with no rounding configured, and the case list of tests/test_gpu_gru_kernels.py against the host mirrors of the dispatch: every case on
the variant and tile it names, every variant x tile reached, every pipeline hand-over straddled.  No GPU.  fp64 against fp64: 1e-12."""
import numpy as np
import pytest
import torch

import gru_ref as R
import test_gpu_gru_kernels as G

TOL = 1e-12
F8 = torch.float64


def close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.allclose(got, want, rtol=tol, atol=tol), np.abs(got - want).max()


def chain(M, H, T, I, seed):
    rng = np.random.RandomState(seed)
    gru = torch.nn.GRU(I, H).to(F8)
    x, h0 = rng.normal(0, 1, (T, M, I)), rng.normal(0, 0.5, (M, H))
    p = {k: v.detach().numpy() for k, v in gru.named_parameters()}
    gi = x @ p['weight_ih_l0'].T + p['bias_ih_l0']
    return gru, x, h0, p, gi


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('M,H,T', [(1, 4, 1), (5, 12, 3), (17, 24, 4)])
def test_forward_vs_torch_gru(M, H, T, reverse):
    torch.manual_seed(M + H)
    gru, x, h0, p, gi = chain(M, H, T, 7, M * H + T)
    xs = x[::-1].copy() if reverse else x                                            # the reversed chain consumes time T-1-s at step s
    want, _ = gru(torch.tensor(xs), torch.tensor(h0)[None])
    h, gates = R.gru_forward(gi, None, p['weight_hh_l0'], p['bias_hh_l0'], h0, None, reverse, None)
    close(h, want.detach().numpy())
    half = gi * 0.25                                                                 # gi2 is an addend; gi_idx gathers gi rows only
    idx = np.arange(M)[::-1].copy()
    h2, g2 = R.gru_forward((gi - half)[:, idx], half, p['weight_hh_l0'], p['bias_hh_l0'], h0, None, reverse, np.argsort(idx))
    close(h2, h), close(g2, gates)
    hp = np.concatenate([h0[None], h[:-1]])
    close(gates[:, 3], hp @ p['weight_hh_l0'][2 * H:].T + p['bias_hh_l0'][2 * H:])
    close(h, (1 - gates[:, 1]) * gates[:, 2] + gates[:, 1] * hp)


def where_loop(gi, w, b, h0, lengths, reverse):
    gi, w, b, h = (torch.tensor(a, dtype=F8) for a in (gi, w, b, h0))
    T, H = gi.shape[0], h.shape[1]
    L = torch.tensor(lengths)
    out = []
    for s in range(T):
        t = T - 1 - s if reverse else s
        gh = h @ w.T + b
        r = torch.sigmoid(gi[t][:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[t][:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[t][:, 2 * H:] + r * gh[:, 2 * H:])
        h = torch.where((t < L)[:, None], (1 - z) * n + z * h, h)
        out.append(h)
    return torch.stack(out).numpy()


@pytest.mark.parametrize('reverse', [False, True])
def test_forward_lengths_vs_where_loop(reverse):
    M, H, T = 9, 8, 4
    _, x, h0, p, gi = chain(M, H, T, 5, 3)
    lengths = np.array([0, 4, 1, 2, 3, 4, 0, 2, 4])
    assert 0 in lengths and T in lengths
    h, gates = R.gru_forward(gi, None, p['weight_hh_l0'], p['bias_hh_l0'], h0, lengths, reverse, None)
    close(h, where_loop(gi, p['weight_hh_l0'], p['bias_hh_l0'], h0, lengths, reverse))
    assert np.array_equal(h[:, lengths == 0], np.broadcast_to(h0[lengths == 0], (T,) + h0[lengths == 0].shape))
    for s in range(T):
        dead = ~(R.time_of(s, T, reverse) < lengths)
        assert (gates[s, 0][dead] == 0).all() and (gates[s, 1][dead] == 1).all() and (gates[s, 2][dead] == 0).all()
    # h0_operand: only the product of step 0 sees it
    op = h0 + 0.25
    h_op, g_op = R.gru_forward(gi, None, p['weight_hh_l0'], p['bias_hh_l0'], h0, None, reverse, None, h0_operand=op)
    close(g_op[0, 3], op @ p['weight_hh_l0'][2 * H:].T + p['bias_hh_l0'][2 * H:])
    close(h_op[0], (1 - g_op[0, 1]) * g_op[0, 2] + g_op[0, 1] * h0)


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('lens', [False, True])
@pytest.mark.parametrize('lr_k', [0, 1, 3])
def test_backward_vs_autograd(lr_k, lens, reverse):
    M, H, T = 7, 8, 3
    rng = np.random.RandomState(10 + lr_k)
    w, b = rng.uniform(-.4, .4, (3 * H, H)), rng.uniform(-.4, .4, 3 * H)
    gi, h0 = rng.normal(0, 1, (T, M, 3 * H)), rng.normal(0, 0.5, (M, H))
    lengths = np.array([3, 0, 2, 1, 3, 0, 2]) if lens else None
    ext, last = rng.normal(0, 1, (T, M, H)), rng.normal(0, 1, (M, H))
    lr_a, lr_b = (rng.normal(0, 1, (T, M, lr_k)), rng.normal(0, 1, (lr_k, H))) if lr_k else (None, None)
    tg, tw, tb, th = (torch.tensor(a, dtype=F8, requires_grad=True) for a in (gi, w, b, h0))
    h, hs = th, []
    for s in range(T):
        t = T - 1 - s if reverse else s
        gh = h @ tw.T + tb
        r = torch.sigmoid(tg[t][:, :H] + gh[:, :H])
        z = torch.sigmoid(tg[t][:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(tg[t][:, 2 * H:] + r * gh[:, 2 * H:])
        new = (1 - z) * n + z * h
        h = new if lengths is None else torch.where((t < torch.tensor(lengths))[:, None], new, h)
        hs.append(h)
    hs = torch.stack(hs)
    loss = (hs * torch.tensor(ext)).sum() + (hs[-1] * torch.tensor(last)).sum()
    if lr_k:
        loss = loss + (torch.tensor(lr_a @ lr_b) * hs).sum()
    loss.backward()
    hf, gates = R.gru_forward(gi, None, w, b, h0, lengths, reverse, None)
    hprev = np.concatenate([h0[None], hf[:-1]])
    dgi, dgh, dh0, dhz = R.gru_backward(hprev, gates, w, ext, last, lr_a, lr_b, reverse)
    close(dgi, tg.grad.numpy()), close(dh0, th.grad.numpy())
    close(dgh.sum((0, 1)), tb.grad.numpy())
    close(np.einsum('smg,smh->gh', dgh, hprev), tw.grad.numpy())
    # None operands are zeros; dh_last arrives at step T-1 only
    e2 = ext.copy()
    e2[-1] += last
    for a, c in zip(R.gru_backward(hprev, gates, w, e2, None, lr_a, lr_b, reverse), (dgi, dgh, dh0, dhz)):
        close(a, c)
    close(dh0, dgh[0] @ w + dhz)


def test_kernel_precision_evaluations_are_the_same_formulas():
    """with no rounding configured the kp functions follow the fp64 ones to fp32 round-off (1e-6 of each array's scale)"""
    M, H, T = 19, 24, 3
    rng = np.random.RandomState(4)
    f4 = lambda a: a.astype(np.float32)
    w, b = f4(rng.uniform(-.2, .2, (3 * H, H))), f4(rng.uniform(-.2, .2, 3 * H))
    gi, gi2, h0 = f4(rng.normal(0, 1, (T, 3, 3 * H))), f4(rng.normal(0, .5, (T, M, 3 * H))), f4(rng.normal(0, .5, (M, H)))
    lengths, idx = G.lengths_of(M, T), np.arange(M) % 3
    rel = lambda a, r: np.abs(a - r).max() / np.abs(r).max()
    for reverse in (False, True):
        for op in (None, f4(h0 + 0.125)):
            a = (gi, gi2, w, b, h0, lengths, reverse, idx, op)
            (h, g), (hk, gk, h16) = R.gru_forward(*a), R.kp_forward(*a)
            assert rel(hk, h) < 1e-6 and all(rel(gk[:, p], g[:, p]) < 1e-6 for p in range(4))
            assert np.array_equal(h16, R.bf16_round(hk))
            hk2, gk2, _ = R.kp_forward(*a, bf16=True, gates_bf16=True)                # ... and to bf16 accuracy when it is
            assert 1e-5 < rel(hk2, h) < 2e-2 and R.is_bf16(gk2)
        hp = np.concatenate([h0[None], f4(h[:-1])])
        ext, last = f4(rng.normal(0, 1, (T, M, H))), f4(rng.normal(0, 1, (M, H)))
        for k in (0, 2, 3):
            lr_a, lr_b = (f4(rng.normal(0, 1, (T, M, k))), f4(rng.normal(0, 1, (k, H)))) if k else (None, None)
            a = (hp, f4(g), w, ext, last, lr_a, lr_b, reverse)
            for x, y in zip(R.kp_backward(*a), R.gru_backward(*a)):
                assert rel(x, y) < 1e-6
            kb = R.kp_backward(*a, bf16=True, dg_bf16=True)
            assert R.is_bf16(kb[0]) and R.is_bf16(kb[1]) and all(rel(x, y) < 2e-2 for x, y in zip(kb, R.gru_backward(*a)))


# ================================================================================================ the GPU file's case list
def fwd_list():
    return [(k, None) for k in G.FWD_SMALL + G.PROBES] + [(k, tile) for tile, k in G.FWD_TILES]


def bwd_list():
    return [(k, None) for k in G.BWD_SMALL] + [(k, tile) for tile, k in G.BWD_TILES]


def test_every_case_runs_the_variant_and_tile_it_names():
    seen = {'fwd': set(), 'bwd': set()}
    for direction, cases, cfgs, names, plan in (('fwd', fwd_list(), G.FWD_CFG, G.FWD_VARIANT_OF, R.plan_fwd),
                                                ('bwd', bwd_list(), G.BWD_CFG, G.BWD_VARIANT_OF, R.plan_bwd)):
        for key, tile in cases:
            c = dict(key)
            variant, got_tile = plan(c['M'], c['H'], cfgs[c['cfg']])
            assert variant == names[c['cfg']], (key, variant)
            assert got_tile == (tile or '64x32'), (key, got_tile)
            seen[direction].add((variant, got_tile))
    # every variant on the 64x32 tile; the other tiles by the FAST and the F32 variant
    assert {v for v, t in seen['fwd'] if t == '64x32'} == set(R.FWD_VARIANTS)
    assert {v for v, t in seen['bwd'] if t == '64x32'} == set(R.BWD_VARIANTS)
    assert {(v, t) for v in ('FAST2', 'F32') for t in R.FWD_TILES} <= seen['fwd']
    assert {(v, t) for v in ('FAST', 'F32') for t in R.BWD_TILES} <= seen['bwd']
    # the features the issue lists, each on the configuration that reaches it
    f = [dict(k) | G.FWD_CFG[dict(k)['cfg']] for k in G.FWD_SMALL]
    for name in ('FAST1', 'FAST2', 'FAST1 no gates', 'FAST2 no gates'):
        own = [c for c in f if c['cfg'] == name]
        assert any(c['lengths'] for c in own) and any(not c['lengths'] for c in own)
    assert any(c['gi2_bcast'] for c in f) and any(c.get('gi2') and not c['gi2_bcast'] for c in f) and any(c['gi_pad'] for c in f)
    b = [dict(k) | G.BWD_CFG[dict(k)['cfg']] for k in G.BWD_SMALL]
    assert {c.get('lr_k', 0) for c in b if G.BWD_VARIANT_OF[c['cfg']] == 'FAST'} == {0, 1, 2}
    assert {c.get('ext') for c in b if G.BWD_VARIANT_OF[c['cfg']] == 'FAST'} == {None, 'b'}
    for cs in (f, b):
        assert {c['M'] for c in cs} == set(G.SMALL_M) and {c['T'] for c in cs} == {1, 2, 3}
        assert any(c['reverse'] and c['T'] == 3 and c['lengths'] for c in cs)
    assert any(c['no_ext'] for c in b) and any(c['no_dh0'] for c in b) and {c['last'] for c in b} == {None, 'dense', 'pad'}
    assert any(c['ext_pad'] and not c['no_ext'] for c in b) and any(c['integer'] and c['lengths'] and c['M'] > c['T'] for c in b)


def test_every_pipeline_hand_over_is_straddled():
    """a full tile (BM rows of M, BN units of H) runs gemm_body's pipeline from K = 2 PF BK on (K = H forward, 3H backward).  Per
    direction, tile and precision the list holds a full-tile launch with K at or above the hand-over and, where a full tile can have a
    smaller K at all (BN units make K >= BN or 3 BN), one below; where it cannot, a launch of that tile with a smaller K and a ragged N
    if the dispatch lets any H reach it (the backward 128x128 tile in fp32 does not: N > 64 makes K >= 204)"""
    for direction, cases, cfgs, plan in (('fwd', fwd_list(), G.FWD_CFG, R.plan_fwd), ('bwd', bwd_list(), G.BWD_CFG, R.plan_bwd)):
        per = 1 if direction == 'fwd' else 3
        full, ragged = {}, {}
        for key, _ in cases:
            c = dict(key)
            cfg = cfgs[c['cfg']]
            tile = plan(c['M'], c['H'], cfg)[1]
            bm, bn = (int(v) for v in tile.split('x'))
            if direction == 'bwd' and c['T'] == 1:                                   # (the backward's last step has K = 0)
                continue
            (full if c['M'] >= bm and c['H'] >= bn else ragged).setdefault((tile, cfg['prec']), set()).add(c['H'] * per)
        for tile in (R.FWD_TILES if direction == 'fwd' else R.BWD_TILES):
            bn = int(tile.split('x')[1])
            for prec in ('bf16', 'fp32'):
                k0 = R.handover(direction, tile, prec)
                have, step = full[(tile, prec)], 8 if prec == 'bf16' else 4
                assert max(have) >= k0, (direction, tile, prec, k0, sorted(have))
                if per * bn < k0:
                    assert min(have) < k0, (direction, tile, prec, k0, sorted(have))
                else:
                    least_h = step if tile != '128x128' else R.BWD_BIG_MIN_N + step      # the smallest H the dispatch sends to the tile
                    assert (per * least_h >= k0) or min(ragged[(tile, prec)]) < k0, (direction, tile, prec, k0)
                if tile == '64x32':                                                  # the nearest legal H on either side, and one more
                    assert {h * per for h in R.handover_H(direction, tile, prec)} <= have


def test_constants_parsed_from_the_sources():
    assert R.BK['bf16'] > 0 and R.BK['fp32'] > 0 and set(R.PF_FWD) == set(R.FWD_TILES) and set(R.PF_BWD) == set(R.BWD_TILES)
    assert R.plan_fwd(64 * R.FWD_BIG_BLOCKS, 64, dict(prec='fp32'))[1] == '64x64'
    assert R.plan_fwd(64 * R.FWD_BIG_BLOCKS - 64, 64, dict(prec='fp32'))[1] == '64x32'
    assert R.plan_bwd(128 * R.BWD_BIG_BLOCKS, R.BWD_BIG_MIN_N, dict(prec='fp32'))[1] == '64x64'         # N <= 64 never takes the 128 tile
    assert R.plan_bwd(128 * R.BWD_BIG_BLOCKS, R.BWD_BIG_MIN_N + 4, dict(prec='fp32'))[1] == '128x128'
