"""Guards tests/pgru_ref.py, the oracle side of tests/test_gpu_pgru_kernels.py: the exchange layout against the header's index formula,
the reference functions as that file calls them against torch float64 (nn.GRU where it applies, an explicit masked loop and autograd
otherwise), the kernel-precision evaluation against the reference, and the case table against the host mirrors of the dispatch of
csrc/gru_persist.hip at 256 CUs: every instantiation, both block_map branches, RG > 1, empty row groups, every H and NC.  No GPU."""
import numpy as np
import pytest
import torch

import pgru_ref as P

TOL = 1e-11
F8 = torch.float64
NCU = 256


def close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.allclose(got, want, rtol=tol, atol=tol), np.abs(got - want).max()


@pytest.mark.parametrize('M,K', [(1, 8), (5, 24), (64, 256), (130, 768)])
def test_blocked_round_trip_and_index_formula(M, K):
    a = np.arange(M * K, dtype=np.float32).reshape(M, K)
    x = P.blocked(a)
    assert x.shape == (K // 8, M, 8)
    flat = x.reshape(-1)
    rows, ks = np.meshgrid(np.arange(M), np.arange(K), indexing='ij')
    assert np.array_equal(flat[((ks // 8) * M + rows) * 8 + ks % 8], a)              # include/ptvae_hip.h: [k/8][row][8]
    assert np.array_equal(P.unblocked(flat, M, K), a)


def torch_chain(ins, want_grads):
    """the chain in torch float64: a masked loop over processing steps; loss = sum(ext . h) + last . h_T"""
    gi, w, b, h0 = (torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in (ins['gi'], ins['w'], ins['b'], ins['h0']))
    T, M, H = gi.shape[0], h0.shape[0], h0.shape[1]
    gi2 = None if ins['gi2'] is None else torch.tensor(np.asarray(ins['gi2'], np.float64))
    L = None if ins['lengths'] is None else torch.tensor(ins['lengths'])
    h, hs, pre = h0, [], []
    for s in range(T):
        t = T - 1 - s if ins['reverse'] else s
        x = gi[t] if gi2 is None else gi[t] + gi2[t if gi2.shape[0] > 1 else 0]
        gh = h @ w.T + b
        gh.retain_grad(), x.retain_grad()
        r = torch.sigmoid(x[:, :H] + gh[:, :H])
        z = torch.sigmoid(x[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(x[:, 2 * H:] + r * gh[:, 2 * H:])
        new = (1 - z) * n + z * h
        h = new if L is None else torch.where((t < L)[:, None], new, h)
        hs.append(h), pre.append((t, x, gh))
    hs = torch.stack(hs)
    if not want_grads:
        return hs.detach().numpy()
    loss = hs.sum() * 0
    if ins['ext'] is not None:
        loss = loss + (hs * torch.tensor(np.asarray(ins['ext'], np.float64))).sum()
    if ins['last'] is not None:
        loss = loss + (hs[-1] * torch.tensor(np.asarray(ins['last'], np.float64))).sum()
    loss.backward()
    dgi = np.zeros((T, M, 3 * H))
    dgh = np.zeros((T, M, 3 * H))
    for s, (t, x, gh) in enumerate(pre):
        dgi[t] = x.grad.numpy() if x.grad is not None else 0
        dgh[s] = gh.grad.numpy() if gh.grad is not None else 0
    return hs.detach().numpy(), dgi, dgh, h0.grad.numpy()


SMALL = [P.CASES[0], P.CASES[1], P.CASES[12], P.CASES[15], P._case(40, 256, 2, NC=2, lengths=True, gi2='step', last='pad')]


@pytest.mark.parametrize('case', SMALL, ids=P.case_id)
def test_reference_vs_torch_float64(case):
    """every chain of the table's smallest launches: odd chains reversed, masked rows (length 0 included), gi2 broadcast and per step,
    dh_last + dh_ext + dh0"""
    for ch in range(case['NC']):
        ins = P.chain_inputs(case, ch)
        st, gates = P.forward(ins['gi'], ins['gi2'], ins['w'], ins['b'], ins['h0'], ins['lengths'], ins['reverse'])
        hs, dgi_t, dgh_t, dh0_t = torch_chain(ins, True)
        close(st[1:], hs)
        assert np.array_equal(st[0], ins['h0'])
        if ins['lengths'] is not None:
            assert 0 in ins['lengths'] or case['M'] < 3
            dead0 = ins['lengths'] == 0
            assert np.array_equal(st[:, dead0], np.broadcast_to(st[0, dead0], st[:, dead0].shape))
        dgi, dgh, dh0 = P.backward(st[:-1], gates, ins['w'], ins['ext'], ins['last'], ins['reverse'])
        close(dgi, dgi_t), close(dgh, dgh_t), close(dh0, dh0_t)


def test_forward_vs_nn_gru():
    case = P.CASES[1]
    ins = P.chain_inputs(dict(case, lengths=False, gi2=None), 0)
    M, H, T = case['M'], case['H'], case['T']
    torch.manual_seed(1)
    gru = torch.nn.GRU(3 * H, H).to(F8)                                # gi = x . I + 0: the input side is the identity
    with torch.no_grad():
        gru.weight_hh_l0.copy_(torch.tensor(ins['w'], dtype=F8)), gru.bias_hh_l0.copy_(torch.tensor(ins['b'], dtype=F8))
        gru.weight_ih_l0.copy_(torch.eye(3 * H, dtype=F8)), gru.bias_ih_l0.zero_()
        want, _ = gru(torch.tensor(ins['gi'], dtype=F8), torch.tensor(ins['h0'], dtype=F8)[None])
    st, _ = P.forward(ins['gi'], None, ins['w'], ins['b'], ins['h0'], None, False)
    close(st[1:], want.numpy())
    assert (M, T) == (40, 2)


def test_kernel_precision_evaluation_is_close_to_the_reference():
    """kp_* is the yardstick, no reference: its distance is bf16-sized, and it reproduces the reference's masked rows exactly"""
    case = P.CASES[1]
    ins = P.chain_inputs(case, 0)
    ref = P.chain_reference(ins)
    assert 0 < np.abs(ref['kst'] - ref['st']).max() < 2e-2
    assert np.abs(ref['kgates'] - ref['gates']).max() < 2e-2
    for got, want in zip(ref['kbwd'], ref['bwd']):
        assert 0 < np.abs(got - want).max() < 2e-2 * max(1.0, np.abs(want).max())
    dead0 = ins['lengths'] == 0
    assert dead0.any() and np.array_equal(ref['kst'][:, dead0], np.broadcast_to(ins['h0'][dead0], ref['kst'][:, dead0].shape))
    assert np.array_equal(ref['kst16'], P.bf16_round(ref['kst']))


# ================================================================================================ the table against the dispatch
def test_plan_mirror_known_answers():
    """worked by hand from plan() of gru_persist.hip"""
    assert P.plan(256, 1, 512, 1024) == dict(RG=4, rows=128, FM=2)
    assert P.plan(256, 1, 257, 256) == dict(RG=4, rows=128, FM=2) and P.empty_groups(P.plan(256, 1, 257, 256), 257) == 1
    assert P.plan(256, 1, 520, 256) == dict(RG=8, rows=128, FM=2) and P.empty_groups(P.plan(256, 1, 520, 256), 520) == 3
    assert P.plan(256, 3, 300, 256) == dict(RG=4, rows=128, FM=2) and P.block_map_branch(3, 4, 256) == 'plain'
    assert P.plan(16, 1, 130, 256) == dict(RG=1, rows=256, FM=4)
    assert P.plan(16, 1, 300, 256) is None and P.plan(16, 1, 300, 256, 8) == dict(RG=1, rows=512, FM=8)
    assert P.plan(256, 4, 1024, 1024) is None and P.plan(256, 5, 64, 256) is None and P.plan(256, 0, 64, 256) is None
    assert all(P.plan(256, 1, 64, H) is None for H in (128, 384, 1280)) and P.plan(256, 1, 0, 256) is None
    assert P.plan(15, 1, 64, 256) is None                                  # fewer CUs than unit groups
    assert P.plan(1024, 1, 4096, 256) is None and P.plan(512, 1, 4096, 256) == dict(RG=32, rows=128, FM=2)      # 32 row-group counters
    assert P.splitk_ok(256, 2) and P.splitk_ok(768, 4) and not P.splitk_ok(256, 3) and not P.splitk_ok(256, 8)
    assert P.part_elems(256, 1, 512, 1024, 2) == 2 * 4 * 128 * 1024 * 2 and P.part_elems(256, 1, 512, 1024, 3) == 0
    assert P.ku_plain(1, 512) == 8 and P.ku_plain(1, 768) == 4 and P.ku_plain(1, 1536) == 8 and P.ku_splitk(8) == 1
    assert P.SYNC_WORDS == 16 * (1 + 32 + 128) and (P.PU, P.PMAXC) == (16, 4)


def test_case_table_reaches_every_variant_at_256_cus():
    fwd, bwd, sk = set(), set(), set()
    branch = {'fwd': set(), 'bwd': set(), 'sk': set()}
    rg_gt1, empty, Hs, NCs, Ts, sk_Ts = set(), set(), set(), set(), set(), set()
    for c in P.ALL_CASES:
        r = P.reached(NCU, c)
        assert r, 'case %s runs nothing at 256 CUs' % P.case_id(c)
        Hs.add(c['H']), NCs.add(c['NC']), Ts.add(c['T'])
        if 'plain' in r:
            p = r['plain']
            fwd.add(r['fwd']), bwd.add(r['bwd'])
            b = P.block_map_branch(c['NC'], p['RG'], c['H'])
            branch['fwd'].add(b), branch['bwd'].add(b)
            if p['RG'] > 1:
                rg_gt1.add('plain')
            if P.empty_groups(p, c['M']):
                empty.add('plain')
        for S in (2, 4):
            q = r.get('S%d' % S)
            if q is not None:
                sk.add((q['FM'], S)), sk_Ts.add(c['T'])
                branch['sk'].add(P.block_map_branch(c['NC'], q['RG'], c['H']))
                if q['RG'] > 1:
                    rg_gt1.add('sk')
                if P.empty_groups(q, c['M']):
                    empty.add('sk')
    assert fwd == set(P.PLAIN_INSTANCES), 'forward (FM, KU) reached: %s' % sorted(fwd)
    assert bwd == set(P.PLAIN_INSTANCES), 'plain BPTT (FM, KU) reached: %s' % sorted(bwd)
    assert sk == set(P.SK_INSTANCES), 'split-K (FM, S) reached: %s' % sorted(sk)
    for k, v in branch.items():
        assert v == {'xcd', 'plain'}, 'block_map branches of %s: %s' % (k, v)
    assert rg_gt1 == {'plain', 'sk'} and empty == {'plain', 'sk'}
    assert Hs == {256, 512, 768, 1024} and NCs == {1, 2, 3, 4}
    assert {1, 2, 5, 32} <= Ts and 6 in sk_Ts


def test_case_table_holds_the_named_shapes():
    """the issue's table, row by row: (M, H, NC, reserve) -> what it must reach at 256 CUs"""
    want = {(1, 256, 1, 0): (1, 4), (40, 256, 1, 0): (1, 4), (64, 256, 1, 0): (1, 4), (48, 512, 2, 0): (1, 8), (1024, 256, 1, 0): (1, 4),
            (100, 256, 1, 0): (2, 4), (96, 768, 1, 0): (2, 4), (72, 1024, 1, 0): (2, 4), (130, 256, 1, 0): (2, 4), (257, 256, 1, 0): (2, 4),
            (520, 256, 1, 0): (2, 4), (40, 256, 3, 0): (1, 4), (70, 256, 3, 0): (2, 4), (300, 256, 3, 0): (2, 4), (33, 256, 4, 0): (1, 4),
            (130, 256, 1, 240): (4, 2), (200, 256, 1, 240): (4, 2), (300, 256, 1, 240): None, (300, 256, 2, 224): None}
    have = {(c['M'], c['H'], c['NC'], c['reserve']): P.reached(NCU, c) for c in P.ALL_CASES}
    for k, inst in want.items():
        assert k in have, k
        assert have[k].get('fwd') == inst and have[k].get('bwd') == (inst if inst is None or k[1] != 512 else (1, 8)), (k, have[k])
    assert have[(1024, 256, 1, 0)]['plain']['RG'] == 16 and P.block_map_branch(1, 16, 256) == 'plain'
    assert have[(130, 256, 1, 0)]['plain'] == dict(RG=2, rows=128, FM=2)
    assert have[(300, 256, 1, 240)]['S2']['FM'] == 8 and have[(300, 256, 2, 224)]['S4']['FM'] == 8
    assert P.empty_groups(have[(300, 256, 3, 0)]['plain'], 300) == 1 and 3 * have[(300, 256, 3, 0)]['plain']['RG'] == 12


def test_mixed_lengths_hold_what_the_issue_asks():
    for c in P.ALL_CASES:
        if not c['lengths'] or c['M'] < c['T'] + 3:
            continue
        p = P.plan(NCU - c['reserve'], c['NC'], c['M'], c['H'], P.FM_MAX_SK)
        for ch in range(c['NC']):
            ln = P.lengths_of(c['M'], c['T'], p['rows'], p['RG'], ch)
            assert 0 in ln and c['T'] in ln and (ln > c['T']).any()
            if p['RG'] > 1:
                assert (ln[p['rows']:2 * p['rows']] == 0).all() and (ln[:p['rows']] > 0).any()
    assert any(c['lengths'] and P.plan(NCU - c['reserve'], c['NC'], c['M'], c['H'], P.FM_MAX_SK)['RG'] > 1 for c in P.ALL_CASES)


def test_identity_pairs_share_their_inputs():
    a, b = P.ALONE_VS_NC3
    x, y = P.chain_inputs(a, 0), P.chain_inputs(b, 0)
    assert all(np.array_equal(x[k], y[k]) for k in ('w', 'b', 'gi', 'gi2', 'h0', 'ext', 'last', 'lengths')) and x['has_dh0'] == y['has_dh0']
    a, b = P.RESERVE_PAIR
    assert P.plan(NCU, 1, a['M'], a['H']) != P.plan(NCU - 240, 1, b['M'], b['H'])
