"""tests/rowgru_ref.py -- the oracle of tests/test_gpu_rowgru_kernels.py -- held to torch's float64 operators without a GPU: the H = 128
reference (fused input product, packed-sequence mask, both directions, final state, BPTT from the final state) against nn.GRU with
pack_padded_sequence and autograd; the H = 512 reference (hoisted input part, a gradient arriving at every state) against a float64
nn.GRU whose input carries the hoisted operand; the layout helpers against the element formulas of the header and the index
expressions of the sources; perm = identity against no perm; and the row lists of the GPU cases against the properties those tests rely
on -- every prediction class (LIVE / ZERO / UNWRITTEN / EITHER) is exercised."""
import os

import numpy as np
import pytest
import torch

import rowgru_ref as RR
import test_gpu_rowgru_kernels as G
from rowgru_ref import EITHER, LIVE, UNWRITTEN, ZERO

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'polyphonic_chord_texture_disentanglement_amd', 'csrc')
TOL = 1e-11


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max()), (what, np.abs(a - b).max())


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def test_h128_reference_is_the_packed_bidirectional_gru_of_torch():
    H, E, R, T = 128, RR.E, 11, 5
    rng = np.random.RandomState(3)
    k = 1.0 / np.sqrt(H)
    U = lambda *s: rng.uniform(-k, k, s)
    w = {d: dict(w_x=U(3 * H, E), w_hh=U(3 * H, H), b_ih=U(3 * H), b_hh=U(3 * H)) for d in (0, 1)}
    x = rng.randn(T, R, E) * 0.7
    lengths = RR.lengths_of(R, T, 'mixed')
    assert lengths.min() == 0 and lengths.max() == T
    dout = rng.randn(R, 2 * H) * 0.3
    gru = torch.nn.GRU(E, H, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in ((0, ''), (1, '_reverse')):
            for name, key in (('weight_ih_l0', 'w_x'), ('weight_hh_l0', 'w_hh'), ('bias_ih_l0', 'b_ih'), ('bias_hh_l0', 'b_hh')):
                getattr(gru, name + sfx).copy_(t64(w[d][key]))
    live = np.flatnonzero(lengths > 0)                                   # (pack_padded_sequence takes no empty sequence: their final state is h0 = 0)
    xt = t64(x[:, live]).requires_grad_()
    packed = torch.nn.utils.rnn.pack_padded_sequence(xt, torch.from_numpy(lengths[live]).long(), enforce_sorted=False)
    _, hn = gru(packed)
    (hn * t64(np.stack([dout[live, :H], dout[live, H:]]))).sum().backward()
    dx = np.zeros_like(x)
    for d, sfx in ((0, ''), (1, '_reverse')):
        p = w[d]
        h0 = np.zeros((R, H))
        st, gates = RR.forward(H, x, p['w_x'], p['w_hh'], p['b_hh'], h0, b_ih=p['b_ih'], lengths=lengths, reverse=bool(d))
        close(st[T][live], hn[d].detach().numpy(), 'final state')
        assert (st[:, lengths == 0] == 0).all(), 'a row of length 0 never leaves h0'
        dh_last = dout[:, d * H:(d + 1) * H]
        dgi, dgh, dh0 = RR.backward(H, st[:T], gates, p['w_hh'], None, dh_last, bool(d))
        dx += dgi @ p['w_x']
        close(np.einsum('trg,tre->ge', dgi, x), getattr(gru, 'weight_ih_l0' + sfx).grad.numpy(), 'grad W_ih: dgi is indexed by TIME')
        close(np.einsum('srg,srh->gh', dgh, st[:T]), getattr(gru, 'weight_hh_l0' + sfx).grad.numpy(), 'grad W_hh: dgh pairs with the states by STEP')
        close(dgi.sum((0, 1)), getattr(gru, 'bias_ih_l0' + sfx).grad.numpy(), 'grad b_ih')
        assert np.array_equal(dh0[lengths == 0], dh_last[lengths == 0]), 'dh0 of an empty row is its dh_last'
    close(dx[:, live], xt.grad.numpy(), 'dx')
    assert (dx[:, lengths == 0] == 0).all()


def test_h512_reference_is_a_gru_with_a_hoisted_input_term_and_a_gradient_at_every_state():
    H, E, R, T, Kc = 512, RR.E, 5, 3, 8
    rng = np.random.RandomState(4)
    k = 1.0 / np.sqrt(H)
    U = lambda *s: rng.uniform(-k, k, s)
    w_c, w_tok, w_hh, b_ih, b_hh = U(3 * H, Kc), U(3 * H, E), U(3 * H, H), U(3 * H), U(3 * H)
    ns, emb, h0, ext = rng.randn(R, Kc), rng.randn(T, R, E) * 0.5, rng.randn(R, H) * 0.5, rng.randn(T, R, H) * 0.1
    gc = ns @ w_c.T + b_ih                                                # the hoisted part, b_ih folded in
    gru = torch.nn.GRU(Kc + E, H).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(t64(np.concatenate([w_c, w_tok], 1))); gru.weight_hh_l0.copy_(t64(w_hh))
        gru.bias_ih_l0.copy_(t64(b_ih)); gru.bias_hh_l0.copy_(t64(b_hh))
    nst, embt, h0t = t64(ns).requires_grad_(), t64(emb).requires_grad_(), t64(h0).requires_grad_()
    out, _ = gru(torch.cat([nst[None].expand(T, R, Kc), embt], 2), h0t[None])
    (out * t64(ext)).sum().backward()
    st, gates = RR.forward(H, emb, w_tok, w_hh, b_hh, h0, gc=gc)
    close(st[1:], out.detach().numpy(), 'states')
    assert np.array_equal(st[0], h0)
    dgi, dgh_n, dh0 = RR.backward(H, st[:T], gates, w_hh, ext)
    close(dh0, h0t.grad.numpy(), 'dh0')
    close(dgi @ w_tok, embt.grad.numpy(), 'd emb')
    close(dgi.sum(0) @ w_c, nst.grad.numpy(), 'd ns through gc')
    # "the r and z thirds of dgh are dgi's": grad W_hh[0:2H] = dgi[:, 0:2H]^T . h and grad W_hh[2H:] = dgh^T . h
    gw = np.concatenate([np.einsum('srg,srh->gh', dgi[:, :, :2 * H], st[:T]), np.einsum('srg,srh->gh', dgh_n, st[:T])])
    close(gw, gru.weight_hh_l0.grad.numpy(), 'grad W_hh')
    assert dgh_n.shape == (T, R, H)


def test_kernel_precision_evaluation_is_close_to_the_reference_and_rounds_where_the_kernels_round():
    H, R, T = 128, 9, 3
    rng = np.random.RandomState(5)
    k = 1.0 / np.sqrt(H)
    w_x, w_hh = RR.bf16_round(rng.uniform(-k, k, (3 * H, RR.E))), RR.bf16_round(rng.uniform(-k, k, (3 * H, H)))
    b = rng.uniform(-k, k, 3 * H).astype(np.float32)
    x, h0 = (rng.randn(T, R, RR.E) * 0.7).astype(np.float32), (rng.randn(R, H) * 0.5).astype(np.float32)
    st, gates = RR.forward(H, x, w_x, w_hh, b, h0, b_ih=b)
    kst, kg, k16 = RR.kp_forward(H, x, w_x, w_hh, b, h0, b_ih=b)
    assert kst.dtype == np.float32 and RR.G.is_bf16(kg) and RR.G.is_bf16(k16) and np.array_equal(k16, RR.bf16_round(kst))
    assert 0 < np.abs(kst - st).max() < 2e-2 and np.abs(kg - gates).max() < 2e-2
    dgi, dgh, dh0 = RR.backward(H, st[:T], gates, w_hh, None, x[0, :, :H])
    kdgi, kdgh, kdh0 = RR.kp_backward(H, kst[:T], kg, w_hh, None, x[0, :, :H])
    assert RR.G.is_bf16(kdgi) and RR.G.is_bf16(kdgh) and kdh0.dtype == np.float32
    assert np.abs(kdgi - dgi).max() < 2e-2 * np.abs(dgi).max() + 1e-3 and np.abs(kdh0 - dh0).max() < 2e-2 * np.abs(dh0).max() + 1e-3


def test_layout_helpers_round_trip_and_match_the_header_and_the_sources():
    rng = np.random.RandomState(6)
    R, T = 7, 3
    for H in (128, 512):
        w = RR.gate_block(H)
        g = rng.randn(T, 4, R, H)
        blk = RR.gates_blocked(g, H)
        assert blk.shape == (T, 4, H // w, R, w) and np.array_equal(RR.gates_unblocked(blk, H), g)
        flat = blk.reshape(T, 4, -1)
        for t, q, row, u in ((0, 0, 0, 0), (2, 3, 6, H - 1), (1, 2, 3, w), (1, 1, 5, w + 1), (2, 0, 4, 3 * w - 1)):
            assert flat[t, q, ((u // w) * R + row) * w + u % w] == g[t, q, row, u]       # plane[u / w][row][u % w] of the header
    gc = rng.randn(R, 3 * 512)
    b = RR.gc_blocked(gc)
    assert b.shape == (96, R, 16) and np.array_equal(RR.from_blocked(b, 16), gc) and b.reshape(-1)[((40 // 16) * R + 5) * 16 + 40 % 16] == gc[5, 40]
    ext = rng.randn(T, R, 512)
    b = RR.ext_blocked(ext)
    assert b.shape == (16, T * R, 32) and np.array_equal(RR.ext_unblocked(b, T), ext)
    assert b.reshape(-1)[((100 // 32) * (T * R) + 2 * R + 4) * 32 + 100 % 32] == ext[2, 4, 100]   # [H/32][T*R][32], row s * R + m
    dgh = rng.randn(T, R, 3 * 512)
    assert np.array_equal(RR.dgh_stored(dgh, 512), dgh[:, :, 1024:]) and RR.dgh_stored(dgh[:, :, :384], 128).shape == (T, R, 384)
    # the index expressions the helpers stand for, as the sources write them
    persist, roles = open(os.path.join(CSRC, 'notes_persist.hip')).read(), open(os.path.join(CSRC, 'notes_roles.hip')).read()
    for text, src in (('gate_off(long row, int u, long R) { return ((long)(u >> 5) * R + row) * 32 + (u & 31); }', persist),
                      ('ext_off(int s, long row, int u, long R, int T) { return ((long)(u >> 5) * ((long)T * R) + (long)s * R + row) * 32 + (u & 31); }', persist),
                      ('(EMB ? gate_off(grow[i], u, R) : ((long)(u >> 4) * R + grow[i]) * 16 + (u & 15))', persist),
                      ('stnt_bf16x8(a.dgh + (long)s * RH + grow[i] * H + u, dnr);', persist),
                      ('g_off[i] = (unsigned)(grow[i] * 32 + (q & 1) * 16 + (long)(q >> 1) * R * 32);', roles),
                      ('const unsigned vo16[2] = {(unsigned)(grow[0] * 32 + hh * 16), (unsigned)(grow[1] * 32 + hh * 16)};', roles),
                      ('e_off[i] = (unsigned)(grow[i] * 64 + q * 16);', roles)):
        assert text in src, 'the sources no longer hold %r: rowgru_ref\'s layouts must be read against them again' % text


def test_perm_identity_is_no_perm_and_positions_invert():
    rng = np.random.RandomState(7)
    R, T = 70, 4
    ident = np.arange(R, dtype=np.int32)
    lengths = RR.lengths_of(R, T, 'mixed')
    for rev in (False, True):
        a, b = RR.expect_fwd128(R, T, lengths, None, rev), RR.expect_fwd128(R, T, lengths, ident, rev)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        a, b = RR.expect_bwd128(R, T, lengths, None, rev, True, -1), RR.expect_bwd128(R, T, lengths, ident, rev, True, -1)
        assert all(np.array_equal(a[k], b[k]) for k in a)
    perm = RR.by_length(lengths)
    assert sorted(perm) == list(range(R)) and (np.diff(lengths[perm]) <= 0).all()
    assert np.array_equal(perm, torch.sort(torch.from_numpy(lengths).long(), descending=True, stable=True)[1].numpy())
    x = rng.randn(3, R, 2)
    assert np.array_equal(RR.to_pos(x, ident, 1), x) and np.array_equal(RR.to_nat(RR.to_pos(x, perm, 1), perm, 1), x)
    assert np.array_equal(RR.to_pos(x, perm, 1)[:, 5], x[:, perm[5]])


def test_top_step_and_limits_of_the_expectations():
    T, R = 5, 130
    ext = np.ones((T, R, 4), np.float32)
    ext[3:] = -0.0                                                       # -0.0 counts as zero
    ext[2, 64:] = 0
    e = RR.expect_bwd512(R, T, ext, True, None, None, False, True, -1)
    assert e['top'] == 2 and list(e['last'][[0, 64, 129]]) == [2, 1, 1] and (e['dgi'][3:] == ZERO).all() and (e['dgi'][2, :64] == LIVE).all()
    assert RR.expect_bwd512(R, T, ext, True, None, None, False, True, T + 5)['top'] == T + 5       # atomicMax into the caller's value
    e = RR.expect_bwd512(R, T, ext, True, 1, None, False, True, -1)
    assert e['top'] == 1 and (e['dgi'][2:] == UNWRITTEN).all()
    e = RR.expect_bwd512(R, T, ext, False, 1, None, False, True, -1)     # zero-skip off: bound is ignored
    assert e['top'] == T - 1 and (e['dgi'] == LIVE).all()
    e = RR.expect_fwd512(R, T, -1)                                       # live_top < 0 still runs step 0
    assert (e['HN16'][:2] == LIVE).all() and (e['HN16'][2:] == UNWRITTEN).all() and (e['gates'][0] == LIVE).all() and (e['gates'][1:] != LIVE).all()
    lengths = np.array([0, 3, 9, 2] * 16, np.int32)                      # H = 128: the largest min(length, T) - 1
    assert RR.expect_bwd128(64, T, lengths, None, False, True, -1)['top'] == T - 1
    assert RR.expect_bwd128(64, T, np.minimum(lengths, 3), None, False, True, -1)['top'] == 2
    assert RR.expect_bwd128(64, T, lengths * 0, None, False, True, -1)['top'] == -1
    # the launch-wide limit needs R % 32 == 0
    short = RR.lengths_of(64, T, 'short')
    assert (RR.expect_fwd128(64, T, short)['HN'][T] == UNWRITTEN).all() and (RR.expect_fwd128(63, T, short[:63])['HN'][T] == LIVE).all()


def test_the_gpu_cases_exercise_every_prediction_class():
    seen = {k: set() for k in ('fwd128', 'bwd128', 'fwd512', 'bwd512')}
    props = set()
    for i, key in enumerate(G.CASES128):
        c = dict(key)
        R, T = c['R'], c['T']
        lengths = RR.lengths_of(R, T, c['lens']) if c.get('lens') else None
        perm = G.perm_of(c, lengths)
        rev = bool(c.get('reverse'))
        f = RR.expect_fwd128(R, T, lengths, perm, rev)
        b = RR.expect_bwd128(R, T, lengths, perm, rev, i % 2 == 0, -1)
        seen['fwd128'] |= set(np.unique(f['HN'][1:])) | set(np.unique(f['gates']))
        seen['bwd128'] |= set(np.unique(b['dgi'])) | set(np.unique(b['dgh']))
        if lengths is None:
            continue
        lens = RR.to_pos(lengths, perm, 0)
        if (lengths == 0).any() and (lengths == T).any():
            props.add('a row of length 0 and one of length T')
        if any(lens[a:e].max() < T and (f['HN'][T, a:e] == LIVE).all() for a, e in RR.panels(R)):
            props.add('a panel whose late steps are all dead')
        if rev and R % 32 == 0 and T > 1 and (f['HN'][1] == UNWRITTEN).all() and (f['HN'][2:] == LIVE).any():
            props.add('a dead prefix of the reversed direction')
        if any(lens[a:e].max() == 0 for a, e in RR.panels(R)) and perm is None:
            props.add('a panel of empty rows with dh0 wanted')
    for key in G.FWD512:
        c = dict(key)
        rl = RR.row_len_of(c['R'], c['T']) if c.get('rl') else None
        f = RR.expect_fwd512(c['R'], c['T'], c.get('live_top'), rl, bool(c.get('nofill')))
        seen['fwd512'] |= set(np.unique(f['HN16'])) | set(np.unique(f['gates']))
        if rl is not None and c['R'] > RR.BLOCK and rl[RR.BLOCK] == 0 and rl[0] > 0:
            props.add('a 128-row block that is dead under row_len')
    kinds = set()
    for key in G.FWD512:
        c = dict(key)
        if c.get('entry') == 'top':
            kinds |= {n for n, v in (('-1', -1), ('0', 0), ('T-2', c['T'] - 2), ('T-1', c['T'] - 1), ('T+3', c['T'] + 3)) if c['live_top'] == v}
    assert kinds == {'-1', '0', 'T-2', 'T-1', 'T+3'}, kinds
    for key in G.BWD512:
        c = dict(key)
        d = dict(ext=np.ones((c['T'], c['R'], 4), np.float32))
        b = RR.expect_bwd512(c['R'], c['T'], G.ext_of(c, d), True, c.get('bound'), RR.row_len_of(c['R'], c['T']) if c.get('rl') else None,
                             bool(c.get('nofill')), 'top' in c, c.get('top', -1))
        seen['bwd512'] |= set(np.unique(b['dgi']))
    assert seen['fwd128'] == {LIVE, UNWRITTEN} and seen['bwd128'] == {LIVE, ZERO, UNWRITTEN}
    assert seen['fwd512'] == {LIVE, ZERO, UNWRITTEN, EITHER} and seen['bwd512'] == {LIVE, ZERO, UNWRITTEN, EITHER}
    assert props == {'a row of length 0 and one of length T', 'a panel whose late steps are all dead', 'a dead prefix of the reversed direction',
                     'a panel of empty rows with dh0 wanted', 'a 128-row block that is dead under row_len'}, props
    # shapes the issue names, per kernel family
    for cases in (G.CASES128, G.FWD512, G.BWD512):
        assert {1, 63, 64, 65, 96, 130, 200, 2176, 2182} <= {dict(k)['R'] for k in cases}
        assert {1, 2, 5} <= {dict(k)['T'] for k in cases}
    assert 16 in {dict(k)['T'] for k in G.CASES128} and 15 in {dict(k)['T'] for k in G.FWD512} and 15 in {dict(k)['T'] for k in G.BWD512}


@pytest.mark.parametrize('R', [1, 63, 64, 65, 130, 200])
def test_row_lists_are_what_their_docstrings_say(R):
    for T in (1, 2, 5, 16):
        m, s = RR.lengths_of(R, T, 'mixed'), RR.lengths_of(R, T, 'short')
        assert m.min() >= 0 and m.max() <= T and m[0] == T and (R <= T or (m == 0).any()) and (m[64:] <= T // 2).all()
        assert s.min() == 0 and s.max() <= max(T - 2, 0)
        rl = RR.row_len_of(R, T)
        assert rl[0] == T and (np.diff(rl) <= 0).all() and (rl[RR.BLOCK:] == 0).all()
