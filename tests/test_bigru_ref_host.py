"""CPU-only checks of tests/bigru_ref.py, the fp64 oracle of tests/test_gpu_bigru_node.py.

1. The reference itself: forward / backward against torch's float64 nn.GRU(bidirectional=True) over pack_padded_sequence with autograd
   (rows of length 0 stay outside the pack: zeros out, no gradient), ragged lengths with 0, 1 and T, and lengths None; 1e-12 relative.
2. Sharpness: at the exact inputs of GPU cases -- the rows branch's sorted (M 4096, T 3), dense and launch-wide-dead (T 16, no row longer
   than 6) cases and the fp32 step case with lengths -- the bound the GPU test will use (bound_of of tests/test_gpu_dur_kernels.py, from
   the reference and its kernel-precision evaluation alone; dx per time plane) is violated by each of seven wrong variants of the
   reference: a node that computed any of them would fail.  Nothing here looks at a kernel's output.  The inputs are the generators'
   plain ones (x = 0.7 N, dout = 0.3 N, weights U(+-1/sqrt(H))): every variant is caught at them as they are, nothing had to be scaled.
   What the variants stand for where a choice was open: (a) drops rows 64 .. 127, the second panel in natural row order, from direction
   0's weight_ih product; (b) drops, at processing step 1 of direction 0, the last 128 positions of the live prefix in descending-length
   order (seg_n[1] - 128 .. seg_n[1]) from the weight_hh product and its bias sum.  (a) and (b) need panels and blocks: rows cases only.
3. The case list reaches what it claims."""
import functools

import numpy as np
import pytest
import torch

import bigru_ref as BR
import rowgru_ref as RR
import wgrad_ref as WG
from test_gpu_dur_kernels import bound_of

F8 = np.float64


# ================================================================================================ 1. the reference against torch
def torch_bigru(x, lengths, w8, dout):
    T, M, I = x.shape
    H = w8[1].shape[1]
    gru = torch.nn.GRU(I, H, bidirectional=True).double()
    names = [n + s for s in ('', '_reverse') for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]
    with torch.no_grad():
        for n, w in zip(names, w8):
            getattr(gru, n).copy_(torch.from_numpy(np.asarray(w, F8)))
    xt = torch.from_numpy(np.asarray(x, F8)).requires_grad_()
    lens = np.full(M, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    live = np.flatnonzero(lens > 0)
    out = torch.zeros(M, 2 * H, dtype=torch.float64)
    if live.size:
        packed = torch.nn.utils.rnn.pack_padded_sequence(xt[:, live], torch.from_numpy(lens[live]), enforce_sorted=False)
        h_n = gru(packed)[1]                                        # [2, rows, H]
        out = out.index_put((torch.from_numpy(live),), torch.cat([h_n[0], h_n[1]], dim=1))
        (out * torch.from_numpy(np.asarray(dout, F8))).sum().backward()
    dx = xt.grad.numpy() if xt.grad is not None else np.zeros((T, M, I))
    grads = [getattr(gru, n).grad.numpy() if getattr(gru, n).grad is not None else np.zeros(w.shape) for n, w in zip(names, w8)]
    return out.detach().numpy(), dx, grads


def close(a, b):
    a, b = np.asarray(a, F8), np.asarray(b, F8)
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0)


@pytest.mark.parametrize('M,T,H,I,lens', [(9, 5, 6, 4, 'ragged'), (9, 5, 6, 4, None), (3, 1, 4, 5, 'ragged'), (70, 4, 8, 8, 'zero'),
                                          (130, 7, 16, 12, 'ragged')])
def test_reference_equals_torch_float64_packed_bigru_and_autograd(M, T, H, I, lens):
    rng = np.random.RandomState(M * 100 + T)
    k = 1.0 / np.sqrt(H)
    w8 = [rng.uniform(-k, k, size=s) for _ in range(2) for s in ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,))]
    x, dout = rng.standard_normal((T, M, I)), rng.standard_normal((M, 2 * H))
    lengths = None
    if lens == 'zero':
        lengths = np.zeros(M, np.int32)
    elif lens == 'ragged':
        lengths = rng.randint(0, T + 1, size=M).astype(np.int32)
        lengths[:3] = (0, 1, T)
        assert {0, 1, T} <= set(lengths.tolist())
    out, dx, grads = torch_bigru(x, lengths, w8, dout)
    assert close(BR.forward(x, lengths, w8), out)
    rdx, rg = BR.backward(x, lengths, w8, dout)
    assert close(rdx, dx)
    for a, b in zip(rg, grads):
        assert close(a, b)
    if lengths is not None:
        ln = np.asarray(lengths)
        assert not BR.forward(x, lengths, w8)[ln == 0].any()                       # a row of length 0: zeros in both halves
        assert not rdx[np.arange(T)[:, None] >= ln[None, :]].any()                 # dx exactly zero at t >= len


# ================================================================================================ 2. sharpness of the bound
SHARP_CASES = (BR.ROWS_CASES[0], BR.ROWS_CASES[1], BR.ROWS_CASES[4], BR.STEP_FP32_CASES[0])
VARIANTS = ('a', 'b', 'c', 'd', 'e', 'f', 'g')


def results(out, dx, grads):
    r = {'out': out}
    r.update({'dx[%d]' % t: p for t, p in enumerate(dx)})
    r.update(dict(zip(BR.NAMES, grads)))
    return r


def violated(c, wrong):
    """the outputs of `wrong` that are over the GPU test's bound: the reference and its kernel-precision evaluation decide, nothing else"""
    ref = BR.reference(c)
    good, kp = results(ref['out'], ref['dx'], ref['grads']), results(ref['kp_out'], ref['kp_dx'], ref['kp_grads'])
    bad = []
    for k in good:
        bound, _ = bound_of(good[k], kp[k])
        if (np.abs(np.asarray(wrong[k], F8) - good[k]) > bound).any():
            bad.append(k)
    return bad


@functools.lru_cache(maxsize=1)
def right_chain(cid):
    """the fp64 chain of a sharpness case and each direction's gradients, computed once for its seven variants"""
    c = next(k for k in SHARP_CASES if BR.case_id(k) == cid)
    ins = BR.inputs(c)
    tr = BR.trace(ins['x'], ins['lengths'], ins['w8'], ins['dout'])
    return tr, BR.grads_of(ins['x'], tr, 0), BR.grads_of(ins['x'], tr, 1)


def wrong_variant(c, v):
    ins = BR.inputs(c)
    x, lengths, w8, dout = np.asarray(ins['x'], F8), ins['lengths'], ins['w8'], ins['dout']
    T, M, I = x.shape
    x2 = x.reshape(T * M, I)
    if v == 'f':                                                                   # every length clipped to len - 1
        short = np.maximum((np.full(M, T) if lengths is None else np.asarray(lengths)) - 1, 0)
        return results(BR.forward(x, short, w8), *BR.backward(x, short, w8, dout))
    tr, (g0, dx0), (g1, dx1) = right_chain(BR.case_id(c))
    g0, g1 = list(g0), list(g1)
    out, dx = BR.out_of(tr), dx0 + dx1
    H3 = tr[0]['dgi'].shape[2]
    H = H3 // 3
    row, step = np.tile(np.arange(M), T), np.repeat(np.arange(T), M)
    if v == 'a':                                                                   # weight_ih gradient without one 64-row panel
        live = ~((row >= BR.PANEL) & (row < 2 * BR.PANEL))
        g0[0] = WG.product(tr[0]['dgi'].reshape(T * M, H3), x2, live)
    elif v == 'b':                                                                 # seg short by one 128-row block at one step
        lens = np.full(M, T) if lengths is None else np.asarray(lengths)
        pos_of = np.empty(M, np.int64)
        pos_of[RR.by_length(lens)] = np.arange(M)
        seg1 = BR.BLOCK * -(-int((lens > 1).sum()) // BR.BLOCK)                  # (step 1: before step 0 the state is zero)
        live = ~((step == 1) & (pos_of[row] >= seg1 - BR.BLOCK))
        dgh2 = tr[0]['dgh'].reshape(T * M, H3)
        g0[1], g0[3] = WG.product(dgh2, tr[0]['states'][:T].reshape(T * M, H), live), WG.colsum(dgh2, live)
    elif v == 'c':                                                                 # weight_hh gradient on h_t in place of h_{t-1}
        for g, t in ((g0, tr[0]), (g1, tr[1])):
            g[1] = WG.product(t['dgh'].reshape(T * M, H3), t['states'][1:].reshape(T * M, H))
    elif v == 'd':                                                                 # the two halves of out swapped
        out = np.concatenate([out[:, H:], out[:, :H]], axis=1)
    elif v == 'e':                                                                 # direction 1's dgi by processing step, not by time
        t1 = dict(tr[1], dgi=tr[1]['dgi'][::-1])
        g1, dx1 = BR.grads_of(x, [tr[0], t1], 1)
        dx = dx0 + dx1
    elif v == 'g':                                                                 # dx of direction 1 dropped
        dx = dx0
    return results(out, dx, g0 + g1)


@pytest.mark.parametrize('c', SHARP_CASES, ids=BR.case_id)
def test_the_gpu_bound_rejects_every_wrong_variant_of_the_reference(c):
    ref = BR.reference(c)
    assert violated(c, results(ref['out'], ref['dx'], ref['grads'])) == []       # (the reference itself is inside its own bound)
    for v in VARIANTS:
        if v in 'ab' and c['branch'] != 'rows':
            continue
        bad = violated(c, wrong_variant(c, v))
        print('variant (%s) at %s: over the bound in %s' % (v, BR.case_id(c), bad))
        assert bad, 'wrong variant (%s) passes the bound at %s' % (v, BR.case_id(c))


# ================================================================================================ 3. what the case list reaches
def test_rows_cases_reach_what_they_claim():
    rows = [(c, BR.inputs(c)['lengths']) for c in BR.ROWS_CASES]
    given = [(c, ln) for c, ln in rows if ln is not None]
    assert all(c['H'] == 128 and c['I'] == 128 and c['M'] >= 4096 and c['bf16'] for c, _ in rows)          # row_gru_ok's floor
    assert any((ln == 0).any() and (ln > 0).any() for _, ln in given)                                       # a row of length 0
    assert any((ln == c['T']).any() for c, ln in given) and any(ln is None for _, ln in rows)               # a full-length row; dense
    # a 64-row panel whose rows are all shorter than T -- in row order and in the descending-length order of the sorted panels
    # (in row order only the T = 16 case, whose longest row is 6, has one; sorted, the T = 3 cases have their tail panels too)
    for order in (lambda ln: ln, lambda ln: ln[RR.by_length(ln)]):
        assert any(any(order(ln)[a:b].max() < c['T'] and order(ln)[a:b].max() > 0 for a, b in RR.panels(c['M'])) for c, ln in given)
    assert any(0 < ln.max() < c['T'] and c['M'] % 32 == 0 for c, ln in given)                               # launch-wide dead steps, with `top`
    assert any(c['M'] % 32 != 0 for c, _ in given)                                                          # no top, no seg
    # (implied by row_gru_ok's floor: 4096 rows are 64 panels -- every rows case crosses panel 32; kept because the issue lists it)
    assert any(len(RR.panels(c['M'])) > 32 for c, _ in rows)                                                # krot changes at panel 32
    assert any(c['M'] % 128 == 0 and c['M'] // 128 == 33 for c, _ in given)                                 # 33 blocks, 66 panels
    assert any(ln.max() == 0 for _, ln in given)                                                            # the all-zero results
    # sorted with seg: a step whose live prefix ends inside the rows (a dead 128-row block to clip)
    c, ln = rows[0]
    assert c['M'] % 128 == 0 and any(128 * -(-int((ln > s).sum()) // 128) < c['M'] for s in range(c['T']))


def test_step_and_persist_case_lists():
    assert [(c['M'], c['H'], c['I'], c['T']) for c in BR.STEP_FP32_CASES] == [(8, 16, 16, 3), (8, 16, 16, 3), (5, 16, 12, 1)]
    assert not any(c['bf16'] for c in BR.STEP_FP32_CASES) and {c['lens'] for c in BR.STEP_FP32_CASES[:2]} == {'random', None}
    pc = BR.persist_cases(24, 8)
    assert {(c['lens'], c['I'], c['x_bf16']) for c in pc} == {(l, i, b) for l in ('random', None) for i in (64, 36) for b in (False, True)}
    for c in pc:                                                                  # bf16-exact operands where the branch rounds them anyway
        ins = BR.inputs(c)
        assert c['T'] == 3 and all(BR.GM.is_bf16(w) for w in ins['w8']) and BR.GM.is_bf16(ins['x']) == c['x_bf16']
        assert (ins['lengths'] is None) == (c['lens'] is None)
