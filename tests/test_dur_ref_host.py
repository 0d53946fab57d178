"""Guards tests/dur_ref.py, the fp64 references of the duration-decoder kernel tests, against the same network built in torch
float64 -- a GRU cell with explicit W_ih, W_hh and biases, the <sos> token, one-hot feedback, the 2-wide output layer -- and torch's
autograd of sum(est_dur * ddur) with the tokens forced.  No GPU.  Agreement is to 1e-10 relative: fp64 against fp64, round-off times a
sum of at most 5 x 130 terms."""
import numpy as np
import pytest
import torch

import dur_ref as R

RTOL = 1e-10
H = 64
MS = [1, 17, 130]


def close(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    s = np.abs(want).max() if scale is None else scale
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max() <= RTOL * max(s, 1e-300), (np.abs(got - want).max(), s)


def params(seed, I=5):
    rng = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(H)
    u = lambda *s: rng.uniform(-k, k, s)
    return dict(w_ih=u(3 * H, I), w_hh=u(3 * H, H), b_ih=u(3 * H), b_hh=u(3 * H), w_out=u(2, H), b_out=u(2), sos=rng.uniform(0, 1, I))


def torch_net(p, h0, force, ddur):
    """the network in torch float64 -> (outputs, autograd gradients of sum(est_dur * ddur))"""
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    h = torch.tensor(h0, dtype=torch.float64, requires_grad=True)
    I, M = p['sos'].size, h0.shape[0]
    h_in = h
    hs, gates, ests = [], [], []
    tok = t['sos'].expand(M, I)
    for d in range(5):
        gi = tok @ t['w_ih'].T + t['b_ih']
        gh = h @ t['w_hh'].T + t['b_hh']
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs.append(h), gates.append(torch.stack([r, z, n, gh[:, 2 * H:]])), ests.append(h @ t['w_out'].T + t['b_out'])
        tok = torch.nn.functional.one_hot(torch.tensor(force[d]), I).to(torch.float64)
    est = torch.cat(ests, 1)
    (est * torch.tensor(ddur)).sum().backward()
    out = dict(h=torch.stack(hs).detach().numpy(), gates=torch.stack(gates).detach().numpy(), est_dur=est.detach().numpy())
    grads = {k: v.grad.numpy() for k, v in t.items()}
    grads['h0'] = h_in.grad.numpy()
    return out, grads


def case(M, I=5, seed=0):
    p = params(100 * I + M + seed, I)
    rng = np.random.RandomState(M + 7 * I)
    h0 = rng.normal(0, 0.5, (M, H))
    force = rng.randint(0, 2, (5, M))
    ddur = rng.normal(0, 0.1, (M, 10))
    tab0, tab = R.gate_tables(p['w_ih'], p['b_ih'], p['sos'])
    return p, h0, force, ddur, tab0, tab


@pytest.mark.parametrize('M', MS)
def test_forward_vs_torch(M):
    p, h0, force, ddur, tab0, tab = case(M)
    want, _ = torch_net(p, h0, force, ddur)
    got = R.dur_forward(h0, p['w_hh'], p['b_hh'], tab0, tab, p['w_out'], p['b_out'], force)
    for k in ('h', 'gates', 'est_dur'):
        close(got[k], want[k])
    assert np.array_equal(got['idx'], force)


@pytest.mark.parametrize('M', MS)
def test_backward_and_recompute_vs_autograd(M):
    p, h0, force, ddur, tab0, tab = case(M)
    _, g = torch_net(p, h0, force, ddur)
    f = R.dur_forward(h0, p['w_hh'], p['b_hh'], tab0, tab, p['w_out'], p['b_out'], force)
    hprev = np.concatenate([h0[None], f['h'][:4]])
    dh0, S = R.dur_backward(f['gates'], hprev, ddur, force, p['w_hh'], p['w_out'])
    dh0_rc, S_rc = R.dur_backward_recompute(hprev, ddur, force, p['w_hh'], p['b_hh'], tab0, tab, p['w_out'])
    assert S.shape == (256, 80) and not S[:, 67:].any()
    for a, b in ((dh0, S), (dh0_rc, S_rc)):
        close(a, g['h0'])
        inc = R.dur_finalize(b, p['w_ih'], p['sos'])
        for got, name in zip(inc, ('w_hh', 'b_hh', 'b_ih', 'w_ih', 'sos')):
            close(got, g[name])
    # the class columns count every step of every row once: summed over the classes they are the bias gradients of both halves
    close(S[:128, 64:67].sum(1), g['b_ih'][:128])
    close(S[128:192, 64:67].sum(1), g['b_hh'][128:])
    close(S[192:, 64:67].sum(1), g['b_ih'][128:])


@pytest.mark.parametrize('I', [2, 5, 8])
def test_finalize_mapping_at_the_entry_points_input_widths(I):
    """dn r (rows 128..191) feeds the hidden half only, dn (rows 192..255) the input half only: the two differ, and so must the results"""
    p, h0, force, ddur, tab0, tab = case(17, I)
    _, g = torch_net(p, h0, force, ddur)
    hprev = np.concatenate([h0[None], R.dur_forward(h0, p['w_hh'], p['b_hh'], tab0, tab, p['w_out'], p['b_out'], force)['h'][:4]])
    _, S = R.dur_backward_recompute(hprev, ddur, force, p['w_hh'], p['b_hh'], tab0, tab, p['w_out'])
    inc = R.dur_finalize(S, p['w_ih'], p['sos'])
    assert inc[3].shape == (192, I) and inc[4].shape == (I,)
    for got, name in zip(inc, ('w_hh', 'b_hh', 'b_ih', 'w_ih', 'sos')):
        close(got, g[name])
    assert np.abs(g['b_ih'][128:] - g['b_hh'][128:]).max() > 1e-3 * np.abs(g['b_ih']).max()
    close(inc[1][:128], inc[2][:128])


def test_argmax_first_maximum_wins_a_tie():
    est = np.array([[0.5, 0.5], [0.25, 0.5], [0.5, 0.25], [-0.0, 0.0], [1.0, np.nextafter(1.0, 2.0)]])
    assert R.argmax2(est).tolist() == [0, 1, 0, 0, 1]
    assert R.argmax2(est).tolist() == torch.tensor(est).max(-1)[1].tolist()
    # through dur_forward: a zero output layer with equal biases ties every decision
    p, h0, force, ddur, tab0, tab = case(17)
    f = R.dur_forward(h0, p['w_hh'], p['b_hh'], tab0, tab, np.zeros((2, H)), np.array([0.3, 0.3]))
    assert not f['idx'].any() and (f['est_dur'] == 0.3).all()
    est, idx = R.dur_out_token(h0, np.zeros((2, H)), np.array([0.3, 0.3]))
    assert not idx.any()


def test_free_running_tokens_feed_the_next_step():
    p, h0, _, ddur, tab0, tab = case(130)
    f = R.dur_forward(h0, p['w_hh'], p['b_hh'], tab0, tab, p['w_out'] * 8, p['b_out'])
    assert {0, 1} <= set(f['idx'].reshape(-1).tolist())
    assert np.array_equal(f['idx'], R.argmax2(f['est_dur'].reshape(-1, 5, 2)).T)
    want, _ = torch_net(p | dict(w_out=p['w_out'] * 8), h0, f['idx'], ddur)          # replaying its own decisions reproduces it
    close(f['est_dur'], want['est_dur'])


def test_out_token_and_out_wgrad_vs_autograd():
    rng = np.random.RandomState(3)
    for Hh in (64, 20):
        h, w, b = rng.normal(0, 1, (33, Hh)), rng.normal(0, 1, (2, Hh)), rng.normal(0, 1, 2)
        est, idx = R.dur_out_token(h, w, b)
        close(est, h @ w.T + b)
        assert np.array_equal(idx, np.argmax(est, 1))
    hpl, ddur = rng.normal(0, 1, (5, 33, H)), rng.normal(0, 1, (33, 10))
    ddur[rng.rand(33, 5).repeat(2, 1) < 0.5] = 0
    w = torch.zeros(2, H, dtype=torch.float64, requires_grad=True)
    (torch.cat([torch.tensor(hpl[d]) @ w.T for d in range(5)], 1) * torch.tensor(ddur)).sum().backward()
    close(R.dur_out_wgrad(ddur, hpl), w.grad.numpy())
    poisoned = hpl.copy()
    for d in range(5):
        poisoned[d][(ddur[:, 2 * d:2 * d + 2] == 0).all(1)] = np.nan
    assert np.array_equal(R.dur_out_wgrad(ddur, poisoned), R.dur_out_wgrad(ddur, hpl))


def test_kernel_precision_evaluation_is_the_same_formula():
    """the float32 / bf16 evaluation follows the fp64 reference to bf16 accuracy (it is a yardstick for kernel tests, not a reference)"""
    p, h0, force, ddur, tab0, tab = case(130)
    w16 = R.bf16_round(p['w_hh'])
    assert R.is_bf16(w16) and not R.is_bf16(p['w_hh'].astype(np.float32))
    assert R.bf16_round(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], np.float32)).tolist() == [1.0, 1 + 2.0 ** -6]      # ties to even
    f = R.dur_forward(h0, w16, p['b_hh'], tab0, tab, p['w_out'], p['b_out'], force)
    k = R.kp_forward(h0, w16, p['b_hh'], tab0, tab, p['w_out'], p['b_out'], force)
    for name in ('h', 'gates', 'est_dur'):
        assert np.abs(k[name] - f[name]).max() < 2e-2 * max(1.0, np.abs(f[name]).max())
    hprev = np.concatenate([h0[None], f['h'][:4]])
    dh0, S = R.dur_backward(f['gates'], hprev, ddur, force, w16, p['w_out'])
    for gates in (f['gates'], None):
        kd, kS = R.kp_backward(gates, hprev, ddur, force, w16, p['w_out'], p['b_hh'], tab0, tab)
        assert np.abs(kd - dh0).max() < 2e-2 * np.abs(dh0).max() and np.abs(kS - S).max() < 2e-2 * np.abs(S).max()
    zero = [np.zeros(s, np.float32) for s in ((192, 64), (192,), (192,), (192, 5), (5,))]
    for a, b in zip(R.kp_finalize(S, p['w_ih'], p['sos'], zero), R.dur_finalize(S, p['w_ih'], p['sos'])):
        assert np.abs(a - b).max() <= 1e-5 * max(np.abs(b).max(), 1e-30)
    # the output layer and its weight gradient: exact inputs, so only fp32 round-off separates the two (1e-5 of the sums' scale)
    rng = np.random.RandomState(9)
    for Hh in (64, 20):
        h, w, b = (rng.normal(0, 1, s).astype(np.float32) for s in ((33, Hh), (2, Hh), (2,)))
        est, _ = R.dur_out_token(h, w, b)
        assert np.abs(R.kp_out_token(h, w, b) - est).max() <= 1e-5 * (np.abs(h) @ np.abs(w).T).max()
    hpl = R.bf16_round(rng.normal(0, 1, (5, 33, H)))
    dd = rng.normal(0, 1, (33, 10)).astype(np.float32)
    dd[rng.rand(33, 5).repeat(2, 1) < 0.5] = 0
    start = rng.normal(0, 1, (2, H)).astype(np.float32)
    want = start + R.dur_out_wgrad(dd, hpl)
    poisoned = hpl.copy()
    for d in range(5):
        poisoned[d][(dd[:, 2 * d:2 * d + 2] == 0).all(1)] = np.nan                   # excluded there too, not multiplied
    for planes in (hpl, poisoned):
        assert np.abs(R.kp_out_wgrad(dd, planes, start) - want).max() <= 1e-5 * R.dur_out_wgrad(np.abs(dd), np.abs(hpl)).max()
