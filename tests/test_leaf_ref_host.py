"""Guards tests/leaf_ref.py, the fp64 references of the leaf-kernel tests, against torch's own float64 CPU operators and autograd.
No GPU.  Agreement is to 1e-12 relative."""
import numpy as np
import torch
import torch.nn.functional as F

import leaf_ref as R

RTOL = 1e-12


def close(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    s = np.abs(want).max() if scale is None else scale
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= RTOL * max(s, 1e-300), (np.abs(got - want).max(), s)


def ce_case(seed, rows, C, ignore, frac):
    rng = np.random.RandomState(seed)
    x = rng.normal(0, 3, (rows, C))
    x[1] += 3e4
    x[2, :] = 1.5                                                     # exact ties
    x[3, 1::3] = -np.inf
    t = rng.randint(0, C, rows)
    t[3] = 0
    t[rng.rand(rows) < frac] = ignore
    return x, t


def test_ce_sum_and_grad_vs_torch_cross_entropy():
    for C, ignore, frac in ((130, 130, 0.6), (2, 2, 0.5), (12, -1, 0.0), (17, 17, 0.3)):
        x, t = ce_case(C, 37, C, ignore, frac)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        loss = F.cross_entropy(xt, torch.tensor(t), ignore_index=ignore, reduction='sum')
        loss.backward()
        close(R.ce_sum(x, t, ignore), loss.item())
        close(R.ce_grad(x, t, ignore, -0.37), -0.37 * xt.grad.numpy(), scale=0.37)


def test_ce_ignored_rows_are_excluded_not_multiplied():
    x, t = ce_case(5, 37, 130, 130, 0.6)
    want, wantg = R.ce_sum(x, t, 130), R.ce_grad(x, t, 130, 2.0)
    x[t == 130] = np.nan
    assert R.ce_sum(x, t, 130) == want and np.array_equal(R.ce_grad(x, t, 130, 2.0), wantg)
    assert R.ce_sum(x, np.full(37, 130), 130) == 0.0 and not R.ce_grad(x, np.full(37, 130), 130).any()


def test_ce_groups_vs_torch_per_group():
    G, gs = 5, np.array([1.0, -0.37, 0.0, 0.5, 2.25])
    x, t = ce_case(9, 35, 2, 2, 0.4)
    t[3::G] = 2                                                       # a group without targets
    sums, counts = R.ce_sum(x, t, 2, groups=G)
    grad = R.ce_grad(x, t, 2, gs)
    for g in range(G):
        xt = torch.tensor(x[g::G], dtype=torch.float64, requires_grad=True)
        loss = F.cross_entropy(xt, torch.tensor(t[g::G]), ignore_index=2, reduction='sum')
        loss.backward()
        close(sums[g], loss.item(), scale=max(abs(loss.item()), 1.0))
        assert counts[g] == int((t[g::G] != 2).sum())
        close(grad[g::G], gs[g] * xt.grad.numpy(), scale=1.0)
    assert counts[3] == 0 and sums[3] == 0.0


def test_kl_and_reparam_vs_autograd():
    rng = np.random.RandomState(3)
    mu, sd = rng.normal(0, 1, (7, 9)), np.exp(rng.uniform(np.log(1e-3), np.log(30), (7, 9)))
    eps, dz, de, ds = (rng.normal(0, 1, (7, 9)) for _ in range(4))
    mt, st = (torch.tensor(a, requires_grad=True) for a in (mu, sd))
    # the KL of N(mu, sd) against N(0, 1), by torch.distributions, and its sum under autograd
    kl = torch.distributions.kl_divergence(torch.distributions.Normal(mt, st), torch.distributions.Normal(0., 1.)).sum()
    close(R.kl_sum(mu, sd), kl.item())
    gm, gs = torch.autograd.grad(0.1 * kl, (mt, st))
    dmu, dsd = R.kl_grad(mu, sd, 0.1)
    close(dmu, gm.numpy())
    close(dsd, gs.numpy())
    # z = mu + sd eps with sd = exp(lv); loss = <dz, z> + klw * kl + <dmu_ext, mu> + <dsd_ext, sd>
    lv = torch.tensor(np.log(sd), requires_grad=True)
    s2 = lv.exp()
    z = mt + s2 * torch.tensor(eps)
    z_ref, kl_ref = R.reparam_fwd(mu, sd, eps)
    close(z_ref, z.detach().numpy())
    close(kl_ref, kl.item())
    assert np.array_equal(R.reparam_fwd(mu, sd, None)[0], mu)
    klt = (-s2.log() + (s2 * s2 + mt * mt) * 0.5 - 0.5).sum()
    obj = (torch.tensor(dz) * z).sum() + 0.1 * klt + (torch.tensor(de) * mt).sum() + (torch.tensor(ds) * s2).sum()
    g_mu, g_lv = torch.autograd.grad(obj, (mt, lv))
    dmu, dlv = R.reparam_bwd(mu, sd, eps, dz, de, ds, 0.1, 1)
    close(dmu, g_mu.numpy())
    close(dlv, g_lv.numpy())
    close(R.reparam_bwd(mu, sd, eps, dz, de, ds, 0.1, 0)[1], g_lv.numpy() / sd)
    dmu0, dsd0 = R.reparam_bwd(mu, sd, None, dz, None, None, 0.0, 0)
    assert np.array_equal(dmu0, dz) and not dsd0.any()


def composition(s, c, beta, w0, w1, n_kl, n_root, n_chroma):
    pl, dl = s[0] / c[0], s[1] / c[1]
    klc, klr = s[2] / n_kl, s[3] / n_kl
    root, chroma, bass = s[4] / n_root, s[5] / n_chroma, s[6] / n_root
    recon, kl, chord = w0 * pl + w1 * dl, klc + klr, root + chroma + bass
    return torch.stack([recon + beta * kl + chord, recon, pl, dl, kl, klc, klr, chord, root, chroma, bass])


def test_loss_finalize_and_bwd_scales_vs_autograd_of_the_composition():
    rng = np.random.RandomState(4)
    sums, counts = rng.uniform(1, 900, 7), np.array([311, 1777])
    args = (0.1, 1.0, 0.5, 512.0 * 256, 4096.0, 4096.0 * 12)
    st = torch.tensor(sums, requires_grad=True)
    out = composition(st, torch.tensor(counts, dtype=torch.float64), *args)
    close(R.loss_finalize(sums, counts, *args), out.detach().numpy())
    for g in (np.eye(11)[0], rng.normal(0, 1, 11)):
        gs, = torch.autograd.grad(out, st, torch.tensor(g), retain_graph=True)
        close(R.loss_bwd_scales(g, counts, *args), gs.numpy())
    empty = R.loss_finalize(np.zeros(7), np.array([0, 5]), *args)
    assert np.isnan(empty[[0, 1, 2]]).all() and not np.isnan(empty[3:]).any()


def test_wdur_pair_vs_autograd():
    rng = np.random.RandomState(6)
    gsum, gcnt, w = rng.uniform(1, 50, 5), np.array([9, 31, 2, 77, 5]), np.array([1, .6, .4, .3, .3])
    st = torch.tensor(gsum, requires_grad=True)
    dl = (torch.tensor(w) * st / torch.tensor(gcnt, dtype=torch.float64)).sum()
    got, one = R.wdur_finalize(gsum, gcnt, w)
    assert one == 1
    close(got, dl.item())
    g, = torch.autograd.grad(-0.7 * dl, st)
    close(R.wdur_scales(-0.7, gcnt, w), g.numpy())


def test_clip_adam_three_steps_vs_clip_grad_norm_and_torch_adam():
    rng = np.random.RandomState(8)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    for n, clip, gscale in ((1000, 3.0, 1.0), (1000, 1e4, 1.0), (77, 3.0, 0.5), (5, 0.0, 0.5)):
        p0 = rng.normal(0, 1, n)
        pt = torch.nn.Parameter(torch.tensor(p0))
        opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
        p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
        for step in (1, 2, 3):
            g = rng.normal(0, 1, n) * rng.choice([0.3, 1.0, 4.0])
            pt.grad = torch.tensor(g * gscale)                       # gscale is applied before clipping ...
            if clip > 0:
                torch.nn.utils.clip_grad_norm_([pt], clip)
            opt.step()
            p, m, v = R.clip_adam(p, g, m, v, R.sumsq(g), gscale, clip, lr, b1, b2, eps, step)      # ... sumsq is of the unscaled buffer
            close(p - p0, pt.detach().numpy() - p0, scale=lr)
            close(m, opt.state[pt]['exp_avg'].numpy())
            close(v, opt.state[pt]['exp_avg_sq'].numpy())


def test_targets_and_reductions_on_hand_made_cases():
    x = np.zeros((2, 32, 16, 6), np.int64)
    x[..., 0], x[..., 1:] = 130, 2
    x[1, 4, 15] = [60, 1, 0, 2, 2, 2]                                 # sample 1: one live slot, note step 14
    x[0, 7, 3, 3] = 1                                                 # sample 0: a duration bit alone makes note step 2 live
    for sm in (0, 1):
        pt, dt, counts, row_live = R.pianotree_targets(x, sm)
        assert pt.shape == (960,) and dt.shape == (960, 5) and row_live.shape == (32, 2)
        assert counts.tolist() == [1, 3, 14] and row_live[4, 1] == 15 and row_live[7, 0] == 3 and row_live.sum() == 18
        r = (14 * 32 + 4) * 2 + 1 if sm else (1 * 32 + 4) * 15 + 14
        assert pt[r] == 60 and dt[r].tolist() == [1, 0, 2, 2, 2] and (np.delete(pt, r) == 130).all()
    x[1, 4, 15] = [130, 2, 2, 2, 2, 2]
    assert R.pianotree_targets(x, 0)[2].tolist() == [0, 1, 2]
    c = np.zeros((2, 8, 36))
    c[0, 1, 11] = c[0, 1, 24] = c[1, 0, 0] = c[1, 0, 35] = c[1, 0, 13] = 1
    root, chroma, bass = R.chord_targets(c, 0)
    assert root[1] == 11 and bass[1] == 0 and root[8] == 0 and bass[8] == 11 and chroma[8].tolist() == [0, 1] + [0] * 10
    assert root[0] == 0 and bass[0] == 0                              # all-zero row: the first maximum
    root, _, bass = R.chord_targets(c, 1)
    assert root[1 * 2 + 0] == 11 and bass[0 * 2 + 1] == 11
    a = np.arange(12.).reshape(4, 3)
    assert R.colsum(a).tolist() == [[18, 22, 26]]
    assert R.colsum(a, [0, 1, 1, 2], 2).tolist() == [[0, 1, 2], [9, 11, 13]]
    assert R.sum_steps(a).tolist() == [18, 22, 26] and R.sum_steps(a, 1).tolist() == [3, 5, 7]
    z = np.zeros((200, 4))
    assert R.last_nonzero_unit(z, 64) == -1 and R.last_nonzero_unit(z, 64, 5) == 5
    z[70, 1] = np.nan
    z[130, 0] = -0.0
    assert R.last_nonzero_unit(z, 64) == 1 and R.last_nonzero_unit(z, 1) == 127 and R.last_nonzero_unit(z, 96) == 1
    z[199, 3] = 1e-30
    assert R.last_nonzero_unit(z, 64) == 3 and R.last_nonzero_unit(z, 1) == 199 and R.last_nonzero_unit(z, 64, 9) == 9
    assert R.sumsq([3, 4]) == 25
