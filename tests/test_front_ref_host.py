"""Guards tests/front_ref.py, the references of tests/test_gpu_front_kernels.py, against torch's own float64 CPU operators and
autograd, the oracle and the committed goldens, and shows that the inputs that module builds meet the conditions it relies on: at
most 0.1 % of the pooled positions of every float texture case are undecided, and the slerp pairs are well conditioned (two fp32
evaluations of the formula that sum their dot products in different orders agree within each other's bound).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import front_ref as R
from helpers import load_npz

RTOL = 1e-12


def close(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    s = np.abs(want).max() if scale is None else scale
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= RTOL * max(s, 1e-300), (np.abs(got - want).max(), s)


# ------------------------------------------------------------------------------------------------ texture front end
@pytest.mark.parametrize('B,C', [(1, 1), (3, 10), (5, 16)])
def test_texture_reference_vs_torch_float64(B, C):
    c = R.texture_case('float', B, C)
    pr, d = torch.tensor(c['pr'], dtype=torch.float64), torch.tensor(c['d'], dtype=torch.float64)
    w = torch.tensor(c['w'], dtype=torch.float64).reshape(C, 1, 4, 12).requires_grad_()
    b = torch.tensor(c['bias'], dtype=torch.float64).requires_grad_()
    conv = TF.conv2d(pr.unsqueeze(1), w, b, stride=(4, 1))                                      # [B,C,8,117]
    v = R.txt_conv(c['pr'], c['w'], c['bias'])
    close(v, conv.detach()[..., :116].reshape(B, C, 8, 29, 4).numpy())
    pooled, arg = R.txt_fwd(c['pr'], c['w'], c['bias'])
    ref = TF.max_pool2d(torch.relu(conv), (1, 4))
    close(pooled, ref.detach().numpy())
    (ref * d).sum().backward()
    dw, db = R.txt_bwd(c['pr'], arg, c['d'])
    close(dw, w.grad.reshape(C, 48).numpy())
    close(db, b.grad.numpy())
    assert (pooled[arg < 0] == 0).all() and (pooled[arg >= 0] > 0).all()
    assert np.array_equal(np.take_along_axis(v, np.maximum(arg, 0)[..., None], -1)[..., 0][arg >= 0], pooled[arg >= 0])
    assert np.array_equal(R.txt_feat_rows(pooled).reshape(-1), pooled.reshape(-1))              # the raw view: the same memory
    assert R.txt_arg_rows(arg)[1 * 8 + 3 if B > 1 else 3, (C - 1) * 29 + 5] == arg[1 if B > 1 else 0, C - 1, 3, 5]


def test_texture_tie_and_relu_rules_on_hand_made_windows():
    pr = np.zeros((1, 32, 128), np.float32)
    pr[0, 0, 40] = 3                                    # beat 0: one note, seen by the windows at columns 29 .. 40
    w = np.zeros((3, 48), np.float32)
    w[:, 0:12] = 1                                      # every tap of the first row: v = bias + 3 wherever the note is in the window
    bias = np.array([1, 0, -4], np.float32)
    pooled, arg = R.txt_fwd(pr, w, bias)
    assert (arg[0, 0, 1:] == 0).all() and (pooled[0, 0, 1:] == 1).all()                          # empty beats, bias > 0: a four-way tie -> 0
    assert (arg[0, 1, 1:] == -1).all() and (pooled[0, 1, 1:] == 0).all()                         # bias = 0: nothing exceeds 0
    assert (arg[0, 2] == -1).all() and not pooled[0, 2].any()                                    # 3 - 4 < 0: cut by the ReLU
    # beat 0, channel 0: columns 29 .. 40 give 4, the others 1 -> position 7 (columns 28 .. 31) takes its second window, 8 .. 10 the first
    assert arg[0, 0, 0, 6:12].tolist() == [0, 1, 0, 0, 0, 0] and pooled[0, 0, 0, 6:12].tolist() == [1, 4, 4, 4, 4, 1]
    assert arg[0, 1, 0, 6:12].tolist() == [-1, 1, 0, 0, 0, -1]
    d = np.ones((1, 3, 8, 29), np.float32)
    dw, db = R.txt_bwd(pr, arg, d)
    assert db.tolist() == [8 * 29, 4, 0] and not dw[2].any()
    assert dw[1, :12].tolist() == [3, 0, 0, 0, 3, 0, 0, 0, 3, 0, 0, 3]       # the note's tap in the windows at columns 40, 36, 32, 29
    und = R.txt_undecided(pr, w, bias)
    assert not und[0, 0, 1:].any() and not und[0, 1, 1:].any()  # identical windows tie exactly; bias = 0 over an empty window IS the 0 candidate
    assert np.nonzero(und[0, 0, 0])[0].tolist() == [7, 8, 9]     # equal values of windows with DIFFERENT inputs: equal by these weights only
    assert R.txt_undecided(pr, w, np.array([1e-9, 0, -3 + 1e-9], np.float32))[0, 2, 0, 7]         # 3 - 3 + 1e-9 against 0: undecided


@pytest.mark.parametrize('B,C', R.TXT_SHAPES)
def test_texture_cases_are_decided_and_the_integer_ones_exact(B, C):
    c = R.texture_case('float', B, C)
    share = R.txt_undecided(c['pr'], c['w'], c['bias']).mean()
    print('undecided share B=%d C=%d: %.2e' % (B, C, share))
    assert share <= 1e-3
    c = R.texture_case('int', B, C)
    pooled, arg = R.txt_fwd(c['pr'], c['w'], c['bias'])
    assert sorted(set(c['bias'].tolist())) == ([1] if C == 1 else [-2, 0, 1])
    empty = ~R.txt_patches(c['pr']).any(-1)                                                      # [B,8,29,4]
    all_empty = empty.all(-1)
    assert 0.005 < all_empty.mean() < 0.05                                                       # the exact four-way ties of the issue
    for ch in range(C):
        a = arg[:, ch][all_empty]
        assert (a == (0 if c['bias'][ch] > 0 else -1)).all()
    assert 0.01 <= (arg < 0).mean() <= 0.9
    dw, db = R.txt_bwd(c['pr'], arg, c['d'])
    adw, adb = R.txt_bwd(c['pr'], arg, c['d'], absolute=True)
    assert max(adw.max() + 5, adb.max() + 5, R.txt_conv(c['pr'], c['w'], c['bias'], absolute=True).max()) < 2 ** 24
    assert np.array_equal(dw, np.round(dw)) and np.array_equal(pooled, np.round(pooled))


# ------------------------------------------------------------------------------------------------ note embedding
def test_embedding_references_vs_the_oracle_at_the_default_geometry():
    from oracle.ptvae_oracle import Oracle
    rng = np.random.RandomState(2)
    x = R.grid_case(3, 5, R.DEFAULT_GEOM)
    x[..., 0] = np.clip(x[..., 0], 0, 130)                                                       # the oracle scatters: indices 0 .. 130 only
    W, bias = rng.randint(-256, 257, (24, 135)) / 64.0, rng.randint(-256, 257, 24) / 64.0       # the oracle's fp32 sums are exact
    o = Oracle.__new__(Oracle)
    o.p = {'decoder.note_embedding.weight': torch.tensor(W, dtype=torch.float32), 'decoder.note_embedding.bias': torch.tensor(bias, dtype=torch.float32)}
    emb, lengths = o.emb_x(torch.tensor(x))                                                      # [B,32,16,E], [B,32]
    got, scale = R.embed(x, W, bias, 130)
    assert np.array_equal(got, emb.permute(2, 1, 0, 3).numpy().astype(np.float64))
    assert np.array_equal(R.grid_lengths(x, 130), lengths.numpy().T)
    mh = R.multihot(x, 130)
    assert np.array_equal(mh @ W.T + bias, got.reshape(-1, 24)) and mh[:, :130].sum(1).max() == 1 and mh[:, 130:].max() == 2
    assert (scale >= np.abs(got)).all()


def test_embedding_out_of_range_pitches_add_no_column():
    for geom in [R.DEFAULT_GEOM] + R.GEOMS:
        S, N, P, D, pad = geom
        x = R.grid_case(5, 2, geom)
        assert x[..., 0].reshape(2, -1)[:, :4].tolist() == [[-1, P - 1, P, P + 1]] * 2
        rng = np.random.RandomState(1)
        W, bias = rng.normal(0, 1, (6, P + D)), rng.normal(0, 1, 6)
        emb, _ = R.embed(x, W, bias, P)
        mh = R.multihot(x, P)
        assert mh.shape == (N * S * 2, P + D) and emb.shape == (N, S, 2, 6)
        close(emb.reshape(-1, 6), mh @ W.T + bias, scale=10.0)
        rows = mh.reshape(N, S, 2, P + D)
        first = [(k // N, k % N) for k in range(4)]                                              # (step, slot) of the four special pitches
        assert [int(rows[n, s, 0, :P].sum()) for s, n in first] == [0, 1, 0, 0]
        assert rows[first[1][1], first[1][0], 0, P - 1] == 1
        assert R.grid_lengths(x, pad)[0, 0] == N - (x[0, 0, :, 0] == pad).sum()


# ------------------------------------------------------------------------------------------------ layout, routing, tokens
def test_layout_references_on_hand_made_cases():
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    assert R.transpose01(a)[2, 1].tolist() == a[1, 2].tolist() and R.transpose01(a).shape == (3, 2, 4)
    idx = np.array([2, 0, 1])
    g = R.gather_rows(a, idx)
    assert g[1, 0].tolist() == a[1, 2].tolist() and np.array_equal(R.scatter_rows(g, idx), a)
    assert R.scatter_rows(a, idx)[0, 2].tolist() == a[0, 0].tolist()
    dst = np.ones((2, 3), np.float32)
    assert R.copy2d(dst, [1, 2, 3], -0.5, 1).tolist() == [[0.5, 0, -0.5]] * 2
    assert R.copy2d(dst, [[1, 2, 3], [4, 5, 6]], 1.0, 0).tolist() == [[1, 2, 3], [4, 5, 6]]
    src = np.arange(6, dtype=np.float32).reshape(3, 2)
    A, B = np.full((3, 2), 7, np.float32), np.full((3, 2), 9, np.float32)
    ra, rb = R.route_slices(src, [1, 0, 1], A, B, 0)
    assert ra.tolist() == [[0, 1], [7, 7], [4, 5]] and rb.tolist() == [[9, 9], [2, 3], [9, 9]]
    ra, rb = R.route_slices(src, [1, 0, 1], A, None, 1)
    assert ra.tolist() == [[7, 8], [7, 7], [11, 12]] and rb is None


def test_token_references_vs_the_reference_models_indexing():
    rng = np.random.RandomState(4)
    M = 6
    pitch = rng.normal(0, 3, (M, 130))
    pitch[0, [1, 129]] = 50                                                                      # tie: the first
    pitch[1, :] = 2.0
    pitch[2, 129] = 60
    bits = rng.randint(0, 2, (5, M))
    W, bias = rng.normal(0, 1, (8, 135)), rng.normal(0, 1, 8)
    plen = np.array([0, 4, 0, 0, 7, 0])
    force = np.array([-1, -1, -1, 129, 129, 5])
    idx, pred, scale, xhat, L = R.note_token(pitch, bits, W, bias, plen, 9, 0, force)
    assert idx.tolist()[:2] == [1, 0] and idx.tolist()[2:] == [129, 129, 129, 5]
    assert L.tolist() == [0, 4, 9, 9, 7, 0] and R.note_token(pitch, bits, W, bias, plen, 9, 1, force)[4].tolist() == [9, 4, 9, 9, 7, 9]
    tok = torch.zeros(M, 135, dtype=torch.float64)                                               # ptvae.py:328-334
    tok[range(M), torch.tensor(idx)] = 1.
    tok[:, 130:] = torch.tensor(bits.T, dtype=torch.float64)
    close(pred, (tok @ torch.tensor(W).t() + torch.tensor(bias)).numpy(), scale=scale.max())
    assert xhat[:, 0].tolist() == idx.tolist() and np.array_equal(xhat[:, 1:], bits.T)
    free = R.note_token(pitch, bits, W, bias, plen, 9, 0)[0]
    assert torch.equal(torch.tensor(pitch).max(1)[1], torch.tensor(free))
    B = 5
    root, bass, chroma = rng.normal(0, 1, (B, 12)), rng.normal(0, 1, (B, 12)), rng.normal(0, 1, (B, 24))
    root[0, [3, 9]] = 5
    chroma[:, 4:6] = 0.25                                                                        # an equal pair: 0
    rt, bt, ct = (torch.tensor(a) for a in (root, bass, chroma.reshape(B, 1, 12, 2)))
    t_root = torch.zeros(B, 1, 12)                                                               # ptvae.py:73-78
    t_root[torch.arange(0, B), 0, rt.unsqueeze(1).max(-1)[-1]] = 1.
    t_bass = torch.zeros(B, 1, 12)
    t_bass[torch.arange(0, B), 0, bt.unsqueeze(1).max(-1)[-1]] = 1.
    want = torch.cat([t_root, ct.max(-1)[-1].float(), t_bass], -1)[:, 0].numpy()
    got = R.chord_token(root, chroma, bass)
    assert np.array_equal(got, want.astype(np.int64)) and got[0, 3] == 1 and not got[:, 14].any()
    assert (got[:, :12] == got[0, :12]).all() and got[0, :12].sum() == len(set(root.argmax(1)))


# ------------------------------------------------------------------------------------------------ slerp path
def test_slerp_reference_vs_the_committed_golden():
    g = load_npz('reduced_family.npz')
    out, length = R.slerp_path(g['z_chd1'][:1], g['z_chd2'][:1], 7)
    np.testing.assert_allclose(out[0], g['interp_path'], rtol=0, atol=2e-6)
    out, length = R.slerp_path(g['z_chd1'][:3], g['z_chd2'][:3], 5)
    np.testing.assert_allclose(out, g['interp_z_chd'][:3], rtol=0, atol=2e-6)
    close(np.linalg.norm(out, axis=-1), length)
    close(out[:, 0], g['z_chd1'][:3].astype(np.float64), scale=1.0)
    close(out[:, -1], g['z_chd2'][:3].astype(np.float64), scale=1.0)


@pytest.mark.parametrize('angles', sorted(R.SLERP_ANGLES))
@pytest.mark.parametrize('B,D,n', R.SLERP_SHAPES)
def test_slerp_cases_are_well_conditioned(B, D, n, angles):
    z1, z2 = R.slerp_case(B, D, n, angles)
    lo, hi = R.SLERP_ANGLES[angles]
    cos = (z1.astype(np.float64) * z2).sum(1) / np.linalg.norm(z1.astype(np.float64), axis=1) / np.linalg.norm(z2.astype(np.float64), axis=1)
    assert (np.arccos(cos) > lo * 0.99).all() and (np.arccos(cos) < hi * 1.01).all()
    norms = np.concatenate([np.linalg.norm(z1, axis=1), np.linalg.norm(z2, axis=1)])
    assert norms.min() >= 0.99e-2 and norms.max() <= 1.01e2 and (B < 300 or (norms.min() < 3e-2 and norms.max() > 30))
    ref, length = R.slerp_path(z1, z2, n)
    rel = ref / length[..., None]                                                                # every row has unit length: the scale is 1
    a, b = (R.slerp_f32(z1, z2, n, o).astype(np.float64) / length[..., None] for o in ('pair', 'lanes'))
    print('slerp %s B=%d D=%d n=%d: fp32 errors %.2e (pairwise sums), %.2e (64 lanes)' % (angles, B, D, n, np.abs(a - rel).max(), np.abs(b - rel).max()))
    for x, y in ((a, b), (b, a)):
        bound, _ = R.check_bound(rel, x, 1.0)
        assert np.abs(y - rel).max() <= bound.min()
