"""GPU tests of the detrended-texture-encoder variant: the byte multi-hot embedding kernel (ptv_embed_multihot_fwd) and its backward
operand (ptv_multihot_bytes_rows) in isolation against fp64, EmbedMultihotFn's gradients, PtvaeEncoder.encode_multihot against the
float-copy route encoder(dt_x.float(), lengths), and the whole variant -- DisentangleVAE.init_model_detrended, the wiring of the
reference's train.py:31-39 -- against vectors the reference itself produced (tests/golden/make_golden_r9.py -> detrended_b4.npz).

Tolerances are taken from where the issue points: the embedding's forward bound is the (K+1)-term fp32 summation bound, the
weight-gradient tolerances are tests/test_gpu_kernels.py's TOL, 2e-5 on the encoder's mean / scale is tests/test_gpu_next_rows.py's bound for
this encoder, and the whole-model bounds are tests/test_gpu_model_wide.py's TF1_BOUNDS (its B = 4 conv-encoder case)."""
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from helpers import load_npz, reduced_params
from test_gpu_kernels import TOL
from test_gpu_model_wide import TF1_BOUNDS
from test_host_surface import build_reduced
from polyphonic_chord_texture_disentanglement_amd import dataset as D, functional as F_, model as M
from polyphonic_chord_texture_disentanglement_amd._lib import call, ptr, stream_ptr
from polyphonic_chord_texture_disentanglement_amd.ptvae import PtvaeEncoder
from polyphonic_chord_texture_disentanglement_amd.synthetic import fill_state_dict, synth_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
# (B, S, N, K, E, pad_col); the first is the dt_x geometry with real data, the others random bytes in 0..2
GEOMS = [(3, 32, 16, 39, 128, 3), (2, 4, 3, 12, 8, 11), (5, 3, 2, 64, 24, 0)]


def _host(t):
    return t.detach().cpu().numpy()


_CASES = {}


def _case(i):
    """(mh uint8 [B,S,N,K], W, bias, x or None) on the host, built once per geometry"""
    if i not in _CASES:
        B, S, N, K, E, pad = GEOMS[i]
        rs = np.random.RandomState(100 + i)
        x = None
        if i == 0:
            x, c, _ = synth_batch(B, 2024)
            mh = _host(D.detrend_pianotree(torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV)))
            assert mh.shape == (B, S, N, K) and mh.max() == 2
        else:
            mh = (rs.randint(0, 3, size=(B, S, N, K)) * (rs.rand(B, S, N, K) < 0.4)).astype(np.uint8)
            mh[0, 0, 0] = 0                                       # a row that is all zero ...
            mh[0, 0, 1] = rs.randint(1, 3, size=K)                # ... and one that is all non-zero
            mh[B - 1, S - 1, N - 1] = 2
        W = (rs.randn(E, K) / 3).astype(np.float32)
        bias = rs.randn(E).astype(np.float32)
        _CASES[i] = (mh, W, bias, x)
    return _CASES[i]


def _embed(mh, W, bias, pad, want_lengths=True):
    B, S, N, K = mh.shape
    E = W.shape[0]
    emb = torch.full((N, S, B, E), float('nan'), device=DEV)
    lengths = torch.full((S * B,), -7, device=DEV, dtype=torch.int32)
    call('ptv_embed_multihot_fwd', ptr(mh), ptr(W), ptr(bias), ptr(emb), ptr(lengths) if want_lengths else None, B, E, S, N, K,
         pad if want_lengths else -1, stream_ptr())
    torch.cuda.synchronize()
    return emb, lengths


@pytest.mark.parametrize('i', range(len(GEOMS)))
def test_embed_multihot_kernel_vs_fp64_bound_bits_and_lengths(i):
    B, S, N, K, E, pad = GEOMS[i]
    mh, W, bias, x = _case(i)
    mhd, Wd, bd = (torch.from_numpy(a).to(DEV) for a in (mh, W, bias))
    emb, lengths = _embed(mhd, Wd, bd, pad)
    A = mh.reshape(-1, K).astype(np.float64)
    ref = (A @ W.T.astype(np.float64) + bias.astype(np.float64)).reshape(B, S, N, E)
    mag = (A @ np.abs(W.T).astype(np.float64) + np.abs(bias).astype(np.float64)).reshape(B, S, N, E)
    got = _host(emb.permute(2, 1, 0, 3)).astype(np.float64)
    assert np.isfinite(got).all()
    err, bound = np.abs(got - ref), (K + 1) * U * mag
    print('EMBED_MH geometry', GEOMS[i], 'max err / bound', float((err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    zero_rows = ~mh.reshape(-1, K).any(-1)
    assert zero_rows.any() or i == 0
    assert np.array_equal(got.reshape(-1, E)[zero_rows], np.broadcast_to(bias.astype(np.float64), (int(zero_rows.sum()), E)))
    emb2, lengths2 = _embed(mhd, Wd, bd, pad)
    assert torch.equal(emb, emb2) and torch.equal(lengths, lengths2)                    # a pure function of the inputs
    emb3, untouched = _embed(mhd, Wd, bd, pad, want_lengths=False)
    assert torch.equal(emb, emb3) and (untouched == -7).all()
    want = (mh[..., pad] == 0).sum(-1)                                                   # [B,S]
    assert np.array_equal(_host(lengths).reshape(S, B).T, want)
    if x is not None:
        xd = torch.from_numpy(x).to(DEV)
        ref_len = torch.empty(S * B, device=DEV, dtype=torch.int32)
        call('ptv_grid_lengths', ptr(xd), ptr(ref_len), B, stream_ptr())
        assert torch.equal(lengths, ref_len)
        assert int(lengths.min()) < 16 and int(lengths.max()) >= 3
    # a misaligned view of the same bytes takes the byte-staging path: same result
    pad_buf = torch.zeros(mhd.numel() + 1, dtype=torch.uint8, device=DEV)
    pad_buf[1:] = mhd.reshape(-1)
    emb4, lengths4 = _embed(pad_buf[1:].view(B, S, N, K), Wd, bd, pad)
    assert torch.equal(emb, emb4) and torch.equal(lengths, lengths4)


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('i', range(len(GEOMS)))
def test_multihot_bytes_rows_is_the_permuted_widened_bytes(i, bf16):
    B, S, N, K, _E, _pad = GEOMS[i]
    mh = _case(i)[0]
    mhd = torch.from_numpy(mh).to(DEV)
    dt = torch.bfloat16 if bf16 else torch.float32
    want = torch.from_numpy(mh).permute(2, 1, 0, 3).reshape(N * S * B, K).float()
    for ld in (K, (K + 7) // 8 * 8):
        out = torch.full((N * S * B, ld), -1.0, device=DEV, dtype=dt)
        call('ptv_multihot_bytes_rows', ptr(mhd), ptr(out), ld, B, S, N, K, bf16, stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out[:, :K].float().cpu(), want), ld
        assert (out[:, K:] == 0).all(), ld


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('i', [0, 1])
def test_embed_multihot_fn_backward_vs_fp64_autograd(i, prec):
    B, S, N, K, E, pad = GEOMS[i]
    mh, W, bias, _ = _case(i)
    w = torch.nn.Parameter(torch.from_numpy(W).to(DEV))
    b = torch.nn.Parameter(torch.from_numpy(bias).to(DEV))
    G = torch.randn(N, S, B, E, generator=torch.Generator().manual_seed(5 + i))
    emb, lengths = F_.EmbedMultihotFn.apply(torch.from_numpy(mh).to(DEV), w, b, 1 if prec == 'bf16' else 0, pad)
    assert lengths.dtype == torch.int32 and lengths.shape == (S * B,) and not lengths.requires_grad
    (emb * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    w64 = torch.from_numpy(W).double().requires_grad_(True)
    b64 = torch.from_numpy(bias).double().requires_grad_(True)
    ref = torch.from_numpy(mh).double().permute(2, 1, 0, 3) @ w64.t() + b64               # [N,S,B,E]
    (ref * G.double()).sum().backward()
    for name, got, want in (('grad_W', w.grad, w64.grad), ('grad_b', b.grad, b64.grad)):
        err = float((got.cpu().double() - want).abs().max())
        lim = TOL[prec] * max(1.0, float(want.abs().max()))
        print('EMBED_MH_BWD', GEOMS[i], prec, name, 'err', err, 'limit', lim)
        assert err < lim, (name, err, lim)


def _train32_encoder():
    torch.manual_seed(0)
    enc = PtvaeEncoder(torch.device(DEV), z_size=256, max_pitch=39 - 8, min_pitch=0)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in enc.state_dict().items())
    enc.load_state_dict(fill_state_dict(shapes, seed=977))
    return enc.to(DEV)


def test_encode_multihot_vs_the_float_copy_route():
    enc = _train32_encoder()
    mh, _, _, x = _case(0)
    dt = torch.from_numpy(mh).to(DEV)
    lengths = enc.get_len_index_tensor(torch.from_numpy(x).to(DEV))                        # [B,32], the reference's
    with torch.no_grad():
        old, emb_old = enc.encoder(dt.float(), lengths)
        new, emb_new = enc.encode_multihot(dt, pad_col=3)
        given, _ = enc.encode_multihot(dt, lengths=lengths)
    assert emb_new.shape == emb_old.shape == (3, 32, 16, 128)
    assert not emb_new.is_contiguous() and emb_new.permute(2, 1, 0, 3).is_contiguous()      # the permuted step-major view
    for a, b_ in ((new.mean, old.mean), (new.scale, old.scale)):
        d = float((a - b_).abs().max())
        print('ENCODE_MH vs encoder(): max diff', d)
        assert d <= 2e-5
    assert torch.equal(given.mean, new.mean) and torch.equal(given.scale, new.scale)       # lengths given == lengths from pad_col
    assert (emb_new - emb_old).abs().max() <= 2e-5
    with pytest.raises(ValueError):
        enc.encode_multihot(dt)
    with pytest.raises(ValueError):
        enc.encode_multihot(dt.float(), pad_col=3)
    # the parameters' gradients flow through the new node
    dist, _ = enc.encode_multihot(dt, pad_col=3)
    (dist.mean.sum() + dist.scale.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0 for p in enc.parameters())


# ---------------------------------------------------------------------------------------------- the whole variant
@pytest.fixture(scope='module')
def golden():
    return load_npz('detrended_b4.npz')


@pytest.fixture(scope='module')
def inputs(golden):
    x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(int(golden['B']), int(golden['data_seed'])))
    return x, c, pr, torch.from_numpy(golden['dt_x']).to(DEV)


def _variant(golden, prec):
    m = M.DisentangleVAE.init_model_detrended(torch.device(DEV))
    shapes = OrderedDict((str(n), tuple(int(t) for t in s.strip('()').split(',') if t.strip())) for n, s in zip(golden['names'], golden['shapes']))
    m.load_state_dict(fill_state_dict(shapes, seed=1234))
    m = m.to(DEV).set_precision(prec)
    m.eps_source = lambda name, shape, device: torch.from_numpy(golden['eps_' + name]).to(device)
    return m


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_detrended_variant_teacher_forced_step_vs_reference(golden, inputs, prec):
    """train.py:31-39's model on (x, c, dt_x): both posteriors, the 11 losses, the gradient norms and 64 elements of every gradient tensor
    against the reference, held to the bounds of the B = 4 conv-encoder case.  Fails without the feature: run() had no way to take dt_x."""
    g = golden
    x, c, pr, dt_x = inputs
    m = _variant(g, prec)
    m.zero_grad()
    outs = m.run(x, c, pr, 1., 1., 1., dt_x=dt_x)
    losses = m.loss_function(x, c, *outs, float(g['beta']), [float(w) for w in g['weights']])
    dist_chd, dist_rhy = outs[2], outs[3]
    dpost = {k: float(np.abs(_host(t) - g[k]).max()) for k, t in (('mu_rhy', dist_rhy.mean), ('std_rhy', dist_rhy.scale),
                                                                   ('mu_chd', dist_chd.mean), ('std_chd', dist_chd.scale))}
    got = np.array([l.item() for l in losses])
    dloss = float(np.abs(got - g['losses']).max())
    losses[0].backward()
    worst_norm, worst_el, worst_name, tot2, ref2 = 0.0, 0.0, None, 0.0, 0.0
    for k, p in m.named_parameters():
        gn, ref = float(p.grad.double().pow(2).sum().sqrt()), float(g['gnorm.' + k])
        tot2, ref2 = tot2 + gn * gn, ref2 + ref * ref
        worst_norm = max(worst_norm, abs(gn - ref) / max(ref, 1e-30))
        idx = torch.from_numpy(g['gslice.%s.idx' % k]).to(DEV)
        el = float((p.grad.detach().reshape(-1)[idx].cpu() - torch.from_numpy(g['gslice.%s.val' % k])).abs().max()) / max(float(g['gmax.' + k]), 1e-30)
        if el > worst_el:
            worst_el, worst_name = el, k
    gnorm_rel = abs(tot2 ** 0.5 - ref2 ** 0.5) / ref2 ** 0.5
    print('DETRENDED_B4', prec, dict(dpost, dloss=dloss, gnorm_rel=gnorm_rel, worst_tensor_norm_rel=worst_norm, worst_elem_over_max=worst_el,
                                     worst_elem_tensor=worst_name))
    b = TF1_BOUNDS[prec]
    if prec == 'fp32':
        assert dpost['mu_rhy'] <= 2e-5 and dpost['std_rhy'] <= 2e-5, dpost
    assert dloss <= b[0], (dloss, got, g['losses'])
    assert gnorm_rel <= b[2], gnorm_rel
    assert worst_norm <= b[3], worst_norm
    assert worst_el <= b[4] + 2e-6, (worst_el, worst_name)
    assert np.array_equal(_host(m.decoder.get_len_index_tensor(x)), g['lengths'])


def test_loss_without_dt_x_is_loss_with_it_bit_for_bit(golden, inputs):
    x, c, pr, dt_x = inputs
    m = _variant(golden, 'bf16')
    res = []
    for args in ((x, c, pr), (x, c, pr, dt_x)):
        m.zero_grad()
        random.seed(3)
        losses = m.loss(*args, 1., 1., 1., 0.1, [1, 0.5])
        losses[0].backward()
        torch.cuda.synchronize()
        res.append((torch.stack([l.detach() for l in losses]), m.rhy_encoder.note_embedding.weight.grad.clone(),
                    m.rhy_encoder.enc_time_gru.weight_hh_l0.grad.clone()))
    for a, b_ in zip(*res):
        assert torch.equal(a, b_)
    assert torch.equal(D.detrend_pianotree(x, c), dt_x)
    with pytest.raises(ValueError, match='dt_x'):
        m.loss(x, c, pr, pr, 1., 1., 1.)                                                   # a piano-roll in the dt_x slot
    with pytest.raises(ValueError, match='dt_x'):
        m.run(x, c, pr, 1., 1., 1., dt_x=dt_x[:2])


def test_three_eager_training_steps_of_the_variant(monkeypatch, tmp_path):
    from polyphonic_chord_texture_disentanglement_amd import graph_step
    from polyphonic_chord_texture_disentanglement_amd.amc_dl import torch_plus as tp
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import MusicDataLoaders, TrainingVAE
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('PTV_GRAPH_STEP', raising=False)
    built = []
    real = graph_step.GraphedTrainStep
    monkeypatch.setattr(graph_step, 'GraphedTrainStep', lambda *a, **k: built.append(1) or real(*a, **k))

    def go():
        torch.manual_seed(0)
        random.seed(7)
        m = M.DisentangleVAE.init_model_detrended(torch.device(DEV)).to(DEV).set_precision('bf16')
        m.use_philox(seed=7)
        before = {k: p.detach().clone() for k, p in m.rhy_encoder.named_parameters()}
        opt = FusedClipAdam(m.parameters(), lr=1e-3)
        osch = tp.OptimizerScheduler(opt, tp.MinExponentialLR(opt, gamma=0.9999, minimum=1e-5), 1)
        ps = tp.ParameterScheduler(tfr1=tp.ConstantScheduler(1.), tfr2=tp.ConstantScheduler(1.), tfr3=tp.ConstantScheduler(1.),
                                   beta=tp.ConstantScheduler(0.1), weights=tp.ConstantScheduler([1, 0.5]))
        loaders = MusicDataLoaders.get_loaders(21, bs_train=8, bs_val=8, n_train_batch=3, n_val_batch=1, slots=('dt_x',))
        pm = tp.LogPathManager(None)
        sw = tp.SummaryWriters(M.LOSS_NAMES, {'loss': None}, pm.writer_path)
        tr = TrainingVAE(torch.device(DEV), m, False, pm, loaders, sw, osch, ps, 1)
        tr.freeze_gc_after_steps = None
        assert len(tr._batch_to_inputs(next(iter(loaders.train_loader)))) == 4
        sums = tr.train()
        torch.cuda.synchronize()
        assert tr.train_step == 3 and all(np.isfinite(v) for v in sums.values()), sums
        for k, p in m.rhy_encoder.named_parameters():
            assert not torch.equal(p.detach(), before[k]), k
        return sums, [p.detach().clone() for p in m.parameters()]
    sums_a, params_a = go()
    sums_b, params_b = go()
    assert sums_a == sums_b
    assert all(torch.equal(a, b_) for a, b_ in zip(params_a, params_b))
    assert not built                                                                       # the replayed step was never entered


def test_inference_family_takes_dt_x_in_the_pr_mat_slot(golden, inputs):
    x, c, pr, dt_x = inputs
    m = _variant(golden, 'fp32')
    est = m.inference(dt_x[:2], c[:2], sample=False)
    assert est.shape == (2, 32, 15, 6)
    sw = m.swap(dt_x[:2], dt_x[2:4], c[:2], c[2:4], True, False)                           # texture of the first pair, chords of the second
    assert sw.shape == (2, 32, 15, 6)
    dist_chd, dist_rhy = m.inference_encode(dt_x[:2], c[2:4])
    assert np.array_equal(sw, m.inference_decode(dist_chd.mean, dist_rhy.mean))
    assert np.abs(_host(m.inference_encode(dt_x, c)[1].mean) - golden['mu_rhy']).max() <= 2e-5
    for bad in (pr[:2], dt_x[:2].float()):
        with pytest.raises(ValueError, match='dt_x'):
            m.inference(bad, c[:2], sample=False)
        with pytest.raises(ValueError, match='dt_x'):
            m.swap(bad, bad, c[:2], c[:2], True, True)


def test_conv_model_inference_is_what_it_was():
    """with a TextureEncoder the pr_mat slot is the piano-roll and inference() is the encoders' means decoded, as before"""
    m = build_reduced(DEV)
    m.load_state_dict(reduced_params())
    m = m.to(DEV)
    assert not m.detrended
    x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(3, 107))
    est = m.inference(pr, c, sample=False)
    with torch.no_grad():
        zc, zr = m.chd_encoder(c).mean, m.rhy_encoder(pr).mean
    assert est.shape == (3, 32, 15, 6) and np.array_equal(est, m.inference_decode(zc, zr))
    assert np.array_equal(est, m.inference(pr, c, sample=False))
    dt_x = D.detrend_pianotree(x, c)
    m.zero_grad()
    random.seed(1)
    m.eps_source = lambda name, shape, device: torch.zeros(shape, device=device)
    a = torch.stack([l.detach() for l in m.loss(x, c, pr, 1., 1., 1.)])
    random.seed(1)
    b_ = torch.stack([l.detach() for l in m.loss(x, c, pr, dt_x, 1., 1., 1.)])              # the fourth tensor is still ignored
    assert torch.equal(a, b_)
