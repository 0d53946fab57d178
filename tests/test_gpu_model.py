"""GPU parity of the full train-step path (model -> loss -> backward) against the golden vectors
produced by the reference itself, and against the CPU oracle on fresh inputs."""
import numpy as np
import pytest
import torch

from helpers import CoinList, full_params, load_npz, reduced_params
from oracle.ptvae_oracle import Oracle
from polyphonic_chord_texture_disentanglement_amd import model as M
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch
from test_host_surface import build_reduced

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _eps_source(g):
    def src(name, shape, device):
        return torch.from_numpy(g['eps_' + name]).to(device)
    return src


def _run(m, g, x, c, pr):
    m.eps_source = _eps_source(g)
    m.zero_grad()
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    outs = m.run(xt, ct, prt, 1., 1., 1.)
    losses = m.loss_function(xt, ct, *outs, float(g['beta']), [float(w) for w in g['weights']])
    return outs, losses


def test_reduced_tf1_forward_backward_vs_reference_golden():
    g = load_npz('reduced_tf1.npz')
    m = build_reduced(DEV).to(DEV)
    outs, losses = _run(m, g, g['x'], g['c'], g['pr_mat'])
    got = np.array([l.item() for l in losses])
    np.testing.assert_allclose(got, g['losses'], rtol=0, atol=1e-4)       # the north-star bar
    np.testing.assert_allclose(got, g['losses'], rtol=0, atol=1e-5)       # what fp32 MFMA actually achieves
    pitch, dur, dc, dr, root, chroma, bass = outs
    assert pitch.shape == (3, 32, 15, 130) and dur.shape == (3, 32, 15, 5, 2)
    assert root.shape == (3, 8, 12) and chroma.shape == (3, 8, 12, 2) and bass.shape == (3, 8, 12)
    for name, t in (('pitch_outs', pitch), ('dur_outs', dur), ('mu_chd', dc.mean), ('std_chd', dc.scale),
                    ('mu_rhy', dr.mean), ('std_rhy', dr.scale), ('recon_root', root), ('recon_chroma', chroma),
                    ('recon_bass', bass)):
        np.testing.assert_allclose(t.detach().cpu().numpy(), g[name], rtol=0, atol=2e-5, err_msg=name)
    losses[0].backward()
    for k, p in m.named_parameters():
        ref = g['grad.' + k]
        assert p.grad is not None, k
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=0, atol=2e-6 + 2e-4 * np.abs(ref).max(), err_msg=k)


@pytest.mark.parametrize('case', ['tf1_b4', 'tf1_b16'])
def test_full_config_vs_reference_golden(case):
    g = load_npz('full_%s.npz' % case)
    x, c, pr = synth_batch(int(g['B']), int(g['data_seed']))
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV)
    outs, losses = _run(m, g, x, c, pr)
    got = np.array([l.item() for l in losses])
    np.testing.assert_allclose(got, g['losses'], rtol=0, atol=1e-4)
    for name, t in (('pitch_outs', outs[0]), ('dur_outs', outs[1])):
        flat = t.detach().contiguous().cpu().numpy().reshape(-1)
        np.testing.assert_allclose(flat[g[name + '.idx']], g[name + '.val'], rtol=0, atol=1e-4)
        assert abs(flat.astype(np.float64).sum() - float(g[name + '.sum'])) < 1e-3 * max(1.0, float(g[name + '.abssum']) * 1e-3)
    losses[0].backward()
    for k, p in m.named_parameters():
        gn = float(p.grad.double().pow(2).sum().sqrt())
        ref = float(g['gnorm.' + k])
        assert abs(gn - ref) <= 1e-5 + 2e-3 * ref, (k, gn, ref)
        gs = float(p.grad.double().sum())
        assert abs(gs - float(g['gsum.' + k])) <= 1e-4 + 2e-3 * ref * np.sqrt(p.numel()), (k, gs)


def test_bf16_path_tracks_fp32_loss():
    """the benched dtype against the reference-generated golden (full geometry, B = 16).  Measured with scripts/bf16_parity.py
    (profiles/r03_bf16_parity.jsonl): max |d loss| 2.1e-5 over the 11 losses, global gradient norm 6.2e-5 relative, worst
    per-tensor gradient norm 6.1e-4 relative -- the bf16 path (bf16 MFMA operands AND bf16-stored saved tensors) meets the
    north-star 1e-4 loss bar on this fixture; bounds = 3x the measured values (the reductions are ordered: the values reproduce)"""
    g = load_npz('full_tf1_b16.npz')
    x, c, pr = synth_batch(int(g['B']), int(g['data_seed']))
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    outs, losses = _run(m, g, x, c, pr)
    got = np.array([l.item() for l in losses])
    np.testing.assert_allclose(got, g['losses'], rtol=0, atol=1e-4)       # the north-star bar
    np.testing.assert_allclose(got, g['losses'], rtol=0, atol=6e-5)       # 3x measured
    losses[0].backward()
    tot = sum(float(p.grad.double().pow(2).sum()) for p in m.parameters()) ** 0.5
    ref = sum(float(g['gnorm.' + k]) ** 2 for k, _ in m.named_parameters()) ** 0.5
    assert abs(tot - ref) < 2e-4 * ref
    for k, p in m.named_parameters():
        gn, r = float(p.grad.double().pow(2).sum().sqrt()), float(g['gnorm.' + k])
        assert abs(gn - r) <= 1e-7 + 2e-3 * r, (k, gn, r)


def test_decoder_tf_composite_entry_point_equals_launch_by_launch_and_reference():
    """ptv_decoder_tf_fwd and ptv_chord_decoder_fwd (csrc/composite.hip: the two teacher-forced decoder forwards as ONE C call each --
    launch sequence, persistent turn and shape decisions in C++) against (a) the same launches sequenced from Python, bit for bit (losses and every gradient), and (b) the
    reference's golden losses at full geometry.  bf16 with the optimiser's bf16 weight shadows, which is what the train step runs."""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    g = load_npz('full_tf1_b4.npz')
    x, c, pr = synth_batch(int(g['B']), int(g['data_seed']))
    res = {}
    for comp in (True, False):
        m = M.DisentangleVAE.init_model(torch.device(DEV))
        m.load_state_dict(full_params())
        m.to(DEV).set_precision('bf16')
        opt = FusedClipAdam(m.parameters(), lr=1e-3)
        old, F_.DEC_COMPOSITE, F_.CHD_COMPOSITE, F_.CHD_BWD_COMPOSITE = (F_.DEC_COMPOSITE, F_.CHD_COMPOSITE, F_.CHD_BWD_COMPOSITE), comp, comp, comp
        calls, chd_calls, bwd_calls = F_._DTF.get('calls', 0), F_._DTF.get('chd_calls', 0), F_._CDB.get('calls', 0)
        try:
            opt.zero_grad()
            outs, losses = _run(m, g, x, c, pr)
            losses[0].backward()
        finally:
            F_.DEC_COMPOSITE, F_.CHD_COMPOSITE, F_.CHD_BWD_COMPOSITE = old
        assert (F_._DTF.get('calls', 0) > calls) == comp                    # the composites really ran (or really did not)
        assert (F_._DTF.get('chd_calls', 0) > chd_calls) == comp
        assert (F_._CDB.get('calls', 0) > bwd_calls) == comp                # ... ptv_chord_decoder_bwd too
        res[comp] = (np.array([l.item() for l in losses]), {k: p.grad.detach().clone() for k, p in m.named_parameters()},
                     outs[0].detach().clone(), outs[1].detach().clone())
        F_.persist_check()
    np.testing.assert_allclose(res[True][0], g['losses'], rtol=0, atol=3e-4)   # (bf16 weight shadows + bf16-stored activations: the bf16 bound of test_gpu_model_wide)
    assert np.array_equal(res[True][0], res[False][0])
    assert torch.equal(res[True][2], res[False][2]) and torch.equal(res[True][3], res[False][3])
    for k in res[True][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k


@pytest.mark.parametrize('prec,B,via_loss', [('bf16', 512, True), ('bf16', 64, True), ('bf16', 24, True), ('bf16', 16, False), ('fp32', 8, True)])
def test_backward_composites_equal_python_sequencing(prec, B, via_loss, monkeypatch):
    """ptv_chord_decoder_bwd, ptv_decoder_tf_bwd and ptv_bigru_final_bwd (one C call each: the chord decoder's / the PianoTree decoder's / an
    encoder bi-GRU's whole backward -- chain,
    the forks of the weight-gradient groups onto the sibling stream, the persistent launches with their event turn) against the launch
    sequences of ChordDecoderTFFn.backward / decoder_bwd_core: every gradient of the step bit for bit.  bf16 at B = 512 (persistent BPTTs,
    split-K teams) and small batches, through loss() (the decoder stops at the last live note step) and through run() + loss_function()
    (all 15 steps); fp32 (the chord decoder's composite takes it, the PianoTree decoder's declines: still the Python path)"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, 77))
    monkeypatch.setattr(F_, 'SORT_DEC_ROWS', False)             # (length-sorted rows exist behind the C ABI only: the Python sequencing is the (t, b) order)
    res = {}
    for comp in (True, False):
        m = M.DisentangleVAE.init_model(torch.device(DEV))
        m.load_state_dict(full_params())
        m.to(DEV).set_precision(prec)
        m.use_philox(11, 0)
        opt = FusedClipAdam(m.parameters(), lr=1e-3)        # (the bf16 weight shadows the composites read are the optimiser's)
        old, F_.CHD_BWD_COMPOSITE, F_.DEC_BWD_COMPOSITE, F_.BIGRU_BWD_COMPOSITE = (F_.CHD_BWD_COMPOSITE, F_.DEC_BWD_COMPOSITE, F_.BIGRU_BWD_COMPOSITE), comp, comp, comp
        old_l, F_.LOSS_COMPOSITE = F_.LOSS_COMPOSITE, comp
        n6, n7 = F_._VL.get('calls', 0), F_._VL.get('bwd_calls', 0)
        n0, n1, n2, n3 = F_._CDB.get('calls', 0), F_._DTB.get('calls', 0), F_._BGB.get('calls', 0), F_._BGF.get('calls', 0)
        n4, n5 = F_._BRF.get('calls', 0), F_._BRB.get('calls', 0)
        try:
            opt.zero_grad()
            if via_loss:
                losses = m.loss(x, c, pr, 1., 1., 1., 0.1, [1, 0.5])
            else:
                losses = m.loss_function(x, c, *m.run(x, c, pr, 1., 1., 1.), 0.1, [1, 0.5])
            losses[0].backward()
            torch.cuda.synchronize()
        finally:
            F_.CHD_BWD_COMPOSITE, F_.DEC_BWD_COMPOSITE, F_.BIGRU_BWD_COMPOSITE = old
            F_.LOSS_COMPOSITE = old_l
        assert (F_._VL.get('calls', 0) - n6) == int(comp) and (F_._VL.get('bwd_calls', 0) - n7) == int(comp)      # the loss node, both ways
        assert (F_._CDB.get('calls', 0) > n0) == comp
        assert (F_._DTB.get('calls', 0) > n1) == (comp and prec == 'bf16')
        assert (F_._BGB.get('calls', 0) - n2) == (2 if (comp and prec == 'bf16' and 8 * B >= 512) else 0)      # the two encoders' bi-GRUs
        # ... and their forwards (the chord encoder's 36-wide input weight has no bf16 shadow: its fp32 master is the operand)
        assert (F_._BGF.get('calls', 0) - n3) == (2 if (comp and prec == 'bf16') else 0)
        # ... and the note-summary bi-GRU (row kernels), forward and backward
        rows_branch = prec == 'bf16' and F_.row_gru_ok(1, 128, 128, 32 * B, torch.bfloat16)        # (many rows: the row kernels run it)
        assert (F_._BRF.get('calls', 0) - n4) == (1 if (comp and rows_branch) else 0)
        assert (F_._BRB.get('calls', 0) - n5) == (1 if (comp and rows_branch) else 0)
        res[comp] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        res[comp]['_losses'] = torch.stack([l.detach() for l in losses]).clone()
        F_.persist_check()
    for k in res[True]:
        assert torch.isfinite(res[True][k]).all(), k
        assert torch.equal(res[True][k], res[False][k]), k


def test_fresh_batch_vs_oracle_with_weighted_outputs():
    """Independent check on inputs no fixture holds: oracle on CPU vs HIP path, all 11 outputs given
    non-trivial upstream gradients (exercises the loss backward's scale mixing)."""
    params = reduced_params(requires_grad=True)
    x, c, pr = synth_batch(5, 4242)
    gen = torch.Generator().manual_seed(99)
    eps = {'eps_chd': torch.randn(5, 16, generator=gen).numpy(), 'eps_rhy': torch.randn(5, 16, generator=gen).numpy()}
    wts = torch.rand(11, generator=gen)
    o = Oracle(params)
    lo = o.loss(torch.from_numpy(x), torch.from_numpy(c), torch.from_numpy(pr), 1., 1., 1., 0.3, [0.7, 0.4],
                torch.from_numpy(eps['eps_chd']), torch.from_numpy(eps['eps_rhy']), lambda: 0.0)
    (torch.stack(lo) * wts).sum().backward()
    m = build_reduced(DEV)
    m.load_state_dict({k: v.detach() for k, v in params.items()})
    m.to(DEV)
    m.eps_source = _eps_source(eps)
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    lg = m('train', xt, ct, prt, tfr1=1., tfr2=1., tfr3=1., beta=0.3, weights=[0.7, 0.4])
    np.testing.assert_allclose(np.array([l.item() for l in lg]), np.array([l.item() for l in lo]), rtol=0, atol=1e-5)
    (torch.stack(lg) * wts.to(DEV)).sum().backward()
    for k, p in m.named_parameters():
        ref = params[k].grad.numpy()
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=0, atol=2e-6 + 2e-4 * np.abs(ref).max(), err_msg=k)


def test_three_step_training_trace_with_fused_clip_adam():
    """zero_grad -> loss -> backward -> clip_grad_norm_(1) + Adam (fused HIP) -> MinExponentialLR, 3 steps,
    against the trace recorded from the reference (torch.optim.Adam + clip_grad_norm_)."""
    from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus import MinExponentialLR
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    g = load_npz('reduced_train3.npz')
    m = build_reduced(DEV).to(DEV)
    opt = FusedClipAdam(m.parameters(), lr=1e-3)
    sched = MinExponentialLR(opt, gamma=0.9999, minimum=1e-5)
    for step in range(3):
        x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(3, 200 + step))
        m.eps_source = lambda name, shape, device, s=step: torch.from_numpy(g['eps_%s.%d' % (name, s)]).to(device)
        opt.zero_grad()
        losses = m('train', x, c, pr, tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
        losses[0].backward()
        assert opt.arena.holds_all_grads()                     # every gradient was produced in the flat bucket
        opt.clip_and_step(1)
        sched.step()
        np.testing.assert_allclose(np.array([l.item() for l in losses]), g['losses.%d' % step], rtol=0, atol=1e-4)
        assert abs(opt.grad_norm().item() - float(g['gnorm.%d' % step])) < 1e-3 * float(g['gnorm.%d' % step])
        assert abs(opt.param_groups[0]['lr'] - float(g['lr.%d' % step])) < 1e-12
        psum = np.array([p.detach().double().sum().item() for p in m.parameters()])
        pabs = np.array([p.detach().double().abs().sum().item() for p in m.parameters()])
        np.testing.assert_allclose(psum, g['psum.%d' % step], rtol=0, atol=5e-4)
        np.testing.assert_allclose(pabs, g['pabs.%d' % step], rtol=1e-4, atol=1e-4)


def test_fused_optimizer_matches_torch_adam_on_same_grads():
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ((37, 5), (130,), (8, 3, 4, 12), (1,))]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref = torch.optim.Adam(qs, lr=1e-3)
    opt = FusedClipAdam(ps, lr=1e-3)
    for it in range(4):
        grads = [torch.randn_like(p) * (3.0 if it % 2 == 0 else 0.01) for p in ps]
        for p, q, gr in zip(ps, qs, grads):
            p.grad = gr.clone()
            q.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(qs, 1.0)
        ref.step()
        opt.clip_and_step(1.0)
        for p, q in zip(ps, qs):
            assert (p - q).abs().max() < 2e-6


def test_trainer_surface_runs_one_epoch_and_saves_checkpoints(tmp_path, monkeypatch):
    """TrainingVAE.run(): train + eval + the three checkpoint flavours (module.py:195-213), one D2H per step."""
    from polyphonic_chord_texture_disentanglement_amd.amc_dl import torch_plus as tp
    from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus.train_utils import kl_anealing
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import MusicDataLoaders, TrainingVAE
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    monkeypatch.chdir(tmp_path)
    m = build_reduced(DEV).to(DEV)
    loaders = MusicDataLoaders.get_loaders(3345, bs_train=4, bs_val=4, n_train_batch=3, n_val_batch=1)
    pm = tp.LogPathManager(None)
    opt = FusedClipAdam(m.parameters(), lr=1e-3)
    osch = tp.OptimizerScheduler(opt, tp.MinExponentialLR(opt, gamma=0.9999, minimum=1e-5), 1)
    names = M.LOSS_NAMES
    sw = tp.SummaryWriters(names, {'loss': None}, pm.writer_path)
    ps = tp.ParameterScheduler(tfr1=tp.ConstantScheduler(1.), tfr2=tp.ConstantScheduler(1.), tfr3=tp.ConstantScheduler(1.),
                               beta=tp.TeacherForcingScheduler(0.1, 0., f=kl_anealing), weights=tp.ConstantScheduler([1, 0.5]))
    tr = TrainingVAE(torch.device(DEV), m, False, pm, loaders, sw, osch, ps, 1)
    before = [p.detach().clone() for p in m.parameters()]
    tr.run()
    assert tr.train_step == 3 and tr.val_step == 1 and tr.epoch == 1
    assert any((a - b.detach()).abs().max() > 0 for a, b in zip(before, m.parameters()))
    for kind in ('epoch', 'valid', 'final'):
        sd = torch.load(str(tmp_path / pm.model_path / ('disvae_%s.pt' % kind)), map_location='cpu')
        assert list(sd.keys()) == list(m.state_dict().keys())
    m2 = build_reduced(DEV)
    m2.load_model(pm.final_model_path('disvae'))
    x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(2, 5))
    # positional reference-style call, and the reference trainer's 4-tensor call, both work
    l1 = m2.loss(x, c, pr, 1., 1., 1., 0.1, (1, 0.5))
    m2.eps_source = m.eps_source = lambda name, shape, device: torch.zeros(shape, device=device)
    l2 = m2('train', x, c, pr, torch.zeros(2, 1, device=DEV), tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
    l3 = m('train', x, c, pr, tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
    assert len(l1) == 11 and abs(l2[0].item() - l3[0].item()) < 1e-5      # same weights; block-sum order differs


def _coin_hook(monkeypatch, coins):
    import random as _r
    seq = CoinList(coins)
    monkeypatch.setattr(_r, 'random', seq)
    return seq


@pytest.mark.parametrize('case', ['tf0', 'tfh'])
def test_reduced_step_loop_vs_reference_golden(case, monkeypatch):
    """Free-running (tfr=0) and scheduled-sampling (tfr=0.5, recorded coin flips) training step: losses,
    logits and every gradient against the reference, with the reference's coin stream replayed through
    random.random (487 draws in the reference's order)."""
    g = load_npz('reduced_%s.npz' % case)
    m = build_reduced(DEV).to(DEV)
    seq = _coin_hook(monkeypatch, g['coins'])
    m.eps_source = _eps_source(g)
    m.zero_grad()
    xt, ct, prt = (torch.from_numpy(g[k]).to(DEV) for k in ('x', 'c', 'pr_mat'))
    tfr = [float(v) for v in g['tfr']]
    outs = m.run(xt, ct, prt, *tfr)
    assert seq.i == 487
    losses = m.loss_function(xt, ct, *outs, float(g['beta']), [float(w) for w in g['weights']])
    # argmax decisions must match the reference's (margins in this fixture are >> fp32 noise)
    est = torch.cat([outs[0].max(-1)[1].unsqueeze(-1), outs[1].max(-1)[1]], -1).cpu().numpy()
    ref_est = np.concatenate([g['pitch_outs'].argmax(-1)[..., None], g['dur_outs'].argmax(-1)], -1)
    assert (est == ref_est).mean() > 0.999
    np.testing.assert_allclose(np.array([l.item() for l in losses]), g['losses'], rtol=0, atol=1e-4)
    for name, t in (('pitch_outs', outs[0]), ('dur_outs', outs[1]), ('recon_root', outs[4]), ('recon_chroma', outs[5]),
                    ('recon_bass', outs[6])):
        np.testing.assert_allclose(t.detach().cpu().numpy(), g[name], rtol=0, atol=5e-5, err_msg=name)
    losses[0].backward()
    for k, p in m.named_parameters():
        ref = g['grad.' + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=0, atol=2e-6 + 3e-4 * np.abs(ref).max(), err_msg=k)


def test_reduced_inference_decode_vs_reference_golden():
    g = load_npz('reduced_infer.npz')
    m = build_reduced(DEV).to(DEV)
    est_x = m.inference_decode(torch.from_numpy(g['z_chd']).to(DEV), torch.from_numpy(g['z_rhy']).to(DEV))
    assert est_x.shape == (3, 32, 15, 6) and est_x.dtype == np.int64
    assert (est_x == g['est_x']).mean() >= 0.999


def test_full_free_running_vs_reference_golden(monkeypatch):
    g = load_npz('full_tf0_b4.npz')
    x, c, pr = synth_batch(int(g['B']), int(g['data_seed']))
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV)
    _coin_hook(monkeypatch, g['coins'])
    m.eps_source = _eps_source(g)
    m.zero_grad()
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    outs = m.run(xt, ct, prt, 0., 0., 0.)
    losses = m.loss_function(xt, ct, *outs, float(g['beta']), [float(w) for w in g['weights']])
    got = np.array([l.item() for l in losses])
    # untrained weights give near-tie pitch argmaxes: a flipped decision changes the tail of
    # that sample's trajectory, so the free-running gate is looser than the teacher-forced one
    np.testing.assert_allclose(got, g['losses'], rtol=0, atol=5e-3)
    flat = outs[0].detach().contiguous().cpu().numpy().reshape(-1)
    close = np.abs(flat[g['pitch_outs.idx']] - g['pitch_outs.val']) < 1e-3
    assert close.mean() > 0.9
    losses[0].backward()
    tot = sum(float(p.grad.double().pow(2).sum()) for p in m.parameters()) ** 0.5
    ref = sum(float(g['gnorm.' + k]) ** 2 for k, _ in m.named_parameters()) ** 0.5
    assert abs(tot - ref) < 0.02 * ref


def test_graph_replayed_decode_equals_eager():
    g = load_npz('reduced_infer.npz')
    m = build_reduced(DEV).to(DEV)
    zc, zr = torch.from_numpy(g['z_chd']).to(DEV), torch.from_numpy(g['z_rhy']).to(DEV)
    eager = m.inference_decode(zc, zr)
    m.decoder.use_graph = True
    first = m.inference_decode(zc, zr)                 # captures
    again = m.inference_decode(zc.flip(0), zr.flip(0))  # replays with new latent codes
    assert np.array_equal(eager, first)
    assert np.array_equal(eager[::-1], again)


@pytest.mark.parametrize('B', [4, 3])          # 480*B rows: whole 64-row tiles / a ragged last tile
def test_fused_duration_gru_kernel_equals_per_step_kernels(B):
    """csrc/dur.hip + dur_bwd.hip (one kernel each for the 5 duration steps, forward and backward) vs the per-step
    kernels, bf16 precision, full config."""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    g = dict(load_npz('full_tf1_b4.npz'))
    x, c, pr = synth_batch(B, int(g['data_seed']))
    for k in [k for k in g if k.startswith('eps_')]:
        g[k] = g[k][:B]
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    res = {}
    for fused in (True, False):
        F_.FUSED_DUR = fused
        try:
            outs, losses = _run(m, g, x, c, pr)
            losses[0].backward()
            dec = m.decoder
            grads = {n: p.grad.clone() for n, p in dec.named_parameters()
                     if n.startswith(('dec_dur_gru.', 'dur_sos_token', 'dur_out_linear.', 'dur_hid_linear.', 'pitch_out_linear.'))}
            res[fused] = (outs[1].detach().clone(), dec.last_dur_idx.clone(), np.array([l.item() for l in losses]), grads)
            m.zero_grad()
        finally:
            F_.FUSED_DUR = True
    d_f, i_f, l_f, g_f = res[True]
    d_s, i_s, l_s, g_s = res[False]
    assert (i_f == i_s).float().mean() > 0.999                       # same argmax feedback decisions
    assert (d_f - d_s).abs().max() < 2e-2                            # bf16 operand rounding only
    np.testing.assert_allclose(l_f, l_s, rtol=0, atol=2e-3)
    # the fused backward (csrc/dur_bwd.hip: in-kernel parameter-gradient accumulation) against the per-step BPTT
    # kernels + split-K products: every duration-GRU parameter and what sits upstream of dh0
    assert len(g_f) >= 10
    for n in g_s:
        assert (g_f[n] - g_s[n]).abs().max() < 0.05 * g_s[n].abs().max() + 1e-6, n


def test_fused_duration_gru_in_the_step_loop(monkeypatch):
    """free-running (tfr=0) bf16 forward/backward with the fused duration kernel on [B]-row windows vs per-step kernels"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    g = load_npz('full_tf0_b4.npz')
    x, c, pr = synth_batch(int(g['B']), int(g['data_seed']))
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    res = {}
    for fused in (True, False):
        F_.FUSED_DUR = fused
        try:
            m.eps_source = _eps_source(g)
            m.zero_grad()
            outs = m.run(xt, ct, prt, 0., 0., 0.)
            losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
            losses[0].backward()
            res[fused] = (m.decoder.last_xhat.clone(), np.array([l.item() for l in losses]),
                          m.decoder.dec_dur_gru.weight_hh_l0.grad.clone())
        finally:
            F_.FUSED_DUR = True
    assert (res[True][0] == res[False][0]).float().mean() > 0.995          # same predicted grid
    np.testing.assert_allclose(res[True][1], res[False][1], rtol=0, atol=5e-3)
    assert (res[True][2] - res[False][2]).abs().max() < 0.1 * res[False][2].abs().max()


def test_graphed_training_forward_twice_before_backward_keeps_the_first_graph_intact():
    """a second forward while the first replay's backward is still pending must not overwrite the captured buffers: it runs
    eagerly (graphed_decoder_step), and the first backward gives the gradients of the first batch; returned outputs are copies"""
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    g = load_npz('full_tf0_b4.npz')
    batches = [tuple(torch.from_numpy(a).to(DEV) for a in synth_batch(int(g['B']), int(g['data_seed']) + i)) for i in range(2)]

    def fwd(b):
        m.eps_source = _eps_source(g)
        outs = m.run(*b, 0., 0., 0.)
        return outs, m.loss_function(b[0], b[1], *outs, 0.1, [1, 0.5])[0]

    m.decoder.use_graph = False
    m.zero_grad()
    fwd(batches[0])[1].backward()
    want = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.decoder.use_graph = True
    m.zero_grad()
    fwd(batches[0])[1].backward()                               # capture + first replay, backward done
    m.zero_grad()
    outs_a, loss_a = fwd(batches[0])                            # replay, backward pending
    pitch_a = outs_a[0].clone()
    ent = next(iter(m.decoder._train_graphs.values()))
    assert ent.busy()
    outs_b, loss_b = fwd(batches[1])                            # must not touch the captured buffers
    assert torch.equal(outs_a[0], pitch_a)
    loss_a.backward()
    assert not ent.busy()
    torch.cuda.synchronize()
    m.decoder.use_graph = False
    for n, w in want.items():
        got = dict(m.named_parameters())[n].grad
        assert (got - w).abs().max() <= 0.05 * w.abs().max() + 1e-6, n
    del outs_b, loss_b


def test_graph_captured_free_running_training_step_equals_eager():
    """tfr = 0 training step with the decoder forward replayed from a captured hipGraph (use_graph) vs the eager step loop:
    same losses and gradients, on the capture call and on a replay with different data"""
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    g = load_npz('full_tf0_b4.npz')
    res = {}
    for graph in (False, True):
        m.decoder.use_graph = graph
        out = []
        for seed in (int(g['data_seed']), int(g['data_seed']) + 1, int(g['data_seed'])):
            x, c, pr = synth_batch(int(g['B']), seed)
            xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
            m.eps_source = _eps_source(g)
            m.zero_grad()
            outs = m.run(xt, ct, prt, 0., 0., 0.)
            losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
            losses[0].backward()
            torch.cuda.synchronize()
            out.append((np.array([l.item() for l in losses]), m.decoder.last_xhat.clone(),
                        {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
        res[graph] = out
    m.decoder.use_graph = False
    assert len(m.decoder._train_graphs) == 1
    for (l0, x0, g0), (l1, x1, g1) in zip(res[False], res[True]):
        np.testing.assert_allclose(l1, l0, rtol=0, atol=5e-3)
        assert (x0 == x1).float().mean() > 0.995
        for n in g0:
            assert (g1[n] - g0[n]).abs().max() <= 0.05 * g0[n].abs().max() + 1e-6, n


# ---------------------------------------------------------------------------------------------
# replay mode: free-running outputs depend on discrete argmaxes, and untrained weights give
# near-ties (pitch top1-top2 margins down to 3e-6 in this fixture) that fp32 re-association can flip.  The gate is
# therefore (i) with the reference's own decisions forced -> logits / losses / gradients at the teacher-forced tolerance,
# (ii) un-forced -> >= 99.9 % of the decisions agree and every disagreement sits at a margin < 1e-4.
# ---------------------------------------------------------------------------------------------
def _force_from_trace(tr, B):
    pitch = torch.from_numpy(tr['pitch_inds'].astype(np.int32)).permute(2, 1, 0).reshape(15, 32 * B).contiguous().to(DEV)
    dur = torch.from_numpy(tr['dur_inds'].astype(np.int32)).permute(3, 2, 1, 0).reshape(5, 15 * 32 * B).contiguous().to(DEV)
    return {'pitch': pitch, 'dur': dur}


def test_full_free_running_replay_mode_vs_reference_golden(monkeypatch):
    g, tr = load_npz('full_tf0_b4.npz'), load_npz('full_tf0_b4_trace.npz')
    B = int(g['B'])
    x, c, pr = synth_batch(B, int(g['data_seed']))
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV)
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    # (i) forced
    _coin_hook(monkeypatch, g['coins'])
    m.eps_source = _eps_source(g)
    m.decoder.force_trace = _force_from_trace(tr, B)
    m.zero_grad()
    outs = m.run(xt, ct, prt, 0., 0., 0.)
    losses = m.loss_function(xt, ct, *outs, float(g['beta']), [float(w) for w in g['weights']])
    m.decoder.force_trace = None
    np.testing.assert_allclose(np.array([l.item() for l in losses]), g['losses'], rtol=0, atol=1e-4)
    flat = outs[0].detach().contiguous().cpu().numpy().reshape(-1)
    np.testing.assert_allclose(flat[g['pitch_outs.idx']], g['pitch_outs.val'], rtol=0, atol=1e-4)
    for name, t in (('recon_root', outs[4]), ('recon_chroma', outs[5]), ('recon_bass', outs[6])):
        np.testing.assert_allclose(t.detach().cpu().numpy(), tr[name], rtol=0, atol=1e-4, err_msg=name)
    losses[0].backward()
    for k, p in m.named_parameters():
        gn, ref = float(p.grad.double().pow(2).sum().sqrt()), float(g['gnorm.' + k])
        assert abs(gn - ref) <= 1e-5 + 2e-3 * ref, (k, gn, ref)
    # (ii) un-forced: decisions agree except at near-ties
    _coin_hook(monkeypatch, g['coins'])
    with torch.no_grad():
        outs = m.run(xt, ct, prt, 0., 0., 0.)
    pi = outs[0].max(-1)[1].cpu().numpy()
    di = outs[1].max(-1)[1].cpu().numpy()
    # a flipped pitch decision changes the rest of that time step's note sequence: compare decision by decision up to the
    # first flip of each (sample, step), which must itself be a near-tie
    first_bad = []
    agree = 0
    total = 0
    for b in range(B):
        for t in range(32):
            row_ok = True
            for n in range(15):
                same = pi[b, t, n] == tr['pitch_inds'][b, t, n] and (di[b, t, n] == tr['dur_inds'][b, t, n]).all()
                total += 1
                if row_ok and same:
                    agree += 1
                elif row_ok:
                    row_ok = False
                    first_bad.append(min(float(tr['pitch_margin'][b, t, n]), float(tr['dur_margin'][b, t, n].min())))
    assert all(mg < 1e-4 for mg in first_bad), first_bad
    assert (pi == tr['pitch_inds']).mean() >= 0.999 or len(first_bad) <= 2, ((pi == tr['pitch_inds']).mean(), first_bad)


def test_full_dims_inference_decode_vs_reference_golden():
    """configs[3] workload at full dimensions (B=4 here): est_x of inference_decode, forced and un-forced"""
    g = load_npz('full_infer_b4.npz')
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV)
    zc, zr = torch.from_numpy(g['z_chd']).to(DEV), torch.from_numpy(g['z_rhy']).to(DEV)
    est = m.inference_decode(zc, zr)
    assert est.shape == (4, 32, 15, 6) and est.dtype == np.int64
    ref = g['est_x']
    margin = np.minimum(g['pitch_margin'], g['dur_margin'].min(-1))
    bad = (est != ref).any(-1)
    # every (sample, step) whose note sequence differs must contain a near-tie decision at or before the first difference
    for b, t in zip(*np.nonzero(bad.any(-1))):
        n0 = int(np.argmax(bad[b, t]))
        assert margin[b, t, :n0 + 1].min() < 1e-4, (b, t, n0, margin[b, t, :n0 + 1])
    assert (est == ref).mean() >= 0.99
    # forced: the logits of the replayed trajectory match at 1e-4
    B = 4
    m.decoder.force_trace = {'pitch': torch.from_numpy(ref[..., 0].astype(np.int32)).permute(2, 1, 0).reshape(15, 32 * B).contiguous().to(DEV),
                             'dur': torch.from_numpy(ref[..., 1:].astype(np.int32)).permute(3, 2, 1, 0).reshape(5, 15 * 32 * B).contiguous().to(DEV)}
    with torch.no_grad():
        po, do = m.decoder(torch.cat([zc, zr], -1), True, None, None, 0., 0.)
    m.decoder.force_trace = None
    flat = po.contiguous().cpu().numpy().reshape(-1)
    np.testing.assert_allclose(flat[g['pitch_outs.idx']], g['pitch_outs.val'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(do.cpu().numpy(), g['dur_outs'], rtol=0, atol=1e-4)


# ---------------------------------------------------------------------------------------------
# BASELINE configs[4]: fp32 encoders + bf16 MFMA decoders, the schedules of train.py:59-63 (free-running from step 2)
# ---------------------------------------------------------------------------------------------
def _train_steps(precisions, n_steps, B, schedule=True, seed0=50):
    import random
    from polyphonic_chord_texture_disentanglement_amd.amc_dl import torch_plus as tp
    from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus.train_utils import kl_anealing
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV)
    enc_p, dec_p = precisions
    m.chd_encoder.precision = m.rhy_encoder.precision = enc_p
    m.decoder.precision = m.chd_decoder.precision = dec_p
    opt = FusedClipAdam(m.parameters(), lr=1e-3)
    sched = tp.MinExponentialLR(opt, gamma=0.9999, minimum=1e-5)
    if schedule:                                                             # train.py:23-24,59-63
        ps = tp.ParameterScheduler(tfr1=tp.TeacherForcingScheduler(0.6, 0), tfr2=tp.TeacherForcingScheduler(0.5, 0),
                                   tfr3=tp.TeacherForcingScheduler(0.5, 0), beta=tp.TeacherForcingScheduler(0.1, 0., f=kl_anealing),
                                   weights=tp.ConstantScheduler([1, 0.5]))
    else:
        ps = tp.ParameterScheduler(tfr1=tp.ConstantScheduler(1.), tfr2=tp.ConstantScheduler(1.), tfr3=tp.ConstantScheduler(1.),
                                   beta=tp.ConstantScheduler(0.1), weights=tp.ConstantScheduler([1, 0.5]))
    m.use_philox(7, 0)
    random.seed(7)
    out = []
    for step in range(n_steps):
        x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, seed0 + step))
        opt.zero_grad()
        kw = ps.step()
        losses = m('train', x, c, pr, **kw)
        losses[0].backward()
        opt.clip_and_step(1.0)           # (scheduled-sampling steps accumulate note_embedding's gradient from two nodes: gathered)
        sched.step()
        out.append(np.array([l.item() for l in losses]))
    return np.array(out), kw


def test_config4_fp32_encoders_bf16_decoders_with_train_py_schedule():
    """4 optimisation steps with the published schedules: step 0 tfr ~0.6/0.5, step 1 ~0.004, steps 2-3 free-running;
    the mixed-precision run tracks the all-fp32 run at the loss-curve tolerance"""
    mixed, kw = _train_steps(('fp32', 'bf16'), 4, 8)
    ref, _ = _train_steps(('fp32', 'fp32'), 4, 8)
    assert kw['tfr1'] < 1e-6 and abs(kw['beta'] - 0.1) < 1e-6                       # free-running, beta saturated
    assert np.isfinite(mixed).all()
    np.testing.assert_allclose(mixed[:, 0], ref[:, 0], rtol=0, atol=5e-2)
    np.testing.assert_allclose(mixed[:, 1:], ref[:, 1:], rtol=0, atol=5e-2)
    assert ref[3, 0] < ref[0, 0] + 0.5                                              # and it trains


def test_bf16_loss_curve_tracks_fp32_over_20_steps():
    """the benched dtype against the parity dtype over a 20-step teacher-forced training run (same data, eps, optimiser):
    every loss of every step within 2e-2, no drift"""
    bf, _ = _train_steps(('bf16', 'bf16'), 20, 16, schedule=False)
    fp, _ = _train_steps(('fp32', 'fp32'), 20, 16, schedule=False)
    d = np.abs(bf - fp)
    assert d[:, 0].max() < 2e-2, d[:, 0]
    assert d.max() < 2e-2
    assert fp[-1, 0] < fp[0, 0] - 0.3                                               # 20 Adam steps visibly reduce the loss
    assert abs((bf[-1, 0] - bf[0, 0]) - (fp[-1, 0] - fp[0, 0])) < 1e-2


def test_bf16_training_horizon_200_steps_tracks_fp32():
    """round-5 review: at the benched batch the bf16 path's global gradient-norm error is 1e-3 -- does it show over a training HORIZON?
    200 teacher-forced optimiser steps at B = 64 from the same weights, data, Philox noise and optimiser in both dtypes.  Trajectories of
    two correct implementations separate (Adam's early +-lr steps amplify sign flips of near-zero gradients), so the test holds what
    matters for training: the bf16 run trains as far as the fp32 run does (loss decrease within 3 %), the per-step total loss stays within
    a band that does not widen over the run, and nothing is ever non-finite.  Measured on MI355X (profiles/r06_bf16_horizon.txt): mean
    |d loss| 0.016 over steps 0-99 and 0.012 over 100-199, max 0.054 / 0.044, loss decrease 5.153 (fp32) vs 5.149 (bf16); bounds = 3x measured."""
    bf, _ = _train_steps(('bf16', 'bf16'), 200, 64, schedule=False)
    fp, _ = _train_steps(('fp32', 'fp32'), 200, 64, schedule=False)
    assert np.isfinite(bf).all() and np.isfinite(fp).all()
    d = np.abs(bf[:, 0] - fp[:, 0])
    import os
    rep = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(rep):
        with open(os.path.join(rep, 'bf16_horizon.txt'), 'w') as f:
            f.write('bf16 vs fp32, 200 teacher-forced steps, B = 64, full geometry\n')
            f.write('step  loss_fp32  loss_bf16  |d|\n')
            for i in list(range(0, 200, 10)) + [199]:
                f.write('%4d  %9.4f  %9.4f  %.4f\n' % (i, fp[i, 0], bf[i, 0], d[i]))
            f.write('mean |d| steps 0-99: %.4f   100-199: %.4f   max 0-99: %.4f   100-199: %.4f\n'
                    % (d[:100].mean(), d[100:].mean(), d[:100].max(), d[100:].max()))
            f.write('decrease fp32 %.4f  bf16 %.4f\n' % (fp[0, 0] - fp[-10:, 0].mean(), bf[0, 0] - bf[-10:, 0].mean()))
    dec_fp, dec_bf = fp[0, 0] - fp[-10:, 0].mean(), bf[0, 0] - bf[-10:, 0].mean()
    assert dec_fp > 1.0                                                             # 200 Adam steps train visibly
    assert abs(dec_bf - dec_fp) < 0.03 * dec_fp + 0.05
    assert d[100:].mean() < 0.04 and d.max() < 0.17
    assert d[100:].mean() < 3 * d[:100].mean() + 0.01                               # the band does not widen over the horizon


def test_full_batch_512_bf16_step_on_the_benched_code_paths():
    """B = 512, bf16: the kernel variants bench.py runs (128x128 BPTT tile, grid-stride duration kernels, 16-byte CE / embed
    kernels) produce the fp32 path's losses within the bf16 tolerance and every gradient lands in the flat arena"""
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    res = {}
    for prec in ('fp32', 'bf16'):
        m = M.DisentangleVAE.init_model(torch.device(DEV))
        m.load_state_dict(full_params())
        m.to(DEV).set_precision(prec)
        opt = FusedClipAdam(m.parameters(), lr=1e-3)
        m.use_philox(7, 0)
        x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(512, 4321))
        opt.zero_grad()
        losses = m('train', x, c, pr, tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
        losses[0].backward()
        assert opt.arena.holds_all_grads()
        res[prec] = (np.array([l.item() for l in losses]), float(opt.arena.flat.double().pow(2).sum().sqrt()))
        del m, opt
        torch.cuda.empty_cache()
    np.testing.assert_allclose(res['bf16'][0], res['fp32'][0], rtol=0, atol=2e-2)
    assert abs(res['bf16'][1] - res['fp32'][1]) < 0.03 * res['fp32'][1]


# ---------------------------------------------------------------------------------------------
# csrc/freerun.hip: the step loop as row-partitioned persistent kernels (one launch per time step for all 15 note steps of a
# 16-sample panel + one for the re-summarisation) against the per-step kernels it replaces, bf16 precision, full config
# ---------------------------------------------------------------------------------------------
def _free_run(m, g, B, seed, persist, tfr, force=None, coins=None, monkeypatch=None):
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    x, c, pr = synth_batch(B, seed)
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    gen = torch.Generator().manual_seed(5)
    eps = {'chd': torch.randn(B, 256, generator=gen), 'rhy': torch.randn(B, 256, generator=gen)}
    m.eps_source = lambda name, shape, device: eps[name].to(device)
    old = FF_.FREE_PERSIST
    FF_.FREE_PERSIST = persist
    try:
        import random
        random.seed(3)
        m.decoder.force_trace = force
        m.zero_grad()
        outs = m.run(xt, ct, prt, *tfr)
        losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
        losses[0].backward()
        torch.cuda.synchronize()
    finally:
        FF_.FREE_PERSIST = old
        m.decoder.force_trace = None
    return (outs[0].detach().clone(), outs[1].detach().clone(), m.decoder.last_xhat.clone(), m.decoder.last_dur_idx.clone(),
            np.array([l.item() for l in losses]), {n: p.grad.clone() for n, p in m.named_parameters()})


@pytest.mark.parametrize('B,tfr', [(4, (0., 0., 0.)), (19, (0., 0., 0.)), (8, (0.5, 0.5, 0.5))])
def test_persistent_step_loop_kernels_equal_the_per_step_kernels(B, tfr):
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    ref = _free_run(m, None, B, 77, False, tfr)
    # replay the per-step path's decisions: every tensor must agree to bf16 rounding of the operands
    R = 32 * B
    xh = ref[2]                                                  # [B,32,16,6]
    force = {'pitch': xh[:, :, 1:, 0].permute(2, 1, 0).reshape(15, R).int().contiguous(),
             'dur': ref[3].clone()}
    a = _free_run(m, None, B, 77, True, tfr, force=force)
    b = _free_run(m, None, B, 77, False, tfr, force=force)
    assert (a[0] - b[0]).abs().max() < 3e-2 and (a[1] - b[1]).abs().max() < 3e-2          # logits
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])                             # forced decisions, grid, lengths
    np.testing.assert_allclose(a[4], b[4], rtol=0, atol=5e-3)
    for n in b[5]:
        assert (a[5][n] - b[5][n]).abs().max() <= 0.05 * b[5][n].abs().max() + 1e-6, n
    # un-forced: same trajectory except at near-ties
    u = _free_run(m, None, B, 77, True, tfr)
    assert (u[2] == ref[2]).float().mean() > 0.99
    np.testing.assert_allclose(u[4], ref[4], rtol=0, atol=2e-2)


def test_persistent_step_loop_inference_decode_and_graph():
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    g = load_npz('full_infer_b4.npz')
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    zc, zr = torch.from_numpy(g['z_chd']).to(DEV), torch.from_numpy(g['z_rhy']).to(DEV)
    est = {}
    for persist in (True, False):
        FF_.FREE_PERSIST = persist
        try:
            est[persist] = m.inference_decode(zc, zr)
        finally:
            FF_.FREE_PERSIST = True
    # un-forced bf16 trajectories of an UNTRAINED model: this fixture has pitch margins down to 1e-7, and one flipped near-tie
    # changes the rest of that time step -- both bf16 paths agree with each other and with the fp32 reference to a few percent
    # of the cells (the forced comparison of the test above is the exact one)
    assert (est[True] == est[False]).mean() > 0.97
    assert (est[True] == g['est_x']).mean() > 0.96 and (est[False] == g['est_x']).mean() > 0.96
    m.decoder.use_graph = True
    first = m.inference_decode(zc, zr)
    again = m.inference_decode(zc.flip(0), zr.flip(0))
    m.decoder.use_graph = False
    # (split-K products accumulate with atomics: run-to-run rounding differs in the last bit, which near-ties amplify)
    assert (first == est[True]).mean() > 0.97 and (again == est[True][::-1]).mean() > 0.97


def test_free_running_training_batched_recompute_equals_streamed_states(monkeypatch):
    """tfr = 0 training step, full geometry: the default forward stores only decisions / logits / fed tokens in the step loop and
    recomputes states and gates for the backward with the batched kernels (functional_free.FREE_REPLAY); against the variant whose
    16-row panels stream states and gates out note step by note step: identical losses and decisions (same forward), gradients
    equal to bf16 rounding of the recomputed activations"""
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    g = load_npz('full_tf0_b4.npz')
    B = 32
    x, c, pr = synth_batch(B, int(g['data_seed']) + 5)
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    eps = {n: torch.randn(B, 256, generator=torch.Generator().manual_seed(i)).to(DEV) for i, n in enumerate(('chd', 'rhy'))}
    res = {}
    for replay in (False, True):
        monkeypatch.setattr(FF_, 'FREE_REPLAY', replay)
        m.eps_source = lambda name, shape, device: eps[name]
        m.zero_grad()
        outs = m.run(xt, ct, prt, 0., 0., 0.)
        losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
        losses[0].backward()
        torch.cuda.synchronize()
        res[replay] = (np.array([l.item() for l in losses]), m.decoder.last_xhat.clone(),
                       {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    (l0, x0, g0), (l1, x1, g1) = res[False], res[True]
    np.testing.assert_allclose(l1, l0, rtol=0, atol=5e-3)
    assert (x0 == x1).float().mean() > 0.995
    assert set(g0) == set(g1)
    for n in g0:
        assert (g1[n] - g0[n]).abs().max() <= 0.04 * g0[n].abs().max() + 1e-6, n


@pytest.mark.parametrize('B,tfr,bwd_call', [(8, 0.5, None), (8, 0.0, None), (40, 0.0, None), (24, 0.5, None), (512, 0.0, True), (512, 0.5, True)])
def test_decoder_free_composite_entry_point_equals_python_sequencing(B, tfr, bwd_call, monkeypatch):
    """ptv_decoder_free_fwd / ptv_decoder_free_bwd (csrc/composite.hip; SURVEY 8b's decoder_free_{fwd,bwd}): the free-running /
    scheduled-sampling decoder node as ONE C call per direction.  Forward --
    prologue, the 32-step loop (time-GRU cell, note loop, re-summarisation or the ground-truth summary by the time coins), the batched
    recompute -- as ONE C call makes the same launches as functional_free.DecoderStepFn's own sequencing: losses, the predicted grid and
    every gradient bit-identical; a ragged last panel, cluster mode, mixed coins (tfr = 0.5: both token routes), the benched batch, and
    inference_decode"""
    import random
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    opt = FusedClipAdam(m.parameters(), lr=1e-3)            # (the bf16 weight shadows the backward composites read are the optimiser's)
    x, c, pr = synth_batch(B, 77)
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    eps = {n: torch.randn(B, 256, generator=torch.Generator().manual_seed(i)).to(DEV) for i, n in enumerate(('chd', 'rhy'))}
    res = {}
    for comp in (False, True):
        monkeypatch.setattr(FF_, 'FREE_COMPOSITE', comp)
        FF_._DFF.pop('calls', None)
        FF_._DFF.pop('bcalls', None)
        random.seed(3)
        m.eps_source = lambda name, shape, device: eps[name]
        opt.zero_grad()
        outs = m.run(xt, ct, prt, tfr, tfr, tfr)
        losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
        losses[0].backward()
        torch.cuda.synchronize()
        assert bool(FF_._DFF.get('calls')) == comp                 # the composites ran exactly when asked to: forward ...
        if bwd_call:                                               # ... and backward (ptv_decoder_free_bwd: when every stage of the node has its
            assert bool(FF_._DFF.get('bcalls')) == comp            # composite -- at small batches the re-summarisation BPTT runs on the persistent
                                                                   # kernels, launched from Python: the node then goes out stage by stage)
        with torch.no_grad():
            z = torch.cat([outs[2].mean, outs[3].mean], -1).detach()
            est = m.inference_decode(z[:, :256], z[:, 256:])
        res[comp] = ([l.detach().clone() for l in losses], m.decoder.last_xhat.clone(), est,
                     {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    (l0, x0, e0, g0), (l1, x1, e1, g1) = res[False], res[True]
    for a, b in zip(l0, l1):
        assert torch.equal(a, b), (a, b)
    assert torch.equal(x0, x1) and (e0 == e1).all()
    assert set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), (n, (g0[n] - g1[n]).abs().max())
    from polyphonic_chord_texture_disentanglement_amd.functional import persist_check
    persist_check()


def test_note_loop_producer_head_split_kernel_equals_four_wave_kernel(monkeypatch):
    """csrc/freerun.hip has two note-loop kernels (4 waves phase by phase / producers + heads over 8 waves, chosen by panel count):
    same decisions and logits from both, in inference and in a free-running training step (full geometry)"""
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    B = 40                                                       # 3 panels, the last one ragged
    g = torch.Generator().manual_seed(11)
    z = (torch.randn(B, 512, generator=g) * 0.8).to(DEV)
    x, c, pr = synth_batch(B, 321)
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    eps = {n: torch.randn(B, 256, generator=torch.Generator().manual_seed(i)).to(DEV) for i, n in enumerate(('chd', 'rhy'))}
    res = {}
    for split in (False, True):
        monkeypatch.setattr(FF_, 'NOTE_LOOP_SPLIT', split)
        with torch.no_grad():
            pitch, dur = m.decoder(z, True, None, None, 0., 0.)
        xh = m.decoder.last_xhat.clone()
        m.eps_source = lambda name, shape, device: eps[name]
        m.zero_grad()
        outs = m.run(xt, ct, prt, 0., 0., 0.)
        losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
        losses[0].backward()
        torch.cuda.synchronize()
        res[split] = (pitch.clone(), dur.clone(), xh, np.array([l.item() for l in losses]), m.decoder.last_xhat.clone(),
                      {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    a, b = res[False], res[True]
    # (split-K atomics make near-tie argmaxes flip from run to run, and a flipped note changes the rest of its time step)
    assert (a[2] == b[2]).float().mean() > 0.99 and (a[4] == b[4]).float().mean() > 0.99
    same = (a[2] == b[2]).all(-1)[:, :, 1:].permute(2, 1, 0)     # [15,32,B]: compare logits where the fed history agrees
    assert same.float().mean() > 0.97
    np.testing.assert_allclose(b[3], a[3], rtol=0, atol=5e-3)
    for n in a[5]:
        assert (b[5][n] - a[5][n]).abs().max() <= 0.05 * a[5][n].abs().max() + 1e-6, n


def test_zero_skip_backward_equals_dense_backward(monkeypatch):
    """functional.ZERO_SKIP: the backward passes over note steps / tiles at which no gradient arrives and over packed-sequence
    padding; against the dense run (PTV_ZERO_SKIP=0): same losses, same gradients (the skipped contributions are exact zeros; what
    differs is the order of the fp32 atomics in the weight-gradient products)"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    B = 72                                                       # R = 2304 rows: 36 panels
    x, c, pr = synth_batch(B, 777)
    xt, ct, prt = (torch.from_numpy(a).to(DEV) for a in (x, c, pr))
    eps = {n: torch.randn(B, 256, generator=torch.Generator().manual_seed(i)).to(DEV) for i, n in enumerate(('chd', 'rhy'))}
    res = {}
    for skip in (False, True):
        monkeypatch.setattr(F_, 'ZERO_SKIP', skip)
        for tfr in (1.0, 0.0):
            m.eps_source = lambda name, shape, device: eps[name]
            m.zero_grad()
            outs = m.run(xt, ct, prt, tfr, tfr, tfr)
            losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
            losses[0].backward()
            torch.cuda.synchronize()
            res[skip, tfr] = (np.array([l.item() for l in losses]), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    monkeypatch.setattr(F_, 'ZERO_SKIP', True)
    F_.zero_skip_sync()
    import os
    ordered = os.environ.get('PTV_WGRAD_ORDERED', '1') != '0'
    for tfr in (1.0, 0.0):
        (l0, g0), (l1, g1) = res[False, tfr], res[True, tfr]
        np.testing.assert_allclose(l1, l0, rtol=0, atol=(3e-5 if tfr == 1.0 else 5e-3))     # (atomics mode: ~1e-6 relative run to run)
        for n in g0:
            tol = 2e-3 if tfr == 1.0 else 0.05                  # tfr = 0: near-tie argmaxes may flip between two runs
            assert (g1[n] - g0[n]).abs().max() <= tol * g0[n].abs().max() + 1e-7, (tfr, n)
        if ordered and tfr == 1.0:
            # ordered reductions: the skipped contributions are exact zeros and x + 0 = x, so skipping changes NO bit of the losses and of
            # every gradient -- except the duration GRU's, whose per-block partials are split differently when tiles drop out (1e-7)
            assert np.array_equal(l1, l0)
            for n in g0:
                if 'dec_dur_gru' in n or 'dur_sos_token' in n:       # (what ptv_dur_bwd_finalize assembles from the per-block partials)
                    assert (g1[n] - g0[n]).abs().max() <= 1e-6 * g0[n].abs().max(), n
                else:
                    assert torch.equal(g1[n], g0[n]), n


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_sibling_streams_do_not_change_a_steady_state_training_run(prec, monkeypatch):
    """functional.Side: the weight-gradient products run on sibling HIP streams, the decoder's joined only when the backward pass
    ends.  Against the same run with everything on one stream (functional.OVERLAP = False), in STEADY STATE -- models built one after
    the other in one process and several optimiser steps each, so every block comes from the caching allocator's warm pool (no
    hipMalloc, which would serialise and hide a missing dependency or a buffer released under a queued reader): same losses, same
    gradients at every step"""
    import os
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    B, steps = 16, 4
    runs = {}
    for tag, overlap in (('warmup', True), ('serial', False), ('overlap', True), ('overlap2', True)):
        monkeypatch.setattr(F_, 'OVERLAP', overlap)
        m = M.DisentangleVAE.init_model(torch.device(DEV))
        m.load_state_dict(full_params())
        m.to(DEV).set_precision(prec)
        opt = FusedClipAdam(m.parameters(), lr=1e-3)
        m.use_philox(7, 0)
        out = []
        for step in range(steps):
            x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, 50 + step))
            opt.zero_grad()
            losses = m('train', x, c, pr, tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
            losses[0].backward()
            assert opt.arena.holds_all_grads()                     # every gradient adopted in place (no early clone)
            out.append((np.array([l.item() for l in losses]), opt.arena.flat.clone()))
            opt.clip_and_step(1.0)
        runs[tag] = (out, [(n, o, p.numel()) for (n, p), o in zip(m.named_parameters(), opt.arena.offsets)])
        del m, opt
    ref, index = runs['serial']
    for tag in ('overlap', 'overlap2'):
        for step in range(steps):
            (l0, g0), (l1, g1) = ref[step], runs[tag][0][step]
            # (bf16: the order of the fp32 atomics flips roundings of the bf16 operands; after an Adam step that is ~1e-3 on a loss --
            # measured up to 8e-4 at step 3; a missing dependency shows as >= 2e-2)
            np.testing.assert_allclose(l1, l0, rtol=0, atol=(2e-3 if prec == 'bf16' else 2e-4) * (step + 1), err_msg='%s step %d' % (tag, step))
            for n, o, k in index:
                a, b = g0[o:o + k], g1[o:o + k]
                tol = (1e-2 if prec == 'bf16' else 5e-4) * (step + 1)   # (atomics mode: order of the fp32 atomics + the bf16 roundings they flip; grows per step)
                assert (a - b).abs().max() <= tol * a.abs().max() + 1e-7, (tag, step, n, float((a - b).abs().max()), float(a.abs().max()))
            if prec == 'fp32' and os.environ.get('PTV_WGRAD_ORDERED', '1') != '0':
                # ordered reductions: the same kernels in the same association whatever stream they run on -- a missing dependency or a
                # buffer recycled under a queued reader cannot hide inside a tolerance: every loss and every gradient bit-identical.
                # (bf16 builds the embedding gradient's multi-hot operand with a different kernel when the streams are on.)
                assert np.array_equal(l1, l0), (tag, step)
                assert torch.equal(g0, g1), (tag, step, float((g0 - g1).abs().max()))


# ---------------------------------------------------------------------------------------------
# the whole step as one hipGraph launch (graph_step.GraphedTrainStep)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec,B', [('fp32', 4), ('bf16', 64)])
def test_graph_replayed_train_steps_equal_eager_steps(prec, B):
    """4 optimisation steps with a changing batch, Philox noise, a decaying learning rate and an annealed beta: replayed from the
    captured graph vs enqueued eagerly (reference loop body amc_dl/torch_plus/module.py:129-150).  Same losses per step and the same
    parameters at the end, to the run-to-run noise of the fp32 atomics (helpers); building the graph (warm-up steps + capture) must
    leave no trace in the training state: step count, draw counter and coin stream end where the eager run's do."""
    import random
    from helpers import ADAM_NOISE_FRAC_OF_LR
    from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus import MinExponentialLR
    from polyphonic_chord_texture_disentanglement_amd.graph_step import GraphedTrainStep
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    full = prec == 'bf16'
    batches = [tuple(torch.from_numpy(a).to(DEV) for a in synth_batch(B, 700 + i)) for i in range(4)]
    betas = [0.0, 0.03, 0.06, 0.1]
    res = {}
    for mode in ('eager', 'graph'):
        if full:
            m = M.DisentangleVAE.init_model(torch.device(DEV))
            m.load_state_dict(full_params())
            m.to(DEV).set_precision('bf16')
        else:
            m = build_reduced(DEV).to(DEV)
        opt = FusedClipAdam(m.parameters(), lr=1e-3)
        sched = MinExponentialLR(opt, gamma=0.9, minimum=1e-5)
        m.use_philox(seed=11, sample_offset=0)
        random.seed(5)
        gs = GraphedTrainStep(m, opt, B) if mode == 'graph' else None
        losses = []
        for i, (x, c, pr) in enumerate(batches):
            if gs is not None:
                losses.append(gs(x, c, pr, beta=betas[i]).cpu().numpy().copy())
            else:
                opt.zero_grad()
                out = m('train', x, c, pr, tfr1=1., tfr2=1., tfr3=1., beta=betas[i], weights=[1, 0.5])
                out[0].backward()
                opt.clip_and_step(1.0)
                losses.append(np.array([float(o) for o in out]))
            sched.step()
        F_.persist_check()
        res[mode] = (np.stack(losses), opt.flat_p.detach().cpu().clone(), opt.step_count, m._draws, random.random(), float(opt.grad_norm()))
        del m, opt, gs
    le, lg = res['eager'][0], res['graph'][0]
    tol = 2e-3 if full else 2e-5
    for i in range(4):
        np.testing.assert_allclose(lg[i], le[i], rtol=0, atol=tol * (i + 1), err_msg='step %d' % i)
    assert abs(lg[1][0] - lg[0][0]) > 10 * tol                       # (the steps really differ: batch, beta, lr)
    assert res['graph'][2:5] == res['eager'][2:5]                       # step count, Philox draws, position of the coin stream
    assert abs(res['graph'][5] - res['eager'][5]) <= (2e-2 if full else 1e-3) * res['eager'][5]
    dp = (res['graph'][1] - res['eager'][1]).abs().max()
    assert dp <= 1e-3 * ADAM_NOISE_FRAC_OF_LR * 4 * (25 if full else 1), float(dp)
    import os
    if not full and os.environ.get('PTV_WGRAD_ORDERED', '1') != '0':
        # ordered reductions + the same kernels: a replayed fp32 step is the eager step bit for bit (losses and parameters)
        assert np.array_equal(lg, le) and torch.equal(res['graph'][1], res['eager'][1])


def test_trainer_surface_with_graph_replayed_steps(tmp_path, monkeypatch):
    """TrainingVAE.train() with graph_step = True (device batch transform -> replayed step -> schedulers -> async logging) against the
    same epoch run eagerly: epoch losses, LR / beta schedule positions and optimiser step count"""
    import random
    from polyphonic_chord_texture_disentanglement_amd.amc_dl import torch_plus as tp
    from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus.train_utils import kl_anealing
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import MusicDataLoaders, TrainingVAE
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_raw_bank
    monkeypatch.chdir(tmp_path)
    bank = synth_raw_bank(10, 3)
    out = {}
    for graph in (False, True):
        m = build_reduced(DEV).to(DEV)
        m.use_philox(seed=2, sample_offset=0)
        random.seed(8)
        opt = FusedClipAdam(m.parameters(), lr=1e-3)
        osch = tp.OptimizerScheduler(opt, tp.MinExponentialLR(opt, gamma=0.99, minimum=1e-5), 1)
        ps = tp.ParameterScheduler(tfr1=tp.ConstantScheduler(1.), tfr2=tp.ConstantScheduler(1.), tfr3=tp.ConstantScheduler(1.),
                                   beta=tp.TeacherForcingScheduler(0.1, 0., f=kl_anealing), weights=tp.ConstantScheduler([1, 0.5]))
        loaders = MusicDataLoaders.get_loaders(11, bs_train=12, bs_val=4, device_bank=bank)
        loaders.train_loader.drop_last = True
        pm = tp.LogPathManager(None)
        sw = tp.SummaryWriters(M.LOSS_NAMES, {'loss': None}, pm.writer_path)
        tr = TrainingVAE(torch.device(DEV), m, False, pm, loaders, sw, osch, ps, 1, graph_step=graph)
        dic = tr.train()
        assert ('_graph_steps' in tr.__dict__ and len(tr._graph_steps) == 1) == graph
        out[graph] = (dic, opt.step_count, opt.param_groups[0]['lr'], tr.train_step, opt.flat_p.detach().cpu().clone())
    n = out[True][3]
    assert n == out[False][3] and n >= 4 and out[True][1] == out[False][1] == n
    assert abs(out[True][2] - out[False][2]) < 1e-15
    for k in out[False][0]:
        assert abs(out[True][0][k] - out[False][0][k]) <= 2e-5 * n * max(1.0, abs(out[False][0][k])), k
    assert (out[True][4] - out[False][4]).abs().max() <= 2e-5 * n
    import os
    if os.environ.get('PTV_WGRAD_ORDERED', '1') != '0':          # ordered reductions: the replayed epoch leaves the same bits as the eager one
        assert torch.equal(out[True][4], out[False][4])


@pytest.mark.parametrize('B', [64, 160])
def test_repeated_backward_passes_are_bit_identical_and_no_reduction_fell_back_to_atomics(B):
    """Found in round 4: from B = 64 on the duration GRU's partial sums (320 column blocks) exceeded the ordered-reduction counter
    budget and ran on fp32 atomics SILENTLY -- the B = 32 trace below never saw it.  Now the budget covers them, every fallback is
    counted (ptv_ordered_fallbacks) and this test holds both: four backward passes of one step give the same bits, counter 0."""
    import os
    import random
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    if os.environ.get('PTV_WGRAD_ORDERED', '1') == '0':
        pytest.skip('fp32 atomics requested')
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV).set_precision('bf16')
    opt = FusedClipAdam(m.parameters(), lr=1e-3)
    x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, 55))
    F_.ordered_fallbacks(reset=True)
    runs = []
    for i in range(4):
        m.use_philox(7, 0)
        random.seed(7)
        opt.zero_grad()
        ls = m('train', x, c, pr, tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
        ls[0].backward()
        torch.cuda.synchronize()
        runs.append(opt.arena.flat.detach().clone())
    assert F_.ordered_fallbacks() == 0
    for i in (1, 2, 3):
        assert torch.equal(runs[0], runs[i]), (i, float((runs[0] - runs[i]).abs().max()))


def test_fp32_atomics_mode_matches_the_ordered_reductions():
    """round-3 advice: keep the PTV_WGRAD_ORDERED=0 path (every reduction ends in fp32 atomics: arrival-order rounding) exercised.
    Same full-geometry bf16 backward pass in both modes of ptv_ordered_reductions: losses to a few ulps, gradients equal to the
    noise of fp32 summation order amplified by the bf16 rounding of saved tensors (1e-2 of each tensor's largest element; measured 2e-3)."""
    from polyphonic_chord_texture_disentanglement_amd._lib import lib
    g = load_npz('full_tf1_b4.npz')
    x, c, pr = synth_batch(int(g['B']), int(g['data_seed']))
    res = {}
    try:
        for ordered in (1, 0):
            assert lib().ptv_ordered_reductions(ordered) == 0
            m = M.DisentangleVAE.init_model(torch.device(DEV))
            m.load_state_dict(full_params())
            m.to(DEV).set_precision('bf16')
            outs, losses = _run(m, g, x, c, pr)
            losses[0].backward()
            res[ordered] = (np.array([l.item() for l in losses]), {k: p.grad.detach().clone() for k, p in m.named_parameters()})
    finally:
        lib().ptv_ordered_reductions(1)
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=0, atol=1e-5)      # (the loss sums are grid reductions too: a few fp32 ulps)
    for k, a in res[1][1].items():
        b = res[0][1][k]
        # (bf16 saved tensors upstream: an fp32 ulp of summation noise can flip a bf16 rounding, 2^-9 relative, of what the next product reads)
        assert float((a - b).abs().max()) <= 1e-7 + 1e-2 * float(a.abs().max()), k


@pytest.mark.parametrize('prec,tfr', [('fp32', 1.0), ('bf16', 1.0), ('bf16', 0.0)])
def test_two_runs_of_a_training_trace_are_bit_identical(prec, tfr):
    """Ordered reductions (include/ptvae_hip.h: ptv_ordered_reductions, the default): no result of the step depends on the arrival
    order of fp32 atomics, so -- like the reference on the CPU -- two runs of the same 3-step trace give the same
    bits: every loss, the gradient norm and every parameter.  Sibling streams, persistent launches and the zero-skip stay on."""
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    import os
    import random
    if os.environ.get('PTV_WGRAD_ORDERED', '1') == '0':
        pytest.skip('fp32 atomics requested (PTV_WGRAD_ORDERED=0): summation order follows arrival order')
    runs = []
    for rep in range(2):
        if prec == 'fp32':
            m = build_reduced(DEV).to(DEV)
            B = 5
        else:
            m = M.DisentangleVAE.init_model(torch.device(DEV))
            m.load_state_dict(full_params())
            m.to(DEV).set_precision('bf16')
            B = 32
        opt = FusedClipAdam(m.parameters(), lr=1e-3)
        m.use_philox(seed=3, sample_offset=0)
        random.seed(4)
        trace = []
        for step in range(3):
            x, c, pr = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, 900 + step))
            opt.zero_grad()
            losses = m('train', x, c, pr, tfr1=tfr, tfr2=tfr, tfr3=tfr, beta=0.1, weights=[1, 0.5])
            losses[0].backward()
            opt.clip_and_step(1.0)
            trace.append((torch.stack([l.detach() for l in losses]).cpu(), opt.grad_norm().cpu(), opt.arena.flat.detach().cpu().clone()))
        runs.append((trace, opt.flat_p.detach().cpu().clone()))
        del m, opt
    for step, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        assert torch.equal(a[0], b[0]), (step, (a[0] - b[0]).abs().max())
        assert torch.equal(a[2], b[2]), (step, float((a[2] - b[2]).abs().max()))
        assert torch.equal(a[1], b[1]), step
    assert torch.equal(runs[0][1], runs[1][1])
