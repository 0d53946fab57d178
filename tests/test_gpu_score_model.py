"""Per-sample scores through the public surface: DisentangleVAE.score / reconstruction_report, PtvaeDecoder.score_outputs and the
trainer's eval_metrics switch, against the reference model's golden losses, the package's own loss() and the fp64 formulas of
tests/score_ref.py.  Float comparisons that name no golden tolerance use the measured-fp32 rule of test_gpu_score_kernels.check()."""
import numpy as np
import pytest
import torch

import score_ref as S
from helpers import full_params, load_npz
from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd import model as M
from polyphonic_chord_texture_disentanglement_amd.ptvae import HipNormal
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch
from test_gpu_score_kernels import check, steps_f32, step_scale
from test_host_surface import build_reduced

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POOLED = (2, 3, 5, 6, 8, 9, 10)          # pl, dl, kl_chd, kl_rhy, root, chroma, bass of the 11 losses


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def eps_source(g):
    return lambda name, shape, device: torch.from_numpy(g['eps_' + name]).to(device)


def pooled(s, Z):
    """score()'s per-sample sums -> the seven batch means loss() reports, pooled in fp64 on the host"""
    h = {k: v.cpu().numpy().astype(np.float64) for k, v in s.items()}
    B = h['counts'].shape[0]
    cnt = h['counts'].sum(0)
    return np.array([h['pitch_nll'].sum() / cnt[0], h['dur_nll'].sum() / cnt[2], h['kl_chd'].sum() / (B * Z), h['kl_rhy'].sum() / (B * Z),
                     h['root_nll'].sum() / (B * 8), h['chroma_nll'].sum() / (B * 96), h['bass_nll'].sum() / (B * 8)])


@pytest.fixture(scope='module')
def full():
    g = load_npz('full_tf1_b4.npz')
    m = M.DisentangleVAE.init_model(torch.device(DEV))
    m.load_state_dict(full_params())
    m.to(DEV)
    m.eps_source = eps_source(g)
    x, c, pr = dev(*synth_batch(int(g['B']), int(g['data_seed'])))
    return g, m, x, c, pr


def test_full_geometry_pooled_scores_equal_the_golden_losses_and_loss(full):
    g, m, x, c, pr = full
    s = m.score(x, c, pr, sample=True, beta=float(g['beta']))
    for k in ('pitch_nll', 'dur_nll', 'kl_chd', 'kl_rhy', 'root_nll', 'chroma_nll', 'bass_nll', 'elbo'):
        assert s[k].shape == (4,) and s[k].dtype == torch.float32 and not s[k].requires_grad, k
    assert s['counts'].shape == (4, 6) and s['chord_counts'].shape == (4, 3) and s['counts'].dtype == torch.int32
    assert s['step_scores'].shape == (4, 32, 2) and s['step_counts'].shape == (4, 32, 6)
    got = pooled(s, 256)
    print('SCORE_POOLED full', np.abs(got - g['losses'][list(POOLED)]).max())
    np.testing.assert_allclose(got, g['losses'][list(POOLED)], rtol=0, atol=1e-4)       # the bar loss() is held to on this fixture
    # elbo = -(pitch_nll + dur_nll) - beta (kl_chd + kl_rhy), by the elementwise kernels: four fp32 operations per sample
    h = {k: v.cpu().numpy() for k, v in s.items()}
    beta = np.float32(g['beta'])
    want = -(h['pitch_nll'].astype(np.float64) + h['dur_nll']) - float(beta) * (h['kl_chd'].astype(np.float64) + h['kl_rhy'])
    f32 = ((-h['pitch_nll'] - h['dur_nll']) - beta * h['kl_chd']) - beta * h['kl_rhy']
    check('elbo', h['elbo'], want, f32, np.abs(h['pitch_nll']) + np.abs(h['dur_nll']) + np.abs(h['kl_chd']) + np.abs(h['kl_rhy']))
    # ... and what loss() returns on the same inputs and noise: both are measured against the fp64 value of the same logits
    with torch.no_grad():
        outs = m.run(x, c, pr, 1., 1., 1.)
        losses = m.loss_function(x, c, *outs, float(g['beta']), [float(w) for w in g['weights']])
    loss = np.array([l.item() for l in losses])[list(POOLED)]
    ref, f32 = fp64_and_fp32_means(x, c, outs)
    print('SCORE_VS_LOSS full', np.abs(got - loss).max())
    check('pooled scores', got, ref, f32, np.abs(ref))
    check('loss()', loss, ref, f32, np.abs(ref))


def fp64_and_fp32_means(x, c, outs):
    """the seven pooled means of run()'s outputs: in fp64 (score_ref) and by the same formulas in fp32 (torch, CPU)"""
    pitch, dur, dc, dr, root, chroma, bass = outs
    xh, ch = x.cpu().numpy(), c.cpu().numpy()
    P, D, R, C, Bs = (t.detach().contiguous().cpu().numpy() for t in (pitch, dur, root, chroma, bass))
    B, Z = dc.mean.shape
    sc, cn = S.score_fold(*S.recon_step_scores(P, D, xh))
    chord, _ = S.chord_step_scores(R, C, Bs, ch)
    kl = [S.kl_rows(d.mean.cpu().numpy(), d.scale.cpu().numpy()).sum() / (B * Z) for d in (dc, dr)]
    ref = np.array([sc[:, 0].sum() / cn[:, 0].sum(), sc[:, 1].sum() / cn[:, 2].sum(), kl[0], kl[1], chord[:, 0].sum() / (B * 8),
                    chord[:, 1].sum() / (B * 96), chord[:, 2].sum() / (B * 8)])
    ce = torch.nn.functional.cross_entropy
    xt = torch.from_numpy(xh)
    rt, ct, bt = (torch.from_numpy(np.ascontiguousarray(t)) for t in S.chord_targets(ch))
    kl32 = [float((-torch.log(d.scale.cpu()) + (d.scale.cpu() ** 2 + d.mean.cpu() ** 2) * 0.5 - 0.5).mean()) for d in (dc, dr)]
    f32 = np.array([float(ce(torch.from_numpy(P).reshape(-1, 130), xt[:, :, 1:, 0].reshape(-1), ignore_index=130)),
                    float(ce(torch.from_numpy(D).reshape(-1, 2), xt[:, :, 1:, 1:].reshape(-1), ignore_index=2)), kl32[0], kl32[1],
                    float(ce(torch.from_numpy(R).reshape(-1, 12), rt.reshape(-1))), float(ce(torch.from_numpy(C).reshape(-1, 2), ct.reshape(-1))),
                    float(ce(torch.from_numpy(Bs).reshape(-1, 12), bt.reshape(-1)))])
    return ref, f32


def test_score_outputs_against_the_fp64_formulas_on_the_models_own_logits(full):
    g, m, x, c, pr = full
    with torch.no_grad():
        pitch, dur = m.run(x, c, pr, 1., 1., 1.)[:2]
    assert not pitch.is_contiguous()                                                   # the decoder's step-major view: read in place
    out = m.decoder.score_outputs(x, pitch, dur)
    P, D, xh = pitch.contiguous().cpu().numpy(), dur.contiguous().cpu().numpy(), x.cpu().numpy()
    ref_s, ref_c = S.recon_step_scores(P, D, xh)
    assert np.array_equal(out['step_counts'].cpu().numpy(), ref_c)
    assert np.array_equal(out['counts'].cpu().numpy(), ref_c.sum(1))
    check('model step scores', out['step_scores'].cpu().numpy(), ref_s, steps_f32(xh, P, D), step_scale(xh, P, D))
    f32 = steps_f32(xh, P, D).sum(1, dtype=np.float32)
    check('model scores', out['scores'].cpu().numpy(), ref_s.sum(1), f32, step_scale(xh, P, D).sum(1))
    # batch-major copies of the same logits: the same bits
    again = m.decoder.score_outputs(x, pitch.contiguous(), dur.contiguous())
    for k in out:
        assert again[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k


def test_reduced_model_pooled_scores_equal_the_golden_losses():
    g = load_npz('reduced_tf1.npz')
    m = build_reduced(DEV).to(DEV)
    m.eps_source = eps_source(g)
    s = m.score(*dev(g['x'], g['c'], g['pr_mat']), sample=True, beta=float(g['beta']))
    got = pooled(s, 16)
    print('SCORE_POOLED reduced', np.abs(got - g['losses'][list(POOLED)]).max())
    np.testing.assert_allclose(got, g['losses'][list(POOLED)], rtol=0, atol=1e-5)


def test_detrended_variant_scores_through_the_pr_mat_slot():
    """train.py:31-39's model: dt_x as the fourth argument, in the pr_mat slot (the inference family's rule) or derived from x and c give
    the same bits, and pool to the golden losses within the bound test_gpu_detrended.py holds loss() to on this fixture"""
    from collections import OrderedDict
    from polyphonic_chord_texture_disentanglement_amd.synthetic import fill_state_dict
    from test_gpu_model_wide import TF1_BOUNDS
    g = load_npz('detrended_b4.npz')
    m = M.DisentangleVAE.init_model_detrended(torch.device(DEV))
    shapes = OrderedDict((str(n), tuple(int(t) for t in sh.strip('()').split(',') if t.strip())) for n, sh in zip(g['names'], g['shapes']))
    m.load_state_dict(fill_state_dict(shapes, seed=1234))
    m = m.to(DEV).set_precision('fp32')
    m.eps_source = eps_source(g)
    x, c, pr = dev(*synth_batch(int(g['B']), int(g['data_seed'])))
    dt_x, = dev(g['dt_x'])
    a = m.score(x, c, pr, dt_x, sample=True, beta=float(g['beta']))
    got = pooled(a, 256)
    print('SCORE_POOLED detrended', np.abs(got - g['losses'][list(POOLED)]).max())
    np.testing.assert_allclose(got, g['losses'][list(POOLED)], rtol=0, atol=TF1_BOUNDS['fp32'][0])
    for other in (m.score(x, c, dt_x, sample=True, beta=float(g['beta'])), m.score(x, c, pr, sample=True, beta=float(g['beta']))):
        for k in a:
            assert other[k].cpu().numpy().tobytes() == a[k].cpu().numpy().tobytes(), k
    with pytest.raises(ValueError):
        m.score(x, c, pr, dt_x[:2])
    with pytest.raises(ValueError):
        m.score(x, c, pr, dt_x.float())
    rep = m.reconstruction_report(x, c, dt_x)
    assert set(rep) == set(M.DisentangleVAE.REPORT_NAMES) and rep == m.reconstruction_report(x, c, pr, dt_x)


def test_mean_scores_are_deterministic_and_their_kl_is_ptv_kl_rows():
    import random
    g = load_npz('reduced_tf1.npz')
    m = build_reduced(DEV).to(DEV)
    m.use_philox(3)
    x, c, pr = dev(g['x'], g['c'], g['pr_mat'])
    random.seed(11)
    coins = random.getstate()
    a, b = m.score(x, c, pr), m.score(x, c, pr)
    assert random.getstate() == coins and m._draws == 0                                # neither a coin nor a noise draw was consumed
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    dc, dr = m.inference_encode(pr, c)
    for name, d in (('kl_chd', dc), ('kl_rhy', dr)):
        out = torch.empty(3, device=DEV)
        F_.call('ptv_kl_rows', F_.ptr(d.mean.contiguous()), F_.ptr(d.scale.contiguous()), 3, 16, F_.ptr(out), F_.stream_ptr())
        assert out.cpu().numpy().tobytes() == a[name].cpu().numpy().tobytes(), name
    s = m.score(x, c, pr, sample=True)                                                 # the usual noise path: one draw per latent
    assert m._draws == 2 and not np.array_equal(s['pitch_nll'].cpu().numpy(), a['pitch_nll'].cpu().numpy())
    np.testing.assert_array_equal(s['kl_chd'].cpu().numpy(), a['kl_chd'].cpu().numpy())          # (the posterior does not depend on z)


def test_reconstruction_report_of_a_batch_the_model_decodes_to_itself(monkeypatch):
    m = build_reduced(DEV).to(DEV)
    B = 6
    gen = torch.Generator().manual_seed(9)
    z_chd, z_rhy = ((2.0 * torch.randn(B, 16, generator=gen)).to(DEV) for _ in range(2))
    pr, x, c, _, count, err = m.decode_to_inputs(z_chd, z_rhy, max_notes=15)           # (x: every note the canonical grid keeps)
    one = torch.ones(B, 16, device=DEV)
    monkeypatch.setattr(m.chd_encoder, 'forward', lambda *a, **k: HipNormal(z_chd, one))
    monkeypatch.setattr(m.rhy_encoder, 'forward', lambda *a, **k: HipNormal(z_rhy, one))
    t = m.reconstruction_counts(x, c, pr)
    assert set(t) == set(M.DisentangleVAE.TALLY_NAMES)
    assert t['ref_n'] > 0, 'the decoded batch holds no note: pick another z'
    assert t['est_n'] == t['ref_n'] == t['onset_tp'] == t['exact_tp']                  # the free-running pass regenerates the grid
    rep = m.report_from_counts(t)
    assert rep['onset_f1'] == 1.0 and rep['exact_f1'] == 1.0 and rep['onset_precision'] == 1.0 and rep['onset_recall'] == 1.0
    assert set(rep) == set(M.DisentangleVAE.REPORT_NAMES)
    assert rep == m.reconstruction_report(x, c, pr)
    # the host reference of the same report, from the per-sample tensors
    s = m.score(x, c, pr)
    want = S.report(s['counts'].cpu().numpy(), s['chord_counts'].cpu().numpy(), [[t[k] for k in ('est_n', 'ref_n', 'onset_tp', 'exact_tp')]],
                    float((s['pitch_nll'].double() + s['dur_nll'].double()).sum()))
    for k in rep:
        assert abs(rep[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k
    # one note of x moved to a pitch its step does not hold: one reference cell misses, one estimated cell is unmatched
    xh = x.cpu().numpy()
    b, s_, n = next((b, s_, n) for b, s_, n in zip(*np.nonzero(xh[:, :, 1:, 0] < 128))
                    if (xh[b, s_, 1:, 0] == xh[b, s_, n + 1, 0]).sum() == 1)               # (a pitch its step holds once)
    held = set(xh[b, s_, 1:, 0].tolist())
    x2 = x.clone()
    x2[b, s_, n + 1, 0] = next(p for p in range(128) if p not in held)
    t2 = m.reconstruction_counts(x2, c, pr)
    assert (t2['est_n'], t2['ref_n']) == (t['est_n'], t['ref_n'])
    assert (t2['onset_tp'], t2['exact_tp']) == (t['onset_tp'] - 1, t['exact_tp'] - 1)


def make_trainer(m, tmp_path, **kw):
    from polyphonic_chord_texture_disentanglement_amd.amc_dl import torch_plus as tp
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import MusicDataLoaders, TrainingVAE
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    loaders = MusicDataLoaders.get_loaders(3345, bs_train=4, bs_val=4, n_train_batch=1, n_val_batch=2)
    pm = tp.LogPathManager(None)
    opt = FusedClipAdam(m.parameters(), lr=1e-3)
    osch = tp.OptimizerScheduler(opt, tp.MinExponentialLR(opt, gamma=0.9999, minimum=1e-5), 1)
    sw = tp.SummaryWriters(M.LOSS_NAMES, {'loss': None}, pm.writer_path, **kw.pop('writers', {}))
    ps = tp.ParameterScheduler(tfr1=tp.ConstantScheduler(1.), tfr2=tp.ConstantScheduler(1.), tfr3=tp.ConstantScheduler(1.),
                               beta=tp.ConstantScheduler(0.1), weights=tp.ConstantScheduler([1, 0.5]))
    return TrainingVAE(torch.device(DEV), m, False, pm, loaders, sw, osch, ps, 1, **kw)


def test_trainer_eval_metrics_switch(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    m = build_reduced(DEV).to(DEV)
    m.eps_source = lambda name, shape, device: torch.zeros(shape, device=device)
    plain, off = make_trainer(m, tmp_path), make_trainer(m, tmp_path, eval_metrics=False)
    assert 'eval_metrics' not in plain.__dict__ and off.__dict__['eval_metrics'] is False
    a, b = plain.eval(), off.eval()
    assert list(a) == list(b) == M.LOSS_NAMES
    assert np.array([a[k] for k in a]).tobytes() == np.array([b[k] for k in b]).tobytes()          # bit for bit
    assert plain.val_metrics is None and off.val_metrics is None
    written = []
    on = make_trainer(m, tmp_path, eval_metrics=True, writers=dict(extra={'val_metrics': M.DisentangleVAE.REPORT_NAMES}))
    monkeypatch.setattr(on.summary_writers, 'single_write', lambda name, tag, val, step: written.append((name, tag, val, step)))
    c = on.eval()
    assert np.array([c[k] for k in c]).tobytes() == np.array([a[k] for k in a]).tobytes()          # the losses are not touched
    vm = on.val_metrics
    assert set(vm) == set(M.DisentangleVAE.REPORT_NAMES)
    for k in vm:
        assert isinstance(vm[k], float) and (k == 'nll_per_note' or 0.0 <= vm[k] <= 1.0), (k, vm[k])
    assert vm['nll_per_note'] > 0
    n_pitch = sum(int((on._batch_to_inputs(batch)[0][:, :, 1:, 0] != 130).sum()) for batch in on.data_loaders.val_loader)
    assert on.val_counts['pitch_n'] == n_pitch > 0                                     # the counts of both validation batches, pooled
    assert on.val_counts['chord_steps'] == 8 * 4 * 2
    assert [(n, t, v) for n, t, v, _ in written if t == 'val_metrics'] == [(k, 'val_metrics', vm[k]) for k in M.DisentangleVAE.REPORT_NAMES]
    on.epoch_report(0.0, 1.0, 1.0, 1.0)
    # a writer without the extra task: the attribute only
    quiet = make_trainer(m, tmp_path, eval_metrics=True)
    monkeypatch.setattr(quiet.summary_writers, 'write_task', lambda task, vals, step: task != 'val_metrics' or 1 / 0)
    quiet.eval()
    assert quiet.val_metrics == vm


def test_bad_inputs_raise_before_any_launch(monkeypatch):
    g = load_npz('reduced_tf1.npz')
    m = build_reduced(DEV).to(DEV)
    x, c, pr = dev(g['x'], g['c'], g['pr_mat'])
    with torch.no_grad():
        pitch, dur = m.run(x, c, pr, 1., 1., 1.)[:2]
    torch.cuda.synchronize()
    launches = []

    def refuse(*a, **k):
        launches.append(a[:1])
        raise AssertionError('a launch was attempted')
    monkeypatch.setattr(F_, 'call', refuse)
    monkeypatch.setattr(F_, 'lib', refuse)
    monkeypatch.setattr(F_, 'check', refuse)
    bad = [(x.cpu(), c, pr), (x, c.cpu(), pr), (x, c, pr.cpu()), (x[:2], c, pr), (x, c[:2], pr), (x, c, pr[:1]), (x[:, :, :15], c, pr),
           (x, c[:, :, :35], pr), (x, c, pr[:, :, :127]), (x.float(), c, pr)]
    for args in bad:
        for fn in (m.score, m.reconstruction_report, m.reconstruction_counts):
            with pytest.raises(ValueError):
                fn(*args)
    for args in ((x.cpu(), pitch, dur), (x, pitch.cpu(), dur), (x, pitch, dur.cpu()), (x[:2], pitch, dur), (x, pitch[:2], dur),
                 (x, pitch, dur[:, :, :, :4]), (x, pitch[..., :129], dur)):
        with pytest.raises(ValueError):
            m.decoder.score_outputs(*args)
    ss, sc = torch.zeros(3, 32, 2, device=DEV), torch.zeros(3, 32, 6, dtype=torch.int32, device=DEV)
    for fn, args in ((F_.score_fold, (ss.cpu(), sc)), (F_.score_fold, (ss, sc[:2])), (F_.kl_rows, (ss[:, 0].cpu(), ss[:, 0])),
                     (F_.kl_rows, (ss[:, 0], ss[:2, 0])), (F_.roll_match, (pr.cpu(), pr)), (F_.roll_match, (pr, pr[:2])),
                     (F_.chord_scores, (c, pitch, dur, dur))):
        with pytest.raises(ValueError):
            fn(*args)
    assert not launches
