"""The loss node in one launch per direction (csrc/loss.hip: vae_loss_fwd_kernel / vae_loss_bwd_kernel behind ptv_vae_loss_fwd / _bwd)
against the launch-by-launch path, bit for bit: the 11 outputs and the nine gradients, the forward that writes the gradients for
losses[0].backward() and the backward that returns on its record, the recomputing backward, and ptv_reparam_kl_fwd without a KL sum.

Batch sizes, chosen where the block map changes: 1 (every small term one block), 3 (a partly filled tail block in the duration term),
35 (16 800 pitch rows > 8 * 2048: the pitch term wraps its grid-stride loop), 219 (525 600 duration rows > 256 * 2048: so does the
duration term)."""
import pytest
import torch

from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd._lib import lib, ptr, stream_ptr
from test_gpu_chord_loss_nodes import _loss_inputs, Z

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = F_.LossGrads._fields
BETA, W0, W1 = 0.3, 0.7, 0.4


def _e0(**other):
    g = torch.zeros(11)
    g[0] = 1.0
    for k, v in other.items():
        g[int(k[1:])] = v
    return g.to(DEV)


def _rand11(seed=3):
    return torch.rand(11, generator=torch.Generator().manual_seed(seed)).to(DEV) + 0.5


def _plan(x):
    """a LiveRows plan as loss() hands one to the node: the step-major targets of x, computed in front"""
    B = x.shape[0]
    pt, dt, cnt = F_._pianotree_target_buffers(B, x.device)
    F_.call('ptv_pianotree_targets', ptr(x), B, 1, ptr(pt), ptr(dt), ptr(cnt), stream_ptr())
    plan = F_.LiveRows(x, pt, dt, cnt)
    plan.record_order(False)
    return plan


def _early():
    return int(F_._vl_early(torch.device(DEV)).item())


def _node(ins, x, c, beta=BETA, plan=False):
    return F_.VaeLossFn.apply(*ins, x, c, beta, W0, W1, False, _plan(x) if plan else None)


def _run(ins, x, c, gout, beta=BETA, plan=False, forget=False):
    """-> (out, grads); forget: the forward's record is cleared before the backward, which then has to recompute"""
    out = _node(ins, x, c, beta, plan)
    if forget:
        out.grad_fn.fused[1].zero_()
    return out.detach().clone(), [g.clone() for g in torch.autograd.grad(out, ins, gout)]


def _same(a, b, what=''):
    assert torch.equal(a[0], b[0]), what + ' out'
    for n, ga, gb in zip(NAMES, a[1], b[1]):
        assert ga.shape == gb.shape and torch.equal(ga, gb), what + ' ' + n


def _inputs(B):
    """_loss_inputs(B).  'sm1': B = 1 with the pitch logits as a slice of a [15, 32, 1, 136] buffer: the one-sample dimension then has
    a stride consistent with its neighbours (a view(15, 32, 1, 130) of padded rows has not), so the node takes the logits step-major --
    the vectorised pitch form, every small term a single block -- and a LiveRows plan accepts them.  Plain _loss_inputs(1) is taken
    batch-major and runs the one-wave-per-row pitch form."""
    if B != 'sm1':
        return _loss_inputs(B)
    ins, x, c = _loss_inputs(1)
    buf = torch.zeros(15, 32, 1, 136, device=DEV)
    buf[..., :130] = ins[0].detach().permute(2, 1, 0, 3)
    ins[0] = buf[..., :130].permute(2, 1, 0, 3).detach().requires_grad_(True)
    return ins, x, c


def _launches(monkeypatch, *args, **kw):
    monkeypatch.setattr(F_, 'LOSS_COMPOSITE', False)
    res = _run(*args, **kw)
    monkeypatch.setattr(F_, 'LOSS_COMPOSITE', True)
    return res


@pytest.mark.parametrize('B,plan', [(1, False), ('sm1', False), ('sm1', True), (3, False), (3, True), (35, False), (35, True), (219, False)])
def test_composite_equals_launch_by_launch(B, plan, monkeypatch):
    """11 outputs and nine gradients, a random upstream vector (the backward recomputes), targets computed by the node or passed in
    through a LiveRows plan.  B = 1 twice: as _loss_inputs builds it (taken batch-major, where no plan applies) and step-major
    (_inputs), with and without a plan.  B = 219 is the plain comparison alone."""
    ins, x, c = _inputs(B)
    gout = _rand11()
    node = _node(ins, x, c)
    assert node.grad_fn.saved_state.sm_p is (B != 1) and node.grad_fn.saved_state.sm_c is True
    n = F_._VL.get('calls', 0), F_._VL.get('bwd_calls', 0), lib().ptv_ordered_fallbacks(0)
    fused = _run(ins, x, c, gout, plan=plan)
    assert (F_._VL.get('calls', 0) - n[0], F_._VL.get('bwd_calls', 0) - n[1]) == (1, 1)
    assert lib().ptv_ordered_fallbacks(0) == n[2]                    # (the one-launch forward ran, not the sequence behind it)
    ref = _launches(monkeypatch, ins, x, c, gout, plan=plan)
    assert torch.isfinite(fused[0]).all() and all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in fused[1])
    _same(fused, ref)


@pytest.mark.parametrize('B', [1, 'sm1', 3, 35])
def test_backward_returns_on_the_forwards_record(B, monkeypatch):
    """upstream exactly e0: the gradients the forward wrote = those of the same node with the record cleared = launch by launch; the
    kernel counted the early exit (a run that never takes the shortcut fails here)"""
    ins, x, c = _inputs(B)
    n = _early()
    n_bufs = F_._VL.get('fwd_grads', 0)
    short = _run(ins, x, c, _e0())
    assert _early() == n + 1 and F_._VL.get('fwd_grads', 0) == n_bufs + 1
    recomputed = _run(ins, x, c, _e0(), forget=True)
    assert _early() == n + 1
    ref = _launches(monkeypatch, ins, x, c, _e0())
    assert _early() == n + 1
    assert all(g.abs().sum() > 0 for g in short[1])
    _same(short, recomputed, 'record cleared:')
    _same(short, ref, 'launches:')


@pytest.mark.parametrize('gout', ['one_more', 'minus_zero', 'random'])
def test_backward_recomputes_on_another_upstream(gout, monkeypatch):
    """e0 with one other entry set, e0 with a -0.0 (equal as a number, not as bits) and a random vector: no early exit, bits of the launches"""
    ins, x, c = _loss_inputs(3)
    g = {'one_more': _e0(g8=0.25), 'minus_zero': _e0(g5=-0.0), 'random': _rand11(9)}[gout]
    n = _early()
    fused = _run(ins, x, c, g)
    assert _early() == n
    _same(fused, _launches(monkeypatch, ins, x, c, g))


def test_second_backward_over_a_retained_graph_recomputes():
    ins, x, c = _loss_inputs(3)
    out = _node(ins, x, c)
    n = _early()
    first = torch.autograd.grad(out, ins, _e0(), retain_graph=True)
    assert _early() == n + 1 and out.grad_fn.fused is None
    kept = [g.clone() for g in first]
    first[0].add_(1.0)                                               # (the decoder's backward updates dpitch in place)
    second = torch.autograd.grad(out, ins, _e0())
    assert _early() == n + 1                                          # fresh buffers, a cleared record: recomputed
    for name, buf, a, b in zip(NAMES, first, kept, second):
        assert buf.data_ptr() != b.data_ptr() and torch.equal(a, b), name


def test_forward_without_a_wanted_gradient_allocates_and_writes_no_gradients(monkeypatch):
    ins, x, c = _loss_inputs(3)
    ref = _node(ins, x, c).detach().clone()
    n = F_._VL.get('fwd_grads', 0)
    dpitch_bytes = ins[0].numel() * 4
    for mode in ('no_grad', 'no_leaf'):
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        if mode == 'no_grad':
            with torch.no_grad():
                out = _node(ins, x, c)
        else:
            out = _node([t.detach() for t in ins], x, c)
        torch.cuda.synchronize()
        assert out.grad_fn is None and torch.equal(out, ref), mode
        assert torch.cuda.memory_allocated() - m0 < dpitch_bytes // 2, mode      # (the targets and the 11 outputs: no dpitch, no ddur)
    assert F_._VL.get('fwd_grads', 0) == n
    # what such a forward may write: its 11 outputs, its sums and the chord targets it saves -- buffers of its own.  Not its inputs, not
    # the targets a plan hands in, not the early-exit word; a record does not exist (no gradient buffers: counted above)
    plan = _plan(x)
    held = [t.detach().clone() for t in ins] + [x.clone(), c.clone(), plan.pitch_t.clone(), plan.dur_t.clone(), plan.counts.clone()]
    early = _early()
    with torch.no_grad():
        out = F_.VaeLossFn.apply(*ins, x, c, BETA, W0, W1, False, plan)
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and _early() == early
    for a, b in zip(held, [t.detach() for t in ins] + [x, c, plan.pitch_t, plan.dur_t, plan.counts]):
        assert torch.equal(a, b)
    monkeypatch.setattr(F_, 'LOSS_COMPOSITE', False)
    with torch.no_grad():
        assert torch.equal(_node(ins, x, c), ref)


@pytest.mark.parametrize('B', [3, 35])
def test_logits_of_ignored_rows_are_never_read(B):
    """NaN in every logit row whose target is the ignore index: outputs and gradients as without, forward-written and recomputed"""
    ins, x, c = _loss_inputs(B)
    clean = _run(ins, x, c, _e0())
    ins2, _, _ = _loss_inputs(B)
    with torch.no_grad():
        dead_p = x[:, :, 1:, 0] == 130                                # [B,32,15]
        dead_d = x[:, :, 1:, 1:] == 2                                 # [B,32,15,5]
        assert dead_p.any() and dead_d.any() and not dead_p.all()
        ins2[0][dead_p] = float('nan')
        ins2[1][dead_d] = float('nan')
    assert torch.isnan(ins2[0]).any() and torch.isnan(ins2[1]).any()
    n = _early()
    _same(_run(ins2, x, c, _e0()), clean, 'forward-written:')
    assert _early() == n + 1
    _same(_run(ins2, x, c, _e0(), forget=True), clean, 'recomputed:')
    assert _early() == n + 1


def test_step_params_beta_reaches_both_directions_and_the_record(monkeypatch):
    """ptv_step_params: beta of a graph-replayed step is read from the device array by the forward (outputs, scales, record) and by the
    backward's comparison and scales.  (Replayed whole steps against eager ones: tests/test_gpu_model.py.)"""
    ins, x, c = _loss_inputs(3)
    sp = torch.tensor([0.85, 0.0, 0.0, 0.0], device=DEV)
    by_value = _run(ins, x, c, _e0(), beta=0.85)
    try:
        assert lib().ptv_step_params(sp.data_ptr()) == 0
        n = _early()
        out = _node(ins, x, c, beta=0.3)                              # (the by-value beta is overridden)
        rec = out.grad_fn.fused[1]
        grads = torch.autograd.grad(out, ins, _e0())
        assert _early() == n + 1
        assert torch.equal(rec[:11], _e0()) and rec[11].item() == sp[0].item() and rec[12:13].view(torch.int32).item() == 1
        _same((out.detach(), grads), by_value, 'step params:')
        _same(_launches(monkeypatch, ins, x, c, _e0(), beta=0.3), by_value, 'launches, step params:')
        # beta changes between the forward and the backward: the record no longer matches, the backward recomputes with the new one
        out = _node(ins, x, c, beta=0.3)
        sp[0] = 0.5
        grads = torch.autograd.grad(out, ins, _e0())
        assert _early() == n + 1
        for name, a, b in zip(NAMES, grads, _run(ins, x, c, _e0(), beta=0.5)[1]):
            assert torch.equal(a, b), 'beta moved: ' + name
    finally:
        lib().ptv_step_params(None)


@pytest.mark.parametrize('B', [1, 3])
def test_reparam_without_a_kl_sum_gives_the_same_z(B):
    gen = torch.Generator().manual_seed(40 + B)
    mu, eps = torch.randn(B, Z, generator=gen).to(DEV), torch.randn(B, Z, generator=gen).to(DEV)
    sd = torch.randn(B, Z, generator=gen).mul(0.2).exp().to(DEV)
    z_sum, z_none, kl = torch.zeros(B, Z, device=DEV), torch.zeros(B, Z, device=DEV), torch.zeros(1, device=DEV)
    F_.call('ptv_reparam_kl_fwd', ptr(mu), ptr(sd), ptr(eps), ptr(z_sum), Z, ptr(kl), B, Z, stream_ptr())
    F_.call('ptv_reparam_kl_fwd', ptr(mu), ptr(sd), ptr(eps), ptr(z_none), Z, None, B, Z, stream_ptr())
    assert kl.item() > 0 and z_none.abs().sum() > 0 and torch.equal(z_sum, z_none)
    ref = mu.double() + sd.double() * eps.double()
    assert (z_none.double() - ref).abs().max() <= 2.0 ** -22 * ref.abs().max()       # (two fp32 roundings of values below max |z|)
    assert torch.equal(F_.ReparamFn.apply(mu, sd, eps), z_none)
