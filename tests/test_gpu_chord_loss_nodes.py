"""The chord decoder nodes and the three loss nodes called directly (no model around them): the composite entry points against the same
launches sequenced from Python bit for bit, the named record every forward leaves as `grad_fn.saved_state`, and the launches the loss
nodes share (the chord cross-entropies of VaeLossFn and ChordLossFn)."""
import pytest
import torch

from helpers import full_params
from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd._lib import prec_code
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, I, Z = 512, 36, 256


_CHD_CPU = []


def _chd_params():
    if not _CHD_CPU:                                                 # (the full state dict is generated once for the module)
        sd = full_params()
        _CHD_CPU.extend(sd['chd_decoder.' + n].detach() for n in F_.CHD_PARAM_NAMES)
    return [torch.nn.Parameter(t.to(DEV)) for t in _CHD_CPU]


def _chd_inputs(B, T, seed=5):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(B, Z, generator=gen).to(DEV).requires_grad_(True)
    c_sm = torch.from_numpy(synth_batch(B, 40 + B)[1]).float().transpose(0, 1)[:T].contiguous().to(DEV)       # [T, B, 36] one-hot | bits | one-hot
    dl = [torch.randn(T, B, n, generator=gen).to(DEV) for n in (12, 24, 12)]
    return z, c_sm, dl


def _smallest_persistent_batch():
    return next((b for b in range(1, 2049) if F_.persist_supported(1, b, H, 8)), None)


@pytest.mark.parametrize('prec,batch,T', [('fp32', 3, 8), ('bf16', 3, 8), ('bf16', 3, 1), ('bf16', 'persistent', 8)])
def test_chord_decoder_node_composites_equal_the_launch_sequence_and_leave_a_named_state(prec, batch, T, monkeypatch):
    """ChordDecoderTFFn through ptv_chord_decoder_fwd / ptv_chord_decoder_bwd and launch by launch: the logits, dz and the 15 parameter
    gradients bit for bit, the call counters, the ChordDecoderState on the node and its release.  bf16 reads the optimiser's bf16 weight
    shadows; T = 1 has no token copy and no persistent launch; 'persistent' is the smallest batch whose BPTT the persistent kernel takes"""
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam, refresh_weight_shadows
    Bp = _smallest_persistent_batch()
    assert Bp is not None
    B = Bp if batch == 'persistent' else batch
    if batch != 'persistent' and Bp <= B:
        monkeypatch.setattr(F_, 'PERSIST', '0')                      # (the non-persistent leg where even B = 3 would be taken)
    params = _chd_params()
    opt = FusedClipAdam(params, lr=1e-3)
    z, c_sm, dl = _chd_inputs(B, T)
    code = prec_code(prec)
    res = {}
    for comp in (True, False):
        monkeypatch.setattr(F_, 'CHD_COMPOSITE', comp)
        monkeypatch.setattr(F_, 'CHD_BWD_COMPOSITE', comp)
        opt.zero_grad()
        refresh_weight_shadows()
        n_fwd, n_bwd = F_._DTF.get('chd_calls', 0), F_._CDB.get('calls', 0)
        root, chroma, bass = F_.ChordDecoderTFFn.apply(z, c_sm, code, *params)
        st = root.grad_fn.saved_state
        assert isinstance(st, F_.ChordDecoderState) and (st.T, st.B, st.H, st.I, st.prec) == (T, B, H, I, code)
        assert st.gates.dtype == F_._act_dtype(code, H) and st.hall.shape == (T + 1, B, H) and st.toks.shape == (T, B, I)
        assert (root.shape, chroma.shape, bass.shape) == ((T, B, 12), (T, B, 24), (T, B, 12))
        n_sync = len(F_._PERSIST_SYNC)
        grads = torch.autograd.grad((root, chroma, bass), [z] + params, dl)
        assert len(F_._PERSIST_SYNC) - n_sync == int(batch == 'persistent')      # one persistent BPTT, or none
        assert root.grad_fn.saved_state is None
        assert F_._DTF.get('chd_calls', 0) - n_fwd == int(comp) and F_._CDB.get('calls', 0) - n_bwd == int(comp)
        res[comp] = [t.detach().clone() for t in (root, chroma, bass) + tuple(grads)]
        del grads, st
        F_.persist_check()
    assert len(res[True]) == 3 + 1 + 15
    for name, a, b in zip(['root', 'chroma', 'bass', 'dz'] + F_.CHD_PARAM_NAMES, res[True], res[False]):
        assert torch.isfinite(a).all() and a.abs().sum() > 0, name
        assert torch.equal(a, b), name


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_chord_decoder_step_node_backward_is_chord_decoder_bwd(prec):
    """ChordDecoderStepFn (scheduled sampling: coins T F T F ...) leaves the same ChordDecoderState; its backward returns what
    chord_decoder_bwd returns for that state and those incoming gradients, through the composite like the teacher-forced node's"""
    B, T = 3, 8
    params = _chd_params()
    z, c_sm, dl = _chd_inputs(B, T, seed=6)
    code = prec_code(prec)
    root, chroma, bass = FF_.ChordDecoderStepFn.apply(z, c_sm, [True, False] * 4, None, code, *params)
    st = root.grad_fn.saved_state
    assert isinstance(st, F_.ChordDecoderState) and (st.T, st.B, st.H, st.I, st.prec) == (T, B, H, I, code)
    assert st.gates.dtype == F_._act_dtype(code, H)
    n = F_._CDB.get('calls', 0)
    got = torch.autograd.grad((root, chroma, bass), [z] + params, dl)
    assert F_._CDB.get('calls', 0) - n == 1 and root.grad_fn.saved_state is None
    dz, G = F_.chord_decoder_bwd(dict(zip(F_.CHD_PARAM_NAMES, params)), st, z.detach(), *dl)       # (no optimiser: fresh zeroed gradient buffers)
    assert F_._CDB.get('calls', 0) - n == 2
    assert len(got) == 16 and torch.equal(got[0], dz) and dz.abs().sum() > 0
    for name, g in zip(F_.CHD_PARAM_NAMES, got[1:]):
        assert torch.isfinite(g).all() and g.abs().sum() > 0, name
        assert torch.equal(g, G[name]), name
    F_.persist_check()


# ---- loss nodes -------------------------------------------------------------------------------------------------------------------
def _loss_inputs(B):
    """logits as run() returns them: API-shaped views of step-major buffers (the pitch rows padded to 136 floats), leaves that take a gradient"""
    gen = torch.Generator().manual_seed(17 + B)
    rn = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    leaf = lambda t: t.detach().requires_grad_(True)
    M = 15 * 32 * B
    pitch = leaf(rn(M, 136)[:, :130].view(15, 32, B, 130).permute(2, 1, 0, 3))
    dur = leaf(rn(M, 5, 2).view(15, 32, B, 5, 2).permute(2, 1, 0, 3, 4))
    dists = [leaf(rn(B, Z)), leaf(rn(B, Z).mul(0.2).exp()), leaf(rn(B, Z)), leaf(rn(B, Z).mul(0.2).exp())]
    root, bass = leaf(rn(8, B, 12).transpose(0, 1)), leaf(rn(8, B, 12).transpose(0, 1))
    chroma = leaf(rn(8, B, 24).view(8, B, 12, 2).transpose(0, 1))
    x, c, _ = synth_batch(B, 300 + B)
    return [pitch, dur] + dists + [root, chroma, bass], torch.from_numpy(x).to(DEV).long(), torch.from_numpy(c).to(DEV).float()


def _vae_loss(ins, x, c, gout, weighted=False):
    out = F_.VaeLossFn.apply(*ins, x, c, 0.3, 0.7, 0.4, weighted, None)
    st = out.grad_fn.saved_state
    assert isinstance(st, F_.LossState) and st.sm_p is True and st.sm_c is True and (st.gcnt is not None) == weighted
    assert st.scal == (0.3, 0.7, 0.4, float(x.shape[0] * Z), float(x.shape[0] * 8), float(x.shape[0] * 96))
    return out.detach().clone(), [g.clone() for g in torch.autograd.grad(out, ins, gout)]


@pytest.mark.parametrize('B', [3, 4])
def test_loss_nodes_composite_equals_launches_and_share_the_chord_launches(B, monkeypatch):
    """VaeLossFn through ptv_vae_loss_fwd / ptv_vae_loss_bwd and launch by launch: 11 outputs and nine gradients bit for bit, one call each
    way exactly when the switch is on, none for the weighted duration form.  ChordLossFn's four values are VaeLossFn's out[7:11], and its
    three gradients VaeLossFn's for a gradient of one on those four outputs alone: the same launches, run once from each node"""
    ins, x, c = _loss_inputs(B)
    gout = torch.rand(11, generator=torch.Generator().manual_seed(3)).to(DEV) + 0.5
    res = {}
    for comp in (True, False):
        monkeypatch.setattr(F_, 'LOSS_COMPOSITE', comp)
        n = F_._VL.get('calls', 0), F_._VL.get('bwd_calls', 0)
        res[comp] = _vae_loss(ins, x, c, gout)
        assert (F_._VL.get('calls', 0) - n[0], F_._VL.get('bwd_calls', 0) - n[1]) == (int(comp), int(comp))
    assert torch.isfinite(res[True][0]).all() and torch.equal(res[True][0], res[False][0])
    for i, (a, b) in enumerate(zip(res[True][1], res[False][1])):
        assert a.shape == ins[i].shape and torch.isfinite(a).all() and a.abs().sum() > 0, i
        assert torch.equal(a, b), i
    monkeypatch.setattr(F_, 'LOSS_COMPOSITE', True)
    n = F_._VL.get('calls', 0), F_._VL.get('bwd_calls', 0)
    out_w, grads_w = _vae_loss(ins, x, c, gout, weighted=True)
    assert (F_._VL.get('calls', 0), F_._VL.get('bwd_calls', 0)) == n
    assert torch.isfinite(out_w).all() and all(torch.isfinite(g).all() for g in grads_w)
    assert torch.equal(out_w[4:], res[True][0][4:]) and torch.equal(out_w[2], res[True][0][2])          # (only the duration term and the sums over it differ)
    assert not torch.equal(out_w[3], res[True][0][3])
    # ChordLossFn beside VaeLossFn
    chord = ins[6:9]
    out4 = F_.ChordLossFn.apply(*chord, c)
    st = out4.grad_fn.saved_state
    assert isinstance(st, F_.LossState) and st.sm_c is True and st.sm_p is None and st.gcnt is None
    assert torch.equal(out4.detach(), res[True][0][7:11]) and torch.equal(out4.detach(), res[False][0][7:11])
    g3 = torch.autograd.grad(out4, chord, torch.ones(4, device=DEV))
    only_chord = torch.zeros(11, device=DEV)
    only_chord[7:11] = 1.0
    monkeypatch.setattr(F_, 'LOSS_COMPOSITE', False)
    _, grads = _vae_loss(ins, x, c, only_chord)
    for name, a, b in zip(('droot', 'dchroma', 'dbass'), g3, grads[6:9]):
        assert a.abs().sum() > 0 and torch.equal(a, b), name


@pytest.mark.parametrize('B', [3, 4])
def test_recon_loss_node_equals_the_vae_loss_nodes_reconstruction_terms(B, monkeypatch):
    """ReconLossFn = (w0 pl + w1 dl, pl, dl) is out[1:4] of VaeLossFn for the same logits and x, plain and weighted; it leaves a LossState"""
    ins, x, c = _loss_inputs(B)
    monkeypatch.setattr(F_, 'LOSS_COMPOSITE', False)
    for weighted in (False, True):
        out3 = F_.ReconLossFn.apply(ins[0], ins[1], x, 0.7, 0.4, weighted)
        st = out3.grad_fn.saved_state
        assert isinstance(st, F_.LossState) and st.sm_p is True and st.sm_c is None and (st.gcnt is not None) == weighted
        g3 = torch.rand(3, generator=torch.Generator().manual_seed(4)).to(DEV) + 0.5
        g11 = torch.zeros(11, device=DEV)
        g11[1:4] = g3
        out11, grads = _vae_loss(ins, x, c, g11, weighted)
        assert torch.equal(out3.detach(), out11[1:4])
        for a, b in zip(torch.autograd.grad(out3, ins[:2], g3), grads[:2]):
            assert a.abs().sum() > 0 and torch.equal(a, b)
