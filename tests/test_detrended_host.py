"""Host side of the detrended-texture-encoder variant (ptv_embed_multihot_fwd, ptv_multihot_bytes_rows, DisentangleVAE.init_model_detrended,
the trainer's four-tensor batches): symbols, argument checks that return before any launch, state_dict parity with the reference's
train.py:31-39 wiring (names and shapes recorded in tests/golden/detrended_b4.npz), and the signature-level rules.  No GPU."""
import ctypes
import types

import numpy as np
import pytest
import torch

import dataset_ref as R
from helpers import load_npz
from polyphonic_chord_texture_disentanglement_amd import _lib, model as M
from polyphonic_chord_texture_disentanglement_amd.ptvae import PtvaeEncoder, TextureEncoder
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

NEW_SYMBOLS = ('ptv_embed_multihot_fwd', 'ptv_multihot_bytes_rows')


@pytest.fixture(scope='module')
def fixture():
    return load_npz('detrended_b4.npz')


@pytest.fixture(scope='module')
def detrended_model():
    return M.DisentangleVAE.init_model_detrended(torch.device('cpu'))


def test_symbols_are_declared_and_exported():
    assert set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    l = _lib.lib()
    for n in NEW_SYMBOLS:
        assert getattr(l, n) is not None
    assert l.ptv_abi_version() == _lib.EXPECTED_ABI


def test_argument_errors_return_before_any_launch():
    """every refusal is decided on the host: the pointers are host buffers that a launch would fault on, and no device is needed"""
    l = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 63) // 64 * 64                  # 64-byte aligned, non-NULL
    mh, W, bias, emb, lengths = p, p + 4096, p + 8192, p + 16384, p + 32768
    f = l.ptv_embed_multihot_fwd
    good = dict(mh=mh, W=W, bias=bias, emb=emb, lengths=lengths, B=2, E=128, S=32, N=16, K=39, pad_col=3)

    def rc(**kw):
        a = dict(good, **kw)
        return f(a['mh'], a['W'], a['bias'], a['emb'], a['lengths'], a['B'], a['E'], a['S'], a['N'], a['K'], a['pad_col'], None)
    for name in ('mh', 'W', 'bias', 'emb'):
        assert rc(**{name: None}) != 0, name
    assert rc(B=0) != 0 and rc(B=-3) != 0
    assert rc(S=0) != 0 and rc(N=0) != 0 and rc(K=0) != 0
    assert rc(K=65) != 0                                          # K <= 64
    assert rc(E=260) != 0 and rc(E=0) != 0 and rc(E=126) != 0     # E <= 256, whole 16-byte stores
    assert rc(K=64, E=1024) != 0                                  # (E bound; K * E * 4 = 256 KB is over the 150 KB of staged weight too)
    assert rc(N=300, K=64) != 0                                   # one (sample, step) slab over the staged-tile bound
    assert rc(pad_col=-1) != 0                                    # lengths wanted, no column named
    assert rc(pad_col=39) != 0
    assert rc(emb=emb + 4) != 0                                   # misaligned output
    g = l.ptv_multihot_bytes_rows
    for bf in (0, 1):
        assert g(None, emb, 40, 2, 32, 16, 39, bf, None) != 0
        assert g(mh, None, 40, 2, 32, 16, 39, bf, None) != 0
        assert g(mh, emb, 40, 0, 32, 16, 39, bf, None) != 0
        assert g(mh, emb, 38, 2, 32, 16, 39, bf, None) != 0       # ld < K
        assert g(mh, emb, 40, 2, 0, 16, 39, bf, None) != 0


def test_init_model_detrended_has_the_reference_state_dict(fixture, detrended_model):
    """names, order and shapes of train.py:31-39's model, as the reference's own state_dict gave them"""
    sd = detrended_model.state_dict()
    assert list(sd.keys()) == [str(n) for n in fixture['names']]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in fixture['shapes']]
    enc = detrended_model.rhy_encoder
    assert isinstance(enc, PtvaeEncoder) and enc.note_size == 39 and enc.z_size == 256
    assert detrended_model.detrended and detrended_model.name == 'disvae-nozoth'
    assert not M.DisentangleVAE.init_model(torch.device('cpu')).detrended


def _trainer(model):
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import TrainingVAE
    tr = TrainingVAE.__new__(TrainingVAE)
    tr.model, tr.device = model, torch.device('cpu')
    return tr


def test_batch_to_inputs_arity_follows_the_encoder_type(fixture, detrended_model):
    x, c, pr = (torch.from_numpy(a) for a in synth_batch(4, int(fixture['data_seed'])))
    z = torch.zeros(4, 1)
    dt = torch.from_numpy(fixture['dt_x'])
    conv = types.SimpleNamespace(rhy_encoder=TextureEncoder(8, 8, 4, 1), detrended=False)
    out = _trainer(conv)._batch_to_inputs((z, z, pr, x, c, dt))
    assert len(out) == 3 and out[0].dtype == torch.int64 and out[2].dtype == torch.float32
    out = _trainer(detrended_model)._batch_to_inputs((z, z, pr, x, c, dt.float()))          # (a loader that cast it, as the reference's does)
    assert len(out) == 4 and out[3].dtype == torch.uint8 and torch.equal(out[3], dt)
    # a placeholder in the sixth slot: dt_x is computed by the device kernel -- which refuses the CPU loudly, nothing is made up
    with pytest.raises(RuntimeError, match='no CPU'):
        _trainer(detrended_model)._batch_to_inputs((z, z, pr, x, c, z))


def test_graphed_step_is_not_entered_for_four_inputs(monkeypatch):
    from polyphonic_chord_texture_disentanglement_amd import graph_step
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import TrainingVAE
    built = []
    monkeypatch.setattr(graph_step, 'GraphedTrainStep', lambda *a, **k: built.append(a) or object())
    monkeypatch.delenv('PTV_GRAPH_STEP', raising=False)
    tr = TrainingVAE.__new__(TrainingVAE)
    tr.graph_step, tr.grad_sync, tr.model = True, None, None
    tr.opt_scheduler = types.SimpleNamespace(optimizer=types.SimpleNamespace(clip_and_step=lambda c: None), clip=1)
    t = types.SimpleNamespace(is_cuda=True, shape=(8, 32, 16, 6))
    params = dict(tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
    assert tr._graphed((t, t, t, t), params) is None and not built
    assert tr._graphed((t, t, t), params) is not None and len(built) == 1      # (the three-input step still replays)


def test_data_parallel_training_of_the_variant_is_refused_at_construction(detrended_model):
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import TrainingVAE
    with pytest.raises(NotImplementedError, match='data parallelism'):
        TrainingVAE(torch.device('cpu'), detrended_model, True, None, None, None, None, None, 1)


def test_loss_passes_the_fourth_tensor_on_only_for_the_detrended_variant(monkeypatch, detrended_model):
    x, c, pr = (torch.from_numpy(a) for a in synth_batch(2, 5))
    dt = torch.zeros(2, 32, 16, 39, dtype=torch.uint8)
    for m, want in ((M.DisentangleVAE.init_model(torch.device('cpu')), False), (detrended_model, True)):
        seen = {}

        def run(*a, **k):
            seen['a'], seen['k'] = a, k
            return ()
        monkeypatch.setattr(m, 'run', run)
        monkeypatch.setattr(m, 'loss_function', lambda *a, **k: 'losses')
        with torch.no_grad():
            assert m.loss(x, c, pr, dt, 1., 0.5, 0.25, beta=0.2) == 'losses'
        assert seen['a'][3:] == (1., 0.5, 0.25)
        assert ('dt_x' in seen['k']) == want
        if want:
            assert seen['k']['dt_x'] is dt
            with torch.no_grad():
                m.loss(x, c, pr, 1., 1., 1.)
            assert seen['k']['dt_x'] is None                     # (run() then computes it on the device)


def test_texture_input_of_the_wrong_kind_is_a_value_error(detrended_model):
    c = torch.zeros(2, 8, 36)
    for bad in (torch.zeros(2, 32, 128), torch.zeros(2, 32, 16, 39), torch.zeros(2, 32, 16, 38, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='dt_x'):
            detrended_model.inference(bad, c, sample=False)
        with pytest.raises(ValueError, match='dt_x'):
            detrended_model.inference_encode(bad, c)
        with pytest.raises(ValueError, match='dt_x'):
            detrended_model.swap(bad, bad, c, c, True, True)
    for name in ('inference_encode', 'inference', 'swap', 'posterior_sample', 'prior_sample', 'interp'):
        assert 'dt_x' in getattr(M.DisentangleVAE, name).__doc__, name


def test_get_loaders_forwards_slots():
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import MusicDataLoaders
    bank = (torch.zeros(20, 32, 128, dtype=torch.uint8), torch.zeros(20, 8, 14))
    with pytest.raises(ValueError, match='slots'):                # a (pr, chord14) bank has no notes: DeviceBatcher got the slots and refuses
        MusicDataLoaders.get_loaders(1, 4, 4, device_bank=bank, slots=('dt_x',))
    ld = MusicDataLoaders.get_loaders(1, 4, 4, n_train_batch=1, slots=('dt_x',))      # synthetic: placeholders
    assert len(ld.train_loader) == 1


def test_fixture_dt_x_and_lengths_are_consistent_with_its_inputs(fixture):
    """oracle/data_oracle.py has no detrend; tests/dataset_ref.py restates it (checked against the reference in the dataset tests)"""
    x, c, _ = synth_batch(int(fixture['B']), int(fixture['data_seed']))
    dt = fixture['dt_x']
    assert dt.dtype == np.uint8 and dt.shape == (4, 32, 16, 39)
    for b in range(4):
        assert np.array_equal(dt[b], R.detrend(x[b], c[b])), b
    assert np.array_equal(fixture['lengths'], 16 - (x[..., 0] == 130).sum(-1))
    assert np.array_equal(fixture['lengths'], (dt[..., 3] == 0).sum(-1))
    assert fixture['losses'].shape == (11,) and fixture['mu_rhy'].shape == (4, 256)
