"""Fixture of the detrended-texture-encoder variant, recorded from the REFERENCE itself (build container only):
tests/golden/detrended_b4.npz.

Imports `/root/reference` unmodified (stubs and recorders of make_golden.py).  Nothing of the reference is copied: the file holds
seeds, inputs and recorded results only.

The model is the wiring of the reference's train.py:31-39 (`disvae-nozoth`): RnnEncoder(36, 1024, 256), PtvaeEncoder(z_size=256,
max_pitch=39 - 8, min_pitch=0) as the texture encoder (note_size 34 + 5 = 39), RnnDecoder(z_dim=256), PtvaeDecoder(dec_dur_hid_size=64,
z_size=512), with filler weights `fill_state_dict(shapes, 1234)` over ITS state_dict (names and shapes are stored, no weights).
`DisentangleVAE.run` cannot execute that wiring (it hands the piano-roll to PtvaeEncoder.forward), so the forward
is composed here the way the script intends it, from the reference's own methods:

    dt_x[b]  = dataset.detrend_pianotree(x[b], c[b])                                   (dataset.py:123-168, per sample)
    dist_rhy = rhy_encoder.encoder(dt_x.float(), decoder.get_len_index_tensor(x))[0]   (ptvae.py:190-206)
    dist_chd = chd_encoder(c);  z_chd, z_rhy = rsample() in that order (recorded eps)
    decoder / chd_decoder teacher-forced (tfr = 1), loss_function(beta 0.1, weights (1, 0.5))

Stored: B, data_seed (x, c, pr_mat = synth_batch(B, data_seed)), dt_x (uint8), lengths, eps, both means and scales, the 11 losses, and
per parameter the gradient norm, max |g| and a 64-element slice at stored positions (as full_tf1_b4_gslices.npz).

    python tests/golden/make_golden_r9.py        # needs /root/reference; about a minute
"""
import os
import sys
import warnings
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden_r4 import grad_slices  # noqa: E402

from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch, fill_state_dict  # noqa: E402

B, DATA_SEED, RNG_SEED, FILL_SEED = 4, 520, 20, 1234
BETA, WEIGHTS = 0.1, (1, 0.5)


def build(ref_model, ref_ptvae):
    """train.py:31-39 on the CPU"""
    torch.manual_seed(0)
    dev = torch.device('cpu')
    chd_encoder = ref_ptvae.RnnEncoder(36, 1024, 256)
    rhy_encoder = ref_ptvae.PtvaeEncoder(device=dev, z_size=256, max_pitch=39 - 8, min_pitch=0)
    chd_decoder = ref_ptvae.RnnDecoder(z_dim=256)
    pt_decoder = ref_ptvae.PtvaeDecoder(note_embedding=None, dec_dur_hid_size=64, z_size=512)
    pt_decoder.device = dev
    m = ref_model.DisentangleVAE('disvae-nozoth', dev, chd_encoder, rhy_encoder, pt_decoder, chd_decoder)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    m.load_state_dict(fill_state_dict(shapes, seed=FILL_SEED))
    return m, shapes


def main():
    ref_model, ref_ptvae, _ = mg.import_reference()
    import dataset as ref_dataset
    warnings.simplefilter('ignore')
    m, shapes = build(ref_model, ref_ptvae)
    x, c, pr = synth_batch(B, DATA_SEED)
    dt_x = np.stack([ref_dataset.detrend_pianotree(x[b], c[b]) for b in range(B)])
    assert dt_x.shape == (B, 32, 16, 39) and dt_x.min() >= 0 and dt_x.max() <= 2
    xt, ct = torch.from_numpy(x), torch.from_numpy(c)
    m.zero_grad()
    torch.manual_seed(RNG_SEED)
    with mg.EpsRecorder() as er, mg.CoinRecorder(RNG_SEED):
        embedded_x, lengths = m.decoder.emb_x(xt)
        dist_chd = m.chd_encoder(ct)
        dist_rhy, _ = m.rhy_encoder.encoder(torch.from_numpy(dt_x).float(), m.decoder.get_len_index_tensor(xt))
        z_chd, z_rhy = dist_chd.rsample(), dist_rhy.rsample()                 # chd first (train_utils.py:33-34)
        pitch_outs, dur_outs = m.decoder(torch.cat([z_chd, z_rhy], dim=-1), False, embedded_x, lengths, 1., 1.)
        root, chroma, bass = m.chd_decoder(z_chd, False, 1., ct)
        losses = m.loss_function(xt, ct, pitch_outs, dur_outs, dist_chd, dist_rhy, root, chroma, bass, BETA, list(WEIGHTS))
    losses[0].backward()
    # the <pad> cell of dt_x (is_note class 3) counts what get_len_index_tensor counts
    assert np.array_equal(16 - dt_x[..., 3].sum(-1), lengths.numpy())
    out = OrderedDict(B=np.int64(B), data_seed=np.int64(DATA_SEED), beta=np.float64(BETA), weights=np.array(WEIGHTS, dtype=np.float64),
                      names=np.array(list(shapes.keys())), shapes=np.array([str(s) for s in shapes.values()]),
                      dt_x=dt_x.astype(np.uint8), lengths=lengths.numpy().astype(np.int16),
                      eps_chd=er.eps[0].numpy(), eps_rhy=er.eps[1].numpy(),
                      mu_chd=dist_chd.mean.detach().numpy(), std_chd=dist_chd.scale.detach().numpy(),
                      mu_rhy=dist_rhy.mean.detach().numpy(), std_rhy=dist_rhy.scale.detach().numpy(),
                      losses=np.array([l.item() for l in losses], dtype=np.float64))
    res = OrderedDict()
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        res['grad.' + n] = p.grad.detach().numpy()
        out['gnorm.' + n] = np.float64(p.grad.double().pow(2).sum().sqrt().item())
    grad_slices(res, out)
    path = os.path.join(HERE, 'detrended_b4.npz')
    np.savez_compressed(path, **out)
    print('losses', out['losses'])
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 200000


if __name__ == '__main__':
    main()
