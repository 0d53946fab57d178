"""GPU: the host paths of the free-running decode agree bit for bit.  For each of the four kinds of a decode (argmax, sampled, truncated,
constrained), with and without kept steps, at B = 17 -- two 16-sample panels, the second with one live row: the smallest batch with a ragged
panel and a cluster choice -- the decode through ptv_decoder_free_fwd equals the same launches sequenced from Python, and the eager decode
equals its graph replay, in the pitch logits, the duration logits and the grid.  The model, the latents and the patching helper are
those of tests/test_gpu_truncated_sampling.py."""
import functools

import pytest
import torch

import test_gpu_truncated_sampling as TT
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = TT.DEV
B = 17
KINDS = {'argmax': None, 'sampled': dict(), 'truncated': dict(top_k=8, top_p=0.9), 'constrained': dict(ascending=True, mask=True)}


@functools.lru_cache(maxsize=None)
def inputs():
    """(z [17, 512], the chord-tone mask [17, 32, 4], the Keep of the first 16 steps of a synthetic grid): made once, never modified"""
    m = TT.model()
    x, c, _ = (torch.from_numpy(a).to(DEV) for a in synth_batch(B, 5))
    return TT.latents(32)[:B].contiguous(), m.pitch_mask(c=c.float(), lo=24, hi=96), m.keep(x.long(), range(16))


def block_of(kind):
    kw = KINDS[kind]
    if kw is None:
        return None
    kw = dict(kw)
    mask = inputs()[1] if kw.pop('mask', False) else None
    return FF_.sampling_block(DEV, TT.T_PITCH, TT.T_DUR, seed=TT.SEED, draw=TT.DRAW, pitch_mask=mask, **kw)


def decode(kind, keep, **attrs):
    """one inference decode -> clones of (pitch logits, duration logits, grid)"""
    m = TT.model()
    z, _, kp = inputs()
    with TT.patched(attrs), torch.no_grad():
        pitch, dur = m.decoder(z, True, None, None, 0., 0., sampling=block_of(kind), keep=kp if keep else None)
        out = pitch.clone(), dur.clone(), m.decoder.last_xhat.clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('keep', [False, True], ids=['free', 'keep16'])
@pytest.mark.parametrize('kind', list(KINDS))
def test_composite_python_sequencing_and_graph_replay_decode_the_same_bits(kind, keep):
    m = TT.model()
    assert FF_.block_kind(block_of(kind)).kind == list(KINDS).index(kind)
    n = FF_._DFF.get('calls', 0)
    on = decode(kind, keep, FREE_COMPOSITE=True)
    assert FF_._DFF.get('calls', 0) == n + 1                      # the one C call ran ...
    off = decode(kind, keep, FREE_COMPOSITE=False)
    assert FF_._DFF.get('calls', 0) == n + 1                      # ... and then did not
    assert on[0].shape == (B, 32, 15, 130) and on[1].shape == (B, 32, 15, 5, 2) and on[2].shape == (B, 32, 16, 6)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    m.decoder._graphs.clear()
    m.decoder.use_graph = True
    try:
        before = m.decoder.graph_captures
        first = decode(kind, keep)                                # captures, replays once
        again = decode(kind, keep)                                # replays the capture with refreshed static inputs
        assert m.decoder.graph_captures == before + 1 and len(m.decoder._graphs) == 1
        (key,) = m.decoder._graphs
        assert len(key) == (6 if keep else 5) and key[4] == FF_.block_kind(block_of(kind)).kind and key[0] == B
    finally:
        m.decoder.use_graph = False
        m.decoder._graphs.clear()
    for a, b, c in zip(on, first, again):
        assert torch.equal(a, b) and torch.equal(a, c)
