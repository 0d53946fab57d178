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


def test_pointer_table_builders_put_every_tensor_in_its_named_slot():
    """each builder's array holds data_ptr() of the tensor given for name i at entry i and NULL for an omitted name, 21 entries without a
    block and 22 with one; the weight arrays over the model's parameters are the sequences include/ptvae_hip.h lists, written out here"""
    one = lambda: torch.zeros(1, device=DEV)
    for build, names in ((FF_.note_loop_io, FF_.NOTE_IO[:21]), (FF_.note_loop_io, FF_.NOTE_IO), (FF_.resum_io, FF_.RESUM_IO)):
        ts = {n: one() for n in names}
        assert len({t.data_ptr() for t in ts.values()}) == len(names)
        arr = build(**ts)
        assert len(arr) == len(names) and list(arr) == [ts[n].data_ptr() for n in names]
        some = {n: ts[n] for n in names[1::2]}
        arr = build(**some)
        assert len(arr) == (21 if build is FF_.note_loop_io and 'BLOCK' not in some else len(names))
        assert list(arr) == [some[n].data_ptr() if n in some else None for n in names[:len(arr)]]
    P = dict(TT.model().decoder.named_parameters())
    pk = FF_._free_packs(P, 1024)
    with torch.no_grad():
        tab0, tab = FF_.dur_tabs(P, torch.device(DEV))
    assert tab0.shape == (1, 192) and tab.shape == (2, 192) and tab0.dtype == tab.dtype == torch.float32
    want = [pk['wg_h'], pk['wg_t'], pk['wp'], pk['wd_h'], pk['wd_p'], pk['wdur'], P['dec_notes_gru.bias_hh_l0'], P['pitch_out_linear.bias'],
            P['dur_hid_linear.bias'], P['dec_dur_gru.bias_hh_l0'], tab0, tab, P['dur_out_linear.weight'], P['dur_out_linear.bias'],
            pk['w_embT'], P['note_embedding.bias']]
    assert list(FF_.note_loop_weights(P, pk, tab0, tab)) == [t.data_ptr() for t in want]
    want = [pk['e_ih'], pk['e_hh'], pk['e_ih_r'], pk['e_hh_r'], P['dec_notes_emb_gru.bias_ih_l0'], P['dec_notes_emb_gru.bias_hh_l0'],
            P['dec_notes_emb_gru.bias_ih_l0_reverse'], P['dec_notes_emb_gru.bias_hh_l0_reverse']]
    assert list(FF_.resum_weights(P, pk)) == [t.data_ptr() for t in want]
