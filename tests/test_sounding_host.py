"""CPU: the host surface of sounding= (INTEGRATION.md "Sounding state"): every bad value is a ValueError before anything touches the GPU,
sounding is one of DECODE_KEYS and reaches every entry point through _request, the promotion rules follow the keep family, and
DecodeRequest.tiled tiles its tables."""
import numpy as np
import pytest
import torch

from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M


def host_sounding(batch=3, no_restrike=False, ceiling=False, floor=False, rows=1):
    """a Sounding over host tensors: what the promotion rules and tiled() read; no entry point accepts it (its tables are not on a GPU)"""
    u8 = lambda v: torch.full((rows, 32), v, dtype=torch.uint8)
    k = (torch.arange(rows * 32) % 7).to(torch.uint8).view(rows, 32) if ceiling else u8(0)
    return FF_.Sounding(torch.tensor([int(no_restrike)], dtype=torch.int32), k, u8(2 if floor else 0), u8(1), batch, no_restrike, ceiling,
                        floor)


def test_bad_values_are_value_errors_before_the_gpu():
    t32 = torch.full((4, 32), 3, dtype=torch.int32)
    for bad in (dict(), dict(no_restrike=False), dict(no_restrike=1), dict(no_restrike='yes'), dict(max_sounding=0), dict(max_sounding=128),
                dict(max_sounding=-1), dict(max_sounding=True), dict(max_sounding=4.0), dict(max_sounding='4'), dict(min_sounding=-1),
                dict(min_sounding=16), dict(min_sounding=False), dict(min_sounding=1.5), dict(max_sounding=t32), dict(min_sounding=t32),
                dict(max_sounding=4, steps=[32]), dict(max_sounding=4, steps=[-1]), dict(max_sounding=4, steps=7),
                dict(max_sounding=4, steps=torch.ones(4, 32, dtype=torch.bool)), dict(max_sounding=4, batch=0), dict(max_sounding=4, batch=True),
                dict(max_sounding=4, batch=2.0), dict(steps=range(8))):
        with pytest.raises(ValueError):
            FF_.build_sounding('cuda', **dict(dict(batch=4) if 'batch' not in bad else {}, **bad))
    with pytest.raises(ValueError):
        FF_.build_sounding('cuda', max_sounding=4)                       # nothing tells the batch
    with pytest.raises(ValueError):
        FF_.build_sounding('cpu', no_restrike=True, batch=4)             # the state lives on the device
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    with pytest.raises(ValueError):
        m.sounding(max_sounding=200, batch=4)
    with pytest.raises(ValueError):
        m.sounding(no_restrike=True, batch=4)                            # a model on the host


def test_sounding_is_a_decode_key_of_every_entry_point():
    assert 'sounding' in M.DECODE_KEYS and 'rows' in M.DECODE_KEYS[:-2] and 'sounding' in M.DECODE_KEYS[:-2]
    assert M.DECODE_KEYS[-2:] == ('pitch_mask', 'keep')
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    m._sample_draws = 5
    m.train()
    z = torch.zeros(3, 256)
    tex, c = torch.zeros(3, 32, 128), torch.zeros(3, 8, 36)
    for bad in ('a string', host_sounding(3), host_sounding(4)):
        with pytest.raises(ValueError) as direct:
            m._request(3, sounding=bad)
        kw = dict(sounding=bad)
        for fn in (lambda: m.inference_decode(z, z, **kw), lambda: m.decode_to_inputs(z, z, **kw), lambda: m.decode_logprob(z, z, **kw),
                   lambda: m.decode_best_of(z, z, 2, temperature=1.0, **kw), lambda: m.reencode(z, z, **kw),
                   lambda: m.inference(tex, c, False, **kw), lambda: m.swap(tex, tex, c, c, True, False, **kw),
                   lambda: m.posterior_sample(tex, c, scale=2.0, **kw), lambda: m.prior_sample(tex, c, **kw),
                   lambda: m.interp(tex, c, tex, c, int_count=1, **kw)):
            with pytest.raises(ValueError) as got:
                fn()
            assert str(got.value) == str(direct.value)
            assert m._sample_draws == 5 and m.training                   # before eval(), before the draw counter moves


def test_check_sounding():
    FF_.check_sounding(None)
    for bad in (3, (1, 2), host_sounding(3)):
        with pytest.raises(ValueError):
            FF_.check_sounding(bad)
    with pytest.raises(ValueError):
        M.DisentangleVAE.init_model(torch.device('cpu')).decoder(torch.zeros(3, 512), False, None, None, 0., 0., sounding=host_sounding(3))


def request_of(m, snd, **kw):
    """the DecodeRequest _request would make of a device Sounding (a host one stops at check_sounding)"""
    base = m._request(snd.batch, **kw)
    return base._replace(kw=dict(base.kw, sounding=snd))


def test_promotion_follows_the_keep_family():
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    cons_argmax = FF_.sampling_words(0.0, 0.0, 0, 0, 0, ascending=False)
    for snd in (host_sounding(no_restrike=True), host_sounding(floor=True), host_sounding(no_restrike=True, ceiling=True, floor=True)):
        assert snd.needs_constrained
        # no temperature: the constrained argmax, an `ascending` nobody gave becomes False; the draw counter stays
        assert m._sampling_words(request_of(m, snd)) == cons_argmax and m._sample_draws == 0
        w = m._sampling_words(request_of(m, snd, temperature=0.5, seed=9, draw=2))
        assert w == FF_.sampling_words(0.5, None, 9, 2, 0, ascending=False) and len(w) == 8
        w = m._sampling_words(request_of(m, snd, temperature=0.5, seed=9, draw=2, ascending=True))
        assert w == FF_.sampling_words(0.5, None, 9, 2, 0, ascending=True)                       # a given `ascending` stays
    cap = host_sounding(ceiling=True)
    assert not cap.needs_constrained and cap.needs_force and not host_sounding(no_restrike=True).needs_force
    assert m._sampling_words(request_of(m, cap)) is None                                         # a ceiling alone: the plain argmax
    assert m._sampling_words(request_of(m, cap, temperature=0.5, seed=9, draw=2)) == FF_.sampling_words(0.5, None, 9, 2, 0)
    assert m._sampling_words(request_of(m, cap, temperature=0.5, seed=9, draw=2, top_k=4)) == FF_.sampling_words(0.5, None, 9, 2, 0, top_k=4)
    assert m._sample_draws == 0


def test_tiled_and_sliced():
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    one = host_sounding(3, ceiling=True, rows=1)
    per = host_sounding(3, no_restrike=True, ceiling=True, rows=3)
    req = request_of(m, one, temperature=1.0)
    t = req.tiled(4)
    assert t.batch == 12 and t.kw['sounding'].batch == 12 and t.kw['sounding'].max_sounding is one.max_sounding       # one row serves all
    assert req.kw['sounding'] is one and t.kw['temperature'] == 1.0
    t = request_of(m, per, temperature=1.0).tiled(4).kw['sounding']
    assert t.batch == 12 and t.control is per.control and (t.no_restrike, t.ceiling, t.floor) == (True, True, False)
    for a, b in zip(t.tables(), per.tables()):
        assert tuple(a.shape) == (12, 32) and np.array_equal(a.numpy(), np.tile(b.numpy(), (4, 1)))                # candidate k of row b: k * B + b
    s = per.sliced(1, 3)
    assert s.batch == 2 and np.array_equal(s.max_sounding.numpy(), per.max_sounding.numpy()[1:3]) and s.max_sounding.is_contiguous()
    assert one.sliced(1, 3).max_sounding is one.max_sounding
    for lo, hi in ((-1, 2), (2, 2), (0, 4)):
        with pytest.raises(ValueError):
            per.sliced(lo, hi)
    plain = m._request(3)
    assert plain.tiled(2).kw is plain.kw and plain.kw['sounding'] is None
