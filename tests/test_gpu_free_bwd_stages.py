"""functional_free.DecoderStepFn.backward stage by stage: the decoder's composite backward and the re-summarisation bi-GRU's are PREPARED
(functional.PreparedCall) and go out as one ptv_decoder_free_bwd call, or -- when a stage declines -- each by its own means, in the same
order and with the same bits; the host's bookkeeping of a prepared call runs only after its launches went out.

Full-geometry model in bf16 with a FusedClipAdam (its weight shadows are what the backward composites read), one train step per case
(m.run -> loss_function -> backward) at B0 = 8.  B0: the smallest of 8, 17, 24, 40, 64 at which the parent commit (3cd0810) makes the one
call with teacher-forcing ratio 0 -- found by running such a step at each of the five on the parent and reading _DFF['bcalls']: it went up
by one at all five (and _DTB['calls'], _BRB['calls'] with it), so the smallest.  At B0 the ground-truth note-summary node (ratio > 0)
does not go through ptv_bigru_rows_bwd, so _BRB counts the free-running node's re-summarisation alone.  Every comparison is torch.equal
(the suite runs with ordered reductions)."""
import collections
import random

import pytest
import torch

from helpers import full_params
from polyphonic_chord_texture_disentanglement_amd import functional as F_
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
from polyphonic_chord_texture_disentanglement_amd import model as M
from polyphonic_chord_texture_disentanglement_amd._lib import lib
from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B0 = 8
Step = collections.namedtuple('Step', 'losses xhat grads bcalls dtb brb word')


class Rig:
    """the model, one batch, and the reference steps every case compares with (each computed once, then left alone)"""

    def __init__(self):
        self.m = M.DisentangleVAE.init_model(torch.device(DEV))
        self.m.load_state_dict(full_params())
        self.m.to(DEV).set_precision('bf16')
        self.opt = FusedClipAdam(self.m.parameters(), lr=1e-3)
        self.data = tuple(torch.from_numpy(a).to(DEV) for a in synth_batch(B0, 77))
        self.eps = {n: torch.randn(B0, 256, generator=torch.Generator().manual_seed(i)).to(DEV) for i, n in enumerate(('chd', 'rhy'))}
        self.refs = {}

    def step(self, tfrs, before_backward=lambda: None):
        """one train step with the ratios (time level, note level, chord) -> Step; before_backward() runs between loss and backward"""
        m = self.m
        xt, ct, prt = self.data
        random.seed(3)
        m.eps_source = lambda name, shape, device: self.eps[name]
        self.opt.zero_grad()
        outs = m.run(xt, ct, prt, *tfrs)
        losses = m.loss_function(xt, ct, *outs, 0.1, [1, 0.5])
        n0 = (FF_._DFF.get('bcalls', 0), F_._DTB.get('calls', 0), F_._BRB.get('calls', 0))
        before_backward()
        losses[0].backward()
        torch.cuda.synchronize()
        n1 = (FF_._DFF.get('bcalls', 0), F_._DTB.get('calls', 0), F_._BRB.get('calls', 0))
        return Step([l.detach().clone() for l in losses], m.decoder.last_xhat.clone(),
                    {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, *(b - a for a, b in zip(n0, n1)), FF_._DFB_PATH)

    def ref(self, key, tfrs, **switches):
        """the step with module switches set (FF_.FREE_COMPOSITE for the whole step, F_.* for the backward only), computed once per key"""
        if key not in self.refs:
            with pytest.MonkeyPatch.context() as mp:
                if 'FREE_COMPOSITE' in switches:
                    mp.setattr(FF_, 'FREE_COMPOSITE', switches.pop('FREE_COMPOSITE'))
                self.refs[key] = self.step(tfrs, lambda: [mp.setattr(F_, k, v) for k, v in switches.items()])
        return self.refs[key]


@pytest.fixture(scope='module')
def rig():
    return Rig()


def _same(a, b):
    for x, y in zip(a.losses, b.losses):
        assert torch.equal(x, y), (x, y)
    assert torch.equal(a.xhat, b.xhat)
    assert set(a.grads) == set(b.grads)
    for n in a.grads:
        assert torch.equal(a.grads[n], b.grads[n]), (n, (a.grads[n] - b.grads[n]).abs().max())


@pytest.mark.parametrize('tfr', [0.0, 0.5])
def test_one_call(rig, tfr):
    """both stages prepared: ONE ptv_decoder_free_bwd call, counted for the node and for both stages' tables (the step re-summarises at
    either ratio: some time coin is false); same bits as the node sequenced from Python (FREE_COMPOSITE off)"""
    got = rig.step((tfr,) * 3)
    assert (got.bcalls, got.dtb, got.brb, got.word) == (1, 1, 1, 'one call')
    ref = rig.ref(('python', tfr), (tfr,) * 3, FREE_COMPOSITE=False)
    assert (ref.bcalls, ref.word) == (0, 'FREE_COMPOSITE off')
    _same(got, ref)
    F_.persist_check()


@pytest.mark.parametrize('tfr', [0.0, 0.5])
def test_rows_stage_declines_after_the_decoder_stage_was_prepared(rig, tfr, monkeypatch):
    """the prepared decoder call goes out through its own entry point, the re-summarisation backward kernel by kernel: same bits as the
    one call's"""
    one = rig.step((tfr,) * 3)
    assert one.word == 'one call'
    got = rig.step((tfr,) * 3, lambda: monkeypatch.setattr(F_, 'bigru_rows_bwd_prepare', lambda *a, **k: None))
    assert (got.bcalls, got.dtb, got.brb) == (0, 1, 0) and 'rows' in got.word, got[3:]
    _same(got, one)
    F_.persist_check()


@pytest.mark.parametrize('tfr', [0.0, 0.5])
def test_decoder_stage_declines(rig, tfr, monkeypatch):
    """ptv_decoder_tf_bwd declines in the backward: the decoder stage is launched kernel by kernel at once, the re-summarisation still takes
    its composite; same bits as the step whose backward has the decoder composite switched off (PTV_BWD_COMPOSITES' switch of that stage)"""
    got = rig.step((tfr,) * 3, lambda: monkeypatch.setattr(F_, 'decoder_bwd_composite_static_ok', lambda *a, **k: False))
    assert (got.bcalls, got.dtb, got.brb) == (0, 0, 1) and 'decoder' in got.word, got[3:]
    ref = rig.ref(('dec off', tfr), (tfr,) * 3, DEC_BWD_COMPOSITE=False)
    assert (ref.bcalls, ref.dtb, ref.brb, ref.word) == (0, 0, 1, 'DEC_BWD_COMPOSITE off')
    _same(got, ref)
    F_.persist_check()


def test_no_resummarisation(rig):
    """every time coin true (the time-level ratio, run()'s first, is 1; note coins all false): no step re-summarises, the one call goes out
    with NULL rows tables"""
    tfrs = (1.0, 0.0, 0.0)
    got = rig.step(tfrs)
    assert (got.bcalls, got.dtb, got.brb, got.word) == (1, 1, 0, 'one call')
    _same(got, rig.ref(('python', tfrs), tfrs, FREE_COMPOSITE=False))
    F_.persist_check()


def test_bookkeeping_runs_after_the_call(rig, monkeypatch):
    """when ptv_decoder_free_bwd is entered, and still when it returns, _PERSIST_LAST holds the previous persistent launch's event (the one
    the decoder stage's turn waits for); only then does the turn's taken() publish the event the call recorded"""
    dev = torch.device(DEV).index
    turns, log = [], []

    class SpyTurn(F_._CompositeTurn):
        def __init__(self, cur):
            super().__init__(cur)
            turns.append(self)

        def taken(self):
            super().taken()
            log.append(('taken', self, F_._PERSIST_LAST.get(dev)))

    real = lib().ptv_decoder_free_bwd

    def shim(*args):
        log.append(('enter', turns[-1], F_._PERSIST_LAST.get(dev)))       # (the decoder stage's turn: the rows stage takes none)
        rc = real(*args)
        log.append(('exit', turns[-1], F_._PERSIST_LAST.get(dev)))
        return rc

    monkeypatch.setattr(F_, '_CompositeTurn', SpyTurn)
    monkeypatch.setattr(lib(), 'ptv_decoder_free_bwd', shim)
    got = rig.step((0.0,) * 3)
    assert (got.bcalls, got.word) == (1, 'one call')
    i = [k for k, e in enumerate(log) if e[0] == 'enter']
    assert len(i) == 1
    (_, turn, at_entry), (what, _, at_exit), (then, taken, after) = log[i[0]: i[0] + 3]
    assert turn.prev is not None and at_entry is turn.prev and at_entry is not turn.done
    assert what == 'exit' and at_exit is turn.prev
    assert then == 'taken' and taken is turn and after is turn.done
    assert not any(e[0] == 'taken' and e[1] is turn for e in log[:i[0]])
    F_.persist_check()
