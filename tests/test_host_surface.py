"""CPU: the host-side mirror keeps the reference's class surface, state_dict keys, default
initialisation and schedules.  No kernels run here (the model refuses CPU tensors)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from helpers import full_shapes, load_npz
from polyphonic_chord_texture_disentanglement_amd import model as M
from polyphonic_chord_texture_disentanglement_amd import ptvae as P
from polyphonic_chord_texture_disentanglement_amd.amc_dl import torch_plus as tp
from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus.train_utils import kl_anealing, scheduled_sampling


def build_reduced(device='cpu'):
    torch.manual_seed(0)
    chd_enc = P.RnnEncoder(36, 32, 16)
    rhy_enc = P.TextureEncoder(24, 32, 16, 3)
    chd_dec = P.RnnDecoder(z_input_dim=16, hidden_dim=24, z_dim=16)
    dec = P.PtvaeDecoder(device=device, note_emb_size=20, z_size=32, dec_emb_hid_size=12, dec_time_hid_size=40,
                         dec_notes_hid_size=28, dec_z_in_size=16, dec_dur_hid_size=8)
    return M.DisentangleVAE('disvae', device, chd_enc, rhy_enc, dec, chd_dec)


def test_state_dict_keys_and_shapes_match_reference():
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    ref = full_shapes()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got.keys()) == list(ref.keys())
    assert got == dict(ref)
    assert sum(p.numel() for p in m.parameters()) == 27310079


def test_default_init_reproduces_reference_rng_stream():
    g = load_npz('full_init.npz')
    torch.manual_seed(0)
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    sd = m.state_dict()
    assert [str(n) for n in g['names']] == list(sd.keys())
    psum = np.array([v.double().sum().item() for v in sd.values()])
    pabs = np.array([v.double().abs().sum().item() for v in sd.values()])
    np.testing.assert_allclose(psum, g['psum'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(pabs, g['pabs'], rtol=1e-12, atol=0)


def test_reduced_config_init_is_bit_identical():
    ref = load_npz('reduced_state.npz')
    sd = build_reduced().state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), ref[k]), k


def test_mode_dispatch_and_aliases():
    m = build_reduced()
    assert M.PolyphonicVAE is M.DisentangleVAE
    with pytest.raises(NotImplementedError):
        m('bogus-mode')
    x = torch.zeros(2, 32, 16, 6, dtype=torch.long)
    with pytest.raises(RuntimeError, match='no CPU'):          # product path fails loudly off-GPU
        m('train', x, torch.zeros(2, 8, 36), torch.zeros(2, 32, 128), tfr1=1., tfr2=1., tfr3=1.)


def test_schedules_match_reference_tables():
    g = load_npz('schedules.npz')
    tf1 = tp.TeacherForcingScheduler(0.6, 0)
    tf2 = tp.TeacherForcingScheduler(0.5, 0)
    beta = tp.TeacherForcingScheduler(0.1, 0., f=kl_anealing)
    ps = tp.ParameterScheduler(tfr1=tf1, tfr2=tf2, beta=beta, weights=tp.ConstantScheduler([1, 0.5]))
    rows = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for _ in range(75):
            d = ps.step()
            rows.append([d['tfr1'], d['tfr2'], d['beta']])
            assert d['weights'] == [1, 0.5]
    np.testing.assert_allclose(np.array(rows)[g['steps']], g['table'], rtol=1e-12, atol=0)
    ps.eval()                                                    # frozen in eval mode (scheduler.py:10-16)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a, b = ps.step(), ps.step()
    assert a == b
    lin = torch.nn.Linear(2, 2)
    opt = torch.optim.SGD(lin.parameters(), lr=1e-3)
    sch = tp.MinExponentialLR(opt, gamma=0.9999, minimum=1e-5)
    lrs = []
    for _ in range(5):
        opt.step()
        sch.step()
        lrs.append(opt.param_groups[0]['lr'])
    np.testing.assert_allclose(lrs, g['lrs'], rtol=1e-12)
    opt2 = torch.optim.SGD(lin.parameters(), lr=1e-3)
    sch2 = tp.MinExponentialLR(opt2, gamma=0.5, minimum=1e-5)
    for _ in range(20):
        opt2.step()
        sch2.step()
    assert opt2.param_groups[0]['lr'] == 1e-5                    # floor


def test_path_manager_and_writers(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pm = tp.LogPathManager(None)
    assert pm.epoch_model_path('disvae').endswith('models/disvae_epoch.pt')
    assert pm.valid_model_path('disvae').endswith('disvae_valid.pt')
    assert pm.final_model_path('disvae').endswith('disvae_final.pt')
    names = ['loss', 'recon_loss']
    sw = tp.SummaryWriters(names, {'loss': None}, pm.writer_path)
    sw.write_task('train', {'loss': 1.0, 'recon_loss': 2.0}, 0)
    assert sw.all_tags['train'] == {'train_loss': (0, 1)}


def test_reference_method_names_exist_on_the_decoder_and_encoder():
    """every method of the reference's PtvaeDecoder / PtvaeEncoder (ptvae.py:125-215, 218-575) is defined under its own name"""
    for n in ('get_len_index_tensor', 'index_tensor_to_multihot_tensor', 'get_sos_token', 'dur_ind_to_dur_token',
              'pitch_dur_ind_to_note_token', 'decode_note', 'decode_notes', 'decoder', 'forward', 'recon_loss', 'emb_x',
              'output_to_numpy', 'pr_to_notes', 'grid_to_pr_and_notes'):
        assert callable(getattr(P.PtvaeDecoder, n, None)), n
    for n in ('get_len_index_tensor', 'index_tensor_to_multihot_tensor', 'encoder', 'forward'):
        assert callable(getattr(P.PtvaeEncoder, n, None)), n
    with pytest.raises((AssertionError, RuntimeError)):            # no CPU fallback: the helpers refuse host tensors too
        build_reduced().decoder.get_len_index_tensor(torch.zeros(1, 32, 16, 6, dtype=torch.long))


def test_checkpoint_keeps_each_ranks_random_state(tmp_path, monkeypatch):
    """round-3 advice: rank 0 writes the checkpoint -- a data-parallel resume must not hand rank 0's Philox sample offset / generator
    states to every rank (identical noise for different samples).  Every other rank saves its own block next to the file and restores
    it; a checkpoint without such a block (written by a single process) restores the shared parts only (seed, draw counter, coins)."""
    import random
    from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus.module import TrainingInterface

    class Stub:
        def state_dict(self):
            return {}

        def load_state_dict(self, sd):
            pass

    class Model(Stub):
        _philox, _draws = None, 0

    def trainer(rank, offset, draws):
        t = object.__new__(TrainingInterface)
        t.model = Model()
        t.model._philox, t.model._draws = (9, offset), draws
        t.device = torch.device('cpu')
        t.parallel = False
        t.data_loaders = None
        t.epoch = t.train_step = t.val_step = 0
        t.param_scheduler = Stub()
        t.opt_scheduler = type('O', (), {'optimizer': Stub(), 'scheduler': Stub(), '_step': 0})()
        monkeypatch.setattr(TrainingInterface, 'is_main', property(lambda self: self._r == 0))
        monkeypatch.setattr(TrainingInterface, '_rank', lambda self: self._r)
        t._r = rank
        return t

    fn = str(tmp_path / 'ck.pt')
    t0, t1 = trainer(0, 0, 5), trainer(1, 16, 5)
    random.seed(3)
    t0.save_checkpoint(fn)
    t1.save_checkpoint(fn)                                       # rank 1: only its own random-state block
    assert (tmp_path / 'ck.pt.rng1').exists()
    r1 = trainer(1, 999, 0)
    r1.load_checkpoint(fn)
    assert r1.model._philox == (9, 16) and r1.model._draws == 5   # ITS offset, not rank 0's
    r0 = trainer(0, 999, 0)
    r0.load_checkpoint(fn)
    assert r0.model._philox == (9, 0) and r0.model._draws == 5
    (tmp_path / 'ck.pt.rng1').unlink()                           # a single-process checkpoint resumed on two ranks
    r1 = trainer(1, 16, 0)
    random.seed(12345)
    r1.load_checkpoint(fn)
    assert r1.model._philox == (9, 16) and r1.model._draws == 5   # seed + draw counter shared, sample offset kept
    assert random.getstate() == torch.load(fn, weights_only=False)['rng']['python_random']      # the coin stream is the checkpoint's


def test_dead_helpers_of_the_reference_model_exist_and_compute_what_it_defines():
    """model.py:22-40 (`confuse_prmat`, `get_chroma`: defined, never called -- both call sites are commented out).  Plain tensor code:
    checked on the CPU against the reference's own expressions restated inline."""
    m = build_reduced('cpu')
    g = torch.Generator().manual_seed(1)
    pr = ((torch.rand(3, 32, 128, generator=g) < 0.05).float() * torch.randint(1, 9, (3, 32, 128), generator=g).float())
    pad = torch.zeros(3, 32, 4)
    ref = torch.log(torch.cat([pr, pad], -1).view(3, 32, -1, 12).sum(-2).view(3, 8, 4, 12).sum(-2).float() + 1)
    assert torch.equal(m.get_chroma(pr.clone()), ref) and ref.shape == (3, 8, 12)
    torch.manual_seed(5)
    out = m.confuse_prmat(pr.clone())
    torch.manual_seed(5)
    nz = torch.nonzero(pr.long())
    eps = ((2 * torch.randint(0, 2, (nz.size(0),))) - 1).long()
    exp = pr.clone()
    exp[nz[:, 0], nz[:, 1], torch.clamp(nz[:, 2] + eps, min=0, max=127)] = exp[nz[:, 0], nz[:, 1], nz[:, 2]]
    assert torch.equal(out, exp) and (out != pr).any()


def test_loss_node_zero_skip_hint_matches_only_the_very_tensors():
    """functional._loss_top_hint: the loss node's zero-skip bound must be honoured for exactly the gradient tensors it produced -- the same
    storage, shape, strides and version, whatever Python wrapper they arrive in (the engine hands them over through C++) -- and for nothing
    else: not a copy, not an in-place modified tensor, not a view with another shape.  (Round 5: an identity-based key never matched and the
    decoder silently scanned the gradients every step.)"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    dp, dd, top = torch.zeros(6, 8), torch.zeros(6, 10), torch.tensor([3], dtype=torch.int32)

    def arm():
        F_._LOSS_TOP.clear()
        F_._LOSS_TOP['hint'] = (dp, dd, dp._version, dd._version, top)
    arm()
    assert F_._loss_top_hint(dp.view(6, 8), dd.view(6, 10)) is top          # new wrapper objects of the same tensors: accepted
    assert F_._loss_top_hint(dp, dd) is None                                 # consumed: one use
    arm()
    assert F_._loss_top_hint(dp.clone(), dd) is None                         # a copy (autograd accumulated another contribution)
    arm()
    dp.add_(0)
    assert F_._loss_top_hint(dp, dd) is None                                 # modified in place (a tensor hook): version bumped
    arm()
    assert F_._loss_top_hint(dp.view(8, 6), dd) is None                      # same storage, other shape
    arm()
    assert F_._loss_top_hint(None, dd) is None
    F_._LOSS_TOP.clear()


def test_live_rows_plan_hands_out_the_targets_of_the_recorded_row_order_for_its_own_x_only():
    """functional.LiveRows: loss()'s plan gives the loss node the targets in the row order the decoder node recorded -- and only for the
    very x it was built for, unmodified, with step-major logits; anything else raises instead of pairing targets with the wrong rows"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    x = torch.zeros(4, 32, 16, 6, dtype=torch.long)
    pt, dt, counts = torch.arange(8, dtype=torch.int32), torch.arange(40, dtype=torch.int32), torch.tensor([5, 7, 3], dtype=torch.int32)
    pt_s, dt_s = pt.flip(0), dt.flip(0)

    def plan(sort=True):
        return F_.LiveRows(x, pt, dt, counts, dict(perm=None, len=None, pt=pt_s, dt=dt_s, seg_n=None) if sort else None)
    p = plan()
    assert p.top.tolist() == [3]
    with pytest.raises(RuntimeError):
        p.targets(x, True)                                                   # no decoder recorded its row order yet
    p.record_order(True)
    got = p.targets(x.view(4, 32, 16, 6), True)                              # another wrapper of the same tensor: accepted
    assert got[0] is pt_s and got[1] is dt_s and got[2] is counts
    with pytest.raises(RuntimeError):
        p.record_order(False)                                                # one plan, one forward
    p = plan()
    p.record_order(False)
    got = p.targets(x, True)
    assert got[0] is pt and got[1] is dt and got[2] is counts
    with pytest.raises(RuntimeError):
        p.targets(x.clone(), True)                                           # another tensor
    with pytest.raises(RuntimeError):
        p.targets(x[:2], True)                                               # same storage, other shape
    with pytest.raises(RuntimeError):
        p.targets(x, False)                                                  # batch-major logits
    x.add_(0)
    with pytest.raises(RuntimeError):
        p.targets(x, True)                                                   # modified in place: version bumped
    with pytest.raises(RuntimeError):
        plan(sort=False).record_order(True)                                  # sorted logits need a row order


def test_grad_arena_views_are_fresh_objects_over_the_bucket():
    """optim.GradArena.view: a new tensor object per call (autograd adopts a gradient only when nothing else references it) that aliases
    the parameter's 16-byte aligned range of the flat bucket with the parameter's shape"""
    from polyphonic_chord_texture_disentanglement_amd.optim import GradArena
    ps = [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2, 3, 4))]
    a = GradArena(ps)
    for i, p in enumerate(ps):
        v1, v2 = a.view(p), a.view(p)
        assert v1 is not v2 and v1.shape == p.shape and v1.is_contiguous()
        assert v1.data_ptr() == a.flat.data_ptr() + 4 * a.offsets[i] and a.offsets[i] % 8 == 0
        v1.fill_(i + 1)
        assert float(a.flat[a.offsets[i]:a.offsets[i] + p.numel()].sum()) == (i + 1) * p.numel()
    assert a.take(ps[0]) is not None and a.take(ps[0]) is None               # handed out once per zero()
    a.zero()
    assert float(a.flat.abs().sum()) == 0 and a.take(ps[0]) is not None


@pytest.mark.parametrize('tag', ['BRF', 'BRB', 'BGF', 'BGB', 'DTF', 'DTB', 'CDF', 'CDB', 'VL', 'DFF', 'DFB'])
def test_slot_table_fills_the_tables_of_every_composite_enum_pair(tag):
    """_lib.SlotTable(tag): both enums of include/ptvae_hip.h parsed, the arrays as long as their *_COUNT enumerators say, a value given under
    a slot's short name at the index header_enum reports, every other slot NULL / 0, a name that is no enumerator a KeyError"""
    import ctypes
    from polyphonic_chord_texture_disentanglement_amd._lib import SlotTable, header_enum
    name = 'Ptv%s' % tag.capitalize()
    T, D = header_enum(name + 'Tensor'), header_enum(name + 'Dim')
    n_t, n_d = T.pop('PTV_%s_COUNT' % tag), D.pop('PTV_%s_D_COUNT' % tag)
    assert n_t == len(T) and n_d == len(D)
    tab = SlotTable(tag)
    tab.count(), tab.count(), tab.count('other')
    assert tab == {'calls': 2, 'other': 1}                                   # (the dict holds the call counters, nothing else)
    for full, i in T.items():
        short = full[len('PTV_%s_' % tag):]
        arr = tab.pointers({short: None}, handles={short: 0x1000 + i})       # (the handle is written after the tensors' None)
        assert isinstance(arr, ctypes.c_void_p * n_t) and len(arr) == n_t
        assert [arr[j] for j in range(n_t)] == [0x1000 + i if j == i else None for j in range(n_t)]
    for full, i in D.items():
        arr = tab.dims({full[len('PTV_%s_D_' % tag):]: 7 + i})
        assert isinstance(arr, ctypes.c_long * n_d) and list(arr) == [7 + i if j == i else 0 for j in range(n_d)]
    assert all(v is None for v in tab.pointers({}, {k[len('PTV_%s_' % tag):]: None for k in T})) and not any(tab.dims({}))
    for bad in (lambda: tab.pointers({'NO_SUCH_SLOT': None}), lambda: tab.pointers(handles={'NO_SUCH_SLOT': 1}),
                lambda: tab.pointers(handles={'COUNT': 1}), lambda: tab.dims({'NO_SUCH_SLOT': 1}), lambda: tab.dims({'COUNT': 1})):
        with pytest.raises(KeyError, match=name):
            bad()


def test_bigru_state_refuses_what_its_backward_could_not_read():
    """functional.BiGruState (what a bi-GRU forward leaves for its backward): the row and the persistent kernels save bf16 gates and bf16
    states, K segments count rows in the order of a permutation, a permutation sorts by the lengths the kernels skip by -- every other
    combination is refused at construction; what it holds stays within reach of _record_stream"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    T, M, H = 3, 8, 16
    t = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    bf = torch.bfloat16
    d16 = [(t(T + 1, M, H), t(T, 4, M, H, dt=bf), t(T + 1, M, H, dt=bf)) for _ in range(2)]
    d32 = [(t(T + 1, M, H), t(T, 4, M, H), None) for _ in range(2)]
    no_h16 = [d16[0], (d16[1][0], d16[1][1], None)]
    f32_gates = [(d16[0][0], d32[0][1], d16[0][2]), d16[1]]
    ints = lambda n: t(n, dt=torch.int32)
    for branch in ('rows', 'persist'):
        for dirs in (d32, no_h16, f32_gates):
            with pytest.raises(ValueError, match=branch):
                F_.BiGruState(branch, dirs)
    with pytest.raises(ValueError, match='branch'):
        F_.BiGruState('row', d16)
    with pytest.raises(ValueError, match='seg'):
        F_.BiGruState('rows', d16, lengths=ints(M), seg=ints(T))
    with pytest.raises(ValueError, match='perm'):
        F_.BiGruState('rows', d16, perm=ints(M))
    with pytest.raises(ValueError, match='perm'):
        F_.BiGruState('rows', d16, perm=ints(M), seg=ints(T))
    s = F_.BiGruState('rows', d16, ints(M), ints(M), ints(T))
    assert (s.branch, s.hall, s.gates, s.h16) == ('rows',) + tuple(zip(*d16))
    assert F_.BiGruState('step', d32).h16 == (None, None) and F_.BiGruState('step', d16).lengths is None
    assert F_.BiGruState('persist', iter(d16)).branch == 'persist' and F_.BiGruState('rows', d16).seg is None
    # the row kernels switched off between forward and backward: refused before anything is launched (meta tensors: a launch would fail otherwise)
    w = [t(*sh) for _ in range(2) for sh in ((3 * H, H), (3 * H, H), (3 * H,), (3 * H,))]
    old, F_.NOTES_PERSIST = F_.NOTES_PERSIST, False
    try:
        with pytest.raises(RuntimeError, match='row kernels'):
            F_._bigru_backward(1, t(T, M, H), w, s, t(M, 2 * H), True)
    finally:
        F_.NOTES_PERSIST = old
    # (Side keeps the state alive and tells the caching allocator about it through _record_stream: all nine tensors must be within its reach)
    seen = []

    class Probe(torch.Tensor):
        is_cuda = True

        def record_stream(self, stream):
            seen.append(self)
    probe = lambda: torch.Tensor._make_subclass(Probe, torch.empty(1, dtype=bf))
    dirs = [(probe(), probe(), probe()) for _ in range(2)]
    extras = [probe(), probe(), probe()]
    F_._record_stream(F_.BiGruState('rows', dirs, *extras), None)
    assert {id(x) for x in seen} == {id(x) for x in extras + [x for d in dirs for x in d]}


def test_decoder_state_refuses_what_no_forward_leaves():
    """functional.DecoderState (what a PianoTree decoder forward leaves for its backward) names the kernels that ran; its constructor takes
    every combination a forward produces and refuses the others: an unknown name, a 'rows' state without bf16 gates and bf16 states,
    'fused16' without HD16, rebuilt duration gates (gates_d None) anywhere else, sorted rows or a dead-step limit unless the whole chain
    honours them.  What it holds -- the sorted record and the step loop's extras too -- stays within reach of _record_stream"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    B, E, He, Ht, Hn, Hd, NP = 1, 8, 8, 16, 16, 8, 10
    R, M = 32 * B, 15 * 32 * B
    dims = (B, R, E, He, Ht, Hn, Hd, NP)
    bf = torch.bfloat16
    t = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    ints = lambda *s: t(*s, dt=torch.int32)

    def saved(dt=bf, pad=True, **over):
        """the tensors of a bf16-storage forward (dt = bf) or of an fp32 one (no bf16 shadows)"""
        h16 = (lambda *s: t(*s, dt=bf)) if dt == bf else (lambda *s: None)
        kw = dict(NS=t(33, B, Ht), NS16=h16(33, B, Ht), z_in=t(B, 4), TOKS=t(33, B, 2 * He), gates_t=t(32, 4, B, Ht, dt=dt),
                  HN=t(16, R, Hn), HN16=h16(16, R, Hn), gates_n=t(15, 4, R, Hn, dt=dt), pitch=t(M, 16 if pad else NP)[:, :NP],
                  HD=t(6, M, Hd), HD16=h16(6, M, Hd), gates_d=t(5, 4, M, Hd, dt=dt), idx=ints(5, M), dur_tabs=(t(1, 3 * Hd), t(2, 3 * Hd)))
        kw.update(over)
        return kw
    srt = F_.DecoderSorted(ints(R), ints(R), t(R, Ht, dt=bf), t(15, R, E), ints(16))
    loop = dict(TOK=t(15, R, E), PRED=t(16, R, E), xhat=t(B, 32, 16, 6, dt=torch.long), XH=[t(17, R, He)] * 2, XG=[t(16, 4, R, He, dt=bf)] * 2,
                XH16=[None, None], plen=ints(R), skipped=True, coins=([[False] * 14] * 32, [False] * 31), has_xs=True)
    # what the forwards produce: the composite and the launch-by-launch fused chain (gates rebuilt or saved, with and without the limit and
    # sorted rows), mixed chains with one stage switched off, fp32 storage, and the step loop with and without its batched recompute
    S = F_.DecoderState
    s = S(dims, 1, 'rows', 'fused', 'fused16', **saved(gates_d=None), live_top=ints(1), sorted=srt)
    assert (s.B, s.R, s.E, s.He, s.Ht, s.Hn, s.Hd, s.NP, s.prec) == dims + (1,) and s.sorted.seg_n is srt.seg_n and s.gates_d is None
    assert S(dims, 1, 'rows', 'fused', 'fused16', **saved()).live_top is None
    for names in (('step', 'fused', 'fused16'), ('rows', 'gemm', 'fused16'), ('rows', 'fused', 'step'), ('step', 'gemm', 'step')):
        assert S(dims, 1, *names, **saved()).sorted is None
    assert S(dims, 0, 'step', 'gemm', 'step', **saved(torch.float32, pad=False)).HN16 is None
    assert FF_.DecoderStepState(dims, 1, 'rows', 'fused', 'fused16', **saved(gates_d=None), **loop).plen is loop['plen']
    assert FF_.DecoderStepState(dims, 1, 'step', 'gemm', 'fused', **saved(NS16=None, HN16=None, HD16=None), **loop).dur == 'fused'
    # ... and what none of them does
    for names in (('row', 'fused', 'fused16'), ('rows', 'fuse', 'fused16'), ('rows', 'fused', 'fused32')):
        with pytest.raises(ValueError, match='unknown'):
            S(dims, 1, *names, **saved())
    for over in (dict(HN16=None), dict(gates_n=t(15, 4, R, Hn)), dict(gates_n=None)):
        with pytest.raises(ValueError, match="'rows'"):
            S(dims, 1, 'rows', 'gemm', 'fused16', **saved(**over))
    with pytest.raises(ValueError, match="'fused16'"):
        S(dims, 1, 'step', 'gemm', 'fused16', **saved(HD16=None))
    for dur in ('fused', 'step'):
        with pytest.raises(ValueError, match='gates_d'):
            S(dims, 1, 'rows', 'fused', dur, **saved(gates_d=None))
    for extra in (dict(sorted=srt), dict(live_top=ints(1))):
        for names in (('step', 'fused', 'fused16'), ('rows', 'gemm', 'fused16'), ('rows', 'fused', 'step')):
            with pytest.raises(ValueError, match='whole chain'):
                S(dims, 1, *names, **saved(), **extra)
    with pytest.raises(ValueError, match='DecoderSorted'):
        S(dims, 1, 'rows', 'fused', 'fused16', **saved(), sorted=dict(srt._asdict()))
    # (Side keeps the state alive and tells the caching allocator about it through _record_stream: every tensor must be within its reach)
    seen = []

    class Probe(torch.Tensor):
        is_cuda = True

        def record_stream(self, stream):
            seen.append(self)
    probe = lambda *a, **k: torch.Tensor._make_subclass(Probe, torch.empty(1, dtype=bf))
    kw = saved(gates_d=None)
    kw = {k: probe() for k in kw if k not in ('dur_tabs', 'pitch', 'gates_d')}
    kw.update(dur_tabs=(probe(), probe()), pitch=torch.Tensor._make_subclass(Probe, torch.empty(M, 16)[:, :NP]), gates_d=None)
    srt_p = F_.DecoderSorted(*[probe() for _ in range(5)])
    loop_p = dict(loop, **{k: probe() for k in ('TOK', 'PRED', 'xhat', 'plen')}, XH=[probe(), probe()], XG=[probe(), probe()],
                  XH16=[probe(), probe()])
    top = probe()
    F_._record_stream(FF_.DecoderStepState(dims, 1, 'rows', 'fused', 'fused16', **kw, **loop_p, live_top=top, sorted=srt_p), None)
    want = ([v for k, v in kw.items() if k not in ('dur_tabs', 'gates_d')] + list(kw['dur_tabs']) + list(srt_p) + [top]
            + [loop_p[k] for k in ('TOK', 'PRED', 'xhat', 'plen')] + loop_p['XH'] + loop_p['XG'] + loop_p['XH16'])
    assert len(want) == 14 + 5 + 1 + 10 and {id(x) for x in seen} == {id(x) for x in want}


def test_chord_decoder_state_refuses_what_no_forward_leaves(monkeypatch):
    """functional.ChordDecoderState (what either chord decoder forward leaves for chord_decoder_bwd): fp32 states of T + 1 steps, gates of the
    storage dtype of (prec, H), the fed tokens, z_in, all contiguous and of the stated geometry; what it holds stays within reach of
    _record_stream"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    monkeypatch.setattr(F_, 'BF16_STORAGE', True)
    T, B, H, I, Zi = 8, 3, 16, 36, 5
    bf = torch.bfloat16
    t = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)

    def saved(gdt=torch.float32, h=H, **over):
        kw = dict(hall=t(T + 1, B, h), gates=t(T, 4, B, h, dt=gdt), toks=t(T, B, I), z_in=t(B, Zi))
        kw.update(over)
        return kw
    S = F_.ChordDecoderState
    s = S(T, B, H, I, 0, **saved())
    assert (s.T, s.B, s.H, s.I, s.prec) == (T, B, H, I, 0) and s.gates.dtype == torch.float32 and s.z_in.shape == (B, Zi)
    assert S(T, B, H, I, 1, **saved(bf)).gates.dtype == bf
    assert S(T, B, 12, I, 1, **saved(h=12)).gates.dtype == torch.float32                # (H no multiple of 8: fp32 storage in bf16 precision)
    assert S(1, B, H, I, 1, hall=t(2, B, H), gates=t(1, 4, B, H, dt=bf), toks=t(1, B, I), z_in=t(B, Zi)).T == 1
    for prec, gdt, h in ((0, bf, H), (1, torch.float32, H), (1, bf, 12)):
        with pytest.raises(ValueError, match='gates'):
            S(T, B, h, I, prec, **saved(gdt, h))
    for name, over in (('hall', dict(hall=t(T, B, H))), ('hall', dict(hall=t(T + 1, B, H, dt=bf))), ('hall', dict(hall=t((T + 1) * B, H))),
                       ('toks', dict(toks=t(T, B, I + 1))), ('toks', dict(toks=t(T, B + 1, I))), ('gates', dict(gates=t(T, 3, B, H))),
                       ('z_in', dict(z_in=t(B + 1, Zi))), ('z_in', dict(z_in=t(B))),
                       ('hall', dict(hall=t(T + 1, H, B).transpose(1, 2))), ('gates', dict(gates=t(T, 4, B, 2 * H)[..., ::2])),
                       ('toks', dict(toks=t(B, T, I).transpose(0, 1))), ('z_in', dict(z_in=t(Zi, B).t()))):
        with pytest.raises(ValueError, match='ChordDecoderState: ' + name):
            S(T, B, H, I, 0, **saved(**over))
    seen = []

    class Probe(torch.Tensor):
        is_cuda = True

        def record_stream(self, stream):
            seen.append(self)
    kw = {k: torch.Tensor._make_subclass(Probe, torch.empty(v.shape, dtype=v.dtype)) for k, v in saved(bf).items()}
    F_._record_stream(S(T, B, H, I, 1, **kw), None)
    assert len(seen) == 4 and {id(x) for x in seen} == {id(x) for x in kw.values()}


def test_chord_decoder_slot_helpers_name_only_slots_of_each_enum():
    """functional._chd_slots, the one parameter-to-slot statement of the chord decoder's three tables: every name
    it hands a table is an enumerator of that table's enum; CDF and CDS (whose C side refuses a NULL parameter) get all 15, CDB the seven
    weight matrices and all 15 gradients"""
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    from polyphonic_chord_texture_disentanglement_amd._lib import header_enum
    P = {n: torch.empty(1) for n in F_.CHD_PARAM_NAMES}
    enum = lambda tag: {k[len('PTV_%s_' % tag):] for k in header_enum('Ptv%sTensor' % tag.capitalize())}
    every, weights, grads = F_._chd_slots(P), F_._chd_slots(P, biases=False), F_._chd_slots(P, 'G_')
    assert len(every) == 15 and [every[F_._CHD_SLOTS[n]] is P[n] for n in P] == [True] * 15
    params = lambda tag: {s for s in enum(tag) if s == 'INIT_INPUT' or s.split('_')[0] in ('W', 'B')}
    assert set(every) == params('CDF') == params('CDS')
    assert set(weights) == params('CDB') and len(weights) == 7 and all(weights[s] is every[s] for s in weights)
    assert set(grads) == {s for s in enum('CDB') if s.startswith('G_')} and len(grads) == 15
    assert [grads['G_' + F_._CHD_SLOTS[n]] is P[n] for n in P] == [True] * 15
    for tag, maps in (('CDF', (every,)), ('CDS', (every,)), ('CDB', (weights, grads))):
        F_.SlotTable(tag).pointers(*({s: None for s in m} for m in maps))               # (raises on a name the enum lacks)
    with pytest.raises(KeyError, match='PtvCdb'):
        F_.SlotTable('CDB').pointers({s: None for s in every})                           # CDB has no bias slot: nothing swallows that


def test_loss_tensors_round_trip_in_saved_order():
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    names = ['pitch', 'dur', 'mu_c', 'sd_c', 'mu_r', 'sd_r', 'root', 'chroma', 'bass', 'pitch_t', 'dur_t', 'counts', 'root_t', 'chroma_t',
             'bass_t']
    assert list(F_.LossTensors._fields) == names
    ts = tuple(torch.full((1,), float(i)) for i in range(15))
    L = F_.LossTensors(*ts)
    assert tuple(L) == ts and all(getattr(L, n) is ts[i] for i, n in enumerate(names))
    assert all(a is b for a, b in zip(F_.LossTensors(*tuple(L)), ts))                    # ctx.save_for_backward(*L) -> LossTensors(*saved_tensors)
    assert F_._vl_slots(L) == {n.upper(): ts[i] for i, n in enumerate(names)}
    assert F_.LossGrads._fields == ('dpitch', 'ddur', 'dmu_c', 'dsd_c', 'dmu_r', 'dsd_r', 'droot', 'dchroma', 'dbass')
    assert F_.LossState._fields == ('scal', 'gcnt', 'sm_p', 'sm_c')
    with pytest.raises(TypeError):
        F_.LossTensors(*ts[:14])


# ---- the free-running decode's host path: the kind of a block, the note loop's word, the coin masks, the decode request, the plan
KIND_TABLE = {None: (0, 0, 0, 0, 0, 0, 'ptv_note_token', 'ptv_dur_gru_fwd', 'ptv_dur_out_token'),
              4: (4, 0x800000, 0, 0, 1, 32, 'ptv_note_token_sample', 'ptv_dur_gru_fwd_sample', 'ptv_dur_out_token_sample'),
              6: (6, 0x1800000, 1, 0, 2, 48, 'ptv_note_token_sample_trunc', 'ptv_dur_gru_fwd_sample', 'ptv_dur_out_token_sample'),
              8: (8, 0x3800000, 1, 1, 3, 64, 'ptv_note_token_sample_cons', 'ptv_dur_gru_fwd_sample', 'ptv_dur_out_token_sample')}


def _kind_of(words):
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    return FF_.block_kind(None if words is None else torch.zeros(words, dtype=torch.int64))


def test_block_kind_states_every_variant_once():
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    for words, want in KIND_TABLE.items():
        k = _kind_of(words)
        assert tuple(k) == want
        assert (k.words, k.bits, k.trunc, k.cons, k.kind, k.nbytes, k.note_token, k.dur_gru, k.dur_token) == want
        with pytest.raises(AttributeError):
            k.bits = 0                                                   # (immutable)
    assert [_kind_of(w).kind for w in KIND_TABLE] == [0, 1, 2, 3]
    assert (FF_.SAMPLE_BIT, FF_.TRUNC_BIT, FF_.CONS_BIT) == (0x800000, 0x1000000, 0x2000000)
    for words in (0, 1, 3, 5, 7, 9, 16):
        with pytest.raises(ValueError, match='sampling_block'):
            _kind_of(words)
    # the words sampling_words makes are the counts the kinds name
    assert _kind_of(len(FF_.sampling_words(1.0))).kind == 1 and _kind_of(len(FF_.sampling_words(1.0, top_k=3))).kind == 2
    assert _kind_of(len(FF_.sampling_words(1.0, ascending=True))).kind == 3


def test_note_loop_word_is_the_parents_expression():
    import itertools
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    seen = set()
    for train, replay, split, cluster, words in itertools.product((0, 1), (0, 1), (None, True, False), (0, 2, 4, 8), KIND_TABLE):
        kind = _kind_of(words)
        samp_bit = 0 if words is None else (0x800000 | {4: 0, 6: 0x1000000, 8: 0x1000000 | 0x2000000}[words])
        want = ((2 if replay else int(train)) | (0 if split is None else (0x20000 if split else 0x10000))
                | (0x400000 if cluster == 8 else (cluster << 18)) | samp_bit)
        eager = FF_.note_loop_word(train, replay, split, cluster, kind)
        assert eager == want
        # the composite's form: the same word without the sampling bits (they travel as dims)
        assert FF_.note_loop_word(train, replay, split, cluster) == want & ~0x3800000 == eager & ~kind.bits
        assert FF_.note_loop_word(bool(train), bool(replay), split, cluster, kind) == want
        seen.add((want, replay or train, split, cluster, words))
    assert len(seen) == 2 * 3 * 4 * 4 + 3 * 4 * 4                        # (replay hides train: 3 distinct low fields, nothing else collides)


def test_coin_masks():
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    none = ([[False] * 14] * 32, [False] * 31)
    every = ([[True] * 14] * 32, [True] * 31)
    odd = ([[(t * 5 + n * 3) % 7 < 3 for n in range(14)] for t in range(32)], [t % 3 == 1 for t in range(31)])

    def lists(coins, inference):
        masks, time = FF_.coin_masks(coins, inference)
        assert len(masks) == 32 and len(time) == 31 and masks._type_ is ctypes.c_uint and time._type_ is ctypes.c_ubyte
        assert bytes(time) == bytes(list(time)) and all(type(masks[t]) is int for t in range(32))
        return list(masks), list(time)
    assert lists(none, False) == ([0] * 32, [0] * 31)
    assert lists(every, False) == ([0x3fff] * 32, [1] * 31)
    masks, time = lists(odd, False)
    for t in range(32):
        want = 0
        for n in range(14):
            want |= int(bool(odd[0][t][n])) << n
        assert masks[t] == want and 0 <= want < 1 << 14
    assert time == [int(t % 3 == 1) for t in range(31)] and len(set(masks)) > 4
    for coins in (none, every, odd):                                     # inference: the kernels see no coin
        assert lists(coins, True) == ([0] * 32, [0] * 31)
    assert lists(([np.ones(14)] * 32, np.ones(31)), False) == ([0x3fff] * 32, [1] * 31)   # numpy / 0-1 coins count like bools


NAN, INF = float('nan'), float('inf')
BAD_DECODE_KEYWORDS = [
    # sampling (test_sample_ref_host)
    dict(temperature=-0.5), dict(temperature=NAN), dict(temperature=INF), dict(temperature=1.0, dur_temperature=-1.0),
    dict(temperature=1.0, dur_temperature=NAN), dict(temperature=1.0, sample_offset=-1), dict(temperature='1'), dict(seed=3), dict(draw=1),
    dict(sample_offset=4), dict(temperature=1.0, seed=-1), dict(temperature=1.0, seed=1 << 64), dict(temperature=1.0, draw=1 << 63),
    dict(temperature=1.0, sample_offset=1 << 47), dict(temperature=True),
    # truncation (test_gpu_truncated_sampling, test_nucleus_ref)
    dict(top_k=8), dict(min_p=0.5), dict(top_p=0.5), dict(temperature=1.0, top_k=0), dict(temperature=1.0, top_k=-3),
    dict(temperature=1.0, top_k=True), dict(temperature=1.0, top_k=2.0), dict(temperature=1.0, min_p=1.5), dict(temperature=1.0, min_p=-0.1),
    dict(temperature=1.0, min_p=NAN), dict(temperature=1.0, min_p=INF), dict(temperature=1.0, min_p=True), dict(temperature=1.0, top_p=0.0),
    dict(temperature=1.0, top_p=1.5), dict(temperature=1.0, top_p=NAN), dict(temperature=1.0, top_p=True), dict(ascending=True, top_k=3),
    # constraints (test_gpu_constrained_decode): what needs no device
    dict(pitch_mask=torch.zeros(2, 32, 4, dtype=torch.int32)), dict(pitch_mask=np.zeros((2, 32, 4), dtype=np.int32)), dict(ascending=1),
    dict(ascending='yes'), dict(temperature=1.0, ascending=0), dict(temperature=1.0, pitch_mask=torch.zeros(1, 32, 4, dtype=torch.int32)),
    # keep (test_keep_ref_host)
    dict(keep={'pitch': None, 'dur': None}), dict(keep=(1, 2, 3, 4)), dict(temperature=1.0, keep='first bar')]


@pytest.mark.parametrize('kw', BAD_DECODE_KEYWORDS, ids=lambda kw: ','.join('%s=%s' % (k, type(v).__name__ if hasattr(v, 'shape') else v)
                                                                         for k, v in kw.items()))
def test_decode_request_raises_what_the_keywords_always_raised_and_moves_nothing(kw):
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    m._sample_draws = 5
    m.train()
    with pytest.raises(ValueError) as direct:
        M.DisentangleVAE._check_sampling(**kw, batch=2)
    z, tex, c = torch.zeros(2, 256), torch.zeros(2, 32, 128), torch.zeros(2, 8, 36)
    calls = [lambda: m._request(2, **kw), lambda: m.inference_decode(z, z, **kw), lambda: m.decode_to_inputs(z, z, **kw),
             lambda: m.decode_logprob(z, z, **kw), lambda: m.reencode(z, z, **kw), lambda: m.inference(tex, c, False, **kw),
             lambda: m.swap(tex, tex, c, c, True, True, **kw), lambda: m.posterior_sample(tex, c, **kw),
             lambda: m.posterior_sample(tex, c, scale=2.0, **kw), lambda: m.prior_sample(tex, c, **kw),
             lambda: m.interp(tex, c, tex, c, int_count=1, **kw)]
    if kw.get('temperature') is not None or kw.get('dur_temperature') is not None:
        calls.append(lambda: m.decode_best_of(z, z, 2, **kw))
    for fn in calls:
        with pytest.raises(ValueError) as got:
            fn()
        assert str(got.value) == str(direct.value)                       # the validator's own text, whichever entry point was asked
        assert m._sample_draws == 5 and m.training                       # before eval(), before the draw counter moves


def test_decode_request_carries_the_validated_keywords():
    m = M.DisentangleVAE.init_model(torch.device('cpu'))
    req = m._request(3)
    assert isinstance(req, M.DecodeRequest) and req.sampled is False and req.mask is None and req.keep is None and req.batch == 3
    assert set(req.kw) == set(M.DECODE_KEYS[:-2]) and all(v is None for v in req.kw.values())
    assert m._sampling_words(req) is None and m._sample_draws == 0
    req = m._request(3, temperature=0.5, top_k=4, seed=9)
    assert req.sampled is True and req.kw['temperature'] == 0.5 and req.kw['top_k'] == 4 and req.kw['seed'] == 9 and req.kw['draw'] is None
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    assert m._sampling_words(req) == FF_.sampling_words(0.5, None, 9, 0, 0, top_k=4) and m._sample_draws == 1
    assert m._sampling_words(req) == FF_.sampling_words(0.5, None, 9, 1, 0, top_k=4) and m._sample_draws == 2
    assert m._sampling_words(m._request(3, temperature=0.5, draw=7)) == FF_.sampling_words(0.5, None, 7, 7, 0) and m._sample_draws == 2
    assert m._sampling_words(m._request(3, ascending=False)) == FF_.sampling_words(0.0, 0.0, 0, 0, 0, ascending=False) and m._sample_draws == 2
    assert req.tiled(4).batch == 12 and req.tiled(4).kw is req.kw and req.tiled(4).mask is None and req.tiled(4).keep is None
    with pytest.raises(TypeError):
        m._request(3, temperatur=1.0)


def test_free_plan_decides_the_step_loops_path_once(monkeypatch):
    from polyphonic_chord_texture_disentanglement_amd import functional as F_, functional_free as FF_
    for mod, name, v in ((FF_, 'FREE_COMPOSITE', True), (FF_, 'FREE_PERSIST', True), (FF_, 'FREE_REPLAY', True), (FF_, 'NOTE_LOOP_SPLIT', None),
                         (FF_, 'NOTE_LOOP_CLUSTER', None), (FF_, 'NOTE_CLUSTER8', True), (FF_, 'NOTE_CLUSTER4_MAX_WGS', 0),
                         (F_, 'BF16_STORAGE', True), (F_, 'NOTES_PERSIST', True), (F_, 'FUSED_DUR', True)):
        monkeypatch.setattr(mod, name, v)
    B = 17
    dims = (B, 32 * B, 128, 128, 1024, 512, 64, 130)                    # init_model()
    none = ([[False] * 14] * 32, [False] * 31)
    mixed = ([[n % 2 == 0 for n in range(14)]] * 32, [t % 2 == 0 for t in range(31)])
    every_time = ([[False] * 14] * 32, [True] * 31)
    f32, kind = torch.float32, FF_.ARGMAX

    def plan(prec=1, coins=none, inference=False, needs_grad=True, forced=False, kind=kind, ncu=256, capturing=False, z=f32, dims=dims):
        return FF_._free_plan(prec, dims, z, coins, inference, needs_grad, forced, kind, ncu, capturing)
    assert FF_.FreePlan._fields[:8] == ('train', 'fast', 'comp', 'replay', 'need_resum', 'cluster', 'capturing', 'kind')
    # inference: nothing is saved, the composite runs, every time token is re-summarised, two panels take eight members each
    p = plan(inference=True, needs_grad=False, kind=FF_.SAMPLED)
    assert tuple(p) == (False, True, True, False, True, 8, False, FF_.SAMPLED, False, True)
    assert tuple(plan(inference=True)) [:6] == (False, True, True, False, True, 8)            # (a z that needs a gradient changes nothing)
    # training, all coins false: the replayed loop and the batched recompute on bf16 state copies
    p = plan()
    assert tuple(p) == (True, True, True, True, True, 8, False, kind, True, True)
    assert plan(needs_grad=False).train is False and plan(needs_grad=False).replay is False
    # training, mixed coins: the same path; only with every time coin true no token is re-summarised
    assert tuple(plan(coins=mixed)) == tuple(p)
    assert plan(coins=every_time)._replace(need_resum=True) == p and plan(coins=every_time).need_resum is False
    # force arrays: no replay
    assert plan(forced=True) == p._replace(replay=False)
    # prec = 0: the plain loop
    p0 = plan(prec=0)
    assert tuple(p0) == (True, False, False, False, True, 0, False, kind, False, False)
    assert tuple(plan(prec=0, inference=True, needs_grad=False))[:6] == (False, False, False, False, True, 0)
    # the composite needs an fp32 z and the switch; another geometry takes the plain loop
    assert plan(z=torch.float64) == p._replace(comp=False)
    monkeypatch.setattr(FF_, 'FREE_COMPOSITE', False)
    assert plan() == p._replace(comp=False)
    monkeypatch.setattr(FF_, 'FREE_COMPOSITE', True)
    assert plan(dims=(B, 32 * B, 20, 12, 40, 28, 8, 130)).fast is False
    # the cluster choice by panels and compute units, and the capture rule that zeroes it (a captured TRAINING forward only)
    assert [plan(dims=(b,) + dims[1:]).cluster for b in (16, 512, 528, 1024, 1040, 2048, 2064)] == [8, 8, 4, 4, 2, 2, 0]
    assert plan(ncu=8).cluster == 4 and plan(ncu=4).cluster == 2 and plan(ncu=2).cluster == 0
    assert plan(capturing=True) == p._replace(cluster=0, capturing=True)
    with torch.no_grad():
        assert plan(capturing=True, inference=True, needs_grad=False).cluster == 8


def test_free_pointer_tables_are_named_in_the_headers_order():
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    # include/ptvae_hip.h, ptv_free_note_loop / ptv_free_resummarize: w and io slot by slot
    assert FF_.NOTE_W == ('WG_H', 'WG_T', 'WP', 'WD_H', 'WD_P', 'WDUR', 'B_HH_N', 'B_P', 'B_DH', 'B_HH_D', 'TAB0', 'TAB', 'W_OUT_D', 'B_OUT_D',
                          'W_EMBT', 'B_EMB')
    assert FF_.NOTE_IO == ('GC', 'EMB', 'HN', 'GATES_N', 'PITCH', 'HD', 'GATES_D', 'DUR', 'IDX', 'TOK', 'PRED', 'XHAT', 'PLEN', 'FORCE_PITCH',
                           'FORCE_DUR', 'HN16', 'HD16', 'RESERVED17', 'H0GC', 'XCH', 'CNT', 'BLOCK')
    assert FF_.RESUM_W == ('E_IH', 'E_HH', 'E_IH_R', 'E_HH_R', 'B_IH', 'B_HH', 'B_IH_R', 'B_HH_R')
    assert FF_.RESUM_IO == ('PRED', 'PLEN', 'XH0', 'XH1', 'XG0', 'XG1', 'TOK_OUT')
    assert [len(n) for n in (FF_.NOTE_W, FF_.NOTE_IO, FF_.RESUM_W, FF_.RESUM_IO)] == [16, 22, 8, 7]
    assert [FF_.NOTE_IO.index(n) for n in ('H0GC', 'XCH', 'CNT', 'BLOCK')] == [18, 19, 20, 21]
    for build in (FF_.note_loop_io, FF_.resum_io):
        with pytest.raises(TypeError, match='NOPE'):
            build(NOPE=torch.zeros(1))
    # (host tensors have addresses too: omitted slots are NULL, the block is the 22nd pointer only when given)
    a, b = torch.zeros(1), torch.zeros(1)
    io = FF_.note_loop_io(PLEN=a)
    assert len(io) == 21 and io[12] == a.data_ptr() and [io[i] for i in range(21) if i != 12] == [None] * 20
    io = FF_.note_loop_io(PLEN=a, BLOCK=b)
    assert len(io) == 22 and io[12] == a.data_ptr() and io[21] == b.data_ptr()
    io = FF_.resum_io(TOK_OUT=a)
    assert len(io) == 7 and io[6] == a.data_ptr() and list(io[:6]) == [None] * 6


def test_free_branches_names_the_saved_states_kernels(monkeypatch):
    from polyphonic_chord_texture_disentanglement_amd import functional as F_, functional_free as FF_
    for mod, name, v in ((FF_, 'FREE_COMPOSITE', True), (FF_, 'FREE_PERSIST', True), (FF_, 'FREE_REPLAY', True), (FF_, 'NOTE_LOOP_SPLIT', None),
                         (FF_, 'NOTE_LOOP_CLUSTER', None), (F_, 'BF16_STORAGE', True), (F_, 'NOTES_PERSIST', True), (F_, 'FUSED_DUR', True),
                         (F_, 'HEADS_FUSED', True), (F_, 'DUR_RECOMPUTE', True)):
        monkeypatch.setattr(mod, name, v)
    B = 17
    dims = (B, 32 * B, 128, 128, 1024, 512, 64, 130)                    # init_model()
    small = (B, 32 * B, 20, 12, 40, 28, 8, 130)
    none = ([[False] * 14] * 32, [False] * 31)

    def case(prec=1, dims=dims):
        """(the plan, gates_d as the forward allocates it) of a training forward"""
        plan = FF_._free_plan(prec, dims, torch.float32, none, False, True, False, FF_.ARGMAX, 256, False)
        saves = plan.train and not (plan.replay and F_.DUR_RECOMPUTE)
        return plan, torch.empty(1, dtype=F_._act_dtype(prec, dims[6])) if saves else None

    def rule(plan, prec, dims, gates_d):
        """the three names as the forward chose them before the helper existed"""
        Hn, Hd, NP = dims[5:8]
        return ('rows' if plan.replay else 'step',
                'fused' if F_.heads_ok(prec, Hn, NP, Hd, plan.state16 or None, plan.state16 or None) else 'gemm',
                'fused16' if plan.state16 else 'fused' if F_.dur_bwd_fusable(prec, Hd, gates_d) else 'step')

    def both(prec=1, dims=dims):
        plan, gates_d = case(prec, dims)
        got = FF_._free_branches(plan, prec, dims, None if gates_d is None else gates_d.dtype)
        assert got == rule(plan, prec, dims, gates_d)
        return plan, gates_d, got
    plan, gates_d, names = both()                                     # the replayed training forward
    assert plan.replay and gates_d is None and names == ('rows', 'fused', 'fused16')
    assert both(prec=0)[2] == ('step', 'gemm', 'step')
    assert both(dims=small)[2] == ('step', 'gemm', 'step')            # (Hd = 8: no fused duration backward)
    monkeypatch.setattr(FF_, 'FREE_REPLAY', False)                    # the persistent loop's own states, with their bf16 copies
    plan, gates_d, names = both()
    assert plan.fast and plan.state16 and not plan.replay and gates_d.dtype == torch.bfloat16 and names == ('step', 'fused', 'fused16')
    monkeypatch.setattr(FF_, 'FREE_PERSIST', False)                   # the per-step loop in bf16: saved bf16 gates, fp32 states
    plan, gates_d, names = both()
    assert not plan.fast and names == ('step', 'gemm', 'fused')
    monkeypatch.setattr(F_, 'BF16_STORAGE', False)                    # ... and with fp32 gates
    assert both()[2] == ('step', 'gemm', 'step')
