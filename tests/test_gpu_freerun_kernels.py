"""ptv_free_note_loop and ptv_free_resummarize (csrc/freerun.hip) one launch at a time through the C ABI of include/ptvae_hip.h, against
the plain fp64 references of tests/freerun_ref.py: every selectable note-loop path (4-wave resident, 4-wave with streamed heads, 8-wave
split, clusters of 2 / 4 / 8) in its FORCE and its plain instantiation, each held to the reference on its own and never to another path,
at the smallest shapes where these kernels can go wrong -- B = 1, 15, 16, 17, 33 (a lone row, a panel short by one, an exact panel, a
one-row tail panel, three panels with a tail), t = 0, 13, 31 (B = 33 with t = 31 reaches the last row of every tensor), two pitch strides.

Inputs are built on the CPU from seeded generators (freerun_ref.weights / inputs); everything a kernel consumes as bf16 is
bf16-representable, so kernel and reference see the same numbers; the packs are made by the project's own ptv_pack_mfma_b path.
FORCED REPLAY is the main check: the reference runs free, its decisions become the force arrays, and every floating-point output of the
rows of t is compared with the fp64 reference.  There is no pre-chosen tolerance: the same formulas are evaluated on the CPU in fp32
with bf16 rounding where the kernels round (freerun_ref.kp_*), that evaluation's error against the reference is measured per note-step
(or duration-step) plane, and the kernel's error may be at most 4x that with a floor of 8 fp32 ulps of the plane's scale (bound_of of
test_gpu_dur_kernels.py).  The bound never sees the kernel's output.  Integer outputs are exact; HN16 / HD16 are the RNE of the fp32
state of the same launch, bit for bit; every decision without a force word is the first maximal index of the logits the same launch
emitted.  FREE runs (no force arrays) on the 'wide' inputs follow the reference's trajectory: a first difference must be a near-tie
of the reference (margin <= 2 x that plane's logit bound), and at most 2 % of a case's decisions may lie behind first differences.
Every output is pre-filled with a sentinel and carries pad elements behind its end: other time steps' rows and the pad keep it, inputs
compare equal with their copies.  Every launch is synchronised before and after.  Each check prints `FREERUN_RATIO family
kernel-error/bound` (pytest -s; table in profiles/LOG.md)."""
import functools

import numpy as np
import pytest
import torch

import freerun_ref as R
from test_gpu_dur_kernels import bound_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT, ISENT = 768.0, -7                                                 # (768 is exact in bf16)
BF = torch.bfloat16
PAD = 1536                                                              # sentinel elements behind the end of every output
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
RATIOS = {}
GATES = ((0, 'r'), (1, 'z'), (2, 'n'), (3, 'hn'))
F32, I32, I64 = torch.float32, torch.int32, torch.int64
# name -> (dtype, shape from (B, R, ld), the axis that holds the R rows); xhat's rows are [:, t]
NOTE_OUT = {'HN': (F32, lambda B, R, ld: (16, R, 512), 1), 'gates_n': (BF, lambda B, R, ld: (15, 4, R, 512), 2),
            'pitch': (F32, lambda B, R, ld: (15, R, ld), 1), 'HD': (F32, lambda B, R, ld: (6, 15, R, 64), 2),
            'gates_d': (BF, lambda B, R, ld: (5, 4, 15, R, 64), 3), 'dur': (F32, lambda B, R, ld: (15, R, 10), 1),
            'idx': (I32, lambda B, R, ld: (5, 15, R), 2), 'TOK': (F32, lambda B, R, ld: (15, R, 128), 1),
            'PRED': (F32, lambda B, R, ld: (16, R, 128), 1), 'xhat': (I64, lambda B, R, ld: (B, 32, 16, 6), None),
            'plen': (I32, lambda B, R, ld: (R,), 0), 'HN16': (BF, lambda B, R, ld: (16, R, 512), 1),
            'HD16': (BF, lambda B, R, ld: (6, 15, R, 64), 2)}
RESUM_OUT = {'XH0': (F32, lambda B, R, ld: (17, R, 128), 1), 'XH1': (F32, lambda B, R, ld: (17, R, 128), 1),
             'XG0': (BF, lambda B, R, ld: (16, 4, R, 128), 2), 'XG1': (BF, lambda B, R, ld: (16, 4, R, 128), 2),
             'tok_next': (F32, lambda B, R, ld: (B, 256), None)}


def lib():
    from polyphonic_chord_texture_disentanglement_amd._lib import lib as _l
    return _l()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))                                  # (a writable copy: the cached inputs are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.float().cpu().numpy() if t.dtype == BF else t.cpu().numpy()


def check(family, got, ref, kp):
    """got against ref plane by plane (the first axis): each plane under its own bound_of(ref, kp)"""
    got, ref, kp = (np.asarray(a, np.float64) for a in (got, ref, kp))
    assert got.shape == ref.shape == kp.shape, (family, got.shape, ref.shape, kp.shape)
    assert np.isfinite(got).all(), '%s: non-finite output' % family
    worst, msg = 0.0, None
    for i in range(got.shape[0]):
        bound, errk = bound_of(ref[i], kp[i])
        err = np.abs(got[i] - ref[i]).max()
        ratio = float(err / bound)
        if ratio > worst:
            worst, msg = ratio, 'plane %d: kernel error %.3e over the bound %.3e (kernel-precision CPU evaluation: %.3e)' % (i, err, bound, errk)
    RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    print('FREERUN_RATIO %s %.3f' % (family, worst))
    assert worst <= 1.0, '%s: %s' % (family, msg)


@pytest.fixture(scope='module', autouse=True)
def ratio_table():
    yield
    for k in sorted(RATIOS):
        print('FREERUN_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


# ================================================================================================ device side
@functools.lru_cache(maxsize=None)
def wdev(wset):
    """the weights of a set on the device: the sixteen `w` entries of the note loop (packs by ptv_pack_mfma_b) and the eight of the
    re-summarisation, each with a copy to compare with after the launches"""
    from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_
    W = R.weights(wset)
    d = {k: dev(W[k]) for k in ('w_hh_n', 'w_ih_tok', 'w_p', 'w_dh_h', 'w_dh_p', 'w_hh_d', 'b_hh_n', 'b_p', 'b_dh', 'b_hh_d', 'tab0', 'tab',
                                'w_out', 'b_out', 'w_embT', 'b_emb')}
    wl = [FF_._pack(d[k]) for k in ('w_hh_n', 'w_ih_tok', 'w_p', 'w_dh_h', 'w_dh_p', 'w_hh_d')]
    wl += [d[k] for k in ('b_hh_n', 'b_p', 'b_dh', 'b_hh_d', 'tab0', 'tab', 'w_out', 'b_out', 'w_embT', 'b_emb')]
    for k in ('e_w_ih', 'e_w_hh'):
        d[k] = [dev(W[k][0]), dev(W[k][1])]
    wr = [FF_._pack(d['e_w_ih'][0]), FF_._pack(d['e_w_hh'][0]), FF_._pack(d['e_w_ih'][1]), FF_._pack(d['e_w_hh'][1]),
          dev(W['e_b_ih'][0]), dev(W['e_b_hh'][0]), dev(W['e_b_ih'][1]), dev(W['e_b_hh'][1])]
    torch.cuda.synchronize()
    return dict(wl=wl, wr=wr, wl_copy=[t.clone() for t in wl], wr_copy=[t.clone() for t in wr])


def outputs(spec, names, B, ld=136):
    """sentinel-filled outputs with PAD sentinel elements behind the end -> {name: (flat, view)}"""
    out = {}
    for k in names:
        dt, shape, _ = spec[k]
        shape = shape(B, 32 * B, ld)
        flat = torch.full((int(np.prod(shape)) + PAD,), ISENT if dt in (I32, I64) else SENT, dtype=dt, device=DEV)
        out[k] = (flat, flat[:int(np.prod(shape))].view(shape))
    return out


def rows_of(spec, k, v, t, B):
    ax = spec[k][2]
    if k == 'xhat':
        return v[:, t]
    return v if ax is None else v.narrow(ax, t * B, B)


def take_rows(spec, out, t, B):
    """the rows of t of every output as host arrays; on the device those rows are then reset to the sentinel, so that afterwards
    `untouched` holds iff nothing outside them was written"""
    got = {}
    for k, (flat, v) in out.items():
        r = rows_of(spec, k, v, t, B)
        got[k] = host(r.clone())
        r.fill_(ISENT if flat.dtype in (I32, I64) else SENT)
    return got


def untouched(out):
    return [k for k, (flat, _) in out.items() if not bool((flat == (ISENT if flat.dtype in (I32, I64) else SENT)).all())]


def parr(ts):
    from polyphonic_chord_texture_disentanglement_amd import functional as F_
    return F_._parr(ts)


def stream():
    from polyphonic_chord_texture_disentanglement_amd._lib import stream_ptr
    return stream_ptr()


def call_note_loop(wl, io, ld, B, t, coin, train):
    """one synchronised launch -> the status code"""
    torch.cuda.synchronize()
    rc = lib().ptv_free_note_loop(parr(wl), parr(io), ld, B, t, coin, train, stream())
    torch.cuda.synchronize()
    return rc


def call_resummarize(wr, io, B, t, train):
    torch.cuda.synchronize()
    rc = lib().ptv_free_resummarize(parr(wr), parr(io), B, t, train, stream())
    torch.cuda.synchronize()
    return rc


class NoteRun:
    """the buffers of one case: outputs (sentinel), inputs of the launches and their copies"""

    def __init__(self, c):
        self.c, self.B, self.R, self.ld = c, c['B'], 32 * c['B'], c['ld']
        names = [k for k in NOTE_OUT if c['s16'] or k not in ('HN16', 'HD16')]
        self.out = outputs(NOTE_OUT, names, self.B, self.ld)
        self.S = R.CLUSTER.get(c['path'], 1)
        self.panels = (self.B + 15) // 16
        self.xch = torch.zeros(self.panels * 2 * 16 * 512 * 2, dtype=BF, device=DEV) if self.S > 1 else None
        self.cnt = torch.zeros(self.panels + 1, dtype=I32, device=DEV) if self.S > 1 else None
        self.launches = 0

    def v(self, k):
        return self.out[k][1] if k in self.out else None

    def launch(self, t, x, force, train_extra=0):
        """write the caller's part (slot 0 of HN unless io[18], slot 0 of TOK, zeroed plen rows), launch, compare the inputs with their
        copies -> status code"""
        c, B, R_ = self.c, self.B, self.R
        gc, h0, tok0, emb = x
        wd = wdev(c['wset'])
        rows = slice(t * B, (t + 1) * B)
        ins = {}
        if c['h0gc']:
            ins['h0gc'] = dev(np.concatenate([h0, gc], axis=1))
        else:
            ins['gc'] = dev(gc)
            self.v('HN')[0, rows] = dev(h0)
        self.v('TOK')[0, rows] = dev(tok0)
        self.v('plen')[rows] = 0
        if c['coin']:
            e = np.full((16, R_, 128), SENT, np.float32)                    # other time steps' rows: nothing the decode may feed
            e[:, rows] = emb
            ins['emb'] = dev(e)
        if force[0] is not None:
            fp, fd = np.full((15, R_), 3, np.int32), np.full((5, 15, R_), 1, np.int32)
            fp[:, rows], fd[:, :, rows] = force
            ins['fp'], ins['fd'] = dev(fp), dev(fd)
        if c['samp']:                                                   # {uint64 seed, uint64 draw, int64 sample_offset, float T_pitch, float T_dur}
            blk = np.array([12345, 3, 0, 0], np.int64)
            blk[3:].view(np.float32)[:] = (1.0, 0.7)
            ins['samp'] = dev(blk)
            train_extra |= R.BIT_SAMPLE
        copies = {k: a.clone() for k, a in ins.items()}
        io = [ins.get('gc'), ins.get('emb'), self.v('HN'), self.v('gates_n'), self.v('pitch'), self.v('HD'), self.v('gates_d'), self.v('dur'),
              self.v('idx'), self.v('TOK'), self.v('PRED'), self.v('xhat'), self.v('plen'), ins.get('fp'), ins.get('fd'), self.v('HN16'),
              self.v('HD16'), None, ins.get('h0gc'), self.xch, self.cnt, ins.get('samp')]
        train = c['mode'] | R.PATHS[c['path']] | train_extra
        if self.S > 1 and self.panels * self.S > torch.cuda.get_device_properties(DEV).multi_processor_count:
            assert call_note_loop(wd['wl'], io, self.ld, B, t, c['coin'], train) == ERR_UNSUPPORTED
            pytest.skip('more cluster members than CUs')
        rc = call_note_loop(wd['wl'], io, self.ld, B, t, c['coin'], train)
        self.launches += rc == OK
        for k, a in ins.items():
            assert torch.equal(a, copies[k]), 'input %s changed' % k
        for a, b in zip(wd['wl'], wd['wl_copy']):
            assert torch.equal(a, b), 'a weight changed'
        if self.S > 1 and rc == OK:
            cnt = self.cnt.cpu().numpy()
            assert cnt[-1] == 0 and (cnt[:-1] == 15 * self.S * self.launches).all(), cnt
        return rc

    def take(self, t):
        return take_rows(NOTE_OUT, self.out, t, self.B)


# ================================================================================================ what a launch must have written
def rne_bits(a):
    return R.bf16_round(np.asarray(a, np.float32)).view(np.uint32)


def check_structure(c, got, x, force, tag):
    """everything that holds for any launch, with or without force arrays, judged on the launch's own outputs: sentinels where the mode
    writes nothing, the caller's slots, decisions = force word or first maximal index of the emitted logits, integers consistent, PRED the
    fp32 embedding of the decisions, TOK the coin's choice, HN16 / HD16 the RNE of the states"""
    gc, h0, tok0, emb = x
    B, mode, W = c['B'], c['mode'], R.weights(c['wset'])
    fs = lambda a: bool((a == SENT).all())
    assert fs(got['pitch'][:, :, R.NP:]) and fs(got['PRED'][0]) and (got['xhat'][:, 0] == ISENT).all(), tag
    assert np.array_equal(got['TOK'][0], tok0) and np.array_equal(got['HN'][0], h0), tag
    if mode != 1:                                                       # what only the backward reads keeps its sentinel
        assert fs(got['HN'][1:]) and fs(got['gates_n']) and fs(got['HD']) and fs(got['gates_d']), tag
    if mode == 0:
        assert fs(got['TOK'][1:]), tag
    if c['s16']:
        if mode == 1:
            assert fs(got['HD'][1:]), tag                               # HD16 replaces HD[1..5]
            assert np.array_equal(got['HN16'].view(np.uint32), rne_bits(got['HN'])), tag
            assert np.array_equal(got['HD16'][0].view(np.uint32), rne_bits(got['HD'][0])), tag
        else:
            assert fs(got['HN16']) and fs(got['HD16']), tag
    logit, est = got['pitch'][:, :, :R.NP], got['dur']
    assert np.isfinite(logit).all() and np.isfinite(est).all(), tag
    pidx, idx = got['xhat'][:, 1:, 0].T, got['idx'].astype(np.int64)
    fp, fd = force
    want_p = np.argmax(logit, axis=-1) if fp is None else np.where(fp >= 0, fp, np.argmax(logit, axis=-1))
    free_d = (est[:, :, 1::2] > est[:, :, 0::2]).astype(np.int64).transpose(2, 0, 1)
    want_d = free_d if fd is None else np.where(fd >= 0, fd, free_d)
    assert np.array_equal(pidx, want_p), (tag, np.argwhere(pidx != want_p)[:4])
    assert np.array_equal(idx, want_d), (tag, np.argwhere(idx != want_d)[:4])
    assert np.array_equal(got['xhat'][:, 1:, 1:], idx.transpose(2, 1, 0)), tag
    eos = pidx == R.EOS
    assert np.array_equal(got['plen'], np.where(eos.any(0), eos.argmax(0) + 1, 15)), tag
    pred = (W['b_emb'] + W['w_embT'][pidx]).astype(np.float32)
    for d in range(5):
        pred = (pred + idx[d][:, :, None].astype(np.float32) * W['w_embT'][R.NP + d]).astype(np.float32)
    assert np.array_equal(got['PRED'][1:], pred), (tag, np.abs(got['PRED'][1:] - pred).max())
    if mode:
        for n in range(14):
            assert np.array_equal(got['TOK'][n + 1], emb[n + 1] if (c['coin'] >> n) & 1 else got['PRED'][n + 1]), (tag, n)
    return pidx, idx


def check_floats(c, got, ref, kp, tag):
    """every floating-point output of the rows of t against the fp64 reference of the same decisions, per plane"""
    p, mode = c['path'], c['mode']
    ks = R.to_stored(kp)
    check(p + '.pitch', got['pitch'][:, :, :R.NP], ref['pitch'], kp['pitch'])
    check(p + '.dur', got['dur'].reshape(15, -1, 5, 2).transpose(2, 0, 1, 3), ref['dur'].reshape(15, -1, 5, 2).transpose(2, 0, 1, 3),
          kp['dur'].reshape(15, -1, 5, 2).transpose(2, 0, 1, 3))
    check(p + '.PRED', got['PRED'][1:], ref['PRED'][1:], kp['PRED'][1:])
    if mode:
        check(p + '.TOK', got['TOK'][1:], ref['TOK'][1:], kp['TOK'][1:])
    if mode == 1:
        check(p + '.HN', got['HN'][1:], ref['HN'][1:], kp['HN'][1:])
        check(p + '.HD', got['HD'][:1], ref['HD'][:1], kp['HD'][:1])
        if c['s16']:
            check(p + '.HD16', got['HD16'][1:], ref['HD'][1:], ks['HD16'][1:])
        else:
            check(p + '.HD', got['HD'][1:], ref['HD'][1:], kp['HD'][1:])
        for g, name in GATES:
            check('%s.gates_n.%s' % (p, name), got['gates_n'][:, g], ref['gates_n'][:, g], ks['gates_n'][:, g])
            check('%s.gates_d.%s' % (p, name), got['gates_d'][:, g], ref['gates_d'][:, g], ks['gates_d'][:, g])


def check_ints(got, ref, tag):
    assert np.array_equal(got['idx'], ref['idx']) and np.array_equal(got['xhat'][:, 1:], ref['xhat']) and np.array_equal(got['plen'], ref['plen']), tag


@functools.lru_cache(maxsize=None)
def kp_replay(wset, B, seed, coin):
    """the kernel-precision evaluation that replays the reference's decisions (shared, read only)"""
    ref = R._ref_free(wset, B, seed, coin)
    gc, h0, tok0, emb = R.inputs(B, seed, wset)
    return R.kp_note_loop(R.weights(wset), gc, h0, tok0, emb, coin, *R.decisions(ref))


# ================================================================================================ the note loop
@pytest.mark.parametrize('c', R.REPLAY_CASES, ids=R.case_id)
def test_note_loop_forced_replay_vs_fp64_reference(c):
    W, x, ref, force = R.case_data(c)
    run = NoteRun(c)
    assert run.launch(c['t'], x, force) == OK
    got = run.take(c['t'])
    assert untouched(run.out) == []
    tag = R.case_id(c)
    check_structure(c, got, x, force, tag)
    check_ints(got, ref, tag)
    check_floats(c, got, ref, kp_replay(c['wset'], c['B'], c['seed'], c['coin']), tag)


@pytest.mark.parametrize('c', R.FREE_CASES, ids=R.case_id)
def test_note_loop_free_decisions_and_trajectory(c):
    """no force arrays (the FORCE = 0 instantiation): every decision is the first maximal index of the emitted logits (exact); on the 'wide'
    inputs the trajectory is the reference's up to near-ties of the reference"""
    W, x, ref, force = R.case_data(c)
    run = NoteRun(c)
    assert run.launch(c['t'], x, force) == OK
    got = run.take(c['t'])
    assert untouched(run.out) == []
    tag = R.case_id(c)
    pidx, idx = check_structure(c, got, x, force, tag)
    if c['wset'] != 'wide':
        return
    kp = kp_replay(c['wset'], c['B'], c['seed'], c['coin'])
    bp, bd = R.plane_bounds(ref, kp, bound_of)
    first, left = R.walk(ref, pidx, idx)
    for b, n, k in first:                                               # a first difference must be a near-tie of the reference
        assert R.margin_at(ref, b, n, k) <= 2 * (bp[n] if k < 0 else bd[k]), (tag, b, n, k, R.margin_at(ref, b, n, k))
    print('FREERUN_LEFT_OUT %s %d of %d' % (tag, left, 90 * c['B']))
    assert left <= 0.02 * 90 * c['B'], (tag, first, left)
    if not first:                                                       # the same decisions everywhere: the floats are the replay's
        check_ints(got, ref, tag)
        check_floats(c, got, ref, kp, tag)


@pytest.mark.parametrize('c', R.PARTIAL_CASES, ids=R.case_id)
def test_note_loop_obeys_the_forced_entries_and_decides_the_rest(c):
    W, x, ref, force = R.case_data(c)
    assert (force[0] >= 0).sum() >= 3 and (force[1] >= 0).sum() >= 3 and (force[0] < 0).sum() > 200
    run = NoteRun(c)
    assert run.launch(c['t'], x, force) == OK
    got = run.take(c['t'])
    assert untouched(run.out) == []
    pidx, idx = check_structure(c, got, x, force, R.case_id(c))       # (force word where >= 0, the argmax of the emitted logits elsewhere)
    assert (pidx[force[0] >= 0] == force[0][force[0] >= 0]).all() and (idx[force[1] >= 0] == force[1][force[1] >= 0]).all()
    assert (pidx[0] != ref['pidx'][0]).any() or (idx[:, 0] != ref['idx'][:, 0]).any()     # obeying shows: the forced values are not the reference's


@pytest.mark.parametrize('c', R.TIE_CASES, ids=R.case_id)
def test_note_loop_ties_go_to_the_lower_index(c):
    """pitch-head rows 7 and 77 (different 16-row tiles) identical under the largest bias, the two rows of dur_out_linear identical: the
    emitted logits of each pair are the same bits, the decisions 7 and 0"""
    W, x, ref, force = R.case_data(c)
    run = NoteRun(c)
    assert run.launch(c['t'], x, force) == OK
    got = run.take(c['t'])
    assert untouched(run.out) == []
    pidx, idx = check_structure(c, got, x, force, R.case_id(c))
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(u(got['pitch'][:, :, 7]), u(got['pitch'][:, :, 77]))
    assert (got['pitch'][:, :, 7:8] >= got['pitch'][:, :, :R.NP]).all() and (pidx == 7).all()
    assert np.array_equal(u(got['dur'][:, :, 0::2]), u(got['dur'][:, :, 1::2])) and (idx == 0).all()
    check(c['path'] + '.pitch', got['pitch'][:, :, :R.NP], ref['pitch'], kp_replay(c['wset'], c['B'], c['seed'], c['coin'])['pitch'])


@pytest.mark.parametrize('c', R.SEQ_CASES, ids=R.case_id)
def test_note_loop_two_time_steps_on_the_same_buffers(c):
    """t = 0 then t = 1: the cluster's step tags and arrival counters run on, the rows of t = 0 stay as written"""
    run = NoteRun(c)
    tag = R.case_id(c)
    first = None
    for t in (0, 1):
        W, x, ref, force = R.case_data(c, t_offset=t)
        assert run.launch(t, x, force) == OK
        if t == 1:                                                      # the rows of t = 0 as the first launch left them
            again = {k: host(rows_of(NOTE_OUT, k, v, 0, c['B'])) for k, (_, v) in run.out.items()}
            for k in again:
                assert np.array_equal(again[k], first[k], equal_nan=True), (tag, k)
            for k, (flat, v) in run.out.items():
                rows_of(NOTE_OUT, k, v, 0, c['B']).fill_(ISENT if flat.dtype in (I32, I64) else SENT)
            got = run.take(1)
            assert untouched(run.out) == []
        else:
            first = {k: host(rows_of(NOTE_OUT, k, v, 0, c['B']).clone()) for k, (_, v) in run.out.items()}
            got = first
        check_structure(c, got, x, force, tag)
        check_ints(got, ref, tag)
        check_floats(c, got, ref, kp_replay(c['wset'], c['B'], c['seed'] + 7 * t, c['coin']), tag)


def test_note_loop_refuses_bad_arguments_and_writes_nothing():
    c = R.case('res', 16, 0, 1, 'init', seed=90, coin=0)
    W, x, ref, force = R.case_data(c)
    gc, h0, tok0, emb = x
    wd = wdev('init')
    run = NoteRun(dict(c, s16=1))
    B, Rr = 16, 512
    gcd, embd = dev(gc), dev(np.zeros((16, Rr, 128), np.float32))
    xch, cnt = torch.zeros(2 * 16 * 512 * 2, dtype=BF, device=DEV), torch.zeros(2, dtype=I32, device=DEV)
    v = run.v
    base = [gcd, embd, v('HN'), v('gates_n'), v('pitch'), v('HD'), v('gates_d'), v('dur'), v('idx'), v('TOK'), v('PRED'), v('xhat'), v('plen'),
            None, None, v('HN16'), v('HD16'), None, None, xch, cnt]

    def refused(what, wl=None, io=None, B=16, t=0, coin=0, train=1 | R.BIT_4WAVE, want=ERR_ARG):
        rc = call_note_loop(wd['wl'] if wl is None else wl, base if io is None else io, 136, B, t, coin, train)
        assert rc == want, (what, rc)
        assert untouched(run.out) == [], what
        assert int(cnt.abs().sum()) == 0 and int(xch.float().abs().sum()) == 0, what

    def without(lst, *idx):
        return [None if i in idx else a for i, a in enumerate(lst)]

    for i in (0, 5, 7, 15):
        refused('w[%d] NULL' % i, wl=without(wd['wl'], i))
    for i in (2, 4, 7, 8, 9, 10, 11, 12):
        refused('io[%d] NULL' % i, io=without(base, i))
    refused('neither gc nor [h0 | gc]', io=without(base, 0))
    for i in (3, 5, 6):
        refused('train mode without io[%d]' % i, io=without(base, i))
    refused('coin_mask without emb', io=without(base, 1), coin=0x15a5)
    refused('t = 32', t=32)
    refused('t = -1', t=-1)
    refused('B = 0', B=0)
    refused('B < 0', B=-16)
    for bits in (2 << 18, 4 << 18, R.BIT_S8):
        refused('cluster with the 8-wave bit', train=bits | R.BIT_8WAVE)
    refused('a cluster of 3', train=3 << 18, want=ERR_UNSUPPORTED)
    refused('cluster without xch / cnt', io=without(base, 19, 20), train=2 << 18, want=ERR_UNSUPPORTED)


# ================================================================================================ the re-summarisation
def resum_inputs(B, t, kind):
    rng = np.random.RandomState(500 + 3 * B + t)
    return rng.normal(0, 0.5, (16, B, R.E)).astype(np.float32), R.resum_lengths(B, kind)


@pytest.mark.parametrize('B,t,train,kind', R.RESUM_CASES)
def test_resummarize_vs_fp64_reference(B, t, train, kind):
    """flags 0 and 2 (next token only) and 1 and 3 (states and gates saved), resident and streamed weights, each held to the reference"""
    W, wd = R.weights('init'), wdev('init')
    PRED, plen = resum_inputs(B, t, kind)
    ref, kp = R.resummarize(W, PRED, plen), R.to_stored_resum(R.kp_resummarize(W, PRED, plen))
    Rr, rows = 32 * B, slice(t * B, (t + 1) * B)
    P = np.full((16, Rr, R.E), SENT, np.float32)
    L = np.full(Rr, 16, np.int32)                                       # other time steps: every step live, garbage tokens
    P[:, rows], L[rows] = PRED, plen
    Pd, Ld = dev(P), dev(L)
    out = outputs(RESUM_OUT, list(RESUM_OUT), B)
    io = [Pd, Ld] + [out[k][1] for k in ('XH0', 'XH1', 'XG0', 'XG1', 'tok_next')]
    assert call_resummarize(wd['wr'], io, B, t, train) == OK
    assert torch.equal(Pd, dev(P)) and torch.equal(Ld, dev(L))
    for a, b in zip(wd['wr'], wd['wr_copy']):
        assert torch.equal(a, b)
    got = take_rows(RESUM_OUT, out, t, B)
    assert untouched(out) == []
    fam = 'resum%d' % train
    check(fam + '.tok_next', got['tok_next'][None], ref['tok_next'][None], kp['tok_next'][None])
    for dr in range(2):
        XH, XG = got['XH%d' % dr], got['XG%d' % dr]
        if not train & 1:
            assert (XH == SENT).all() and (XG == SENT).all()
            continue
        assert (XH[0] == SENT).all()                                    # slot 0 is the caller's
        check(fam + '.XH', XH[1:], ref['XH'][dr, 1:], kp['XH'][dr, 1:])
        for g, name in GATES:
            check('%s.XG.%s' % (fam, name), XG[:, g], ref['XG'][dr, :, g], kp['XG'][dr, :, g])
        for s in range(16):
            dead = (15 - s if dr else s) >= plen
            assert (XG[s, 0][dead] == 0).all() and (XG[s, 1][dead] == 1).all() and (XG[s, 2][dead] == 0).all(), (dr, s)
            assert np.array_equal(XH[s + 1][dead], (XH[s] if s else np.zeros_like(XH[1]))[dead]), (dr, s)
        if kind == 'empty':
            assert (XH[1:] == 0).all()
    if kind == 'empty':
        assert (got['tok_next'] == 0).all()


def test_resummarize_refuses_bad_arguments_and_writes_nothing():
    wd = wdev('init')
    B = 16
    Pd, Ld = dev(np.zeros((16, 32 * B, R.E), np.float32)), dev(np.full(32 * B, 3, np.int32))
    out = outputs(RESUM_OUT, list(RESUM_OUT), B)
    base = [Pd, Ld] + [out[k][1] for k in ('XH0', 'XH1', 'XG0', 'XG1', 'tok_next')]

    def refused(what, wr=None, io=None, B=16, t=0, train=1):
        rc = call_resummarize(wd['wr'] if wr is None else wr, base if io is None else io, B, t, train)
        assert rc == ERR_ARG, (what, rc)
        assert untouched(out) == [], what

    for i in (0, 3, 7):
        refused('w[%d] NULL' % i, wr=[None if j == i else a for j, a in enumerate(wd['wr'])])
    for i in (0, 1, 6):
        refused('io[%d] NULL' % i, io=[None if j == i else a for j, a in enumerate(base)], train=0)
    for i in (2, 3, 4, 5):
        refused('train without io[%d]' % i, io=[None if j == i else a for j, a in enumerate(base)])
    refused('t = 32', t=32)
    refused('t = -1', t=-1)
    refused('B = 0', B=0)
