"""Guards tests/freerun_ref.py, the fp64 references of the free-running note loop and of the re-summarisation (csrc/freerun.hip): held to
oracle/ptvae_oracle.py's decode_notes / decode_note and _bigru_final run in torch float64 on the same weights mapped into a parameter dict
(free, teacher-forced by coins, and with every decision forced); the kernel-precision evaluations against the references (off by what
bf16 operands allow, and not by nothing); the case tables of tests/test_gpu_freerun_kernels.py (every path, mode, FORCE instantiation,
batch, time step, <eos> at note step 0 / never / later, the tie weights); and the inputs of the free-trajectory cases (every reference
margin above twice its plane's bound, the kernel-precision trajectory inside the left-out cap).  No GPU.  fp64 against fp64: 1e-11."""
import numpy as np
import pytest
import torch

import freerun_ref as R
from test_gpu_dur_kernels import bound_of

TOL = 1e-11
HT = 8                                                      # width of the time-step summary in the oracle's parameter dict


def close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.allclose(got, want, rtol=tol, atol=tol), np.abs(got - want).max()


@pytest.fixture
def f64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                  # the oracle builds its one-hot tokens in the default dtype
    yield
    torch.set_default_dtype(old)


def oracle_of(W, rng):
    """an Oracle over the weights of freerun_ref.weights(): the kernel's split tensors put back into the reference's state_dict layout,
    with a random time-summary part (Ht = HT) in front of the notes GRU's input weight -> oracle, W_ih[:, :Ht], b_ih, (W, b) of
    dec_time_to_notes_hid"""
    from oracle.ptvae_oracle import Oracle
    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    w_head, b_ih = rng.normal(0, 0.3, (3 * R.HN, HT)), rng.normal(0, 0.3, 3 * R.HN)
    w_t2n, b_t2n = rng.normal(0, 0.3, (R.HN, HT)), rng.normal(0, 0.3, R.HN)
    p = {'dec_time_to_notes_hid.weight': w_t2n, 'dec_time_to_notes_hid.bias': b_t2n,
         'dec_notes_gru.weight_ih_l0': np.concatenate([w_head, W['w_ih_tok']], 1), 'dec_notes_gru.weight_hh_l0': W['w_hh_n'],
         'dec_notes_gru.bias_ih_l0': b_ih, 'dec_notes_gru.bias_hh_l0': W['b_hh_n'],
         'pitch_out_linear.weight': W['w_p'], 'pitch_out_linear.bias': W['b_p'],
         'dur_hid_linear.weight': np.concatenate([W['w_dh_h'], W['w_dh_p']], 1), 'dur_hid_linear.bias': W['b_dh'],
         'dur_sos_token': W['sos'], 'dec_dur_gru.weight_ih_l0': W['w_ih_d'], 'dec_dur_gru.weight_hh_l0': W['w_hh_d'],
         'dec_dur_gru.bias_ih_l0': W['b_ih_d'], 'dec_dur_gru.bias_hh_l0': W['b_hh_d'],
         'dur_out_linear.weight': W['w_out'], 'dur_out_linear.bias': W['b_out'],
         'note_embedding.weight': W['w_emb'], 'note_embedding.bias': W['b_emb']}
    for dr, s in enumerate(('', '_reverse')):
        p['dec_notes_emb_gru.weight_ih_l0' + s], p['dec_notes_emb_gru.weight_hh_l0' + s] = W['e_w_ih'][dr], W['e_w_hh'][dr]
        p['dec_notes_emb_gru.bias_ih_l0' + s], p['dec_notes_emb_gru.bias_hh_l0' + s] = W['e_b_ih'][dr], W['e_b_hh'][dr]
    orc = Oracle.__new__(Oracle)
    orc.p = {'decoder.' + k: T(v) for k, v in p.items()}
    orc.trace, orc.force = {'pitch_inds': {}, 'dur_inds': {}}, None
    return orc, w_head, b_ih, w_t2n, b_t2n


@pytest.mark.parametrize('wset,B,coin,forced', [('init', 5, 0, False), ('init', 7, 0x15a5, False), ('wide', 6, 0x3fff, False),
                                                ('wide', 4, 0, False), ('init', 5, 0x2b3, True), ('tie', 3, 0, False)])
def test_note_loop_is_the_oracles_decode_notes(f64_default, wset, B, coin, forced):
    """note_loop (fp64) against Oracle.decode_notes on the same weights: logits, predicted tokens, decisions and lengths; with coins the
    oracle is fed the same ground-truth notes; `forced` replays random decisions through both"""
    W = R.weights(wset)
    rng = np.random.RandomState(B + coin)
    orc, w_head, b_ih, w_t2n, b_t2n = oracle_of(W, rng)
    ns = rng.normal(0, 1, (B, HT))
    _, _, tok0, emb = R.inputs(B, 3, wset)
    gc, h0 = ns @ w_head.T + b_ih, ns @ w_t2n.T + b_t2n                       # what the caller's product hands the kernel, here in fp64
    fp = fd = None
    if forced:
        fp, fd = rng.randint(0, R.NP, (15, B)), rng.randint(0, 2, (5, 15, B))
        orc.force = {'pitch_inds': {(4, n): torch.tensor(fp[n]) for n in range(15)},
                     'dur_inds': {(4, n): torch.tensor(fd[:, n].T.copy()) for n in range(15)}}
    W = dict(W)                                                                # (the tables as the fp64 products they round: the oracle forms them so)
    W['tab0'], W['tab'] = R.D.gate_tables(W['w_ih_d'], W['b_ih_d'], W['sos'])
    got = R.note_loop(W, gc, h0, tok0, emb, coin, fp, fd)
    notes = torch.tensor(np.asarray(emb, np.float64).transpose(1, 0, 2).copy())
    notes[:, 0] = torch.tensor(np.asarray(tok0, np.float64))
    bits = iter([(coin >> n) & 1 for n in range(14)])
    po, do, pred, length = orc.decode_notes(torch.tensor(ns), notes, False, 0.5, lambda: 0.0 if next(bits) else 1.0, 4)
    close(got['pitch'], po.numpy().transpose(1, 0, 2))
    close(got['dur'], do.numpy().reshape(B, 15, 10).transpose(1, 0, 2))
    close(got['PRED'], pred.numpy().transpose(1, 0, 2))
    assert np.array_equal(got['plen'], length.numpy().astype(np.int64))
    for n in range(15):
        assert np.array_equal(got['pidx'][n], orc.trace['pitch_inds'][(4, n)].numpy())
        assert np.array_equal(got['idx'][:, n].T, orc.trace['dur_inds'][(4, n)].numpy())
    assert np.array_equal(got['xhat'][:, :, 0], got['pidx'].T) and np.array_equal(got['xhat'][:, :, 1:], got['idx'].transpose(2, 1, 0))
    # the fed tokens: the ground truth where the coin says so, the prediction otherwise; the states chain through the saved gates
    for n in range(14):
        assert np.array_equal(got['TOK'][n + 1], np.asarray(emb[n + 1], np.float64) if (coin >> n) & 1 else got['PRED'][n + 1])
    r, z, nn, hn = got['gates_n'].transpose(1, 0, 2, 3)
    close(got['HN'][1:], (1 - z) * nn + z * got['HN'][:-1])
    r, z, nn, hn = got['gates_d'].transpose(1, 0, 2, 3, 4)
    close(got['HD'][1:], (1 - z) * nn + z * got['HD'][:-1])
    if wset == 'tie':                                                              # first maximal index: 7 before 77, bit 0 before bit 1
        assert (got['pitch'][:, :, 7] == got['pitch'][:, :, 77]).all() and (got['pidx'] == 7).all() and (got['margin_p'] == 0).all()
        assert (got['dur'][:, :, 0::2] == got['dur'][:, :, 1::2]).all() and (got['idx'] == 0).all()


@pytest.mark.parametrize('B,kind', [(9, 'mixed'), (3, 'full'), (2, 'empty')])
def test_resummarize_is_the_oracles_packed_bigru(f64_default, B, kind):
    W = R.weights('init')
    rng = np.random.RandomState(B)
    orc = oracle_of(W, rng)[0]
    PRED, plen = rng.normal(0, 0.5, (16, B, R.E)), R.resum_lengths(B, kind)
    got = R.resummarize(W, PRED, plen)
    want = orc._bigru_final('decoder.dec_notes_emb_gru', torch.tensor(PRED.transpose(1, 0, 2).copy()), torch.tensor(plen.astype(np.int64)))
    close(got['tok_next'], want.numpy())
    assert (got['XH'][:, 0] == 0).all()
    for dr in range(2):
        for s in range(16):
            dead = (15 - s if dr else s) >= plen
            r, z, nn, hn = got['XG'][dr, s]
            assert (r[dead] == 0).all() and (z[dead] == 1).all() and (nn[dead] == 0).all() and np.isfinite(hn).all()
            assert np.array_equal(got['XH'][dr, s + 1][dead], got['XH'][dr, s][dead])
            close(got['XH'][dr, s + 1], (1 - z) * nn + z * got['XH'][dr, s])
    if kind == 'empty':
        assert (got['tok_next'] == 0).all() and (got['XH'] == 0).all()
    if kind == 'full':
        assert (got['XG'][:, :, 1] < 1).all()


def test_kernel_precision_evaluations_are_off_by_bf16_rounding_and_not_by_zero():
    """one cell from exact inputs: a pre-activation's error is at most 2^-9 sum_k |w_k| |x_k| (every operand within half a bf16 ulp)
    plus fp32 arithmetic; through sigmoid (slope <= 1/4) and tanh (slope <= 1) that bounds the new state.  Over a whole launch the errors
    stay at the bf16 scale and are not zero."""
    W = R.weights('init')
    gc, h0, tok0, emb = R.inputs(17, 0, 'init')
    ref = R.note_loop(W, gc, h0, tok0)
    fp, fd = R.decisions(ref)
    kp = R.kp_note_loop(W, gc, h0, tok0, None, 0, fp, fd)
    u = 2.0 ** -9
    A = u * (np.abs(h0).astype(np.float64) @ np.abs(W['w_hh_n']).T.astype(np.float64) + np.abs(tok0).astype(np.float64) @ np.abs(W['w_ih_tok']).T.astype(np.float64))
    Ar, Az, An = A[:, :R.HN], A[:, R.HN:2 * R.HN], A[:, 2 * R.HN:]
    r, z, nn, hn = ref['gates_n'][0]
    slack = 1e-5
    e_n = An + np.abs(hn) * Ar / 4 + slack                    # n = tanh(x_n + acc_n + r hn): acc_n holds both operands' share of An
    bound = e_n + (Az / 4 + slack) * np.abs(nn - h0) + slack
    err = np.abs(kp['HN'][1] - ref['HN'][1])
    assert (err <= bound).all() and err.max() > 1e-6
    for k in ('pitch', 'dur', 'HN', 'HD', 'gates_n', 'gates_d'):
        e = np.abs(kp[k] - ref[k]).max()
        assert 1e-6 < e < 2.0 ** -6 * max(1.0, np.abs(ref[k]).max()), (k, e)
    assert np.array_equal(kp['PRED'].astype(np.float32), kp['PRED']) and np.abs(kp['PRED'] - ref['PRED']).max() < 1e-6
    PRED, plen = ref['PRED'], R.resum_lengths(17, 'mixed')
    a, b = R.resummarize(W, PRED, plen), R.kp_resummarize(W, PRED, plen)
    for k in ('tok_next', 'XH', 'XG'):
        e = np.abs(a[k] - b[k]).max()
        assert 1e-6 < e < 2.0 ** -6, (k, e)
    dead = a['XG'][:, :, 1] == 1
    assert dead.any() and (b['XG'][:, :, 1][dead] == 1).all() and (b['XG'][:, :, 0][dead] == 0).all()
    for k in R.BF16_KEYS:
        for ws in ('init', 'wide', 'tie'):
            assert R.is_bf16(R.weights(ws)[k]), (ws, k)


def test_case_tables_reach_every_path_mode_shape_and_edge():
    cases = R.NOTE_CASES
    for group in (R.REPLAY_CASES, R.FREE_CASES):
        assert {(c['path'], c['B']) for c in group} == {(p, B) for p in R.PATHS for B in R.BATCHES}
        for p in R.PATHS:
            mine = [c for c in group if c['path'] == p]
            assert {c['mode'] for c in mine} == {0, 1, 2} and {c['t'] for c in mine} == set(R.STEPS), p
            assert {c['ld'] for c in mine} == set(R.LD_PITCH) and {c['h0gc'] for c in mine} == {0, 1}, p
            assert any(c['B'] == 33 and c['t'] == 31 for c in mine)
    for p in R.PATHS:                                         # both FORCE instantiations, HN16 / HD16 given and NULL in train mode
        assert {c['force'] == 'free' for c in cases if c['path'] == p} == {True, False}
        assert {c['s16'] for c in R.REPLAY_CASES if c['path'] == p and c['mode'] == 1} == {0, 1}, p
    assert {c['coin'] for c in R.REPLAY_CASES if c['path'] == 'res' and c['mode'] == 1} >= set(R.COINS)
    assert all(c['mode'] for c in cases if c['coin'])
    assert {c['path'] for c in R.TIE_CASES} == {'res', 'split', 's2'} and all(c['wset'] == 'tie' for c in R.TIE_CASES)
    assert {c['path'] for c in R.SEQ_CASES} >= {'res', 's4'} and R.PARTIAL_CASES
    assert {(B, tr) for B, _, tr, k in R.RESUM_CASES if k == 'mixed'} == {(B, tr) for B in R.BATCHES for tr in range(4)}
    assert {t for _, t, _, _ in R.RESUM_CASES} == set(R.STEPS) and {k for *_, k in R.RESUM_CASES} == {'mixed', 'full', 'empty'}
    assert set(R.resum_lengths(16, 'mixed')) >= {1, 2, 8, 15}
    # the second weight set: <eos> at note step 0, never, and later -- each on some row of the cases that use it
    plens = np.concatenate([R.case_data(c)[2]['plen'] for c in cases if c['wset'] == 'wide'])
    pidx = np.concatenate([R.case_data(c)[2]['pidx'] for c in cases if c['wset'] == 'wide'], axis=1)
    assert (plens == 1).any() and ((plens > 1) & (plens < 15)).any() and (~(pidx == R.EOS).any(0)).any()
    assert (pidx[0] == R.EOS).any() and len(np.unique(pidx)) > 40
    for c in R.TIE_CASES:
        ref = R.case_data(c)[2]
        assert (ref['pidx'] == 7).all() and (ref['margin_p'] == 0).all() and (ref['idx'] == 0).all() and (ref['margin_d'] == 0).all()


@pytest.mark.parametrize('c', [c for c in R.FREE_CASES if c['wset'] == 'wide'], ids=R.case_id)
def test_free_trajectory_inputs_keep_the_reference_far_from_a_tie(c):
    """the kernel-precision evaluation, run free, against the fp64 reference: at most 0.5 % of the case's decisions left out behind a
    first difference; and the stronger property the seeds were chosen for: every margin above twice its plane's bound"""
    W, (gc, h0, tok0, emb), ref, _ = R.case_data(c)
    kp = R.kp_note_loop(W, gc, h0, tok0, emb, c['coin'])
    first, left = R.walk(ref, kp['pidx'], kp['idx'])
    assert left <= 0.005 * 90 * c['B'], (first, left)
    fp, fd = R.decisions(ref)
    bp, bd = R.plane_bounds(ref, R.kp_note_loop(W, gc, h0, tok0, emb, c['coin'], fp, fd), bound_of)
    mp, md = R.margins_over_bounds(ref, bp, bd)
    assert mp > 1.5 and md > 1.5, (mp, md)
    for b, n, k in first:
        assert R.margin_at(ref, b, n, k) <= 2 * (bp[n] if k < 0 else bd[k])
