"""Host side of the output path (ptv_grid_to_pr, ptv_chord_tokens and the methods over them): the symbols and methods exist, CPU tensors
are refused, and the numpy restatement the GPU tests lean on agrees with the fixture recorded from the reference
(tests/golden/make_golden_r7.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import output_path_ref as R
from helpers import load_npz
from polyphonic_chord_texture_disentanglement_amd import _lib
from polyphonic_chord_texture_disentanglement_amd import model as M
from polyphonic_chord_texture_disentanglement_amd import ptvae as P
from test_host_surface import build_reduced

NEW_SYMBOLS = ('ptv_grid_to_pr', 'ptv_chord_tokens')


def test_new_entry_points_are_declared_exported_and_bound():
    declared = _lib.exported_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name + ' is not declared in include/ptvae_hip.h'
    assert _lib.EXPECTED_ABI == 7
    assert os.path.exists(_lib.LIB_PATH), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    l = _lib.lib()
    assert l.ptv_abi_version() == 7
    for name in NEW_SYMBOLS:
        fn = getattr(l, name)
        assert fn.restype is ctypes.c_int and fn.argtypes[-1] is ctypes.c_void_p
    # argument checks run before anything touches a device
    assert l.ptv_grid_to_pr(None, 1, 16, 10, 0, 129, None, None, None, None, None, None) != 0
    assert l.ptv_chord_tokens(None, None, None, None, None, 8, 1, None) != 0


def test_new_methods_exist_on_the_classes():
    for cls, names in ((P.PtvaeDecoder, ('grid_to_pr_and_notes_batch', 'notes_to_tuples')), (P.RnnDecoder, ('decode_tokens',)),
                       (M.DisentangleVAE, ('decode_to_inputs', 'reencode'))):
        for n in names:
            assert callable(getattr(cls, n, None)), '%s.%s' % (cls.__name__, n)
    assert callable(getattr(P, 'chord_tokens', None))


def test_cpu_tensors_are_refused():
    m = build_reduced()
    z = torch.zeros(2, 16)
    with pytest.raises(RuntimeError, match='no CPU'):
        m.decoder.grid_to_pr_and_notes_batch(torch.zeros(2, 32, 16, 6, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU'):
        m.chd_decoder.decode_tokens(z)
    with pytest.raises(RuntimeError, match='no CPU'):
        m.decode_to_inputs(z, z)
    with pytest.raises(RuntimeError, match='no CPU'):
        m.reencode(z, z)
    with pytest.raises(RuntimeError, match='no CPU'):
        P.chord_tokens(torch.zeros(8, 2, 12), torch.zeros(8, 2, 24), torch.zeros(8, 2, 12))


def test_notes_to_tuples_equals_the_host_methods_tuples():
    g = load_npz('output_path.npz')
    grids, _ = R.fixture_groups(g)['dec']
    dec = build_reduced().decoder
    for bpm, start in ((60., 0.), (97., 0.3)):
        want = [dec.grid_to_pr_and_notes(x, bpm=bpm, start=start)[1] for x in grids]
        rows = [R.grid_to_pr(x)[1] for x in grids]
        notes = torch.zeros(len(rows), 320, 3, dtype=torch.int32)
        for b, r in enumerate(rows):
            notes[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
        count = torch.tensor([len(r) for r in rows], dtype=torch.int32)
        assert P.PtvaeDecoder.notes_to_tuples(notes, count, bpm=bpm, start=start) == want


def test_numpy_restatement_agrees_with_the_reference_fixture():
    g = load_npz('output_path.npz')
    seen = {0: 0, 1: 0, 2: 0}
    for tag, (grids, min_pitch) in R.fixture_groups(g).items():
        bpm, start = g[tag + '.bpm_start']
        for b, grid in enumerate(grids):
            pr_ref, notes_ref, times_ref, exc = R.fixture_sample(g, tag, b)
            pr, notes, x_clean, err = R.grid_to_pr(grid, min_pitch=min_pitch)
            seen[exc] += 1
            if exc == 0:
                assert err == 0, (tag, b, err)
                assert np.array_equal(pr, pr_ref), (tag, b)
                assert np.array_equal(np.array(notes, dtype=np.int64).reshape(-1, 3), notes_ref), (tag, b)
                tup = R.note_tuples(notes, bpm, start)
                assert [(s, e) for _, s, e in tup] == [tuple(r) for r in times_ref.tolist()], (tag, b)
                pr2, notes2, x2, err2 = R.grid_to_pr(x_clean)                      # the canonical grid reads back as what was read
                assert err2 == 0 and np.array_equal(pr2, pr) and notes2 == notes and np.array_equal(x2, x_clean), (tag, b)
            else:
                assert err & 3, (tag, b)
                assert bool(err & R.ERR_FIRST_IS_DUR) == (exc == 2), (tag, b, err)
    assert seen[0] >= 40 and seen[1] >= 6 and seen[2] >= 6, seen
    assert 2 * int((g['dec.exc'] == 0).sum()) >= len(g['dec.exc'])          # the decoded grids really compare something


def test_x_clean_of_a_ground_truth_grid_is_that_grid():
    x = load_npz('data_contract.npz')['x']
    for grid in x[:8]:
        pr, notes, x_clean, err = R.grid_to_pr(grid, max_notes=14)
        assert err == 0 and np.array_equal(x_clean, grid)


def test_chord_restatement_agrees_with_the_tokens_the_reference_fed_back():
    g = load_npz('output_path.npz')
    c, chord14 = R.chord_tokens(g['chd.root'], g['chd.chroma'], g['chd.bass'])
    assert c.shape == (6, 8, 36) and chord14.shape == (6, 8, 14)
    assert np.array_equal(c[:, :7], g['chd.tokens'].astype(np.float32))
    # the bank layout expands back to the token (the forward contract's expand_chord at shift 0)
    from oracle import data_oracle as do
    _, _, c_back = do.batch_transform(np.zeros((6, 32, 128), dtype=np.uint8), chord14, np.zeros(6, dtype=np.int32))
    assert np.array_equal(c_back, c)
    # ties go to the lowest index
    z = np.zeros((1, 12), dtype=np.float32)
    c0, k0 = R.chord_tokens(z, np.zeros((1, 12, 2), dtype=np.float32), z)
    assert c0[0, 0] == 1 and c0[0, 24] == 1 and c0.sum() == 2 and k0.sum() == 0
