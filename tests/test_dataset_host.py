"""Host side of the dataset path (ptv_window_rolls, ptv_detrend_pianotree, dataset.py): the symbols and names exist, the index rules
and the bank builder behave, and the numpy restatement the GPU tests lean on agrees with the fixture recorded from the reference
(tests/golden/make_golden_r8.py) on every id."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dataset_ref as R
from helpers import load_npz
from polyphonic_chord_texture_disentanglement_amd import _lib

NEW_SYMBOLS = ('ptv_window_rolls', 'ptv_detrend_pianotree')
NAMES = ('mel', 'prs', 'pr_mat', 'x', 'c', 'dt_x')


@pytest.fixture(scope='module')
def g():
    return load_npz('dataset_path.npz')


def dataset_module():
    from polyphonic_chord_texture_disentanglement_amd import dataset
    return dataset


def host_dataset(g, tag, **kw):
    """the class without a device: only its host side is used here"""
    D = dataset_module()
    lo, hi = (int(v) for v in g[tag + '.shift_range'])
    return D.ArrangementDataset(R.fixture_data(g, tag), g[tag + '.indicator'].astype(np.int64), lo, hi, num_bar=2, contain_chord=True, **kw)


def test_new_entry_points_are_declared_exported_and_bound():
    declared = _lib.exported_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name + ' is not declared in include/ptvae_hip.h'
    assert os.path.exists(_lib.LIB_PATH), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    l = _lib.lib()
    assert l.ptv_abi_version() == 7
    for name in NEW_SYMBOLS:
        fn = getattr(l, name)
        assert fn.restype is ctypes.c_int and fn.argtypes[-1] is ctypes.c_void_p
    # argument checks run before anything touches a device
    assert l.ptv_window_rolls(None, None, None, None, None, 16, None, None, 1, None, None, None, None, None, None) != 0
    assert l.ptv_detrend_pianotree(None, None, None, 1, None) != 0


def test_names_exist():
    D = dataset_module()
    for n in ('ArrangementDataset', 'SongDataset', 'detrend_pianotree', 'get_valid_song_inds', 'pack_bank'):
        assert callable(getattr(D, n, None)), n
    for n in ('batch', '__getitem__', '__len__', 'subset'):
        assert callable(getattr(D.ArrangementDataset, n, None)), n
    assert callable(getattr(D.SongDataset, 'get_song_batch', None))


def test_only_two_bar_windows_in_four_four():
    D = dataset_module()
    data = [[None, None, np.zeros((4, 14))]] * 4
    with pytest.raises(NotImplementedError):
        D.ArrangementDataset(data, np.array([1, 1, 1, 0]), -6, 5)                  # the reference's default num_bar = 8
    with pytest.raises(NotImplementedError):
        D.ArrangementDataset(data, np.array([1, 1, 1, 0]), -6, 5, num_bar=2, ts=3)
    with pytest.raises(ValueError):
        D.ArrangementDataset(data, np.array([1, 1, 1, 1]), -6, 5, num_bar=2)       # a window cannot start on the last bar


def test_cpu_device_is_refused():
    D = dataset_module()
    data = [[None, None, np.zeros((4, 14))]] * 4
    with pytest.raises(RuntimeError, match='no CPU'):
        D.ArrangementDataset(data, np.array([1, 1, 1, 0]), 0, 0, num_bar=2, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU'):
        D.detrend_pianotree(torch.zeros(1, 32, 16, 6, dtype=torch.int64), torch.zeros(1, 8, 36))
    if not torch.cuda.is_available():
        ds = D.ArrangementDataset(data, np.array([1, 1, 1, 0]), 0, 0, num_bar=2)
        with pytest.raises(RuntimeError, match='no CPU'):
            ds.batch([0])
        with pytest.raises(RuntimeError, match='no CPU'):
            ds[0]


@pytest.mark.parametrize('tag', ['main', 'bad'])
def test_index_rules_equal_the_reference(g, tag):
    ds = host_dataset(g, tag)
    assert ds.valid_inds == g[tag + '.valid_inds'].tolist()
    assert ds.num_sample == len(ds.valid_inds)
    assert len(ds) == int(g[tag + '.len']) == len(g[tag + '.exc'])
    lo, hi = (int(v) for v in g[tag + '.shift_range'])
    n = hi - lo + 1
    for id in (0, 1, n - 1, n, len(ds) - 1):
        assert ds.id_to_no_shift(id) == (id // n, id % n + lo)
        assert R.id_to_window(ds.valid_inds, lo, hi, id) == (ds.valid_inds[id // n], id % n + lo)


def test_bank_layout_and_checks(g):
    D = dataset_module()
    data = R.fixture_data(g, 'main')
    bank = D.pack_bank(data)
    n_bar = len(data)
    for tr, k in (('mel', 0), ('acc', 1)):
        off = bank[tr + '_off']
        assert off.dtype == np.int32 and off.shape == (n_bar + 1,) and off[0] == 0
        assert np.diff(off).tolist() == [0 if b[k] is None else len(b[k]) for b in data]
        assert bank[tr + '_rec'].dtype == np.uint32 and len(bank[tr + '_rec']) >= off[-1]
    assert bank['chord_bars'].shape == (n_bar, 4, 14) and bank['chord_bars'].dtype == np.float32
    # one record: pitch | both places' onset and (clipped) end
    rec = int(D.pack_bank([[None, np.array([[2, 2, 4, 9, 1, 4, 61, 90]]), np.zeros((4, 14))]])['acc_rec'][0])
    assert (rec & 255, (rec >> 8) & 63, (rec >> 14) & 63, (rec >> 20) & 63, (rec >> 26) & 63) == (61, 10, 32, 26, 32)
    # far fewer bytes than a rasterised window per bar
    assert sum(v.nbytes for v in bank.values()) < 4096 * n_bar / 2
    chord = np.zeros((4, 14))
    for bad in ([[-1, 0, 4, 1, 0, 4, 60, 80]], [[0, 0, 4, 1, 0, 4, -3, 80]], [[0, 0, 4, -1, 0, 4, 60, 80]], [[0, -1, 4, 1, 0, 4, 60, 80]]):
        for k in (0, 1):
            bar = [None, None, chord]
            bar[k] = np.array(bad)
            with pytest.raises(ValueError, match='negative'):
                D.pack_bank([bar, [None, None, chord]])
    half = chord.copy()
    half[1, 5] = 0.5
    with pytest.raises(ValueError, match='chroma'):
        D.pack_bank([[None, None, half]])


@pytest.mark.parametrize('tag', ['main', 'bad'])
def test_numpy_restatement_agrees_with_the_reference_fixture(g, tag):
    data = R.fixture_data(g, tag)
    lo, hi = (int(v) for v in g[tag + '.shift_range'])
    valid = g[tag + '.valid_inds'].tolist()
    exc = g[tag + '.exc']
    for id in range(len(exc)):
        bar, shift = R.id_to_window(valid, lo, hi, id)
        it = R.item(data, bar, shift)
        assert it['exc'] is R.EXC[int(exc[id])], (tag, id)
        if exc[id]:
            continue
        assert it['err'] == 0
        for n in NAMES:
            assert np.array_equal(it[n].astype(np.int64), g['%s.%s' % (tag, n)][id].astype(np.int64)), (tag, id, n)
        assert np.array_equal(it['pr'], g[tag + '.pr_unshifted'][id // (hi - lo + 1)]), (tag, id)
    assert (exc == 0).sum() >= (150 if tag == 'main' else 2) and (tag == 'main' or (exc == 1).sum() >= 5)


def test_song_index_rules_equal_the_record(g):
    D = dataset_module()
    k = 0
    while 'song.list%d' % k in g:
        for mb in (16, 8):
            inds, lens = D.get_valid_song_inds(g['song.list%d' % k].tolist(), min_bars=mb)
            assert inds == g['song.inds%d_%d' % (k, mb)].tolist() and lens == g['song.lens%d_%d' % (k, mb)].tolist(), (k, mb)
        k += 1
    assert k >= 4 and len(g['song.inds1_8']) >= 2
    for k in range(3):
        start, length, shift = (int(v) for v in g['song.whole%d_args' % k])
        assert D.song_ids(start, length, shift) == g['song.whole%d_ids' % k].tolist()
