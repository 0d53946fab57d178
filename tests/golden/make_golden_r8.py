"""Fixture of the dataset path, recorded from the REFERENCE itself (build container only): tests/golden/dataset_path.npz.

Imports `/root/reference` unmodified (`pretty_midi` and `tensorboardX` stubbed as in make_golden_r7.py).  Nothing of the reference is
copied: the file holds the inputs built here and the results its own `ArrangementDataset.__getitem__` (dataset.py:67-120) and
`collect_song.py` gave.

Group `main`: 16 bars, shifts -6..5, every id recorded (all six arrays, smallest integer dtypes).  The bars hold, on purpose:
None as first / second / both bars of a window for the melody and the accompaniment; indicator zeros inside the run and at its end;
a first-bar note sustaining across the barline onto a same-pitch onset in the second bar; two same-pitch notes of one bar where the
later one's sustain overwrites the earlier onset; a note ending past step 32; notes with end <= onset; pitches 2 and 125 (the shifts
wrap at both ends); overlapping melody notes; fractional positions in a float matrix; bars of 600 and 257 accompaniment and 300 melody notes (the kernel stages 256 records per pass); random
chords with root != bass.  main() asserts that every n_state class and every chroma-pair state occurs and that no id raises.
Group `bad`: 10 bars, shift 0, with the failing items (onset step >= 32 as a first and only as a second bar, in either track;
accompaniment pitch 128; 15 onsets in one step) and the exception class the reference raised per id (0 none, 1 IndexError).
`song.*`: get_valid_song_inds on a few index lists, and the ids get_whole_song_data asks a dataset for.

    python tests/golden/make_golden_r8.py        # needs /root/reference; about a minute
"""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from make_golden_r7 import import_reference      # noqa: E402
import dataset_ref as DR                          # noqa: E402


def note(s, e, p, de=4):
    """(sb, sq, sde, eb, eq, ede, pitch, velocity) of a note from step s to step e, de steps per beat"""
    return [s // de, s % de, de, e // de, e % de, de, p, 80]


def random_bar(rng, n, pitches, max_per_step=8):
    rows, per_step = [], {}
    while len(rows) < n:
        s = int(rng.integers(0, 16))
        if per_step.get(s, 0) >= max_per_step:
            continue
        per_step[s] = per_step.get(s, 0) + 1
        rows.append(note(s, s + int(rng.integers(1, 12)), int(rng.choice(pitches))))
    return rows


def random_chords(rng):
    ch = np.zeros((4, 14))
    ch[:, 0] = rng.integers(0, 12, 4)
    ch[:, 1:13] = rng.integers(0, 2, (4, 12))
    ch[:, 13] = rng.integers(0, 12, 4)
    return ch


def main_group(rng):
    mid = list(range(36, 96))
    acc = [random_bar(rng, int(rng.integers(6, 30)), mid) for _ in range(16)]
    mel = [random_bar(rng, int(rng.integers(2, 9)), list(range(55, 90)), 1) for _ in range(16)]
    for i in (2, 5, 6):
        mel[i] = None
    for i in (3, 8, 9):
        acc[i] = None
    acc[1] += [note(0, 6, 2), note(3, 9, 125), note(8, 12, 127), note(9, 10, 0)]
    mel[1] += [note(15, 18, 2), note(1, 3, 125)]
    acc[10] = [note(12, 20, 60), note(2, 5, 61), note(14, 17, 62)]                       # 60 sustains over the barline ...
    acc[11] = [note(2, 6, 60), note(6, 8, 64), note(4, 10, 64), note(0, 1, 62)]          # ... onto an onset; 64: sustain over an onset
    acc[12] += [note(10, 40, 50), note(5, 5, 70), note(7, 3, 71), note(15, 16, 72)]      # past step 32; end <= onset
    mel[4] = [note(0, 8, 72), note(4, 12, 76), note(6, 6, 79), note(10, 30, 74), note(9, 2, 80)]      # overlapping; end <= onset
    mel[12] = [[0, 2.7, 4, 1, 1.2, 4, 66.0, 80.0], [2, 0.5, 4, 3, 3.9, 4, 69.9, 80.0]]  # fractional positions truncate
    acc[13] = random_bar(rng, 600, [30, 41, 52, 63, 64, 65, 77, 88, 99, 110], 64)       # three passes of the chunk loop; <= 10 onsets per step
    mel[13] = random_bar(rng, 300, list(range(50, 100)), 32)                            # two passes on the melody side (fewer than the other track)
    acc[2] = random_bar(rng, 257, [33, 44, 55, 66, 78, 89, 100, 111], 32)               # one record past a full pass
    is_float = {('mel', 12), ('acc', 14)}
    indicator = np.ones(16, dtype=np.int64)
    indicator[[7, 14, 15]] = 0
    data = []
    for i in range(16):
        bar = []
        for name, tr in (('mel', mel), ('acc', acc)):
            t = tr[i]
            bar.append(None if t is None else np.array(t, dtype=np.float64 if (name, i) in is_float else np.int64).reshape(-1, 8))
        bar.append(random_chords(rng))
        data.append(bar)
    return data, indicator


def bad_group(rng):
    acc = [random_bar(rng, 8, list(range(40, 80))) for _ in range(10)]
    mel = [random_bar(rng, 3, list(range(60, 80)), 1) for _ in range(10)]
    acc[2] += [note(33, 35, 60)]                                     # onset >= 32 in either place
    acc[4] += [note(3, 5, 128)]                                      # pitch 128
    acc[6] = [note(3, 5, 40 + 2 * k) for k in range(15)]             # 15 onsets in a step
    acc[7] += [note(17, 19, 61)]                                     # fine as a first bar, step 33 as a second
    mel[9] += [note(20, 22, 70)]                                     # the same in the melody
    mel[3] += [note(40, 41, 71)]
    indicator = np.ones(10, dtype=np.int64)
    indicator[9] = 0
    data = [[np.array(mel[i], dtype=np.int64), np.array(acc[i], dtype=np.int64), random_chords(rng)] for i in range(10)]
    return data, indicator


def pack_data(data, indicator, tag, out):
    out[tag + '.indicator'] = indicator.astype(np.uint8)
    out[tag + '.chord'] = np.stack([b[-1] for b in data]).astype(np.uint8)
    for k, tr in enumerate(('mel', 'acc')):
        rows = [b[k] for b in data]
        out['%s.%s_none' % (tag, tr)] = np.array([r is None for r in rows])
        out['%s.%s_float' % (tag, tr)] = np.array([r is not None and r.dtype == np.float64 for r in rows])
        out['%s.%s_bar' % (tag, tr)] = np.concatenate([np.full(len(r), i, dtype=np.int16) for i, r in enumerate(rows) if r is not None])
        out['%s.%s_nmat' % (tag, tr)] = np.concatenate([r.astype(np.float64) for r in rows if r is not None])


def small(a, dtype=np.uint8):
    b = np.asarray(a).astype(dtype)
    assert np.array_equal(b.astype(np.float64), np.asarray(a, dtype=np.float64))
    return b


def record(ref_dataset, tag, shift_low, shift_high, out, must_pass):
    data = DR.fixture_data(out, tag)                                 # what the tests will rebuild, not what was built above
    ds = ref_dataset.ArrangementDataset(data, out[tag + '.indicator'].astype(np.int64), shift_low, shift_high, num_bar=2, contain_chord=True)
    out[tag + '.shift_range'] = np.array([shift_low, shift_high], dtype=np.int16)
    out[tag + '.valid_inds'] = np.array(ds.valid_inds, dtype=np.int16)
    out[tag + '.len'] = np.int32(len(ds))
    names = ('mel', 'prs', 'pr_mat', 'x', 'c', 'dt_x')
    shapes = ((1, 32, 130), (32, 128, 3), (32, 128), (32, 16, 6), (8, 36), (32, 16, 39))
    dtypes = (np.float64, np.int64, np.float64, np.int64, np.float64, np.int64)
    got = {n: [] for n in names}
    exc = []
    for id in range(len(ds)):
        try:
            item = ds[id]
            for n, a, s, d in zip(names, item, shapes, dtypes):
                assert a.shape == s and a.dtype == d, (n, a.shape, a.dtype)
            exc.append(0)
        except IndexError:
            item = [np.zeros(s) for s in shapes]
            exc.append(1)
        for n, a in zip(names, item):
            got[n].append(small(a))
    for n in names:
        out['%s.%s' % (tag, n)] = np.stack(got[n])
    out[tag + '.exc'] = np.array(exc, dtype=np.uint8)
    if must_pass:
        assert not any(exc), exc
    # the unshifted accompaniment roll of every window, from the reference's own rasteriser
    rolls = []
    for i in ds.valid_inds:
        try:
            rolls.append(small(ref_dataset.ext_nmat_to_pr(ds._combine_segments([data[i][1], data[i + 1][1]]))))
        except IndexError:
            rolls.append(np.zeros((32, 128), dtype=np.uint8))
    out[tag + '.pr_unshifted'] = np.stack(rolls)
    print(tag, 'ids', len(ds), 'exc', exc if not must_pass else 'none')
    return ds


class Asked:
    """a stand-in dataset that notes which ids get_whole_song_data asks for"""

    def __init__(self):
        self.ids = []

    def __getitem__(self, i):
        self.ids.append(i)
        return tuple(np.zeros(1) for _ in range(6))


def main():
    import_reference()
    import dataset as ref_dataset
    import collect_song as ref_song
    rng = np.random.default_rng(808)
    out = OrderedDict()
    pack_data(*main_group(rng), 'main', out)
    pack_data(*bad_group(rng), 'bad', out)
    record(ref_dataset, 'main', -6, 5, out, True)
    record(ref_dataset, 'bad', 0, 0, out, False)
    assert set(out['bad.exc'].tolist()) == {0, 1}
    dt = out['main.dt_x']
    assert dt[..., :34].reshape(-1, 34).any(0)[[0, 1, 2, 3, 4, 6] + list(range(19, 34))].all(), 'a class of dt_x never occurs'
    assert not dt[..., 5].any()                                      # (the first row of a beat is <sos>: is_bass class 1 cannot occur)
    states = np.concatenate([DR.chroma_states(c.astype(np.float64))[2] for c in out['main.c']])
    assert all(set(states[:, d]) == ({0, 2} if d in (0, 4) else {0, 1, 2, 3}) for d in range(7)), 'a chroma-pair state never occurs'
    assert (out['main.pr_mat'] != 0).sum(-1).max() <= 14
    lists = [out['main.valid_inds'].tolist(), list(range(3, 20)) + list(range(22, 30)) + list(range(40, 53)), list(range(13)), [5], []]
    for k, v in enumerate(lists):
        out['song.list%d' % k] = np.array(v, dtype=np.int16)
        for mb in (16, 8):
            inds, lens = ref_song.get_valid_song_inds(v, min_bars=mb)
            out['song.inds%d_%d' % (k, mb)] = np.array(inds, dtype=np.int16)
            out['song.lens%d_%d' % (k, mb)] = np.array(lens, dtype=np.int16)
    for k, (start, length, shift) in enumerate(((3, 14, 0), (3, 15, 1), (0, 6, 2))):
        asked = Asked()
        ref_song.get_whole_song_data(asked, start, length, shift)
        out['song.whole%d_args' % k] = np.array([start, length, shift], dtype=np.int16)
        out['song.whole%d_ids' % k] = np.array(asked.ids, dtype=np.int16)
    path = os.path.join(HERE, 'dataset_path.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main()
