"""Numpy restatement of the dataset path as the package implements it (csrc/dataset.hip, dataset.py): from per-bar note matrices to
the six arrays of an item.  Written from the rules, not from the reference's text; tests/test_dataset_host.py checks it against the
fixture recorded from the reference (tests/golden/make_golden_r8.py), the GPU tests lean on it where inputs are new.

The last stage (unshifted roll + raw chords -> pr_mat, x, c) is oracle/data_oracle.py, which earlier fixtures already pin."""
import numpy as np

from oracle import data_oracle as do

ERR_NOTE = 1               # err bit 0 of ptv_window_rolls
EXC = {0: None, 1: IndexError}


def fixture_data(g, tag):
    """the `data` list of a fixture group: per bar [mel | None, acc | None, chord [4,14]]"""
    n_bar = len(g[tag + '.chord'])
    data = []
    for i in range(n_bar):
        bar = []
        for tr in ('mel', 'acc'):
            if g['%s.%s_none' % (tag, tr)][i]:
                bar.append(None)
                continue
            rows = g['%s.%s_nmat' % (tag, tr)][g['%s.%s_bar' % (tag, tr)] == i]
            bar.append(rows.copy() if g['%s.%s_float' % (tag, tr)][i] else rows.astype(np.int64))
        bar.append(g[tag + '.chord'][i].astype(np.float64))
        data.append(bar)
    return data


def note_steps(track, add):
    """(onset step, end step, pitch) of every row of a bar's note matrix, the bar shifted by `add` beats; Python ints, truncated
    towards zero"""
    if track is None:
        return []
    out = []
    for row in np.asarray(track):
        sb, sq, sde, eb, eq, ede, p = row[:7]
        out.append((int((sb + add) * sde + sq), int((eb + add) * ede + eq), int(p)))
    return out


def window_notes(data, first_bar, track, ts=4):
    return note_steps(data[first_bar][track], 0) + note_steps(data[first_bar + 1][track], ts)


def acc_roll(notes):
    """2 at the onset, 1 from the next step up to (not including) the end, clipped at 32; notes in order, later ones overwrite"""
    pr = np.zeros((32, 128), dtype=np.uint8)
    err = 0
    for s, e, p in notes:
        if s >= 32 or p > 127:
            err |= ERR_NOTE
            continue
        pr[s, p] = 2
        pr[s + 1:max(min(e, 32), 0), p] = 1
    return pr, err


def mel_roll(notes):
    """[32,130]: pitch cell at the onset; column 128 'held' over (s, e); column 129 'rest' everywhere but over [s, e)"""
    pr = np.zeros((32, 130), dtype=np.uint8)
    pr[:, 129] = 1
    err = 0
    for s, e, p in notes:
        if s >= 32 or p > 127:
            err |= ERR_NOTE
            continue
        e = max(min(e, 32), 0)
        pr[s, p] = 1
        pr[s:e, 129] = 0
        pr[s + 1:e, 128] = 1
    return pr, err


def chroma_states(c):
    """c [8,36] -> root [8], bass [8], state [8,7]: the chord's chroma seen from its root; degree 0 (unison) and 4 (fifth) have one
    chroma each (0 present, 2 absent), the others a (low, high) pair: low only 0, high only 1, neither 2, both 3"""
    root = np.argmax(c[:, :12], axis=-1)
    bass = np.argmax(c[:, 24:], axis=-1)
    state = np.zeros((8, 7), dtype=np.int64)
    low = (0, 1, 3, 5, 7, 8, 10)
    for t in range(8):
        ch = [int(c[t, 12 + (k + root[t]) % 12] != 0) for k in range(12)]
        for d, k in enumerate(low):
            if d in (0, 4):
                state[t, d] = 2 * (1 - ch[k])
            else:
                state[t, d] = {(1, 0): 0, (0, 1): 1, (0, 0): 2, (1, 1): 3}[(ch[k], ch[k + 1])]
    return root, bass, state


DEG = (0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 6)
SEMI = (0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1)


def detrend(x, c):
    """x [32,16,6] int, c [8,36] -> [32,16,39] uint8: one-hots is_note 4 | is_bass 3 | octave 12 | degree 8 | n_state 7, then the five
    duration columns.  SEMI is looked up by the scale degree; only the very first row of a beat keeps its own is_bass class."""
    root, bass, state = chroma_states(c)
    out = np.zeros((32, 16, 39), dtype=np.uint8)
    out[:, :, 34:] = x[:, :, 1:]
    for t in range(32):
        beat = t // 4
        for j in range(16):
            p = int(x[t, j, 0])
            if 128 <= p <= 130:
                cls = (p - 127, 2, 11, 7, 6)
            elif 0 <= p < 144:
                degree = (p - root[beat]) % 12
                d = DEG[degree]
                cs, semi = state[beat, d], SEMI[d]
                n_state = (0 if semi else 1) if cs == 0 else (1 if semi else 0) if cs == 1 else semi + 2 if cs == 2 else semi + 4
                cls = (0, int(bass[beat] == degree), p // 12, d, n_state)
            else:
                continue
            is_bass = cls[1] if (t % 4 == 0 and j == 0) else 0
            out[t, j, cls[0]] = 1
            out[t, j, 4 + is_bass] = 1
            out[t, j, 7 + cls[2]] = 1
            out[t, j, 19 + cls[3]] = 1
            out[t, j, 27 + cls[4]] = 1
    return out


def item(data, first_bar, shift):
    """the six arrays of the window (first_bar, first_bar + 1) at `shift`, uint8 / as the kernels write them, and the exception class
    the reference raises for it (None, IndexError): -> dict"""
    acc, err_a = acc_roll(window_notes(data, first_bar, 1))
    mel, err_m = mel_roll(window_notes(data, first_bar, 0))
    chord14 = np.concatenate([np.asarray(data[first_bar + k][-1], dtype=np.float32).reshape(4, 14) for k in (0, 1)])
    out = {'pr': acc, 'err': err_a | err_m, 'chord14': chord14}
    rolled = np.roll(acc, shift, axis=-1)
    out['prs'] = np.stack([rolled == 2, rolled == 1, rolled == 0], axis=-1).astype(np.uint8)
    out['mel'] = np.concatenate([np.roll(mel[:, :128], shift, axis=-1), mel[:, 128:]], axis=-1)[None].astype(np.float32)
    over = False
    try:
        pr_mat, x, c = do.batch_transform(acc[None], chord14[None], np.array([shift], dtype=np.int32))
        out['pr_mat'], out['x'], out['c'] = pr_mat[0], x[0], c[0]
        out['dt_x'] = detrend(x[0], c[0])
    except IndexError:
        over = True
    out['exc'] = IndexError if (out['err'] or over) else None
    return out


def id_to_window(valid_inds, shift_low, shift_high, id):
    n_shift = shift_high - shift_low + 1
    return valid_inds[id // n_shift], id % n_shift + shift_low
