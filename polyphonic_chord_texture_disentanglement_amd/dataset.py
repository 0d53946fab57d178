"""The reference's dataset (`dataset.py`, `collect_song.py`) served from a note bank in HBM.

`ArrangementDataset` takes what the reference's class takes -- `data`, per bar `[mel_nmat | None, acc_nmat | None, ..., chord [4,14]]`,
and `indicator`, one flag per bar: a two-bar window starts here -- packs the notes ONCE on the host into 4-byte records
(`include/ptvae_hip.h`, `ptv_window_rolls`) and keeps them on the device.  `batch(ids)` then serves the reference's complete 6-tuple
`(mel_segments, prs, pr_mat, x, c, dt_x)` with no host work: `ptv_window_rolls` rasterises the windows, the existing
`ptv_batch_transform` turns the unshifted rolls into `(pr_mat, x, c)` and `ptv_detrend_pianotree` gives `dt_x`.

Reading POP909 files (`collect_data_fns`, `init_music`, `score.py`) stays outside: the boundary is this constructor."""
import numpy as np
import torch
from torch.utils.data import Dataset

from ._lib import call, ptr, stream_ptr
from .ptvae import _require_cuda

SLOTS = ('mel', 'prs', 'dt_x')


def _trunc(v):
    """int() of every element: towards zero"""
    return np.trunc(np.asarray(v, dtype=np.float64)).astype(np.int64)


def _bar_records(track, ts, what):
    """One bar's note matrix [n, >= 7] = (sb, sq, sde, eb, eq, ede, pitch, ...) -> uint32 records.  The steps are evaluated as the
    reference evaluates them (converter.py:41-43, in the matrix's own dtype, then int()), for the bar as it stands and translated by
    ts beats (dataset.py:43-47), so the device sees integers only."""
    if track is None:
        return np.zeros(0, dtype=np.uint32)
    nm = np.asarray(track)
    if nm.ndim != 2 or nm.shape[1] < 7:
        raise ValueError('%s: a note matrix is [n, 8] (sb, sq, sde, eb, eq, ede, pitch, velocity), got shape %s' % (what, nm.shape))
    cols = []
    for add in (0, ts):
        cols.append(_trunc((nm[:, 0] + add) * nm[:, 2] + nm[:, 1]))
        cols.append(_trunc((nm[:, 3] + add) * nm[:, 5] + nm[:, 4]))
    pitch = _trunc(nm[:, 6])
    if (pitch < 0).any() or any((c < 0).any() for c in cols):
        raise ValueError('%s: negative step or pitch (numpy would wrap it around in the reference; a bank does not take it)' % what)
    s0, e0, s1, e1 = cols
    rec = (np.minimum(pitch, 255) | (np.minimum(s0, 63) << 8) | (np.minimum(e0, 32) << 14) | (np.minimum(s1, 63) << 20)
           | (np.minimum(e1, 32) << 26))
    return rec.astype(np.uint32)


def pack_bank(data, ts=4):
    """data (one entry per bar) -> the host arrays of the bank: acc_rec / mel_rec uint32, acc_off / mel_off int32 [n_bar+1],
    chord_bars f32 [n_bar,4,14]"""
    out = {}
    for name, k in (('mel', 0), ('acc', 1)):
        recs = [_bar_records(bar[k], ts, 'bar %d (%s)' % (i, name)) for i, bar in enumerate(data)]
        off = np.zeros(len(recs) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in recs], out=off[1:])
        if off[-1] >= 2 ** 31:
            raise ValueError('more than 2^31 notes in one bank')
        # (never empty: the kernel takes no NULL table)
        out[name + '_rec'] = np.concatenate(recs + [np.zeros(1, dtype=np.uint32)])
        out[name + '_off'] = off.astype(np.int32)
    chord = np.stack([np.asarray(bar[-1], dtype=np.float32).reshape(4, 14) for bar in data]) if len(data) else np.zeros((0, 4, 14), np.float32)
    bits = chord[:, :, 1:13]
    if not np.logical_or(bits == 0, bits == 1).all():
        raise ValueError('chroma bits must be exactly 0 or 1')
    out['chord_bars'] = np.ascontiguousarray(chord)
    return out


def detrend_pianotree(x, c):
    """dataset.py:123-213 for a device batch: x int64 [B,32,16,6], c f32 [B,8,36] -> dt_x uint8 [B,32,16,39]"""
    _require_cuda(x, 'detrend_pianotree')
    _require_cuda(c, 'detrend_pianotree')
    assert x.dtype == torch.int64 and x.shape[1:] == (32, 16, 6) and c.shape[1:] == (8, 36) and c.shape[0] == x.shape[0]
    x, c = x.contiguous(), c.float().contiguous()
    dt_x = torch.empty(x.shape[0], 32, 16, 39, device=x.device, dtype=torch.uint8)
    call('ptv_detrend_pianotree', ptr(x), ptr(c), ptr(dt_x), x.shape[0], stream_ptr())
    return dt_x


class ArrangementDataset(Dataset):
    """The reference's class (dataset.py:18-120) over a device note bank; same positional signature.

    Departures: only two-bar windows in 4/4 exist (`num_bar=2, ts=4`, what every reference script passes and the only kind the model
    takes; anything else raises NotImplementedError), a negative step or pitch raises ValueError here (the reference would let numpy
    wrap it around), chroma bits must be exactly 0 or 1, an indicator set on the last bar raises ValueError here rather than on
    access, and a melody pitch above 127 is an IndexError like an accompaniment one."""

    def __init__(self, data, indicator, shift_low, shift_high, num_bar=8, ts=4, contain_chord=False, device=None, _bank=None):
        if num_bar != 2 or ts != 4:
            raise NotImplementedError('only two-bar windows in 4/4 reach the model: num_bar=2, ts=4 (got num_bar=%r, ts=%r)' % (num_bar, ts))
        if device is not None and torch.device(device).type != 'cuda':
            _require_cuda(torch.empty(0, device=device), 'ArrangementDataset')
        if device is None and torch.cuda.is_available():
            device = torch.device('cuda', torch.cuda.current_device())
        # (without a GPU the host side -- valid_inds, len(), the id rule, the bank's checks -- still works; batch() then refuses)
        self.device = torch.device(device) if device is not None else None
        self.data, self.indicator = data, np.asarray(indicator)
        self.shift_low, self.shift_high = shift_low, shift_high
        self.num_sample = int(self.indicator.sum())
        self.valid_inds = [i for i, ind in enumerate(self.indicator) if ind]
        self.num_bar, self.ts, self.contain_chord = num_bar, ts, contain_chord
        self.n_bar = len(data)
        if self.n_bar < 2 or (self.valid_inds and self.valid_inds[-1] + 1 >= self.n_bar):
            raise ValueError('a window is two bars: the indicator cannot be set on the last bar (%d bars)' % self.n_bar)
        if _bank is None:
            host = pack_bank(data, ts)
            _bank = host if self.device is None else {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(self.device)
                                                      for k, v in host.items()}
        self.bank = _bank
        self._valid = torch.tensor(self.valid_inds, dtype=torch.int64, device=self.device)

    def subset(self, valid_inds, shift_low, shift_high):
        """the same device bank with other windows and shifts (a train / validation split costs no second upload)"""
        ind = np.zeros(len(self.indicator), dtype=np.int64)
        ind[list(valid_inds)] = 1
        return ArrangementDataset(self.data, ind, shift_low, shift_high, self.num_bar, self.ts, self.contain_chord, self.device, _bank=self.bank)

    @property
    def n_shift(self):
        return self.shift_high - self.shift_low + 1

    @property
    def bank_bytes(self):
        return sum(int(v.nbytes) for v in self.bank.values())

    def __len__(self):
        return self.num_sample * self.n_shift

    def id_to_no_shift(self, id):
        """dataset.py:68-70"""
        return id // self.n_shift, id % self.n_shift + self.shift_low

    def window_rolls(self, first_bar, shift=None, want=('pr', 'prs', 'mel', 'chord14')):
        """ptv_window_rolls on this bank: first_bar int32 [B], shift int32 [B] | None -> {name: tensor}, plus 'err' int32 [B]"""
        B, dev = first_bar.numel(), self.device
        shapes = {'pr': ((B, 32, 128), torch.uint8), 'prs': ((B, 32, 128, 3), torch.uint8), 'mel': ((B, 1, 32, 130), torch.float32),
                  'chord14': ((B, 8, 14), torch.float32)}
        out = {k: torch.empty(*shapes[k][0], device=dev, dtype=shapes[k][1]) for k in want}
        out['err'] = torch.empty(B, device=dev, dtype=torch.int32)
        k = self.bank
        call('ptv_window_rolls', ptr(k['acc_rec']), ptr(k['acc_off']), ptr(k['mel_rec']), ptr(k['mel_off']), ptr(k['chord_bars']), self.n_bar,
             ptr(first_bar), ptr(shift), B, ptr(out.get('pr')), ptr(out.get('prs')), ptr(out.get('mel')), ptr(out.get('chord14')),
             ptr(out['err']), stream_ptr())
        return out

    def batch(self, ids, slots=SLOTS, check=False):
        """ids [B] (device tensor, or anything torch.as_tensor takes) -> the device tuple (mel_segments f32 [B,1,32,130], prs u8
        [B,32,128,3], pr_mat f32 [B,32,128], x i64 [B,32,16,6], c f32 [B,8,36], dt_x u8 [B,32,16,39]); a slot not named in `slots` is
        the empty tensor.  check=False reads nothing back (with a device `ids` the call captures into a graph; an id outside
        0..len-1 gives an empty sample, flagged in the kernel's err); check=True synchronises and raises IndexError for the first
        sample the reference would raise on."""
        unknown = set(slots) - set(SLOTS)
        if unknown:
            raise ValueError('unknown slots %s (of %s)' % (sorted(unknown), SLOTS))
        if self.device is None:
            _require_cuda(torch.empty(0), 'ArrangementDataset.batch')
        dev = self.device
        ids = torch.as_tensor(ids, device=dev).long().reshape(-1)
        if ids.numel() == 0:
            raise ValueError('an empty batch')
        if self.num_sample == 0:
            raise IndexError('the dataset has no window')
        no = torch.div(ids, self.n_shift, rounding_mode='floor')
        shift = (ids - no * self.n_shift + self.shift_low).int()
        # an id outside 0..len-1 becomes window -1, which the kernel flags (err bit 1) and serves as an empty sample: no gather out of range
        inside = (ids >= 0) & (ids < len(self))
        first_bar = torch.where(inside, self._valid[no.clamp(0, self.num_sample - 1)], -1).int()
        r = self.window_rolls(first_bar, shift, ('pr', 'chord14') + tuple(s for s in ('prs', 'mel') if s in slots))
        B = ids.numel()
        pr_mat = torch.empty(B, 32, 128, device=dev, dtype=torch.float32)
        x = torch.empty(B, 32, 16, 6, device=dev, dtype=torch.int64)
        c = torch.empty(B, 8, 36, device=dev, dtype=torch.float32)
        over = torch.zeros(1, device=dev, dtype=torch.int32)
        # (the same launch dataset_loaders.batch_transform makes, on the batch's own scratch rolls: index = NULL)
        call('ptv_batch_transform', ptr(r['pr']), ptr(r['chord14']), None, ptr(shift), ptr(pr_mat), ptr(x), ptr(c), ptr(over), B, stream_ptr())
        empty = torch.empty(0, device=dev)
        dt_x = detrend_pianotree(x, c) if 'dt_x' in slots else empty
        if check:
            bad = r['err'] != 0
            if int(over.item()):
                bad = bad | ((pr_mat != 0).sum(-1) > 14).any(1)
            if bool(bad.any()):
                b = int(torch.nonzero(bad)[0])
                e = int(r['err'][b])
                why = ('the id is outside 0..%d' % (len(self) - 1) if e & 2 else
                       'a note with an onset step >= 32 or a pitch > 127' if e else 'more than 14 onsets in a step')
                raise IndexError('sample %d of the batch (id %d): %s (the reference raises IndexError here)' % (b, int(ids[b]), why))
        return r.get('mel', empty), r.get('prs', empty), pr_mat, x, c, dt_x

    def __getitem__(self, id):
        """The host form: the reference's arrays for one id, in its dtypes and shapes."""
        id = int(id)
        if not 0 <= id < len(self):
            raise IndexError('id %d out of range 0..%d' % (id, len(self) - 1))
        mel, prs, pr_mat, x, c, dt_x = self.batch([id], SLOTS if self.contain_chord else ('mel', 'prs'), check=True)
        out = (mel[0].cpu().numpy().astype(np.float64), prs[0].cpu().numpy().astype(np.int64), pr_mat[0].cpu().numpy().astype(np.float64),
               x[0].cpu().numpy())
        if self.contain_chord:
            out += (c[0].cpu().numpy().astype(np.float64), dt_x[0].cpu().numpy().astype(np.int64))
        return out


def get_valid_song_inds(valid_inds, min_bars=16):
    """collect_song.py:7-31: the runs of consecutive bar numbers in valid_inds that are long enough (length + 3 >= min_bars), as
    (position in valid_inds of each run's first window, run lengths)"""
    inds, lengths = [], []
    start = 0
    n = len(valid_inds)
    while start < n:
        stop = start + 1
        while stop < n and valid_inds[stop] - valid_inds[start] == stop - start:
            stop += 1
        if stop - start + 3 >= min_bars:
            inds.append(start)
            lengths.append(stop - start)
        start = stop
    return inds, lengths


def song_ids(start_ind, length, shift=0):
    """collect_song.py:41-43: every other id from start_ind + shift up to start_ind + length"""
    return list(range(start_ind + shift, start_ind + length, 2))


class SongDataset:
    """collect_song.py:60-75 over a device dataset: whole songs as one batch of every other window.  As in the reference the ids of
    a song are taken as dataset ids, so this is meant for a dataset without augmentation (shift_low = shift_high = 0, the validation
    set).  All six entries are whole-batch tensors (the reference returns only the last window's `prs` in the second slot)."""

    def __init__(self, dataset):
        self.dataset = dataset
        self.song_ind, self.song_len = get_valid_song_inds(dataset.valid_inds, min_bars=16)

    def get_song_batch(self, song_id, length=None, shift=0):
        if length is None:
            length = self.song_len[song_id]
        assert length + shift <= self.song_len[song_id]
        return self.dataset.batch(song_ids(self.song_ind[song_id], length + shift, shift))
