"""Serving batches of B = 512 from the note bank (dataset.ArrangementDataset.batch: ptv_window_rolls + ptv_batch_transform
[+ ptv_detrend_pianotree]) with and without the three extra slots, against the rasterised (pr, chord14) bank of DeviceBatcher on the
same windows (dataset_loaders.batch_transform) and against the numpy restatement on the host (tests/dataset_ref.py, per item, as the
reference's loader works).  Device side by events over --reps calls after a warm-up, host loop by perf_counter over --host-items.
With --train also one timed epoch of TrainingVAE.train() on each bank (bf16, teacher-forced, as bench.py's trainer-surface figure).
Prints one JSON line.

    python scripts/bench_dataset_path.py [--batch 512] [--reps 50] [--bars 4096] [--train]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from polyphonic_chord_texture_disentanglement_amd import dataset as D                                     # noqa: E402
from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import DeviceBatcher, batch_transform   # noqa: E402


def synth_song_bank(n_bar, seed):
    """POP909-like bars: about 24 accompaniment notes (at most 8 onsets a step) and 6 melody notes, a chord per beat"""
    rng = np.random.default_rng(seed)
    data = []
    for _ in range(n_bar):
        tracks = []
        for n, lo, hi in ((int(rng.integers(3, 10)), 55, 90), (int(rng.integers(12, 37)), 36, 96)):
            s = rng.integers(0, 16, n)
            if n > 10:
                s = np.concatenate([np.repeat(np.arange(0, 16, 4), 3), s[12:]])[:n]
            e = s + rng.integers(1, 12, n)
            tracks.append(np.stack([s // 4, s % 4, np.full(n, 4), e // 4, e % 4, np.full(n, 4), rng.integers(lo, hi, n), np.full(n, 80)], 1))
        ch = np.zeros((4, 14))
        ch[:, 0], ch[:, 1:13], ch[:, 13] = rng.integers(0, 12, 4), rng.integers(0, 2, (4, 12)), rng.integers(0, 12, 4)
        data.append(tracks + [ch])
    indicator = np.ones(n_bar, dtype=np.int64)
    indicator[-1] = 0
    return data, indicator


def events_ms(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def train_epoch(dev, loader, B):
    from polyphonic_chord_texture_disentanglement_amd.amc_dl import torch_plus as tp
    from polyphonic_chord_texture_disentanglement_amd.amc_dl.torch_plus.train_utils import kl_anealing
    from polyphonic_chord_texture_disentanglement_amd.dataset_loaders import TrainingVAE
    from polyphonic_chord_texture_disentanglement_amd.model import DisentangleVAE, LOSS_NAMES
    from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam
    torch.manual_seed(0)
    m = DisentangleVAE.init_model(dev).to(dev).set_precision('bf16')
    m.use_philox(7, 0)
    opt = FusedClipAdam(m.parameters(), lr=1e-3)

    class _L:
        train_loader, val_loader = loader, []
    pm = tp.LogPathManager(None, log_path_name=os.path.join(os.environ.get('TMPDIR', '/tmp'), 'ptvae_bench_dataset'))
    osch = tp.OptimizerScheduler(opt, tp.MinExponentialLR(opt, gamma=0.9999, minimum=1e-5), 1)
    ps = tp.ParameterScheduler(tfr1=tp.ConstantScheduler(1.), tfr2=tp.ConstantScheduler(1.), tfr3=tp.ConstantScheduler(1.),
                               beta=tp.TeacherForcingScheduler(0.1, 0., f=kl_anealing), weights=tp.ConstantScheduler([1, 0.5]))
    sw = tp.SummaryWriters(LOSS_NAMES, {'loss': None}, pm.writer_path)
    tr = TrainingVAE(dev, m, False, pm, _L, sw, osch, ps, 1)
    tr.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train()
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / len(loader)
    del m, opt, tr
    torch.cuda.empty_cache()
    return round(B / t, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--bars', type=int, default=4096)
    ap.add_argument('--host-items', type=int, default=64)
    ap.add_argument('--train', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    B = a.batch
    data, indicator = synth_song_bank(a.bars, 17)
    t0 = time.perf_counter()
    ds = D.ArrangementDataset(data, indicator, -6, 5, num_bar=2, contain_chord=True, device=dev)
    pack_s = time.perf_counter() - t0
    n_win = ds.num_sample
    # the parent's capability on the same windows: every window rasterised once (here by the new kernel), 4 KB + 448 B each
    r = ds.window_rolls(ds._valid.int(), None, ('pr', 'chord14'))
    pr_bank, ch_bank = r['pr'], r['chord14']
    assert int(r['err'].abs().sum()) == 0
    ids = torch.randperm(len(ds), device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:B]
    index, shift = (ids // 12).int(), (ids % 12 - 6).int()
    first_bar = ds._valid[index.long()].int()
    full = ds.batch(ids, check=True)
    want = batch_transform(pr_bank, ch_bank, shift, index)
    assert all(torch.equal(u, v) for u, v in zip(full[2:5], want))
    ms = {'note_bank_3_slots': events_ms(lambda: ds.batch(ids, slots=()), a.reps),
          'note_bank_6_slots': events_ms(lambda: ds.batch(ids), a.reps),
          'roll_bank_3_slots': events_ms(lambda: batch_transform(pr_bank, ch_bank, shift, index), a.reps),
          'window_rolls_all_outputs': events_ms(lambda: ds.window_rolls(first_bar, shift), a.reps),
          'detrend': events_ms(lambda: D.detrend_pianotree(full[3], full[4]), a.reps)}
    import dataset_ref as R
    host_ids = ids[:a.host_items].tolist()
    t0 = time.perf_counter()
    for id in host_ids:
        bar, sh = R.id_to_window(ds.valid_inds, -6, 5, id)
        R.item(data, bar, sh)
    host_ms_item = (time.perf_counter() - t0) * 1e3 / len(host_ids)
    out = {'what': 'note bank -> batches', 'batch': B, 'reps': a.reps, 'bars': a.bars, 'windows': n_win,
           'ms_per_batch_events': {k: round(v, 4) for k, v in ms.items()},
           'batches_per_s': {k: round(1e3 / v, 1) for k, v in ms.items()},
           'host_restatement_ms_per_item': round(host_ms_item, 2), 'host_restatement_batches_per_s': round(1e3 / (host_ms_item * B), 3),
           'bank_bytes_per_window': round(ds.bank_bytes / n_win, 1), 'roll_bank_bytes_per_window': 4096 + 448,
           'pack_and_upload_s': round(pack_s, 2)}
    if a.train:
        out['train_samples_per_s'] = {
            'roll_bank': train_epoch(dev, DeviceBatcher(pr_bank[:1024], ch_bank[:1024], B, seed=1, device=dev, drop_last=True), B),
            'note_bank': train_epoch(dev, DeviceBatcher(ds.subset(ds.valid_inds[:1024], -6, 5), None, B, seed=1, drop_last=True), B),
            'note_bank_6_slots': train_epoch(dev, DeviceBatcher(ds.subset(ds.valid_inds[:1024], -6, 5), None, B, seed=1, drop_last=True,
                                                                slots=D.SLOTS), B)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
