"""The per-sample score pass beside the loss node's forward pass over the same logits, same process, same tensors (full geometry, the
decoder's step-major layout with 136-float pitch rows): ptv_recon_step_scores + ptv_score_fold against ptv_pianotree_targets +
ptv_ce_fwd (pitch) + ptv_ce_fwd (duration).  --reps interleaved repetitions after a warm-up, each timed by its own event pair on one
stream with nothing else on the device; prints one JSON line with the medians, their ratio and the achieved GB/s.

    python scripts/bench_score.py [--batch 512] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphonic_chord_texture_disentanglement_amd._lib import call, ptr, stream_ptr      # noqa: E402
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    B, rows = a.batch, a.batch * 480
    torch.manual_seed(0)
    xh = synth_batch(B, 31)[0]
    x = torch.from_numpy(xh).to(dev).long().contiguous()
    pitch = torch.randn(rows, 136, device=dev) * 3.0                                     # [15][32][B] rows, 130 classes + 6 floats of padding
    dur = torch.randn(rows, 10, device=dev) * 3.0
    step_scores = torch.empty(B, 32, 2, device=dev)
    step_counts = torch.empty(B, 32, 6, device=dev, dtype=torch.int32)
    scores = torch.empty(B, 2, device=dev)
    counts = torch.empty(B, 6, device=dev, dtype=torch.int32)
    pitch_t = torch.empty(rows, device=dev, dtype=torch.int32)
    dur_t = torch.empty(rows * 5, device=dev, dtype=torch.int32)
    sums = torch.zeros(8, device=dev)
    tcounts = torch.zeros(3, device=dev, dtype=torch.int32)
    st = stream_ptr()

    def new():
        call('ptv_recon_step_scores', ptr(pitch), 136, ptr(dur), ptr(x), B, 1, ptr(step_scores), ptr(step_counts), st)
        call('ptv_score_fold', ptr(step_scores), ptr(step_counts), B, ptr(scores), ptr(counts), st)

    def parent():
        call('ptv_pianotree_targets', ptr(x), B, 1, ptr(pitch_t), ptr(dur_t), ptr(tcounts), st)
        call('ptv_ce_fwd', ptr(pitch), 136, ptr(pitch_t), rows, 130, 130, ptr(sums[0:]), st)
        call('ptv_ce_fwd', ptr(dur), 2, ptr(dur_t), rows * 5, 2, 2, ptr(sums[1:]), st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                                                 # us

    for _ in range(a.warmup):
        new()
        parent()
    torch.cuda.synchronize()
    us = {'scores': [], 'loss_forward': []}
    for _ in range(a.reps):                                                              # interleaved: drift of the box hits both alike
        us['scores'].append(timed(new))
        us['loss_forward'].append(timed(parent))
    med = {k: statistics.median(v) for k, v in us.items()}
    # the two passes agree on what they computed (sums of the same NLLs, counts of the same targets)
    sums.zero_()
    tcounts.zero_()
    parent()
    new()
    torch.cuda.synchronize()
    s, c = scores.double().sum(0).tolist(), counts.long().sum(0).tolist()
    ls, lc = sums.tolist(), tcounts.tolist()
    assert c[0] == lc[0] and c[2] == lc[1], (c, lc)
    assert abs(s[0] - ls[0]) <= 1e-5 * abs(ls[0]) and abs(s[1] - ls[1]) <= 1e-5 * abs(ls[1]), (s, ls)
    live_p = int((xh[:, :, 1:, 0] != 130).sum())
    live_d = int((xh[:, :, 1:, 1:] != 2).sum())
    nominal = rows * (130 + 10) * 4 + x.numel() * 8                                      # every logit once + x
    touched = live_p * 130 * 4 + live_d * 2 * 4 + x.numel() * 8                          # ignored rows and bits are never loaded
    print(json.dumps({'what': 'per-sample scores (step scores + fold) vs the loss forward (targets + 2 x ce_fwd), step-major logits',
                      'batch': B, 'reps': a.reps, 'us_median': {k: round(v, 2) for k, v in med.items()},
                      'us_min': {k: round(min(v), 2) for k, v in us.items()}, 'us_max': {k: round(max(v), 2) for k, v in us.items()},
                      'scores_over_loss_forward': round(med['scores'] / med['loss_forward'], 3),
                      'live_pitch_rows': live_p, 'pitch_rows': rows, 'bytes_nominal': nominal, 'bytes_touched': touched,
                      'scores_gbps_nominal': round(nominal / med['scores'] * 1e-3, 1),
                      'scores_gbps_touched': round(touched / med['scores'] * 1e-3, 1),
                      'device': torch.cuda.get_device_name(0)}))


if __name__ == '__main__':
    main()
