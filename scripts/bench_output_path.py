"""From a finished free-running decode to piano-rolls plus note lists at B = 2048: the device output path
(PtvaeDecoder.grid_to_pr_and_notes_batch, one ptv_grid_to_pr launch) against the host way (last_xhat[:, :, 1:].cpu().numpy() and
grid_to_pr_and_notes per sample).  Device side by events over --reps calls after a warm-up, host loop by perf_counter, once.
Prints one JSON line.

    python scripts/bench_output_path.py [--batch 2048] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphonic_chord_texture_disentanglement_amd import model as M                       # noqa: E402
from polyphonic_chord_texture_disentanglement_amd.synthetic import fill_state_dict        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    m = M.DisentangleVAE.init_model(dev)
    m.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 1234))
    m.to(dev).set_precision('bf16')
    gen = torch.Generator().manual_seed(3)
    zc, zr = (torch.randn(a.batch, 256, generator=gen).to(dev) for _ in range(2))
    with torch.no_grad():
        m.eval()
        m.decoder(torch.cat([zc, zr], -1), True, None, None, 0., 0.)
    xhat = m.decoder.last_xhat
    torch.cuda.synchronize()
    dec = m.decoder

    for _ in range(5):
        outs = dec.grid_to_pr_and_notes_batch(xhat)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        outs = dec.grid_to_pr_and_notes_batch(xhat)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.reps
    t0 = time.perf_counter()                                 # the same plus the note lists as host tuples
    pr_mat, notes, count, _, err = dec.grid_to_pr_and_notes_batch(xhat)
    tuples = dec.notes_to_tuples(notes, count)
    torch.cuda.synchronize()
    dev_tuples_ms = (time.perf_counter() - t0) * 1e3

    t0 = time.perf_counter()
    est_x = xhat[:, :, 1:, :].cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    raised, same = 0, 0
    pr_h, err_h = pr_mat.cpu().numpy(), err.cpu().numpy()
    t0 = time.perf_counter()
    host = []
    for b in range(a.batch):
        try:
            host.append(dec.grid_to_pr_and_notes(est_x[b]))
        except (IndexError, ValueError):
            host.append(None)
    loop_ms = (time.perf_counter() - t0) * 1e3
    for b, h in enumerate(host):
        if h is None:
            raised += 1
            assert err_h[b] != 0
        else:
            assert err_h[b] == 0 and np.array_equal(pr_h[b], h[0].astype(np.float32)) and tuples[b] == h[1]
            same += 1
    print(json.dumps({'what': 'decoded grid -> piano-rolls + note lists', 'batch': a.batch, 'reps': a.reps,
                      'device_path_ms_events': round(dev_ms, 4), 'device_path_plus_host_tuples_ms_wall': round(dev_tuples_ms, 2),
                      'host_path_ms_wall': round(copy_ms + loop_ms, 1), 'host_copy_ms': round(copy_ms, 2), 'host_loop_ms': round(loop_ms, 1),
                      'notes': int(count.sum()), 'samples_equal': same, 'samples_the_host_method_raised_on': raised}))


if __name__ == '__main__':
    main()
