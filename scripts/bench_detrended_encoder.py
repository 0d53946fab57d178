"""The detrended texture encoder (PtvaeEncoder(z_size=256, max_pitch=31) on dt_x, train.py:32) at B = 512, fp32 and bf16, by device events:

  (a) encoder(dt_x.float(), lengths)   the float-copy route: 40-MB fp32 copy, [B*512, 39] product, Transpose01 of the 134-MB embedding
  (b) encode_multihot(dt_x, pad_col=3) the byte multi-hot embedding kernel (ptv_embed_multihot_fwd), no copy and no transpose
  each forward + backward (loss = sum of mean and scale), and the forward alone;
  (c) the eager train step (loss + backward + FusedClipAdam, teacher-forced) of DisentangleVAE.init_model_detrended next to init_model's.

(a) and (b) alternate inside every round (--rounds rounds of --reps calls each, after a warm-up of both): the figure is the median over
rounds, the spread its min / max.  A measurement path without a GPU fails.  Prints one JSON line.

    python scripts/bench_detrended_encoder.py [--batch 512] [--rounds 7] [--reps 10] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polyphonic_chord_texture_disentanglement_amd import dataset as D, model as M          # noqa: E402
from polyphonic_chord_texture_disentanglement_amd.optim import FusedClipAdam               # noqa: E402
from polyphonic_chord_texture_disentanglement_amd.ptvae import PtvaeEncoder                # noqa: E402
from polyphonic_chord_texture_disentanglement_amd.synthetic import fill_state_dict, synth_batch   # noqa: E402


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, rounds, reps):
    """{name: fn} timed in turn inside every round -> {name: {'median_ms', 'min_ms', 'max_ms'}}"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(events_ms(fn, reps))
    return {k: {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    B = a.batch
    x, c, pr = (torch.from_numpy(t).to(dev) for t in synth_batch(B, 77))
    dt_x = D.detrend_pianotree(x, c)
    out = OrderedDict(batch=B, rounds=a.rounds, reps=a.reps, device=torch.cuda.get_device_name(0))

    torch.manual_seed(0)
    enc = PtvaeEncoder(dev, z_size=256, max_pitch=39 - 8, min_pitch=0)
    enc.load_state_dict(fill_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in enc.state_dict().items()), seed=977))
    enc = enc.to(dev)
    lengths = enc.get_len_index_tensor(x)
    for prec in ('fp32', 'bf16'):
        enc.precision = prec

        def old_fwd():
            with torch.no_grad():
                enc.encoder(dt_x.float(), lengths)

        def new_fwd():
            with torch.no_grad():
                enc.encode_multihot(dt_x, pad_col=3)

        def old_fb():
            enc.zero_grad(set_to_none=True)
            d, _ = enc.encoder(dt_x.float(), lengths)
            (d.mean.sum() + d.scale.sum()).backward()

        def new_fb():
            enc.zero_grad(set_to_none=True)
            d, _ = enc.encode_multihot(dt_x, pad_col=3)
            (d.mean.sum() + d.scale.sum()).backward()
        with torch.no_grad():
            da, db = enc.encoder(dt_x.float(), lengths)[0], enc.encode_multihot(dt_x, pad_col=3)[0]
            out['max_diff_mean_%s' % prec] = float((da.mean - db.mean).abs().max())
        out['encoder_%s' % prec] = alternate(OrderedDict(a_float_copy_fwd=old_fwd, b_multihot_fwd=new_fwd, a_float_copy_fwd_bwd=old_fb,
                                                         b_multihot_fwd_bwd=new_fb), a.rounds, a.reps)
    del enc

    if not a.no_step:
        import random
        steps = OrderedDict()
        for name, build, inputs in (('conv', M.DisentangleVAE.init_model, (x, c, pr)),
                                    ('detrended', M.DisentangleVAE.init_model_detrended, (x, c, pr, dt_x))):
            torch.manual_seed(0)
            random.seed(7)
            m = build(dev).to(dev).set_precision('bf16')
            m.use_philox(7, 0)
            opt = FusedClipAdam(m.parameters(), lr=1e-3)

            def step(m=m, opt=opt, inputs=inputs):
                opt.zero_grad()
                losses = m('train', *inputs, tfr1=1., tfr2=1., tfr3=1., beta=0.1, weights=[1, 0.5])
                with torch.autograd.set_multithreading_enabled(False):
                    losses[0].backward()
                opt.clip_and_step(1)
            steps[name] = step
        out['eager_train_step_bf16'] = alternate(steps, a.rounds, a.reps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
