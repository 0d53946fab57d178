"""The free-running chord decode on its own, same process, same batch: RnnDecoder.decode_tokens (the Python-sequenced step loop with the
reference's union-over-the-batch token: 4 + 8 * 5 + 7 launches, a memset and ptv_chord_tokens) beside RnnDecoder.decode_chords (one C
call, ptv_chord_decode: 4 + 8 * 6 + 1 launches) as argmax, sampled, and sampled with return_logprob.  --rounds interleaved rounds of
--reps decodes each, timed by device events after a warm-up; every round of the sampled rows uses another draw.  Prints one JSON line
with the ranges.  The two paths do not compute the same chords at B > 1: this compares their cost, not their output.
The chord grammar (ptv_chord_decode_grammar: the same launches with the decide launch replaced) runs beside them in the same process:
the identity rule, a key mask per row, and key + 'sevenths' + chord-tone bass, each as argmax and sampled with log-probabilities.

    python scripts/bench_chord_decode.py [--batch 2048] [--rounds 5] [--reps 20] [--temperature 1.0] [--precision bf16]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphonic_chord_texture_disentanglement_amd import model as M                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--precision', default='bf16', choices=('fp32', 'bf16'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = M.DisentangleVAE.init_model(dev).to(dev).set_precision(a.precision)
    m.eval()
    cd = m.chd_decoder
    z = torch.randn(a.batch, 256, device=dev)
    kinds = {
        'decode_tokens': lambda d: cd.decode_tokens(z),
        'decode_chords argmax': lambda d: cd.decode_chords(z),
        'decode_chords sampled': lambda d: cd.decode_chords(z, temperature=a.temperature, seed=7, draw=d),
        'decode_chords sampled+logprob': lambda d: cd.decode_chords(z, temperature=a.temperature, seed=7, draw=d, return_logprob=True),
    }
    key = torch.arange(a.batch, device=dev) % 12
    grammars = {'identity': m.chord_grammar(batch=a.batch), 'key': m.chord_grammar(key=key),
                'key+sevenths+bass': m.chord_grammar(key=key, qualities='sevenths', bass_in_chord=True)}
    for name, g in grammars.items():
        kinds['grammar %s argmax' % name] = lambda d, g=g: cd.decode_chords(z, grammar=g)
        kinds['grammar %s sampled+logprob' % name] = lambda d, g=g: cd.decode_chords(z, temperature=a.temperature, seed=7, draw=d, grammar=g,
                                                                                     return_logprob=True)

    def timed(f, r):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            f(r * a.reps + i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for _ in range(3):                                       # warm-up: code objects loaded, allocator settled
        for f in kinds.values():
            f(0)
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    for r in range(a.rounds):                                # interleaved: drift of the box hits all alike
        for k, f in kinds.items():
            ms[k].append(timed(f, r))
    out = {'what': 'free-running chord decode: decode_tokens (Python-sequenced, union token) and decode_chords (one C call, row-independent)',
           'batch': a.batch, 'precision': a.precision, 'reps': a.reps, 'temperature': a.temperature,
           'ms_per_decode': {k: [round(x, 4) for x in v] for k, v in ms.items()},
           'range_ms': {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           'launches': {'decode_tokens': 4 + 8 * 5 + 7 + 2, 'decode_chords': 4 + 8 * 6 + 1, 'decode_chords grammar': 4 + 8 * 6 + 1},
           'decode_chords_argmax_over_decode_tokens_by_round': [round(x / y, 4) for x, y in zip(ms['decode_chords argmax'], ms['decode_tokens'])],
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
