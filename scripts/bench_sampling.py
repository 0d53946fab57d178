"""The sampled and the truncated-sampled free-running decode beside the argmax decode, same process, same batch (BASELINE configs[3]: batch
2048, the step loop replayed from a captured hipGraph): --rounds interleaved rounds of --reps decodes each, timed by events after a warm-up;
every round uses another draw, none needs a new capture.  Prints one JSON line with the ranges, the cost of sampling and the cost of
truncation (top_k / min_p: the 32-round select and the row maximum in the pitch phase of every note step; top_p: nine exponentials and
the 32-round select on integer masses), the nucleus rows -- top_p alone and top_k + top_p -- beside the others in the same process.
The constrained rows (pitch masks / ascending notes: one 16-byte mask load per row and launch, a few integer operations per class) are
the chord-tone mask of a synthetic batch's c, `ascending`, and both with top_k + top_p; they are reported against the plain sampled
decode of the same process.
The keep rows (kept time steps, keep=: six force words per row and note step, one select per decision) decode the same batch with the
first bar of a synthetic grid kept under plain sampling, and with a per-row alternating pattern ((t + b) % 4 < 2) kept under mask +
ascending + top_k + top_p; each is reported against the same setting without a keep.
The rhythm rows (kept rhythm, DisentangleVAE.keep_rhythm: every step of the same grid keeps its note count and durations, the pitches are
drawn again) run under plain sampling -- sent as the constrained kind with a block that constrains nothing, as the model sends it -- and
under mask + ascending + top_k + top_p; each beside the same setting without a keep.
The top rows (kept top voice, DisentangleVAE.keep_top: every step of the same grid keeps its top note and its note count, the notes under it
are drawn again under their ceilings) run under plain sampling -- sent as the constrained kind with the ascending flag, as the model sends
it, and reported beside `ascending` -- and under mask + ascending + top_k + top_p, beside the same setting without a keep.
The limits rows (duration limits, DisentangleVAE.dur_limits: every step fit to the bar with a floor of two sixteenths, every decision
free inside its range) run under plain sampling -- sent as the constrained kind with the vacuous constraint, like the rhythm row, and to
be read beside it -- and under mask + ascending + top_k + top_p, beside the same setting without a keep and beside the rhythm row.
The count rows (note-count limits, DisentangleVAE.count_limits: every step gets at least two and at most four notes -- two floor words
and one forced <eos> per step) run under plain sampling, sent as the constrained kind with the vacuous constraint like the rhythm row and
to be read beside it, and under mask + ascending + top_k + top_p, beside the same setting without a keep and beside the rhythm row.
The logprob rows (--logprob 1; PtvaeDecoder.decode_logprob, DisentangleVAE.decode_best_of) time the log-probability pass ALONE -- the two
launches after a plain sampled decode, and after the mask + ascending + top_k + top_p decode, where every row also runs the allowed rule
and both 32-round selects -- and decode_best_of(n=4) at a quarter of the batch (as many decoded rows as one plain decode of the batch).
The rows rows (--rows 1; per-row sampling, DisentangleVAE.row_sampling: the row-wise kind, whose kernels read temperature, top_k, min_p,
top_p and the sample id of every row from a table) run (a) a uniform table holding the plain sampled values, beside the plain sampled
decode and beside the constrained scalar kind with the same values ('constrained plain': the kernels the row-wise kind is made from), and
(b) the six-group table of the tests -- no rule, T = 0, top_k = 4, top_p = 0.85, min_p = 0.2, top_k = 8 + top_p = 0.9 + min_p = 0.05 by
row % 6, so that every wave holds four rules and both selects diverge between its rows -- beside 'constrained top_k+top_p', the scalar
decode of its most expensive member.
The sounding rows (--sounding 1; sounding state, DisentangleVAE.sounding: one ptv_sounding_step launch between two note loops, 32 more
launches on the decode's chain, and the note loops on the effective mask and force arrays) run no_restrike under plain sampling -- sent
as the constrained kind with the vacuous constraint, as the model sends it -- beside the plain sampled decode, and no_restrike +
max_sounding = 4 + min_sounding = 1 under mask + ascending + top_k + top_p, beside the same setting without sounding.

    python scripts/bench_sampling.py [--batch 2048] [--rounds 3] [--reps 5] [--temperature 1.0] [--top-k 8] [--min-p 0.9] [--top-p 0.9]
                                     [--constrained 1] [--keep 1] [--logprob 1] [--rows 1] [--sounding 1] [--eager]

--top-k 0, --min-p 0 and --top-p 0 switch the rule off; with top_k and min_p both off the 'truncated' decode is not timed, with top_p
off the two nucleus rows are not; --constrained 0 leaves the constrained rows out.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphonic_chord_texture_disentanglement_amd import functional_free as FF_          # noqa: E402
from polyphonic_chord_texture_disentanglement_amd import model as M                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--top-k', type=int, default=8, help='0 = off')
    ap.add_argument('--min-p', type=float, default=0.9, help='0 = off')
    ap.add_argument('--top-p', type=float, default=0.9, help='0 = off')
    ap.add_argument('--constrained', type=int, default=1, help='0 = no constrained rows')
    ap.add_argument('--keep', type=int, default=1, help='0 = no keep rows')
    ap.add_argument('--logprob', type=int, default=1, help='0 = no logprob / best-of rows')
    ap.add_argument('--rows', type=int, default=1, help='0 = no per-row sampling rows')
    ap.add_argument('--sounding', type=int, default=1, help='0 = no sounding rows')
    ap.add_argument('--eager', action='store_true', help='no graph replay')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = M.DisentangleVAE.init_model(dev).to(dev).set_precision('bf16')
    m.eval()
    m.decoder.use_graph = not a.eager
    z = torch.randn(a.batch, 512, device=dev)
    trunc = dict(top_k=a.top_k or None, min_p=a.min_p or None)
    kinds = ['argmax', 'sampled'] + (['truncated'] if a.top_k or a.min_p else [])
    nucleus = {}
    if a.top_p:
        nucleus['top_p'] = dict(top_p=a.top_p)
        if a.top_k:
            nucleus['top_k+top_p'] = dict(top_k=a.top_k, top_p=a.top_p)
    kinds += list(nucleus)
    constrained = {}
    if a.constrained:
        from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch
        c = torch.from_numpy(synth_batch(64, 5)[1]).to(dev)
        mask = m.pitch_mask(c=c[torch.arange(a.batch, device=dev) % 64].contiguous())        # [batch, 32, 4]: every row its own chord tones
        constrained['mask'] = dict(pitch_mask=mask)
        constrained['ascending'] = dict(ascending=True)
        constrained['mask+ascending+top_k+top_p'] = dict(pitch_mask=mask, ascending=True, top_k=a.top_k or None, top_p=a.top_p or None)
    kinds += list(constrained)
    keeps = {}                                               # kind -> (the kind it is compared with, its Keep)
    if a.keep:
        from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch
        rows = torch.arange(a.batch, device=dev)
        x = torch.from_numpy(synth_batch(64, 5)[0]).to(dev)[rows % 64].contiguous()          # [batch, 32, 16, 6]
        keeps['keep first bar'] = ('sampled', m.keep(x, range(16)))
        if a.constrained:
            alt = ((torch.arange(32, device=dev)[None, :] + rows[:, None]) % 4 < 2)
            keeps['keep alternating+mask+ascending+top_k+top_p'] = ('mask+ascending+top_k+top_p', m.keep(x, alt))
        keeps['keep rhythm'] = ('sampled', m.keep_rhythm(x, range(32)))
        if a.constrained:
            keeps['keep rhythm+mask+ascending+top_k+top_p'] = ('mask+ascending+top_k+top_p', m.keep_rhythm(x, range(32)))
        keeps['keep top'] = ('ascending' if a.constrained else 'sampled', m.keep_top(x, range(32)))
        if a.constrained:
            keeps['keep top+mask+ascending+top_k+top_p'] = ('mask+ascending+top_k+top_p', m.keep_top(x, range(32)))
        keeps['dur limits'] = ('sampled', m.dur_limits(min_dur=2, fit='bar', batch=a.batch))
        if a.constrained:
            keeps['dur limits+mask+ascending+top_k+top_p'] = ('mask+ascending+top_k+top_p', m.dur_limits(min_dur=2, fit='bar', batch=a.batch))
        keeps['count limits'] = ('sampled', m.count_limits(min_count=2, max_count=4, batch=a.batch))
        if a.constrained:
            keeps['count limits+mask+ascending+top_k+top_p'] = ('mask+ascending+top_k+top_p', m.count_limits(min_count=2, max_count=4, batch=a.batch))
    kinds += list(keeps)
    rowwise = {}                                             # kind -> (the kinds it is compared with, its RowSampling)
    if a.rows:
        six = (dict(), dict(t=0.0), dict(top_k=4), dict(top_p=0.85), dict(min_p=0.2), dict(top_k=8, top_p=0.9, min_p=0.05))
        col = lambda key, default=None: [six[b % 6].get(key, default) for b in range(a.batch)]           # noqa: E731
        rowwise['rows uniform'] = (('sampled', 'constrained plain'), m.row_sampling(a.batch, a.temperature))
        rowwise['rows mixed'] = (('constrained top_k+top_p',), m.row_sampling(a.batch, col('t', a.temperature), top_k=col('top_k'),
                                                                           min_p=col('min_p'), top_p=col('top_p')))
        kinds += ['constrained plain', 'constrained top_k+top_p'] + list(rowwise)
    sounds = {}                                              # kind -> (the kind it is compared with, its Sounding)
    if a.sounding:
        sounds['sounding no_restrike'] = ('sampled', m.sounding(no_restrike=True, batch=a.batch))
        if a.constrained:
            sounds['sounding all+mask+ascending+top_k+top_p'] = ('mask+ascending+top_k+top_p',
                                                                 m.sounding(no_restrike=True, max_sounding=4, min_sounding=1, batch=a.batch))
        kinds += list(sounds)
    blocks = {'argmax': [None] * (a.rounds + 1),
              'sampled': [FF_.sampling_block(dev, a.temperature, seed=7, draw=d) for d in range(a.rounds + 1)],
              'truncated': [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, **trunc) for d in range(a.rounds + 1)]}
    for k, kw in nucleus.items():
        blocks[k] = [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, **kw) for d in range(a.rounds + 1)]
    for k, kw in constrained.items():
        blocks[k] = [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, **kw) for d in range(a.rounds + 1)]

    if a.rows:
        blocks['constrained plain'] = [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, ascending=False) for d in range(a.rounds + 1)]
        blocks['constrained top_k+top_p'] = [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, ascending=False, top_k=8, top_p=0.9)
                                             for d in range(a.rounds + 1)]
    for k, (_, rs) in rowwise.items():
        blocks[k] = [FF_.sampling_block(dev, seed=7, draw=d, rows=rs) for d in range(a.rounds + 1)]
    for k, (base, _) in keeps.items():
        blocks[k] = blocks[base]
    if 'keep rhythm' in keeps:                               # a rhythm keep needs the constrained kind: the vacuous constraint
        blocks['keep rhythm'] = [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, ascending=False) for d in range(a.rounds + 1)]
    if 'dur limits' in keeps:                                # ... and so do duration limits
        blocks['dur limits'] = blocks['keep rhythm']
    if 'count limits' in keeps:                              # ... and a floor of note-count limits
        blocks['count limits'] = blocks['keep rhythm']
    if 'keep top' in keeps:                                  # a top keep needs the constrained kind with the ascending flag
        blocks['keep top'] = [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, ascending=True) for d in range(a.rounds + 1)]

    for k, (base, _) in sounds.items():
        blocks[k] = blocks[base]
    if 'sounding no_restrike' in sounds:                     # no_restrike needs the constrained kind: the vacuous constraint
        blocks['sounding no_restrike'] = [FF_.sampling_block(dev, a.temperature, seed=7, draw=d, ascending=False) for d in range(a.rounds + 1)]

    def run(block, keep=None, snd=None):
        with torch.no_grad():
            m.decoder(z, True, None, None, 0., 0., sampling=block, keep=keep, sounding=snd)

    def timed(block, keep=None, snd=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            run(block, keep, snd)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for _ in range(2):                                       # warm-up: every graph captured, allocator settled
        for k in kinds:
            run(blocks[k][-1], keeps[k][1] if k in keeps else None, sounds[k][1] if k in sounds else None)
    torch.cuda.synchronize()
    captures = m.decoder.graph_captures
    ms = {k: [] for k in kinds}
    for r in range(a.rounds):                                # interleaved: drift of the box hits all alike
        for k in kinds:
            ms[k].append(timed(blocks[k][r], keeps[k][1] if k in keeps else None, sounds[k][1] if k in sounds else None))
    assert m.decoder.graph_captures == captures              # a new draw is not a new capture
    rate = {k: [round(a.batch / (v * 1e-3), 1) for v in vs] for k, vs in ms.items()}
    best = {k: max(v) for k, v in rate.items()}
    out = {'what': 'free-running decode: argmax, sampled, truncated-sampled, nucleus-sampled and constrained decisions, kept steps, per-row sampling', 'batch': a.batch, 'graph': not a.eager, 'reps': a.reps,
           'temperature': a.temperature, 'top_k': a.top_k, 'min_p': a.min_p, 'top_p': a.top_p, 'ms_per_decode': {k: [round(x, 3) for x in v] for k, v in ms.items()},
           'samples_per_s': rate, 'sampled_over_argmax_best': round(best['sampled'] / best['argmax'], 4)}
    if 'truncated' in kinds:
        out['truncated_over_sampled_best'] = round(best['truncated'] / best['sampled'], 4)
        out['truncated_over_argmax_best'] = round(best['truncated'] / best['argmax'], 4)
    for k in list(nucleus) + list(constrained):
        out[k + '_over_sampled_best'] = round(best[k] / best['sampled'], 4)
    for k, (base, _) in keeps.items():
        out[k + '_over_' + base + '_best'] = round(best[k] / best[base], 4)
        out[k + '_over_' + base + '_by_round'] = [round(x / y, 4) for x, y in zip(rate[k], rate[base])]
    for k, other in (('count limits', 'keep rhythm'), ('count limits+mask+ascending+top_k+top_p', 'keep rhythm+mask+ascending+top_k+top_p')):
        if k in keeps and other in keeps:                    # the count limits beside the keep they are made like, round by round
            out[k + '_over_' + other + '_by_round'] = [round(x / y, 4) for x, y in zip(rate[k], rate[other])]
    for k, (base, _) in sounds.items():
        out[k + '_over_' + base + '_best'] = round(best[k] / best[base], 4)
        out[k + '_over_' + base + '_by_round'] = [round(x / y, 4) for x, y in zip(rate[k], rate[base])]
        out[k + '_minus_' + base + '_ms_by_round'] = [round(x - y, 3) for x, y in zip(ms[k], ms[base])]
    for k, (bases, _) in rowwise.items():
        for base in bases:
            out[k + '_over_' + base + '_best'] = round(best[k] / best[base], 4)
            out[k + '_over_' + base + '_by_round'] = [round(x / y, 4) for x, y in zip(rate[k], rate[base])]
    if a.logprob:
        def timed_pass():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            m.decoder.decode_logprob()                       # (warm-up of the pass itself)
            e0.record()
            for _ in range(a.reps):
                m.decoder.decode_logprob()
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) / a.reps, 4)

        lp = {}
        full = 'mask+ascending+top_k+top_p'
        for k in ['sampled'] + ([full] if full in blocks else []):
            lp[k] = []
            for r in range(a.rounds):
                run(blocks[k][r])
                lp[k].append(timed_pass())
        out['logprob_pass_ms'] = lp
        out['logprob_pass_over_sampled_decode'] = {k: round(min(v) / min(ms['sampled']), 5) for k, v in lp.items()}
        nb, n = max(a.batch // 4, 1), 4
        zc, zr = z[:nb, :256].contiguous(), z[:nb, 256:].contiguous()
        bo = []
        for r in range(a.rounds + 1):                        # (round 0: warm-up and the capture of the tiled batch, dropped)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.reps):
                m.decode_best_of(zc, zr, n, temperature=a.temperature, seed=7, draw=r * a.reps + i)
            e1.record()
            torch.cuda.synchronize()
            bo.append(round(e0.elapsed_time(e1) / a.reps, 3))
        out['best_of_4_ms'] = {'batch': nb, 'decoded_rows': nb * n, 'ms_per_call': bo[1:]}
    out['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
