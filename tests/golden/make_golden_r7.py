"""Fixture of the output path, recorded from the REFERENCE itself (build container only): tests/golden/output_path.npz.

Imports `/root/reference` unmodified; `pretty_midi` is stubbed by a `Note` class that keeps its four arguments, so the notes the
reference's `PtvaeDecoder.grid_to_pr_and_notes` (ptvae.py:558-575) builds can be read back.  Nothing of the reference is copied: the
file holds inputs and recorded results only.

Grid groups (per sample: the reference's piano-roll and notes, or which exception it raised):
  gt      the ground-truth grids `x` of data_contract.npz                                   (R = 16, not stored again)
  dec     reference-decoded grids of reduced_family.npz: inference_mean, swap_tf             (R = 15, not stored again)
  hand16 / hand15 / handmp   hand-made grids, R = 16 / R = 15 / R = 15 with min_pitch = 21   (stored as uint8)
The method reads only min_pitch, pitch_eos and max_simu_note from `self`: a stand-in object carries them.

At least half of the `dec` samples must pass through the reference without raising (a fixture that compares nothing proves
nothing); main() asserts it.  inference_mean + swap_tf of reduced_family.npz as they stand: 6 of 6 pass.

Chord side: the reference RnnDecoder of the reduced model (weights of reduced_state.npz) in inference, ONE sample per call: with a
batch the reference's index broadcast (ptvae.py:74,77) writes the union of the batch's root / bass argmaxes into every row, with one
sample the token is the row's own.  Recorded: the logits of the 8 steps and the 7 tokens fed back (input of the GRU at steps 1..7).

    python tests/golden/make_golden_r7.py        # needs /root/reference; seconds
"""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = '/root/reference'

DEC_KEYS = ('inference_mean', 'swap_tf')
EXC = {None: 0, IndexError: 1, ValueError: 2}
BPM_START = {'gt': (60., 0.), 'dec': (60., 0.), 'hand16': (90., 1.5), 'hand15': (60., 0.), 'handmp': (120., 0.25)}
MIN_PITCH = {'handmp': 21}


class Note:
    def __init__(self, velocity, pitch, start, end):
        self.velocity, self.pitch, self.start, self.end = velocity, pitch, start, end


def import_reference():
    pm = types.ModuleType('pretty_midi')
    pm.Note = Note
    for n in ('PrettyMIDI', 'Instrument'):
        setattr(pm, n, type(n, (), {'__init__': lambda self, *a, **k: None}))
    sys.modules['pretty_midi'] = pm
    tb = types.ModuleType('tensorboardX')
    tb.SummaryWriter = type('SummaryWriter', (), {'__init__': lambda self, *a, **k: None, 'add_scalar': lambda self, *a, **k: None})
    sys.modules['tensorboardX'] = tb
    sys.path.insert(0, REF)
    import model as ref_model      # noqa
    import ptvae as ref_ptvae      # noqa
    return ref_model, ref_ptvae


def bits(d):
    """5 MSB-first bits of dur - 1"""
    return [((d - 1) >> s) & 1 for s in (4, 3, 2, 1, 0)]


def step_rows(R, notes, eos=True, sos=None):
    """one time step: [<sos>] notes <eos> <pad>...; a note is (pitch, dur) or a ready 6-vector"""
    sos = (R == 16) if sos is None else sos
    rows = [[128, 2, 2, 2, 2, 2]] if sos else []
    for n in notes:
        rows.append(list(n) if len(n) == 6 else [n[0]] + bits(n[1]))
    if eos:
        rows.append([129, 2, 2, 2, 2, 2])
    rows = rows[:R]
    while len(rows) < R:
        rows.append([130, 2, 2, 2, 2, 2])
    return rows


def hand_grid(R, steps):
    """{t: rows}; every other step is empty (<eos> first)"""
    g = np.empty((32, R, 6), dtype=np.int64)
    for t in range(32):
        g[t] = steps.get(t, step_rows(R, []))
    return g


def hand_cases(R):
    S = lambda notes, **k: step_rows(R, notes, **k)
    N = lambda p, d: [p] + bits(d)
    EOS, PAD = [129, 2, 2, 2, 2, 2], [130, 2, 2, 2, 2, 2]
    raw = lambda rows: (([[128, 2, 2, 2, 2, 2]] if R == 16 else []) + rows + [PAD] * R)[:R]      # rows as given, no <eos> added
    many = [(40 + 2 * i, 1 + i) for i in range(14)]
    cases = OrderedDict()
    cases['plain'] = hand_grid(R, {0: S([(60, 4), (64, 4), (67, 8)]), 8: S([(48, 16)]), 31: S([(72, 1)])})
    cases['duplicate_pitch'] = hand_grid(R, {3: S([(60, 2), (62, 5), (60, 7)]), 4: S([(60, 1), (60, 1)])})
    cases['no_eos_in_10'] = hand_grid(R, {5: S(many), 6: S(many[:10]), 7: S(many[:11], eos=False)})
    cases['eos_first'] = hand_grid(R, {})
    cases['eos_then_notes'] = hand_grid(R, {2: raw([EOS, N(50, 3), N(55, 3)]), 3: S([(52, 2)])})
    cases['overrun'] = hand_grid(R, {20: S([(60, 32), (61, 13), (62, 12)]), 31: S([(30, 32), (31, 2)]), 0: S([(0, 32), (127, 32)])})
    cases['sos_before_eos'] = hand_grid(R, {1: S([(60, 4)]), 9: S([(62, 2), [128, 0, 0, 1, 0, 1], (65, 2)])})
    cases['pad_pitch_valid_bits'] = hand_grid(R, {9: S([[130, 0, 0, 0, 0, 0], (65, 2)]), 12: S([(70, 3)])})
    cases['dur_bit_2'] = hand_grid(R, {4: S([(60, 4)]), 10: S([(62, 2), [64, 0, 1, 2, 0, 1], (65, 2)])})
    cases['pad_row_before_eos'] = hand_grid(R, {10: S([(62, 2), [130, 2, 2, 2, 2, 2], (65, 2)])})
    cases['index_then_value'] = hand_grid(R, {2: S([[128, 1, 1, 1, 1, 1]]), 3: S([[60, 2, 0, 0, 0, 0]])})
    cases['bad_after_eos'] = hand_grid(R, {6: raw([N(61, 6), EOS, [128, 0, 0, 0, 0, 0], [60, 2, 2, 2, 2, 2]])})
    cases['bad_in_row_11'] = hand_grid(R, {6: raw([N(*n) for n in many[:10]] + [PAD, [60, 2, 2, 2, 2, 2]])})
    return cases


def record(ref_ptvae, grids, min_pitch, bpm, start):
    """the reference's own grid_to_pr_and_notes per sample"""
    me = types.SimpleNamespace(min_pitch=min_pitch, pitch_eos=129, max_simu_note=16)
    prs, notes, times, count, exc = [], [], [], [], []
    for g in grids:
        try:
            pr, ns = ref_ptvae.PtvaeDecoder.grid_to_pr_and_notes(me, g, bpm, start)
            kind = None
        except (IndexError, ValueError) as e:
            pr, ns, kind = np.zeros((32, 128), dtype=int), [], type(e)
        assert pr.min() >= 0 and pr.max() <= 32
        prs.append(pr.astype(np.uint8))
        alpha = 0.25 * 60 / bpm
        for n in ns:
            assert n.velocity == 100
            t = int(round((n.start - start) / alpha))
            d = int(round((n.end - start) / alpha)) - t
            assert start + t * alpha == n.start and start + (t + d) * alpha == n.end, 'onset / duration not recoverable'
            notes.append((int(n.pitch), t, d))
            times.append((n.start, n.end))
        count.append(len(ns))
        exc.append(EXC[kind])
    return OrderedDict(pr=np.stack(prs), notes=np.array(notes, dtype=np.uint8).reshape(-1, 3),
                       times=np.array(times, dtype=np.float64).reshape(-1, 2), count=np.array(count, dtype=np.int16),
                       exc=np.array(exc, dtype=np.uint8), bpm_start=np.array([bpm, start], dtype=np.float64),
                       min_pitch=np.uint8(min_pitch))


def chord_side(ref_model, ref_ptvae):
    from make_golden import build_reduced
    m = build_reduced(ref_model, ref_ptvae)
    with np.load(os.path.join(HERE, 'reduced_state.npz')) as f:
        m.load_state_dict(OrderedDict((k, torch.from_numpy(f[k])) for k in f.files))
    dec = m.chd_decoder.eval()
    fed = []
    hook = dec.gru.register_forward_pre_hook(lambda mod, args: fed.append(args[0][:, 0, :36].detach().clone()))
    torch.manual_seed(77)
    z = torch.randn(6, 16) * 1.5
    out = OrderedDict(z=z.numpy(), root=[], chroma=[], bass=[], tokens=[])
    with torch.no_grad():
        for b in range(6):
            del fed[:]
            root, chroma, bass = dec(z[b:b + 1], True, 0.)
            out['root'].append(root[0].numpy())
            out['chroma'].append(chroma[0].numpy())
            out['bass'].append(bass[0].numpy())
            out['tokens'].append(torch.cat(fed[1:], 0).numpy())          # (step 0 is fed init_input)
    hook.remove()
    for k in ('root', 'chroma', 'bass'):
        out[k] = np.stack(out[k]).astype(np.float32)
    tok = np.stack(out['tokens'])
    assert tok.shape == (6, 7, 36) and set(np.unique(tok)) <= {0., 1.}
    out['tokens'] = tok.astype(np.uint8)
    return out


def main():
    ref_model, ref_ptvae = import_reference()
    out = OrderedDict()
    with np.load(os.path.join(HERE, 'data_contract.npz')) as f:
        groups = OrderedDict(gt=f['x'])
    with np.load(os.path.join(HERE, 'reduced_family.npz')) as f:
        groups['dec'] = np.concatenate([f[k] for k in DEC_KEYS])
    out['dec.keys'] = np.array(DEC_KEYS)
    for tag, R in (('hand16', 16), ('hand15', 15), ('handmp', 15)):
        cases = hand_cases(R)
        g = np.stack(list(cases.values()))
        if tag == 'handmp':                        # pitches are offsets from min_pitch: bring the notes down so that most stay in range
            g = g.copy()
            note = g[..., 0] < 128
            g[..., 0][note] = np.maximum(g[..., 0][note] - 15, 0)
        groups[tag] = g
        out[tag + '.grid'] = g.astype(np.uint8)
        out[tag + '.names'] = np.array(list(cases.keys()))
        assert np.array_equal(out[tag + '.grid'].astype(np.int64), g)
    for tag, g in groups.items():
        rec = record(ref_ptvae, g, MIN_PITCH.get(tag, 0), *BPM_START[tag])
        for k, v in rec.items():
            out['%s.%s' % (tag, k)] = v
        print(tag, g.shape, 'notes', int(rec['count'].sum()), 'exc', rec['exc'].tolist())
    ok = int((out['dec.exc'] == 0).sum())
    assert 2 * ok >= len(out['dec.exc']), 'fewer than half of the decoded grids pass the reference: take other decodes'
    for tag in ('hand16', 'hand15', 'handmp'):
        assert {0, 1, 2} <= set(out[tag + '.exc'].tolist())
    for k, v in chord_side(ref_model, ref_ptvae).items():
        out['chd.' + k] = v
    path = os.path.join(HERE, 'output_path.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
