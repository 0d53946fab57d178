"""Numpy restatement of the output path (test side only -- never imported by the product): what ptv_grid_to_pr and ptv_chord_tokens
define, per sample, in plain loops.  Checked against the reference-generated fixture (tests/golden/output_path.npz) on the CPU; the GPU
tests compare the kernels with it where the fixture has no case (large batches, flagged samples' skip rule, x_clean)."""
import numpy as np

ERR_PITCH, ERR_DUR, ERR_FIRST_IS_DUR, ERR_CLEAN_FULL = 1, 2, 4, 8


def grid_to_pr(grid, max_notes=10, min_pitch=0, pitch_eos=129, max_simu_note=16):
    """grid [32,R,6] -> (pr int [32,128], notes [(pitch, t, dur)], x_clean int64 [32,16,6], err).  A row the reference would raise on
    (pitch outside 0..127: IndexError; a duration bit that is not 0 or 1: ValueError, which it meets first) is skipped and flagged.
    Stricter than the reference on values no decoder emits: a negative pitch is flagged (numpy would wrap the index), and so is a
    duration "bit" such as 10 or 11 (int(''.join(..), 2) would read its digits as binary)."""
    grid = np.asarray(grid)
    if grid.shape[1] == max_simu_note:
        grid = grid[:, 1:]
    pr = np.zeros((32, 128), dtype=np.int64)
    x_clean = np.full((32, 16, 6), 2, dtype=np.int64)
    x_clean[:, :, 0] = 130
    x_clean[:, 0, 0] = 128
    notes, err = [], 0
    for t in range(32):
        kept = 0
        for n in range(min(max_notes, grid.shape[1])):
            row = [int(v) for v in grid[t, n]]
            if row[0] == pitch_eos:
                break
            pitch = row[0] + min_pitch
            bad_dur = any(v not in (0, 1) for v in row[1:])
            bad_pitch = not 0 <= pitch <= 127
            if bad_dur or bad_pitch:
                if not err & (ERR_PITCH | ERR_DUR) and bad_dur:
                    err |= ERR_FIRST_IS_DUR
                err |= (ERR_PITCH if bad_pitch else 0) | (ERR_DUR if bad_dur else 0)
                continue
            dur = 1 + sum(v << (4 - k) for k, v in enumerate(row[1:]))
            pr[t, pitch] = min(dur, 32 - t)
            notes.append((pitch, t, dur))
            if kept < 14:
                x_clean[t, 1 + kept] = [pitch] + row[1:]
            else:
                err |= ERR_CLEAN_FULL
            kept += 1
        x_clean[t, 1 + min(kept, 14), 0] = 129
    return pr, notes, x_clean, err


def note_tuples(notes, bpm=60., start=0.):
    alpha = 0.25 * 60 / bpm
    return [(p, start + t * alpha, start + (t + d) * alpha) for p, t, d in notes]


def chord_tokens(root, chroma, bass):
    """logits root [..., 12], chroma [..., 12, 2], bass [..., 12] -> (c [..., 36], chord14 [..., 14]) f32; first maximal index"""
    root, chroma, bass = (np.asarray(a) for a in (root, chroma, bass))
    ir, ib = root.argmax(-1), bass.argmax(-1)                           # (numpy: first occurrence of the maximum)
    bits = (chroma[..., 1] > chroma[..., 0]).astype(np.float32)
    eye = np.eye(12, dtype=np.float32)
    c = np.concatenate([eye[ir], bits, eye[ib]], axis=-1)
    chord14 = np.concatenate([ir[..., None].astype(np.float32), bits, ib[..., None].astype(np.float32)], axis=-1)
    return c, chord14


def fixture_groups(g):
    """{tag: (grids int64 [n,32,R,6], min_pitch)} of output_path.npz; the grids of `gt` and `dec` live in the older fixtures"""
    from helpers import load_npz
    fam = load_npz('reduced_family.npz')
    groups = {'gt': (load_npz('data_contract.npz')['x'], 0),
              'dec': (np.concatenate([fam[str(k)] for k in g['dec.keys']]), 0)}
    for tag in ('hand16', 'hand15', 'handmp'):
        groups[tag] = (g[tag + '.grid'].astype(np.int64), int(g[tag + '.min_pitch']))
    return groups


def fixture_sample(g, tag, b):
    """the reference's record of sample b of a group: (pr [32,128], notes [n,3], times [n,2], exc 0 / 1 IndexError / 2 ValueError)"""
    count = g[tag + '.count'].astype(np.int64)
    lo = int(count[:b].sum())
    hi = lo + int(count[b])
    return g[tag + '.pr'][b].astype(np.int64), g[tag + '.notes'][lo:hi].astype(np.int64), g[tag + '.times'][lo:hi], int(g[tag + '.exc'][b])
