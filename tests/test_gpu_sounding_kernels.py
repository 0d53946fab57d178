"""GPU: ptv_sounding_step alone (include/ptvae_hip.h "Sounding state") on crafted grids, exact integer equality against
tests/sounding_ref.py at B = 1, 5 and 67 (67 rows do not fill the last workgroup of four): t_done = -1, pitches on the word and lane
boundaries (0, 31, 32, 63, 64, 127), duration 32 at step 0, duration 1, an overhang at step 30, the later slot wins, h >= K (word 0
becomes <eos>), K - h >= 15 (nothing written), an owned step, a forced prefix longer than the ceiling, one-row tables, a NULL base mask, a
NULL force pair, unselected steps, and every PTV_ERR_ARG.  The outputs are poisoned first: every element of the step is written and
nothing of any other step."""
import functools

import numpy as np
import pytest
import torch

import sounding_ref as SR
from polyphonic_chord_texture_disentanglement_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -77                                                         # no launch writes it: no mask of the tests, no force word, no count
SENT8 = 0xb3                                                       # rem never exceeds 31
EOS = 129


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def note(p, d):
    v = d - 1
    return (p, (v >> 4) & 1, (v >> 3) & 1, (v >> 2) & 1, (v >> 1) & 1, v & 1)


@functools.lru_cache(maxsize=None)
def crafted(B):
    """(x, K, F, steps, mask, force): random grids and tables with the named cases spliced into row 0 (see the module docstring)"""
    rng = np.random.default_rng(900 + B)
    x = SR.random_grids(B, 40 + B)
    for s in range(6):
        x[0, s] = 2
        x[0, s, :, 0] = 130
        x[0, s, 0, 0] = 128
        x[0, s, 1, 0] = EOS
    for j, (p, d) in enumerate(((0, 32), (31, 1), (32, 2), (63, 5), (64, 32), (127, 3)), 1):
        x[0, 0, j] = note(p, d)
    x[0, 0, 7, 0] = EOS
    x[0, 1, 1], x[0, 1, 2], x[0, 1, 3, 0] = note(40, 9), note(40, 2), EOS          # the later slot wins: 40 is free again at step 3
    x[0, 30] = x[0, 1]
    x[0, 30, 1], x[0, 30, 2, 0] = note(90, 8), EOS                                 # overhang: cut to 2, held at step 31
    K = rng.integers(0, 10, (B, 32)).astype(np.uint8)
    F = rng.integers(0, 6, (B, 32)).astype(np.uint8)
    steps = (rng.random((B, 32)) < 0.75).astype(np.uint8)
    mask = rng.integers(-2 ** 31, 2 ** 31, (B, 32, 4)).astype(np.int32)
    mask[mask == SENT] = 0
    force = np.full((15, 32 * B), -1, dtype=np.int32)
    for r in range(32 * B):
        kind = rng.integers(0, 6)
        if kind == 1:
            force[:int(rng.integers(1, 8)), r] = 50
        elif kind == 2:
            force[int(rng.integers(0, 15)), r] = EOS
        elif kind == 3:
            force[int(rng.integers(0, 3)), r] = -2
        elif kind == 4:
            force[1, r] = -300                                                     # a BELOW word: owned
    steps[0, :6] = (1, 1, 1, 1, 1, 0)
    K[0, :6], F[0, :6] = (3, 1, 127, 4, 3, 1), (2, 0, 3, 0, 5, 5)
    force[:, [t * B for t in range(6)]] = -1
    force[4, 2 * B] = EOS                                                          # step 2 of row 0 is owned
    force[:6, 3 * B] = (41, 43, 45, 47, 49, 51)                                    # step 3: a prefix of 6 over the ceiling 4 - h
    for a in (x, K, F, steps, mask, force):
        a.setflags(write=False)
    return x, K, F, steps, mask, force


def launch(x, t_done, B, mask_base, force_base, K, F, steps, control, out):
    return lib().ptv_sounding_step(ptr(x), t_done, B, ptr(mask_base), 1 if mask_base is None else mask_base.shape[0], ptr(force_base),
                                   ptr(K), K.shape[0], ptr(F), F.shape[0], ptr(steps), steps.shape[0], ptr(control), ptr(out['rem']),
                                   ptr(out.get('mask_eff')), ptr(out.get('force_eff')), ptr(out['held']), stream_ptr())


def poisoned(B, mask=True, force=True):
    out = dict(rem=torch.full((B, 128), SENT8, dtype=torch.uint8, device=DEV), held=torch.full((B, 32), SENT, dtype=torch.int32, device=DEV))
    if mask:
        out['mask_eff'] = torch.full((B, 32, 4), SENT, dtype=torch.int32, device=DEV)
    if force:
        out['force_eff'] = torch.full((15, 32 * B), SENT, dtype=torch.int32, device=DEV)
    return out


def walk(B, upto, no_restrike, K, F, steps, mask, force, want_mask=True, want_force=True, check_each=False):
    """the launches t_done = -1 .. upto - 1 on poisoned outputs against the reference; with check_each the poison is looked at after
    every launch"""
    x = crafted(B)[0]
    xd, Kd, Fd, Sd, Md, Pd = dev(x), dev(K), dev(F), dev(steps), dev(mask), dev(force)
    control = torch.tensor([1 if no_restrike else 0], dtype=torch.int32, device=DEV)
    out = poisoned(B, want_mask, want_force)
    for t_done in range(-1, upto):
        assert launch(xd if t_done >= 0 else None, t_done, B, Md, Pd, Kd, Fd, Sd, control, out) == 0
        if check_each or t_done == upto - 1:
            torch.cuda.synchronize()
            s1 = t_done + 1
            want = SR.run(x, B, no_restrike, K, F, steps, mask, force, upto=s1)
            got = {k: v.cpu().numpy() for k, v in out.items()}
            assert np.array_equal(got['rem'], want['rem']), (B, s1)
            assert np.array_equal(got['held'][:, :s1 + 1], want['held'][:, :s1 + 1]) and (got['held'][:, s1 + 1:] == SENT).all(), (B, s1)
            if want_mask:
                assert np.array_equal(got['mask_eff'][:, :s1 + 1], want['mask_eff'][:, :s1 + 1]), (B, s1)
                assert (got['mask_eff'][:, s1 + 1:] == SENT).all()
            if want_force:
                n = (s1 + 1) * B
                assert np.array_equal(got['force_eff'][:, :n], want['force_eff'][:, :n]), (B, s1)
                assert (got['force_eff'][:, n:] == SENT).all()
    return got, want


@pytest.mark.parametrize('B', (1, 5, 67))
def test_1_every_step_against_the_reference(B):
    x, K, F, steps, mask, force = crafted(B)
    got, want = walk(B, 31, True, K, F, steps, mask, force, check_each=(B == 5))
    for k in got:
        assert not (got[k] == (SENT8 if k == 'rem' else SENT)).any(), k            # every element of every step was written
    w = got['force_eff'].reshape(15, 32, B)[:, :, 0].T                              # row 0: [32, 15]
    held = got['held'][0]
    bit = lambda s, p: (int(got['mask_eff'][0, s, p >> 5]) >> (p & 31)) & 1
    base = lambda s, p: (int(mask[0, s, p >> 5]) >> (p & 31)) & 1
    assert held[0] == 0 and (w[0, :2] == -2).all() and w[0, 3] == EOS               # step 0: nothing held, F' = 2, H' = 3
    assert held[1] == 5 and all(bit(1, p) == 0 for p in (0, 32, 63, 64, 127)) and bit(1, 31) == base(1, 31)     # duration 1 holds nothing
    assert w[1, 0] == EOS and (w[1, 1:] == -1).all()                                # h >= K: the step is a rest
    assert held[2] == 5 and bit(2, 40) == 0 and bit(2, 32) == base(2, 32)           # 40 struck at step 1; 32 (duration 2) is over
    assert w[2].tolist() == [-1] * 4 + [EOS] + [-1] * 10                            # owned: copied, although K - h >= 15 and F' > 0
    assert held[3] == 3 and bit(3, 40) == base(3, 40) and bit(3, 127) == base(3, 127)     # the later, shorter onset of 40 won; 127 is over
    assert w[3].tolist() == [41, 43, 45, 47, 49, 51, EOS] + [-1] * 8                # the prefix of 6 is longer than the ceiling 4 - 3
    assert held[4] == 3 and w[4].tolist() == [EOS] + [-1] * 14                      # 63 (duration 5) still sounds; K = 3 = h wins over F' = 2
    assert (w[5] == -1).all() and got['mask_eff'][0, 5].tolist() == mask[0, 5].tolist() and held[5] == 2        # unselected: the base
    assert bit(31, 90) == (0 if steps[0, 31] else base(31, 90)) and want['rem'][0, 90] == 1 and want['rem'][0, 0] == 1


@pytest.mark.parametrize('B', (5, 67))
def test_2_one_row_tables_null_bases_and_rules_off(B):
    x, K, F, steps, mask, force = crafted(B)
    one = lambda a: np.ascontiguousarray(a[:1])
    walk(B, 8, True, one(K), one(F), one(steps), one(mask), force)
    walk(B, 8, True, K, one(F), steps, None, force)                                 # NULL base mask: every pitch allowed
    walk(B, 8, True, one(K), F, one(steps), mask, None)                             # NULL base force: every word -1
    walk(B, 8, True, K, F, steps, None, None, want_force=False)                     # NULL force pair: the mask rule alone
    walk(B, 8, False, K, F, steps, None, None, want_mask=False)                     # ... and the count rule alone
    got, _ = walk(B, 8, False, K, F, steps, mask, force)                            # control bit clear: the base mask
    assert np.array_equal(got['mask_eff'][:, :9], mask[:, :9])
    none = np.zeros((1, 32), np.uint8)
    got, _ = walk(B, 8, True, K, F, none, mask, force)                              # nothing selected: the base arrays, the state all the same
    assert np.array_equal(got['mask_eff'][:, :9], mask[:, :9]) and np.array_equal(got['force_eff'][:, :9 * B], force[:, :9 * B])
    assert (got['held'][:, 1:9] > 0).any()
    got, _ = walk(B, 8, False, np.full((1, 32), 127, np.uint8), none, one(steps), None, None, want_mask=False)
    assert (got['force_eff'][:, :9 * B] == -1).all()                                # K - h >= 15: nothing is written


def test_3_arguments():
    B = 5
    x, K, F, steps, mask, force = crafted(B)
    xd, Kd, Fd, Sd, Md, Pd = dev(x), dev(K), dev(F), dev(steps), dev(mask), dev(force)
    control = torch.tensor([1], dtype=torch.int32, device=DEV)
    out = poisoned(B)
    f = lib().ptv_sounding_step
    ok = [ptr(xd), 3, B, ptr(Md), B, ptr(Pd), ptr(Kd), B, ptr(Fd), B, ptr(Sd), B, ptr(control), ptr(out['rem']), ptr(out['mask_eff']),
          ptr(out['force_eff']), ptr(out['held']), stream_ptr()]
    cases = [(0, None), (6, None), (8, None), (10, None), (12, None), (13, None), (16, None),       # a NULL required pointer
             (14, None), (15, None),                                                                # a base table without its output
             (14, ptr(Md)), (15, ptr(Pd)),                                                          # an output that is its source
             (4, 2), (4, 0), (7, 3), (9, 4), (11, B + 1), (11, -1),                                 # a row count outside {1, B}
             (2, 0), (2, -5), (1, -2), (1, 31), (1, 32)]                                            # B < 1, t_done outside -1..30
    for i, v in cases:
        bad = list(ok)
        bad[i] = v
        assert f(*bad) == -1, (i, v)
    torch.cuda.synchronize()
    assert (out['rem'] == SENT8).all().item() and all((out[k] == SENT).all().item() for k in ('mask_eff', 'force_eff', 'held'))
    first = list(ok)
    first[0], first[1] = None, -1                                                                   # t_done = -1 reads no grid
    assert f(*first) == 0
    torch.cuda.synchronize()
    assert not out['rem'].any().item() and not out['held'][:, 0].any().item() and (out['held'][:, 1:] == SENT).all().item()
    assert torch.equal(out['mask_eff'][:, 0], Md[:, 0])                                             # nothing is held at step 0
