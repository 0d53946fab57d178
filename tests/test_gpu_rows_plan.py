"""ptv_rows_plan (csrc/notes_persist.hip): the row plan of a length-sorted pass -- the permutation, the lengths in that order and the
128-row segment counts of every step -- from one launch of independent workgroups.

Reference: numpy.  perm = argsort(-clip(len, 0, max_len), kind='stable'); len_sorted = clip(len)[perm]; seg_n[s] = 128 * ceil(C_s / 128)
with C_s = #{rows: clip(len) > s}.  Everything is compared for exact equality, against the reference and against the three entry points
the call stands for (ptv_rows_by_length, ptv_gather_rows of the clamped lengths, ptv_rows_seg_counts).  Outputs are poisoned first, so
an element nobody wrote shows; refusals must leave them poisoned."""
import numpy as np
import pytest
import torch

import kernel_ops as K_

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = 0x3fffffff
ERR_ARG, ERR_UNSUPPORTED = -1, -3
MAX_R = 65536                                    # PTV_ROWS_PLAN_MAX_R of include/ptvae_hip.h
PATTERNS = ('equal', 'zero', 'descending', 'ascending', 'random', 'clamp')


def lengths_of(pattern, R, max_len, rng):
    r = np.arange(R, dtype=np.int64)
    if pattern == 'equal':
        return np.full(R, max(max_len - 2, 0), np.int32)
    if pattern == 'zero':
        return np.zeros(R, np.int32)
    if pattern == 'descending':                  # (strictly descending where R <= max_len + 1; a descending staircase otherwise)
        return (max_len - (r * (max_len + 1)) // R).astype(np.int32)
    if pattern == 'ascending':                   # (every row moves; ties keep their row order)
        return ((r * (max_len + 1)) // R).astype(np.int32)
    if pattern == 'random':
        return rng.randint(0, max_len + 1, R).astype(np.int32)
    assert pattern == 'clamp'                    # values below 0 and above max_len
    v = rng.randint(-5, max_len + 6, R).astype(np.int32)
    v[::7] = -2 ** 31
    v[3::11] = 2 ** 31 - 1
    return v


def reference(lengths, max_len, steps):
    c = np.clip(lengths.astype(np.int64), 0, max_len)
    perm = np.argsort(-c, kind='stable')
    live = np.array([(c > s).sum() for s in range(steps)], np.int64)
    return perm.astype(np.int32), c[perm].astype(np.int32), ((live + 127) // 128 * 128).astype(np.int32)


def poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int32, device=DEV)


def old_entry_points(len_d, R, max_len, steps, with_seg):
    """the three calls the plan stands for, on the clamped lengths"""
    clamped = len_d.clamp(0, max_len)
    perm, len_s = poisoned(R), poisoned(R)
    assert K_.leaf_rc('ptv_rows_by_length', len_d, perm, R, max_len) == 0
    assert K_.leaf_rc('ptv_gather_rows', len_s, clamped, perm, R, 1, 0, 0, 1) == 0
    seg = None
    if with_seg:
        seg = poisoned(steps)
        assert K_.leaf_rc('ptv_rows_seg_counts', len_s, R, steps, seg) == 0
    return perm, len_s, seg


@pytest.mark.parametrize('R', [1, 100, 128, 384, 2176, 16384])
def test_plan_equals_numpy_and_the_three_entry_points(R):
    """every pattern x max_len 15 / 38 x steps 15 / 16 / 64; R = 1 and 100 are no multiple of 128 and take no segment counts"""
    rng = np.random.RandomState(R)
    with_seg = R % 128 == 0
    for max_len in (15, 38):
        for pattern in PATTERNS:
            lengths = lengths_of(pattern, R, max_len, rng)
            len_d = torch.from_numpy(lengths).to(DEV)
            old = {}
            for steps in (15, 16, 64):
                tag = 'R %d max_len %d %s steps %d' % (R, max_len, pattern, steps)
                perm, len_s, seg = poisoned(R + 8), poisoned(R + 8), poisoned(steps + 8)
                rc = K_.leaf_rc('ptv_rows_plan', len_d, R, max_len, steps, perm, len_s, seg if with_seg else None)
                assert rc == 0, tag
                want_perm, want_len, want_seg = reference(lengths, max_len, steps)
                got_perm, got_len, got_seg = perm.cpu().numpy(), len_s.cpu().numpy(), seg.cpu().numpy()
                assert np.array_equal(got_perm[:R], want_perm), tag
                assert np.array_equal(got_len[:R], want_len), tag
                assert (got_perm[R:] == POISON).all() and (got_len[R:] == POISON).all(), tag      # nothing beyond the R rows
                if with_seg:
                    assert np.array_equal(got_seg[:steps], want_seg), tag
                    assert (got_seg[steps:] == POISON).all(), tag
                else:
                    assert (got_seg == POISON).all(), tag
                key = steps if with_seg else 0
                if key not in old:
                    old[key] = old_entry_points(len_d, R, max_len, steps, with_seg)
                o_perm, o_len, o_seg = old[key]
                assert torch.equal(perm[:R], o_perm) and torch.equal(len_s[:R], o_len), tag
                if with_seg:
                    assert torch.equal(seg[:steps], o_seg), tag


def test_optional_outputs_may_be_null():
    R, max_len = 384, 15
    lengths = lengths_of('random', R, max_len, np.random.RandomState(5))
    len_d = torch.from_numpy(lengths).to(DEV)
    want_perm, want_len, want_seg = reference(lengths, max_len, 15)
    perm = poisoned(R)
    assert K_.leaf_rc('ptv_rows_plan', len_d, R, max_len, 15, perm, None, None) == 0
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    perm, seg = poisoned(R), poisoned(15)
    assert K_.leaf_rc('ptv_rows_plan', len_d, R, max_len, 15, perm, None, seg) == 0
    assert np.array_equal(perm.cpu().numpy(), want_perm) and np.array_equal(seg.cpu().numpy(), want_seg)


def test_refusals_leave_the_outputs_untouched():
    R = MAX_R + 128
    len_d = torch.zeros(R, dtype=torch.int32, device=DEV)
    perm, len_s, seg = poisoned(R), poisoned(R), poisoned(64)

    def untouched():
        torch.cuda.synchronize()
        return bool((perm == POISON).all()) and bool((len_s == POISON).all()) and bool((seg == POISON).all())

    assert K_.leaf_rc('ptv_rows_plan', len_d, 100, 15, 15, perm, len_s, seg) == ERR_ARG           # segment counts: whole 128-row blocks
    assert K_.leaf_rc('ptv_rows_plan', len_d, 128, 15, 65, perm, len_s, seg) == ERR_ARG           # at most 64 steps
    assert K_.leaf_rc('ptv_rows_plan', len_d, 128, 15, 0, perm, len_s, seg) == ERR_ARG
    assert K_.leaf_rc('ptv_rows_plan', len_d, 0, 15, 15, perm, len_s, seg) == ERR_ARG
    assert K_.leaf_rc('ptv_rows_plan', len_d, 128, -1, 15, perm, len_s, seg) == ERR_ARG
    assert K_.leaf_rc('ptv_rows_plan', None, 128, 15, 15, perm, len_s, seg) == ERR_ARG
    assert K_.leaf_rc('ptv_rows_plan', len_d, 128, 15, 15, None, len_s, seg) == ERR_ARG
    assert K_.leaf_rc('ptv_rows_plan', len_d, 128, 39, 15, perm, len_s, seg) == ERR_UNSUPPORTED   # lengths up to 38
    assert K_.leaf_rc('ptv_rows_plan', len_d, R, 15, 15, perm, len_s, seg) == ERR_UNSUPPORTED     # above the row limit
    assert untouched()
    assert K_.leaf_rc('ptv_rows_plan', len_d, MAX_R, 15, 15, perm, len_s, seg) == 0               # the limit itself is taken
    torch.cuda.synchronize()
    assert torch.equal(perm[:MAX_R].cpu(), torch.arange(MAX_R, dtype=torch.int32))
    assert bool((len_s[:MAX_R] == 0).all()) and bool((seg[:15] == 0).all())
    assert bool((perm[MAX_R:] == POISON).all()) and bool((len_s[MAX_R:] == POISON).all()) and bool((seg[15:] == POISON).all())
