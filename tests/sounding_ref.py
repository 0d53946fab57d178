"""numpy restatement of the sounding state of the free-running decode (include/ptvae_hip.h "Sounding state", INTEGRATION.md "Sounding
state"): grid -> rem, mask_eff, force_eff, held, step by step.

Accepted notes of step s of a row: the slots 1..15 in order up to the first pitch 129; a slot whose pitch lies outside 0..127 is skipped;
d = 1 + the five bit columns read most significant first (v & 1 each), cut to min(d, 32 - s).  rem[128] is zero before step 0; after
step s: rem[p] = max(rem[p] - 1, 0), then rem[p] = d - 1 for each accepted (p, d) in slot order.  H = {p: rem[p] > 0} is held going into
step s + 1, h = |H|, held[s + 1] = h, held[0] = 0.  At a selected step: no_restrike clears the bits of H in the base mask row; the pitch
words are count_limits_ref.step's (no room) of the base words with lo = clamp(F - h, 0, 15), hi = clamp(K - h, 0, 15) (15 where K = 0).
An unselected step gets the base row and words.  Plain loops on purpose: no code shared with the kernel."""
import numpy as np

import count_limits_ref as CL


def accepted(step_rows, s):
    """the accepted notes [(pitch, duration)] of one step [16, 6] at time s, in slot order"""
    out = []
    for j in range(1, 16):
        p = int(step_rows[j][0])
        if p == 129:
            break
        if p < 0 or p > 127:
            continue
        d = 0
        for k in range(1, 6):
            d = 2 * d + (int(step_rows[j][k]) & 1)
        out.append((p, min(d + 1, 32 - s)))
    return out


def advance(rem, notes):
    """rem [128] after a step with these accepted notes"""
    new = [max(int(v) - 1, 0) for v in rem]
    for p, d in notes:
        new[p] = d - 1
    return new


def bits_of(pitches):
    w = [0, 0, 0, 0]
    for p in pitches:
        w[p >> 5] |= 1 << (p & 31)
    return [_i32(v) for v in w]


def _i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >= (1 << 31) else v


def rows_of(a, B, width):
    a = np.asarray(a)
    assert a.shape[0] in (1, B) and a.shape[1] == width, a.shape
    return [a[0 if a.shape[0] == 1 else b] for b in range(B)]


def effective_step(base_mask_row, base_words, H, K, F, selected, no_restrike):
    """-> (the 4 mask words as int32 values, the 15 pitch words, H', F') of one (row, step) going in with the held set H"""
    h = len(H)
    Hc = 15 if K == 0 else min(max(K - h, 0), 15)
    Fc = min(max(F - h, 0), 15)
    mask = [int(v) for v in base_mask_row]
    words = [int(v) for v in base_words]
    if selected:
        if no_restrike:
            hb = bits_of(H)
            mask = [_i32((m & 0xffffffff) & ~(b & 0xffffffff)) for m, b in zip(mask, hb)]
        words = CL.step(words, Fc, Hc, False)[0]
    return mask, words, Hc, Fc


def run(xhat, B, no_restrike=False, K=None, F=None, steps=None, mask_base=None, force_base=None, upto=31):
    """the whole walk over a grid int [B, 32, 16, 6] -> dict(rem uint8 [B, 128] after step `upto` - 1 was decided (what the launch
    t_done = upto - 1 leaves), mask_eff int32 [B, 32, 4], force_eff int32 [15, 32 B], held int32 [B, 32], Hc / Fc int [B, 32]); steps
    above `upto` are left as the base (mask / force) and 0 (held).  K, F, steps: [rows, 32]; None = 0, 0, all selected"""
    xhat = np.asarray(xhat)
    K = np.zeros((1, 32), np.uint8) if K is None else K
    F = np.zeros((1, 32), np.uint8) if F is None else F
    steps = np.ones((1, 32), np.uint8) if steps is None else steps
    Kr, Fr, Sr = rows_of(K, B, 32), rows_of(F, B, 32), rows_of(steps, B, 32)
    mb = np.full((1, 32, 4), -1, np.int32) if mask_base is None else np.asarray(mask_base)
    assert mb.shape[0] in (1, B)
    fb = np.full((15, 32 * B), -1, np.int32) if force_base is None else np.asarray(force_base)
    mask_eff = np.zeros((B, 32, 4), np.int32)
    force_eff = np.array(fb, dtype=np.int32, copy=True)
    held = np.zeros((B, 32), np.int32)
    Hc, Fc = np.full((B, 32), -1), np.full((B, 32), -1)
    rem_out = np.zeros((B, 128), np.uint8)
    for b in range(B):
        rem = [0] * 128
        mrow = mb[0 if mb.shape[0] == 1 else b]
        for s in range(32):
            mask_eff[b, s] = mrow[s]
        for s in range(0, upto + 1):
            if s > 0:
                rem = advance(rem, accepted(xhat[b, s - 1], s - 1))
            H = [p for p in range(128) if rem[p] > 0]
            m, w, hc, fc = effective_step(mrow[s], [fb[n, s * B + b] for n in range(15)], H, int(Kr[b][s]), int(Fr[b][s]),
                                          bool(Sr[b][s]), no_restrike)
            mask_eff[b, s] = m
            for n in range(15):
                force_eff[n, s * B + b] = w[n]
            held[b, s] = len(H)
            Hc[b, s], Fc[b, s] = hc, fc
        rem_out[b] = rem
    return dict(rem=rem_out, mask_eff=mask_eff, force_eff=force_eff, held=held, Hc=Hc, Fc=Fc)


def random_grids(B, seed):
    """grids int64 [B, 32, 16, 6] in the model's layout with everything the parse has a rule for: <sos> (128) in note slots, a pitch twice
    in one step, durations that overhang the segment, rests, 15-note steps without <eos>, pad pitches and pad bits (2) in note slots"""
    rng = np.random.default_rng(seed)
    x = np.full((B, 32, 16, 6), 2, dtype=np.int64)
    x[:, :, :, 0] = 130
    x[:, :, 0, 0] = 128
    for b in range(B):
        for s in range(32):
            kind = rng.integers(0, 8)
            n = 0 if kind == 0 else (15 if kind == 1 else int(rng.integers(1, 7)))
            for j in range(1, n + 1):
                x[b, s, j, 0] = rng.integers(30, 50) if kind != 2 else rng.integers(40, 44)     # kind 2: a narrow range, pitches repeat
                x[b, s, j, 1:] = rng.integers(0, 2, 5)
                if rng.random() < 0.15:
                    x[b, s, j, 1:] = 1                                                           # duration 32: overhangs wherever it starts
                if rng.random() < 0.08:
                    x[b, s, j, 0] = 128                                                          # <sos> in a note slot: skipped
                if rng.random() < 0.04:
                    x[b, s, j, 0] = 130                                                          # <pad> before the <eos>: skipped
                if rng.random() < 0.04:
                    x[b, s, j, 3] = 2                                                            # a pad bit: v & 1 = 0
            if n < 15:
                x[b, s, n + 1, 0] = 129
                if n < 14 and rng.random() < 0.3:                                                # notes behind the <eos> are not read
                    x[b, s, n + 2, 0] = rng.integers(0, 128)
                    x[b, s, n + 2, 1:] = 1
    x[0, 0, 1] = (0, 1, 1, 1, 1, 1)
    x[0, 0, 2] = (127, 0, 0, 0, 0, 0)
    x[0, 0, 3] = (0, 0, 0, 0, 1, 0)                                                              # pitch 0 again: the later slot wins
    x[0, 0, 4, 0] = 129
    return x
