"""numpy restatement of the sampled decode's noise and decision rules (csrc/philox.hpp) -- oracle side only, never imported by the product.

A decision of the free-running decoder at (global sample g, time step t, note step n) is the first maximal index of
logit + T * gumbel(word), every word one output of Philox4x32-10 (oracle.rng_oracle) with
    key     = (seed lo, seed hi)
    counter = (g lo,  g hi << 16 | t << 11 | n << 7 | kind << 6 | sub,  draw lo,  2^31 | draw hi)
    kind 0 (pitch):    sub = q * 16 + j; word w is column j + 16 * (4 q + w)
    kind 1 (duration): sub = q;          word w is index 4 q + w = 2 d + c (class c of duration bit d)
and gumbel(word) = -log(-log(u)), u = ((word >> 9) + 1/2) * 2^-23: here in float64, rounded once to float32.
"""
import numpy as np

from oracle.rng_oracle import philox4x32_10

NP_, ND_ = 130, 5

# max |g_device - g_ref| over the draws of tests/test_gpu_sampling.py::test_1_noise_equals_the_restatement (B = 20, two (t, n), offsets 0
# and 1000: 2 * 2 * 20 * 140 values), measured on an MI355X on the tree of the commit that introduced the sampled decode (the child of
# d208ca8): 9.537e-07 = 2^-20, i.e. 4 ulp of a value in [2, 4) -- the device takes both logarithms with the fp32 hardware logarithm
# (v_log_f32).  A wider probe (4096 rows, g up to 13.2) gave the same maximum.  NOISE_TOL = 4 * NOISE_DELTA rounded up to one significant
# digit; the factor 4 covers other draws than the ones measured.
NOISE_DELTA = 9.537e-07
NOISE_TOL = 4e-06


def counter(draw, g, t, n, kind, sub):
    """the four counter words of a call before Philox: broadcastable integer arrays -> uint64 [..., 4], every word < 2^32"""
    g, t, n, sub = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) for a in (g, t, n, sub)))
    c1 = ((g >> np.uint64(32)) << np.uint64(16)) | (t << np.uint64(11)) | (n << np.uint64(7)) | np.uint64(kind << 6) | sub
    return np.stack([g & np.uint64(0xFFFFFFFF), c1 & np.uint64(0xFFFFFFFF), np.full(g.shape, draw & 0xFFFFFFFF, dtype=np.uint64),
                     np.full(g.shape, 0x80000000 | (draw >> 32), dtype=np.uint64)], -1)


def words(seed, draw, g, t, n, kind, sub):
    """broadcastable integer arrays -> uint32 [..., 4]"""
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(counter(draw, g, t, n, kind, sub), key)


def uniform_from_word(w):
    """float64, exactly the fp32 value the device forms: in [2^-24, 1 - 2^-24]"""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_from_word(w):
    return (-np.log(-np.log(uniform_from_word(w)))).astype(np.float32)


def pitch_noise(seed, draw, g, t, n):
    """g, t, n broadcastable -> float32 [..., 130]"""
    g, t, n = np.broadcast_arrays(*(np.asarray(a, dtype=np.int64) for a in (g, t, n)))
    q = np.arange(3).reshape(3, 1)
    j = np.arange(16).reshape(1, 16)
    w = words(seed, draw, g[..., None, None], t[..., None, None], n[..., None, None], 0, q * 16 + j)        # [..., 3, 16, 4]
    # column j + 16 * (4 q + w): order the axes (q, w, j) and flatten
    return gumbel_from_word(np.moveaxis(w, -1, -2).reshape(g.shape + (192,))[..., :NP_])


def dur_noise(seed, draw, g, t, n):
    """-> float32 [..., 5, 2]: (class 0, class 1) of every duration bit"""
    g, t, n = np.broadcast_arrays(*(np.asarray(a, dtype=np.int64) for a in (g, t, n)))
    w = words(seed, draw, g[..., None], t[..., None], n[..., None], 1, np.arange(3))                          # [..., 3, 4]
    return gumbel_from_word(w.reshape(g.shape + (12,))[..., :10]).reshape(g.shape + (ND_, 2))


def decode_noise(seed, draw, g):
    """the noise of a whole decode of the samples g [B]: pitch [B, 32, 15, 130], dur [B, 32, 15, 5, 2]"""
    g = np.asarray(g, dtype=np.int64).reshape(-1, 1, 1)
    t = np.arange(32).reshape(1, 32, 1)
    n = np.arange(15).reshape(1, 1, 15)
    return pitch_noise(seed, draw, g, t, n), dur_noise(seed, draw, g, t, n)


def perturbed(logits, noise, T):
    """fp32 as the device: fl(logit + fl(T * g))"""
    return (np.asarray(logits, dtype=np.float32) + (np.float32(T) * np.asarray(noise, dtype=np.float32)).astype(np.float32)).astype(np.float32)


def decide_pitch(logits, noise, T):
    """first maximal index over the 130 classes of logit + T * g"""
    return np.argmax(perturbed(logits, noise, T), axis=-1)


def decide_dur(logits, noise, T):
    """logits / noise [..., 2] -> 1 iff e1 + T g1 > e0 + T g0 (first maximum wins)"""
    x = perturbed(logits, noise, T)
    return (x[..., 1] > x[..., 0]).astype(np.int64)


def top2_gap(logits, noise, T):
    """float64 gap between the two best perturbed values, and the larger |logit| of the two"""
    v = np.asarray(logits, dtype=np.float64) + float(T) * np.asarray(noise, dtype=np.float64)
    idx = np.argsort(v, axis=-1)[..., -2:]
    top = np.take_along_axis(v, idx, -1)
    lg = np.abs(np.take_along_axis(np.asarray(logits, dtype=np.float64), idx, -1)).max(-1)
    return top[..., 1] - top[..., 0], lg


def skippable(logits, noise, T, noise_tol):
    """a decision the device may take either way: its two best perturbed values are closer than T * noise_tol + 4 ulp of the larger logit"""
    gap, lg = top2_gap(logits, noise, T)
    return gap < T * noise_tol + 4 * np.spacing(lg.astype(np.float32)).astype(np.float64)
