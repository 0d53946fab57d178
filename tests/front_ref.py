"""Plain numpy references (CPU; fp64 for floats, int64 for integers) of the kernels that feed and surround the model's large kernel
families: the texture front end (ptv_txt_conv_relu_pool_*), the index-grid note embedding (ptv_embed_fwd*, ptv_grid_lengths*,
ptv_multihot*), the layout and routing kernels (ptv_copy2d, ptv_transpose01, ptv_gather_rows / ptv_scatter_rows, ptv_route_slices),
the free-running tokens (ptv_note_token, ptv_chord_token) and ptv_slerp_path -- written from the formulas of include/ptvae_hip.h and
of the reference model (ptvae.py:72-78, 95-99, 112-114, 292-313, 328-334, 408-425; model.py:216-242), the oracle side of
tests/test_gpu_front_kernels.py, itself guarded by tests/test_front_ref_host.py.

The case builders at the end of each section make the inputs both test modules use: the host module shows on the CPU that they meet
the conditions the GPU module relies on (share of undecided pooling positions, conditioning of the slerp angles)."""
import numpy as np

F8 = np.float64
F4 = np.float32


def _f8(a):
    return np.asarray(a, dtype=F8)


def check_bound(ref, f32, scale):
    """the error a kernel may show against `ref`: max(4 * max|f32 - ref|, 8 ulp_fp32(scale)) with f32 the same formula evaluated in fp32
    on the CPU; scale: a scalar, or one figure per output element.  Returns (bound, max|f32 - ref|)."""
    ref, f32 = _f8(ref), _f8(f32)
    err32 = np.abs(f32 - ref).max() if ref.size else 0.0
    ulp = np.spacing(np.abs(_f8(scale)).astype(F4)).astype(F8)
    return np.maximum(4.0 * err32, 8.0 * ulp), err32


# ------------------------------------------------------------------------------------------------ texture front end
def txt_patches(pr):
    """pr [B,32,128] -> [B,8,29,4,48]: the 4 x 12 input window (tap i * 12 + j) of conv column pp * 4 + q of beat k.  The convolution is
    117 columns wide; MaxPool2d((1,4)) uses the first 116."""
    pr = _f8(pr)
    B = pr.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(pr.reshape(B, 8, 4, 128), 12, axis=3)       # [B,8,4,117,12]
    win = win[:, :, :, :116].reshape(B, 8, 4, 29, 4, 12)                                        # (b, k, i, pp, q, j)
    return np.ascontiguousarray(win.transpose(0, 1, 3, 4, 2, 5)).reshape(B, 8, 29, 4, 48)


def txt_conv(pr, w, bias, absolute=False):
    """v [B,C,8,29,4]: the four conv values of every pooled position (absolute: |b| + sum |w| |x|, the scale of each)"""
    X, w, bias = txt_patches(pr), _f8(w).reshape(-1, 48), _f8(bias)
    if absolute:
        X, w, bias = np.abs(X), np.abs(w), np.abs(bias)
    return (X @ w.T + bias).transpose(0, 4, 1, 2, 3)


def txt_pool(v):
    """first maximum over (0, v0 .. v3), a later value winning only when strictly greater -> pooled [B,C,8,29], arg (-1: nothing > 0)"""
    cand = np.concatenate([np.zeros(v.shape[:-1] + (1,), F8), v], -1)
    return cand.max(-1), cand.argmax(-1).astype(np.int64) - 1


def txt_fwd(pr, w, bias):
    return txt_pool(txt_conv(pr, w, bias))


def txt_feat_rows(pooled):
    """the pooled map as the rows of the reference's raw view (ptvae.py:114): [B,C,8,29] memory read as [B*8, C*29]"""
    B, C = pooled.shape[:2]
    return pooled.reshape(B * 8, C * 29)


def txt_arg_rows(arg):
    """the arg-max map as the entry points hold it: row b * 8 + beat, column ch * 29 + pp"""
    B, C = arg.shape[:2]
    return arg.transpose(0, 2, 1, 3).reshape(B * 8, C * 29)


def txt_bwd(pr, arg, d, absolute=False):
    """dW [C,48] = sum d * x, dbias [C] = sum d over the pooled positions with arg >= 0, x the winning window
    (absolute: sum |d * x| and sum |d|, the scale of each tap)"""
    X, d = txt_patches(pr), _f8(d)
    C = arg.shape[1]
    dw, db = np.zeros((C, 48), F8), np.zeros(C, F8)
    for c in range(C):
        a = arg[:, c]                                                                            # [B,8,29]
        x = np.take_along_axis(X, np.maximum(a, 0)[..., None, None], axis=3)[:, :, :, 0, :]      # [B,8,29,48]
        dm = np.where(a >= 0, d[:, c], 0.0)
        if absolute:
            x, dm = np.abs(x), np.abs(dm)
        dw[c], db[c] = np.tensordot(dm, x, 3), dm.sum()
    return dw, db


def txt_undecided(pr, w, bias, ulps=64.0):
    """[B,C,8,29] bool: positions whose pooling decision fp32 arithmetic need not reproduce -- a candidate of (0, v0 .. v3) other than
    the winner lies within ulps * 2^-24 * (|b| + sum |w| |x|) of it (the largest of the four windows' scales), unless both are windows
    with identical inputs (their values are then equal in any arithmetic and the first wins).  From the fp64 values alone."""
    X = txt_patches(pr)
    v = txt_conv(pr, w, bias)
    thr = ulps * 2.0 ** -24 * txt_conv(pr, w, bias, absolute=True).max(-1)
    cand = np.concatenate([np.zeros(v.shape[:-1] + (1,), F8), v], -1)
    win = cand.argmax(-1)
    close = (cand.max(-1)[..., None] - cand) < thr[..., None]
    np.put_along_axis(close, win[..., None], False, axis=-1)
    eq = (X[:, :, :, :, None, :] == X[:, :, :, None, :, :]).all(-1)                              # [B,8,29,4,4]
    eq = np.broadcast_to(eq[:, None], v.shape + (4,))
    same = np.take_along_axis(eq, np.maximum(win - 1, 0)[..., None, None], axis=-1)[..., 0] & (win >= 1)[..., None]
    same = np.concatenate([np.zeros(same.shape[:-1] + (1,), bool), same], -1)
    return (close & ~same).any(-1)


TXT_SHAPES = [(1, 1), (3, 10), (5, 16), (129, 10), (257, 10)]


def texture_case(kind, B, C):
    """inputs of one texture case, all fp32: pr [B,32,128] a 6 % dense piano roll of 1 .. 8, w [C,48], bias [C], d [B,C,8,29], and what
    dw / dbias hold before the backward.  kind 'int': w in -2 .. 2, bias 1 / 0 / -2 by channel, d in -3 .. 3 -- every sum is exact in
    fp32.  kind 'float': w N(0, 0.15), bias N(0, 0.1), d N(0, 1)."""
    rng = np.random.RandomState(1000 * B + C + (7 if kind == 'int' else 0))
    pr = ((rng.rand(B, 32, 128) < 0.06) * rng.randint(1, 9, (B, 32, 128))).astype(F4)
    if kind == 'int':
        w = rng.randint(-2, 3, (C, 48)).astype(F4)
        bias = np.array([(1, 0, -2)[c % 3] for c in range(C)], F4)
        d = rng.randint(-3, 4, (B, C, 8, 29)).astype(F4)
        dw0, db0 = rng.randint(-5, 6, (C, 48)).astype(F4), rng.randint(1, 6, C).astype(F4)
    else:
        w, bias = rng.normal(0, 0.15, (C, 48)).astype(F4), rng.normal(0, 0.1, C).astype(F4)
        d = rng.normal(0, 1, (B, C, 8, 29)).astype(F4)
        dw0, db0 = rng.normal(0, 1, (C, 48)).astype(F4), rng.normal(0, 1, C).astype(F4)
    return dict(pr=pr, w=w, bias=bias, d=d, dw0=dw0, db0=db0)


# ------------------------------------------------------------------------------------------------ index-grid note embedding
def embed(x, W, bias, P, dtype=F8):
    """x [B,S,N,1+D] int, W [E,P+D], bias [E] -> (emb step-major [N,S,B,E] = bias + W[:, p] [0 <= p < P] + sum_d W[:, P+d] x[..., 1+d],
    the sum of the terms' magnitudes).  The terms are added in this order in `dtype`."""
    x = np.asarray(x, np.int64)
    W, bias = np.asarray(W, dtype), np.asarray(bias, dtype)
    xs = x.transpose(2, 1, 0, 3)                                                                 # [N,S,B,1+D]
    p = xs[..., 0]
    ok = (p >= 0) & (p < P)
    term = np.where(ok[..., None], W.T[np.where(ok, p, 0)], dtype(0))
    v = np.broadcast_to(bias, term.shape) + term
    s = np.abs(bias) + np.abs(term)
    for d in range(x.shape[-1] - 1):
        term = W[:, P + d] * xs[..., 1 + d, None].astype(dtype)
        v, s = v + term, s + np.abs(term)
    return v, s


def grid_lengths(x, pad):
    """lengths [S,B] = N - #{n : pitch == pad}"""
    x = np.asarray(x, np.int64)
    return (x.shape[2] - (x[..., 0] == pad).sum(-1)).T.copy()


def multihot(x, P):
    """rows [N*S*B, P+D] in the (n, s, b) order: one-hot of the pitch over 0 .. P-1 (none for a pitch outside), then the D entries"""
    x = np.asarray(x, np.int64)
    xs = x.transpose(2, 1, 0, 3).reshape(-1, x.shape[-1])
    out = np.zeros((xs.shape[0], P + x.shape[-1] - 1), np.int64)
    out[:, :P] = xs[:, :1] == np.arange(P)[None, :]
    out[:, P:] = xs[:, 1:]
    return out


DEFAULT_GEOM = (32, 16, 130, 5, 130)
GEOMS = [(32, 12, 34, 4, 33), (3, 2, 7, 0, 6), (24, 10, 34, 8, 33)]


def grid_case(seed, B, geom):
    """x [B,S,N,1+D] int64: pitches 0 .. P-1, about a third of the slots <pad>, the four pitches -1, P-1, P, P+1 in the first slots of
    every sample's first step (as far as there are slots); entries 0 .. 2"""
    S, N, P, D, pad = geom
    rng = np.random.RandomState(seed)
    x = np.concatenate([rng.randint(0, P, (B, S, N, 1)), rng.randint(0, 3, (B, S, N, D))], -1).astype(np.int64)
    x[..., 0][rng.rand(B, S, N) < 0.35] = pad
    flat = x[..., 0].reshape(B, S * N)
    flat[:, :4] = [-1, P - 1, P, P + 1]
    x[..., 0] = flat.reshape(B, S, N)
    return x


# ------------------------------------------------------------------------------------------------ layout and routing
def copy2d(dst, src, alpha, accumulate):
    """dst [rows, cols] (+)= alpha * src (src [cols]: one row for all) in fp32, one multiply and one add -- exactly what fp32 gives"""
    v = F4(alpha) * np.broadcast_to(np.asarray(src, F4), dst.shape)
    return (np.asarray(dst, F4) + v) if accumulate else v


def transpose01(a):
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))


def gather_rows(src, idx):
    """src [planes, rows, w] -> dst[pl][p] = src[pl][idx[p]]"""
    return src[:, np.asarray(idx)]


def scatter_rows(src, idx):
    """dst[pl][idx[p]] = src[pl][p]"""
    out = np.empty_like(src)
    out[:, np.asarray(idx)] = src
    return out


def route_slices(src, mask, dst_a, dst_b, accumulate):
    """src [nslices, n]: slice s goes to dst_a (mask != 0) or dst_b (None: nowhere), added in fp32 or stored; the rest stays"""
    a, b = dst_a.copy(), None if dst_b is None else dst_b.copy()
    for s in range(src.shape[0]):
        d = a if mask[s] else b
        if d is not None:
            d[s] = (d[s] + src[s]) if accumulate else src[s]
    return a, b


# ------------------------------------------------------------------------------------------------ free-running tokens
def note_token(pitch, bits, W, bias, plen, n, last, force=None, dtype=F8):
    """pitch [M,130] logits, bits [5,M] -> idx [M] (first maximal index; force[r] >= 0 replaces it), pred [M,E] = bias + W[:, idx] +
    sum_d W[:, 130+d] bit_d with the sum of the terms' magnitudes, xhat [M,6] = (idx, bits), plen: the first <eos> (129) sets n where
    plen == 0, and `last` fills what is still 0 with n"""
    idx = np.asarray(pitch).argmax(1).astype(np.int64)
    if force is not None:
        idx = np.where(np.asarray(force) >= 0, force, idx).astype(np.int64)
    W, bias, bits = np.asarray(W, dtype), np.asarray(bias, dtype), np.asarray(bits, np.int64)
    term = W.T[idx]
    v, s = bias + term, np.abs(bias) + np.abs(term)
    for d in range(5):
        term = W[:, 130 + d] * bits[d][:, None].astype(dtype)
        v, s = v + term, s + np.abs(term)
    L = np.asarray(plen, np.int64).copy()
    L[(L == 0) & (idx == 129)] = n
    if last:
        L[L == 0] = n
    return idx, v, s, np.concatenate([idx[:, None], bits.T], 1), L


def chord_token(root, chroma, bass):
    """root / bass [B,12], chroma [B,12,2] logits -> token [B,36]: the UNION over the batch of the rows' first-maximum one-hots in the
    root and bass parts of every row (ptvae.py:74,77 index a [bs,1,12] tensor with two [bs] index vectors), the row's own chroma bits"""
    B = root.shape[0]
    tok = np.zeros((B, 36), np.int64)
    tok[:, np.asarray(root).argmax(1)] = 1
    tok[:, 24 + np.asarray(bass).argmax(1)] = 1
    tok[:, 12:24] = np.asarray(chroma).reshape(B, 12, 2).argmax(-1)
    return tok


# ------------------------------------------------------------------------------------------------ slerp path
def slerp_path(z1, z2, n):
    """oracle.ptvae_oracle.interp_path (model.py:216-242) per sample -> (out [B,n,D] fp64, the interpolated lengths [B,n])"""
    from oracle.ptvae_oracle import interp_path
    z1, z2 = _f8(z1), _f8(z2)
    out = np.stack([interp_path(a, b, n) for a, b in zip(z1, z2)])
    la, lb = np.log(np.linalg.norm(z1, axis=1)), np.log(np.linalg.norm(z2, axis=1))
    return out, np.exp(la[:, None] + (lb - la)[:, None] * np.linspace(0.0, 1.0, n)[None, :])


def _sum32(a, order):
    """fp32 sum over the last axis: 'pair' numpy's pairwise sum; 'lanes' 64 interleaved partial sums, each sequential, then pairwise"""
    if order == 'pair':
        return a.sum(-1, dtype=F4)
    D = a.shape[-1]
    pad = np.zeros(a.shape[:-1] + ((-D) % 64,), F4)
    chunks = np.concatenate([a, pad], -1).reshape(a.shape[:-1] + (-1, 64))
    acc = np.zeros(a.shape[:-1] + (64,), F4)
    for k in range(chunks.shape[-2]):
        acc = acc + chunks[..., k, :]
    return acc.sum(-1, dtype=F4)


def slerp_f32(z1, z2, n, order='pair'):
    """the interp_path formula evaluated in fp32, the three dot products summed in the given order"""
    a, q = np.asarray(z1, F4), np.asarray(z2, F4)
    na, nq = np.sqrt(_sum32(a * a, order)), np.sqrt(_sum32(q * q, order))
    omega = np.arccos(_sum32(a * q, order) / (na * nq))
    so = np.sin(omega)
    t = (np.arange(n, dtype=F4) / F4(max(n - 1, 1)))[None, :]
    wa, wq = np.sin((F4(1) - t) * omega[:, None]) / so[:, None], np.sin(t * omega[:, None]) / so[:, None]
    la, lq = np.log(na), np.log(nq)
    length = np.exp(la[:, None] + (lq - la)[:, None] * t)
    out = (wa[..., None] * (a / na[:, None])[:, None, :] + wq[..., None] * (q / nq[:, None])[:, None, :]) * length[..., None]
    assert out.dtype == F4
    return out


SLERP_SHAPES = [(B, D, n) for B in (1, 300) for D in (16, 100, 256) for n in (1, 2, 7)]
SLERP_ANGLES = {'wide': (0.05, 2.8), 'near-parallel': (1e-2, 1e-2)}


def slerp_case(B, D, n, angles='wide'):
    """z1, z2 fp32 [B,D]: norms log-uniform in 1e-2 .. 1e2, the angle between a pair prescribed (uniform in the range)"""
    rng = np.random.RandomState(D * 1000 + B + n)
    u, v = rng.normal(0, 1, (B, D)), rng.normal(0, 1, (B, D))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v -= (v * u).sum(1, keepdims=True) * u
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    th = rng.uniform(*SLERP_ANGLES[angles], size=(B, 1))
    n1, n2 = (np.exp(rng.uniform(np.log(1e-2), np.log(1e2), (B, 1))) for _ in range(2))
    return (n1 * u).astype(F4), (n2 * (np.cos(th) * u + np.sin(th) * v)).astype(F4)
