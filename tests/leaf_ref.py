"""Plain fp64 references (numpy, CPU) of the loss, optimiser and reduction kernels, written from the formulas of include/ptvae_hip.h
("reparameterize()", "Losses", "clip_grad_norm_ + Adam") and the kernel comments of csrc/misc.hip -- the oracle side of
tests/test_gpu_leaf_kernels.py, itself guarded by tests/test_leaf_ref_host.py.  Every function widens its inputs to float64 and
returns float64 (integer outputs: int64).  Ignored rows are EXCLUDED, never multiplied by zero: a NaN in one cannot reach a result."""
import numpy as np

F8 = np.float64


def _f8(a):
    return np.asarray(a, dtype=F8)


# ------------------------------------------------------------------------------------------------ cross-entropy
def _log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide='ignore'):
        return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def ce_rows(logits, targets, ignore=-1):
    """(index of the non-ignored rows, their -log softmax(logits)[target])"""
    logits, targets = _f8(logits), np.asarray(targets)
    live = np.nonzero(targets != ignore)[0]
    ls = _log_softmax(logits[live])
    return live, -ls[np.arange(live.size), targets[live]]


def ce_sum(logits, targets, ignore=-1, groups=None):
    """sum of the non-ignored rows' nll; with groups = G: (sums [G], counts [G]) of the rows r with r % G == g"""
    live, nll = ce_rows(logits, targets, ignore)
    if groups is None:
        return nll.sum()
    sums, counts = np.zeros(groups, F8), np.zeros(groups, np.int64)
    for g in range(groups):
        sel = (live % groups) == g
        sums[g], counts[g] = nll[sel].sum(), int(sel.sum())
    return sums, counts


def ce_grad(logits, targets, ignore=-1, gscale=1.0):
    """gscale * (softmax - onehot) on the non-ignored rows, 0 on the others; gscale: a scalar, or [G] per-group scales (row r: r % G)"""
    logits, targets = _f8(logits), np.asarray(targets)
    out = np.zeros(logits.shape, F8)
    live = np.nonzero(targets != ignore)[0]
    sm = np.exp(_log_softmax(logits[live]))
    sm[np.arange(live.size), targets[live]] -= 1.0
    gs = _f8(gscale)
    out[live] = sm * (gs[live % gs.size][:, None] if gs.ndim else gs)
    return out


# ------------------------------------------------------------------------------------------------ KL / reparameterisation
def kl_terms(mu, sd):
    mu, sd = _f8(mu), _f8(sd)
    return -np.log(sd) + (sd * sd + mu * mu) * 0.5 - 0.5


def kl_sum(mu, sd):
    return kl_terms(mu, sd).sum()


def kl_grad(mu, sd, gscale=1.0):
    mu, sd = _f8(mu), _f8(sd)
    return gscale * mu, gscale * (sd - 1.0 / sd)


def reparam_fwd(mu, sd, eps=None):
    """z = mu + sd * eps (eps None: z = mu), kl sum"""
    mu, sd = _f8(mu), _f8(sd)
    return (mu if eps is None else mu + sd * _f8(eps)), kl_sum(mu, sd)


def reparam_bwd(mu, sd, eps=None, dz=None, dmu_ext=None, dsd_ext=None, klw=0.0, mul_sd=1):
    """dmu = dz + klw mu + dmu_ext; dsd = dz eps + klw (sd - 1/sd) + dsd_ext; second result dsd * sd (mul_sd) or dsd itself"""
    mu, sd = _f8(mu), _f8(sd)
    z0 = np.zeros_like(mu)
    g = z0 if dz is None else _f8(dz)
    dmu = g + klw * mu + (z0 if dmu_ext is None else _f8(dmu_ext))
    dsd = g * (z0 if eps is None else _f8(eps)) + klw * (sd - 1.0 / sd) + (z0 if dsd_ext is None else _f8(dsd_ext))
    return dmu, (dsd * sd if mul_sd else dsd)


# ------------------------------------------------------------------------------------------------ finalisation
def loss_finalize(sums, counts, beta, w0, w1, n_kl, n_root, n_chroma):
    """7 sums + 2 counts -> loss, recon, pl, dl, kl, kl_chd, kl_rhy, chord, root, chroma, bass (a count of 0: the 0/0 of a mean over nothing)"""
    s, c = _f8(sums), _f8(counts)
    with np.errstate(divide='ignore', invalid='ignore'):
        pl, dl = s[0] / c[0], s[1] / c[1]
    klc, klr = s[2] / n_kl, s[3] / n_kl
    root, chroma, bass = s[4] / n_root, s[5] / n_chroma, s[6] / n_root
    recon, kl, chord = w0 * pl + w1 * dl, klc + klr, root + chroma + bass
    return np.array([recon + beta * kl + chord, recon, pl, dl, kl, klc, klr, chord, root, chroma, bass], F8)


def loss_bwd_scales(g, counts, beta, w0, w1, n_kl, n_root, n_chroma):
    """upstream gradients of the 11 scalars -> d(sum over them) / d(each of the 7 sums)"""
    g, c = _f8(g), _f8(counts)
    g_recon, g_kl, g_chord = g[0] + g[1], g[0] * beta + g[4], g[0] + g[7]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.array([(g_recon * w0 + g[2]) / c[0], (g_recon * w1 + g[3]) / c[1], (g_kl + g[5]) / n_kl, (g_kl + g[6]) / n_kl,
                         (g_chord + g[8]) / n_root, (g_chord + g[9]) / n_chroma, (g_chord + g[10]) / n_root], F8)


def wdur_finalize(gsum, gcnt, w):
    """dl = sum_d w[d] * gsum[d] / gcnt[d] -> (sums1, counts1 = 1)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return (_f8(w) * (_f8(gsum) / _f8(gcnt))).sum(), 1


def wdur_scales(gs1, gcnt, w):
    with np.errstate(divide='ignore', invalid='ignore'):
        return F8(gs1) * _f8(w) / _f8(gcnt)


# ------------------------------------------------------------------------------------------------ targets
def pianotree_targets(x, step_major):
    """x [B,32,16,6] int -> pitch_t [rows], dur_t [rows,5] (rows ordered [15][32][B] if step_major else [B][32][15]),
    counts (live pitch targets, live duration targets, last note step 0..14 with any live target -- 0 if none),
    row_live [32,B] = 1 + the last live note step of row (t, b), 0 if none.  Pitch 130 / duration bit 2 = ignored."""
    x = np.asarray(x, np.int64)
    note = x[:, :, 1:, :]                                          # [B,32,15,6]
    if step_major:
        note = note.transpose(2, 1, 0, 3)                          # [15,32,B,6]
    pitch_t, dur_t = note[..., 0].reshape(-1), note[..., 1:].reshape(-1, 5)
    live = (x[:, :, 1:, 0] != 130) | (x[:, :, 1:, 1:] != 2).any(-1)                   # [B,32,15]
    last = np.where(live, np.arange(1, 16)[None, None, :], 0).max(-1)                 # [B,32]
    counts = np.array([(pitch_t != 130).sum(), (dur_t != 2).sum(), max(int(last.max()) - 1, 0)], np.int64)
    return pitch_t, dur_t, counts, last.T.copy()


def chord_targets(c, step_major):
    """c [B,8,36] -> root_t [rows] (first maximum of c[..., :12]), chroma_t [rows,12] (int of c[..., 12:24]), bass_t [rows]
    (c[..., 24:]); rows ordered [8][B] if step_major else [B][8]"""
    c = _f8(c)
    if step_major:
        c = c.transpose(1, 0, 2)
    c = c.reshape(-1, 36)
    return c[:, :12].argmax(-1), c[:, 12:24].astype(np.int64), c[:, 24:].argmax(-1)


# ------------------------------------------------------------------------------------------------ optimiser
def sumsq(g):
    g = _f8(g)
    return (g * g).sum()


def clip_adam(p, g, m, v, sumsq, gscale, clip, lr, b1, b2, eps, step):
    """clip_grad_norm_(., clip) + Adam.step() on flat buffers -> (p, m, v).  The gradient is g * gscale; `sumsq` is of the UNSCALED g
    (so its norm is sqrt(sumsq) * gscale); clip <= 0 disables clipping."""
    p, g, m, v = _f8(p), _f8(g), _f8(m), _f8(v)
    norm = np.sqrt(F8(sumsq)) * gscale
    coef = min(clip / (norm + 1e-6), 1.0) if clip > 0 else 1.0
    gi = g * (coef * gscale)
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - F8(b1) ** step, 1.0 - F8(b2) ** step
    return p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps), m, v


# ------------------------------------------------------------------------------------------------ reductions
def colsum(a, sel=None, groups=1):
    """a [rows, N] -> [groups, N]: row r goes to group sel[r] (0 without sel); rows of any other group are dropped"""
    a = _f8(a)
    sel = np.zeros(a.shape[0], np.int64) if sel is None else np.asarray(sel)
    return np.stack([a[sel == g].sum(0) for g in range(groups)])


def sum_steps(planes, t_top=None):
    """planes [T, n] -> sum over the planes 0 .. min(T - 1, t_top)"""
    planes = _f8(planes)
    T = planes.shape[0] if t_top is None else min(planes.shape[0], t_top + 1)
    return planes[:T].sum(0)


def last_nonzero_unit(x, unit, top=-1, chunk=64):
    """max(top, unit-row block of the LAST ROW of the last `chunk`-row chunk of x [rows, cols] that holds a non-zero): the kernel
    scans whole 64-row chunks.  -0.0 is zero, NaN is not.  (Equals the block of the last non-zero row when unit % chunk == 0.)"""
    x = _f8(x)
    nz = np.nonzero((x != 0).any(axis=1))[0]
    if nz.size == 0:
        return int(top)
    r1 = min(x.shape[0], (int(nz[-1]) // chunk + 1) * chunk)
    return max(int(top), (r1 - 1) // unit)
