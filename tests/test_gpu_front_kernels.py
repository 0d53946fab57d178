"""The kernels that feed and surround the large kernel families, one at a time against the plain references of tests/front_ref.py:
the texture front end of csrc/texture.hip, the index-grid note embedding and the layout kernels of csrc/elementwise.hip, the
free-running tokens and ptv_route_slices of csrc/misc.hip and ptv_slerp_path of csrc/data.hip -- at the shapes where each entry point
changes path (16-byte / word rows, float4 / scalar features, compile-time / run-time grid geometry, ordered / atomic reduction) and one
size per kernel above its block cap so that the grid-stride loop takes a second trip.

Every case builds its inputs on the CPU from a seeded generator (front_ref's case builders) and gives the same values to the kernel
and, widened, to the reference.  Every output buffer is filled with a sentinel first, and what the header leaves unwritten must still
hold it.  Integer outputs, pure data movement and the exact-integer texture regime are compared bit for bit.  Floating-point outputs
have no pre-chosen tolerance: the same formula is evaluated in fp32 on the CPU, that evaluation's error against the fp64 reference is
measured, and the kernel's error may be at most 4x that, with a floor of 8 fp32 ulps of the case's scale, the sum of the magnitudes of
an output element's terms (check() below).  The bound never sees the kernel's output.  Each check prints `FRONT_RATIO family
kernel-error/bound` (pytest -s shows them; profiles/LOG.md has the table).

Texture, float regime: a pooled position is undecided when fp32 arithmetic need not reproduce its pooling decision
(front_ref.txt_undecided: a candidate within 64 * 2^-24 * (|b| + sum |w| |x|) of the winner that is not a window with the winner's
inputs -- every such candidate, not only the runner-up).  There dpooled is 0 and `arg` is not compared; tests/test_front_ref_host.py
shows that these are at most 0.1 % of the positions.  Slerp: the angle ranges of front_ref.SLERP_ANGLES, the near-parallel pairs
included, passed the conditioning check of the host module as they stand; the paths are compared relative to their interpolated
length."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import front_ref as R
import kernel_ops as K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F4 = np.float32
SENT = np.float32(777.0)
ERR_ARG = -1
MODE0 = 0 if os.environ.get('PTV_WGRAD_ORDERED', '')[:1] == '0' else 1
RATIOS = {}


def lib():
    from polyphonic_chord_texture_disentanglement_amd._lib import lib as _l
    return _l()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def filled(n, value=SENT, dtype=torch.float32):
    return torch.full((int(n),), value, dtype=dtype, device=DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(family, got, ref, f32, scale):
    """|got - ref| <= max(4 * max|f32 - ref|, 8 ulp_fp32(scale)); scale: a scalar, or one figure per output element"""
    got, ref, f32 = (np.asarray(a, np.float64) for a in (got, ref, f32))
    assert got.shape == ref.shape == f32.shape, (got.shape, ref.shape, f32.shape)
    assert np.isfinite(ref).all() and np.isfinite(f32).all() and got.size
    bound, err32 = R.check_bound(ref, f32, scale)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = float(np.where(err == 0, 0.0, err / bound).max())
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print('FRONT_RATIO %s %.3f (kernel err %.3e, fp32 err %.3e)' % (family, ratio, np.nanmax(err), err32))
    assert (err <= bound).all(), '%s: kernel error %.3e over the bound %.3e (fp32 evaluation: %.3e)' % (
        family, np.nanmax(err), float(np.min(bound)), err32)


@pytest.fixture(scope='module', autouse=True)
def no_ordered_fallback_and_ratio_table():
    fb = lib().ptv_ordered_fallbacks(0)
    yield
    assert lib().ptv_ordered_fallbacks(0) == fb                       # every ordered reduction of this module had its workspace
    for k in sorted(RATIOS):
        print('FRONT_RATIO_MAX %s %.3f' % (k, RATIOS[k]))


# ================================================================================================ texture conv + ReLU + pool
def txt_f32(c, d, C):
    """torch's own conv2d / relu / max_pool2d and autograd in fp32 -> pooled [B,C,8,29], dw0 + dW, db0 + dbias"""
    w = torch.from_numpy(c['w']).reshape(C, 1, 4, 12).requires_grad_()
    b = torch.from_numpy(c['bias']).clone().requires_grad_()
    out = TF.max_pool2d(torch.relu(TF.conv2d(torch.from_numpy(c['pr']).unsqueeze(1), w, b, stride=(4, 1))), (1, 4))
    (out * torch.from_numpy(d)).sum().backward()
    return out.detach().numpy(), c['dw0'] + w.grad.reshape(C, 48).numpy(), c['db0'] + b.grad.numpy()


def txt_bwd_call(prd, wd, bd, dfeat, ld, c, B, C, arg, ordered):
    dw, db = dev(np.append(c['dw0'].reshape(-1), SENT)), dev(np.append(c['db0'], SENT))
    try:
        assert lib().ptv_ordered_reductions(ordered) == 0
        K.leaf('ptv_txt_conv_relu_pool_bwd_rows', prd, wd, bd, dfeat, ld, dw, db, B, C, arg)
        torch.cuda.synchronize()
    finally:
        assert lib().ptv_ordered_reductions(MODE0) == 0
    dw, db = host(dw), host(db)
    assert dw[-1] == SENT and db[-1] == SENT
    return dw[:-1].reshape(C, 48), db[:-1]


def run_txt(kind, B, C, ld):
    c = R.texture_case(kind, B, C)
    Wd, rows = C * 29, B * 8
    pooled, arg = R.txt_fwd(c['pr'], c['w'], c['bias'])
    und = R.txt_undecided(c['pr'], c['w'], c['bias']) if kind == 'float' else np.zeros(arg.shape, bool)
    assert und.mean() <= 1e-3
    d = np.where(und, F4(0), c['d'])
    feat_ref, arg_ref, decided = R.txt_feat_rows(pooled), R.txt_arg_rows(arg), ~R.txt_arg_rows(und)
    pool32, dw32, db32 = txt_f32(c, d, C)
    prd, wd, bd = dev(c['pr']), dev(c['w']), dev(c['bias'])
    # ---- forward
    feat, argd = filled((rows + 1) * ld), filled(rows * Wd + 16, 77, torch.int8)
    K.leaf('ptv_txt_conv_relu_pool_fwd_rows', prd, wd, bd, feat, ld, B, C, argd)
    out, am = host(feat).reshape(rows + 1, ld), host(argd)
    assert (out[rows] == SENT).all() and (am[rows * Wd:] == 77).all()
    assert same_bits(out[:rows, Wd:], np.zeros((rows, ld - Wd), F4))                 # the row padding reads zero
    got_arg = am[:rows * Wd].reshape(rows, Wd).astype(np.int64)
    assert np.array_equal(got_arg[decided], arg_ref[decided])
    if kind == 'int':
        assert same_bits(out[:rows, :Wd], feat_ref.astype(F4))
        assert (arg_ref == -1).mean() > 0.01 and (arg_ref == 0).mean() > 0.01
    else:
        check('txt fwd', out[:rows, :Wd], feat_ref, R.txt_feat_rows(pool32),
              R.txt_feat_rows(R.txt_conv(c['pr'], c['w'], c['bias'], absolute=True).max(-1)))
    feat2 = filled((rows + 1) * ld)
    K.leaf('ptv_txt_conv_relu_pool_fwd_rows', prd, wd, bd, feat2, ld, B, C, None)      # no arg-max map wanted
    assert same_bits(host(feat2), host(feat))
    # ---- backward: recomputed convolution / the forward's map, ordered (twice) / atomic
    dfeat = np.full((rows, ld), SENT, F4)                                             # (the padding of dfeat is not read)
    dfeat[:, :Wd] = d.reshape(rows, Wd)
    dfeat = dev(dfeat)
    dw_ref, db_ref = R.txt_bwd(c['pr'], arg, d)
    dw_ref, db_ref = dw_ref + c['dw0'], db_ref + c['db0']
    adw, adb = R.txt_bwd(c['pr'], arg, d, absolute=True)
    adw, adb = adw + np.abs(c['dw0']), adb + np.abs(c['db0'])
    res = {}
    for ordered in (1, 0):
        for mode in ('recompute', 'argmap'):
            a = (prd, wd, bd, dfeat, ld, c, B, C, None) if mode == 'recompute' else (prd, None, None, dfeat, ld, c, B, C, argd)
            res[ordered, mode] = txt_bwd_call(*a, ordered)
            if ordered:
                again = txt_bwd_call(*a, ordered)
                assert same_bits(again[0], res[ordered, mode][0]) and same_bits(again[1], res[ordered, mode][1])
    assert same_bits(res[1, 'recompute'][0], res[1, 'argmap'][0]) and same_bits(res[1, 'recompute'][1], res[1, 'argmap'][1])
    for (ordered, mode), (dw, db) in res.items():
        if kind == 'int':                                                             # integer sums are exact in any order
            assert same_bits(dw, dw_ref.astype(F4)) and same_bits(db, db_ref.astype(F4)), (ordered, mode)
        else:
            fam = 'txt bwd ' + ('ordered' if ordered else 'atomic')
            check(fam, dw, dw_ref, dw32, adw)
            check(fam, db, db_ref, db32, adb)


@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('B,C', R.TXT_SHAPES)
@pytest.mark.parametrize('kind', ['int', 'float'])
def test_texture_front_end(kind, B, C, pad):
    """(5, 16): 464 outputs for the forward's 320 threads; (129, 10): 258 > 256 ordered backward blocks; (257, 10): 2056 > 2048
    forward blocks and 514 > 512 atomic backward blocks.  pad: ld = C * 29 rounded up to 8 (C = 16: 464 + 8)"""
    ld = C * 29 if not pad else (C * 29 + 7) // 8 * 8
    if pad and ld == C * 29:
        ld += 8
    run_txt(kind, B, C, ld)


def test_texture_plain_entry_points_equal_the_rows_form():
    B, C = 3, 10
    c = R.texture_case('float', B, C)
    n = B * C * 8 * 29
    prd, wd, bd, dd = dev(c['pr']), dev(c['w']), dev(c['bias']), dev(c['d'])
    a, b = filled(n + 1), filled(n + 1)
    K.leaf('ptv_txt_conv_relu_pool_fwd', prd, wd, bd, a, B, C)
    K.leaf('ptv_txt_conv_relu_pool_fwd_rows', prd, wd, bd, b, C * 29, B, C, None)
    assert same_bits(host(a), host(b)) and host(a)[n] == SENT
    pooled, _ = R.txt_fwd(c['pr'], c['w'], c['bias'])
    assert np.abs(host(a)[:n] - pooled.reshape(-1)).max() < 1e-4                        # (the rows form is checked above: the same layout)
    res = []
    for name, extra in (('ptv_txt_conv_relu_pool_bwd', ()), ('ptv_txt_conv_relu_pool_bwd_rows', (C * 29,))):
        dw, db = dev(np.append(c['dw0'].reshape(-1), SENT)), dev(np.append(c['db0'], SENT))
        tail = (B, C) if not extra else (B, C, None)
        K.leaf(name, prd, wd, bd, dd, *extra, dw, db, *tail)
        res.append((host(dw), host(db)))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]) and res[0][0][-1] == SENT
    assert not same_bits(res[0][0][:-1], c['dw0'].reshape(-1))


def test_texture_refusals_leave_the_outputs_alone():
    B = 2
    c = R.texture_case('float', B, 16)
    prd, bd, w17 = dev(c['pr']), dev(np.zeros(17, F4)), dev(np.zeros((17, 48), F4))
    wd, b16 = dev(c['w']), dev(c['bias'])
    feat, argd = filled(B * 8 * 17 * 29), filled(B * 8 * 17 * 29, 77, torch.int8)
    dw, db = filled(17 * 48), filled(17)
    dfeat = dev(np.zeros(B * 8 * 17 * 29, F4))
    assert K.leaf_rc('ptv_txt_conv_relu_pool_fwd_rows', prd, w17, bd, feat, 17 * 29, B, 17, argd) == ERR_ARG
    assert K.leaf_rc('ptv_txt_conv_relu_pool_fwd', prd, w17, bd, feat, B, 17) == ERR_ARG
    assert K.leaf_rc('ptv_txt_conv_relu_pool_fwd_rows', prd, wd, b16, feat, 16 * 29 - 1, B, 16, argd) == ERR_ARG
    assert K.leaf_rc('ptv_txt_conv_relu_pool_bwd_rows', prd, w17, bd, dfeat, 17 * 29, dw, db, B, 17, None) == ERR_ARG
    assert K.leaf_rc('ptv_txt_conv_relu_pool_bwd_rows', prd, wd, b16, dfeat, 16 * 29 - 1, dw, db, B, 16, None) == ERR_ARG
    assert K.leaf_rc('ptv_txt_conv_relu_pool_bwd_rows', prd, None, None, dfeat, 16 * 29, dw, db, B, 16, None) == ERR_ARG
    assert K.leaf_rc('ptv_txt_conv_relu_pool_bwd_rows', prd, wd, None, dfeat, 16 * 29, dw, db, B, 16, None) == ERR_ARG
    torch.cuda.synchronize()
    assert (host(feat) == SENT).all() and (host(argd) == 77).all() and (host(dw) == SENT).all() and (host(db) == SENT).all()


# ================================================================================================ index-grid note embedding
def embed_call(default, geom, *args):
    S, N, P, D, pad = geom
    return ('ptv_embed_fwd',) + args if default else ('ptv_embed_fwd_geom',) + args + (S, N, P, D, pad)


def run_embed(E, B, geom, default):
    S, N, P, D, pad = geom
    notes = B * S * N
    x = R.grid_case(100 * E + B, B, geom)
    rng = np.random.RandomState(E + B)
    W, bias = rng.normal(0, 1, (E, P + D)).astype(F4), rng.normal(0, 1, E).astype(F4)
    xd, Wd, bd = dev(x), dev(W), dev(bias)
    emb, lens = filled(notes * E + 8), filled(S * B + 1, -7, torch.int32)
    K.leaf(*embed_call(default, geom, xd, Wd, bd, emb, lens, B, E))
    ref, scale = R.embed(x, W, bias, P)
    f32, _ = R.embed(x, W, bias, P, dtype=F4)
    assert f32.dtype == F4
    got = host(emb)
    assert (got[notes * E:] == SENT).all()
    path = 'float4' if E % 4 == 0 else 'scalar'
    check('embed %s %s' % (path, 'default' if default else 'geom'), got[:notes * E].reshape(N, S, B, E), ref, f32, scale)
    ref_len = R.grid_lengths(x, pad)
    assert np.array_equal(host(lens)[:-1].reshape(S, B), ref_len) and host(lens)[-1] == -7
    emb2 = filled(notes * E + 8)
    K.leaf(*embed_call(default, geom, xd, Wd, bd, emb2, None, B, E))                   # lengths = NULL is accepted
    assert same_bits(host(emb2), got)
    lens2 = filled(S * B + 1, -7, torch.int32)
    if default:
        K.leaf('ptv_grid_lengths', xd, lens2, B)
    else:
        K.leaf('ptv_grid_lengths_geom', xd, lens2, B, S, N, D, pad)
    assert same_bits(host(lens2), host(lens))


@pytest.mark.parametrize('E,B', [(128, 1), (128, 5), (128, 9), (128, 33), (256, 1), (256, 5), (4, 5), (4, 9), (10, 1), (10, 5), (10, 9), (10, 26)])
def test_embed_fwd_default_geometry(E, B):
    """E = 128 / 256 / 4: 8 / 4 / 256 notes a block on the float4 path, E = 10 the scalar path (25 notes a block); B = 9: 288 > 256
    (step, sample) pairs for the lengths; B = 33, E = 128: 16896 > 512 x 8 x 4 notes, the clamped loads of the four-note trip; B = 26,
    E = 10: 13312 > 512 x 25 notes"""
    run_embed(E, B, R.DEFAULT_GEOM, True)


@pytest.mark.parametrize('E', [128, 10])
@pytest.mark.parametrize('B', [1, 5, 9])
@pytest.mark.parametrize('geom', R.GEOMS + [R.DEFAULT_GEOM])
def test_embed_fwd_run_time_geometry(geom, B, E):
    run_embed(E, B, geom, False)


def test_embed_refusals_leave_the_outputs_alone():
    B = 2
    x = dev(R.grid_case(1, B, R.DEFAULT_GEOM))
    W, bias = dev(np.zeros((300, 135), F4)), dev(np.zeros(300, F4))
    emb, lens = filled(B * 512 * 300), filled(32 * B, -7, torch.int32)
    assert K.leaf_rc('ptv_embed_fwd', x, W, bias, emb, lens, B, 300) == ERR_ARG
    x9 = dev(np.zeros((B, 4, 3, 10), np.int64))
    assert K.leaf_rc('ptv_embed_fwd_geom', x9, W, bias, emb, lens, B, 8, 4, 3, 20, 9, 19) == ERR_ARG
    assert K.leaf_rc('ptv_grid_lengths_geom', x9, lens, B, 4, 3, 9, 19) == ERR_ARG
    assert K.leaf_rc('ptv_multihot_geom', x9, emb, 64, B, 4, 3, 20, 9, 0) == ERR_ARG
    assert K.leaf_rc('ptv_multihot_geom', x, emb, 134, B, 32, 16, 130, 5, 0) == ERR_ARG
    assert K.leaf_rc('ptv_multihot_bf16', x, emb, 135, B) == ERR_ARG
    torch.cuda.synchronize()
    assert (host(emb) == SENT).all() and (host(lens) == -7).all()


def run_multihot(B, geom, ld, bf16, entry):
    S, N, P, D, pad = geom
    rows, C = B * S * N, P + D
    x = R.grid_case(7 * B + ld, B, geom)
    ref = R.multihot(x, P)
    sent = 3.0 if bf16 else SENT
    out = filled(rows * ld + 8, sent, torch.bfloat16 if bf16 else torch.float32)
    if entry == 'geom':
        K.leaf('ptv_multihot_geom', dev(x), out, ld, B, S, N, P, D, int(bf16))
    else:
        K.leaf(entry, dev(x), out, ld, B)
    got = host(out.float())
    assert (got[rows * ld:] == sent).all()
    got = got[:rows * ld].reshape(rows, ld)
    cols = min(ld, (C + 7) // 8 * 8) if bf16 else C                                     # bf16 rows: zero-filled to the 8-column granule
    assert np.array_equal(got[:, :C], ref.astype(F4))
    assert not got[:, C:cols].any() and (got[:, cols:] == sent).all()
    assert {0, 1, 2} <= set(np.unique(ref).tolist()) or D == 0


@pytest.mark.parametrize('B', [1, 5, 65])                                               # 65: 33280 notes > 8192 blocks x 4 rows
def test_multihot_default_geometry(B):
    for ld in (135, 136):
        run_multihot(B, R.DEFAULT_GEOM, ld, False, 'ptv_multihot')
    for ld in (136, 144):
        run_multihot(B, R.DEFAULT_GEOM, ld, True, 'ptv_multihot_bf16')
    run_multihot(B, R.DEFAULT_GEOM, 136, False, 'geom')
    run_multihot(B, R.DEFAULT_GEOM, 144, True, 'geom')


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('geom', R.GEOMS)
def test_multihot_run_time_geometry(geom, B):
    C = geom[2] + geom[3]
    for ld in (C, C + 1, 136):
        run_multihot(B, geom, ld, False, 'geom')
    for ld in sorted({C, (C + 7) // 8 * 8, (C + 7) // 8 * 8 + 8}):                      # C = 38: the whole row and nothing beyond it
        run_multihot(B, geom, ld, True, 'geom')


# ================================================================================================ layout and routing (all exact)
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('alpha', [1.0, -0.5, 0.3])
@pytest.mark.parametrize('rows,cols,ldd,lds', [(7, 5, 9, 6), (7, 5, 5, 0), (1, 1, 1, 1), (4125, 256, 260, 256), (4125, 256, 256, 0)])
def test_copy2d(rows, cols, ldd, lds, alpha, accumulate):
    """lds = 0: one source row for all; 4125 x 256 = 1 056 000 elements > 4096 blocks x 256.  alpha = 0.3: the product is rounded
    before the sum (the library is built without floating-point contraction); with 1 and -0.5 it is exact either way"""
    alpha = float(F4(alpha))
    rng = np.random.RandomState(rows + cols + ldd)
    src = rng.normal(0, 1, (rows if lds else 1, max(lds, cols))).astype(F4)
    base = rng.normal(0, 1, (rows, cols)).astype(F4)
    buf = np.full((rows + 1, ldd), SENT, F4)
    buf[:rows, :cols] = base
    dst = dev(buf)
    K.leaf('ptv_copy2d', dst, ldd, dev(src), lds, rows, cols, alpha, accumulate)
    got = host(dst)
    want = R.copy2d(base, src[:, :cols] if lds else src[0, :cols], alpha, accumulate)
    assert want.dtype == F4 and same_bits(got[:rows, :cols], want)
    assert (got[:rows, cols:] == SENT).all() and (got[rows] == SENT).all()


def test_copy2d_of_no_rows_is_ok():
    dst, src = filled(8), filled(8, 1.0)
    assert K.leaf_rc('ptv_copy2d', dst, 4, src, 4, 0, 4, 1.0, 0) == 0 and K.leaf_rc('ptv_copy2d', dst, 4, src, 4, 2, 0, 1.0, 0) == 0
    assert K.leaf_rc('ptv_copy2d', dst, 4, src, 4, -1, 4, 1.0, 0) == ERR_ARG
    torch.cuda.synchronize()
    assert (host(dst) == SENT).all()


@pytest.mark.parametrize('shape', [(3, 5, 7), (1, 9, 1), (135, 128, 1), (32, 64, 128), (64, 130, 128)])   # the last: 1 064 960 > 4096 x 256
def test_transpose01(shape):
    n = int(np.prod(shape))
    a = np.arange(n, dtype=np.int32).view(F4).reshape(shape)                            # every element a different bit pattern
    dst = filled(n + 1)
    K.leaf('ptv_transpose01', dst, dev(a), *shape)
    got = host(dst)
    assert same_bits(got[:n].reshape(shape[1], shape[0], shape[2]), R.transpose01(a)) and got[n] == SENT


ROWS_CASES = [(37, 4, 3, 8, 12, 0, 'vec'), (37, 128, 3, 4, 0, 0, 'vec'), (37, 6, 3, 3, 5, 0, 'word'), (37, 4, 3, 8, 12, 1, 'word'),
              (37, 4, 3, 2, 4, 0, 'word'), (300, 128, 1, 0, 0, 0, 'vec'), (16400, 128, 4, 0, 4, 0, 'vec')]


@pytest.mark.parametrize('rows,w,planes,gap_s,gap_d,off,path', ROWS_CASES)
def test_gather_and_scatter_rows(rows, w, planes, gap_s, gap_d, off, path):
    """rows of 4 / 128 words as 16-byte pieces, of 6 words / from a base pointer one word off / with a plane stride off the 16-byte
    grid word by word; 16400 x 128 x 4 planes = 2 099 200 pieces > 8192 blocks x 256"""
    sps, dps = rows * w + gap_s, rows * w + gap_d
    assert ((w % 4 == 0) and sps % 4 == 0 and dps % 4 == 0 and off == 0) == (path == 'vec')
    rng = np.random.RandomState(rows + w)
    idx = rng.permutation(rows).astype(np.int32)
    data = np.arange(planes * rows * w, dtype=np.int32).reshape(planes, rows, w) * 7 + 1
    idxd = dev(idx)

    def plane_buffer(stride, body=None):
        buf = np.full(off + planes * stride + 4, -7, np.int32)
        if body is not None:
            for p in range(planes):
                buf[off + p * stride: off + p * stride + rows * w] = body[p].reshape(-1)
        return dev(buf)

    def body_of(t, stride):
        a = host(t)
        body = np.stack([a[off + p * stride: off + p * stride + rows * w].reshape(rows, w) for p in range(planes)])
        mask = np.ones(a.size, bool)
        for p in range(planes):
            mask[off + p * stride: off + p * stride + rows * w] = False
        assert (a[mask] == -7).all()                                                   # the gaps between planes and both ends
        return body

    src = plane_buffer(sps, data)
    g = plane_buffer(dps)
    K.leaf('ptv_gather_rows', g[off:], src[off:], idxd, rows, w, sps, dps, planes)
    gathered = body_of(g, dps)
    assert same_bits(gathered, R.gather_rows(data, idx))
    back = plane_buffer(sps)
    K.leaf('ptv_scatter_rows', back[off:], g[off:], idxd, rows, w, dps, sps, planes)     # scatter of gather: the identity
    assert same_bits(body_of(back, sps), data)
    s = plane_buffer(dps)
    K.leaf('ptv_scatter_rows', s[off:], src[off:], idxd, rows, w, sps, dps, planes)
    assert same_bits(body_of(s, dps), R.scatter_rows(data, idx))


def test_gather_and_scatter_of_no_rows_are_ok():
    dst, src, idx = filled(8, -7, torch.int32), filled(8, 1, torch.int32), filled(4, 0, torch.int32)
    for name in ('ptv_gather_rows', 'ptv_scatter_rows'):
        assert K.leaf_rc(name, dst, src, idx, 0, 4, 8, 8, 1) == 0
        assert K.leaf_rc(name, dst, src, idx, 1, 0, 8, 8, 1) == ERR_ARG
    torch.cuda.synchronize()
    assert (host(dst) == -7).all()


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('with_b', [True, False])
@pytest.mark.parametrize('n,nslices', [(5, 7), (1, 1), (2200, 480)])                    # the last: 1 056 000 > 4096 x 256
def test_route_slices(n, nslices, with_b, accumulate):
    rng = np.random.RandomState(n + nslices)
    src = rng.normal(0, 1, (nslices, n)).astype(F4)
    mask = (rng.rand(nslices) < 0.5).astype(np.int32) * rng.randint(1, 9, nslices).astype(np.int32)      # any non-zero routes to A
    if nslices > 1:
        mask[0], mask[1] = 0, 3
    a0, b0 = (rng.normal(0, 1, (nslices, n)).astype(F4) if accumulate else np.full((nslices, n), SENT, F4) for _ in range(2))
    da, db = dev(np.append(a0.reshape(-1), SENT)), dev(np.append(b0.reshape(-1), SENT))
    K.leaf('ptv_route_slices', dev(src), da, db if with_b else None, dev(mask), n, nslices, accumulate)
    wa, wb = R.route_slices(src, mask, a0, b0 if with_b else None, accumulate)
    ga, gb = host(da), host(db)
    assert same_bits(ga[:-1].reshape(nslices, n), wa) and ga[-1] == SENT
    assert same_bits(gb[:-1].reshape(nslices, n), wb if with_b else b0) and gb[-1] == SENT
    assert same_bits(ga[:-1].reshape(nslices, n)[mask == 0], a0[mask == 0])             # not routed here: as it was


# ================================================================================================ tokens
TIES = [(0, 64), (63, 64), (1, 129), (128, 129)]


def note_inputs(M, E, seed):
    """row r takes pattern r % 8: 0, 6, 7 plain N(0, 3); 1 .. 4 an exact tie for the maximum at the column pairs of TIES; 5 all equal"""
    rng = np.random.RandomState(seed)
    pitch = rng.normal(0, 3, (M, 130)).astype(F4)
    k = np.arange(M) % 8
    for i, (a, b) in enumerate(TIES, 1):
        pitch[k == i, a] = pitch[k == i, b] = F4(40)
    pitch[k == 5] = F4(-1.25)
    bits = rng.randint(0, 2, (5, M)).astype(np.int32)
    W, bias = rng.normal(0, 1, (E, 135)).astype(F4), rng.normal(0, 1, E).astype(F4)
    plen = np.where(rng.rand(M) < 0.5, 0, rng.randint(1, 15, M)).astype(np.int32)
    force = np.where(rng.rand(M) < 0.5, -1, rng.randint(0, 130, M)).astype(np.int32)
    force[1::5] = 129
    force[:1] = -1 if M > 1 else 129
    return pitch, bits, W, bias, plen, force


@pytest.mark.parametrize('forced', [False, True])
@pytest.mark.parametrize('E,ld_pitch,xstride', [(128, 136, 96), (100, 130, 6)])
@pytest.mark.parametrize('M', [1, 5, 13, 16385])                                        # the last: > 4096 blocks x 4 rows
def test_note_token_argmax(M, E, ld_pitch, xstride, forced):
    pitch, bits, W, bias, plen, force = note_inputs(M, E, M + E)
    dstride, ld_pred = M + 3, E + 4
    pbuf = np.full((M, ld_pitch), SENT, F4)                                             # (larger than every logit: never to be read)
    pbuf[:, :130] = pitch
    dbuf = np.full((5, dstride), -7, np.int32)
    dbuf[:, :M] = bits
    args = (dev(pbuf), ld_pitch, dev(dbuf), dstride, dev(W), dev(bias), E)
    for n, last in ((5, 0), (15, 1), (9, 1)):
        pred, xhat, pl = filled(M * ld_pred + 1), filled(M * xstride + 1, -7, torch.int64), dev(np.append(plen, -7).astype(np.int32))
        K.leaf('ptv_note_token', *args, pred, ld_pred, xhat, xstride, pl, n, last, dev(force) if forced else None, M)
        idx, ref, scale, xref, L = R.note_token(pitch, bits, W, bias, plen, n, last, force if forced else None)
        f32 = R.note_token(pitch, bits, W, bias, plen, n, last, force if forced else None, dtype=F4)[1]
        assert f32.dtype == F4
        if not forced and M >= 5:
            assert idx[1:5].tolist() == [0, 63, 1, 128] and (M < 6 or idx[5] == 0)
        xg = host(xhat)
        assert xg[-1] == -7 and np.array_equal(xg[:-1].reshape(M, xstride)[:, :6], xref) and (xg[:-1].reshape(M, xstride)[:, 6:] == -7).all()
        assert np.array_equal(host(pl)[:-1], L) and host(pl)[-1] == -7
        pg = host(pred)
        assert pg[-1] == SENT and (pg[:-1].reshape(M, ld_pred)[:, E:] == SENT).all()
        check('note token pred', pg[:-1].reshape(M, ld_pred)[:, :E], ref, f32, scale)
        assert last == 0 or (L > 0).all()


@pytest.mark.parametrize('B', [1, 7, 300])
def test_chord_token(B):
    rng = np.random.RandomState(B)
    root, bass, chroma = (rng.normal(0, 1, s).astype(F4) for s in ((B, 12), (B, 12), (B, 24)))
    root[0, [3, 9]] = F4(5)                                                             # ties: the lowest index
    bass[0, :] = F4(0.5)
    chroma[:, 4:6] = F4(0.25)                                                           # an equal pair: 0
    chroma[:, 6], chroma[:, 7] = F4(1), F4(-1)
    chroma[:, 8], chroma[:, 9] = F4(-1), F4(1)
    if B > 1:
        root[1, [0, 11]], bass[1, [10, 11]] = F4(6), F4(6)
    token = filled(B * 36 + 1)
    masks = dev(np.array([-1, 0x5a5a5a5a], np.int32))                                   # garbage: the entry point clears it
    K.leaf('ptv_chord_token', dev(root), dev(chroma), dev(bass), masks, token, B)
    want = R.chord_token(root, chroma, bass)
    got = host(token)
    assert same_bits(got[:-1].reshape(B, 36), want.astype(F4)) and got[-1] == SENT
    assert want[0, 3] == 1 and want[0, 24] == 1 and (B > 1 or want[0, :12].sum() == 1) and want[0, 14:17].tolist() == [0, 0, 1]
    assert B == 1 or ((want[:, 0] == 1).all() and (want[:, 24 + 10] == 1).all() and 1 < want[0, :12].sum() <= min(B, 12))


# ================================================================================================ slerp path
@pytest.mark.parametrize('angles', sorted(R.SLERP_ANGLES))
@pytest.mark.parametrize('B,D,n', R.SLERP_SHAPES)
def test_slerp_path(B, D, n, angles):
    z1, z2 = R.slerp_case(B, D, n, angles)
    out = filled(B * n * D + 1)
    K.leaf('ptv_slerp_path', dev(z1), dev(z2), out, B, D, n)
    got = host(out)
    assert got[-1] == SENT
    ref, length = R.slerp_path(z1, z2, n)
    f32 = R.slerp_f32(z1, z2, n)
    s = length[..., None]
    check('slerp ' + angles, got[:-1].reshape(B, n, D) / s, ref / s, f32 / s, 1.0)      # relative to the interpolated length
