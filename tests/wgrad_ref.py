"""Plain references (numpy, float64 / int64, CPU) of the weight-gradient family -- ptv_wgrad / ptv_wgrad_cat / ptv_wgrad_batch,
csrc/wgrad.hip -- written from the text of include/ptvae_hip.h ("Weight-gradient product", ptv_wgrad_job): the oracle side of
tests/test_gpu_wgrad_kernels.py, itself held to torch's float64 operators and to brute-force loops by tests/test_wgrad_ref_host.py.

    C[m, n] (+)= alpha * sum over the LIVE rows k of A[k, m] * B[k, n]          colsum_a[m] += sum over the live rows k of A[k, m]

A row is live unless a limit (k_top / k_unit / k_rev) or a segment count (seg_n / seg_unit / seg_period) declares it zero.  The dead
rows of A are zero by contract, so for A the restriction changes nothing; B's dead rows "may never have been written", and the tests put
NaN there.

CASES names every branch of the host dispatch (plan_job of csrc/wgrad.hip): the fields of a job and the plan the library must report
for it through ptv_debug_wgrad_plan (include/ptvae_hip_debug.h).  The expectations were worked out by hand from plan_job; the CPU
test holds the library to them, so a GPU case cannot silently leave the branch it is named after.  Leading dimensions and column
offsets are chosen such that the plan is the same for bf16 and fp32 operands (ld a multiple of 8, or 2 mod 4; an offset of one
element is off the 16-byte grid either way)."""
import numpy as np

from gemm_ref import bf16_round, exact_ok, int_case     # noqa: F401  (re-exported: the exact operands of the GPU tests)

F8, F4 = np.float64, np.float32
PLAN_FIELDS = ('kfast', 'tiles_m', 'tiles_n', 'nslab_fast', 'kper_fast', 'map_fast', 'nslab_tail', 'kper_tail', 'map_tail', 'total_slabs')


def live_rows(K, k_top=None, k_unit=0, k_rev=0, seg_n=None, seg_unit=0, seg_period=0):
    """bool [K]: the rows that enter the product.
    k_top: "the rows of A from (*k_top + 1) * k_unit on are zero"; k_rev > 0: "the zero part is then the rows BEFORE
    (k_rev - *k_top - 1) * k_unit".  seg_n: "of unit q only the first seg_n[q % seg_period] rows (seg_period < 0:
    seg_n[|seg_period| - 1 - q % |seg_period|]) hold anything"."""
    r = np.arange(K, dtype=np.int64)
    live = np.ones(K, bool)
    if k_top is not None:
        if k_rev > 0:
            live &= r >= (int(k_rev) - int(k_top) - 1) * int(k_unit)
        else:
            live &= r < (int(k_top) + 1) * int(k_unit)
    if seg_n is not None:
        n = np.asarray(seg_n, np.int64)
        q, P = r // int(seg_unit), abs(int(seg_period))
        idx = q % P if seg_period > 0 else P - 1 - q % P
        live &= (r % int(seg_unit)) < n[idx]
    return live


def product(A, B, live=None, alpha=1.0, C0=None, accumulate=0):
    """A [K, M], B [K, N] as stored (row per sample) -> float64 [M, N]; the dead rows of B are never looked at (they may hold NaN)"""
    A, B = np.asarray(A, F8), np.asarray(B, F8)
    assert A.shape[0] == B.shape[0]
    if live is not None:
        A, B = A[live], B[live]
    v = F8(alpha) * (A.T @ B) if A.shape[0] else np.zeros((A.shape[1], B.shape[1]), F8)
    return v + np.asarray(C0, F8) if accumulate else v


def colsum(A, live=None, b0=None):
    A = np.asarray(A, F8)
    if live is not None:
        A = A[live]
    v = A.sum(axis=0) if A.shape[0] else np.zeros(A.shape[1], F8)
    return v if b0 is None else v + np.asarray(b0, F8)


def abs_product(A, B, live=None):
    """|A|^T |B| over the live rows: the scale of the rounding-error bound of the real-valued tests"""
    return product(np.abs(np.asarray(A, F8)), np.abs(np.nan_to_num(np.asarray(B, F8))), live)


def ceil8(x):
    return -(-x // 8) * 8


def _case(M, N, K, slabs=0, lda=None, ldb=None, offa=0, offb=0, seg=None, reaches=(), **expect):
    """lda / ldb in elements (default: the width rounded up to 8 -- 16-byte aligned rows in both dtypes); offa / offb: the operand is a view
    that starts at this column of its array; seg = (seg_unit, seg_n, seg_period)"""
    e = dict.fromkeys(PLAN_FIELDS, 0)
    e.update(expect)
    assert set(e) == set(PLAN_FIELDS)
    return dict(M=M, N=N, K=K, slabs=slabs, lda=lda or ceil8(M + offa), ldb=ldb or ceil8(N + offb), offa=offa, offb=offb, seg=seg,
                reaches=tuple(reaches), expect=e)


def _p(kfast, tm, tn, fast=None, tail=None):
    f, t = fast or (0, 0, 0), tail or (0, 0, 0)
    return dict(kfast=kfast, tiles_m=tm, tiles_n=tn, nslab_fast=f[0], kper_fast=f[1], map_fast=f[2], nslab_tail=t[0], kper_tail=t[1],
                map_tail=t[2], total_slabs=f[0] + t[0])


# `reaches`: what tests/test_wgrad_ref_host.py's census looks for (each tag is re-derived there from the reported plan, not believed)
CASES = {
    # ---- plain jobs, aligned operands: the unguarded launch alone
    'one_slab':        _case(128, 128, 96, reaches=('fast_only', 'single_slab', 'map0'), **_p(96, 1, 1, (1, 96, 0))),
    'map0_explicit3':  _case(256, 128, 1024, 3, reaches=('map0', 'explicit'), **_p(1024, 2, 1, (3, 352, 0))),
    'map1_explicit8':  _case(128, 128, 1024, 8, reaches=('map1', 'explicit'), **_p(1024, 1, 1, (8, 128, 1))),
    'map1_maxs':       _case(128, 128, 1024, 16, reaches=('map1', 'maxs'), **_p(1024, 1, 1, (8, 128, 1))),
    'map1_beyond_k':   _case(128, 128, 1056, 8, reaches=('map1', 'map1_beyond_k'), **_p(1056, 1, 1, (8, 160, 1))),
    'map2_auto':       _case(256, 512, 1024, reaches=('map2', 'deep'), **_p(1024, 2, 4, (4, 256, 2))),
    'map2_over_map1':  _case(256, 512, 1024, 8, reaches=('map2', 'explicit'), **_p(1024, 2, 4, (8, 128, 2))),
    'map1_deep_k':     _case(256, 512, 16384, reaches=('map1', 'deep'), **_p(16384, 2, 4, (8, 2048, 1))),
    'deep_clamp7':     _case(128, 128, 2016, reaches=('map0', 'deep'), **_p(2016, 1, 1, (7, 288, 0))),
    # ---- widths that are no multiple of 8: the unguarded launch stops short of the last row, a guarded tail takes the rest
    'tail32':          _case(130, 128, 160, reaches=('fast_tail',), **_p(128, 2, 1, (1, 128, 0), (1, 32, 0))),
    'tail22':          _case(130, 128, 150, reaches=('fast_tail',), **_p(128, 2, 1, (1, 128, 0), (1, 32, 0))),
    'tail_multi':      _case(130, 128, 1056, 4, reaches=('fast_tail', 'explicit'), **_p(1024, 2, 1, (4, 256, 0), (1, 32, 0))),
    'tail_only':       _case(130, 128, 32, reaches=('tail_only', 'single_slab'), **_p(0, 2, 1, None, (1, 32, 0))),
    'tail_only_k1':    _case(128, 128, 1, reaches=('tail_only', 'single_slab'), **_p(0, 1, 1, None, (1, 32, 0))),
    'tail_only_k31':   _case(130, 128, 31, reaches=('tail_only', 'single_slab'), **_p(0, 2, 1, None, (1, 32, 0))),
    'narrow_12x36':    _case(12, 36, 288, reaches=('fast_tail',), **_p(256, 1, 1, (1, 256, 0), (1, 32, 0))),
    'narrow_200x135':  _case(200, 135, 288, reaches=('fast_tail',), **_p(256, 2, 2, (1, 256, 0), (1, 32, 0))),
    # ---- rows that are not 16-byte aligned: everything goes through the guarded launch, which then carries the slabs
    'unaligned_auto':  _case(64, 130, 999, lda=70, reaches=('tail_only', 'deep'), **_p(0, 1, 2, None, (3, 352, 0))),
    'unaligned_3':     _case(64, 130, 999, 3, lda=70, reaches=('tail_only', 'explicit'), **_p(0, 1, 2, None, (3, 352, 0))),
    'offgrid_a':       _case(64, 128, 512, offa=1, reaches=('tail_only',), **_p(0, 1, 1, None, (2, 256, 0))),
    'offgrid_b':       _case(128, 64, 512, offb=1, reaches=('tail_only',), **_p(0, 1, 1, None, (2, 256, 0))),
    # ---- K segments (through ptv_wgrad_batch); K spans more than one period so that q % seg_period wraps
    'seg_map0':        _case(128, 128, 512, seg=(128, (96, 32), 2), reaches=('seg_map0',), **_p(512, 1, 1, (4, 128, 0))),
    'seg_map1_9to16':  _case(128, 128, 1152, seg=(128, (128, 96, 32, 0), 4), reaches=('seg_map1', 'seg_map1_padded'),
                             **_p(1152, 1, 1, (16, 128, 1))),
    'seg_map2':        _case(256, 512, 1024, seg=(128, (128, 96, 32, 0), 4), reaches=('seg_map2',), **_p(1024, 2, 4, (8, 128, 2))),
    'seg_unit384':     _case(128, 128, 1536, seg=(384, (160, 32), 2), reaches=('seg_map1', 'seg_map1_padded', 'seg_three_per_unit'),
                             **_p(1536, 1, 1, (16, 128, 1))),
    'seg_tail_live':   _case(130, 128, 512, seg=(128, (128, 96, 32, 128), 4), reaches=('seg_map0', 'seg_tail'),
                             **_p(480, 2, 1, (4, 128, 0), (1, 128, 0))),
    'seg_tail_dead':   _case(130, 128, 512, seg=(128, (128, 96, 32, 96), 4), reaches=('seg_map0', 'seg_tail'),
                             **_p(480, 2, 1, (4, 128, 0), (1, 128, 0))),
}
SEG_CASES = tuple(n for n, c in CASES.items() if c['seg'])
CENSUS = ('map0', 'map1', 'map2', 'seg_map0', 'seg_map1', 'seg_map2', 'fast_only', 'tail_only', 'fast_tail', 'single_slab', 'map1_beyond_k',
          'seg_map1_padded', 'seg_three_per_unit', 'seg_tail', 'maxs', 'deep', 'explicit')


def cdiv(a, b):
    return -(-a // b)


def tags_of(c, plan):
    """the census tags a case really earns, from the plan the library reported for it (a dict over PLAN_FIELDS) and the job's own fields --
    the definitions of the branches in words of the plan, independent of `reaches`"""
    K, kf, seg = c['K'], plan['kfast'], c['seg']
    tiles = plan['tiles_m'] * plan['tiles_n']
    parts = [(k0, kn, plan['nslab_' + w], plan['kper_' + w], plan['map_' + w], want)
             for w, k0, kn, want in (('fast', 0, kf, c['slabs']), ('tail', kf, K - kf, None if kf else c['slabs'])) if kn > 0]
    t = set()
    t.add('fast_only' if kf == K else ('tail_only' if kf == 0 else 'fast_tail'))
    if plan['total_slabs'] == 1:
        t.add('single_slab')
    for k0, kn, ns, kper, mp, want in parts:
        if ns > 1 or len(parts) == 1:
            t.add(('seg_map%d' if seg else 'map%d') % mp)
        if mp == 1 and not seg and (ns - 1) * kper >= kn:
            t.add('map1_beyond_k')
        if mp == 1 and seg and ns % 8 == 0 and ns > cdiv(kn, kper):
            t.add('seg_map1_padded')
        if seg or want is None:                                    # (the tail behind a fast launch is one slab by construction)
            continue
        if want > 0:
            t.add('maxs' if want > ns and ns == max(kn // 128, 1) else 'explicit')
        else:
            shortk = kn <= 8192
            wide = cdiv(256, tiles) if shortk else (768 if tiles >= 32 else 256) // tiles
            deep = (kn // 1024 if kn >= 2048 else kn // 256) if shortk else kn // 2048
            if 1 < deep < wide and ns == (deep // 8 * 8 if deep >= 8 else deep) and ns <= max(kn // 128, 1):
                t.add('deep')
    if seg:
        unit, n, _ = seg
        kper = plan['kper_fast'] or plan['kper_tail']
        per = unit // kper
        if per >= 3 and any(0 < v - kper < kper and v <= unit - kper for v in n):     # one full slab, one clipped, at least one dead
            t.add('seg_three_per_unit')
        if 0 < kf < K:
            t.add('seg_tail')
    return t
