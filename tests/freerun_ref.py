"""Plain fp64 references (numpy, CPU) of the two persistent kernels of csrc/freerun.hip -- ptv_free_note_loop (one time step t, all 15
note steps, B rows) and ptv_free_resummarize (the bi-GRU over the 16 predicted notes, packed by the predicted length) -- written against
the KERNELS' inputs as include/ptvae_hip.h lists them, not against model parameters: the oracle side of
tests/test_gpu_freerun_kernels.py, itself held to oracle/ptvae_oracle.py's decode_notes / _bigru_final (torch float64) by
tests/test_freerun_ref_host.py.  Never imported by the product.

One note step n of note_loop(), from the state h_n, the fed token tok_n and the hoisted input part gc (b_ih included):

    h_{n+1} = GRU(gc + W_ih[:, Ht:] tok_n, h_n)                 r | z | n thirds, hn = W_hn h + b_hn       (gru_ref.gru_forward)
    pitch_n = W_p h_{n+1} + b_p                                  p_n = first maximal index (or the force word when it is >= 0)
    hd_0    = W_dh [h_{n+1} | pitch_n] + b_dh
    hd_{d+1} = GRU_d(token_d, hd_d),  est_d = W_out hd_{d+1} + b_out,  bit_d = [est_d1 > est_d0] (or forced)      (dur_ref._cell)
    PRED_{n+1} = b_emb + w_embT[p_n] + sum_d bit_d w_embT[130 + d]
    tok_{n+1} = emb_{n+1} where bit n of coin_mask is set (teacher forcing), else PRED_{n+1}
    plen = n + 1 at the first p_n = 129 (<eos>), 15 when there is none

The second half (kp_*) evaluates the same formulas in float32 with bf16 rounding at the points where the kernels round.  It is no
reference: its error against the fp64 functions is the yardstick the kernels' error is held to (bound_of of test_gpu_dur_kernels.py).
Every array is in the kernel's layout restricted to the rows of t: an [R]- or [M]-row plane becomes its B rows, [15, B] for an [M] plane."""
import functools

import numpy as np

import dur_ref as D
import gru_ref as G
from gemm_ref import bf16_round, is_bf16

F8, F4 = np.float64, np.float32
HN, HD, E, NP, HE, EOS = 512, 64, 128, 130, 128, 129
NOTE_KEYS = ('w_hh_n', 'w_ih_tok', 'b_hh_n', 'w_p', 'b_p', 'w_dh_h', 'w_dh_p', 'b_dh', 'w_hh_d', 'b_hh_d', 'tab0', 'tab', 'w_out', 'b_out',
             'w_embT', 'b_emb')
BF16_KEYS = ('w_hh_n', 'w_ih_tok', 'w_p', 'w_dh_h', 'w_dh_p', 'w_hh_d', 'e_w_ih', 'e_w_hh')     # consumed as bf16: representable as given


def first_argmax(v):
    """first maximal index along the last axis, and the top-1 minus top-2 margin"""
    v = np.asarray(v)
    i = np.argmax(v, axis=-1)
    s = np.sort(v, axis=-1)
    return i.astype(np.int64), (s[..., -1] - s[..., -2]).astype(F8)


def _forced(words, decided):
    """the header's rule: a word >= 0 overrides the decision, a negative word leaves it free"""
    if words is None:
        return decided
    words = np.asarray(words).astype(np.int64)
    return np.where(words >= 0, words, decided)


def _loop(W, gc, h0, tok0, emb, coin_mask, force_pitch, force_dur, kp):
    F = F4 if kp else F8
    rnd = bf16_round if kp else (lambda a: np.asarray(a, F8))
    w = {k: np.asarray(W[k], F) for k in NOTE_KEYS}
    gc, h, tok = np.asarray(gc, F), np.asarray(h0, F), np.asarray(tok0, F)
    B = gc.shape[0]
    o = dict(HN=np.zeros((16, B, HN), F), gates_n=np.zeros((15, 4, B, HN), F), pitch=np.zeros((15, B, NP), F), HD=np.zeros((6, 15, B, HD), F),
             gates_d=np.zeros((5, 4, 15, B, HD), F), dur=np.zeros((15, B, 10), F), idx=np.zeros((5, 15, B), np.int64),
             TOK=np.zeros((15, B, E), F), PRED=np.zeros((16, B, E), F), pidx=np.zeros((15, B), np.int64), margin_p=np.zeros((15, B), F8),
             margin_d=np.zeros((5, 15, B), F8), plen=np.zeros(B, np.int64))
    o['HN'][0], o['TOK'][0], o['PRED'][0] = h, tok, tok
    for n in range(15):
        # ---- notes-GRU cell: the token part of the input product joins the hoisted part
        tp = (rnd(tok) @ w['w_ih_tok'].T).astype(F)
        if kp:
            hs, g, _ = G.kp_forward(gc[None], tp[None], w['w_hh_n'], w['b_hh_n'], h, None, False, None, bf16=True)
        else:
            hs, g = G.gru_forward(gc[None], tp[None], w['w_hh_n'], w['b_hh_n'], h, None, False, None)
        h = hs[0]
        o['HN'][n + 1], o['gates_n'][n] = h, g[0]
        hop = rnd(h)
        # ---- pitch head and decision
        logit = (hop @ w['w_p'].T + w['b_p']).astype(F)
        free, o['margin_p'][n] = first_argmax(logit)
        p = _forced(None if force_pitch is None else force_pitch[n], free)
        o['pitch'][n], o['pidx'][n] = logit, p
        # ---- dur_hid_linear([h | logits]) and the five duration steps with argmax feedback
        hd = (hop @ w['w_dh_h'].T + rnd(logit) @ w['w_dh_p'].T + w['b_dh']).astype(F)
        o['HD'][0, n] = hd
        bits = np.zeros((5, B), np.int64)
        for d in range(5):
            gi = np.broadcast_to(w['tab0'], (B, 3 * HD)) if d == 0 else w['tab'][bits[d - 1]]
            r, z, nn, hn, hd = (D._kp_cell if kp else D._cell)(hd, gi, w['w_hh_d'], w['b_hh_d'])
            est = (hd @ w['w_out'].T + w['b_out']).astype(F)
            o['HD'][d + 1, n], o['gates_d'][d, :, n], o['dur'][n, :, 2 * d:2 * d + 2] = hd, (r, z, nn, hn), est
            o['margin_d'][d, n] = np.abs(est[:, 1].astype(F8) - est[:, 0].astype(F8))
            bits[d] = _forced(None if force_dur is None else force_dur[d][n], D.argmax2(est))
        o['idx'][:, n] = bits
        # ---- the predicted token and the token fed to the next note step
        pred = (w['b_emb'] + w['w_embT'][p]).astype(F)
        for d in range(5):
            pred = (pred + bits[d][:, None].astype(F) * w['w_embT'][NP + d]).astype(F)
        o['PRED'][n + 1] = pred
        if n < 14:
            tok = np.asarray(emb[n + 1], F) if (coin_mask >> n) & 1 else pred
            o['TOK'][n + 1] = tok
    eos = o['pidx'] == EOS
    o['plen'] = np.where(eos.any(0), eos.argmax(0) + 1, 15).astype(np.int64)
    o['xhat'] = np.concatenate([o['pidx'][:, :, None], o['idx'].transpose(1, 2, 0)], axis=2).transpose(1, 0, 2)     # [B, 15, 6]: slots 1..15
    return o


def note_loop(W, gc, h0, tok0, emb=None, coin_mask=0, force_pitch=None, force_dur=None):
    """one launch of ptv_free_note_loop in float64.  W: the sixteen `w` entries unpacked (NOTE_KEYS); gc [B, 1536]; h0 [B, 512]; tok0
    [B, 128]; emb [16, B, 128] (needed with coin_mask); force_pitch [15, B], force_dur [5, 15, B] or None.  -> dict, the rows of t:
    HN [16, B, 512] (slot 0 = h0), gates_n [15, 4, B, 512] (r, z, n, hn), pitch [15, B, 130], HD [6, 15, B, 64], gates_d [5, 4, 15, B, 64],
    dur [15, B, 10], idx [5, 15, B], TOK [15, B, 128] (slot 0 = tok0), PRED [16, B, 128] (slot 0 = tok0: the caller's), xhat [B, 15, 6]
    (slots 1..15), plen [B], pidx [15, B] and the top-1 minus top-2 margins margin_p [15, B], margin_d [5, 15, B]"""
    return _loop(W, gc, h0, tok0, emb, coin_mask, force_pitch, force_dur, False)


def kp_note_loop(W, gc, h0, tok0, emb=None, coin_mask=0, force_pitch=None, force_dur=None):
    """note_loop at the kernels' precision: fp32 arithmetic, fp32 states and logits, and bf16 rounding (RNE) exactly where freerun.hip
    rounds --
      * the state operand of the gate products h . W_hh^T (h16; the z h term of the update keeps the fp32 state hf),
      * the token operand of token . W_ih[:, Ht:]^T (tok16: the first token, the predicted token and the ground-truth token alike),
      * the six packed weights (given bf16-representable, so nothing changes),
      * the new state as the operand of the pitch head and of the state part of dur_hid_linear (h16[nxt]),
      * the pitch logits as the operand of the logits part of dur_hid_linear (pit16, K padded 130 -> 160 with zeros),
      * the duration state as the operand of hd . W_hh_d^T (hd16; est_dur is an fp32 dot product of the fp32 state),
      * the stored gate planes gates_n / gates_d and the state copies HN16 / HD16 (rounded by to_stored()).
    Biases, tables, dur_out_linear and the token embedding are fp32 throughout.  Sigmoid and tanh are numpy's fp32 ones (the kernel's
    are v_exp_f32 / v_rcp_f32 forms: a few fp32 ulps away, far below a bf16 operand's rounding)."""
    return _loop(W, gc, h0, tok0, emb, coin_mask, force_pitch, force_dur, True)


def to_stored(o):
    """a kernel-precision result with what the kernel stores in bf16 rounded: the gate planes, and HN16 / HD16 beside the fp32 states"""
    s = dict(o)
    s['gates_n'], s['gates_d'] = bf16_round(o['gates_n']), bf16_round(o['gates_d'])
    s['HN16'], s['HD16'] = bf16_round(o['HN']), bf16_round(o['HD'])
    return s


def decisions(o):
    """-> force_pitch [15, B], force_dur [5, 15, B] (int32) that replay the decisions of a run"""
    return o['pidx'].astype(np.int32), o['idx'].astype(np.int32)


def walk(ref, pidx, idx):
    """the free trajectory of another evaluation against the reference's: per row the first decision that differs, in the order the
    decoder takes them (note step n: pitch, then duration bits 0..4).  -> list of (b, n, k) with k = -1 for the pitch and d for duration
    bit d, and the number of decisions AFTER those first differences (what a comparison has to leave out), of 90 per row"""
    a = np.concatenate([ref['pidx'][:, None], ref['idx'].transpose(1, 0, 2)], axis=1)                   # [15, 6, B]
    b = np.concatenate([np.asarray(pidx)[:, None], np.asarray(idx).transpose(1, 0, 2)], axis=1)
    B = a.shape[2]
    diff = (a != b).reshape(90, B)
    first, left = [], 0
    for r in range(B):
        if diff[:, r].any():
            q = int(diff[:, r].argmax())
            first.append((r, q // 6, q % 6 - 1))
            left += 89 - q
    return first, left


def margin_at(ref, b, n, k):
    return float(ref['margin_p'][n, b] if k < 0 else ref['margin_d'][k, n, b])


# ================================================================================================ resummarize
def _resum(W, PRED, plen, kp):
    F = F4 if kp else F8
    rnd = bf16_round if kp else (lambda a: np.asarray(a, F8))
    PRED, plen = np.asarray(PRED, F), np.asarray(plen)
    B = PRED.shape[1]
    o = dict(XH=np.zeros((2, 17, B, HE), F), XG=np.zeros((2, 16, 4, B, HE), F), tok_next=np.zeros((B, 2 * HE), F))
    for dr in range(2):
        w_ih, w_hh = np.asarray(W['e_w_ih'][dr], F), np.asarray(W['e_w_hh'][dr], F)
        gi = ((rnd(PRED).reshape(16 * B, E) @ w_ih.T).astype(F).reshape(16, B, 3 * HE) + np.asarray(W['e_b_ih'][dr], F)).astype(F)
        h0 = np.zeros((B, HE), F)
        if kp:
            hs, g, _ = G.kp_forward(gi, None, w_hh, W['e_b_hh'][dr], h0, plen, bool(dr), None, bf16=True)
        else:
            hs, g = G.gru_forward(gi, None, w_hh, W['e_b_hh'][dr], h0, plen, bool(dr), None)
        o['XH'][dr, 1:], o['XG'][dr] = hs, g
        o['tok_next'][:, dr * HE:(dr + 1) * HE] = hs[15]
    return o


def resummarize(W, PRED, plen):
    """one launch of ptv_free_resummarize in float64: the bidirectional GRU 128 -> 128 over PRED [16, B, 128] (the rows of t) with
    packed-sequence masking -- step tt is live when tt < plen, the backward direction walks tt = 15 .. 0; a dead step copies the state and
    stores the gates (0, 1, 0, hn) with the computed hn.  W: e_w_ih / e_w_hh [2, 384, 128], e_b_ih / e_b_hh [2, 384] (forward, reverse).
    -> XH [2, 17, B, 128] (slot 0 zero, slot s + 1 = the state after PROCESSING step s), XG [2, 16, 4, B, 128], tok_next [B, 256] =
    [forward final | backward final]"""
    return _resum(W, PRED, plen, False)


def kp_resummarize(W, PRED, plen):
    """resummarize at the kernel's precision: fp32, with PRED (x16) and the state operand (h16) rounded to bf16 before their products, the
    weights bf16 as given, the fp32 state in the z h term; the stored gates XG are bf16 (to_stored_resum)"""
    return _resum(W, PRED, plen, True)


def to_stored_resum(o):
    s = dict(o)
    s['XG'] = bf16_round(o['XG'])
    return s


# ================================================================================================ inputs
def _u(rng, k, *shape):
    return rng.uniform(-k, k, shape).astype(F4)


WIDE_EOS_UNITS = 8              # 'wide': the <eos> logit reads this many row-driven state units with weight WIDE_EOS_W
WIDE_EOS_W = 1.5


@functools.lru_cache(maxsize=None)
def weights(kind='init'):
    """kind 'init': every tensor at torch's default init scale (uniform +-1/sqrt(fan)), what the model starts training from.
    'wide': well-separated decisions by construction (see inputs(..., 'wide')): the embedding lives on the 1/16 lattice (tokens are
    bf16-exact), the token part of the notes GRU drives the candidate state of the first 256 units with one +-64 weight each (a saturated
    sign that depends on the previous pitch), the pitch head and dur_out_linear carry a gain, the <eos> logit reads WIDE_EOS_UNITS
    row-driven units.  'tie': 'init' with pitch-head rows 7 and 77 identical under the largest bias and the two rows of
    dur_out_linear identical.  Everything the kernels consume as bf16 is bf16-representable."""
    rng = np.random.RandomState({'init': 11, 'wide': 12, 'tie': 13}[kind])
    kn, kd, ke, kh, km = 1 / np.sqrt(HN), 1 / np.sqrt(HD), 1 / np.sqrt(HE), 1 / np.sqrt(HN + NP), 1 / np.sqrt(NP + 5)
    W = dict(w_hh_n=_u(rng, kn, 3 * HN, HN), w_ih_tok=_u(rng, kn, 3 * HN, E), b_hh_n=_u(rng, kn, 3 * HN), w_p=_u(rng, kn, NP, HN),
             b_p=_u(rng, kn, NP), w_dh_h=_u(rng, kh, HD, HN), w_dh_p=_u(rng, kh, HD, NP), b_dh=_u(rng, kh, HD),
             w_hh_d=_u(rng, kd, 3 * HD, HD), b_hh_d=_u(rng, kd, 3 * HD), w_ih_d=_u(rng, kd, 3 * HD, 5), b_ih_d=_u(rng, kd, 3 * HD),
             sos=rng.uniform(0, 1, 5).astype(F4), w_out=_u(rng, kd, 2, HD), b_out=_u(rng, kd, 2), w_emb=_u(rng, km, E, NP + 5),
             b_emb=_u(rng, km, E), e_w_ih=_u(rng, ke, 2, 3 * HE, E), e_w_hh=_u(rng, ke, 2, 3 * HE, HE), e_b_ih=_u(rng, ke, 2, 3 * HE),
             e_b_hh=_u(rng, ke, 2, 3 * HE))
    if kind == 'wide':
        W['w_emb'] = (rng.choice([-8, 8], (E, NP + 5)) / 16.0).astype(F4)                 # pitch columns +-1/2 ...
        W['w_emb'][:, NP:] = (rng.choice([-1, 1], (E, 5)) / 16.0).astype(F4)              # ... duration columns +-1/16: never flip the sign
        W['b_emb'] = np.zeros(E, F4)
        W['w_ih_tok'][:] = 0
        sgn = rng.choice([-64.0, 64.0], HN // 2)
        W['w_ih_tok'][2 * HN + np.arange(HN // 2), np.arange(HN // 2) % E] = sgn          # candidate of unit u < 256: +-64 tok[u % 128]
        W['w_p'] *= F4(4.0)
        W['w_p'][EOS] = 0
        W['w_p'][EOS, HN // 2:HN // 2 + WIDE_EOS_UNITS] = WIDE_EOS_W
        W['b_p'][EOS] = 0
        W['w_dh_p'] *= F4(1.0 / 64)
        W['w_hh_d'] *= F4(1.0 / 32)
        W['w_ih_d'] *= F4(8.0)
        W['w_out'] *= F4(4.0)
    if kind == 'tie':
        W['w_p'][77] = W['w_p'][7]
        W['b_p'][7] = W['b_p'][77] = F4(3.0)
        W['w_out'][1], W['b_out'][1] = W['w_out'][0], W['b_out'][0]
    for k in BF16_KEYS:
        W[k] = bf16_round(W[k])
    tab0, tab = D.gate_tables(W['w_ih_d'], W['b_ih_d'], W['sos'])
    W['tab0'], W['tab'] = tab0.astype(F4), tab.astype(F4)                                 # the kernels and the references see these fp32 tables
    W['w_embT'] = np.ascontiguousarray(W['w_emb'].T)
    for v in W.values():
        v.setflags(write=False)
    return W


def embed(W, pitch, bits):
    """note_embedding of (pitch [..], bits [.., 5]) in fp32"""
    return (W['b_emb'] + W['w_embT'][pitch] + (np.asarray(bits, F4)[..., None] * W['w_embT'][NP:]).sum(-2)).astype(F4)


@functools.lru_cache(maxsize=None)
def inputs(B, seed=0, kind='init'):
    """the per-launch inputs of B rows: gc [B, 1536], h0 [B, 512], tok0 [B, 128], emb [16, B, 128] (fp32).
    'wide' (for weights('wide')): gc's update third is -12 (z ~ 0: the state is the candidate), its candidate third is 0 on units < 256
    (the token's +-64 weight decides: |pre-activation| >= 12) and +-8 by a random sign per row on units >= 256, so every state unit
    saturates and rounds to exactly +-1 as a bf16 operand -- the rounding is a common factor of all logits, not noise; tokens are
    embeddings of notes.  Row 0 has all <eos> units positive (<eos> at note step 0), row 1 all negative (never <eos>)."""
    rng = np.random.RandomState(1000 + 64 * seed + B)
    gc = rng.normal(0, 0.6, (B, 3 * HN)).astype(F4)
    h0 = rng.normal(0, 0.5, (B, HN)).astype(F4)
    tok0 = rng.normal(0, 0.5, (B, E)).astype(F4)
    emb = rng.normal(0, 0.5, (16, B, E)).astype(F4)
    if kind == 'wide':
        W = weights('wide')
        gc[:, HN:2 * HN] = -12.0
        gc[:, 2 * HN:2 * HN + HN // 2] = 0.0
        s = rng.choice([-8.0, 8.0], (B, HN // 2)).astype(F4)
        s[0, :WIDE_EOS_UNITS] = 8.0
        if B > 1:
            s[1, :WIDE_EOS_UNITS] = -8.0
        gc[:, 2 * HN + HN // 2:] = s
        emb = embed(W, rng.randint(0, NP, (16, B)), rng.randint(0, 2, (16, B, 5)))
        tok0 = embed(W, rng.randint(0, NP, B), rng.randint(0, 2, (B, 5)))
    for v in (gc, h0, tok0, emb):
        v.setflags(write=False)
    return gc, h0, tok0, emb


def resum_lengths(B, kind):
    """plen [B] of a resummarize case: 'mixed' = 1, 2, 8, 15 (and a few more) inside every panel, 'full' = 16 (every step live),
    'empty' = 0 (no step live)"""
    if kind == 'full':
        return np.full(B, 16, np.int32)
    if kind == 'empty':
        return np.zeros(B, np.int32)
    return np.array([(1, 2, 8, 15, 3, 15, 1, 11)[b % 8] for b in range(B)], np.int32)


def plane_bounds(ref, kpf, bound_of):
    """the logit bounds a free trajectory is judged by: per note-step plane of the pitch logits [15] and per duration-step plane of the
    duration logits [5]; kpf = the kernel-precision evaluation that REPLAYS the reference's decisions"""
    bp = np.array([float(bound_of(ref['pitch'][n], kpf['pitch'][n])[0]) for n in range(15)])
    bd = np.array([float(bound_of(ref['dur'][:, :, 2 * d:2 * d + 2], kpf['dur'][:, :, 2 * d:2 * d + 2])[0]) for d in range(5)])
    return bp, bd


def margins_over_bounds(ref, bp, bd):
    """the smallest (reference margin) / (2 x plane bound) over the pitch and over the duration decisions: above 1, no evaluation that
    keeps the bound can decide differently"""
    return float((ref['margin_p'] / (2 * bp[:, None])).min()), float((ref['margin_d'] / (2 * bd[:, None, None])).min())


# ================================================================================================ the case tables of the GPU test
BIT_4WAVE, BIT_8WAVE, BIT_STREAM, BIT_S8, BIT_SAMPLE = 0x10000, 0x20000, 0x200000, 0x400000, 0x800000
PATHS = {'res': BIT_4WAVE,                      # 4-wave kernel, head weights resident
         'stream': BIT_4WAVE | BIT_STREAM,      # 4-wave kernel, head weights streamed every note step
         'split': BIT_8WAVE,                    # 8-wave producer / head kernel
         's2': 2 << 18, 's4': 4 << 18,          # cluster of 2 / 4 workgroups per panel
         's8': BIT_S8}                          # cluster of 8
CLUSTER = {'s2': 2, 's4': 4, 's8': 8}
BATCHES = (1, 15, 16, 17, 33)                   # a lone row, a panel short by one, an exact panel, a one-row tail panel, three panels with a tail
STEPS = (0, 13, 31)
LD_PITCH = (136, 131)
COINS = (0, 0x3fff, 0x15a5)
# seeds of inputs(B, seed, 'wide') under which EVERY decision of the fp64 reference has a margin above twice its plane's logit bound (found
# by search over the reference alone; test_freerun_ref_host.py asserts it): no evaluation that keeps the bound can then decide differently
WIDE_SEEDS = {(1, 0): 0, (15, 0): 0, (16, 0): 4, (17, 0): 1, (33, 0): 3, (15, 0x15a5): 9, (16, 0x15a5): 17, (17, 0x15a5): 8, (1, 0x15a5): 2}


def case(path, B, t, mode=0, wset='init', seed=0, ld=136, h0gc=0, s16=0, coin=0, force='replay', samp=0):
    """path: a key of PATHS; mode = train & 3; wset: weights(); h0gc: io[18] given; s16: HN16 / HD16 given; coin: the coin mask (with a
    ground-truth emb); force: 'replay' (the reference's decisions as force arrays), 'free' (no force arrays: the FORCE = 0 instantiation)
    or 'partial' (force arrays of -1 but for a few entries); samp: a sampling block as io[21] with train bit 23 (inference only; with every
    decision forced the draw decides nothing and the outputs are the argmax decode's)"""
    assert not samp or (mode == 0 and coin == 0 and force == 'replay')
    if wset == 'wide':
        seed = WIDE_SEEDS[B, coin]
    return dict(path=path, B=B, t=t, mode=mode, wset=wset, seed=seed, ld=ld, h0gc=h0gc, s16=s16, coin=coin, force=force, samp=samp)


def case_id(c):
    return '%s-B%d-t%d-m%d-%s-ld%d%s%s-c%x-%s%s' % (c['path'], c['B'], c['t'], c['mode'], c['wset'], c['ld'], '-h0gc' if c['h0gc'] else '',
                                                     '-s16' if c['s16'] else '', c['coin'], c['force'], '-samp' if c['samp'] else '')


def _replay_cases():
    """every path x every B, forced replay; t, mode, weight set, ld_pitch, io[18], HN16 / HD16 and the coin mask rotate so that every value
    meets every path; B = 33 always runs t = 31 (the last row of every tensor)"""
    out = []
    for pi, path in enumerate(PATHS):
        for bi, B in enumerate(BATCHES):
            k = pi + bi
            mode = (1, 0, 2)[k % 3]
            out.append(case(path, B, 31 if B == 33 else STEPS[k % 3], mode, ('init', 'wide')[(k // 2) % 2] if B != 33 else 'init',
                            seed=k, ld=LD_PITCH[k % 2], h0gc=(k // 3) % 2,
                            coin=0x15a5 if mode and bi in (1, 3) else 0))
    # HN16 / HD16 given (the rotation above leaves them NULL), with io[18]
    out += [case(path, 17, 31, 1, 'init', seed=50 + pi, ld=131, h0gc=1, s16=1) for pi, path in enumerate(PATHS)]
    # the three coin masks in train mode on one path, and the one the rotation above leaves out on two more
    out += [case('res', 17, 13, 1, 'init', seed=40 + i, coin=c) for i, c in enumerate(COINS)]
    out += [case('split', 17, 0, 1, 'init', seed=44, coin=0x3fff), case('s2', 17, 31, 2, 'init', seed=45, coin=0x3fff)]
    # a sampling block present (the SAMP = 1, FORCE = 1 instantiations), every decision forced
    out += [case(path, 17, 13, 0, 'init', seed=46 + i, samp=1) for i, path in enumerate(('res', 'split', 's4'))]
    return out


def _free_cases():
    """every path x every B without force arrays on the 'wide' set (the trajectory is held to the reference's), and one 'init' run per
    path (only the decisions-are-the-argmax-of-the-emitted-logits check applies there)"""
    out = []
    for pi, path in enumerate(PATHS):
        for bi, B in enumerate(BATCHES):
            mode = (pi + bi) % 3
            coin = 0x15a5 if mode and bi in (1, 3) else 0
            out.append(case(path, B, 31 if B == 33 else STEPS[(pi + 2 * bi) % 3], mode, 'wide', ld=LD_PITCH[(pi + bi + 1) % 2], h0gc=(pi + bi) % 2,
                            coin=coin, force='free'))
        out.append(case(path, 17, STEPS[pi % 3], 0, 'init', seed=60 + pi, force='free'))
    return out


REPLAY_CASES = _replay_cases()
FREE_CASES = _free_cases()
PARTIAL_CASES = [case(p, 17, 13, 0, 'wide', force='partial') for p in ('res', 'split', 's4')]
TIE_CASES = [case(p, 17, 13, 0, 'tie', seed=70, force='free') for p in ('res', 'split', 's2')]
SEQ_CASES = [case(p, 17, 0, 1, 'init', seed=80, force='replay') for p in ('res', 's4', 's8')]           # t = 0 then t = 1 on the same buffers
NOTE_CASES = REPLAY_CASES + FREE_CASES + PARTIAL_CASES + TIE_CASES + SEQ_CASES
# resummarize: (B, t, train, lengths)
RESUM_CASES = [(B, 31 if B == 33 else STEPS[(bi + tr) % 3], tr, 'mixed') for bi, B in enumerate(BATCHES) for tr in (0, 1, 2, 3)] + \
              [(17, 13, tr, kind) for kind in ('full', 'empty') for tr in (1, 2)]


def case_data(c, t_offset=0):
    """weights, inputs and the force arrays of a case -> W, (gc, h0, tok0, emb), ref (the free fp64 run), (force_pitch, force_dur) or
    (None, None).  t_offset: the second launch of a SEQ case takes fresh inputs"""
    W = weights(c['wset'])
    x = inputs(c['B'], c['seed'] + 7 * t_offset, c['wset'])
    ref = _ref_free(c['wset'], c['B'], c['seed'] + 7 * t_offset, c['coin'])
    fp, fd = decisions(ref)
    if c['force'] == 'free':
        fp = fd = None
    elif c['force'] == 'partial':
        fp, fd = partial_force(ref)
    return W, x, ref, (fp, fd)


@functools.lru_cache(maxsize=None)
def _ref_free(wset, B, seed, coin):
    gc, h0, tok0, emb = inputs(B, seed, wset)
    return note_loop(weights(wset), gc, h0, tok0, emb, coin)


def partial_force(ref):
    """force arrays of -1 everywhere but a few entries, each set to a value the reference did NOT decide (so obeying shows)"""
    fp, fd = np.full(ref['pidx'].shape, -1, np.int32), np.full(ref['idx'].shape, -1, np.int32)
    B = fp.shape[1]
    for n, b in ((0, 0), (3, B - 1), (7, B // 2), (14, B - 1)):
        fp[n, b] = (ref['pidx'][n, b] + 5) % 128
    for d, n, b in ((0, 0, B - 1), (2, 5, 0), (4, 14, B // 2), (4, 9, B - 1)):
        fd[d, n, b] = 1 - ref['idx'][d, n, b]
    return fp, fd
