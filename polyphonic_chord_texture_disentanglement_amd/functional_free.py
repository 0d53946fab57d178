"""Scheduled-sampling / free-running PianoTree decoder and chord decoder (the step loop).

Reference: `PtvaeDecoder.decoder/decode_notes/decode_note` (ptvae.py:336-496) with arbitrary
teacher-forcing coins, `inference=True` (model.py:124-131), and `RnnDecoder.forward` (ptvae.py:51-87).

Forward is inherently sequential -- every next token is an argmax of the previous step -- so it walks
32 x 15 x (1 + 5) cell steps on [B]-row windows of the SAME step-major buffers the teacher-forced path
uses.  Backward is not: argmax is not differentiable, so given the recorded tokens every recurrent chain is
independent across time steps and the whole BPTT runs batched over all 32*B rows exactly like the
teacher-forced path; token gradients are routed to the ground-truth embedding or to the predicted-token
buffer (whose gradient reaches `note_embedding` and, through the re-summarising bi-GRU,
`dec_notes_emb_gru`) -- never into the logits that produced the argmax.
"""
import collections
import contextlib
import ctypes
import math
import os
import struct
import weakref

import numpy as np
import torch

from . import functional as F_
from ._lib import SlotTable, call, lib, ptr, stream_ptr
from .functional import (DEC_PARAM_NAMES, BiGruState, Side, _bgrad, _bigru_backward, _empty, _eye2, _gbuf, _onehot2x5, _zeros,
                         colsum, copy2d, gemm, gru_bwd, sum_steps)

FREE_PARAM_NAMES = DEC_PARAM_NAMES + ['note_embedding.weight', 'note_embedding.bias']
EMB_GRU = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0', 'weight_ih_l0_reverse', 'weight_hh_l0_reverse',
           'bias_ih_l0_reverse', 'bias_hh_l0_reverse')

_SOS = {}
_ROUTE_MASKS = {}


def _route_mask(key, dev):
    """device int32 mask of a coin pattern (the backward's gradient routing): cached per pattern -- with tfr = 0 or 1 it is one
    constant, and a host-to-device copy per step is a synchronisation point (and impossible inside a graph capture)"""
    k = (key, str(dev))
    m = _ROUTE_MASKS.get(k)
    if m is None:
        if len(_ROUTE_MASKS) > 64:
            _ROUTE_MASKS.clear()
        if key[0] == 'tok':
            t_ = torch.ones(15, 32, dtype=torch.int32)
            for t in range(32):
                for n in range(14):
                    t_[n + 1, t] = 1 if key[1][t][n] else 0
        else:
            t_ = torch.tensor([1 if c else 0 for c in key[1]] + [1], dtype=torch.int32)
        m = _ROUTE_MASKS[k] = t_.to(dev)
    return m


def _sos_grid(dev):
    """a [1,32,16,6] grid whose every row is <sos> (ptvae.py:315-320); cached so graph capture sees no H2D copy"""
    k = str(dev)
    if k not in _SOS:
        _SOS[k] = torch.tensor([128, 2, 2, 2, 2, 2], dtype=torch.long).view(1, 1, 1, 6).expand(1, 32, 16, 6).contiguous().to(dev)
    return _SOS[k]


# ---------------------------------------------------------------------------------------------
# row-partitioned persistent kernels for the step loop (csrc/freerun.hip): one launch per time step walks all 15 note steps of
# a 16-sample panel, one more re-summarises the predicted notes.  bf16 precision, init_model() geometry.
# ---------------------------------------------------------------------------------------------
FREE_PERSIST = True
# the persistent path of DecoderStepFn.forward behind ONE C call (ptv_decoder_free_fwd, csrc/composite.hip: ~170 launches -- prologue, the
# 32-step loop, the batched recompute); PTV_FREE_COMPOSITE=0: the same launches sequenced from here (bit-identical)
FREE_COMPOSITE = os.environ.get('PTV_FREE_COMPOSITE', '1') != '0'
_DFF, _DFB = SlotTable('DFF'), SlotTable('DFB')
_DFF_KEEP = []              # what the last ptv_decoder_free_fwd call points to: its launches are queued, not run, when the call returns
_DFB_PATH = ''              # (diagnostic) the last DecoderStepFn.backward: 'one call' (ptv_decoder_free_bwd), else the first reason against it
# training forward of the step loop: the panels store only decisions, logits and fed tokens; states and gates the backward needs are
# recomputed afterwards for all 480*B rows at once by the teacher-forced kernels (same tokens, same decisions forced)
FREE_REPLAY = True
# note-loop kernel: None = by panel count (csrc/freerun.hip), True / False = force the producers-heads split / the 4-wave kernel
NOTE_LOOP_SPLIT = None
# cluster mode of the 4-wave kernel: S workgroups per 16-sample panel, each streaming 1/S of the notes-GRU gate weights (bound by ONE
# CU's L2 port), the new state all-gathered once per note step.  None = by panel count (4 up to 32 panels, 2 up to 64), 0 = off
LAST_CLUSTER_COUNTERS = None
NOTE_LOOP_CLUSTER = None if os.environ.get('PTV_NOTE_CLUSTER') is None else int(os.environ['PTV_NOTE_CLUSTER'])


# ---------------------------------------------------------------------------------------------
# sampled decode (DESIGN.md "Sampled decode"): the decisions of the free-running decoder as seeded draws from softmax(logits / T).
# The parameters travel as a 32-byte DEVICE block {uint64 seed, uint64 draw, int64 sample_offset, float T_pitch, float T_dur} that the
# kernels read when they run -- a captured graph holds its address, so seed / draw / temperatures change without a new capture.
# ---------------------------------------------------------------------------------------------
SAMPLE_BIT = 0x800000           # ptv_free_note_loop's `train` word: io[21] is the sampling block
# truncated sampling (top_k / min_p bound the support of the PITCH draw): the block grows to 48 bytes -- the 32 above, then {int32 top_k
# (0 = off), float ln(min_p) (LN_MIN_P_OFF = off), uint32 round(top_p * 2^24) (0 = off), 4 reserved bytes} -- and the word count of the
# tensor (4 or 6) picks the instantiation
TRUNC_BIT = 0x1000000           # ... io[21] is the 48-byte block (only together with SAMPLE_BIT)
LN_MIN_P_OFF = 1.0              # any ln_min_p > 0 switches the min_p rule off (ln(min_p) <= 0 for every min_p in (0, 1])
TOP_P_ONE = 1 << 24             # nucleus: the block holds top_p as round(top_p * 2^24) in [1, 2^24]; 0 = off (top_p = 1.0 or None)
# constrained decode (pitch masks, ascending notes: restrictions on the SUPPORT of the pitch decision, applied before any truncation): the
# block grows to 64 bytes -- the 48 above (without a truncation rule: top_k 0, LN_MIN_P_OFF, 0), then {uint32 flags, uint32 reserved, uint64
# device address of the mask or 0} -- eight words
CONS_BIT = 0x2000000            # ... io[21] is the 64-byte block (only together with SAMPLE_BIT)
CONS_ASCENDING = 1              # flags bit 0: a pitch < 128 must exceed the largest pitch < 128 already decided in the time step; never <sos>
CONS_MASK_ROW1 = 2              # flags bit 1: the mask has one row [32, 4] for the whole batch
# row-wise decode (per-row sampling parameters: the constrained kind with its six scalars -- both temperatures, top_k, ln_min_p, top_p and
# the noise stream -- replaced by one 32-byte record per row): the block grows to 80 bytes -- the 64 above (temperatures 0, no rule, sample
# offset 0: the kernels read only seed, draw, flags and mask of them), then {uint64 device address of the row table int32 [B, 8], 8 reserved
# bytes} -- ten words.  Row b of the table: {float T_pitch, float T_dur, int32 top_k, float ln_min_p, uint32 top_p_q24, 0, int64 sample_id}
ROWS_BIT = 0x4000000            # ... io[21] is the 80-byte block (only together with SAMPLE_BIT)
SAMPLE_ID_TOP = 1 << 47         # a sample id, like sample_offset + row, lies in [0, 2^47)

# the five variants of a decode, each stated once: words of the block, its bits in ptv_free_note_loop's `train` word, the composite's
# SAMPLE_TRUNC / SAMPLE_CONS / SAMPLE_ROWS dims, the kind number of PtvaeDecoder's graph keys, the bytes ptv_decode_logprob reads, and the
# entry points of the non-persistent loop (note token, fused duration GRU, per-step duration token).  The row-wise kind is a constrained
# kind (cons = 1: mask, flags and force words as there) whose duration entries take the force array or NULL under one name
class BlockKind(collections.namedtuple('BlockKind', 'words bits trunc cons kind nbytes note_token dur_gru dur_token')):
    __slots__ = ()

    @property
    def rows(self):
        """1 for the row-wise kind (the composite's SAMPLE_ROWS dim), else 0"""
        return int(self.kind == 4)


ARGMAX = BlockKind(0, 0, 0, 0, 0, 0, 'ptv_note_token', 'ptv_dur_gru_fwd', 'ptv_dur_out_token')
SAMPLED = BlockKind(4, SAMPLE_BIT, 0, 0, 1, 32, 'ptv_note_token_sample', 'ptv_dur_gru_fwd_sample', 'ptv_dur_out_token_sample')
TRUNCATED = SAMPLED._replace(words=6, bits=SAMPLE_BIT | TRUNC_BIT, trunc=1, kind=2, nbytes=48, note_token='ptv_note_token_sample_trunc')
CONSTRAINED = TRUNCATED._replace(words=8, bits=SAMPLE_BIT | TRUNC_BIT | CONS_BIT, cons=1, kind=3, nbytes=64,
                                 note_token='ptv_note_token_sample_cons')
ROWWISE = CONSTRAINED._replace(words=10, bits=SAMPLE_BIT | TRUNC_BIT | CONS_BIT | ROWS_BIT, kind=4, nbytes=80,
                               note_token='ptv_note_token_sample_rows', dur_gru='ptv_dur_gru_fwd_sample_rows',
                               dur_token='ptv_dur_out_token_sample_rows')


def block_kind(sampling):
    """the BlockKind of a sampling block by its word count; None is the argmax decode"""
    if sampling is None:
        return ARGMAX
    for k in (SAMPLED, TRUNCATED, CONSTRAINED, ROWWISE):
        if sampling.numel() == k.words:
            return k
    raise ValueError('sampling must be a block made by functional_free.sampling_block() on the device of z')


def check_sampling(temperature, dur_temperature=None, sample_offset=0, seed=0, draw=0, *, top_k=None, min_p=None, top_p=None):
    """(T_pitch, T_dur, sample_offset, seed, draw) validated -- ValueError before anything touches a GPU (top_k / min_p / top_p:
    check_truncation)"""
    check_truncation(top_k, min_p, top_p)
    tp = 0.0 if temperature is None else temperature
    td = tp if dur_temperature is None else dur_temperature
    for name, v in (('temperature', tp), ('dur_temperature', td)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or math.isinf(v) or v < 0:
            raise ValueError('%s must be a finite float >= 0, got %r' % (name, v))
    for name, v, top in (('sample_offset', sample_offset, 1 << 47), ('seed', seed, 1 << 64), ('draw', draw, 1 << 63)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0 or v >= top:
            raise ValueError('%s must be an integer in [0, 2^%d), got %r' % (name, top.bit_length() - 1, v))
    return float(tp), float(td), sample_offset, seed, draw


def check_truncation(top_k=None, min_p=None, top_p=None):
    """(top_k word, ln_min_p, top_p word) validated, or None when no rule is given -- ValueError before anything touches a GPU.
    top_k: an integer >= 1 (stored clipped to 130: k >= 130 keeps every class); min_p: a finite float in [0, 1], 0 = off;
    ln(min_p) is taken in float64 (the block stores it rounded to fp32); top_p (nucleus): a finite float in (0, 1], stored as
    round(top_p * 2^24) but never below 1, and 1.0 = off (the word 0)"""
    if top_k is None and min_p is None and top_p is None:
        return None
    k = 0
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1:
            raise ValueError('top_k must be an integer >= 1, got %r' % (top_k,))
        k = min(top_k, 130)
    ln = LN_MIN_P_OFF
    if min_p is not None:
        if isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or math.isnan(min_p) or math.isinf(min_p) or not 0 <= min_p <= 1:
            raise ValueError('min_p must be a finite float in [0, 1], got %r' % (min_p,))
        if min_p > 0:
            ln = math.log(float(min_p))
    q = 0
    if top_p is not None:
        if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or math.isnan(top_p) or math.isinf(top_p) or not 0 < top_p <= 1:
            raise ValueError('top_p must be a finite float in (0, 1], got %r' % (top_p,))
        if top_p < 1:
            q = min(max(int(math.floor(float(top_p) * TOP_P_ONE + 0.5)), 1), TOP_P_ONE)
    return k, ln, q


def check_constraints(pitch_mask=None, ascending=None, batch=None):
    """flags word of a constrained decode, or None when neither keyword is given -- ValueError before anything is launched.
    pitch_mask: an int32 device tensor [B, 32, 4] or [1, 32, 4] (bit p & 31 of word p >> 5 of [b, t]: grid pitch p allowed at step t);
    batch: the rows of the decode when the caller knows them (a mask of another row count, 1 excepted, is refused);
    ascending: a bool -- False alone still selects the constrained kernels (a vacuous constraint)"""
    if pitch_mask is None and ascending is None:
        return None
    if ascending is not None and not isinstance(ascending, bool):
        raise ValueError('ascending must be a bool, got %r' % (ascending,))
    flags = CONS_ASCENDING if ascending else 0
    if pitch_mask is not None:
        if not torch.is_tensor(pitch_mask) or pitch_mask.device.type != 'cuda':
            raise ValueError('pitch_mask must be a device tensor (DisentangleVAE.pitch_mask builds one)')
        if pitch_mask.dtype != torch.int32:
            raise ValueError('pitch_mask must be int32, got %s' % (pitch_mask.dtype,))
        if pitch_mask.dim() != 3 or tuple(pitch_mask.shape[1:]) != (32, 4) or pitch_mask.shape[0] < 1:
            raise ValueError('pitch_mask must have shape [B, 32, 4] or [1, 32, 4], got %s' % (tuple(pitch_mask.shape),))
        if batch is not None and pitch_mask.shape[0] not in (1, batch):
            raise ValueError('pitch_mask has %d rows, the decoded batch has %d' % (pitch_mask.shape[0], batch))
        if pitch_mask.shape[0] == 1:
            flags |= CONS_MASK_ROW1
    return flags


class Keep(collections.namedtuple('Keep', 'pitch dur err batch')):
    """the kept time steps of a free-running decode as its force arrays on the device (ptv_keep_force_build; INTEGRATION.md "Kept steps"):
    pitch int32 [15, 32 B], dur int32 [5, 480 B] (>= 0: the decision is forced to that value, negative: free), err int32 [B] (bit 0: a kept
    step held a pitch outside 0..129 before its <eos> -- that decision stays free), batch = B.
    What a keep demands of the decode is stated here, by class (attributes, not fields), and read by DisentangleVAE._request /
    _sampling_words and PtvaeDecoder.decoder: needs_constrained -- its arrays hold words only the constrained kernels honour, so a decode
    with it is always sent as the constrained kind and refused beside any other block; needs_ascending -- that block must carry the
    `ascending` flag too"""
    __slots__ = ()
    needs_constrained = False
    needs_ascending = False


def keep_steps_row(steps):
    """a host selection of time steps (an iterable of indices 0..31, or a slice) -> 32 bytes, one per step -- ValueError for anything else"""
    row = bytearray(32)
    if isinstance(steps, slice):
        steps = range(*steps.indices(32))
    try:
        items = list(steps)
    except TypeError:
        raise ValueError('steps must be a device bool / uint8 tensor [B, 32] or [1, 32], an iterable of step indices or a slice, got %r'
                         % (steps,)) from None
    for t in items:
        if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < 32:
            raise ValueError('a kept time step must be an integer in 0..31, got %r' % (t,))
        row[t] = 1
    return bytes(row)


def build_keep(x, steps):
    """(x int64 device [B, 32, 16, 6] in the model's grid layout, steps) -> Keep; steps: a device bool / uint8 tensor [B, 32] or [1, 32], or
    a host selection (keep_steps_row) that becomes one [1, 32] row.  ValueError before any launch; nothing is copied to the host."""
    _check_grid(x)
    B = x.shape[0]
    if torch.is_tensor(steps):
        _check_step_selections(x, (('steps', steps),))
        steps = steps.contiguous()
        steps = steps.view(torch.uint8) if steps.dtype == torch.bool else steps     # (uint8 bytes go as they are: non-zero = kept)
    else:
        steps = torch.frombuffer(bytearray(keep_steps_row(steps)), dtype=torch.uint8).view(1, 32).to(x.device)
    x = x.contiguous()
    pitch, dur, err, _ = _force_outputs(B, x.device, counts=False)
    call('ptv_keep_force_build', ptr(x), ptr(steps), steps.shape[0], B, ptr(pitch), ptr(dur), ptr(err), stream_ptr())
    return Keep(pitch, dur, err, B)


def _check_grid(x):
    if not torch.is_tensor(x) or x.device.type != 'cuda':
        raise ValueError('x must be a device tensor: the grid int64 [B, 32, 16, 6]')
    if x.dtype != torch.int64 or x.dim() != 4 or tuple(x.shape[1:]) != (32, 16, 6) or x.shape[0] < 1:
        raise ValueError('x must be int64 [B, 32, 16, 6], got %s %s' % (x.dtype, tuple(x.shape)))


def _check_step_selections(x, named):
    """ValueError unless every selection of named = ((name, selection), ...) that is a tensor is a bool / uint8 tensor [B, 32] or [1, 32]
    on the device of the (checked) grid x"""
    B = x.shape[0]
    for name, s in named:
        if torch.is_tensor(s):
            if s.device != x.device:
                raise ValueError('%s must be on the device of x (or a host iterable of step indices / a slice)' % name)
            if s.dtype not in (torch.bool, torch.uint8):
                raise ValueError('%s must be bool or uint8, got %s' % (name, s.dtype))
            if s.dim() != 2 or s.shape[1] != 32 or s.shape[0] not in (1, B):
                raise ValueError('%s must have shape [B, 32] or [1, 32] with B = %d, got %s' % (name, B, tuple(s.shape)))


def _force_outputs(B, device, counts=True):
    """the outputs of a builder, every element of which its kernel writes: -> (pitch int32 [15, 32 B], dur int32 [5, 480 B], err int32
    [B], counts int32 [B, 32] -- kept_n / yielded -- or None)"""
    def i32(*shape):
        return torch.empty(*shape, dtype=torch.int32, device=device)
    return i32(15, 32 * B), i32(5, 480 * B), i32(B), i32(B, 32) if counts else None


def _ptr_rows(t):
    """an optional per-step operand [rows, 32] as the entry points take it: its address and row count (NULL still names one: 1)"""
    return ptr(t), 1 if t is None else t.shape[0]


def _mode_bytes(x, first, whole, code):
    """two validated selections (a device tensor or the 32 bytes of keep_steps_row; whole may be None) -> mode uint8 [rows, 32] on the
    device of x: `code` at the steps of `first`, 1 at the steps of `whole` -- a step in both is a whole step.  Raises nothing."""
    if not torch.is_tensor(first) and not torch.is_tensor(whole):
        row = bytearray(code * v for v in first)
        for t, w in enumerate(whole or b''):
            if w:
                row[t] = 1
        return torch.frombuffer(row, dtype=torch.uint8).view(1, 32).to(x.device)
    first, whole = (s if s is None or torch.is_tensor(s) else torch.frombuffer(bytearray(s), dtype=torch.uint8).view(1, 32).to(x.device)
                    for s in (first, whole))
    mode = (first != 0).to(torch.uint8) * code
    if whole is not None:
        mode = torch.where(whole != 0, torch.ones_like(mode[:1, :1]), mode)
    return mode.contiguous()


def _selection(x, name, steps, code, whole_steps, limits=(), need_one=None):
    """the arguments the grid-reading builders and splits share, validated -- every ValueError before any launch, in this order: the
    host limits, need_one, the selections, the grid, the device limits -- and then put on the device: -> (x contiguous, mode uint8
    [rows, 32]: `code` at the steps of `steps`, 1 at those of whole_steps, a step in both is a whole step; then one int32 [rows, 32] or
    None = no limit per entry of limits).  name: the argument name of `steps`; limits: ((name, value, top), ...), value None, a host int
    0..top or an int32 device tensor [B, 32] / [1, 32]; need_one: the message for a call that gives none of them, if that is an error"""
    for lname, v, top in limits:
        if v is not None and not torch.is_tensor(v) and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= top):
            raise ValueError('%s must be an integer in 0..%d or an int32 device tensor [B, 32] / [1, 32], got %r' % (lname, top, v))
    if need_one and all(v is None for _, v, _ in limits):
        raise ValueError(need_one)
    sels = [s if s is None or torch.is_tensor(s) else keep_steps_row(s) for s in (steps, whole_steps)]
    if sels[0] is None:
        raise ValueError('%s must be a device bool / uint8 tensor [B, 32] or [1, 32], an iterable of step indices or a slice' % name)
    _check_grid(x)
    B = x.shape[0]
    _check_step_selections(x, ((name, sels[0]), ('whole_steps', sels[1])))
    for lname, v, _ in limits:
        if torch.is_tensor(v):
            if v.device != x.device or v.dtype != torch.int32:
                raise ValueError('%s must be int32 on the device of x, got %s on %s' % (lname, v.dtype, v.device))
            if v.dim() != 2 or v.shape[1] != 32 or v.shape[0] not in (1, B):
                raise ValueError('%s must have shape [B, 32] or [1, 32] with B = %d, got %s' % (lname, B, tuple(v.shape)))
    # ---- nothing below raises
    on_device = tuple(None if v is None else v.contiguous() if torch.is_tensor(v)
                      else torch.full((1, 32), v, dtype=torch.int32, device=x.device) for _, v, _ in limits)
    return (x.contiguous(), _mode_bytes(x, sels[0], sels[1], code)) + on_device


def _voice_selection(x, voice_steps, below, lowest, whole_steps):
    """build_keep_voice's and split_voice's: mode 2 = voice step; below / lowest, at least one of the two"""
    return _selection(x, 'voice_steps', voice_steps, 2, whole_steps, (('below', below, 128), ('lowest', lowest, 15)),
                      'a kept voice needs below (keep the notes under that pitch) or lowest (keep that many notes), or both')


def _top_selection(x, top_steps, above, highest, whole_steps):
    """build_keep_top's and split_top's: mode 4 = top step; above / highest, neither given: the very top note"""
    return _selection(x, 'top_steps', top_steps, 4, whole_steps, (('above', above, 128), ('highest', highest, 15)))


def _split(entry, x, mode, pitch_lim, count_lim):
    """a selection as two model grids, by ptv_grid_split_voice / ptv_grid_split_top -> (voice, rest, kept_n, err)"""
    B = x.shape[0]
    voice, rest = torch.empty_like(x), torch.empty_like(x)
    kept_n = torch.empty(B, 32, dtype=torch.int32, device=x.device)
    err = torch.empty(B, dtype=torch.int32, device=x.device)
    call(entry, ptr(x), ptr(mode), mode.shape[0], *_ptr_rows(pitch_lim), *_ptr_rows(count_lim), B, ptr(voice), ptr(rest), ptr(kept_n),
         ptr(err), stream_ptr())
    return voice, rest, kept_n, err


def build_keep_voice(x, voice_steps, below=None, lowest=None, durations=True, whole_steps=None, return_counts=False):
    """the kept VOICE of a free-running decode -> Keep (ptv_keep_voice_force_build; INTEGRATION.md "Kept voices"): at the steps of
    voice_steps the lowest notes of x's step -- those under pitch `below`, at most `lowest` of them, a prefix of the step -- are forced
    and the decoder goes on above them; the steps of whole_steps are kept whole as by build_keep (a step in both is a whole step).
    voice_steps / whole_steps: selections as build_keep's steps; below / lowest: a host int (0..128 / 0..15; 128 / 15 = no limit) or an
    int32 device tensor [B, 32] / [1, 32], at least one of the two; durations=False leaves the duration bits of the voice steps free.
    return_counts: -> (Keep, kept_n int32 [B, 32], the forced pitch decisions per step).  ValueError before any launch; nothing is
    copied to the host."""
    if not isinstance(durations, bool):
        raise ValueError('durations must be a bool, got %r' % (durations,))
    x, mode, below, lowest = _voice_selection(x, voice_steps, below, lowest, whole_steps)
    B = x.shape[0]
    pitch, dur, err, kept_n = _force_outputs(B, x.device)
    call('ptv_keep_voice_force_build', ptr(x), ptr(mode), mode.shape[0], *_ptr_rows(below), *_ptr_rows(lowest), 0 if durations else 1, B,
         ptr(pitch), ptr(dur), ptr(kept_n), ptr(err), stream_ptr())
    keep = Keep(pitch, dur, err, B)
    return (keep, kept_n) if return_counts else keep


FORCE_NOT_EOS = -2          # PTV_FORCE_NOT_EOS: a pitch word that leaves the decision free but takes <eos> out of its support


class RhythmKeep(Keep):
    """a Keep whose pitch array holds FORCE_NOT_EOS words (ptv_keep_rhythm_force_build; INTEGRATION.md "Kept rhythm"): the same four
    fields, so it goes wherever a Keep goes -- but only the constrained kernels honour the word, so a decode with one is always sent as
    the constrained kind (DisentangleVAE._sampling_words), and PtvaeDecoder refuses it beside any other block"""
    __slots__ = ()
    needs_constrained = True


def build_keep_rhythm(x, steps, durations=True, whole_steps=None, return_counts=False):
    """the kept RHYTHM of a free-running decode -> RhythmKeep (ptv_keep_rhythm_force_build; INTEGRATION.md "Kept rhythm"): at the steps of
    `steps` the decode has exactly the notes of x's step -- K decisions that are free but may not be <eos>, then a forced <eos> -- with
    x's duration bits (durations=False: pitches and durations are both drawn, only the count is kept); the steps of whole_steps are
    kept whole as by build_keep (a step in both is a whole step).  Selections as build_keep's steps.  return_counts: -> (RhythmKeep,
    kept_n int32 [B, 32]: K at a rhythm step, the forced pitch decisions at a whole step).  ValueError before any launch; nothing is
    copied to the host."""
    if not isinstance(durations, bool):
        raise ValueError('durations must be a bool, got %r' % (durations,))
    x, mode = _selection(x, 'steps', steps, 3, whole_steps)            # (3 = rhythm step; no limits)
    B = x.shape[0]
    pitch, dur, err, kept_n = _force_outputs(B, x.device)
    call('ptv_keep_rhythm_force_build', ptr(x), ptr(mode), mode.shape[0], 0 if durations else 1, B, ptr(pitch), ptr(dur), ptr(kept_n),
         ptr(err), stream_ptr())
    keep = RhythmKeep(pitch, dur, err, B)
    return (keep, kept_n) if return_counts else keep


FORCE_BELOW_BASE = -256     # PTV_FORCE_BELOW(u) = FORCE_BELOW_BASE - u, u in 1..128: a free pitch word, never <eos>, a note under the ceiling u


class TopKeep(Keep):
    """a Keep whose pitch array holds FORCE_BELOW words under the kept top notes (ptv_keep_top_force_build; INTEGRATION.md "Kept top
    voice"): the same four fields, so it goes wherever a Keep goes -- but only the constrained kernels honour the words and the ceilings
    leave room only for notes that ascend, so a decode with one is always sent as the constrained kind with ascending=True
    (DisentangleVAE._sampling_words), and PtvaeDecoder refuses it beside any other block"""
    __slots__ = ()
    needs_constrained = True
    needs_ascending = True


def build_keep_top(x, top_steps, above=None, highest=None, durations=True, lanes=True, whole_steps=None, return_counts=False):
    """the kept TOP VOICE of a free-running decode -> TopKeep (ptv_keep_top_force_build; INTEGRATION.md "Kept top voice"): at the steps of
    top_steps the highest notes of x's step -- those at or over pitch `above`, at most `highest` of them, a suffix of the step; neither
    given: the very top note -- are forced in their slots, the step keeps its note count, and the notes under them are drawn again, each
    under a ceiling: x's next note (lanes=True: no voice crosses its old neighbour) or the lowest kept pitch less a semitone per decision
    still to come (lanes=False).  durations: True = x's bits for every note of the step, 'kept' = only for the kept notes, False = every
    duration of a top step is drawn.  The steps of whole_steps are kept whole as by build_keep (a step in both is a whole step).
    Selections as build_keep's steps; above / highest: a host int (0..128 / 0..15) or an int32 device tensor [B, 32] / [1, 32].
    return_counts: -> (TopKeep, kept_n int32 [B, 32]: the kept notes of a top step, the forced pitch decisions of a whole step).
    ValueError before any launch; nothing is copied to the host."""
    if not (isinstance(durations, bool) or (isinstance(durations, str) and durations == 'kept')):
        raise ValueError("durations must be True, 'kept' or False, got %r" % (durations,))
    if not isinstance(lanes, bool):
        raise ValueError('lanes must be a bool, got %r' % (lanes,))
    x, mode, above, highest = _top_selection(x, top_steps, above, highest, whole_steps)
    B = x.shape[0]
    pitch, dur, err, kept_n = _force_outputs(B, x.device)
    call('ptv_keep_top_force_build', ptr(x), ptr(mode), mode.shape[0], *_ptr_rows(above), *_ptr_rows(highest),
         (0 if durations is True else 1) | (0 if lanes else 2), B, ptr(pitch), ptr(dur), ptr(kept_n), ptr(err), stream_ptr())
    if durations is False:                                     # every duration word of a top step is free: the [t, b] rows of mode 4
        top = (mode == 4).expand(B, 32).t().reshape(1, 1, 32 * B)
        dur = dur.view(5, 15, 32 * B).masked_fill(top, -1).view(5, 480 * B)
    keep = TopKeep(pitch, dur, err, B)
    return (keep, kept_n) if return_counts else keep


def split_top(x, top_steps, above=None, highest=None, whole_steps=None):
    """the selection of build_keep_top as two model grids (ptv_grid_split_top) -> (x_top, x_rest int64 [B, 32, 16, 6], kept_n int32
    [B, 32], err int32 [B]): per step the kept top notes and what the decoder would re-draw under them, each a valid step"""
    return _split('ptv_grid_split_top', *_top_selection(x, top_steps, above, highest, whole_steps))


FORCE_DUR_RANGE_BASE = -1024    # PTV_FORCE_DUR_RANGE(lo, hi) = FORCE_DUR_RANGE_BASE - (lo | hi << 5), 0 <= lo <= hi <= 31: a free duration word
DUR_FITS = ('segment', 'bar', 'beat')


class DurKeep(Keep):
    """a Keep whose duration array holds FORCE_DUR_RANGE words (ptv_dur_range_force_build; INTEGRATION.md "Duration limits"): the same
    four fields, so it goes wherever a Keep goes -- but only the constrained kernels honour the words, so a decode with one is always
    sent as the constrained kind (DisentangleVAE._sampling_words), and PtvaeDecoder refuses it beside any other block"""
    __slots__ = ()
    needs_constrained = True


class RhythmDurKeep(RhythmKeep, DurKeep):
    """duration limits built into a RhythmKeep: it stays one"""
    __slots__ = ()


class TopDurKeep(TopKeep, DurKeep):
    """duration limits built into a TopKeep: it stays one, `ascending` rule included"""
    __slots__ = ()


class CountKeep(Keep):
    """a Keep whose pitch array holds the floor words of note-count limits (ptv_note_count_force_build; INTEGRATION.md "Note-count
    limits"): FORCE_NOT_EOS, or with room=True FORCE_BELOW ceilings -- then the class it comes back as also has needs_ascending.  The
    same four fields, so it goes wherever a Keep goes; only the constrained kernels honour the words.  (Limits without a floor write
    plain forced <eos> words and need no class of their own.)"""
    __slots__ = ()
    needs_constrained = True


_COMPOSED_KEEPS = {}


def _limits_keep_type(keep, added, ascending=False):
    """the class of the keep that results from building limits into `keep` (None: into nothing).  added: DurKeep, CountKeep, or None for
    limits that write no word of their own kind (a ceiling-only count limit); ascending: the limits' words count on ascending notes.
    The result demands the union of what both demand (needs_constrained / needs_ascending).  A keep that already is of the added kind
    stays what it is, the pairs that have a name keep it (RhythmDurKeep, TopDurKeep), and every other pair is ONE composed class made
    here on first use -- there is no class per combination to maintain."""
    have = Keep if keep is None else type(keep)
    if added is None or issubclass(have, added):
        cls = have
    elif have is Keep:
        cls = added
    elif added is DurKeep and have in (TopKeep, RhythmKeep):
        cls = TopDurKeep if have is TopKeep else RhythmDurKeep
    else:
        cls = (have, added)
    if isinstance(cls, tuple) or (ascending and not cls.needs_ascending):
        bases = cls if isinstance(cls, tuple) else (cls,)
        key = bases + (bool(ascending),)
        if key not in _COMPOSED_KEEPS:
            name = ''.join(b.__name__[:-4] for b in bases) + ('Ascending' if ascending and not any(b.needs_ascending for b in bases) else '')
            _COMPOSED_KEEPS[key] = type(name + 'Keep', bases, {
                '__slots__': (), '__doc__': 'limits built into a keep: the demands of %s' % ' and '.join(b.__name__ for b in bases),
                'needs_constrained': True, 'needs_ascending': bool(ascending) or any(b.needs_ascending for b in bases)})
        cls = _COMPOSED_KEEPS[key]
    return cls


def dur_fit_row(fit):
    """the ceiling of a fit per time step, 32 host ints in durations: 'segment' 32 - t, 'bar' 16 - t % 16, 'beat' 4 - t % 4"""
    if not isinstance(fit, str) or fit not in DUR_FITS:
        raise ValueError("fit must be 'segment', 'bar' or 'beat', got %r" % (fit,))
    return [{'segment': 32 - t, 'bar': 16 - t % 16, 'beat': 4 - t % 4}[fit] for t in range(32)]


def build_dur_limits(device, min_dur=None, max_dur=None, fit=None, steps=None, batch=None, keep=None, return_counts=False):
    """duration limits of a free-running decode -> DurKeep (ptv_dur_range_force_build; INTEGRATION.md "Duration limits"): at the selected
    steps every note decision whose duration bits are free gets the range [floor, ceiling] in durations 1..32.  min_dur / max_dur: a host
    int 1..32 or an integer device tensor [32] / [B, 32]; fit: 'segment' / 'bar' / 'beat' (dur_fit_row).  Whatever is given is combined:
    the ceiling is the smallest of max_dur and the fit's, then the floor, which yields to it.  steps: as build_keep's, None = all 32.
    keep: an existing keep to build into -- its forced and foreign words survive bit for bit, and the result stays what it is (a
    RhythmKeep / TopKeep keeps its promotion).  batch: B, needed when neither keep nor a [B, 32] tensor tells it.  return_counts: ->
    (keep, yielded int32 [B, 32]: 1 where a selected step's floor lay over its ceiling).  ValueError before any launch; nothing is
    copied to the host."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('duration limits are built on the device, got %s' % (dev,))
    if keep is not None:
        check_keep(keep)
        dev = keep.pitch.device
    if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or batch < 1):
        raise ValueError('batch must be an integer >= 1, got %r' % (batch,))
    sizes = set() if batch is None else {batch}
    if keep is not None:
        sizes.add(keep.batch)
    for name, v in (('min_dur', min_dur), ('max_dur', max_dur)):
        if v is None:
            continue
        if torch.is_tensor(v):
            if v.device.type != 'cuda' or (keep is not None and v.device != dev):
                raise ValueError('%s must be a device tensor (on the device of keep), got one on %s' % (name, v.device))
            if v.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError('%s must be an integer tensor, got %s' % (name, v.dtype))
            if not ((v.dim() == 1 and v.shape[0] == 32) or (v.dim() == 2 and v.shape[1] == 32 and v.shape[0] >= 1)):
                raise ValueError('%s must have shape [32] or [B, 32], got %s' % (name, tuple(v.shape)))
            if v.dim() == 2 and v.shape[0] > 1:
                sizes.add(v.shape[0])
        elif isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 32:
            raise ValueError('%s must be an integer in 1..32 or an integer device tensor [32] / [B, 32], got %r' % (name, v))
    fit_row = None if fit is None else dur_fit_row(fit)
    sel = steps if steps is None or torch.is_tensor(steps) else keep_steps_row(steps)
    if torch.is_tensor(sel):
        if sel.device.type != 'cuda' or (keep is not None and sel.device != dev):
            raise ValueError('steps must be on the device (or a host iterable of step indices / a slice)')
        if sel.dtype not in (torch.bool, torch.uint8):
            raise ValueError('steps must be bool or uint8, got %s' % (sel.dtype,))
        if sel.dim() != 2 or sel.shape[1] != 32 or sel.shape[0] < 1:
            raise ValueError('steps must have shape [B, 32] or [1, 32], got %s' % (tuple(sel.shape),))
        if sel.shape[0] > 1:
            sizes.add(sel.shape[0])
    if len(sizes) > 1:
        raise ValueError('the batch sizes of keep, batch, min_dur, max_dur and steps disagree: %s' % (sorted(sizes),))
    if not sizes:
        raise ValueError('batch is needed: neither a keep nor a [B, 32] tensor tells the number of samples')
    B = sizes.pop()
    # ---- nothing below raises
    def rows(v, fill):
        if v is None:
            return torch.full((1, 32), fill, dtype=torch.uint8, device=dev)
        if torch.is_tensor(v):
            return v.to(dev).view(-1, 32).clamp(0, 255).to(torch.uint8)
        return torch.full((1, 32), v, dtype=torch.uint8, device=dev)
    lo, hi = rows(min_dur, 1).contiguous(), rows(max_dur, 32)
    if fit_row is not None:
        hi = torch.minimum(hi, torch.tensor(fit_row, dtype=torch.uint8, device=dev).view(1, 32))
    hi = hi.contiguous()
    if sel is None:
        sel = torch.ones(1, 32, dtype=torch.uint8, device=dev)
    elif torch.is_tensor(sel):
        sel = sel.to(dev).contiguous()
        sel = sel.view(torch.uint8) if sel.dtype == torch.bool else sel
    else:
        sel = torch.frombuffer(bytearray(sel), dtype=torch.uint8).view(1, 32).to(dev)
    pitch, dur, err, yielded = _force_outputs(B, dev)
    src = (None, None) if keep is None else (keep.pitch.contiguous(), keep.dur.contiguous())
    call('ptv_dur_range_force_build', ptr(lo), lo.shape[0], ptr(hi), hi.shape[0], ptr(sel), sel.shape[0], ptr(src[0]), ptr(src[1]), B,
         ptr(pitch), ptr(dur), ptr(yielded), stream_ptr())
    err = err.zero_() if keep is None else keep.err          # (this builder reports nothing: the err of the keep it built into)
    out = _limits_keep_type(keep, DurKeep)(pitch, dur, err, B)
    return (out, yielded) if return_counts else out


def build_count_limits(device, min_count=None, max_count=None, onsets=None, rests=None, steps=None, room=False, batch=None, keep=None,
                       return_counts=False):
    """note-count limits of a free-running decode -> keep (ptv_note_count_force_build; INTEGRATION.md "Note-count limits"): a selected
    step gets at least `min_count` and at most `max_count` notes (the ceiling wins).  min_count / max_count: a host int 0..15 or an
    integer device tensor [32] / [B, 32] (clamped into 0..15).  steps: as build_keep's, None = all 32.  onsets / rests: selections too,
    selected whatever `steps` says -- onsets: a floor of at least 1, rests: the ceiling 0; a step in both is a rest.  At least one of
    the four is needed.  room=True: the floor words are FORCE_BELOW ceilings that leave a semitone for each note still owed, which
    under `ascending` guarantees the floor (without it a floor is "not <eos> while anything else is allowed" and can fall short under
    a narrow mask or `ascending`).  keep: an existing keep to build into -- its words survive bit for bit, a step whose count it
    already fixes is left alone.  The result: without a floor (min_count and onsets both None) only forced <eos> words are written
    and the type of `keep` stays (a plain Keep without one); with a floor a CountKeep (needs_constrained), with room=True one that
    needs_ascending too; built into another keep, the union of both keeps' demands (_limits_keep_type).  batch: B, needed when neither
    keep nor a [B, 32] tensor tells it.  return_counts: -> (keep, yielded int32 [B, 32]: bit 0 the floor lay over the ceiling, bit 1
    the keep owns the step's count, bit 2 a kept prefix is longer than the ceiling, bit 3 the room above a kept prefix may not hold the
    floor).  ValueError before any launch; nothing is copied to the host."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('note-count limits are built on the device, got %s' % (dev,))
    if keep is not None:
        check_keep(keep)
        dev = keep.pitch.device
    if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or batch < 1):
        raise ValueError('batch must be an integer >= 1, got %r' % (batch,))
    if not isinstance(room, bool):
        raise ValueError('room must be a bool, got %r' % (room,))
    sizes = set() if batch is None else {batch}
    if keep is not None:
        sizes.add(keep.batch)
    for name, v in (('min_count', min_count), ('max_count', max_count)):
        if v is None:
            continue
        if torch.is_tensor(v):
            if v.device.type != 'cuda' or (keep is not None and v.device != dev):
                raise ValueError('%s must be a device tensor (on the device of keep), got one on %s' % (name, v.device))
            if v.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError('%s must be an integer tensor, got %s' % (name, v.dtype))
            if not ((v.dim() == 1 and v.shape[0] == 32) or (v.dim() == 2 and v.shape[1] == 32 and v.shape[0] >= 1)):
                raise ValueError('%s must have shape [32] or [B, 32], got %s' % (name, tuple(v.shape)))
            if v.dim() == 2 and v.shape[0] > 1:
                sizes.add(v.shape[0])
        elif isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 15:
            raise ValueError('%s must be an integer in 0..15 or an integer device tensor [32] / [B, 32], got %r' % (name, v))
    sels = {}
    for name, s in (('steps', steps), ('onsets', onsets), ('rests', rests)):
        s = s if s is None or torch.is_tensor(s) else keep_steps_row(s)
        if torch.is_tensor(s):
            if s.device.type != 'cuda' or (keep is not None and s.device != dev):
                raise ValueError('%s must be on the device (or a host iterable of step indices / a slice)' % name)
            if s.dtype not in (torch.bool, torch.uint8):
                raise ValueError('%s must be bool or uint8, got %s' % (name, s.dtype))
            if s.dim() != 2 or s.shape[1] != 32 or s.shape[0] < 1:
                raise ValueError('%s must have shape [B, 32] or [1, 32], got %s' % (name, tuple(s.shape)))
            if s.shape[0] > 1:
                sizes.add(s.shape[0])
        sels[name] = s
    if min_count is None and max_count is None and onsets is None and rests is None:
        raise ValueError('note-count limits need min_count, max_count, onsets or rests')
    if len(sizes) > 1:
        raise ValueError('the batch sizes of keep, batch, min_count, max_count, steps, onsets and rests disagree: %s' % (sorted(sizes),))
    if not sizes:
        raise ValueError('batch is needed: neither a keep nor a [B, 32] tensor tells the number of samples')
    B = sizes.pop()
    # ---- nothing below raises
    def rows(v, fill):
        if torch.is_tensor(v):
            return v.to(dev).reshape(-1, 32).clamp(0, 255).to(torch.uint8)
        return torch.full((1, 32), fill if v is None else v, dtype=torch.uint8, device=dev)

    def selection(s):                                          # -> bool [rows, 32]
        if torch.is_tensor(s):
            return s.to(dev) != 0
        return torch.frombuffer(bytearray(s), dtype=torch.uint8).view(1, 32).to(dev) != 0
    lo, hi = rows(min_count, 0), rows(max_count, 15)
    sel = torch.ones(1, 32, dtype=torch.bool, device=dev) if sels['steps'] is None else selection(sels['steps'])
    rest = None if sels['rests'] is None else selection(sels['rests'])
    if sels['onsets'] is not None:                             # a floor of at least 1 -- but at a step that is a rest as well
        on = selection(sels['onsets'])
        sel = sel | on
        lo = torch.where(on if rest is None else on & ~rest, lo.clamp(min=1), lo)
    if rest is not None:
        sel = sel | rest
        hi = torch.where(rest, torch.zeros_like(hi[:1, :1]), hi)
    lo, hi, sel = lo.contiguous(), hi.contiguous(), sel.to(torch.uint8).contiguous()
    pitch, dur, err, yielded = _force_outputs(B, dev)
    src = (None, None) if keep is None else (keep.pitch.contiguous(), keep.dur.contiguous())
    call('ptv_note_count_force_build', ptr(lo), lo.shape[0], ptr(hi), hi.shape[0], ptr(sel), sel.shape[0], ptr(src[0]), ptr(src[1]),
         1 if room else 0, B, ptr(pitch), ptr(dur), ptr(yielded), stream_ptr())
    err = err.zero_() if keep is None else keep.err          # (this builder reports nothing: the err of the keep it built into)
    floor = min_count is not None or onsets is not None
    out = _limits_keep_type(keep, CountKeep if floor else None, floor and room)(pitch, dur, err, B)
    return (out, yielded) if return_counts else out


# ---------------------------------------------------------------------------------------------
# sounding state (INTEGRATION.md "Sounding state"; include/ptvae_hip.h states the rule): restrictions that see what the
# decode itself decided at earlier time steps.  A Sounding holds the caller's tables; a SoundingRun what one decode reads and writes.
# ---------------------------------------------------------------------------------------------
SOUNDING_NO_RESTRIKE = 1        # bit 0 of the control word


class Sounding:
    """the sounding rules of a decode, for sounding= (DisentangleVAE.sounding; ptv_sounding_step): control (int32 device tensor [1], bit 0
    = no_restrike), max_sounding / min_sounding / steps (uint8 device tensors [rows, 32], rows 1 or batch; 0 in max_sounding = no
    ceiling), batch, and what the host knows of them: no_restrike, ceiling, floor (a rule of that kind was given).  What it demands of
    the decode, like a Keep: needs_constrained -- a mask rule or PTV_FORCE_NOT_EOS words, which only the constrained kernels honour;
    needs_force -- count words, so the decode runs with force arrays (an all-free keep where the caller gave none)"""

    def __init__(self, control, max_sounding, min_sounding, steps, batch, no_restrike=False, ceiling=False, floor=False):
        self.control, self.max_sounding, self.min_sounding, self.steps, self.batch = control, max_sounding, min_sounding, steps, batch
        self.no_restrike, self.ceiling, self.floor = bool(no_restrike), bool(ceiling), bool(floor)

    @property
    def needs_constrained(self):
        return self.no_restrike or self.floor

    @property
    def needs_force(self):
        return self.ceiling or self.floor

    def tables(self):
        return self.max_sounding, self.min_sounding, self.steps

    def _with(self, fn, batch):
        return Sounding(self.control, *(fn(t) if t.shape[0] > 1 else t for t in self.tables()), batch, self.no_restrike, self.ceiling,
                        self.floor)

    def tiled(self, n):
        """the rules of the batch repeated n times (decode_best_of): a table with one row per sample is tiled like a mask's rows"""
        return self._with(lambda t: t.repeat(n, 1), n * self.batch)

    def sliced(self, lo, hi):
        """the rules of the rows lo..hi-1 of the batch (a shard of a decode: the state of a row depends on that row alone)"""
        if not 0 <= lo < hi <= self.batch:
            raise ValueError('rows %r..%r are not rows of a batch of %d' % (lo, hi, self.batch))
        return self._with(lambda t: t[lo:hi].contiguous(), hi - lo)


def build_sounding(device, no_restrike=False, max_sounding=None, min_sounding=None, steps=None, batch=None):
    """the sounding rules of a free-running decode -> Sounding (INTEGRATION.md "Sounding state").  no_restrike: a bool -- a pitch that
    still sounds is not struck again; max_sounding: at most that many pitches sound at a step, a host int 1..127 or an integer device
    tensor [32] / [B, 32] (0 = no ceiling there); min_sounding: at least that many, a host int 0..15 or such a tensor (a floor is "not
    <eos> while anything else is allowed": nothing guarantees it).  steps: as build_keep's, None = all 32 -- the rules act at the selected
    steps, the state is tracked at all of them.  At least one of the three rules must be given.  batch: the rows of the decode.
    ValueError before anything touches the GPU; nothing is copied to the host."""
    if not isinstance(no_restrike, bool):
        raise ValueError('no_restrike must be a bool, got %r' % (no_restrike,))
    if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or batch < 1):
        raise ValueError('batch must be an integer >= 1, got %r' % (batch,))
    sizes = set() if batch is None else {batch}
    for name, v, lo, hi in (('max_sounding', max_sounding, 1, 127), ('min_sounding', min_sounding, 0, 15)):
        if v is None:
            continue
        if torch.is_tensor(v):
            if v.device.type != 'cuda':
                raise ValueError('%s must be a device tensor, got one on %s' % (name, v.device))
            if v.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError('%s must be an integer tensor, got %s' % (name, v.dtype))
            if not ((v.dim() == 1 and v.shape[0] == 32) or (v.dim() == 2 and v.shape[1] == 32 and v.shape[0] >= 1)):
                raise ValueError('%s must have shape [32] or [B, 32], got %s' % (name, tuple(v.shape)))
            if v.dim() == 2 and v.shape[0] > 1:
                sizes.add(v.shape[0])
        elif isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError('%s must be an integer in %d..%d or an integer device tensor [32] / [B, 32], got %r' % (name, lo, hi, v))
    sel = steps if steps is None or torch.is_tensor(steps) else keep_steps_row(steps)
    if torch.is_tensor(sel):
        if sel.device.type != 'cuda':
            raise ValueError('steps must be on the device (or a host iterable of step indices / a slice)')
        if sel.dtype not in (torch.bool, torch.uint8):
            raise ValueError('steps must be bool or uint8, got %s' % (sel.dtype,))
        if sel.dim() != 2 or sel.shape[1] != 32 or sel.shape[0] < 1:
            raise ValueError('steps must have shape [B, 32] or [1, 32], got %s' % (tuple(sel.shape),))
        if sel.shape[0] > 1:
            sizes.add(sel.shape[0])
    if not no_restrike and max_sounding is None and min_sounding is None:
        raise ValueError('sounding needs no_restrike=True, max_sounding or min_sounding')
    if len(sizes) > 1:
        raise ValueError('the batch sizes of batch, max_sounding, min_sounding and steps disagree: %s' % (sorted(sizes),))
    if not sizes:
        raise ValueError('batch is needed: no [B, 32] tensor tells the number of samples')
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('the sounding state lives on the device, got %s' % (dev,))
    # ---- nothing below raises
    def rows(v, hi):
        if torch.is_tensor(v):
            return v.to(dev).reshape(-1, 32).clamp(0, hi).to(torch.uint8).contiguous()
        return torch.full((1, 32), 0 if v is None else v, dtype=torch.uint8, device=dev)
    if sel is None:
        sel = torch.ones(1, 32, dtype=torch.uint8, device=dev)
    elif torch.is_tensor(sel):
        sel = (sel.to(dev) != 0).to(torch.uint8).contiguous()
    else:
        sel = torch.frombuffer(bytearray(sel), dtype=torch.uint8).view(1, 32).to(dev)
    control = torch.tensor([SOUNDING_NO_RESTRIKE if no_restrike else 0], dtype=torch.int32, device=dev)
    return Sounding(control, rows(max_sounding, 127), rows(min_sounding, 15), sel, sizes.pop(), no_restrike, max_sounding is not None,
                    min_sounding is not None)


def check_sounding(sounding, batch=None, device=None):
    """ValueError unless sounding is None or a Sounding whose tables fit its batch (and `batch` / `device`, where the caller knows them)"""
    if sounding is None:
        return
    if not isinstance(sounding, Sounding):
        raise ValueError('sounding must be what DisentangleVAE.sounding(...) returns, got %r' % (type(sounding).__name__,))
    B = sounding.batch
    c = sounding.control
    if not torch.is_tensor(c) or c.device.type != 'cuda' or c.dtype != torch.int32 or tuple(c.shape) != (1,):
        raise ValueError('sounding.control must be an int32 device tensor [1]')
    for name, t_ in zip(('max_sounding', 'min_sounding', 'steps'), sounding.tables()):
        if (not torch.is_tensor(t_) or t_.device != c.device or t_.dtype != torch.uint8 or t_.dim() != 2 or t_.shape[1] != 32
                or t_.shape[0] not in (1, B) or not t_.is_contiguous()):
            raise ValueError('sounding.%s must be a contiguous uint8 tensor [1, 32] or [%d, 32] on the device of its control word' % (name, B))
    if batch is not None and B != batch:
        raise ValueError('sounding was built for a batch of %d, the decoded batch has %d rows' % (B, batch))
    if device is not None and c.device != device:
        raise ValueError('sounding is on %s, the decode on %s' % (c.device, device))


class SoundingRun:
    """what ONE decode with a Sounding reads and writes: the rules `snd`, the base tables (mask_base int32 [rows, 32, 4] / force_base int32
    [15, 32 B], or None), the state rem uint8 [B, 128], and the outputs mask_eff int32 [B, 32, 4] / force_eff int32 [15, 32 B] (each None
    where that rule is off) and held int32 [B, 32].  The note loop is handed the effective arrays; step() is the launch between two of
    them.  Nothing is zeroed here: ptv_sounding_step(-1) initialises the state"""

    def __init__(self, snd, B, dev, mask=False, mask_base=None, force=False, force_base=None):
        i32 = dict(dtype=torch.int32, device=dev)
        self.snd, self.B = snd, B
        self.mask_base, self.force_base = (mask_base if mask else None), (force_base if force else None)
        self.rem = torch.empty(B, 128, dtype=torch.uint8, device=dev)
        self.held = torch.empty(B, 32, **i32)
        self.mask_eff = torch.empty(B, 32, 4, **i32) if mask else None
        self.force_eff = torch.empty(15, 32 * B, **i32) if force else None

    def step(self, xhat, t_done):
        """ptv_sounding_step on the current stream: everything of time step t_done + 1 (t_done = -1: step 0 and the zeroed state)"""
        s, mb = self.snd, self.mask_base
        call('ptv_sounding_step', ptr(xhat), t_done, self.B, ptr(mb), 1 if mb is None else mb.shape[0], ptr(self.force_base),
             ptr(s.max_sounding), s.max_sounding.shape[0], ptr(s.min_sounding), s.min_sounding.shape[0], ptr(s.steps), s.steps.shape[0],
             ptr(s.control), ptr(self.rem), ptr(self.mask_eff), ptr(self.force_eff), ptr(self.held), stream_ptr())

    def slots(self):
        """(the PTV_DFF_SND_* tensors, the PTV_DFF_D_SND* dims) of ptv_decoder_free_fwd"""
        s, mb = self.snd, self.mask_base
        return (dict(SND_MASK_BASE=mb, SND_FORCE_BASE=self.force_base, SND_MAX=s.max_sounding, SND_MIN=s.min_sounding, SND_STEPS=s.steps,
                     SND_CONTROL=s.control, SND_REM=self.rem, SND_MASK_EFF=self.mask_eff, SND_FORCE_EFF=self.force_eff, SND_HELD=self.held),
                dict(SND=1, SND_MASK_ROWS=1 if mb is None else mb.shape[0], SND_MAX_ROWS=s.max_sounding.shape[0],
                     SND_MIN_ROWS=s.min_sounding.shape[0], SND_STEPS_ROWS=s.steps.shape[0]))


def sounding_block(blk, mask_eff):
    """the block of a decode under a SoundingRun with a mask rule: a copy of `blk` whose mask address is mask_eff's and whose "one mask
    row" flag is clear (mask_eff has a row per sample); it carries mask_eff as its pitch_mask.  Device operations only"""
    out = clone_block(blk, mask_eff)
    out[6:7].bitwise_and_(~CONS_MASK_ROW1)
    out[7:8].copy_(torch.tensor([mask_eff.data_ptr()], dtype=torch.int64))
    return out


def split_voice(x, voice_steps, below=None, lowest=None, whole_steps=None):
    """the selection of build_keep_voice as two model grids (ptv_grid_split_voice) -> (x_voice, x_rest int64 [B, 32, 16, 6], kept_n int32
    [B, 32], err int32 [B]): per step the kept notes and what the decoder would re-draw, each a valid step"""
    return _split('ptv_grid_split_voice', *_voice_selection(x, voice_steps, below, lowest, whole_steps))


def check_keep(keep, batch=None):
    """ValueError unless keep is None or a Keep whose arrays fit its batch (and `batch`, the rows of the decode, where the caller knows them)"""
    if keep is None:
        return
    if not isinstance(keep, Keep):
        raise ValueError('keep must be what DisentangleVAE.keep(x, steps) returns, got %r' % (type(keep).__name__,))
    B = keep.batch
    for name, t_, shape in (('pitch', keep.pitch, (15, 32 * B)), ('dur', keep.dur, (5, 480 * B))):
        if (not torch.is_tensor(t_) or t_.device.type != 'cuda' or t_.dtype != torch.int32 or tuple(t_.shape) != shape
                or not t_.is_contiguous()):
            raise ValueError('keep.%s must be a contiguous int32 device tensor %s' % (name, list(shape)))
    if batch is not None and B != batch:
        raise ValueError('keep was built for a batch of %d, the decoded batch has %d rows' % (B, batch))


def _row_values(name, v, batch):
    """one rule argument of row_sampling_words as a list of `batch` host values: a scalar (or None) broadcast, a host sequence or numpy
    array of length batch taken element by element (numpy scalars become Python ones: the validators take those)"""
    if v is None or isinstance(v, (bool, int, float, np.generic)):
        v = [v] * batch
    elif isinstance(v, np.ndarray):
        v = v.tolist() if v.ndim == 1 else None
    elif torch.is_tensor(v) or isinstance(v, (str, bytes)) or not hasattr(v, '__len__'):
        v = None
    if v is None or len(v) != batch:
        raise ValueError('%s must be a scalar or a host sequence of %d values (one per row)' % (name, batch))
    return [x.item() if isinstance(x, np.generic) else x for x in v]


def row_sampling_words(batch, temperature, dur_temperature=None, top_k=None, min_p=None, top_p=None, sample_id=None, sample_offset=0):
    """the row table of a row-wise decode as a host numpy int32 [batch, 8] (INTEGRATION.md "Per-row sampling"); touches no GPU.  Each of
    the five rule arguments is a scalar (every row alike) or a host sequence / numpy array of `batch` values; None, or a None element,
    is what it is for the scalar block (no temperature: 0; no rule).  Row b holds {T_pitch, T_dur, top_k, ln_min_p, top_p_q24} exactly as
    check_sampling / check_truncation make them for b's values -- each distinct combination is validated once, and a ValueError is the
    scalar one prefixed with the row --, then 0 and the int64 sample_id.  sample_id: None (sample_offset + b, the scalar block's rule) or
    `batch` integers in [0, 2^47), the row's index in the Philox counter: a row reproduces alone in a scalar decode with that
    sample_offset"""
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise ValueError('batch must be an integer >= 1, got %r' % (batch,))
    cols = [_row_values(name, v, batch) for name, v in (('temperature', temperature), ('dur_temperature', dur_temperature),
                                                         ('top_k', top_k), ('min_p', min_p), ('top_p', top_p))]
    if sample_id is None:
        check_sampling(0.0, None, sample_offset)
        ids = [sample_offset + b for b in range(batch)]
    else:
        ids = _row_values('sample_id', sample_id, batch)
    out = np.zeros((batch, 8), dtype=np.int32)
    f32, i64, seen = out.view(np.float32), out.view(np.int64), {}
    for b, key in enumerate(zip(*cols)):
        try:
            tkey = tuple((type(x), x) for x in key)                # (2, 2.0 and True are equal as keys and not as values)
            rec = seen.get(tkey) if all(isinstance(x, (int, float, type(None))) for x in key) else None
            if rec is None:
                t, td, k, mp, pp = key
                tp_, td_ = check_sampling(t, td, top_k=k, min_p=mp, top_p=pp)[:2]
                rec = (tp_, td_) + (check_truncation(k, mp, pp) or (0, LN_MIN_P_OFF, 0))
                seen[tkey] = rec
            v = ids[b]
            if isinstance(v, bool) or not isinstance(v, int) or v < 0 or v >= SAMPLE_ID_TOP:
                raise ValueError('sample_id must be an integer in [0, 2^47), got %r' % (v,))
        except ValueError as e:
            raise ValueError('row %d: %s' % (b, e)) from None
        f32[b, 0], f32[b, 1], out[b, 2], f32[b, 3], out[b, 4], i64[b, 3] = rec[0], rec[1], rec[2], rec[3], rec[4], v
    return out


class RowSampling:
    """the row table of a row-wise decode on the device, for rows= (DisentangleVAE.row_sampling; INTEGRATION.md "Per-row sampling"):
    table (int32 device tensor [batch, 8], row_sampling_words' layout), batch, and sample_offset, the default of update()"""

    def __init__(self, table, batch, sample_offset=0):
        self.table, self.batch, self.sample_offset = table, batch, sample_offset

    def __iter__(self):
        return iter((self.table, self.batch))

    def update(self, temperature, dur_temperature=None, top_k=None, min_p=None, top_p=None, sample_id=None, sample_offset=None):
        """new parameters into the SAME device tensor (one host-to-device copy): a captured graph, or a block made before, sees them.
        A bad value is a ValueError that leaves the table as it was"""
        words = row_sampling_words(self.batch, temperature, dur_temperature, top_k, min_p, top_p, sample_id,
                                   self.sample_offset if sample_offset is None else sample_offset)
        self.table.copy_(torch.from_numpy(words))
        return self

    def tiled(self, n):
        """the table of the batch repeated n times (decode_best_of): candidate k of row b is row k * batch + b and draws as sample
        sample_id[b] + k * batch -- with default ids the scalar block's rule; ids past 2^47 are the caller's to avoid"""
        t = self.table.repeat(n, 1)
        t.view(torch.int64)[:, 3] += (torch.arange(n, device=t.device) * self.batch).repeat_interleave(self.batch)
        return RowSampling(t, n * self.batch, self.sample_offset)


def check_rows(rows, batch=None, device=None):
    """ValueError unless rows is None or a RowSampling whose table fits its batch (and `batch` / `device`, where the caller knows them)"""
    if rows is None:
        return
    if not isinstance(rows, RowSampling):
        raise ValueError('rows must be what DisentangleVAE.row_sampling(batch, ...) returns, got %r' % (type(rows).__name__,))
    t_ = rows.table
    if (not torch.is_tensor(t_) or t_.device.type != 'cuda' or t_.dtype != torch.int32 or tuple(t_.shape) != (rows.batch, 8)
            or not t_.is_contiguous() or t_.data_ptr() % 16):
        raise ValueError('rows.table must be a contiguous, 16-byte aligned int32 device tensor [%d, 8]' % (rows.batch,))
    if batch is not None and rows.batch != batch:
        raise ValueError('rows was built for a batch of %d, the decoded batch has %d rows' % (rows.batch, batch))
    if device is not None and t_.device != device:
        raise ValueError('rows.table is on %s, the decode on %s' % (t_.device, device))


def sampling_words(temperature, dur_temperature=None, seed=7, draw=0, sample_offset=0, *, top_k=None, min_p=None, top_p=None,
                   pitch_mask=None, ascending=None, rows=None):
    """the block as four int64 words (host list); six with top_k / min_p / top_p; eight with pitch_mask / ascending (the last word is
    the address of pitch_mask as given: the caller keeps that tensor alive and contiguous -- sampling_block does); ten with rows (a
    RowSampling: the ninth word is the address of its table, and the scalars it replaces must be left out -- the block then holds
    temperatures 0, no rule and sample offset 0)"""
    if rows is not None:
        check_rows(rows)
        if any(v is not None for v in (temperature, dur_temperature, top_k, min_p, top_p)) or sample_offset:
            raise ValueError('rows carries temperature, dur_temperature, top_k, min_p, top_p and the sample ids of every row: '
                             'leave the scalar keywords out')
        temperature = 0.0
    tp, td, off, seed, draw = check_sampling(temperature, dur_temperature, sample_offset, seed, draw)
    words = [seed - (1 << 64) if seed >= (1 << 63) else seed, draw, off, struct.unpack('<q', struct.pack('<ff', tp, td))[0]]
    tr = check_truncation(top_k, min_p, top_p)
    flags = check_constraints(pitch_mask, ascending)
    if rows is not None and flags is None:
        flags = 0
    if flags is not None and tr is None:
        tr = (0, LN_MIN_P_OFF, 0)
    if tr is not None:
        words += [struct.unpack('<q', struct.pack('<if', *tr[:2]))[0], tr[2]]
    if flags is not None:
        if pitch_mask is not None and not pitch_mask.is_contiguous():
            raise ValueError('pitch_mask must be contiguous')
        words += [flags, 0 if pitch_mask is None else pitch_mask.data_ptr()]
    if rows is not None:
        words += [rows.table.data_ptr(), 0]
    return words


def sampling_block(device, temperature=None, dur_temperature=None, seed=7, draw=0, sample_offset=0, *, top_k=None, min_p=None, top_p=None,
                   pitch_mask=None, ascending=None, rows=None):
    """the device block of a sampled decode: PtvaeDecoder.decoder(..., sampling=block).  Four int64 words; six with top_k / min_p /
    top_p (truncated sampling, INTEGRATION.md "Sampled decode"); eight with pitch_mask / ascending (INTEGRATION.md "Constrained
    decode"; temperature 0 is then the constrained argmax).  The word count selects the kernels.  An eight-word block carries the mask
    it points at as its attribute `pitch_mask` (None without one): that keeps the mask alive, and tells the decoder its row count; ten
    with rows (a RowSampling; INTEGRATION.md "Per-row sampling"), which the block carries as its attribute `rows`"""
    if pitch_mask is not None and torch.is_tensor(pitch_mask):
        pitch_mask = pitch_mask.contiguous()
    words = sampling_words(temperature, dur_temperature, seed, draw, sample_offset, top_k=top_k, min_p=min_p, top_p=top_p,
                           pitch_mask=pitch_mask, ascending=ascending, rows=rows)
    if torch.device(device).type != 'cuda':
        raise RuntimeError('a sampled decode runs on the GPU: the sampling block lives in device memory (got device %s)' % (device,))
    blk = make_block(words, pitch_mask, device, rows)
    if pitch_mask is not None and pitch_mask.device != blk.device:
        raise ValueError('pitch_mask is on %s, the block on %s' % (pitch_mask.device, blk.device))
    check_rows(rows, device=blk.device)
    return blk


def make_block(words, pitch_mask, device, rows=None):
    """validated host words (sampling_words) and the contiguous mask their eighth word points at -> the device block; the eight-word form
    gets the mask as its attribute, and its ascending flag as the host bool `ascending`; the ten-word form also the RowSampling whose
    table its ninth word points at, as `rows`"""
    blk = torch.tensor(words, dtype=torch.int64, device=device)
    if len(words) >= CONSTRAINED.words:
        blk.pitch_mask = pitch_mask
        blk.ascending = bool(words[6] & 1)
    if len(words) == ROWWISE.words:
        blk.rows = rows
    return blk


def clone_block(blk, pitch_mask=None):
    """a copy of a block (clone() alone drops the attributes); an eight-word copy carries `pitch_mask`, or the original's when none is
    given, and `ascending`; a ten-word copy also `rows`"""
    out = blk.clone()
    if hasattr(blk, 'pitch_mask'):
        out.pitch_mask = blk.pitch_mask if pitch_mask is None else pitch_mask
        out.ascending = getattr(blk, 'ascending', False)
    if hasattr(blk, 'rows'):
        out.rows = blk.rows
    return out


def _check_block(sampling, dev, B=None):
    if not (torch.is_tensor(sampling) and sampling.dtype == torch.int64 and sampling.is_contiguous() and sampling.device == dev):
        raise ValueError('sampling must be a block made by functional_free.sampling_block() on the device of z')
    if block_kind(sampling).cons:
        if not hasattr(sampling, 'pitch_mask'):
            raise ValueError('a constrained block must come from functional_free.sampling_block(): it carries the mask it points at')
        mask = sampling.pitch_mask
        if mask is not None and (mask.device != dev or (B is not None and mask.shape[0] not in (1, B))):
            raise ValueError('pitch_mask has %d rows on %s, the decoded batch has %s rows on %s' % (mask.shape[0], mask.device, B, dev))
    if block_kind(sampling).rows:
        if getattr(sampling, 'rows', None) is None:
            raise ValueError('a row-wise block must come from functional_free.sampling_block(rows=...): it carries the table it points at')
        check_rows(sampling.rows, B, dev)
    return sampling


NOTE_CLUSTER4_MAX_WGS = 0      # 0 = the CU count
NOTE_CLUSTER8 = os.environ.get('PTV_NOTE_CLUSTER8', '1') != '0'
_NCU = []


def _num_cu():
    if not _NCU:
        _NCU.append(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    return _NCU[0]


def note_loop_cluster(B, ncu=None):
    """members per 16-sample panel of the note loop's cluster mode (0 = off) on a device of `ncu` compute units (None: the current one)"""
    panels = (B + 15) // 16
    ncu = _num_cu() if ncu is None else ncu
    # round 6: from 96 panels on the 8-wave producer / head kernel used to take over; with the head weights resident and the state exchange
    # flag-in-data, two members per panel on the 4-wave kernel win up to one member per CU (B = 2048: 34.9 vs 41.7 us per note step)
    if NOTE_LOOP_SPLIT or (NOTE_LOOP_SPLIT is None and panels >= 96 and panels * 2 > ncu):
        return 0
    if NOTE_LOOP_CLUSTER is not None:
        return NOTE_LOOP_CLUSTER if NOTE_LOOP_CLUSTER in (2, 4, 8) and panels * NOTE_LOOP_CLUSTER <= ncu else 0
    if NOTE_CLUSTER8 and panels * 8 <= ncu:
        return 8                 # round 6: eight members per panel (B <= 512 on 256 CUs): each streams an eighth of the gate weights
    # round 4: four members per panel up to ONE MEMBER PER CU (64 panels = B 1024, the per-GPU batch of BASELINE configs[4]); it was capped at
    # half the chip.  Free-running training, same box, S = 2 -> 4: B = 640 21.4k -> 23.8k samples/s, 768 23.4k -> 26.5k, 1024 27.2k -> 30.6k
    cap4 = NOTE_CLUSTER4_MAX_WGS if NOTE_CLUSTER4_MAX_WGS > 0 else ncu
    return 4 if panels * 4 <= cap4 else (2 if panels * 2 <= ncu else 0)


def cluster_bits(c):
    """the cluster size in ptv_free_note_loop's `train` word: bits 18-20 = 2 / 4, bit 22 = eight members"""
    return 0x400000 if c == 8 else (c << 18)


def note_loop_word(train, replay, split, cluster, kind=ARGMAX):
    """ptv_free_note_loop's `train` word: 2 = the replayed training forward (decisions, logits and fed tokens only), else the train flag;
    split = NOTE_LOOP_SPLIT; the cluster size; the kind's sampling bits (the composite takes the word without them: they travel as dims)"""
    return (2 if replay else int(train)) | (0 if split is None else (0x20000 if split else 0x10000)) | cluster_bits(cluster) | kind.bits


def coin_masks(coins, inference):
    """the teacher-forcing coins as the kernels take them -> (32 words: bit n = note coin n of the time step, 31 bytes: the time coins),
    as the C arrays ptv_decoder_free_fwd reads; all zero at inference"""
    masks, time = (ctypes.c_uint * 32)(), (ctypes.c_ubyte * 31)()
    if not inference:
        masks[:] = [sum(int(bool(c)) << n for n, c in enumerate(row[:14])) for row in coins[0]]
        time[:] = [int(bool(c)) for c in coins[1]]
    return masks, time


FreePlan = collections.namedtuple('FreePlan', 'train fast comp replay need_resum cluster capturing kind state16 ns16')


def _free_plan(prec, dims, z_dtype, coins, inference, needs_grad, forced, kind, ncu, capturing):
    """the path one DecoderStepFn.forward takes, decided once before anything is allocated or launched -> FreePlan: train (the backward's
    state is saved), fast (the persistent kernels of csrc/freerun.hip), comp (all of it behind ptv_decoder_free_fwd), replay (the loop
    stores decisions and tokens only, a batched recompute leaves what the backward reads), need_resum (a time token is re-summarised
    from predicted notes), cluster (members per panel of the note loop, 0 = off), capturing, kind (BlockKind), state16 / ns16 (bf16
    copies of the note and duration states / of the time states exist).  forced: force arrays were given; ncu, capturing: device facts"""
    B, R, E, He, Ht, Hn, Hd, NP = dims
    train = (not inference) and needs_grad
    fast = free_persist_ok(prec, E, He, Hn, Hd, NP) and (not train or F_._act_dtype(prec, Hn) == torch.bfloat16)
    ns16 = fast and Ht % 8 == 0                              # ... operands of the time GRU / the per-step products in the loop
    state16 = fast and train                                 # MFMA operands of the batched backward
    # the persistent path as ONE library call (ptv_decoder_free_fwd): then nothing is launched from Python before that call
    comp = FREE_COMPOSITE and ns16 and z_dtype == torch.float32
    replay = (state16 and FREE_REPLAY and F_.notes_persist_ok(prec, Hn, E) and Hd == 64 and F_.FUSED_DUR and ns16 and not forced)
    need_resum = inference or not all(coins[1])
    cluster = note_loop_cluster(B, ncu) if fast else 0
    if capturing and torch.is_grad_enabled():
        cluster = 0              # a captured training forward replays next to other streams' persistent launches, unordered with them
    return FreePlan(train, fast, comp, replay, need_resum, cluster, capturing, kind, state16, ns16)


_PACKS = F_.PackCache()
_PACK_SRC = ('dec_notes_gru.weight_hh_l0', 'dec_notes_gru.weight_ih_l0', 'pitch_out_linear.weight', 'dur_hid_linear.weight',
             'dec_dur_gru.weight_hh_l0', 'note_embedding.weight', 'dec_notes_emb_gru.weight_ih_l0', 'dec_notes_emb_gru.weight_hh_l0',
             'dec_notes_emb_gru.weight_ih_l0_reverse', 'dec_notes_emb_gru.weight_hh_l0_reverse', 'dec_time_to_notes_hid.weight',
             'dec_time_to_notes_hid.bias', 'dec_notes_gru.bias_ih_l0')


def free_persist_ok(prec, E, He, Hn, Hd, NP):
    return FREE_PERSIST and prec == 1 and F_.BF16_STORAGE and (E, He, Hn, Hd, NP) == (128, 128, 512, 64, 130)


def _pack(w2d, K=None, pairs=False):
    """fp32 [N, >=K] (any row stride) -> MFMA B-fragment-major bf16 (ptv_pack_mfma_b)"""
    N = w2d.shape[0]
    K = w2d.shape[1] if K is None else K
    out = torch.empty(lib().ptv_pack_mfma_b_size(N, K), device=w2d.device, dtype=torch.bfloat16)
    call('ptv_pack_mfma_b', ptr(w2d), w2d.stride(0), N, K, ptr(out), int(pairs), stream_ptr())
    return out


def _free_packs(P, Ht):
    """fragment-major bf16 copies of the weights the persistent step-loop kernels stream, re-packed when a parameter changed
    (in-place version counters + the fused optimiser's step count, like the bf16 weight shadows of optim.py)"""
    from .optim import _SHADOW_OF
    src = [P[n] for n in _PACK_SRC]
    ent = _SHADOW_OF.get(src[0].data_ptr())
    opt = ent[0]() if ent is not None else None
    stamp = (sum(p._version for p in src), opt.step_count if opt is not None else -1, opt._dirty if opt is not None else -1)
    hit = _PACKS.get(src, stamp)
    if hit is not None:
        return hit
    w_ih_n, w_dh, w_emb = P['dec_notes_gru.weight_ih_l0'], P['dur_hid_linear.weight'], P['note_embedding.weight']
    w_embT = torch.empty(w_emb.shape[1], w_emb.shape[0], device=w_emb.device, dtype=torch.float32)
    call('ptv_transpose01', ptr(w_embT), ptr(w_emb), w_emb.shape[0], w_emb.shape[1], 1, stream_ptr())
    pk = dict(wg_h=_pack(P['dec_notes_gru.weight_hh_l0']), wg_t=_pack(w_ih_n[:, Ht:]), wp=_pack(P['pitch_out_linear.weight']),
              wd_h=_pack(w_dh[:, :512]), wd_p=_pack(w_dh[:, 512:]), wdur=_pack(P['dec_dur_gru.weight_hh_l0']), w_embT=w_embT,
              e_ih=_pack(P['dec_notes_emb_gru.weight_ih_l0']), e_hh=_pack(P['dec_notes_emb_gru.weight_hh_l0']),
              e_ih_r=_pack(P['dec_notes_emb_gru.weight_ih_l0_reverse']), e_hh_r=_pack(P['dec_notes_emb_gru.weight_hh_l0_reverse']),
              w_cat=torch.cat([P['dec_time_to_notes_hid.weight'], w_ih_n[:, :Ht]], 0).to(torch.bfloat16).contiguous(),
              b_cat=torch.cat([P['dec_time_to_notes_hid.bias'], P['dec_notes_gru.bias_ih_l0']], 0).contiguous())
    return _PACKS.put(src, stamp, pk)


def gru_step(prec, hprev, gi, gi_ld, w_hh, b_hh, hout, *, gi2=None, gates=None, plane=0, lengths=None, t=0, gi_idx=None, hout16=None,
             hprev16=None):
    """one GRU cell on a window of rows; with a bf16 copy of the previous state (hprev16) the weight may be its bf16 shadow"""
    M, H = hout.shape
    if hprev16 is None and w_hh.dtype == torch.bfloat16:
        raise ValueError('a bf16 weight shadow needs the bf16 copy of the previous state')
    call('ptv_gru_step_fwd', prec, M, H, ptr(hprev), hprev.stride(0), ptr(hprev16), ptr(hout16), ptr(gi), gi_ld, ptr(gi2),
         gi2.stride(0) if gi2 is not None else 0, ptr(w_hh), ptr(b_hh), ptr(hout), hout.stride(0), ptr(gates), plane,
         ptr(lengths), t, ptr(gi_idx), F_._gru_flags(gates, gi, gi2, w=w_hh), stream_ptr())


# ---------------------------------------------------------------------------------------------
# The host pointer arrays of ptv_free_note_loop and ptv_free_resummarize, slot by slot in the order of include/ptvae_hip.h (the header is
# the authority; tests/test_gpu_freerun_kernels.py states the order a second time, by hand).
# ---------------------------------------------------------------------------------------------
NOTE_W = ('WG_H', 'WG_T', 'WP', 'WD_H', 'WD_P', 'WDUR', 'B_HH_N', 'B_P', 'B_DH', 'B_HH_D', 'TAB0', 'TAB', 'W_OUT_D', 'B_OUT_D', 'W_EMBT',
          'B_EMB')
NOTE_IO = ('GC', 'EMB', 'HN', 'GATES_N', 'PITCH', 'HD', 'GATES_D', 'DUR', 'IDX', 'TOK', 'PRED', 'XHAT', 'PLEN', 'FORCE_PITCH', 'FORCE_DUR',
           'HN16', 'HD16', 'RESERVED17', 'H0GC', 'XCH', 'CNT', 'BLOCK')       # BLOCK: the sampling block, present only in a sampled decode
RESUM_W = ('E_IH', 'E_HH', 'E_IH_R', 'E_HH_R', 'B_IH', 'B_HH', 'B_IH_R', 'B_HH_R')
RESUM_IO = ('PRED', 'PLEN', 'XH0', 'XH1', 'XG0', 'XG1', 'TOK_OUT')


def _slot_array(names, slots):
    unknown = [n for n in slots if n not in names]
    if unknown:
        raise TypeError('no slot named %s; the slots are %s' % (', '.join(unknown), ', '.join(names)))
    return F_._parr([slots.get(n) for n in names])


def dur_tabs(P, dev):
    """(tab0 [1, 3 Hd], tab [2, 3 Hd]): the duration GRU's input side for <sos> and for the two one-hot tokens, in fp32"""
    w_ih_d, b_ih_d = P['dec_dur_gru.weight_ih_l0'], P['dec_dur_gru.bias_ih_l0']
    return (gemm(P['dur_sos_token'].view(1, -1), w_ih_d, bias=b_ih_d, prec=0), gemm(_onehot2x5(dev), w_ih_d, bias=b_ih_d, prec=0))


def note_loop_weights(P, pk, tab0, tab):
    """ptv_free_note_loop's w (NOTE_W) from the parameters, the packs of _free_packs and dur_tabs"""
    return _slot_array(NOTE_W, dict(
        WG_H=pk['wg_h'], WG_T=pk['wg_t'], WP=pk['wp'], WD_H=pk['wd_h'], WD_P=pk['wd_p'], WDUR=pk['wdur'], B_HH_N=P['dec_notes_gru.bias_hh_l0'],
        B_P=P['pitch_out_linear.bias'], B_DH=P['dur_hid_linear.bias'], B_HH_D=P['dec_dur_gru.bias_hh_l0'], TAB0=tab0, TAB=tab,
        W_OUT_D=P['dur_out_linear.weight'], B_OUT_D=P['dur_out_linear.bias'], W_EMBT=pk['w_embT'], B_EMB=P['note_embedding.bias']))


def resum_weights(P, pk):
    """ptv_free_resummarize's w (RESUM_W) from dec_notes_emb_gru's biases and the packs of _free_packs"""
    return _slot_array(RESUM_W, dict(
        E_IH=pk['e_ih'], E_HH=pk['e_hh'], E_IH_R=pk['e_ih_r'], E_HH_R=pk['e_hh_r'], B_IH=P['dec_notes_emb_gru.bias_ih_l0'],
        B_HH=P['dec_notes_emb_gru.bias_hh_l0'], B_IH_R=P['dec_notes_emb_gru.bias_ih_l0_reverse'],
        B_HH_R=P['dec_notes_emb_gru.bias_hh_l0_reverse']))


def note_loop_io(BLOCK=None, **slots):
    """ptv_free_note_loop's io by slot name (NOTE_IO): 21 pointers, a slot not given is NULL; the sampling block is the 22nd when given"""
    return _slot_array(NOTE_IO[:21] if BLOCK is None else NOTE_IO, slots if BLOCK is None else dict(slots, BLOCK=BLOCK))


def resum_io(**slots):
    """ptv_free_resummarize's io by slot name (RESUM_IO); a slot not given is NULL"""
    return _slot_array(RESUM_IO, slots)


class FreeBuffers:
    """What one step-loop forward allocates, by its plan (fills and allocations only, nothing is launched through the library):
    NS [33,B,Ht] / HN [16,R,Hn] / HD [6,M,Hd] states with their bf16 copies NS16 / HN16 / HD16 (or None), the time tokens TOKS, the gates
    gates_t / gates_n / gates_d (training), the fed and predicted note tokens TOK / PRED, the outputs pitch, dur, idx and xhat (filled with
    padding rows behind <sos>), plen (zero), the re-summarisation's XH / XG / XH16 per direction (XH None: no token is re-summarised), the
    cluster mode's exchange words xch and counters xcnt (zero, or None), sos_emb (inference) and z_in / zg, which the prologue allocates
    when the forward is not the composite.  dims: the plan's eight, then Zi"""

    def __init__(self, plan, dims, prec, inference, dev):
        B, R, E, He, Ht, Hn, Hd, NP, Zi = dims
        M, bf16, train = 15 * R, torch.bfloat16, plan.train
        self.dims = dims[:8]
        self.NS = _empty(33, B, Ht, dev=dev)
        self.TOKS = _empty(33, B, 2 * He, dev=dev)
        self.z_in, self.zg = (_empty(B, Zi, dev=dev), _empty(B, 3 * Ht, dev=dev)) if plan.comp else (None, None)
        self.gates_t = _empty(32, 4, B, Ht, dev=dev, dtype=F_._act_dtype(prec, Ht)) if train else None
        self.HN = _empty(16, R, Hn, dev=dev)
        self.gates_n = _empty(15, 4, R, Hn, dev=dev, dtype=F_._act_dtype(prec, Hn)) if train else None
        self.TOK = _empty(15, R, E, dev=dev)
        self.xhat = torch.full((B, 32, 16, 6), 2, device=dev, dtype=torch.long)
        self.xhat[:, :, :, 0] = 130
        self.xhat[:, :, 0, 0] = 128
        self.plen = torch.zeros(R, device=dev, dtype=torch.int32)
        # the persistent note loop writes every slot of PRED, and its heads read row-padded logits
        self.PRED = _empty(16, R, E, dev=dev) if plan.fast else _zeros(16, R, E, dev=dev)
        self.pitch = _empty(M, F_._pad8(NP), dev=dev)[:, :NP] if plan.fast else _empty(M, NP, dev=dev)
        self.HD = _empty(6, M, Hd, dev=dev)
        # (the batched recompute's duration GRU saves no gates: csrc/dur_bwd.hip rebuilds them)
        self.gates_d = (_empty(5, 4, M, Hd, dev=dev, dtype=F_._act_dtype(prec, Hd))
                        if train and not (plan.replay and F_.DUR_RECOMPUTE) else None)
        self.idx = torch.empty(5, M, device=dev, dtype=torch.int32)
        self.dur = _empty(M, 5, 2, dev=dev)
        self.sos_emb = _empty(16, 32, 1, E, dev=dev) if inference else None
        # bf16 state copies: MFMA operands of the batched backward, and of the time GRU / the per-step products in the loop
        self.HN16 = _empty(16, R, Hn, dev=dev, dtype=bf16) if plan.state16 else None
        self.HD16 = _empty(6, M, Hd, dev=dev, dtype=bf16) if plan.state16 else None
        self.NS16 = _empty(33, B, Ht, dev=dev, dtype=bf16) if plan.ns16 else None
        self._resum_buffers(plan, prec, dev)
        self._cluster_buffers(plan, dev)

    def _resum_buffers(self, plan, prec, dev):
        R, He, bf16 = self.dims[1], self.dims[3], torch.bfloat16
        self.XH = self.XG = None
        self.XH16 = [None, None]
        if plan.need_resum and plan.replay:                      # the batched recompute writes every row of every slot but slot 0
            self.XH = [_empty(17, R, He, dev=dev) for _ in range(2)]
            for d in range(2):
                self.XH[d][0].zero_()
            self.XG = [_empty(16, 4, R, He, dev=dev, dtype=bf16) for _ in range(2)]
            self.XH16 = [_empty(17, R, He, dev=dev, dtype=bf16) for _ in range(2)]
        elif plan.need_resum:
            self.XH = [_zeros(17, R, He, dev=dev) for _ in range(2)]
            self.XG = ([torch.zeros(16, 4, R, He, device=dev, dtype=F_._act_dtype(prec, He)) for _ in range(2)] if plan.train
                       else [None, None])

    def _cluster_buffers(self, plan, dev):
        self.xch = self.xcnt = None
        if plan.cluster:
            global LAST_CLUSTER_COUNTERS
            panels, Hn, bf16 = (self.dims[0] + 15) // 16, self.dims[5], torch.bfloat16
            self.xch = torch.zeros(panels * 2 * 16 * Hn * 2, device=dev, dtype=bf16)   # 8-byte words {2 units, step tag}: tag 0 = nothing sent yet
            self.xcnt = torch.zeros(panels + 1, device=dev, dtype=torch.int32)         # arrival counters of t = 0..31 + error word
            LAST_CLUSTER_COUNTERS = self.xcnt        # (tests: every panel counts 32 * 15 * S arrivals, the error word stays 0)
            F_._CLUSTER_SYNC.append(self.xcnt)
            if len(F_._CLUSTER_SYNC) > 64:
                del F_._CLUSTER_SYNC[:32]

    def saved(self):
        """the tensors of DecoderStepState, by its keyword names"""
        return {n: getattr(self, n) for n in ('NS', 'NS16', 'z_in', 'TOKS', 'gates_t', 'HN', 'HN16', 'gates_n', 'pitch', 'HD', 'HD16', 'gates_d',
                                              'idx', 'TOK', 'PRED', 'xhat', 'XH', 'XG', 'XH16', 'plen')}

    def note_io(self, inp, **more):
        """the note loop's io over these buffers; the caller adds GC or H0GC, and the BLOCK of a sampled decode"""
        return note_loop_io(EMB=inp.emb3, HN=self.HN, GATES_N=self.gates_n, PITCH=self.pitch, HD=self.HD, GATES_D=self.gates_d, DUR=self.dur,
                            IDX=self.idx, TOK=self.TOK, PRED=self.PRED, XHAT=self.xhat, PLEN=self.plen, FORCE_PITCH=inp.force_pitch,
                            FORCE_DUR=inp.force_dur, HN16=self.HN16, HD16=self.HD16, XCH=self.xch, CNT=self.xcnt, **more)

    def resum_io(self, tok_out=None):
        """the re-summarisation's io over these buffers"""
        return resum_io(PRED=self.PRED, PLEN=self.plen, XH0=self.XH[0], XH1=self.XH[1], XG0=self.XG[0], XG1=self.XG[1], TOK_OUT=tok_out)


# what a step-loop forward was called with, beside the parameters: emb3 = the ground-truth embedding as [16, R, E] or None, coins as given,
# masks / time_coins = coin_masks(coins), force_pitch [15, R] / force_dur [5, 15 R] int32 or None, sampling = the block or None
# sounding = the SoundingRun of a decode with sounding rules (force_pitch / the block's mask are then its EFFECTIVE arrays) or None
FreeInputs = collections.namedtuple('FreeInputs', 'z emb3 xs coins masks time_coins force_pitch force_dur sampling inference prec sounding',
                                    defaults=(None,))
# the packs and tables of a step-loop forward: tok0 / tok0_lds = the first note token of every time step and its row stride (0: one <sos>
# row), dur_tabs, the MFMA operands of the time GRU and of the per-step products (bf16 shadows on the persistent path), wE =
# dec_notes_emb_gru's eight, and on the persistent path pk = _free_packs, wl / wr = note_loop_weights / resum_weights
FreeTables = collections.namedtuple('FreeTables', 'tok0 tok0_lds tab0 tab w_hh_t w_ih_t16 w_tn16 w_ih_n16 wE pk wl wr')


def _free_branches(plan, prec, dims, gates_d_dtype):
    """(notes, heads, dur) of the DecoderStepState a forward by this plan leaves: the batched recompute ran the row kernel; the loop's own
    heads and duration steps leave what csrc/heads.hip / csrc/dur_bwd.hip take back wherever the bf16 copies exist.  gates_d_dtype: None when
    no duration gates are saved"""
    Hn, Hd, NP = dims[5], dims[6], dims[7]
    s16 = plan.state16 or None
    dur_fused = F_.dur_bwd_fusable(prec, Hd, None) and gates_d_dtype in (None, torch.bfloat16)
    return ('rows' if plan.replay else 'step', 'fused' if F_.heads_ok(prec, Hn, NP, Hd, s16, s16) else 'gemm',
            'fused16' if plan.state16 else 'fused' if dur_fused else 'step')


def _free_prologue(P, buf, z, prec):
    """what does not depend on the loop: the first time state, the z part of the time GRU's input side, the first time token"""
    w_ih_t = P['dec_time_gru.weight_ih_l0']
    gemm(z, P['z2dec_hid_linear.weight'], buf.NS[0], bias=P['z2dec_hid_linear.bias'], prec=prec)
    buf.z_in = gemm(z, P['z2dec_in_linear.weight'], bias=P['z2dec_in_linear.bias'], prec=prec)
    buf.zg = gemm(buf.z_in, w_ih_t[:, 2 * buf.dims[3]:], bias=P['dec_time_gru.bias_ih_l0'], prec=prec)
    copy2d(buf.TOKS[0], P['dec_init_input'].view(1, -1), lds=0)


def _free_tables(plan, P, buf, inp):
    """FreeTables of a forward; what it launches -- the <sos> embedding at inference, dur_tabs, the bf16 copy of the first time state
    when the forward is not the composite, packs and shadows that are out of date -- reads no buffer but NS[0]"""
    B, R, E, He, Ht, Hn, Hd, NP = buf.dims
    prec, dev, st = inp.prec, inp.z.device, stream_ptr()
    if inp.inference:
        call('ptv_embed_fwd', ptr(_sos_grid(dev)), ptr(P['note_embedding.weight']), ptr(P['note_embedding.bias']), ptr(buf.sos_emb), None, 1,
             E, st)
        tok0, tok0_lds = buf.sos_emb.view(-1, E)[0:1], 0
    else:
        tok0, tok0_lds = inp.emb3[0], E
    tab0, tab = dur_tabs(P, dev)
    if plan.ns16 and not plan.comp:
        call('ptv_cast_bf16', ptr(buf.NS[0]), ptr(buf.NS16[0]), B * Ht, st)
    # per time step the loop runs four M = B products whose cost is reading the weights: their bf16 shadows halve it
    w_ih_t, w_tn, w_ih_n = P['dec_time_gru.weight_ih_l0'], P['dec_time_to_notes_hid.weight'], P['dec_notes_gru.weight_ih_l0']
    w_hh_t = F_._W(P['dec_time_gru.weight_hh_l0'], prec) if plan.ns16 else P['dec_time_gru.weight_hh_l0']
    ops = (F_._W(w_ih_t, prec), F_._W(w_tn, prec), F_._W(w_ih_n, prec)) if plan.fast else (w_ih_t, w_tn, w_ih_n)
    pk = _free_packs(P, Ht) if plan.fast else None
    return FreeTables(tok0, tok0_lds, tab0, tab, w_hh_t, *ops, [P['dec_notes_emb_gru.' + n] for n in EMB_GRU], pk,
                      note_loop_weights(P, pk, tab0, tab) if plan.fast else None, resum_weights(P, pk) if plan.fast else None)


def _composite_tensors(plan, P, buf, tbl, inp):
    """the DFF slots of ptv_decoder_free_fwd by name: buffers, inputs, parameters, packs, and the scratch of the call"""
    B, R, E, He, Ht, Hn, Hd, NP = buf.dims
    M, dev, pk = 15 * R, inp.z.device, tbl.pk
    XH, XG = buf.XH or [None, None], buf.XG or [None, None]
    t = dict(NS=buf.NS, NS16=buf.NS16, Z_IN=buf.z_in, ZG=buf.zg, TOKS=buf.TOKS, GATES_T=buf.gates_t, TOK=buf.TOK, PRED=buf.PRED,
             PITCH=buf.pitch, HN=buf.HN, HN16=buf.HN16, GATES_N=buf.gates_n, HD=buf.HD, HD16=buf.HD16, GATES_D=buf.gates_d, IDX=buf.idx,
             PLEN=buf.plen, XH0=XH[0], XH1=XH[1], XH16_0=buf.XH16[0], XH16_1=buf.XH16[1], XG0=XG[0], XG1=XG[1], TAB0=tbl.tab0, TAB=tbl.tab,
             SAMPLE=inp.sampling,                    # (the composite appends the block to the note loop's io itself)
             Z=inp.z, XS=inp.xs, TOK0_SRC=tbl.tok0, W_ZHID=P['z2dec_hid_linear.weight'], B_ZHID=P['z2dec_hid_linear.bias'],
             W_ZIN=P['z2dec_in_linear.weight'], B_ZIN=P['z2dec_in_linear.bias'], W_IH_T=P['dec_time_gru.weight_ih_l0'],
             B_IH_T=P['dec_time_gru.bias_ih_l0'], INIT_INPUT=P['dec_init_input'], B_HH_T=P['dec_time_gru.bias_hh_l0'],
             W_IH_T_OP=tbl.w_ih_t16, W_HH_T_OP=tbl.w_hh_t, W_CAT=pk['w_cat'], B_CAT=pk['b_cat'], GI=_empty(B, 3 * Ht, dev=dev),
             H0GC=_empty(B, 4 * Hn, dev=dev))
    if plan.replay:
        w_ih_n = P['dec_notes_gru.weight_ih_l0']
        pkn = F_.notes_packs(w_ih_n, P['dec_notes_gru.weight_hh_l0'], Ht)
        t.update(W_IH_N=w_ih_n, B_IH_N=P['dec_notes_gru.bias_ih_l0'], B_HH_N=P['dec_notes_gru.bias_hh_l0'], W_DH=P['dur_hid_linear.weight'],
                 B_DH=P['dur_hid_linear.bias'], W_HH_D=P['dec_dur_gru.weight_hh_l0'], B_HH_D=P['dec_dur_gru.bias_hh_l0'],
                 W_OUT_D=P['dur_out_linear.weight'], B_OUT_D=P['dur_out_linear.bias'], PK_NOTES_H=pkn['wg_h'], PK_NOTES_T=pkn['wg_t'],
                 GC16=_empty(R, 3 * Hn, dev=dev, dtype=torch.bfloat16), DUR_SCR=_empty(M, 10, dev=dev),
                 IDX_SCR=torch.empty(5, M, device=dev, dtype=torch.int32))
        if plan.need_resum:
            for d_ in range(2):
                w_ih_e, w_hh_e, b_ih_e, b_hh_e = tbl.wE[4 * d_: 4 * d_ + 4]
                pke = F_.notes_packs(w_ih_e, w_hh_e, 0)
                t.update({'PK_E_H%d' % d_: pke['wg_h'], 'PK_E_T%d' % d_: pke['wg_t'], 'B_HH_E%d' % d_: b_hh_e, 'B_IH_E%d' % d_: b_ih_e})
    return t


def _free_fwd_composite(plan, P, buf, tbl, inp):
    """the persistent path through ptv_decoder_free_fwd (one C call: prologue, loop and batched recompute); True when it ran"""
    B, R, E, He, Ht, Hn, Hd, NP = buf.dims
    if plan.replay:
        F_.zero_skip_sync()
    t = _composite_tensors(plan, P, buf, tbl, inp)
    cluster = int(bool(plan.cluster) and not plan.capturing)
    dvals = {'B': B, 'ZS': inp.z.shape[1], 'ZI': buf.z_in.shape[1], 'HE': He, 'HT': Ht, 'HN': Hn, 'HD': Hd, 'E': E, 'NP': NP,
                       'LDP': buf.pitch.stride(0), 'TRAIN': int(plan.train), 'REPLAY': int(plan.replay),
                       'INFERENCE': int(bool(inp.inference)),
                       'LOOP_FLAGS': note_loop_word(plan.train, plan.replay, NOTE_LOOP_SPLIT, plan.cluster), 'CLUSTER': cluster,
                       'RESUM_TRAIN': int(plan.train and not plan.replay), 'TOK0_LDS': tbl.tok0_lds,
                       'W_IH_T_BF16': tbl.w_ih_t16.dtype == torch.bfloat16, 'W_HH_T_BF16': tbl.w_hh_t.dtype == torch.bfloat16,
                       'SAMPLE_TRUNC': plan.kind.trunc, 'SAMPLE_CONS': plan.kind.cons, 'SAMPLE_ROWS': plan.kind.rows}
    if inp.sounding is not None:                            # (without it the call launches nothing new)
        snd_t, snd_d = inp.sounding.slots()
        t.update(snd_t)
        dvals.update(snd_d)
    dvals = _DFF.dims(dvals)
    masks, tc = inp.masks, inp.time_coins
    # the cluster-mode note loops take the persistent-launch turn (functional._PersistTurn): the library records again after the last one
    turn = F_._CompositeTurn(F_.cur_stream()) if cluster else None
    slots = _DFF.pointers(t, handles=turn.handles if turn else None)
    F_._chain_prio()
    rc = lib().ptv_decoder_free_fwd(slots, dvals, tbl.wl, buf.note_io(inp, H0GC=t['H0GC']), tbl.wr,
                                    buf.resum_io() if plan.need_resum else None, masks, tc, stream_ptr())
    if rc == -3:
        return False
    F_.check(rc, 'ptv_decoder_free_fwd')
    if turn:
        turn.taken()
    _DFF.count()
    _DFF_KEEP[:] = (t, masks, tc)                           # (the scratch tensors stay referenced until the next call)
    return True


def _first_tokens(buf, tbl):
    """the first note token of every time step is the <sos> embedding (ptvae.py:388-392): one copy for all 32 steps"""
    copy2d(buf.TOK[0], tbl.tok0, lds=tbl.tok0_lds)
    copy2d(buf.PRED[0], buf.TOK[0])


def _time_step(plan, P, buf, tbl, inp, t):
    """the time GRU's cell t -> the new time state as the note level's operand (its bf16 copy where one exists)"""
    B, He, Ht = buf.dims[0], buf.dims[3], buf.dims[4]
    NS, NS16 = buf.NS, buf.NS16
    gi = gemm(buf.TOKS[t], tbl.w_ih_t16[:, :2 * He], prec=inp.prec)
    gru_step(inp.prec, NS[t], gi, 3 * Ht, tbl.w_hh_t, P['dec_time_gru.bias_hh_l0'], NS[t + 1], gi2=buf.zg,
             gates=buf.gates_t[t] if plan.train else None, plane=B * Ht, hout16=NS16[t + 1] if NS16 is not None else None,
             hprev16=NS16[t] if NS16 is not None else None)
    return NS16[t + 1] if NS16 is not None else NS[t + 1]


def _next_time_token(plan, P, buf, tbl, inp, t):
    """TOKS[t + 1]: the ground-truth summary (time coin t), or the final states of dec_notes_emb_gru over the predicted notes of step t
    (ptvae.py:480-486) -- one persistent launch, or cell by cell"""
    B, R, E, He = buf.dims[:4]
    prec, rows = inp.prec, slice(t * B, (t + 1) * B)
    if inp.time_coins[t]:
        copy2d(buf.TOKS[t + 1], inp.xs[rows])
    elif plan.fast:
        call('ptv_free_resummarize', tbl.wr, buf.resum_io(buf.TOKS[t + 1]), B, t, int(plan.train and not plan.replay), stream_ptr())
    else:
        wE, XH, XG = tbl.wE, buf.XH, buf.XG
        PT = _empty(16, B * E, dev=inp.z.device)
        copy2d(PT, buf.PRED.view(16, R * E)[:, t * B * E:(t + 1) * B * E])
        for d in range(2):
            gi_e = gemm(PT.view(16 * B, E), wE[4 * d], bias=wE[4 * d + 2], prec=prec).view(16, B, 3 * He)
            for s_ in range(16):
                tt = 15 - s_ if d else s_
                gru_step(prec, XH[d][s_][rows], gi_e[tt], 3 * He, wE[4 * d + 1], wE[4 * d + 3], XH[d][s_ + 1][rows],
                         gates=XG[d][s_][:, rows] if plan.train else None, plane=R * He, lengths=buf.plen[rows], t=tt)
            copy2d(buf.TOKS[t + 1][:, d * He:(d + 1) * He], XH[d][16][rows])


def _free_fwd_persistent(plan, P, buf, tbl, inp):
    """the persistent kernels of csrc/freerun.hip sequenced from here: per time step the time GRU's cell, the initial notes-GRU state and
    the hoisted input part in ONE product against the stacked weights ([512 | 1536] rows: 256 blocks, no split-K, no zero fill), all 15
    note steps in ONE launch, and the next time token"""
    B, pk, st = buf.dims[0], tbl.pk, stream_ptr()
    word = note_loop_word(plan.train, plan.replay, NOTE_LOOP_SPLIT, plan.cluster, plan.kind)
    _first_tokens(buf, tbl)
    if inp.sounding is not None:
        inp.sounding.step(buf.xhat, -1)
    for t in range(32):
        ns = _time_step(plan, P, buf, tbl, inp, t)
        H0GC = gemm(ns, pk['w_cat'], bias=pk['b_cat'], prec=inp.prec)
        io = buf.note_io(inp, H0GC=H0GC, BLOCK=inp.sampling)
        # (cluster mode: the members of a panel spin on each other -- like every persistent launch it takes its turn, so that
        # it is never half-resident next to another spinning grid, e.g. the chord decoder's on its sibling stream)
        with (F_._PersistTurn() if plan.cluster and not plan.capturing else contextlib.nullcontext()):
            call('ptv_free_note_loop', tbl.wl, io, buf.pitch.stride(0), B, t, inp.masks[t], word, st)
        if t < 31:
            if inp.sounding is not None:
                inp.sounding.step(buf.xhat, t)
            _next_time_token(plan, P, buf, tbl, inp, t)


def _free_fwd_steps(plan, P, buf, tbl, inp):
    """the generic loop, one launch per cell and head: 32 time steps of 15 note steps of 5 duration steps"""
    B, Ht = buf.dims[0], buf.dims[4]
    _first_tokens(buf, tbl)
    if inp.sounding is not None:
        inp.sounding.step(buf.xhat, -1)
    for t in range(32):
        rows = slice(t * B, (t + 1) * B)
        ns = _time_step(plan, P, buf, tbl, inp, t)
        gemm(ns, tbl.w_tn16, buf.HN[0][rows], bias=P['dec_time_to_notes_hid.bias'], prec=inp.prec)
        GCt = gemm(ns, tbl.w_ih_n16[:, :Ht], bias=P['dec_notes_gru.bias_ih_l0'], prec=inp.prec)
        for n in range(15):
            _note_step(plan, P, buf, tbl, inp, t, n, GCt)
        if t < 31:
            if inp.sounding is not None:
                inp.sounding.step(buf.xhat, t)
            _next_time_token(plan, P, buf, tbl, inp, t)


def _note_step(plan, P, buf, tbl, inp, t, n, GCt):
    """note step n of time step t of the generic loop: the notes GRU's cell, the pitch head, the duration GRU (fused, or five cells and
    heads), the predicted token, and the token fed next"""
    B, R, E, He, Ht, Hn, Hd, NP = buf.dims
    M, prec, kind, st, train = 15 * R, inp.prec, plan.kind, stream_ptr(), plan.train
    HN, HD, TOK, PRED, pitch, idx, gates_d, force_dur = buf.HN, buf.HD, buf.TOK, buf.PRED, buf.pitch, buf.idx, buf.gates_d, inp.force_dur
    w_dh, w_hh_d, b_hh_d = P['dur_hid_linear.weight'], P['dec_dur_gru.weight_hh_l0'], P['dec_dur_gru.bias_hh_l0']
    w_out_d, b_out_d, dur2 = P['dur_out_linear.weight'], P['dur_out_linear.bias'], buf.dur.view(M, 10)
    smp = () if inp.sampling is None else (ptr(inp.sampling),)      # sampled forms: the block, then (t, n) of the rows
    rows, pr = slice(t * B, (t + 1) * B), slice(n * R + t * B, n * R + (t + 1) * B)
    gi_tok = gemm(TOK[n][rows], P['dec_notes_gru.weight_ih_l0'][:, Ht:], prec=prec)
    gru_step(prec, HN[n][rows], gi_tok, 3 * Hn, P['dec_notes_gru.weight_hh_l0'], P['dec_notes_gru.bias_hh_l0'], HN[n + 1][rows], gi2=GCt,
             gates=buf.gates_n[n][:, rows] if train else None, plane=R * Hn)
    h = HN[n + 1][rows]
    gemm(h, P['pitch_out_linear.weight'], pitch[pr], bias=P['pitch_out_linear.bias'], prec=prec)
    gemm(h, w_dh[:, :Hn], HD[0][pr], bias=P['dur_hid_linear.bias'], prec=prec)
    gemm(pitch[pr], w_dh[:, Hn:], HD[0][pr], acc=True, prec=prec)
    # (the constrained kind with force arrays: the entries that honour a duration range word -- INTEGRATION.md "Duration limits")
    # (the row-wise kind: one entry each, with the force array or NULL)
    cons_dur = bool(kind.cons) and force_dur is not None
    sfx = '' if kind.rows else '_cons'
    if prec == 1 and Hd == 64 and F_.FUSED_DUR:
        call(kind.dur_gru + (sfx if cons_dur else ''), Hd, B, ptr(HD[0][pr]), Hd, ptr(w_hh_d), ptr(b_hh_d), ptr(tbl.tab0), ptr(tbl.tab), ptr(w_out_d), ptr(b_out_d),
             ptr(HD[1][pr]), M * Hd, None, ptr(gates_d[0][0][pr]) if train else None, M * Hd, 4 * M * Hd, F_._bf(gates_d), ptr(dur2[pr]), 10,
             ptr(idx[0][pr]), M, ptr(force_dur[0][pr]) if force_dur is not None else None, M, *(smp and smp + (t, n)), st)
    else:
        for d in range(5):
            g_, g_ld, g_idx = (tbl.tab0, 0, None) if d == 0 else (tbl.tab, 3 * Hd, idx[d - 1][pr])
            gru_step(prec, HD[d][pr], g_, g_ld, w_hh_d, b_hh_d, HD[d + 1][pr], gates=gates_d[d][:, pr] if train else None, plane=M * Hd,
                     gi_idx=g_idx)
            if cons_dur or kind.rows:
                call(kind.dur_token + sfx, ptr(HD[d + 1][pr]), Hd, ptr(w_out_d), ptr(b_out_d), ptr(dur2[pr][:, 2 * d:]), 10,
                     ptr(idx[d][pr]), M, ptr(force_dur[d][pr]) if force_dur is not None else None, B, *smp, t, n, d, st)
                continue
            call(kind.dur_token, ptr(HD[d + 1][pr]), Hd, ptr(w_out_d), ptr(b_out_d), ptr(dur2[pr][:, 2 * d:]), 10, ptr(idx[d][pr]),
                 ptr(force_dur[d][pr]) if force_dur is not None else None, B, *(smp and smp + (t, n, d)), st)
    call(kind.note_token, ptr(pitch[pr]), NP, ptr(idx[0][pr]), M, ptr(P['note_embedding.weight']), ptr(P['note_embedding.bias']), E,
         ptr(PRED[n + 1][rows]), E, ptr(buf.xhat[0, t, n + 1]), 32 * 16 * 6, ptr(buf.plen[rows]), n + 1, int(n == 14),
         ptr(inp.force_pitch[n][rows]) if inp.force_pitch is not None else None, B, *(smp and smp + (t,)), st)
    if n < 14:
        use_gt = (not inp.inference) and inp.coins[0][t][n]
        copy2d(TOK[n + 1][rows], inp.emb3[n + 1][rows] if use_gt else PRED[n + 1][rows])


def _free_recompute(plan, P, buf, tbl, prec):
    """what the backward reads, recomputed batched over all rows by the teacher-forced kernels (the replayed loop stored decisions and
    tokens only): notes-GRU states and gates, the duration GRU with the stored decisions forced, the re-summarisation bi-GRU"""
    B, R, E, He, Ht, Hn, Hd, NP = buf.dims
    M, st, dev, bf16 = 15 * R, stream_ptr(), buf.NS.device, torch.bfloat16
    HD, HD16 = buf.HD, buf.HD16
    w_ih_n, w_hh_n, w_dh = P['dec_notes_gru.weight_ih_l0'], P['dec_notes_gru.weight_hh_l0'], P['dur_hid_linear.weight']
    F_.zero_skip_sync()
    GC16 = gemm(buf.NS16[1:].view(R, Ht), w_ih_n[:, :Ht], bias=P['dec_notes_gru.bias_ih_l0'], prec=prec, out_dtype=bf16,
                out_blocked=16)      # (column-blocked by 16: the layout the row kernel reads)
    pkn = F_.notes_packs(w_ih_n, w_hh_n, Ht)
    call('ptv_notes_gru_persist_fwd', ptr(pkn['wg_h']), ptr(pkn['wg_t']), ptr(P['dec_notes_gru.bias_hh_l0']), ptr(GC16), ptr(buf.TOK),
         ptr(buf.HN), ptr(buf.HN16), ptr(buf.gates_n), R, 15, st)
    gemm(buf.HN16[1:].view(M, Hn), w_dh[:, :Hn], HD[0], bias=P['dur_hid_linear.bias'], prec=prec)
    gemm(buf.pitch, w_dh[:, Hn:], HD[0], acc=True, prec=prec)
    dur_scr, idx_scr = _empty(M, 10, dev=dev), torch.empty(5, M, device=dev, dtype=torch.int32)
    call('ptv_dur_gru_fwd', Hd, M, ptr(HD[0]), Hd, ptr(P['dec_dur_gru.weight_hh_l0']), ptr(P['dec_dur_gru.bias_hh_l0']), ptr(tbl.tab0),
         ptr(tbl.tab), ptr(P['dur_out_linear.weight']), ptr(P['dur_out_linear.bias']), None, M * Hd, ptr(HD16[1]), ptr(buf.gates_d), M * Hd,
         4 * M * Hd, 1, ptr(dur_scr), 10, ptr(idx_scr), M, ptr(buf.idx), M, st)
    call('ptv_cast_bf16', ptr(HD[0]), ptr(HD16[0]), M * Hd, st)
    if plan.need_resum:
        for d in range(2):
            w_ih_e, w_hh_e, b_ih_e, b_hh_e = tbl.wE[4 * d: 4 * d + 4]
            pke = F_.notes_packs(w_ih_e, w_hh_e, 0)
            call('ptv_row_gru_persist_fwd', He, ptr(pke['wg_h']), ptr(pke['wg_t']), ptr(b_hh_e), ptr(b_ih_e), None, ptr(buf.PRED), R * E,
                 ptr(buf.plen), ptr(buf.XH[d]), ptr(buf.XH16[d]), ptr(buf.XG[d]), None, 0, R, 16, d, st)


def _free_bwd_switch_off(prec):
    """the first switch that keeps DecoderStepFn.backward from asking for its one-call form (ptv_decoder_free_bwd), or None"""
    for on, word in ((FREE_COMPOSITE, 'FREE_COMPOSITE off'), (prec == 1, 'not bf16'), (F_.DEC_BWD_COMPOSITE, 'DEC_BWD_COMPOSITE off'),
                     (F_.BIGRU_BWD_COMPOSITE, 'BIGRU_BWD_COMPOSITE off'), (F_.WGRAD_FUSE_BIAS, 'WGRAD_FUSE_BIAS off')):
        if not on:
            return word
    return 'capturing' if torch.cuda.is_current_stream_capturing() else None


class FreeRoutes:
    """where DecoderStepFn.backward routes the token gradients: demb / dPRED [16,R,E] the note tokens' -- ground-truth embedding (coin true / slot 0)
    vs predicted tokens -- and dxs / dxsp [32,B,2He] the time tokens' -- ground-truth summaries (coin true) vs re-summarised predictions"""

    def __init__(self, st, dev):
        coin_notes, coin_time = st.coins
        self.demb, self.dPRED = _zeros(16, st.R, st.E, dev=dev), _zeros(16, st.R, st.E, dev=dev)
        self.mask_tok = _route_mask(('tok', tuple(tuple(bool(v) for v in row) for row in coin_notes)), dev)
        self.dxs, self.dxsp = _zeros(32, st.B, 2 * st.He, dev=dev), _zeros(32, st.B, 2 * st.He, dev=dev)
        self.mask_time = _route_mask(('time', tuple(bool(v) for v in coin_time)), dev)


def _free_bwd_route(st, tf, rt):
    sp = stream_ptr()
    call('ptv_route_slices', ptr(tf.dtok), ptr(rt.demb), ptr(rt.dPRED), ptr(rt.mask_tok), st.B * st.E, 15 * 32, 0, sp)
    call('ptv_route_slices', ptr(tf.dTOKS[1:]), ptr(rt.dxs), ptr(rt.dxsp), ptr(rt.mask_time), st.B * 2 * st.He, 32, 0, sp)


def _free_resum_operands(P, st):
    """-> the re-summarisation bi-GRU's weights and the BiGruState its backward reads"""
    wE = [P['dec_notes_emb_gru.' + n] for n in EMB_GRU]
    # (the batched recompute ran the row kernels -- they left bf16 states -- and skipped dead panel steps by plen)
    return wE, BiGruState('rows' if st.XH16[0] is not None else 'step', zip(st.XH, st.XG, st.XH16), lengths=st.plen if st.skipped else None)


def _free_bwd_tail(st, rt, mh, gw, gb):
    """predicted tokens -> note_embedding (slot 0 is the ground-truth <sos> embedding); weight and bias gradient in ONE pass (ptv_wgrad's colsum_a)"""
    copy2d(rt.demb[0], rt.dPRED[0], acc=True)
    rt.dPRED[0].zero_()
    call('ptv_multihot', ptr(st.xhat), ptr(mh), 136, st.B, stream_ptr())
    F_.wgrad_bias(rt.dPRED.view(16 * st.R, st.E), mh[:, :135], gw, gb, st.prec)


class DecoderStepState(F_.DecoderState):
    """DecoderState of the step loop: what decoder_bwd_core reads, and beside it what only DecoderStepFn.backward does -- TOK [15,R,E] the
    note tokens that were fed, PRED [16,R,E] the predicted ones, xhat the predicted grid, XH / XG / XH16 the re-summarisation bi-GRU's
    states, gates and bf16 states per direction (XH None: no re-summarisation), plen the predicted rows' lengths and whether the kernels
    skipped by them, the teacher-forcing coins, has_xs: ground-truth summaries were given; plan: the FreePlan the forward ran by"""

    def __init__(self, dims, prec, notes, heads, dur, *, TOK, PRED, xhat, XH, XG, XH16, plen, skipped, coins, has_xs, plan=None, **saved):
        super().__init__(dims, prec, notes, heads, dur, **saved)
        self.plan = plan
        self.TOK, self.PRED, self.xhat, self.XH, self.XG, self.XH16 = TOK, PRED, xhat, XH, XG, XH16
        self.plen, self.skipped, self.coins, self.has_xs = plen, skipped, coins, has_xs


class DecoderStepFn(torch.autograd.Function):
    """(z, emb [16,32,B,E] or None, xs [32B,2He] or None, coins, inference, force, prec, *params[, sampling block])
    -> pitch [15,32,B,130], dur [15*32*B,5,2], xhat int64 [B,32,16,6] (predicted grid), dur idx"""

    @staticmethod
    def forward(ctx, z, emb, xs, coins, inference, force, prec, *params):
        # the optional trailing argument: the sampling block of a sampled decode (inference only); absent = the argmax kernels
        sampling = None
        if len(params) == len(FREE_PARAM_NAMES) + 1:
            sampling, params = params[-1], params[:-1]
        P = dict(zip(FREE_PARAM_NAMES, params))
        dev = z.device
        if sampling is not None:
            if not inference or any(any(r) for r in coins[0]) or any(coins[1]):
                raise ValueError('sampling is inference only: it cannot be combined with training or teacher forcing')
            _check_block(sampling, dev, z.shape[0])
        z = z.contiguous()
        B, R = z.shape[0], 32 * z.shape[0]
        E, NP, Zi = (P[n + '.weight'].shape[0] for n in ('note_embedding', 'pitch_out_linear', 'z2dec_in_linear'))
        He, Ht, Hn, Hd = (P['dec_%s_gru.weight_hh_l0' % n].shape[1] for n in ('notes_emb', 'time', 'notes', 'dur'))
        dims = (B, R, E, He, Ht, Hn, Hd, NP)
        force_pitch, force_dur = (force.get('pitch'), force.get('dur')) if force else (None, None)       # [15, R], [5, 15 R] int32
        run = force.get('sounding') if force else None      # a SoundingRun: 'pitch' and the block's mask are its effective arrays
        if run is not None and (not inference or any(any(r) for r in coins[0]) or any(coins[1])):
            raise ValueError('sounding is inference only: it cannot be combined with training or teacher forcing')
        plan = _free_plan(prec, dims, z.dtype, coins, inference, any(ctx.needs_input_grad),
                          force_pitch is not None or force_dur is not None, block_kind(sampling), _num_cu(),
                          torch.cuda.is_current_stream_capturing())
        inp = FreeInputs(z, emb.view(16, R, E) if emb is not None else None, xs, coins, *coin_masks(coins, inference), force_pitch, force_dur,
                         sampling, inference, prec, run)

        # ---- allocate by the plan, then launch (the composite runs the prologue itself)
        buf = FreeBuffers(plan, dims + (Zi,), prec, inference, dev)
        if not plan.comp:
            _free_prologue(P, buf, z, prec)
        tbl = _free_tables(plan, P, buf, inp)
        if plan.comp:
            done = _free_fwd_composite(plan, P, buf, tbl, inp)
            assert done, 'ptv_decoder_free_fwd declined a configuration free_persist_ok() accepted'
        elif plan.fast:
            _free_fwd_persistent(plan, P, buf, tbl, inp)
        else:
            _free_fwd_steps(plan, P, buf, tbl, inp)
        if plan.replay and not plan.comp:
            _free_recompute(plan, P, buf, tbl, prec)
        if plan.train:
            ctx.save_for_backward(z, emb, *params)
            ctx.saved_state = DecoderStepState(
                dims, prec, *_free_branches(plan, prec, dims, None if buf.gates_d is None else buf.gates_d.dtype), plan=plan,
                dur_tabs=(tbl.tab0, tbl.tab), skipped=F_.ZERO_SKIP, coins=coins, has_xs=xs is not None, **buf.saved())
        ctx.mark_non_differentiable(buf.xhat, buf.idx)
        return buf.pitch.view(15, 32, B, NP), buf.dur, buf.xhat, buf.idx

    @staticmethod
    def backward(ctx, dpitch, ddur, _dx, _di):
        z, emb, *params = ctx.saved_tensors
        P = dict(zip(FREE_PARAM_NAMES, params))
        st = ctx.saved_state
        if not getattr(ctx, 'keep_state', False):        # a captured forward (GraphedDecoderStepFn) reuses its buffers
            ctx.saved_state = None
        global _DFB_PATH
        B, R, E, He, prec, dev = st.B, st.R, st.E, st.He, st.prec, z.device
        # ---- the stages, in order: the decoder's batched BPTT (duration GRU, heads, notes GRU, time GRU: the teacher-forced path's, on the
        # recorded fed tokens), the two routings, the re-summarisation bi-GRU's backward and its accumulate, the note_embedding gradients.
        # They go out as ONE C call (ptv_decoder_free_bwd) when no switch is off and both composite stages come back prepared, else stage
        # by stage: same launches, same order, same bits.  `why`: the first reason against the one call
        why = _free_bwd_switch_off(prec)
        tf = F_.decoder_bwd_core(P, st, z, st.TOK.view(15 * R, E), dpitch, ddur, launch=why is not None)
        if why is None and tf.call is None:
            why = 'decoder stage declined'
        G = {**dict.fromkeys(FREE_PARAM_NAMES), **tf.G}
        rt = FreeRoutes(st, dev)
        rows, dout = None, rt.dxsp.view(R, 2 * He)
        if st.XH is not None:
            wE, state = _free_resum_operands(P, st)
            if why is None:                # (prepared before anything is launched: it reads dxsp, which the second route writes)
                rows = F_.bigru_rows_bwd_prepare(prec, st.PRED, wE, state, dout, True)
                if rows is None or not rows[1][1].is_contiguous():
                    why = 'rows stage declined' if rows is None else 'dx_pred not contiguous'
        mh = _empty(B * 512, 136, dev=dev)
        for n in ('note_embedding.weight', 'note_embedding.bias'):
            if G[n] is None:
                G[n] = _gbuf(P[n])
        gw, gb = G['note_embedding.weight'], G['note_embedding.bias']
        _DFB_PATH = why or 'one call'
        ge, dx_pred = rows[1] if rows else ((), None)
        if why is None:
            slots = _DFB.pointers({'DTOK': tf.dtok, 'DTOKS': tf.dTOKS, 'DEMB': rt.demb, 'DPRED': rt.dPRED, 'DXS': rt.dxs, 'DXSP': rt.dxsp,
                                   'MASK_TOK': rt.mask_tok, 'MASK_TIME': rt.mask_time, 'DX_PRED': dx_pred, 'XHAT': st.xhat, 'MH': mh,
                                   'G_W_EMB': gw, 'G_B_EMB': gb})
            F_._chain_prio()
            rc = lib().ptv_decoder_free_bwd(tf.call.ptrs, tf.call.dims, rows[0].ptrs if rows else None, rows[0].dims if rows else None, slots,
                                            _DFB.dims({'B': B, 'E': E, 'HE': He}), stream_ptr())
            for c in (tf.call,) + ((rows[0],) if rows else ()):
                c.ran_inside(rc, 'ptv_decoder_free_bwd')
            _DFF.count('bcalls')                # (counted beside the forward's)
        else:
            if tf.call is not None:
                tf.call.launch()
            _free_bwd_route(st, tf, rt)
            if st.XH is not None:
                if rows is not None:
                    rows[0].launch()
                else:
                    ge, dx_pred = _bigru_backward(prec, st.PRED, wE, state, dout, True)
                copy2d(rt.dPRED.view(16 * R, E), dx_pred.view(16 * R, E), acc=True)
            _free_bwd_tail(st, rt, mh, gw, gb)
        G.update(('dec_notes_emb_gru.' + n, gg) for n, gg in zip(EMB_GRU, ge))
        tf.side.join()
        grads = tuple(G[n] for n in FREE_PARAM_NAMES)
        return (tf.dz, rt.demb.view(16, 32, B, E), rt.dxs.view(R, 2 * He) if st.has_xs else None, None, None, None, None) + grads


# =============================================================================================
# RnnDecoder (chord decoder) with arbitrary coins: ptvae.py:51-87
# =============================================================================================
class _CapturedCtx:
    """stands in for the autograd ctx of DecoderStepFn while its forward is captured into a hipGraph"""

    def __init__(self, n_inputs):
        self.needs_input_grad = (True,) * n_inputs
        self.saved_tensors = ()
        self.saved_state = None
        self.keep_state = True

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *a):
        pass


class _GraphEntry:
    """one captured free-running training forward + the buffers its backward reads.  `pending` is a weak reference to the
    autograd ctx of the replay whose backward has not run yet: a second replay before that would overwrite NS / HN / gates /
    PRED under it (two loss() calls and one backward, gradient accumulation over micro-batches, ...)"""

    def __init__(self, g, sz, se, cap, outs):
        self.g, self.sz, self.se, self.cap, self.outs = g, sz, se, cap, outs
        self.pending = None

    def busy(self):
        c = self.pending() if self.pending is not None else None
        return c is not None and not getattr(c, 'done', True)


GRAPH_CACHE_SLOTS = 3          # e.g. train and validation batch sizes alternating: no re-capture (~9,000 launches + warm-up) per switch


def _graph_key(z, emb, xs, prec, params):
    return (z.shape[0], prec, z.device.index, tuple(p.data_ptr() for p in params), tuple(emb.shape), xs is not None,
            F_.FUSED_DUR, F_.BF16_STORAGE, F_.NOTES_PERSIST, F_.PERSIST, FREE_PERSIST)


def graphed_decoder_step(cache, z, emb, xs, prec, *params):
    """GraphedDecoderStepFn when its captured buffers are free, the eager DecoderStepFn (same kernels, own buffers) while an
    earlier replay of the same graph still waits for its backward"""
    ent = cache.get(_graph_key(z, emb, xs, prec, params))
    if ent is not None and ent.busy():
        coins = ([[False] * 14] * 32, [False] * 31)
        return DecoderStepFn.apply(z, emb, xs, coins, False, None, prec, *params)
    return GraphedDecoderStepFn.apply(cache, z, emb, xs, prec, *params)


class GraphedDecoderStepFn(torch.autograd.Function):
    """Free-running TRAINING forward (every teacher-forcing coin false: what the reference's schedules reach after two
    steps) replayed from a captured hipGraph.  The launch order and arguments of the step loop depend only on (B, precision,
    parameter storage, the module-level kernel toggles): capture DecoderStepFn.forward once -- every buffer the backward needs
    is the graph's static storage -- then one graph launch per step; the backward is DecoderStepFn.backward on those buffers.
    The returned tensors are copies (they do not change under the caller at the next replay).  `cache` is a dict owned by the
    decoder module, a small LRU.  Call through graphed_decoder_step(), which falls back to the eager path while a replay's
    backward is pending."""

    @staticmethod
    def forward(ctx, cache, z, emb, xs, prec, *params):
        key = _graph_key(z, emb, xs, prec, params)
        ent = cache.get(key)
        coins = ([[False] * 14] * 32, [False] * 31)
        if ent is not None and ent.busy():
            raise RuntimeError('GraphedDecoderStepFn: the previous replay of this graph has not been back-propagated yet; '
                               'call graphed_decoder_step(), which runs such forwards eagerly')
        if ent is None:
            sz, se = z.detach().clone().contiguous(), emb.detach().clone()
            sx = xs.detach().clone() if xs is not None else None
            cur = torch.cuda.current_stream()
            s = torch.cuda.Stream(device=z.device)
            s.wait_stream(cur)
            with torch.cuda.stream(s):                       # warm-up outside capture (lazy inits, allocator)
                DecoderStepFn.forward(_CapturedCtx(7 + len(params)), sz, se, sx, coins, False, None, prec, *params)
            cur.wait_stream(s)
            cap = _CapturedCtx(7 + len(params))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = DecoderStepFn.forward(cap, sz, se, sx, coins, False, None, prec, *params)
            while len(cache) >= GRAPH_CACHE_SLOTS:           # least recently used first (dicts keep insertion order)
                victim = next((k for k, e in cache.items() if not e.busy()), None)
                if victim is None:
                    break
                del cache[victim]
            ent = cache[key] = _GraphEntry(g, sz, se, cap, outs)
        else:
            cache[key] = cache.pop(key)                      # most recently used last
        ent.sz.copy_(z)
        ent.se[0].copy_(emb[0])                               # only the <sos> slot of the ground truth is read when no coin is true
        ent.g.replay()
        ctx.cap = ent.cap
        ctx.done = not any(ctx.needs_input_grad)
        ent.pending = weakref.ref(ctx)
        outs = tuple(o.clone() for o in ent.outs)
        ctx.mark_non_differentiable(outs[2], outs[3])
        return outs

    @staticmethod
    def backward(ctx, dpitch, ddur, _dx, _di):
        r = DecoderStepFn.backward(ctx.cap, dpitch, ddur, None, None)
        ctx.done = True
        # DecoderStepFn inputs: (z, emb, xs, coins, inference, force, prec, *params) -> ours: (cache, z, emb, xs, prec, *params)
        return (None, r[0], r[1], r[2], None) + tuple(r[7:])


# ---------------------------------------------------------------------------------------------
# The reference's note-level METHODS (ptvae.py:315-428) as callable entry points: forward-only helpers for reference-side code that
# calls `decoder.decode_note(...)` / `decode_notes(...)` / the token builders directly (training goes through DecoderTFFn /
# DecoderStepFn, which run the same kernels fused).  Rows = whatever batch the caller hands over.
# ---------------------------------------------------------------------------------------------
def note_token_rows(P, pitch_inds, dur_inds):
    """pitch_dur_ind_to_note_token (ptvae.py:328-334): note_embedding(onehot(pitch) | 5 duration bits) -> [B, E]"""
    dev = pitch_inds.device
    B = pitch_inds.shape[0]
    w_emb, b_emb = P['note_embedding.weight'], P['note_embedding.bias']
    E = w_emb.shape[0]
    NP = w_emb.shape[1] - 5
    dummy = _zeros(B, NP, dev=dev)
    idx = dur_inds.reshape(B, 5).t().contiguous().int()
    pred = _empty(B, E, dev=dev)
    xhat = torch.empty(B, 6, device=dev, dtype=torch.long)
    plen = torch.zeros(B, device=dev, dtype=torch.int32)
    call('ptv_note_token', ptr(dummy), NP, ptr(idx), B, ptr(w_emb), ptr(b_emb), E, ptr(pred), E, ptr(xhat), 6, ptr(plen), 1, 0,
         ptr(pitch_inds.int().contiguous()), B, stream_ptr())
    return pred


def decode_note_rows(P, h, prec, force_dur=None):
    """decode_note (ptvae.py:336-368) for B rows: h [B, Hn] -> est_pitch [B, NP], est_durs [B, 5, 2], duration argmaxes [5, B]"""
    dev = h.device
    B, Hn = h.shape
    Hd = P['dec_dur_gru.weight_hh_l0'].shape[1]
    w_dh = P['dur_hid_linear.weight']
    w_ih_d, b_ih_d = P['dec_dur_gru.weight_ih_l0'], P['dec_dur_gru.bias_ih_l0']
    w_hh_d, b_hh_d = P['dec_dur_gru.weight_hh_l0'], P['dec_dur_gru.bias_hh_l0']
    pitch = gemm(h, P['pitch_out_linear.weight'], bias=P['pitch_out_linear.bias'], prec=prec)
    HD = _empty(6, B, Hd, dev=dev)
    gemm(h, w_dh[:, :Hn], HD[0], bias=P['dur_hid_linear.bias'], prec=prec)
    gemm(pitch, w_dh[:, Hn:], HD[0], acc=True, prec=prec)
    tab0 = gemm(P['dur_sos_token'].view(1, -1), w_ih_d, bias=b_ih_d, prec=0)
    tab = gemm(_onehot2x5(dev), w_ih_d, bias=b_ih_d, prec=0)
    idx = torch.empty(5, B, device=dev, dtype=torch.int32)
    dur = _empty(B, 5, 2, dev=dev)
    dur2 = dur.view(B, 10)
    for d in range(5):
        g_, g_ld, g_idx = (tab0, 0, None) if d == 0 else (tab, 3 * Hd, idx[d - 1])
        gru_step(prec, HD[d], g_, g_ld, w_hh_d, b_hh_d, HD[d + 1], plane=B * Hd, gi_idx=g_idx)
        call('ptv_dur_out_token', ptr(HD[d + 1]), Hd, ptr(P['dur_out_linear.weight']), ptr(P['dur_out_linear.bias']),
             ptr(dur2[:, 2 * d:]), 10, ptr(idx[d]), ptr(force_dur[d]) if force_dur is not None else None, B, stream_ptr())
    return pitch, dur, idx


def decode_notes_rows(P, ns, notes, coins, inference, prec):
    """decode_notes (ptvae.py:370-428) for B rows: ns [B, Ht] time-level summary, notes [B, 16, E] ground-truth embedded notes (or
    None when `inference`), coins [14] teacher-forcing decisions -> pitch_outs [B,15,NP], dur_outs [B,15,5,2],
    predicted_notes [B,16,E], lengths [B] float"""
    dev = ns.device
    B, Ht = ns.shape
    E = P['note_embedding.weight'].shape[0]
    Hn = P['dec_notes_gru.weight_hh_l0'].shape[1]
    NP = P['pitch_out_linear.weight'].shape[0]
    w_emb, b_emb = P['note_embedding.weight'], P['note_embedding.bias']
    w_ih_n, w_hh_n, b_hh_n = P['dec_notes_gru.weight_ih_l0'], P['dec_notes_gru.weight_hh_l0'], P['dec_notes_gru.bias_hh_l0']
    st = stream_ptr()
    HN = _empty(16, B, Hn, dev=dev)
    gemm(ns, P['dec_time_to_notes_hid.weight'], HN[0], bias=P['dec_time_to_notes_hid.bias'], prec=prec)
    GC = gemm(ns, w_ih_n[:, :Ht], bias=P['dec_notes_gru.bias_ih_l0'], prec=prec)
    TOK = _empty(15, B, E, dev=dev)
    PRED = _zeros(16, B, E, dev=dev)
    if inference:
        sos = _sos_grid(dev)
        sos_emb = _empty(16, 32, 1, E, dev=dev)
        call('ptv_embed_fwd', ptr(sos), ptr(w_emb), ptr(b_emb), ptr(sos_emb), None, 1, E, st)
        copy2d(TOK[0], sos_emb.view(-1, E)[0:1], lds=0)
    else:
        nt = notes.float().transpose(0, 1).contiguous()                  # [16, B, E]
        copy2d(TOK[0], nt[0])
    copy2d(PRED[0], TOK[0])
    pitch = _empty(15, B, NP, dev=dev)
    dur = _empty(15, B, 5, 2, dev=dev)
    xhat = torch.full((B, 16, 6), 2, device=dev, dtype=torch.long)
    plen = torch.zeros(B, device=dev, dtype=torch.int32)
    for n in range(15):
        gi_tok = gemm(TOK[n], w_ih_n[:, Ht:], prec=prec)
        gru_step(prec, HN[n], gi_tok, 3 * Hn, w_hh_n, b_hh_n, HN[n + 1], gi2=GC, plane=B * Hn)
        p_, d_, idx = decode_note_rows(P, HN[n + 1], prec)
        copy2d(pitch[n], p_)
        copy2d(dur[n].view(B, 10), d_.view(B, 10))
        call('ptv_note_token', ptr(p_), NP, ptr(idx), B, ptr(w_emb), ptr(b_emb), E, ptr(PRED[n + 1]), E, ptr(xhat[0, n + 1]), 16 * 6,
             ptr(plen), n + 1, int(n == 14), None, B, st)
        if n < 14:
            use_gt = (not inference) and coins[n]
            copy2d(TOK[n + 1], nt[n + 1] if use_gt else PRED[n + 1])
    return (pitch.transpose(0, 1), dur.transpose(0, 1), PRED.transpose(0, 1), plen.float())


class ChordDecoderStepFn(torch.autograd.Function):
    """(z_chd, c_sm [8,B,36] or None, coins [8] bools, force, prec, *params) -> root [8,B,12], chroma [8,B,24], bass [8,B,12]
    force (tests: replay mode): {'root' [8,B,12], 'chroma' [8,B,24], 'bass' [8,B,12]} logits of a recorded run whose
    argmax decisions build the fed-back tokens instead of this run's own (a near-tie flipped by rounding changes the trajectory)"""

    @staticmethod
    def forward(ctx, z, c_sm, coins, force, prec, *params):
        P = dict(zip(F_.CHD_PARAM_NAMES, params))
        dev = z.device
        z = z.contiguous()
        B = z.shape[0]
        T = len(coins)
        H = P['gru.weight_hh_l0'].shape[1]
        I = P['init_input'].shape[0]
        hall = _empty(T + 1, B, H, dev=dev)
        gemm(z, P['z2dec_hid.weight'], hall[0], bias=P['z2dec_hid.bias'], prec=prec)
        z_in = gemm(z, P['z2dec_in.weight'], bias=P['z2dec_in.bias'], prec=prec)
        w_ih = P['gru.weight_ih_l0']
        zg = gemm(z_in, w_ih[:, I:], bias=P['gru.bias_ih_l0'], prec=prec)
        toks = _empty(T, B, I, dev=dev)
        copy2d(toks[0], P['init_input'].view(1, -1), lds=0)
        gates = _empty(T, 4, B, H, dev=dev, dtype=F_._act_dtype(prec, H))
        root, chroma, bass = _empty(T, B, 12, dev=dev), _empty(T, B, 24, dev=dev), _empty(T, B, 12, dev=dev)
        masks = torch.zeros(2, device=dev, dtype=torch.int32)
        for t in range(T):
            gi = gemm(toks[t], w_ih[:, :I], prec=prec)
            gru_step(prec, hall[t], gi, 3 * H, P['gru.weight_hh_l0'], P['gru.bias_hh_l0'], hall[t + 1], gi2=zg, gates=gates[t],
                     plane=B * H)
            gemm(hall[t + 1], P['root_out.weight'], root[t], bias=P['root_out.bias'], prec=prec)
            gemm(hall[t + 1], P['chroma_out.weight'], chroma[t], bias=P['chroma_out.bias'], prec=prec)
            gemm(hall[t + 1], P['bass_out.weight'], bass[t], bias=P['bass_out.bias'], prec=prec)
            if t + 1 < T:
                if coins[t] and c_sm is not None:
                    copy2d(toks[t + 1], c_sm[t])
                else:
                    src = (force['root'], force['chroma'], force['bass']) if force else (root, chroma, bass)
                    call('ptv_chord_token', ptr(src[0][t]), ptr(src[1][t]), ptr(src[2][t]), ptr(masks), ptr(toks[t + 1]), B,
                         stream_ptr())
        F_._chord_decoder_leave(ctx, F_.ChordDecoderState(T, B, H, I, prec, hall=hall, gates=gates, toks=toks, z_in=z_in), z, params)
        return root, chroma, bass

    @staticmethod
    def backward(ctx, droot, dchroma, dbass):
        # tokens are constants (ground truth or argmax one-hots): same BPTT as the teacher-forced path
        z, *params = ctx.saved_tensors
        state, ctx.saved_state = ctx.saved_state, None
        dz, G = F_.chord_decoder_bwd(dict(zip(F_.CHD_PARAM_NAMES, params)), state, z, droot, dchroma, dbass)
        return (dz, None, None, None, None) + tuple(G[n] for n in F_.CHD_PARAM_NAMES)


# =============================================================================================
# Row-independent free-running chord decode (csrc/chord_decode.hip): every row feeds back its OWN token, decisions may be
# seeded draws, kept or scored.  Inference only; ChordDecoderStepFn above keeps the reference's union-over-the-batch token.
# =============================================================================================
CHORD_STEPS = 8
_CDS = SlotTable('CDS')

ChordLogprob = collections.namedtuple('ChordLogprob', 'logp logq forced err step_logp step_logq step_forced')
ChordDecode = collections.namedtuple('ChordDecode', 'c chord14 root chroma bass logprob')      # root / chroma / bass: step-major logits


class ChordKeep(collections.namedtuple('ChordKeep', 'c steps batch')):
    """the kept chord steps of a chord decode (INTEGRATION.md "Chord decode"): c f32 [B, 8, 36] and steps uint8 [B, 8] or [1, 8] on the
    device (a non-zero byte: the step's decisions are forced from c[b, t]), batch = B"""
    __slots__ = ()


def chord_keep_steps_row(steps):
    """a host selection of chord steps (an iterable of indices 0..7, or a slice) -> 8 bytes, one per step -- ValueError for anything else"""
    row = bytearray(CHORD_STEPS)
    if isinstance(steps, slice):
        steps = range(*steps.indices(CHORD_STEPS))
    try:
        items = list(steps)
    except TypeError:
        raise ValueError('steps must be a device bool / uint8 tensor [B, 8] or [1, 8], an iterable of step indices or a slice, got %r'
                         % (steps,)) from None
    for t in items:
        if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < CHORD_STEPS:
            raise ValueError('a kept chord step must be an integer in 0..7, got %r' % (t,))
        row[t] = 1
    return bytes(row)


def build_chord_keep(c, steps):
    """(c f32 device [B, 8, 36] as decode_chords / decode_to_inputs give it, steps) -> ChordKeep; steps: a device bool / uint8 tensor
    [B, 8] or [1, 8], or a host selection (chord_keep_steps_row) that becomes one [1, 8] row.  ValueError before any launch; nothing is
    copied to the host (the contents of c are judged by the kernel: ChordLogprob.err)."""
    if not torch.is_tensor(c) or c.device.type != 'cuda':
        raise ValueError('c must be a device tensor: the chords f32 [B, 8, 36]')
    if c.dtype != torch.float32 or c.dim() != 3 or tuple(c.shape[1:]) != (CHORD_STEPS, 36) or c.shape[0] < 1:
        raise ValueError('c must be float32 [B, 8, 36], got %s %s' % (c.dtype, tuple(c.shape)))
    B = c.shape[0]
    if torch.is_tensor(steps):
        if steps.device != c.device:
            raise ValueError('steps must be on the device of c (or a host iterable of step indices / a slice)')
        if steps.dtype not in (torch.bool, torch.uint8):
            raise ValueError('steps must be bool or uint8, got %s' % (steps.dtype,))
        if steps.dim() != 2 or steps.shape[1] != CHORD_STEPS or steps.shape[0] not in (1, B):
            raise ValueError('steps must have shape [B, 8] or [1, 8] with B = %d, got %s' % (B, tuple(steps.shape)))
        steps = steps.contiguous()
        steps = steps.view(torch.uint8) if steps.dtype == torch.bool else steps
    else:
        steps = torch.frombuffer(bytearray(chord_keep_steps_row(steps)), dtype=torch.uint8).view(1, CHORD_STEPS).to(c.device)
    return ChordKeep(c.detach().contiguous(), steps, B)


def check_chord_keep(keep, batch=None):
    """ValueError unless keep is None or a ChordKeep whose arrays fit its batch (and `batch`, the rows of the decode, where known)"""
    if keep is None:
        return
    if not isinstance(keep, ChordKeep):
        raise ValueError('keep_chords must be what DisentangleVAE.keep_chords(c, steps) returns, got %r' % (type(keep).__name__,))
    B = keep.batch
    c, steps = keep.c, keep.steps
    if (not torch.is_tensor(c) or c.device.type != 'cuda' or c.dtype != torch.float32 or tuple(c.shape) != (B, CHORD_STEPS, 36)
            or not c.is_contiguous()):
        raise ValueError('keep_chords.c must be a contiguous float32 device tensor [%d, 8, 36]' % B)
    if (not torch.is_tensor(steps) or steps.device != c.device or steps.dtype != torch.uint8 or steps.dim() != 2
            or steps.shape[1] != CHORD_STEPS or steps.shape[0] not in (1, B) or not steps.is_contiguous()):
        raise ValueError('keep_chords.steps must be a contiguous uint8 tensor [%d, 8] or [1, 8] on the device of c' % B)
    if batch is not None and B != batch:
        raise ValueError('keep_chords was built for a batch of %d, the decoded batch has %d rows' % (B, batch))


def check_chord_sampling(temperature=None, chroma_temperature=None, seed=None, draw=None, sample_offset=None):
    """ValueError for a bad keyword of a chord decode; True for a sampled decode, False for the argmax decode.  No side effect, no launch.
    temperature (root and bass) / chroma_temperature (the 12 bits; default: temperature): finite floats >= 0"""
    if temperature is None:
        if chroma_temperature is not None:
            raise ValueError('chroma_temperature belongs to a sampled chord decode: give chord_temperature as well')
        if seed is not None or draw is not None or sample_offset is not None:
            raise ValueError('seed / draw / sample_offset belong to a sampled decode: give a temperature')
        return False
    try:
        check_sampling(temperature, chroma_temperature, 0 if sample_offset is None else sample_offset, 0 if seed is None else seed,
                       0 if draw is None else draw)
    except ValueError as e:
        raise ValueError(str(e).replace('dur_temperature', 'chroma_temperature')) from None
    return True


# ---- the chord grammar (include/ptvae_hip.h "Chord grammar"; INTEGRATION.md "Chord grammar"): a rule word per row and chord step, a
# vocabulary of chord qualities
_CDG = SlotTable('CDG')
CHORD_RULE_VOCAB, CHORD_RULE_ROOT_IN_CHORD, CHORD_RULE_BASS_IN_CHORD = 1 << 24, 1 << 25, 1 << 26
CHORD_RULE_IDENTITY = 0x00ffffff
CHORD_ERR_KEEP, CHORD_ERR_ROOT_MASK, CHORD_ERR_NO_TEMPLATE, CHORD_ERR_NO_BASS = 1, 2, 4, 8
CHORD_MAX_VOCAB = 64
CHORD_SCALES = {'major': 0xab5, 'minor': 0x5ad, 'harmonic_minor': 0x9ad}       # degrees 0 2 4 5 7 9 11 / 0 2 3 5 7 8 10 / 0 2 3 5 7 8 11
_TRIADS = ((0, 4, 7), (0, 3, 7), (0, 3, 6), (0, 4, 8))                             # maj, min, dim, aug
_SEVENTHS = _TRIADS + ((0, 4, 7, 11), (0, 4, 7, 10), (0, 3, 7, 10), (0, 3, 6, 10), (0, 3, 6, 9), (0, 3, 7, 11))   # maj7 7 m7 m7b5 dim7 mMaj7
CHORD_QUALITIES = {'triads': _TRIADS, 'sevenths': _SEVENTHS}


class ChordGrammar(collections.namedtuple('ChordGrammar', 'rule vocab batch')):
    """the grammar of a chord decode: rule int32 [R, 8] (R = batch or 1: one row serves every sample) and vocab int32 [V], V <= 64, on one
    device; batch = R"""
    __slots__ = ()


def pitch_class_set(value, what):
    """a 12-bit set, or an iterable of integers 0..11 -> the set as an int; ValueError for anything else"""
    if isinstance(value, bool):
        raise ValueError('%s must be a 12-bit set or an iterable of integers 0..11, got %r' % (what, value))
    if isinstance(value, int):
        if not 0 <= value <= 0xfff:
            raise ValueError('%s must be a 12-bit set, got %r' % (what, value))
        return value
    try:
        items = list(value)
    except TypeError:
        raise ValueError('%s must be a 12-bit set or an iterable of integers 0..11, got %r' % (what, value)) from None
    k = 0
    for q in items:
        if isinstance(q, bool) or not isinstance(q, int) or not 0 <= q < 12:
            raise ValueError('%s: an entry must be an integer in 0..11, got %r' % (what, q))
        k |= 1 << q
    return k


def chord_vocabulary(qualities):
    """None / 'triads' / 'sevenths' / an iterable of 12-bit ints or interval tuples -> the list of root-relative templates (ints); every
    template holds interval 0, fits 12 bits and is distinct from the others; at most 64.  ValueError otherwise."""
    if qualities is None:
        return []
    if isinstance(qualities, str):
        if qualities not in CHORD_QUALITIES:
            raise ValueError("qualities must be 'triads', 'sevenths' or an iterable of templates, got %r" % (qualities,))
        qualities = CHORD_QUALITIES[qualities]
    try:
        items = list(qualities)
    except TypeError:
        raise ValueError("qualities must be 'triads', 'sevenths' or an iterable of templates, got %r" % (qualities,)) from None
    out = [pitch_class_set(q, 'a chord quality') for q in items]
    if not out:
        raise ValueError('qualities names no chord: a vocabulary needs at least one template (None = no vocabulary)')
    if len(out) > CHORD_MAX_VOCAB:
        raise ValueError('a vocabulary holds at most %d templates, got %d' % (CHORD_MAX_VOCAB, len(out)))
    for q in out:
        if not q & 1:
            raise ValueError('a chord quality must hold interval 0 (its root), got 0x%03x' % q)
    if len(set(out)) != len(out):
        raise ValueError('the chord qualities must be distinct')
    return out


def _rot12(x, r):
    """the 12-bit sets x (int tensor or int) moved up by r (int tensor): interval i -> pitch class (r + i) % 12"""
    return ((x << r) | (x >> (12 - r))) & 0xfff


def build_chord_grammar(device, key=None, scale=0xab5, roots=None, pitch_classes=None, vocab=(), root_in_chord=False, bass_in_chord=False,
                        steps=None, batch=None):
    """checked host values (DisentangleVAE.chord_grammar judges them) -> ChordGrammar on `device`, built with torch operations there: nothing
    is copied back and no element is visited on the host.  key: None, an int 0..11 or an int tensor [B] / [B, 8] on the device (its values
    are taken modulo 12: they are never read on the host, so there is nothing to refuse); scale /
    roots / pitch_classes: 12-bit sets (roots None: the scale; both relative to the key); vocab: a list of templates; steps: None, 8 host
    bytes (chord_keep_steps_row) or a device bool / uint8 tensor [B, 8] / [1, 8]: the other steps get the identity word."""
    R = 1 if batch is None else batch
    for t in (key, steps):
        if torch.is_tensor(t) and t.shape[0] != 1:
            R = t.shape[0]
    flags = (CHORD_RULE_VOCAB if vocab else 0) | (CHORD_RULE_ROOT_IN_CHORD if root_in_chord else 0) | \
        (CHORD_RULE_BASS_IN_CHORD if bass_in_chord else 0)
    i64 = dict(dtype=torch.int64, device=device)
    if key is None:
        k = torch.zeros(1, 1, **i64)
    elif torch.is_tensor(key):
        k = key.to(torch.int64).remainder(12)
        k = k.view(-1, 1) if k.dim() == 1 else k
    else:
        k = torch.full((1, 1), key, **i64)
    rset = scale if roots is None else roots
    word = _rot12(torch.full((1, 1), rset, **i64), k) | (_rot12(torch.full((1, 1), scale, **i64), k) << 12)
    if pitch_classes is not None:
        word = word & ((pitch_classes << 12) | 0xfff)
    word = (word | flags).expand(R if word.shape[0] == 1 else word.shape[0], CHORD_STEPS)
    if steps is not None:
        if not torch.is_tensor(steps):
            steps = torch.frombuffer(bytearray(steps), dtype=torch.uint8).view(1, CHORD_STEPS).to(device)
        word = torch.where(steps != 0, word, torch.full((1, 1), CHORD_RULE_IDENTITY, **i64))
    rule = word.to(torch.int32).contiguous()
    return ChordGrammar(rule, torch.tensor(list(vocab), dtype=torch.int32, device=device), rule.shape[0])


def check_chord_grammar(grammar, batch=None):
    """ValueError unless grammar is None or a ChordGrammar whose arrays fit its batch (and `batch`, the rows of the decode, where known)"""
    if grammar is None:
        return
    if not isinstance(grammar, ChordGrammar):
        raise ValueError('a chord grammar must be what DisentangleVAE.chord_grammar(...) returns, got %r' % (type(grammar).__name__,))
    rule, vocab, R = grammar
    if (not torch.is_tensor(rule) or rule.dtype != torch.int32 or rule.dim() != 2 or rule.shape[1] != CHORD_STEPS or rule.shape[0] != R
            or R < 1 or not rule.is_contiguous()):
        raise ValueError('chord_grammar.rule must be a contiguous int32 tensor [%r, 8]' % (R,))
    if (not torch.is_tensor(vocab) or vocab.dtype != torch.int32 or vocab.dim() != 1 or vocab.shape[0] > CHORD_MAX_VOCAB
            or vocab.device != rule.device or not vocab.is_contiguous()):
        raise ValueError('chord_grammar.vocab must be a contiguous int32 tensor [V], V <= %d, on the device of the rule' % CHORD_MAX_VOCAB)
    if batch is not None and R not in (1, batch):
        raise ValueError('the chord grammar was built for a batch of %d, the decoded batch has %d rows' % (R, batch))


def chord_decode(z, P, prec, sampling=None, keep=None, grammar=None):
    """z f32 [B, Z] on the device, P {CHD_PARAM_NAMES: parameter} -> ChordDecode, through ptv_chord_decode (ONE C call: 53 launches).
    sampling: None (argmax) or the 32-byte sampling_block(device, T_chord, T_chroma, seed, draw, sample_offset); keep: None or a checked
    ChordKeep of B rows; grammar: None or a checked ChordGrammar of B rows or one -- the call is then ptv_chord_decode_grammar (the same
    launches with the decide launch replaced).  No autograd, no synchronisation."""
    dev = z.device
    if grammar is not None and grammar.rule.device != dev:
        raise ValueError('the chord grammar must be on the device of z (%s), it is on %s' % (dev, grammar.rule.device))
    z = z.detach().float().contiguous()
    B, Z = z.shape
    w_ih = P['gru.weight_ih_l0'].detach()
    H, Zi = P['gru.weight_hh_l0'].shape[1], P['z2dec_in.weight'].shape[0]
    if (P['init_input'].shape[0] != 36 or w_ih.shape[1] != 36 + Zi or P['root_out.weight'].shape[0] != 12
            or P['chroma_out.weight'].shape[0] != 24 or P['bass_out.weight'].shape[0] != 12):
        raise ValueError('the chord decode is built for tokens of 36 and heads of 12 / 24 / 12')
    if sampling is not None and not (torch.is_tensor(sampling) and sampling.dtype == torch.int64 and sampling.numel() == SAMPLED.words
                                     and sampling.is_contiguous() and sampling.device == dev):
        raise ValueError('sampling must be a four-word block made by functional_free.sampling_block() on the device of z')
    T = CHORD_STEPS
    i32 = dict(device=dev, dtype=torch.int32)
    out = dict(HALL=_empty(T + 1, B, H, dev=dev), Z_IN=_empty(B, Zi, dev=dev), ZG=_empty(B, 3 * H, dev=dev), GI=_empty(B, 3 * H, dev=dev),
               TOK=_empty(B, 36, dev=dev), ROOT=_empty(T, B, 12, dev=dev), CHROMA=_empty(T, B, 24, dev=dev), BASS=_empty(T, B, 12, dev=dev),
               C=_empty(B, T, 36, dev=dev), CHORD14=_empty(B, T, 14, dev=dev), STEP_LOGP=_empty(B, T, 3, dev=dev),
               STEP_LOGQ=_empty(B, T, 3, dev=dev), STEP_FORCED=torch.empty(B, T, 3, **i32), STEP_ERR=torch.empty(B, T, **i32),
               LOGP=_empty(B, 3, dev=dev), LOGQ=_empty(B, 3, dev=dev), FORCED=torch.empty(B, 3, **i32), ERR=torch.empty(B, **i32))
    tens = dict(F_._chd_slots(P), Z=z, SAMPLE=sampling, KEEP_C=None if keep is None else keep.c,
                KEEP_STEPS=None if keep is None else keep.steps)
    for k, v in tens.items():
        if v is not None and k not in ('SAMPLE', 'KEEP_STEPS') and (v.dtype != torch.float32 or not v.is_contiguous()):
            raise ValueError('ptv_chord_decode takes contiguous float32 tensors (%s is %s)' % (k, v.dtype))
    dims = {'B': B, 'H': H, 'Z': Z, 'ZI': Zi, 'PREC': prec, 'KEEP_ROWS': 0 if keep is None else keep.steps.shape[0]}
    F_._chain_prio()
    if grammar is None:
        F_.check(lib().ptv_chord_decode(_CDS.pointers(tens, out), _CDS.dims(dims), stream_ptr()), 'ptv_chord_decode')
        _CDS.count()
    else:
        n_vocab = grammar.vocab.shape[0]
        tens.update(RULE=grammar.rule, VOCAB=grammar.vocab if n_vocab else None)
        dims.update(RULE_ROWS=grammar.rule.shape[0], N_VOCAB=n_vocab)
        F_.check(lib().ptv_chord_decode_grammar(_CDG.pointers(tens, out), _CDG.dims(dims), stream_ptr()), 'ptv_chord_decode_grammar')
        _CDG.count()
    lp = ChordLogprob(out['LOGP'], out['LOGQ'], out['FORCED'], out['ERR'], out['STEP_LOGP'], out['STEP_LOGQ'], out['STEP_FORCED'])
    return ChordDecode(out['C'], out['CHORD14'], out['ROOT'], out['CHROMA'], out['BASS'], lp)
