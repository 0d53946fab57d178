"""Network blocks of the polyphonic chord/texture VAE on MI355X HIP kernels.

Host-side mirror of the reference `ptvae.py`: same class names, constructor signatures, method
names, `state_dict` keys and default initialisation (same RNG draws, so `torch.manual_seed(s)`
gives the reference's weights).  The modules hold parameters only; every forward/backward is a
sequence of libptvae_hip.so kernels (see functional.py).  There is no CPU fallback: calling a
module with CPU tensors raises.

Reference: /root/reference/ptvae.py  (RnnEncoder :11-29, RnnDecoder :32-87, TextureEncoder :90-122,
PtvaeEncoder :125-215, PtvaeDecoder :218-575).
"""
import collections
import math
import os
import random

import torch
from torch import nn

from . import functional as F_
from . import functional_free as FF_
from ._lib import prec_code

# stream slot of the ground-truth note summaries (functional.Side; autograd replays their BPTT on the same stream): -1 = the caller's
SUMMARY_SLOT = 5


# ---------------------------------------------------------------------------------------------
# parameter containers (same names / shapes / init order as torch.nn.{Linear,GRU,Conv2d})
# ---------------------------------------------------------------------------------------------
class Linear(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1 / math.sqrt(in_features) if in_features > 0 else 0
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, prec=0):
        shp = x.shape
        y = F_.LinearFn.apply(x.reshape(-1, shp[-1]), self.weight, self.bias, prec)
        return y.view(shp[:-1] + (self.out_features,))


class GRU(nn.Module):
    """Parameters of a single-layer (bi)GRU, keys weight_ih_l0 ... bias_hh_l0[_reverse]."""

    def __init__(self, input_size, hidden_size, bidirectional=False):
        super().__init__()
        self.input_size, self.hidden_size, self.bidirectional = input_size, hidden_size, bidirectional
        for sfx in ([''] + (['_reverse'] if bidirectional else [])):
            setattr(self, 'weight_ih_l0' + sfx, nn.Parameter(torch.empty(3 * hidden_size, input_size)))
            setattr(self, 'weight_hh_l0' + sfx, nn.Parameter(torch.empty(3 * hidden_size, hidden_size)))
            setattr(self, 'bias_ih_l0' + sfx, nn.Parameter(torch.empty(3 * hidden_size)))
            setattr(self, 'bias_hh_l0' + sfx, nn.Parameter(torch.empty(3 * hidden_size)))
        stdv = 1.0 / math.sqrt(hidden_size) if hidden_size > 0 else 0
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def weights(self):
        names = ['weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0']
        if self.bidirectional:
            names += [n + '_reverse' for n in names]
        return [getattr(self, n) for n in names]


class Conv2dParams(nn.Module):
    def __init__(self, in_ch, out_ch, kernel_size):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_ch, in_ch, *kernel_size))
        self.bias = nn.Parameter(torch.empty(out_ch))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        fan_in = in_ch * kernel_size[0] * kernel_size[1]
        bound = 1 / math.sqrt(fan_in)
        nn.init.uniform_(self.bias, -bound, bound)


class HipNormal:
    """Duck-typed torch.distributions.Normal (`.mean`, `.scale`, `.loc`, `.stddev`, `.rsample()`,
    `.sample()`) whose rsample runs the reparameterisation kernel.  The model's run() returns
    these where the reference returns Normal (model.py:45-48)."""

    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale

    mean = property(lambda self: self.loc)
    stddev = property(lambda self: self.scale)
    variance = property(lambda self: self.scale * self.scale)

    def rsample(self, sample_shape=torch.Size(), eps=None):
        if eps is None:
            eps = torch.randn(self.loc.shape, device=self.loc.device, dtype=self.loc.dtype)
        return F_.ReparamFn.apply(self.loc, self.scale, eps.contiguous())

    def sample(self, sample_shape=torch.Size()):
        with torch.no_grad():
            return self.rsample(sample_shape)


def _require_cuda(t, who):
    if not t.is_cuda:
        raise RuntimeError('%s: input is on %s -- this build runs on MI355X HIP kernels only (no CPU '
                           'fallback); move the model and inputs to a cuda device' % (who, t.device))


class _PrecMixin:
    """`precision` = 'fp32' (exact fp32 MFMA, parity path) or 'bf16' (bf16 MFMA operands)."""
    precision = 'fp32'

    @property
    def _prec(self):
        return prec_code(self.precision)


# ---------------------------------------------------------------------------------------------
class RnnEncoder(nn.Module, _PrecMixin):
    """Chord encoder: bi-GRU over 8 chord steps -> Normal(mu, exp(linear_var)).  ptvae.py:11-29"""

    def __init__(self, input_dim, hidden_dim, z_dim):
        super().__init__()
        self.gru = GRU(input_dim, hidden_dim, bidirectional=True)
        self.linear_mu = Linear(hidden_dim * 2, z_dim)
        self.linear_var = Linear(hidden_dim * 2, z_dim)
        self.input_dim, self.hidden_dim, self.z_dim = input_dim, hidden_dim, z_dim

    def forward(self, x):
        _require_cuda(x, 'RnnEncoder')
        x_sm = F_.Transpose01Fn.apply(x.float())                       # [T,B,I]
        h = F_.BiGruFinalFn.apply(x_sm, None, self._prec, *self.gru.weights())
        mu, sd = F_.EncoderHeadsFn.apply(h, self.linear_mu.weight, self.linear_mu.bias, self.linear_var.weight,
                                         self.linear_var.bias, self._prec)
        return HipNormal(mu, sd)


class TextureEncoder(nn.Module, _PrecMixin):
    """Piano-roll texture encoder (ptvae.py:90-122): conv(4x12,stride 4x1)+ReLU+maxpool(1x4) ->
    raw view [B,8,C*29] -> fc1 -> fc2 -> bi-GRU(8 steps) -> Normal."""

    def __init__(self, emb_size, hidden_dim, z_dim, num_channel=10):
        super().__init__()
        self.cnn = nn.Sequential(Conv2dParams(1, num_channel, (4, 12)))     # key 'cnn.0.*' as in the reference
        self.fc1 = Linear(num_channel * 29, 1000)
        self.fc2 = Linear(1000, emb_size)
        self.gru = GRU(emb_size, hidden_dim, bidirectional=True)
        self.linear_mu = Linear(hidden_dim * 2, z_dim)
        self.linear_var = Linear(hidden_dim * 2, z_dim)
        self.emb_size, self.hidden_dim, self.z_dim = emb_size, hidden_dim, z_dim

    def forward(self, pr):
        _require_cuda(pr, 'TextureEncoder')
        bs = pr.size(0)
        conv = self.cnn[0]
        feat = F_.TextureFrontFn.apply(pr.float(), conv.weight, conv.bias)              # [B*8, C*29]: the reference's raw .view(bs, 8, -1) of [B,C,8,29]
        feat = F_.LinearFn.apply(feat, self.fc1.weight, self.fc1.bias, self._prec)
        feat = F_.LinearFn.apply(feat, self.fc2.weight, self.fc2.bias, self._prec)
        x_sm = F_.Transpose01Fn.apply(feat.view(bs, 8, -1))
        h = F_.BiGruFinalFn.apply(x_sm, None, self._prec, *self.gru.weights())
        mu, sd = F_.EncoderHeadsFn.apply(h, self.linear_mu.weight, self.linear_mu.bias, self.linear_var.weight,
                                         self.linear_var.bias, self._prec)
        return HipNormal(mu, sd)


class RnnDecoder(nn.Module, _PrecMixin):
    """Chord decoder (ptvae.py:32-87)."""

    def __init__(self, input_dim=36, z_input_dim=256, hidden_dim=512, z_dim=256, num_step=32):
        super().__init__()
        self.z2dec_hid = Linear(z_dim, hidden_dim)
        self.z2dec_in = Linear(z_dim, z_input_dim)
        self.gru = GRU(input_dim + z_input_dim, hidden_dim)
        self.init_input = nn.Parameter(torch.rand(36))
        self.input_dim, self.hidden_dim, self.z_dim = input_dim, hidden_dim, z_dim
        self.root_out = Linear(hidden_dim, 12)
        self.chroma_out = Linear(hidden_dim, 24)
        self.bass_out = Linear(hidden_dim, 12)
        self.num_step = num_step
        self.force_trace = None            # {'root' [B,8,12], 'chroma' [B,8,12,2], 'bass' [B,8,12]} logits: replay mode (tests)
        self.last_chord_logits = None      # step-major (root, chroma, bass) logits of the last decode_chords()

    def _params(self):
        sd = dict(self.named_parameters())
        return [sd[n] for n in F_.CHD_PARAM_NAMES]

    def draw_coins(self, tfr):
        """one teacher-forcing coin per chord step for the whole batch (ptvae.py:81; the `break` at :79
        never fires, so 8 draws)"""
        return [random.random() < tfr for _ in range(int(self.num_step / 4))]

    def forward(self, z_chd, inference, tfr, c=None, coins=None):
        _require_cuda(z_chd, 'RnnDecoder')
        T = int(self.num_step / 4)
        if inference:
            tfr = 0.
        if coins is None:
            coins = self.draw_coins(tfr)
        c_sm = F_.Transpose01Fn.apply(c.float()).detach() if (c is not None and not inference) else None
        if all(coins) and not inference:
            root, chroma, bass = F_.ChordDecoderTFFn.apply(z_chd, c_sm, self._prec, *self._params())
        else:
            force = None
            if self.force_trace is not None:
                ft = self.force_trace
                force = {'root': ft['root'].float().transpose(0, 1).contiguous(), 'bass': ft['bass'].float().transpose(0, 1).contiguous(),
                         'chroma': ft['chroma'].float().reshape(z_chd.size(0), T, 24).transpose(0, 1).contiguous()}
            root, chroma, bass = FF_.ChordDecoderStepFn.apply(z_chd, c_sm, list(coins), force, self._prec, *self._params())
        bs = z_chd.size(0)
        # reference shapes [B,8,12] / [B,8,12,2] / [B,8,12] as views of the step-major buffers
        return root.transpose(0, 1), chroma.view(T, bs, 12, 2).transpose(0, 1), bass.transpose(0, 1)

    def decode_tokens(self, z_chd):
        """Inference chord decode of z_chd [B, z_dim] -> (c [B,8,36], chord14 [B,8,14]) on the device: per step and sample the token
        the reference feeds back (root one-hot | 12 chroma bits | bass one-hot, ptvae.py:72-78) and the same chord in the bank
        layout batch_transform reads (root index | chroma bits | bass index).  No autograd graph."""
        _require_cuda(z_chd, 'RnnDecoder.decode_tokens')
        T = int(self.num_step / 4)
        with torch.no_grad():
            root, chroma, bass = self.forward(z_chd.detach(), True, 0.)
            # forward() hands out reference-shaped views of its step-major buffers: undo them
            return chord_tokens(root.transpose(0, 1), chroma.transpose(0, 1).reshape(T, z_chd.size(0), 24), bass.transpose(0, 1))

    def decode_chords(self, z_chd, *, temperature=None, chroma_temperature=None, seed=7, draw=0, sample_offset=0, keep=None,
                      return_logprob=False, grammar=None):
        """Row-independent free-running chord decode of z_chd [B, z_dim] -> (c [B,8,36], chord14 [B,8,14]) on the device (ptv_chord_decode,
        one C call; INTEGRATION.md "Chord decode").  Every row feeds back its OWN token: unlike decode_tokens -- which keeps the
        reference's union over the batch (ptvae.py:74-77) -- a row's chords do not depend on the rest of the batch; at B = 1 the two agree.
        temperature (root and bass) / chroma_temperature (the 12 chroma bits; default: temperature), floats >= 0: the decisions are
        draws from softmax(logits / T), Philox noise keyed by (seed, draw, sample_offset + row, chord step); None: the argmax.
        keep: a functional_free.ChordKeep (DisentangleVAE.keep_chords) whose steps are forced and fed back like decisions.
        grammar: a functional_free.ChordGrammar (DisentangleVAE.chord_grammar; INTEGRATION.md "Chord grammar"): allowed roots and pitch
        classes, a chord-quality vocabulary, a chord-tone bass -- ptv_chord_decode_grammar; ChordLogprob.logq is then taken over the
        allowed sets, and err carries the grammar's yield bits.
        return_logprob=True appends a ChordLogprob(logp [B,3], logq [B,3], forced [B,3], err [B], step_logp [B,8,3], step_logq [B,8,3],
        step_forced [B,8,3]) of device tensors, heads in the order (root, chroma, bass).  The step-major logits of the decode stay in
        last_chord_logits = (root [8,B,12], chroma [8,B,24], bass [8,B,12]).  No autograd graph, no synchronisation."""
        sampled = FF_.check_chord_sampling(temperature, chroma_temperature, *((seed, draw, sample_offset) if temperature is not None
                                                                             else (None, None, None)))
        if not torch.is_tensor(z_chd) or z_chd.dim() != 2 or z_chd.shape[0] < 1 or z_chd.shape[1] != self.z_dim:
            raise ValueError('z_chd must be a tensor [B, %d]' % self.z_dim)
        FF_.check_chord_keep(keep, z_chd.shape[0])
        FF_.check_chord_grammar(grammar, z_chd.shape[0])
        _require_cuda(z_chd, 'RnnDecoder.decode_chords')
        if grammar is not None and grammar.rule.device != z_chd.device:
            raise ValueError('the chord grammar must be on the device of z_chd (%s), it is on %s' % (z_chd.device, grammar.rule.device))
        if int(self.num_step / 4) != FF_.CHORD_STEPS:
            raise NotImplementedError('the chord decode is built for 8 chord steps')
        with torch.no_grad():
            block = FF_.sampling_block(z_chd.device, temperature, chroma_temperature, seed, draw, sample_offset) if sampled else None
            out = FF_.chord_decode(z_chd, dict(zip(F_.CHD_PARAM_NAMES, self._params())), self._prec, block, keep, grammar)
        self.last_chord_logits = (out.root, out.chroma, out.bass)
        return (out.c, out.chord14, out.logprob) if return_logprob else (out.c, out.chord14)


def chord_tokens(root, chroma, bass):
    """Chord-decoder logits in step-major layout (root [T,B,12], chroma [T,B,24] as 12 pairs, bass [T,B,12]) -> (c [B,T,36],
    chord14 [B,T,14]) f32 (ptv_chord_tokens); argmax ties go to the lowest index.  No synchronisation."""
    _require_cuda(root, 'chord_tokens')
    root, chroma, bass = (a.detach().float().contiguous() for a in (root, chroma, bass))
    T, B = root.shape[0], root.shape[1]
    assert root.shape == (T, B, 12) and chroma.shape == (T, B, 24) and bass.shape == (T, B, 12), 'step-major [T,B,12|24|12] logits'
    c = torch.empty(B, T, 36, device=root.device, dtype=torch.float32)
    chord14 = torch.empty(B, T, 14, device=root.device, dtype=torch.float32)
    F_.call('ptv_chord_tokens', F_.ptr(root), F_.ptr(chroma), F_.ptr(bass), F_.ptr(c), F_.ptr(chord14), T, B, F_.stream_ptr())
    return c, chord14


DecodeLogprob = collections.namedtuple('DecodeLogprob', 'logp logq counts err step_logp step_counts')
LastDecode = collections.namedtuple('LastDecode', 'pitch dur xhat sampling force')      # what an inference decode leaves for decode_logprob()


class _DecodeGraph(collections.namedtuple('_DecodeGraph', 'graph z outs block mask mask_addr force rows rows_addr run',
                                          defaults=(None, None, None))):
    """one captured inference decode: graph, z (static input), outs (static outputs), block / mask / mask_addr (static sampling block, the
    static pitch mask of a constrained one and the one-word tensor holding that mask's address; None where the kind has none), force (the
    static force arrays of a decode with kept steps, or None), rows / rows_addr (the static row table of a row-wise decode and the
    one-word tensor holding its address, or None), run (the static functional_free.SoundingRun of a decode with sounding rules, or None:
    its Sounding holds static tables and a static control word, its base tables are static too -- force['pitch'] is then its force_eff,
    mask its mask_base and mask_addr the address of its mask_eff)"""

    def refresh(self, z, sampling, keep, sounding=None):
        """the caller's inputs into the static tensors, before every replay"""
        self.z.copy_(z)
        if self.run is not None:
            return self._refresh_sounding(sampling, keep, sounding)
        if self.force is not None:
            self.force['pitch'].copy_(keep.pitch)
            self.force['dur'].copy_(keep.dur)
        if self.block is not None:
            self.block.copy_(sampling)
            if self.mask is not None and sampling.pitch_mask is not None:
                self.mask[:sampling.pitch_mask.shape[0]].copy_(sampling.pitch_mask)   # (a one-row mask: row 0, the block's flag says so)
                self.block[7:8].copy_(self.mask_addr)
            if self.rows is not None:
                self.rows.copy_(sampling.rows.table)
                self.block[8:9].copy_(self.rows_addr)

    def _refresh_sounding(self, sampling, keep, sounding):
        """a decode with sounding rules: the caller's rules, mask and keep into the static BASE tables (every table has a row per sample
        here, so one capture serves every Sounding); the block keeps pointing at the effective mask"""
        run, B = self.run, self.z.shape[0]
        run.snd.control.copy_(sounding.control)
        for dst, src in zip(run.snd.tables(), sounding.tables()):
            dst.copy_(src.expand(B, 32))
        if keep is None:
            run.force_base.fill_(-1)
            self.force['dur'].fill_(-1)
        else:
            run.force_base.copy_(keep.pitch)
            self.force['dur'].copy_(keep.dur)
        if self.block is not None:
            self.block.copy_(sampling)
            if self.mask is not None:
                if sampling.pitch_mask is None:
                    self.mask.fill_(-1)
                else:
                    self.mask.copy_(sampling.pitch_mask.expand(B, 32, 4))
                self.block[6:7].bitwise_and_(~FF_.CONS_MASK_ROW1)
                self.block[7:8].copy_(self.mask_addr)
            if self.rows is not None:
                self.rows.copy_(sampling.rows.table)
                self.block[8:9].copy_(self.rows_addr)


class PtvaeDecoder(nn.Module, _PrecMixin):
    """PianoTree decoder (ptvae.py:218-575): time GRU (32) -> notes GRU (15) -> pitch head +
    5-step duration GRU."""

    def __init__(self, device=None, note_embedding=None, max_simu_note=16, max_pitch=127, min_pitch=0,
                 pitch_sos=128, pitch_eos=129, pitch_pad=130, dur_pad=2, dur_width=5, num_step=32,
                 note_emb_size=128, z_size=512, dec_emb_hid_size=128, dec_time_hid_size=1024,
                 dec_notes_hid_size=512, dec_z_in_size=256, dec_dur_hid_size=16):
        super().__init__()
        self.max_pitch, self.min_pitch = max_pitch, min_pitch
        self.pitch_sos, self.pitch_eos, self.pitch_pad = pitch_sos, pitch_eos, pitch_pad
        self.pitch_range = max_pitch - min_pitch + 3
        self.dur_pad, self.dur_width = dur_pad, dur_width
        self.note_size = self.pitch_range + dur_width
        self.max_simu_note, self.num_step = max_simu_note, num_step
        self.device = device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu')
        if (max_simu_note, num_step, dur_width, self.pitch_range, pitch_pad, dur_pad) != (16, 32, 5, 130, 130, 2):
            raise NotImplementedError('HIP kernels are specialised to the 32x16x(130+5) PianoTree grid')
        self.note_emb_size, self.z_size = note_emb_size, z_size
        self.dec_z_in_size, self.dec_emb_hid_size = dec_z_in_size, dec_emb_hid_size
        self.dec_time_hid_size, self.dec_notes_hid_size = dec_time_hid_size, dec_notes_hid_size
        self.dec_dur_hid_size = dec_dur_hid_size
        self.dec_init_input = nn.Parameter(torch.rand(2 * dec_emb_hid_size))
        self.dur_sos_token = nn.Parameter(torch.rand(dur_width))
        self.note_embedding = Linear(self.note_size, note_emb_size) if note_embedding is None else note_embedding
        self.z2dec_hid_linear = Linear(z_size, dec_time_hid_size)
        self.z2dec_in_linear = Linear(z_size, dec_z_in_size)
        self.dec_notes_emb_gru = GRU(note_emb_size, dec_emb_hid_size, bidirectional=True)
        self.dec_time_gru = GRU(dec_z_in_size + 2 * dec_emb_hid_size, dec_time_hid_size)
        self.dec_time_to_notes_hid = Linear(dec_time_hid_size, dec_notes_hid_size)
        self.dec_notes_gru = GRU(dec_time_hid_size + note_emb_size, dec_notes_hid_size)
        self.pitch_out_linear = Linear(dec_notes_hid_size, self.pitch_range)
        self.dec_dur_gru = GRU(dur_width, dec_dur_hid_size)
        self.dur_hid_linear = Linear(self.pitch_range + dec_notes_hid_size, dec_dur_hid_size)
        self.dur_out_linear = Linear(dec_dur_hid_size, 2)
        self.force_dur_idx = None          # [5, 480*B] int32: replay the oracle's duration argmaxes (tests)
        self.force_trace = None            # {'pitch': [15, 32B] int32, 'dur': [5, 480B] int32}: replay mode (tests)
        self.last_xhat = None              # predicted grid [B,32,16,6] int64 of the last step-loop decode
        self.use_graph = False             # replay inference decodes from a captured hipGraph
        self._graphs = {}
        self._graph_stream = None          # warm-up and capture stream of _graph_decode (one per decoder: the library keeps a workspace per stream)
        self.graph_captures = 0            # inference decodes captured so far (a sampled decode's seed / draw / temperatures need no new one)
        self._train_graphs = {}
        self._summary = None
        self.summaries_needed = True       # emb_x() starts the ground-truth note summaries early unless told they are dead values
        self.last_dur_idx = None
        self._last_decode = None           # LastDecode of the last inference decode: decode_logprob()
        self.last_sounding = None          # (mask_eff or None, force_pitch_eff or None, held) of the last inference decode with sounding=
        self._graph_effective = None

    def _params(self):
        sd = dict(self.named_parameters())
        return [sd[n] for n in F_.DEC_PARAM_NAMES]

    def _graph_decode(self, z, coins, sampling=None, keep=None, sounding=None):
        """Free-running decode replayed from a captured hipGraph: the step loop is ~9,000 tiny launches whose order and arguments depend
        only on (B, precision) -- capture once, then one graph launch per call.  The graph holds raw parameter pointers, so it is
        re-captured if the parameter storage moves.  Each kind of decode (functional_free.BlockKind: argmax, sampled, truncated,
        constrained, row-wise) is a graph of its own (other kernels), and kept steps (keep: functional_free.Keep) double the kinds: the key holds
        the kind number and, only with a keep, one more element.  What a caller may vary -- z, seed / draw / temperatures / top_k / min_p
        / top_p / flags in the block, the pitch mask, the row table, the force arrays of a keep -- lives in static tensors that _DecodeGraph.refresh
        fills before every replay, so one capture per key serves them all.  A decode with sounding rules (sounding: functional_free.Sounding)
        has one more key element instead of the keep's: its graph always holds force arrays, the base and effective tables, the state and
        the control word as static tensors, so one capture serves every Sounding, with a keep or without."""
        ps = self._params_free()
        kind = FF_.block_kind(sampling)
        key = (z.shape[0], self._prec, z.device.index, tuple(p.data_ptr() for p in ps), kind.kind) + ((True,) if keep is not None and sounding is None else ()) \
            + (('sounding',) if sounding is not None else ())
        ent = self._graphs.get(key)
        if ent is None and sounding is not None:
            ent = self._graphs[key] = self._capture_sounding(z, coins, sampling, keep, sounding, kind, ps, key)
        if ent is None:
            block = mask = mask_addr = rows = rows_addr = None
            if kind.cons:                                      # (captured with every pitch allowed; the flags are the first caller's)
                mask = torch.full((z.shape[0], 32, 4), -1, dtype=torch.int32, device=z.device)
                mask_addr = torch.tensor([mask.data_ptr()], dtype=torch.int64, device=z.device)
            if sampling is not None:
                block = FF_.clone_block(sampling, mask)
                ps = ps + [block]
            if kind.cons:
                block[7:8].copy_(mask_addr if sampling.pitch_mask is not None else torch.zeros_like(mask_addr))
            if kind.rows:                                      # (a static table: any caller's table is copied into it before a replay)
                rows = sampling.rows.table.clone()
                rows_addr = torch.tensor([rows.data_ptr()], dtype=torch.int64, device=z.device)
                block.rows = FF_.RowSampling(rows, z.shape[0])
                block[8:9].copy_(rows_addr)
            static_z = z.detach().clone()
            force = None if keep is None else {'pitch': keep.pitch.clone(), 'dur': keep.dur.clone()}
            cur = torch.cuda.current_stream()
            # warm-up and capture share ONE stream (as graph_step.py): the library's split-K workspaces are per stream and cannot be
            # allocated inside a capture -- captured on another stream the small products fell back to fp32 atomics, and the replayed
            # logits differed from the eager ones in the last bits from replay to replay (which a truncation threshold turns into
            # other decisions)
            s = self._graph_stream = self._graph_stream or torch.cuda.Stream(device=z.device)
            s.wait_stream(cur)
            with torch.cuda.stream(s):                         # warm-up outside capture (lazy inits, allocator)
                FF_.DecoderStepFn.apply(static_z, None, None, coins, True, force, self._prec, *ps)
            cur.wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                outs = FF_.DecoderStepFn.apply(static_z, None, None, coins, True, force, self._prec, *ps)
            for k in [k for k in self._graphs if k[4:] == key[4:]]:         # one graph per kind (argmax, sampled, truncated, constrained; each
                del self._graphs[k]                                         # with and without kept steps) is kept
            self.graph_captures += 1
            ent = self._graphs[key] = _DecodeGraph(g, static_z, outs, block, mask, mask_addr, force, rows, rows_addr)
        ent.refresh(z, sampling, keep, sounding)
        ent.graph.replay()
        if ent.run is not None:                                # what decode_logprob() and last_sounding read: the effective arrays
            self._graph_effective = (ent.block, ent.force, ent.run)
        return ent.outs

    def _capture_sounding(self, z, coins, sampling, keep, sounding, kind, ps, key):
        """the _DecodeGraph of a decode with sounding rules (see _graph_decode): static tables with a row per sample, every rule wired --
        the mask rule wherever the kind has a mask, the count rule always; what a Sounding switches off it switches off in its tables"""
        B, dev = z.shape[0], z.device
        u8 = dict(dtype=torch.uint8, device=dev)
        snd = FF_.Sounding(sounding.control.clone(), torch.zeros(B, 32, **u8), torch.zeros(B, 32, **u8), torch.ones(B, 32, **u8), B,
                           True, True, True)
        block = mask = mask_addr = rows = rows_addr = None
        if kind.cons:
            mask = torch.full((B, 32, 4), -1, dtype=torch.int32, device=dev)
        force_base = torch.full((15, 32 * B), -1, dtype=torch.int32, device=dev)
        run = FF_.SoundingRun(snd, B, dev, mask=bool(kind.cons), mask_base=mask, force=True, force_base=force_base)
        if sampling is not None:
            block = FF_.sounding_block(sampling, run.mask_eff) if kind.cons else FF_.clone_block(sampling)
            ps = ps + [block]
        if kind.cons:
            mask_addr = torch.tensor([run.mask_eff.data_ptr()], dtype=torch.int64, device=dev)
        if kind.rows:
            rows = sampling.rows.table.clone()
            rows_addr = torch.tensor([rows.data_ptr()], dtype=torch.int64, device=dev)
            block.rows = FF_.RowSampling(rows, B)
            block[8:9].copy_(rows_addr)
        static_z = z.detach().clone()
        force = {'pitch': run.force_eff, 'dur': torch.full((5, 480 * B), -1, dtype=torch.int32, device=dev), 'sounding': run}
        ent = _DecodeGraph(None, static_z, None, block, mask, mask_addr, force, rows, rows_addr, run)
        ent.refresh(z, sampling, keep, sounding)               # (warm-up and capture run on the first caller's tables)
        cur = torch.cuda.current_stream()
        s = self._graph_stream = self._graph_stream or torch.cuda.Stream(device=dev)      # (one stream for both: see _graph_decode)
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            FF_.DecoderStepFn.apply(static_z, None, None, coins, True, force, self._prec, *ps)
        cur.wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs = FF_.DecoderStepFn.apply(static_z, None, None, coins, True, force, self._prec, *ps)
        for k in [k for k in self._graphs if k[4:] == key[4:]]:
            del self._graphs[k]
        self.graph_captures += 1
        return ent._replace(graph=g, outs=outs)

    def _params_free(self):
        sd = dict(self.named_parameters())
        return [sd[n] for n in FF_.FREE_PARAM_NAMES]

    # ---- ptvae.py:531-535 (+ :292-313)
    def emb_x(self, x):
        """-> (embedded [B,32,16,E], lengths [B,32]).  Shapes are the reference's; the memory behind
        them is the decoder's step-major layout ([16,32,B,E] / [32,B]) exposed through permuted views,
        so handing them back to `decoder()` costs no transpose (134 MB each way at B=512)."""
        _require_cuda(x, 'PtvaeDecoder.emb_x')
        emb, lengths = F_.EmbedFn.apply(x.long(), self.note_embedding.weight, self.note_embedding.bias, self._prec)
        # The ground-truth note summaries (packed bi-GRU over the embedded notes, ptvae.py:446-453) depend
        # on the embedding only: start them now on a sibling stream so they overlap the encoders;
        # decoder() picks the result up.
        # (not when the caller knows that no time step will be teacher-forced -- DisentangleVAE.run with tfr1 = 0, the reference's
        # schedule from its third batch on: the summaries are then dead values with zero gradient, ptvae.py:476-478)
        self._summary = None
        if self.summaries_needed:
            if SUMMARY_SLOT < 0:                             # on the caller's stream (idle while the encoders run)
                self._summary = (emb, self._summarize(emb, lengths), None)
            else:
                side = F_.Side(SUMMARY_SLOT)
                xs = side(lambda: self._summarize(emb, lengths), emb, lengths)
                self._summary = (emb, xs, side)
        return emb.permute(2, 1, 0, 3), lengths.view(32, x.size(0)).t()

    def _summarize(self, emb, len32):
        n, t, b, e = emb.shape
        F_.emb_link_arm(emb)
        return F_.BiGruFinalFn.apply(emb.view(n, t * b, e), len32, self._prec, *self.dec_notes_emb_gru.weights())

    def draw_coins(self, tfr1, tfr2):
        """Teacher-forcing decisions in the reference's draw order (ptvae.py:420,476): per time step 14
        note-level coins (tfr2), then one time-level coin (tfr1) for t < 31 -> (notes [32][14], time [31])."""
        notes, time = [], []
        for t in range(self.num_step):
            notes.append([random.random() < tfr2 for _ in range(self.max_simu_note - 2)])
            if t < self.num_step - 1:
                time.append(random.random() < tfr1)
        return notes, time

    def decoder(self, z, inference, x, lengths, teacher_forcing_ratio1, teacher_forcing_ratio2, coins=None, *, live=None, sampling=None,
                keep=None, sounding=None):
        """sampling: None (argmax decisions) or a block of functional_free.sampling_block() -- the decisions of the free-running decode
        are then seeded draws from softmax(logits / T), with top_k / min_p / top_p in the block over the truncated support of the pitch row,
        and with pitch_mask / ascending over the allowed classes only (temperature 0: the constrained argmax);
        inference only (ValueError otherwise, before any launch).
        keep: None or a functional_free.Keep (DisentangleVAE.keep) -- the decisions of its kept time steps are forced where they are taken,
        so they reach the following steps as if decided; everything else is decided as without it.  Its rows are the rows of z.  Inference
        only, and not together with force_trace (ValueError before any launch).
        sounding: None or a functional_free.Sounding (DisentangleVAE.sounding) -- between two time steps the next step's mask row and
        pitch force words are rewritten from what is sounding (INTEGRATION.md "Sounding state"); the decode runs on the EFFECTIVE arrays,
        which last_sounding = (mask_eff or None, force_pitch_eff or None, held) and decode_logprob() then read.  Inference only, not
        together with force_trace; no_restrike or a floor needs a constrained block (ValueError before any launch)"""
        if sounding is not None:
            if not inference or teacher_forcing_ratio1 != 0 or teacher_forcing_ratio2 != 0 or coins is not None:
                raise ValueError('sounding is inference only: it cannot be combined with training or teacher forcing')
            FF_.check_sounding(sounding, z.size(0), z.device)
            if self.force_trace is not None:
                raise ValueError('sounding cannot be combined with force_trace: both fill the force arrays')
            if sounding.needs_constrained and not (torch.is_tensor(sampling) and FF_.block_kind(sampling).cons):
                raise ValueError('sounding with no_restrike or min_sounding needs a constrained block (functional_free.sampling_block(..., '
                                 'ascending=False) at least): only the constrained kernels honour its mask and its words')
        if sampling is not None and (not inference or teacher_forcing_ratio1 != 0 or teacher_forcing_ratio2 != 0 or coins is not None):
            raise ValueError('sampling is inference only: it cannot be combined with training or teacher forcing')
        if keep is not None:
            if not inference or teacher_forcing_ratio1 != 0 or teacher_forcing_ratio2 != 0 or coins is not None:
                raise ValueError('keep is inference only: it cannot be combined with training or teacher forcing')
            FF_.check_keep(keep, z.size(0))
            cons = sampling is not None and torch.is_tensor(sampling) and FF_.block_kind(sampling).cons
            if keep.needs_constrained and not cons:
                raise ValueError('a %s needs a constrained block (functional_free.sampling_block(..., ascending=%s)%s): only the '
                                 'constrained kernels honour its words'
                                 % (type(keep).__name__, keep.needs_ascending, '' if keep.needs_ascending else ' at least'))
            if keep.needs_ascending and not getattr(sampling, 'ascending', False):
                raise ValueError('a %s needs a constrained block with the ascending flag (functional_free.sampling_block(..., '
                                 'ascending=True)): its ceilings count on ascending notes' % (type(keep).__name__,))
            if self.force_trace is not None:
                raise ValueError('keep cannot be combined with force_trace: both fill the force arrays')
        _require_cuda(z, 'PtvaeDecoder')
        B = z.size(0)
        if inference:
            assert x is None and lengths is None
            assert teacher_forcing_ratio1 == 0 and teacher_forcing_ratio2 == 0
            coins = ([[False] * (self.max_simu_note - 2)] * self.num_step, [False] * (self.num_step - 1))
            smp = () if sampling is None else (FF_._check_block(sampling, z.device, B),)
            force = self.force_trace if keep is None else {'pitch': keep.pitch, 'dur': keep.dur}
            graphed = self.use_graph and not torch.is_grad_enabled() and self.force_trace is None
            self.last_sounding = run = None
            if sounding is not None and not graphed:
                sampling, force, run = self._sounding_run(z, sampling, keep, sounding)
                smp = () if sampling is None else (sampling,)
            if graphed:
                pitch, dur, xhat, idx = self._graph_decode(z, coins, sampling, keep, sounding)
                if sounding is not None:
                    sampling, force, run = self._graph_effective
            else:
                pitch, dur, xhat, idx = FF_.DecoderStepFn.apply(z, None, None, coins, True, force, self._prec,
                                                                *self._params_free(), *smp)
            if run is not None:
                force = {'pitch': force.get('pitch'), 'dur': force.get('dur')} if force else None
                self.last_sounding = (run.mask_eff, run.force_eff, run.held)
            self.last_dur_idx, self.last_xhat = idx, xhat
            self._last_decode = LastDecode(pitch, dur, xhat, sampling, force)      # what decode_logprob() reads: references, nothing copied (an eager decode's logits live until the next decode)
            return pitch.permute(2, 1, 0, 3), dur.view(15, 32, B, 5, 2).permute(2, 1, 0, 3, 4)
        if coins is None:
            coins = self.draw_coins(teacher_forcing_ratio1, teacher_forcing_ratio2)
        all_tf = all(all(r) for r in coins[0]) and all(coins[1])
        emb = x.permute(2, 1, 0, 3)                                            # [16,32,B,E]
        if not emb.is_contiguous():                                            # caller built a plain [B,32,16,E]
            E = x.size(-1)
            emb = F_.Transpose01Fn.apply(x.transpose(1, 2).reshape(B, 16 * 32, E)).view(16, 32, B, E)
        len32 = lengths.t()
        len32 = (len32 if (len32.is_contiguous() and len32.dtype == torch.int32) else len32.contiguous().int()).reshape(-1)
        cached = getattr(self, '_summary', None)
        self._summary = None
        if cached is not None and cached[0].data_ptr() == emb.data_ptr() and cached[0].shape == emb.shape:
            xs = cached[1]
            if cached[2] is not None:
                cached[2].join()
        elif any(coins[1]):
            xs = self._summarize(emb, len32)
        else:
            xs = None                                                          # no time step reads a ground-truth summary
        if not all_tf:
            none_tf = not any(any(r) for r in coins[0]) and not any(coins[1])
            if self.use_graph and none_tf and self.force_trace is None and torch.is_grad_enabled():
                # free-running training step: forward replayed from a captured hipGraph
                pitch, dur, xhat, idx = FF_.graphed_decoder_step(self._train_graphs, z, emb, xs, self._prec, *self._params_free())
            else:
                pitch, dur, xhat, idx = FF_.DecoderStepFn.apply(z, emb, xs, coins, False, self.force_trace, self._prec,
                                                                *self._params_free())
            if live is not None:
                live.record_order(False)                                       # (every step computed, rows in (t, b) order)
            self.last_dur_idx, self.last_xhat = idx, xhat
            return pitch.permute(2, 1, 0, 3), dur.view(15, 32, B, 5, 2).permute(2, 1, 0, 3, 4)
        pitch, dur, idx = F_.DecoderTFFn.apply(z, emb, xs, self.force_dur_idx, live, self._prec, *self._params())
        self.last_dur_idx = idx
        # reference shapes [B,32,15,130] / [B,32,15,5,2] as permuted views of the step-major buffers
        return pitch.permute(2, 1, 0, 3), dur.view(15, 32, B, 5, 2).permute(2, 1, 0, 3, 4)

    def _sounding_run(self, z, sampling, keep, sounding):
        """an eager decode with sounding rules -> (the effective block, the force dict of DecoderStepFn, the SoundingRun): the effective
        arrays are allocated here -- a mask only where no_restrike is on, force arrays only where a count rule is on or a keep is given
        (an all-free keep where the caller gave none) -- and the block is cloned with mask_eff's address"""
        B, dev = z.size(0), z.device
        want_mask = sounding.no_restrike
        want_force = sounding.needs_force or keep is not None
        mask_base = getattr(sampling, 'pitch_mask', None) if want_mask else None
        run = FF_.SoundingRun(sounding, B, dev, mask=want_mask, mask_base=mask_base, force=want_force,
                              force_base=keep.pitch if keep is not None else None)
        if want_mask:
            sampling = FF_.sounding_block(sampling, run.mask_eff)
        force = {'sounding': run}
        if want_force:
            force.update(pitch=run.force_eff,
                         dur=keep.dur if keep is not None else torch.full((5, 480 * B), -1, dtype=torch.int32, device=dev))
        return sampling, force, run

    def decode_logprob(self):
        """Log-probabilities of the LAST inference decode (ptv_decode_logprob + ptv_decode_logprob_fold; INTEGRATION.md "Decode
        log-probabilities") -> DecodeLogprob(logp [B,2], logq [B,2], counts int32 [B,4], err int32 [B], step_logp [B,32,4],
        step_counts int32 [B,32,4]): per sample the (pitch, duration) sums of log p -- the model's own softmax at the decided classes
        -- and of log q -- the distribution the decode drew from (temperature, pitch_mask / ascending, top_k / min_p / top_p; 0 where
        the decision was the argmax or forced by keep) --, counts = (pitch_n, dur_n, forced_pitch_n, forced_dur_n), err bit 0 = a free
        decision outside the recomputed kept set (never on a decode's own outputs); step_logp = (logp pitch, logp dur, logq pitch,
        logq dur) per time step.  A post-pass over the logits, grid, block and keep the decode left on the device: launched eagerly on
        the current stream, never captured (graph keys and capture counts stay what they were); everything stays on the device.  The
        tensors of a graph-replayed decode are the graph's own: call this before the next decode."""
        last = self._last_decode
        if last is None:
            raise RuntimeError('decode_logprob() follows an inference decode: there is none yet')
        pitch, dur, xhat, sampling, force = last
        fp, fd = (None, None) if not force else (force.get('pitch'), force.get('dur'))
        B, dev = xhat.shape[0], xhat.device
        assert pitch.shape == (15, 32, B, 130) and pitch.stride(3) == 1 and pitch.stride(1) == B * pitch.stride(2) \
            and pitch.stride(0) == 32 * B * pitch.stride(2) and dur.is_contiguous() and xhat.is_contiguous()
        step_logp = torch.empty(B, 32, 4, device=dev, dtype=torch.float32)
        step_counts = torch.empty(B, 32, 4, device=dev, dtype=torch.int32)
        sums = torch.empty(B, 4, device=dev, dtype=torch.float32)
        counts = torch.empty(B, 4, device=dev, dtype=torch.int32)
        err = torch.empty(B, device=dev, dtype=torch.int32)
        F_.call('ptv_decode_logprob', F_.ptr(pitch), pitch.stride(2), F_.ptr(dur), F_.ptr(xhat), B, 1, F_.ptr(sampling),
                FF_.block_kind(sampling).nbytes, F_.ptr(fp), F_.ptr(fd), F_.ptr(step_logp), F_.ptr(step_counts),
                F_.ptr(err), F_.stream_ptr())
        F_.call('ptv_decode_logprob_fold', F_.ptr(step_logp), F_.ptr(step_counts), B, F_.ptr(sums), F_.ptr(counts), F_.stream_ptr())
        return DecodeLogprob(sums[:, 0:2], sums[:, 2:4], counts, err, step_logp, step_counts)

    def forward(self, z, inference, x, lengths, teacher_forcing_ratio1, teacher_forcing_ratio2, coins=None, *, live=None, sampling=None,
                keep=None, sounding=None):
        return self.decoder(z, inference, x, lengths, teacher_forcing_ratio1, teacher_forcing_ratio2, coins=coins, live=live, sampling=sampling,
                            keep=keep, sounding=sounding)

    # ---- the reference's helper METHODS (ptvae.py:292-428), callable by reference-side code.  Forward-only entry points onto the
    # kernels the fused path runs (`decoder()` never calls them: it runs DecoderTFFn / DecoderStepFn); results carry no autograd graph.
    def _P(self):
        return dict(zip(FF_.FREE_PARAM_NAMES, self._params_free()))

    def _geom(self):
        return (self.num_step, self.max_simu_note, self.pitch_range, self.dur_width, self.pitch_pad)

    def get_len_index_tensor(self, ind_x):
        """ptvae.py:292-297: lengths [B, num_step] (int64) = max_simu_note - number of <pad> pitches per step"""
        _require_cuda(ind_x, 'PtvaeDecoder.get_len_index_tensor')
        x = ind_x.long().contiguous()
        B = x.size(0)
        S, N, _P, D, pad = PtvaeDecoder._geom(self)
        lengths = torch.empty(S * B, device=x.device, dtype=torch.int32)
        F_.call('ptv_grid_lengths_geom', F_.ptr(x), F_.ptr(lengths), B, S, N, D, pad, F_.stream_ptr())
        return lengths.view(S, B).t().long()

    def index_tensor_to_multihot_tensor(self, ind_x):
        """ptvae.py:299-313: piano grid [B,32,16,6] -> multi-hot [B,32,16,135] (one-hot pitch of 130 | 5 duration bits); a permuted
        view of the step-major matrix the note_embedding weight gradient multiplies.  (Any grid geometry; the reference's own
        `view(-1, 32, ...)` fixes num_step = 32.)"""
        _require_cuda(ind_x, 'PtvaeDecoder.index_tensor_to_multihot_tensor')
        x = ind_x.long().contiguous()
        B = x.size(0)
        S, N, P, D, _pad = PtvaeDecoder._geom(self)
        out = torch.empty(N, S, B, self.note_size, device=x.device, dtype=torch.float32)
        F_.call('ptv_multihot_geom', F_.ptr(x), F_.ptr(out), self.note_size, B, S, N, P, D, 0, F_.stream_ptr())
        return out.permute(2, 1, 0, 3)

    def get_sos_token(self):
        """ptvae.py:315-320: the <sos> note token [135] = onehot(128) | 2 2 2 2 2"""
        dev = self.note_embedding.weight.device
        return self.index_tensor_to_multihot_tensor(FF_._sos_grid(dev))[0, 0, 0].clone()

    def dur_ind_to_dur_token(self, inds, batch_size):
        """ptvae.py:322-326: [B] indices -> one-hot rows [B, dur_width]"""
        dev = self.note_embedding.weight.device
        inds = torch.as_tensor(inds, device=dev).long().view(batch_size, 1)
        return torch.zeros(batch_size, self.dur_width, device=dev).scatter_(1, inds, 1.0)

    def pitch_dur_ind_to_note_token(self, pitch_inds, dur_inds, batch_size):
        """ptvae.py:328-334: note_embedding(onehot(pitch) | duration bits) -> [B, note_emb_size] (ptv_note_token)"""
        dev = self.note_embedding.weight.device
        with torch.no_grad():
            return FF_.note_token_rows(self._P(), torch.as_tensor(pitch_inds, device=dev).view(batch_size),
                                       torch.as_tensor(dur_inds, device=dev).view(batch_size, self.dur_width))

    def decode_note(self, note_summary, batch_size):
        """ptvae.py:336-368: note_summary [B,1,Hn] -> est_pitch [B,130], est_durs [B,5,2] (pitch head + the 5-step duration GRU
        with argmax feedback)"""
        _require_cuda(note_summary, 'PtvaeDecoder.decode_note')
        with torch.no_grad():
            p, d, _ = FF_.decode_note_rows(self._P(), note_summary.detach().reshape(batch_size, -1).float().contiguous(), self._prec)
        return p, d

    def decode_notes(self, notes_summary, batch_size, notes, inference, teacher_forcing_ratio=0.5):
        """ptvae.py:370-428: one time step's 15 note steps.  notes_summary [B,1,Ht], notes [B,16,E] or None ->
        pitch_outs [B,15,130], dur_outs [B,15,5,2], predicted_notes [B,16,E], lengths [B].  Coins in the reference's order
        (one random.random() after each of the first 14 note steps)."""
        _require_cuda(notes_summary, 'PtvaeDecoder.decode_notes')
        if inference:
            assert teacher_forcing_ratio == 0
            assert notes is None
        coins = [random.random() < teacher_forcing_ratio for _ in range(self.max_simu_note - 2)]
        with torch.no_grad():
            return FF_.decode_notes_rows(self._P(), notes_summary.detach().reshape(batch_size, -1).float().contiguous(),
                                         None if notes is None else notes.detach(), coins, bool(inference), self._prec)

    # ---- ptvae.py:537-544
    def output_to_numpy(self, recon_pitch, recon_dur):
        est_pitch = recon_pitch.max(-1)[1].unsqueeze(-1)
        est_dur = recon_dur.max(-1)[1]
        est_x = torch.cat([est_pitch, est_dur], dim=-1).cpu().numpy()
        return est_x, recon_pitch.detach().cpu().numpy(), recon_dur.detach().cpu().numpy()

    # ---- ptvae.py:498-529
    def recon_loss(self, x, recon_pitch, recon_dur, weights=(1, 0.5), weighted_dur=False):
        out = F_.recon_loss(x.long(), recon_pitch, recon_dur, float(weights[0]), float(weights[1]), bool(weighted_dur))
        return out[0], out[1], out[2]

    # ---- per-sample scores of logits the caller already holds (INTEGRATION.md "Per-sample scores"; forward only)
    def score_outputs(self, x, pitch_outs, dur_outs):
        """x int [B,32,16,6], pitch_outs [B,32,15,130], dur_outs [B,32,15,5,2] (what decoder() returns, consumed in place) -> dict of
        detached device tensors: step_scores f32 [B,32,2] = (pitch NLL sum, duration NLL sum) per time step, step_counts int32 [B,32,6] =
        (pitch_n, pitch_hit, dur_n, dur_hit, note_n, note_hit), and their sums over the time steps scores [B,2] / counts [B,6].  Rows and
        bits whose target is <pad> are never read.  ValueError for CPU tensors or wrong shapes, before any launch."""
        step_scores, step_counts, scores, counts = F_.recon_scores(x, pitch_outs, dur_outs)
        return dict(step_scores=step_scores, step_counts=step_counts, scores=scores, counts=counts)

    # ---- ptvae.py:546-575, MIDI-free: notes come back as (pitch, start, end) tuples (velocity is the constant 100 of the
    # reference's pretty_midi.Note calls); pretty_midi is not needed
    def pr_to_notes(self, pr, bpm=80, start=0., one_hot=False):
        """pr: [32,128] duration matrix (pr_mat layout).  The reference routes through an undefined `pr_to_pr_matrix`
        (ptvae.py:547); a duration matrix is what its loop body consumes."""
        import numpy as np
        pr_matrix = np.asarray(pr)
        alpha = 0.25 * 60 / bpm
        notes = []
        for t in range(32):
            for p in range(128):
                if pr_matrix[t, p] >= 1:
                    notes.append((int(p), alpha * t + start, alpha * (t + pr_matrix[t, p]) + start))
        return notes

    def grid_to_pr_and_notes(self, grid, bpm=60., start=0.):
        import numpy as np
        grid = np.asarray(grid)
        if grid.shape[1] == self.max_simu_note:
            grid = grid[:, 1:]
        pr = np.zeros((32, 128), dtype=int)
        alpha = 0.25 * 60 / bpm
        notes = []
        for t in range(32):
            for n in range(10):                          # the reference reads at most 10 notes per step (ptvae.py:563)
                note = grid[t, n]
                if note[0] == self.pitch_eos:
                    break
                pitch = int(note[0]) + self.min_pitch
                dur = int(''.join(str(int(v)) for v in note[1:]), 2) + 1
                pr[t, pitch] = min(dur, 32 - t)
                notes.append((pitch, start + t * alpha, start + (t + dur) * alpha))
        return pr, notes

    # ---- the same transform for a whole batch on the device (ptv_grid_to_pr): nothing comes back to the host
    def grid_to_pr_and_notes_batch(self, grid, max_notes=10, check=False):
        """grid int64 [B,32,R,6], R = 15 or 16 (a 16-row step starts with <sos>, which is skipped) -> (pr_mat f32 [B,32,128],
        notes int32 [B,32*max_notes,3] = (pitch, t, dur), count int32 [B], x_clean int64 [B,32,16,6], err int32 [B]), all on the
        device.  pr_mat is the duration-at-onset layout the texture encoder takes, x_clean the canonical input grid of what was read
        (emb_x / loss()); notes_to_tuples() turns notes / count into this class's (pitch, start, end) tuples.  A row the reference
        would raise on is skipped and flagged in err (bit 0 pitch outside 0..127, bit 1 a duration bit that is not 0 or 1).
        check=False neither synchronises nor reads back (graph-capturable); check=True synchronises and raises the reference's
        IndexError / ValueError for the first flagged sample."""
        _require_cuda(grid, 'PtvaeDecoder.grid_to_pr_and_notes_batch')
        if grid.dim() != 4 or grid.shape[1] != 32 or grid.shape[2] not in (15, 16) or grid.shape[3] != 6:
            raise ValueError('grid: [B,32,15|16,6] expected, got %s' % (tuple(grid.shape),))
        B, R = grid.shape[0], grid.shape[2]
        if not 1 <= int(max_notes) <= R:
            raise ValueError('max_notes must be in 1..%d' % R)
        g = grid.detach().long().contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        dev = g.device
        pr_mat = torch.empty(B, 32, 128, device=dev, dtype=torch.float32)
        notes = torch.empty(B, 32 * int(max_notes), 3, device=dev, dtype=torch.int32)
        count = torch.empty(B, device=dev, dtype=torch.int32)
        x_clean = torch.empty(B, 32, 16, 6, device=dev, dtype=torch.int64)
        err = torch.empty(B, device=dev, dtype=torch.int32)
        F_.call('ptv_grid_to_pr', F_.ptr(g), B, R, int(max_notes), int(self.min_pitch), int(self.pitch_eos), F_.ptr(pr_mat), F_.ptr(notes),
                F_.ptr(count), F_.ptr(x_clean), F_.ptr(err), F_.stream_ptr())
        if check:
            e = err.cpu().numpy()
            bad = (e & 3).nonzero()[0]                  # (bit 3 alone only says x_clean kept 14 of a step's 15 notes)
            if len(bad):
                b = int(bad[0])
                if e[b] & 4:
                    raise ValueError('sample %d: a duration bit before <eos> is not 0 or 1 (ptvae.py:570 raises here)' % b)
                raise IndexError('sample %d: a pitch before <eos> is outside 0..127 (ptvae.py:571 raises here)' % b)
        return pr_mat, notes, count, x_clean, err

    @staticmethod
    def notes_to_tuples(notes, count, bpm=60., start=0.):
        """notes [B,N,3] / count [B] of grid_to_pr_and_notes_batch -> per sample the list of (pitch, start + t * alpha,
        start + (t + dur) * alpha), alpha = 0.25 * 60 / bpm: the tuples grid_to_pr_and_notes returns.  Host helper (copies back)."""
        notes, count = notes.cpu().tolist(), count.cpu().tolist()
        alpha = 0.25 * 60 / bpm
        return [[(p, start + t * alpha, start + (t + d) * alpha) for p, t, d in rows[:n]] for rows, n in zip(notes, count)]


class PtvaeEncoder(nn.Module, _PrecMixin):
    """PianoTree note -> time hierarchical encoder (ptvae.py:125-215): note embedding, bi-GRU over the <= 16 notes of each
    step (packed by length), bi-GRU over the 32 step summaries, Normal(linear_mu, exp(linear_std)).  The reference's train.py:32
    constructs it (unusable in that wiring); it is the encoder of the original PianoTree-VAE pairing.
    Runs on the same kernels as the hot path: `EmbedFn` (gather embedding + lengths), `BiGruFinalFn` with per-row lengths,
    `BiGruFinalFn` over time, `EncoderHeadsFn`.  No transposes: the step-major embedding [16][32*B] feeds the note GRU, whose
    [32*B, 2H] summaries ARE the step-major [32][B] input of the time GRU."""

    def __init__(self, device, max_simu_note=16, max_pitch=127, min_pitch=0, pitch_sos=128, pitch_eos=129,
                 pitch_pad=130, dur_pad=2, dur_width=5, num_step=32, note_emb_size=128, enc_notes_hid_size=256,
                 enc_time_hid_size=512, z_size=512):
        super().__init__()
        self.max_pitch, self.min_pitch = max_pitch, min_pitch
        self.pitch_sos, self.pitch_eos, self.pitch_pad = pitch_sos, pitch_eos, pitch_pad
        self.pitch_range = max_pitch - min_pitch + 3
        self.dur_pad, self.dur_width = dur_pad, dur_width
        self.note_size = self.pitch_range + dur_width
        self.max_simu_note, self.num_step = max_simu_note, num_step
        self.device = device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu')
        self.note_emb_size, self.z_size = note_emb_size, z_size
        self.enc_notes_hid_size, self.enc_time_hid_size = enc_notes_hid_size, enc_time_hid_size
        self.note_embedding = Linear(self.note_size, note_emb_size)
        self.enc_notes_gru = GRU(note_emb_size, enc_notes_hid_size, bidirectional=True)
        self.enc_time_gru = GRU(2 * enc_notes_hid_size, enc_time_hid_size, bidirectional=True)
        self.linear_mu = Linear(2 * enc_time_hid_size, z_size)
        self.linear_std = Linear(2 * enc_time_hid_size, z_size)

    def _check_grid(self):
        """Every geometry the reference's constructor accepts runs (train.py:32 builds max_pitch = 31: pitch_range 34); the bounds are
        those of the kernels' fixed-size staging (dur_width <= 8 index columns per note, the [P+D][E] weight in 150 KB of LDS)"""
        if self.dur_width > 8 or (self.note_size * self.note_emb_size * 4) > 150 * 1024 or self.note_emb_size > 256:
            raise NotImplementedError('PtvaeEncoder on HIP: dur_width <= 8, note_emb_size <= 256, note_size * note_emb_size <= 38400')

    # ---- ptvae.py:160-206: the reference's method surface
    def get_len_index_tensor(self, ind_x):
        return PtvaeDecoder.get_len_index_tensor(self, ind_x)

    def index_tensor_to_multihot_tensor(self, ind_x):
        return PtvaeDecoder.index_tensor_to_multihot_tensor(self, ind_x)

    def encoder(self, x, lengths):
        """ptvae.py:190-206: MULTI-HOT x [B,32,16,135] + lengths [B,32] -> (Normal, embedded [B,32,16,E]); differentiable.  forward()
        embeds the index grid by a gather instead of multiplying the multi-hot matrix; this entry point takes what the reference's
        takes (the embedding is then a [B*512,135] product)"""
        _require_cuda(x, 'PtvaeEncoder.encoder')
        self._check_grid()
        B = x.size(0)
        E = self.note_emb_size
        S, N = self.num_step, self.max_simu_note
        emb_b = F_.LinearFn.apply(x.reshape(B * S * N, self.note_size).float(), self.note_embedding.weight, self.note_embedding.bias,
                                  self._prec).view(B, S, N, E)
        emb = F_.Transpose01Fn.apply(emb_b.transpose(1, 2).reshape(B, N * S, E)).view(N, S, B, E)
        len32 = lengths.t().contiguous().int().reshape(-1)
        notes = F_.BiGruFinalFn.apply(emb.view(N, S * B, E), len32, self._prec, *self.enc_notes_gru.weights())
        h = F_.BiGruFinalFn.apply(notes.view(S, B, -1), None, self._prec, *self.enc_time_gru.weights())
        mu, sd = F_.EncoderHeadsFn.apply(h, self.linear_mu.weight, self.linear_mu.bias, self.linear_std.weight, self.linear_std.bias,
                                         self._prec)
        return HipNormal(mu, sd), emb_b

    def encode_multihot(self, mh, lengths=None, pad_col=None):
        """encoder() for a BYTE multi-hot grid: mh uint8 [B,S,N,note_size] on the device (the detrended grid dt_x of
        dataset.detrend_pianotree is one: train.py:32 builds this class for it) -> (Normal, embedded [B,S,N,E] as the permuted view of
        the step-major buffer); differentiable in the parameters.  lengths: the reference's [B,S] (get_len_index_tensor of the grid the
        multi-hot came from), or derived from pad_col: the rows whose byte in that column is 0 (dt_x: pad_col = 3, the is_note class of
        the <pad> pitch).  One embedding launch (EmbedMultihotFn): no float copy of mh, no [B*S*N, note_size] product, no transpose."""
        _require_cuda(mh, 'PtvaeEncoder.encode_multihot')
        self._check_grid()
        S, N, K = self.num_step, self.max_simu_note, self.note_size
        if mh.dtype != torch.uint8 or mh.dim() != 4 or tuple(mh.shape[1:]) != (S, N, K):
            raise ValueError('encode_multihot: uint8 [B,%d,%d,%d] expected, got %s %s' % (S, N, K, mh.dtype, tuple(mh.shape)))
        if K > 64 or self.note_emb_size % 4:
            raise NotImplementedError('encode_multihot on HIP: note_size <= 64, note_emb_size a multiple of 4')
        if lengths is None and pad_col is None:
            raise ValueError('encode_multihot: give lengths [B,%d] or pad_col (the column whose zero marks a live note row)' % S)
        if lengths is None and not 0 <= int(pad_col) < K:
            raise ValueError('encode_multihot: pad_col must be in 0..%d' % (K - 1))
        B = mh.size(0)
        emb, len32 = F_.EmbedMultihotFn.apply(mh, self.note_embedding.weight, self.note_embedding.bias, self._prec,
                                              -1 if lengths is not None else int(pad_col))
        if lengths is not None:
            if tuple(lengths.shape) != (B, S):
                raise ValueError('encode_multihot: lengths [%d,%d] expected, got %s' % (B, S, tuple(lengths.shape)))
            len32 = lengths.t().contiguous().int().reshape(-1)
        notes = F_.BiGruFinalFn.apply(emb.view(N, S * B, -1), len32, self._prec, *self.enc_notes_gru.weights())       # [S*B, 2Hn]
        h = F_.BiGruFinalFn.apply(notes.view(S, B, -1), None, self._prec, *self.enc_time_gru.weights())              # [B, 2Ht]
        mu, sd = F_.EncoderHeadsFn.apply(h, self.linear_mu.weight, self.linear_mu.bias, self.linear_std.weight, self.linear_std.bias,
                                         self._prec)
        return HipNormal(mu, sd), emb.permute(2, 1, 0, 3)

    def forward(self, x, return_iterators=False):
        _require_cuda(x, 'PtvaeEncoder')
        self._check_grid()
        B = x.size(0)
        emb, lengths = F_.EmbedFn.apply(x.long(), self.note_embedding.weight, self.note_embedding.bias, self._prec,
                                        PtvaeDecoder._geom(self))                                                      # [N,S,B,E]
        n, t, b, e = emb.shape
        notes = F_.BiGruFinalFn.apply(emb.view(n, t * b, e), lengths, self._prec, *self.enc_notes_gru.weights())      # [S*B, 2Hn]
        h = F_.BiGruFinalFn.apply(notes.view(t, b, -1), None, self._prec, *self.enc_time_gru.weights())               # [B, 2Ht]
        mu, sd = F_.EncoderHeadsFn.apply(h, self.linear_mu.weight, self.linear_mu.bias, self.linear_std.weight,
                                         self.linear_std.bias, self._prec)
        embedded_x = emb.permute(2, 1, 0, 3)                                # reference shape [B,S,N,E], step-major memory
        if return_iterators:
            return mu, sd, embedded_x
        return HipNormal(mu, sd), embedded_x, lengths.view(t, b).t()
