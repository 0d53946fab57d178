"""DisentangleVAE (alias PolyphonicVAE): chord/texture disentanglement VAE, MI355X train-step path.

Host-side mirror of the reference `model.py` (DisentangleVAE :11-96, inference family :117-184,
init_model :244-265): same constructor, `forward(mode, ...)` dispatch, `run` / `loss` /
`loss_function` / `kl_loss` / `chord_loss` signatures and return tuples, same `state_dict` keys.
All arithmetic runs in libptvae_hip.so kernels.
"""
import collections
import os

import torch

from . import functional as F_
from ._lib import call, ptr, stream_ptr
from .amc_dl.torch_plus import PytorchModel
from .functional_free import (CHORD_SCALES, CHORD_STEPS, RowSampling, build_chord_grammar, build_chord_keep, build_count_limits, build_dur_limits,
                              build_sounding, check_sounding, build_keep, build_keep_rhythm, build_keep_top, build_keep_voice, check_chord_grammar, check_chord_keep,
                              check_chord_sampling, check_constraints, check_keep, check_rows, check_sampling, chord_keep_steps_row,
                              chord_vocabulary, make_block, pitch_class_set, row_sampling_words, sampling_words, split_top, split_voice)
from .optim import refresh_weight_shadows
from .ptvae import HipNormal, PtvaeDecoder, PtvaeEncoder, RnnDecoder, RnnEncoder, TextureEncoder, _require_cuda

LOSS_NAMES = ['loss', 'recon_loss', 'pl', 'dl', 'kl_loss', 'kl_chd', 'kl_rhy', 'chord_loss', 'root_loss',
              'chroma_loss', 'bass_loss']                       # train.py:54-55


# Stream slots of the two encoders (pool stream = slot mod 4; autograd replays a branch's backward on the stream of its forward).  Round 5,
# after loss() stopped computing the dead note steps and the backward passes moved behind the C ABI, the schedule was measured again
# (scripts/ab_combo.py, 5-6 interleaved rounds per setting, profiles/r05_ab_runs.txt): the chord encoder on pool stream 3 -- the stream of
# the decoder's deferred weight-gradient products, so its BPTT runs AFTER them in the tail instead of beside them -- with the bi-GRUs'
# reversed-direction products on pool stream 0 (functional.BIGRU_SLOT_BWD = 4): 6.97-7.15 ms per step against 7.49-7.68 (slots 1 / 7);
# both encoders on stream 3: 7.47-7.56 (their forwards serialise); the texture encoder on 1 instead of 2: the same.
CHD_ENC_SLOT = 3
RHY_ENC_SLOT = 2
CHD_DEC_SLOT = 4        # the chord decoder beside the PianoTree decoder
# The two encoders ARE the latency chain of the head of the step (the decoder waits for z; the embedding / note summaries beside them are
# needed later): their products keep the raised wave priority although they run inside sibling-stream calls, the note-summary GRUs drop it
ENC_CHAIN = True
DT_PAD_COL = 3          # column of dt_x that is set for a <pad> row (is_note class 3, dataset.py:194-195): its zeros count the live rows
DT_SHAPE = (32, 16, 39)
# the keywords of a free-running decode (inference_decode); rows (a functional_free.RowSampling), sounding (a functional_free.Sounding)
# and the last two are device objects, the rest host values
DECODE_KEYS = ('temperature', 'dur_temperature', 'seed', 'draw', 'sample_offset', 'top_k', 'min_p', 'top_p', 'rows', 'sounding', 'ascending',
               'pitch_mask', 'keep')


class DecodeRequest(collections.namedtuple('DecodeRequest', 'sampled kw mask keep batch')):
    """the validated keywords of one decode (DisentangleVAE._request): sampled (a temperature was given), kw (the host keywords), mask
    (pitch_mask made contiguous -- the block holds its address -- or None), keep (functional_free.Keep or None), batch (the decoded rows)"""

    def tiled(self, n):
        """the request of the batch repeated n times (decode_best_of): a mask or keep with one row per sample is tiled alike, and so is
        the table of rows= -- candidate k of row b draws as sample sample_id[b] + k * B -- and so are the tables of sounding="""
        mask, keep, B = self.mask, self.keep, self.batch
        if self.kw.get('rows') is not None:
            self = self._replace(kw=dict(self.kw, rows=self.kw['rows'].tiled(n)))
        if self.kw.get('sounding') is not None:
            self = self._replace(kw=dict(self.kw, sounding=self.kw['sounding'].tiled(n)))
        if mask is not None and mask.shape[0] == B and B > 1:
            mask = mask.repeat(n, 1, 1)
        if keep is not None:
            keep = type(keep)(keep.pitch.view(15, 32, 1, B).expand(15, 32, n, B).reshape(15, 32 * n * B),
                              keep.dur.view(5, 15, 32, 1, B).expand(5, 15, 32, n, B).reshape(5, 480 * n * B), keep.err.repeat(n), n * B)
        return self._replace(mask=mask, keep=keep, batch=n * B)


class ChordRequest(collections.namedtuple('ChordRequest', 'sampled temperature chroma_temperature seed draw sample_offset keep grammar',
                                          defaults=(None,))):
    """the validated keywords of one row-independent chord decode (DisentangleVAE._chord_request); seed / draw / sample_offset None = the
    model's (use_philox, the draw counter)"""


class DisentangleVAE(PytorchModel):

    def __init__(self, name, device, chd_encoder, rhy_encoder, decoder, chd_decoder):
        super().__init__(name, device)
        self.chd_encoder = chd_encoder
        self.rhy_encoder = rhy_encoder
        self.decoder = decoder
        self.num_step = self.decoder.num_step
        self.chd_decoder = chd_decoder
        self.eps_source = None      # optional callable (name, shape, device) -> eps tensor (tests)
        self._philox = None         # (seed, global index of this process's first sample): see use_philox()
        self._draws = 0
        self._sample_draws = 0      # draw number of the next sampled decode that names none (advances once per sampled decode)
        self._mean_only = False     # set by score(sample=False) around its run()

    # ---- the texture encoder decides what the texture input is.  A TextureEncoder (init_model) reads the piano-roll pr_mat; a PtvaeEncoder
    # (init_model_detrended: the wiring of the reference's train.py:31-39) reads the detrended PianoTree grid dt_x, uint8 [B,32,16,39]
    @property
    def detrended(self):
        return isinstance(self.rhy_encoder, PtvaeEncoder)

    @staticmethod
    def _check_dt_x(dt_x, batch=None):
        if not torch.is_tensor(dt_x) or dt_x.dtype != torch.uint8 or dt_x.dim() != 4 or tuple(dt_x.shape[1:]) != DT_SHAPE \
                or (batch is not None and dt_x.shape[0] != batch):
            got = '%s %s' % (dt_x.dtype, tuple(dt_x.shape)) if torch.is_tensor(dt_x) else type(dt_x).__name__
            raise ValueError('this model\'s texture encoder is a PtvaeEncoder: its input is the detrended grid dt_x, uint8 [%s,32,16,39] '
                             '(dataset.detrend_pianotree(x, c)), not the piano-roll; got %s' % ('B' if batch is None else batch, got))
        return dt_x

    def _encode_texture(self, t):
        """the texture encoder on what the reference's signatures call `pr_mat`: pr_mat itself, or dt_x for the detrended variant"""
        if not self.detrended:
            return self.rhy_encoder(t)
        return self.rhy_encoder.encode_multihot(self._check_dt_x(t), pad_col=DT_PAD_COL)[0]

    # ---- precision switch: 'fp32' (exact, parity) | 'bf16' (bf16 MFMA operands, fp32 accumulate)
    def set_precision(self, precision):
        assert precision in ('fp32', 'bf16')
        for m in (self.chd_encoder, self.rhy_encoder, self.decoder, self.chd_decoder):
            m.precision = precision
        return self

    # ---- reparameterisation noise.  Default = torch's device generator (the reference draws from torch's global generator,
    # train_utils.py:33-34).  use_philox(seed, sample_offset) makes eps a pure function of (seed, draw number, GLOBAL sample
    # index, column) -- the same batch sees the same noise whether it runs on one GPU or is sharded over N ranks
    # (sample_offset = rank * per-rank batch; SURVEY.md section 8 d/e).  Every rank must make the same sequence of draws.
    def use_philox(self, seed=7, sample_offset=0):
        self._philox = (int(seed), int(sample_offset))
        self._draws = 0
        return self

    def _rsample(self, name, dist):
        if self._mean_only:                              # score(sample=False): z is the posterior mean, no draw is consumed
            return dist.mean
        eps = None
        if self.eps_source is not None:
            eps = self.eps_source(name, dist.mean.shape, dist.mean.device)
        elif self._philox is not None:
            B, Z = dist.mean.shape
            eps = torch.empty(B, Z, device=dist.mean.device, dtype=torch.float32)
            F_.call('ptv_philox_normal', F_.ptr(eps), B, Z, self._philox[0], self._draws, self._philox[1], F_.stream_ptr())
            self._draws += 1
        return dist.rsample(eps=eps)

    # ---- model.py:22-40: two helpers the reference defines and never calls (both call sites are commented out, model.py:44-46,102).
    # Plain tensor glue, kept for the method surface; not part of the hot path
    def confuse_prmat(self, pr_mat):
        """model.py:22-29: every non-zero entry of the piano-roll is also written one semitone up or down (coin per entry, clamped to
        0..127), in place.  Draw order = the reference's: one torch.randint(0, 2, (nnz,)) from the default CPU generator."""
        nz = torch.nonzero(pr_mat.long())
        eps = ((2 * torch.randint(0, 2, (nz.size(0),))) - 1).long().to(pr_mat.device)
        tgt = torch.clamp(nz[:, 2] + eps, min=0, max=127)
        pr_mat[nz[:, 0], nz[:, 1], tgt] = pr_mat[nz[:, 0], nz[:, 1], nz[:, 2]]
        return pr_mat

    def get_chroma(self, pr_mat):
        """model.py:31-40: log(1 + per-beat, per-pitch-class sum of the [B,32,128] piano-roll) -> [B,8,12]"""
        bs = pr_mat.size(0)
        pr = torch.cat([pr_mat, torch.zeros(bs, 32, 4, device=pr_mat.device, dtype=pr_mat.dtype)], dim=-1)
        c = pr.view(bs, 32, -1, 12).sum(dim=-2).view(bs, 8, 4, 12).sum(dim=-2).float()
        return torch.log(c + 1)

    # ---- model.py:42-55
    def run(self, x, c, pr_mat, tfr1, tfr2, tfr3, confuse=True, *, live=None, dt_x=None):
        """dt_x: the detrended variant's texture input (uint8 [B,32,16,39]; None = computed here by dataset.detrend_pianotree(x, c));
        ignored when the texture encoder is a TextureEncoder"""
        F_.mark('run:start')
        refresh_weight_shadows()                         # bf16 operand copies of the flat parameter buffer (if any)
        F_.mark('run:shadows')
        # the two encoders are independent of each other and of the embedding: sibling HIP streams
        # (autograd replays each branch's backward on the stream its forward ran on).  They fork FIRST: a sibling stream waits for
        # what its parent has queued so far, and the embedding (queued on the parent next) is not their input
        _require_cuda(x, 'DisentangleVAE.run')               # (fails loudly off-GPU before any stream is touched)
        if self.detrended:
            if dt_x is None:
                from .dataset import detrend_pianotree
                dt_x = detrend_pianotree(x.long(), c)        # (on the caller's stream: the sibling stream below waits for it)
            else:
                self._check_dt_x(dt_x, x.size(0))
        s_chd, s_rhy = F_.Side(CHD_ENC_SLOT, chain=ENC_CHAIN), F_.Side(RHY_ENC_SLOT, chain=ENC_CHAIN)
        self.decoder.summaries_needed = tfr1 > 0             # with tfr1 = 0 no time step is fed a ground-truth note summary
        # (creating the embedding / note-summary nodes FIRST, so that autograd runs the encoders' BPTTs before the note-summary BPTT, measured
        # inside box noise, 8.11-9.0 ms per step: the plain order stays)
        dist_chd = s_chd(lambda: self.chd_encoder(c), c)
        if self.detrended:
            dist_rhy = s_rhy(lambda: self._encode_texture(dt_x), dt_x)
        else:
            dist_rhy = s_rhy(lambda: self.rhy_encoder(pr_mat), pr_mat)
        try:
            embedded_x, lengths = self.decoder.emb_x(x)
        finally:
            self.decoder.summaries_needed = True
        F_.mark('run:emb_x')
        s_chd.join()
        s_rhy.join()
        F_.mark('run:encoders')
        z_chd = self._rsample('chd', dist_chd)           # chd first, then rhy (train_utils.py:33-34)
        z_rhy = self._rsample('rhy', dist_rhy)
        dec_z = torch.cat([z_chd, z_rhy], dim=-1)
        # chord decoder (8 small steps) rides a sibling stream next to the PianoTree decoder.  Its coin
        # flips come AFTER the decoder's in the reference's draw order: draw them first
        # on the host in that order, then enqueue.
        dec_coins = self.decoder.draw_coins(tfr1, tfr2)
        chd_coins = self.chd_decoder.draw_coins(tfr3)
        s_cd = F_.Side(CHD_DEC_SLOT)
        recon_root, recon_chroma, recon_bass = s_cd(
            lambda: self.chd_decoder(z_chd, False, tfr3, c, coins=chd_coins), z_chd, c)
        pitch_outs, dur_outs = self.decoder(dec_z, False, embedded_x, lengths, tfr1, tfr2, coins=dec_coins, live=live)
        s_cd.join()
        return pitch_outs, dur_outs, dist_chd, dist_rhy, recon_root, recon_chroma, recon_bass

    # ---- model.py:57-68: one fused loss node (CE with ignore_index x2, KL x2, chord CE x3)
    def loss_function(self, x, c, recon_pitch, recon_dur, dist_chd, dist_rhy, recon_root, recon_chroma,
                      recon_bass, beta, weights, weighted_dur=False, *, live=None):
        out = F_.VaeLossFn.apply(recon_pitch, recon_dur, dist_chd.mean, dist_chd.scale, dist_rhy.mean,
                                 dist_rhy.scale, recon_root, recon_chroma, recon_bass, x.long(), c.float(),
                                 float(beta), float(weights[0]), float(weights[1]), bool(weighted_dur), live)
        return F_.SplitScalarsFn.apply(out)

    # ---- model.py:70-90 (stand-alone forms; loss_function computes them fused)
    def chord_loss(self, c, recon_root, recon_chroma, recon_bass):
        out = F_.ChordLossFn.apply(recon_root, recon_chroma, recon_bass, c.float())
        return out[0], out[1], out[2], out[3]

    def kl_loss(self, *dists):
        kl_chd = F_.KlFn.apply(dists[0].mean, dists[0].scale)
        kl_rhy = F_.KlFn.apply(dists[1].mean, dists[1].scale)
        return kl_chd + kl_rhy, kl_chd, kl_rhy

    # ---- model.py:92-96.  Same positional/keyword signature (x, c, pr_mat, tfr1=0., tfr2=0., tfr3=0.,
    # beta=0.1, weights=(1, 0.5)); additionally a 4th positional TENSOR, the `dt_x` the reference's trainer passes (its own loss() has no
    # slot for it -- SURVEY.md §0.2), is accepted: the detrended variant's texture input; ignored with a TextureEncoder.
    def loss(self, x, c, pr_mat, *args, **kwargs):
        args = list(args)
        dt_x = None
        while args and torch.is_tensor(args[0]):
            t = args.pop(0)
            dt_x = t if dt_x is None else dt_x
        names = ('tfr1', 'tfr2', 'tfr3', 'beta', 'weights')
        if len(args) > len(names):
            raise TypeError('loss() takes at most %d scalar arguments after pr_mat' % len(names))
        p = dict(tfr1=0., tfr2=0., tfr3=0., beta=0.1, weights=(1, 0.5))
        for n, v in zip(names, args):
            if n in kwargs:
                raise TypeError("loss() got multiple values for argument '%s'" % n)
            p[n] = v
        for k, v in kwargs.items():
            if k not in p:
                raise TypeError("loss() got an unexpected keyword argument '%s'" % k)
            p[k] = v
        # run()'s outputs go nowhere but into the loss, which ignores the padded note slots: the teacher-forced decoder may leave the note
        # steps after the batch's last target uncomputed.  Both nodes get the plan (functional.live_rows): the decoder records the row order
        # of its logits, the loss takes the targets in that order (run() on its own gets no plan and always computes every step)
        live = F_.live_rows(x) if (torch.is_grad_enabled() and p['tfr1'] >= 1. and p['tfr2'] >= 1.) else None
        if self.detrended:
            outputs = self.run(x, c, pr_mat, p['tfr1'], p['tfr2'], p['tfr3'], live=live, dt_x=dt_x)
        else:
            outputs = self.run(x, c, pr_mat, p['tfr1'], p['tfr2'], p['tfr3'], live=live)
        return self.loss_function(x, c, *outputs, p['beta'], p['weights'], live=live)

    # ---- per-sample scores and reconstruction accuracy (INTEGRATION.md "Per-sample scores"; forward only, csrc/score.hip)
    def _score_inputs(self, x, c, pr_mat, dt_x, who):
        """ValueError for a CPU tensor, a wrong trailing shape or differing batch sizes, before anything is launched -> the texture
        encoder's input (pr_mat; for the detrended variant dt_x, or a dt_x grid in the pr_mat slot, or None = derived from x and c)"""
        B = F_._need(x, who + ' x', (32, 16, 6), F_._INT_GRID)
        sizes = dict(x=B, c=F_._need(c, who + ' c', (8, 36)))
        tex = pr_mat
        if self.detrended:
            tex = dt_x if dt_x is not None else (pr_mat if torch.is_tensor(pr_mat) and pr_mat.dtype == torch.uint8 else None)
            if tex is not None:
                if not torch.is_tensor(tex) or not tex.is_cuda:
                    raise ValueError(who + ' dt_x: a device tensor expected')
                sizes['dt_x'] = self._check_dt_x(tex).shape[0]
            elif pr_mat is not None:
                sizes['pr_mat'] = F_._need(pr_mat, who + ' pr_mat', (32, 128))
        else:
            sizes['pr_mat'] = F_._need(pr_mat, who + ' pr_mat', (32, 128))
        F_._same_batch(**sizes)
        return tex

    def score(self, x, c, pr_mat, dt_x=None, *, sample=False, beta=1.0):
        """One teacher-forced pass (all ratios 1) without gradients -> a dict of detached device tensors, one entry per sample; nothing
        synchronises.  pitch_nll, dur_nll, kl_chd, kl_rhy, root_nll, chroma_nll, bass_nll: f32 [B], SUMS over the sample's targets /
        latent (loss() reports their batch means); elbo = -(pitch_nll + dur_nll) - beta * (kl_chd + kl_rhy); counts int32 [B,6] =
        (pitch_n, pitch_hit, dur_n, dur_hit, note_n, note_hit); chord_counts int32 [B,3] = root hits of 8, chroma-bit hits of 96, bass
        hits of 8; step_scores f32 [B,32,2] / step_counts int32 [B,32,6]: the reconstruction terms per time step.
        sample=False: z is the posterior mean (deterministic); True: the model's usual noise (eps_source / use_philox / torch).
        pr_mat: the texture encoder's input as in the inference family (for the detrended variant dt_x, here or as the 4th argument;
        neither: derived from x and c).  The teacher-forcing coins it draws are put back: the `random` stream is left as it was."""
        import random
        tex = self._score_inputs(x, c, pr_mat, dt_x, 'score()')
        coins = random.getstate()
        self._mean_only = not sample
        try:
            with torch.no_grad():
                if self.detrended:
                    outs = self.run(x, c, pr_mat, 1., 1., 1., dt_x=tex)
                else:
                    outs = self.run(x, c, tex, 1., 1., 1.)
                pitch, dur, dist_chd, dist_rhy, root, chroma, bass = outs
                step_scores, step_counts, scores, counts = F_.recon_scores(x, pitch, dur)
                kl_chd, kl_rhy = F_.kl_rows(dist_chd.mean, dist_chd.scale), F_.kl_rows(dist_rhy.mean, dist_rhy.scale)
                chord, chord_counts = F_.chord_scores(c, root, chroma, bass)
                B = scores.shape[0]
                elbo = torch.empty(B, device=scores.device, dtype=torch.float32)
                col = lambda t, j: t[:, j:j + 1]
                F_.copy2d(elbo.view(B, 1), col(scores, 0), alpha=-1.0)
                F_.copy2d(elbo.view(B, 1), col(scores, 1), alpha=-1.0, acc=True)
                F_.copy2d(elbo.view(B, 1), kl_chd.view(B, 1), alpha=-float(beta), acc=True)
                F_.copy2d(elbo.view(B, 1), kl_rhy.view(B, 1), alpha=-float(beta), acc=True)
        finally:
            self._mean_only = False
            random.setstate(coins)
        return dict(pitch_nll=scores[:, 0], dur_nll=scores[:, 1], kl_chd=kl_chd, kl_rhy=kl_rhy, root_nll=chord[:, 0],
                    chroma_nll=chord[:, 1], bass_nll=chord[:, 2], elbo=elbo, counts=counts, chord_counts=chord_counts,
                    step_scores=step_scores, step_counts=step_counts)

    TALLY_NAMES = ('pitch_n', 'pitch_hit', 'dur_n', 'dur_hit', 'note_n', 'note_hit', 'root_hit', 'chroma_hit', 'bass_hit', 'chord_steps',
                   'est_n', 'ref_n', 'onset_tp', 'exact_tp', 'nll')

    REPORT_NAMES = ('pitch_acc', 'dur_acc', 'note_acc', 'root_acc', 'chroma_acc', 'bass_acc', 'onset_precision', 'onset_recall', 'onset_f1',
                    'exact_f1', 'nll_per_note')

    def reconstruction_counts(self, x, c, pr_mat, dt_x=None):
        """The pooled counts behind reconstruction_report, as Python numbers from ONE host read (a trainer adds them over batches:
        pool the counts, not the ratios).  Keys TALLY_NAMES: score(sample=False)'s six counts and three chord hit counts summed over the
        batch, chord_steps = 8 B, the four roll-match counts of the free-running reconstruction inference(pr_mat, c, sample=False)
        against the roll the same output path makes of x itself (so both sides carry the same 14-note and duration clipping), and
        nll = sum(pitch_nll + dur_nll)."""
        tex = self._score_inputs(x, c, pr_mat, dt_x, 'reconstruction_counts()')
        s = self.score(x, c, pr_mat, dt_x, sample=False)
        mode = self.training
        with torch.no_grad():
            if self.detrended and tex is None:
                from .dataset import detrend_pianotree
                tex = detrend_pianotree(x.long(), c)
            dist_chd, dist_rhy = self.inference_encode(tex, c)
            self._decode(dist_chd.mean, dist_rhy.mean, self._request(x.shape[0]))
            # the decoded grid goes through the output path's canonical form first (x_clean: a step's first 14 readable notes, <eos>,
            # <pad>), the layout x itself has: both rolls are then made from grids with the same clipping
            to_pr = lambda grid: self.decoder.grid_to_pr_and_notes_batch(grid, 15, check=False)
            est_pr = to_pr(to_pr(self.decoder.last_xhat)[3])[0]
            ref_pr = to_pr(x)[0]
            roll = F_.roll_match(est_pr, ref_pr)
            flat = torch.cat([s['counts'].reshape(-1), s['chord_counts'].reshape(-1), roll.reshape(-1),
                              s['pitch_nll'].contiguous().view(torch.int32), s['dur_nll'].contiguous().view(torch.int32)])
        self.train(mode)
        import numpy as np
        B = x.shape[0]
        h = flat.cpu().numpy()
        cnt = h[:6 * B].reshape(B, 6).astype(np.int64).sum(0)
        chd = h[6 * B:9 * B].reshape(B, 3).astype(np.int64).sum(0)
        rm = h[9 * B:13 * B].reshape(B, 4).astype(np.int64).sum(0)
        nll = float(h[13 * B:].view(np.float32).astype(np.float64).sum())
        vals = [int(v) for v in cnt] + [int(v) for v in chd] + [8 * B] + [int(v) for v in rm] + [nll]
        return dict(zip(self.TALLY_NAMES, vals))

    @staticmethod
    def report_from_counts(t):
        """reconstruction_counts' tally (or the sum of several) -> the report: pooled ratios, total hits over total targets; a zero
        denominator gives 0.0"""
        div = lambda a, b: float(a) / float(b) if b else 0.0
        f1 = lambda tp: div(2 * tp, t['est_n'] + t['ref_n'])
        return dict(pitch_acc=div(t['pitch_hit'], t['pitch_n']), dur_acc=div(t['dur_hit'], t['dur_n']),
                    note_acc=div(t['note_hit'], t['note_n']), root_acc=div(t['root_hit'], t['chord_steps']),
                    chroma_acc=div(t['chroma_hit'], 12 * t['chord_steps']), bass_acc=div(t['bass_hit'], t['chord_steps']),
                    onset_precision=div(t['onset_tp'], t['est_n']), onset_recall=div(t['onset_tp'], t['ref_n']),
                    onset_f1=f1(t['onset_tp']), exact_f1=f1(t['exact_tp']), nll_per_note=div(t['nll'], t['note_n']))

    def reconstruction_report(self, x, c, pr_mat, dt_x=None):
        """Pitch / duration / note / chord accuracies of the teacher-forced pass, onset and exact (onset + duration) precision / recall / F1
        of the free-running reconstruction, and the NLL per note, as Python floats from one host read (report_from_counts of
        reconstruction_counts)."""
        return self.report_from_counts(self.reconstruction_counts(x, c, pr_mat, dt_x))

    # ---- model.py:117-122.  In the whole inference family (inference_encode, inference, swap, posterior_sample, prior_sample, interp) the
    # argument the reference names `pr_mat` (`x` in prior_sample) is the texture encoder's input: the piano-roll f32 [B,32,128] for a
    # TextureEncoder, the detrended grid dt_x uint8 [B,32,16,39] for the detrended variant (anything else: ValueError)
    def inference_encode(self, pr_mat, c):
        """pr_mat: the texture encoder's input -- the piano-roll, or dt_x for the detrended variant"""
        if self.detrended:
            self._check_dt_x(pr_mat)                     # (a piano-roll here is a ValueError, not a shape crash inside a kernel)
        self.eval()
        refresh_weight_shadows()                         # no-op unless the parameters changed since the last cast
        with torch.no_grad():
            dist_chd = self.chd_encoder(c)
            dist_rhy = self._encode_texture(pr_mat)
        return dist_chd, dist_rhy

    # ---- model.py:124-131: free-running decode; est_x = the argmax grid the step loop produced on device
    # (identical to output_to_numpy's argmax of the returned logits, ptvae.py:537-544)
    #
    # Sampled decode (keyword-only; INTEGRATION.md "Sampled decode").  temperature (pitch) / dur_temperature (duration bits; default: the
    # pitch temperature), floats >= 0: every decision of the free-running decoder becomes a draw from softmax(logits / T) instead of the
    # argmax (T = 0 is the argmax).  The draw is Philox noise keyed by (seed, draw, sample_offset + row, time step, note step): reproducible,
    # independent of how a batch is cut.  seed / sample_offset default to use_philox()'s, else 7 / 0; draw defaults to a per-model counter
    # that advances once per sampled decode.  temperature=None (default): the argmax decode, unchanged.  The same keywords pass through
    # decode_to_inputs, reencode, inference, swap, posterior_sample, prior_sample and interp (sample index = row of the decoded batch).
    # Truncated sampling bounds the support of the PITCH draw (the duration bits keep dur_temperature, the chord decoder its argmax):
    # top_k (int >= 1) keeps the classes >= the k-th largest logit of the row, ties with it included; min_p (float in [0, 1], 0 / None =
    # off) keeps the classes with p >= min_p * p_max under softmax(logits / temperature); both: a class must pass both.  The draw is then
    # exact from the renormalised truncated softmax, with the same noise words.  top_p (float in (0, 1], 1.0 / None = off) is nucleus
    # truncation: the smallest set of best classes whose mass under softmax(logits / temperature) reaches top_p, ties with the last kept
    # value included.  Every rule is judged on the untruncated row and a class must pass all that are given -- not the sequential
    # renormalising chain of other libraries.
    # Constrained decode (INTEGRATION.md "Constrained decode") restricts the SUPPORT of the pitch decision, before any truncation:
    # pitch_mask (int32 device tensor [B, 32, 4] or [1, 32, 4]; pitch_mask() below builds one) says which grid pitches a time step may
    # use, ascending=True makes the notes of a time step strictly increasing and never <sos> -- the PianoTree grammar.  <eos> is always
    # allowed.  The mask's rows are the rows of the decoded batch (sample_offset moves only the noise).  With temperature=None the decode
    # is the constrained ARGMAX (the draw counter does not advance; seed / draw / sample_offset stay a ValueError).
    # Per-row sampling (INTEGRATION.md "Per-row sampling"): rows= (row_sampling() below builds one) gives every row of the batch its own
    # temperature, dur_temperature, top_k, min_p, top_p and sample id -- a batch of different requests, or a sweep of one z, as ONE decode.
    # It makes the decode a sampled one (the draw counter advances as with temperature=), excludes those five keywords and sample_offset,
    # and combines with seed, draw, pitch_mask, ascending and keep like a constrained decode.
    @staticmethod
    def _check_sampling(temperature=None, dur_temperature=None, seed=None, draw=None, sample_offset=None, top_k=None, min_p=None,
                        top_p=None, rows=None, sounding=None, pitch_mask=None, ascending=None, keep=None, batch=None):
        """ValueError for a bad sampling keyword; True for a sampled decode, False for the argmax decode (constrained or not).  No side
        effect, no launch.  batch: the rows of the decoded batch where the caller knows them (pitch_mask's row count and keep's batch are
        held to it)"""
        check_constraints(pitch_mask, ascending, batch)
        check_keep(keep, batch)
        check_sounding(sounding, batch)
        if rows is not None:                                   # per-row sampling: a sampled decode whose rule is the table's
            if any(v is not None for v in (temperature, dur_temperature, top_k, min_p, top_p, sample_offset)):
                raise ValueError('rows carries temperature, dur_temperature, top_k, min_p, top_p and the sample ids of every row: it cannot '
                                 'be combined with those keywords or with sample_offset')
            check_rows(rows, batch)
            check_sampling(0.0, None, 0, 0 if seed is None else seed, 0 if draw is None else draw)
            return True
        if temperature is None and dur_temperature is None:
            if seed is not None or draw is not None or sample_offset is not None:
                raise ValueError('seed / draw / sample_offset belong to a sampled decode: give a temperature')
            if top_k is not None or min_p is not None or top_p is not None:
                raise ValueError('top_k / min_p / top_p belong to a sampled decode: give a temperature')
            return False
        check_sampling(temperature, dur_temperature, 0 if sample_offset is None else sample_offset, 0 if seed is None else seed,
                       0 if draw is None else draw, top_k=top_k, min_p=min_p, top_p=top_p)
        return True

    def _request(self, batch, **sampling):
        """the keywords of a decode of `batch` rows, validated once -> DecodeRequest.  _check_sampling's ValueErrors, and what only this
        model knows: kept steps and the decoder's replay mode exclude each other, and a kept top voice needs ascending notes.  Before
        anything is encoded or launched, and before the draw counter moves."""
        if getattr(sampling.get('keep'), 'needs_ascending', False) and sampling.get('ascending') is False:
            raise ValueError('a %s needs ascending notes: its ceilings leave room only for notes that ascend -- leave ascending out '
                             '(it becomes True) or give ascending=True' % (type(sampling['keep']).__name__,))
        sampled = self._check_sampling(**sampling, batch=batch)
        keep, mask = sampling.get('keep'), sampling.get('pitch_mask')
        if keep is not None and self.decoder.force_trace is not None:
            raise ValueError('keep cannot be combined with decoder.force_trace: both fill the force arrays')
        if sampling.get('sounding') is not None and self.decoder.force_trace is not None:
            raise ValueError('sounding cannot be combined with decoder.force_trace: both fill the force arrays')
        return DecodeRequest(sampled, {k: sampling.get(k) for k in DECODE_KEYS[:-2]}, None if mask is None else mask.contiguous(), keep, batch)

    def _sampling_words(self, req):
        """None (argmax decode) or the request's sampling block as host words (keep puts nothing into the block: it travels beside it);
        a sampled decode that names no draw takes the model's counter and advances it.  A rhythm keep promotes the decode to the constrained
        kind, whose kernels alone honour its words: an `ascending` nobody gave becomes False, the vacuous constraint (flags 0, no mask).  A
        top keep does the same with True: its ceilings count on notes that ascend (_request has refused ascending=False).  A keep with
        duration limits (DurKeep) is promoted like a rhythm keep; built into a top keep it stays a top keep.  Note-count limits with a
        floor (CountKeep) are promoted like a rhythm keep, with room=True like a top keep; without a floor they promote nothing.
        Sounding rules follow the keep family: no_restrike or a floor (Sounding.needs_constrained) promotes like a rhythm keep, a ceiling
        alone promotes nothing and runs in every kind"""
        kw = req.kw
        ascending = kw['ascending']
        if ascending is None and req.keep is not None and req.keep.needs_constrained:
            ascending = req.keep.needs_ascending
        if ascending is None and kw['sounding'] is not None and kw['sounding'].needs_constrained:
            ascending = False
        if not req.sampled:
            if req.mask is None and ascending is None:
                return None
            return sampling_words(0.0, 0.0, 0, 0, 0, pitch_mask=req.mask, ascending=ascending)   # the constrained argmax: no noise, no draw used
        ph = self._philox or (7, 0)
        seed, draw, offset = kw['seed'], kw['draw'], kw['sample_offset']
        if kw['rows'] is not None:                             # (the table holds every row's rule and sample id; seed and draw stay shared)
            words = sampling_words(None, None, ph[0] if seed is None else seed, self._sample_draws if draw is None else draw, 0,
                                   pitch_mask=req.mask, ascending=ascending, rows=kw['rows'])
        else:
            words = sampling_words(kw['temperature'], kw['dur_temperature'], ph[0] if seed is None else seed,
                                   self._sample_draws if draw is None else draw, ph[1] if offset is None else offset, top_k=kw['top_k'],
                                   min_p=kw['min_p'], top_p=kw['top_p'], pitch_mask=req.mask, ascending=ascending)
        if draw is None:
            self._sample_draws += 1
        return words

    def _decode(self, z_chd, z_rhy, req):
        """the free-running decode of both inference forms; req: the DecodeRequest of its keywords"""
        words = self._sampling_words(req)
        if words is not None:
            _require_cuda(z_chd, 'DisentangleVAE sampled decode')
            _require_cuda(z_rhy, 'DisentangleVAE sampled decode')
        dec_z = torch.cat([z_chd, z_rhy], dim=-1)
        block = None if words is None else make_block(words, req.mask, dec_z.device, req.kw['rows'])
        if req.keep is not None:
            _require_cuda(dec_z, 'DisentangleVAE decode with kept steps')
        if req.kw['sounding'] is not None:
            _require_cuda(dec_z, 'DisentangleVAE decode with sounding rules')
            return self.decoder(dec_z, True, None, None, 0., 0., sampling=block, keep=req.keep, sounding=req.kw['sounding'])
        return self.decoder(dec_z, True, None, None, 0., 0., sampling=block, keep=req.keep)

    def row_sampling(self, batch, temperature, dur_temperature=None, top_k=None, min_p=None, top_p=None, sample_id=None, sample_offset=None):
        """The sampling rule of every row of a decode -> functional_free.RowSampling(table, batch) for rows= (INTEGRATION.md "Per-row
        sampling").  Each of temperature, dur_temperature, top_k, min_p, top_p is a scalar (every row alike) or a host sequence / numpy
        array of `batch` values with the meaning of the scalar keyword; sample_id: None (sample_offset + row; sample_offset defaults to
        use_philox()'s, else 0) or `batch` integers in [0, 2^47), the row's own index in the noise stream.  table is an int32 device
        tensor [batch, 8] on the decoder's device; RowSampling.update(...) rewrites it in place.  A bad value is a ValueError naming its
        row, before anything touches the GPU."""
        offset = (self._philox or (7, 0))[1] if sample_offset is None else sample_offset
        words = row_sampling_words(batch, temperature, dur_temperature, top_k, min_p, top_p, sample_id, offset)
        dev = next(self.decoder.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('a sampled decode runs on the GPU: the row table lives in device memory (the model is on %s)' % (dev,))
        return RowSampling(torch.from_numpy(words).to(dev), batch, offset)

    def keep(self, x, steps):
        """The kept time steps of a decode -> functional_free.Keep(pitch, dur, err, batch) for keep= (ptv_keep_force_build; INTEGRATION.md
        "Kept steps").  x: int64 device tensor [B, 32, 16, 6], the model's grid (what decode_to_inputs, the dataset path and synth_batch
        give); steps: a device bool / uint8 tensor [B, 32] or [1, 32], or a host iterable of step indices / a slice (one row for every
        sample: range(16) = the first bar).  The notes of a kept step up to its <eos> are forced where the decoder takes its decisions
        and fed back like decisions; everything else is decided as without it.  err[b] bit 0: a kept step of sample b held a pitch outside
        0..129 before its <eos>; that decision stays free.  Nothing is copied to the host."""
        return build_keep(x, steps)

    def keep_voice(self, x, voice_steps, below=None, lowest=None, durations=True, whole_steps=None, return_counts=False):
        """The kept voice of a decode -> functional_free.Keep for keep=, as keep() gives it (ptv_keep_voice_force_build; INTEGRATION.md
        "Kept voices").  x: the grid as in keep(); voice_steps / whole_steps: selections as keep()'s steps.  At a voice step the LOWEST
        notes of x's step are forced -- the notes under pitch `below` (0..128), at most `lowest` of them (0..15): a prefix of the step,
        which the grammar orders by ascending pitch -- with their duration bits (durations=False: pitches only); the <eos> is not forced,
        so above the voice the decoder decides as without a keep: it may add notes or end the step.  A whole step is kept as by keep(); a
        step in both selections is a whole step.  below / lowest: a host int or an int32 device tensor [B, 32] / [1, 32]; at least one is
        given.  A pitch_mask or ascending never checks a forced decision, and ascending continues strictly above the kept voice.
        err[b] bit 0: a kept step of sample b held an unforcible pitch before its <eos> (the voice ends there); bit 1: a mode byte that
        is none of 0 / 1 / 2 (never from here).  return_counts=True: -> (Keep, kept_n int32 [B, 32], the forced pitch decisions per
        step).  Nothing is copied to the host."""
        return build_keep_voice(x, voice_steps, below, lowest, durations, whole_steps, return_counts)

    def keep_rhythm(self, x, steps, durations=True, whole_steps=None, return_counts=False):
        """The kept rhythm of a decode -> functional_free.RhythmKeep for keep= (ptv_keep_rhythm_force_build; INTEGRATION.md "Kept rhythm").
        x: the grid as in keep(); steps / whole_steps: selections as keep()'s steps.  At a rhythm step the decode gets exactly the notes of
        x's step: its K note decisions are free but cannot be <eos>, decision K is a forced <eos> (K = 0 keeps a rest, K = 15 forces no
        <eos>), and the duration bits are x's (durations=False: only the note count is kept).  The pitches are drawn again under whatever
        the decode is given -- temperature, top_k / min_p / top_p, pitch_mask, ascending.  Where a mask and ascending leave no pitch, <eos> is
        the fallback and the step ends short: compare the note counts to see it.  A whole step is kept as by keep(); a step in both
        selections is a whole step.  A decode with this keep always runs the constrained kernels (without a mask or ascending: with a
        constraint that excludes nothing).  err[b] bit 0: a kept step of sample b held a pitch that is no note before its <eos> (a
        rhythm step still counts the slot); bit 1: a mode byte that is none of 0 / 1 / 3 (never from here).  return_counts=True: ->
        (RhythmKeep, kept_n int32 [B, 32]).  Nothing is copied to the host."""
        return build_keep_rhythm(x, steps, durations, whole_steps, return_counts)

    def keep_top(self, x, top_steps, above=None, highest=None, durations=True, lanes=True, whole_steps=None, return_counts=False):
        """The kept top voice of a decode -> functional_free.TopKeep for keep= (ptv_keep_top_force_build; INTEGRATION.md "Kept top voice").
        x: the grid as in keep(); top_steps / whole_steps: selections as keep()'s steps.  At a top step the HIGHEST notes of x's step are
        forced in their slots -- the notes at or over pitch `above` (0..128), at most `highest` of them (0..15), a suffix of the step;
        neither given: the very top note -- the step keeps its note count K (decision K is a forced <eos>), and the notes under the kept
        ones are drawn again under whatever the decode is given.  Each of them is free, never <eos>, above the note before it and under a
        ceiling: x's next note (lanes=True: every voice stays between its old neighbours) or the lowest kept pitch less one semitone per
        decision still to come (lanes=False).  Where a pitch_mask leaves no note in that lane the mask yields for that decision; the count
        and the kept notes never do.  durations: True = x's bits for every note, 'kept' = for the kept notes only, False = all drawn.
        A whole step is kept as by keep(); a step in both selections is a whole step.  A decode with this keep always runs the
        constrained kernels with ascending=True (ascending=False is a ValueError).  above / highest: a host int or an int32 device tensor
        [B, 32] / [1, 32].  err[b] bit 0: a top step of sample b held a pitch that is no note before its <eos>, or notes that do not
        ascend strictly (a lane may then be empty and the step end short); bit 1: a mode byte that is none of 0 / 1 / 4 (never from
        here).  return_counts=True: -> (TopKeep, kept_n int32 [B, 32]).  Nothing is copied to the host."""
        return build_keep_top(x, top_steps, above, highest, durations, lanes, whole_steps, return_counts)

    def dur_limits(self, min_dur=None, max_dur=None, fit=None, steps=None, batch=None, keep=None, return_counts=False):
        """Duration limits of a decode -> functional_free.DurKeep for keep= (ptv_dur_range_force_build; INTEGRATION.md "Duration limits").
        At the selected steps every note whose duration bits are not forced gets a duration (1..32 sixteenths) in [floor, ceiling], and
        the decoder still chooses inside that range and feeds its choice back.  min_dur / max_dur: an int 1..32 or an integer device
        tensor [32] / [B, 32]; fit: 'segment' (ceiling 32 - t: nothing hangs over the end), 'bar' (16 - t % 16: nothing crosses the bar
        line) or 'beat' (4 - t % 4).  Whatever is given is combined: the ceiling is the smallest, then the floor, which yields where
        it lies above the ceiling.  steps: as keep()'s, default all 32.  batch: the number of samples, needed when neither `keep` nor a
        [B, 32] tensor tells it.  keep: an existing keep to build into; its forced words survive bit for bit and it stays what it is (a
        RhythmKeep / TopKeep keeps its promotion and its `ascending` rule).  The decision of each duration bit is the model's own,
        with the values that cannot end in the range removed: the bit-by-bit chain cut to the range, not the joint distribution over
        the 32 durations renormalised.  A decode with such a keep always runs the constrained kernels.  return_counts=True: -> (keep,
        yielded int32 [B, 32]: 1 where a selected step's floor yielded).  ValueError before any launch; nothing is copied to the host."""
        return build_dur_limits(self.device, min_dur, max_dur, fit, steps, batch, keep, return_counts)

    def count_limits(self, min_count=None, max_count=None, onsets=None, rests=None, steps=None, room=False, batch=None, keep=None,
                     return_counts=False):
        """Note-count limits of a decode -> a keep for keep= (ptv_note_count_force_build; INTEGRATION.md "Note-count limits"): how many
        notes sound at a time step, with no grid to copy the count from.  At the selected steps (steps: as keep()'s, default all 32) a
        step gets at least min_count and at most max_count notes; each an int 0..15 or an integer device tensor [32] / [B, 32].  The
        ceiling wins where the floor lies above it; max_count=0 is a rest, 15 no ceiling.  onsets / rests: selections that are selected
        whatever `steps` says -- a floor of at least 1 / the ceiling 0; a step in both is a rest, so count_limits(onsets=pattern,
        rests=~pattern) is "notes exactly on this pattern".  At least one of the four is needed.  A floor is "not <eos> while anything
        else is allowed": under a narrow pitch_mask or `ascending` the step can run out of pitches and fall short -- count the notes.
        room=True writes ceilings that leave a semitone for every note still owed instead: the decode then runs with ascending=True
        (ascending=False is a ValueError) and always reaches the floor; a mask yields before the count does.  keep: an existing keep to
        build into; its words survive bit for bit, a step whose count it fixes already (whole, rhythm, top steps) is left alone, and the
        result demands what both demand.  Without a floor the result is a plain Keep (or stays what `keep` is) and every decode kind
        takes it unchanged; with one it is a functional_free.CountKeep and the decode always runs the constrained kernels.  batch: the
        number of samples, needed when neither `keep` nor a [B, 32] tensor tells it.  return_counts=True: -> (keep, yielded int32
        [B, 32]: bit 0 the floor yielded to the ceiling, bit 1 the keep owns the step, bit 2 a kept voice is longer than the ceiling,
        bit 3 the room over a kept voice may not hold the floor).  decode_to_inputs(max_notes=) is the capacity of the note list the
        output path writes, not a limit on the decode: this is.  ValueError before any launch; nothing is copied to the host."""
        return build_count_limits(self.device, min_count, max_count, onsets, rests, steps, room, batch, keep, return_counts)

    def sounding(self, no_restrike=False, max_sounding=None, min_sounding=None, steps=None, batch=None):
        """The sounding rules of a decode -> functional_free.Sounding for sounding= (ptv_sounding_step; INTEGRATION.md "Sounding state"):
        restrictions that see what the decode itself decided at earlier time steps.  no_restrike=True: a pitch that still sounds is not
        struck again; max_sounding: at most that many pitches sound at a step (held ones included), a host int 1..127 or an integer
        device tensor [32] / [B, 32]; min_sounding: at least that many, a host int 0..15 or such a tensor -- "not <eos> while anything
        else is allowed", as a note-count floor without room.  steps: as keep()'s, default all.  At least one rule must be given;
        batch: the rows of the decode.  no_restrike or a floor makes the decode the constrained kind (an `ascending` nobody gave becomes
        False, no temperature is the constrained argmax); a ceiling alone runs in every kind.  Kept notes win over the cap.  Every bad
        value is a ValueError before anything touches the GPU."""
        return build_sounding(self.device, no_restrike, max_sounding, min_sounding, steps, batch)

    def split_top(self, x, top_steps, above=None, highest=None, whole_steps=None):
        """The selection of keep_top as two grids -> (x_top, x_rest, kept_n, err) (ptv_grid_split_top), the mirror of split_voice: x_top
        holds per step the notes keep_top forces (a top step: the kept notes and an <eos>; a whole step: the step; a free step: the empty
        step), x_rest the notes under them; x_rest's notes followed by x_top's are x's.  Split x and a decode that kept its top with the
        same arguments to compare the re-drawn lower voices with the original ones.  Nothing is copied to the host."""
        return split_top(x, top_steps, above, highest, whole_steps)

    def split_voice(self, x, voice_steps, below=None, lowest=None, whole_steps=None):
        """The selection of keep_voice as two grids -> (x_voice, x_rest, kept_n, err) (ptv_grid_split_voice): x_voice holds per step the
        notes keep_voice forces (a voice step: the kept notes and an <eos>; a whole step: the step; a free step: the empty step), x_rest
        the others moved down to slot 1, both int64 [B, 32, 16, 6] in the model's layout -- what score, reconstruction_report, keep and
        grid_to_pr_and_notes_batch take; kept_n int32 [B, 32] and err int32 [B] as keep_voice's.  Split x and a decode that kept its voice
        with the same arguments to compare the re-drawn upper voices with the original ones.  Nothing is copied to the host."""
        return split_voice(x, voice_steps, below, lowest, whole_steps)

    def pitch_mask(self, c=None, pitch_classes=None, lo=None, hi=None, batch=None):
        """int32 device tensor [B, 32, 4] for pitch_mask= (ptv_pitch_mask_build): bit p & 31 of word p >> 5 of [b, t] set = grid pitch p
        allowed at time step t.  The constraints given are ANDed: c (f32 [B, 8, 36] on the device, the chord input): the chord tones --
        p passes at step t iff c[b, t // 4, 12 + p % 12] != 0; pitch_classes: the allowed pitch classes, an iterable of 0..11 or a 12-bit
        set; lo / hi: the pitch range lo <= p <= hi.  B = c.shape[0], else batch, else 1 (one row serves every batch)."""
        k = 0xfff
        if pitch_classes is not None:
            if isinstance(pitch_classes, bool):
                raise ValueError('pitch_classes must be a 12-bit set or an iterable of pitch classes 0..11')
            if isinstance(pitch_classes, int):
                k = pitch_classes
            else:
                k = 0
                for q in pitch_classes:
                    if isinstance(q, bool) or not isinstance(q, int) or not 0 <= q < 12:
                        raise ValueError('a pitch class must be an integer in 0..11, got %r' % (q,))
                    k |= 1 << q
            if not 0 <= k <= 0xfff:
                raise ValueError('pitch_classes must be a 12-bit set, got %r' % (pitch_classes,))
        lo_, hi_ = 0 if lo is None else lo, 127 if hi is None else hi
        for name, v in (('lo', lo_), ('hi', hi_)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 127:
                raise ValueError('%s must be an integer in 0..127, got %r' % (name, v))
        if lo_ > hi_:
            raise ValueError('lo must not exceed hi, got [%d, %d]' % (lo_, hi_))
        if c is not None:
            if not torch.is_tensor(c) or c.device.type != 'cuda' or c.dtype != torch.float32 or c.dim() != 3 or tuple(c.shape[1:]) != (8, 36):
                raise ValueError('c must be a float32 device tensor [B, 8, 36]')
            if batch is not None and batch != c.shape[0]:
                raise ValueError('batch is %r, c has %d rows' % (batch, c.shape[0]))
            c = c.contiguous()
        B = c.shape[0] if c is not None else (1 if batch is None else batch)
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError('batch must be an integer >= 1, got %r' % (batch,))
        out = torch.empty(B, 32, 4, dtype=torch.int32, device=c.device if c is not None else self.device)
        call('ptv_pitch_mask_build', ptr(out), B, lo_, hi_, k, ptr(c) if c is not None else None, stream_ptr())
        return out

    def inference_decode(self, z_chd, z_rhy, *, temperature=None, dur_temperature=None, seed=None, draw=None, sample_offset=None,
                         top_k=None, min_p=None, top_p=None, rows=None, pitch_mask=None, ascending=None, keep=None, sounding=None):
        kw = locals()
        return self._inference_decode(z_chd, z_rhy, self._request(z_chd.shape[0], **{k: kw[k] for k in DECODE_KEYS}))

    def _inference_decode(self, z_chd, z_rhy, req):
        self.eval()
        refresh_weight_shadows()
        with torch.no_grad():
            self._decode(z_chd, z_rhy, req)
            est_x = self.decoder.last_xhat[:, :, 1:, :].cpu().numpy()
        return est_x

    # ---- the row-independent chord decode (INTEGRATION.md "Chord decode"; ptv_chord_decode).  decode_tokens -- the default of the output path
    # below -- feeds back the reference's union over the batch of the rows' root / bass decisions (ptvae.py:74-77): right for parity with the
    # training step, but a row's chords then depend on the rest of the batch.  chord_temperature / chroma_temperature / keep_chords select the
    # decode in which every row feeds back its own token: sharding-invariant like the note decode, sampled from the same Philox domain
    # (note step 15: a slot no note decision uses), with kept chords and log-probabilities.
    def _chord_request(self, batch, chord_temperature=None, chroma_temperature=None, keep_chords=None, seed=None, draw=None,
                       sample_offset=None, note_sampled=False, required=False, grammar=None):
        """None when no chord keyword is given (the caller keeps decode_tokens), else the ChordRequest; every bad value is a ValueError
        here: no launch, no side effect.  note_sampled: the note decode of the same call is sampled (seed / draw / sample_offset then
        belong to it as well and are no error without a chord temperature); required: the caller runs the chord decode whatever is given"""
        if chord_temperature is None and chroma_temperature is None and keep_chords is None and grammar is None and not required:
            return None
        given = (seed, draw, sample_offset)
        sampled = check_chord_sampling(chord_temperature, chroma_temperature, *((None, None, None) if note_sampled and chord_temperature is None
                                                                                 else given))
        check_chord_keep(keep_chords, batch)
        check_chord_grammar(grammar, batch)
        return ChordRequest(sampled, chord_temperature, chroma_temperature, seed, draw, sample_offset, keep_chords, grammar)

    @staticmethod
    def _check_grammar_device(creq, z_chd):
        """ValueError, before anything is launched, for a grammar that lives on another device than the latents"""
        if creq is not None and creq.grammar is not None and creq.grammar.rule.device != z_chd.device:
            raise ValueError('the chord grammar must be on the device of z_chd (%s), it is on %s' % (z_chd.device, creq.grammar.rule.device))

    def _decode_chords(self, z_chd, creq, draw, return_logprob=False):
        """the chord decode of a ChordRequest; draw: the draw number a request that names none uses"""
        ph = self._philox or (7, 0)
        return self.chd_decoder.decode_chords(
            z_chd, temperature=creq.temperature, chroma_temperature=creq.chroma_temperature, seed=ph[0] if creq.seed is None else creq.seed,
            draw=draw if creq.draw is None else creq.draw, sample_offset=ph[1] if creq.sample_offset is None else creq.sample_offset,
            keep=creq.keep, return_logprob=return_logprob, grammar=creq.grammar)

    def keep_chords(self, c, steps):
        """The kept chord steps of a chord decode -> functional_free.ChordKeep(c, steps, batch) for keep_chords= (INTEGRATION.md "Chord
        decode").  c: f32 device tensor [B, 8, 36] (what decode_chords, decode_to_inputs and the dataset path give); steps: a device
        bool / uint8 tensor [B, 8] or [1, 8], or a host iterable of step indices / a slice (one row for every sample: range(4) = the
        first bar).  At a kept step root, chroma bits and bass are forced from c[b, t] and fed back like decisions.  A root or bass block
        without exactly one non-zero entry forces nothing for that head and sets bit 0 of ChordLogprob.err[b].  Nothing is copied to the
        host."""
        return build_chord_keep(c, steps)

    def chord_grammar(self, key=None, scale='major', roots=None, pitch_classes=None, qualities=None, root_in_chord=None, bass_in_chord=False,
                      steps=None, batch=None):
        """The grammar of a chord decode -> functional_free.ChordGrammar(rule int32 [R, 8], vocab int32 [V], batch) for grammar= /
        chord_grammar= (INTEGRATION.md "Chord grammar"), built on the device; nothing is copied to the host.
        key: None, an int 0..11, or an int device tensor [B] / [B, 8] (a key per row, or per row and chord step).  The values of a tensor
        are not read on the host, so they cannot be refused: they are taken modulo 12 (-1 is B, 12 is C), where an int outside 0..11 is a
        ValueError.
        scale: 'major', 'minor' (natural), 'harmonic_minor', a 12-bit set or an iterable of degrees 0..11 above the key.  With a key the
        scale on it is the chroma mask -- the pitch classes a chord may hold -- and the root mask, unless roots= (a 12-bit set or an
        iterable, relative to the key; absolute without one) names another set.  Without a key the scale is not applied: every root and
        pitch class is allowed but for roots / pitch_classes.  pitch_classes: an absolute chroma mask, ANDed with the key's.
        qualities: None (the twelve chroma bits stay independent draws), 'triads' (maj, min, dim, aug), 'sevenths' (the triads, maj7, 7,
        m7, m7b5, dim7, mMaj7), or an iterable of 12-bit sets / interval tuples that hold 0: the chroma becomes ONE draw from these chords
        on the decided root, from the model's own distribution conditioned on them (at most 64).
        root_in_chord (default: True with qualities, else False): the decided root's chroma bit is 1.  bass_in_chord: the bass is a tone
        of the decided chord.  steps: the chord steps the rule applies to -- an iterable of 0..7, a slice, or a device bool / uint8 tensor
        [B, 8] / [1, 8]; the others decode as without a grammar.  batch: the rows R of the rule when no tensor gives them (default 1: one
        row serves every batch).  Every bad value is a ValueError before any device work."""
        vocab = chord_vocabulary(qualities)
        if isinstance(scale, str):
            if scale not in CHORD_SCALES:
                raise ValueError("scale must be one of %s, a 12-bit set or an iterable of degrees, got %r" % (sorted(CHORD_SCALES), scale))
            scale_set = CHORD_SCALES[scale]
        else:
            scale_set = pitch_class_set(scale, 'scale')
        roots_set = None if roots is None else pitch_class_set(roots, 'roots')
        pcs = None if pitch_classes is None else pitch_class_set(pitch_classes, 'pitch_classes')
        for name, v in (('root_in_chord', root_in_chord), ('bass_in_chord', bass_in_chord)):
            if not isinstance(v, bool) and not (name == 'root_in_chord' and v is None):
                raise ValueError('%s must be a bool, got %r' % (name, v))
        if vocab and root_in_chord is False:
            raise ValueError('root_in_chord=False contradicts qualities: every chord of a vocabulary holds its root')
        if batch is not None and (isinstance(batch, bool) or not isinstance(batch, int) or batch < 1):
            raise ValueError('batch must be an integer >= 1, got %r' % (batch,))
        rows = batch
        if torch.is_tensor(key):
            if key.dtype not in (torch.int32, torch.int64) or key.dim() not in (1, 2) or key.shape[0] < 1 or \
                    (key.dim() == 2 and key.shape[1] != CHORD_STEPS):
                raise ValueError('key must be an int 0..11 or an int32 / int64 tensor [B] or [B, 8], got %s %s' % (key.dtype, tuple(key.shape)))
            if rows is not None and key.shape[0] != rows:
                raise ValueError('batch is %r, key has %d rows' % (batch, key.shape[0]))
            rows = key.shape[0]
        elif key is not None and (isinstance(key, bool) or not isinstance(key, int) or not 0 <= key < 12):
            raise ValueError('key must be an int 0..11 or an int tensor [B] / [B, 8], got %r' % (key,))
        dev = key.device if torch.is_tensor(key) else None
        if torch.is_tensor(steps):
            if steps.dtype not in (torch.bool, torch.uint8) or steps.dim() != 2 or steps.shape[1] != CHORD_STEPS or steps.shape[0] < 1:
                raise ValueError('steps must be a bool / uint8 tensor [B, 8] or [1, 8], an iterable of step indices or a slice')
            if rows is not None and steps.shape[0] not in (1, rows):
                raise ValueError('steps has %d rows, the grammar %d' % (steps.shape[0], rows))
            if dev is not None and steps.device != dev:
                raise ValueError('steps must be on the device of key')
            dev = steps.device
        elif steps is not None:
            steps = chord_keep_steps_row(steps)
        if key is None:
            scale_set = 0xfff                                # a scale stands on a key: without one only roots / pitch_classes restrict
        return build_chord_grammar(self.device if dev is None else dev, key, scale_set, roots_set, pcs, vocab,
                                   bool(vocab) if root_in_chord is None else root_in_chord, bass_in_chord, steps, batch)

    def decode_chords(self, z_chd, *, chord_temperature=None, chroma_temperature=None, seed=None, draw=None, sample_offset=None,
                      keep_chords=None, return_logprob=False, grammar=None):
        """Row-independent free-running chord decode of z_chd -> (c f32 [B,8,36], chord14 f32 [B,8,14]), with return_logprob=True also a
        ChordLogprob (RnnDecoder.decode_chords).  seed / sample_offset default to use_philox()'s, else 7 / 0; draw defaults to the
        model's draw counter, which a sampled decode that names none advances.  Without a temperature: the argmax (of each row's own
        trajectory).  grammar: what chord_grammar() returns -- allowed roots and pitch classes, a chord-quality vocabulary, a chord-tone
        bass; a grammar alone is no sampled decode (the argmax snapped to the grammar; the counter stays).  Bad values are a ValueError
        before anything is launched and before the counter moves."""
        if not torch.is_tensor(z_chd) or z_chd.dim() != 2:
            raise ValueError('z_chd must be a tensor [B, z_dim]')
        creq = self._chord_request(z_chd.shape[0], chord_temperature, chroma_temperature, keep_chords, seed, draw, sample_offset, required=True,
                                   grammar=grammar)
        _require_cuda(z_chd, 'DisentangleVAE.decode_chords')
        self._check_grammar_device(creq, z_chd)
        self.eval()
        out = self._decode_chords(z_chd, creq, self._sample_draws, return_logprob)
        if creq.sampled and draw is None:
            self._sample_draws += 1
        return out

    # ---- the output path on the device: decoded grid and chord logits -> the three tensors the model consumes plus a note list
    # (ptv_grid_to_pr, ptv_chord_tokens); inference_decode above stays the reference's host form
    def decode_to_inputs(self, z_chd, z_rhy, max_notes=10, *, temperature=None, dur_temperature=None, seed=None, draw=None,
                         sample_offset=None, top_k=None, min_p=None, top_p=None, rows=None, pitch_mask=None, ascending=None, keep=None,
                         sounding=None, return_logprob=False, chord_temperature=None, chroma_temperature=None, keep_chords=None, chord_grammar=None):
        """Free-running decode of (z_chd, z_rhy) -> (pr_mat f32 [B,32,128], x int64 [B,32,16,6], c f32 [B,8,36], notes int32
        [B,32*max_notes,3], count int32 [B], err int32 [B]); nothing leaves the device.  (pr_mat, c) feed inference_encode, (x, c,
        pr_mat) feed loss(); notes / count / err as PtvaeDecoder.grid_to_pr_and_notes_batch.  The keywords of a sampled decode as
        inference_decode's (they leave the chord decoder at its argmax).  return_logprob=True appends the decode's log-probabilities
        (PtvaeDecoder.decode_logprob: a DecodeLogprob of device tensors) as a seventh element.
        chord_temperature / chroma_temperature / keep_chords / chord_grammar (any of them given): c comes from the row-independent chord decode
        (decode_chords above) instead of decode_tokens, and return_logprob appends its ChordLogprob as an eighth element.  One call is one
        draw: both decoders take seed / draw / sample_offset, and when no draw is named both use the counter's value and it advances
        once.  chord_grammar: what chord_grammar() returns (INTEGRATION.md "Chord grammar"); alone it is no sampled decode.  With none of
        the four the call is what it was: the same launches, the same bits."""
        kw = locals()
        B = z_chd.shape[0]
        note_sampled = temperature is not None or dur_temperature is not None or rows is not None
        creq = self._chord_request(B, chord_temperature, chroma_temperature, keep_chords, seed, draw, sample_offset, note_sampled,
                                   grammar=chord_grammar)
        note_kw = {k: kw[k] for k in DECODE_KEYS}
        if creq is not None and creq.sampled and not note_sampled:
            note_kw.update(seed=None, draw=None, sample_offset=None)                # (they belong to the chord decode alone)
        req = self._request(B, **note_kw)                                           # (bad values are a ValueError whatever device the inputs are on)
        _require_cuda(z_chd, 'DisentangleVAE.decode_to_inputs')
        _require_cuda(z_rhy, 'DisentangleVAE.decode_to_inputs')
        self._check_grammar_device(creq, z_chd)
        self.eval()
        refresh_weight_shadows()
        draw0 = self._sample_draws
        with torch.no_grad():
            self._decode(z_chd, z_rhy, req)
            pr_mat, notes, count, x, err = self.decoder.grid_to_pr_and_notes_batch(self.decoder.last_xhat, max_notes)
            if creq is None:
                c, _ = self.chd_decoder.decode_tokens(z_chd)
                if return_logprob:
                    return pr_mat, x, c, notes, count, err, self.decoder.decode_logprob()
                return pr_mat, x, c, notes, count, err
            out = self._decode_chords(z_chd, creq, draw0, return_logprob)
            if creq.sampled and draw is None and self._sample_draws == draw0:
                self._sample_draws += 1
            if return_logprob:
                return pr_mat, x, out[0], notes, count, err, self.decoder.decode_logprob(), out[2]
        return pr_mat, x, out[0], notes, count, err

    def decode_logprob(self, z_chd, z_rhy, max_notes=10, **sampling):
        """decode_to_inputs' tuple plus the log-probabilities of that decode (INTEGRATION.md "Decode log-probabilities"): a
        DecodeLogprob(logp [B,2], logq [B,2], counts [B,4], err [B], step_logp [B,32,4], step_counts [B,32,4]) of device tensors --
        log p under the model's own softmax and log q under the distribution the decode drew from, (pitch, duration) sums over the
        decisions taken.  **sampling: the keywords of a sampled decode (inference_decode); with chord_temperature / chroma_temperature /
        keep_chords / chord_grammar the ChordLogprob of the row-independent chord decode follows the DecodeLogprob."""
        return self.decode_to_inputs(z_chd, z_rhy, max_notes, return_logprob=True, **sampling)

    @staticmethod
    def _check_best_of(n, rank_by='logp', length_normalize=False, temperature=None, dur_temperature=None, rows=None, **_):
        """ValueError for a bad decode_best_of argument; no side effect, no launch"""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError('n must be an integer >= 1, got %r' % (n,))
        if rank_by not in ('logp', 'logq'):
            raise ValueError("rank_by must be 'logp' or 'logq', got %r" % (rank_by,))
        if not isinstance(length_normalize, bool):
            raise ValueError('length_normalize must be a bool, got %r' % (length_normalize,))
        if temperature is None and dur_temperature is None and rows is None:
            raise ValueError('decode_best_of ranks draws of a sampled decode: give a temperature (an argmax decode has one candidate)')

    def decode_best_of(self, z_chd, z_rhy, n, *, rank_by='logp', length_normalize=False, max_notes=10, **sampling):
        """n sampled decodes of every row, the best of them by log-probability (INTEGRATION.md "Best of n") -> decode_to_inputs' tuple of
        the winners plus (best int32 [B], sums f32 [B,4] = the winner's (logp pitch, logp dur, logq pitch, logq dur)); all on the device.
        The batch is tiled n times: candidate k of row b is row k*B + b and draws the noise of global sample sample_offset + k*B + b, so
        the candidates are bit-equal to a plain decode of the tiled batch with the same keywords; a pitch_mask or keep with B rows is
        tiled alike.  rank_by: 'logp' (the model's own probability of what was drawn) or 'logq' (the proposal's); length_normalize
        divides the score by the number of counted decisions.  The first maximal candidate wins (ptv_best_of_gather); a NaN score never
        wins.  err is the output path's, with two bits above it: bit 8 = a candidate of the row held a decision outside the recomputed kept
        set (never on the decoder's own outputs), bit 9 = every score of the row was NaN (candidate 0 is returned).  A temperature
        is required: without one there is one candidate."""
        self._check_best_of(n, rank_by, length_normalize, **sampling)
        B = z_chd.shape[0]
        req = self._request(B, **sampling)
        _require_cuda(z_chd, 'DisentangleVAE.decode_best_of')
        _require_cuda(z_rhy, 'DisentangleVAE.decode_best_of')
        self.eval()
        refresh_weight_shadows()
        with torch.no_grad():
            self._decode(z_chd.repeat(n, 1), z_rhy.repeat(n, 1), req.tiled(n))
            lp = self.decoder.decode_logprob()
            sums = torch.cat([lp.logp, lp.logq], dim=1)
            score = (lp.logp if rank_by == 'logp' else lp.logq).sum(1)
            if length_normalize:
                score = score / (lp.counts[:, 0] + lp.counts[:, 1]).clamp(min=1).float()
            grids = self.decoder.last_xhat
            dev = grids.device
            best = torch.empty(B, dtype=torch.int32, device=dev)
            berr = torch.empty(B, dtype=torch.int32, device=dev)
            grid = torch.empty(B, 32, 16, 6, dtype=torch.int64, device=dev)
            bsums = torch.empty(B, 4, dtype=torch.float32, device=dev)
            call('ptv_best_of_gather', ptr(score.contiguous()), ptr(grids), ptr(sums), n, B, ptr(best), ptr(grid), ptr(bsums), ptr(berr),
                 stream_ptr())
            pr_mat, notes, count, x, err = self.decoder.grid_to_pr_and_notes_batch(grid, max_notes)
            c, _ = self.chd_decoder.decode_tokens(z_chd)
        return pr_mat, x, c, notes, count, err | ((berr | lp.err.view(n, B).amax(0)) << 8), best, bsums

    def reencode(self, z_chd, z_rhy, **sampling):
        """(dist_chd, dist_rhy) of the music decoded from (z_chd, z_rhy): decode_to_inputs, then inference_encode; **sampling: the
        keywords of a sampled decode (inference_decode) and of the chord decode (chord_temperature, chroma_temperature, keep_chords,
        chord_grammar)"""
        pr_mat, _, c, _, _, _ = self.decode_to_inputs(z_chd, z_rhy, **sampling)
        return self.inference_encode(pr_mat, c)

    # ---- model.py:133-142
    def inference(self, pr_mat, c, sample, **sampling):
        """pr_mat: the texture encoder's input -- the piano-roll, or dt_x for the detrended variant; **sampling: the keywords of a sampled
        decode (inference_decode), here and in swap / posterior_sample / prior_sample / interp -- a bad value is a ValueError before
        anything is encoded"""
        req = self._request(pr_mat.shape[0], **sampling)
        if self.detrended:
            self._check_dt_x(pr_mat)                     # (a piano-roll here is a ValueError, not a shape crash inside a kernel)
        self.eval()
        refresh_weight_shadows()
        with torch.no_grad():
            dist_chd = self.chd_encoder(c)
            dist_rhy = self._encode_texture(pr_mat)
            z_chd = self._rsample('chd', dist_chd) if sample else dist_chd.mean
            z_rhy = self._rsample('rhy', dist_rhy) if sample else dist_rhy.mean
        return self._inference_decode(z_chd, z_rhy, req)

    # ---- model.py:144-148
    def swap(self, pr_mat1, pr_mat2, c1, c2, fix_rhy, fix_chd, **sampling):
        """pr_mat1 / pr_mat2: texture encoder inputs -- piano-rolls, or dt_x grids for the detrended variant"""
        pr_mat = pr_mat1 if fix_rhy else pr_mat2
        c = c1 if fix_chd else c2
        return self.inference(pr_mat, c, sample=False, **sampling)

    # ---- model.py:150-172
    def posterior_sample(self, pr_mat, c, scale=None, sample_chd=True, sample_txt=True, **sampling):
        """pr_mat: the texture encoder's input -- the piano-roll, or dt_x for the detrended variant"""
        if scale is None and sample_chd and sample_txt:
            return self.inference(pr_mat, c, sample=True, **sampling)
        req = self._request(pr_mat.shape[0], **sampling)
        dist_chd, dist_rhy = self.inference_encode(pr_mat, c)
        if scale is not None:
            dist_chd = HipNormal(dist_chd.mean, dist_chd.scale * scale)
            dist_rhy = HipNormal(dist_rhy.mean, dist_rhy.scale * scale)
        with torch.no_grad():
            # the reference draws BOTH latents (get_zs_from_dists(..., True), model.py:165) and then overrides the unsampled one with
            # its mean: the generator / draw counter advances by two draws whatever the flags say, so the sampled latent sees the
            # same noise as in the reference under a seeded generator
            z_chd, z_rhy = self._rsample('chd', dist_chd), self._rsample('rhy', dist_rhy)
            if not sample_chd:
                z_chd = dist_chd.mean
            if not sample_txt:
                z_rhy = dist_rhy.mean
        return self._inference_decode(z_chd, z_rhy, req)

    # ---- model.py:174-184
    def prior_sample(self, x, c, sample_chd=False, sample_rhy=False, scale=1., **sampling):
        """x: the texture encoder's input (the reference's name for this slot here) -- the piano-roll, or dt_x for the detrended variant"""
        req = self._request(x.shape[0], **sampling)
        dist_chd, dist_rhy = self.inference_encode(x, c)
        mean = torch.zeros_like(dist_rhy.mean)
        loc = torch.ones_like(dist_rhy.mean) * scale
        if sample_chd:
            dist_chd = HipNormal(mean, loc)
        if sample_rhy:
            dist_rhy = HipNormal(mean, loc)
        with torch.no_grad():
            z_chd, z_rhy = self._rsample('chd', dist_chd), self._rsample('rhy', dist_rhy)
        return self._inference_decode(z_chd, z_rhy, req)

    # ---- model.py:186-188
    def gt_sample(self, x):
        return x[:, :, 1:].cpu().numpy()

    # ---- model.py:190-209: decode int_count points on the path between two items' latent codes
    def interp(self, pr_mat1, c1, pr_mat2, c2, interp_chd=False, interp_rhy=False, int_count=10, **sampling):
        """pr_mat1 / pr_mat2: texture encoder inputs -- piano-rolls, or dt_x grids for the detrended variant; a sampled decode's sample
        index is the row of the flattened [bs * int_count] batch, and so are the rows of a pitch_mask (or it has one row)"""
        req = self._request(pr_mat1.shape[0] * int_count, **sampling)
        dist_chd1, dist_rhy1 = self.inference_encode(pr_mat1, c1)
        dist_chd2, dist_rhy2 = self.inference_encode(pr_mat2, c2)
        z_chd1, z_rhy1, z_chd2, z_rhy2 = dist_chd1.mean, dist_rhy1.mean, dist_chd2.mean, dist_rhy2.mean
        z_chds = self.interp_z(z_chd1, z_chd2, int_count) if interp_chd else z_chd1.unsqueeze(1).repeat(1, int_count, 1)
        z_rhys = self.interp_z(z_rhy1, z_rhy2, int_count) if interp_rhy else z_rhy1.unsqueeze(1).repeat(1, int_count, 1)
        bs = z_chds.size(0)
        estxs = self._inference_decode(z_chds.reshape(bs * int_count, -1).contiguous(), z_rhys.reshape(bs * int_count, -1).contiguous(), req)
        return estxs.reshape((bs, int_count, 32, 15, -1))

    # ---- model.py:211-216: [B,D] x [B,D] -> [B,int_count,D]; the reference loops over numpy rows on the host, here the
    # whole batch is one launch on the device holding z (ptv_slerp_path)
    def interp_z(self, z1, z2, int_count=10):
        z1, z2 = z1.detach().float().contiguous(), z2.detach().float().contiguous()
        if not z1.is_cuda:
            z1, z2 = z1.to(self.device), z2.to(self.device)
        B, D = z1.shape
        out = torch.empty(B, int_count, D, device=z1.device, dtype=torch.float32)
        F_.call('ptv_slerp_path', F_.ptr(z1), F_.ptr(z2), F_.ptr(out), B, D, int_count, F_.stream_ptr())
        return out

    # ---- model.py:218-242: one pair of codes (any shape); spherical interpolation of the directions, geometric of the norms
    def interp_path(self, z1, z2, interpolation_count=10):
        t1 = torch.as_tensor(z1, dtype=torch.float32)
        shape = list(t1.shape)
        out = self.interp_z(t1.reshape(1, -1), torch.as_tensor(z2, dtype=torch.float32).reshape(1, -1), interpolation_count)
        return out.reshape([interpolation_count] + shape)

    # ---- model.py:244-265
    @staticmethod
    def init_model(device=None, chd_size=256, txt_size=256, num_channel=10):
        name = 'disvae'
        if device is None:
            device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        chd_encoder = RnnEncoder(36, 1024, chd_size)
        rhy_encoder = TextureEncoder(256, 1024, txt_size, num_channel)
        chd_decoder = RnnDecoder(z_dim=chd_size)
        pt_decoder = PtvaeDecoder(note_embedding=None, dec_dur_hid_size=64, z_size=chd_size + txt_size)
        return DisentangleVAE(name, device, chd_encoder, rhy_encoder, pt_decoder, chd_decoder)

    # ---- train.py:31-39: the reference's own entry script wires a PtvaeEncoder over the 39-wide detrended grid as the texture encoder
    @staticmethod
    def init_model_detrended(device=None):
        name = 'disvae-nozoth'
        if device is None:
            device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        chd_encoder = RnnEncoder(36, 1024, 256)
        rhy_encoder = PtvaeEncoder(device=device, z_size=256, max_pitch=39 - 8, min_pitch=0)
        chd_decoder = RnnDecoder(z_dim=256)
        pt_decoder = PtvaeDecoder(note_embedding=None, dec_dur_hid_size=64, z_size=512)
        return DisentangleVAE(name, device, chd_encoder, rhy_encoder, pt_decoder, chd_decoder)


PolyphonicVAE = DisentangleVAE      # the name BASELINE.json's north_star uses
