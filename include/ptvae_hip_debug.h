/* ptvae_hip_debug.h -- instrumentation and test aids of libptvae_hip.so.  NOT part of the product ABI (include/ptvae_hip.h): nothing on
 * the training / inference path calls these; bench.py's roofline block, scripts/ and two tests do.  Same conventions as ptvae_hip.h
 * (device pointers, hipStream_t as void*, 0 = ok).  Split out of ptvae_hip.h in round 6 (review item: the product header carried
 * debug hooks). */
#ifndef PTVAE_HIP_DEBUG_H
#define PTVAE_HIP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* timing experiments: device buffer of 8 x 2048 uint64 that one workgroup of the following forward launches fills with per-wave event
 * stamps (timing probe of round 5), or NULL */
int ptv_debug_notes_trace(void* buf);

/* test / diagnosis aid: nwg idle workgroups holding lds_bytes of LDS each for usec microseconds on `stream` (a stand-in for another
 * library's collective kernel sitting on the CUs the persistent recurrences were sized for; tests/test_gpu_zz_dist.py) */
int ptv_debug_pin_cus(int nwg, int lds_bytes, int usec, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optional launch timing (bench.py roofline): HIP events recorded on the launch stream around every launch of the enabled
 * kernel families.  Tags: 1 = GRU forward step, 2 = GRU backward step (csrc/gru.hip), 3 = row-partitioned persistent GRU forward,
 * 4 = its BPTT (csrc/notes_roles.hip / notes_persist.hip; M = rows R), 5 = weight-gradient products (ptv_wgrad / ptv_wgrad_cat: product +
 * reduction launches of one call), 6 = BPTT of the persistent small-M recurrences (ptv_gru_persist_bwd*), 7 = the free-running note loop (ptv_free_note_loop: 15 note steps per launch).  ptv_prof_enable takes a bit mask
 * (bit tag-1), ptv_prof_config restricts tags 1-4 to launches with the given (M, H) (0 = any).  ptv_prof_read_tag waits for the recorded events and returns the number of launches of
 * one tag (0 = all), their summed duration and their summed algorithmic MFMA FLOPs.
 */
int ptv_prof_enable(int mask);
int ptv_prof_config(int M, int H);
int ptv_prof_reset(void);
int ptv_prof_read_tag(int tag, long* count, double* total_ms, double* flops);
int ptv_prof_read(long* count, double* total_ms, double* flops);
/* of a tag's summed FLOPs, the part that runs under a device-side row limit (ptv_wgrad's k_top): products over the decoder's 15 note steps
 * (lim15) and over the note-summary GRU's 16 note positions (lim16) -- what bench.py scales by the batch's live fraction */
int ptv_prof_read_limited(int tag, double* lim15, double* lim16);
/* the part of lim15 whose products also skip the dead 128-row blocks of every note step (ptv_wgrad_job.seg_n) */
int ptv_prof_read_segmented(int tag, double* seg);

/* A/B / test aid: what "the library's rule" of the notes GRU panel height (ptvae_hip.h, T bits 25-26 of ptv_notes_gru_persist_fwd*, bits
 * 17-18 of ptv_notes_gru_persist_bwd*) answers: 0 (default) = the rule itself, 64 / 32 = that height.  Callers that force a height
 * are not affected.  Process-wide. */
int ptv_debug_notes_panel_rule(int rows);

/* A/B aid: how ptv_wgrad_batch issues its products (same bits in every mode): 0 = one by one (one product + one reduction launch each);
 * 1 = one product launch for all + one reduction launch; 2 = one product launch each + one reduction launch; 3 (default) = the small
 * products in one launch, the deep ones alone, one reduction launch.  Anything else is refused.  Process-wide; PTV_WGRAD_BATCH sets it at load. */
int ptv_wgrad_batch_mode(int batched);

/* test aid: the plan ptv_wgrad / ptv_wgrad_batch would run `job` (a ptv_wgrad_job of ptvae_hip.h) on, without running it.  Host only: launches
 * nothing and reads no device memory; the job's pointers are looked at for null and for alignment only.  out[10] =
 * {kfast, tiles_m, tiles_n, nslab_fast, kper_fast, map_fast, nslab_tail, kper_tail, map_tail, total_slabs}: rows [0, kfast) go to the unguarded
 * launch, the rest to the guarded one; a part that does not exist reports 0, 0, 0; all zero for M, N or K = 0.  Maps: 0 = slab-major, 1 =
 * whole slabs per XCD, 2 = tile ranges per XCD (csrc/wgrad.hip).  Returns what the product call would return for a job it refuses. */
struct ptv_wgrad_job;
int ptv_debug_wgrad_plan(const struct ptv_wgrad_job* job, int* out);

/* test aid of the sampled decode (ptvae_hip.h "Sampled decode"): the Gumbel values the decoder uses for rows [0, rows) -- samples
 * sample_offset + row of the block -- at time step t, note step n, through the decoder's own device functions: out_pitch [rows, 130],
 * out_dur [rows, 5, 2] (duration bit d: class 0, class 1) */
int ptv_debug_sample_noise(const void* block, long rows, int t, int n, float* out_pitch, float* out_dur, void* stream);

/* test aid of truncated sampling (ptvae_hip.h "Sampled decode", top_k / min_p / top_p): the decoder's own keep-threshold function
 * (csrc/philox.hpp pitch_keep_threshold) on caller-supplied rows, logits [rows, 130] fp32, under the 48-byte block (its T_pitch, top_k,
 * ln_min_p, top_p_q24 are read).  layout 0: 16 lanes per row, lane j owns columns j + 16 i (the note loops); layout 1: a wave per row, lane l owns
 * columns l + 64 i (the step loop).  keep_out [rows, 130] uint8 = logit >= threshold, thr_out [rows] fp32 = the threshold (-inf: no rule) */
int ptv_debug_pitch_keep(const void* block48, const float* logits, long rows, int layout, unsigned char* keep_out, float* thr_out, void* stream);

/* test aid of the constrained decode (ptvae_hip.h "Constrained decode"): the decoder's own allowed rule (csrc/philox.hpp pitch_constrain)
 * followed by pitch_keep_threshold on caller-supplied rows: logits [rows, 130] fp32, masks [rows, 4] int32 (the four mask words of each
 * row), lo [rows] int32, under the 64-byte block (its T_pitch, top_k, ln_min_p, top_p_q24 and flags are read, its mask address is not).
 * Layouts as above.  keep_out [rows, 130] uint8 = allowed and logit >= threshold, thr_out [rows] fp32 = the threshold */
int ptv_debug_pitch_constrain(const void* block64, const float* logits, const int* masks, const int* lo, long rows, int layout,
                              unsigned char* keep_out, float* thr_out, void* stream);
/* ... with the force word of each row, words [rows] int32 (ptvae_hip.h "Kept rhythm"): a row whose word is PTV_FORCE_NOT_EOS loses <eos> from its
 * allowed set unless nothing else is allowed, before the threshold is formed; a row whose word is PTV_FORCE_BELOW(u) has the allowed set of
 * "Kept top voice" (the notes under u, above lo under the ascending flag, within the mask unless that leaves none); every other word leaves the row what the entry above makes of
 * it (all words -1: the same bytes).  A NULL words is PTV_ERR_ARG. */
int ptv_debug_pitch_constrain_words(const void* block64, const float* logits, const int* masks, const int* lo, const int* words, long rows,
                                    int layout, unsigned char* keep_out, float* thr_out, void* stream);
/* ... with a row table in place of the block's scalars (ptvae_hip.h "Per-row sampling"): table int32 [rows, 8], 16-byte aligned -- row r is
 * judged with T_pitch, top_k, ln_min_p and top_p_q24 of record r; of the block only the flags are read.  In layout 0 a wave holds four rows,
 * so four records: the branches of the keep rule diverge between them.  words may be NULL (every decision plainly free).  A row whose record
 * holds the block's scalars gets the bytes the entry above writes for it. */
int ptv_debug_pitch_constrain_rows(const void* block64, const int* table, const float* logits, const int* masks, const int* lo,
                                   const int* words, long rows, int layout, unsigned char* keep_out, float* thr_out, void* stream);

/* test aid of the duration limits (ptvae_hip.h "Duration limits"): the decoder's own rule (csrc/philox.hpp dur_range_allowed /
 * dur_range_bit) on caller-supplied triples, words / d / prefix int32 [rows]: out [rows] uint8 -- bit 0 / bit 1: value 0 / 1 of duration bit
 * d is allowed after the prefix (a word that is no range word allows both), bit 2 / bit 3: the decision the rule makes of a decided 0 / a
 * decided 1.  0xff for a d outside 0..4 or a prefix outside 0..2^d - 1. */
int ptv_debug_dur_range(const int* words, const int* d, const int* prefix, long rows, unsigned char* out, void* stream);

/* test aid of the chord decode (ptvae_hip.h "Row-independent free-running chord decode"): the Gumbel values ptv_chord_decide uses for rows
 * [0, rows) -- samples sample_offset + row of the 32-byte block -- at chord step t, through the device function that kernel calls:
 * out [rows, 12, 4], lane j's four values in word order (root class j, bass class j, class 0 and class 1 of chroma bit j) */
int ptv_debug_chord_noise(const void* block, long rows, int t, float* out, void* stream);
/* ... and of the chord grammar's vocabulary draw (ptvae_hip.h "Chord grammar"), through the device function ptv_chord_decide_grammar
 * calls: out f32 [rows, n_vocab], the Gumbel value of template v, and words uint32 [rows, n_vocab], the Philox word it was made from
 * (word v >> 4 of the call sub = 16 + (v & 15)); n_vocab in 1..64 */
int ptv_debug_chord_vocab_noise(const void* block, long rows, int t, int n_vocab, float* out, unsigned* words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTVAE_HIP_DEBUG_H */
