// version.hip -- build identification of libptvae_hip.so
#include "../../include/ptvae_hip.h"
extern "C" const char* ptv_arch(void) { return "gfx950"; }
// 2 (round 3): ptv_step_params / ptv_ordered_reductions / ptv_wgrad_mode added; ptv_gemm dtypes bit 3 (column-blocked C); the
// row-partitioned GRU pair takes gc / ext column-blocked and keeps its gate planes unit-blocked
// 3 (round 4): ptv_dur_gru_bwd takes b_hh / tab0 / tab (gates may be NULL: recompute); ptv_txt_conv_relu_pool_*_rows take the arg-max
// map; ptv_*_geom, ptv_heads_*, ptv_pack_mfma_b2 / _multi, ptv_gru_persist_bwd_splitk, ptv_gradnorm_clip_adam_step and the composites
// ptv_decoder_tf_fwd / ptv_chord_decoder_fwd added
// 4 (round 5): ptv_notes_gru_persist_fwd is the wave-role kernel (pairs = 0 packs, gc / gate planes unit-blocked by 16, h0 read only: no
// fp32 states written); ptv_notes_gru_persist_bwd / ptv_row_gru_persist_bwd(H = 512) take the bf16 states; ptv_gemm dtypes bit 4 (C
// column-blocked by 16); ptv_pianotree_targets writes counts[3] (since round 4, unversioned then); ptv_debug_notes_trace added
// 5 (round 5): ptv_row_gru_persist_{fwd,bwd}_perm and ptv_rows_by_length added (panels of rows sorted by length)
// 6 (round 6): the ptv_*_top entry points / PTV_DTF_LIVE_TOP (round 5, unversioned then), the bwd / loss / bigru composites, row limits in
// ptv_wgrad's guarded tail and ptv_dur_out_wgrad, PTV_BGF_D_W_IH_F32; debug / profiling entry points moved to ptvae_hip_debug.h;
// ptv_header_hash added (the loader compares it with the headers it binds from)
// 7 (round 7): the output path and the device song bank (ptv_grid_to_pr, ptv_chord_tokens, ptv_window_rolls, ptv_detrend_pianotree)
// still 7: ptv_rows_plan (sort + sorted lengths + segment counts in one multi-block launch) and ptv_gemm_mtop_seg_map (a row map on the
// plain product's C) added, PTV_DTB_DNS_S / PTV_DTB_DTOK_S removed (ptv_decoder_tf_bwd's sorted branch stores through PERM).  The number
// stays because the host tests of the two round-7 families pin it; ptv_header_hash below is what refuses a library built from other headers
// still 7: the per-sample scores (csrc/score.hip: ptv_recon_step_scores, ptv_score_fold, ptv_kl_rows, ptv_chord_step_scores, ptv_roll_match)
// added; no existing entry point changed, and the same host tests pin the number
// still 7: the row-wise decode kind (ptv_note_token_sample_rows, ptv_dur_gru_fwd_sample_rows, ptv_dur_out_token_sample_rows, bit 26 of
// ptv_free_note_loop's train word, PTV_DFF_D_SAMPLE_ROWS appended, the 80-byte block of ptv_decode_logprob) added; no existing entry
// point changed its arguments, and the same host tests pin the number
// still 7: ptv_note_count_force_build (csrc/keep.hip, "Note-count limits") added as the builders before it were -- a new entry point, no
// existing one changed, the same host tests pin the number; the header hash moves with the declaration
// still 7: the chord grammar (csrc/chord_decode.hip: ptv_chord_decide_grammar, ptv_chord_decode_grammar and its PTV_CDG_* tables) added;
// no existing entry point changed, the same host tests pin the number
// still 7: the sounding state (csrc/sounding.hip: ptv_sounding_step; PTV_DFF_SND_* / PTV_DFF_D_SND* appended to ptv_decoder_free_fwd's
// enums, all zero = the call as it was) added; no existing entry point changed, the header hash moves with the declarations
extern "C" int ptv_abi_version(void) { return 7; }
#ifndef PTV_HEADER_HASH
#define PTV_HEADER_HASH "unknown"
#endif
extern "C" const char* ptv_header_hash(void) { return PTV_HEADER_HASH; }
