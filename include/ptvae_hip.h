/* ptvae_hip.h -- C ABI of libptvae_hip.so: the MI355X (gfx950) kernels behind the polyphonic-VAE
 * training step (reference: ZZWaang/polyphonic-chord-texture-disentanglement, ptvae.py / model.py).
 *
 * The reference has no native layer of its own: its "FFI" for this path is PyTorch's ATen
 * (nn.GRU / nn.Linear / nn.Conv2d / CrossEntropyLoss / Normal / Adam).  Each entry point below
 * names the reference call site(s) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes binding the Python host uses.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors on the Python side) unless an entry point
 *     says "HOST array"; matrices are row-major with explicit leading dimensions (in elements)
 *   - element types: fp32 by default.  In bf16 precision the tensors that only ever feed MFMA operands or epilogues may be
 *     held as bf16 in HBM -- the caller says which through the dtype bits below (PTV_A/B/C_BF16 for ptv_gemm, PTV_GRU_*_BF16
 *     for the GRU entry points); parameters, optimiser state, recurrent state h, logits and all reductions stay fp32
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it, nothing synchronises
 *   - return value: 0 = ok, <0 = error (-1 bad argument, -2 launch failure, -3 unsupported shape for a
 *     specialised kernel: use the generic entry point); no exceptions cross the ABI
 *   - `prec`: PTV_PREC_F32 (0) = v_mfma_f32_16x16x4_f32, exact fp32 (parity path; every tensor fp32);
 *             PTV_PREC_BF16 (1) = v_mfma_f32_16x16x32_bf16, bf16 operands / fp32 accumulate (fp32 tensors are converted
 *             while staged, tensors flagged bf16 are read as they are)
 */
#ifndef PTVAE_HIP_H
#define PTVAE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PTV_PREC_F32 0
#define PTV_PREC_BF16 1

/* dtype bits of ptv_gemm: operands / result held as bf16 in HBM (bf16 precision only).  In bf16 mode
 * tensors that only ever feed MFMA operands are kept as bf16: half the traffic, no conversion. */
#define PTV_A_BF16 1
#define PTV_B_BF16 2
#define PTV_C_BF16 4
/* dtype bits of the GRU entry points */
#define PTV_GRU_GATES_BF16 1   /* saved gate planes */
#define PTV_GRU_GI_BF16 2      /* gi */
#define PTV_GRU_GI2_BF16 4     /* gi2 */
#define PTV_GRU_DG_BF16 8      /* dgi / dgh (backward) */
#define PTV_GRU_W_BF16 16       /* w_hh points at a bf16 copy of the weight (needs hall16 / DG_BF16);
                                   forward: W_hh [3H,H]; backward: the TRANSPOSED copy W_hh^T [H,3H] */
#define PTV_GRU_EXT_BF16 64     /* dh_ext (backward) holds bf16 */
#define PTV_GRU_SKIP_CAST0 32  /* hall16 slot 0 is already valid (chained single-step calls) */

/* Library / build identification ("gfx950"; ABI version 2 since round 3). */
const char* ptv_arch(void);
int ptv_abi_version(void);
/* first 16 hex digits of sha256(ptvae_hip.h || ptvae_hip_debug.h) as they were when the library was built (csrc/Makefile); a loader that
 * binds from these headers compares it with its own hash of them and refuses a stale library */
const char* ptv_header_hash(void);

/* ------------------------------------------------------------------------------------------------
 * Dense product  C[M,N] = act(alpha * A.B^T + bias) (+ C)      -- every nn.Linear forward
 * (ptvae.py:16-17,37-38,100-101,264-267,286-293), its input gradient (transB) and weight gradient
 * (transA+transB, split-K: each split stores its partial into a per-stream workspace and one more launch adds them in split
 * order; fp32 atomics into C only after ptv_ordered_reductions(0) / when no workspace can be had, see ptv_ordered_fallbacks).
 *   transA = 0: A[m*lda + k]   1: A[k*lda + m]
 *   transB = 0: B[n*ldb + k] (nn.Linear weight layout)   1: B[k*ldb + n]
 *   act: 0 none, 1 exp (linear_var(...).exp_(), ptvae.py:27,120)
 *   splitk: 0 auto, >0 forced number of K splits, <0 never split.  The count is rounded so that every split covers whole K tiles and
 *           none is empty (K = 0: one).  act != 0 with splitk > 1 is refused (PTV_ERR_ARG): exp of a partial sum is not a part of the
 *           result; the automatic split never splits a product with act.  bf16 C and column-blocked C refuse splitk > 1 as well.
 *   dtypes: bit 0 / 1 / 2 = A / B / C hold bf16 (bf16 precision only); bit 3 (8) / bit 4 (16) = C is COLUMN-BLOCKED by w = 32 / 16:
 *           element (m, n) lives at ((n / w) * M + m) * w + n % w (ldc unused, N a multiple of w, no K split) -- the layout in which the
 *           row-partitioned recurrences (ptv_notes_gru_persist_fwd: gc, w = 16; ptv_notes_gru_persist_bwd: ext, w = 32) read their
 *           per-row operands: a wave touches one contiguous kilobyte instead of 16 half cache lines
 */
int ptv_gemm(int prec, int transA, int transB, int M, int N, int K,
             const void* A, long lda, const void* B, long ldb,
             void* C, long ldc, const float* bias, float alpha,
             int accumulate, int act, int splitk, int dtypes, void* stream);
/* the same with a row limit on A (transA = 0): the rows of A from (*m_top + 1) * m_unit on are known to be zero (device int written
 * by the kernel that produced A, see ptv_notes_gru_persist_bwd): those row tiles skip the product, C gets bias / stays as it is */
int ptv_gemm_mtop(int prec, int transA, int transB, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                  void* C, long ldc, const float* bias, float alpha, int accumulate, int act, int splitk, int dtypes,
                  const int* m_top, long m_unit, void* stream);
/* ... and with ROW SEGMENTS of A (round 6; seg_n or NULL): the rows of A are units of seg_unit rows (a multiple of 128: a note step's decoder rows
 * in length order) of which only the first seg_n[unit % seg_period] (device ints, multiples of 128) hold anything -- the other row tiles are
 * treated like the ones beyond m_top (no K loop; C = bias / zero / unchanged) */
int ptv_gemm_mtop_seg(int prec, int transA, int transB, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                      void* C, long ldc, const float* bias, float alpha, int accumulate, int act, int splitk, int dtypes,
                      const int* m_top, long m_unit, const int* seg_n, long seg_unit, int seg_period, void* stream);
/* ... and with a ROW MAP on C (round 7; c_rows or NULL = ptv_gemm_mtop_seg): product row m is stored at -- and with accumulate read from --
 * C row (m / c_unit) * c_unit + c_rows[m % c_unit] (device ints); K order and epilogue arithmetic are those of the unmapped product, dead
 * row tiles put their zero / bias rows through the map (or return early where they change nothing).  THE CALLER GUARANTEES that c_rows is a
 * permutation of [0, c_unit): nothing checks it, a repeated index leaves a row unwritten and races on another, an index outside writes
 * outside C.  Refused (PTV_ERR_ARG, nothing launched): c_rows with column-blocked C (dtypes bits 3 / 4), with splitk > 1, with transA,
 * c_unit <= 0, M not a multiple of c_unit.  With splitk = 0 the product takes the K split the unmapped call would take (shallow grids of
 * deep products; the ordered reduction then stores through the map), so at every shape the result equals the unmapped product's bit for
 * bit.  The decoder's backward writes the gradients it computes in length-sorted row order straight into their natural-order tensors
 * this way. */
int ptv_gemm_mtop_seg_map(int prec, int transA, int transB, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                          void* C, long ldc, const float* bias, float alpha, int accumulate, int act, int splitk, int dtypes,
                          const int* m_top, long m_unit, const int* seg_n, long seg_unit, int seg_period,
                          const int* c_rows, long c_unit, void* stream);
/* plain products enqueued after this call raise their wave priority (p != 0) or run at the default one (0): host-side marker for the
 * launches of a latency chain that share the GPU with weight-gradient products on sibling streams.  Process-wide, read at enqueue time. */
int ptv_gemm_priority(int p);

/* ------------------------------------------------------------------------------------------------
 * GRU recurrence over T steps for M independent rows (torch.nn.GRU cell semantics; replaces the
 * per-step `self.gru(...)` / `dec_*_gru(...)` calls at ptvae.py:23,64-65,116,360,396-398,450,461-462,484).
 *   gi  [T] x [M,3H]   input-side pre-activations W_i x + b_i (gate order r,z,n), produced by ptv_gemm
 *   gi2 optional second addend with its own strides (may be NULL)
 *   hall [T+1][M][H]   slot 0 = initial state (written by the caller), slot s+1 = state after step s
 *   hall16 [T+1][M][H] optional bf16 copy of hall (bf16 precision): read as the MFMA operand of each step,
 *                 written next to hall, and reused by the caller as a bf16 operand of later products
 *   gates [T][4][M][H] saved r,z,n,(W_hn h + b_hn) for the backward pass, or NULL (inference)
 *   lengths[M] or NULL: packed-sequence masking (row m updated at time t iff t < lengths[m]),
 *                 the pack_padded_sequence semantics of ptvae.py:446-453,480-486
 *   reverse: processing step s consumes time index t = T-1-s (the *_reverse direction)
 *   gi_idx[M] or NULL: row m reads gi row gi_idx[m] instead of m (the duration GRU's input is a
 *                 one-hot token, so W_i x + b_i is a 2-row table indexed by the previous argmax)
 */
int ptv_gru_seq_fwd(int prec, int M, int H, int T,
                    const void* gi, long gi_step_stride, long gi_ld,
                    const void* gi2, long gi2_step_stride, long gi2_ld,
                    const void* w_hh, const float* b_hh,
                    float* hall, void* hall16, void* gates,
                    const int* lengths, int reverse, const int* gi_idx, int flags, void* stream);

/* One GRU cell step with explicit strides (same kernel as ptv_gru_seq_fwd, T = 1): the free-running
 * decoder (ptvae.py:395-424,460-486) advances a [B]-row window of the step-major buffers per step. */
int ptv_gru_step_fwd(int prec, int M, int H,
                     const float* hprev, long ld_hprev, const void* hprev16, void* hout16,
                     const void* gi, long gi_ld, const void* gi2, long gi2_ld,
                     const void* w_hh, const float* b_hh,
                     float* hout, long ld_hout,
                     void* gates, long gates_plane,
                     const int* lengths, int t, const int* gi_idx, int flags, void* stream);

/* BPTT through ptv_gru_seq_fwd (replaces autograd through the same call sites).
 *   dh_ext [T] x [M,H]  gradient arriving at the state after processing step s (may be NULL)
 *   dh_last [M,H]       gradient arriving at the final state only (may be NULL)
 *   lr_a/lr_b           optional low-rank external gradient: dh_s += lr_a_s[M,k] . lr_b[k,H]
 *                       (the 2-wide dur_out_linear feeding back into the duration GRU state)
 *   dgi [T][M][3H] (indexed by TIME t), dgh [T][M][3H] (indexed by processing step s)
 *   dhz scratch [2][M][H];  dh0 [M,H] gradient w.r.t. the initial state (may be NULL)
 * Weight gradients follow with ptv_gemm(transA=1,transB=1): dW_hh += dgh^T.hall[0:T], dW_ih += dgi^T.x
 */
int ptv_gru_seq_bwd(int prec, int M, int H, int T,
                    const float* hall, const void* gates, const void* w_hh,
                    const void* dh_ext, long ext_step_stride, long ext_ld,
                    const float* dh_last, long last_ld,
                    const float* lr_a, long lr_step_stride, long lr_lda, int lr_k, const float* lr_b,
                    void* dgi, void* dgh, float* dhz, float* dh0,
                    int reverse, int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Persistent, weight-stationary form of ptv_gru_seq_fwd / ptv_gru_seq_bwd for the small-M chains (the 32-step
 * dec_time_gru ptvae.py:461-462, the encoder bi-GRUs ptvae.py:23,116, the chord decoder ptvae.py:64-65):
 * ONE launch walks all T steps of up to 4 independent chains (e.g. both directions of a bi-GRU).  A workgroup
 * keeps its W_hh slice in LDS and the state of its own cells in registers for the whole sequence; per step only
 * the bf16 MFMA operand (h_s, or dgh_s in the BPTT) is exchanged between the workgroups of one row group
 * (write-through stores + arrival counter + L1-bypassing loads).  bf16 precision / bf16 storage only:
 *   gi, gi2, gates, dgi, dgh are bf16; w_hh16 = bf16 W_hh [3H,H]; w_t16 = bf16 W_hh^T [H,3H]; hall fp32 + hall16.
 * Same tensor layouts and semantics as ptv_gru_seq_fwd / ptv_gru_seq_bwd (dgi by time, dgh by processing step).
 * All array arguments are HOST arrays of NC entries (device pointers / strides per chain).
 * `xch`: per chain a bf16 scratch tensor for the exchanged operand, (T+1)*M*H elements (forward) / T*M*3H (backward),
 *   held K-blocked [step][k/8][row][8] so that the consumers' MFMA-fragment loads are contiguous across lanes.
 * `sync`: 16 * (1 + 32) device words (the host allocates 16 * (1 + 32 + 128): see the split-K form below) ZEROED by the caller on `stream` before the call: word 0 = error flag (non-zero
 *   after the launch = a bounded spin gave up, results invalid), word 16*(1+g) = arrival counter of row group g.
 * Returns PTV_ERR_UNSUPPORTED (-3) when the shape does not fit one workgroup per CU (H % 256, H <= 1024,
 * rows per workgroup <= 256): the caller then uses the per-step entry points.  At most ONE persistent launch may
 * be in flight on the device at a time (chain them with events across streams).
 * The plan (row groups RG, rows per workgroup 64 / 128 / 256, split-K: up to 512) is made from NC, M, H AND from the device's CU count
 *   minus ptv_gru_persist_cu_reserve: the same shape may be supported on one device or reserve and not on another, so ask
 *   ptv_gru_persist_supported / _splitk_supported (and _part_elems) after the reserve is set, on the device that runs the launch.
 *   RG is a power of two and M need not fill it: row groups that hold no row at all are legal (M = 257, H = 256 at 256 CUs: 4 groups
 *   of 128 rows, the last one empty); their workgroups only take part in the hand-offs.
 * Limits of `sync`: NC * RG <= 32 row-group counters and, split-K, NC * RG * (H / 16 / S) <= 128 team counters; a plan beyond either
 *   is PTV_ERR_UNSUPPORTED from every entry point below (neither can happen with 512 CUs or fewer).
 * Refused with PTV_ERR_ARG (-1) before any launch: T <= 0; a NULL table or entry among gi, gi_step, gi_ld, w_hh16, b_hh, hall, hall16,
 *   reverse, xch, sync (BPTT: hall, gates, w_t16, dgi, dgh, reverse, xch, sync; split-K: part too); a stride table missing for a
 *   pointer that is given; gi_ld, gi_step, gi2_ld, gi2_step, ext_ld, ext_step or last_ld not a multiple of 4; a misaligned pointer.
 *   Alignment: 16 bytes for w_hh16, w_t16, b_hh, hall, xch, part, fp32 dh_ext, dh_last and dh0 (float4 / 8 x bf16 accesses), 8 bytes
 *   for gi, gi2, hall16, gates, dgi, dgh and bf16 dh_ext (4 x bf16), 4 bytes for lengths and sync.
 *   NC outside 1 .. 4, M <= 0, H not 256 / 512 / 768 / 1024 and (split-K) S not 2 or 4 are PTV_ERR_UNSUPPORTED.
 * Optional: gi2 (table or entry NULL; gi2_step = 0 broadcasts one [M][3H] addend), gates (table NULL: none saved), lengths, dh_ext,
 *   dh_last, dh0.  dh0 may be given for some chains of a launch and be NULL for others: a chain's step count and its row groups'
 *   counters are its own.  A row whose step is dead (t >= lengths[row]) copies its state and saves the gates (0, 1, 0, hn).
 */
int ptv_gru_persist_supported(int NC, int M, int H);
/* CUs the persistent grids leave free (default 0 = size to every CU): a data-parallel run may set it so that RCCL's channel kernels
 * always find a CU without a 96-KB workgroup on it (dist.GradSync, PTV_PERSIST_CU_RESERVE); the grids are sized from CUs - reserve */
int ptv_gru_persist_cu_reserve(int cus);
/* how consumers read the exchanged operand: 0 = sc1 loads, 1 = nt loads, 2 = plain loads behind one agent acquire per step */
int ptv_gru_persist_load_policy(int lp);
int ptv_gru_persist_fwd(int NC, int M, int H, int T,
                        const void* const* gi, const long* gi_step, const long* gi_ld,
                        const void* const* gi2, const long* gi2_step, const long* gi2_ld,
                        const void* const* w_hh16, const float* const* b_hh,
                        float* const* hall, void* const* hall16, void* const* gates,
                        const int* const* lengths, const int* reverse, void* const* xch, unsigned* sync, void* stream);
int ptv_gru_persist_bwd(int NC, int M, int H, int T,
                        const float* const* hall, const void* const* gates, const void* const* w_t16,
                        const void* const* dh_ext, const long* ext_step, const long* ext_ld, const int* ext_bf16,
                        const float* const* dh_last, const long* last_ld,
                        void* const* dgi, void* const* dgh, float* const* dh0,
                        const int* reverse, void* const* xch, unsigned* sync, void* stream);
/* The BPTT with split-K TEAMS (round 4): S = 2 or 4 consecutive workgroups share 16*S hidden units and split K = 3H, so a workgroup
 * reads 1/S of the exchanged operand per step (the classic kernel is bound by exactly that read: 64 unit groups x M x 3H bf16 per
 * step); the team adds its fp32 partial tiles in a fixed order (bit-reproducible).  Same arguments and results as
 * ptv_gru_persist_bwd (summation order differs) plus
 *   part: per chain ptv_gru_persist_part_elems(NC, M, H, S) floats of scratch (partial tiles, ring of two steps),
 *   sync: 16 * (1 + 32 + 128) ZEROED words (row-group counters as above, then one counter per team from word 16*33 on).
 * Up to 512 rows per workgroup: the four chains of two bi-GRUs at M = 512, H = 1024 fit ONE launch. */
int ptv_gru_persist_splitk_supported(int NC, int M, int H, int S);
long ptv_gru_persist_part_elems(int NC, int M, int H, int S);
int ptv_gru_persist_bwd_splitk(int S, int NC, int M, int H, int T,
                               const float* const* hall, const void* const* gates, const void* const* w_t16,
                               const void* const* dh_ext, const long* ext_step, const long* ext_ld, const int* ext_bf16,
                               const float* const* dh_last, const long* last_ld,
                               void* const* dgi, void* const* dgh, float* const* dh0,
                               const int* reverse, void* const* xch, float* const* part, unsigned* sync, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming helpers (layout shuffles and reductions that torch would do with cat/transpose/sum).
 */
/* dst[r*ldd + c] = (accumulate ? dst : 0) + alpha*src[r*lds + c]   (lds = 0 broadcasts one row) */
int ptv_copy2d(float* dst, long ldd, const float* src, long lds, long rows, int cols, float alpha,
               int accumulate, void* stream);
/* [D0,D1,W] -> [D1,D0,W]  (batch-major API tensors <-> step-major internal layout) */
int ptv_transpose01(float* dst, const float* src, int D0, int D1, int W, void* stream);
/* out[i] = (accumulate ? out[i] : 0) + sum_t in[t*stride + i] */
int ptv_sum_steps(float* out, const void* in, long n, int T, long stride, int accumulate, int in_bf16, void* stream);
/* the same over the planes 0 .. *t_top only (device int; the later planes are known to be zero, see ptv_notes_gru_persist_bwd) */
/* *top = max(*top, index of the `unit`-row block that holds the LAST ROW of the last 64-row chunk of x [rows, cols] (fp32, row stride ld)
 * with a non-zero in it): which trailing note steps of a gradient received nothing (the loss ignores padded slots) -- the limit handed to
 * ptv_gemm_mtop / ptv_wgrad.  The scan goes by 64-row chunks, so this is the block of the last non-zero row when unit is a multiple of
 * 64 and an upper bound of it otherwise; -0.0 counts as zero, NaN as non-zero.  Rows whose padding columns cols .. ld - 1 are not zero
 * may raise it further (whole chunks are read as one span when they are 16-byte aligned). */
/* process-wide switch (default 1): the backward kernels pass over work whose result is exactly zero -- note steps / tiles at which no
 * gradient arrives (tested on the arriving gradient), panel steps beyond the longest packed sequence.  0 = run everything dense. */
int ptv_zero_skip(int enable);
int ptv_last_nonzero_unit(const float* x, long rows, int cols, long ld, long unit, int* top, void* stream);
int ptv_sum_steps_top(float* out, const void* in, long n, int T, long stride, int accumulate, int in_bf16, const int* t_top,
                      void* stream);
/* ... and with ROW SEGMENTS (round 6; seg_n or NULL): the planes are note steps over length-sorted rows of row_elems elements each, plane t holds
 * something in its first seg_n[t] rows only (device ints, not growing with t: ptv_rows_seg_counts) -- the rest is zero and is not read */
int ptv_sum_steps_seg(float* out, const void* in, long n, int T, long stride, int accumulate, int in_bf16, const int* t_top,
                      const int* seg_n, long row_elems, void* stream);
/* out[g*N + n] += sum over rows r with (sel ? sel[r] : 0) == g of A[r*lda + n]   (bias gradients;
 * with sel: the duration GRU's W_ih gradient, whose inputs are one-hot tokens) */
int ptv_colsum(float* out, const void* A, long lda, long rows, int N, const int* sel, int G, int a_bf16, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Note embedding as a gather: PtvaeDecoder.emb_x (ptvae.py:531-535) = get_len_index_tensor
 * (ptvae.py:292-297) + index_tensor_to_multihot_tensor (ptvae.py:299-313) + note_embedding Linear.
 *   x [B,32,16,6] int64 -> emb STEP-MAJOR [16][32][B][E], lengths [32][B] int32 (lengths may be NULL)
 * bwd: ptv_multihot materialises the [16*32*B, 135] multi-hot matrix (same row order, row stride ld) so
 *      that dW[E,135] = demb^T . multihot runs as a split-K ptv_gemm; dbias = ptv_colsum(demb).
 */
int ptv_embed_fwd(const long* x, const float* W, const float* bias, float* emb, int* lengths, int B, int E, void* stream);
int ptv_multihot(const long* x, float* out, long ld, int B, void* stream);
/* get_len_index_tensor alone (ptvae.py:292-297): lengths [32][B] int32 = 16 - number of <pad> pitches of each (step, sample) */
int ptv_grid_lengths(const long* x, int* lengths, int B, void* stream);
/* the same rows as bf16 (exact), ld >= 136 with column 135 zeroed: operand of the bf16-precision note_embedding weight gradient */
int ptv_multihot_bf16(const long* x, void* out, long ld, int B, void* stream);
/* The same three for ANY grid geometry the reference's constructors accept (ptvae.py:127-147 PtvaeEncoder, :220-241 PtvaeDecoder):
 * S = num_step, N = max_simu_note, P = pitch_range = max_pitch - min_pitch + 3, D = dur_width (<= 8), pad = pitch_pad.
 *   x [B,S,N,1+D] int64 -> emb step-major [N][S][B][E], lengths [S][B], multihot rows [N*S*B][P+D] (bf16 != 0: bf16 rows zero-filled to
 *   the 8-column granule, ld >= that).  A pitch index outside [0, P) contributes no pitch column (the reference drops column P, the
 *   <pad> column: ptvae.py:186,311).  train.py:32 constructs PtvaeEncoder(max_pitch=31): P = 34. */
int ptv_embed_fwd_geom(const long* x, const float* W, const float* bias, float* emb, int* lengths, int B, int E,
                       int S, int N, int P, int D, int pad, void* stream);
int ptv_grid_lengths_geom(const long* x, int* lengths, int B, int S, int N, int D, int pad, void* stream);
int ptv_multihot_geom(const long* x, void* out, long ld, int B, int S, int N, int P, int D, int bf16, void* stream);
/* Note embedding of a BYTE multi-hot grid: the input of the texture encoder train.py:32 builds, the detrended PianoTree grid dt_x of
 * ptv_detrend_pianotree (K = 39: 34 class columns of 0/1, 5 duration columns of 0/1/2; a row holds at most 10 non-zero bytes).
 *   mh [B,S,N,K] uint8 (any values), W [E,K], bias [E] -> emb step-major [N][S][B][E] fp32 (the layout of ptv_embed_fwd_geom):
 *   emb[n][s][b][:] = bias + sum_k mh[b,s,n,k] * W[:,k]; zero bytes are skipped, the other terms added in ascending k -- a pure function
 *   of the inputs (bit-reproducible); an all-zero row gives bias.
 *   lengths [S][B] int32 (or NULL) = number of rows n with mh[b,s,n,pad_col] == 0; for dt_x pad_col = 3, the is_note class of the <pad>
 *   pitch, which makes it get_len_index_tensor (ptvae.py:167-172) of the grid the dt_x came from.  pad_col < 0: no lengths wanted.
 * One launch: W is staged transposed in LDS, a tile is one step and 8 samples, a row's E floats leave as 16-byte stores.
 * PTV_ERR_ARG before any launch for: a NULL mh / W / bias / emb, B, S, N or K <= 0, K > 64, E > 256 or not a multiple of 4, K*E*4 > 150 KB,
 * N*K > 16384, pad_col >= K, lengths without a pad_col >= 0, emb not 16-byte aligned (mh may sit anywhere). */
int ptv_embed_multihot_fwd(const unsigned char* mh, const float* W, const float* bias, float* emb, int* lengths,
                           int B, int E, int S, int N, int K, int pad_col, void* stream);
/* the same bytes widened (0 / 1 / 2 are exact in both types): out [N*S*B][ld] fp32 (bf16 != 0: bf16) in the step-major row order of emb,
 * ld >= K, columns K .. ld-1 zeroed -- what ptv_multihot_geom is to the index grid: the operand of grad_W = demb^T . rows(mh) */
int ptv_multihot_bytes_rows(const unsigned char* mh, void* out, long ld, int B, int S, int N, int K, int bf16, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TextureEncoder front end (ptvae.py:95-99,112-114): Conv2d(1,C,(4,12),stride(4,1)) + ReLU +
 * MaxPool2d((1,4)) fused; pr_mat [B,32,128] -> pooled [B,C,8,29].  bwd recomputes the conv and
 * accumulates dW[C,48], dbias[C] (pr_mat is an input: no dX).
 */
int ptv_txt_conv_relu_pool_fwd(const float* pr_mat, const float* w, const float* bias, float* pooled, int B, int C, void* stream);
int ptv_txt_conv_relu_pool_bwd(const float* pr_mat, const float* w, const float* bias, const float* dpooled,
                               float* dw, float* dbias, int B, int C, void* stream);
/* the same with the pooled map held as the rows of the reference's raw view (ptvae.py:114): feat [B*8][ld], ld >= C*29 -- element
 * (b, ch, beat, pp) at row b*8 + f / (C*29), column f % (C*29), f = (ch*8 + beat)*29 + pp.  A 16-byte-multiple ld keeps the rows of fc1's
 * operand aligned for the MFMA loaders; ld = C*29 is the plain tensor of the entry points above. */
int ptv_txt_conv_relu_pool_fwd_rows(const float* pr_mat, const float* w, const float* bias, float* feat, long ld, int B, int C,
                                    signed char* arg, void* stream);
/* arg (may be NULL): int8 [B*8][C*29], written by the forward -- which of the 4 pooled positions won (-1: ReLU cut all four).  Given to the
 * backward, the convolution is not recomputed (w / bias may then be NULL): same decisions, same gradients, a fifth of the arithmetic
 * (this kernel is the LAST launch of the backward pass's longest chain) */
int ptv_txt_conv_relu_pool_bwd_rows(const float* pr_mat, const float* w, const float* bias, const float* dfeat, long ld,
                                    float* dw, float* dbias, int B, int C, const signed char* arg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * reparameterize(): get_zs_from_dists / Normal.rsample (amc_dl/torch_plus/train_utils.py:33-34)
 *   z[b*ldz + j] = mu + sd*eps (eps NULL -> z = mu); kl_sum += sum(-log sd + (sd^2+mu^2)/2 - 1/2)
 *   kl_sum NULL: z alone, from a kernel that computes no KL and reduces nothing (the same z bits)
 * bwd: dmu = dz + klw*mu + dmu_ext ; dsd = dz*eps + klw*(sd - 1/sd) + dsd_ext ; dlv = dsd*sd
 *      (lv = log sd is the linear_var output, ptvae.py:27,120); any of dz/eps/ext may be NULL;
 *      mul_sd = 0 returns dsd itself in `dlv`.
 */
/* eps for the reparameterisation as a pure function of (seed, stream_id, GLOBAL sample index row_offset + r, column):
 * Philox4x32-10 + Box-Muller.  The same batch gives the same noise however it is sharded over ranks (SURVEY.md 8 d/e). */
int ptv_philox_normal(float* out, long rows, int Z, unsigned long long seed, unsigned long long stream_id, long row_offset,
                      void* stream);
int ptv_reparam_kl_fwd(const float* mu, const float* sd, const float* eps, float* z, long ldz, float* kl_sum, int B, int Z, void* stream);
int ptv_reparam_kl_bwd(const float* mu, const float* sd, const float* eps, const float* dz, long lddz,
                       const float* dmu_ext, const float* dsd_ext, float klw, int mul_sd, float* dmu, float* dlv, int B, int Z, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Losses: DisentangleVAE.loss_function (model.py:57-68), PtvaeDecoder.recon_loss (ptvae.py:498-511),
 * chord_loss (model.py:70-83), kl_loss (model.py:85-90) + kl_with_normal (train_utils.py:45-49).
 *   targets: int32 arrays in the row order of the logits (step_major = 1: [15][32][B], else [B][32][15];
 *            chord: [8][B] or [B][8]); counts[0/1] += number of non-ignored pitch / duration targets; counts[2] (three zero-initialised
 *            ints) = max(counts[2], last note step 0..14 that holds any non-ignored target): an upper bound of where the logits' gradient
 *            can be non-zero, the decoder backward's zero-skip limit (round 4; replaces two scans of the 134-MB gradient)
 *   ptv_ce_fwd: nll_sum += sum over non-ignored rows of -log softmax(logits)[target]
 *   ptv_ce_bwd: dlogits = gscale[0] * (softmax - onehot), 0 on ignored rows (gscale is a DEVICE scalar)
 *   ptv_loss_finalize: 7 sums + 2 counts -> the 11 scalars in train.py:54-55 order
 *   ptv_loss_bwd_scales: upstream grads of the 11 scalars -> 7 per-component scale factors (device)
 */
int ptv_pianotree_targets(const long* x, int B, int step_major, int* pitch_t, int* dur_t, int* counts, void* stream);
/* the same + row_live (int32 [32 B], ZEROED by the caller, or NULL): row (t, b)'s number of live note steps = 1 + the last note step at
 * which it holds a target (what the teacher-forced decoder needs of that row when only the loss consumes it) */
int ptv_pianotree_targets_rows(const long* x, int B, int step_major, int* pitch_t, int* dur_t, int* counts, int* row_live, void* stream);
/* rows by index, `planes` planes of `rows` rows of row_words 4-byte words: gather dst[pl][p] = src[pl][idx[p]], scatter dst[pl][idx[p]] =
 * src[pl][p] (plane strides in words).  The decoder's rows in length-sorted order and back. */
int ptv_gather_rows(void* dst, const void* src, const int* idx, long rows, int row_words, long src_plane_words, long dst_plane_words, int planes,
                    void* stream);
int ptv_scatter_rows(void* dst, const void* src, const int* idx, long rows, int row_words, long src_plane_words, long dst_plane_words, int planes,
                     void* stream);
/* ... with ROW SEGMENTS (round 6; seg_n int32 [planes] or NULL = the calls above): of plane q only the first seg_n[q] rows IN SORTED ORDER hold
 * anything (ptv_rows_seg_counts).  The gather leaves the other rows of dst unwritten (its readers clip to the same segments); the scatter
 * writes zeros to their places in dst without reading src. */
int ptv_gather_rows_seg(void* dst, const void* src, const int* idx, long rows, int row_words, long src_plane_words, long dst_plane_words,
                        int planes, const int* seg_n, void* stream);
int ptv_scatter_rows_seg(void* dst, const void* src, const int* idx, long rows, int row_words, long src_plane_words, long dst_plane_words,
                         int planes, const int* seg_n, void* stream);
int ptv_chord_targets(const float* c, int B, int step_major, int* root_t, int* chroma_t, int* bass_t, void* stream);
int ptv_ce_fwd(const float* logits, long ld, const int* targets, long rows, int C, int ignore_index, float* nll_sum, void* stream);
int ptv_ce_bwd(const float* logits, long ld, const int* targets, long rows, int C, int ignore_index, const float* gscale,
               float* dlogits, long ldd, void* stream);
/* weighted duration loss (recon_loss(..., weighted_dur=True), ptvae.py:512-527): the 5 duration bit positions are 5 separate
 * CrossEntropyLoss(ignore_index = 2) means combined with weights (1, .6, .4, .3, .3).  Row r of the [rows*5, 2] logits
 * belongs to group r % G: per-group nll sums / valid counts (fwd), per-group gradient scales (bwd).
 * ptv_wdur_finalize folds them into (sums1 = dl, counts1 = 1) so ptv_loss_finalize / ptv_loss_bwd_scales apply unchanged;
 * ptv_wdur_scales turns the upstream scale of dl into the 5 per-group scales gs1 * w[d] / cnt[d]. */
int ptv_ce_group_fwd(const float* logits, long ld, const int* targets, long rows, int C, int ignore_index, int G,
                     float* nll_sum, int* count, void* stream);
int ptv_ce_group_bwd(const float* logits, long ld, const int* targets, long rows, int C, int ignore_index, int G,
                     const float* gscale, float* dlogits, long ldd, void* stream);
int ptv_wdur_finalize(const float* gsum5, const int* gcnt5, float w0, float w1, float w2, float w3, float w4, float* sums1,
                      int* counts1, void* stream);
int ptv_wdur_scales(const float* gs1, const int* gcnt5, float w0, float w1, float w2, float w3, float w4, float* out5,
                    void* stream);
int ptv_kl_fwd(const float* mu, const float* sd, long n, float* kl_sum, void* stream);
int ptv_kl_bwd(const float* mu, const float* sd, long n, const float* gscale, float* dmu, float* dsd, void* stream);
int ptv_loss_finalize(const float* sums, const int* counts, float beta, float w0, float w1, float n_kl, float n_root,
                      float n_chroma, float* out11, void* stream);
int ptv_loss_bwd_scales(const float* gout11, const int* counts, float beta, float w0, float w1, float n_kl, float n_root,
                        float n_chroma, float* gs7, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Duration head (ptvae.py:361-367): dur_out[r*ld_out + 0..1] = dur_out_linear(h[r]); idx[r] = argmax
 * (force_idx, if given, overrides the argmax where its entry is >= 0: replay mode for parity checks, kept steps).
 */
int ptv_dur_out_token(const float* h, int H, const float* w_out, const float* b_out, float* dur_out, long ld_out,
                      int* idx, const int* force_idx, long rows, void* stream);
/* weight gradient of dur_out_linear (autograd of ptvae.py:361-362 over the 5 duration steps) in one pass over the bf16 state
 * planes: gw[c*64 + u] += sum_d sum_m ddur[m*ld_dd + 2d + c] * hall16[(d+1)*plane_h + m*64 + u]   (H = 64) */
int ptv_dur_out_wgrad(const float* ddur, long ld_dd, const void* hall16, long plane_h, float* gw, long rows, int H, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The whole 5-step duration GRU of decode_note (ptvae.py:353-367) in ONE kernel (bf16 precision, H = 64):
 * W_hh and the 3-row gate table stay in LDS, the state in registers, each wave owns 16 rows for all 5
 * steps; est_dur and the argmax feedback are computed in the same kernel.  Returns PTV_ERR_ARG for other
 * H (callers then use ptv_gru_step_fwd + ptv_dur_out_token per step).
 *   hall / hall16: state after step d at base + d*plane_h + row*64 (either may be NULL)
 *   gates: plane p of step d at base + d*step_g + p*plane_g + row*64 (NULL = inference)
 *   dur_out[row*ld_out + 2d..2d+1], idx[d*idx_stride + row]; force (replay) may be NULL
 */
int ptv_dur_gru_fwd(int H, long M, const float* h0, long ld_h0, const float* w_hh, const float* b_hh,
                    const float* tab0, const float* tab, const float* w_out, const float* b_out,
                    float* hall, long plane_h, void* hall16, void* gates, long plane_g, long step_g, int gates_bf16,
                    float* dur_out, long ld_out, int* idx, long idx_stride, const int* force, long force_stride,
                    void* stream);
/* the same with a LIVE-ROW LIMIT: m_top (device int32, or NULL = all rows) and m_unit (a multiple of 16) -- only the rows below
 * (*m_top + 1) * m_unit are computed; the other rows of hall / hall16 / gates / dur_out / idx stay unwritten.  For callers whose loss
 * ignores the padded note slots (ptvae.py:498-511): rows are ordered [note step][32 B], m_unit = 32 B, *m_top = the last note step with a
 * target. */
int ptv_dur_gru_fwd_top(int H, long M, const float* h0, long ld_h0, const float* w_hh, const float* b_hh,
                        const float* tab0, const float* tab, const float* w_out, const float* b_out,
                        float* hall, long plane_h, void* hall16, void* gates, long plane_g, long step_g, int gates_bf16,
                        float* dur_out, long ld_out, int* idx, long idx_stride, const int* force, long force_stride,
                        const int* m_top, long m_unit, void* stream);
/* ... and with the rows of every note step sorted by descending length (row_len int32 [m_unit]): 16-row tiles whose first row has no target
 * at their note step are passed over (outputs unwritten) */
int ptv_dur_gru_fwd_rows(int H, long M, const float* h0, long ld_h0, const float* w_hh, const float* b_hh,
                         const float* tab0, const float* tab, const float* w_out, const float* b_out,
                         float* hall, long plane_h, void* hall16, void* gates, long plane_g, long step_g, int gates_bf16,
                         float* dur_out, long ld_out, int* idx, long idx_stride, const int* force, long force_stride,
                         const int* m_top, long m_unit, const int* row_len, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the 5-step duration GRU (autograd of ptvae.py:353-367) in ONE kernel (bf16 gates, H = 64): dh
 * stays in registers over the 5 steps, dgh_d . W_hh runs against W_hh^T resident in LDS, and the parameter
 * gradients are accumulated in-kernel from LDS-transposed row tiles.  Writes dh0 [M,64] (gradient reaching
 * dur_hid_linear's output) and one [256 x 80] fp32 partial per block into part[nblocks][ptv_dur_gru_bwd_part_size()]:
 *   rows 0..191 = (dr, dz, dn*r) gate units, rows 192..255 = dn;  columns 0..63 = . h_d (dW_hh),
 *   columns 64..66 = sums over the rows whose step input was <sos> / one-hot token 0 / token 1.
 * ptv_dur_bwd_finalize folds the column-summed partial S [256 x 80] into the gradients of weight_hh, bias_hh,
 * bias_ih, weight_ih [192, I] and the <sos> token [I] (all +=).
 *   gates/hall as written by ptv_dur_gru_fwd (hall: the fp32 states or, h_bf16 = 1, their bf16 copies hall16); ddur [M, 10] = d loss / d est_dur; idx[d*idx_stride + row].
 *   gates == NULL: RECOMPUTE mode -- the forward was called with gates = NULL (it then writes a third of the bytes) and the backward
 *   rebuilds r, z, n, hn of each step from h_{d-1}, W_hh, b_hh and the gate tables tab0 / tab the forward was given (the forward's own
 *   MFMA product and fp32 expressions, hence the forward's values); otherwise b_hh / tab0 / tab may be NULL.
 */
int ptv_dur_gru_bwd_part_size(void);
int ptv_dur_gru_bwd(int H, long M, const void* gates, long plane_g, long step_g, const void* hall, long plane_h, int h_bf16,
                    const float* ddur, long ld_dd, const float* w_hh, const float* w_out,
                    const int* idx, long idx_stride, float* dh0, float* part, int nblocks,
                    const float* b_hh, const float* tab0, const float* tab, void* stream);
int ptv_dur_bwd_finalize(const float* S, float* g_whh, float* g_bhh, float* g_bih, float* g_wih, float* g_sos,
                         const float* w_ih, const float* sos, int I, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The per-note heads fused (csrc/heads.hip, bf16 precision, init_model() geometry Hn = 512 / 130 classes / Hd = 64): one pass over the
 * note summaries for decode_note's two Linears (ptvae.py:343-352) and one for their input gradients.
 *   fwd: pitch [M][ldp] = hn16 . W_p^T + b_p (fp32);  hd0 [M][64] = hn16 . W_dh[:, :512]^T + pitch . W_dh[:, 512:]^T + b_dh
 *        (+ bf16 copy hd16, may be NULL).  wp / wdh / wdp: ptv_pack_mfma_b of W_p [130,512], W_dh[:, :512] [64,512], W_dh[:, 512:] [64,130].
 *   bwd: dp [M][ldp] += dhd0 . W_dh[:, 512:] (in place);  dnsum [M][512] bf16 = dp . W_p + dhd0 . W_dh[:, :512], row-major or
 *        (blocked != 0) column-blocked by 32 ([16][M][32], what ptv_notes_gru_persist_bwd reads).  wdpT: pack of W_dh[:, 512:]^T
 *        [130,64];  wcat: PAIR-interleaved pack of the [512][224] matrix [W_p^T (130 columns, zero-padded to 160) | W_dh[:, :512]^T].
 *        Rows from (*m_top + 1) * m_unit on (device int, or NULL) are known to be zero: their dnsum is written as zeros -- or, with bit 1 of
 *        `blocked` set (blocked = 3), left unwritten: the consumer is ptv_notes_gru_persist_bwd_top with the same limit as its bound.
 *        dy16 (or NULL): [M][200] bf16 = [dp (130) | 0 (6) | dhd0 (64)] of the live rows -- ONE ptv_wgrad operand for the weight gradients
 *        of both Linears over the note summaries (one pass over the [M][512] summaries instead of two).
 *   The logits and dp as operands of the second products (130 columns in k-blocks of 32: 160) have their columns 130 .. 159 zeroed by the
 *        kernels themselves, whatever the packs hold beyond their N and K: the staging memory there holds stale bits.
 *   Alignment (checked on the host before the launch, PTV_ERR_ARG otherwise -- the kernels make float4 / bf16x8 accesses): 16 bytes for
 *        hn16, pitch, dp (ldp a multiple of 4), b_dh, hd0, dhd0, dnsum16, dy16 and every pack; 8 bytes for hd16.  b_p is read by element.
 */
int ptv_heads_fwd(const void* hn16, const void* wp_packed, const void* wdh_packed, const void* wdp_packed, const float* b_p,
                  const float* b_dh, float* pitch, long ldp, float* hd0, void* hd16, long M, void* stream);
/* the same with the live-row limit of ptv_dur_gru_fwd_top (m_unit a multiple of 128): later rows of pitch / hd0 / hd16 stay unwritten */
int ptv_heads_fwd_top(const void* hn16, const void* wp_packed, const void* wdh_packed, const void* wdp_packed, const float* b_p,
                      const float* b_dh, float* pitch, long ldp, float* hd0, void* hd16, long M, const int* m_top, long m_unit,
                      void* stream);
int ptv_heads_bwd(float* dp, long ldp, const float* dhd0, const void* wdpT_packed, const void* wcat_packed, void* dnsum16,
                  int blocked, void* dy16, const int* m_top, long m_unit, long M, void* stream);
/* ... with the rows of every note step sorted by descending length (row_len int32 [m_unit], needs m_top): 128-row blocks whose first row
 * has no target at their note step are passed over -- forward: their logits are written as zeros (finite operands of a weight-gradient
 * product), hd0 / hd16 stay unwritten; backward: their dy16 rows are zeros, their dnsum rows unwritten */
int ptv_heads_fwd_rows(const void* hn16, const void* wp_packed, const void* wdh_packed, const void* wdp_packed, const float* b_p,
                       const float* b_dh, float* pitch, long ldp, float* hd0, void* hd16, long M, const int* m_top, long m_unit,
                       const int* row_len, void* stream);
int ptv_heads_bwd_rows(float* dp, long ldp, const float* dhd0, const void* wdpT_packed, const void* wcat_packed, void* dnsum16,
                       int blocked, void* dy16, const int* m_top, long m_unit, const int* row_len, long M, void* stream);

/* ------------------------------------------------------------------------------------------------
 * COMPOSITE: PtvaeDecoder.decoder, teacher-forced, FORWARD -- ptvae.py:430-496 with decode_notes (:370-428) and decode_note (:336-368)
 * restructured to 32 + 15 + 5 sequential steps -- behind one call: the 15 launches, the persistent launch's turn (event wait /
 * record) and every shape decision are C++ host code (csrc/composite.hip); the caller owns the tensors and hands them over as one
 * pointer table t[PTV_DTF_COUNT] and one dimension table d[PTV_DTF_D_COUNT].  bf16 precision at the init_model() sizes only
 * (E = 128, Hn = 512, Hd = 64, 130 pitch classes, Ht with a persistent plan): ptv_decoder_tf_supported(d) == 0 / PTV_ERR_UNSUPPORTED
 * otherwise, before anything is launched -- the caller then sequences the entry points above itself.
 *   rows: R = 32*B (time step, sample), M = 15*R (note, time step, sample).  Layouts as documented at the entry points it calls.
 */
enum PtvDtfTensor {
  /* inputs */
  PTV_DTF_Z = 0,          /* [B, Zs] fp32 */
  PTV_DTF_EMB,            /* [16, R, E] fp32: the embedded ground-truth notes, step-major (ptv_embed_fwd) */
  PTV_DTF_XS,             /* [R, 2He] fp32: ground-truth note summaries (ptvae.py:446-453) */
  PTV_DTF_FORCE_DUR,      /* [5, M] int32 or NULL: replayed duration decisions (tests) */
  /* fp32 parameters */
  PTV_DTF_B_ZHID, PTV_DTF_B_ZIN, PTV_DTF_INIT_INPUT, PTV_DTF_B_IH_T, PTV_DTF_B_HH_T, PTV_DTF_B_T2N, PTV_DTF_B_IH_N, PTV_DTF_B_HH_N,
  PTV_DTF_B_P, PTV_DTF_B_DH, PTV_DTF_W_HH_D, PTV_DTF_B_HH_D, PTV_DTF_W_IH_D, PTV_DTF_B_IH_D, PTV_DTF_SOS,
  PTV_DTF_ONEHOT,         /* [2, 5] fp32 constant: rows onehot(0), onehot(1) */
  PTV_DTF_W_OUT_D, PTV_DTF_B_OUT_D,
  /* bf16 operand copies of the weights, [out, in] row-major */
  PTV_DTF_W16_ZHID, PTV_DTF_W16_ZIN, PTV_DTF_W16_IH_T, PTV_DTF_W16_HH_T, PTV_DTF_W16_T2N, PTV_DTF_W16_IH_N,
  /* MFMA-fragment packs (ptv_pack_mfma_multi): notes GRU W_hh / token part of W_ih; pitch_out, dur_hid[:, :Hn], dur_hid[:, Hn:] */
  PTV_DTF_PK_NOTES_H, PTV_DTF_PK_NOTES_T, PTV_DTF_PK_WP, PTV_DTF_PK_WDH, PTV_DTF_PK_WDP,
  /* outputs and what the backward keeps */
  PTV_DTF_NS,             /* [33, B, Ht] fp32 time states (slot 0 = z2dec_hid(z)) */
  PTV_DTF_NS16,           /* the same, bf16 */
  PTV_DTF_Z_IN,           /* [B, Zi] fp32 */
  PTV_DTF_TOKS,           /* [33, B, 2He] fp32 time-step tokens */
  PTV_DTF_GI_T,           /* [R, 3Ht] bf16 */
  PTV_DTF_ZG,             /* [B, 3Ht] bf16 */
  PTV_DTF_GATES_T,        /* [32, 4, B, Ht] bf16 */
  PTV_DTF_HN,             /* [16, R, Hn] fp32 note states */
  PTV_DTF_HN16,           /* the same, bf16 */
  PTV_DTF_GC,             /* [R, 3Hn] bf16, column-blocked by 32 */
  PTV_DTF_GATES_N,        /* [15, 4, R, Hn] bf16 */
  PTV_DTF_PITCH,          /* [M, ldp] fp32 pitch logits (130 used) */
  PTV_DTF_HD,             /* [6, M, Hd] fp32 (slot 0 written) */
  PTV_DTF_HD16,           /* [6, M, Hd] bf16 */
  PTV_DTF_TAB0, PTV_DTF_TAB,    /* [1, 3Hd], [2, 3Hd] fp32 gate tables of the duration GRU */
  PTV_DTF_GATES_D,        /* [5, 4, M, Hd] bf16, or NULL (the backward then recomputes them: ptv_dur_gru_bwd) */
  PTV_DTF_DUR,            /* [M, 10] fp32 duration logits */
  PTV_DTF_IDX,            /* [5, M] int32 duration decisions */
  /* workspaces and the persistent launch's turn */
  PTV_DTF_XCH,            /* 33*B*Ht bf16 exchange buffer of ptv_gru_persist_fwd */
  PTV_DTF_SYNC,           /* its zeroed sync words */
  PTV_DTF_WAIT_EVENT,     /* hipEvent_t recorded after the previous persistent launch of the process, or NULL */
  PTV_DTF_RECORD_EVENT,   /* hipEvent_t to record after this one, or NULL */
  PTV_DTF_LIVE_TOP,       /* device int32 or NULL: the caller uses the outputs of the note steps 0 .. *LIVE_TOP only (a loss that ignores the
                           * padded note slots, ptvae.py:498-511): the notes GRU, the heads and the duration GRU leave the later steps' rows of
                           * HN16 / GATES_N / PITCH / HD / HD16 / GATES_D / DUR / IDX unwritten */
  /* rows sorted by length (round 6: per-row dead work; all four or none).  With them the notes GRU, the heads and the duration GRU work on
   * the decoder's rows in the order PERM -- row p of their tensors is row PERM[p] of the time states / tokens -- and pass over the
   * (note step, 64-row panel) pairs whose longest row has no target there; the loss must be given its targets in the same order. */
  PTV_DTF_PERM,           /* int32 [R]: rows by descending ROW_LEN (ptv_rows_by_length), or NULL */
  PTV_DTF_ROW_LEN,        /* int32 [R]: live note steps of the row at position p (ptv_pianotree_targets_rows, gathered by PERM) */
  PTV_DTF_NS16S,          /* out [R, Ht] bf16: the time states NS16[1:] gathered by PERM (operand of the hoisted products, kept for the backward) */
  PTV_DTF_TOK_S,          /* out [15, R, E] fp32: the fed tokens EMB[:15] gathered by PERM */
  PTV_DTF_SEG_N,          /* int32 [15] (ptv_rows_seg_counts) or NULL, sorted mode only: TOK_S is gathered for the live blocks of every note step only -- the
                             backward must then be given PTV_DTB_SEG_N (its products never read the other rows) */
  PTV_DTF_COUNT
};
enum PtvDtfDim { PTV_DTF_D_B = 0, PTV_DTF_D_E, PTV_DTF_D_HE, PTV_DTF_D_HT, PTV_DTF_D_HN, PTV_DTF_D_HD, PTV_DTF_D_NP, PTV_DTF_D_ZS, PTV_DTF_D_ZI,
                 PTV_DTF_D_LDP, PTV_DTF_D_COUNT };
int ptv_decoder_tf_supported(const long* d);
int ptv_decoder_tf_fwd(const void* const* t, const long* d, void* stream);

/* COMPOSITE: RnnDecoder.forward, teacher-forced (ptvae.py:51-87 with tfr = 1), FORWARD in one call: z -> h0 / z_in, the tokens
 * [init ; c_0 .. c_{T-2}], the hoisted input product, the T-step GRU, the three heads.  Any sizes; d[PTV_CDF_D_PREC] = 0 (fp32) / 1 (bf16
 * MFMA operands, fp32 masters converted per tile); all tensors fp32 except GATES when d[PTV_CDF_D_GATES_BF16]. */
enum PtvCdfTensor {
  PTV_CDF_Z = 0,          /* [B, Z] */
  PTV_CDF_C_SM,           /* [T, B, I] the chord steps, step-major */
  PTV_CDF_W_ZHID, PTV_CDF_B_ZHID, PTV_CDF_W_ZIN, PTV_CDF_B_ZIN, PTV_CDF_INIT_INPUT,
  PTV_CDF_W_IH,           /* [3H, I + Zi] */
  PTV_CDF_B_IH, PTV_CDF_W_HH, PTV_CDF_B_HH, PTV_CDF_W_ROOT, PTV_CDF_B_ROOT, PTV_CDF_W_CHROMA, PTV_CDF_B_CHROMA, PTV_CDF_W_BASS, PTV_CDF_B_BASS,
  PTV_CDF_HALL,           /* out [T+1, B, H] states (slot 0 = z2dec_hid(z)) */
  PTV_CDF_Z_IN,           /* out [B, Zi] */
  PTV_CDF_TOKS,           /* out [T, B, I] */
  PTV_CDF_GI,             /* out [T*B, 3H] */
  PTV_CDF_ZG,             /* out [B, 3H] */
  PTV_CDF_GATES,          /* out [T, 4, B, H] fp32 or bf16 */
  PTV_CDF_ROOT, PTV_CDF_CHROMA, PTV_CDF_BASS,   /* out [T*B, 12 / 24 / 12] logits */
  PTV_CDF_COUNT
};
enum PtvCdfDim { PTV_CDF_D_B = 0, PTV_CDF_D_T, PTV_CDF_D_H, PTV_CDF_D_I, PTV_CDF_D_Z, PTV_CDF_D_ZI, PTV_CDF_D_PREC, PTV_CDF_D_GATES_BF16,
                 PTV_CDF_D_NROOT, PTV_CDF_D_NCHROMA, PTV_CDF_D_NBASS, PTV_CDF_D_COUNT };
int ptv_chord_decoder_fwd(const void* const* t, const long* d, void* stream);

/* ptv_chord_decoder_bwd: autograd through RnnDecoder.forward, teacher-forced (ptvae.py:51-87) -- what ChordDecoderTFFn.backward sequences:
 * the three heads' input / weight / bias gradients, the GRU's BPTT (one persistent launch with its event turn when d[PTV_CDB_D_PERSIST],
 * S = d[PTV_CDB_D_SPLITK] teams; else the per-step kernels), the weight / bias gradients of the GRU, of the start token and of the two
 * z projections, and dz.  26 launches.  Every G_* slot is the parameter's gradient buffer and is ACCUMULATED into (the caller zeroes it
 * once per step); a NULL D* slot = that head received no gradient.  fp32 tensors except GATES / DGI / DGH (bf16 when d[PTV_CDB_D_ACT_BF16])
 * and WT16 / XCH.  Same arithmetic, launch by launch, as the Python sequencing it replaces (bit-identical results). */
enum PtvCdbTensor {
  PTV_CDB_Z = 0,          /* [B, Z] */
  PTV_CDB_W_ZHID, PTV_CDB_W_ZIN, PTV_CDB_W_IH, PTV_CDB_W_HH, PTV_CDB_W_ROOT, PTV_CDB_W_CHROMA, PTV_CDB_W_BASS,   /* fp32 masters */
  PTV_CDB_WT16_HH,        /* bf16 W_hh^T [H, 3H] (persistent BPTT and the bf16 per-step kernels), or NULL: fp32 W_hh */
  PTV_CDB_HALL, PTV_CDB_GATES, PTV_CDB_TOKS, PTV_CDB_Z_IN,                                 /* saved by the forward */
  PTV_CDB_DROOT, PTV_CDB_DCHROMA, PTV_CDB_DBASS,                                           /* in: [T*B, n] or NULL */
  PTV_CDB_DZ,             /* out [B, Z] */
  PTV_CDB_G_INIT_INPUT, PTV_CDB_G_W_ZHID, PTV_CDB_G_B_ZHID, PTV_CDB_G_W_ZIN, PTV_CDB_G_B_ZIN, PTV_CDB_G_W_IH, PTV_CDB_G_B_IH, PTV_CDB_G_W_HH,
  PTV_CDB_G_B_HH, PTV_CDB_G_W_ROOT, PTV_CDB_G_B_ROOT, PTV_CDB_G_W_CHROMA, PTV_CDB_G_B_CHROMA, PTV_CDB_G_W_BASS, PTV_CDB_G_B_BASS,
  PTV_CDB_DHS,            /* scratch [T*B, H] fp32 */
  PTV_CDB_DGI, PTV_CDB_DGH,      /* scratch [T, B, 3H] */
  PTV_CDB_DHZ,            /* scratch [2, B, H] fp32 (per-step kernels) or NULL */
  PTV_CDB_DH0,            /* scratch [B, H] */
  PTV_CDB_DZG,            /* scratch [B, 3H] fp32 */
  PTV_CDB_DZ_IN,          /* scratch [B, Zi] */
  PTV_CDB_DTOK0,          /* scratch [B, I] */
  PTV_CDB_XCH, PTV_CDB_PART, PTV_CDB_SYNC,   /* persistent launch: exchange buffer T*B*3H bf16, split-K partials or NULL, zeroed sync words */
  PTV_CDB_WAIT_EVENT, PTV_CDB_RECORD_EVENT,  /* hipEvent_t of the previous persistent launch of the process / to record after this one, or NULL */
  PTV_CDB_COUNT
};
enum PtvCdbDim { PTV_CDB_D_B = 0, PTV_CDB_D_T, PTV_CDB_D_H, PTV_CDB_D_I, PTV_CDB_D_Z, PTV_CDB_D_ZI, PTV_CDB_D_PREC, PTV_CDB_D_ACT_BF16,
                 PTV_CDB_D_NROOT, PTV_CDB_D_NCHROMA, PTV_CDB_D_NBASS, PTV_CDB_D_PERSIST, PTV_CDB_D_SPLITK, PTV_CDB_D_COUNT };
int ptv_chord_decoder_bwd(const void* const* tensors, const long* dims, void* stream);

/* ptv_decoder_tf_bwd: autograd through PtvaeDecoder.decoder, teacher-forced (ptvae.py:430-496) -- what functional.decoder_bwd_core sequences
 * on its fused bf16 path at the init_model() sizes: the chain  duration-GRU BPTT -> heads -> notes-GRU BPTT -> note-token / time-state
 * gradients -> time-GRU BPTT (persistent, split-K teams, event turn) -> dTOKS, dz  on `stream`, and the four groups of weight / bias
 * gradient products on the SIDE stream, each forked (event record / wait) where the Python sequencing forks it.  The caller joins the side
 * stream (or defers the join) and keeps every tensor of the table alive until then.  ~50 launches, the same arithmetic launch by launch
 * (bit-identical results).  Every G_* slot is the parameter's gradient buffer and is ACCUMULATED into.  TOP_H: device int, the last note
 * step whose gradient is non-zero (zero-skip limit of the head / duration products), or NULL = dense. */
enum PtvDtbTensor {
  /* inputs */
  PTV_DTB_Z = 0,          /* [B, Zs] fp32 */
  PTV_DTB_TOK_OP,         /* [15 R, E] fp32: the note tokens fed to the notes GRU */
  PTV_DTB_DP,             /* [M, ldp] fp32: gradient of the pitch logits; ACCUMULATED into (dP += dHD0 . W_dh[:, Hn:]) */
  PTV_DTB_DDUR,           /* [M, 10] fp32 */
  PTV_DTB_TOP_H,
  /* parameters (fp32 masters) and their packed / transposed bf16 forms */
  PTV_DTB_W_HH_D, PTV_DTB_B_HH_D, PTV_DTB_W_IH_D, PTV_DTB_W_OUT_D, PTV_DTB_SOS,
  PTV_DTB_PK_WDPT, PTV_DTB_PK_WCAT,                      /* heads_packs: 'wdpT', 'wcat' */
  PTV_DTB_PK_NOTES_WT,                                   /* notes_packs: 'wt' */
  PTV_DTB_WT_IH_N, PTV_DTB_WT_T2N, PTV_DTB_WT_IH_T, PTV_DTB_WT_HH_T, PTV_DTB_WT_ZHID, PTV_DTB_WT_ZIN,   /* transposed bf16 shadows [in, out] */
  /* saved by the forward */
  PTV_DTB_NS, PTV_DTB_NS16, PTV_DTB_Z_IN, PTV_DTB_TOKS, PTV_DTB_GATES_T, PTV_DTB_HN16, PTV_DTB_GATES_N, PTV_DTB_PITCH, PTV_DTB_HD16,
  PTV_DTB_TAB0, PTV_DTB_TAB, PTV_DTB_IDX,
  /* outputs */
  PTV_DTB_DZ,             /* [B, Zs] */
  PTV_DTB_DTOK,           /* [16, R, E] (slot 15 zeroed here) */
  PTV_DTB_DTOKS,          /* [33, B, 2He] (slot 32 zeroed here) */
  /* gradient buffers, DEC_PARAM_NAMES order */
  PTV_DTB_G_W_ZHID, PTV_DTB_G_B_ZHID, PTV_DTB_G_W_ZIN, PTV_DTB_G_B_ZIN, PTV_DTB_G_INIT_INPUT,
  PTV_DTB_G_W_IH_T, PTV_DTB_G_W_HH_T, PTV_DTB_G_B_IH_T, PTV_DTB_G_B_HH_T,
  PTV_DTB_G_W_T2N, PTV_DTB_G_B_T2N,
  PTV_DTB_G_W_IH_N, PTV_DTB_G_W_HH_N, PTV_DTB_G_B_IH_N, PTV_DTB_G_B_HH_N,
  PTV_DTB_G_W_P, PTV_DTB_G_B_P, PTV_DTB_G_W_DH, PTV_DTB_G_B_DH, PTV_DTB_G_W_OUT_D, PTV_DTB_G_B_OUT_D,
  PTV_DTB_G_W_IH_D, PTV_DTB_G_W_HH_D, PTV_DTB_G_B_IH_D, PTV_DTB_G_B_HH_D, PTV_DTB_G_SOS,
  /* scratch */
  PTV_DTB_DHD0,           /* [M, Hd] fp32 */
  PTV_DTB_PART,           /* [NBLK, ptv_dur_gru_bwd_part_size()] fp32 */
  PTV_DTB_S,              /* [part_size] fp32, ZEROED by the caller */
  PTV_DTB_TMP64,          /* [64] fp32, ZEROED */
  PTV_DTB_DNSUM,          /* [M, Hn] bf16 */
  PTV_DTB_DY16,           /* [M, 200] bf16 */
  PTV_DTB_TMP200,         /* [200, Hn] fp32 */
  PTV_DTB_CS200,          /* [200] fp32, ZEROED */
  PTV_DTB_DGI_N, PTV_DTB_DGH_N, PTV_DTB_DHN0, PTV_DTB_SCRATCH_N,
  PTV_DTB_TOP_STEP,       /* device int initialised to -1 */
  PTV_DTB_DGC, PTV_DTB_DNS,
  PTV_DTB_DGI_T, PTV_DTB_DGH_T, PTV_DTB_DZHID, PTV_DTB_DZG, PTV_DTB_DZ_IN,
  PTV_DTB_XCH, PTV_DTB_PART_T, PTV_DTB_SYNC,             /* the time GRU's persistent BPTT */
  PTV_DTB_WAIT_EVENT, PTV_DTB_RECORD_EVENT,              /* hipEvent_t: persistent launches take turns */
  PTV_DTB_SIDE_STREAM,    /* hipStream_t of the sibling stream */
  PTV_DTB_FORK_EVENT0, PTV_DTB_FORK_EVENT1, PTV_DTB_FORK_EVENT2, PTV_DTB_FORK_EVENT3,   /* hipEvent_t, one per fork */
  /* the forward ran on rows sorted by length (PTV_DTF_PERM ...): all or none.  NS16 / TOK_OP are then the gathered copies the forward left
   * (NS16: slot 0 unused, rows from NS16S - B*Ht ... the table holds NS16S itself in PTV_DTB_NS16S), DNS / DTOK come out in natural row order
   * (their products store through PERM: ptv_gemm_mtop_seg_map) */
  PTV_DTB_PERM, PTV_DTB_ROW_LEN,
  PTV_DTB_NS16S,          /* [R, Ht] bf16 gathered time states (operand of the weight_ih / time_to_notes gradients) */
  PTV_DTB_SEG_N,         /* int32 [15] (ptv_rows_seg_counts of ROW_LEN) or NULL: the weight-gradient products over (note step, row) skip the dead
                             blocks of every step (sorted mode only) */
  PTV_DTB_COUNT
};
enum PtvDtbDim { PTV_DTB_D_B = 0, PTV_DTB_D_E, PTV_DTB_D_HE, PTV_DTB_D_HT, PTV_DTB_D_HN, PTV_DTB_D_HD, PTV_DTB_D_NP, PTV_DTB_D_ZS, PTV_DTB_D_ZI,
                 PTV_DTB_D_LDP, PTV_DTB_D_NBLK, PTV_DTB_D_SPLITK, PTV_DTB_D_COUNT };
int ptv_decoder_tf_bwd(const void* const* tensors, const long* dims, void* stream);

/* ptv_bigru_final_bwd: autograd through a bidirectional GRU whose final states are its output (RnnEncoder / TextureEncoder, ptvae.py:23-31,
 * 116-122), bf16 precision, both directions' BPTT in ONE persistent launch (event turn in here), then per direction the weight / bias
 * gradients dW_ih += dgi^T . x, dW_hh += dgh^T . h (bias sums fused) -- the reversed direction's on the side stream, forked and joined in
 * here -- and, with DX, the input gradient dx (+)= dgi_0 . W_ih_0 + dgi_1 . W_ih_1.  What functional._bigru_backward sequences on its
 * persistent branch, bit-identical to it.  G_* slots are accumulated into. */
enum PtvBgbTensor {
  PTV_BGB_X = 0,          /* [T*M, I] the forward's input rows (fp32, or bf16 with d[PTV_BGB_D_X_BF16]) */
  PTV_BGB_DOUT,           /* [M, 2H] fp32: gradient of the two final states */
  PTV_BGB_HALL0, PTV_BGB_H16_0, PTV_BGB_GATES0, PTV_BGB_WT_HH0, PTV_BGB_WT_IH0,   /* forward direction: fp32 / bf16 states [T+1, M, H], gate planes,
                                                                                   * bf16 W_hh^T [H, 3H], bf16 W_ih^T [I, 3H] (NULL without DX) */
  PTV_BGB_HALL1, PTV_BGB_H16_1, PTV_BGB_GATES1, PTV_BGB_WT_HH1, PTV_BGB_WT_IH1,   /* reversed direction */
  PTV_BGB_G_W_IH0, PTV_BGB_G_W_HH0, PTV_BGB_G_B_IH0, PTV_BGB_G_B_HH0, PTV_BGB_G_W_IH1, PTV_BGB_G_W_HH1, PTV_BGB_G_B_IH1, PTV_BGB_G_B_HH1,
  PTV_BGB_DX,             /* out [T*M, I] fp32, or NULL: no input gradient wanted */
  PTV_BGB_DGI0, PTV_BGB_DGH0, PTV_BGB_DGI1, PTV_BGB_DGH1,                        /* scratch [T, M, 3H] bf16 */
  PTV_BGB_XCH0, PTV_BGB_XCH1, PTV_BGB_PART0, PTV_BGB_PART1, PTV_BGB_SYNC,        /* persistent launch (PART*: split-K partials or NULL) */
  PTV_BGB_WAIT_EVENT, PTV_BGB_RECORD_EVENT, PTV_BGB_SIDE_STREAM, PTV_BGB_FORK_EVENT, PTV_BGB_JOIN_EVENT,
  PTV_BGB_COUNT
};
enum PtvBgbDim { PTV_BGB_D_M = 0, PTV_BGB_D_T, PTV_BGB_D_H, PTV_BGB_D_I, PTV_BGB_D_X_BF16, PTV_BGB_D_DX_ACC, PTV_BGB_D_SPLITK, PTV_BGB_D_COUNT };
int ptv_bigru_final_bwd(const void* const* tensors, const long* dims, void* stream);

/* ptv_bigru_final_fwd: the forward of the above (functional._bigru_forward's persistent branch): per direction the input product
 * gi = x . W_ih^T + b_ih (bf16 out), the zero initial state, both recurrences in ONE persistent launch (event turn in here), the two final
 * states copied into OUT [M, 2H].  Saved for the backward: HALL / H16 / GATES.  bf16 precision; lengths (packed sequences) or NULL. */
enum PtvBgfTensor {
  PTV_BGF_X = 0,          /* [T*M, I] fp32 (or bf16 with d[PTV_BGF_D_X_BF16]) */
  PTV_BGF_LENGTHS,        /* [M] int32 or NULL */
  PTV_BGF_W16_IH0, PTV_BGF_B_IH0, PTV_BGF_W16_HH0, PTV_BGF_B_HH0, PTV_BGF_W16_IH1, PTV_BGF_B_IH1, PTV_BGF_W16_HH1, PTV_BGF_B_HH1,   /* bf16 weight shadows, fp32 biases */
  PTV_BGF_OUT,            /* out [M, 2H] fp32 */
  PTV_BGF_GI0, PTV_BGF_HALL0, PTV_BGF_H16_0, PTV_BGF_GATES0, PTV_BGF_GI1, PTV_BGF_HALL1, PTV_BGF_H16_1, PTV_BGF_GATES1,
  PTV_BGF_XCH0, PTV_BGF_XCH1, PTV_BGF_SYNC, PTV_BGF_WAIT_EVENT, PTV_BGF_RECORD_EVENT,
  PTV_BGF_COUNT
};
enum PtvBgfDim { PTV_BGF_D_M = 0, PTV_BGF_D_T, PTV_BGF_D_H, PTV_BGF_D_I, PTV_BGF_D_X_BF16,
                 PTV_BGF_D_WIH_F32,   /* W16_IH* are the fp32 masters (an input width that is no multiple of 8 has no bf16 shadow) */
                 PTV_BGF_D_COUNT };
int ptv_bigru_final_fwd(const void* const* tensors, const long* dims, void* stream);

/* ptv_bigru_rows_fwd / ptv_bigru_rows_bwd: the same pair for a bi-GRU over MANY short independent rows (dec_notes_emb_gru, the ground-truth
 * note summaries, ptvae.py:446-453: 32 B rows x 16 notes, H = 128) on the row-partitioned kernels -- one launch per direction for the whole
 * sequence, the input product fused, the reversed direction on the side stream (forked and joined in here).  What functional._bigru_forward
 * / _bigru_backward sequence on their row-kernel branch, bit-identical to it.  LENGTHS / PERM as ptv_row_gru_persist_fwd_perm; TOP0 / TOP1:
 * device ints initialised to -1 (the BPTT reports the last live time index; the products stop there), NULL = no limit. */
enum PtvBrfTensor {
  PTV_BRF_X = 0,          /* [T, M, I] fp32 */
  PTV_BRF_LENGTHS, PTV_BRF_PERM,           /* int32 [M] or NULL */
  PTV_BRF_PK_WG_H0, PTV_BRF_PK_WG_T0, PTV_BRF_B_HH0, PTV_BRF_B_IH0, PTV_BRF_PK_WG_H1, PTV_BRF_PK_WG_T1, PTV_BRF_B_HH1, PTV_BRF_B_IH1,
  PTV_BRF_OUT,            /* out [M, 2H] */
  PTV_BRF_HALL0, PTV_BRF_H16_0, PTV_BRF_GATES0, PTV_BRF_HALL1, PTV_BRF_H16_1, PTV_BRF_GATES1,
  PTV_BRF_SIDE_STREAM, PTV_BRF_FORK_EVENT, PTV_BRF_JOIN_EVENT,
  PTV_BRF_COUNT
};
enum PtvBrfDim { PTV_BRF_D_M = 0, PTV_BRF_D_T, PTV_BRF_D_H, PTV_BRF_D_I, PTV_BRF_D_COUNT };
int ptv_bigru_rows_fwd(const void* const* tensors, const long* dims, void* stream);
enum PtvBrbTensor {
  PTV_BRB_X = 0, PTV_BRB_DOUT, PTV_BRB_LENGTHS, PTV_BRB_PERM,
  PTV_BRB_PK_WT0, PTV_BRB_HALL0, PTV_BRB_H16_0, PTV_BRB_GATES0, PTV_BRB_WT_IH0,       /* WT_IH*: bf16 W_ih^T [I, 3H], NULL without DX */
  PTV_BRB_PK_WT1, PTV_BRB_HALL1, PTV_BRB_H16_1, PTV_BRB_GATES1, PTV_BRB_WT_IH1,
  PTV_BRB_G_W_IH0, PTV_BRB_G_W_HH0, PTV_BRB_G_B_IH0, PTV_BRB_G_B_HH0, PTV_BRB_G_W_IH1, PTV_BRB_G_W_HH1, PTV_BRB_G_B_IH1, PTV_BRB_G_B_HH1,
  PTV_BRB_DX,             /* out [T*M, I] fp32 or NULL */
  PTV_BRB_DGI0, PTV_BRB_DGH0, PTV_BRB_SCRATCH0, PTV_BRB_TOP0, PTV_BRB_DGI1, PTV_BRB_DGH1, PTV_BRB_SCRATCH1, PTV_BRB_TOP1,
  PTV_BRB_SIDE_STREAM, PTV_BRB_FORK_EVENT, PTV_BRB_JOIN_EVENT,
  PTV_BRB_SEG,            /* int32 [T] or NULL, with PERM = ptv_rows_by_length(LENGTHS) only: ptv_rows_seg_counts of the lengths in that order -- the
                             weight_hh products (operands indexed by position) skip the dead 128-row blocks of every step */
  PTV_BRB_COUNT
};
enum PtvBrbDim { PTV_BRB_D_M = 0, PTV_BRB_D_T, PTV_BRB_D_H, PTV_BRB_D_I, PTV_BRB_D_DX_ACC, PTV_BRB_D_DOUT_LD, PTV_BRB_D_COUNT };
int ptv_bigru_rows_bwd(const void* const* tensors, const long* dims, void* stream);

/* ptv_vae_loss_fwd / ptv_vae_loss_bwd: DisentangleVAE.loss_function (model.py:57-68: PianoTree reconstruction CE x2 with ignore_index, the
 * two KL terms, the three chord CEs, the 11 output scalars) and its backward, one call each -- what functional.VaeLossFn sequences.
 * scal = {beta, w0, w1, B * Z, 8 B, 96 B} as doubles.  PITCH_T / DUR_T / COUNTS: the targets of ptv_pianotree_targets; with
 * d[PTV_VL_D_HAVE_TARGETS] they were computed by the caller already (DisentangleVAE.loss() does, before the decoder).
 * One launch per direction (csrc/loss.hip: vae_loss_fwd_kernel / vae_loss_bwd_kernel; ptv_pianotree_targets in front when the forward
 * computes the targets), bit for bit what the launch sequence gives (9 / 8 launches: what runs without an ordered-reduction workspace,
 * and the backward without REC).
 * Forward with the nine D* slots and REC: the same launch also writes the gradients for the upstream (1, 0, ..., 0) -- losses[0].backward()
 * -- and REC, the record of that (upstream vector and beta, as bits, and a valid word; all nine or none; REC is cleared when the launch
 * sequence ran).  Backward with REC and EARLY: every block compares GOUT and beta with REC; equal bit for bit, the gradients stand in the
 * D* buffers of that forward already, the launch returns and adds one to EARLY; otherwise it computes the scales and writes every row.
 * A caller that hands other buffers than the forward's to the backward passes a cleared REC.
 * On a stream that is being captured both directions are the launch sequence; a forward with REC is PTV_ERR_ARG there. */
enum PtvVlTensor {
  PTV_VL_X = 0, PTV_VL_C,                                    /* int64 [B,32,16,6], fp32 [B,8,36] */
  PTV_VL_PITCH, PTV_VL_DUR,                                  /* logits in memory order: [480 B, ldp], [2400 B, 2] */
  PTV_VL_MU_C, PTV_VL_SD_C, PTV_VL_MU_R, PTV_VL_SD_R,        /* [B, Z] */
  PTV_VL_ROOT, PTV_VL_CHROMA, PTV_VL_BASS,                   /* [8 B, 12], [96 B, 2], [8 B, 12] */
  PTV_VL_PITCH_T, PTV_VL_DUR_T, PTV_VL_COUNTS, PTV_VL_ROOT_T, PTV_VL_CHROMA_T, PTV_VL_BASS_T,   /* int32 targets / counts[3] */
  PTV_VL_SUMS,            /* fwd: [8] fp32 ZEROED */
  PTV_VL_OUT,             /* fwd out: [11] */
  PTV_VL_GOUT,            /* bwd in: [11] */
  PTV_VL_GS,              /* bwd scratch: [8]; only the launch sequence (no REC) needs it */
  PTV_VL_DPITCH, PTV_VL_DDUR, PTV_VL_DMU_C, PTV_VL_DSD_C, PTV_VL_DMU_R, PTV_VL_DSD_R, PTV_VL_DROOT, PTV_VL_DCHROMA, PTV_VL_DBASS,   /* bwd out; fwd out with REC */
  PTV_VL_REC,             /* [16] 32-bit words: the record of a forward that wrote the gradients, or NULL */
  PTV_VL_EARLY,           /* bwd with REC: uint32 [1], counts the launches that returned on a matching record */
  PTV_VL_COUNT
};
enum PtvVlDim { PTV_VL_D_B = 0, PTV_VL_D_Z, PTV_VL_D_NP, PTV_VL_D_LDP, PTV_VL_D_SM_P, PTV_VL_D_SM_C, PTV_VL_D_HAVE_TARGETS, PTV_VL_D_COUNT };
int ptv_vae_loss_fwd(const void* const* tensors, const long* dims, const double* scal, void* stream);
int ptv_vae_loss_bwd(const void* const* tensors, const long* dims, const double* scal, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Free-running tokens.
 * ptv_note_token (ptvae.py:408-416 + pitch_dur_ind_to_note_token :328-334): per row pitch argmax (first
 *   maximal index), predicted token pred[r] = note_embedding(onehot(pitch) | 5 duration bits) with
 *   dur_idx[d*dur_stride + r] the duration argmaxes, predicted grid row xhat[r] = (pitch, bits) int64,
 *   running predicted length plen[r] (first <eos> step n; the last step fills 15).
 * ptv_chord_token (ptvae.py:72-78): next chord-decoder token [B,36]; root/bass parts are the UNION over
 *   the batch of the rows' argmax one-hots (the reference's index-broadcast quirk), chroma = per-row bits.
 * ptv_route_slices: dst(mask[s]) (+)= src for nslices consecutive slices of slice_elems floats -- routes
 *   token gradients to the ground-truth embedding (mask 1) or the predicted-token buffer (mask 0).
 */
int ptv_note_token(const float* pitch, long ld_pitch, const int* dur_idx, long dur_stride, const float* W, const float* bias, int E,
                   float* pred, long ld_pred, long* xhat, long xhat_stride, int* plen, int n, int last,
                   const int* force_pitch, int M, void* stream);
int ptv_chord_token(const float* root, const float* chroma, const float* bass, unsigned* masks2, float* token, int B, void* stream);
int ptv_route_slices(const float* src, float* dstA, float* dstB, const int* mask, long slice_elems, int nslices, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data contract on device: what ArrangementDataset.__getitem__ (dataset.py:88-112) does per item
 * with converter.py:65-68 (augment_pr), :78-113 (pr_to_onehot_pr + piano_roll_to_target), :116-147 (target_to_3dtarget
 * with the arguments of dataset.py:98-104) and :150-164 (expand_chord), for a whole batch in one launch.
 *   pr      [N,32,128] uint8 accompaniment piano-rolls (2 onset, 1 sustain, 0 silence; converter.py:35-47)
 *   chord14 [N,8,14] float  raw chords [root, 12 chroma bits, bass]
 *   index[B] (NULL = identity) picks the item of sample b, shift[B] (NULL = 0) its transposition in semitones
 *   -> pr_mat [B,32,128] f32, x [B,32,16,6] int64, c [B,8,36] f32;  *err |= 1 if a step held more than 14 onsets
 *      (the reference raises IndexError there; the kernel keeps the lowest 14)
 */
int ptv_batch_transform(const unsigned char* pr, const float* chord14, const int* index, const int* shift,
                        float* pr_mat, long* x, float* c, int* err, int B, void* stream);
/* interp_path (model.py:216-242): out[b, i, :] = slerp between z1[b] and z2[b] at i/(n-1), norms interpolated geometrically */
int ptv_slerp_path(const float* z1, const float* z2, float* out, int B, int D, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Output path on device: the inverse of the data contract above, from what the decoders emit to what the model consumes.
 * ptv_grid_to_pr (PtvaeDecoder.grid_to_pr_and_notes, ptvae.py:558-575, for a whole batch; one workgroup per sample, csrc/output.hip):
 *   grid [B,32,R,6] int64 contiguous, 16-byte aligned, R = 15 or 16; with R = 16 row 0 of every step is <sos> and is skipped (the
 *   reference's grid[:, 1:]).  A step's rows are read in order up to the first row whose pitch is pitch_eos, at most max_notes
 *   (1..R; the reference reads 10) and at most the 15 rows a step holds after <sos>.  pitch = row[0] + min_pitch,
 *   dur = 1 + the MSB-first binary value of row[1..5].  Every output but err may be NULL (notes and count go together):
 *   -> pr_mat  [B,32,128] f32    0, then pr[t, pitch] = min(dur, 32 - t); of two rows of a step with one pitch the later wins
 *      notes   [B,32*max_notes,3] int32 (pitch, t, dur) with dur unclipped, time step major, row minor (both rows of a duplicate
 *              pitch); count [B] int32 entries are valid, the rest is not written
 *      x_clean [B,32,16,6] int64  the layout ptv_batch_transform writes: <sos>, the step's first 14 accepted notes in decoded order
 *              as (pitch, 5 duration bits), <eos>, <pad> rows
 *      err     [B] int32, written for every sample: bit 0 = a row before <eos> has a pitch outside 0..127 (the reference raises
 *              IndexError), bit 1 = a duration bit is not 0 or 1 (ValueError); such a row is skipped (no cell, no note, no x_clean
 *              row) and the sample goes on.  Bit 2 = the FIRST skipped row (time step major) had a bad duration bit, i.e. the
 *              reference's exception for this sample is ValueError (it parses the duration before it indexes the pitch);
 *              bit 3 = a step held 15 accepted notes, x_clean kept 14 (only with max_notes >= 15).
 * ptv_chord_tokens (the token RnnDecoder.forward feeds back, ptvae.py:72-78, per row): logits in the chord decoder's step-major
 *   layout root [T,B,12], chroma [T,B,24] (12 pairs), bass [T,B,12] -> c [B,T,36] f32 = root one-hot | 12 chroma bits | bass one-hot
 *   (the layout chd_encoder and loss() take) and chord14 [B,T,14] f32 = root index | 12 chroma bits | bass index (the bank layout
 *   ptv_batch_transform reads); either may be NULL.  Argmax ties resolve to the lowest index.
 */
int ptv_grid_to_pr(const long* grid, int B, int R, int max_notes, int min_pitch, int pitch_eos, float* pr_mat, int* notes, int* count,
                   long* x_clean, int* err, void* stream);
int ptv_chord_tokens(const float* root, const float* chroma, const float* bass, float* c, float* chord14, int T, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-sample scores (csrc/score.hip; forward only): what the loss node above reduces to 11 batch means, kept per sample, plus the arg-max
 * hit counts behind the reconstruction accuracies.  Every output element has one writer and one fixed summation order (no float atomics,
 * no workspace): results are bit-identical from run to run and do not depend on the layout the logits come in.
 * ptv_recon_step_scores: pitch / dur fp32 logits; row i of pitch starts at pitch + i * ld_pitch (ld_pitch >= 130; 16-byte loads when
 *   ld_pitch % 4 == 0, ld_pitch >= 132 and pitch is 16-byte aligned, 4-byte loads of the same values otherwise), row i of dur is 10
 *   contiguous floats (5 bits x 2 classes); i = (n*32 + t)*B + b if step_major, else (b*32 + t)*15 + n (ptv_pianotree_targets' orders).
 *   Targets are read from x (int64 [B,32,16,6]), row n + 1: pitch x[..,0] (130 = ignored), duration bits x[..,1..5] (2 = ignored).
 *   A row or bit whose target is ignored is never loaded; a pitch target outside 0..130 / a bit outside 0..2 is skipped the same way.
 *   -> step_scores [B,32,2] f32 = (pitch NLL sum, duration NLL sum) of the step, rows added in ascending n, bits in ascending order;
 *      NLL = -(l[target] - max - log(sum exp(l - max))) in fp32
 *      step_counts [B,32,6] int32 = pitch_n (pitch targets != 130), pitch_hit (those whose arg-max over the 130 classes is the target),
 *      dur_n (bit targets != 2), dur_hit (those whose arg-max of the two classes is the target), note_n (pitch targets < 128),
 *      note_hit (those with the pitch hit and all five bits hit; an ignored bit is not a hit).  Arg-max ties resolve to the lowest
 *      index (a tied duration pair is class 0).  A step without targets writes zeros.  Both outputs are batch-major whatever the input.
 * ptv_score_fold: scores [B,2] f32 / counts [B,6] int32 = the sums over t = 0..31 in ascending order (fp32, sequential).
 * ptv_kl_rows: out[b] = sum_z (-log sd + (sd^2 + mu^2)/2 - 1/2) over mu / sd [B,Z]; one wave per row, lane l adds z = l, l + 64, ...
 *   and a xor tree folds the lanes: the order depends on Z only, not on B.
 * ptv_chord_step_scores: root [.,12], chroma [.,12,2], bass [.,12] logits with rows [8][B] if step_major else [B][8]; targets derived from
 *   c [B,8,36] as ptv_chord_targets derives them -> scores [B,3] f32 = root / chroma / bass NLL sums over the 8 steps (ascending step,
 *   chroma bits ascending), counts [B,3] int32 = root hits of 8, chroma-bit hits of 96, bass hits of 8.  The tie rules as above.
 * ptv_roll_match: est_pr / ref_pr f32 [B,32,128] (ptv_grid_to_pr's pr_mat) -> counts [B,4] int32 = cells > 0 in est, cells > 0 in ref,
 *   cells > 0 in both (onset matches), cells > 0 in both and equal (onset and duration match).
 * All five return PTV_ERR_ARG for a NULL pointer or B <= 0 and write nothing then.
 */
int ptv_recon_step_scores(const float* pitch, long ld_pitch, const float* dur, const long* x, int B, int step_major, float* step_scores,
                          int* step_counts, void* stream);
int ptv_score_fold(const float* step_scores, const int* step_counts, int B, float* scores, int* counts, void* stream);
int ptv_kl_rows(const float* mu, const float* sd, int B, int Z, float* out, void* stream);
int ptv_chord_step_scores(const float* root, const float* chroma, const float* bass, const float* c, int B, int step_major, float* scores,
                          int* counts, void* stream);
int ptv_roll_match(const float* est_pr, const float* ref_pr, int B, int* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Log-probabilities of a free-running decode and best-of-n (csrc/decode_score.hip; DESIGN.md 7e, INTEGRATION.md "Decode log-probabilities").
 * A post-pass over what a decode leaves on the device; forward only, no atomics, no workspace: every output element has one writer and one
 * fixed summation order, so the results are bit-identical from run to run, across the two row orders and across the load paths.
 * ptv_decode_logprob: one wave per (sample b, time step t).
 *   pitch / ld_pitch / step_major / dur: the plain logits a decode wrote, rows and load rule as ptv_recon_step_scores (row of (b, t, n) =
 *     (n*32 + t)*B + b if step_major else (b*32 + t)*15 + n; 16-byte loads iff ld_pitch % 4 == 0, ld_pitch >= 132 and the base is 16-byte
 *     aligned, else 4-byte loads of the same classes); xhat: the decided grid int64 [B][32][16][6].
 *   sample / sample_bytes: NULL / 0 (an argmax decode) or the decode's sampling block of 32, 48, 64 or 80 bytes ("Sampled decode" / "Per-row sampling" below);
 *     anything else is PTV_ERR_ARG.  force_pitch [15][32B] / force_dur [5][480B] (ptv_keep_force_build's layout), or NULL, each on its own.
 *   What counts: for (b, t) L = the first slot s in 1..15 with xhat[b][t][s][0] == 129, else 15 (ptv_keep_force_build's rule).  The pitch
 *     decisions of the note steps n = 0..L-1 count (the <eos> among them); the five duration bits of those notes whose pitch is < 128
 *     count.  Logit rows and bits that do not count are never loaded.  A counted pitch outside 0..129 or a counted bit outside {0, 1}
 *     names no class: it is skipped (not counted), and the pitch sets bit 0 of err[b].
 *   For a counted decision with decided class d:
 *     logp = log softmax(logits)[d] over all 130 classes (both classes of a bit): temperature 1, no truncation, no constraint; forced
 *       decisions included.
 *     logq = the log-probability under the distribution the decode drew from.  Pitch: (v[d] - m) / T_pitch - log sum exp((v - m) /
 *       T_pitch) over the classes that are allowed and kept, m their maximum -- the set is the decoder's own (pitch_constrain and
 *       pitch_keep_threshold of csrc/philox.hpp on the block's mask row, flags, top_k, ln_min_p, top_p_q24, with lo = the largest decided
 *       pitch < 128 before n in the step).  Bit: log softmax of the pair divided by T_dur.  0 when the temperature is 0 or sample is NULL
 *       (the argmax is certain).  A forced decision (force word >= 0) contributes 0 and is counted in forced_*.  A free decision outside
 *       the recomputed set sets bit 0 of err[b] and contributes 0: it never happens on a decode's own outputs.
 *   step_logp [B][32][4] f32 = (logp pitch, logp dur, logq pitch, logq dur), each added over ascending n, a note's pitch term before its
 *     bits (ascending); step_counts [B][32][4] int32 = (pitch_n, dur_n, forced_pitch_n, forced_dur_n); err [B] int32.
 * ptv_decode_logprob_fold: sums [B][4] f32 / counts [B][4] int32 = the sums over t = 0..31 in ascending order (fp32, sequential).
 * ptv_best_of_gather: score f32 [n][B], grids int64 [n*B][32][16][6], sums f32 [n*B][4], candidate k of row b at row k*B + b ->
 *   best [B] int32 = the first k whose score is maximal (a NaN never wins; all NaN: k = 0 and err[b] = 2, else err[b] = 0),
 *   out_grid [B][32][16][6] = grids[best*B + b], out_sums [B][4] = sums[best*B + b].
 * All three return PTV_ERR_ARG for a NULL pointer (those marked optional excepted), B < 1 or n < 1 and write nothing then.
 */
int ptv_decode_logprob(const float* pitch, long ld_pitch, const float* dur, const long* xhat, int B, int step_major, const void* sample,
                       int sample_bytes, const int* force_pitch, const int* force_dur, float* step_logp, int* step_counts, int* err,
                       void* stream);
int ptv_decode_logprob_fold(const float* step_logp, const int* step_counts, int B, float* sums, int* counts, void* stream);
int ptv_best_of_gather(const float* score, const long* grids, const float* sums, int n, int B, int* best, long* out_grid, float* out_sums,
                       int* err, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row-independent free-running chord decode (csrc/chord_decode.hip; DESIGN.md 7f, INTEGRATION.md "Chord decode"): seeded sampling, kept
 * chords and log-probabilities of the chord decoder (RnnDecoder, ptvae.py:32-87).  Every row feeds back its OWN token (root one-hot | 12
 * chroma bits | bass one-hot): the union over the batch that ptv_chord_token forms for parity with the reference's training step is not
 * formed here, so a row's chords do not depend on what else is in the batch.  Inference only; every output element has one writer, no
 * atomics: results are bit-identical from run to run.
 * ptv_chord_decide: the decisions of ONE chord step t (0..7) for B rows, 16 lanes per row, lane j < 12 owns root class j, bass class j and
 *   chroma pair j.
 *   root [B][12], chroma [B][24] (12 pairs: class 0, class 1), bass [B][12]: the step's fp32 logits.
 *   sample: NULL (argmax, logq = 0) or the 32-byte sampling block ("Sampled decode" above): seed, draw, sample_offset, T_chord in the
 *     t_pitch word, T_chroma in the t_dur word.  A decision is the first maximal index of logit + T * gumbel(word) (T = 0: the plain
 *     argmax, ties to the lowest index); chroma bit j is 1 iff e1 + T g1 > e0 + T g0.  Root and bass take T_chord, the bits T_chroma.
 *     The words are those of the decoder's Philox domain at the note step nothing else uses, n = 15, kind 0, sub = j, global sample
 *     sample_offset + b: word 0 perturbs root class j, word 1 bass class j, word 2 / 3 class 0 / 1 of chroma bit j.
 *   keep_c f32 [B][8][36] or NULL (no keep), keep_steps uint8 [keep_rows][8] with keep_rows = B or 1 (required with keep_c): at a step
 *     whose byte is non-zero the decisions are forced from keep_c[b][t] -- root = the index of the single non-zero entry of [0:12], bass
 *     the same of [24:36], chroma bit k = keep_c[b][t][12 + k] != 0.  A root / bass block without exactly one non-zero entry forces
 *     nothing for that head (the decision stays free) and sets bit 0 of step_err[b][t].  keep_c of a step that is not kept is not read.
 *   -> tok [B][36] (or NULL: the last step) the token of the next step; row [b][t] of c [B][8][36] (the same token) and of chord14
 *      [B][8][14] (ptv_chord_tokens' layout: root index, 12 bits, bass index); row [b][t] of step_logp / step_logq f32 [B][8][3], of
 *      step_forced int32 [B][8][3] and of step_err int32 [B][8], heads in the order (root, chroma, bass):
 *        logp = log softmax(logits) at the decided class, the chroma figure the sum over its 12 bits in ascending order; forced
 *          decisions included
 *        logq = log softmax(logits / T) at the decided class; 0 where T = 0 or sample is NULL, and 0 for a forced decision
 *        forced = the number of forced decisions: 0 / 1, 0 / 12, 0 / 1
 *   PTV_ERR_ARG (nothing launched): a NULL logit array or output (tok excepted), B < 1, t outside 0..7, keep_c without keep_steps,
 *   keep_rows other than 1 or B.
 * ptv_chord_logprob_fold: logp / logq f32 [B][3] = the sums of step_logp / step_logq over t = 0..7 in ascending order (fp32, sequential),
 *   forced int32 [B][3] the same of step_forced, err int32 [B] the OR of step_err.  One thread per output element.
 * ptv_chord_decode: the whole decode of z [B][Z] in one call -- z2dec_hid, z2dec_in and the z part of the input product once, then per
 *   step the token part of the input product (K = 36), ptv_gru_step_fwd, the three head products and ptv_chord_decide, then the fold:
 *   4 + 8 * 6 + 1 launches.  fp32 or bf16 precision as ptv_chord_decoder_fwd (fp32 tensors either way); no gates are saved.  The geometry
 *   is the model's: 8 steps, tokens of 36, heads of 12 / 24 / 12; H a multiple of 4.  Optional slots (NULL): SAMPLE, KEEP_C, KEEP_STEPS.
 *   ROOT / CHROMA / BASS keep the step-major logits of the decode.
 */
int ptv_chord_decide(const float* root, const float* chroma, const float* bass, int B, int t, const void* sample, const float* keep_c,
                     const unsigned char* keep_steps, int keep_rows, float* tok, float* c, float* chord14, float* step_logp,
                     float* step_logq, int* step_forced, int* step_err, void* stream);
int ptv_chord_logprob_fold(const float* step_logp, const float* step_logq, const int* step_forced, const int* step_err, int B,
                           float* logp, float* logq, int* forced, int* err, void* stream);
enum PtvCdsTensor {
  PTV_CDS_Z = 0,          /* [B, Z] */
  PTV_CDS_W_ZHID, PTV_CDS_B_ZHID, PTV_CDS_W_ZIN, PTV_CDS_B_ZIN, PTV_CDS_INIT_INPUT,
  PTV_CDS_W_IH,           /* [3H, 36 + Zi] */
  PTV_CDS_B_IH, PTV_CDS_W_HH, PTV_CDS_B_HH, PTV_CDS_W_ROOT, PTV_CDS_B_ROOT, PTV_CDS_W_CHROMA, PTV_CDS_B_CHROMA, PTV_CDS_W_BASS, PTV_CDS_B_BASS,
  PTV_CDS_SAMPLE,         /* the 32-byte sampling block, or NULL */
  PTV_CDS_KEEP_C,         /* [B, 8, 36], or NULL */
  PTV_CDS_KEEP_STEPS,     /* uint8 [KEEP_ROWS, 8], with KEEP_C */
  PTV_CDS_HALL,           /* out [9, B, H] states (slot 0 = z2dec_hid(z)) */
  PTV_CDS_Z_IN,           /* out [B, Zi] */
  PTV_CDS_ZG,             /* out [B, 3H] */
  PTV_CDS_GI,             /* scratch [B, 3H] */
  PTV_CDS_TOK,            /* scratch [B, 36] */
  PTV_CDS_ROOT, PTV_CDS_CHROMA, PTV_CDS_BASS,   /* out [8, B, 12 / 24 / 12] logits, step-major */
  PTV_CDS_C,              /* out [B, 8, 36] */
  PTV_CDS_CHORD14,        /* out [B, 8, 14] */
  PTV_CDS_STEP_LOGP, PTV_CDS_STEP_LOGQ,   /* out f32 [B, 8, 3] */
  PTV_CDS_STEP_FORCED,    /* out int32 [B, 8, 3] */
  PTV_CDS_STEP_ERR,       /* out int32 [B, 8] */
  PTV_CDS_LOGP, PTV_CDS_LOGQ,   /* out f32 [B, 3] */
  PTV_CDS_FORCED,         /* out int32 [B, 3] */
  PTV_CDS_ERR,            /* out int32 [B] */
  PTV_CDS_COUNT
};
enum PtvCdsDim { PTV_CDS_D_B = 0, PTV_CDS_D_H, PTV_CDS_D_Z, PTV_CDS_D_ZI, PTV_CDS_D_PREC, PTV_CDS_D_KEEP_ROWS, PTV_CDS_D_COUNT };
int ptv_chord_decode(const void* const* tensors, const long* dims, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Chord grammar (csrc/chord_decode.hip; DESIGN.md 7f, INTEGRATION.md "Chord grammar"): the chord step above under a rule -- which roots and
 * pitch classes are allowed, a vocabulary of chord qualities in place of twelve independent bits, a chord-tone bass.
 * rule int32 [rule_rows][8], rule_rows = B or 1 (one row serves every sample); the word of (row b, step t):
 *   bits 0..11   root mask: bit r set = root r allowed
 *   bits 12..23  chroma mask: bit 12 + p set = absolute pitch class p may be set in the chroma
 *   bit 24       PTV_CHORD_RULE_VOCAB: the chroma is ONE draw from the vocabulary instead of twelve bit draws (ignored when n_vocab = 0)
 *   bit 25       PTV_CHORD_RULE_ROOT_IN_CHORD: the chroma bit of the decided root is 1 (a vocabulary implies it: every template holds 0)
 *   bit 26       PTV_CHORD_RULE_BASS_IN_CHORD: bass interval i is allowed iff the decided chroma holds pitch class (root + i) % 12
 *   bits 27..31  0 (the kernel ignores them)
 *   PTV_CHORD_RULE_IDENTITY = 0x00ffffff with n_vocab = 0: every output of ptv_chord_decide, bit for bit.
 * vocab int32 [n_vocab], 0 <= n_vocab <= 64: root-relative 12-bit templates, bit i = interval i above the root is in the chord (the
 *   caller keeps bit 0 set, the value inside 12 bits and the templates distinct).
 * The decisions of (b, t), every set judged on the plain logits:
 *   a kept step (keep_c / keep_steps) is ptv_chord_decide's: the rule is not consulted, error bit 0 as there.
 *   root: the first maximal index over the allowed roots of logit + T_chord * gumbel (word 0 of sub = j, as ptv_chord_decide).  No root
 *     allowed: all twelve are, and PTV_CHORD_ERR_ROOT_MASK is set.  logq = log softmax(logits / T_chord) over the allowed roots (one
 *     allowed root: exactly 0); logp stays the model's log softmax over all twelve, here and below.
 *   chroma without a vocabulary: bit p is free iff mask bit p is set, else 0; under ROOT_IN_CHORD bit r is 1 whatever the mask says.
 *     Free bits are decided as by ptv_chord_decide (words 2 / 3 of sub = p); logq adds the free bits in ascending order, forced bits 0.
 *   chroma with a vocabulary: template v stands for A_v = its bits rotated up by r (mod 12); it is allowed iff A_v lies inside the chroma
 *     mask united with {r}.  None allowed: all n_vocab are (the vocabulary wins, the mask yields) and PTV_CHORD_ERR_NO_TEMPLATE is set.
 *     Score s_v = the sum over p = 0..11 ascending of (p in A_v ? e1[p] : e0[p]), fp32 from 0: softmax(s / T_chroma) over the allowed
 *     templates is the model's bit-product distribution conditioned on them.  The decision is the first maximal allowed v of
 *     s_v + T_chroma * gumbel(word v >> 4 of the Philox call at n = 15, kind 0, sub = 16 + (v & 15)); the step's bits are A_v.
 *     logq = s_v / T - log sum over the allowed u of exp(s_u / T) (0 at T_chroma = 0): a lane adds its templates j, j + 16, j + 32,
 *     j + 48 in that order, a disallowed one as 0, then the 16-lane rotation tree.
 *   bass under BASS_IN_CHORD: over the intervals i whose pitch class (r + i) % 12 is a decided bit, decision and logq as the root's with
 *     word 1.  All twelve bits 0: all twelve intervals, and PTV_CHORD_ERR_NO_BASS is set.
 * step_forced counts the decisions a keep forced, as before; the error bits are ORed into step_err / err.
 * ptv_chord_decide_grammar: PTV_ERR_ARG (nothing launched) in the cases of ptv_chord_decide and for rule = NULL, rule_rows other than 1
 *   or B, n_vocab outside 0..64, n_vocab > 0 with vocab = NULL.
 * ptv_chord_decode_grammar: ptv_chord_decode with the decide launch replaced -- the same launches in the same order.  Its tables repeat
 *   PTV_CDS_* slot for slot and add RULE (required), VOCAB (NULL with N_VOCAB = 0) and the dimensions RULE_ROWS, N_VOCAB.
 */
#define PTV_CHORD_RULE_VOCAB (1 << 24)
#define PTV_CHORD_RULE_ROOT_IN_CHORD (1 << 25)
#define PTV_CHORD_RULE_BASS_IN_CHORD (1 << 26)
#define PTV_CHORD_RULE_IDENTITY 0x00ffffff
#define PTV_CHORD_ERR_KEEP 1        /* a kept root / bass block without exactly one non-zero entry (ptv_chord_decide's bit) */
#define PTV_CHORD_ERR_ROOT_MASK 2   /* no root allowed: all twelve were */
#define PTV_CHORD_ERR_NO_TEMPLATE 4 /* no template inside the chroma mask: all of them were allowed */
#define PTV_CHORD_ERR_NO_BASS 8     /* no chroma bit under BASS_IN_CHORD: all twelve intervals were allowed */
int ptv_chord_decide_grammar(const float* root, const float* chroma, const float* bass, int B, int t, const void* sample,
                             const float* keep_c, const unsigned char* keep_steps, int keep_rows, const int* rule, int rule_rows,
                             const int* vocab, int n_vocab, float* tok, float* c, float* chord14, float* step_logp, float* step_logq,
                             int* step_forced, int* step_err, void* stream);
enum PtvCdgTensor {
  PTV_CDG_Z = 0,
  PTV_CDG_W_ZHID, PTV_CDG_B_ZHID, PTV_CDG_W_ZIN, PTV_CDG_B_ZIN, PTV_CDG_INIT_INPUT,
  PTV_CDG_W_IH,
  PTV_CDG_B_IH, PTV_CDG_W_HH, PTV_CDG_B_HH, PTV_CDG_W_ROOT, PTV_CDG_B_ROOT, PTV_CDG_W_CHROMA, PTV_CDG_B_CHROMA, PTV_CDG_W_BASS, PTV_CDG_B_BASS,
  PTV_CDG_SAMPLE,
  PTV_CDG_KEEP_C,
  PTV_CDG_KEEP_STEPS,
  PTV_CDG_HALL,
  PTV_CDG_Z_IN,
  PTV_CDG_ZG,
  PTV_CDG_GI,
  PTV_CDG_TOK,
  PTV_CDG_ROOT, PTV_CDG_CHROMA, PTV_CDG_BASS,
  PTV_CDG_C,
  PTV_CDG_CHORD14,
  PTV_CDG_STEP_LOGP, PTV_CDG_STEP_LOGQ,
  PTV_CDG_STEP_FORCED,
  PTV_CDG_STEP_ERR,
  PTV_CDG_LOGP, PTV_CDG_LOGQ,
  PTV_CDG_FORCED,
  PTV_CDG_ERR,            /* ... every slot above as its PTV_CDS_ namesake */
  PTV_CDG_RULE,           /* int32 [RULE_ROWS, 8] */
  PTV_CDG_VOCAB,          /* int32 [N_VOCAB], or NULL with N_VOCAB = 0 */
  PTV_CDG_COUNT
};
enum PtvCdgDim { PTV_CDG_D_B = 0, PTV_CDG_D_H, PTV_CDG_D_Z, PTV_CDG_D_ZI, PTV_CDG_D_PREC, PTV_CDG_D_KEEP_ROWS, PTV_CDG_D_RULE_ROWS,
                 PTV_CDG_D_N_VOCAB, PTV_CDG_D_COUNT };
int ptv_chord_decode_grammar(const void* const* tensors, const long* dims, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Note-matrix song bank on device (csrc/dataset.hip): what ArrangementDataset.__getitem__ does BEFORE the data contract above, from
 * the per-bar note matrices (dataset.py:67-93 over converter.py:35-76), and detrend_pianotree (dataset.py:123-213) after it.
 * Bank: the bars of all songs in order.  acc_rec / mel_rec hold one 32-bit record per note, bar after bar, acc_off / mel_off [n_bar+1]
 * int32 the first record of every bar (a bar whose track is None has none).  A record is
 *     bits 0..7   pitch, 255 = anything above 254
 *     bits 8..13  onset step when the bar is the FIRST bar of a window, int(sb*sde+sq) of converter.py:41; 63 = anything above 62
 *     bits 14..19 end step in that place, int(eb*ede+eq), already clipped to 32
 *     bits 20..25 / 26..31  the same two steps when the bar is the SECOND bar (the note translated by ts beats, dataset.py:58)
 * all evaluated by the host builder in the reference's own arithmetic; negative values never enter a bank.
 * chord_bars [n_bar,4,14] f32: the bars' raw chords [root, 12 chroma bits, bass].
 * ptv_window_rolls, one workgroup per sample: the window of sample b is bars first_bar[b], first_bar[b]+1, shift[b] (NULL = 0) its
 *   transposition.  Notes are applied first bar first, in record order.  Every output but err may be NULL; pr, prs, mel 16-byte aligned:
 *   -> pr      [B,32,128] u8     ext_nmat_to_pr UNSHIFTED (what ptv_batch_transform reads): per note pr[s,p] = 2, then
 *                                pr[s+1:min(e,32), p] = 1, later notes overwriting earlier ones
 *      prs     [B,32,128,3] u8   onset / sustain / silence one-hots of that roll rolled by shift along the pitch axis (wraps)
 *      mel     [B,1,32,130] f32  ext_nmat_to_mel_pr: column 129 is 1 except over [s,e), column 128 is 1 over [s+1,e), mel[s,p] = 1;
 *                                then the 128 pitch columns rolled by shift
 *      chord14 [B,8,14] f32      the two bars' chord rows
 *      err     [B] int32, written for every sample: bit 0 = a note of the window has an onset step >= 32 or a pitch > 127 (the
 *                                reference raises IndexError; the note is skipped, the sample goes on); bit 1 = first_bar[b] is not in
 *                                0 .. n_bar-2 (the sample is an empty window with zero chords)
 * ptv_detrend_pianotree, one workgroup per sample, one thread per row: x [B,32,16,6] int64 and c [B,8,36] f32 (what
 *   ptv_batch_transform writes), x and dt_x 16-byte aligned -> dt_x [B,32,16,39] u8 = one-hots is_note 4 | is_bass 3 | octave 12 | degree 8 |
 *   n_state 7, then the row's five duration columns as they are.  A pitch outside 0..143 sets none of the 34 class cells.
 */
int ptv_window_rolls(const unsigned* acc_rec, const int* acc_off, const unsigned* mel_rec, const int* mel_off, const float* chord_bars,
                     int n_bar, const int* first_bar, const int* shift, int B, unsigned char* pr, unsigned char* prs, float* mel,
                     float* chord14, int* err, void* stream);
int ptv_detrend_pianotree(const long* x, const float* c, unsigned char* dt_x, int B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Free-running / scheduled-sampling decoder as row-partitioned persistent kernels (csrc/freerun.hip): PtvaeDecoder.decode_notes
 * + decode_note (ptvae.py:336-428) for ONE time step t and ALL 15 note steps in one launch, a workgroup per panel of 16 samples
 * (state in LDS / registers, weights streamed from L2 in MFMA-fragment-major packing), and the re-summarisation of the
 * predicted notes (bi-GRU with packed-sequence masking, ptvae.py:476-486) that yields the next time-step token.
 * bf16 MFMA operands, fp32 state / logits; init_model() geometry only (E = He = 128, Hn = 512, Hd = 64, 130 pitches).
 *   ptv_pack_mfma_b: W fp32 [N][ld] (K columns from the given base) -> bf16 [ceil(N/16)][ceil(K/32)][64 lanes][8]: the B fragment
 *     of 16 rows x 32 k as one contiguous 1-KB wave load (zero padded); ptv_pack_mfma_b_size = elements of `out`.
 *     pairs = 1 (N % 32 == 0) interleaves the rows of every pair of tiles so that lane (row, quad) of the MFMA C layout owns the 8
 *     consecutive output columns 32t + 8*quad .. +7 across the pair's two accumulators (no cross-lane movement in the epilogue).
 *   ptv_free_note_loop: w / io are HOST arrays of 16 / 17 device pointers:
 *     w  = { pack(dec_notes_gru.weight_hh), pack(dec_notes_gru.weight_ih[:, Ht:]), pack(pitch_out_linear.weight),
 *            pack(dur_hid_linear.weight[:, :512]), pack(dur_hid_linear.weight[:, 512:]), pack(dec_dur_gru.weight_hh),
 *            dec_notes_gru.bias_hh, pitch_out_linear.bias, dur_hid_linear.bias, dec_dur_gru.bias_hh, tab0 [192] = W_ih_d sos + b,
 *            tab [2][192] = W_ih_d onehot(0/1) + b, dur_out_linear.weight, .bias, note_embedding.weight^T [135][128], .bias }
 *     io = { gc [B][1536] (W_ih_n[:, :Ht] ns + b_ih for this t), emb [16][R][128] ground-truth embedding or NULL,
 *            HN [16][R][512] (slot 0 rows of t = initial state, written by the caller), gates_n [15][4][R][512] bf16,
 *            pitch [M][ld_pitch], HD [6][M][64], gates_d [5][4][M][64] bf16, dur [M][10], idx [5][M] int32,
 *            TOK [15][R][128] (slot 0 rows of t = first token, written by the caller), PRED [16][R][128],
 *            xhat [B][32][16][6] int64, plen [R] int32 (zeroed), force_pitch [15][R] or NULL, force_dur [5][M] or NULL,
 *            HN16 [16][R][512] bf16 or NULL, HD16 [6][M][64] bf16 or NULL (bf16 state copies for the backward; HD16 replaces HD[1..5]) }
 *     io[17] = NULL (timing experiments), io[18] = NULL or fp32 [B][2048] = [initial state | gc] of this time step (then io[0] is
 *     ignored and slot 0 of HN is written by the kernel); io[19] = xch, 8-byte words [ceil(B/16)][2][16][256], io[20] = cnt, uint32
 *     [ceil(B/16) + 1] ZEROED by the caller before the launch of t = 0 (cluster mode below; else NULL): io has 21 entries;
 *     with R = 32*B, M = 15*R; the rows of time step t are [t*B, (t+1)*B).  coin_mask bit n = feed the ground-truth note n+1
 *     (teacher-forcing coin, ptvae.py:420).  train = 0 skips what only the backward reads (HN, gates, HD, TOK); train = 2 stores only
 *     the fed tokens TOK: the caller then recomputes states and gates for ALL rows with the batched kernels (ptv_notes_gru_persist_fwd,
 *     ptv_dur_gru_fwd with the stored decisions forced), cheaper than 16-row panels streaming them out note step by note step.
 *     Bits 16 / 17 of train force the 4-wave kernel / the 8-wave kernel whose producer waves stream the next note step's state
 *     products under the head phases of the current one (default: by panel count).
 *     Bits 18-20 of train = S in {2, 4}, or bit 22 = eight members: cluster mode of the 4-wave kernel -- S workgroups (co-resident: ceil(B/16) * S <= the CU count, else
 *     PTV_ERR_UNSUPPORTED; together with bit 17, the 8-wave kernel: PTV_ERR_ARG) share a panel: each streams 1/S of the notes-GRU gate weights (the product bound by one CU's L2 port), the
 *     new bf16 state is all-gathered through xch once per note step as 8-byte words {2 units, step tag} that the readers poll
 *     (agent-scope stores / loads; xch = ceil(B/16) x 2 x 16 x 256 words = 64 KB per panel, ZEROED by the caller before t = 0; cnt counts
 *     arrivals for diagnostics; the launches of t = 0..31 must follow each other in order on one stream), heads / duration GRU /
 *     embedding are computed redundantly by all members and written by member 0.  cnt[ceil(B/16)] != 0 afterwards: a member gave up
 *     waiting (results void).
 *     Bit 21 of train: the 4-wave kernel streams the head weights from L2 every note step instead of keeping them in registers / LDS
 *     for the whole launch (the kernel before round 6; timing comparisons, bit-identical results).
 *     force_pitch / force_dur (replay mode of the tests, kept steps of a decode): PER DECISION.  Row t*B + b of force_pitch[n] holds the
 *     pitch decision of (b, t, note step n), row n*R + t*B + b of force_dur[d] duration bit d of that note; an entry >= 0 overrides the
 *     decision (the value is fed back and written out as if decided), A NEGATIVE ENTRY MEANS "FREE": the decision is taken as without
 *     the array -- argmax or draw.  The same holds for force_pitch of ptv_note_token*, force_idx of ptv_dur_out_token* and force of
 *     ptv_dur_gru_fwd*.  The words of a note step are requested at its top, before the cell's products; the members of a cluster read
 *     the same words.
 *   ptv_free_resummarize: w = { pack(W_ih), pack(W_hh), pack(W_ih_reverse), pack(W_hh_reverse), b_ih, b_hh, b_ih_r, b_hh_r } of
 *     dec_notes_emb_gru; io = { PRED, plen, XH fwd [17][R][128] (slot 0 zero), XH bwd, XG fwd [16][4][R][128] bf16, XG bwd,
 *     tok_next = TOKS[t+1] [B][256] }.  train bit 0: save states and gates (XH, XG) for the backward; bit 1: stream the weights from L2
 *     every step instead of keeping a wave's 48 fragments in registers for the launch (timing comparisons, bit-identical).
 */
long ptv_pack_mfma_b_size(int N, int K);
int ptv_pack_mfma_b(const float* W, long ld, int N, int K, void* out, int pairs, void* stream);
/* the same for a TRANSPOSED source (trans != 0: element (n, k) at W[k*ld + n]) and / or into the k-block sub-range [kb0, kb0 + ceil(K/32)) of
 * a packed buffer holding NT tiles x KBtot k-blocks (two sources side by side along K; rows n >= N and columns k >= K are zero) */
int ptv_pack_mfma_b2(const float* W, long ld, int N, int K, void* out, int pairs, int trans, int NT, int kb0, int KBtot, void* stream);
/* up to 8 such packs in ONE launch: jobs = n rows of 10 longs {W, ld, N, K, out, pairs, trans, NT, kb0, KBtot} (host array) */
int ptv_pack_mfma_multi(const long* jobs, int n, void* stream);
int ptv_free_note_loop(const void* const* w, const void* const* io, long ld_pitch, int B, int t, unsigned coin_mask, int train,
                       void* stream);
/* ------------------------------------------------------------------------------------------------
 * Sampled decode: seeded temperature sampling of the free-running decoder's pitch and duration decisions (DESIGN.md "Sampled decode").
 * The sampling block is 32 bytes of DEVICE memory { uint64 seed, uint64 draw, int64 sample_offset, float T_pitch, float T_dur } that the
 * kernels read when they run (a captured graph holds the pointer).  The pitch decision of (row b, time step t, note step n) is the first
 * maximal index over c < 130 of logit[c] + T_pitch * g[b, t, n, c]; duration bit d is 1 iff e1 + T_dur * g1 > e0 + T_dur * g0, with
 * g = -log(-log(u)) standard Gumbel, u = (top 23 bits of a Philox4x32-10 word + 1/2) * 2^-23, the word a pure function of (seed, draw,
 * sample_offset + b, t, n, kind, index) (csrc/philox.hpp).  T = 0 is the argmax, ties included.  The logits written out are the plain ones;
 * force_pitch / force_dur still override where their entry is >= 0 (a negative entry leaves the decision to the draw; a forced decision
 * leaves its noise words unused, nothing is re-keyed; under `ascending` a forced pitch is not checked but does update lo).  Inference only: with train != 0 or teacher-forcing coins every entry point returns PTV_ERR_ARG.
 *   ptv_free_note_loop: bit 23 of train announces the block as io[21] (io then has 22 entries; without the bit io[21] is not read).
 *   ptv_note_token_sample / ptv_dur_out_token_sample / ptv_dur_gru_fwd_sample: ptv_note_token / ptv_dur_out_token / ptv_dur_gru_fwd with the
 *     block and the position of the rows: row r is sample sample_offset + r at time step t; note step n = 0..14 for the duration forms,
 *     the duration bit d for ptv_dur_out_token_sample; ptv_note_token_sample decides note step n - 1 (its n is the slot it fills, 1..15).
 * Truncated sampling (top_k / min_p / top_p) bounds the support of the PITCH draw; the duration bits keep T_dur as their only control.  The
 * block is then 48 bytes: the 32 above unchanged, followed by { int32 top_k, float ln_min_p, uint32 top_p_q24, 4 reserved bytes (zero) }.
 *   top_k >= 1: class c is kept iff logit[c] >= v_k, the k-th largest of the row's 130 logits counted with multiplicity -- classes tied
 *     with the k-th value are ALL kept (so more than k may survive), whatever their column; top_k >= 130 keeps every class; 0 = off.
 *   ln_min_p = ln(min_p) rounded from float64 to fp32, min_p in (0, 1]: class c is kept iff logit[c] >= m + T_pitch * ln_min_p in fp32
 *     (the product rounded, then the sum), m the row's largest logit: p_c >= min_p * p_max under softmax(logits / T_pitch).  Any value
 *     > 0 (write 1.0f) = off: the kernels test the word and never multiply an infinity by T.
 *   top_p_q24 = round(top_p * 2^24) in [1, 2^24], top_p in (0, 1) (nucleus); 0 = off, which is what top_p = 1 is written as (the word was
 *     reserved and zero before: every block written then keeps its meaning).  Under softmax(logits / T_pitch) of the UNTRUNCATED row, keep
 *     the smallest set of best classes whose mass reaches top_p; classes tied with the last kept value are ALL kept (the tie rule of
 *     top_k).  As a threshold: the largest value t with mass{c: logit[c] >= t} >= top_p * Z; class c is kept iff logit[c] >= t, i.e. iff
 *     the mass of the classes strictly above it is < top_p * Z.  The masses are integers, so that every lane layout and every member of
 *     a cluster forms the same sums: w_c = trunc(e * 2^20), e = the device's fast fp32 exponential (v_exp_f32 of x * log2(e)) of
 *     x = (logit[c] - m) / T_pitch, the difference and the quotient each correctly rounded to fp32, m the row's largest logit (w = 2^20
 *     there; a class whose w is 0 carries no mass); Z = sum of w_c; the test is mass * 2^24 >= Z * top_p_q24 in 64-bit integers.
 *     T_pitch = 0: no nucleus rule (the decode is the argmax decode).
 *   Several rules: a class must pass every one, each judged on the untruncated row -- the largest of the thresholds.  This is NOT the
 *   sequential chain of other libraries (top_k first, then top_p on the renormalised survivors, ...).  All comparisons are fp32
 *   comparisons of the emitted logits (-0.0 == +0.0); the best class passes every rule, so the kept set is never empty.
 *   The decision is the first maximal index over the KEPT classes of logit + T_pitch * g with
 *   exactly the noise words above (a dropped class leaves its word unused, nothing is re-keyed): an exact draw from the renormalised
 *   truncated softmax, still a pure function of (seed, draw, global sample, t, n) and the row's logits.  T_pitch = 0 is the argmax.
 *   ptv_free_note_loop: bit 24 of train, together with bit 23, says io[21] is the 48-byte block; bit 24 without bit 23, with
 *     train & 3 != 0, a coin mask or a NULL block is PTV_ERR_ARG before any launch.
 *   ptv_note_token_sample_trunc: ptv_note_token_sample with the 48-byte block.
 *   ptv_decoder_free_fwd: PTV_DFF_D_SAMPLE_TRUNC != 0 says PTV_DFF_SAMPLE is the 48-byte block.
 * Constrained decode (pitch masks, ascending notes) restricts the SUPPORT of the pitch decision before any truncation.  The block is then 64
 * bytes: the 48 above unchanged, followed by { uint32 flags, uint32 reserved (zero), uint64 device address of the mask or 0 }.
 *   flags bit 0 (ascending): a pitch c < 128 is allowed iff c > lo, lo the largest pitch < 128 already decided in this time step (after
 *     force_pitch where it overrides; -1 at note step 0); <sos> (128) is never allowed.
 *   flags bit 1: the mask has one row [32, 4] that serves every row of the batch.
 *   mask: int32 [B, 32, 4] on the device, rows as the rows of the decoded batch (sample_offset moves only the noise): bit p & 31 of word
 *     p >> 5 of [b, t] set = grid pitch p (0..127) is allowed at time step t.  Classes 128 / 129 are not covered by it.
 *   <eos> (129) is always allowed, so the allowed set is never empty.  A disallowed class enters the truncation rules as -infinity: top_k
 *   counts the k best ALLOWED classes (fewer than k allowed: all of them), the nucleus mass, Z and min_p's maximum are those of the allowed
 *   classes.  The decision is the first maximal index of logit + T_pitch * g over the classes that are allowed and kept, with exactly the
 *   noise words above: an exact draw from the softmax renormalised over that set, a pure function of (seed, draw, global sample, t, n), the
 *   row's logits, its mask words and lo.  T_pitch = T_dur = 0 is the constrained argmax.  The emitted logits stay the plain ones.
 *   ptv_free_note_loop: bit 25 of train, together with bit 23, says io[21] is the 64-byte block (bit 24 then adds nothing); the guards of
 *     bit 24 apply.  The mask row of a sample is loaded once per launch.
 *   ptv_note_token_sample_cons: ptv_note_token_sample with the 64-byte block; M is the batch, row r takes mask row r.  xhat points at
 *     slot n of row 0 of a [M, 32, 16, 6] grid as in the other forms, and under `ascending` the slots 1 .. n - 1 before it are read.
 *   ptv_decoder_free_fwd: PTV_DFF_D_SAMPLE_CONS != 0 says PTV_DFF_SAMPLE is the 64-byte block.
 *   ptv_pitch_mask_build: mask [B, 32, 4] from a pitch range lo <= p <= hi (0, 127 = no restriction), a 12-bit pitch-class set (bit p % 12;
 *     0xfff = no restriction) and, unless NULL, the chroma of chroma [B, 8, 36] fp32: p at step t passes iff chroma[b, t / 4, 12 + p % 12]
 *     != 0.  The three are ANDed.  lo / hi outside 0 <= lo <= hi <= 127 or a set outside 0..0xfff: PTV_ERR_ARG.
 */
int ptv_note_token_sample(const float* pitch, long ld_pitch, const int* dur_idx, long dur_stride, const float* W, const float* bias, int E,
                          float* pred, long ld_pred, long* xhat, long xhat_stride, int* plen, int n, int last,
                          const int* force_pitch, int M, const void* sample, int t, void* stream);
int ptv_note_token_sample_trunc(const float* pitch, long ld_pitch, const int* dur_idx, long dur_stride, const float* W, const float* bias, int E,
                                float* pred, long ld_pred, long* xhat, long xhat_stride, int* plen, int n, int last,
                                const int* force_pitch, int M, const void* sample48, int t, void* stream);
int ptv_note_token_sample_cons(const float* pitch, long ld_pitch, const int* dur_idx, long dur_stride, const float* W, const float* bias, int E,
                               float* pred, long ld_pred, long* xhat, long xhat_stride, int* plen, int n, int last,
                               const int* force_pitch, int M, const void* sample64, int t, void* stream);
int ptv_pitch_mask_build(int* mask, long B, int lo, int hi, int pitch_classes, const float* chroma, void* stream);
/* Kept steps: the force arrays of a free-running decode that keeps some time steps of a grid and decides the rest (INTEGRATION.md "Kept
 * steps").  x: int64 [B][32][16][6], the model's grid (slot 0 <sos>, pitches 0..127, <eos> 129, <pad> 130; duration bits 0 / 1, 2 = pad);
 * steps: uint8 [steps_rows][32], steps_rows = 1 (one row serves every sample) or B; != 0 = time step kept.  For a kept (b, t): L = the first
 * slot s in 1..15 with x[b][t][s][0] == 129, else 15; for n < L force_pitch[n][t*B + b] = x[b][t][n+1][0] if that lies in 0..129, else -1 and
 * bit 0 of err[b] is set; force_dur[d][n*R + t*B + b] = x[b][t][n+1][1+d] if that is 0 or 1, else -1; n >= L and steps not kept: -1.
 * EVERY element of force_pitch [15][32B] and force_dur [5][480B] and every err[b] (int32 [B]) is written, by one thread each.
 * B < 1, steps_rows not in {1, B} or a NULL pointer: PTV_ERR_ARG before any launch. */
int ptv_keep_force_build(const long* x, const unsigned char* steps, int steps_rows, long B, int* force_pitch, int* force_dur, int* err,
                         void* stream);
/* Kept voices: the force arrays of a decode that keeps the LOWEST notes of a time step and decides the rest of it (csrc/keep.hip;
 * INTEGRATION.md "Kept voices").  The grammar orders the notes of a step by ascending pitch, so the lowest voice is a PREFIX of
 * the step's note decisions: the note loop is forced through it and goes on freely.  x as in "Kept steps".  mode: uint8 [mode_rows][32],
 * mode_rows = 1 (one row serves every sample) or B, per (b, t):
 *   0  the step is free: every word -1.
 *   1  the whole step is kept: ptv_keep_force_build's rule element for element, the <eos> included.
 *   2  the voice of the step is kept.  Scan the slots s = 1, 2, ..., 15 with K = 0; at each slot, in this order:
 *        (1) K == lowest[b][t]: stop;  (2) p = x[b][t][s][0]; p == 129: stop;  (3) p outside 0..127: set bit 0 of err[b] and stop (the bit's
 *        meaning in "Kept steps": a kept step held an unforcible pitch before its <eos>);  (4) p >= below[b][t]: stop;  (5) the note is
 *        kept: K += 1.
 *      For n < K force_pitch[n][t*B + b] = x[b][t][n+1][0] and force_dur[d][n*R + t*B + b] = x[b][t][n+1][1+d] where that is 0 or 1 (else
 *      -1) -- unless bit 0 of flags ("durations stay free") is set: then every duration word of a voice step is -1.  Every other word of
 *      the step is -1: the <eos> of a voice step is never forced, after the voice the decoder decides as without a keep and may add notes
 *      or end the step.
 *   any other value: the step is free and bit 1 of err[b] is set.
 * below / lowest: int32 [below_rows][32] / [lowest_rows][32], each with its own row count in {1, B}; NULL = no limit (its row count
 * must still be 1 or B).  below is clamped to 0..128 and lowest to 0..15 on the device; 128 / 15 are no limit.  flags: bit 0 as above (it does not
 * touch the steps of mode 1).  kept_n int32 [B][32] = the number of forced pitch decisions of the step (the >= 0 words of its force_pitch
 * column), in every mode.  EVERY element of force_pitch [15][32B], force_dur [5][480B], kept_n and err [B] is written, by one thread each.
 * ptv_grid_split_voice: the same selection as two model grids, voice and rest int64 [B][32][16][6].  Slot 0 of both is slot 0 of x; unused
 * slots are <pad> (130) with duration bits 2; an <eos> slot written here has duration bits 2.
 *   mode 2: voice = the K kept slots 1..K of x, then <eos> (none when K = 15); rest = the slots K+1.. of x moved down to slot 1, up to and
 *     including its first <eos>; where x holds none, all of them and, while a slot is left, an <eos> behind them.
 *   mode 1: voice = the step of x as it is (all 16 slots), rest = the empty step (<eos> in slot 1).  Mode 0 and any other value: the
 *     reverse.  kept_n and err are the builder's (flags = 0).
 * A NULL required pointer (below / lowest are optional), B < 1, a row count outside {1, B} or flags outside 0..1:
 * PTV_ERR_ARG before any launch. */
int ptv_keep_voice_force_build(const long* x, const unsigned char* mode, int mode_rows, const int* below, int below_rows, const int* lowest,
                               int lowest_rows, int flags, long B, int* force_pitch, int* force_dur, int* kept_n, int* err, void* stream);
int ptv_grid_split_voice(const long* x, const unsigned char* mode, int mode_rows, const int* below, int below_rows, const int* lowest,
                         int lowest_rows, long B, long* voice, long* rest, int* kept_n, int* err, void* stream);
/* Kept rhythm: a decode that keeps the number of notes of a time step, its rests and its durations, and draws the pitches again
 * (csrc/keep.hip; INTEGRATION.md "Kept rhythm").
 * PTV_FORCE_NOT_EOS (-2), a word of force_pitch: the decision is FREE, but <eos> (129) is not in its support unless nothing else is.  <eos>
 *   leaves the allowed set of that decision iff at least one other class is allowed (after the mask, after `ascending`, never <sos> under
 *   `ascending`, columns < 130).  If no other class is allowed <eos> stays: the allowed set is never empty, the step ends short, and nothing
 *   reports it at decode time -- count the notes.  The removal is part of the allowed rule, so it precedes every truncation: top_k, the
 *   nucleus mass, min_p's maximum and Z are those of the allowed classes without <eos>.  T_pitch = 0: the argmax over that set.  Every other
 *   negative word, -1 included, is a plainly free decision as before.
 *   ONLY the constrained kind (64-byte block: bit 25 of ptv_free_note_loop's train word, ptv_note_token_sample_cons, PTV_DFF_D_SAMPLE_CONS,
 *   sample_bytes = 64 of ptv_decode_logprob) honours the word.  A -2 that reaches an argmax, sampled or truncated kernel is a free decision
 *   like -1: send a decode with such words as the constrained kind (flags 0 and no mask constrain nothing).
 *   ptv_decode_logprob: a -2 decision counts as free, its log q is taken over the same reduced support (a decided <eos> outside it sets
 *   bit 0 of err); log p is untouched.
 * ptv_keep_rhythm_force_build: the force arrays.  x as in "Kept steps"; mode: uint8 [mode_rows][32], mode_rows = 1 or B, per (b, t):
 *   0  the step is free: every word -1.
 *   1  the whole step is kept: ptv_keep_force_build's rule element for element.
 *   3  the rhythm of the step is kept.  L = the first slot s in 1..15 with x[b][t][s][0] == 129, else 15 (the rule of "Kept steps");
 *      K = L - 1 notes, or 15 where the step holds no <eos>.  For n < K force_pitch[n][t*B + b] = PTV_FORCE_NOT_EOS and
 *      force_dur[d][n*R + t*B + b] = x[b][t][n+1][1+d] where that is 0 or 1 (else -1) -- unless bit 0 of flags ("pitches only") is set:
 *      then every duration word of a rhythm step is -1.  For n = K < 15 force_pitch[n] = 129 (the step ends exactly there) with duration
 *      words -1.  Every other word of the step is -1.  K = 0 keeps a rest.  A slot before L whose pitch lies outside 0..127 still counts
 *      as a note position (-2) and sets bit 0 of err[b].
 *   any other value: the step is free and bit 1 of err[b] is set.
 * kept_n int32 [B][32]: K at a rhythm step, the number of forced pitch decisions at a whole step, 0 at a free step.  EVERY element of
 * force_pitch [15][32B], force_dur [5][480B], kept_n and err [B] is written, by one thread each.  A NULL pointer, B < 1, mode_rows outside
 * {1, B} or flags outside 0..1: PTV_ERR_ARG before any launch. */
#define PTV_FORCE_NOT_EOS (-2)
int ptv_keep_rhythm_force_build(const long* x, const unsigned char* mode, int mode_rows, int flags, long B, int* force_pitch, int* force_dur,
                                int* kept_n, int* err, void* stream);
/* Kept top voice: a decode that keeps the HIGHEST notes of a time step -- a suffix of its note decisions -- and its note count, and draws
 * the notes under them again (csrc/keep.hip; INTEGRATION.md "Kept top voice").
 * PTV_FORCE_BELOW(u) = -256 - u, u in 1..128 (the words -257..-384 of force_pitch): the decision is FREE, is never <eos>, and its pitch is a
 *   note strictly below the ceiling u.  The rule is part of the allowed rule: after the mask and `ascending`, before every truncation
 *   (top_k, the nucleus mass, min_p's maximum and Z are those of the set below).  With lane = the notes c < 128 with c < u -- under the
 *   `ascending` flag also c > lo -- the allowed set of the decision is
 *     lane & mask   if that is not empty;
 *     lane          if it is: the mask yields, so the step neither ends short nor loses the notes kept behind this decision;
 *     {<eos>}       if lane itself is empty.  Only hand-made words get here: the builder emits no such ceiling on a grid that raises no err bit.
 *   <sos> and <eos> are in no other case part of it.  T_pitch = 0: the argmax over that set.  Every other negative word keeps its meaning:
 *   -2 is PTV_FORCE_NOT_EOS, -1 and any other value are plainly free.
 *   ONLY the constrained kind honours the word, at the sites that honour PTV_FORCE_NOT_EOS (see "Kept rhythm"); anywhere else it is a free
 *   decision like -1.  ptv_decode_logprob: such a decision counts as free, its log q is taken over the same set, relaxed or not (a decided
 *   class outside it sets bit 0 of err); log p is untouched.
 * ptv_keep_top_force_build: the force arrays.  x as in "Kept steps"; mode: uint8 [mode_rows][32], mode_rows = 1 or B, per (b, t):
 *   0  the step is free: every word -1.
 *   1  the whole step is kept: ptv_keep_force_build's rule element for element.
 *   4  the top of the step is kept.  L = the first slot s in 1..15 with x[b][t][s][0] == 129, else 15 (the rule of "Kept steps"); K = L - 1
 *      notes, or 15 where the step holds no <eos>.  The kept notes are the last h of them: from slot K downwards, stop at h == highest
 *      (int32 [highest_rows][32], clamped to 0..15), at a pitch outside 0..127 and at the first pitch < above (int32 [above_rows][32],
 *      clamped to 0..128).  A NULL limit does not limit; both NULL: h = min(1, K), the very top note.  J = K - h.
 *      n < J:       force_pitch[n][t*B + b] = PTV_FORCE_BELOW(u_n), u_n clamped into 1..128.  Bit 1 of flags clear ("lanes"): u_n = the
 *                   pitch of x's next note, x[b][t][n+2][0] (128 behind the last note): no re-drawn voice crosses its old upper neighbour.
 *                   Bit 1 set ("room"): u_n = p_J - (J - 1 - n), p_J the lowest kept pitch, 128 where h = 0: a semitone for each decision
 *                   still to come.  Under the `ascending` flag either leaves lane non-empty at every decision, whatever was drawn before
 *                   it, if the step ascends strictly: the decode has K notes and the kept ones sit in their slots.
 *      J <= n < K:  force_pitch = x's pitch.     n = K < 15: force_pitch = 129.     n > K: -1.
 *      force_dur[d][n*R + t*B + b] = x[b][t][n+1][1+d] where that is 0 or 1 (else -1) for n < K; with bit 0 of flags set only for
 *      J <= n < K (the durations under the kept notes are drawn).  Every other duration word of the step is -1.
 *      Bit 0 of err[b]: a slot 1..K of a top step of the sample holds a pitch outside 0..127, or one not above the slot before it.
 *   any other value: the step is free and bit 1 of err[b] is set.
 * kept_n int32 [B][32]: h at a top step, the number of forced pitch decisions at a whole step, 0 at a free step.  EVERY element of
 * force_pitch [15][32B], force_dur [5][480B], kept_n and err [B] is written, by one thread each.  A NULL pointer (but above / highest),
 * B < 1, a row count outside {1, B} or flags outside 0..3: PTV_ERR_ARG before any launch.
 * ptv_grid_split_top: the same selection as two model grids, voice and rest int64 [B][32][16][6], as ptv_grid_split_voice's.  A top step:
 * voice = the h kept notes, <eos>, <pad>; rest = the J notes under them, <eos>, <pad> (rest's notes followed by voice's are x's).  A whole
 * step: voice = the step, rest = the empty step; a free step the other way round.  kept_n and err as above. */
#define PTV_FORCE_BELOW(u) (-256 - (u))
int ptv_keep_top_force_build(const long* x, const unsigned char* mode, int mode_rows, const int* above, int above_rows, const int* highest,
                             int highest_rows, int flags, long B, int* force_pitch, int* force_dur, int* kept_n, int* err, void* stream);
int ptv_grid_split_top(const long* x, const unsigned char* mode, int mode_rows, const int* above, int above_rows, const int* highest,
                       int highest_rows, long B, long* voice, long* rest, int* kept_n, int* err, void* stream);
/* Duration limits: a decode whose notes have durations in a range per (sample, time step) -- "nothing longer than a beat", "nothing shorter
 * than an eighth", "no note across the bar line" -- while the decoder still chooses inside the range and feeds its choice back
 * (csrc/keep.hip, csrc/philox.hpp; INTEGRATION.md "Duration limits").
 * A note's duration is D = v + 1, v the 5-bit value of its duration bits, bit 0 the most significant.
 * PTV_FORCE_DUR_RANGE(lo, hi) = -1024 - (lo | hi << 5), 0 <= lo <= hi <= 31 (the words -1024..-2047 of force_dur): the decision is FREE and
 *   v ends in [lo, hi].  It is negative, so every "forced?" test answers as before; -1 and every other negative word stay plainly free.
 *   ALL FIVE planes of one decision (n, row) hold the same word.  The rule of bit d, with p = the value of the bits 0..d-1 decided for the
 *   note: value b is allowed iff [q << (4-d), (q << (4-d)) + (1 << (4-d)) - 1], q = 2p + b, meets [lo, hi].
 *     one value allowed:  that is the decision; its noise words stay unused.
 *     both allowed:       the decision is what it is without the word: the first maximum of logit + T_dur * g, same noise words.
 *     neither allowed:    (forced bits mixed into the decision) the bit is plainly free.  A hand-made word with lo > hi is no range word.
 *   A word >= 0 overrides everything.  The logits stored are the plain logits.  The draw is the model's own bit-by-bit chain with the
 *   infeasible branches removed -- NOT the joint distribution of the 32 durations renormalised over the range.
 *   ONLY the constrained kind honours the word, at the duration decisions of the SAMP = 3, FORCE = 1 note loops,
 *   ptv_dur_gru_fwd_sample_cons / ptv_dur_out_token_sample_cons (the constrained step loop with force arrays) and ptv_decode_logprob;
 *   anywhere else it is a free decision like -1.  ptv_decode_logprob (64-byte block): a bit the word determines adds its model
 *   log-probability to log p, 0 to log q, and counts with the forced decisions (a decided value the range excludes sets bit 0 of err); a
 *   bit with both values allowed is a free decision as ever.
 * ptv_dur_range_force_build: the force arrays.  lo / hi: uint8 [rows][32] in DURATIONS 1..32 (rows = 1 or B, each its own), steps: uint8
 *   [steps_rows][32], non-zero = the limits apply at that (b, t).  Per (b, t): H = hi clamped into 1..32, F = max(lo, 1), L = min(F, H) --
 *   the ceiling wins -- and yielded[b][t] (int32 [B][32]) = 1 iff the step is selected and F > H, else 0.
 *   src_pitch / src_dur: the arrays of an existing keep to build INTO, or both NULL (= every word -1); they may not be the outputs.
 *   force_pitch [15][32B] = src_pitch.  For each of the 15 decisions (n, t*B + b) of a selected step whose five words of src_dur are ALL
 *   negative, all five planes of force_dur [5][480B] get PTV_FORCE_DUR_RANGE(L - 1, H - 1) (a range word already there is replaced); every
 *   other word is src_dur's, bit for bit.  EVERY element of the three outputs is written, by one thread each.  A NULL pointer (but the
 *   src pair), one of the pair alone, an output that is its source, B < 1 or a row count outside {1, B}: PTV_ERR_ARG before any launch. */
#define PTV_FORCE_DUR_RANGE(lo, hi) (-1024 - ((lo) | (hi) << 5))
int ptv_dur_range_force_build(const unsigned char* lo, int lo_rows, const unsigned char* hi, int hi_rows, const unsigned char* steps,
                              int steps_rows, const int* src_pitch, const int* src_dur, long B, int* force_pitch, int* force_dur, int* yielded,
                              void* stream);
/* Note-count limits: a decode whose time steps have a number of notes in a range per (sample, time step) -- "at most four notes per step",
 * "at least a dyad on every beat", "rests on the off-beats", "notes exactly on this onset pattern" -- with no grid to copy the count from
 * (csrc/keep.hip; INTEGRATION.md "Note-count limits").  The count-side twin of "Duration limits": no new word, the builder
 * writes a forced <eos> (129), PTV_FORCE_NOT_EOS and PTV_FORCE_BELOW(u) from limits instead of from a grid.
 * ptv_note_count_force_build: the force arrays.  lo / hi: uint8 [rows][32] in NOTE COUNTS (rows = 1 or B, each its own), steps: uint8
 *   [steps_rows][32], non-zero = the step is SELECTED.  src_pitch / src_dur: the arrays of an existing keep to build INTO, or both NULL
 *   (= every word -1); they may not be the outputs.  flags: bit 0 = "room" (below).  Per (b, t) of a selected step:
 *   F = lo and H = hi, each clamped into 0..15; the ceiling wins: L = min(F, H).  w[n], n = 0..14: the step's words of src_pitch.
 *   Owned step: some w[n] is 129, or is a negative word other than -1 (the keep already fixes this step's count: whole, rhythm and top
 *     steps).  The step is copied bit for bit and bit 1 (value 2) of yielded[b][t] is set.
 *   Otherwise: J = 1 + the index of the last w[n] >= 0, or 0 with none (the forced prefix of a kept voice); E = max(H, J).  Only words
 *     equal to -1 are ever replaced.
 *     Floor:   for n < L with w[n] == -1 the word is PTV_FORCE_NOT_EOS, or with the room flag PTV_FORCE_BELOW(128 - (L - 1 - n)).
 *              Under `ascending` the room ceilings guarantee the floor: decision n lies at or below 128 - L + n, so decision n + 1 always
 *              has a note left; with a mask the BELOW rule lets the mask yield, never the count.
 *              WITHOUT the room flag a floor is "not <eos> while anything else is allowed", the meaning PTV_FORCE_NOT_EOS already has:
 *              under a narrow mask or `ascending` the allowed set can shrink to <eos> alone and the count FALLS SHORT of L; nothing
 *              reports it at decode time -- count the notes.
 *     Ceiling: if E <= 14 and w[E] == -1, w[E] = 129.  H = 0 makes the step a rest; H = 15 is no ceiling.  A forced <eos> behind a step
 *              that already ended is inert: the note loop decides nothing behind the first <eos> of a step.
 *     yielded[b][t] (int32 [B][32]) bits: bit 0 (1): F > H.  bit 2 (4): J > H, the prefix is longer than the ceiling and the <eos>
 *              follows the prefix.  bit 3 (8): room flag set, 0 < J < L and the prefix's last forced pitch p (0..127) has
 *              p + 1 >= 128 - (L - 1 - J): the floor may fall short above that voice.
 *   Unselected step: copied, yielded = 0.  Duration words are src_dur's (or -1) everywhere.
 *   Without a floor (L = 0 everywhere) only plain forced <eos> words are written, which every decode kind honours; PTV_FORCE_NOT_EOS and
 *   PTV_FORCE_BELOW are honoured ONLY by the constrained kind, and the room ceilings leave room only for notes that ascend.
 *   EVERY element of force_pitch [15][32B], force_dur [5][480B] and yielded is written, by one thread each.  A NULL pointer (but the src
 *   pair), one of the pair alone, an output that is its source, flags outside 0..1, B < 1 or a row count outside {1, B}: PTV_ERR_ARG
 *   before any launch. */
int ptv_note_count_force_build(const unsigned char* lo, int lo_rows, const unsigned char* hi, int hi_rows, const unsigned char* steps,
                               int steps_rows, const int* src_pitch, const int* src_dur, int flags, long B, int* force_pitch, int* force_dur,
                               int* yielded, void* stream);
/* Sounding state: restrictions that depend on what the decode itself decided at earlier time steps -- "do not strike a key that is still
 * down", "at most four voices", "never silent" (csrc/sounding.hip; INTEGRATION.md "Sounding state").  A launch of the note
 * loop decides ONE time step and reads that step's mask row and force words from memory, so the rule is one small launch between two note
 * loops that writes the next step's row and words; no decode kernel knows of it.
 * Accepted notes of a step s of row b: the slots 1..15 of xhat[b][s] in order, up to the first pitch 129.  A slot whose pitch lies outside
 *   0..127 is skipped.  The duration is d = 1 + the five bit columns read most significant first (v & 1 of each), cut to min(d, 32 - s)
 *   (ptv_grid_to_pr's parse).
 * State: rem uint8 [B][128], zero before step 0.  After step s is decided: rem[p] = max(rem[p] - 1, 0) for every p; then for each accepted
 *   note (p, d) in slot order rem[p] = d - 1 -- a later onset of a pitch replaces the earlier one, as in the piano-roll.  The held set
 *   going into step s + 1 is H = {p : rem[p] > 0}, h = |H|; held[b][s + 1] = h and held[b][0] = 0 (int32 [B][32]).
 * The effective step s + 1 of a SELECTED (row, step) (steps uint8 [rows][32], non-zero = selected), from the caller's base mask row and
 *   base pitch force words w[0..14]:
 *   no_restrike (bit 0 of the control word, a uint32 in DEVICE memory): mask_eff = mask_base & ~bits(H).  It is a pitch mask like any
 *     other: a forced pitch is never checked against it, and where PTV_FORCE_BELOW lets a mask yield this one yields too.
 *   max_sounding K (uint8 [rows][32]: 1..127, 0 = none) and min_sounding F (uint8 [rows][32]: 0..15) count SOUNDING pitches: with
 *     H' = clamp(K - h, 0, 15) (15 where K is 0) and F' = clamp(F - h, 0, 15) the step's words are what ptv_note_count_force_build's rule
 *     makes of lo = F', hi = H' without the room flag -- an owned step is copied, J is the forced prefix, E = max(H', J), only words equal
 *     to -1 are replaced, the ceiling wins.  Duration words are never touched.  At a selected step that the keep does not own,
 *     onsets + h <= K whenever J <= H'; kept notes win over the cap as they win over the note-count limits.  A floor is "not <eos> while
 *     anything else is allowed": nothing guarantees it.
 *   An unselected step gets the base row and the base words.  The state is tracked at every step regardless.
 * ptv_sounding_step: one launch takes t_done in -1..30 and writes everything of step t_done + 1: rem, mask_eff[b][t_done + 1][0..3], the
 *   15 words of row (t_done + 1) * B + b of force_eff [15][32B], held[b][t_done + 1] -- every element by one writer, nothing of any other
 *   step.  t_done = -1 reads no grid (xhat may be NULL) and writes zeros to rem: the first call initialises the state.
 *   xhat: int64 [B][32][16][6], the grid the decode writes.  mask_base: int32 [mask_rows][32][4], or NULL = every pitch allowed;
 *   force_base: int32 [15][32B], or NULL = every word -1; max_sounding / min_sounding / steps: each with its own row count in {1, B}.
 *   mask_eff int32 [B][32][4] or NULL (then mask_base must be NULL: no mask rule is written); force_eff int32 [15][32B] or NULL (then
 *   force_base must be NULL: no count rule is on).  The note loop of step t_done + 1 is handed the EFFECTIVE arrays.
 *   A NULL required pointer (max_sounding, min_sounding, steps, control, rem, held; xhat unless t_done = -1), a base table without its
 *   output, an output that is its source, a row count outside {1, B}, B < 1 or t_done outside -1..30: PTV_ERR_ARG before any launch. */
int ptv_sounding_step(const long* xhat, int t_done, long B, const int* mask_base, int mask_rows, const int* force_base,
                      const unsigned char* max_sounding, int max_rows, const unsigned char* min_sounding, int min_rows,
                      const unsigned char* steps, int steps_rows, const unsigned* control, unsigned char* rem, int* mask_eff,
                      int* force_eff, int* held, void* stream);
/* the duration entries of the constrained step loop with force arrays: as the two below, and a word PTV_FORCE_DUR_RANGE of force / force_idx
 * limits the note.  ptv_dur_out_token_sample_cons: idx is plane d of the decisions, the planes of the bits before it lie idx_stride words
 * apart below it (idx - k * idx_stride, k = 1..d, written by the calls before).  idx and the force array must be given. */
int ptv_dur_out_token_sample_cons(const float* h, int H, const float* w_out, const float* b_out, float* dur_out, long ld_out,
                                  int* idx, long idx_stride, const int* force_idx, long rows, const void* sample, int t, int n, int d,
                                  void* stream);
int ptv_dur_gru_fwd_sample_cons(int H, long M, const float* h0, long ld_h0, const float* w_hh, const float* b_hh,
                                const float* tab0, const float* tab, const float* w_out, const float* b_out,
                                float* hall, long plane_h, void* hall16, void* gates, long plane_g, long step_g, int gates_bf16,
                                float* dur_out, long ld_out, int* idx, long idx_stride, const int* force, long force_stride,
                                const void* sample, int t, int n, void* stream);
int ptv_dur_out_token_sample(const float* h, int H, const float* w_out, const float* b_out, float* dur_out, long ld_out,
                             int* idx, const int* force_idx, long rows, const void* sample, int t, int n, int d, void* stream);
int ptv_dur_gru_fwd_sample(int H, long M, const float* h0, long ld_h0, const float* w_hh, const float* b_hh,
                           const float* tab0, const float* tab, const float* w_out, const float* b_out,
                           float* hall, long plane_h, void* hall16, void* gates, long plane_g, long step_g, int gates_bf16,
                           float* dur_out, long ld_out, int* idx, long idx_stride, const int* force, long force_stride,
                           const void* sample, int t, int n, void* stream);
/* Per-row sampling: a decode whose rows each have their own sampling rule -- a batch of requests that differ in temperature, top_k,
 * min_p or top_p, or a sweep of one z over several settings, decoded as ONE batch (csrc/philox.hpp SampleBlockR; INTEGRATION.md "Per-row
 * sampling").  The ROW-WISE kind is the constrained kind with the six scalars of its block replaced by one record per row;
 * everything the constrained kind honours stays: the pitch mask and the ascending flag, every force word (forced classes,
 * PTV_FORCE_NOT_EOS, PTV_FORCE_BELOW(u), PTV_FORCE_DUR_RANGE(lo, hi)), <eos> always allowed, constraints before truncation.
 * Block: 80 bytes, ten int64 words.  The first 64 are laid out as the constrained block; then { uint64 device address of the row table,
 *   uint32 reserved (zero), uint32 reserved (zero) }.  Of the first 64 bytes the row-wise kernels read only seed, draw, flags and mask;
 *   the host writes T_pitch = T_dur = 0, top_k = 0, ln_min_p = 1.0f (off), top_p_q24 = 0 and sample_offset = 0 there.
 * Row table: int32 [B, 8] on the device, contiguous, 16-byte aligned, 32 bytes per row (two 16-byte loads), row b of the decoded batch:
 *   words 0..4 = { float T_pitch, float T_dur, int32 top_k (0 = off), float ln_min_p (1.0f = off), uint32 top_p_q24 (0 = off) } -- the
 *   encodings of the scalar block, bit for bit; word 5 = reserved (zero); words 6..7 = int64 sample_id, the global sample index g of the
 *   Philox counter in place of sample_offset + b, range [0, 2^47).  seed and draw stay shared: sample_id already gives every row its own
 *   stream.  Row b decides exactly as row b of a constrained decode whose block holds b's five words and sample_offset = sample_id[b] - b:
 *   the same logits, the same noise words, the same decisions, bit for bit.
 * A row's record is loaded once per launch by the lanes that decide for the row; rows past B are clamped like every other per-row load.
 * Where 16 lanes hold a row (the note loops) the four rows of a wave take their own branches of the keep rule; the rule's cross-lane
 * steps stay inside the row.
 *   ptv_free_note_loop: bit 26 of train, together with bit 23, says io[21] is the 80-byte block (bits 24 / 25 then add nothing); the
 *     guards of bit 25 apply: bit 26 without bit 23, with train & 3 != 0, a coin mask or a NULL block is PTV_ERR_ARG before any launch.
 *     (Bits 0-1, 8-15, 16-25 of the word are taken; 26 was free.)
 *   ptv_note_token_sample_rows: ptv_note_token_sample_cons with the 80-byte block; row r takes mask row r and record r.
 *   ptv_dur_gru_fwd_sample_rows / ptv_dur_out_token_sample_rows: the duration entries of the row-wise step loop -- row r draws with T_dur and
 *     sample_id of record r; a word PTV_FORCE_DUR_RANGE of force / force_idx limits the note as in the _cons forms, and the force array may
 *     be NULL (every decision free).  ptv_dur_out_token_sample_rows reads the planes idx - k * idx_stride, k = 1..d, like its _cons form.
 *   ptv_decoder_free_fwd: PTV_DFF_D_SAMPLE_ROWS != 0 says PTV_DFF_SAMPLE is the 80-byte block.
 *   ptv_decode_logprob: sample_bytes = 80 takes T_pitch, T_dur and the truncation words from record b (one workgroup is one sample); log q
 *     of a row-wise decode is the log-probability under that row's own proposal. */
int ptv_note_token_sample_rows(const float* pitch, long ld_pitch, const int* dur_idx, long dur_stride, const float* W, const float* bias, int E,
                               float* pred, long ld_pred, long* xhat, long xhat_stride, int* plen, int n, int last,
                               const int* force_pitch, int M, const void* sample80, int t, void* stream);
int ptv_dur_out_token_sample_rows(const float* h, int H, const float* w_out, const float* b_out, float* dur_out, long ld_out,
                                  int* idx, long idx_stride, const int* force_idx, long rows, const void* sample80, int t, int n, int d,
                                  void* stream);
int ptv_dur_gru_fwd_sample_rows(int H, long M, const float* h0, long ld_h0, const float* w_hh, const float* b_hh,
                                const float* tab0, const float* tab, const float* w_out, const float* b_out,
                                float* hall, long plane_h, void* hall16, void* gates, long plane_g, long step_g, int gates_bf16,
                                float* dur_out, long ld_out, int* idx, long idx_stride, const int* force, long force_stride,
                                const void* sample80, int t, int n, void* stream);
int ptv_free_resummarize(const void* const* w, const void* const* io, int B, int t, int train, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ptv_decoder_free_fwd (COMPOSITE, round 6; SURVEY.md 8b's decoder_free_fwd): the forward of the free-running / scheduled-sampling
 * PianoTree decoder as ONE call -- PtvaeDecoder.decoder with teacher-forcing coins (ptvae.py:430-496), decode_notes / decode_note
 * (:336-428) and the re-summarisation of the predicted notes (:476-486): what train.py's schedule runs from its third batch on
 * (scheduler.py:48-54, train.py:23-24,59-63) and what inference_decode always runs (model.py:124-131).  The launch sequence of
 * functional_free.DecoderStepFn.forward's persistent path, bit-identical to it:
 *   prologue   z -> initial time state, z_in, its gate contribution; first time token; first note token
 *   32 x       time-GRU input product, time-GRU cell (ptv_gru_step_fwd), [initial notes state | hoisted input part] in one product,
 *              ptv_free_note_loop (all 15 note steps of the time step), then the next time token: the ground-truth summary (time coin) or
 *              ptv_free_resummarize over the predicted notes
 *   recompute  (training, D_REPLAY) what the batched backward reads, for all 480*B rows at once by the teacher-forced kernels on the
 *              recorded tokens with the stored duration decisions forced: hoisted input part, notes GRU (ptv_notes_gru_persist_fwd),
 *              dur_hid, the duration GRU (ptv_dur_gru_fwd), and the re-summarisation bi-GRU (ptv_row_gru_persist_fwd x 2)
 * bf16 precision at the init_model() sizes (E = 128, He = 128, Hn = 512, Hd = 64, 130 pitches): anything else returns
 * PTV_ERR_UNSUPPORTED before the first launch.  t: pointer table (enum PtvDffTensor; the caller owns every tensor), d: dimension table
 * (enum PtvDffDim).  wl / io: the HOST pointer arrays of ptv_free_note_loop (io[18] = the H0GC scratch), wr / ior: those of
 * ptv_free_resummarize (ior[6] is overwritten per time step with TOKS[t + 1]).  note_mask: HOST [32] -- bit n of word t = note coin n of
 * time step t (ptvae.py:420); time_coin: HOST [31] bytes -- time step t + 1 is fed the ground-truth summary (ptvae.py:476).
 * The autograd backward of this node is ptv_decoder_tf_bwd on the recorded tokens plus the routing of the token gradients
 * (ptv_route_slices) and ptv_bigru_rows_bwd over the predicted notes: functional_free.DecoderStepFn.backward.
 */
enum PtvDffTensor {
  PTV_DFF_Z = 0,            /* [B, Zs] fp32 */
  PTV_DFF_XS,               /* [32 B, 2He] fp32 ground-truth note summaries, or NULL (inference / no time coin set) */
  PTV_DFF_TOK0_SRC,         /* first note token of every time step: [R, E] rows (the embedded ground-truth slot 0) or ONE row (<sos>, D_TOK0_LDS = 0) */
  /* parameters (fp32) and their operand copies */
  PTV_DFF_W_ZHID, PTV_DFF_B_ZHID, PTV_DFF_W_ZIN, PTV_DFF_B_ZIN, PTV_DFF_W_IH_T, PTV_DFF_B_IH_T, PTV_DFF_INIT_INPUT, PTV_DFF_B_HH_T,
  PTV_DFF_W_IH_T_OP,        /* dec_time_gru.weight_ih_l0 as the per-step product's operand: bf16 shadow (D_W_IH_T_BF16) or the fp32 weight */
  PTV_DFF_W_HH_T_OP,        /* dec_time_gru.weight_hh_l0 likewise (D_W_HH_T_BF16) */
  PTV_DFF_W_CAT, PTV_DFF_B_CAT,   /* [dec_time_to_notes_hid ; dec_notes_gru.weight_ih[:, :Ht]] bf16 [Hn + 3Hn, Ht] and its bias fp32 */
  /* recompute block (D_REPLAY): fp32 weights + packs */
  PTV_DFF_W_IH_N, PTV_DFF_B_IH_N, PTV_DFF_B_HH_N, PTV_DFF_W_DH, PTV_DFF_B_DH, PTV_DFF_W_HH_D, PTV_DFF_B_HH_D, PTV_DFF_TAB0, PTV_DFF_TAB,
  PTV_DFF_W_OUT_D, PTV_DFF_B_OUT_D, PTV_DFF_PK_NOTES_H, PTV_DFF_PK_NOTES_T,
  PTV_DFF_PK_E_H0, PTV_DFF_PK_E_T0, PTV_DFF_B_HH_E0, PTV_DFF_B_IH_E0, PTV_DFF_PK_E_H1, PTV_DFF_PK_E_T1, PTV_DFF_B_HH_E1, PTV_DFF_B_IH_E1,
  /* state / outputs */
  PTV_DFF_NS, PTV_DFF_NS16, PTV_DFF_Z_IN, PTV_DFF_ZG, PTV_DFF_TOKS, PTV_DFF_GATES_T,
  PTV_DFF_GI, PTV_DFF_H0GC,          /* scratch [B, 3Ht] / [B, Hn + 3Hn] fp32, reused by every time step */
  PTV_DFF_TOK, PTV_DFF_PRED, PTV_DFF_PITCH, PTV_DFF_HN, PTV_DFF_HN16, PTV_DFF_GATES_N, PTV_DFF_HD, PTV_DFF_HD16, PTV_DFF_GATES_D,
  PTV_DFF_IDX, PTV_DFF_PLEN, PTV_DFF_GC16, PTV_DFF_DUR_SCR, PTV_DFF_IDX_SCR,
  PTV_DFF_XH0, PTV_DFF_XH1, PTV_DFF_XH16_0, PTV_DFF_XH16_1, PTV_DFF_XG0, PTV_DFF_XG1,
  PTV_DFF_WAIT_EVENT, PTV_DFF_RECORD_EVENT,   /* hipEvent_t or NULL: the persistent-launch turn around the cluster-mode note loops */
  PTV_DFF_SAMPLE,           /* NULL, or the sampling block of a sampled decode (32 bytes on the device, 48 with D_SAMPLE_TRUNC, 64 with D_SAMPLE_CONS, 80 with D_SAMPLE_ROWS; "Sampled decode" above): D_INFERENCE only,
                             * anything else is PTV_ERR_ARG before the first launch */
  /* the sounding state ("Sounding state" above): with D_SND != 0 the call runs ptv_sounding_step(-1) before the loop and
   * ptv_sounding_step(ts) behind every note loop for ts < 31, on the call's own stream.  The caller hands the note loop the EFFECTIVE arrays
   * itself: io[13] is SND_FORCE_EFF (where given) and the block's mask address is SND_MASK_EFF (where given); the grid is io[11] */
  PTV_DFF_SND_MASK_BASE, PTV_DFF_SND_FORCE_BASE,      /* the base tables, or NULL */
  PTV_DFF_SND_MAX, PTV_DFF_SND_MIN, PTV_DFF_SND_STEPS, PTV_DFF_SND_CONTROL, PTV_DFF_SND_REM,
  PTV_DFF_SND_MASK_EFF, PTV_DFF_SND_FORCE_EFF, PTV_DFF_SND_HELD,
  PTV_DFF_COUNT
};
enum PtvDffDim {
  PTV_DFF_D_B = 0, PTV_DFF_D_ZS, PTV_DFF_D_ZI, PTV_DFF_D_HE, PTV_DFF_D_HT, PTV_DFF_D_HN, PTV_DFF_D_HD, PTV_DFF_D_E, PTV_DFF_D_NP,
  PTV_DFF_D_LDP,            /* row stride of the pitch logits */
  PTV_DFF_D_TRAIN, PTV_DFF_D_REPLAY, PTV_DFF_D_INFERENCE,
  PTV_DFF_D_LOOP_FLAGS,     /* the `train` word of ptv_free_note_loop (mode, kernel choice, cluster size); in cluster mode the call zeroes io[19] / io[20] itself */
  PTV_DFF_D_CLUSTER,        /* != 0: the note loops take the persistent-launch turn (WAIT / RECORD events) */
  PTV_DFF_D_RESUM_TRAIN,    /* the `train` word of ptv_free_resummarize */
  PTV_DFF_D_TOK0_LDS,       /* row stride of TOK0_SRC (0 = one row for all) */
  PTV_DFF_D_W_IH_T_BF16, PTV_DFF_D_W_HH_T_BF16,
  PTV_DFF_D_SAMPLE_TRUNC,   /* != 0: PTV_DFF_SAMPLE is the 48-byte block of a truncated sampled decode (top_k / min_p / top_p); without PTV_DFF_SAMPLE: PTV_ERR_ARG */
  PTV_DFF_D_SAMPLE_CONS,    /* != 0: PTV_DFF_SAMPLE is the 64-byte block of a constrained decode (pitch mask / ascending notes); without PTV_DFF_SAMPLE: PTV_ERR_ARG */
  PTV_DFF_D_SAMPLE_ROWS,    /* != 0: PTV_DFF_SAMPLE is the 80-byte block of a row-wise decode ("Per-row sampling"); without PTV_DFF_SAMPLE: PTV_ERR_ARG */
  PTV_DFF_D_SND,            /* != 0: the sounding state is tracked (the PTV_DFF_SND_* slots); D_INFERENCE only -- with D_TRAIN, D_REPLAY or a coin: PTV_ERR_ARG.  0: nothing new is launched */
  PTV_DFF_D_SND_MASK_ROWS, PTV_DFF_D_SND_MAX_ROWS, PTV_DFF_D_SND_MIN_ROWS, PTV_DFF_D_SND_STEPS_ROWS,   /* the row counts of ptv_sounding_step's tables */
  PTV_DFF_D_COUNT
};
int ptv_decoder_free_fwd(const void* const* t, const long* d, const void* const* wl, const void* const* io, const void* const* wr,
                         const void* const* ior, const unsigned* note_mask, const unsigned char* time_coin, void* stream);

/* ptv_decoder_free_bwd (COMPOSITE, round 6; SURVEY.md 8b's decoder_free_bwd): autograd through the node above (argmax is not
 * differentiable: with the fed tokens recorded every chain is the batched BPTT of the teacher-forced path) as ONE call --
 *   ptv_decoder_tf_bwd(t_tf, d_tf)            the decoder's whole backward on the recorded tokens (tables of that entry point)
 *   ptv_route_slices x 2                      token gradients to the ground-truth embedding (coin set / slot 0) or to the predicted
 *                                             tokens; time-token gradients to the ground-truth summaries or to the re-summarised ones
 *   ptv_bigru_rows_bwd(t_rows, d_rows)        (t_rows != NULL) BPTT of the re-summarisation bi-GRU over the predicted notes
 *                                             (ptvae.py:480-486), its input gradient added to the predicted tokens' gradient
 *   slot 0 of the predicted tokens is the ground-truth <sos> embedding: its gradient moves over; then the predicted tokens ->
 *   note_embedding: multi-hot operand of the predicted grid (ptv_multihot) and grad_W / grad_b in one ptv_wgrad pass
 * -- functional_free.DecoderStepFn.backward's launch sequence, bit-identical to it.  t: enum PtvDfbTensor, d: enum PtvDfbDim. */
enum PtvDfbTensor {
  PTV_DFB_DTOK = 0,         /* [15, R, E] fp32 (slot 15 of the [16, R, E] buffer unused): gradient w.r.t. the fed note tokens (out of t_tf) */
  PTV_DFB_DTOKS,            /* [33, B, 2He] fp32: gradient w.r.t. the time-step tokens (out of t_tf) */
  PTV_DFB_DEMB, PTV_DFB_DPRED,   /* [16, R, E] fp32, zero on entry: gradient of the ground-truth embedding / of the predicted tokens */
  PTV_DFB_DXS, PTV_DFB_DXSP,     /* [32, B, 2He] fp32, zero on entry: gradient of the ground-truth / re-summarised time tokens */
  PTV_DFB_MASK_TOK, PTV_DFB_MASK_TIME,   /* int32 [15 * 32] / [32] routing masks of the coins */
  PTV_DFB_DX_PRED,          /* [16 R, E] fp32: the input gradient t_rows produces (its PTV_BRB_DX), or NULL without t_rows */
  PTV_DFB_XHAT,             /* [B, 32, 16, 6] int64 predicted grid */
  PTV_DFB_MH,               /* [16 R, 136] fp32 scratch: its multi-hot rows */
  PTV_DFB_G_W_EMB, PTV_DFB_G_B_EMB,     /* note_embedding gradients [E, 135] / [E], accumulated into */
  PTV_DFB_COUNT
};
enum PtvDfbDim { PTV_DFB_D_B = 0, PTV_DFB_D_E, PTV_DFB_D_HE, PTV_DFB_D_COUNT };
int ptv_decoder_free_bwd(const void* const* t_tf, const long* d_tf, const void* const* t_rows, const long* d_rows, const void* const* t,
                         const long* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The teacher-forced notes GRU (dec_notes_gru over 15 note steps x 32*B rows, ptvae.py:395-398 restructured per SURVEY.md 7.1)
 * as row-partitioned persistent kernels: ONE launch for the whole sequence, a workgroup owns 64 rows, the state stays on the CU, W_hh
 * streams from L2 in ptv_pack_mfma_b packing, the token product is fused.  bf16 precision, Hn = 512, E = 128.
 *   fwd (csrc/notes_roles.hip, round 5): 8 waves per workgroup with ROLES -- four product waves stream the weights L2 -> registers and
 *        issue the MFMAs, four cell waves move every HBM operand / result and run the gate arithmetic with the fp32 state of their
 *        cells in registers for all T steps; accumulators pass through 16-KB LDS slots.
 *        wg_h = pack(W_hh [1536,512]), wg_t = pack(W_ih[:, Ht:] [1536,128]), both with pairs = 0; gc bf16 = W_ih[:, :Ht] ns + b_ih,
 *        the [R][1536] matrix stored COLUMN-BLOCKED by 16 ([96][R][16]: ptv_gemm dtypes bit 4 writes it that way); emb fp32 [T][R][128]
 *        fed tokens; h0 fp32 [R][512] the initial state (read only: the fp32 states of the later steps never leave the CU); HN16 bf16
 *        [T+1][R][512] every state, slot 0 included (the operand of the heads, the weight-gradient products and the BPTT); gates bf16
 *        [T][4] planes (r, z, n, W_hn h + b_hn) or NULL -- PRIVATE to this forward / BPTT pair: each plane is unit-blocked by 16,
 *        plane[u / 16][row][u % 16] (whole-kilobyte wave accesses), not the [R][512] of ptv_gru_seq_fwd.
 *        T: bits 0-7 = steps (1 .. 255; 0 steps: PTV_ERR_ARG); bits 8-15 = debug flags and bits 16-23 = weight-ring depth of the timing
 *        scripts (0 = defaults); bit 24: see ptv_notes_gru_persist_fwd_rows; bits 25-26 = panel height (rows per workgroup): 0 = 64
 *        (what every caller that does not set them gets), 1 = 32, 2 = the library's rule (32 rows when 64-row panels would leave the
 *        dispatcher nothing to balance with: ceil(R / 64) <= CUs / 2, or row_len given and ceil(R / 64) <= CUs; else 64), 3: PTV_ERR_ARG.
 *        Both heights write the same bits to the same slots; the timing variants (bits 8-10, 16-23) exist at 64 rows only
 *        (PTV_ERR_UNSUPPORTED with 32).  R <= 1048575 (32-bit buffer offsets: R * 2048 bytes of h0
 *        within one descriptor), PTV_ERR_UNSUPPORTED above.
 *   bwd: wt = pack(W_hh^T [512,1536]) (pairs = 1); HN16 / gates as the forward left them (the previous state enters the gate
 *        gradients at bf16 precision); ext bf16 = gradient arriving at the state after step s, the [T*R][512] matrix of the heads'
 *        input-gradient products stored COLUMN-BLOCKED by 32 ([16][T*R][32], ptv_gemm dtypes bit 3);
 *        dgi bf16 [T][R][1536]; dgh bf16 [T][R][512] = the n third (dn * r) only -- the r and z thirds of dgh are dgi's, so
 *        grad W_hh[0:1024] = dgi[:, 0:1024]^T . h and grad W_hh[1024:] = dgh^T . h; dh0 fp32 [R][512] or NULL; scratch:
 *        ptv_notes_gru_persist_scratch_elems(R) bf16 elements.  The BPTT passes over the late steps of a 64-row panel at which no gradient
 *        arrives (zero rows of ext: the padded note slots the loss ignores) and writes zero rows for them; top_step (or NULL; device int,
 *        initialised to -1 by the caller) receives the last step at which anything arrived for any panel, so that the products over dgi /
 *        dgh can stop after that step's rows (ptv_wgrad k_top).
 *        T: bits 0-7 = steps on every path (0 steps: PTV_ERR_ARG); bits 8-15 = flags of the timing scripts, bit 16: see
 *        ptv_notes_gru_persist_bwd_rows; bits 17-18 = panel height, as bits 25-26 of the forward's T (0 = 64 rows, 1 = 32, 2 = the
 *        library's rule): same dgi / dgh / dh0 / top_step, except that the zero-row scan is per panel -- a 32-row panel may write as
 *        zero rows what the 64-row panel around it computes as zeros of either sign; the 32-row kernel does not touch `scratch` (all
 *        read by the 8-wave kernel only).  8-wave kernel: R <= 699050 (R * 3072 bytes of a dgi step within
 *        one buffer descriptor) and R * (16 * steps - 1) <= 67108863 (the 32-bit offset into ext), PTV_ERR_UNSUPPORTED above; the 4-wave kernel
 *        addresses with 64-bit offsets: R <= 2^31 - 1.
 */
int ptv_notes_gru_persist_fwd(const void* wg_h, const void* wg_t, const float* b_hh, const void* gc, const float* emb,
                              const float* h0, void* HN16, void* gates, long R, int T, void* stream);
/* the same with a live-step limit: live_top (device int32, or NULL) -- only the note steps 0 .. *live_top run; the later slots of HN16 and
 * planes of gates stay unwritten (the BPTT must then be given a top_step limit <= *live_top: ptv_notes_gru_persist_bwd).  Step 0 always
 * runs: *live_top < 0 is taken as 0; *live_top >= steps - 1 is the whole sequence. */
int ptv_notes_gru_persist_fwd_top(const void* wg_h, const void* wg_t, const float* b_hh, const void* gc, const float* emb,
                                  const float* h0, void* HN16, void* gates, long R, int T, const int* live_top, void* stream);
long ptv_notes_gru_persist_scratch_elems(long R);
int ptv_notes_gru_persist_bwd(const void* wt, const void* HN16, const void* gates, const void* ext, void* dgi, void* dgh,
                              float* dh0, void* scratch, long R, int T, int* top_step, void* stream);
/* the same with a caller-given bound (device int, or NULL = the call above): no gradient arrives after note step *bound -- the forward
 * stopped there (ptv_notes_gru_persist_fwd_top) or the loss says so -- and every consumer of dgi / dgh stops at top_step (<= *bound,
 * required non-NULL then).  The note steps beyond the bound are not touched: neither is `ext` read there (it may be unwritten) nor are
 * zero rows of dgi / dgh written (without the bound: 64 KB read and 256 KB of zeros written per 64-row panel and dead step). */
int ptv_notes_gru_persist_bwd_top(const void* wt, const void* HN16, const void* gates, const void* ext, void* dgi, void* dgh,
                                  float* dh0, void* scratch, long R, int T, const int* bound, int* top_step, void* stream);
/* both with the rows sorted by descending length (row_len int32 [R] = live note steps of the row at each position, or NULL): a 64-row panel
 * runs the steps its first (= longest) row has.  Forward: the HN16 slots of a panel's dead steps up to *live_top are zero-filled (not with
 * bit 24 of T: the caller's products clip to the same segments), their gate planes unwritten.  Backward (needs bound): `ext` is not read at a panel's dead steps; dgi / dgh get zero rows there up to *bound -- unless
 * bit 16 of T is set (round 6): the caller's consumers clip to the same 128-row segments (ptv_wgrad_job.seg_n, ptv_sum_steps_seg,
 * ptv_gemm_mtop_seg) and the rows may stay unwritten. */
int ptv_notes_gru_persist_fwd_rows(const void* wg_h, const void* wg_t, const float* b_hh, const void* gc, const float* emb,
                                   const float* h0, void* HN16, void* gates, long R, int T, const int* live_top, const int* row_len,
                                   void* stream);
int ptv_notes_gru_persist_bwd_rows(const void* wt, const void* HN16, const void* gates, const void* ext, void* dgi, void* dgh,
                                   float* dh0, void* scratch, long R, int T, const int* bound, const int* row_len, int* top_step,
                                   void* stream);
/* which kernel ptv_notes_gru_persist_bwd runs: 1 (default) = 8 waves per workgroup, the A operand LDS-resident, the carry dh (x) z in registers
 * (csrc/notes_roles.hip), 0 = the 4-wave kernel of rounds 2-4 (csrc/notes_persist.hip); same arguments, same results to rounding.
 * Process-wide. */
int ptv_notes_bwd_variant(int eight_waves);

/* The same kernels for any GRU whose rows are many and independent; H = 512 (above) or H = 128 with 128 inputs, which is one
 * direction of dec_notes_emb_gru, the note-summary bi-GRU over the 16 notes of each of the 32*B steps (ptvae.py:446-453,480-486).
 *   fwd: w_hh = pack(W_hh [3H,H]), w_x = pack(W_ih [3H,128]) (H = 128: pairs = 1; H = 512: pairs = 0, as above); b_ih NULL when folded
 *        into gc; gc: H = 512 only, the column-blocked-by-16 matrix of ptv_notes_gru_persist_fwd, NULL for H = 128;
 *        x fp32, row m of step t at x + t*x_step + m*128 (x, HN and out 16-byte aligned, x_step % 4 == 0: PTV_ERR_ARG otherwise);
 *        HN fp32 [T+1][R][H], slot 0 = the initial state, written by the caller (H = 512: only slot 0 exists, it is h0); HN16 bf16
 *        [T+1][R][H], slot 0 included, written here; gates bf16 [T][4] planes or NULL, PRIVATE to the forward / BPTT pair: H = 128
 *        unit-blocked by 32, plane[u / 32][row][u % 32]; H = 512 by 16 (above);
 *        lengths int32 [R] or NULL (row m is updated at time t iff t < lengths[m],
 *        as nn.utils.rnn.pack_padded_sequence does); reverse = 1 walks time T-1..0; out (or NULL) receives the final state,
 *        row m at out + m*out_ld (out_ld % 4 == 0).
 *        The two instances are specialised: H = 512 needs gc and takes no b_ih / lengths / reverse / out; H = 128 needs b_ih and no
 *        gc (PTV_ERR_UNSUPPORTED otherwise).
 *        T = steps, 1 .. 255; H = 128 defines no flag bits (any bit above bit 7: PTV_ERR_ARG), H = 512 as ptv_notes_gru_persist_fwd.
 *        With lengths (and ptv_zero_skip on) the time indices at or beyond the longest row of the whole launch are dead when R % 32 == 0:
 *        their HN / HN16 slots and gate planes stay unwritten, except the slot in front of the first live step of the reversed direction.
 *        R <= 2^31 - 1 for H = 128.
 *   bwd: ext bf16 = the [T*R][H] matrix column-blocked by 32 as above (H = 512 only, required there); dh_last fp32 (row stride last_ld) = gradient of the final state (H = 128
 *        only), or NULL; lengths: the lengths the forward ran with, or NULL -- with lengths both kernels pass over the steps that lie
 *        beyond the longest row of a 64-row panel (identity for the whole panel, as pack_padded_sequence leaves them out;
 *        the forward then leaves that step's gates unwritten, so the backward MUST be given the same lengths); H = 512 writes only the n third of dgh ([T][R][512], see above); dgi is indexed by
 *        TIME, dgh by processing step (so dgh pairs with HN16[:T] and dgi with x in the weight-gradient products).
 *        T = steps as in the forward (0 steps or, for H = 128, any bit above bit 7: PTV_ERR_ARG).  H = 128 with lengths: top_step (or NULL)
 *        is atomicMax'ed with the last TIME index any row reaches; given top_step and R % 32 == 0, the dgi / dgh rows of the time indices
 *        beyond it stay unwritten.  dh0 of a row that never ran (length 0) is its dh_last.
 */
int ptv_row_gru_persist_fwd(int H, const void* w_hh, const void* w_x, const float* b_hh, const float* b_ih, const void* gc,
                            const float* x, long x_step, const int* lengths, float* HN, void* HN16, void* gates,
                            float* out, long out_ld, long R, int T, int reverse, void* stream);
long ptv_row_gru_persist_scratch_elems(int H, long R);
int ptv_row_gru_persist_bwd(int H, const void* wt, const void* HN, const void* gates, const void* ext,
                            const float* dh_last, long last_ld, const int* lengths, void* dgi, void* dgh, float* dh0,
                            void* scratch, long R, int T, int reverse, int* top_step, void* stream);
/* The same with a ROW PERMUTATION (H = 128): panel position p works on row perm[p] of x / lengths / out (forward) and of dh_last / lengths
 * / dgi (backward); the kernels' private tensors HN / HN16 / gates and dgh are indexed by position (dgh pairs with HN16[:T], dgi with x in
 * the weight-gradient products, as before).  With perm = ptv_rows_by_length(lengths) a 64-row panel holds rows of (almost) one length, so
 * the passing-over of a panel's masked steps -- what pack_padded_sequence does for the reference, ptvae.py:446-453 -- removes the masked
 * work itself instead of only the steps beyond the LONGEST of 64 unrelated rows.  perm NULL = the entry points above.  dh0 unsupported. */
int ptv_row_gru_persist_fwd_perm(int H, const void* w_hh, const void* w_x, const float* b_hh, const float* b_ih, const void* gc,
                                 const float* x, long x_step, const int* lengths, const int* perm, float* HN, void* HN16,
                                 void* gates, float* out, long out_ld, long R, int T, int reverse, void* stream);
int ptv_row_gru_persist_bwd_perm(int H, const void* wt, const void* HN, const void* gates, const void* ext,
                                 const float* dh_last, long last_ld, const int* lengths, const int* perm, void* dgi, void* dgh,
                                 float* dh0, void* scratch, long R, int T, int reverse, int* top_step, void* stream);
/* perm [R] = the rows in order of DESCENDING lengths[row] (0 <= length <= max_len <= 38), ties in row order: a stable counting sort in one
 * workgroup (deterministic: the order of the K rows of the weight-gradient products depends on it) */
int ptv_rows_by_length(const int* lengths, int* perm, long R, int max_len, void* stream);
/* The row plan of a length-sorted pass in ONE launch of many workgroups (round 7): perm as ptv_rows_by_length writes it, bit for bit;
 * len_sorted[p] (or NULL) = the clamped length min(max(lengths[perm[p]], 0), max_len) that perm orders by; seg_n[s], s < steps (or NULL) =
 * ptv_rows_seg_counts of len_sorted = 128 * ceil(#{rows: length > s} / 128).  Every workgroup of 256 rows counts all R lengths itself
 * (no workgroup waits for or adds to another: no counters, no global atomics), work quadratic in R: R above PTV_ROWS_PLAN_MAX_R returns
 * PTV_ERR_UNSUPPORTED with nothing written -- then call ptv_rows_by_length, ptv_gather_rows and ptv_rows_seg_counts.  max_len <= 38.
 * seg_n needs R a multiple of 128 and 0 < steps <= 64 (PTV_ERR_ARG otherwise). */
#define PTV_ROWS_PLAN_MAX_R 65536
int ptv_rows_plan(const int* lengths, long R, int max_len, int steps, int* perm, int* len_sorted, int* seg_n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * clip_grad_norm_ (module.py:142-143) + torch.optim.Adam.step (train.py:50, scheduler.py:69-74) over
 * flat fp32 buffers: sumsq = |g|^2 (device scalar), then p,m,v updated with g*gscale clipped to `clip`.
 */
/* dst[i] = bf16(src[i]): refreshes the bf16 shadow of the flat parameter buffer once per step */
int ptv_cast_bf16(const float* src, void* dst, long n, void* stream);
/* dst[c*rows + r] = bf16(src[r*cols + c]): transposed bf16 copy of a weight matrix (operand of the dX products) */
int ptv_transpose_cast_bf16(const float* src, void* dst, int rows, int cols, void* stream);
/* the same for every matrix of the flat parameter buffer in one launch: desc[i] = {offset, rows, cols, first 32x32 tile}
 * (device array of nmat x 4 longs, tiles numbered consecutively; ntiles = their total); flat_t[offset + c*rows + r] */
int ptv_transpose_cast_bf16_batched(const float* flat, void* flat_t, const long* desc, int nmat, long ntiles, void* stream);
int ptv_grad_sumsq(const float* g, long n, float* sumsq, void* stream);
int ptv_clip_adam_step(float* p, const float* g, float* m, float* v, long n, const float* sumsq, float gscale, float clip,
                       float lr, float beta1, float beta2, float eps, int step, void* stream);
/* the same step that also writes the bf16 operand copy p16[i] = bf16(p[i]) of the updated parameters (p16 may be NULL) */
int ptv_clip_adam_step_shadow(float* p, const float* g, float* m, float* v, long n, const float* sumsq, float gscale, float clip,
                              float lr, float beta1, float beta2, float eps, int step, void* p16, void* stream);
/* SURVEY 8b's gradnorm_clip_adam_step: torch.nn.utils.clip_grad_norm_(params, clip) + Adam.step() (module.py:142-144, train.py:50) over
 * the flat buffers in ONE call -- sumsq[0] = sum g^2 (left on the device: the pre-clip norm is sqrt(sumsq) * gscale), then the clipped
 * update of ptv_clip_adam_step_shadow.  gscale: 1/world under data parallelism (the bucket holds a SUM over ranks). */
int ptv_gradnorm_clip_adam_step(float* p, const float* g, float* m, float* v, long n, float* sumsq, float gscale, float clip,
                                float lr, float beta1, float beta2, float eps, int step, void* p16, void* stream);

/* Reproducible reductions (default ON; environment PTV_WGRAD_ORDERED=0 or ptv_ordered_reductions(0) turn them off).  The
 * reference's CPU path is run-to-run deterministic.  With the switch on, nothing on the train step ends in an fp32
 * atomicAdd whose order depends on arrival: the K slabs of ptv_wgrad and the K splits of ptv_gemm store partial tiles into a
 * per-stream workspace and one more launch adds them in slab order; the grid reductions (ptv_grad_sumsq, ptv_kl_fwd,
 * ptv_reparam_kl_fwd, ptv_ce_fwd, ptv_ce_group_fwd, ptv_colsum, ptv_dur_out_wgrad, ptv_txt_conv_relu_pool_bwd) park one partial per
 * block and the last block to arrive adds them in block order.  Two runs of the same step then produce the same bits.
 * ptv_wgrad_mode switches the two product paths only. */
int ptv_ordered_reductions(int on);
int ptv_wgrad_mode(int ordered);
/* bf16 x bf16 weight-gradient products through the LDS-DMA kernel (global_load_lds staging, three stage buffers; default 0 = register-staged:
 * faster standalone, slower beside the persistent recurrences -- csrc/wgrad.hip); process-wide, PTV_WGRAD_DMA sets the initial value */
int ptv_wgrad_dma(int enable);
/* reductions that ran on fp32 atomics although ordered mode is on (no workspace: first use inside a capture, > 64 streams, a need
 * beyond the scratch); 0 after any step is what makes the step bit-reproducible.  reset != 0 clears the counter. */
long ptv_ordered_fallbacks(int reset);

/* Per-step scalars on the device (graph-replayed train steps, graph_step.py): while dev4 is set, ptv_loss_finalize /
 * ptv_loss_bwd_scales read beta = dev4[0] (the KL weight of train.py:56-58's schedule; only where the call's own beta is non-zero) and
 * ptv_clip_adam_step* read lr = dev4[1], 1 - beta1^t = dev4[2], sqrt(1 - beta2^t) = dev4[3] (Adam's bias corrections,
 * scheduler.py:69-74 + train.py:50) instead of their by-value arguments.  NULL restores by-value behaviour. */
int ptv_step_params(const float* dev4);

/* ------------------------------------------------------------------------------------------------
 * Weight-gradient product (csrc/wgrad.hip): C[M,N] (fp32, row stride ldc) (+)= alpha * sum_k A[k*lda + m] * B[k*ldb + n], i.e.
 * grad_W = grad_out^T . input as autograd forms it for every nn.Linear / nn.GRU weight (ptvae.py:16-17,23,64,116,360,396,450,461),
 * with both operands stored row-per-sample.  bf16 MFMA, fp32 accumulate; dtypes bit 0 / 1 = A / B already bf16 in HBM (fp32
 * otherwise, rounded to bf16 on the way in).  K is cut into slabs that reduce into C with fp32 atomics; slabs = 0 picks the count.
 * colsum_a (or NULL): fp32 [M] += sum_k A[k*lda + m], the bias gradient that belongs to the same layer (grad_b = column sums of
 * grad_out), taken from the A tiles while they are in LDS instead of a second pass over A (always accumulates).
 * k_top (or NULL): device int; the rows of A from (*k_top + 1) * k_unit on are zero (the kernel that wrote A says so: the notes BPTT
 * reports the last note step at which any gradient arrived) -- the product stops there.  k_unit must be a multiple of 32.
 * k_rev > 0: A holds its k_rev units in reversed order (the *_reverse direction of a GRU, gradients indexed by processing step):
 * the zero part is then the rows BEFORE (k_rev - *k_top - 1) * k_unit and the product starts there.
 * ptv_gemm(prec = bf16, transA = transB = 1) routes here.
 */
int ptv_wgrad(int M, int N, int K, const void* A, long lda, const void* B, long ldb, float* C, long ldc, float alpha,
              int accumulate, int dtypes, int slabs, float* colsum_a, const int* k_top, long k_unit, int k_rev, void* stream);
/* the same for a gradient matrix that lives in TWO arrays: C[M1 + M2, N] (+)= alpha * [A1 | A2]^T . B, rows 0 .. M1-1 of C from the columns
 * of A1, the rest from A2 (same dtype, M1 a multiple of 128) -- one pass over B instead of two (the notes GRU's weight_hh gradient:
 * [dgi[:, :1024] | dgh]^T . h, ptv_notes_gru_persist_bwd) */
int ptv_wgrad_cat(int M1, const void* A1, long lda1, int M2, const void* A2, long lda2, int N, int K, const void* B, long ldb,
                  float* C, long ldc, float alpha, int accumulate, int dtypes, int slabs, float* colsum_a, const int* k_top,
                  long k_unit, int k_rev, void* stream);
/* Several weight-gradient products in ONE launch (plus one launch for their ordered reductions): the parameter gradients that become ready
 * at the same point of a backward pass -- a GRU's W_ih / W_hh with their bias sums, a decoder's z projections (ptvae.py:16-17,23,64,116,
 * 360,396,450,461 as above).  Each job has exactly the meaning of one ptv_wgrad call with the same fields, and gives the same bits as that
 * call would (same slab plan, same reduction order); the jobs' outputs (C, colsum_a) must not overlap.  HOST array of jobs. */
typedef struct ptv_wgrad_job {
  int M, N, K;
  const void* A; long lda;
  const void* B; long ldb;
  float* C; long ldc;
  float alpha;
  int accumulate, dtypes, slabs;
  float* colsum_a;
  const int* k_top; long k_unit; int k_rev;
  /* round 6, K SEGMENTS (or seg_n = NULL): K runs over units of seg_unit rows (a note step's R decoder rows in length order); of unit q only the
   * first seg_n[q % seg_period] rows (seg_period < 0: seg_n[|seg_period| - 1 - q % |seg_period|], units in reversed order; device ints,
   * multiples of 32) hold anything -- the rest of A is zero and the rest of B may never have
   * been written.  The product skips them (slabs never straddle a unit: ptv_wgrad_seg_supported(K, seg_unit)), and so does
   * the ordered reduction; against the same product without segments the result is bit-identical when the skipped rows of A are zero. */
  const int* seg_n; long seg_unit; int seg_period;
} ptv_wgrad_job;
int ptv_wgrad_batch(const ptv_wgrad_job* jobs, int njobs, void* stream);
/* 1 if a product of depth K can take segments of seg_unit rows: seg_unit a multiple of 128 that divides K, and K cut into at most 248 slabs of
 * the largest power of two that divides seg_unit (B = 512: 16384-row units; 3 * 2^k units work too; 128 * 129 rows do not) */
int ptv_wgrad_seg_supported(long K, long seg_unit);
/* seg_n[s] = 128 * #{128-row blocks whose FIRST row has row_len > s}, s < steps: the live prefix of every note step when the decoder's rows run
 * in descending length order (ptv_rows_by_length) and a block is dead beyond its first row's length -- what the *_rows kernels of the decoder
 * skip and ptv_wgrad_batch's segments clip.  R a multiple of 128. */
int ptv_rows_seg_counts(const int* row_len, long R, int steps, int* seg_n, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* PTVAE_HIP_H */
