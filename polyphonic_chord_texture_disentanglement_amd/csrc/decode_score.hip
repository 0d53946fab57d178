// decode_score.hip -- log-probabilities of a free-running decode and best-of-n (forward only).
//   ptv_decode_logprob:      per (sample, time step) the sums of log p (the model's own softmax) and log q (the distribution the decode drew
//                            from: temperature, allowed set, kept set) over the decisions the decode took, and their counts
//   ptv_decode_logprob_fold: the 32 time steps of a sample added in ascending order
//   ptv_best_of_gather:      of n candidates per row the first with the largest score: its index, grid and sums
// A post-pass over what a decode leaves behind: plain logits, decided grid, sampling block, force arrays.  The allowed / kept set is NOT
// restated here: it comes from pitch_constrain() and pitch_keep_threshold() of philox.hpp, the calls every decision site makes.
// Every output element has ONE writer and one fixed summation order: no atomics, no scratch, results bit-identical from run to run and
// independent of the logits' layout.  A row or bit that does not count is never loaded.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

constexpr int DS_NP = 130;

// sum over the 16 lanes of a DPP row; every lane ends with the same bits (each rotation adds two values that were formed alike)
__device__ __forceinline__ float row16_sum(float x) {
  x += __builtin_bit_cast(float, dpp_row_ror<8>(__builtin_bit_cast(int, x)));
  x += __builtin_bit_cast(float, dpp_row_ror<4>(__builtin_bit_cast(int, x)));
  x += __builtin_bit_cast(float, dpp_row_ror<2>(__builtin_bit_cast(int, x)));
  x += __builtin_bit_cast(float, dpp_row_ror<1>(__builtin_bit_cast(int, x)));
  return x;
}

// One workgroup per sample b, one wave per (b, t): wave w takes t = w, w + 4, ..., so that err[b] has one writer.  A wave's four DPP rows
// take the note steps n = 4k + g, g = 0..3, k = 0..3: a step's 15 rows are four trips.  Within a row lane j owns the classes j + 16 i,
// i = 0..8 -- the W = 16 layout of pitch_constrain() / pitch_keep_threshold().  VEC: the row is fetched by 16-byte loads (lane j: classes
// 4j..4j+3 and 64+4j..64+4j+3; lane 0: 128, 129) and handed to the owners by shuffles; else nine 4-byte loads of the owned classes: the
// same values in the same registers, so everything after the load is the same arithmetic.  Lanes j = 0..4 of a row also take the note's
// five duration bits.  Nothing diverges around a cross-lane operation: a dead row only guards its loads.  All lanes keep the same running
// sums (n ascending; a note's pitch term, then its bits ascending); lane 0 writes them.
template <bool VEC>
__global__ void __launch_bounds__(256) decode_logprob_kernel(const float* __restrict__ pitch, long ld, const float* __restrict__ dur,
                                                             const long* __restrict__ x, int B, int step_major, const void* __restrict__ blk,
                                                             int blk_bytes, const int* __restrict__ force_pitch,
                                                             const int* __restrict__ force_dur, float* __restrict__ step_logp,
                                                             int* __restrict__ step_counts, int* __restrict__ err) {
  __shared__ int errs[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  const int b = blockIdx.x;
  const long R = 32L * B, M = 15 * R;
  float Tp = 0.f, Td = 0.f;
  Trunc tr{0, LN_MIN_P_OFF, 0u};
  Cons cn{0u, nullptr};
  if (blk) {
    const SampleBlock* s = reinterpret_cast<const SampleBlock*>(blk);
    Tp = s->t_pitch; Td = s->t_dur;
    if (blk_bytes >= 48) tr = load_trunc(reinterpret_cast<const SampleBlockT*>(blk));
    if (blk_bytes >= 64) cn = load_cons(reinterpret_cast<const SampleBlockC*>(blk));
    if (blk_bytes >= 80) {                                                 // row-wise: sample b's own record (one workgroup, one sample: still uniform)
      const RowRule rw = load_row_rule(load_row_table(blk), b);
      Tp = rw.t_pitch; Td = rw.t_dur; tr = rw.tr;
    }
  }
  int e = 0;
  for (int t = wv; t < 32; t += 4) {
    const long* xs = x + ((long)b * 32 + t) * 96;                          // the step's 16 slots of 6
    // lane s < 16 holds the pitch of slot s; L, and the largest pitch < 128 of the slots 1..s (the `lo` of note step n = s)
    const long pl = (lane >= 1 && lane < 16) ? xs[lane * 6] : -1;
    const int P = (pl >= 0 && pl < DS_NP) ? (int)pl : -1;                    // (a pitch outside 0..129 names no class)
    const unsigned long long eos = __ballot(P == 129) & 0xfffeull;
    const int L = eos ? __ffsll((long long)eos) - 1 : 15;
    int lo_incl = P < 128 ? P : -1;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { const int u = __shfl_up(lo_incl, o, 64); if (lane >= o) lo_incl = max(lo_incl, u); }
    unsigned mw[4];
    pitch_mask_words(cn, b, t, mw);
    const unsigned own = pitch_mask_own<9, 16>(mw, j);
    float sp = 0.f, sd = 0.f, qp = 0.f, qd = 0.f;
    int pn = 0, dn = 0, fpn = 0, fdn = 0;
    for (int k = 0; k < 4; k++) {
      const int n = 4 * k + g;
      const bool cnt = n < L;                                              // (n < 15 with it)
      const int p = __shfl(P, n < 15 ? n + 1 : 15, 64);
      const int lo = __shfl(lo_incl, n < 15 ? n : 0, 64);                   // (lane 0 holds -1)
      const bool plive = cnt && p >= 0;
      const bool bad = cnt && p < 0;
      const bool note = plive && p < 128;
      if (!__any(cnt)) break;                                              // (wave-uniform: the trips after L are dead)
      const long i = step_major ? ((long)n * 32 + t) * B + b : ((long)b * 32 + t) * 15 + n;
      const long fr = (long)n * R + (long)t * B + b;                       // the force arrays are step-major whatever the logits are
      // ---- the row: v[i] = class j + 16 i, -inf where the class does not exist (a dead row: zeros, so that nothing below forms a NaN)
      float v[9];
#pragma unroll
      for (int q = 0; q < 9; q++) v[q] = j + 16 * q < DS_NP ? 0.f : -INFINITY;
      float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0;
      if (plive) {
        const float* lr = pitch + i * ld;
        if (VEC) {
          a0 = *reinterpret_cast<const float4*>(lr + 4 * j);
          a1 = *reinterpret_cast<const float4*>(lr + 64 + 4 * j);
          if (j == 0) a2 = *reinterpret_cast<const float4*>(lr + 128);
        } else {
#pragma unroll
          for (int q = 0; q < 8; q++) v[q] = lr[j + 16 * q];
          if (j < 2) v[8] = lr[128 + j];
        }
      }
      if (VEC) {
        const int c = j & 3, row0 = lane & 48;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int src = row0 + (j >> 2) + 4 * q;
          const float x0 = __shfl(a0.x, src, 64), x1 = __shfl(a0.y, src, 64), x2 = __shfl(a0.z, src, 64), x3 = __shfl(a0.w, src, 64);
          const float y0 = __shfl(a1.x, src, 64), y1 = __shfl(a1.y, src, 64), y2 = __shfl(a1.z, src, 64), y3 = __shfl(a1.w, src, 64);
          const float lo4 = c == 0 ? x0 : c == 1 ? x1 : c == 2 ? x2 : x3, hi4 = c == 0 ? y0 : c == 1 ? y1 : c == 2 ? y2 : y3;
          if (plive) { v[q] = lo4; v[4 + q] = hi4; }
        }
        const float z0 = __shfl(a2.x, row0, 64), z1 = __shfl(a2.y, row0, 64);
        if (plive && j < 2) v[8] = j == 0 ? z0 : z1;
      }
      const int fp = (plive && force_pitch) ? force_pitch[fr] : -1;
      const bool pforced = fp >= 0;
      // ---- log p: log softmax over the 130 classes at the decided one
      const int pc = plive ? p : 0;
      float mine = 0.f;
#pragma unroll
      for (int q = 0; q < 9; q++) if ((pc >> 4) == q) mine = v[q];
      const float vd = __shfl(mine, (lane & 48) + (pc & 15), 64);
      float m = v[0];
#pragma unroll
      for (int q = 1; q < 9; q++) m = fmaxf(m, v[q]);
      m = row_max<16>(m);
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 9; q++) s += expf(v[q] - m);
      s = row16_sum(s);
      const float lpp = plive ? vd - m - logf(s) : 0.f;
      // ---- log q: the decoder's own allowed and kept set, softmax of (v - m) / T over it
      float lqp = 0.f;
      bool outside = false;
      if (Tp > 0.f) {                                                      // (uniform: the block's word, or the sample's)
        float tv[9];
        // (a PTV_FORCE_NOT_EOS or PTV_FORCE_BELOW decision is free, its support the decoder's reduced one; only the 64-byte kind honours the word)
        const unsigned al = pitch_constrain<9, 16>(v, own, lo, cn.flags, j, tv, blk_bytes >= 64 ? fp : -1);
        const float thr = pitch_keep_threshold<9, 16>(tr, Tp, tv);
        unsigned kept = 0u;
#pragma unroll
        for (int q = 0; q < 9; q++) if (((al >> q) & 1u) && v[q] >= thr) kept |= 1u << q;
        float mk = -INFINITY;
#pragma unroll
        for (int q = 0; q < 9; q++) if ((kept >> q) & 1u) mk = fmaxf(mk, v[q]);
        mk = row_max<16>(mk);
        float sk = 0.f;
#pragma unroll
        for (int q = 0; q < 9; q++) if ((kept >> q) & 1u) sk += expf((v[q] - mk) / Tp);
        sk = row16_sum(sk);
        const int kd = __shfl((int)((kept >> (pc >> 4)) & 1u), (lane & 48) + (pc & 15), 64);
        if (plive && !pforced) {
          if (kd) lqp = (vd - mk) / Tp - logf(sk);
          else outside = true;
        }
      }
      // ---- duration bit j of the note: two classes
      const int dt = (note && j < 5) ? (int)xs[(n + 1) * 6 + 1 + j] : 2;
      const bool dlive = dt == 0 || dt == 1;
      // (duration limits: the value of the note's bits before bit j, from the ones of the row's lanes 0..j-1 -- every lane takes the ballot)
      const unsigned ones = (unsigned)(__ballot(dt == 1) >> (lane & 48)) & 31u;
      int dpre = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) if (q < j) dpre = 2 * dpre + (int)((ones >> q) & 1u);
      float lpd = 0.f, lqd = 0.f;
      bool dforced = false;
      if (dlive) {
        const float* dr = dur + i * 10 + 2 * j;
        const float l0 = dr[0], l1 = dr[1];
        const float dm = fmaxf(l0, l1);
        lpd = (dt ? l1 : l0) - dm - logf(expf(l0 - dm) + expf(l1 - dm));
        const int fdw = force_dur ? force_dur[(long)j * M + fr] : -1;
        dforced = fdw >= 0;
        // a PTV_FORCE_DUR_RANGE word (only the 64-byte kind honours it): a bit the range determines is no draw -- log p as ever, log q 0,
        // counted with the forced decisions; a decided value the range excludes sets bit 0 of err.  Both values allowed: a free decision
        if (!dforced && blk_bytes >= 64) {
          const unsigned dal = dur_range_allowed(fdw, j, dpre);
          if (dal == 1u || dal == 2u) { dforced = true; if (dal != (1u << dt)) outside = true; }
        }
        if (!dforced && Td > 0.f) {
          const float a0_ = l0 / Td, a1_ = l1 / Td, am = fmaxf(a0_, a1_);
          lqd = (dt ? a1_ : a0_) - am - logf(expf(a0_ - am) + expf(a1_ - am));
        }
      }
      if (bad || outside) e |= 1;
      // ---- the running sums: rows 4k .. 4k + 3 in order (every lane adds the same values)
      const unsigned long long dvm = __ballot(dlive), dfm = __ballot(dforced);
#pragma unroll
      for (int h = 0; h < 4; h++) {
        const int pl_ = __shfl((int)plive, 16 * h, 64), pf_ = __shfl((int)pforced, 16 * h, 64);
        const float lpp_ = __shfl(lpp, 16 * h, 64), lqp_ = __shfl(lqp, 16 * h, 64);
        if (pl_) { sp += lpp_; qp += lqp_; }
        pn += pl_; fpn += pf_;
        const int vm = (int)((dvm >> (16 * h)) & 31), fm = (int)((dfm >> (16 * h)) & 31);
#pragma unroll
        for (int d = 0; d < 5; d++) {
          const float lpd_ = __shfl(lpd, 16 * h + d, 64), lqd_ = __shfl(lqd, 16 * h + d, 64);
          if ((vm >> d) & 1) { sd += lpd_; qd += lqd_; }
        }
        dn += __popc(vm); fdn += __popc(fm);
      }
    }
    if (lane == 0) {
      float* so = step_logp + ((long)b * 32 + t) * 4;
      int* co = step_counts + ((long)b * 32 + t) * 4;
      so[0] = sp; so[1] = sd; so[2] = qp; so[3] = qd;
      co[0] = pn; co[1] = dn; co[2] = fpn; co[3] = fdn;
    }
  }
  e = __any(e) ? 1 : 0;
  if (lane == 0) errs[wv] = e;
  __syncthreads();
  if (threadIdx.x == 0) err[b] = errs[0] | errs[1] | errs[2] | errs[3];
}

static inline bool ds_vec_ok(const float* p, long ld) {
  return (ld & 3) == 0 && ld >= ((DS_NP + 3) & ~3) && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// thread (b, column): columns 0..3 = the float sums, 4..7 = the counts; t = 0..31 in ascending order
__global__ void decode_logprob_fold_kernel(const float* __restrict__ step_logp, const int* __restrict__ step_counts, int B,
                                           float* __restrict__ sums, int* __restrict__ counts) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * 8) return;
  const long b = i >> 3; const int col = (int)(i & 7);
  if (col < 4) {
    float s = 0.f;
    for (int t = 0; t < 32; t++) s += step_logp[(b * 32 + t) * 4 + col];
    sums[b * 4 + col] = s;
  } else {
    int s = 0;
    for (int t = 0; t < 32; t++) s += step_counts[(b * 32 + t) * 4 + (col - 4)];
    counts[b * 4 + (col - 4)] = s;
  }
}

// one workgroup per row b: every thread finds the winner (n is small), then the 3072 words of its grid are copied, 12 per thread
__global__ void __launch_bounds__(256) best_of_gather_kernel(const float* __restrict__ score, const long* __restrict__ grids,
                                                             const float* __restrict__ sums, int n, int B, int* __restrict__ best,
                                                             long* __restrict__ out_grid, float* __restrict__ out_sums,
                                                             int* __restrict__ err) {
  const long b = blockIdx.x;
  int kb = -1; float sb = 0.f;
  for (int k = 0; k < n; k++) {
    const float s = score[(long)k * B + b];
    if (s != s) continue;                                                  // (a NaN never wins)
    if (kb < 0 || s > sb) { kb = k; sb = s; }
  }
  const int k = kb < 0 ? 0 : kb;
  const long src = (long)k * B + b;
  for (int i = threadIdx.x; i < 3072; i += 256) out_grid[b * 3072 + i] = grids[src * 3072 + i];
  if (threadIdx.x < 4) out_sums[b * 4 + threadIdx.x] = sums[src * 4 + threadIdx.x];
  if (threadIdx.x == 0) { best[b] = k; err[b] = kb < 0 ? 2 : 0; }
}

}  // namespace ptv

using namespace ptv;

extern "C" int ptv_decode_logprob(const float* pitch, long ld_pitch, const float* dur, const long* xhat, int B, int step_major,
                                  const void* sample, int sample_bytes, const int* force_pitch, const int* force_dur, float* step_logp,
                                  int* step_counts, int* err, void* stream) {
  if (!pitch || !dur || !xhat || !step_logp || !step_counts || !err || B < 1 || ld_pitch < DS_NP) return PTV_ERR_ARG;
  if (sample ? (sample_bytes != 32 && sample_bytes != 48 && sample_bytes != 64 && sample_bytes != 80) : sample_bytes != 0) return PTV_ERR_ARG;
  const dim3 grid(B), block(256);
  if (ds_vec_ok(pitch, ld_pitch))
    hipLaunchKernelGGL((decode_logprob_kernel<true>), grid, block, 0, (hipStream_t)stream, pitch, ld_pitch, dur, xhat, B, step_major, sample,
                       sample_bytes, force_pitch, force_dur, step_logp, step_counts, err);
  else
    hipLaunchKernelGGL((decode_logprob_kernel<false>), grid, block, 0, (hipStream_t)stream, pitch, ld_pitch, dur, xhat, B, step_major, sample,
                       sample_bytes, force_pitch, force_dur, step_logp, step_counts, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_decode_logprob_fold(const float* step_logp, const int* step_counts, int B, float* sums, int* counts, void* stream) {
  if (!step_logp || !step_counts || !sums || !counts || B < 1) return PTV_ERR_ARG;
  hipLaunchKernelGGL(decode_logprob_fold_kernel, dim3(cdiv((long)B * 8, 256)), dim3(256), 0, (hipStream_t)stream, step_logp, step_counts, B,
                     sums, counts);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_best_of_gather(const float* score, const long* grids, const float* sums, int n, int B, int* best, long* out_grid,
                                  float* out_sums, int* err, void* stream) {
  if (!score || !grids || !sums || !best || !out_grid || !out_sums || !err || B < 1 || n < 1) return PTV_ERR_ARG;
  hipLaunchKernelGGL(best_of_gather_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, score, grids, sums, n, B, best, out_grid, out_sums,
                     err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
