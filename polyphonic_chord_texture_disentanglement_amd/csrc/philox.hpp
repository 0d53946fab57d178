// philox.hpp -- Philox4x32-10 and what is keyed by it: the reparameterisation noise (rng.hip) and the Gumbel noise of the sampling
// decoder (freerun.hip, misc.hip, dur.hip).  Device code only.
//
// Sampling noise (DESIGN.md "Sampled decode"): a decision at (global sample g, time step t, note step n) perturbs its logits by
// T * gumbel(word), and every word is a pure function of (seed, draw, g, t, n, kind, index) -- nothing of the launch geometry enters.
//   key     = (seed lo, seed hi)
//   counter = ( g lo,
//               g hi * 2^16 | t << 11 | n << 7 | kind << 6 | sub,        g < 2^48, t < 32, n < 16
//               draw lo,
//               2^31 | draw hi )                                         draw < 2^63
//   kind 0 (pitch):    sub = q * 16 + j, q < 3, j < 16: word w of the call is column j + 16 * (4 q + w) -- the nine columns j + 16 k a lane
//                      of the note loop owns are words 0..3 of q = 0, 1 and word 0 of q = 2: three calls
//   kind 1 (duration): sub = q < 3: word w of the call is index 4 q + w = 2 d + c, the draw of class c of duration bit d (ten of twelve used)
// The eps streams of ptv_philox_normal (rng.hip) keep counter word 3 = stream hi with stream ids < 2^63: bit 31 of word 3 separates the two.
#pragma once
#include <hip/hip_runtime.h>

namespace ptv {

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// the sampling parameters, a DEVICE block (a captured graph holds the pointer, not the values): 32 bytes
struct SampleBlock {
  unsigned long long seed, draw;
  long long sample_offset;               // global index of row 0
  float t_pitch, t_dur;                  // temperatures (>= 0; 0 = argmax)
};

// standard Gumbel from one 32-bit word: u = (top 23 bits + 1/2) * 2^-23 is exact in fp32 and lies in [2^-24, 1 - 2^-24] for every word, so
// both logarithms are finite: g in [-2.82, 16.64]
__device__ __forceinline__ float gumbel_from_word(unsigned w) {
  const float u = ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;
  return -__logf(-__logf(u));
}

__device__ __forceinline__ void sample_words(const SampleBlock& s, long long g, int t, int n, int kind, int sub, unsigned (&c)[4]) {
  const unsigned long long gu = (unsigned long long)g;
  c[0] = (unsigned)gu;
  c[1] = ((unsigned)(gu >> 32) << 16) | ((unsigned)t << 11) | ((unsigned)n << 7) | ((unsigned)kind << 6) | (unsigned)sub;
  c[2] = (unsigned)s.draw;
  c[3] = 0x80000000u | (unsigned)(s.draw >> 32);
  philox4x32_10(c, (unsigned)s.seed, (unsigned)(s.seed >> 32));
}

// Gumbel values of the pitch columns j + 16 k, k = 0..8, of row g (columns >= 130 included: their owners ignore them)
__device__ __forceinline__ void pitch_gumbel9(const SampleBlock& s, long long g, int t, int n, int j, float (&out)[9]) {
#pragma unroll
  for (int q = 0; q < 3; q++) {
    unsigned c[4];
    sample_words(s, g, t, n, 0, q * 16 + j, c);
#pragma unroll
    for (int w = 0; w < 4; w++) if (4 * q + w < 9) out[4 * q + w] = gumbel_from_word(c[w]);
  }
}
// Gumbel value of ONE pitch column (a call per column: the step-loop kernels, whose lanes own other column sets)
__device__ __forceinline__ float pitch_gumbel1(const SampleBlock& s, long long g, int t, int n, int col) {
  const int k = col >> 4;
  unsigned c[4];
  sample_words(s, g, t, n, 0, (k >> 2) * 16 + (col & 15), c);
  return gumbel_from_word(c[k & 3]);
}
// Gumbel values of the duration decisions of row g: out[2 d + c], d < 5, c < 2
__device__ __forceinline__ void dur_gumbel10(const SampleBlock& s, long long g, int t, int n, float (&out)[10]) {
#pragma unroll
  for (int q = 0; q < 3; q++) {
    unsigned c[4];
    sample_words(s, g, t, n, 1, q, c);
#pragma unroll
    for (int w = 0; w < 4; w++) if (4 * q + w < 10) out[4 * q + w] = gumbel_from_word(c[w]);
  }
}
// ... and of ONE duration bit d: (class 0, class 1)
__device__ __forceinline__ void dur_gumbel2(const SampleBlock& s, long long g, int t, int n, int d, float& g0, float& g1) {
  unsigned c[4];
  sample_words(s, g, t, n, 1, (2 * d) >> 2, c);
  g0 = gumbel_from_word(c[(2 * d) & 3]); g1 = gumbel_from_word(c[(2 * d + 1) & 3]);
}

// the decision rules, shared by every kernel: the first maximal index of logit + T * g (T = 0: logit + 0 = the plain argmax, ties included)
__device__ __forceinline__ float perturbed(float logit, float T, float g) { return logit + T * g; }

// ---------------------------------------------------------------------------------------------------------------------------------
// Truncated sampling (DESIGN.md "Sampled decode": the select): the pitch draw over the classes whose logit reaches a per-row threshold.
// The extended block is the 32 bytes above, unchanged, followed by 16 more: 48 bytes.
//   top_k:    keep the classes >= the k-th largest logit of the row (counted with multiplicity; ties with it are all kept); 0 = off,
//             k >= 130 keeps everything
//   ln_min_p: keep the classes >= m + T_pitch * ln(min_p), m the row's largest logit (p_c >= min_p * p_max under softmax(logits / T));
//             any value > 0 = off (the host writes LN_MIN_P_OFF; ln(min_p) <= 0 for every min_p in (0, 1]) -- the test is on the
//             word itself, no infinity is ever multiplied by T
//   top_p_q24: nucleus -- round(top_p * 2^24) in [1, 2^24], 0 = off (the first of the two words that were reserved and zero: every
//             block written before keeps its meaning).  Keep the smallest set of best classes whose mass under softmax(logits / T) reaches
//             top_p, ties with the last kept value all kept: class c is kept iff the mass of the classes strictly above it is < top_p * Z.
//             The masses are INTEGERS, w_c = trunc(__expf((logit_c - m) / T) * 2^20) (fp32 difference and quotient, each correctly
//             rounded), so Z and every partial mass are exact sums, the same on every lane layout and in every cluster member
//             (a class whose w truncates to 0 carries no mass).  T = 0: no rule (the decode is the argmax decode anyway)
// All given: the largest threshold -- every rule is judged on the untruncated row.  The row's best class passes each rule, so the kept
// set is never empty.
// ---------------------------------------------------------------------------------------------------------------------------------
struct SampleBlockT {
  SampleBlock s;
  int top_k;
  float ln_min_p;
  unsigned top_p_q24;
  unsigned reserved;
};
static_assert(sizeof(SampleBlock) == 32 && sizeof(SampleBlockT) == 48, "sampling blocks: 32 / 48 bytes (include/ptvae_hip.h)");
constexpr float LN_MIN_P_OFF = 1.f;
struct Trunc { int top_k; float ln_min_p; unsigned top_p_q24; };   // what a kernel keeps of the extension
__device__ __forceinline__ Trunc load_trunc(const SampleBlockT* q) { return Trunc{q->top_k, q->ln_min_p, q->top_p_q24}; }
constexpr int TOP_P_MASS_BITS = 20;                                // a class's integer mass is <= 2^20: 130 of them stay below 2^28

// order-preserving integer key of a float (-0.0 is +0.0: they compare equal) and its inverse
__device__ __forceinline__ unsigned order_key(float v) {
  unsigned u = __builtin_bit_cast(unsigned, v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_key_value(unsigned k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// reductions over the W lanes that hold a row, every lane ends with the result.  W = 16: a DPP row (the note loops: lane j of the 16 owns
// columns j + 16 i), the rotations of the argmax; W = 64: the wave (the step loop: lane l owns columns l + 64 i), two more exchanges
template <int N> __device__ __forceinline__ int dpp_row_ror(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x120 + N, 0xf, 0xf, false); }
template <int W> __device__ __forceinline__ int row_sum(int x) {
  x += dpp_row_ror<8>(x); x += dpp_row_ror<4>(x); x += dpp_row_ror<2>(x); x += dpp_row_ror<1>(x);
  if constexpr (W == 64) { x += __shfl_xor(x, 16, 64); x += __shfl_xor(x, 32, 64); }
  return x;
}
template <int W> __device__ __forceinline__ float row_max(float x) {
  x = fmaxf(x, __builtin_bit_cast(float, dpp_row_ror<8>(__builtin_bit_cast(int, x))));
  x = fmaxf(x, __builtin_bit_cast(float, dpp_row_ror<4>(__builtin_bit_cast(int, x))));
  x = fmaxf(x, __builtin_bit_cast(float, dpp_row_ror<2>(__builtin_bit_cast(int, x))));
  x = fmaxf(x, __builtin_bit_cast(float, dpp_row_ror<1>(__builtin_bit_cast(int, x))));
  if constexpr (W == 64) { x = fmaxf(x, __shfl_xor(x, 16, 64)); x = fmaxf(x, __shfl_xor(x, 32, 64)); }
  return x;
}

// THE keep rule, shared by every decision site (and ptv_debug_pitch_keep): class c of the row is kept iff logit[c] >= the value returned.
// v: the NV logits this lane owns, -INFINITY where the column does not exist; all W lanes of the row call it together.  tr and T are
// uniform over the W lanes of a row.  The block kinds pass the block's own words, uniform over the wave: the tests below are scalar
// branches.  The row-wise kind (SampleBlockR below) passes each row's record, so with W = 16 the four rows of a wave may take different
// branches: the rule holds all the same, because every cross-lane step inside a branch -- the rotations of row_sum<16> / row_max<16> --
// stays inside one DPP row, whose 16 lanes are active or inactive together (a rotation never reads an inactive lane), and the select
// loops run a fixed 32 rounds.  W = 64 also crosses DPP rows (__shfl_xor), and there the row is the wave: uniform again.
// top_k: a 32-round bitwise select of the k-th largest order key -- a round counts the row's keys >= the candidate (NV compares per
// lane, one W-lane sum) and keeps the bit if there are at least k; fixed cost, no LDS, independent of the lane layout.  The padding
// keys are below every real one and k < 130 real values exist, so the selected key is a real logit's.
// top_p: the same select with masses in place of counts -- a round keeps the bit iff mass{key >= candidate} * 2^24 >= Z * top_p_q24 (64-bit;
// the right side is formed once).  The largest such candidate is the key of a class with w > 0 (the mass changes only there; the best
// class has w = 2^20, so Z > 0 and the padding, w = 0, is never selected).  Same cost for every row, no LDS.
template <int NV, int W>
__device__ __forceinline__ float pitch_keep_threshold(const Trunc tr, float T, const float (&v)[NV]) {
  float thr = -INFINITY;
  if (tr.top_k > 0 && tr.top_k < 130) {
    unsigned key[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) key[i] = order_key(v[i]);
    unsigned sel = 0u;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      const unsigned cand = sel | (1u << b);
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < NV; i++) cnt += key[i] >= cand ? 1 : 0;
      if (row_sum<W>(cnt) >= tr.top_k) sel = cand;
    }
    thr = order_key_value(sel);
  }
  if (tr.top_p_q24 != 0u && T > 0.f) {
    float m = v[0];
#pragma unroll
    for (int i = 1; i < NV; i++) m = fmaxf(m, v[i]);
    m = row_max<W>(m);
    unsigned key[NV];
    int w[NV], z = 0;
#pragma unroll
    for (int i = 0; i < NV; i++) {
      key[i] = order_key(v[i]);
      w[i] = (int)(__expf((v[i] - m) / T) * (float)(1 << TOP_P_MASS_BITS));   // (-inf: 0; the best class: exactly 2^20)
      z += w[i];
    }
    const unsigned long long need = (unsigned long long)(unsigned)row_sum<W>(z) * tr.top_p_q24;
    unsigned sel = 0u;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      const unsigned cand = sel | (1u << b);
      int g = 0;
#pragma unroll
      for (int i = 0; i < NV; i++) g += key[i] >= cand ? w[i] : 0;
      if (((unsigned long long)(unsigned)row_sum<W>(g) << 24) >= need) sel = cand;
    }
    thr = fmaxf(thr, order_key_value(sel));
  }
  if (tr.ln_min_p <= 0.f) {
    float m = v[0];
#pragma unroll
    for (int i = 1; i < NV; i++) m = fmaxf(m, v[i]);
    thr = fmaxf(thr, row_max<W>(m) + T * tr.ln_min_p);
  }
  return thr + 0.f;                                                // (a zero threshold is +0.0)
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Constrained decode: restrictions on the SUPPORT of the pitch decision, applied before the truncation above.  The block is
// the 48 bytes above, unchanged, followed by 16 more: 64 bytes.
//   flags bit 0 (CONS_ASCENDING): a pitch c < 128 is allowed iff c > lo, lo the largest pitch < 128 already decided in this time step
//             (after force_pitch; -1 at note step 0); <sos> (128) is never allowed
//   flags bit 1 (CONS_MASK_ROW1): the mask has ONE row [32, 4] for the whole batch (row stride 0)
//   mask:     0, or the device address of int32 [B, 32, 4]: bit p & 31 of word p >> 5 of [b, t] set = grid pitch p allowed at time step t;
//             classes 128 / 129 are not covered by it
// <eos> (129) is always allowed: the allowed set is never empty.  A disallowed class enters pitch_keep_threshold() as -INFINITY (top_k counts
// the k best ALLOWED classes, the nucleus mass, Z and min_p's maximum are those of the allowed classes; with fewer than k allowed the
// select ends at the -INFINITY key: all of them are kept), and the draw tests the returned bitmap beside the threshold.
// Kept rhythm: a decision whose force word is PTV_FORCE_NOT_EOS (-2) is free, but <eos> leaves its allowed set unless nothing
// else is allowed -- inside the allowed rule, so before any truncation.  Only the kernels of this 64-byte kind honour the word.
// Kept top voice: a word PTV_FORCE_BELOW(u) is free, never <eos>, and a note under the ceiling u -- same place, same kernels.
// ---------------------------------------------------------------------------------------------------------------------------------
struct SampleBlockC {
  SampleBlockT s;
  unsigned flags;
  unsigned reserved;
  const unsigned* mask;
};
static_assert(sizeof(SampleBlockC) == 64, "constrained sampling block: 64 bytes (include/ptvae_hip.h)");
constexpr unsigned CONS_ASCENDING = 1u, CONS_MASK_ROW1 = 2u;
struct Cons { unsigned flags; const unsigned* mask; };             // what a kernel keeps of the extension
__device__ __forceinline__ Cons load_cons(const SampleBlockC* q) { return Cons{q->flags, q->mask}; }

// the four mask words of row b at time step t (all ones without a mask): ONE 16-byte row, loaded once per launch by the note loops
__device__ __forceinline__ void pitch_mask_words(const Cons cn, long b, int t, unsigned (&m)[4]) {
  m[0] = m[1] = m[2] = m[3] = 0xffffffffu;
  if (cn.mask) {
    const unsigned* p = cn.mask + (((cn.flags & CONS_MASK_ROW1) ? 0 : b) * 32 + t) * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = p[i];
  }
}
// ... reduced to what a lane needs: bit i = the mask's verdict on the lane's column j + W i (classes 128 / 129: set; columns >= 130: clear)
template <int NV, int W>
__device__ __forceinline__ unsigned pitch_mask_own(const unsigned (&m)[4], int j) {
  unsigned own = 0u;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    const int c = j + W * i, w = c >> 5;                           // (W = 16: w = i >> 1, a constant)
    const unsigned word = w == 0 ? m[0] : w == 1 ? m[1] : w == 2 ? m[2] : m[3];
    const unsigned bit = c < 128 ? (word >> (c & 31)) & 1u : (c < 130 ? 1u : 0u);
    own |= bit << i;
  }
  return own;
}
// largest pitch < 128 among the decisions so far: the running `lo` of a lane
__device__ __forceinline__ int pitch_lo_next(int lo, int decision) { return decision < 128 && decision > lo ? decision : lo; }

// THE allowed rule, shared by every decision site (and ptv_debug_pitch_constrain).  v: the NV logits of this lane's columns j + W i;
// own: pitch_mask_own() of the row's mask words; lo, flags as above (flags is uniform over the block: a scalar branch).
// tv: v with the disallowed classes (and the columns >= 130) at -INFINITY -- the input of pitch_keep_threshold(); returns the bitmap of the
// lane's allowed columns: the draw takes column i iff bit i is set and v[i] >= the threshold.
// word: the decision's force word (uniform over the W lanes of the row, it may differ between the rows of a wave); a caller that leaves it
// out compiles to what it did without it.  Two families of it change the set, every other value (a forced class included) does not:
//   PTV_FORCE_NOT_EOS (-2, a kept rhythm): <eos> (129) leaves the allowed set iff another class is allowed.
//   PTV_FORCE_BELOW(u) = -256 - u, u in 1..128 (a kept top voice): lane = the notes c < u (under CONS_ASCENDING also c > lo);
//     the allowed set is lane & mask; if that is empty it is lane (the mask yields); if lane is empty it is <eos> alone.
// The three counts these need -- the allowed classes beside <eos>, lane & mask, lane: each <= 130 -- travel as three bytes of ONE integer
// sum over the row, which every lane takes whatever its word, so nothing diverges around it.
template <int NV, int W>
__device__ __forceinline__ unsigned pitch_constrain(const float (&v)[NV], unsigned own, int lo, unsigned flags, int j, float (&tv)[NV],
                                                    int word = -1) {
  unsigned al = own;
  if (flags & CONS_ASCENDING) {
#pragma unroll
    for (int i = 0; i < NV; i++) {
      const int c = j + W * i;
      if (!(c == 129 || (c < 128 && c > lo))) al &= ~(1u << i);
    }
  }
  {
    constexpr int EI = 129 / W, EJ = 129 % W;                      // <eos> is column EJ + W * EI: bit EI of lane EJ
    static_assert(EI < NV, "the row holds column 129");
    const unsigned eos_bit = j == EJ ? 1u << EI : 0u;
    const bool no_eos = word == -2;                                // PTV_FORCE_NOT_EOS
    const int u = -256 - word;                                     // the ceiling of PTV_FORCE_BELOW(u)
    const bool below = u >= 1 && u <= 128;
    const int lo_u = (flags & CONS_ASCENDING) ? lo : -1;
    unsigned lane = 0u;
#pragma unroll
    for (int i = 0; i < NV; i++) {
      const int c = j + W * i;
      if (below && c < u && c > lo_u) lane |= 1u << i;             // (u <= 128: a note)
    }
    const int sums = row_sum<W>(__popc(al & ~eos_bit) | (__popc(al & lane) << 8) | (__popc(lane) << 16));
    const int others = sums & 0xff, in_mask = (sums >> 8) & 0xff, in_lane = sums >> 16;
    if (below) al = in_mask > 0 ? (al & lane) : (in_lane > 0 ? lane : eos_bit);
    else if (no_eos && others > 0) al &= ~eos_bit;
  }
#pragma unroll
  for (int i = 0; i < NV; i++) tv[i] = (al >> i) & 1u ? v[i] : -INFINITY;
  return al;
}
// ... from the row's four mask words (the step loop and the debug entry, which see a row once)
template <int NV, int W>
__device__ __forceinline__ unsigned pitch_constrain(const float (&v)[NV], const unsigned (&m)[4], int lo, unsigned flags, int j, float (&tv)[NV],
                                                    int word = -1) {
  return pitch_constrain<NV, W>(v, pitch_mask_own<NV, W>(m, j), lo, flags, j, tv, word);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Row-wise decode: the constrained kind with the six scalars of the block -- t_pitch, t_dur, top_k, ln_min_p, top_p_q24 and
// the noise stream sample_offset + row -- replaced by one 32-byte record per row.  The block is the 64 bytes above followed by 16 more: 80
// bytes, ten int64 words.  Of the first 64 the row-wise kernels read only seed, draw, flags and mask (the host writes t_pitch = t_dur = 0,
// top_k = 0, LN_MIN_P_OFF, top_p_q24 = 0, sample_offset = 0); mask, ascending and every force word are honoured as by the 64-byte kind.
//   rows:     the device address of int32 [B, 8], contiguous and 16-byte aligned -- row b:
//             {float t_pitch, float t_dur, int top_k (0 = off), float ln_min_p (LN_MIN_P_OFF = off), uint32 top_p_q24 (0 = off),
//              uint32 reserved = 0, int64 sample_id}
//             the encodings of the scalar block, word for word; sample_id is the g of the Philox counter (sample_words), in place of
//             sample_offset + row, range [0, 2^47).  seed and draw stay shared: sample_id already gives every row its own stream, and a
//             row reproduces alone in a scalar decode that passes its id as sample_offset.
// A row's record is two 16-byte loads, made once per launch by the lanes that decide for the row (rows past B clamped by the caller).
// ---------------------------------------------------------------------------------------------------------------------------------
struct SampleBlockR {
  SampleBlockC s;
  const int* rows;
  unsigned reserved0, reserved1;
};
static_assert(sizeof(SampleBlockR) == 80, "row-wise sampling block: 80 bytes (include/ptvae_hip.h)");
struct RowRule { float t_pitch, t_dur; Trunc tr; long long id; };   // what a kernel keeps of a row's record
__device__ __forceinline__ RowRule load_row_rule(const int* table, long r) {
  const int4 a = *reinterpret_cast<const int4*>(table + r * 8), b = *reinterpret_cast<const int4*>(table + r * 8 + 4);
  return RowRule{__builtin_bit_cast(float, a.x), __builtin_bit_cast(float, a.y),
                 Trunc{a.z, __builtin_bit_cast(float, a.w), (unsigned)b.x},
                 (long long)(((unsigned long long)(unsigned)b.w << 32) | (unsigned)b.z)};
}
__device__ __forceinline__ const int* load_row_table(const void* blk) { return reinterpret_cast<const SampleBlockR*>(blk)->rows; }

// ---------------------------------------------------------------------------------------------------------------------------------
// Duration limits: THE rule of a duration range word, shared by every duration site that honours it (and
// ptv_debug_dur_range).  A note's duration is D = v + 1, v the 5-bit value of its duration bits, bit 0 the most significant.
// word = PTV_FORCE_DUR_RANGE(lo, hi) = -1024 - (lo | hi << 5), 0 <= lo <= hi <= 31 (the words -1024..-2047 of force_dur; all five planes of
// a decision hold the same one): the decision of bit d is free, but v ends in [lo, hi].  With p = the value of the bits 0..d-1 already
// decided, bit value b is ALLOWED iff some completion can still end in the range: the interval [q << (4-d), (q << (4-d)) + (1 << (4-d)) - 1],
// q = 2p + b, meets [lo, hi].  Returns bit b set = value b allowed; a word that is no range word allows both.
// One value allowed: that is the decision (its noise words stay unused); both: the caller's own decision, the first maximum of
// logit + T g; neither (forced bits mixed into a range decision): the bit is free.  A word in -1024..-2047 with lo > hi is no range word.  A word >= 0 still overrides everything:
// forced() comes after.  The draw is the model's own bit-by-bit chain with the infeasible branches cut, NOT the joint renormalised over
// the range.  Only the kernels of the 64-byte kind honour the word; nothing is loaded for it and no state but p is carried.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned dur_range_allowed(int word, int d, int p) {
  const int r = -1024 - word;
  const int lo = r & 31, hi = r >> 5, s = 4 - d;
  if (r < 0 || r > 1023 || lo > hi) return 3u;
  const int a0 = (2 * p) << s, a1 = (2 * p + 1) << s, w = (1 << s) - 1;
  return (a0 <= hi && a0 + w >= lo ? 1u : 0u) | (a1 <= hi && a1 + w >= lo ? 2u : 0u);
}
// ... applied to a decision: `decided` where both values or neither are allowed, else the allowed one
__device__ __forceinline__ int dur_range_bit(int word, int d, int p, int decided) {
  const unsigned al = dur_range_allowed(word, d, p);
  return al == 1u ? 0 : al == 2u ? 1 : decided;
}

}  // namespace ptv
