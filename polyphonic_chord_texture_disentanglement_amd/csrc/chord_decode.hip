// chord_decode.hip -- the row-independent free-running chord decode (inference only).
//   ptv_chord_decide:       the decisions of one chord step -- seeded sampling, kept chords, the step's log p / log q -- and the row's OWN
//                           next token (ptv_chord_token of misc.hip feeds back the union over the batch: the reference's training quirk)
//   ptv_chord_logprob_fold: the 8 steps of a row added in ascending order
//   ptv_chord_decode:       z -> chords in one C call: the products and GRU cells of the chord decoder around ptv_chord_decide
//   ptv_debug_chord_noise:  the noise of ptv_chord_decide through the device function it calls
//   ptv_chord_decide_grammar / ptv_chord_decode_grammar / ptv_debug_chord_vocab_noise: the same step and decode under a chord grammar
//                           (DESIGN.md 7f "Chord grammar"): a rule word per row and step, a vocabulary of chord templates
// The noise lives in the decoder's Philox domain (philox.hpp) at note step n = 15, a slot no note decision uses (n = 0..14), kind 0,
// sub = j < 12: ONE call gives lane j everything it owns -- word 0 root class j, word 1 bass class j, words 2 / 3 class 0 / 1 of chroma bit j.
// The vocabulary draw of the grammar kernel takes sub = 16 + j, j < 16: word k of lane j's call is template j + 16 k.
// Every output element has ONE writer and one fixed summation order: no atomics, no scratch, results bit-identical from run to run.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/ptvae_hip.h"
#include "../../include/ptvae_hip_debug.h"

namespace ptv {

constexpr int CD_STEPS = 8, CD_TOK = 36, CD_NOISE_N = 15;

// the four Gumbel values of lane j at (global sample g, chord step t)
__device__ __forceinline__ void chord_gumbel4(const SampleBlock& s, long long g, int t, int j, float (&out)[4]) {
  unsigned c[4];
  sample_words(s, g, t, CD_NOISE_N, 0, j, c);
#pragma unroll
  for (int w = 0; w < 4; w++) out[w] = gumbel_from_word(c[w]);
}

// sum over the 16 lanes of a DPP row; every lane ends with the same bits (each rotation adds two values that were formed alike)
__device__ __forceinline__ float cd_row_sum(float x) {
  x += __builtin_bit_cast(float, dpp_row_ror<8>(__builtin_bit_cast(int, x)));
  x += __builtin_bit_cast(float, dpp_row_ror<4>(__builtin_bit_cast(int, x)));
  x += __builtin_bit_cast(float, dpp_row_ror<2>(__builtin_bit_cast(int, x)));
  x += __builtin_bit_cast(float, dpp_row_ror<1>(__builtin_bit_cast(int, x)));
  return x;
}

// first maximal index among the 12 live lanes of a row (x of the lanes 12..15 is -inf): the lanes at the maximum offer 15 - j, the
// largest offer is the lowest index.  A row without any lane at its maximum (a NaN logit: outside the contract) answers 0.
__device__ __forceinline__ int cd_first_max(float x, int j) {
  const float m = row_max<16>(x);
  const float o = row_max<16>((j < 12 && x == m) ? (float)(15 - j) : -1.f);
  return o < 0.f ? 0 : 15 - (int)o;
}

// one 12-class head: v the lane's plain logit (-inf on the lanes 12..15), g its Gumbel value, T the temperature, fd >= 0 a forced
// decision -> the decided class; lp = log softmax(v)[d], lq = log softmax(v / T)[d] (0 when forced or T = 0).  All 16 lanes of the row call
// it together and end with the same values.
__device__ __forceinline__ int cd_head12(float v, float g, float T, bool noisy, int fd, int j, int lane, float& lp, float& lq) {
  const float x = (noisy && j < 12) ? perturbed(v, T, g) : v;
  const int free_d = cd_first_max(x, j);
  const int d = fd >= 0 ? fd : free_d;
  const int src = (lane & 48) + d;
  const float m = row_max<16>(v);
  const float s = cd_row_sum(expf(v - m));
  lp = __shfl(v, src, 64) - m - logf(s);
  lq = 0.f;
  if (T > 0.f) {                                                         // (uniform: the block's word)
    const float a = v / T;
    const float ma = row_max<16>(a);
    const float sa = cd_row_sum(expf(a - ma));
    const float q = __shfl(a, src, 64) - ma - logf(sa);
    if (fd < 0) lq = q;
  }
  return d;
}

// 16 lanes (one DPP row) per sample, 16 samples per workgroup.  Nothing diverges around a cross-lane operation: a dead row (b >= B) and
// the lanes 12..15 only guard their loads and stores.  All 16 lanes of a row end with the decisions and the sums, so the stores are
// spread: lanes 0..11 the token parts, lane 12 / 13 the two indices of chord14, lane 14 the float sums, lane 15 the integers.
__global__ void __launch_bounds__(256) chord_decide_kernel(const float* __restrict__ root, const float* __restrict__ chroma,
                                                           const float* __restrict__ bass, int B, int t, const SampleBlock* __restrict__ blk,
                                                           const float* __restrict__ keep_c, const unsigned char* __restrict__ keep_steps,
                                                           int keep_rows, float* __restrict__ tok, float* __restrict__ c,
                                                           float* __restrict__ chord14, float* __restrict__ step_logp,
                                                           float* __restrict__ step_logq, int* __restrict__ step_forced,
                                                           int* __restrict__ step_err) {
  const int lane = threadIdx.x & 63, j = threadIdx.x & 15;
  const long b = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool live = b < B, own = live && j < 12;
  // ---- the logits this lane owns
  float vr = -INFINITY, vb = -INFINITY, e0 = 0.f, e1 = 0.f;
  if (own) {
    vr = root[b * 12 + j]; vb = bass[b * 12 + j];
    e0 = chroma[b * 24 + 2 * j]; e1 = chroma[b * 24 + 2 * j + 1];
  }
  // ---- temperatures and noise
  float Tc = 0.f, Th = 0.f, g[4] = {0.f, 0.f, 0.f, 0.f};
  const bool noisy = blk != nullptr;
  if (noisy) {
    const SampleBlock s = *blk;
    Tc = s.t_pitch; Th = s.t_dur;
    chord_gumbel4(s, s.sample_offset + b, t, j, g);
  }
  // ---- the kept chord of this step: a head's block forces its decision iff it has exactly one non-zero entry
  const bool kept = live && keep_c && keep_steps[(keep_rows == 1 ? 0 : b) * CD_STEPS + t] != 0;
  int nzr = 0, nzb = 0, kbit = 0;
  if (kept && j < 12) {
    const float* kc = keep_c + (b * CD_STEPS + t) * CD_TOK;
    nzr = kc[j] != 0.f; kbit = kc[12 + j] != 0.f; nzb = kc[24 + j] != 0.f;
  }
  const int cr = row_sum<16>(nzr), cb = row_sum<16>(nzb);
  const int ir = row_sum<16>(nzr ? j : 0), ib = row_sum<16>(nzb ? j : 0);
  const int fr = (kept && cr == 1) ? ir : -1, fb = (kept && cb == 1) ? ib : -1;
  const int err = (kept && (cr != 1 || cb != 1)) ? 1 : 0;
  // ---- root and bass
  float lpr, lqr, lpb, lqb;
  const int dr = cd_head12(vr, g[0], Tc, noisy, fr, j, lane, lpr, lqr);
  const int db = cd_head12(vb, g[1], Tc, noisy, fb, j, lane, lpb, lqb);
  // ---- chroma bit j: two classes, the first maximum wins
  const float x0 = noisy ? perturbed(e0, Th, g[2]) : e0, x1 = noisy ? perturbed(e1, Th, g[3]) : e1;
  const int bit = kept ? kbit : (x1 > x0 ? 1 : 0);
  const float dm = fmaxf(e0, e1);
  const float lpc1 = (bit ? e1 : e0) - dm - logf(expf(e0 - dm) + expf(e1 - dm));
  float lqc1 = 0.f;
  if (Th > 0.f) {
    const float a0 = e0 / Th, a1 = e1 / Th, am = fmaxf(a0, a1);
    const float q = (bit ? a1 : a0) - am - logf(expf(a0 - am) + expf(a1 - am));
    if (!kept) lqc1 = q;
  }
  float lpc = 0.f, lqc = 0.f;                                            // the 12 bits in ascending order: every lane adds the same values
#pragma unroll
  for (int k = 0; k < 12; k++) {
    lpc += __shfl(lpc1, (lane & 48) + k, 64);
    lqc += __shfl(lqc1, (lane & 48) + k, 64);
  }
  // ---- stores
  if (!live) return;
  const long row = b * CD_STEPS + t;
  if (j < 12) {
    const float tr = j == dr ? 1.f : 0.f, tb = j == db ? 1.f : 0.f, tc = (float)bit;
    if (tok) { float* o = tok + b * CD_TOK; o[j] = tr; o[12 + j] = tc; o[24 + j] = tb; }
    float* o = c + row * CD_TOK;
    o[j] = tr; o[12 + j] = tc; o[24 + j] = tb;
    chord14[row * 14 + 1 + j] = tc;
  } else if (j == 12) {
    chord14[row * 14] = (float)dr;
  } else if (j == 13) {
    chord14[row * 14 + 13] = (float)db;
  } else if (j == 14) {
    float* p = step_logp + row * 3; float* q = step_logq + row * 3;
    p[0] = lpr; p[1] = lpc; p[2] = lpb;
    q[0] = lqr; q[1] = lqc; q[2] = lqb;
  } else {
    int* f = step_forced + row * 3;
    f[0] = fr >= 0 ? 1 : 0; f[1] = kept ? 12 : 0; f[2] = fb >= 0 ? 1 : 0;
    step_err[row] = err;
  }
}

// ---------------------------------------------------------------------------------------------
// The chord grammar (include/ptvae_hip.h "Chord grammar"): chord_decide_kernel's step under a rule word per (row, step) and a vocabulary of
// root-relative chord templates.  Root, then chroma given the root, then bass given both; every set is judged on the plain logits.
// ---------------------------------------------------------------------------------------------
constexpr int CG_MAX_VOCAB = 64, CG_IDENTITY = 0x00ffffff;

// the Philox words and the Gumbel values of the templates j, j + 16, j + 32, j + 48 (lane j < 16) at (global sample g, chord step t)
__device__ __forceinline__ void chord_vocab_gumbel4(const SampleBlock& s, long long g, int t, int j, unsigned (&c)[4], float (&out)[4]) {
  sample_words(s, g, t, CD_NOISE_N, 0, 16 + j, c);
#pragma unroll
  for (int w = 0; w < 4; w++) out[w] = gumbel_from_word(c[w]);
}

// cd_head12 over an allowed set (al: this lane's class is in it; never empty over the row): the decision and lq see the allowed classes
// only, lp is the model's own log softmax over all 12.  With every class allowed the arithmetic is cd_head12's, operation for operation.
__device__ __forceinline__ int cg_head12(float v, float g, float T, bool noisy, int fd, bool al, int j, int lane, float& lp, float& lq) {
  const float x = al ? ((noisy && j < 12) ? perturbed(v, T, g) : v) : -INFINITY;
  const int free_d = cd_first_max(x, j);
  const int d = fd >= 0 ? fd : free_d;
  const int src = (lane & 48) + d;
  const float m = row_max<16>(v);
  const float s = cd_row_sum(expf(v - m));
  lp = __shfl(v, src, 64) - m - logf(s);
  lq = 0.f;
  if (T > 0.f) {                                                         // (uniform: the block's word)
    const float a = al ? v / T : -INFINITY;
    const float ma = row_max<16>(a);
    const float sa = cd_row_sum(expf(a - ma));
    const float q = __shfl(a, src, 64) - ma - logf(sa);
    if (fd < 0) lq = q;
  }
  return d;
}

// Geometry, stores and the kept step as chord_decide_kernel.  The rule word and the vocabulary are uniform over a row's 16 lanes; every
// cross-lane step runs for every lane whatever the word says, and the word only selects between values.
__global__ void __launch_bounds__(256) chord_decide_grammar_kernel(const float* __restrict__ root, const float* __restrict__ chroma,
                                                                   const float* __restrict__ bass, int B, int t,
                                                                   const SampleBlock* __restrict__ blk, const float* __restrict__ keep_c,
                                                                   const unsigned char* __restrict__ keep_steps, int keep_rows,
                                                                   const int* __restrict__ rule, int rule_rows, const int* __restrict__ vocab,
                                                                   int V, float* __restrict__ tok, float* __restrict__ c,
                                                                   float* __restrict__ chord14, float* __restrict__ step_logp,
                                                                   float* __restrict__ step_logq, int* __restrict__ step_forced,
                                                                   int* __restrict__ step_err) {
  const int lane = threadIdx.x & 63, j = threadIdx.x & 15, base = lane & 48;
  const long b = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool live = b < B, own = live && j < 12;
  // ---- the logits this lane owns
  float vr = -INFINITY, vb = -INFINITY, e0 = 0.f, e1 = 0.f;
  if (own) {
    vr = root[b * 12 + j]; vb = bass[b * 12 + j];
    e0 = chroma[b * 24 + 2 * j]; e1 = chroma[b * 24 + 2 * j + 1];
  }
  // ---- temperatures and noise
  float Tc = 0.f, Th = 0.f, g[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
  const bool noisy = blk != nullptr;
  if (noisy) {
    const SampleBlock s = *blk;
    Tc = s.t_pitch; Th = s.t_dur;
    chord_gumbel4(s, s.sample_offset + b, t, j, g);
    if (V > 0) {                                                         // (uniform over the launch; no cross-lane step inside)
      unsigned wv[4];
      chord_vocab_gumbel4(s, s.sample_offset + b, t, j, wv, gv);
    }
  }
  // ---- the kept chord of this step: a head's block forces its decision iff it has exactly one non-zero entry
  const bool kept = live && keep_c && keep_steps[(keep_rows == 1 ? 0 : b) * CD_STEPS + t] != 0;
  int nzr = 0, nzb = 0, kbit = 0;
  if (kept && j < 12) {
    const float* kc = keep_c + (b * CD_STEPS + t) * CD_TOK;
    nzr = kc[j] != 0.f; kbit = kc[12 + j] != 0.f; nzb = kc[24 + j] != 0.f;
  }
  const int cr = row_sum<16>(nzr), cb = row_sum<16>(nzb);
  const int ir = row_sum<16>(nzr ? j : 0), ib = row_sum<16>(nzb ? j : 0);
  const int fr = (kept && cr == 1) ? ir : -1, fb = (kept && cb == 1) ? ib : -1;
  int err = (kept && (cr != 1 || cb != 1)) ? 1 : 0;
  // ---- the rule of (row, step) and the templates this lane owns; a kept step does not consult the rule
  int word = CG_IDENTITY, tm[4] = {0, 0, 0, 0};
  if (live && !kept) word = rule[(rule_rows == 1 ? 0 : b) * CD_STEPS + t];
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (j + 16 * k < V) tm[k] = vocab[j + 16 * k] & 0xfff;
  const int cmask = (word >> 12) & 0xfff;
  const bool use_vocab = (word & PTV_CHORD_RULE_VOCAB) != 0 && V > 0;
  const bool root_in = (word & PTV_CHORD_RULE_ROOT_IN_CHORD) != 0, bass_in = (word & PTV_CHORD_RULE_BASS_IN_CHORD) != 0;
  // ---- root over the allowed roots (none: all twelve, error bit 1)
  int rmask = word & 0xfff;
  if (rmask == 0) { rmask = 0xfff; err |= PTV_CHORD_ERR_ROOT_MASK; }
  float lpr, lqr, lpb, lqb;
  const int dr = cg_head12(vr, g[0], Tc, noisy, fr, ((rmask >> j) & 1) != 0, j, lane, lpr, lqr);
  // ---- chroma bit j without a vocabulary: free where the mask allows it, else 0; the root's bit 1 under ROOT_IN_CHORD
  const bool bit_free = ((cmask >> j) & 1) != 0 && !(root_in && j == dr);
  const float x0 = noisy ? perturbed(e0, Th, g[2]) : e0, x1 = noisy ? perturbed(e1, Th, g[3]) : e1;
  const int mbit = (root_in && j == dr) ? 1 : (bit_free && x1 > x0 ? 1 : 0);
  // ---- chroma from the vocabulary: template v on the root is A_v, its score the sum of the decided classes' logits over the 12 bits
  const int fit = cmask | (1 << dr);
  float sv[4], xv[4];
  int av[4], nfit = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    av[k] = ((tm[k] << dr) | (tm[k] >> (12 - dr))) & 0xfff;
    nfit += (j + 16 * k < V && (av[k] & ~fit) == 0) ? 1 : 0;
    sv[k] = 0.f;
  }
#pragma unroll
  for (int p = 0; p < 12; p++) {
    const float p0 = __shfl(e0, base + p, 64), p1 = __shfl(e1, base + p, 64);
#pragma unroll
    for (int k = 0; k < 4; k++) sv[k] += ((av[k] >> p) & 1) ? p1 : p0;
  }
  const bool none_fits = row_sum<16>(nfit) == 0;                         // the vocabulary wins, the mask yields (error bit 2)
  if (use_vocab && none_fits) err |= PTV_CHORD_ERR_NO_TEMPLATE;
  bool alv[4];
  float bx = -INFINITY;
  int bv = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    alv[k] = j + 16 * k < V && (none_fits || (av[k] & ~fit) == 0);
    xv[k] = alv[k] ? (noisy ? perturbed(sv[k], Th, gv[k]) : sv[k]) : -INFINITY;
    if (k == 0 || xv[k] > bx) { bx = xv[k]; bv = j + 16 * k; }           // (the lowest k of a lane's ties)
  }
  const float mx = row_max<16>(bx);
  const float ov = row_max<16>(bx == mx ? (float)(CG_MAX_VOCAB - 1 - bv) : -1.f);
  const int dv = ov < 0.f ? 0 : CG_MAX_VOCAB - 1 - (int)ov;             // first maximal template
  const int kv = dv >> 4, srcv = base + (dv & 15);
  const int a_dec = __shfl(kv == 0 ? av[0] : kv == 1 ? av[1] : kv == 2 ? av[2] : av[3], srcv, 64);
  float lqv = 0.f;
  if (Th > 0.f) {                                                        // (uniform: the block's word)
    float a[4], ma = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; k++) { a[k] = alv[k] ? sv[k] / Th : -INFINITY; ma = fmaxf(ma, a[k]); }
    ma = row_max<16>(ma);
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) part += alv[k] ? expf(a[k] - ma) : 0.f;
    const float sa = cd_row_sum(part);
    const float ad = __shfl(kv == 0 ? a[0] : kv == 1 ? a[1] : kv == 2 ? a[2] : a[3], srcv, 64);
    lqv = ad - ma - logf(sa);
  }
  // ---- the step's bit j and its two figures
  const int bit = kept ? kbit : (use_vocab ? (a_dec >> j) & 1 : mbit);
  const float dm = fmaxf(e0, e1);
  const float lpc1 = (bit ? e1 : e0) - dm - logf(expf(e0 - dm) + expf(e1 - dm));
  float lqc1 = 0.f;
  if (Th > 0.f) {
    const float a0 = e0 / Th, a1 = e1 / Th, am = fmaxf(a0, a1);
    const float q = (bit ? a1 : a0) - am - logf(expf(a0 - am) + expf(a1 - am));
    if (!kept && bit_free) lqc1 = q;
  }
  float lpc = 0.f, lqc = 0.f;                                            // the 12 bits in ascending order: every lane adds the same values
#pragma unroll
  for (int k = 0; k < 12; k++) {
    lpc += __shfl(lpc1, base + k, 64);
    lqc += __shfl(lqc1, base + k, 64);
  }
  if (use_vocab) lqc = kept ? 0.f : lqv;                                 // (a kept step has the identity word: never taken with kept)
  // ---- bass over the decided chord's tones (no tone: all twelve, error bit 3)
  const int bits12 = row_sum<16>(j < 12 ? bit << j : 0);
  int bmask = 0xfff;
  if (bass_in) {
    if (bits12 == 0) err |= PTV_CHORD_ERR_NO_BASS;
    else bmask = ((bits12 >> dr) | (bits12 << (12 - dr))) & 0xfff;       // interval i <-> pitch class (root + i) % 12
  }
  const int db = cg_head12(vb, g[1], Tc, noisy, fb, ((bmask >> j) & 1) != 0, j, lane, lpb, lqb);
  // ---- stores
  if (!live) return;
  const long row = b * CD_STEPS + t;
  if (j < 12) {
    const float tr = j == dr ? 1.f : 0.f, tb = j == db ? 1.f : 0.f, tc = (float)bit;
    if (tok) { float* o = tok + b * CD_TOK; o[j] = tr; o[12 + j] = tc; o[24 + j] = tb; }
    float* o = c + row * CD_TOK;
    o[j] = tr; o[12 + j] = tc; o[24 + j] = tb;
    chord14[row * 14 + 1 + j] = tc;
  } else if (j == 12) {
    chord14[row * 14] = (float)dr;
  } else if (j == 13) {
    chord14[row * 14 + 13] = (float)db;
  } else if (j == 14) {
    float* p = step_logp + row * 3; float* q = step_logq + row * 3;
    p[0] = lpr; p[1] = lpc; p[2] = lpb;
    q[0] = lqr; q[1] = lqc; q[2] = lqb;
  } else {
    int* f = step_forced + row * 3;
    f[0] = fr >= 0 ? 1 : 0; f[1] = kept ? 12 : 0; f[2] = fb >= 0 ? 1 : 0;
    step_err[row] = err;
  }
}

// thread (b, column): columns 0..2 = logp, 3..5 = logq, 6..8 = forced, 9 = err; t = 0..7 in ascending order
__global__ void chord_logprob_fold_kernel(const float* __restrict__ step_logp, const float* __restrict__ step_logq,
                                          const int* __restrict__ step_forced, const int* __restrict__ step_err, int B,
                                          float* __restrict__ logp, float* __restrict__ logq, int* __restrict__ forced,
                                          int* __restrict__ err) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * 10) return;
  const long b = i / 10; const int col = (int)(i % 10);
  if (col < 6) {
    const float* src = col < 3 ? step_logp : step_logq;
    const int h = col < 3 ? col : col - 3;
    float s = 0.f;
    for (int t = 0; t < CD_STEPS; t++) s += src[(b * CD_STEPS + t) * 3 + h];
    (col < 3 ? logp : logq)[b * 3 + h] = s;
  } else if (col < 9) {
    int s = 0;
    for (int t = 0; t < CD_STEPS; t++) s += step_forced[(b * CD_STEPS + t) * 3 + (col - 6)];
    forced[b * 3 + (col - 6)] = s;
  } else {
    int e = 0;
    for (int t = 0; t < CD_STEPS; t++) e |= step_err[b * CD_STEPS + t];
    err[b] = e;
  }
}

__global__ void chord_noise_kernel(const SampleBlock* __restrict__ blk, long rows, int t, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 12) return;
  const long r = i / 12; const int j = (int)(i % 12);
  const SampleBlock s = *blk;
  float g[4];
  chord_gumbel4(s, s.sample_offset + r, t, j, g);
#pragma unroll
  for (int w = 0; w < 4; w++) out[i * 4 + w] = g[w];
}

// thread (row, template v < V): the Gumbel value of template v and the 32-bit word it was made from
__global__ void chord_vocab_noise_kernel(const SampleBlock* __restrict__ blk, long rows, int t, int V, float* __restrict__ out,
                                         unsigned* __restrict__ words) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * V) return;
  const long r = i / V; const int v = (int)(i % V);
  const SampleBlock s = *blk;
  unsigned c[4];
  float g[4];
  chord_vocab_gumbel4(s, s.sample_offset + r, t, v & 15, c, g);
  const int k = v >> 4;
  out[i] = k == 0 ? g[0] : k == 1 ? g[1] : k == 2 ? g[2] : g[3];
  words[i] = k == 0 ? c[0] : k == 1 ? c[1] : k == 2 ? c[2] : c[3];
}

inline const void* T_(const void* const* t, int i) { return t[i]; }
template <typename X> inline X* M_(const void* const* t, int i) { return reinterpret_cast<X*>(const_cast<void*>(t[i])); }

}  // namespace ptv

using namespace ptv;

extern "C" int ptv_chord_decide(const float* root, const float* chroma, const float* bass, int B, int t, const void* sample,
                                const float* keep_c, const unsigned char* keep_steps, int keep_rows, float* tok, float* c, float* chord14,
                                float* step_logp, float* step_logq, int* step_forced, int* step_err, void* stream) {
  if (!root || !chroma || !bass || !c || !chord14 || !step_logp || !step_logq || !step_forced || !step_err) return PTV_ERR_ARG;
  if (B < 1 || t < 0 || t >= CD_STEPS) return PTV_ERR_ARG;
  if (keep_c && (!keep_steps || (keep_rows != 1 && keep_rows != B))) return PTV_ERR_ARG;
  hipLaunchKernelGGL(chord_decide_kernel, dim3(cdiv((long)B * 16, 256)), dim3(256), 0, (hipStream_t)stream, root, chroma, bass, B, t,
                     reinterpret_cast<const SampleBlock*>(sample), keep_c, keep_steps, keep_rows, tok, c, chord14, step_logp, step_logq,
                     step_forced, step_err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_chord_logprob_fold(const float* step_logp, const float* step_logq, const int* step_forced, const int* step_err, int B,
                                      float* logp, float* logq, int* forced, int* err, void* stream) {
  if (!step_logp || !step_logq || !step_forced || !step_err || !logp || !logq || !forced || !err || B < 1) return PTV_ERR_ARG;
  hipLaunchKernelGGL(chord_logprob_fold_kernel, dim3(cdiv((long)B * 10, 256)), dim3(256), 0, (hipStream_t)stream, step_logp, step_logq,
                     step_forced, step_err, B, logp, logq, forced, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_chord_decide_grammar(const float* root, const float* chroma, const float* bass, int B, int t, const void* sample,
                                        const float* keep_c, const unsigned char* keep_steps, int keep_rows, const int* rule, int rule_rows,
                                        const int* vocab, int n_vocab, float* tok, float* c, float* chord14, float* step_logp,
                                        float* step_logq, int* step_forced, int* step_err, void* stream) {
  if (!root || !chroma || !bass || !c || !chord14 || !step_logp || !step_logq || !step_forced || !step_err) return PTV_ERR_ARG;
  if (B < 1 || t < 0 || t >= CD_STEPS) return PTV_ERR_ARG;
  if (keep_c && (!keep_steps || (keep_rows != 1 && keep_rows != B))) return PTV_ERR_ARG;
  if (!rule || (rule_rows != 1 && rule_rows != B)) return PTV_ERR_ARG;
  if (n_vocab < 0 || n_vocab > CG_MAX_VOCAB || (n_vocab > 0 && !vocab)) return PTV_ERR_ARG;
  hipLaunchKernelGGL(chord_decide_grammar_kernel, dim3(cdiv((long)B * 16, 256)), dim3(256), 0, (hipStream_t)stream, root, chroma, bass, B, t,
                     reinterpret_cast<const SampleBlock*>(sample), keep_c, keep_steps, keep_rows, rule, rule_rows, vocab, n_vocab, tok, c,
                     chord14, step_logp, step_logq, step_forced, step_err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

// ---------------------------------------------------------------------------------------------
// ptv_chord_decode / ptv_chord_decode_grammar: the launches a Python sequencing of the same entry points makes, in the same order with the
// same arguments (the same bits): z -> h0, z_in and the z part of the input product; per step the token part (K = 36), the GRU cell, the
// three heads and the decisions; the fold.  4 + 8 * 6 + 1 launches.  The grammar's tables repeat the plain decode's slot for slot and add
// theirs behind them, so ONE sequence serves both: rule = NULL is the plain decide.
// ---------------------------------------------------------------------------------------------
#define CDG_SAME(name) static_assert((int)PTV_CDG_##name == (int)PTV_CDS_##name, "PTV_CDG_" #name " is PTV_CDS_" #name)
CDG_SAME(Z); CDG_SAME(W_ZHID); CDG_SAME(B_ZHID); CDG_SAME(W_ZIN); CDG_SAME(B_ZIN); CDG_SAME(INIT_INPUT); CDG_SAME(W_IH);
CDG_SAME(B_IH); CDG_SAME(W_HH); CDG_SAME(B_HH); CDG_SAME(W_ROOT); CDG_SAME(B_ROOT); CDG_SAME(W_CHROMA); CDG_SAME(B_CHROMA);
CDG_SAME(W_BASS); CDG_SAME(B_BASS); CDG_SAME(SAMPLE); CDG_SAME(KEEP_C); CDG_SAME(KEEP_STEPS); CDG_SAME(HALL); CDG_SAME(Z_IN);
CDG_SAME(ZG); CDG_SAME(GI); CDG_SAME(TOK); CDG_SAME(ROOT); CDG_SAME(CHROMA); CDG_SAME(BASS); CDG_SAME(C); CDG_SAME(CHORD14);
CDG_SAME(STEP_LOGP); CDG_SAME(STEP_LOGQ); CDG_SAME(STEP_FORCED); CDG_SAME(STEP_ERR); CDG_SAME(LOGP); CDG_SAME(LOGQ); CDG_SAME(FORCED);
CDG_SAME(ERR); CDG_SAME(D_B); CDG_SAME(D_H); CDG_SAME(D_Z); CDG_SAME(D_ZI); CDG_SAME(D_PREC); CDG_SAME(D_KEEP_ROWS);
#undef CDG_SAME
static_assert(PTV_CDS_COUNT == 37 && PTV_CDS_D_COUNT == 6, "a slot added to the plain decode's tables: add it to the grammar's and to the list above");
static_assert((int)PTV_CDG_RULE == (int)PTV_CDS_COUNT && (int)PTV_CDG_VOCAB == PTV_CDS_COUNT + 1 && PTV_CDG_COUNT == PTV_CDS_COUNT + 2 &&
              (int)PTV_CDG_D_RULE_ROWS == (int)PTV_CDS_D_COUNT && (int)PTV_CDG_D_N_VOCAB == PTV_CDS_D_COUNT + 1 &&
              PTV_CDG_D_COUNT == PTV_CDS_D_COUNT + 2, "the grammar decode's own slots follow the plain decode's");
static int chord_decode_launches(const void* const* t, const long* d, const int* rule, int rule_rows, const int* vocab, int n_vocab,
                                 void* stream) {
  for (int i = 0; i < PTV_CDS_COUNT; i++)
    if (!t[i] && i != PTV_CDS_SAMPLE && i != PTV_CDS_KEEP_C && i != PTV_CDS_KEEP_STEPS) return PTV_ERR_ARG;
  const int B = (int)d[PTV_CDS_D_B], H = (int)d[PTV_CDS_D_H], Z = (int)d[PTV_CDS_D_Z], Zi = (int)d[PTV_CDS_D_ZI], P = (int)d[PTV_CDS_D_PREC],
            kr = (int)d[PTV_CDS_D_KEEP_ROWS];
  if (d[PTV_CDS_D_B] <= 0 || d[PTV_CDS_D_B] > (1L << 26) || H <= 0 || (H & 3) || Z <= 0 || Zi <= 0 || (P != PTV_PREC_F32 && P != PTV_PREC_BF16))
    return PTV_ERR_ARG;
  const float* keep_c = (const float*)T_(t, PTV_CDS_KEEP_C);
  const unsigned char* keep_steps = (const unsigned char*)T_(t, PTV_CDS_KEEP_STEPS);
  if (keep_c ? (!keep_steps || (kr != 1 && kr != B)) : keep_steps != nullptr) return PTV_ERR_ARG;
  if (rule && ((rule_rows != 1 && rule_rows != B) || n_vocab < 0 || n_vocab > CG_MAX_VOCAB || (n_vocab > 0 && !vocab))) return PTV_ERR_ARG;
  constexpr int I = CD_TOK, T = CD_STEPS;
  float* hall = M_<float>(t, PTV_CDS_HALL);
  float* tok = M_<float>(t, PTV_CDS_TOK);
  float* gi = M_<float>(t, PTV_CDS_GI);
  const float* zg = (const float*)T_(t, PTV_CDS_ZG);
  const float* w_ih = (const float*)T_(t, PTV_CDS_W_IH);
  const long ld_ih = (long)I + Zi;
  float* root = M_<float>(t, PTV_CDS_ROOT); float* chroma = M_<float>(t, PTV_CDS_CHROMA); float* bass = M_<float>(t, PTV_CDS_BASS);
  PTV_TRY(ptv_gemm(P, 0, 0, B, H, Z, T_(t, PTV_CDS_Z), Z, T_(t, PTV_CDS_W_ZHID), Z, hall, H, (const float*)T_(t, PTV_CDS_B_ZHID), 1.f, 0, 0, 0, 0, stream));
  PTV_TRY(ptv_gemm(P, 0, 0, B, Zi, Z, T_(t, PTV_CDS_Z), Z, T_(t, PTV_CDS_W_ZIN), Z, M_<void>(t, PTV_CDS_Z_IN), Zi, (const float*)T_(t, PTV_CDS_B_ZIN), 1.f,
                   0, 0, 0, 0, stream));
  PTV_TRY(ptv_gemm(P, 0, 0, B, 3 * H, Zi, T_(t, PTV_CDS_Z_IN), Zi, w_ih + I, ld_ih, M_<void>(t, PTV_CDS_ZG), 3L * H, (const float*)T_(t, PTV_CDS_B_IH),
                   1.f, 0, 0, 0, 0, stream));
  PTV_TRY(ptv_copy2d(tok, I, (const float*)T_(t, PTV_CDS_INIT_INPUT), 0, B, I, 1.f, 0, stream));
  for (int s = 0; s < T; s++) {
    float* hprev = hall + (long)s * B * H;
    float* hout = hprev + (long)B * H;
    float* rs = root + (long)s * B * 12; float* cs = chroma + (long)s * B * 24; float* bs = bass + (long)s * B * 12;
    PTV_TRY(ptv_gemm(P, 0, 0, B, 3 * H, I, tok, I, w_ih, ld_ih, gi, 3L * H, nullptr, 1.f, 0, 0, 0, 0, stream));
    PTV_TRY(ptv_gru_step_fwd(P, B, H, hprev, H, nullptr, nullptr, gi, 3L * H, zg, 3L * H, T_(t, PTV_CDS_W_HH), (const float*)T_(t, PTV_CDS_B_HH),
                             hout, H, nullptr, 0, nullptr, 0, nullptr, 0, stream));
    PTV_TRY(ptv_gemm(P, 0, 0, B, 12, H, hout, H, T_(t, PTV_CDS_W_ROOT), H, rs, 12, (const float*)T_(t, PTV_CDS_B_ROOT), 1.f, 0, 0, 0, 0, stream));
    PTV_TRY(ptv_gemm(P, 0, 0, B, 24, H, hout, H, T_(t, PTV_CDS_W_CHROMA), H, cs, 24, (const float*)T_(t, PTV_CDS_B_CHROMA), 1.f, 0, 0, 0, 0, stream));
    PTV_TRY(ptv_gemm(P, 0, 0, B, 12, H, hout, H, T_(t, PTV_CDS_W_BASS), H, bs, 12, (const float*)T_(t, PTV_CDS_B_BASS), 1.f, 0, 0, 0, 0, stream));
    float* next = s + 1 < T ? tok : nullptr;
    if (rule) {
      PTV_TRY(ptv_chord_decide_grammar(rs, cs, bs, B, s, T_(t, PTV_CDS_SAMPLE), keep_c, keep_steps, kr, rule, rule_rows, vocab, n_vocab, next,
                                       M_<float>(t, PTV_CDS_C), M_<float>(t, PTV_CDS_CHORD14), M_<float>(t, PTV_CDS_STEP_LOGP),
                                       M_<float>(t, PTV_CDS_STEP_LOGQ), M_<int>(t, PTV_CDS_STEP_FORCED), M_<int>(t, PTV_CDS_STEP_ERR), stream));
    } else {
      PTV_TRY(ptv_chord_decide(rs, cs, bs, B, s, T_(t, PTV_CDS_SAMPLE), keep_c, keep_steps, kr, next, M_<float>(t, PTV_CDS_C),
                               M_<float>(t, PTV_CDS_CHORD14), M_<float>(t, PTV_CDS_STEP_LOGP), M_<float>(t, PTV_CDS_STEP_LOGQ),
                               M_<int>(t, PTV_CDS_STEP_FORCED), M_<int>(t, PTV_CDS_STEP_ERR), stream));
    }
  }
  return ptv_chord_logprob_fold((const float*)T_(t, PTV_CDS_STEP_LOGP), (const float*)T_(t, PTV_CDS_STEP_LOGQ), (const int*)T_(t, PTV_CDS_STEP_FORCED),
                                (const int*)T_(t, PTV_CDS_STEP_ERR), B, M_<float>(t, PTV_CDS_LOGP), M_<float>(t, PTV_CDS_LOGQ),
                                M_<int>(t, PTV_CDS_FORCED), M_<int>(t, PTV_CDS_ERR), stream);
}

extern "C" int ptv_chord_decode(const void* const* t, const long* d, void* stream) {
  if (!t || !d) return PTV_ERR_ARG;
  return chord_decode_launches(t, d, nullptr, 0, nullptr, 0, stream);
}

extern "C" int ptv_chord_decode_grammar(const void* const* t, const long* d, void* stream) {
  if (!t || !d || !t[PTV_CDG_RULE]) return PTV_ERR_ARG;
  return chord_decode_launches(t, d, (const int*)T_(t, PTV_CDG_RULE), (int)d[PTV_CDG_D_RULE_ROWS], (const int*)T_(t, PTV_CDG_VOCAB),
                               (int)d[PTV_CDG_D_N_VOCAB], stream);
}

extern "C" int ptv_debug_chord_noise(const void* block, long rows, int t, float* out, void* stream) {
  if (!block || !out || rows < 1 || t < 0 || t >= CD_STEPS) return PTV_ERR_ARG;
  hipLaunchKernelGGL(chord_noise_kernel, dim3(cdiv(rows * 12, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const SampleBlock*>(block), rows, t, out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_debug_chord_vocab_noise(const void* block, long rows, int t, int n_vocab, float* out, unsigned* words, void* stream) {
  if (!block || !out || !words || rows < 1 || t < 0 || t >= CD_STEPS || n_vocab < 1 || n_vocab > CG_MAX_VOCAB) return PTV_ERR_ARG;
  hipLaunchKernelGGL(chord_vocab_noise_kernel, dim3(cdiv(rows * n_vocab, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const SampleBlock*>(block), rows, t, n_vocab, out, words);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
