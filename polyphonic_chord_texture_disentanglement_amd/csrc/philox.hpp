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

}  // namespace ptv
