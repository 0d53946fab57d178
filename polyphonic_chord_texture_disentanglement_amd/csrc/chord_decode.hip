// chord_decode.hip -- the row-independent free-running chord decode (inference only).
//   ptv_chord_decide:       the decisions of one chord step -- seeded sampling, kept chords, the step's log p / log q -- and the row's OWN
//                           next token (ptv_chord_token of misc.hip feeds back the union over the batch: the reference's training quirk)
//   ptv_chord_logprob_fold: the 8 steps of a row added in ascending order
//   ptv_chord_decode:       z -> chords in one C call: the products and GRU cells of the chord decoder around ptv_chord_decide
//   ptv_debug_chord_noise:  the noise of ptv_chord_decide through the device function it calls
// The noise lives in the decoder's Philox domain (philox.hpp) at note step n = 15, a slot no note decision uses (n = 0..14), kind 0,
// sub = j < 12: ONE call gives lane j everything it owns -- word 0 root class j, word 1 bass class j, words 2 / 3 class 0 / 1 of chroma bit j.
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

// ---------------------------------------------------------------------------------------------
// ptv_chord_decode: the launches a Python sequencing of the same entry points makes, in the same order with the same arguments (the same
// bits): z -> h0, z_in and the z part of the input product; per step the token part (K = 36), the GRU cell, the three heads and the
// decisions; the fold.  4 + 8 * 6 + 1 launches.
// ---------------------------------------------------------------------------------------------
extern "C" int ptv_chord_decode(const void* const* t, const long* d, void* stream) {
  if (!t || !d) return PTV_ERR_ARG;
  for (int i = 0; i < PTV_CDS_COUNT; i++)
    if (!t[i] && i != PTV_CDS_SAMPLE && i != PTV_CDS_KEEP_C && i != PTV_CDS_KEEP_STEPS) return PTV_ERR_ARG;
  const int B = (int)d[PTV_CDS_D_B], H = (int)d[PTV_CDS_D_H], Z = (int)d[PTV_CDS_D_Z], Zi = (int)d[PTV_CDS_D_ZI], P = (int)d[PTV_CDS_D_PREC],
            kr = (int)d[PTV_CDS_D_KEEP_ROWS];
  if (d[PTV_CDS_D_B] <= 0 || d[PTV_CDS_D_B] > (1L << 26) || H <= 0 || (H & 3) || Z <= 0 || Zi <= 0 || (P != PTV_PREC_F32 && P != PTV_PREC_BF16))
    return PTV_ERR_ARG;
  const float* keep_c = (const float*)T_(t, PTV_CDS_KEEP_C);
  const unsigned char* keep_steps = (const unsigned char*)T_(t, PTV_CDS_KEEP_STEPS);
  if (keep_c ? (!keep_steps || (kr != 1 && kr != B)) : keep_steps != nullptr) return PTV_ERR_ARG;
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
    PTV_TRY(ptv_chord_decide(rs, cs, bs, B, s, T_(t, PTV_CDS_SAMPLE), keep_c, keep_steps, kr, s + 1 < T ? tok : nullptr, M_<float>(t, PTV_CDS_C),
                             M_<float>(t, PTV_CDS_CHORD14), M_<float>(t, PTV_CDS_STEP_LOGP), M_<float>(t, PTV_CDS_STEP_LOGQ),
                             M_<int>(t, PTV_CDS_STEP_FORCED), M_<int>(t, PTV_CDS_STEP_ERR), stream));
  }
  return ptv_chord_logprob_fold((const float*)T_(t, PTV_CDS_STEP_LOGP), (const float*)T_(t, PTV_CDS_STEP_LOGQ), (const int*)T_(t, PTV_CDS_STEP_FORCED),
                                (const int*)T_(t, PTV_CDS_STEP_ERR), B, M_<float>(t, PTV_CDS_LOGP), M_<float>(t, PTV_CDS_LOGQ),
                                M_<int>(t, PTV_CDS_FORCED), M_<int>(t, PTV_CDS_ERR), stream);
}

extern "C" int ptv_debug_chord_noise(const void* block, long rows, int t, float* out, void* stream) {
  if (!block || !out || rows < 1 || t < 0 || t >= CD_STEPS) return PTV_ERR_ARG;
  hipLaunchKernelGGL(chord_noise_kernel, dim3(cdiv(rows * 12, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const SampleBlock*>(block), rows, t, out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
