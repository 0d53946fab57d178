// score.hip -- per-sample scores of a teacher-forced pass and the counts behind the reconstruction accuracies (forward only).
//   ptv_recon_step_scores: per (sample, time step) the pitch / duration NLL sums and the arg-max hit counts, one pass over the logits
//   ptv_score_fold:        the 32 time steps of a sample added in ascending order
//   ptv_kl_rows:           KL(N(mu, sd) || N(0, 1)) summed over the latent, one figure per sample
//   ptv_chord_step_scores: root / chroma / bass NLL sums and hit counts per sample
//   ptv_roll_match:        cell counts of two piano-rolls (onset / exact matches)
// Every output element has ONE writer and one fixed summation order: no float atomics, no scratch, results bit-identical from run to run
// and independent of the logits' layout.  A row or bit whose target is ignored is never loaded (the guarantee loss()'s dead-step
// elision relies on: those rows may be unwritten memory).
#include "common.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

constexpr int SC_NP = 130;      // pitch classes; 130 itself is the ignored target

__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per (sample b, time step t); its two half-waves take the note steps n = 2k and 2k + 1, k = 0..7, so a step's 15 rows are eight
// trips.  Within a half-wave lane `sub` owns the classes 4 sub .. 4 sub + 3 and (sub = 0) 128, 129 -- one 16-byte load per lane where the
// rows allow it (VEC), four 4-byte loads of the SAME classes otherwise, so that both paths add the same numbers in the same order.
// Lanes sub = 0..4 of the half-wave also take the row's five duration bits.  Nothing diverges around a shuffle: a dead row only guards
// its loads.  The wave's lanes all keep the same running sums (rows in ascending n, bits in ascending order); lane 0 writes them.
template <bool VEC>
__global__ void __launch_bounds__(256) recon_step_scores_kernel(const float* __restrict__ pitch, long ld, const float* __restrict__ dur,
                                                                const long* __restrict__ x, int B, int step_major,
                                                                float* __restrict__ step_scores, int* __restrict__ step_counts) {
  const int lane = threadIdx.x & 63, sub = lane & 31, half = lane >> 5;
  const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= (long)B * 32) return;                                         // (wave-uniform)
  int b, t;
  if (step_major) { b = (int)(q % B); t = (int)(q / B); } else { t = (int)(q % 32); b = (int)(q / 32); }
  const long* xs = x + ((long)b * 32 + t) * 96;                          // the step's 16 rows of 6
  float sp = 0.f, sd = 0.f;
  int pn = 0, ph = 0, dn = 0, dh = 0, nn = 0, nh = 0;
  // the targets of trip k + 1 are fetched while trip k works: the logits' address waits for them
  auto targets = [&](int k, int& p, int& dt) {
    const int n = 2 * k + half;
    const bool row = n < 15;
    const long* xr = xs + (row ? n + 1 : 1) * 6;
    p = row ? (int)xr[0] : SC_NP;
    dt = (row && sub < 5) ? (int)xr[1 + sub] : 2;
  };
  int p_next, dt_next;
  targets(0, p_next, dt_next);
  for (int k = 0; k < 8; k++) {
    const int n = 2 * k + half;
    const int p = p_next, dt = dt_next;
    if (k < 7) targets(k + 1, p_next, dt_next);
    const bool plive = p >= 0 && p < SC_NP;                              // (a pitch outside 0..130 is skipped like <pad>: it indexes nothing)
    const bool dlive = dt == 0 || dt == 1;
    if (!__any(plive || dlive)) continue;                                // (wave-uniform: both rows of the trip are dead)
    const long i = step_major ? ((long)n * 32 + t) * B + b : ((long)b * 32 + t) * 15 + n;
    // ---- pitch: max, first arg-max, sum of exponentials over the 130 classes
    float v[6];
#pragma unroll
    for (int j = 0; j < 6; j++) v[j] = -INFINITY;
    float lt = 0.f;
    if (plive) {
      const float* lr = pitch + i * ld;
      if (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(lr + 4 * sub);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        if (sub == 0) { const float4 c = *reinterpret_cast<const float4*>(lr + 128); v[4] = c.x; v[5] = c.y; }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = lr[4 * sub + j];
        if (sub == 0) { v[4] = lr[128]; v[5] = lr[129]; }
      }
      if (sub == 0) lt = lr[p];
    }
    float m = -INFINITY; int am = 4 * sub;                               // (a lane of -inf names its first class)
#pragma unroll
    for (int j = 0; j < 6; j++) { const int c = j < 4 ? 4 * sub + j : 124 + j; if (v[j] > m) { m = v[j]; am = c; } }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {                                   // the larger value; of equal values the lower class
      const float m2 = __shfl_xor(m, o, 64); const int a2 = __shfl_xor(am, o, 64);
      if (m2 > m || (m2 == m && a2 < am)) { m = m2; am = a2; }
    }
    float s = (expf(v[0] - m) + expf(v[1] - m)) + (expf(v[2] - m) + expf(v[3] - m));
    if (sub == 0) s += expf(v[4] - m) + expf(v[5] - m);
    s = half_sum(s);
    const float nllp = plive ? -(lt - m - logf(s)) : 0.f;
    const int hitp = plive && am == p;
    // ---- duration bit `sub` of the row: two classes, a tie is class 0
    float nlld = 0.f; int hitd = 0;
    if (dlive) {
      const float* dr = dur + i * 10 + 2 * sub;
      const float l0 = dr[0], l1 = dr[1];
      const float dm = fmaxf(l0, l1);
      const float ds = expf(l0 - dm) + expf(l1 - dm);
      nlld = -((dt ? l1 : l0) - dm - logf(ds));
      hitd = (l1 > l0 ? 1 : 0) == dt;
    }
    // ---- the running sums: row 2k, then row 2k + 1 (every lane adds the same values)
    const unsigned long long dvm = __ballot(dlive), dhm = __ballot(hitd);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const float np_ = __shfl(nllp, 32 * h, 64);
      const int pl_ = __shfl((int)plive, 32 * h, 64), hp_ = __shfl(hitp, 32 * h, 64), p_ = __shfl(p, 32 * h, 64);
      if (pl_) sp += np_;
      const int vm = (int)((dvm >> (32 * h)) & 31), hm = (int)((dhm >> (32 * h)) & 31);
#pragma unroll
      for (int d = 0; d < 5; d++) { const float nd_ = __shfl(nlld, 32 * h + d, 64); if ((vm >> d) & 1) sd += nd_; }
      pn += pl_; ph += hp_;
      dn += __popc(vm); dh += __popc(hm);
      const int note = pl_ && p_ < 128;
      nn += note; nh += note && hp_ && hm == 31;
    }
  }
  if (lane == 0) {
    float* so = step_scores + ((long)b * 32 + t) * 2;
    int* co = step_counts + ((long)b * 32 + t) * 6;
    so[0] = sp; so[1] = sd;
    co[0] = pn; co[1] = ph; co[2] = dn; co[3] = dh; co[4] = nn; co[5] = nh;
  }
}

static inline bool score_vec_ok(const float* p, long ld) {
  return (ld & 3) == 0 && ld >= ((SC_NP + 3) & ~3) && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// thread (b, column): column 0, 1 = the float sums, 2..7 = the counts; t = 0..31 in ascending order
__global__ void score_fold_kernel(const float* __restrict__ step_scores, const int* __restrict__ step_counts, int B,
                                  float* __restrict__ scores, int* __restrict__ counts) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * 8) return;
  const long b = i >> 3; const int col = (int)(i & 7);
  if (col < 2) {
    float s = 0.f;
    for (int t = 0; t < 32; t++) s += step_scores[(b * 32 + t) * 2 + col];
    scores[b * 2 + col] = s;
  } else {
    int s = 0;
    for (int t = 0; t < 32; t++) s += step_counts[(b * 32 + t) * 6 + (col - 2)];
    counts[b * 6 + (col - 2)] = s;
  }
}

// one wave per row: lane l adds the columns l, l + 64, ... in ascending order, then the xor tree -- the order depends on Z only
__global__ void kl_rows_kernel(const float* __restrict__ mu, const float* __restrict__ sd, int B, int Z, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  float s = 0.f;
  for (int z = lane; z < Z; z += 64) {
    const float m = mu[b * Z + z], d = sd[b * Z + z];
    s += -logf(d) + (d * d + m * m) * 0.5f - 0.5f;
  }
  s = wave_sum(s);
  if (lane == 0) out[b] = s;
}

__device__ __forceinline__ float ce12(const float* __restrict__ l, int t, int* hit) {
  float m = l[0]; int am = 0;
  for (int k = 1; k < 12; k++) if (l[k] > m) { m = l[k]; am = k; }
  float s = 0.f;
  for (int k = 0; k < 12; k++) s += expf(l[k] - m);
  *hit = am == t;
  return -(l[t] - m - logf(s));
}

// one thread per sample: its 8 chord steps in ascending order, the 12 chroma bits of a step in ascending order
__global__ void chord_step_scores_kernel(const float* __restrict__ root, const float* __restrict__ chroma, const float* __restrict__ bass,
                                         const float* __restrict__ c, int B, int step_major, float* __restrict__ scores,
                                         int* __restrict__ counts) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float sr = 0.f, sc = 0.f, sb = 0.f;
  int hr = 0, hc = 0, hb = 0;
  for (int t = 0; t < 8; t++) {
    const long i = step_major ? (long)t * B + b : b * 8 + t;
    const float* cr = c + (b * 8 + t) * 36;
    int ar = 0, ab = 0; float mr = cr[0], mb = cr[24];                   // (chord_targets_kernel's rule: the first maximum)
    for (int k = 1; k < 12; k++) { if (cr[k] > mr) { mr = cr[k]; ar = k; } if (cr[24 + k] > mb) { mb = cr[24 + k]; ab = k; } }
    int h;
    sr += ce12(root + i * 12, ar, &h); hr += h;
    for (int k = 0; k < 12; k++) {
      const int ct = (int)cr[12 + k];
      if (ct != 0 && ct != 1) continue;                                  // (not a class: it indexes nothing)
      const float l0 = chroma[(i * 12 + k) * 2], l1 = chroma[(i * 12 + k) * 2 + 1];
      const float m = fmaxf(l0, l1);
      sc += -((ct ? l1 : l0) - m - logf(expf(l0 - m) + expf(l1 - m)));
      hc += (l1 > l0 ? 1 : 0) == ct;
    }
    sb += ce12(bass + i * 12, ab, &h); hb += h;
  }
  scores[b * 3 + 0] = sr; scores[b * 3 + 1] = sc; scores[b * 3 + 2] = sb;
  counts[b * 3 + 0] = hr; counts[b * 3 + 1] = hc; counts[b * 3 + 2] = hb;
}

// one workgroup per sample: 4096 cells, 16 per thread
__global__ void __launch_bounds__(256) roll_match_kernel(const float* __restrict__ est, const float* __restrict__ ref, int* __restrict__ counts) {
  __shared__ int red[4][4];
  const long base = (long)blockIdx.x * 4096;
  int ne = 0, nr = 0, on = 0, ex = 0;
  for (int i = threadIdx.x; i < 4096; i += 256) {
    const float e = est[base + i], r = ref[base + i];
    const bool be = e > 0.f, br = r > 0.f;
    ne += be; nr += br; on += be && br; ex += be && br && e == r;
  }
  for (int o = 32; o > 0; o >>= 1) { ne += __shfl_xor(ne, o, 64); nr += __shfl_xor(nr, o, 64); on += __shfl_xor(on, o, 64); ex += __shfl_xor(ex, o, 64); }
  if ((threadIdx.x & 63) == 0) { int* r = red[threadIdx.x >> 6]; r[0] = ne; r[1] = nr; r[2] = on; r[3] = ex; }
  __syncthreads();
  if (threadIdx.x < 4) counts[(long)blockIdx.x * 4 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

}  // namespace ptv

using namespace ptv;

extern "C" int ptv_recon_step_scores(const float* pitch, long ld_pitch, const float* dur, const long* x, int B, int step_major,
                                     float* step_scores, int* step_counts, void* stream) {
  if (!pitch || !dur || !x || !step_scores || !step_counts || B <= 0 || ld_pitch < SC_NP) return PTV_ERR_ARG;
  const dim3 grid(cdiv((long)B * 32, 4)), block(256);
  if (score_vec_ok(pitch, ld_pitch)) hipLaunchKernelGGL((recon_step_scores_kernel<true>), grid, block, 0, (hipStream_t)stream, pitch, ld_pitch, dur, x, B, step_major, step_scores, step_counts);
  else hipLaunchKernelGGL((recon_step_scores_kernel<false>), grid, block, 0, (hipStream_t)stream, pitch, ld_pitch, dur, x, B, step_major, step_scores, step_counts);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_score_fold(const float* step_scores, const int* step_counts, int B, float* scores, int* counts, void* stream) {
  if (!step_scores || !step_counts || !scores || !counts || B <= 0) return PTV_ERR_ARG;
  hipLaunchKernelGGL(score_fold_kernel, dim3(cdiv((long)B * 8, 256)), dim3(256), 0, (hipStream_t)stream, step_scores, step_counts, B, scores, counts);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_kl_rows(const float* mu, const float* sd, int B, int Z, float* out, void* stream) {
  if (!mu || !sd || !out || B <= 0 || Z <= 0) return PTV_ERR_ARG;
  hipLaunchKernelGGL(kl_rows_kernel, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, mu, sd, B, Z, out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_chord_step_scores(const float* root, const float* chroma, const float* bass, const float* c, int B, int step_major,
                                     float* scores, int* counts, void* stream) {
  if (!root || !chroma || !bass || !c || !scores || !counts || B <= 0) return PTV_ERR_ARG;
  hipLaunchKernelGGL(chord_step_scores_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, root, chroma, bass, c, B, step_major, scores, counts);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_roll_match(const float* est_pr, const float* ref_pr, int B, int* counts, void* stream) {
  if (!est_pr || !ref_pr || !counts || B <= 0) return PTV_ERR_ARG;
  hipLaunchKernelGGL(roll_match_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, est_pr, ref_pr, counts);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
