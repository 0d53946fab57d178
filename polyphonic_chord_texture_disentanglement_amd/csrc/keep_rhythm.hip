// keep_rhythm.hip -- kept rhythm of a free-running decode (include/ptvae_hip.h "Kept rhythm"; INTEGRATION.md "Kept rhythm"):
// the force arrays that keep a time step's note count, its rest and its durations while the pitches are drawn again -- K decisions that
// are free but may not be <eos> (PTV_FORCE_NOT_EOS), then a forced <eos>.  The shape of keep_voice.hip's builder: no atomics, no LDS, no
// workspace, every output element has one writer.
#include "common.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

// ---- the rule, stated once ------------------------------------------------------------------------------------------------------------
// the whole-step rule of "Kept steps": first slot 1..15 holding <eos>, else 15; has_eos: whether one was found
__device__ __forceinline__ int rhythm_step_len(const long* __restrict__ xs, bool& has_eos) {
  int L = 15;
  has_eos = false;
  for (int s = 15; s >= 1; s--) if (xs[s * 6] == 129) { L = s; has_eos = true; }
  return L;
}
// (b, t) -> the mode byte as it acts (0 for a value that is none of 0 / 1 / 3, with bit 1 of e); L: the decisions n < L of a whole step are
// forced to the slot's pitch where that lies in 0..129; K: the note decisions of a rhythm step (the forced <eos> follows at n = K < 15)
__device__ __forceinline__ int rhythm_select(const long* __restrict__ xs, const unsigned char* __restrict__ mode, int mode_one, long b, long t,
                                             int& L, int& K, int& e) {
  const int m = mode[(mode_one ? 0 : b * 32) + t];
  L = 0; K = 0;
  if (m == 1 || m == 3) {
    bool has_eos;
    L = rhythm_step_len(xs, has_eos);
    K = has_eos ? L - 1 : 15;
    return m;
  }
  if (m != 0) e |= 2;
  return 0;
}
// err[b], by its one writer: the bits of the sample's 32 steps (the pitch columns again: L2 hits)
__device__ __forceinline__ int rhythm_sample_err(const long* __restrict__ x, const unsigned char* __restrict__ mode, int mode_one, long b) {
  int e = 0;
  for (int t = 0; t < 32; t++) {
    const long* xt = x + (b * 32 + t) * 96;
    int L, K;
    const int m = rhythm_select(xt, mode, mode_one, b, t, L, K, e);
    if (m == 1)
      for (int n = 0; n < L; n++) { const long p = xt[(n + 1) * 6]; if (p < 0 || p > 129) e |= 1; }
    if (m == 3)
      for (int n = 0; n < K; n++) { const long p = xt[(n + 1) * 6]; if (p < 0 || p > 127) e |= 1; }
  }
  return e;
}

// ---- the builder: one thread per (time step, sample) row r = t * B + b of the step-major arrays -- a wave's stores are 64 consecutive
// words of every one of the 15 + 75 planes, while it reads its own 768 contiguous bytes of the sample-major grid
__global__ void keep_rhythm_force_build_kernel(const long* __restrict__ x, const unsigned char* __restrict__ mode, int mode_one, int flags,
                                               long B, int* __restrict__ force_pitch, int* __restrict__ force_dur, int* __restrict__ kept_n,
                                               int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long R = 32 * B, M = 15 * R;
  if (r >= R) return;
  const long t = r / B, b = r % B;
  const long* xs = x + (b * 32 + t) * 96;
  int L, K, e = 0;
  const int m = rhythm_select(xs, mode, mode_one, b, t, L, K, e);
  const int nd = m == 1 ? L : (m == 3 && !(flags & 1) ? K : 0);          // the decisions whose duration words are x's bits
  int cnt = 0;
  for (int n = 0; n < 15; n++) {
    const long p = xs[(n + 1) * 6];
    int w = -1;
    if (m == 1) {
      const bool fp = n < L && p >= 0 && p <= 129;
      w = fp ? (int)p : -1;
      cnt += fp ? 1 : 0;
    } else if (m == 3) {
      w = n < K ? PTV_FORCE_NOT_EOS : (n == K ? 129 : -1);
    }
    force_pitch[n * R + r] = w;
#pragma unroll
    for (int d = 0; d < 5; d++) {
      const long q = xs[(n + 1) * 6 + 1 + d];
      force_dur[d * M + n * R + r] = (n < nd && (q == 0 || q == 1)) ? (int)q : -1;
    }
  }
  kept_n[b * 32 + t] = m == 3 ? K : cnt;
  if (t == 0) err[b] = rhythm_sample_err(x, mode, mode_one, b);
}

}  // namespace ptv
using namespace ptv;

extern "C" int ptv_keep_rhythm_force_build(const long* x, const unsigned char* mode, int mode_rows, int flags, long B, int* force_pitch,
                                           int* force_dur, int* kept_n, int* err, void* stream) {
  if (!x || !mode || !force_pitch || !force_dur || !kept_n || !err || B < 1 || flags < 0 || flags > 1 || (mode_rows != 1 && mode_rows != B))
    return PTV_ERR_ARG;
  const long R = 32 * B;
  hipLaunchKernelGGL(keep_rhythm_force_build_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, mode,
                     (mode_rows == 1 && B != 1) ? 1 : 0, flags, B, force_pitch, force_dur, kept_n, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
