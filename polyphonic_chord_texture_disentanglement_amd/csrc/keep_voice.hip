// keep_voice.hip -- kept voices of a free-running decode (include/ptvae_hip.h "Kept voices"; INTEGRATION.md "Kept voices"):
// the force arrays that keep the lowest notes of a time step -- a prefix of its note decisions, since the grammar orders a step by
// ascending pitch -- and the same selection as two model grids.  No atomics, no LDS, no workspace: every output element has one writer.
#include <initializer_list>
#include "common.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

// the selection of one call: mode / below / lowest with "one row serves every sample" resolved once on the host
struct VoiceSel {
  const unsigned char* mode;
  const int* below;
  const int* lowest;
  int mode_one, below_one, lowest_one;
};

// ---- the rule, stated once for both kernels -----------------------------------------------------------------------------------------
// mode 2: K, the length of the kept prefix.  Slots s = 1..15 in order: stop at K == lowest, at <eos>, at a pitch outside 0..127 (bit 0 of
// e) and at the first pitch >= below; every slot before the stop is a kept note, so K = s - 1 at the stop.
__device__ __forceinline__ int voice_prefix_len(const long* __restrict__ xs, int below, int lowest, int& e) {
  int K = 0;
  for (int s = 1; s <= 15; s++) {
    if (K == lowest) break;
    const long p = xs[s * 6];
    if (p == 129) break;
    if (p < 0 || p > 127) { e |= 1; break; }
    if (p >= below) break;
    K++;
  }
  return K;
}
// mode 1 (the whole-step rule of "Kept steps", restated): first slot 1..15 holding <eos>, else 15
__device__ __forceinline__ int whole_step_len(const long* __restrict__ xs) {
  int L = 15;
  for (int s = 15; s >= 1; s--) if (xs[s * 6] == 129) L = s;
  return L;
}
// (b, t) -> the mode byte as it acts (0 for a value that is none of 0 / 1 / 2, with bit 1 of e) and L: the note decisions n < L of the step
// are the kept ones -- forced to the slot's pitch where that lies in 0..129 (under mode 2 every one of them does: 0..127)
__device__ __forceinline__ int step_select(const long* __restrict__ xs, const VoiceSel& v, long b, long t, int& L, int& e) {
  const int m = v.mode[(v.mode_one ? 0 : b * 32) + t];
  L = 0;
  if (m == 1) { L = whole_step_len(xs); return 1; }
  if (m == 2) {
    int below = v.below ? v.below[(v.below_one ? 0 : b * 32) + t] : 128;
    int lowest = v.lowest ? v.lowest[(v.lowest_one ? 0 : b * 32) + t] : 15;
    below = below < 0 ? 0 : (below > 128 ? 128 : below);
    lowest = lowest < 0 ? 0 : (lowest > 15 ? 15 : lowest);
    L = voice_prefix_len(xs, below, lowest, e);
    return 2;
  }
  if (m != 0) e |= 2;
  return 0;
}
// err[b], by its one writer: the bits of the sample's 32 steps (the pitch columns again: L2 hits)
__device__ __forceinline__ int sample_err(const long* __restrict__ x, const VoiceSel& v, long b) {
  int e = 0;
  for (int t = 0; t < 32; t++) {
    const long* xt = x + (b * 32 + t) * 96;
    int L;
    if (step_select(xt, v, b, t, L, e) == 1)
      for (int n = 0; n < L; n++) { const long p = xt[(n + 1) * 6]; if (p < 0 || p > 129) e |= 1; }
  }
  return e;
}

// ---- the builder: one thread per (time step, sample) row r = t * B + b of the step-major arrays -- a wave's stores are 64 consecutive
// words of every one of the 15 + 75 planes, while it reads its own 768 contiguous bytes of the sample-major grid
__global__ void keep_voice_force_build_kernel(const long* __restrict__ x, VoiceSel v, int flags, long B, int* __restrict__ force_pitch,
                                              int* __restrict__ force_dur, int* __restrict__ kept_n, int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long R = 32 * B, M = 15 * R;
  if (r >= R) return;
  const long t = r / B, b = r % B;
  const long* xs = x + (b * 32 + t) * 96;
  int L, e = 0;
  const int m = step_select(xs, v, b, t, L, e);
  const bool durs = !(m == 2 && (flags & 1));
  int cnt = 0;
  for (int n = 0; n < 15; n++) {
    const long p = xs[(n + 1) * 6];
    const bool fp = n < L && p >= 0 && p <= 129;
    force_pitch[n * R + r] = fp ? (int)p : -1;
    cnt += fp ? 1 : 0;
#pragma unroll
    for (int d = 0; d < 5; d++) {
      const long w = xs[(n + 1) * 6 + 1 + d];
      force_dur[d * M + n * R + r] = (n < L && durs && (w == 0 || w == 1)) ? (int)w : -1;
    }
  }
  kept_n[b * 32 + t] = cnt;
  if (t == 0) err[b] = sample_err(x, v, b);
}

// ---- the split: one thread per (sample, step), which writes its own 768 bytes of both grids
__device__ __forceinline__ void put_slot(long* __restrict__ dst, int j, const long* __restrict__ src) {
#pragma unroll
  for (int k = 0; k < 6; k++) dst[j * 6 + k] = src[k];
}
__device__ __forceinline__ void put_token(long* __restrict__ dst, int j, long pitch) {       // <eos> / <pad>: duration bits 2
  dst[j * 6] = pitch;
#pragma unroll
  for (int k = 1; k < 6; k++) dst[j * 6 + k] = 2;
}
__device__ __forceinline__ void put_empty_step(long* __restrict__ dst) {                      // slots 1..15 of the empty step
  put_token(dst, 1, 129);
  for (int j = 2; j <= 15; j++) put_token(dst, j, 130);
}
__global__ void grid_split_voice_kernel(const long* __restrict__ x, VoiceSel v, long B, long* __restrict__ voice, long* __restrict__ rest,
                                        int* __restrict__ kept_n, int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= 32 * B) return;
  const long b = r >> 5, t = r & 31;
  const long* xs = x + r * 96;
  long* vo = voice + r * 96;
  long* re = rest + r * 96;
  int L, e = 0;
  const int m = step_select(xs, v, b, t, L, e);
  put_slot(vo, 0, xs);
  put_slot(re, 0, xs);
  int cnt = 0;
  if (m == 2) {
    for (int s = 1; s <= L; s++) put_slot(vo, s, xs + s * 6);
    if (L < 15) put_token(vo, L + 1, 129);
    for (int j = L + 2; j <= 15; j++) put_token(vo, j, 130);
    int j = 1;
    bool ended = false;
    for (int s = L + 1; s <= 15 && !ended; s++) {
      put_slot(re, j++, xs + s * 6);
      ended = xs[s * 6] == 129;
    }
    if (!ended && j <= 15) put_token(re, j++, 129);
    for (; j <= 15; j++) put_token(re, j, 130);
    cnt = L;
  } else {
    long* whole = m == 1 ? vo : re;
    for (int s = 1; s <= 15; s++) put_slot(whole, s, xs + s * 6);
    put_empty_step(m == 1 ? re : vo);
    for (int n = 0; n < L; n++) { const long p = xs[(n + 1) * 6]; cnt += (p >= 0 && p <= 129) ? 1 : 0; }     // (L = 0 unless m == 1)
  }
  kept_n[r] = cnt;
  if (t == 0) err[b] = sample_err(x, v, b);
}

static bool voice_sel(VoiceSel& v, const unsigned char* mode, int mode_rows, const int* below, int below_rows, const int* lowest,
                      int lowest_rows, long B) {
  for (int rows : {mode_rows, below_rows, lowest_rows})
    if (rows != 1 && rows != B) return false;
  v.mode = mode; v.below = below; v.lowest = lowest;
  v.mode_one = (mode_rows == 1 && B != 1) ? 1 : 0;
  v.below_one = (below_rows == 1 && B != 1) ? 1 : 0;
  v.lowest_one = (lowest_rows == 1 && B != 1) ? 1 : 0;
  return true;
}
}  // namespace ptv
using namespace ptv;

extern "C" int ptv_keep_voice_force_build(const long* x, const unsigned char* mode, int mode_rows, const int* below, int below_rows,
                                          const int* lowest, int lowest_rows, int flags, long B, int* force_pitch, int* force_dur,
                                          int* kept_n, int* err, void* stream) {
  VoiceSel v;
  if (!x || !mode || !force_pitch || !force_dur || !kept_n || !err || B < 1 || flags < 0 || flags > 1 ||
      !voice_sel(v, mode, mode_rows, below, below_rows, lowest, lowest_rows, B))
    return PTV_ERR_ARG;
  const long R = 32 * B;
  hipLaunchKernelGGL(keep_voice_force_build_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, v, flags, B,
                     force_pitch, force_dur, kept_n, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_grid_split_voice(const long* x, const unsigned char* mode, int mode_rows, const int* below, int below_rows,
                                    const int* lowest, int lowest_rows, long B, long* voice, long* rest, int* kept_n, int* err,
                                    void* stream) {
  VoiceSel v;
  if (!x || !mode || !voice || !rest || !kept_n || !err || B < 1 || !voice_sel(v, mode, mode_rows, below, below_rows, lowest, lowest_rows, B))
    return PTV_ERR_ARG;
  const long R = 32 * B;
  hipLaunchKernelGGL(grid_split_voice_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, v, B, voice, rest,
                     kept_n, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
