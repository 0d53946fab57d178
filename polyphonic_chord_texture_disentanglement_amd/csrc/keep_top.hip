// keep_top.hip -- kept top voice of a free-running decode (include/ptvae_hip.h "Kept top voice"; INTEGRATION.md "Kept top voice"):
// the force arrays that keep the HIGHEST notes of a time step -- a suffix of its note decisions -- while the notes under them are drawn
// again: J decisions that are free, never <eos> and under a ceiling that leaves room for what follows (PTV_FORCE_BELOW), then the kept
// pitches and a forced <eos>; and the same selection as two model grids.  The shape of keep_voice.hip: no atomics, no LDS, no workspace,
// every output element has one writer.
#include <initializer_list>
#include "common.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

// the selection of one call: mode / above / highest with "one row serves every sample" resolved once on the host
struct TopSel {
  const unsigned char* mode;
  const int* above;
  const int* highest;
  int mode_one, above_one, highest_one;
};

// ---- the rule, stated once for both kernels -----------------------------------------------------------------------------------------
// the whole-step rule of "Kept steps": first slot 1..15 holding <eos>, else 15; has_eos: whether one was found
__device__ __forceinline__ int top_step_len(const long* __restrict__ xs, bool& has_eos) {
  int L = 15;
  has_eos = false;
  for (int s = 15; s >= 1; s--) if (xs[s * 6] == 129) { L = s; has_eos = true; }
  return L;
}
// mode 4: h, the length of the kept suffix of the K notes in slots 1..K.  Slots s = K..1 in order: stop at h == highest, at a pitch outside
// 0..127 and at the first pitch < above; every slot before the stop is a kept note.
__device__ __forceinline__ int top_suffix_len(const long* __restrict__ xs, int K, int above, int highest) {
  int h = 0;
  for (int s = K; s >= 1; s--) {
    if (h == highest) break;
    const long p = xs[s * 6];
    if (p < 0 || p > 127) break;
    if (p < above) break;
    h++;
  }
  return h;
}
// bit 0 of err at a top step: a slot 1..K whose pitch is no note, or one that does not lie above the slot before it
__device__ __forceinline__ int top_step_err(const long* __restrict__ xs, int K) {
  int e = 0;
  for (int s = 1; s <= K; s++) {
    const long p = xs[s * 6];
    if (p < 0 || p > 127) e |= 1;
    if (s >= 2 && p <= xs[(s - 1) * 6]) e |= 1;
  }
  return e;
}
// (b, t) -> the mode byte as it acts (0 for a value that is none of 0 / 1 / 4, with bit 1 of e).  L: the decisions n < L of a whole step are
// forced to the slot's pitch where that lies in 0..129; K, h: the notes of a top step and how many of them, the last ones, are kept
__device__ __forceinline__ int top_select(const long* __restrict__ xs, const TopSel& v, long b, long t, int& L, int& K, int& h, int& e) {
  const int m = v.mode[(v.mode_one ? 0 : b * 32) + t];
  L = 0; K = 0; h = 0;
  if (m == 1 || m == 4) {
    bool has_eos;
    L = top_step_len(xs, has_eos);
    if (m == 1) return 1;
    K = has_eos ? L - 1 : 15;
    int above = v.above ? v.above[(v.above_one ? 0 : b * 32) + t] : 0;
    int highest = v.highest ? v.highest[(v.highest_one ? 0 : b * 32) + t] : ((v.above || v.highest) ? 15 : 1);
    above = above < 0 ? 0 : (above > 128 ? 128 : above);
    highest = highest < 0 ? 0 : (highest > 15 ? 15 : highest);
    h = top_suffix_len(xs, K, above, highest);
    e |= top_step_err(xs, K);
    return 4;
  }
  if (m != 0) e |= 2;
  return 0;
}
// the ceiling of the free decision n < J = K - h of a top step, clamped into 1..128.  Lanes: the pitch of x's next note, so every re-drawn
// voice stays under its old upper neighbour; room (flags bit 1): the lowest kept pitch (128 without one) less one semitone per decision
// still to come before it.  Either leaves a note for every later decision whatever is drawn here, if the step ascends strictly.
__device__ __forceinline__ int top_ceiling(const long* __restrict__ xs, int n, int J, int K, int room) {
  long u;
  if (room) u = (J < K ? xs[(J + 1) * 6] : 128) - (J - 1 - n);
  else u = n + 1 < K ? xs[(n + 2) * 6] : 128;
  return u < 1 ? 1 : (u > 128 ? 128 : (int)u);
}
// err[b], by its one writer: the bits of the sample's 32 steps (the pitch columns again: L2 hits)
__device__ __forceinline__ int top_sample_err(const long* __restrict__ x, const TopSel& v, long b) {
  int e = 0;
  for (int t = 0; t < 32; t++) {
    const long* xt = x + (b * 32 + t) * 96;
    int L, K, h;
    if (top_select(xt, v, b, t, L, K, h, e) == 1)
      for (int n = 0; n < L; n++) { const long p = xt[(n + 1) * 6]; if (p < 0 || p > 129) e |= 1; }
  }
  return e;
}

// ---- the builder: one thread per (time step, sample) row r = t * B + b of the step-major arrays -- a wave's stores are 64 consecutive
// words of every one of the 15 + 75 planes, while it reads its own 768 contiguous bytes of the sample-major grid
__global__ void keep_top_force_build_kernel(const long* __restrict__ x, TopSel v, int flags, long B, int* __restrict__ force_pitch,
                                            int* __restrict__ force_dur, int* __restrict__ kept_n, int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long R = 32 * B, M = 15 * R;
  if (r >= R) return;
  const long t = r / B, b = r % B;
  const long* xs = x + (b * 32 + t) * 96;
  int L, K, h, e = 0;
  const int m = top_select(xs, v, b, t, L, K, h, e);
  const int J = K - h;
  // the decisions d0 <= n < d1 whose duration words are x's bits
  const int d0 = (m == 4 && (flags & 1)) ? J : 0, d1 = m == 1 ? L : (m == 4 ? K : 0);
  int cnt = 0;
  for (int n = 0; n < 15; n++) {
    const long p = xs[(n + 1) * 6];
    int w = -1;
    if (m == 1) {
      const bool fp = n < L && p >= 0 && p <= 129;
      w = fp ? (int)p : -1;
      cnt += fp ? 1 : 0;
    } else if (m == 4) {
      if (n < J) w = PTV_FORCE_BELOW(top_ceiling(xs, n, J, K, flags & 2));
      else if (n < K) w = (int)p;                                  // (a kept note: 0..127 by the suffix rule)
      else if (n == K) w = 129;
    }
    force_pitch[n * R + r] = w;
#pragma unroll
    for (int d = 0; d < 5; d++) {
      const long q = xs[(n + 1) * 6 + 1 + d];
      force_dur[d * M + n * R + r] = (n >= d0 && n < d1 && (q == 0 || q == 1)) ? (int)q : -1;
    }
  }
  kept_n[b * 32 + t] = m == 4 ? h : cnt;
  if (t == 0) err[b] = top_sample_err(x, v, b);
}

// ---- the split: one thread per (sample, step), which writes its own 768 bytes of both grids
__device__ __forceinline__ void top_put_slot(long* __restrict__ dst, int j, const long* __restrict__ src) {
#pragma unroll
  for (int k = 0; k < 6; k++) dst[j * 6 + k] = src[k];
}
__device__ __forceinline__ void top_put_token(long* __restrict__ dst, int j, long pitch) {   // <eos> / <pad>: duration bits 2
  dst[j * 6] = pitch;
#pragma unroll
  for (int k = 1; k < 6; k++) dst[j * 6 + k] = 2;
}
// slots 1.. of dst: the cnt slots of src from slot s0 on, an <eos> (if a slot is left for it), <pad>
__device__ __forceinline__ void top_put_notes(long* __restrict__ dst, const long* __restrict__ src, int s0, int cnt) {
  for (int j = 1; j <= cnt; j++) top_put_slot(dst, j, src + (s0 + j - 1) * 6);
  if (cnt < 15) top_put_token(dst, cnt + 1, 129);
  for (int j = cnt + 2; j <= 15; j++) top_put_token(dst, j, 130);
}
__global__ void grid_split_top_kernel(const long* __restrict__ x, TopSel v, long B, long* __restrict__ voice, long* __restrict__ rest,
                                      int* __restrict__ kept_n, int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= 32 * B) return;
  const long b = r >> 5, t = r & 31;
  const long* xs = x + r * 96;
  long* vo = voice + r * 96;
  long* re = rest + r * 96;
  int L, K, h, e = 0;
  const int m = top_select(xs, v, b, t, L, K, h, e);
  top_put_slot(vo, 0, xs);
  top_put_slot(re, 0, xs);
  int cnt = 0;
  if (m == 4) {
    top_put_notes(vo, xs, K - h + 1, h);
    top_put_notes(re, xs, 1, K - h);
    cnt = h;
  } else {
    long* whole = m == 1 ? vo : re;
    for (int s = 1; s <= 15; s++) top_put_slot(whole, s, xs + s * 6);
    top_put_notes(m == 1 ? re : vo, xs, 1, 0);
    for (int n = 0; n < L; n++) { const long p = xs[(n + 1) * 6]; cnt += (p >= 0 && p <= 129) ? 1 : 0; }     // (L = 0 unless m == 1)
  }
  kept_n[r] = cnt;
  if (t == 0) err[b] = top_sample_err(x, v, b);
}

static bool top_sel(TopSel& v, const unsigned char* mode, int mode_rows, const int* above, int above_rows, const int* highest,
                    int highest_rows, long B) {
  for (int rows : {mode_rows, above_rows, highest_rows})
    if (rows != 1 && rows != B) return false;
  v.mode = mode; v.above = above; v.highest = highest;
  v.mode_one = (mode_rows == 1 && B != 1) ? 1 : 0;
  v.above_one = (above_rows == 1 && B != 1) ? 1 : 0;
  v.highest_one = (highest_rows == 1 && B != 1) ? 1 : 0;
  return true;
}
}  // namespace ptv
using namespace ptv;

extern "C" int ptv_keep_top_force_build(const long* x, const unsigned char* mode, int mode_rows, const int* above, int above_rows,
                                        const int* highest, int highest_rows, int flags, long B, int* force_pitch, int* force_dur,
                                        int* kept_n, int* err, void* stream) {
  TopSel v;
  if (!x || !mode || !force_pitch || !force_dur || !kept_n || !err || B < 1 || flags < 0 || flags > 3 ||
      !top_sel(v, mode, mode_rows, above, above_rows, highest, highest_rows, B))
    return PTV_ERR_ARG;
  const long R = 32 * B;
  hipLaunchKernelGGL(keep_top_force_build_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, v, flags, B,
                     force_pitch, force_dur, kept_n, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_grid_split_top(const long* x, const unsigned char* mode, int mode_rows, const int* above, int above_rows,
                                  const int* highest, int highest_rows, long B, long* voice, long* rest, int* kept_n, int* err,
                                  void* stream) {
  TopSel v;
  if (!x || !mode || !voice || !rest || !kept_n || !err || B < 1 || !top_sel(v, mode, mode_rows, above, above_rows, highest, highest_rows, B))
    return PTV_ERR_ARG;
  const long R = 32 * B;
  hipLaunchKernelGGL(grid_split_top_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, v, B, voice, rest,
                     kept_n, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
