// dur_limits.hip -- duration limits of a free-running decode (include/ptvae_hip.h "Duration limits"; INTEGRATION.md "Duration limits",
// DESIGN.md 7j): the force arrays whose duration words are PTV_FORCE_DUR_RANGE(lo, hi) -- the decision stays free, the note's duration
// ends in the range -- alone or built INTO the arrays of an existing keep, and the test aid of the rule itself (dur_range_allowed /
// dur_range_bit, philox.hpp: the only statement of it).  The shape of keep_rhythm.hip's builder: no atomics, no LDS, no workspace, every
// output element has one writer.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/ptvae_hip.h"
#include "../../include/ptvae_hip_debug.h"

namespace ptv {

// ---- the builder: one thread per (time step, sample) row r = t * B + b of the step-major arrays -- a wave's accesses are 64 consecutive
// words of every one of the 15 + 75 planes
__global__ void dur_range_force_build_kernel(const unsigned char* __restrict__ lo, int lo_one, const unsigned char* __restrict__ hi, int hi_one,
                                             const unsigned char* __restrict__ steps, int steps_one, const int* __restrict__ src_pitch,
                                             const int* __restrict__ src_dur, long B, int* __restrict__ force_pitch,
                                             int* __restrict__ force_dur, int* __restrict__ yielded) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long R = 32 * B, M = 15 * R;
  if (r >= R) return;
  const long t = r / B, b = r % B;
  const bool sel = steps[(steps_one ? 0 : b * 32) + t] != 0;
  const int h = min(max((int)hi[(hi_one ? 0 : b * 32) + t], 1), 32);      // the ceiling, clamped into 1..32 ...
  const int f = max((int)lo[(lo_one ? 0 : b * 32) + t], 1);               // ... wins over the floor
  const int l = min(f, h);
  const int word = PTV_FORCE_DUR_RANGE(l - 1, h - 1);
  for (int n = 0; n < 15; n++) {
    force_pitch[n * R + r] = src_pitch ? src_pitch[n * R + r] : -1;
    int w[5];
    bool free5 = true;
#pragma unroll
    for (int d = 0; d < 5; d++) {
      w[d] = src_dur ? src_dur[d * M + n * R + r] : -1;
      free5 = free5 && w[d] < 0;
    }
#pragma unroll
    for (int d = 0; d < 5; d++) force_dur[d * M + n * R + r] = (sel && free5) ? word : w[d];
  }
  yielded[b * 32 + t] = (sel && f > h) ? 1 : 0;
}

// test aid: the rule on caller-supplied triples
__global__ void dur_range_debug_kernel(const int* __restrict__ words, const int* __restrict__ d, const int* __restrict__ prefix, long rows,
                                       unsigned char* __restrict__ out) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int dd = d[r], p = prefix[r], w = words[r];
  unsigned v = 0xffu;
  if (dd >= 0 && dd < 5 && p >= 0 && p < (1 << dd))
    v = dur_range_allowed(w, dd, p) | ((unsigned)dur_range_bit(w, dd, p, 0) << 2) | ((unsigned)dur_range_bit(w, dd, p, 1) << 3);
  out[r] = (unsigned char)v;
}

}  // namespace ptv
using namespace ptv;

extern "C" int ptv_dur_range_force_build(const unsigned char* lo, int lo_rows, const unsigned char* hi, int hi_rows, const unsigned char* steps,
                                         int steps_rows, const int* src_pitch, const int* src_dur, long B, int* force_pitch, int* force_dur,
                                         int* yielded, void* stream) {
  if (!lo || !hi || !steps || !force_pitch || !force_dur || !yielded || B < 1) return PTV_ERR_ARG;
  if ((lo_rows != 1 && lo_rows != B) || (hi_rows != 1 && hi_rows != B) || (steps_rows != 1 && steps_rows != B)) return PTV_ERR_ARG;
  if ((src_pitch == nullptr) != (src_dur == nullptr) || src_pitch == force_pitch || src_dur == force_dur) return PTV_ERR_ARG;
  const long R = 32 * B;
  hipLaunchKernelGGL(dur_range_force_build_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lo,
                     (lo_rows == 1 && B != 1) ? 1 : 0, hi, (hi_rows == 1 && B != 1) ? 1 : 0, steps, (steps_rows == 1 && B != 1) ? 1 : 0, src_pitch,
                     src_dur, B, force_pitch, force_dur, yielded);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_debug_dur_range(const int* words, const int* d, const int* prefix, long rows, unsigned char* out, void* stream) {
  if (!words || !d || !prefix || !out || rows <= 0) return PTV_ERR_ARG;
  hipLaunchKernelGGL(dur_range_debug_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, words, d, prefix, rows, out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
