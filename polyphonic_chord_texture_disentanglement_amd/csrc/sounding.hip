// sounding.hip -- the sounding state of a free-running decode (include/ptvae_hip.h "Sounding state"; INTEGRATION.md under the same name,
// DESIGN.md 7m): the first constraint with memory.  Between two launches of the note loop one small kernel reads the time step the decode
// has just decided, advances rem[b][p] -- how many steps pitch p of row b still sounds -- and writes the NEXT step's mask row and pitch
// force words from the caller's base tables and what is held: no re-struck held pitch, at most K / at least F sounding pitches.
// It sits on the decode's latency chain once per time step, so it is shaped for latency: one wave per row, lane l owns pitches l and
// l + 64 -- the two ballots of "rem > 0" ARE the four mask words, their popcounts the held count.  Lanes 0..14 each load one slot of the
// decided step (one memory round trip for all 15), the slots are then applied in order through wave shuffles ("the later slot wins"), and
// lanes 0..14 each own one force word of the step.  No LDS, no barrier, no atomics, no workspace: every output element has one writer.
#include "common.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

// a per-(sample, time step) operand [rows][32], rows 1 or B (the convention of keep.hip's PerStep)
template <typename T>
struct SndPerStep {
  const T* p;
  int one;
  __device__ __forceinline__ T at(long b, long t) const { return p[(one ? 0 : b * 32) + t]; }
};
template <typename T>
static bool snd_per_step(SndPerStep<T>& o, const T* p, int rows, long B) {
  if (rows != 1 && rows != B) return false;
  o.p = p;
  o.one = (rows == 1 && B != 1) ? 1 : 0;
  return true;
}

constexpr int SND_ROWS_PER_WG = 4;      // one wave per row

__global__ __launch_bounds__(64 * SND_ROWS_PER_WG) void sounding_step_kernel(
    const long* __restrict__ xhat, int t_done, long B, SndPerStep<int> mask_base, const int* __restrict__ force_base,
    SndPerStep<unsigned char> kmax, SndPerStep<unsigned char> fmin, SndPerStep<unsigned char> steps, const unsigned* __restrict__ control,
    unsigned char* __restrict__ rem, int* __restrict__ mask_eff, int* __restrict__ force_eff, int* __restrict__ held) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * SND_ROWS_PER_WG + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= B) return;                              // (wave-uniform)
  const int s1 = t_done + 1;                       // the step this launch prepares
  int r0 = 0, r1 = 0;                              // rem of pitches lane and lane + 64
  if (t_done >= 0) {
    r0 = rem[b * 128 + lane];
    r1 = rem[b * 128 + 64 + lane];
    // the accepted notes of the decided step (grid_to_pr_kernel's parse, output.hip): lane l < 15 reads slot l + 1
    int note = -1;                                 // pitch | duration << 8, or -1: the slot is skipped
    bool eos = false;
    if (lane < 15) {
      const long* xs = xhat + (b * 32 + t_done) * 96 + (lane + 1) * 6;
      const long p = xs[0];
      int d = 0;
#pragma unroll
      for (int k = 1; k < 6; k++) d = 2 * d + (int)(xs[k] & 1);
      eos = p == 129;
      if (p >= 0 && p <= 127) note = (int)p | (min(d + 1, 32 - t_done) << 8);
    }
    const unsigned long long ended = __ballot(eos);
    const int L = ended ? __ffsll((long long)ended) - 1 : 15;    // slots before the first <eos>
    r0 = max(r0 - 1, 0);
    r1 = max(r1 - 1, 0);
#pragma unroll
    for (int s = 0; s < 15; s++) {                 // in slot order: a later onset of a pitch replaces the earlier one
      const int v = __shfl(note, s, 64);
      if (s < L && v >= 0) {
        const int p = v & 255, left = (v >> 8) - 1;
        if (p == lane) r0 = left;
        if (p == lane + 64) r1 = left;
      }
    }
  }
  rem[b * 128 + lane] = (unsigned char)r0;
  rem[b * 128 + 64 + lane] = (unsigned char)r1;
  const unsigned long long h0 = __ballot(r0 > 0), h1 = __ballot(r1 > 0);       // the held set H: mask words 0-1 and 2-3
  const int h = __popcll(h0) + __popcll(h1);
  const bool sel = steps.at(b, s1) != 0;
  if (mask_eff && lane < 4) {
    const unsigned hw = (unsigned)((lane < 2 ? h0 : h1) >> (32 * (lane & 1)));
    const unsigned base = mask_base.p ? (unsigned)mask_base.p[((mask_base.one ? 0 : b * 32) + s1) * 4 + lane] : 0xffffffffu;
    mask_eff[(b * 32 + s1) * 4 + lane] = (int)((sel && (control[0] & 1u)) ? base & ~hw : base);
  }
  if (force_eff) {
    // the rule of note_count_force_build_kernel (keep.hip: the twin of this block) with lo = F', hi = H' and no room flag, one lane per word
    const long R = 32 * B, r = (long)s1 * B + b;
    const int w = (lane < 15 && force_base) ? force_base[lane * R + r] : -1;
    const bool owned = __ballot(lane < 15 && (w == 129 || w < -1)) != 0;
    const unsigned long long forced = __ballot(lane < 15 && w >= 0);
    const int J = forced ? 64 - __clzll((long long)forced) : 0;               // the forced prefix
    const int K = kmax.at(b, s1), F = fmin.at(b, s1);
    const int Hc = K == 0 ? 15 : min(max(K - h, 0), 15), Fc = min(max(F - h, 0), 15);
    const int Lc = min(Fc, Hc), E = max(Hc, J);                               // the ceiling wins
    int v = w;
    if (sel && !owned && v == -1) {
      if (lane < Lc) v = PTV_FORCE_NOT_EOS;
      else if (lane == E) v = 129;
    }
    if (lane < 15) force_eff[lane * R + r] = v;
  }
  if (lane == 0) held[b * 32 + s1] = h;
}

}  // namespace ptv
using namespace ptv;

extern "C" int ptv_sounding_step(const long* xhat, int t_done, long B, const int* mask_base, int mask_rows, const int* force_base,
                                 const unsigned char* max_sounding, int max_rows, const unsigned char* min_sounding, int min_rows,
                                 const unsigned char* steps, int steps_rows, const unsigned* control, unsigned char* rem, int* mask_eff,
                                 int* force_eff, int* held, void* stream) {
  SndPerStep<int> m;
  SndPerStep<unsigned char> k, f, s;
  if (!max_sounding || !min_sounding || !steps || !control || !rem || !held || B < 1 || t_done < -1 || t_done > 30) return PTV_ERR_ARG;
  if (t_done >= 0 && !xhat) return PTV_ERR_ARG;                               // (t_done = -1 reads no grid)
  if (!snd_per_step(m, mask_base, mask_rows, B) || !snd_per_step(k, max_sounding, max_rows, B) ||
      !snd_per_step(f, min_sounding, min_rows, B) || !snd_per_step(s, steps, steps_rows, B))
    return PTV_ERR_ARG;
  if ((mask_base && !mask_eff) || (force_base && !force_eff)) return PTV_ERR_ARG;   // a base table without its output
  if ((mask_eff && mask_eff == mask_base) || (force_eff && force_eff == force_base)) return PTV_ERR_ARG;
  hipLaunchKernelGGL(sounding_step_kernel, dim3((unsigned)((B + SND_ROWS_PER_WG - 1) / SND_ROWS_PER_WG)), dim3(64 * SND_ROWS_PER_WG), 0,
                     (hipStream_t)stream, xhat, t_done, B, m, force_base, k, f, s, control, rem, mask_eff, force_eff, held);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
