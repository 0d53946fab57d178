// keep.hip -- the force arrays of a free-running decode, built on the device (include/ptvae_hip.h "Kept steps", "Kept voices", "Kept
// rhythm", "Kept top voice", "Duration limits"; INTEGRATION.md under the same names).  A time step of a grid x is
// free (0), kept whole (1), keeps its lowest notes -- a prefix of its note decisions, since the grammar orders a step by ascending pitch
// -- (2), keeps its note count and durations (3: K decisions that are free but may not be <eos>, then a forced <eos>), or keeps its
// highest notes -- a suffix -- (4: J decisions that are free, never <eos> and under a ceiling that leaves room for what follows, then the
// kept pitches and a forced <eos>).  Every entry point accepts its own set of these bytes; ONE plan function states what each does to the
// 15 decisions of a step, and the builder kernel, the split kernel and the err scan all read that plan.  The duration-range builder and
// the note-count builder ("Note-count limits") read the arrays of a keep, not a grid, and are kernels of their own.  No atomics, no LDS, no workspace: every output element has one writer.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/ptvae_hip.h"
#include "../../include/ptvae_hip_debug.h"

namespace ptv {

// ---- a per-(sample, time step) operand [rows][32], rows 1 or B, with "one row serves every sample" resolved once on the host
template <typename T>
struct PerStep {
  const T* p;
  int one;
  __device__ __forceinline__ T at(long b, long t) const { return p[(one ? 0 : b * 32) + t]; }
  __device__ __forceinline__ int at_or(long b, long t, int none) const { return p ? (int)at(b, t) : none; }       // (a NULL limit)
};
template <typename T>
static bool per_step(PerStep<T>& o, const T* p, int rows, long B) {      // (a NULL operand still names a row count)
  if (rows != 1 && rows != B) return false;
  o.p = p;
  o.one = (rows == 1 && B != 1) ? 1 : 0;
  return true;
}

// the selection of one call.  accept: bit m set = the mode byte m (1..4) is this entry point's; any other non-zero byte leaves the step
// free and sets bit 1 of err.  ANY_BYTE_WHOLE instead: every non-zero byte is a whole step (ptv_keep_force_build's steps array).
// pitch_lim / count_lim: below / lowest of a voice step, above / highest of a top step
constexpr unsigned WHOLE = 1u << 1, VOICE = 1u << 2, RHYTHM = 1u << 3, TOP = 1u << 4, ANY_BYTE_WHOLE = 1u << 8;
struct StepSel {
  PerStep<unsigned char> mode;
  PerStep<int> pitch_lim, count_lim;
  unsigned accept;
};
static bool step_sel(StepSel& v, unsigned accept, const unsigned char* mode, int mode_rows, const int* pitch_lim, int pitch_rows,
                     const int* count_lim, int count_rows, long B) {
  v.accept = accept;
  return mode && per_step(v.mode, mode, mode_rows, B) && per_step(v.pitch_lim, pitch_lim, pitch_rows, B) &&
         per_step(v.count_lim, count_lim, count_rows, B);
}

// ---- the rules, each stated once ---------------------------------------------------------------------------------------------------
// Every rule reads the PITCH COLUMN of its step, p[s] = x[b][t][s][0] for the slots s = 1..15, which step_plan loads once; the loops
// below run over all 15 slots with constant bounds, so that they unroll and the column stays in registers.
// the length of a step: first slot 1..15 holding <eos>, else 15; has_eos: whether one was found
__device__ __forceinline__ int step_len(const long (&p)[16], bool& has_eos) {
  int L = 15;
  has_eos = false;
#pragma unroll
  for (int s = 15; s >= 1; s--) if (p[s] == 129) { L = s; has_eos = true; }
  return L;
}
// mode 2: K, the length of the kept prefix.  Slots s = 1..15 in order: stop at K == lowest, at <eos>, at a pitch outside 0..127 (bit 0 of
// e) and at the first pitch >= below; every slot before the stop is a kept note, so K = s - 1 at the stop.
__device__ __forceinline__ int voice_prefix_len(const long (&p)[16], int below, int lowest, int& e) {
  int K = 0;
  bool stop = false;
#pragma unroll
  for (int s = 1; s <= 15; s++) {
    stop = stop || K == lowest || p[s] == 129;
    if (!stop && (p[s] < 0 || p[s] > 127)) { e |= 1; stop = true; }
    stop = stop || p[s] >= below;
    K += stop ? 0 : 1;
  }
  return K;
}
// mode 4: h, the length of the kept suffix of the K notes in slots 1..K.  Slots s = K..1 in order: stop at h == highest, at a pitch outside
// 0..127 and at the first pitch < above; every slot before the stop is a kept note.  low: the lowest kept pitch, 128 without one.
__device__ __forceinline__ int top_suffix_len(const long (&p)[16], int K, int above, int highest, long& low) {
  int h = 0;
  bool stop = false;
  low = 128;
#pragma unroll
  for (int s = 15; s >= 1; s--) {
    if (s > K) continue;
    stop = stop || h == highest || p[s] < 0 || p[s] > 127 || p[s] < above;
    if (!stop) { h++; low = p[s]; }
  }
  return h;
}
__device__ __forceinline__ int clamp_to(long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// what a step's mode byte does to its 15 note decisions n = 0..14 (decision n decides slot n + 1):
//   n < lead         free under a word: PTV_FORCE_NOT_EOS (mode 3) or PTV_FORCE_BELOW(top_ceiling) (mode 4)
//   lead <= n < end  forced to the slot's pitch where that lies in 0..129 (under modes 2 and 4 every one of them does: 0..127)
//   n == eos         a forced <eos> (15: the step has 15 notes and no decision is left for it)
//   d0 <= n < d1     the duration words are x's bits where they are 0 / 1
// Everything else is free (-1).  m: the mode byte as it acts (0 for a byte the entry point does not accept); p: the pitch column (not
// loaded for a free step); notes, low: K and the lowest kept pitch of a top step.
struct StepPlan {
  int m, lead, end, eos, d0, d1, notes, kept_n, err;
  long low, p[16];
};
// flags: bit 0 = no durations at a voice / rhythm step, but durations only for the kept notes at a top step; bit 1 = room ceilings
__device__ __forceinline__ StepPlan step_plan(const long* __restrict__ xs, const StepSel& v, int flags, long b, long t) {
  StepPlan pl = {0, 0, 0, 15, 0, 0, 0, 0, 0, 128, {}};
  int m = v.mode.at(b, t);
  if (v.accept & ANY_BYTE_WHOLE) m = m ? 1 : 0;
  else if (m > 4 || !((v.accept >> m) & 1u)) { pl.err = m ? 2 : 0; m = 0; }
  pl.m = m;
  if (m == 0) return pl;
#pragma unroll
  for (int s = 1; s <= 15; s++) pl.p[s] = xs[s * 6];
  if (m == 2) {                                    // the prefix; its <eos> is never forced; err: only what the prefix scan meets
    const int below = clamp_to(v.pitch_lim.at_or(b, t, 128), 0, 128), lowest = clamp_to(v.count_lim.at_or(b, t, 15), 0, 15);
    pl.end = pl.kept_n = voice_prefix_len(pl.p, below, lowest, pl.err);
    pl.d1 = (flags & 1) ? 0 : pl.end;
    return pl;
  }
  bool has_eos;
  const int L = step_len(pl.p, has_eos);
  if (m == 1) {                                    // the whole step, <eos> included; kept_n: the pitch words actually forced
    pl.end = pl.d1 = L;
#pragma unroll
    for (int s = 1; s <= 15; s++) {
      if (s > L) continue;
      if (pl.p[s] >= 0 && pl.p[s] <= 129) pl.kept_n++; else pl.err |= 1;
    }
    return pl;
  }
  const int K = has_eos ? L - 1 : 15;              // K note positions, then the <eos>
  pl.notes = pl.end = pl.eos = pl.d1 = K;
  if (m == 3) {
    pl.lead = pl.kept_n = K;
    if (flags & 1) pl.d1 = 0;
  } else {                                         // (both limits NULL: the very top note)
    const int above = clamp_to(v.pitch_lim.at_or(b, t, 0), 0, 128);
    const int highest = clamp_to(v.count_lim.at_or(b, t, v.pitch_lim.p ? 15 : 1), 0, 15);
    pl.kept_n = top_suffix_len(pl.p, K, above, highest, pl.low);
    pl.lead = K - pl.kept_n;
    if (flags & 1) pl.d0 = pl.lead;
  }
#pragma unroll
  for (int s = 1; s <= 15; s++) {                  // err: a note position that holds no note; at a top step also one not above the slot before it
    if (s > K) continue;
    if (pl.p[s] < 0 || pl.p[s] > 127) pl.err |= 1;
    if (m == 4 && s >= 2 && pl.p[s] <= pl.p[s - 1]) pl.err |= 1;
  }
  return pl;
}
// the ceiling of the free decision n < J = lead of a top step, clamped into 1..128.  Lanes: the pitch of x's next note, so every re-drawn
// voice stays under its old upper neighbour; room (flags bit 1): the lowest kept pitch (128 without one) less one semitone per decision
// still to come before it.  Either leaves a note for every later decision whatever is drawn here, if the step ascends strictly.
__device__ __forceinline__ int top_ceiling(const StepPlan& pl, int n, int room) {
  if (room) return clamp_to(pl.low - (pl.lead - 1 - n), 1, 128);
  return clamp_to(n + 1 < pl.notes ? pl.p[n + 2 < 16 ? n + 2 : 15] : 128, 1, 128);
}
// err[b], by its one writer: the bits of the sample's 32 steps (the pitch columns again: L2 hits)
__device__ __forceinline__ int sample_err(const long* __restrict__ x, const StepSel& v, long b) {
  int e = 0;
  for (int t = 0; t < 32; t++) e |= step_plan(x + (b * 32 + t) * 96, v, 0, b, t).err;
  return e;
}

// ---- the builder: one thread per (time step, sample) row r = t * B + b of the step-major arrays -- a wave's stores are 64 consecutive
// words of every one of the 15 + 75 planes, while it reads its own 768 contiguous bytes of the sample-major grid.  kept_n may be NULL.
__global__ void keep_force_build_kernel(const long* __restrict__ x, StepSel v, int flags, long B, int* __restrict__ force_pitch,
                                        int* __restrict__ force_dur, int* __restrict__ kept_n, int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long R = 32 * B, M = 15 * R;
  if (r >= R) return;
  const long t = r / B, b = r % B;
  const long* xs = x + (b * 32 + t) * 96;
  const StepPlan pl = step_plan(xs, v, flags, b, t);
#pragma unroll
  for (int n = 0; n < 15; n++) {
    const long p = pl.p[n + 1];
    int w = -1;
    if (n < pl.lead) w = pl.m == 4 ? PTV_FORCE_BELOW(top_ceiling(pl, n, flags & 2)) : PTV_FORCE_NOT_EOS;
    else if (n < pl.end) w = (p >= 0 && p <= 129) ? (int)p : -1;
    else if (n == pl.eos) w = 129;
    force_pitch[n * R + r] = w;
#pragma unroll
    for (int d = 0; d < 5; d++) {
      const long q = xs[(n + 1) * 6 + 1 + d];
      force_dur[d * M + n * R + r] = (n >= pl.d0 && n < pl.d1 && (q == 0 || q == 1)) ? (int)q : -1;
    }
  }
  if (kept_n) kept_n[b * 32 + t] = pl.kept_n;
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
// slots 1.. of dst: the cnt slots of src from slot s0 on, an <eos> (if a slot is left for it), <pad>; cnt = 0: the empty step
__device__ __forceinline__ void put_notes(long* __restrict__ dst, const long* __restrict__ src, int s0, int cnt) {
  for (int j = 1; j <= cnt; j++) put_slot(dst, j, src + (s0 + j - 1) * 6);
  if (cnt < 15) put_token(dst, cnt + 1, 129);
  for (int j = cnt + 2; j <= 15; j++) put_token(dst, j, 130);
}
__global__ void grid_split_kernel(const long* __restrict__ x, StepSel v, long B, long* __restrict__ voice, long* __restrict__ rest,
                                  int* __restrict__ kept_n, int* __restrict__ err) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= 32 * B) return;
  const long b = r >> 5, t = r & 31;
  const long* xs = x + r * 96;
  long* vo = voice + r * 96;
  long* re = rest + r * 96;
  const StepPlan pl = step_plan(xs, v, 0, b, t);
  put_slot(vo, 0, xs);
  put_slot(re, 0, xs);
  if (pl.m == 2) {                                 // the prefix; rest: what follows it up to and including x's <eos> (one added where x has none)
    put_notes(vo, xs, 1, pl.end);
    int j = 1;
    bool ended = false;
    for (int s = pl.end + 1; s <= 15 && !ended; s++) {
      put_slot(re, j++, xs + s * 6);
      ended = xs[s * 6] == 129;
    }
    if (!ended && j <= 15) put_token(re, j++, 129);
    for (; j <= 15; j++) put_token(re, j, 130);
  } else if (pl.m == 4) {                          // the suffix; rest: the notes under it
    put_notes(vo, xs, pl.lead + 1, pl.kept_n);
    put_notes(re, xs, 1, pl.lead);
  } else {                                         // a whole step goes to voice as it is, a free one to rest; the other grid gets the empty step
    long* whole = pl.m == 1 ? vo : re;
    for (int s = 1; s <= 15; s++) put_slot(whole, s, xs + s * 6);
    put_notes(pl.m == 1 ? re : vo, xs, 1, 0);
  }
  kept_n[r] = pl.kept_n;
  if (t == 0) err[b] = sample_err(x, v, b);
}

// ---- duration limits: the force arrays whose duration words are PTV_FORCE_DUR_RANGE(lo, hi) -- the decision stays free, the note's
// duration ends in the range -- alone or built INTO the arrays of an existing keep.  One thread per row r = t * B + b as in the builder
// above: a wave's accesses are 64 consecutive words of every one of the 15 + 75 planes
__global__ void dur_range_force_build_kernel(PerStep<unsigned char> lo, PerStep<unsigned char> hi, PerStep<unsigned char> steps,
                                             const int* __restrict__ src_pitch, const int* __restrict__ src_dur, long B,
                                             int* __restrict__ force_pitch, int* __restrict__ force_dur, int* __restrict__ yielded) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long R = 32 * B, M = 15 * R;
  if (r >= R) return;
  const long t = r / B, b = r % B;
  const bool sel = steps.at(b, t) != 0;
  const int h = min(max((int)hi.at(b, t), 1), 32);        // the ceiling, clamped into 1..32 ...
  const int f = max((int)lo.at(b, t), 1);                 // ... wins over the floor
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

// ---- note-count limits: the pitch words of a step written from a floor and a ceiling in note counts instead of from a grid -- a forced
// <eos> at the ceiling, PTV_FORCE_NOT_EOS (room, flags bit 0: PTV_FORCE_BELOW ceilings) under the floor -- alone or built INTO the arrays
// of an existing keep (include/ptvae_hip.h "Note-count limits": the rule).  One thread per row r = t * B + b as above; the 15 source words
// of the step are loaded once, and J, the owned test and E come from that one pass over registers
__global__ void note_count_force_build_kernel(PerStep<unsigned char> lo, PerStep<unsigned char> hi, PerStep<unsigned char> steps,
                                              const int* __restrict__ src_pitch, const int* __restrict__ src_dur, int flags, long B,
                                              int* __restrict__ force_pitch, int* __restrict__ force_dur, int* __restrict__ yielded) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long R = 32 * B, M = 15 * R;
  if (r >= R) return;
  const long t = r / B, b = r % B;
  const bool sel = steps.at(b, t) != 0;
  const int H = min((int)hi.at(b, t), 15), F = min((int)lo.at(b, t), 15);      // (bytes: never below 0)
  const int L = min(F, H);                                                      // the ceiling wins
  int w[15];
#pragma unroll
  for (int n = 0; n < 15; n++) w[n] = src_pitch ? src_pitch[n * R + r] : -1;
  int J = 0;
  long last = -1;                                  // the prefix's last forced pitch
  bool owned = false;
#pragma unroll
  for (int n = 0; n < 15; n++) {
    owned = owned || w[n] == 129 || w[n] < -1;
    if (w[n] >= 0) { J = n + 1; last = w[n]; }
  }
  const int E = max(H, J);
  const bool act = sel && !owned;
#pragma unroll
  for (int n = 0; n < 15; n++) {
    int v = w[n];
    if (act && v == -1) {
      if (n < L) v = (flags & 1) ? PTV_FORCE_BELOW(128 - (L - 1 - n)) : PTV_FORCE_NOT_EOS;
      else if (n == E) v = 129;
    }
    force_pitch[n * R + r] = v;
#pragma unroll
    for (int d = 0; d < 5; d++) force_dur[d * M + n * R + r] = src_dur ? src_dur[d * M + n * R + r] : -1;
  }
  int y = 0;
  if (sel && owned) y = 2;
  else if (sel) {
    if (F > H) y |= 1;
    if (J > H) y |= 4;
    if ((flags & 1) && J > 0 && J < L && last <= 127 && last + 1 >= 128 - (L - 1 - J)) y |= 8;
  }
  yielded[b * 32 + t] = y;
}

// test aid: the rule of a range word itself (dur_range_allowed / dur_range_bit, philox.hpp: the only statement of it) on caller-supplied triples
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

// ---- the host side of the six grid-reading entry points: the argument checks they share, then one launch of 256-thread blocks, one
// thread per row.  Each entry point passes its accepted mode bytes and its largest flags word; nothing is written when it refuses.
static unsigned row_blocks(long B) { return (unsigned)((32 * B + 255) / 256); }

static int keep_build(unsigned accept, int max_flags, bool counts, const long* x, const unsigned char* mode, int mode_rows,
                      const int* pitch_lim, int pitch_rows, const int* count_lim, int count_rows, int flags, long B, int* force_pitch,
                      int* force_dur, int* kept_n, int* err, void* stream) {
  StepSel v;
  if (!x || !force_pitch || !force_dur || (counts && !kept_n) || !err || B < 1 || flags < 0 || flags > max_flags ||
      !step_sel(v, accept, mode, mode_rows, pitch_lim, pitch_rows, count_lim, count_rows, B))
    return PTV_ERR_ARG;
  hipLaunchKernelGGL(keep_force_build_kernel, dim3(row_blocks(B)), dim3(256), 0, (hipStream_t)stream, x, v, flags, B, force_pitch,
                     force_dur, kept_n, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
static int grid_split(unsigned accept, const long* x, const unsigned char* mode, int mode_rows, const int* pitch_lim, int pitch_rows,
                      const int* count_lim, int count_rows, long B, long* voice, long* rest, int* kept_n, int* err, void* stream) {
  StepSel v;
  if (!x || !voice || !rest || !kept_n || !err || B < 1 ||
      !step_sel(v, accept, mode, mode_rows, pitch_lim, pitch_rows, count_lim, count_rows, B))
    return PTV_ERR_ARG;
  hipLaunchKernelGGL(grid_split_kernel, dim3(row_blocks(B)), dim3(256), 0, (hipStream_t)stream, x, v, B, voice, rest, kept_n, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
}  // namespace ptv
using namespace ptv;

extern "C" int ptv_keep_force_build(const long* x, const unsigned char* steps, int steps_rows, long B, int* force_pitch, int* force_dur,
                                    int* err, void* stream) {
  return keep_build(ANY_BYTE_WHOLE, 0, false, x, steps, steps_rows, nullptr, 1, nullptr, 1, 0, B, force_pitch, force_dur, nullptr, err, stream);
}

extern "C" int ptv_keep_voice_force_build(const long* x, const unsigned char* mode, int mode_rows, const int* below, int below_rows,
                                          const int* lowest, int lowest_rows, int flags, long B, int* force_pitch, int* force_dur,
                                          int* kept_n, int* err, void* stream) {
  return keep_build(WHOLE | VOICE, 1, true, x, mode, mode_rows, below, below_rows, lowest, lowest_rows, flags, B, force_pitch, force_dur,
                    kept_n, err, stream);
}

extern "C" int ptv_grid_split_voice(const long* x, const unsigned char* mode, int mode_rows, const int* below, int below_rows,
                                    const int* lowest, int lowest_rows, long B, long* voice, long* rest, int* kept_n, int* err,
                                    void* stream) {
  return grid_split(WHOLE | VOICE, x, mode, mode_rows, below, below_rows, lowest, lowest_rows, B, voice, rest, kept_n, err, stream);
}

extern "C" int ptv_keep_rhythm_force_build(const long* x, const unsigned char* mode, int mode_rows, int flags, long B, int* force_pitch,
                                           int* force_dur, int* kept_n, int* err, void* stream) {
  return keep_build(WHOLE | RHYTHM, 1, true, x, mode, mode_rows, nullptr, 1, nullptr, 1, flags, B, force_pitch, force_dur, kept_n, err,
                    stream);
}

extern "C" int ptv_keep_top_force_build(const long* x, const unsigned char* mode, int mode_rows, const int* above, int above_rows,
                                        const int* highest, int highest_rows, int flags, long B, int* force_pitch, int* force_dur,
                                        int* kept_n, int* err, void* stream) {
  return keep_build(WHOLE | TOP, 3, true, x, mode, mode_rows, above, above_rows, highest, highest_rows, flags, B, force_pitch, force_dur,
                    kept_n, err, stream);
}

extern "C" int ptv_grid_split_top(const long* x, const unsigned char* mode, int mode_rows, const int* above, int above_rows,
                                  const int* highest, int highest_rows, long B, long* voice, long* rest, int* kept_n, int* err,
                                  void* stream) {
  return grid_split(WHOLE | TOP, x, mode, mode_rows, above, above_rows, highest, highest_rows, B, voice, rest, kept_n, err, stream);
}

extern "C" int ptv_dur_range_force_build(const unsigned char* lo, int lo_rows, const unsigned char* hi, int hi_rows, const unsigned char* steps,
                                         int steps_rows, const int* src_pitch, const int* src_dur, long B, int* force_pitch, int* force_dur,
                                         int* yielded, void* stream) {
  PerStep<unsigned char> l, h, s;
  if (!lo || !hi || !steps || !force_pitch || !force_dur || !yielded || B < 1) return PTV_ERR_ARG;
  if (!per_step(l, lo, lo_rows, B) || !per_step(h, hi, hi_rows, B) || !per_step(s, steps, steps_rows, B)) return PTV_ERR_ARG;
  if ((src_pitch == nullptr) != (src_dur == nullptr) || src_pitch == force_pitch || src_dur == force_dur) return PTV_ERR_ARG;
  hipLaunchKernelGGL(dur_range_force_build_kernel, dim3(row_blocks(B)), dim3(256), 0, (hipStream_t)stream, l, h, s, src_pitch, src_dur, B,
                     force_pitch, force_dur, yielded);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_note_count_force_build(const unsigned char* lo, int lo_rows, const unsigned char* hi, int hi_rows, const unsigned char* steps,
                                          int steps_rows, const int* src_pitch, const int* src_dur, int flags, long B, int* force_pitch,
                                          int* force_dur, int* yielded, void* stream) {
  PerStep<unsigned char> l, h, s;
  if (!lo || !hi || !steps || !force_pitch || !force_dur || !yielded || B < 1 || flags < 0 || flags > 1) return PTV_ERR_ARG;
  if (!per_step(l, lo, lo_rows, B) || !per_step(h, hi, hi_rows, B) || !per_step(s, steps, steps_rows, B)) return PTV_ERR_ARG;
  if ((src_pitch == nullptr) != (src_dur == nullptr) || src_pitch == force_pitch || src_dur == force_dur) return PTV_ERR_ARG;
  hipLaunchKernelGGL(note_count_force_build_kernel, dim3(row_blocks(B)), dim3(256), 0, (hipStream_t)stream, l, h, s, src_pitch, src_dur,
                     flags, B, force_pitch, force_dur, yielded);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_debug_dur_range(const int* words, const int* d, const int* prefix, long rows, unsigned char* out, void* stream) {
  if (!words || !d || !prefix || !out || rows <= 0) return PTV_ERR_ARG;
  hipLaunchKernelGGL(dur_range_debug_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, words, d, prefix, rows, out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
