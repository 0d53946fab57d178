// output.hip -- the inverse data contract: what the decoders emit -> the tensors the model consumes, for a whole batch on the device.
//
// data.hip turns a raw bank into (pr_mat, x, c); here the decoded PianoTree grid goes back to a piano-roll, a note list and a canonical
// input grid (PtvaeDecoder.grid_to_pr_and_notes, ptvae.py:558-575, per sample on the host in the reference), and the chord decoder's
// logits go to the chord tokens it feeds back (ptvae.py:72-78) plus the 14-column bank layout.
// Integer / index work, bit-exact against the reference-generated fixture (tests/golden/output_path.npz).
// HBM-bound: reads 24 KB (grid int64) + writes 16 KB (pr_mat f32) + 24 KB (x_clean int64) + <= 5.6 KB (notes) per sample.  The three
// large streams (grid, pr_mat, x_clean) are 16-byte accesses of consecutive lanes to consecutive addresses.  The small ones are not: a
// lane writes a note as three 4-byte stores at off[t] + k (consecutive within a step only), and chord_tokens_kernel gives each thread
// one (step, sample) row, i.e. strides of 48 / 96 bytes on the loads and 144 / 56 bytes on the stores (3 KB per sample in all).
// Where this departs from the reference on values no decoder emits: a grid value outside int32 or below 0 counts as a bad pitch / a
// bad duration bit (numpy would let a negative pitch index wrap around), and a duration "bit" such as 10 or 11 is flagged although
// int(''.join(..), 2) would read the concatenated digits as binary.  tests/output_path_ref.py restates the rule as implemented here.
#include "common.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

constexpr int GP_T = 32;          // time steps
constexpr int GP_NMAX = 15;       // note rows a step can hold after <sos>
constexpr int GP_PRS = 132;       // bytes per piano-roll row in LDS: 33 words, so the 32 parsing lanes fall into 32 different banks

// One workgroup per sample.  The slab is staged into LDS as int32 (values outside int32 become -1: no pitch, no duration bit) with a
// row stride of R*6 + 1 words (odd: lane t reading its row r is conflict-free).  Lanes 0..31 of wave 0 each parse one time step in row
// order -- "stop at <eos>", "later row wins" and the skip rule live there --, a wave prefix sum of the per-step counts gives the note
// offsets, and then the whole workgroup streams the three outputs.
__global__ __launch_bounds__(256) void grid_to_pr_kernel(const long* __restrict__ grid, int R, int skip, int rows, int min_pitch, int pitch_eos,
                                                         float* __restrict__ pr_mat, int* __restrict__ notes, int note_cap,
                                                         int* __restrict__ count, long* __restrict__ x_clean, int* __restrict__ err) {
  __shared__ int g[GP_T * (16 * 6 + 1)];
  __shared__ unsigned char pr[GP_T * GP_PRS];
  __shared__ int acc[GP_T * GP_NMAX];        // accepted notes of step t in decoded order: pitch | dur << 8
  __shared__ int cnt[GP_T], off[GP_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int RW = R * 6, STR = RW + 1;
  const long2* src = reinterpret_cast<const long2*>(grid + (long)b * GP_T * RW);
  for (int i = tid; i < GP_T * RW / 2; i += 256) {
    const long2 v = src[i];
    const int f = 2 * i, t0 = f / RW, t1 = (f + 1) / RW;
    g[t0 * STR + (f - t0 * RW)] = (v.x < 0 || v.x > 0x7fffffffL) ? -1 : (int)v.x;
    g[t1 * STR + (f + 1 - t1 * RW)] = (v.y < 0 || v.y > 0x7fffffffL) ? -1 : (int)v.y;
  }
  for (int i = tid; i < GP_T * GP_PRS / 4; i += 256) reinterpret_cast<int*>(pr)[i] = 0;
  __syncthreads();
  if (tid < 64) {                                  // wave 0; lanes 32..63 only take part in the shuffles
    const int t = tid;
    int n = 0, e = 0, first = 0;
    if (t < GP_T) {
      const int* row = g + t * STR + skip * 6;
      for (int r = 0; r < rows; r++, row += 6) {
        if (row[0] == pitch_eos) break;
        const int pitch = row[0] < 0 ? -1 : row[0] + min_pitch;
        int d = 0, bad = 0;
#pragma unroll
        for (int k = 1; k < 6; k++) { const int v = row[k]; bad |= (v != 0 && v != 1); d = 2 * d + (v & 1); }
        const int f = ((pitch < 0 || pitch > 127) ? 1 : 0) | (bad ? 2 : 0);
        if (f) {                                   // the reference raises here (ValueError from int(.., 2) before IndexError at pr[t, pitch])
          if (!e) first = bad ? 4 : 0;
          e |= f;
          continue;
        }
        pr[t * GP_PRS + pitch] = (unsigned char)min(d + 1, GP_T - t);
        acc[t * GP_NMAX + n] = pitch | ((d + 1) << 8);
        n++;
      }
      cnt[t] = n;
    }
    int incl = n;                                  // inclusive prefix sum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (t >= o) incl += u; }
    if (t < GP_T) off[t] = incl - n;
    const unsigned long long flagged = __ballot(e != 0);
    int all = e;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) all |= __shfl_xor(all, o, 64);
    const int lead = flagged ? __ffsll((long long)flagged) - 1 : 0;
    const int kind = __shfl(first, lead, 64);
    const int over = __ballot(n > 14) ? 8 : 0;     // x_clean keeps 14 notes of a step (only max_notes >= 15 gets here)
    const int total = __shfl(incl, 31, 64);
    if (t == 0) {
      err[b] = all | (flagged ? kind : 0) | (x_clean ? over : 0);
      if (count) count[b] = total;
    }
  }
  __syncthreads();
  if (pr_mat) {
    float4* dst = reinterpret_cast<float4*>(pr_mat + (long)b * GP_T * 128);
    for (int i = tid; i < GP_T * 32; i += 256) {
      const unsigned char* p = pr + (i >> 5) * GP_PRS + (i & 31) * 4;
      dst[i] = make_float4((float)p[0], (float)p[1], (float)p[2], (float)p[3]);
    }
  }
  if (notes) {
    int* dst = notes + (long)b * note_cap * 3;
    for (int j = tid; j < GP_T * GP_NMAX; j += 256) {
      const int t = j / GP_NMAX, k = j - t * GP_NMAX;
      if (k < cnt[t]) {
        const int v = acc[j];
        int* q = dst + (off[t] + k) * 3;
        q[0] = v & 255; q[1] = t; q[2] = v >> 8;
      }
    }
  }
  if (x_clean) {
    long2* dst = reinterpret_cast<long2*>(x_clean + (long)b * GP_T * 96);
    for (int i = tid; i < GP_T * 48; i += 256) {
      long v[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int f = 2 * i + h, t = f / 96, r = (f - t * 96) / 6, k = f - t * 96 - r * 6;
        const int n = min(cnt[t], 14);
        if (r == 0) v[h] = k == 0 ? 128 : 2;
        else if (r <= n) {
          const int a = acc[t * GP_NMAX + r - 1], e = (a >> 8) - 1;
          v[h] = k == 0 ? (a & 255) : ((e >> (5 - k)) & 1);
        } else v[h] = k == 0 ? (r == n + 1 ? 129 : 130) : 2;
      }
      dst[i] = make_long2(v[0], v[1]);
    }
  }
}

// One thread per (step, sample) row of the chord decoder's logits; first maximal index wins, a chroma pair is 1 only where the second
// logit is strictly larger.
__global__ __launch_bounds__(256) void chord_tokens_kernel(const float* __restrict__ root, const float* __restrict__ chroma,
                                                           const float* __restrict__ bass, float* __restrict__ c, float* __restrict__ chord14,
                                                           int T, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T * B) return;
  const int t = i / B, b = i - t * B;
  const float* r = root + (long)i * 12;
  const float* h = chroma + (long)i * 24;
  const float* s = bass + (long)i * 12;
  int ir = 0, ib = 0;
  float mr = r[0], mb = s[0];
#pragma unroll
  for (int k = 1; k < 12; k++) {
    if (r[k] > mr) { mr = r[k]; ir = k; }
    if (s[k] > mb) { mb = s[k]; ib = k; }
  }
  float bits[12];
#pragma unroll
  for (int k = 0; k < 12; k++) bits[k] = h[2 * k + 1] > h[2 * k] ? 1.f : 0.f;
  const long o = (long)b * T + t;
  if (c) {
    float* q = c + o * 36;
#pragma unroll
    for (int k = 0; k < 12; k++) { q[k] = k == ir ? 1.f : 0.f; q[12 + k] = bits[k]; q[24 + k] = k == ib ? 1.f : 0.f; }
  }
  if (chord14) {
    float* q = chord14 + o * 14;
    q[0] = (float)ir;
#pragma unroll
    for (int k = 0; k < 12; k++) q[1 + k] = bits[k];
    q[13] = (float)ib;
  }
}

}  // namespace ptv

extern "C" int ptv_grid_to_pr(const long* grid, int B, int R, int max_notes, int min_pitch, int pitch_eos, float* pr_mat, int* notes, int* count,
                              long* x_clean, int* err, void* stream) {
  if (!grid || !err || B <= 0 || (R != 15 && R != 16) || max_notes < 1 || max_notes > R || min_pitch < 0 || min_pitch > 127 || pitch_eos < 0)
    return PTV_ERR_ARG;
  if ((notes != nullptr) != (count != nullptr)) return PTV_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(grid) | reinterpret_cast<uintptr_t>(pr_mat) | reinterpret_cast<uintptr_t>(x_clean)) & 15) return PTV_ERR_ARG;
  const int skip = R == 16 ? 1 : 0;                                       // row 0 of a 16-row step is <sos> (the reference's grid[:, 1:])
  const int rows = max_notes < R - skip ? max_notes : R - skip;           // a step holds 15 rows after <sos>
  hipLaunchKernelGGL(ptv::grid_to_pr_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, grid, R, skip, rows, min_pitch, pitch_eos, pr_mat, notes,
                     32 * max_notes, count, x_clean, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_chord_tokens(const float* root, const float* chroma, const float* bass, float* c, float* chord14, int T, int B, void* stream) {
  if (!root || !chroma || !bass || (!c && !chord14) || T <= 0 || B <= 0) return PTV_ERR_ARG;
  hipLaunchKernelGGL(ptv::chord_tokens_kernel, dim3(ptv::cdiv((long)T * B, 256)), dim3(256), 0, (hipStream_t)stream, root, chroma, bass, c, chord14,
                     T, B);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
