// dataset.hip -- the input side one step earlier than data.hip: from the per-bar note matrices ArrangementDataset takes (dataset.py:67-120)
// to the tensors of a batch, on the device.
//
// data.hip starts from rasterised two-bar piano-rolls (4 KB per window, every bar stored twice because windows start at every bar).  Here
// the song bank is the notes themselves: one 4-byte record per note and bar, holding the pitch and the onset / end step of the note for
// both places its bar can take in a window (ptvae_hip.h says how it is packed; the host builder evaluated the reference's int(sb*sde+sq)
// once per song, so only integers arrive).  window_rolls_kernel restates _combine_segments + ext_nmat_to_pr / ext_nmat_to_mel_pr
// (converter.py:35-62) + augment_mel_pr + pr_to_onehot_pr for a batch; detrend_kernel restates detrend_pianotree (dataset.py:123-213).
// Integer / index work, bit-exact against the reference-generated fixture (tests/golden/dataset_path.npz).
// HBM-bound.  window_rolls per sample: reads 4 B per note of the two bars + 16 B of offsets + 448 B of chords; writes 4 KB (pr u8) +
// 12 KB (prs u8) + 16.25 KB (mel f32) + 448 B (chord14) + 4 B (err), the three large ones as 16-byte stores of consecutive lanes to
// consecutive addresses.  detrend per sample: reads 24 KB (x int64, 16-byte loads) + 1.1 KB (c), writes 19.5 KB (dt_x u8, 16-byte stores).
// Where this departs from the reference: a melody note of pitch 128 or 129 is flagged like an accompaniment one (the reference's melody
// roll has 130 columns, so it would write into the two control columns), and negative steps or pitches never get here (the bank builder
// refuses them; numpy would wrap them around).  tests/dataset_ref.py restates the rules as implemented here.
#include "common.hpp"
#include "../../include/ptvae_hip.h"

namespace ptv {

constexpr int WR_CH = 256;        // records of one track staged per pass

// bits [a, b) of a 32-step column, b already clipped to 32; empty when b <= a
__device__ __forceinline__ unsigned step_range(int a, int b) {
  const unsigned long long lo = (1ull << a) - 1ull, hi = (1ull << b) - 1ull;
  return (unsigned)(hi & ~lo);
}

// One workgroup of 256 per sample.  Threads 0..127 own the accompaniment's pitch column p = tid, threads 128..255 the melody's: each
// half stages its own track's records of the bar through LDS in chunks of WR_CH and every lane walks the chunk in order, applying the
// records of its pitch.  The column lives in registers as two 32-bit planes (onset, sustain), i.e. the 2-bit x 32 column split by bit:
// "a later note overwrites an earlier one" is (on | bit) & ~sus_range, (su & ~bit) | sus_range.  The melody's pitch cells are set-only
// and its columns 128 (set over [s+1, e)) and 129 (cleared over [s, e)) are order-free masks every melody lane accumulates.
__global__ __launch_bounds__(256) void window_rolls_kernel(const unsigned* __restrict__ acc_rec, const int* __restrict__ acc_off,
                                                           const unsigned* __restrict__ mel_rec, const int* __restrict__ mel_off,
                                                           const float* __restrict__ chord_bars, int n_bar, const int* __restrict__ first_bar,
                                                           const int* __restrict__ shift, unsigned char* __restrict__ pr,
                                                           unsigned char* __restrict__ prs, float* __restrict__ mel, float* __restrict__ chord14,
                                                           int* __restrict__ err) {
  __shared__ unsigned rec[2][WR_CH];
  __shared__ unsigned on_s[128], su_s[128], ml_s[128];
  __shared__ unsigned ctl[2];       // melody column 128, cleared cells of column 129
  __shared__ int flag[2];
  const int b = blockIdx.x, tid = threadIdx.x, half = tid >> 7, p = tid & 127;
  const int fb = first_bar[b];
  const bool in_range = fb >= 0 && fb + 1 < n_bar;                   // (uniform over the workgroup)
  const int sh = shift ? shift[b] : 0;
  const unsigned* src = half ? mel_rec : acc_rec;
  const int* off = half ? mel_off : acc_off;
  unsigned on = 0, su = 0, c128 = 0, c129 = 0;
  int bad = 0;
  if (in_range) {
    for (int pos = 0; pos < 2; pos++) {
      const int na = acc_off[fb + pos + 1] - acc_off[fb + pos], nm = mel_off[fb + pos + 1] - mel_off[fb + pos];
      const int first = off[fb + pos], mine = half ? nm : na, most = max(na, nm);
      for (int base = 0; base < most; base += WR_CH) {
        for (int i = p; i < WR_CH; i += 128)
          if (base + i < mine) rec[half][i] = src[first + base + i];
        __syncthreads();
        const int n = min(WR_CH, mine - base);
        for (int k = 0; k < n; k++) {
          const unsigned r = rec[half][k];
          const int pit = r & 255, s = (r >> (8 + 12 * pos)) & 63, e = min((int)((r >> (14 + 12 * pos)) & 63), 32);
          if (pit > 127 || s >= 32) { bad = 1; continue; }           // the reference raises IndexError at pr[s_ind, p]
          const unsigned bit = 1u << s, tail = step_range(s + 1, e);
          if (half) {
            c128 |= tail;
            c129 |= step_range(s, e);
            if (pit == p) on |= bit;
          } else if (pit == p) {
            on = (on | bit) & ~tail;
            su = (su & ~bit) | tail;
          }
        }
        __syncthreads();
      }
    }
  }
  if (half) {
    ml_s[p] = on;
    if (p == 0) { ctl[0] = c128; ctl[1] = c129; flag[1] = bad; }
  } else {
    on_s[p] = on;
    su_s[p] = su;
    if (p == 0) flag[0] = bad;
  }
  __syncthreads();
  if (tid == 0) err[b] = flag[0] | flag[1] | (in_range ? 0 : 2);
  if (pr) {                                                          // 256 x 16 bytes: row s = tid / 8, pitches 16 * (tid % 8) ..
    const int s = tid >> 3, p0 = (tid & 7) * 16;
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      unsigned v = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int q = p0 + 4 * j + k;
        v |= (2u * ((on_s[q] >> s) & 1u) + ((su_s[q] >> s) & 1u)) << (8 * k);
      }
      w[j] = v;
    }
    reinterpret_cast<uint4*>(pr + (long)b * 32 * 128)[tid] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (prs) {                                                         // [32][128][3] bytes = 768 x 16; a row is 24 of them
    uint4* dst = reinterpret_cast<uint4*>(prs + (long)b * 32 * 128 * 3);
    for (int i = tid; i < 768; i += 256) {
      const int s = i / 24, r0 = (i - s * 24) * 16;
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int r = r0 + 4 * j + k, q = r / 3, ch = r - 3 * q, from = (q - sh) & 127;     // np.roll(pr, sh)[q] = pr[(q - sh) mod 128]
          const unsigned o = (on_s[from] >> s) & 1u, u = (su_s[from] >> s) & 1u;
          v |= (ch == 0 ? o : ch == 1 ? u : 1u - (o | u)) << (8 * k);
        }
        w[j] = v;
      }
      dst[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  if (mel) {                                                         // [32][130] floats = 1040 x 16 bytes
    float4* dst = reinterpret_cast<float4*>(mel + (long)b * 32 * 130);
    const unsigned m128 = ctl[0], m129 = ctl[1];
    for (int i = tid; i < 1040; i += 256) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int f = 4 * i + j, s = f / 130, col = f - 130 * s;
        const unsigned bit = col < 128 ? (ml_s[(col - sh) & 127] >> s) & 1u : col == 128 ? (m128 >> s) & 1u : 1u - ((m129 >> s) & 1u);
        v[j] = (float)bit;
      }
      dst[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
  if (chord14 && tid < 112)                                          // two consecutive bars of [4,14] are one run of 112 floats
    chord14[(long)b * 112 + tid] = in_range ? chord_bars[(long)fb * 56 + tid] : 0.f;
}

constexpr int DT_W = 39;          // is_note 4 | is_bass 3 | octave 12 | degree 8 | n_state 7 | 5 duration columns

// One workgroup per sample, one thread per (t, j) row.  Root, bass and the 7 chroma-pair states of the 8 beats are worked out once in
// LDS; every row builds its 39 bytes in an LDS tile that leaves as 1248 16-byte stores.
__global__ __launch_bounds__(512) void detrend_kernel(const long* __restrict__ x, const float* __restrict__ c, unsigned char* __restrict__ dt_x) {
  __shared__ int root_s[8], bass_s[8], state_s[8][7];
  __shared__ __attribute__((aligned(16))) unsigned char tile[512 * DT_W];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 8) {
    const float* cc = c + ((long)b * 8 + tid) * 36;
    int ir = 0, ib = 0;
    for (int k = 1; k < 12; k++) {                                   // np.argmax: the first maximum
      if (cc[k] > cc[ir]) ir = k;
      if (cc[24 + k] > cc[24 + ib]) ib = k;
    }
    root_s[tid] = ir;
    bass_s[tid] = ib;
    int ch[12];                                                      // chroma rolled by -root: ch[k] = chroma[(k + root) mod 12]
    for (int k = 0; k < 12; k++) ch[k] = cc[12 + (k + ir) % 12] != 0.f ? 1 : 0;
    const int lo[7] = {0, 1, 3, 5, 7, 8, 10};
    for (int d = 0; d < 7; d++) {
      if (d == 0 || d == 4) state_s[tid][d] = 2 * (1 - ch[lo[d]]);   // the unison and the fifth have one chroma each
      else {
        const int a = ch[lo[d]], h = ch[lo[d] + 1];                  // (1,0) -> 0, (0,1) -> 1, (0,0) -> 2, (1,1) -> 3
        state_s[tid][d] = a ? (h ? 3 : 0) : (h ? 1 : 2);
      }
    }
  }
  const long2* row = reinterpret_cast<const long2*>(x + ((long)b * 512 + tid) * 6);
  const long2 v0 = row[0], v1 = row[1], v2 = row[2];
  __syncthreads();
  const int t = tid >> 4, j = tid & 15, beat = t >> 2;
  const long pitch = v0.x;
  int is_note = -1, is_bass = -1, octave = -1, deg = -1, n_state = -1;       // (-1: no cell set; pitches the reference cannot take)
  if (pitch >= 128 && pitch <= 130) {
    is_note = (int)pitch - 127; is_bass = 2; octave = 11; deg = 7; n_state = 6;
  } else if (pitch >= 0 && pitch < 144) {
    const int pi = (int)pitch, degree = ((pi - root_s[beat]) % 12 + 12) % 12;
    const int deg_table[12] = {0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 6};
    const int semi_table[12] = {0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1};
    is_note = 0;
    is_bass = bass_s[beat] == degree ? 1 : 0;
    octave = pi / 12;
    deg = deg_table[degree];
    const int cs = state_s[beat][deg], semi = semi_table[deg];       // (the reference indexes semi_table by the scale degree)
    n_state = cs == 0 ? (semi ? 0 : 1) : cs == 1 ? (semi ? 1 : 0) : cs == 2 ? semi + 2 : semi + 4;
  }
  if (is_note >= 0 && !((t & 3) == 0 && j == 0)) is_bass = 0;        // has_bass: only the first row of a beat keeps its own class
  unsigned char* q = tile + tid * DT_W;
#pragma unroll
  for (int k = 0; k < 34; k++) q[k] = 0;
  if (is_note >= 0) { q[is_note] = 1; q[4 + is_bass] = 1; q[7 + octave] = 1; q[19 + deg] = 1; q[27 + n_state] = 1; }
  q[34] = (unsigned char)v0.y; q[35] = (unsigned char)v1.x; q[36] = (unsigned char)v1.y; q[37] = (unsigned char)v2.x; q[38] = (unsigned char)v2.y;
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(dt_x + (long)b * 512 * DT_W);
  const uint4* tl = reinterpret_cast<const uint4*>(tile);
  for (int i = tid; i < 512 * DT_W / 16; i += 512) dst[i] = tl[i];
}

}  // namespace ptv

extern "C" int ptv_window_rolls(const unsigned* acc_rec, const int* acc_off, const unsigned* mel_rec, const int* mel_off, const float* chord_bars,
                                int n_bar, const int* first_bar, const int* shift, int B, unsigned char* pr, unsigned char* prs, float* mel,
                                float* chord14, int* err, void* stream) {
  if (!acc_rec || !acc_off || !mel_rec || !mel_off || !chord_bars || !first_bar || !err || n_bar < 2 || B <= 0) return PTV_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(pr) | reinterpret_cast<uintptr_t>(prs) | reinterpret_cast<uintptr_t>(mel)) & 15) return PTV_ERR_ARG;
  hipLaunchKernelGGL(ptv::window_rolls_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, acc_rec, acc_off, mel_rec, mel_off, chord_bars, n_bar,
                     first_bar, shift, pr, prs, mel, chord14, err);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_detrend_pianotree(const long* x, const float* c, unsigned char* dt_x, int B, void* stream) {
  if (!x || !c || !dt_x || B <= 0) return PTV_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dt_x)) & 15) return PTV_ERR_ARG;
  hipLaunchKernelGGL(ptv::detrend_kernel, dim3(B), dim3(512), 0, (hipStream_t)stream, x, c, dt_x);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
