// rng.hip -- sharding-invariant reparameterisation noise (SURVEY.md section 8 d/e).
//
// The reference draws eps for Normal.rsample (train_utils.py:33-34) from torch's global generator: the value a sample gets
// depends on its position in the batch and on how the batch is split over processes.  Here eps[row, j] is a pure function of
// (seed, stream, GLOBAL sample index, j): Philox4x32-10 keyed by the seed, counter = (global row, j / 4, stream lo, stream hi),
// four 32-bit words -> two Box-Muller pairs.  One batch on one GPU and the same batch split over N ranks (row_offset =
// rank * B_local) see identical noise; `stream` separates draws (training step x {chd, rhy}).
#include "common.hpp"
#include "philox.hpp"
#include "../../include/ptvae_hip.h"
#include "../../include/ptvae_hip_debug.h"

namespace ptv {

__global__ void philox_normal_kernel(float* __restrict__ out, long rows, int Z, unsigned long long seed, unsigned long long stream,
                                     long row_offset) {
  const int q4 = (Z + 3) >> 2;
  const long n = rows * q4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / q4; const int q = (int)(i - r * q4);
    const unsigned long long g = (unsigned long long)(row_offset + r);
    // counter = (row lo, row hi * 2^16 + column quad, stream lo, stream hi): rows < 2^48, quads < 2^16
    unsigned c[4] = {(unsigned)g, (unsigned)(g >> 32) * 0x10000u + (unsigned)q, (unsigned)stream, (unsigned)(stream >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    float v[4];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const float u1 = ((float)c[2 * h] + 0.5f) * 2.3283064365386963e-10f;        // (0, 1]: 2^-32 * (x + 1/2), rounded
      const float u2 = ((float)c[2 * h + 1] + 0.5f) * 2.3283064365386963e-10f;
      const float rad = sqrtf(-2.0f * logf(fminf(fmaxf(u1, 1.1754944e-38f), 1.0f)));
      const float th = 6.283185307179586f * u2;
      v[2 * h] = rad * cosf(th); v[2 * h + 1] = rad * sinf(th);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) if (q * 4 + e < Z) out[r * Z + q * 4 + e] = v[e];
  }
}

// the Gumbel values the sampling decoder uses for rows [0, rows) at (t, n), through the decoder's own device functions (philox.hpp)
__global__ void sample_noise_kernel(const SampleBlock* __restrict__ blk, long rows, int t, int n, float* __restrict__ out_pitch,
                                    float* __restrict__ out_dur) {
  const SampleBlock sb = *blk;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows * 16; i += (long)gridDim.x * blockDim.x) {
    const long r = i >> 4; const int j = (int)(i & 15);
    float g[9];
    pitch_gumbel9(sb, sb.sample_offset + r, t, n, j, g);
#pragma unroll
    for (int k = 0; k < 9; k++) if (j + 16 * k < 130) out_pitch[r * 130 + j + 16 * k] = g[k];
    if (j == 0) {
      float d[10];
      dur_gumbel10(sb, sb.sample_offset + r, t, n, d);
#pragma unroll
      for (int q = 0; q < 10; q++) out_dur[r * 10 + q] = d[q];
    }
  }
}

// test aid: pitch_keep_threshold() on caller-supplied rows in the two lane layouts of the decision sites.  LAYOUT 0: 16 lanes per row, lane j
// owns columns j + 16 i (the note loops); LAYOUT 1: a wave per row, lane l owns columns l + 64 i (the step loop).  Every lane of a wave
// stays in the loop (rows past the end are clamped and store nothing): the row reductions want whole rows of lanes.
template <int LAYOUT>
__global__ void pitch_keep_kernel(const SampleBlockT* __restrict__ blk, const float* __restrict__ logits, long rows,
                                  unsigned char* __restrict__ keep_out, float* __restrict__ thr_out) {
  constexpr int W = LAYOUT ? 64 : 16, NV = LAYOUT ? 3 : 9;
  const Trunc tr = load_trunc(blk);
  const float T = blk->s.t_pitch;
  const long per = blockDim.x / W, total = (rows + per - 1) / per * per;
  for (long r_ = (long)blockIdx.x * per + threadIdx.x / W; r_ < total; r_ += (long)gridDim.x * per) {
    const bool ok = r_ < rows;
    const long r = ok ? r_ : rows - 1;
    const int j = threadIdx.x % W;
    float v[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = j + W * i < 130 ? logits[r * 130 + j + W * i] : -INFINITY;
    const float thr = pitch_keep_threshold<NV, W>(tr, T, v);
    if (ok) {
#pragma unroll
      for (int i = 0; i < NV; i++) if (j + W * i < 130) keep_out[r * 130 + j + W * i] = v[i] >= thr ? 1 : 0;
      if (j == 0) thr_out[r] = thr;
    }
  }
}

// test aid: pitch_constrain() followed by pitch_keep_threshold() on caller-supplied rows, masks [rows, 4] and lo [rows], in the same two
// layouts; the block's flags are read, its mask address is not (the caller's rows are the masks)
template <int LAYOUT>
__global__ void pitch_constrain_kernel(const SampleBlockC* __restrict__ blk, const float* __restrict__ logits, const int* __restrict__ masks,
                                       const int* __restrict__ lo, const int* __restrict__ words, long rows,
                                       unsigned char* __restrict__ keep_out, float* __restrict__ thr_out) {
  constexpr int W = LAYOUT ? 64 : 16, NV = LAYOUT ? 3 : 9;
  const Trunc tr = load_trunc(&blk->s);
  const float T = blk->s.s.t_pitch;
  const unsigned flags = blk->flags;
  const long per = blockDim.x / W, total = (rows + per - 1) / per * per;
  for (long r_ = (long)blockIdx.x * per + threadIdx.x / W; r_ < total; r_ += (long)gridDim.x * per) {
    const bool ok = r_ < rows;
    const long r = ok ? r_ : rows - 1;
    const int j = threadIdx.x % W;
    float v[NV], tv[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = j + W * i < 130 ? logits[r * 130 + j + W * i] : -INFINITY;
    unsigned mw[4];
#pragma unroll
    for (int i = 0; i < 4; i++) mw[i] = (unsigned)masks[r * 4 + i];
    const int word = words ? words[r] : -1;                        // (words: the force word of each row, NULL = every decision plainly free)
    const unsigned al = pitch_constrain<NV, W>(v, mw, lo[r], flags, j, tv, word);
    const float thr = pitch_keep_threshold<NV, W>(tr, T, tv);
    if (ok) {
#pragma unroll
      for (int i = 0; i < NV; i++) if (j + W * i < 130) keep_out[r * 130 + j + W * i] = ((al >> i) & 1u) && v[i] >= thr ? 1 : 0;
      if (j == 0) thr_out[r] = thr;
    }
  }
}

// test aid: the kernel above with a row table (philox.hpp SampleBlockR) in place of the block's scalars -- row r is judged by record r.  In
// LAYOUT 0 the four rows of a wave hold four records: pitch_keep_threshold()'s branches diverge between them.  Of the block only the
// flags are read; a clamped row takes the last row's record
template <int LAYOUT>
__global__ void pitch_constrain_rows_kernel(const SampleBlockC* __restrict__ blk, const int* __restrict__ table, const float* __restrict__ logits,
                                            const int* __restrict__ masks, const int* __restrict__ lo, const int* __restrict__ words, long rows,
                                            unsigned char* __restrict__ keep_out, float* __restrict__ thr_out) {
  constexpr int W = LAYOUT ? 64 : 16, NV = LAYOUT ? 3 : 9;
  const unsigned flags = blk->flags;
  const long per = blockDim.x / W, total = (rows + per - 1) / per * per;
  for (long r_ = (long)blockIdx.x * per + threadIdx.x / W; r_ < total; r_ += (long)gridDim.x * per) {
    const bool ok = r_ < rows;
    const long r = ok ? r_ : rows - 1;
    const int j = threadIdx.x % W;
    const RowRule rw = load_row_rule(table, r);
    float v[NV], tv[NV];
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = j + W * i < 130 ? logits[r * 130 + j + W * i] : -INFINITY;
    unsigned mw[4];
#pragma unroll
    for (int i = 0; i < 4; i++) mw[i] = (unsigned)masks[r * 4 + i];
    const int word = words ? words[r] : -1;
    const unsigned al = pitch_constrain<NV, W>(v, mw, lo[r], flags, j, tv, word);
    const float thr = pitch_keep_threshold<NV, W>(rw.tr, rw.t_pitch, tv);
    if (ok) {
#pragma unroll
      for (int i = 0; i < NV; i++) if (j + W * i < 130) keep_out[r * 130 + j + W * i] = ((al >> i) & 1u) && v[i] >= thr ? 1 : 0;
      if (j == 0) thr_out[r] = thr;
    }
  }
}

}  // namespace ptv

extern "C" int ptv_debug_pitch_constrain_rows(const void* block64, const int* table, const float* logits, const int* masks, const int* lo,
                                              const int* words, long rows, int layout, unsigned char* keep_out, float* thr_out, void* stream) {
  if (!block64 || !table || !logits || !masks || !lo || !keep_out || !thr_out || rows <= 0 || (layout != 0 && layout != 1)) return PTV_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(table) & 15) return PTV_ERR_ARG;
  long nb = (rows + 3) / 4; if (nb > 4096) nb = 4096;
  if (layout == 0)
    hipLaunchKernelGGL(ptv::pitch_constrain_rows_kernel<0>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const ptv::SampleBlockC*)block64, table,
                       logits, masks, lo, words, rows, keep_out, thr_out);
  else
    hipLaunchKernelGGL(ptv::pitch_constrain_rows_kernel<1>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const ptv::SampleBlockC*)block64, table,
                       logits, masks, lo, words, rows, keep_out, thr_out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

static int debug_pitch_constrain(const void* block64, const float* logits, const int* masks, const int* lo, const int* words, long rows,
                                 int layout, unsigned char* keep_out, float* thr_out, void* stream) {
  if (!block64 || !logits || !masks || !lo || !keep_out || !thr_out || rows <= 0 || (layout != 0 && layout != 1)) return PTV_ERR_ARG;
  long nb = (rows + 3) / 4; if (nb > 4096) nb = 4096;
  if (layout == 0)
    hipLaunchKernelGGL(ptv::pitch_constrain_kernel<0>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const ptv::SampleBlockC*)block64, logits,
                       masks, lo, words, rows, keep_out, thr_out);
  else
    hipLaunchKernelGGL(ptv::pitch_constrain_kernel<1>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const ptv::SampleBlockC*)block64, logits,
                       masks, lo, words, rows, keep_out, thr_out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_debug_pitch_constrain(const void* block64, const float* logits, const int* masks, const int* lo, long rows, int layout,
                                         unsigned char* keep_out, float* thr_out, void* stream) {
  return debug_pitch_constrain(block64, logits, masks, lo, nullptr, rows, layout, keep_out, thr_out, stream);
}

extern "C" int ptv_debug_pitch_constrain_words(const void* block64, const float* logits, const int* masks, const int* lo, const int* words,
                                               long rows, int layout, unsigned char* keep_out, float* thr_out, void* stream) {
  if (!words) return PTV_ERR_ARG;
  return debug_pitch_constrain(block64, logits, masks, lo, words, rows, layout, keep_out, thr_out, stream);
}

extern "C" int ptv_debug_pitch_keep(const void* block48, const float* logits, long rows, int layout, unsigned char* keep_out, float* thr_out,
                                    void* stream) {
  if (!block48 || !logits || !keep_out || !thr_out || rows <= 0 || (layout != 0 && layout != 1)) return PTV_ERR_ARG;
  long nb = (rows + 3) / 4; if (nb > 4096) nb = 4096;
  if (layout == 0)
    hipLaunchKernelGGL(ptv::pitch_keep_kernel<0>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const ptv::SampleBlockT*)block48, logits, rows,
                       keep_out, thr_out);
  else
    hipLaunchKernelGGL(ptv::pitch_keep_kernel<1>, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const ptv::SampleBlockT*)block48, logits, rows,
                       keep_out, thr_out);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_philox_normal(float* out, long rows, int Z, unsigned long long seed, unsigned long long stream_id, long row_offset,
                                 void* stream) {
  if (!out || rows <= 0 || Z <= 0 || Z > 4 * 65536 || row_offset < 0) return PTV_ERR_ARG;
  long nb = (rows * ((Z + 3) / 4) + 255) / 256; if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(ptv::philox_normal_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, out, rows, Z, seed, stream_id, row_offset);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}

extern "C" int ptv_debug_sample_noise(const void* block, long rows, int t, int n, float* out_pitch, float* out_dur, void* stream) {
  if (!block || !out_pitch || !out_dur || rows <= 0 || t < 0 || t >= 32 || n < 0 || n >= 15) return PTV_ERR_ARG;
  long nb = (rows * 16 + 255) / 256; if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(ptv::sample_noise_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const ptv::SampleBlock*)block, rows, t, n, out_pitch,
                     out_dur);
  PTV_CHECK_LAUNCH();
  return PTV_OK;
}
