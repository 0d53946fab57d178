// loss_fused.hpp -- the loss node in one launch per direction (kernels and launchers in loss.hip, called by composite.hip's
// ptv_vae_loss_fwd / ptv_vae_loss_bwd).
#pragma once
#include "common.hpp"

namespace ptv {

constexpr int VL_TERMS = 7;            // pitch CE, duration CE, kl_chd, kl_rhy, root CE, chroma CE, bass CE: the order of sums[]
constexpr int VL_FAN = 16;             // arrival words per big term (ordered_commit's two-level count), from counter VL_SUB0 on
constexpr int VL_SUB0 = 64;
constexpr int VL_REC_WORDS = 16;       // record of a forward that wrote the gradients: [0..10] the upstream vector it assumed (bits),
                                       // [11] the beta it used (bits), [12] 1 = valid; the rest unused

struct VlArgs {
  const float *pitch, *dur, *mu_c, *sd_c, *mu_r, *sd_r, *root, *chroma, *bass;      // logits / posteriors in memory order
  const float* c;                      // [B,8,36]: the chord targets' source (forward only)
  const int *pitch_t, *dur_t, *counts;
  int *root_t, *chroma_t, *bass_t;     // written by the forward's chord terms, read by the backward
  float *sums, *out;                   // forward: [8] zeroed, [11]
  const float* gout;                   // backward: [11]
  float *dpitch, *ddur, *dmu_c, *dsd_c, *dmu_r, *dsd_r, *droot, *dchroma, *dbass;   // null in a forward without gradients
  unsigned* rec;                       // [VL_REC_WORDS] or null
  unsigned* early;                     // backward: counts the launches that returned on a matching record
  const float* sp;                     // ptv_step_params array or null: sp[0] overrides beta
  OrdScratch sc;
  long rows, ldp, nz;                  // 480 B, pitch row stride, B * Z
  int B, NP, sm_c, pitch_vec;
  float beta, w0, w1, n_kl, n_root, n_chroma;
  int start[VL_TERMS + 1];             // block ranges of the seven terms: term k owns blocks start[k] .. start[k + 1] - 1
};

// -> PTV_ERR_UNSUPPORTED when the launch sequence has to run instead (no ordered-reduction workspace, a shape outside the fused kernel's):
// nothing was launched then.  With a.dpitch the forward also writes the nine gradients for the upstream (1, 0, ..., 0) and the record.
int vae_loss_fused_fwd(VlArgs a, hipStream_t s);
int vae_loss_fused_bwd(VlArgs a, hipStream_t s);

}  // namespace ptv
