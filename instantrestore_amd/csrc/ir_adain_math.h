// ir_adain_math.h - the two fp32 expressions every AdaIN statistics kernel shares (adain.hip, adain_weighted.hip): the scale of
// the affine and Chan's merge of (n, mean, M2) partials.  One definition, so the weighted and the unweighted kernels round alike.
#pragma once
#include <hip/hip_runtime.h>

// a = (sigma_v + eps) / (sigma_x + eps) (attn_processors.py:10,16,245) - except where the content std is EXACTLY 0 (M2 == 0:
// every token of the reference channel holds one value; a zero-filled reference, pix2pix_turbo.py:269-273, or a short token
// axis whose values round to the same 16-bit number).  There x - mean(x) is exactly 0 and the reference's adain() returns the
// style mean whatever the ratio, while the affine form a*x + b with a = sigma_v / 1e-5 ~ 1e5 has to cancel a*x against
// -a*mean(x) in fp32 (round-4 soak): the fused result lost the style mean.  Any small ratio gives the same
// function on such a channel; the ideal is a = 0 (what oracle.adain_affine_np reports), but the 64-row attention kernel's
// ratio frame divides by a, so the kernels emit a = 2^-24 (sigma_v + eps): b = mean(V_self) - mean(x) * a then differs from
// the style mean by < 6e-8 |x| sigma_v, and a*x + b from it by the fp32 rounding of that.
__device__ __forceinline__ float adain_scale(float sd_v_eps, float sd_x_eps, bool content_is_constant) {
  return content_is_constant ? sd_v_eps * 5.9604644775390625e-8f : sd_v_eps / sd_x_eps;
}

// Chan et al. merge of (n, mean, M2) partials.
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float meanb, float m2b) {
  if (nb == 0.f) return;
  const float nt = n + nb;
  const float delta = meanb - mean;
  const float f = nb / nt;
  mean = mean + delta * f;
  m2 = m2 + m2b + delta * delta * n * f;
  n = nt;
}
