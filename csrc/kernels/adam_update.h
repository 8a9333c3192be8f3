// The per-element Adam / AdamW update and its bias corrections, shared by every kernel that
// steps a FusedAdam bucket (optim.hip's adam_flat, the in-launch steps of dqn_td.hip, bc_mlp.hip
// and sac_update.hip): one body, so the kernels produce the same bits from the same state.
#pragma once
#include <hip/hip_runtime.h>

#include "launchers.h"

namespace ia {

// bias corrections of step t0 (the already incremented step count): out[0] = t0,
// out[1] = sqrt(1 - beta2^t0), out[2] = lr / (1 - beta1^t0)
__device__ __forceinline__ void adam_bias(const AdamArgs& a, float t0, float* out) {
  out[0] = t0;
  out[1] = sqrtf(1.f - powf(a.beta2, t0));
  out[2] = a.lr / (1.f - powf(a.beta1, t0));
}

// FMA contraction off, the fused multiply-adds spelled out: the float4 path, the scalar tail and the
// folded-reduction blocks (one element per thread) then compute bitwise the same update (with
// contraction left to the compiler, the packed float4 code formed other FMAs than the scalar code).
__device__ __forceinline__ void adam_one(float& p, float& g, float& m, float& v, const AdamArgs& a, float step_size,
                                         float bc2_sqrt) {
#pragma clang fp contract(off)
  float gr = a.maximize ? -g : g;
  if (a.weight_decay != 0.f) {
    if (a.decoupled) p *= 1.f - a.lr * a.weight_decay;
    else gr = __builtin_fmaf(a.weight_decay, p, gr);
  }
  m = __builtin_fmaf(1.f - a.beta1, gr - m, m);
  v = __builtin_fmaf(v, a.beta2, ((1.f - a.beta2) * gr) * gr);
  const float denom = sqrtf(v) / bc2_sqrt + a.eps;
  p = __builtin_fmaf(-step_size, m / denom, p);
  if (a.zero_grad) g = 0.f;
}

}  // namespace ia
