// Reward-net input columns read straight from the transition sources (disc.hip, airl_disc.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "launchers.h"

namespace ia {

// Value of column c of the reward-net input for source row src of the expert / generator set.
// The side is chosen on the loaded pointers: an array of sources indexed at run time would put
// the kernel arguments in scratch.
__device__ __forceinline__ float reward_input_col(const RewardInputLayout& in, const TransitionSrc& e, const TransitionSrc& g,
                                                  bool expert, int64_t src, int c) {
  const int D = in.D, aw = in.aw;
  if (in.use_state) {
    if (c < D) return (expert ? e.obs : g.obs)[src * D + c];
    c -= D;
  }
  if (in.use_action) {
    if (c < aw) {
      if (in.act_discrete) return (int)(expert ? e.acts_i : g.acts_i)[src] == c ? 1.f : 0.f;
      return (expert ? e.acts : g.acts)[src * aw + c];
    }
    c -= aw;
  }
  if (in.use_next_state) {
    if (c < D) return (expert ? e.next_obs : g.next_obs)[src * D + c];
    c -= D;
  }
  return (expert ? e.dones : g.dones)[src] ? 1.f : 0.f;
}

}  // namespace ia
