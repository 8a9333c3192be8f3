// The instance table of ppo_rc_kernel<KT, KW, KB, S0T, NLT, ACTT, HWT, CWT, DT, NW, LEAN>
// (ppo_rc_kernel.h): one row X(name, ns, <the eleven template arguments>) per compiled instance.
// ns = 1: a net-split build (one net per workgroup), 0: both nets per workgroup.
// LEAN = 1 (names *_lean): the build for one row group (G == 1) without cycle counters -- the
// partial exchange, the stash and every a.prof stamp are compiled out, which takes the
// HalfCheetah instance from 571 to 64 SGPR spills. A lean row stands directly BEFORE its full
// twin (same other constants); rc_select passes over lean rows unless the plan has G == 1, no
// prof counters and PPOArgs::rc_lean != 0, so plans with G > 1 and the probe tools (which read
// the counters) run the full twin, and both compute bit-identical updates.
// Everything that has to agree with an instance's compile-time constants is generated from its
// row: the explicit instantiation (IA_RC_GROUP_<g> in ppo_rc_inst_<g>.hip; the groups build in
// parallel), and in ppo_rc.hip the extern declaration and the host row (kRcRows) that the plan
// selects (rc_select: the FIRST row whose constants match the run-time shape), takes its slot
// caps / waves / weight-image format from, and launches. To add an instance, add a row.
// Each group's rows are listed by selection tier -- EXACT (one shape), FAMILY (any 3-layer
// [64, 64] net up to an obs dim bound), GENERIC (run-time shape) -- and IA_RC_TABLE orders the
// tiers: an exact build wins over the family that also covers its shape, the obs dim <= 16
// families over the <= 32 ones, and the generic builds take what is left.
// Scratch budget of every instance: profiles/ppo_barrier_path.md (all 0; before the lean rows:
// profiles/r4_kernel_resources.md).
#pragma once

#define IA_RC_EXACT_A(X) \
  X(ns_cheetah32_lean, 1, 2,3,1,5,3,2,32,64,0,4,1) \
  X(ns_cheetah32, 1, 2,3,1,5,3,2,32,64,0,4,0)  /* HalfCheetah / Walker2d FeedForward32Policy (tanh) */ \
  X(ns_cartpole32_lean, 1, 2,2,1,1,3,2,32,64,1,4,1) \
  X(ns_cartpole32, 1, 2,2,1,1,3,2,32,64,1,4,0) /* CartPole FeedForward32Policy */
// <= 32-wide nets of any shape, 4 waves: net split (one net's items: up to 20 weight tiles and
// 8 vectors), and both nets per workgroup at one wave per SIMD (<= 32-row chunks; 20 weight
// tiles cover 3-layer nets with obs dim <= 32). The 8-wave both-nets build and every 64-wide
// generic build need scratch and are not compiled: such shapes take the LDS kernel (ppo.hip)
#define IA_RC_GENERIC_A(X) \
  X(ns_generic32, 1, 2,5,2,0,0,-1,0,64,-1,4,0) \
  X(narrow32, 0, 2,5,2,0,0,-1,0,0,-1,4,0)
#define IA_RC_GROUP_A(X) IA_RC_EXACT_A(X) IA_RC_GENERIC_A(X)

#define IA_RC_EXACT_B(X) \
  X(ns_hopper64r_lean, 1, 4,6,1,3,3,1,64,64,0,4,1) \
  X(ns_hopper64r, 1, 4,6,1,3,3,1,64,64,0,4,0)  /* Hopper MlpPolicy [64, 64] ReLU (AIRL config) */ \
  X(ns_walker64r_lean, 1, 4,7,1,5,3,1,64,64,0,4,1) \
  X(ns_walker64r, 1, 4,7,1,5,3,1,64,64,0,4,0)  /* Walker2d MlpPolicy [64, 64] ReLU (DRLHP config) */ \
  X(cheetah32_cw64, 0, 2,3,1,5,3,2,32,64,0,8,0) \
  X(cheetah32_cw32, 0, 2,3,1,5,3,2,32,32,0,8,0) \
  X(cartpole32_cw64, 0, 2,2,1,1,3,2,32,64,1,8,0)
#define IA_RC_GROUP_B(X) IA_RC_EXACT_B(X)

// any 3-layer [64, 64] net, obs dim <= 16 (SB3 MlpPolicy default: CartPole, Hopper, ...)
#define IA_RC_FAMILY_C(X) \
  X(ns_64_d16_relu_gauss, 1, 4,6,1,-4,3,1,64,64,0,4,0) \
  X(ns_64_d16_relu_cat, 1, 4,6,1,-4,3,1,64,64,1,4,0) \
  X(ns_64_d16_tanh_gauss, 1, 4,6,1,-4,3,2,64,64,0,4,0) \
  X(ns_64_d16_tanh_cat, 1, 4,6,1,-4,3,2,64,64,1,4,0)
#define IA_RC_GROUP_C(X) IA_RC_FAMILY_C(X)

// the same, obs dim <= 32 (HalfCheetah / Walker2d / Ant, ...)
#define IA_RC_FAMILY_D(X) \
  X(ns_64_d32_relu_gauss, 1, 4,7,1,-8,3,1,64,64,0,4,0) \
  X(ns_64_d32_relu_cat, 1, 4,7,1,-8,3,1,64,64,1,4,0) \
  X(ns_64_d32_tanh_gauss, 1, 4,7,1,-8,3,2,64,64,0,4,0) \
  X(ns_64_d32_tanh_cat, 1, 4,7,1,-8,3,2,64,64,1,4,0)
#define IA_RC_GROUP_D(X) IA_RC_FAMILY_D(X)

#define IA_RC_EXACT_E(X) \
  X(hopper64r_cw32, 0, 4,12,2,3,3,1,64,32,0,4,0)
#define IA_RC_FAMILY_E(X) \
  X(both_64_d16_relu_gauss, 0, 4,12,2,-4,3,1,64,32,0,4,0) \
  X(both_64_d16_relu_cat, 0, 4,12,2,-4,3,1,64,32,1,4,0) \
  X(both_64_d16_tanh_gauss, 0, 4,12,2,-4,3,2,64,32,0,4,0) \
  X(both_64_d16_tanh_cat, 0, 4,12,2,-4,3,2,64,32,1,4,0)
#define IA_RC_GROUP_E(X) IA_RC_EXACT_E(X) IA_RC_FAMILY_E(X)

#define IA_RC_EXACT_F(X) \
  X(walker64r_cw32, 0, 4,14,2,5,3,1,64,32,0,4,0)
// (ReLU + Gaussian head only: the Tanh and categorical builds of this size need scratch)
#define IA_RC_FAMILY_F(X) \
  X(both_64_d32_relu_gauss, 0, 4,14,2,-8,3,1,64,32,0,4,0)
#define IA_RC_GROUP_F(X) IA_RC_EXACT_F(X) IA_RC_FAMILY_F(X)

#define IA_RC_TABLE(X) \
  IA_RC_EXACT_A(X) IA_RC_EXACT_B(X) IA_RC_EXACT_E(X) IA_RC_EXACT_F(X) \
  IA_RC_FAMILY_C(X) IA_RC_FAMILY_D(X) IA_RC_FAMILY_E(X) IA_RC_FAMILY_F(X) \
  IA_RC_GENERIC_A(X)

#define IA_RC_INSTANTIATE(name, ns, ...) template __global__ void ppo_rc_kernel<__VA_ARGS__>(PPOArgs, PPORcGeo);
#define IA_RC_EXTERN(name, ns, ...) extern template __global__ void ppo_rc_kernel<__VA_ARGS__>(PPOArgs, PPORcGeo);
// initialiser of a {name, ns, KT, KW, KB, S0T, NLT, ACTT, HWT, CWT, DT, NW, LEAN, kernel} host row
#define IA_RC_ROW(name, ns, ...) {#name, ns, __VA_ARGS__, ppo_rc_kernel<__VA_ARGS__>},
