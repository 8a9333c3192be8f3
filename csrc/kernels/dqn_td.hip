// Fused DQN TD update (imitation_amd/ops/dqn.py, rl/dqn.py): ALL gradient steps of one
// DQN.train call in ONE launch of ONE workgroup.
//
// The eager step (two replay samples, five cats, target forward + max, online forward + gather,
// smooth_l1_loss, autograd backward, clip_grad_norm_, foreach Adam) is several dozen launches to
// update the ~4.7K parameters of a [64, 64] Q-network on 32 rows. Here a step gathers its rows
// by flat row id from the agent ring (source 0) and SQIL's expert ring (source 1), evaluates the
// target network from its flat bucket, runs the online forward, the Huber loss, the backward
// through the three linear layers, the global-norm clip and the Adam update of the online
// FusedAdam bucket (adam_update.h: the body adam_flat runs), and goes on to the next step.
//
// Everything is fp32 FMAs (the TD target feeds back into itself: no bf16 operands). The
// summation order is fixed, so equal states give equal bits: rows go through in chunks of 64
// with the chunk's activations in LDS; every weight element is owned by one thread, which sums
// its dW over the rows in row order in a register and applies Adam from that register; the loss
// and |g|^2 go through a fixed tree. One workgroup, __syncthreads only: nothing here waits on
// another workgroup.
#include <hip/hip_runtime.h>

#include "adam_update.h"
#include "launchers.h"
#include "mlp_chunk.h"

namespace ia {
namespace {

using namespace chunk;  // kT, kR, kS, kWS, stage, layer, wgrad (mlp_chunk.h)

// the clipped gradient of element idx, its slot in the gradient bucket (last step) and its Adam update
__device__ __forceinline__ void clip_adam(const AdamArgs& a, int idx, float g, float coef, bool store_grad, float step_size,
                                          float bc2_sqrt) {
#pragma clang fp contract(off)
  float gc = g * coef;
  if (store_grad) a.grads[idx] = gc;
  float p = a.params[idx], m = a.exp_avg[idx], v = a.exp_avg_sq[idx];
  adam_one(p, gc, m, v, a, step_size, bc2_sqrt);
  a.params[idx] = p;
  a.exp_avg[idx] = m;
  a.exp_avg_sq[idx] = v;
}

// the same for four adjacent elements at a 16-B aligned slot (the same bits, a quarter of the accesses)
__device__ __forceinline__ void clip_adam4(const AdamArgs& a, int idx, float g0, float g1, float g2, float g3, float coef,
                                           bool store_grad, float step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
  float4 gc = make_float4(g0 * coef, g1 * coef, g2 * coef, g3 * coef);
  if (store_grad) *reinterpret_cast<float4*>(a.grads + idx) = gc;
  float4 p = *reinterpret_cast<const float4*>(a.params + idx);
  float4 m = *reinterpret_cast<const float4*>(a.exp_avg + idx);
  float4 v = *reinterpret_cast<const float4*>(a.exp_avg_sq + idx);
  adam_one(p.x, gc.x, m.x, v.x, a, step_size, bc2_sqrt);
  adam_one(p.y, gc.y, m.y, v.y, a, step_size, bc2_sqrt);
  adam_one(p.z, gc.z, m.z, v.z, a, step_size, bc2_sqrt);
  adam_one(p.w, gc.w, m.w, v.w, a, step_size, bc2_sqrt);
  *reinterpret_cast<float4*>(a.params + idx) = p;
  *reinterpret_cast<float4*>(a.exp_avg + idx) = m;
  *reinterpret_cast<float4*>(a.exp_avg_sq + idx) = v;
}

// VEC: every weight slot of both buckets is made of whole 16-B aligned quads (the launcher's check)
template <bool VEC>
__global__ __launch_bounds__(kT) void dqn_td_kernel(DqnTdArgs a) {
  __shared__ __attribute__((aligned(16))) float sX[kR * kS], sH1[kR * kS], sH2[kR * kS], sQ[kR * kS], sD2[kR * kS],
      sD1[kR * kS];
  __shared__ float sW[64 * kWS];
  __shared__ long long sRow[kR];
  __shared__ int sSrc[kR], sAct[kR];
  __shared__ float sRew[kR], sDone[kR], sY[kR], sDq[kR];
  __shared__ float sLoss[kT], sSq[kT], sBc[3];
  __shared__ DqnTdSrc sDesc[2];  // the ring descriptors: read per lane from here, not held in 28 scalar registers

  const int D = a.D, H1 = a.H1, H2 = a.H2, A = a.A;
  const int B = a.n_a + a.n_e;
  const float invB = 1.f / (float)B;
  // the layers as [N][K] and their slots in the flat buckets
  const int N[3] = {H1, H2, A}, K[3] = {D, H1, H2};
  // (plain Adam: the weight-decay, maximize and zero-grad branches of adam_one fold away)
  AdamArgs ad{};
  ad.params = a.params;
  ad.grads = a.grads;
  ad.exp_avg = a.exp_avg;
  ad.exp_avg_sq = a.exp_avg_sq;
  ad.lr = a.lr;
  ad.beta1 = a.beta1;
  ad.beta2 = a.beta2;
  ad.eps = a.eps;
  const float* P = a.params;
  const float* T = a.target;
  float t = *a.step;
  if (threadIdx.x == 0) {
    sDesc[0] = a.src[0];
    sDesc[1] = a.src[1];
  }
  __syncthreads();

  for (int g = 0; g < a.G; ++g) {
    t += 1.f;
    if (threadIdx.x == 0) adam_bias(ad, t, sBc);
    // this thread's gradient sums: W_l[tid / 4][16 * (tid % 4) .. + 16) of each layer l and, for
    // tid < 192, b_(tid / 64)[tid % 64]
    float aW[3][16];
    float aB = 0.f;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int i = 0; i < 16; ++i) aW[l][i] = 0.f;
    sLoss[threadIdx.x] = 0.f;

    for (int c0 = 0; c0 < B; c0 += kR) {
      const int nr = min(kR, B - c0);
      // (the thread id goes through an opaque copy per chunk, and once more for the Adam phase: the
      // few hundred lane masks and element addresses derived from it are then formed where they
      // are used instead of being hoisted and kept live, in more registers than there are,
      // across both loops)
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      const int bl = tid >> 6, bj = tid & 63;
      const bool own_b = bl < 3 && bj < (bl == 0 ? H1 : (bl == 1 ? H2 : A));
      // the chunk's rows: source, flat row id (clamped into the ring), action, reward, effective done
      if (tid < kR) {
        long long row = 0;
        int src = 0, act = 0;
        float rew = 0.f, dn = 0.f;
        if (tid < nr) {
          const int gi = c0 + tid;
          src = gi < a.n_a ? 0 : 1;
          const DqnTdSrc& s = sDesc[src];
          row = src == 0 ? a.ids_a[(long long)g * a.n_a + gi] : a.ids_b[(long long)g * a.n_e + (gi - a.n_a)];
          row = row < 0 ? 0 : (row >= s.rows ? s.rows - 1 : row);
          const long long ac = s.action[row];
          act = ac < 0 ? 0 : (ac >= A ? A - 1 : (int)ac);
          rew = s.reward[row];
          dn = s.done[row] * (1.f - s.timeout[row]);
        }
        sRow[tid] = row;
        sSrc[tid] = src;
        sAct[tid] = act;
        sRew[tid] = rew;
        sDone[tid] = dn;
      }
      __syncthreads();

      // ---- target network on next_obs -> y
      for (int i = tid; i < kR * kS; i += kT) {
        const int r = i >> 6, k = i & 63;
        sX[i] = (r < nr && k < D) ? sDesc[sSrc[r]].next_obs[sRow[r] * D + k] : 0.f;
      }
      stage<true>(tid, T + a.off[0], H1, D, sW);
      __syncthreads();
      layer<true, false>(tid, sX, sW, T + a.off[1], D, H1, nr, nullptr, sH1);
      __syncthreads();
      stage<true>(tid, T + a.off[2], H2, H1, sW);
      __syncthreads();
      layer<true, false>(tid, sH1, sW, T + a.off[3], H1, H2, nr, nullptr, sH2);
      __syncthreads();
      stage<true>(tid, T + a.off[4], A, H2, sW);
      __syncthreads();
      layer<false, false>(tid, sH2, sW, T + a.off[5], H2, A, nr, nullptr, sQ);
      __syncthreads();
      if (tid < nr) {
        float mx = sQ[tid * kS];
        for (int j = 1; j < A; ++j) mx = fmaxf(mx, sQ[tid * kS + j]);
        sY[tid] = sRew[tid] + (1.f - sDone[tid]) * a.gamma * mx;
      }

      // ---- online forward on obs
      for (int i = tid; i < kR * kS; i += kT) {
        const int r = i >> 6, k = i & 63;
        sX[i] = (r < nr && k < D) ? sDesc[sSrc[r]].obs[sRow[r] * D + k] : 0.f;
      }
      stage<true>(tid, P + a.off[0], H1, D, sW);
      __syncthreads();
      layer<true, false>(tid, sX, sW, P + a.off[1], D, H1, nr, nullptr, sH1);
      __syncthreads();
      stage<true>(tid, P + a.off[2], H2, H1, sW);
      __syncthreads();
      layer<true, false>(tid, sH1, sW, P + a.off[3], H1, H2, nr, nullptr, sH2);
      __syncthreads();
      stage<true>(tid, P + a.off[4], A, H2, sW);
      __syncthreads();
      layer<false, false>(tid, sH2, sW, P + a.off[5], H2, A, nr, nullptr, sQ);
      __syncthreads();

      // ---- Huber loss (beta = 1, mean over B) and dQ: clamp(delta, -1, 1) / B at the taken action
      if (tid < nr) {
        const float delta = sQ[tid * kS + sAct[tid]] - sY[tid];
        const float ad = fabsf(delta);
        sLoss[c0 + tid] = ad < 1.f ? 0.5f * delta * delta : ad - 0.5f;
        sDq[tid] = fminf(fmaxf(delta, -1.f), 1.f) * invB;
      }
      stage<false>(tid, P + a.off[4], A, H2, sW);
      __syncthreads();
      for (int i = tid; i < kR * kS; i += kT) {
        const int r = i >> 6, j = i & 63;
        sQ[i] = (r < nr && j == sAct[r]) ? sDq[r] : 0.f;
      }
      __syncthreads();

      // ---- backward: dz2 = (dQ . W3) * [h2 > 0], dz1 = (dz2 . W2) * [h1 > 0]
      layer<false, true>(tid, sQ, sW, nullptr, A, H2, nr, sH2, sD2);
      __syncthreads();
      stage<false>(tid, P + a.off[2], H2, H1, sW);
      __syncthreads();
      layer<false, true>(tid, sD2, sW, nullptr, H2, H1, nr, sH1, sD1);
      __syncthreads();

      // ---- dW += dz^T . in, db += sum_r dz (rows in order, in the owning thread's registers)
      wgrad(tid, sD1, sX, N[0], K[0], nr, aW[0]);
      wgrad(tid, sD2, sH1, N[1], K[1], nr, aW[1]);
      wgrad(tid, sQ, sH2, N[2], K[2], nr, aW[2]);
      if (own_b) {
        const float* dz = bl == 0 ? sD1 : (bl == 1 ? sD2 : sQ);
        for (int r = 0; r < nr; ++r) aB += dz[r * kS + bj];
      }
      __syncthreads();
    }

    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int wj = tid >> 2, wk = (tid & 3) * 16;
    const int bl = tid >> 6, bj = tid & 63;
    const bool own_b = bl < 3 && bj < (bl == 0 ? H1 : (bl == 1 ? H2 : A));
    const int off_b = bl == 0 ? a.off[1] : (bl == 1 ? a.off[3] : a.off[5]);

    // ---- loss and |g|^2 through a fixed tree (elements a thread does not own stayed zero)
    float ss = aB * aB;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int i = 0; i < 16; ++i) ss = __builtin_fmaf(aW[l][i], aW[l][i], ss);
    sSq[tid] = ss;
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
      if (tid < s) {
        sLoss[tid] += sLoss[tid + s];
        sSq[tid] += sSq[tid + s];
      }
      __syncthreads();
    }
    const float norm = sqrtf(sSq[0]);
    const float coef = fminf(1.f, a.max_norm / (norm + 1e-6f));  // clip_grad_norm_
    if (tid == 0) {
      a.losses[g] = sLoss[0] / (float)B;
      a.gnorm[g] = norm;
    }

    // ---- clip + Adam from the registers; the last step's clipped gradient goes to the bucket
    const bool last = g == a.G - 1;
    const float bc2_sqrt = sBc[1], step_size = sBc[2];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      if (wj < N[l]) {
        const int base = a.off[2 * l] + wj * K[l] + wk;
        if constexpr (VEC) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (wk + 4 * q < K[l]) clip_adam4(ad, base + 4 * q, aW[l][4 * q], aW[l][4 * q + 1], aW[l][4 * q + 2], aW[l][4 * q + 3], coef, last,
                                           step_size, bc2_sqrt);
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (wk + i < K[l]) clip_adam(ad, base + i, aW[l][i], coef, last, step_size, bc2_sqrt);
        }
      }
    }
    if (own_b) clip_adam(ad, off_b + bj, aB, coef, last, step_size, bc2_sqrt);
    __syncthreads();  // the next step stages the updated weights (and rewrites sLoss / sBc)
  }
  if (threadIdx.x == 0) *a.step = t;
}

}  // namespace

hipError_t dqn_td_step(const DqnTdArgs& a, hipStream_t s) {
  auto dim_ok = [](int d) { return d >= 1 && d <= kDqnTdMaxDim; };
  if (!dim_ok(a.D) || !dim_ok(a.H1) || !dim_ok(a.H2) || !dim_ok(a.A)) return hipErrorInvalidValue;
  if (a.n_a < 0 || a.n_e < 0 || a.n_a + a.n_e < 1 || a.n_a + a.n_e > kDqnTdMaxBatch || a.G < 1) return hipErrorInvalidValue;
  if ((a.n_a > 0 && (a.ids_a == nullptr || a.src[0].rows < 1)) || (a.n_e > 0 && (a.ids_b == nullptr || a.src[1].rows < 1)))
    return hipErrorInvalidValue;
  for (int i = 0; i < 2; ++i) {
    const DqnTdSrc& r = a.src[i];
    if ((i == 0 ? a.n_a : a.n_e) > 0 && !(r.obs && r.next_obs && r.action && r.reward && r.done && r.timeout))
      return hipErrorInvalidValue;
  }
  const int sizes[6] = {a.H1 * a.D, a.H1, a.H2 * a.H1, a.H2, a.A * a.H2, a.A};
  for (int i = 0; i < 6; ++i)
    if (a.off[i] < 0 || (int64_t)a.off[i] + sizes[i] > a.n) return hipErrorInvalidValue;
  if (!(a.params && a.grads && a.exp_avg && a.exp_avg_sq && a.step && a.target && a.losses && a.gnorm))
    return hipErrorInvalidValue;
  const bool vec = ((((uintptr_t)a.params | (uintptr_t)a.grads | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq) & 15) |
                    ((a.off[0] | a.off[2] | a.off[4] | a.D | a.H1 | a.H2) & 3)) == 0;
  if (vec) hipLaunchKernelGGL(dqn_td_kernel<true>, dim3(1), dim3(kT), 0, s, a);
  else hipLaunchKernelGGL(dqn_td_kernel<false>, dim3(1), dim3(kT), 0, s, a);
  return hipGetLastError();
}

}  // namespace ia
