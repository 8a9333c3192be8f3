// Device BC engine (imitation_amd/ops/bc_mlp.py, engine/bc.py): G behavioural-cloning minibatch
// steps of a small MLP policy in ONE launch of ONE workgroup.
//
// The eager step (a numpy fancy-index and an H2D copy, the trunk and head forward, a
// distribution, the seven metrics, two kernels per parameter tensor for the L2 term, the
// autograd backward and adam_flat) is dozens of launches to update the few thousand parameters
// of a [32, 32] policy on 32 rows. Here a step gathers its rows by flat row id from the
// device-resident demonstrations, runs the policy trunk (two hidden layers, Tanh or ReLU) and
// action_net, the categorical or diagonal-Gaussian negative log-likelihood with its entropy
// bonus, the backward through head and trunk (log_std included), adds l2_weight * w to every
// bucket element (the value net, which BC never evaluates, gets exactly that), applies Adam to the
// whole FusedAdam bucket (adam_update.h: the body adam_flat runs) and goes on to the next step.
//
// Everything is fp32 FMAs in a fixed order, so equal states give equal bits: rows go through in
// chunks of 64 with the chunk's activations in LDS (mlp_chunk.h, shared with dqn_td.hip); every
// weight element is owned by one thread, which sums its dW over the rows in row order in a
// register; the per-row loss terms and the sum of squares go through a fixed tree. The short
// serial sums behind a logged scalar (over the actions of a row, over a thread's bucket elements)
// are compensated, and so is the tree. One workgroup, __syncthreads only: nothing here waits on another workgroup.
#include <hip/hip_runtime.h>

#include "adam_update.h"
#include "launchers.h"
#include "mlp_chunk.h"

namespace ia {
namespace {

using namespace chunk;  // kT, kR, kS, kWS, stage, layer, wgrad

constexpr float kHalfLog2Pi = 0.91893853320467274f;  // log(2 pi) / 2

// compensated (Kahan) running sum
struct KSum {
  float s = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

// (s, c) += (t, tc): s + t exactly as the new s and its rounding error, which joins the carried terms
__device__ __forceinline__ void two_sum(float& s, float& c, float t, float tc) {
#pragma clang fp contract(off)
  const float x = s + t, bb = x - s;
  const float e = (s - (x - bb)) + (t - bb);
  s = x;
  c = (c + tc) + e;
}

// w * x for a weight given in double as hi + lo: the product rounded once
__device__ __forceinline__ float mul_hl(float hi, float lo, float x) {
#pragma clang fp contract(off)
  const float p = hi * x;
  return p + __builtin_fmaf(lo, x, __builtin_fmaf(hi, x, -p));
}

// the trunk activation of layer's outputs, by the thread that wrote them (0 stays 0 beyond the width)
__device__ __forceinline__ void activate(int tid, float* sH, int nr, bool tanh_act) {
  const int j = tid & 63, r0 = (tid >> 6) * 16;
  if (r0 >= nr) return;  // (wave uniform)
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const float v = sH[(r0 + i) * kS + j];
    sH[(r0 + i) * kS + j] = tanh_act ? tanhf(v) : fmaxf(v, 0.f);
  }
}

// dz = (dh) * f'(z) from the layer's output h = f(z), by the thread that wrote dh
__device__ __forceinline__ void act_grad(int tid, float* sD, const float* sH, int nr, bool tanh_act) {
  const int j = tid & 63, r0 = (tid >> 6) * 16;
  if (r0 >= nr) return;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const float h = sH[(r0 + i) * kS + j], d = sD[(r0 + i) * kS + j];
    sD[(r0 + i) * kS + j] = tanh_act ? d * (1.f - h * h) : (h > 0.f ? d : 0.f);
  }
}

__global__ __launch_bounds__(kT) void bc_mlp_kernel(BcMlpArgs a) {
  // the chunk's images x, h1, h2, head output / its gradient, dz2, dz1; after the last chunk of a
  // step the same memory holds the step's data gradient, compact (sG)
  __shared__ __attribute__((aligned(16))) float sAct[6 * kR * kS];
  __shared__ float sW[64 * kWS];
  __shared__ long long sRow[kR];
  __shared__ float sLs[64], sStd[64];  // Gaussian head: log_std and exp(log_std)
  __shared__ float sM[4][kT];          // per row: -logp, entropy, exp(logp); per thread: sum of w^2
  __shared__ float sC[4][kT];          // the tree's carried rounding errors of sM
  __shared__ float sBc[3];
  float* const sX = sAct;
  float* const sH1 = sAct + kR * kS;
  float* const sH2 = sAct + 2 * kR * kS;
  float* const sO = sAct + 3 * kR * kS;
  float* const sD2 = sAct + 4 * kR * kS;
  float* const sD1 = sAct + 5 * kR * kS;
  float* const sG = sAct;

  const int D = a.D, H1 = a.H1, H2 = a.H2, A = a.A, B = a.B;
  const bool gauss = a.acts_gauss != nullptr, tanh_act = a.tanh_act != 0;
  const float invB = 1.f / (float)B;
  const int N[3] = {H1, H2, A}, K[3] = {D, H1, H2};
  // the bucket segments that have a data gradient (W1, b1, W2, b2, W3, b3, log_std): offset, length
  // and slot in sG (weights first, so that their slots stay 16-B aligned multiples of K)
  const int seg_off[7] = {a.off[0], a.off[1], a.off[2], a.off[3], a.off[4], a.off[5], a.off_log_std};
  const int seg_len[7] = {H1 * D, H1, H2 * H1, H2, A * H2, A, gauss ? A : 0};
  const int cW1 = 0, cW2 = H1 * D, cW3 = cW2 + H2 * H1, cB1 = cW3 + A * H2, cB2 = cB1 + H1, cB3 = cB2 + H2, cLs = cB3 + A;
  const int seg_slot[7] = {cW1, cB1, cW2, cB2, cW3, cB3, cLs};
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
  const int n = (int)a.n;
  float t = *a.step;

  for (int g = 0; g < a.G; ++g) {
    t += 1.f;
    if (threadIdx.x == 0) adam_bias(ad, t, sBc);
    // this thread's gradient sums: W_l[tid / 4][16 * (tid % 4) .. + 16) of each layer l and, for
    // tid < 192, b_(tid / 64)[tid % 64]; tid >= 192: log_std[tid - 192]
    float aW[3][16];
    float aB = 0.f;
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int i = 0; i < 16; ++i) aW[l][i] = 0.f;
    sM[0][threadIdx.x] = 0.f;
    sM[1][threadIdx.x] = 0.f;
    sM[2][threadIdx.x] = 0.f;
    if (gauss && threadIdx.x < A) {
      const float ls = P[a.off_log_std + threadIdx.x];
      sLs[threadIdx.x] = ls;
      sStd[threadIdx.x] = expf(ls);
    }

    for (int c0 = 0; c0 < B; c0 += kR) {
      const int nr = min(kR, B - c0);
      // (the thread id goes through an opaque copy per chunk, and once more for the Adam phase: the
      // lane masks and element addresses derived from it are then formed where they are used
      // instead of being hoisted and kept live across both loops)
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      const int bl = tid >> 6, bj = tid & 63;
      if (tid < kR) {
        long long row = 0;
        if (tid < nr) {
          row = a.ids[(long long)g * B + c0 + tid];
          row = row < 0 ? 0 : (row >= a.rows ? a.rows - 1 : row);
        }
        sRow[tid] = row;
      }
      __syncthreads();

      // ---- forward: x -> h1 -> h2 -> head (logits / mean actions)
      for (int i = tid; i < kR * kS; i += kT) {
        const int r = i >> 6, k = i & 63;
        sX[i] = (r < nr && k < D) ? a.obs_src[sRow[r] * D + k] : 0.f;
      }
      stage<true>(tid, P + a.off[0], H1, D, sW);
      __syncthreads();
      layer<false, false>(tid, sX, sW, P + a.off[1], D, H1, nr, nullptr, sH1);
      activate(tid, sH1, nr, tanh_act);
      __syncthreads();
      stage<true>(tid, P + a.off[2], H2, H1, sW);
      __syncthreads();
      layer<false, false>(tid, sH1, sW, P + a.off[3], H1, H2, nr, nullptr, sH2);
      activate(tid, sH2, nr, tanh_act);
      __syncthreads();
      stage<true>(tid, P + a.off[4], A, H2, sW);
      __syncthreads();
      layer<false, false>(tid, sH2, sW, P + a.off[5], H2, A, nr, nullptr, sO);
      __syncthreads();

      // ---- a row's loss terms; its head output becomes d loss / d head (already / B)
      if (tid < nr) {
        float* z = sO + tid * kS;
        float nlp, ent, pa;
        if (gauss) {
          // DiagGaussianDistribution.log_prob / entropy; sD2 row: d(-logp) / d log_std / B
          const float* ac = a.acts_gauss + sRow[tid] * A;
          KSum lp, en;
          for (int j = 0; j < A; ++j) {
            const float ls = sLs[j], sd = sStd[j];
            const float zz = (ac[j] - z[j]) / sd;
            lp.add(-0.5f * zz * zz - ls - kHalfLog2Pi);
            en.add(0.5f + kHalfLog2Pi + ls);
            z[j] = -(zz / sd) * invB;
            sD2[tid * kS + j] = (1.f - zz * zz) * invB;
          }
          nlp = -lp.s;
          ent = en.s;
          pa = expf(lp.s);
        } else {
          // log-softmax at the action, entropy -sum p log p; sD2 row: p. log p_j is formed as
          // (z_j - max) - log(sum): one rounding at the size of the difference, not at the size
          // of the logsumexp; p at the action straight from the softmax ratio
          const long long ac = a.acts_cat[sRow[tid]];
          const int act = ac < 0 ? 0 : (ac >= A ? A - 1 : (int)ac);
          float mx = z[0];
          for (int j = 1; j < A; ++j) mx = fmaxf(mx, z[j]);
          KSum se;
          for (int j = 0; j < A; ++j) se.add(expf(z[j] - mx));
          const float lg = logf(se.s);
          KSum en;
          float lpa = 0.f;
          pa = 0.f;
          for (int j = 0; j < A; ++j) {
            const float lp = (z[j] - mx) - lg, p = expf(lp);
            sD2[tid * kS + j] = p;
            en.add(-(p * lp));
            if (j == act) {
              lpa = lp;
              pa = expf(z[j] - mx) / se.s;
            }
          }
          ent = en.s;
          // d(-logp_a)/dz_j = p_j - [j == a]; dH/dz_j = -p_j (log p_j + H)
          for (int j = 0; j < A; ++j) {
            const float lp = (z[j] - mx) - lg, p = sD2[tid * kS + j];
            z[j] = ((p - (j == act ? 1.f : 0.f)) + a.ent_weight * (p * (lp + ent))) * invB;
          }
          nlp = -lpa;
        }
        sM[0][c0 + tid] = nlp;
        sM[1][c0 + tid] = ent;
        sM[2][c0 + tid] = pa;
      }
      __syncthreads();
      if (gauss && bl == 3 && bj < A)
        for (int r = 0; r < nr; ++r) aB += sD2[r * kS + bj];
      stage<false>(tid, P + a.off[4], A, H2, sW);
      __syncthreads();

      // ---- backward: dz2 = (dhead . W3) * f'(h2), dz1 = (dz2 . W2) * f'(h1)
      layer<false, false>(tid, sO, sW, nullptr, A, H2, nr, nullptr, sD2);
      act_grad(tid, sD2, sH2, nr, tanh_act);
      __syncthreads();
      stage<false>(tid, P + a.off[2], H2, H1, sW);
      __syncthreads();
      layer<false, false>(tid, sD2, sW, nullptr, H2, H1, nr, nullptr, sD1);
      act_grad(tid, sD1, sH1, nr, tanh_act);
      __syncthreads();

      // ---- dW += dz^T . in, db += sum_r dz (rows in order, in the owning thread's registers)
      wgrad(tid, sD1, sX, N[0], K[0], nr, aW[0]);
      wgrad(tid, sD2, sH1, N[1], K[1], nr, aW[1]);
      wgrad(tid, sO, sH2, N[2], K[2], nr, aW[2]);
      if (bl < 3 && bj < (bl == 0 ? H1 : (bl == 1 ? H2 : A))) {
        const float* dz = bl == 0 ? sD1 : (bl == 1 ? sD2 : sO);
        for (int r = 0; r < nr; ++r) aB += dz[r * kS + bj];
      }
      __syncthreads();
    }

    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const float ent_row0 = sM[1][0];  // (a Gaussian head's entropy is the same for every row)

    // ---- the data gradient, compact, into LDS (the chunk images are dead)
    {
      const int wj = tid >> 2, wk = (tid & 3) * 16;
      const int bl = tid >> 6, bj = tid & 63;
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        if (wj < N[l]) {
          float* dst = sG + seg_slot[2 * l] + wj * K[l] + wk;
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (wk + i < K[l]) dst[i] = aW[l][i];
        }
      }
      if (bl < 3 && bj < (bl == 0 ? H1 : (bl == 1 ? H2 : A))) sG[(bl == 0 ? cB1 : (bl == 1 ? cB2 : cB3)) + bj] = aB;
      // d(-logp)/d log_std summed over the rows, and the entropy bonus: d(-ent_weight * H)/d log_std = -ent_weight
      if (gauss && bl == 3 && bj < A) sG[cLs + bj] = aB - a.ent_weight;
    }
    __syncthreads();

    // ---- every bucket element: g = data gradient + l2_weight * w, Adam; sum of w^2 on the way
    const bool store_grad = a.keep_grad && g == a.G - 1;
    const float bc2_sqrt = sBc[1], step_size = sBc[2];
    KSum l2;
    for (int idx = tid; idx < n; idx += kT) {
      float p = a.params[idx], m = a.exp_avg[idx], v = a.exp_avg_sq[idx];
      float gr = 0.f;
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const int u = idx - seg_off[s];
        if ((unsigned)u < (unsigned)seg_len[s]) gr = sG[seg_slot[s] + u];
      }
      gr = __builtin_fmaf(a.l2_weight, p, gr);
      l2.add(p * p);
      if (store_grad) a.grads[idx] = gr;
      adam_one(p, gr, m, v, ad, step_size, bc2_sqrt);
      a.params[idx] = p;
      a.exp_avg[idx] = m;
      a.exp_avg_sq[idx] = v;
    }
    sM[3][tid] = l2.s;
    sC[0][tid] = 0.f;
    sC[1][tid] = 0.f;
    sC[2][tid] = 0.f;
    sC[3][tid] = -l2.c;
    __syncthreads();

    // ---- the seven metrics: the sums through a fixed tree that carries its rounding errors (the
    // logged means are then rounded once, not once per level at the size of the total)
    for (int s = kT / 2; s > 0; s >>= 1) {
      if (tid < s) {
#pragma unroll
        for (int q = 0; q < 4; ++q) two_sum(sM[q][tid], sC[q][tid], sM[q][tid + s], sC[q][tid + s]);
      }
      __syncthreads();
    }
    if (tid == 0) {
      const float neglogp = (sM[0][0] + sC[0][0]) / (float)B;
      const float entropy = gauss ? ent_row0 : (sM[1][0] + sC[1][0]) / (float)B;
      const float ent_loss = -mul_hl(a.ent_weight, a.ent_weight_lo, entropy);
      const float l2_norm = 0.5f * (sM[3][0] + sC[3][0]);
      const float l2_loss = mul_hl(a.l2_weight, a.l2_weight_lo, l2_norm);
      float* out = a.metrics + (long long)g * 7;
      out[0] = neglogp;
      out[1] = entropy;
      out[2] = ent_loss;
      out[3] = (sM[2][0] + sC[2][0]) / (float)B;
      out[4] = l2_norm;
      out[5] = l2_loss;
      out[6] = neglogp + ent_loss + l2_loss;
    }
    __syncthreads();  // the next step stages the updated weights (and rewrites sM / sBc / sLs)
  }
  if (threadIdx.x == 0) *a.step = t;
}

}  // namespace

hipError_t bc_mlp_steps(const BcMlpArgs& a, hipStream_t s) {
  auto dim_ok = [](int d) { return d >= 1 && d <= kBcMlpMaxDim; };
  if (!dim_ok(a.D) || !dim_ok(a.H1) || !dim_ok(a.H2) || !dim_ok(a.A)) return hipErrorInvalidValue;
  if (a.B < 1 || a.B > kBcMlpMaxBatch || a.G < 1 || a.n < 1 || a.n > kBcMlpMaxBucket || a.rows < 1) return hipErrorInvalidValue;
  if ((a.acts_cat == nullptr) == (a.acts_gauss == nullptr)) return hipErrorInvalidValue;  // exactly one head
  const int sizes[6] = {a.H1 * a.D, a.H1, a.H2 * a.H1, a.H2, a.A * a.H2, a.A};
  for (int i = 0; i < 6; ++i)
    if (a.off[i] < 0 || (int64_t)a.off[i] + sizes[i] > a.n) return hipErrorInvalidValue;
  if (a.acts_gauss != nullptr && (a.off_log_std < 0 || (int64_t)a.off_log_std + a.A > a.n)) return hipErrorInvalidValue;
  if (!(a.obs_src && a.ids && a.params && a.exp_avg && a.exp_avg_sq && a.step && a.metrics)) return hipErrorInvalidValue;
  if (a.keep_grad && a.grads == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bc_mlp_kernel, dim3(1), dim3(kT), 0, s, a);
  return hipGetLastError();
}

}  // namespace ia
