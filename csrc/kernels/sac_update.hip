// Fused SAC update (imitation_amd/ops/sac.py, rl/sac.py): ALL gradient steps of one SAC.train
// call in ONE launch of ONE workgroup.
//
// The eager step (replay samples and cats, two actor forwards, two target critics, two critics
// twice, three autograd backwards, three Adam steps, a foreach Polyak update) is a few hundred
// launches to update three two-hidden-layer MLPs on at most 256 rows. Here a step gathers its
// rows by flat row id from the agent ring (source 0) and SQIL's expert ring (source 1) and makes
// two passes over them in chunks of 64 rows:
//   pass 1: actor on next_obs (noise eps_next) -> a', logp'; target critics on [next_obs | a'] ->
//           y; critics on [obs | act], MSE loss, backward, dW sums; then Adam on the critic bucket;
//   pass 2: actor on obs (noise eps_pi) -> a_pi, logp; the UPDATED critics on [obs | a_pi], each
//           critic's dq/da (q is a scalar: one backward with a unit seed), the min-selected one
//           per row; backward through tanh, the log-prob terms and the log_std clamp into the
//           heads and the trunk, dW sums; then Adam on the actor bucket, the entropy coefficient's
//           loss and its Adam step (both passes use the pre-update coefficient, and the loss needs
//           only this pass's logp, so the eager step's extra actor forward is not needed), Polyak.
//
// Everything is fp32 FMAs (the target feeds back into itself: no bf16 operands) with the accurate
// expf / tanhf / logf. The summation order is fixed, so equal states give equal bits: every
// weight element is owned by one thread, which sums its dW over the rows in a fixed order in
// registers (per chunk four row-interleaved partial sums, each in row order) and applies Adam
// (adam_update.h: the body adam_flat runs) from that register; the losses go through a fixed
// tree. One workgroup, __syncthreads only: nothing here waits on another workgroup.
#include <hip/hip_runtime.h>

#include "adam_update.h"
#include "launchers.h"
#include "mlp_chunk.h"

namespace ia {
namespace {

using namespace chunk;  // kT, kR, kS, kWS, stage, layer, layer_acc (mlp_chunk.h)

constexpr float kLogStdMin = -20.f, kLogStdMax = 2.f;
constexpr float kHalfLog2Pi = 0.91893853320467274178f;
constexpr float kSquashEps = 1e-6f;

__device__ __forceinline__ AdamArgs adam_of(const SacBucket& b) {
  // (plain Adam: the weight-decay, maximize and zero-grad branches of adam_one fold away)
  AdamArgs ad{};
  ad.params = b.params;
  ad.grads = b.grads;
  ad.exp_avg = b.exp_avg;
  ad.exp_avg_sq = b.exp_avg_sq;
  ad.lr = b.lr;
  ad.beta1 = b.beta1;
  ad.beta2 = b.beta2;
  ad.eps = b.eps;
  return ad;
}

// the Adam update of element idx from the gradient g; the last step's gradient goes to the bucket
__device__ __forceinline__ void reg_adam(const AdamArgs& ad, int idx, float g, bool store_grad, float step_size, float bc2_sqrt) {
  if (store_grad) ad.grads[idx] = g;
  float p = ad.params[idx], m = ad.exp_avg[idx], v = ad.exp_avg_sq[idx];
  adam_one(p, g, m, v, ad, step_size, bc2_sqrt);
  ad.params[idx] = p;
  ad.exp_avg[idx] = m;
  ad.exp_avg_sq[idx] = v;
}

// this thread's slice W[tid / 4][16 * (tid % 4) .. + 16) of the [N][K] matrix at `off`
__device__ __forceinline__ void adam_slice(const AdamArgs& ad, int tid, int off, int N, int K, const float (&acc)[16], bool store_grad,
                                           float step_size, float bc2_sqrt) {
  const int wj = tid >> 2, wk = (tid & 3) * 16;
  if (wj >= N) return;
  const int base = off + wj * K + wk;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (wk + i < K) reg_adam(ad, base + i, acc[i], store_grad, step_size, bc2_sqrt);
}

// the chunk's rows: source and flat row id (clamped into the ring)
__device__ __forceinline__ void chunk_rows(const SacUpdateArgs& a, const SacSrc* sDesc, int tid, int g, int c0, int nr, long long* sRow,
                                           int* sSrc) {
  if (tid < kR) {
    long long row = 0;
    int src = 0;
    if (tid < nr) {
      const int gi = c0 + tid;
      src = gi < a.n_a ? 0 : 1;
      const long long rows = sDesc[src].rows;
      row = src == 0 ? a.ids_a[(long long)g * a.n_a + gi] : a.ids_b[(long long)g * a.n_e + (gi - a.n_a)];
      row = row < 0 ? 0 : (row >= rows ? rows - 1 : row);
    }
    sRow[tid] = row;
    sSrc[tid] = src;
  }
}

// sX[r] = [obs or next_obs | action (ACT) | 0], zero rows beyond the chunk
template <bool NEXT, bool ACT>
__device__ __forceinline__ void fill_input(const SacSrc* sDesc, int tid, int nr, int D, int A, const long long* sRow, const int* sSrc,
                                           float* sX) {
  for (int i = tid; i < kR * kS; i += kT) {
    const int r = i >> 6, k = i & 63;
    float v = 0.f;
    if (r < nr) {
      const SacSrc& s = sDesc[sSrc[r]];
      if (k < D) v = (NEXT ? s.next_obs : s.obs)[sRow[r] * D + k];
      else if (ACT && k < D + A) v = s.action[sRow[r] * A + (k - D)];
    }
    sX[i] = v;
  }
}

// The actor on the rows of sX (columns < D; the rest zero): trunk -> sH1, sH2, heads -> sMu and the
// raw (unclamped) log_std -> sLs; then a = tanh(mu + exp(clamp(log_std)) * eps) -> sX[r][D + j] and
// logp[r] = sum_j(-eps^2 / 2 - log_std - log(2 pi) / 2) - sum_j log(1 - a^2 + 1e-6) -> sLogp.
// sMu and sTmp end as scratch. eps: the chunk's noise rows [nr][A]. Ends on a barrier.
__device__ __forceinline__ void actor_forward(const SacUpdateArgs& a, int tid, int nr, const float* __restrict__ eps, float* sX,
                                              float* sH1, float* sH2, float* sMu, float* sLs, float* sTmp, float* sW, float* sLogp) {
  const float* P = a.actor.params;
  const int D = a.D, A = a.A, H1 = a.aH1, H2 = a.aH2;
  stage<true>(tid, P + a.a_off[0], H1, D, sW);
  __syncthreads();
  layer<true, false>(tid, sX, sW, P + a.a_off[1], D, H1, nr, nullptr, sH1);
  __syncthreads();
  stage<true>(tid, P + a.a_off[2], H2, H1, sW);
  __syncthreads();
  layer<true, false>(tid, sH1, sW, P + a.a_off[3], H1, H2, nr, nullptr, sH2);
  __syncthreads();
  stage<true>(tid, P + a.a_off[4], A, H2, sW);
  __syncthreads();
  layer<false, false>(tid, sH2, sW, P + a.a_off[5], H2, A, nr, nullptr, sMu);
  __syncthreads();
  stage<true>(tid, P + a.a_off[6], A, H2, sW);
  __syncthreads();
  layer<false, false>(tid, sH2, sW, P + a.a_off[7], H2, A, nr, nullptr, sLs);
  __syncthreads();
  for (int i = tid; i < nr * A; i += kT) {
    const int r = i / A, j = i - r * A;
    const float ls = fminf(fmaxf(sLs[r * kS + j], kLogStdMin), kLogStdMax);
    const float e = eps[i];
    const float act = tanhf(__builtin_fmaf(expf(ls), e, sMu[r * kS + j]));
    sX[r * kS + D + j] = act;
    sMu[r * kS + j] = -0.5f * e * e - ls - kHalfLog2Pi;
    sTmp[r * kS + j] = logf(1.f - act * act + kSquashEps);
  }
  __syncthreads();
  if (tid < nr) {
    float s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < A; ++j) {
      s1 += sMu[tid * kS + j];
      s2 += sTmp[tid * kS + j];
    }
    sLogp[tid] = s1 - s2;
  }
  __syncthreads();
}

// One critic (its six tensors at off[] of the bucket P) on the rows of sX = [obs | action]:
// hidden activations -> sH1, sH2, q -> column 0 of sQ (the other columns zero). Ends on a barrier.
__device__ __forceinline__ void critic_forward(const SacUpdateArgs& a, int tid, int nr, const float* P, const int* off, const float* sX,
                                               float* sH1, float* sH2, float* sQ, float* sW) {
  const int DA = a.D + a.A, H1 = a.cH1, H2 = a.cH2;
  stage<true>(tid, P + off[0], H1, DA, sW);
  __syncthreads();
  layer<true, false>(tid, sX, sW, P + off[1], DA, H1, nr, nullptr, sH1);
  __syncthreads();
  stage<true>(tid, P + off[2], H2, H1, sW);
  __syncthreads();
  layer<true, false>(tid, sH1, sW, P + off[3], H1, H2, nr, nullptr, sH2);
  __syncthreads();
  stage<true>(tid, P + off[4], 1, H2, sW);
  __syncthreads();
  layer<false, false>(tid, sH2, sW, P + off[5], H2, 1, nr, nullptr, sQ);
  __syncthreads();
}

// s = a + b rounded, e the rounding error of that addition (a + b = s + e exactly)
__device__ __forceinline__ void two_sum(float a, float b, float& s, float& e) {
  s = a + b;
  const float bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// sums of two [kT] arrays through a fixed tree, left in element 0. Every addition's rounding error
// is carried along in e0 / e1 (zero on entry) and added at the end: the mean of 256 rows is then
// as exact as its rows, whatever their sum's magnitude.
__device__ __forceinline__ void tree2(int tid, float* s0, float* e0, float* s1, float* e1) {
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      float sum, err;
      two_sum(s0[tid], s0[tid + s], sum, err);
      s0[tid] = sum;
      e0[tid] = (e0[tid] + e0[tid + s]) + err;
      two_sum(s1[tid], s1[tid + s], sum, err);
      s1[tid] = sum;
      e1[tid] = (e1[tid] + e1[tid + s]) + err;
    }
    __syncthreads();
  }
  if (tid == 0) {
    s0[0] += e0[0];
    s1[0] += e1[0];
  }
  __syncthreads();
}

// wgrad (mlp_chunk.h) for one chunk through four partial sums (rows r = 0, 1, 2, 3 mod 4, each in
// row order), added pairwise and then to acc: a sum over 256 rows carries the rounding of a few
// additions of partial sums, not that of 256 additions to the running total
__device__ __forceinline__ void wgrad4(int tid, const float* sDz, const float* sIn, int N, int K, int nr, float (&acc)[16]) {
  const int j = tid >> 2, kq = (tid & 3) * 16;
  if (j >= N || kq >= K) return;
  float p[4][16];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) p[u][i] = 0.f;
  for (int r0 = 0; r0 < nr; r0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u;
      if (r < nr) {
        const float d = sDz[r * kS + j];
        const float4* x = reinterpret_cast<const float4*>(sIn + r * kS + kq);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = x[q];
          p[u][4 * q + 0] = __builtin_fmaf(d, v.x, p[u][4 * q + 0]);
          p[u][4 * q + 1] = __builtin_fmaf(d, v.y, p[u][4 * q + 1]);
          p[u][4 * q + 2] = __builtin_fmaf(d, v.z, p[u][4 * q + 2]);
          p[u][4 * q + 3] = __builtin_fmaf(d, v.w, p[u][4 * q + 3]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] += (p[0][i] + p[1][i]) + (p[2][i] + p[3][i]);
}

// the same for a bias: sum_r dz[r][bj] of the chunk
__device__ __forceinline__ float bias4(const float* dz, int bj, int nr) {
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < nr; r0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r0 + u < nr) p[u] += dz[(r0 + u) * kS + bj];
  }
  return (p[0] + p[1]) + (p[2] + p[3]);
}

__global__ __launch_bounds__(kT) void sac_update_kernel(SacUpdateArgs a) {
  // eight [kR][kS] activation images (which is which: at their uses below) and one staged weight matrix
  __shared__ __attribute__((aligned(16))) float sImg[8][kR * kS];
  __shared__ float sW[64 * kWS];
  __shared__ long long sRow[kR];
  __shared__ int sSrc[kR];
  __shared__ float sRew[kR], sDone[kR], sY[kR], sLogp[kR], sQv[2][kR];
  __shared__ float sRedA[kT], sRedB[kT], sErrA[kT], sErrB[kT];  // the loss sums and their carried rounding errors
  __shared__ float sBc[3][3];   // adam_bias of the critic, actor and entropy-coefficient buckets
  __shared__ SacSrc sDesc[2];   // the ring descriptors: read per lane from here, not held in scalar registers

  float* const sX = sImg[0];
  const int D = a.D, A = a.A, DA = a.D + a.A;
  const int B = a.n_a + a.n_e;
  const float invB = 1.f / (float)B;
  const bool learned = a.ent.params != nullptr;
  const AdamArgs adC = adam_of(a.critic), adA = adam_of(a.actor), adE = adam_of(a.ent);
  float tC = *a.critic.step, tA = *a.actor.step, tE = learned ? *a.ent.step : 0.f;
  if (threadIdx.x == 0) {
    sDesc[0] = a.src[0];
    sDesc[1] = a.src[1];
  }
  __syncthreads();

  for (int g = 0; g < a.G; ++g) {
    tC += 1.f;
    tA += 1.f;
    tE += 1.f;
    if (threadIdx.x == 0) {
      adam_bias(adC, tC, sBc[0]);
      adam_bias(adA, tA, sBc[1]);
      if (learned) adam_bias(adE, tE, sBc[2]);
    }
    const bool last = g == a.G - 1;
    // the pre-update coefficient: this step's target and actor loss use it (the entropy
    // coefficient's own Adam step comes at the end of the step, behind barriers)
    const float log_ent = learned ? a.ent.params[0] : 0.f;
    const float ent = learned ? expf(log_ent) : a.ent_coef_fixed;

    // ================================================================ pass 1: target and critic update
    {
      // this thread's gradient sums per critic: W_l[tid / 4][16 * (tid % 4) .. + 16) of each layer l
      // and, for tid < 192, b_(tid / 64)[tid % 64]
      float cW[2][3][16];
      float cB[2] = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int i = 0; i < 16; ++i) cW[k][l][i] = 0.f;
      sRedA[threadIdx.x] = 0.f;
      sRedB[threadIdx.x] = 0.f;
      sErrA[threadIdx.x] = 0.f;
      sErrB[threadIdx.x] = 0.f;

      for (int c0 = 0; c0 < B; c0 += kR) {
        const int nr = min(kR, B - c0);
        // (the thread id goes through an opaque copy per chunk: the lane masks and element
        // addresses derived from it are then formed where they are used instead of being hoisted
        // and kept live across both loops)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        float* const sH1 = sImg[1];
        float* const sH2 = sImg[2];
        float* const sMu = sImg[3];
        float* const sLs = sImg[4];
        float* const sQ = sImg[5];
        float* const sD2 = sImg[6];
        float* const sD1 = sImg[7];
        chunk_rows(a, sDesc, tid, g, c0, nr, sRow, sSrc);
        if (tid < kR) {
          float rew = 0.f, dn = 0.f;
          if (tid < nr) {  // (the clamped row id of chunk_rows, by the same thread)
            const SacSrc& s = sDesc[sSrc[tid]];
            rew = s.reward[sRow[tid]];
            dn = s.done[sRow[tid]] * (1.f - s.timeout[sRow[tid]]);
          }
          sRew[tid] = rew;
          sDone[tid] = dn;
        }
        __syncthreads();

        // ---- actor on next_obs -> a' (into sX), logp'; the target critics on [next_obs | a'] -> y
        fill_input<true, false>(sDesc, tid, nr, D, A, sRow, sSrc, sX);
        actor_forward(a, tid, nr, a.eps_next + ((long long)g * B + c0) * A, sX, sH1, sH2, sMu, sLs, sQ, sW, sLogp);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          critic_forward(a, tid, nr, a.target, a.c_off[k], sX, sH1, sH2, sQ, sW);
          if (tid < nr) sQv[k][tid] = sQ[tid * kS];
        }
        __syncthreads();
        if (tid < nr) {
          const float nq = fminf(sQv[0][tid], sQv[1][tid]) - ent * sLogp[tid];
          sY[tid] = sRew[tid] + (1.f - sDone[tid]) * a.gamma * nq;
        }

        // ---- both critics on [obs | act]: MSE against y, backward, dW sums
        fill_input<false, true>(sDesc, tid, nr, D, A, sRow, sSrc, sX);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float* P = a.critic.params;
          const int* off = a.c_off[k];
          critic_forward(a, tid, nr, P, off, sX, sH1, sH2, sQ, sW);
          // critic_loss = 0.5 * (mean (q1 - y)^2 + mean (q2 - y)^2): dq_k = (q_k - y) / B
          if (tid < nr) {
            const float delta = sQ[tid * kS] - sY[tid];
            (k == 0 ? sRedA : sRedB)[c0 + tid] = delta * delta;
            sQ[tid * kS] = delta * invB;
          }
          stage<false>(tid, P + off[4], 1, a.cH2, sW);
          __syncthreads();
          // dz2 = (dq . W3) * [h2 > 0], dz1 = (dz2 . W2) * [h1 > 0]
          layer<false, true>(tid, sQ, sW, nullptr, 1, a.cH2, nr, sH2, sD2);
          __syncthreads();
          stage<false>(tid, P + off[2], a.cH2, a.cH1, sW);
          __syncthreads();
          layer<false, true>(tid, sD2, sW, nullptr, a.cH2, a.cH1, nr, sH1, sD1);
          __syncthreads();
          // dW += dz^T . in, db += sum_r dz (rows in order, in the owning thread's registers)
          wgrad4(tid, sD1, sX, a.cH1, DA, nr, cW[k][0]);
          wgrad4(tid, sD2, sH1, a.cH2, a.cH1, nr, cW[k][1]);
          wgrad4(tid, sQ, sH2, 1, a.cH2, nr, cW[k][2]);
          const int bl = tid >> 6, bj = tid & 63;
          if (bl < 3 && bj < (bl == 0 ? a.cH1 : (bl == 1 ? a.cH2 : 1))) {
            const float* dz = bl == 0 ? sD1 : (bl == 1 ? sD2 : sQ);
            cB[k] += bias4(dz, bj, nr);
          }
          __syncthreads();
        }
      }

      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      tree2(tid, sRedA, sErrA, sRedB, sErrB);
      if (tid == 0) a.critic_loss[g] = 0.5f * (sRedA[0] / (float)B + sRedB[0] / (float)B);
      // ---- Adam on the critic bucket from the registers (SAC clips no gradient)
      const float bc2_sqrt = sBc[0][1], step_size = sBc[0][2];
      const int bl = tid >> 6, bj = tid & 63;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        adam_slice(adC, tid, a.c_off[k][0], a.cH1, DA, cW[k][0], last, step_size, bc2_sqrt);
        adam_slice(adC, tid, a.c_off[k][2], a.cH2, a.cH1, cW[k][1], last, step_size, bc2_sqrt);
        adam_slice(adC, tid, a.c_off[k][4], 1, a.cH2, cW[k][2], last, step_size, bc2_sqrt);
        if (bl < 3 && bj < (bl == 0 ? a.cH1 : (bl == 1 ? a.cH2 : 1)))
          reg_adam(adC, a.c_off[k][2 * bl + 1] + bj, cB[k], last, step_size, bc2_sqrt);
      }
      __syncthreads();  // pass 2 stages the updated critics
    }

    // ================================================================ pass 2: actor update
    {
      // W1, W2, Wmu, Wls slices and, per thread, one element of b1 / b2 / bmu / bls (tid / 64)
      float aW[4][16];
      float aB = 0.f;
#pragma unroll
      for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int i = 0; i < 16; ++i) aW[l][i] = 0.f;
      sRedA[threadIdx.x] = 0.f;
      sRedB[threadIdx.x] = 0.f;
      sErrA[threadIdx.x] = 0.f;
      sErrB[threadIdx.x] = 0.f;

      for (int c0 = 0; c0 < B; c0 += kR) {
        const int nr = min(kR, B - c0);
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        float* const aH1 = sImg[1];
        float* const aH2 = sImg[2];
        float* const sG1 = sImg[3];  // first the actor's mu, then dq1 / d[obs | a]
        float* const sLs = sImg[4];  // the raw log_std, kept for the backward
        float* const cH1 = sImg[5];  // a critic's h1, then its dz1 (in place); at last the actor's d log_std
        float* const cH2 = sImg[6];  // a critic's h2, then its dz2 (in place); after the second critic dq2 / d[obs | a]
        float* const sT = sImg[7];   // q, then the unit seed; at last the actor's d mu
        const float* eps = a.eps_pi + ((long long)g * B + c0) * A;
        chunk_rows(a, sDesc, tid, g, c0, nr, sRow, sSrc);
        __syncthreads();
        fill_input<false, false>(sDesc, tid, nr, D, A, sRow, sSrc, sX);
        actor_forward(a, tid, nr, eps, sX, aH1, aH2, sG1, sLs, sT, sW, sLogp);

        // ---- the updated critics on [obs | a_pi]: q_k and dq_k / d input (a unit seed through the
        // ReLU masks, in place over the activations)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float* P = a.critic.params;
          const int* off = a.c_off[k];
          critic_forward(a, tid, nr, P, off, sX, cH1, cH2, sT, sW);
          if (tid < nr) {
            sQv[k][tid] = sT[tid * kS];
            sT[tid * kS] = 1.f;
          }
          stage<false>(tid, P + off[4], 1, a.cH2, sW);
          __syncthreads();
          layer<false, true>(tid, sT, sW, nullptr, 1, a.cH2, nr, cH2, cH2);
          __syncthreads();
          stage<false>(tid, P + off[2], a.cH2, a.cH1, sW);
          __syncthreads();
          layer<false, true>(tid, cH2, sW, nullptr, a.cH2, a.cH1, nr, cH1, cH1);
          __syncthreads();
          stage<false>(tid, P + off[0], a.cH1, DA, sW);
          __syncthreads();
          layer<false, false>(tid, cH1, sW, nullptr, a.cH1, DA, nr, nullptr, k == 0 ? sG1 : cH2);
          __syncthreads();
        }

        // ---- actor_loss = mean(ent * logp - min(q1, q2)); d mu and d log_std per element
        if (tid < nr) {
          sRedA[c0 + tid] = ent * sLogp[tid] - fminf(sQv[0][tid], sQv[1][tid]);
          sRedB[c0 + tid] = sLogp[tid] + a.target_entropy;
        }
        for (int i = tid; i < kR * kS; i += kT) {
          const int r = i >> 6, j = i & 63;
          float dmu = 0.f, dls = 0.f;
          if (r < nr && j < A) {
            const float act = sX[r * kS + D + j];
            const float dqda = (sQv[0][r] <= sQv[1][r] ? sG1 : cH2)[r * kS + D + j];
            const float om = 1.f - act * act;
            // d/da of ent * (-log(1 - a^2 + 1e-6)) - min q, then through a = tanh(u)
            const float dLda = invB * (ent * (2.f * act / (om + kSquashEps)) - dqda);
            dmu = dLda * om;
            // u = mu + exp(log_std) * eps; logp holds -log_std; clamp passes where -20 <= x <= 2
            const float raw = sLs[i];
            const float ls = fminf(fmaxf(raw, kLogStdMin), kLogStdMax);
            const float d = dmu * (expf(ls) * eps[r * A + j]) - invB * ent;
            dls = (raw >= kLogStdMin && raw <= kLogStdMax) ? d : 0.f;
          }
          sT[i] = dmu;
          cH1[i] = dls;
        }
        __syncthreads();

        // ---- backward: dz2 = (dmu . Wmu + dls . Wls) * [h2 > 0] -> sG1, dz1 = (dz2 . W2) * [h1 > 0] -> cH2
        const float* P = a.actor.params;
        stage<false>(tid, P + a.a_off[4], A, a.aH2, sW);
        __syncthreads();
        layer<false, false>(tid, sT, sW, nullptr, A, a.aH2, nr, nullptr, sG1);
        __syncthreads();
        stage<false>(tid, P + a.a_off[6], A, a.aH2, sW);
        __syncthreads();
        layer_acc<true>(tid, cH1, sW, sG1, A, a.aH2, nr, aH2, sG1);
        __syncthreads();
        stage<false>(tid, P + a.a_off[2], a.aH2, a.aH1, sW);
        __syncthreads();
        layer<false, true>(tid, sG1, sW, nullptr, a.aH2, a.aH1, nr, aH1, cH2);
        __syncthreads();
        wgrad4(tid, cH2, sX, a.aH1, D, nr, aW[0]);
        wgrad4(tid, sG1, aH1, a.aH2, a.aH1, nr, aW[1]);
        wgrad4(tid, sT, aH2, A, a.aH2, nr, aW[2]);
        wgrad4(tid, cH1, aH2, A, a.aH2, nr, aW[3]);
        const int bl = tid >> 6, bj = tid & 63;
        if (bj < (bl == 0 ? a.aH1 : (bl == 1 ? a.aH2 : A))) {
          const float* dz = bl == 0 ? cH2 : (bl == 1 ? sG1 : (bl == 2 ? sT : cH1));
          aB += bias4(dz, bj, nr);
        }
        __syncthreads();
      }

      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      tree2(tid, sRedA, sErrA, sRedB, sErrB);
      if (tid == 0) {
        a.actor_loss[g] = sRedA[0] / (float)B;
        a.ent_coef[g] = ent;
        float ent_loss = 0.f;
        if (learned) {
          // ent_coef_loss = -mean(log_ent_coef * (logp + target_entropy)); Adam on the one element
          const float mean = sRedB[0] / (float)B;
          ent_loss = -(log_ent * mean);
          reg_adam(adE, 0, -mean, last, sBc[2][2], sBc[2][1]);
        }
        a.ent_coef_loss[g] = ent_loss;
      }
      // ---- Adam on the actor bucket from the registers
      const float bc2_sqrt = sBc[1][1], step_size = sBc[1][2];
      const int bl = tid >> 6, bj = tid & 63;
      adam_slice(adA, tid, a.a_off[0], a.aH1, D, aW[0], last, step_size, bc2_sqrt);
      adam_slice(adA, tid, a.a_off[2], a.aH2, a.aH1, aW[1], last, step_size, bc2_sqrt);
      adam_slice(adA, tid, a.a_off[4], A, a.aH2, aW[2], last, step_size, bc2_sqrt);
      adam_slice(adA, tid, a.a_off[6], A, a.aH2, aW[3], last, step_size, bc2_sqrt);
      if (bj < (bl == 0 ? a.aH1 : (bl == 1 ? a.aH2 : A))) reg_adam(adA, a.a_off[2 * bl + 1] + bj, aB, last, step_size, bc2_sqrt);
      // ---- Polyak: target = target * (1 - tau) + tau * critic over the whole bucket
      if (g % a.target_update_interval == 0) {
        for (int64_t i = tid; i < a.critic.n; i += kT) a.target[i] = __builtin_fmaf(a.tau, a.critic.params[i], a.target[i] * a.one_minus_tau);
      }
      __syncthreads();  // the next step stages the updated weights (and rewrites the sums and sBc)
    }
  }
  if (threadIdx.x == 0) {
    *a.critic.step = tC;
    *a.actor.step = tA;
    if (learned) *a.ent.step = tE;
  }
}

bool bucket_ok(const SacBucket& b) { return b.params && b.grads && b.exp_avg && b.exp_avg_sq && b.step && b.n >= 1; }

}  // namespace

hipError_t sac_update_step(const SacUpdateArgs& a, hipStream_t s) {
  auto dim_ok = [](int d) { return d >= 1 && d <= kSacMaxDim; };
  if (!dim_ok(a.D) || !dim_ok(a.aH1) || !dim_ok(a.aH2) || !dim_ok(a.cH1) || !dim_ok(a.cH2)) return hipErrorInvalidValue;
  if (a.A < 1 || a.D + a.A > kSacMaxDim) return hipErrorInvalidValue;
  if (a.n_a < 0 || a.n_e < 0 || a.n_a + a.n_e < 1 || a.n_a + a.n_e > kSacMaxBatch || a.G < 1) return hipErrorInvalidValue;
  if (a.target_update_interval < 1) return hipErrorInvalidValue;
  if ((a.n_a > 0 && (a.ids_a == nullptr || a.src[0].rows < 1)) || (a.n_e > 0 && (a.ids_b == nullptr || a.src[1].rows < 1)))
    return hipErrorInvalidValue;
  for (int i = 0; i < 2; ++i) {
    const SacSrc& r = a.src[i];
    if ((i == 0 ? a.n_a : a.n_e) > 0 && !(r.obs && r.next_obs && r.action && r.reward && r.done && r.timeout))
      return hipErrorInvalidValue;
  }
  if (!bucket_ok(a.actor) || !bucket_ok(a.critic) || (a.ent.params != nullptr && !bucket_ok(a.ent))) return hipErrorInvalidValue;
  if (!(a.eps_pi && a.eps_next && a.target && a.critic_loss && a.actor_loss && a.ent_coef && a.ent_coef_loss))
    return hipErrorInvalidValue;
  const int a_sizes[8] = {a.aH1 * a.D, a.aH1, a.aH2 * a.aH1, a.aH2, a.A * a.aH2, a.A, a.A * a.aH2, a.A};
  for (int i = 0; i < 8; ++i)
    if (a.a_off[i] < 0 || (int64_t)a.a_off[i] + a_sizes[i] > a.actor.n) return hipErrorInvalidValue;
  const int c_sizes[6] = {a.cH1 * (a.D + a.A), a.cH1, a.cH2 * a.cH1, a.cH2, a.cH2, 1};
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 6; ++i)
      if (a.c_off[k][i] < 0 || (int64_t)a.c_off[k][i] + c_sizes[i] > a.critic.n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sac_update_kernel, dim3(1), dim3(kT), 0, s, a);
  return hipGetLastError();
}

}  // namespace ia
