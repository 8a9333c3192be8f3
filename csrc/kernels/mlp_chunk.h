// fp32 row-chunk helpers of the one-workgroup training kernels (dqn_td.hip, bc_mlp.hip, sac_update.hip): a chunk
// of up to 64 rows has its activations in LDS as [kR][kS] images; `stage` puts one layer's weights
// into LDS, `layer` is the chunk's GEMM with the bias, `wgrad` the owning thread's dW sums. fp32
// FMAs in a fixed order: equal inputs give equal bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ia {
namespace chunk {

constexpr int kT = 256;   // threads
constexpr int kR = 64;    // rows per chunk
constexpr int kS = 64;    // activation row stride: [kR][kS] images, zero beyond a layer's width
constexpr int kWS = 65;   // staged weight row stride (odd: staging and reading both conflict-free)

// Stage the row-major matrix W [R][C] for `layer`: sW[red][out], red the index that layer sums
// over. TR: red = column, out = row (a forward layer, W [out][in]); else red = row, out = column
// (the backward's dz . W). The rows red .. round4(red) are zeroed (layer reads whole quads).
template <bool TR>
__device__ __forceinline__ void stage(int tid, const float* __restrict__ W, int R, int C, float* sW) {
  const int red = TR ? C : R;
  const int red4 = (red + 3) & ~3;
  for (int i = tid; i < (red4 - red) * 64; i += kT) sW[(red + (i >> 6)) * kWS + (i & 63)] = 0.f;
  // four loads in flight per thread (one L2 round trip per 1K elements, not one per 256)
  for (int e0 = tid; e0 < R * C; e0 += 4 * kT) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = e0 + u * kT < R * C ? W[e0 + u * kT] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * kT;
      const int r = e / C, c = e - r * C;
      if (e < R * C) sW[TR ? c * kWS + r : r * kWS + c] = v[u];
    }
  }
}

// sOut[r][j] = f(bias[j] + sum_k sIn[r][k] * sW[k][j]) for the chunk's rows, k in order; columns
// j >= nout are written as zeros. A wave takes 16 rows, a lane one column.
template <bool RELU, bool MASK>
__device__ __forceinline__ void layer(int tid, const float* sIn, const float* sW, const float* __restrict__ bias, int red, int nout,
                                      int nr, const float* sMask, float* sOut) {
  const int j = tid & 63, r0 = (tid >> 6) * 16;
  if (r0 >= nr) return;  // (wave uniform)
  float acc[16];
  const float b = (bias != nullptr && j < nout) ? bias[j] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = b;
  for (int k = 0; k < red; k += 4) {
    const float w0 = sW[k * kWS + j], w1 = sW[(k + 1) * kWS + j], w2 = sW[(k + 2) * kWS + j], w3 = sW[(k + 3) * kWS + j];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 x = *reinterpret_cast<const float4*>(sIn + (r0 + i) * kS + k);
      acc[i] = __builtin_fmaf(x.x, w0, acc[i]);
      acc[i] = __builtin_fmaf(x.y, w1, acc[i]);
      acc[i] = __builtin_fmaf(x.z, w2, acc[i]);
      acc[i] = __builtin_fmaf(x.w, w3, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float v = acc[i];
    if (RELU) v = fmaxf(v, 0.f);
    if (MASK) v = sMask[(r0 + i) * kS + j] > 0.f ? v : 0.f;
    sOut[(r0 + i) * kS + j] = j < nout ? v : 0.f;
  }
}

// `layer` without the bias and the ReLU, on top of an earlier product: sOut[r][j] = sInit[r][j] +
// sum_k sIn[r][k] * sW[k][j] (the backward of two heads on one trunk). sOut may be sInit or sMask:
// a thread reads and writes its own elements only.
template <bool MASK>
__device__ __forceinline__ void layer_acc(int tid, const float* sIn, const float* sW, const float* sInit, int red, int nout, int nr,
                                          const float* sMask, float* sOut) {
  const int j = tid & 63, r0 = (tid >> 6) * 16;
  if (r0 >= nr) return;  // (wave uniform)
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = sInit[(r0 + i) * kS + j];
  for (int k = 0; k < red; k += 4) {
    const float w0 = sW[k * kWS + j], w1 = sW[(k + 1) * kWS + j], w2 = sW[(k + 2) * kWS + j], w3 = sW[(k + 3) * kWS + j];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 x = *reinterpret_cast<const float4*>(sIn + (r0 + i) * kS + k);
      acc[i] = __builtin_fmaf(x.x, w0, acc[i]);
      acc[i] = __builtin_fmaf(x.y, w1, acc[i]);
      acc[i] = __builtin_fmaf(x.z, w2, acc[i]);
      acc[i] = __builtin_fmaf(x.w, w3, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float v = acc[i];
    if (MASK) v = sMask[(r0 + i) * kS + j] > 0.f ? v : 0.f;
    sOut[(r0 + i) * kS + j] = j < nout ? v : 0.f;
  }
}

// acc[i] += sum_r sDz[r][j] * sIn[r][kq + i], rows in order: thread t owns W[j = t / 4][kq = 16 * (t % 4) ..]
__device__ __forceinline__ void wgrad(int tid, const float* sDz, const float* sIn, int N, int K, int nr, float (&acc)[16]) {
  const int j = tid >> 2, kq = (tid & 3) * 16;
  if (j >= N || kq >= K) return;
  for (int r = 0; r < nr; ++r) {
    const float d = sDz[r * kS + j];
    const float4* x = reinterpret_cast<const float4*>(sIn + r * kS + kq);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = x[q];
      acc[4 * q + 0] = __builtin_fmaf(d, v.x, acc[4 * q + 0]);
      acc[4 * q + 1] = __builtin_fmaf(d, v.y, acc[4 * q + 1]);
      acc[4 * q + 2] = __builtin_fmaf(d, v.z, acc[4 * q + 2]);
      acc[4 * q + 3] = __builtin_fmaf(d, v.w, acc[4 * q + 3]);
    }
  }
}

}  // namespace chunk
}  // namespace ia
