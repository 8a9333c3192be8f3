// Batch moments of gathered minibatch columns and their Chan merge into a RunningNorm: the one
// copy used by the fused reward updates (disc.hip, airl_disc.hip, pref_rm.hip).
//
// Shift of the moment sums. The batch variance is formed as S2/n - (S1/n)^2 from fp32 block sums
// of (v - shift) and (v - shift)^2, which is only accurate when |mean - shift| is not large
// against the column's spread (a column at 100 +- 1 summed with shift 0 loses three digits of
// its variance). The running mean is such a shift once it has seen data, but it is 0 on the
// first update and absent without a normaliser. So every gather block keeps two pairs of sums
// per column: one shifted by the running mean (or 0), one shifted by the minibatch's own first
// gathered row, which each block re-gathers and the norm kernel reads back from row 0 of the
// gathered minibatch. The norm kernel takes the running-mean pair unless the two variances
// disagree (batch_moments), so well-centred data gives the bits it always gave.
// The DP modes all-reduce the sums over ranks and need a shift every rank agrees on: they use
// the running-mean pair alone. Remaining limitation: there, until the running mean has seen
// data -- or always, without that normaliser -- an off-centre column's variance keeps that
// cancellation error. pref_rm.hip keeps the running-mean pair alone in every mode.
#pragma once
#include <hip/hip_runtime.h>

namespace ia {

constexpr int kMomentSums = 4;  // per block and column: S1, S2 (running-mean shift), S1, S2 (row-0 shift)
// The norm kernels run 1024 threads = 8 block-phases x 128 columns: phase p sums partial blocks
// p, p+8, ... in order, then the 8 phase sums are added in phase order (fixed order: deterministic).
constexpr int kNormPhases = 8;
// The two variances of a column agree to rounding when the running mean is a fair centre of the
// batch; then the running-mean pair is used, as it always was. Where they differ by more than
// kMomentRtol of the row-0 variance, the running-mean pair has lost that much to cancellation
// and the row-0 pair, whose error stays near fp32 rounding whatever the column's offset, is
// used instead.
constexpr double kMomentRtol = 1e-5;

__device__ __forceinline__ void chan_merge(float* rmean, float* rvar, int count, int c, float bmean, float bvar, int n) {
  // RunningNorm.update_stats (networks.py:94-111) in the same operation order (fp32)
  const float fc = (float)count, fn = (float)n, tot = (float)(count + n);
  const float delta = bmean - rmean[c];
  rmean[c] += delta * fn / tot;
  float v = rvar[c] * fc;
  v += bvar * fn;
  v += delta * delta * fc * fn / tot;
  rvar[c] = v / tot;
}

// One thread's four sums of one column over its rows of a gather block.
struct MomentAcc {
  float s[kMomentSums] = {0.f, 0.f, 0.f, 0.f};
  __device__ __forceinline__ void add(float v, float shift, float shift0) {
    const float dv = v - shift;
    s[0] += dv;
    s[1] += dv * dv;
    const float dv0 = v - shift0;
    s[2] += dv0;
    s[3] += dv0 * dv0;
  }
};

// Gather block of 256 threads = 2 row phases x 128 columns: the two phases' sums of column c,
// added in phase order, go to partials[blockIdx.x][k][ncol].
__device__ __forceinline__ void store_block_moments(float (&red)[2][kMomentSums][128], const MomentAcc& m, int ph, int c,
                                                    bool col_ok, float* partials, int ncol) {
#pragma unroll
  for (int k = 0; k < kMomentSums; ++k) red[ph][k][c] = m.s[k];
  __syncthreads();
  if (ph == 0 && col_ok) {
    float* out = partials + (size_t)blockIdx.x * kMomentSums * ncol;
#pragma unroll
    for (int k = 0; k < kMomentSums; ++k) out[k * ncol + c] = red[0][k][c] + red[1][k][c];
  }
}

// Phase ph's sums of the first NS partial rows of blocks ph, ph + 8, ... for one column, added
// in block order; the loads of four blocks are issued together (the loop is latency-bound).
template <int NS>
__device__ __forceinline__ void sum_partials(const float* __restrict__ p, int ph, int nblk, int ncol,
                                             double (&s)[kMomentSums]) {
  constexpr int U = 4;
  const size_t step = (size_t)kNormPhases * kMomentSums * ncol;
  int b = ph;
  for (; b + (U - 1) * kNormPhases < nblk; b += U * kNormPhases, p += U * step) {
    float v[U][NS];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < NS; ++k) v[u][k] = p[u * step + (size_t)k * ncol];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < NS; ++k) s[k] += (double)v[u][k];
  }
  for (; b < nblk; b += kNormPhases, p += step)
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] += (double)p[(size_t)k * ncol];
}

// Every phase's sums of column c (local: all four; the DP sums carry the shared shift only)
// into red, then a barrier.
__device__ __forceinline__ void phase_sums(double (&red)[kNormPhases][kMomentSums][128], const float* partials, int nblk,
                                           int ncol, int c, int ph, bool local) {
  double s[kMomentSums] = {0.0, 0.0, 0.0, 0.0};
  if (c < ncol) {
    const float* p = partials + (size_t)ph * kMomentSums * ncol + c;
    if (local) sum_partials<kMomentSums>(p, ph, nblk, ncol, s);
    else sum_partials<2>(p, ph, nblk, ncol, s);
  }
#pragma unroll
  for (int k = 0; k < kMomentSums; ++k) red[ph][k][c] = s[k];
  __syncthreads();
}

// The phase sums of column c added in phase order.
__device__ __forceinline__ void column_sums(const double (&red)[kNormPhases][kMomentSums][128], int c,
                                            double (&S)[kMomentSums]) {
  for (int q = 0; q < kNormPhases; ++q)
#pragma unroll
    for (int k = 0; k < kMomentSums; ++k) S[k] += red[q][k][c];
}

struct BatchMoments {
  float mean, var;
};

// Batch mean / variance of a column over n rows from its sums S. local: S[2], S[3] are the sums
// under the row-0 shift *row0 (read only where that pair is taken); otherwise S[0], S[1] alone.
__device__ __forceinline__ BatchMoments batch_moments(const double (&S)[kMomentSums], int n, float shift,
                                                      const float* row0, bool local) {
  const double m = S[0] / n;
  double var = S[1] / n - m * m;
  if (var < 0.0) var = 0.0;
  BatchMoments b{(float)((double)shift + m), (float)var};
  if (local) {
    const double m0 = S[2] / n;
    double var0 = S[3] / n - m0 * m0;
    if (var0 < 0.0) var0 = 0.0;
    if (fabs(var - var0) > kMomentRtol * var0) {
      b.mean = (float)((double)*row0 + m0);
      b.var = (float)var0;
    }
  }
  return b;
}

}  // namespace ia
