// Device-resident DQN / SQIL collection (imitation_amd/ops/dqn.py, engine/dqn.py): K steps of
// epsilon-greedy acting, env physics and replay-ring writes for N native vector envs in ONE launch.
//
// The host loop (rl/off_policy.py collect_rollouts) pays per env step a Q forward with a host
// round trip for the action, NativeVecEnv.step and ReplayBuffer.add (six small copies). Here one
// wave owns one env for the whole launch: per step it evaluates the Q-network from the online flat
// bucket (lane j owns output j, the inputs are broadcast lane by lane, fp32 fmaf with k ascending:
// equal states give equal bits), takes the lowest index of the wave maximum, flips the exploration
// coin on the env's action stream (integer-exact splitmix64 draws, separate from the env's own
// stream), steps the env with the IA_HD physics the host BatchedEnv runs (the statements of
// dagger_env_kernel: step, TimeLimit, observation; on episode end the terminal observation, reset
// and the reset observation) and writes the transition into the replay ring.
//
// The three weight matrices are staged once per workgroup into LDS as [k][j] (row stride 65: the
// staging writes and the per-k row reads are both conflict free); that staging is the only place
// with a workgroup barrier. No wave waits on another one after it, nothing here waits on another
// workgroup, and there is no spin loop.
#include <hip/hip_runtime.h>

#include "ia/wave.h"
#include "launchers.h"

namespace ia {
namespace {

constexpr int kWaves = 4;  // envs per workgroup
constexpr int kT = 64 * kWaves;
constexpr int kWS = 65;    // staged weight row stride

// sW[k][j] = W[j][k] for the row-major W [R][C]
__device__ __forceinline__ void stage(int tid, const float* __restrict__ W, int R, int C, float* sW) {
  for (int e = tid; e < R * C; e += kT) {
    const int r = e / C, c = e - r * C;
    sW[c * kWS + r] = W[e];
  }
}

// lane j: f(b_j + sum_k x_k * sW[k][j]), k ascending; x_k sits in lane k. Lanes >= nout give 0.
template <bool RELU>
__device__ __forceinline__ float layer(float x, const float* sW, float b, int red, int nout, int lane) {
  float acc = b;
  for (int k = 0; k < red; ++k) acc = __builtin_fmaf(bcast(x, k), sW[k * kWS + lane], acc);
  if (RELU) acc = fmaxf(acc, 0.f);
  return lane < nout ? acc : 0.f;
}

__global__ __launch_bounds__(kT) void dqn_collect_kernel(DqnCollectArgs a) {
  __shared__ float sW1[64 * kWS], sW2[64 * kWS], sW3[64 * kWS];
  __shared__ float sState[kWaves][kMaxState];
  __shared__ float sNext[kWaves][64], sReset[kWaves][64];
  __shared__ float sAct[kWaves][kMaxJoints];
  __shared__ int sDone[kWaves];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x * kWaves + w;
  const int N = a.N, D = a.D, H1 = a.H1, H2 = a.H2, A = a.A;
  const float* P = a.params;
  // (the online weights do not change inside a launch)
  stage(tid, P + a.off[0], H1, D, sW1);
  stage(tid, P + a.off[2], H2, H1, sW2);
  stage(tid, P + a.off[4], A, H2, sW3);
  __syncthreads();
  if (n >= N) return;  // (wave uniform: the ragged last workgroup)

  const float b1 = lane < H1 ? P[a.off[1] + lane] : 0.f;
  const float b2 = lane < H2 ? P[a.off[3] + lane] : 0.f;
  const float b3 = lane < A ? P[a.off[5] + lane] : 0.f;
  float* st = sState[w];
  if (lane < a.sdim) st[lane] = a.state[(size_t)n * a.sdim + lane];
  float x = lane < D ? a.cur_obs[(size_t)n * D + lane] : 0.f;
  uint64_t er = a.rng[n];      // the env's stream (lane 0's copy advances)
  uint64_t ar = a.act_rng[n];  // the action stream (wave uniform)
  int el = a.elapsed[n];
  float ret = a.ep_ret[n];
  wave_sync();

  for (int t = 0; t < a.K; ++t) {
    // ---- Q forward
    const float h1 = layer<true>(x, sW1, b1, D, H1, lane);
    const float h2 = layer<true>(h1, sW2, b2, H1, H2, lane);
    const float q = layer<false>(h2, sW3, b3, H2, A, lane);
    const bool in = lane < A;
    const size_t kn = (size_t)t * N + n;
    if (a.rec_q != nullptr && in) a.rec_q[kn * A + lane] = q;

    // ---- greedy action: the lowest index attaining the wave maximum (a non-finite Q: error bit, action 0)
    const bool bad = __ballot(in && !(fabsf(q) <= 3.402823466e38f)) != 0ull;
    const float m = wave_max(in ? q : -INFINITY);
    const unsigned long long hit = __ballot(in && q == m);
    const int greedy = (bad || hit == 0ull) ? 0 : (int)__builtin_ctzll(hit);
    if (bad && lane == 0) atomicOr(a.err, 1);

    // ---- epsilon-greedy on the action stream: the coin, and only when exploring the action
    const uint32_t u = (uint32_t)(splitmix64(ar) >> 40);
    const bool explore = u < a.thr[t];
    int action = greedy;
    if (explore) {
      const uint32_t v = (uint32_t)(splitmix64(ar) >> 40);
      action = (int)((v * (uint32_t)A) >> 24);
    }

    // ---- env step, TimeLimit, episode end (BatchedEnv::step) and the row's scalars
    const int slot = (a.pos0 + t) % a.S;
    const size_t row = (size_t)slot * N + n;
    if (lane == 0) {
      sAct[w][0] = (float)action;
      int term = 0;
      const float rew = env_step(a.P, st, sAct[w], &term, er);
      const int tt = el + 1;
      const bool trunc = !term && a.max_steps > 0 && tt >= a.max_steps;
      const float r2 = ret + rew;
      const bool done = term || trunc;
      env_obs(a.P, st, sNext[w]);
      if (done) {
        env_reset(a.P, st, er);
        env_obs(a.P, st, sReset[w]);
      }
      el = done ? 0 : tt;
      ret = done ? 0.f : r2;
      sDone[w] = done;
      a.r_action[row] = action;
      a.r_reward[row] = a.use_reward_const ? a.reward_const : rew;
      a.r_done[row] = done ? 1.f : 0.f;
      if (a.r_timeout != nullptr) a.r_timeout[row] = trunc ? 1.f : 0.f;
      a.rec_done[kn] = done ? 1.f : 0.f;
      a.rec_ep_ret[kn] = done ? r2 : 0.f;
      a.rec_ep_len[kn] = done ? tt : 0;
      a.rec_action[kn] = action;
      if (a.rec_explore != nullptr) a.rec_explore[kn] = explore ? 1 : 0;
    }
    wave_sync();

    // ---- the row's observations: obs before the step, next_obs the terminal one on episode end
    const bool done = sDone[w] != 0;
    float nx = 0.f, rx = 0.f;
    if (lane < D) {
      nx = sNext[w][lane];
      if (done) rx = sReset[w][lane];
      a.r_obs[row * D + lane] = x;
      a.r_next[row * D + lane] = nx;
    }
    x = done ? rx : nx;
    wave_sync();  // (lane 0 rewrites sNext / sDone in the next step)
  }

  if (lane < a.sdim) a.state[(size_t)n * a.sdim + lane] = st[lane];
  if (lane < D) a.cur_obs[(size_t)n * D + lane] = x;
  if (lane == 0) {
    a.rng[n] = er;
    a.act_rng[n] = ar;
    a.elapsed[n] = el;
    a.ep_ret[n] = ret;
  }
}

}  // namespace

hipError_t dqn_collect(const DqnCollectArgs& a, hipStream_t s) {
  auto dim_ok = [](int d) { return d >= 1 && d <= kDqnTdMaxDim; };
  if (a.K < 1 || a.K > kDqnCollectMaxSteps || a.N < 1) return hipErrorInvalidValue;
  if (!dim_ok(a.D) || !dim_ok(a.H1) || !dim_ok(a.H2) || !dim_ok(a.A)) return hipErrorInvalidValue;
  if (a.P.kind == ENV_PONG || a.P.n_actions <= 0 || a.P.n_actions != a.A || a.P.obs_dim != a.D) return hipErrorInvalidValue;
  if (a.sdim != state_size(a.P) || a.sdim < 1 || a.sdim > kMaxState) return hipErrorInvalidValue;
  if (a.S < 1 || a.pos0 < 0 || a.pos0 >= a.S || a.max_steps < 0) return hipErrorInvalidValue;
  for (int t = 0; t < a.K; ++t)
    if (a.thr[t] > (1u << 24)) return hipErrorInvalidValue;
  const int sizes[6] = {a.H1 * a.D, a.H1, a.H2 * a.H1, a.H2, a.A * a.H2, a.A};
  for (int i = 0; i < 6; ++i)
    if (a.off[i] < 0 || (int64_t)a.off[i] + sizes[i] > a.n) return hipErrorInvalidValue;
  if (!(a.params && a.state && a.rng && a.elapsed && a.ep_ret && a.cur_obs && a.act_rng && a.err)) return hipErrorInvalidValue;
  if (!(a.r_obs && a.r_next && a.r_action && a.r_reward && a.r_done)) return hipErrorInvalidValue;
  if (!(a.rec_done && a.rec_ep_ret && a.rec_ep_len && a.rec_action)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dqn_collect_kernel, dim3((a.N + kWaves - 1) / kWaves), dim3(kT), 0, s, a);
  return hipGetLastError();
}

}  // namespace ia
