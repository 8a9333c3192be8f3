// One-shot all-reduce for small data-parallel buckets over xGMI.
//
// The reference has no distributed code; the DP runtime of this framework
// reduces KB-sized buckets -- discriminator gradients (~5 KB), normaliser moment sums
// (<1 KB), PPO statistics -- several times per GAIL round.  A ring all-reduce over the
// point-to-point xGMI mesh costs 2(W-1) latency-bound hops for such a message.  Here every
// rank instead maps every peer's staging region (IPC handles exchanged once), so one
// kernel does the whole collective in ONE hop:
//
//   1. stage   : this rank's (pre-scaled) bucket -> its own staging slot (parity = gen & 1)
//   2. signal  : vmcnt drain + barrier + system-scope release, then `gen` into flag[block][rank]
//                of every peer (MI355X_MICROARCH: inter-workgroup visibility, compiler hazard)
//   3. wait    : relaxed polls (bounded, wall clock) until flag[block][r] >= gen for every r,
//                then one system-scope acquire per block
//   4. reduce  : read slot `parity` of ranks 0..W-1 in rank order, sum, store
//
// fp32 buckets (gradients) and fp64 ones (normaliser column sums) use the same byte-sized
// slices. Blocks are independent (block b owns a FIXED slice of the staging region -- vectors
// [b * per, (b + 1) * per) with per = stage_vectors / kOneShotMaxBlocks, whatever the
// bucket size -- and its own flag row / generation counter), so no inter-block
// synchronisation is needed and partial residency cannot deadlock.  Two staging parities
// make a start-barrier sufficient: a peer's block b can be at most one generation ahead of
// this rank's block b (it needs this rank's block-b flag for gen+1, written only after this
// block finished reading gen), and gen+1 stages into the other parity.  Because the slice
// of block b never depends on the call's size, a block only ever reads staging bytes that
// peers' block b writes: calls that launch fewer blocks leave the higher blocks' counters
// behind without letting two blocks with different parities share bytes.  The generation counter
// lives in device memory, so the launch is graph-capture safe.  Summation order is rank
// order on every rank -> results are bitwise identical across ranks.
//
// The wait is bounded: past `timeout_ticks` of wall clock the block writes NaN into its
// slice of the output and raises the error word, so a lost peer shows up as a NaN / a
// host-visible error instead of a hung GPU.
//
// The one MB-sized bucket of the DP runtime has a kernel of its own further down: the
// two-phase (reduce-scatter + all-gather) all-reduce, same hand-off, same bounded waits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "launchers.h"

namespace ia {
namespace {

constexpr size_t kFlagOff = 0;      // [kOneShotMaxBlocks][kOneShotMaxRanks] uint32, written by peers
constexpr size_t kCntOff = 4096;    // [kOneShotMaxBlocks] uint32 generation counters, local only
constexpr size_t kErrOff = 4096 + 512;
constexpr size_t kDataOff = 8192;   // 2 x stage_bytes staging slots
constexpr int kThreads = 256;

// vectors per block slice: the staging region split into kOneShotMaxBlocks fixed slices
// (at least one 256-thread pass each)
__host__ __device__ __forceinline__ int oneshot_block_vectors(size_t stage_bytes) {
  const size_t sv = stage_bytes / 16;
  const size_t per = (sv + kOneShotMaxBlocks - 1) / kOneShotMaxBlocks;
  return per < (size_t)kThreads ? kThreads : (int)per;
}

__device__ __forceinline__ void store_release_sys(unsigned* p, unsigned v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned load_relaxed_sys(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// 16-byte staging vector of T (float4 / double2): the slice geometry is in bytes, so fp32
// gradients and fp64 normaliser sums share the region and its per-block slices.
template <typename T>
struct alignas(16) Vec16 {
  static constexpr int kN = 16 / sizeof(T);
  T e[kN];
};

template <typename T>
__global__ __launch_bounds__(kThreads) void oneshot_allreduce_kernel(OneShotArgs a) {
  using V = Vec16<T>;
  constexpr int EPV = V::kN;
  __shared__ unsigned s_gen;
  __shared__ int s_fail;
  const int b = blockIdx.x, tid = threadIdx.x;
  char* me = a.base[a.rank];
  unsigned* cnt = reinterpret_cast<unsigned*>(me + kCntOff) + b;
  if (tid == 0) {
    const unsigned g = *cnt + 1u;
    *cnt = g;
    s_gen = g;
    s_fail = 0;
  }
  __syncthreads();
  const unsigned gen = s_gen;
  const size_t par = (gen & 1u) ? a.stage_bytes : 0;
  const T scale = (T)a.scale;
  const T* in = reinterpret_cast<const T*>(a.in);
  T* out = reinterpret_cast<T*>(a.out);

  // fixed slice of 16-byte vectors owned by this block (the n % EPV tail belongs to the
  // block whose slice holds vector nv)
  const int nv = a.n / EPV;
  const int per = oneshot_block_vectors(a.stage_bytes);
  const int v0 = min(nv, b * per), v1 = min(nv, v0 + per);
  const bool tail_owner = b == nv / per;
  const int tail0 = nv * EPV;

  // 1. stage
  T* st = reinterpret_cast<T*>(me + kDataOff + par);
  const V* in4 = reinterpret_cast<const V*>(in);
  V* st4 = reinterpret_cast<V*>(st);
  for (int v = v0 + tid; v < v1; v += kThreads) {
    V x = in4[v];
#pragma unroll
    for (int i = 0; i < EPV; ++i) x.e[i] *= scale;
    st4[v] = x;
  }
  if (tail_owner && tid < a.n - tail0) st[tail0 + tid] = in[tail0 + tid] * scale;
  // every storing wave drains its stores before the barrier; the signalling lanes then
  // release at system scope and wait again (the compiler may drop the fence's own wait)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // 2. signal every rank (self included), 3. wait for every rank: relaxed polls, then ONE
  // system-scope acquire per block
  if (tid < a.world) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(reinterpret_cast<unsigned*>(a.base[tid] + kFlagOff) + b * kOneShotMaxRanks + a.rank, gen,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned* f = reinterpret_cast<const unsigned*>(me + kFlagOff) + b * kOneShotMaxRanks + tid;
    const long long t0 = wall_clock64();
    while ((int)(load_relaxed_sys(f) - gen) < 0) {
      if (wall_clock64() - t0 > a.timeout_ticks) {
        s_fail = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope: peers' staged data is visible
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  if (s_fail) {
    const T nan = (T)__builtin_nanf("");
    for (int v = v0 + tid; v < v1; v += kThreads) {
      V x;
#pragma unroll
      for (int i = 0; i < EPV; ++i) x.e[i] = nan;
      reinterpret_cast<V*>(out)[v] = x;
    }
    if (tail_owner && tid < a.n - tail0) out[tail0 + tid] = nan;
    if (tid == 0) store_release_sys(reinterpret_cast<unsigned*>(me + kErrOff), 1u);
    return;
  }

  // 4. reduce in rank order (identical on every rank)
  for (int v = v0 + tid; v < v1; v += kThreads) {
    V acc = reinterpret_cast<const V*>(a.base[0] + kDataOff + par)[v];
    for (int r = 1; r < a.world; ++r) {
      const V x = reinterpret_cast<const V*>(a.base[r] + kDataOff + par)[v];
#pragma unroll
      for (int i = 0; i < EPV; ++i) acc.e[i] += x.e[i];
    }
    reinterpret_cast<V*>(out)[v] = acc;
  }
  if (tail_owner && tid < a.n - tail0) {
    T acc = reinterpret_cast<const T*>(a.base[0] + kDataOff + par)[tail0 + tid];
    for (int r = 1; r < a.world; ++r) acc += reinterpret_cast<const T*>(a.base[r] + kDataOff + par)[tail0 + tid];
    out[tail0 + tid] = acc;
  }
}


// ---- two-phase all-reduce (reduce-scatter + all-gather) for MB-sized buckets -------------
//
// The one-shot kernel makes every rank read every peer's whole bucket: (W - 1) x bytes per
// rank.  For the one MB-sized bucket of the DP runtime (the NatureCNN gradient of DP BC) this
// kernel moves 2 (W - 1) / W x bytes per rank instead, in one launch over a slot of the
// bucket's size.  Block b owns the same kind of FIXED slice of 16-byte vectors as above
// ([b * per, (b + 1) * per), per = slot_vectors / kTwoPhaseMaxBlocks, whatever the call's
// size); inside it the slice [v0, v1) of the call is cut into `world` contiguous shards
// (twophase_shard_bounds; empty when the slice has fewer vectors than ranks), rank r owning
// shard r.  The n % EPV scalar tail is reduced by rank 0 in the block whose slice holds it.
//
//   1. stage    : in * scale for the block's slice -> this rank's staging area
//   2. hand-off : the one-shot kernel's, link for link, on flag row 1
//   3. reduce   : rank r sums shard r over the staging areas of ranks 0..W-1 in rank order
//                 -> out and this rank's result area
//   4. hand-off : the same on flag row 2
//   5. gather   : for q != r, rank q's reduced shard q from q's result area -> out
//
// Region: [flag row 1][generation counters][error word][flag row 2][staging][result]; the
// first three sit where the one-shot region has them, so the error-word helpers are shared.
//
// ONE staging area and ONE result area are enough (no parities).  A rank's calls on one
// communicator are stream ordered, so its block b of call g+1 starts after its block b of
// call g has ended, loads and stores included.  (a) Staging: block b of call g+1 overwrites
// this rank's slice b of the staging area.  Peers read those bytes only in their step 3 of
// call g, and each signals row 2 after that step (behind its waves' vmcnt drain).  This block
// left call g only after wait 2 saw every peer's row-2 flag of g -- this kernel RELIES on
// wait 2 for that -- so no peer is still reading what stage g+1 overwrites.  (b) Result:
// block b of call g+1 overwrites its shard of the result area in step 3, behind wait 1 of
// g+1 -- this kernel RELIES on wait 1 of the next call here.  A peer signals row 1 of g+1
// only from its own block b of call g+1, which starts after its block b of call g, whose step
// 5 held its last read of this rank's result, has ended.  So a peer's block b is never further
// ahead of this rank's block b than its stage + signal 1 of the next call, which touch only
// the peer's own staging area (free by (a)) and flags this block polls with >=.  A block that
// timed out returns without signalling; its peers time out in the same call (step 2 or 4),
// and the host stops the run on the error word -- nothing is promised about data after that,
// but every access stays inside the slice.
// Calls that launch different block counts: slice b of both areas, flag rows b and counter b
// are touched by block b alone, on every rank (all ranks pass the same n, hence the same
// grid).  A call with fewer blocks leaves the higher blocks' counters behind equally on all
// ranks, and a byte of slice b only ever holds generations of counter b, which (a) and (b)
// order one after the other: two generations never share bytes.
//
// Blocks per launch are capped at kTwoPhaseMaxBlocks = 128: with 8 ranks rehearsed on ONE
// card, 8 x 128 x 256 spinning threads are half of the 256 CUs x 2048 resident threads, so a
// peer's grid always finds room and the bounded waits cannot starve it.

constexpr size_t kFlag2Off = 8192;      // [kTwoPhaseMaxBlocks][kOneShotMaxRanks] uint32 (row 1: kFlagOff)
constexpr size_t kTwoDataOff = 16384;   // staging (slot_bytes), then result (slot_bytes)
static_assert(kTwoPhaseMaxBlocks * kOneShotMaxRanks * 4 <= (int)(kCntOff - kFlagOff), "flag row 1");
static_assert(kTwoPhaseMaxBlocks * 4 <= (int)(kErrOff - kCntOff), "generation counters");
static_assert(kTwoPhaseMaxBlocks * kOneShotMaxRanks * 4 <= (int)(kTwoDataOff - kFlag2Off), "flag row 2");

__host__ __device__ __forceinline__ int twophase_block_vectors(size_t slot_bytes) {
  const size_t sv = slot_bytes / 16;
  const size_t per = (sv + kTwoPhaseMaxBlocks - 1) / kTwoPhaseMaxBlocks;
  return per < (size_t)kThreads ? kThreads : (int)per;
}

// shard r of the slice [v0, v1) cut into `world` contiguous runs of whole vectors
__host__ __device__ __forceinline__ void twophase_shard_bounds(int v0, int v1, int world, int r, int* lo, int* hi) {
  const long long len = v1 - v0;
  *lo = v0 + (int)(len * r / world);
  *hi = v0 + (int)(len * (r + 1) / world);
}

// The one-shot kernel's hand-off on flag row `flag_off` (the callers' storing waves have
// drained their stores and passed a barrier): release + wait, `gen` into every rank's flag
// of this block, bounded relaxed polls, one system-scope acquire, barrier.
__device__ __forceinline__ void twophase_handoff(const TwoPhaseArgs& a, size_t flag_off, int b, int tid, unsigned gen,
                                                 int* s_fail) {
  if (tid < a.world) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(reinterpret_cast<unsigned*>(a.base[tid] + flag_off) + b * kOneShotMaxRanks + a.rank, gen,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned* f = reinterpret_cast<const unsigned*>(a.base[a.rank] + flag_off) + b * kOneShotMaxRanks + tid;
    const long long t0 = wall_clock64();
    while ((int)(load_relaxed_sys(f) - gen) < 0) {
      if (wall_clock64() - t0 > a.timeout_ticks) {
        *s_fail = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope: peers' stores are visible
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kThreads) void twophase_allreduce_kernel(TwoPhaseArgs a) {
  using V = Vec16<T>;
  constexpr int EPV = V::kN;
  __shared__ unsigned s_gen;
  __shared__ int s_fail;
  const int b = blockIdx.x, tid = threadIdx.x;
  char* me = a.base[a.rank];
  unsigned* cnt = reinterpret_cast<unsigned*>(me + kCntOff) + b;
  if (tid == 0) {
    const unsigned g = *cnt + 1u;
    *cnt = g;
    s_gen = g;
    s_fail = 0;
  }
  __syncthreads();
  const unsigned gen = s_gen;
  const T scale = (T)a.scale;
  const T* in = reinterpret_cast<const T*>(a.in);
  T* out = reinterpret_cast<T*>(a.out);
  V* out4 = reinterpret_cast<V*>(out);
  const size_t res_off = kTwoDataOff + a.slot_bytes;

  // fixed slice of this block, this rank's shard of it; the tail belongs to rank 0 of the
  // block whose slice holds vector nv
  const int nv = a.n / EPV;
  const int per = twophase_block_vectors(a.slot_bytes);
  const int v0 = min(nv, b * per), v1 = min(nv, v0 + per);
  const bool tail_block = b == nv / per;
  const int tail0 = nv * EPV;
  const bool has_tail = tail_block && tid < a.n - tail0;
  int s0, s1;
  twophase_shard_bounds(v0, v1, a.world, a.rank, &s0, &s1);

  // 1. stage the whole slice
  T* st = reinterpret_cast<T*>(me + kTwoDataOff);
  const V* in4 = reinterpret_cast<const V*>(in);
  V* st4 = reinterpret_cast<V*>(st);
  for (int v = v0 + tid; v < v1; v += kThreads) {
    V x = in4[v];
#pragma unroll
    for (int i = 0; i < EPV; ++i) x.e[i] *= scale;
    st4[v] = x;
  }
  if (has_tail) st[tail0 + tid] = in[tail0 + tid] * scale;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // 2. signal 1 / wait 1
  twophase_handoff(a, kFlagOff, b, tid, gen, &s_fail);

  if (!s_fail) {
    // 3. reduce-scatter: this rank's shard in rank order -> out and the result area
    V* res4 = reinterpret_cast<V*>(me + res_off);
    for (int v = s0 + tid; v < s1; v += kThreads) {
      V acc = reinterpret_cast<const V*>(a.base[0] + kTwoDataOff)[v];
      for (int r = 1; r < a.world; ++r) {
        const V x = reinterpret_cast<const V*>(a.base[r] + kTwoDataOff)[v];
#pragma unroll
        for (int i = 0; i < EPV; ++i) acc.e[i] += x.e[i];
      }
      out4[v] = acc;
      res4[v] = acc;
    }
    if (has_tail && a.rank == 0) {
      T acc = reinterpret_cast<const T*>(a.base[0] + kTwoDataOff)[tail0 + tid];
      for (int r = 1; r < a.world; ++r) acc += reinterpret_cast<const T*>(a.base[r] + kTwoDataOff)[tail0 + tid];
      out[tail0 + tid] = acc;
      reinterpret_cast<T*>(me + res_off)[tail0 + tid] = acc;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // 4. signal 2 / wait 2
    twophase_handoff(a, kFlag2Off, b, tid, gen, &s_fail);
  }

  if (s_fail) {
    const T nan = (T)__builtin_nanf("");
    for (int v = v0 + tid; v < v1; v += kThreads) {
      V x;
#pragma unroll
      for (int i = 0; i < EPV; ++i) x.e[i] = nan;
      out4[v] = x;
    }
    if (has_tail) out[tail0 + tid] = nan;
    if (tid == 0) store_release_sys(reinterpret_cast<unsigned*>(me + kErrOff), 1u);
    return;
  }

  // 5. all-gather: the peers' reduced shards
  for (int q = 0; q < a.world; ++q) {
    if (q == a.rank) continue;
    int q0, q1;
    twophase_shard_bounds(v0, v1, a.world, q, &q0, &q1);
    const V* src = reinterpret_cast<const V*>(a.base[q] + res_off);
    for (int v = q0 + tid; v < q1; v += kThreads) out4[v] = src[v];
  }
  if (has_tail && a.rank != 0) out[tail0 + tid] = reinterpret_cast<const T*>(a.base[0] + res_off)[tail0 + tid];
}

}  // namespace

size_t oneshot_region_bytes(size_t stage_bytes) { return kDataOff + 2 * stage_bytes; }

int oneshot_blocks(int n, size_t stage_bytes, int elem_bytes) {
  const int epv = 16 / elem_bytes;
  const int nv = (n + epv - 1) / epv;
  const int per = oneshot_block_vectors(stage_bytes);
  const int blocks = (nv + per - 1) / per;
  return blocks < 1 ? 1 : blocks;  // <= kOneShotMaxBlocks since n * 4 <= stage_bytes
}

hipError_t oneshot_alloc(size_t stage_bytes, void** ptr, void* handle) {
  return oneshot_alloc_region(oneshot_region_bytes(stage_bytes), ptr, handle);
}

hipError_t oneshot_alloc_region(size_t bytes, void** ptr, void* handle) {
  hipError_t e = hipExtMallocWithFlags(ptr, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) return e;
  e = hipMemset(*ptr, 0, bytes);
  if (e != hipSuccess) return e;
  e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  hipIpcMemHandle_t h;
  e = hipIpcGetMemHandle(&h, *ptr);
  if (e != hipSuccess) return e;
  memcpy(handle, &h, sizeof(h));
  return hipSuccess;
}

size_t oneshot_handle_bytes() { return sizeof(hipIpcMemHandle_t); }

hipError_t oneshot_open(const void* handle, void** ptr) {
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  return hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess);
}

hipError_t oneshot_close(void* ptr) { return hipIpcCloseMemHandle(ptr); }
hipError_t oneshot_free(void* ptr) { return hipFree(ptr); }

hipError_t oneshot_read_error(void* local, int* err) {
  unsigned v = 0;
  hipError_t e = hipMemcpy(&v, static_cast<char*>(local) + kErrOff, sizeof(v), hipMemcpyDeviceToHost);
  *err = (int)v;
  return e;
}

hipError_t oneshot_read_error_async(void* local, int* host_pinned, hipStream_t s) {
  return hipMemcpyAsync(host_pinned, static_cast<char*>(local) + kErrOff, sizeof(unsigned), hipMemcpyDeviceToHost, s);
}

hipError_t oneshot_clear_error(void* local) { return hipMemset(static_cast<char*>(local) + kErrOff, 0, sizeof(unsigned)); }

long long oneshot_ticks_per_second() {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 100000000LL;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) return 100000000LL;
  return (long long)khz * 1000LL;
}

hipError_t oneshot_allreduce(const OneShotArgs& a, hipStream_t s) {
  if (a.world < 1 || a.world > kOneShotMaxRanks || a.rank < 0 || a.rank >= a.world) return hipErrorInvalidValue;
  const int eb = a.f64 ? 8 : 4;
  if ((size_t)a.n * eb > a.stage_bytes) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out)) & 15) return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  const dim3 g(oneshot_blocks(a.n, a.stage_bytes, eb));
  if (a.f64)
    hipLaunchKernelGGL(oneshot_allreduce_kernel<double>, g, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(oneshot_allreduce_kernel<float>, g, dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

size_t twophase_region_bytes(size_t slot_bytes) { return kTwoDataOff + 2 * slot_bytes; }

int twophase_blocks(int n, size_t slot_bytes, int elem_bytes) {
  const int epv = 16 / elem_bytes;
  const int nv = (n + epv - 1) / epv;
  const int per = twophase_block_vectors(slot_bytes);
  const int blocks = (nv + per - 1) / per;
  return blocks < 1 ? 1 : blocks;  // <= kTwoPhaseMaxBlocks since n * elem_bytes <= slot_bytes
}

void twophase_shard(int v0, int v1, int world, int r, int* lo, int* hi) { twophase_shard_bounds(v0, v1, world, r, lo, hi); }

hipError_t twophase_allreduce(const TwoPhaseArgs& a, hipStream_t s) {
  if (a.world < 1 || a.world > kOneShotMaxRanks || a.rank < 0 || a.rank >= a.world) return hipErrorInvalidValue;
  const int eb = a.f64 ? 8 : 4;
  if (a.n < 0 || (size_t)a.n * eb > a.slot_bytes) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out)) & 15) return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  const dim3 g(twophase_blocks(a.n, a.slot_bytes, eb));
  if (g.x > (unsigned)kTwoPhaseMaxBlocks) return hipErrorInvalidValue;
  if (a.f64)
    hipLaunchKernelGGL(twophase_allreduce_kernel<double>, g, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(twophase_allreduce_kernel<float>, g, dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace ia
