// Register-chained PPO update: the parallel prep kernel, host planning and the launch.
// The kernel template is ppo_rc_kernel.h; its compiled instances are the rows of the table in
// ppo_rc_instances.h (compiled in ppo_rc_inst_*.hip, declared extern below). ppo_rc_plan picks
// the first row whose compile-time constants fit the shape (rc_select) and takes the slot caps,
// waves and weight-image format of the plan from that row; ppo_rc_launch runs the row's kernel.
#include <stdio.h>

#include "ppo_rc_kernel.h"
#include "ppo_rc_instances.h"

namespace ia {
namespace rc {

IA_RC_TABLE(IA_RC_EXTERN)

// ---------------------------------------------------------------- prep (parallel over minibatches)
// One workgroup per minibatch k = epoch * n_mb + mb, one wave per chunk (looping when the
// minibatch has more chunks than waves), one lane per row. Minibatch statistics (obs
// moments, advantage mean / std) are exact two-pass reductions over all its rows.
constexpr int kPrepWaves = 16;
constexpr int kPrepBatch = 16;  // obs loads of a row issued back to back (launch bounds: <= 128 VGPRs)

__device__ __forceinline__ int prep_idx(const PPOArgs& a, const PPORcGeo& g, int e, int mb, int c, int lane) {
  const int Bg = g.G * g.nch * g.cw;
  return a.perm[(size_t)e * a.rows + (size_t)mb * Bg + (size_t)c * g.cw + lane];
}

__global__ __launch_bounds__(64 * kPrepWaves) void ppo_rc_prep_kernel(PPOArgs a, PPORcGeo g) {
  __shared__ float red[kPrepWaves][64];
  __shared__ float stat[2][64];
  __shared__ float adv_stat[2];
  __shared__ float red_a[kPrepWaves];
  const int k = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int CH = g.G * g.nch, cw = g.cw, Bg = CH * cw, D = a.D;
  // the main kernel's arrival counters / flags start at zero (stream order: it runs after
  // this launch) -- replaces a separate memset launch per update
  if (k == 0 && threadIdx.x < 64) g.sync[threadIdx.x] = 0u;
  if (k == 0 && a.zero_stats && threadIdx.x < 5) a.stats[threadIdx.x] = 0.f;  // (and the stats)
  const int n_mb = a.rows / Bg;
  const int e = k / n_mb, mb = k - e * n_mb;
  const bool ok = lane < cw;
  // ---- pass 1: gather, feature sums, advantage sum
  float fs = 0.f, as = 0.f;  // lane c: this wave's sum of feature c; as: advantage sum (lane 0)
  for (int c = wv; c < CH; c += nw) {
    const int idx = ok ? prep_idx(a, g, e, mb, c, lane) : 0;
    const size_t slot = (size_t)k * CH + c;
    float* xr = g.xraw + (slot * 64 + lane) * g.dp;
    // batches of kPrepBatch features: all of a batch's loads are issued before its first store
    // (a store to xraw between two obs loads serialises them -- the buffers may alias as far as
    // the compiler knows: ~20 dependent L2 round trips per row before)
    for (int f0 = 0; f0 < g.dp; f0 += kPrepBatch) {
      float xv[kPrepBatch];
#pragma unroll
      for (int i = 0; i < kPrepBatch; ++i) xv[i] = (ok && f0 + i < D) ? a.obs[(size_t)idx * D + f0 + i] : 0.f;
#pragma unroll
      for (int i = 0; i < kPrepBatch; ++i) {
        const int f = f0 + i;
        if (f < g.dp) {
          if (ok) xr[f] = xv[i];
          if (f < D && a.has_norm) {
            const float s = wave_sum(xv[i]);
            if (lane == f) fs += s;
          }
        }
      }
    }
    float av16[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float v = 0.f;
      if (ok) {
        if (a.discrete) v = j == 0 ? a.acts[idx] : 0.f;
        else v = j < a.A ? a.acts[(size_t)idx * a.A + j] : 0.f;
      }
      av16[j] = v;
    }
    const float adv = ok ? a.adv[idx] : 0.f;
    float* ac = g.acts + (slot * 64 + lane) * 16;
    if (ok)
#pragma unroll
      for (int j = 0; j < 16; ++j) ac[j] = av16[j];
    as += wave_sum(adv);
  }
  red[wv][lane] = fs;
  if (lane == 0) red_a[wv] = as;
  __syncthreads();
  if (wv == 0) {
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i][lane];
    stat[0][lane] = s / (float)Bg;
    if (lane == 0) {
      float t = 0.f;
      for (int i = 0; i < nw; ++i) t += red_a[i];
      adv_stat[0] = t / (float)Bg;
    }
  }
  __syncthreads();
  const float am = adv_stat[0];
  // ---- pass 2: centred second moments
  float fv = 0.f, av = 0.f;
  for (int c = wv; c < CH; c += nw) {
    const int idx = ok ? prep_idx(a, g, e, mb, c, lane) : 0;
    if (a.has_norm) {
      for (int f0 = 0; f0 < D; f0 += kPrepBatch) {  // (batched loads, as in pass 1)
        float xv[kPrepBatch];
#pragma unroll
        for (int i = 0; i < kPrepBatch; ++i) xv[i] = (ok && f0 + i < D) ? a.obs[(size_t)idx * D + f0 + i] : 0.f;
#pragma unroll
        for (int i = 0; i < kPrepBatch; ++i) {
          const int f = f0 + i;
          if (f < D) {
            const float d = ok ? xv[i] - stat[0][f] : 0.f;
            const float s = wave_sum(d * d);
            if (lane == f) fv += s;
          }
        }
      }
    }
    const float d = ok ? a.adv[idx] - am : 0.f;
    av += wave_sum(d * d);
  }
  __syncthreads();
  red[wv][lane] = fv;
  __syncthreads();
  if (wv == 0) {
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i][lane];
    stat[1][lane] = s / (float)Bg;
  }
  __syncthreads();
  if (lane == 0) red_a[wv] = av;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red_a[i];
    adv_stat[1] = sqrtf(s / (float)(Bg > 1 ? Bg - 1 : 1));
  }
  __syncthreads();
  if (a.has_norm && threadIdx.x < D) {
    g.mom[(size_t)k * 128 + threadIdx.x] = stat[0][threadIdx.x];
    g.mom[(size_t)k * 128 + 64 + threadIdx.x] = stat[1][threadIdx.x];
  }
  const float sd = adv_stat[1];
  // ---- pass 3: per-row (old_logp, normalised advantage, return)
  for (int c = wv; c < CH; c += nw) {
    if (!ok) continue;
    const int idx = prep_idx(a, g, e, mb, c, lane);
    float adv = a.adv[idx];
    if (a.normalize_advantage && Bg > 1) adv = (adv - am) / (sd + 1e-8f);
    const size_t slot = (size_t)k * CH + c;
    f4 rd = {a.old_logp[idx], adv, a.returns[idx], 0.f};
    *reinterpret_cast<f4*>(g.rowd + (slot * 64 + lane) * 4) = rd;
  }
}

// Test hook (tests/engine/test_ppo_rc_images.py): an fp32 [rows][feats] matrix goes through the
// update kernel's own image helpers -- stored by 4 row-tile waves as the chain stores a chunk
// (mode 0: img_store4, a lane's four features of a tile; mode 1: img_store1, the layer-0 lane map
// of features 4 s + kk), read back as dw_tiles reads its operands -- and every fragment comes out
// as out[half (hi, lo)][tile][k-step][lane][8] bf16 bit patterns.
constexpr int kProbeMaxRows = 64, kProbeMaxFeats = 64;

__global__ __launch_bounds__(256) void ppo_image_probe_kernel(const float* x, int rows, int feats, int mode, unsigned short* out) {
  __shared__ __attribute__((aligned(16))) float lds[kProbeMaxFeats / 16 * 64 * kProbeMaxRows / 4];
  lf* L = (lf*)lds;
  const int tid = threadIdx.x, gw = tid >> 6, lane = tid & 63, r16 = lane & 15, kk = lane >> 4;
  const int rp = rows > 32 ? 64 : 32, T = feats / 16, ksteps = rp / 32;
  for (int i = tid; i < T * img_strip(rp) / 4; i += 256) L[i] = 0.f;
  __syncthreads();
  const int row = 16 * gw + r16;
  if (row < rows) {
    if (mode == 0) {
      const int st = img_unit(row, kk);
      for (int t = 0; t < T; ++t) {
        const f4 v = *reinterpret_cast<const f4*>(x + (size_t)row * feats + 16 * t + 4 * kk);
        bf16x4 hi, lo;
        split4(v, hi, lo);
        img_store4(L, 0, rp, t, st, hi, lo);
      }
    } else {
      for (int s = 0; s < feats / 4; ++s) img_store1(L, 0, rp, 4 * s + kk, row, x[(size_t)row * feats + 4 * s + kk]);
    }
  }
  __syncthreads();
  // (all lanes of all waves: the transposed reads need EXEC all ones)
  int t0, t1;
  img_lane_terms(r16, kk, t0, t1);
  const int n = T * ksteps;
  for (int i = gw; i < n; i += 4) {  // wave-uniform bounds
    const int t = i / ksteps, ks = i - t * ksteps;
    const lch* p = (const lch*)L + t * img_strip(rp) + kImgKStep * ks + t0;
    const bf16x8 hi = img_read8(p, p + (t1 - t0));
    const bf16x8 lo = img_read8(p + img_lo(rp), p + img_lo(rp) + (t1 - t0));
    bf16x8* oh = reinterpret_cast<bf16x8*>(out) + (size_t)i * 64 + lane;  // (whole fragments: 16-byte stores)
    oh[0] = hi;
    oh[(size_t)n * 64] = lo;
  }
}

}  // namespace rc

using namespace rc;

hipError_t ppo_image_probe_launch(const float* x, int rows, int feats, int mode, unsigned short* out, hipStream_t s) {
  if (rows <= 0 || rows > kProbeMaxRows || rows % 16 != 0 || feats <= 0 || feats > kProbeMaxFeats || feats % 16 != 0 ||
      (mode != 0 && mode != 1))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppo_image_probe_kernel, dim3(1), dim3(256), 0, s, x, rows, feats, mode, out);
  return hipGetLastError();
}

// The instance table as host rows, in selection order. Every row compiles without scratch
// (tools/kernel_resources.py, profiles/r4_kernel_resources.md).
static const PPORcRow kRcRows[] = {IA_RC_TABLE(IA_RC_ROW)};

static bool rc_row_bf3(const PPORcRow& r) { return rc_is_bf3(r.KT, r.S0T, r.NLT, r.HWT, r.CWT, r.NW); }

// The instance that runs a shape: the first row whose compile-time constants all agree with it
// (a constant the row leaves to run time -- ppo_rc_kernel.h, "Shape specialisation" -- agrees
// with anything), so a row is never chosen for a shape its constants do not fit. nullptr: no
// scratch-free build runs this shape. bf3_ok false passes over the split-bf16 rows, lean_ok
// false over the lean ones (a lean row precedes its full twin, so with lean_ok the twin of the
// row chosen without it -- or that row again -- comes back).
static const PPORcRow* rc_select(const PPOArgs& a, int kt, int cw, bool ns, bool bf3_ok, bool lean_ok) {
  const int s0 = (a.D + 3) / 4;
  for (const PPORcRow& r : kRcRows) {
    bool ok = r.ns == (int)ns && r.KT == kt && (r.CWT <= 0 || r.CWT == cw) && (lean_ok || !r.LEAN);
    ok = ok && (r.NLT <= 0 || (a.n_pi == r.NLT && a.n_vf == r.NLT));
    if (r.HWT > 0) {
      for (int l = 1; l < a.n_pi; ++l) ok = ok && a.pi_dims[l] == r.HWT;
      for (int l = 1; l < a.n_vf; ++l) ok = ok && a.vf_dims[l] == r.HWT;
    }
    ok = ok && (r.S0T > 0 ? s0 == r.S0T : (r.S0T == 0 || s0 <= -r.S0T));
    ok = ok && (r.ACTT < 0 || r.ACTT == a.hidden_act) && (r.DT < 0 || r.DT == (a.discrete ? 1 : 0));
    if (ok && (bf3_ok || !rc_row_bf3(r))) return &r;
  }
  return nullptr;
}

int device_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

// Host planning: the instance, LDS images + parameter items + workgroup split, and the launch
// shape. Returns false if the configuration is outside the fast path (falls back to ppo.hip).
// Environment overrides, all read here, once per plan:
//   IMITATION_AMD_PPO_PLAN_DEBUG=1  which check rejected a plan, LDS bytes (stderr)
//   IMITATION_AMD_PPO_NETSPLIT=0    both nets per workgroup
//   IMITATION_AMD_PPO_BF3=0         exact-fp32 PPO products: the split-bf16 instances are not
//       selected (the plan then takes a generic fp32 register-chained build, or the LDS kernel
//       where no scratch-free generic build exists -- slower, bit-for-bit the fp32 formulation)
//   IMITATION_AMD_PPO_XCHG2=0/1     forces the one- / two-level partial exchange
bool ppo_rc_plan(const PPOArgs& a, PPORcPlan& plan) {
  plan = PPORcPlan{};
  PPORcGeo& g = plan.g;
  const auto env = [](const char* name, char v) {
    const char* ev = getenv(name);
    return ev && ev[0] == v;
  };
  const bool debug = env("IMITATION_AMD_PPO_PLAN_DEBUG", '1');
  const bool env_ns = !env("IMITATION_AMD_PPO_NETSPLIT", '0'), env_bf3 = !env("IMITATION_AMD_PPO_BF3", '0');
  const char* env_xchg2 = getenv("IMITATION_AMD_PPO_XCHG2");
  const auto reject = [&](int site) {
    if (debug) fprintf(stderr, "ppo_rc_plan: rejected at check %d\n", site);
    return false;
  };
  if (a.batch % 16 != 0 || a.batch <= 0 || a.rows % a.batch != 0 || a.D > 64 || a.A > 16) return reject(1);
  if (a.n_pi < 1 || a.n_vf < 1 || a.n_pi > kL || a.n_vf > kL) return reject(2);
  const int* dims[2] = {a.pi_dims, a.vf_dims};
  const int nls[2] = {a.n_pi, a.n_vf};
  int wmax = 0;
  for (int q = 0; q < 2; ++q)
    for (int l = 0; l + 1 < nls[q]; ++l) wmax = dims[q][l + 1] > wmax ? dims[q][l + 1] : wmax;
  if (wmax > 64) return reject(3);
  g.kt = wmax <= 32 ? 2 : 4;
  const int KT = g.kt;
  // net split: each workgroup runs ONE net (actor or critic) over 64-row chunks -- its 4
  // row-tile waves at one wave per SIMD, with half of the dW / Adam items a both-nets
  // workgroup owns -- and the two nets meet once per minibatch for clip_grad_norm_
  const bool ns = env_ns && (a.rc_cw == 0 || a.rc_cw == 64) && a.batch % 64 == 0;
  // workgroup split: chunks of cw rows (64 for narrow nets and the net split, 32 for 64-wide
  // nets with both nets per workgroup: LDS, and the 4-wave workgroup has 2 row-tile waves per net)
  int cw = KT == 2 || ns ? 64 : 32;
  if (a.rc_cw == 16 || a.rc_cw == 32 || (a.rc_cw == 64 && KT == 2)) cw = a.rc_cw;
  if (a.batch < cw) cw = a.batch;
  if (a.batch % cw != 0) cw = 16;
  // the instance. No row: the generic 8-wave both-nets build (256 registers per wave) and the
  // generic 64-wide builds (owned items + vectors at run-time shapes) need scratch and are not
  // compiled, so 64-wide nets outside the [64, 64] families take the LDS kernel
  const PPORcRow* row = rc_select(a, KT, cw, ns, env_bf3, false);
  if (row == nullptr) return reject(4);
  if (row->CWT <= 0) {  // run-time chunk width: at most the rows the net's row-tile waves cover,
    // and at most 32: the kernel folds the images' 32 padded rows for these rows at compile time
    int cover = 16 * (ns ? row->NW : row->NW / 2);
    if (cover > 32) cover = 32;
    if (cw > cover) cw = cover;
    if (a.batch % cw != 0) cw = 16;
  }
  plan.row = plan.full = row;
  g.nw = row->NW;
  g.ns = ns ? 1 : 0;
  g.bf3 = rc_row_bf3(*row) ? 1 : 0;
  const int chunks = a.batch / cw;
  const int cus = a.rc_cus > 0 ? a.rc_cus : device_cu_count();
  const int per = ns ? 2 : 1;  // net split: two workgroups per row group
  int gmax = a.rc_gmax > 0 ? (a.rc_gmax < kMaxRcGroups ? a.rc_gmax : kMaxRcGroups) : kMaxRcGroups;
  {  // co-residency: every spinning workgroup must hold a CU of its own (> 80 KiB of LDS: one
     // per CU) while the rest of the chip stays free for concurrent streams (the discriminator
     // runs beside the update), so the working blocks are capped at half the device's CUs
    const int cap = (cus / 2) / per;
    if (cap < 1) return reject(5);
    if (gmax > cap) gmax = cap;
  }
  int G = 1;
  for (int c = gmax; c >= 1; --c)
    if (chunks % c == 0) {
      G = c;
      break;
    }
  g.cw = cw;
  g.G = G;
  g.nch = chunks / G;
  // one row group, no cycle counters: the lean twin of the row, where the table has one (the
  // same constants, so everything planned from the row stays as it is; PPOArgs::rc_lean = 0
  // keeps the full row)
  if (G == 1 && a.rc_lean != 0 && a.prof == nullptr) {
    const PPORcRow* lean = rc_select(a, KT, cw, ns, env_bf3, true);
    if (lean != nullptr && lean->LEAN && lean->NW == row->NW && lean->CWT == row->CWT) plan.row = lean;
  }
  int off = 0;
  auto take = [&](int n) {
    const int o = off;
    off += (n + 3) & ~3;
    return o;
  };
  // parameter images first (zeroed at kernel start); net split: both nets' images start at
  // the same offset (a workgroup holds one net), the region is the larger of the two
  const int pbase = off;
  int pend = off;
  for (int q = 0; q < 2; ++q) {
    if (g.ns) off = pbase;
    for (int l = 0; l < nls[q]; ++l) {
      const int din = dims[q][l], dout = dims[q][l + 1];
      const bool last = l == nls[q] - 1;
      if (!last && dout > 16 * KT) return reject(6);
      if (last && dout > 16) return reject(7);
      if (l > 0 && din > 16 * KT) return reject(8);
      g.din[q][l] = din;
      g.dout[q][l] = dout;
      const int ip = l == 0 ? ((din + 3) & ~3) : ((din + 15) & ~15);
      const int op = (dout + 15) & ~15;
      g.ldw[q][l] = (l == 0 ? ((din + 15) & ~15) : ip) + 4;
      // (BF3: the fp32 masters live in the Adam owners' registers -- no fp32 weight image)
      g.w_off[q][l] = take(g.bf3 ? 0 : op * g.ldw[q][l]);
      g.b_off[q][l] = take(op);
      if (g.bf3) {  // split-bf16 weight images (hi + lo): forward [op][pos(in)], transposed [din][pos(out)]
        const int kin = l == 0 ? 32 : 16 * KT, kout = last ? 32 : 16 * KT;
        g.wf_off[q][l] = take(op * bf3_ld(kin));
        g.wt_off[q][l] = l > 0 ? take(((din + 15) & ~15) * bf3_ld(kout)) : 0;
      }
    }
    pend = off > pend ? off : pend;
  }
  off = pend;
  g.ls_off = take(16);
  take(64);  // (once the zero row of empty dW slots, which now read a real strip; kept so that no plan's LDS moves)
  g.param_lds = off;
  // activation / dZ images for the dW MFMAs, row-major split-bf16 (ppo_rc_kernel.h dw_tiles):
  // per 16-feature tile one strip of rows_pad rows x 16 features, hi then lo, = 16 rows_pad
  // floats. A region keeps the (rows_pad + 4) floats per feature of the earlier feature-major
  // images, so no plan moves; the strips use the first rows_pad of them. Layer-0 input shared by
  // both nets.
  const int rows_pad = cw > 32 ? cw : 32;
  const int ldr = rows_pad + 4;
  const int h0 = take(((a.D + 15) & ~15) * ldr);
  const int abase = off;
  int aend = off;
  for (int q = 0; q < 2; ++q) {
    if (g.ns) off = abase;
    for (int l = 0; l < nls[q]; ++l) {
      if (l == 0) {
        g.h_off[q][0] = h0;
        g.ldh[q][0] = ldr;
      } else {
        g.ldh[q][l] = ldr;
        g.h_off[q][l] = take(((g.din[q][l] + 15) & ~15) * ldr);
      }
      g.ldz[q][l] = ldr;
      g.z_off[q][l] = take(((g.dout[q][l] + 15) & ~15) * ldr);
      g.db_off[q][l] = take(4 * 64);
    }
    aend = off > aend ? off : aend;
  }
  off = aend;
  // the G > 16 first-level stash reuses the activation images (G x 256 floats)
  g.xstash = G > 16 && aend - h0 >= G * 256 ? h0 : -1;
  g.lsp_off = take(4 * 16);
  g.nm_off = take(256);
  g.red_off = take(8 + 8 * 5 + 4);  // wave |g|^2, wave stats, [48] both nets' |g|^2
  g.trash_off = take(64);
  g.lds_floats = off;
  plan.lds_bytes = (size_t)off * 4;
  if (debug) fprintf(stderr, "ppo_rc_plan: %s, %zu B of LDS\n", row->name, plan.lds_bytes);
  if (plan.lds_bytes > 160 * 1024) return reject(9);
  // items: dW tiles first (ids [0, n_witems): a wave's weight items are its first slots),
  // actor's then critic's; then bias vectors: actor's, log_std (an actor item), critic's
  int n = 0;
  for (int q = 0; q < 2; ++q) {
    g.wbase[q] = n;
    for (int l = 0; l < nls[q]; ++l) {
      const int to = (g.dout[q][l] + 15) / 16, ti = (g.din[q][l] + 15) / 16;
      for (int ta = 0; ta < to; ++ta)
        for (int tb = 0; tb < ti; ++tb) {
          if (n >= kMaxRcItems) return reject(10);
          g.items[n++] = q | (l << 1) | (0 << 3) | (ta << 5) | (tb << 9);
        }
    }
    g.nwit[q] = n - g.wbase[q];
  }
  g.n_witems = n;
  for (int q = 0; q < 2; ++q) {
    g.bbase[q] = n;
    for (int l = 0; l < nls[q]; ++l) {
      if (n >= kMaxRcItems) return reject(11);
      g.items[n++] = q | (l << 1) | (1 << 3);
    }
    if (q == 0 && !a.discrete && a.log_std_off >= 0) {
      if (n >= kMaxRcItems) return reject(12);
      g.items[n++] = 2 << 3;
    }
    g.nbit[q] = n - g.bbase[q];
  }
  g.n_items = n;
  // a wave owns at most the KW weight tiles / KB vectors its instance was compiled with
  int wmx = g.n_witems, bmx = n - g.n_witems;
  if (g.ns) {
    wmx = g.nwit[0] > g.nwit[1] ? g.nwit[0] : g.nwit[1];
    bmx = g.nbit[0] > g.nbit[1] ? g.nbit[0] : g.nbit[1];
  }
  if ((wmx + g.nw - 1) / g.nw > row->KW || (bmx + g.nw - 1) / g.nw > row->KB) return reject(13);
  g.dp = (a.D + 3) & ~3;
  // two-level exchange from 4 (64-wide nets) / 16 (<= 32-wide) cooperating workgroups
  // (measured: profiles/r3_ppo64_scale.md)
  g.xchg2 = env_xchg2 ? (env_xchg2[0] == '1' && G > 1) : (G >= (KT == 4 ? 4 : 16));
  // > 80 KiB of LDS keeps the cooperating workgroups one per CU (the measured condition of
  // the sc1 hand-off); all G <= kMaxRcGroups (64) of them are co-resident (256 CUs)
  // (net split: the two workgroups must not share a CU's matrix cores either)
  plan.lds_launch = (G > 1 || ns) && plan.lds_bytes < 96 * 1024 ? 96 * 1024 : plan.lds_bytes;
  const int nblk = per * G;
  {  // cooperating workgroups on as few XCDs as possible (the "xcd" geometry field is the block
     // stride). GAIL emulated W = 2 / 4 / 8: 3.14 / 3.28 / 3.64 -> 2.99 / 2.96 / 3.36 ms per update,
     // headline round 3.63 -> 3.55 ms (profiles/r3_ppo_xcd.md)
    // At most 16 workgroups (half an XCD's 32 CUs) per XCD, so concurrent work on the other
    // stream (the discriminator) never holds a CU a spinning cooperating workgroup waits for:
    // stride 8 / 4 / 2 for <= 16 / 32 / 64 workgroups (blocks b % stride == 0 work: XCDs {0},
    // {0, 4}, {0, 2, 4, 6} of the deal). DRLHP emulated W = 8 (32 workgroups): one XCD 27.3 ms,
    // spread 25.6 ms (profiles/r3_ppo_xcd.md).
    g.xcd = 1;
    if (nblk > 1) g.xcd = nblk <= 16 ? 8 : nblk <= 32 ? 4 : nblk <= 64 ? 2 : 1;
    // never a wider stride than the device has XCDs (32 CUs each; a partitioned device has fewer)
    const int xcds = cus / 32 > 1 ? cus / 32 : 1;
    while (g.xcd > xcds) g.xcd >>= 1;
  }
  plan.grid = nblk * g.xcd;
  plan.block = 64 * g.nw;
  const size_t K = (size_t)a.n_epochs * (a.rows / a.batch);
  plan.workspace_floats = K * G * g.nch * 64 * (g.dp + 16 + 4) + K * 128 + 2 * (size_t)(G + 1) * g.n_items * 256 + 64;
  return true;
}

hipError_t ppo_rc_launch(const PPOArgs& a, const PPORcPlan& plan, float* workspace, hipStream_t s) {
  PPORcGeo g = plan.g;
  const size_t K = (size_t)a.n_epochs * (a.rows / a.batch);
  const size_t slots = K * g.G * g.nch;
  g.xraw = workspace;
  g.acts = g.xraw + slots * 64 * g.dp;
  g.rowd = g.acts + slots * 64 * 16;
  g.mom = g.rowd + slots * 64 * 4;
  g.slab = g.mom + K * 128;
  g.red = g.slab + 2 * (size_t)g.G * g.n_items * 256;
  g.sync = reinterpret_cast<unsigned*>(g.red + 2 * (size_t)g.n_items * 256);
  if (K == 0) return hipSuccess;
  const int nblk = g.ns ? 2 * g.G : g.G;
  if (nblk > 1) {
    // every working block must be resident at once: check the instance's occupancy at this
    // LDS size against the device (the plan capped the working blocks at half the CUs)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(plan.row->kernel),
                                                     (int)plan.block, plan.lds_launch) != hipSuccess)
      per_cu = 1;
    if (per_cu > 1 && plan.lds_launch > 80 * 1024) per_cu = 1;  // LDS holds one block per CU (the API can read high)
    const int cus = a.rc_cus > 0 ? a.rc_cus : device_cu_count();
    if (per_cu < 1 || (long long)per_cu * cus < (long long)nblk) return hipErrorCooperativeLaunchTooLarge;
  }
  const int CH = g.G * g.nch;
  const int prep_waves = CH < kPrepWaves ? CH : kPrepWaves;
  hipLaunchKernelGGL(ppo_rc_prep_kernel, dim3((unsigned)K), dim3(64 * prep_waves), 0, s, a, g);
  hipLaunchKernelGGL(plan.row->kernel, dim3(plan.grid), dim3(plan.block), plan.lds_launch, s, a, g);
  return hipGetLastError();
}

}  // namespace ia
