// Torch-facing wrappers of the one-shot all-reduce (comm.hip).  Regions are passed around
// as integer device addresses; the Python communicator (parallel/oneshot.py) owns them.
#include "common.h"
#include "launchers.h"

namespace {

py::tuple oneshot_alloc(int64_t stage_bytes) {
  TORCH_CHECK(stage_bytes > 0 && stage_bytes % 16 == 0, "stage_bytes must be a positive multiple of 16");
  void* p = nullptr;
  std::string h(ia::oneshot_handle_bytes(), '\0');
  IA_HIP_CHECK(ia::oneshot_alloc((size_t)stage_bytes, &p, &h[0]));
  return py::make_tuple((int64_t)reinterpret_cast<uintptr_t>(p), py::bytes(h));
}

int64_t oneshot_open(py::bytes handle) {
  std::string h = handle;
  TORCH_CHECK(h.size() == ia::oneshot_handle_bytes(), "bad IPC handle size");
  void* p = nullptr;
  IA_HIP_CHECK(ia::oneshot_open(h.data(), &p));
  return (int64_t)reinterpret_cast<uintptr_t>(p);
}

void oneshot_allreduce(const std::vector<int64_t>& bases, int64_t rank, torch::Tensor in, torch::Tensor out, double scale,
                       int64_t stage_bytes, double timeout_s) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda() && in.is_contiguous() && out.is_contiguous(), "contiguous GPU tensors");
  TORCH_CHECK(in.scalar_type() == out.scalar_type() &&
                  (in.scalar_type() == torch::kFloat32 || in.scalar_type() == torch::kFloat64),
              "float32 or float64 in/out of one dtype");
  TORCH_CHECK(in.numel() == out.numel(), "in/out size mismatch");
  TORCH_CHECK(!bases.empty() && bases.size() <= (size_t)ia::kOneShotMaxRanks, "1..8 ranks");
  TORCH_CHECK(rank >= 0 && rank < (int64_t)bases.size(), "rank out of range");
  TORCH_CHECK((size_t)in.numel() * in.element_size() <= (size_t)stage_bytes, "bucket larger than the staging slot");
  TORCH_CHECK(((uintptr_t)in.data_ptr() | (uintptr_t)out.data_ptr()) % 16 == 0, "in/out must be 16-B aligned");
  ia::OneShotArgs a{};
  for (size_t r = 0; r < bases.size(); ++r) a.base[r] = reinterpret_cast<char*>((uintptr_t)bases[r]);
  a.in = in.data_ptr();
  a.out = out.data_ptr();
  a.n = (int)in.numel();
  a.rank = (int)rank;
  a.world = (int)bases.size();
  a.f64 = in.scalar_type() == torch::kFloat64;
  a.scale = scale;
  a.stage_bytes = (size_t)stage_bytes;
  a.timeout_ticks = (long long)(timeout_s * (double)ia::oneshot_ticks_per_second());
  IA_HIP_CHECK(ia::oneshot_allreduce(a, ia_stream()));
}

py::tuple twophase_alloc(int64_t slot_bytes) {
  TORCH_CHECK(slot_bytes > 0 && slot_bytes % 16 == 0, "slot_bytes must be a positive multiple of 16");
  void* p = nullptr;
  std::string h(ia::oneshot_handle_bytes(), '\0');
  IA_HIP_CHECK(ia::oneshot_alloc_region(ia::twophase_region_bytes((size_t)slot_bytes), &p, &h[0]));
  return py::make_tuple((int64_t)reinterpret_cast<uintptr_t>(p), py::bytes(h));
}

void twophase_allreduce(const std::vector<int64_t>& bases, int64_t rank, torch::Tensor in, torch::Tensor out, double scale,
                        int64_t slot_bytes, double timeout_s) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda() && in.is_contiguous() && out.is_contiguous(), "contiguous GPU tensors");
  TORCH_CHECK(in.scalar_type() == out.scalar_type() &&
                  (in.scalar_type() == torch::kFloat32 || in.scalar_type() == torch::kFloat64),
              "float32 or float64 in/out of one dtype");
  TORCH_CHECK(in.numel() == out.numel(), "in/out size mismatch");
  TORCH_CHECK(!bases.empty() && bases.size() <= (size_t)ia::kOneShotMaxRanks, "1..8 ranks");
  TORCH_CHECK(rank >= 0 && rank < (int64_t)bases.size(), "rank out of range");
  TORCH_CHECK(slot_bytes > 0 && slot_bytes % 16 == 0, "slot_bytes must be a positive multiple of 16");
  TORCH_CHECK((size_t)in.numel() * in.element_size() <= (size_t)slot_bytes, "bucket larger than the slot");
  TORCH_CHECK(((uintptr_t)in.data_ptr() | (uintptr_t)out.data_ptr()) % 16 == 0, "in/out must be 16-B aligned");
  ia::TwoPhaseArgs a{};
  for (size_t r = 0; r < bases.size(); ++r) a.base[r] = reinterpret_cast<char*>((uintptr_t)bases[r]);
  a.in = in.data_ptr();
  a.out = out.data_ptr();
  a.n = (int)in.numel();
  a.rank = (int)rank;
  a.world = (int)bases.size();
  a.f64 = in.scalar_type() == torch::kFloat64;
  a.scale = scale;
  a.slot_bytes = (size_t)slot_bytes;
  a.timeout_ticks = (long long)(timeout_s * (double)ia::oneshot_ticks_per_second());
  IA_HIP_CHECK(ia::twophase_allreduce(a, ia_stream()));
}

py::tuple twophase_shard(int64_t v0, int64_t v1, int64_t world, int64_t r) {
  TORCH_CHECK(0 <= v0 && v0 <= v1 && v1 <= INT32_MAX && world >= 1 && world <= ia::kOneShotMaxRanks && r >= 0 && r < world,
              "twophase_shard: 0 <= v0 <= v1, 1..8 ranks, r in range");
  int lo = 0, hi = 0;
  ia::twophase_shard((int)v0, (int)v1, (int)world, (int)r, &lo, &hi);
  return py::make_tuple((int64_t)lo, (int64_t)hi);
}

int64_t oneshot_error(int64_t local) {
  int e = 0;
  IA_HIP_CHECK(ia::oneshot_read_error(reinterpret_cast<void*>((uintptr_t)local), &e));
  return e;
}

}  // namespace

void register_comm(py::module& m) {
  m.def("oneshot_alloc", &oneshot_alloc, "zeroed uncached staging region -> (address, IPC handle bytes)");
  m.def("oneshot_open", &oneshot_open, "map a peer's region from its IPC handle -> address");
  m.def("oneshot_close", [](int64_t p) { IA_HIP_CHECK(ia::oneshot_close(reinterpret_cast<void*>((uintptr_t)p))); });
  m.def("oneshot_free", [](int64_t p) { IA_HIP_CHECK(ia::oneshot_free(reinterpret_cast<void*>((uintptr_t)p))); });
  m.def("oneshot_region_bytes", [](int64_t s) { return (int64_t)ia::oneshot_region_bytes((size_t)s); });
  m.def("oneshot_blocks", [](int64_t n, int64_t stage, int64_t elem_bytes) { return ia::oneshot_blocks((int)n, (size_t)stage, (int)elem_bytes); },
        py::arg("n"), py::arg("stage"), py::arg("elem_bytes") = 4);
  m.def("oneshot_allreduce", &oneshot_allreduce, "one-shot sum all-reduce of in*scale over the mapped ranks into out");
  m.def("twophase_alloc", &twophase_alloc, "zeroed uncached two-phase region -> (address, IPC handle bytes)");
  m.def("twophase_region_bytes", [](int64_t s) { return (int64_t)ia::twophase_region_bytes((size_t)s); });
  m.def("twophase_blocks", [](int64_t n, int64_t slot, int64_t elem_bytes) { return ia::twophase_blocks((int)n, (size_t)slot, (int)elem_bytes); },
        py::arg("n"), py::arg("slot"), py::arg("elem_bytes") = 4);
  m.def("twophase_shard", &twophase_shard, "shard r of the block slice [v0, v1) cut over `world` ranks -> (lo, hi)");
  m.def("twophase_allreduce", &twophase_allreduce,
        "two-phase (reduce-scatter + all-gather) sum all-reduce of in*scale over the mapped ranks into out");
  m.def("oneshot_error", &oneshot_error,"error word of a local region (1: a block timed out)");
  m.def("oneshot_error_async",
        [](int64_t local, torch::Tensor pinned) {
          TORCH_CHECK(!pinned.is_cuda() && pinned.is_pinned() && pinned.scalar_type() == torch::kInt32 && pinned.numel() >= 1,
                      "oneshot_error_async: pinned int32 host tensor");
          IA_HIP_CHECK(ia::oneshot_read_error_async(reinterpret_cast<void*>((uintptr_t)local), pinned.data_ptr<int>(),
                                                    ia_stream()));
        },
        "stream-ordered copy of the error word into a pinned host int32 tensor");
  m.def("oneshot_clear_error",
        [](int64_t p) { IA_HIP_CHECK(ia::oneshot_clear_error(reinterpret_cast<void*>((uintptr_t)p))); });
}
