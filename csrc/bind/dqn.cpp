// dqn_td_step: every gradient step of one DQN.train call in one launch (csrc/kernels/dqn_td.hip;
// imitation_amd/ops/dqn.py). Tensor checks -> raw pointers; the shape limits are the launcher's.
#include "common.h"
#include "launchers.h"

namespace {

// one replay ring as [obs, next_obs, actions, rewards, dones, timeouts] over `rows` flat rows
ia::DqnTdSrc td_source(const std::vector<torch::Tensor>& f, int64_t D, const char* name) {
  TORCH_CHECK(f.size() == 6, name, ": [obs, next_obs, actions, rewards, dones, timeouts]");
  for (const auto& t : f) TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, ": contiguous GPU tensors");
  for (int i : {0, 1, 3, 4, 5}) TORCH_CHECK(f[i].scalar_type() == torch::kFloat32, name, ": float32 fields");
  TORCH_CHECK(f[2].scalar_type() == torch::kInt64, name, ": int64 actions");
  const int64_t rows = f[3].numel();
  TORCH_CHECK(f[0].numel() == rows * D && f[1].numel() == rows * D, name, ": obs / next_obs must be [rows, D]");
  TORCH_CHECK(f[2].numel() == rows && f[4].numel() == rows && f[5].numel() == rows, name, ": one action, done, timeout per row");
  ia::DqnTdSrc s{};
  s.obs = f[0].data_ptr<float>();
  s.next_obs = f[1].data_ptr<float>();
  s.action = f[2].data_ptr<int64_t>();
  s.reward = f[3].data_ptr<float>();
  s.done = f[4].data_ptr<float>();
  s.timeout = f[5].data_ptr<float>();
  s.rows = rows;
  return s;
}

void dqn_td_step(std::vector<torch::Tensor> src_a, c10::optional<std::vector<torch::Tensor>> src_b, torch::Tensor ids_a,
                 c10::optional<torch::Tensor> ids_b, torch::Tensor params, torch::Tensor grads, torch::Tensor exp_avg,
                 torch::Tensor exp_avg_sq, torch::Tensor step, torch::Tensor target, std::vector<int64_t> offsets, int64_t D,
                 int64_t H1, int64_t H2, int64_t A, double lr, double beta1, double beta2, double eps, double gamma,
                 double max_norm, torch::Tensor losses, torch::Tensor gnorm) {
  ia::DqnTdArgs a{};
  for (auto* t : {&params, &grads, &exp_avg, &exp_avg_sq, &target}) {
    IA_CHECK_GPU_F32(*t);
    TORCH_CHECK(t->numel() == params.numel(), "the flat buckets must have equal sizes");
  }
  IA_CHECK_GPU_F32(step);
  IA_CHECK_GPU_F32(losses);
  IA_CHECK_GPU_F32(gnorm);
  TORCH_CHECK(step.numel() == 1, "step must be a 1-element device tensor");
  TORCH_CHECK(offsets.size() == 6, "offsets: W1, b1, W2, b2, W3, b3");
  IA_CHECK_CUDA(ids_a);
  IA_CHECK_CONTIG(ids_a);
  TORCH_CHECK(ids_a.scalar_type() == torch::kInt64 && ids_a.dim() == 2, "ids_a: int64 [G, n_a]");
  a.G = (int)ids_a.size(0);
  a.n_a = (int)ids_a.size(1);
  a.ids_a = ids_a.data_ptr<int64_t>();
  a.src[0] = td_source(src_a, D, "src_a");
  if (ids_b && ids_b->defined() && ids_b->size(1) > 0) {
    IA_CHECK_CUDA(*ids_b);
    IA_CHECK_CONTIG(*ids_b);
    TORCH_CHECK(ids_b->scalar_type() == torch::kInt64 && ids_b->dim() == 2 && ids_b->size(0) == a.G, "ids_b: int64 [G, n_e]");
    TORCH_CHECK(src_b.has_value(), "ids_b without src_b");
    a.n_e = (int)ids_b->size(1);
    a.ids_b = ids_b->data_ptr<int64_t>();
    a.src[1] = td_source(*src_b, D, "src_b");
  }
  TORCH_CHECK(a.G >= 1 && losses.numel() == a.G && gnorm.numel() == a.G, "losses / gnorm: one float per gradient step");
  a.D = (int)D;
  a.H1 = (int)H1;
  a.H2 = (int)H2;
  a.A = (int)A;
  for (int i = 0; i < 6; ++i) a.off[i] = (int)offsets[i];
  a.target = target.data_ptr<float>();
  a.params = params.data_ptr<float>();
  a.grads = grads.data_ptr<float>();
  a.exp_avg = exp_avg.data_ptr<float>();
  a.exp_avg_sq = exp_avg_sq.data_ptr<float>();
  a.step = step.data_ptr<float>();
  a.n = params.numel();
  a.lr = (float)lr;
  a.beta1 = (float)beta1;
  a.beta2 = (float)beta2;
  a.eps = (float)eps;
  a.gamma = (float)gamma;
  a.max_norm = (float)max_norm;
  a.losses = losses.data_ptr<float>();
  a.gnorm = gnorm.data_ptr<float>();
  const hipError_t e = ia::dqn_td_step(a, ia_stream());
  TORCH_CHECK(e == hipSuccess, "dqn_td_step: ", hipGetErrorString(e),
              " (limits: obs dim, hidden widths, actions in 1..64, batch in 1..256)");
}

}  // namespace

void register_dqn(py::module& m) {
  m.def("dqn_td_step", &dqn_td_step, py::arg("src_a"), py::arg("src_b"), py::arg("ids_a"), py::arg("ids_b"),
        py::arg("params"), py::arg("grads"), py::arg("exp_avg"), py::arg("exp_avg_sq"), py::arg("step"), py::arg("target"),
        py::arg("offsets"), py::arg("D"), py::arg("H1"), py::arg("H2"), py::arg("A"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("gamma"), py::arg("max_norm"), py::arg("losses"), py::arg("gnorm"),
        "All gradient steps of one DQN.train call (gather, target, forward, Huber loss, backward, clip, Adam) in one launch");
}
