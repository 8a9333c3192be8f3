// bc_mlp_steps: G behavioural-cloning minibatch steps of a small MLP policy in one launch
// (csrc/kernels/bc_mlp.hip). Python side: imitation_amd/ops/bc_mlp.py. Tensor checks -> raw
// pointers; the shape limits are the launcher's.
#include "common.h"
#include "launchers.h"

namespace {

void bc_mlp_steps(torch::Tensor obs_src, torch::Tensor acts_src, torch::Tensor ids, torch::Tensor params,
                  c10::optional<torch::Tensor> grads, torch::Tensor exp_avg, torch::Tensor exp_avg_sq, torch::Tensor step,
                  std::vector<int64_t> offsets, int64_t off_log_std, int64_t D, int64_t H1, int64_t H2, int64_t A, bool gaussian,
                  bool tanh_act, double lr, double beta1, double beta2, double eps, double ent_weight, double l2_weight,
                  torch::Tensor metrics) {
  ia::BcMlpArgs a{};
  for (auto* t : {&params, &exp_avg, &exp_avg_sq}) {
    IA_CHECK_GPU_F32(*t);
    TORCH_CHECK(t->numel() == params.numel(), "the flat buckets must have equal sizes");
  }
  if (grads && grads->defined()) {
    IA_CHECK_GPU_F32(*grads);
    TORCH_CHECK(grads->numel() == params.numel(), "the flat buckets must have equal sizes");
    a.grads = grads->data_ptr<float>();
    a.keep_grad = 1;
  }
  IA_CHECK_GPU_F32(step);
  IA_CHECK_GPU_F32(metrics);
  IA_CHECK_GPU_F32(obs_src);
  TORCH_CHECK(step.numel() == 1, "step must be a 1-element device tensor");
  TORCH_CHECK(offsets.size() == 6, "offsets: W1, b1, W2, b2, W3, b3");
  IA_CHECK_CUDA(ids);
  IA_CHECK_CONTIG(ids);
  TORCH_CHECK(ids.scalar_type() == torch::kInt64 && ids.dim() == 2, "ids: int64 [G, B]");
  TORCH_CHECK(D >= 1 && A >= 1 && obs_src.dim() == 2 && obs_src.size(1) == D, "obs_src: float32 [N, D]");
  a.rows = obs_src.size(0);
  IA_CHECK_CUDA(acts_src);
  IA_CHECK_CONTIG(acts_src);
  if (gaussian) {
    TORCH_CHECK(acts_src.scalar_type() == torch::kFloat32 && acts_src.numel() == a.rows * A, "acts_src: float32 [N, A]");
    a.acts_gauss = acts_src.data_ptr<float>();
  } else {
    TORCH_CHECK(acts_src.scalar_type() == torch::kInt64 && acts_src.numel() == a.rows, "acts_src: int64 [N]");
    a.acts_cat = acts_src.data_ptr<int64_t>();
  }
  a.obs_src = obs_src.data_ptr<float>();
  a.ids = ids.data_ptr<int64_t>();
  a.G = (int)ids.size(0);
  a.B = (int)ids.size(1);
  TORCH_CHECK(metrics.numel() == (int64_t)a.G * 7, "metrics: float32 [G, 7]");
  a.D = (int)D;
  a.H1 = (int)H1;
  a.H2 = (int)H2;
  a.A = (int)A;
  a.tanh_act = tanh_act ? 1 : 0;
  for (int i = 0; i < 6; ++i) a.off[i] = (int)offsets[i];
  a.off_log_std = (int)off_log_std;
  a.params = params.data_ptr<float>();
  a.exp_avg = exp_avg.data_ptr<float>();
  a.exp_avg_sq = exp_avg_sq.data_ptr<float>();
  a.step = step.data_ptr<float>();
  a.n = params.numel();
  a.lr = (float)lr;
  a.beta1 = (float)beta1;
  a.beta2 = (float)beta2;
  a.eps = (float)eps;
  a.ent_weight = (float)ent_weight;
  a.l2_weight = (float)l2_weight;
  a.ent_weight_lo = (float)(ent_weight - (double)a.ent_weight);
  a.l2_weight_lo = (float)(l2_weight - (double)a.l2_weight);
  a.metrics = metrics.data_ptr<float>();
  const hipError_t e = ia::bc_mlp_steps(a, ia_stream());
  TORCH_CHECK(e == hipSuccess, "bc_mlp_steps: ", hipGetErrorString(e),
              " (limits: obs dim, hidden widths, actions in 1..64, batch in 1..256, bucket of at most 64K elements, G >= 1)");
}

}  // namespace

void register_bc_mlp(py::module& m) {
  m.def("bc_mlp_steps", &bc_mlp_steps, py::arg("obs_src"), py::arg("acts_src"), py::arg("ids"), py::arg("params"),
        py::arg("grads"), py::arg("exp_avg"), py::arg("exp_avg_sq"), py::arg("step"), py::arg("offsets"),
        py::arg("off_log_std"), py::arg("D"), py::arg("H1"), py::arg("H2"), py::arg("A"), py::arg("gaussian"),
        py::arg("tanh_act"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("ent_weight"),
        py::arg("l2_weight"), py::arg("metrics"),
        "G BC minibatch steps (gather, forward, loss + metrics, backward, L2, Adam over the whole bucket) in one launch");
}
