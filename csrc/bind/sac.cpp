// sac_update_step: every gradient step of one SAC.train call in one launch
// (csrc/kernels/sac_update.hip). Python side: imitation_amd/ops/sac.py. Tensor checks -> raw
// pointers; the shape limits are the launcher's.
#include "common.h"
#include "launchers.h"

namespace {

// one replay ring as [obs, next_obs, actions, rewards, dones, timeouts] over `rows` flat rows
ia::SacSrc sac_source(const std::vector<torch::Tensor>& f, int64_t D, int64_t A, const char* name) {
  TORCH_CHECK(f.size() == 6, name, ": [obs, next_obs, actions, rewards, dones, timeouts]");
  for (const auto& t : f) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, ": contiguous GPU tensors");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, ": float32 fields");
  }
  const int64_t rows = f[3].numel();
  TORCH_CHECK(f[0].numel() == rows * D && f[1].numel() == rows * D, name, ": obs / next_obs must be [rows, D]");
  TORCH_CHECK(f[2].numel() == rows * A, name, ": actions must be [rows, A]");
  TORCH_CHECK(f[4].numel() == rows && f[5].numel() == rows, name, ": one done, timeout per row");
  ia::SacSrc s{};
  s.obs = f[0].data_ptr<float>();
  s.next_obs = f[1].data_ptr<float>();
  s.action = f[2].data_ptr<float>();
  s.reward = f[3].data_ptr<float>();
  s.done = f[4].data_ptr<float>();
  s.timeout = f[5].data_ptr<float>();
  s.rows = rows;
  return s;
}

// [flat, grad, exp_avg, exp_avg_sq, step] of a FusedAdam group and its hyper-parameters [lr, beta1, beta2, eps]
ia::SacBucket sac_bucket(const std::vector<torch::Tensor>& b, const std::vector<double>& hp, const char* name) {
  TORCH_CHECK(b.size() == 5, name, ": [flat, grad, exp_avg, exp_avg_sq, step]");
  TORCH_CHECK(hp.size() == 4, name, ": [lr, beta1, beta2, eps]");
  for (const auto& t : b) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kFloat32, name, ": contiguous float32 GPU tensors");
  }
  for (int i = 1; i < 4; ++i) TORCH_CHECK(b[i].numel() == b[0].numel(), name, ": the flat buckets must have equal sizes");
  TORCH_CHECK(b[4].numel() == 1, name, ": step must be a 1-element device tensor");
  ia::SacBucket k{};
  k.params = b[0].data_ptr<float>();
  k.grads = b[1].data_ptr<float>();
  k.exp_avg = b[2].data_ptr<float>();
  k.exp_avg_sq = b[3].data_ptr<float>();
  k.step = b[4].data_ptr<float>();
  k.n = b[0].numel();
  k.lr = (float)hp[0];
  k.beta1 = (float)hp[1];
  k.beta2 = (float)hp[2];
  k.eps = (float)hp[3];
  return k;
}

void sac_update_step(std::vector<torch::Tensor> src_a, c10::optional<std::vector<torch::Tensor>> src_b, torch::Tensor ids_a,
                     c10::optional<torch::Tensor> ids_b, torch::Tensor eps_pi, torch::Tensor eps_next,
                     std::vector<torch::Tensor> actor, std::vector<double> actor_hp, std::vector<torch::Tensor> critic,
                     std::vector<double> critic_hp, c10::optional<std::vector<torch::Tensor>> ent,
                     std::vector<double> ent_hp, double ent_coef_fixed, double target_entropy, torch::Tensor target,
                     std::vector<int64_t> dims, std::vector<int64_t> actor_offsets, std::vector<int64_t> critic_offsets,
                     double gamma, double tau, int64_t target_update_interval, std::vector<torch::Tensor> outs) {
  ia::SacUpdateArgs a{};
  TORCH_CHECK(dims.size() == 6, "dims: D, A, actor H1, H2, critic H1, H2");
  TORCH_CHECK(actor_offsets.size() == 8, "actor offsets: W1, b1, W2, b2, Wmu, bmu, Wls, bls");
  TORCH_CHECK(critic_offsets.size() == 12, "critic offsets: W1, b1, W2, b2, W3, b3 of qf0 and of qf1");
  TORCH_CHECK(outs.size() == 4, "outputs: critic_loss, actor_loss, ent_coef, ent_coef_loss");
  const int64_t D = dims[0], A = dims[1];
  // (the launcher repeats this limit; here it keeps the size checks below meaningful)
  TORCH_CHECK(D >= 1 && A >= 1 && D + A <= ia::kSacMaxDim, "sac_update_step: ", hipGetErrorString(hipErrorInvalidValue),
              " (limits: obs dim + action dim <= 64)");
  IA_CHECK_CUDA(ids_a);
  IA_CHECK_CONTIG(ids_a);
  TORCH_CHECK(ids_a.scalar_type() == torch::kInt64 && ids_a.dim() == 2, "ids_a: int64 [G, n_a]");
  a.G = (int)ids_a.size(0);
  a.n_a = (int)ids_a.size(1);
  a.ids_a = ids_a.data_ptr<int64_t>();
  a.src[0] = sac_source(src_a, D, A, "src_a");
  if (ids_b && ids_b->defined() && ids_b->size(1) > 0) {
    IA_CHECK_CUDA(*ids_b);
    IA_CHECK_CONTIG(*ids_b);
    TORCH_CHECK(ids_b->scalar_type() == torch::kInt64 && ids_b->dim() == 2 && ids_b->size(0) == a.G, "ids_b: int64 [G, n_e]");
    TORCH_CHECK(src_b.has_value(), "ids_b without src_b");
    a.n_e = (int)ids_b->size(1);
    a.ids_b = ids_b->data_ptr<int64_t>();
    a.src[1] = sac_source(*src_b, D, A, "src_b");
  }
  const int64_t B = (int64_t)a.n_a + a.n_e;
  IA_CHECK_GPU_F32(eps_pi);
  IA_CHECK_GPU_F32(eps_next);
  TORCH_CHECK(a.G >= 1 && eps_pi.numel() == a.G * B * A && eps_next.numel() == a.G * B * A, "eps_pi / eps_next: [G, B, A]");
  a.eps_pi = eps_pi.data_ptr<float>();
  a.eps_next = eps_next.data_ptr<float>();
  a.D = (int)D;
  a.A = (int)A;
  a.aH1 = (int)dims[2];
  a.aH2 = (int)dims[3];
  a.cH1 = (int)dims[4];
  a.cH2 = (int)dims[5];
  for (int i = 0; i < 8; ++i) a.a_off[i] = (int)actor_offsets[i];
  for (int i = 0; i < 12; ++i) a.c_off[i / 6][i % 6] = (int)critic_offsets[i];
  a.actor = sac_bucket(actor, actor_hp, "actor");
  a.critic = sac_bucket(critic, critic_hp, "critic");
  if (ent && !ent->empty()) a.ent = sac_bucket(*ent, ent_hp, "ent");
  a.ent_coef_fixed = (float)ent_coef_fixed;
  a.target_entropy = (float)target_entropy;
  IA_CHECK_GPU_F32(target);
  TORCH_CHECK(target.numel() == a.critic.n, "the target bucket must have the critic bucket's size");
  a.target = target.data_ptr<float>();
  a.gamma = (float)gamma;
  a.tau = (float)tau;
  a.one_minus_tau = (float)(1.0 - tau);
  a.target_update_interval = (int)target_update_interval;
  for (const auto& t : outs) {
    IA_CHECK_GPU_F32(t);
    TORCH_CHECK(t.numel() == a.G, "outputs: one float per gradient step");
  }
  a.critic_loss = outs[0].data_ptr<float>();
  a.actor_loss = outs[1].data_ptr<float>();
  a.ent_coef = outs[2].data_ptr<float>();
  a.ent_coef_loss = outs[3].data_ptr<float>();
  const hipError_t e = ia::sac_update_step(a, ia_stream());
  TORCH_CHECK(e == hipSuccess, "sac_update_step: ", hipGetErrorString(e),
              " (limits: obs dim, hidden widths, obs dim + action dim in 1..64, batch in 1..256)");
}

}  // namespace

void register_sac(py::module& m) {
  m.def("sac_update_step", &sac_update_step, py::arg("src_a"), py::arg("src_b"), py::arg("ids_a"), py::arg("ids_b"),
        py::arg("eps_pi"), py::arg("eps_next"), py::arg("actor"), py::arg("actor_hp"), py::arg("critic"),
        py::arg("critic_hp"), py::arg("ent"), py::arg("ent_hp"), py::arg("ent_coef_fixed"), py::arg("target_entropy"),
        py::arg("target"), py::arg("dims"), py::arg("actor_offsets"), py::arg("critic_offsets"), py::arg("gamma"),
        py::arg("tau"), py::arg("target_update_interval"), py::arg("outs"),
        "All gradient steps of one SAC.train call (gather, actor, entropy coefficient, target, critic and actor updates, "
        "Polyak) in one launch");
}
