// dqn_td_step: every gradient step of one DQN.train call in one launch (csrc/kernels/dqn_td.hip);
// dqn_collect: K steps of acting, env physics and replay-ring writes in one launch
// (csrc/kernels/dqn_collect.hip). Python side: imitation_amd/ops/dqn.py. Tensor checks -> raw
// pointers; the shape limits are the launchers'.
#include "common.h"
#include "launchers.h"
#include "vec_env.h"

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

// env: [state [N, sdim], rng [N] int64, elapsed [N] int32, ep_ret [N], cur_obs [N, D]]; ring: the six
// td_source fields over S * N rows; rec: [done, ep_ret, ep_len int32, action int64], each [K, N]
void dqn_collect(const std::string& env_id, int64_t max_steps, std::vector<torch::Tensor> env, torch::Tensor act_rng,
                 std::vector<torch::Tensor> ring, int64_t pos0, int64_t S, torch::Tensor params,
                 std::vector<int64_t> offsets, int64_t D, int64_t H1, int64_t H2, int64_t A, std::vector<int64_t> thr,
                 bool use_reward_const, double reward_const, bool write_timeouts, std::vector<torch::Tensor> rec,
                 c10::optional<torch::Tensor> rec_explore, c10::optional<torch::Tensor> rec_q, torch::Tensor err) {
  ia::DqnCollectArgs a{};
  int ms = 0;
  TORCH_CHECK(ia::make_env_params(env_id, &a.P, &ms), "unknown native env ", env_id);
  TORCH_CHECK(env.size() == 5, "env: [state, rng, elapsed, ep_ret, cur_obs]");
  TORCH_CHECK(rec.size() == 4, "records: [done, ep_ret, ep_len, action]");
  TORCH_CHECK(offsets.size() == 6, "offsets: W1, b1, W2, b2, W3, b3");
  const int64_t K = (int64_t)thr.size(), N = act_rng.numel();
  // (the launcher repeats these limits; here they keep the size checks below meaningful)
  TORCH_CHECK(K >= 1 && K <= ia::kDqnCollectMaxSteps, "dqn_collect: ", hipGetErrorString(hipErrorInvalidValue),
              " (1..16 steps per launch, got ", K, ")");
  TORCH_CHECK(N >= 1 && S >= 1 && S * N < (int64_t(1) << 31) && pos0 >= 0 && pos0 < S, "dqn_collect: ring position / size");
  auto check = [](const torch::Tensor& t, c10::ScalarType dt, int64_t numel, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "dqn_collect: ", name, " must be a contiguous GPU tensor");
    TORCH_CHECK(t.scalar_type() == dt, "dqn_collect: dtype of ", name);
    TORCH_CHECK(t.numel() == numel, "dqn_collect: ", name, " has ", t.numel(), " elements, expected ", numel);
  };
  a.sdim = ia::state_size(a.P);
  check(env[0], torch::kFloat32, N * a.sdim, "state");
  check(env[1], torch::kInt64, N, "rng");
  check(env[2], torch::kInt32, N, "elapsed");
  check(env[3], torch::kFloat32, N, "ep_ret");
  check(env[4], torch::kFloat32, N * D, "cur_obs");
  check(act_rng, torch::kInt64, N, "act_rng");
  IA_CHECK_GPU_F32(params);
  check(err, torch::kInt32, 1, "err");
  const ia::DqnTdSrc r = td_source(ring, D, "ring");
  TORCH_CHECK(r.rows == S * N, "dqn_collect: the ring has ", r.rows, " rows, expected S * N = ", S * N);
  check(rec[0], torch::kFloat32, K * N, "records done");
  check(rec[1], torch::kFloat32, K * N, "records ep_ret");
  check(rec[2], torch::kInt32, K * N, "records ep_len");
  check(rec[3], torch::kInt64, K * N, "records action");
  if (rec_explore && rec_explore->defined()) {
    check(*rec_explore, torch::kInt32, K * N, "records explore");
    a.rec_explore = rec_explore->data_ptr<int>();
  }
  if (rec_q && rec_q->defined()) {
    check(*rec_q, torch::kFloat32, K * N * A, "records q");
    a.rec_q = rec_q->data_ptr<float>();
  }
  a.N = (int)N;
  a.K = (int)K;
  a.max_steps = (int)(max_steps < 0 ? ms : max_steps);
  a.D = (int)D;
  a.H1 = (int)H1;
  a.H2 = (int)H2;
  a.A = (int)A;
  for (int i = 0; i < 6; ++i) a.off[i] = (int)offsets[i];
  a.params = params.data_ptr<float>();
  a.n = params.numel();
  a.state = env[0].data_ptr<float>();
  a.rng = reinterpret_cast<uint64_t*>(env[1].data_ptr<int64_t>());
  a.elapsed = env[2].data_ptr<int>();
  a.ep_ret = env[3].data_ptr<float>();
  a.cur_obs = env[4].data_ptr<float>();
  a.act_rng = reinterpret_cast<uint64_t*>(act_rng.data_ptr<int64_t>());
  for (int64_t t = 0; t < K; ++t) {
    TORCH_CHECK(thr[t] >= 0 && thr[t] <= (int64_t(1) << 24), "dqn_collect: thresholds are 24-bit (0 .. 2^24)");
    a.thr[t] = (uint32_t)thr[t];
  }
  a.S = (int)S;
  a.pos0 = (int)pos0;
  a.r_obs = const_cast<float*>(r.obs);
  a.r_next = const_cast<float*>(r.next_obs);
  a.r_action = const_cast<int64_t*>(r.action);
  a.r_reward = const_cast<float*>(r.reward);
  a.r_done = const_cast<float*>(r.done);
  a.r_timeout = write_timeouts ? const_cast<float*>(r.timeout) : nullptr;
  a.use_reward_const = use_reward_const ? 1 : 0;
  a.reward_const = (float)reward_const;
  a.rec_done = rec[0].data_ptr<float>();
  a.rec_ep_ret = rec[1].data_ptr<float>();
  a.rec_ep_len = rec[2].data_ptr<int>();
  a.rec_action = rec[3].data_ptr<int64_t>();
  a.err = err.data_ptr<int>();
  const hipError_t e = ia::dqn_collect(a, ia_stream());
  TORCH_CHECK(e == hipSuccess, "dqn_collect: ", hipGetErrorString(e),
              " (limits: 1..16 steps, obs dim, hidden widths, actions in 1..64, a discrete-action vector env of that shape)");
}

}  // namespace

void register_dqn(py::module& m) {
  m.def("dqn_td_step", &dqn_td_step, py::arg("src_a"), py::arg("src_b"), py::arg("ids_a"), py::arg("ids_b"),
        py::arg("params"), py::arg("grads"), py::arg("exp_avg"), py::arg("exp_avg_sq"), py::arg("step"), py::arg("target"),
        py::arg("offsets"), py::arg("D"), py::arg("H1"), py::arg("H2"), py::arg("A"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("gamma"), py::arg("max_norm"), py::arg("losses"), py::arg("gnorm"),
        "All gradient steps of one DQN.train call (gather, target, forward, Huber loss, backward, clip, Adam) in one launch");
  m.def("dqn_collect", &dqn_collect, py::arg("env_id"), py::arg("max_steps"), py::arg("env"), py::arg("act_rng"),
        py::arg("ring"), py::arg("pos0"), py::arg("S"), py::arg("params"), py::arg("offsets"), py::arg("D"), py::arg("H1"),
        py::arg("H2"), py::arg("A"), py::arg("thr"), py::arg("use_reward_const"), py::arg("reward_const"),
        py::arg("write_timeouts"), py::arg("rec"), py::arg("rec_explore"), py::arg("rec_q"), py::arg("err"),
        "K steps of epsilon-greedy acting, env physics and replay-ring writes for N native envs in one launch");
}
