// What the plan classes of the fused reward updates (DiscPlan, AirlDiscPlan, PrefRmPlan) share:
// reading persistent tensors out of the constructor's dict, the AirlNet and transition-source
// parsers, and the DiscAdamArgs of the closing disc_adam launch.
#pragma once
#include "common.h"
#include "launchers.h"

// The constructor dict of a plan. Every tensor read through it is checked (contiguous, on the
// GPU, dtype) and kept alive for the plan's lifetime; `plan` names the plan in the messages.
class PlanDict {
 public:
  PlanDict(py::dict d, const char* plan) : d_(std::move(d)), plan_(plan) {}

  torch::Tensor keep(const char* k, bool optional = false) {
    if (!d_.contains(k) || d_[k].is_none()) {
      TORCH_CHECK(optional, plan_, " plan arg missing: ", k);
      return torch::Tensor();
    }
    auto t = d_[k].cast<torch::Tensor>();
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), plan_, " plan arg ", k, " must be a contiguous GPU tensor");
    held_.push_back(t);
    return t;
  }
  float* fptr(const char* k, bool optional = false) { return ptr<float>(k, optional, torch::kFloat32, " must be float32"); }
  int* iptr(const char* k, bool optional = false) { return ptr<int>(k, optional, torch::kInt32, " must be int32"); }
  // the tensor read last (k) holds at least numel elements
  void need(const char* k, int64_t numel) const {
    TORCH_CHECK(held_.back().numel() >= numel, plan_, " plan arg ", k, " too small: ", held_.back().numel(), " < ", numel);
  }
  template <class T>
  T get(const char* k) const {
    return d_[k].cast<T>();
  }
  float getf(const char* k) const { return (float)d_[k].cast<double>(); }
  void hold(const torch::Tensor& t) { held_.push_back(t); }
  const torch::Tensor& last() const { return held_.back(); }
  torch::Device device() const { return held_.front().device(); }

 private:
  template <class T>
  T* ptr(const char* k, bool optional, torch::ScalarType st, const char* what) {
    auto t = keep(k, optional);
    if (!t.defined()) return nullptr;
    TORCH_CHECK(t.scalar_type() == st, k, what);
    return t.data_ptr<T>();
  }
  py::dict d_;
  const char* plan_;
  std::vector<torch::Tensor> held_;
};

// An MLP {"W": [...], "b": [...], "hidden_act": int} under key k. off (reward nets): the net's
// offset in the flat parameter order W0, b0, W1, b1, ..., advanced past it.
inline ia::AirlNet read_airl_net(PlanDict& pd, const char* k, int* off) {
  py::dict nd = pd.get<py::dict>(k);
  auto Ws = nd["W"].cast<std::vector<torch::Tensor>>();
  auto bs = nd["b"].cast<std::vector<torch::Tensor>>();
  TORCH_CHECK(!Ws.empty() && Ws.size() <= (size_t)ia::kAirlMaxLayers && Ws.size() == bs.size(), k, ": 1..4 layers");
  ia::AirlNet n{};
  n.n_layers = (int)Ws.size();
  n.dims[0] = (int)Ws[0].size(1);
  n.hidden_act = nd["hidden_act"].cast<int>();
  n.param_off = off ? *off : 0;
  int o = 0;
  for (size_t l = 0; l < Ws.size(); ++l) {
    TORCH_CHECK(Ws[l].is_cuda() && Ws[l].is_contiguous() && Ws[l].scalar_type() == torch::kFloat32, k, " weights");
    TORCH_CHECK(l == 0 || Ws[l].size(1) == Ws[l - 1].size(0), k, ": layer widths do not chain");
    pd.hold(Ws[l]);
    pd.hold(bs[l]);
    n.dims[l + 1] = (int)Ws[l].size(0);
    n.W[l] = Ws[l].data_ptr<float>();
    n.b[l] = bs[l].data_ptr<float>();
    n.w_off[l] = o;
    o += (int)Ws[l].numel();
    n.b_off[l] = o;
    o += (int)bs[l].numel();
  }
  if (off) *off += o;
  return n;
}

// The expert ("e_*") and generator ("g_*") transition sources.
inline void read_transition_srcs(PlanDict& pd, bool act_discrete, ia::TransitionSrc& e, ia::TransitionSrc& g) {
  e = g = ia::TransitionSrc{};
  e.obs = pd.fptr("e_obs");
  e.next_obs = pd.fptr("e_next_obs");
  e.dones = reinterpret_cast<const bool*>(pd.keep("e_dones").data_ptr());
  g.obs = pd.fptr("g_obs");
  g.next_obs = pd.fptr("g_next_obs");
  g.dones = reinterpret_cast<const bool*>(pd.keep("g_dones").data_ptr());
  if (act_discrete) {
    e.acts_i = pd.keep("e_acts").data_ptr<int64_t>();
    g.acts_i = pd.keep("g_acts").data_ptr<int64_t>();
  } else {
    e.acts = pd.fptr("e_acts");
    g.acts = pd.fptr("g_acts");
  }
}

// The reward-net input layout ("obs_dim", aw_key, "use_*", "act_discrete") and its width.
inline ia::RewardInputLayout read_input_layout(const PlanDict& pd, const char* aw_key) {
  ia::RewardInputLayout in{};
  in.D = pd.get<int>("obs_dim");
  in.aw = pd.get<int>(aw_key);
  in.use_state = pd.get<int>("use_state");
  in.use_action = pd.get<int>("use_action");
  in.use_next_state = pd.get<int>("use_next_state");
  in.use_done = pd.get<int>("use_done");
  in.act_discrete = pd.get<int>("act_discrete");
  return in;
}
inline int input_width(const ia::RewardInputLayout& in) {
  return in.use_state * in.D + in.use_action * in.aw + in.use_next_state * in.D + in.use_done;
}

// Adam on the flat buffers "params" (exactly / at least n_params elements), "exp_avg",
// "exp_avg_sq" with "beta1", "beta2", eps_key and "weight_decay".
inline void fill_adam(PlanDict& pd, ia::DiscAdamArgs& a, int n_params, const char* eps_key, bool exact) {
  a.n_params = n_params;
  a.params = pd.fptr("params");
  const int64_t got = pd.last().numel();
  TORCH_CHECK(exact ? got == n_params : got >= n_params, "flat params size ", got, exact ? " != " : " < ", n_params);
  a.exp_avg = pd.fptr("exp_avg");
  a.exp_avg_sq = pd.fptr("exp_avg_sq");
  a.beta1 = pd.getf("beta1");
  a.beta2 = pd.getf("beta2");
  a.eps = pd.getf(eps_key);
  a.weight_decay = pd.getf("weight_decay");
}
// The slab reduction of n_mb minibatches of fb_blocks rows each (statistics: the last minibatch's).
inline void fill_slab_reduce(ia::DiscAdamArgs& a, int n_mb, int fb_blocks, const float* slab, const float* stats_slab) {
  a.nblk = n_mb * fb_blocks;
  a.stats_nblk = fb_blocks;
  a.slab = slab;
  a.stats_slab = stats_slab + (size_t)(n_mb - 1) * fb_blocks * ia::kDiscStats;
}

inline float* checked_stats_out(const c10::optional<torch::Tensor>& t) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->numel() >= ia::kDiscStats && t->is_contiguous(),
              "stats_out must be a float32 GPU tensor of >= 8 elements");
  return t->data_ptr<float>();
}
// reduce=1: slab -> grads (adam=0) or straight into Adam (adam=1); reduce=0: Adam from grads.
inline void launch_disc_adam(ia::DiscAdamArgs a, int reduce, int do_adam, float* stats_out) {
  a.reduce = reduce;
  a.adam = do_adam;
  a.stats_out = stats_out;
  IA_HIP_CHECK(ia::disc_adam(a, ia_stream()));
}

inline void check_batch_idx(const torch::Tensor& t, int batch) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kInt64 && t.numel() >= batch,
              "indices must be int64 GPU tensors of >= batch entries");
}
