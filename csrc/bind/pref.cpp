// PrefRmPlan: the fused preference reward-model minibatch (csrc/kernels/pref_rm.hip + the
// AdamW of disc.hip). Built once per trainer / dataset store from a dict of persistent
// tensors (device-resident fragment dataset, reward-net weights and RunningNorm buffers, the
// FusedAdam flat parameters, moments and device step counter); a minibatch then passes only
// its pair ids: one pybind call, four launches, no host sync, HIP-graph capturable.
#include "plan_args.h"

#include <algorithm>

namespace {

class PrefRmPlan {
 public:
  explicit PrefRmPlan(py::dict d) : pd_(d, "pref") {
    a_ = ia::PrefRmArgs{};
    a_.L = pd_.get<int>("L");
    B_ = pd_.get<int>("batch");
    cap_ = pd_.get<int>("capacity");
    TORCH_CHECK(a_.L > 0 && B_ > 0 && cap_ >= B_, "fragment length, batch and capacity");
    a_.ds = pd_.get<int>("ds");
    a_.da = pd_.get<int>("da");
    a_.dns = pd_.get<int>("dns");
    const int use_done = pd_.get<int>("use_done");
    a_.din = a_.ds + a_.da + a_.dns + use_done;
    a_.s_all = pd_.fptr("s_all", a_.ds == 0);
    a_.a_all = pd_.fptr("a_all", a_.da == 0);
    a_.ns_all = pd_.fptr("ns_all", a_.dns == 0);
    a_.d_all = pd_.fptr("d_all", use_done == 0);
    a_.prefs_all = pd_.fptr("prefs_all");
    a_.gt_all = pd_.fptr("gt_all", true);
    // reward MLP: flat parameter order W0, b0, W1, b1, ... (the optimizer's flat buffer)
    a_.net = read_airl_net(pd_, "net", &a_.n_params);
    TORCH_CHECK(a_.net.dims[0] == a_.din, "reward-net input width ", a_.net.dims[0], " != gathered width ", a_.din);
    a_.rmean = pd_.fptr("rmean", true);
    a_.rvar = pd_.fptr("rvar", true);
    if (a_.rmean) a_.rcount = pd_.iptr("rcount");
    a_.eps = pd_.getf("eps");
    a_.discount = pd_.getf("discount");
    a_.threshold = pd_.getf("threshold");
    a_.noise = pd_.getf("noise");
    a_.gscale = (float)(1.0 / (double)B_);
    TORCH_CHECK(ia::pref_rm_plan(a_, plan_), "reward net outside the fused kernel's limits (widths <= 64, <= 4 layers, "
                                             "scalar head, <= 128 input columns)");
    // workspaces, sized for `capacity` pairs per minibatch
    const auto fo = torch::TensorOptions().dtype(torch::kFloat32).device(pd_.device());
    const int64_t rows = (int64_t)cap_ * 2 * a_.L;
    const int blocks = ia::pref_rm_blocks(cap_, a_.L);
    ws_.push_back(torch::empty({rows * a_.din}, fo));
    a_.X = ws_.back().data_ptr<float>();
    ws_.push_back(torch::empty({(int64_t)blocks * 2 * a_.din}, fo));
    a_.partials = ws_.back().data_ptr<float>();
    sums_ = torch::zeros({2 * a_.din}, fo.dtype(torch::kFloat64));
    a_.sums = sums_.data_ptr<double>();
    ws_.push_back(torch::zeros({1}, fo.dtype(torch::kInt32)));
    a_.cnt = reinterpret_cast<unsigned*>(ws_.back().data_ptr<int>());
    ws_.push_back(torch::zeros({256}, fo));
    a_.old_mv = ws_.back().data_ptr<float>();
    ws_.push_back(torch::zeros({1}, fo.dtype(torch::kInt32)));
    a_.old_cnt = ws_.back().data_ptr<int>();
    ws_.push_back(torch::zeros({256}, fo));
    a_.nrm = ws_.back().data_ptr<float>();
    ws_.push_back(torch::empty({rows}, fo));
    a_.r = ws_.back().data_ptr<float>();
    ws_.push_back(torch::empty({(int64_t)blocks * a_.n_params}, fo));
    a_.slab = ws_.back().data_ptr<float>();
    ws_.push_back(torch::zeros({(int64_t)cap_ * 8}, fo));
    a_.pstats = ws_.back().data_ptr<float>();
    grads_ = torch::zeros({a_.n_params}, fo);
    metrics_ = torch::zeros({8}, fo);
    // AdamW (disc.hip) on the optimizer's flat buffers, bias corrections from its device step
    ad_ = ia::DiscAdamArgs{};
    fill_adam(pd_, ad_, a_.n_params, "adam_eps", false);
    a_.step = pd_.fptr("step");
    ad_.step = a_.step;
    ad_.lr = pd_.getf("lr");
    ad_.decoupled = pd_.get<bool>("decoupled") ? 1 : 0;
    ad_.grads = grads_.data_ptr<float>();
    ad_.slab = a_.slab;
    ad_.stats_slab = a_.pstats;
  }

  int n_params() const { return a_.n_params; }
  int lds_bytes() const { return plan_.lds_bytes; }
  torch::Tensor sums() const { return sums_; }
  torch::Tensor grads() const { return grads_; }
  torch::Tensor metrics() const { return metrics_; }

  // single rank: gather, forward (+ RunningNorm merge), backward, AdamW -> metrics()
  // ([loss, accuracy, ground-truth loss] minibatch means)
  torch::Tensor step(torch::Tensor idx, bool merge) {
    ia::PrefRmArgs a = args(idx, merge);
    IA_HIP_CHECK(ia::pref_rm_gather(a, ia_stream()));
    IA_HIP_CHECK(ia::pref_rm_fwd(a, plan_, 0, ia_stream()));
    IA_HIP_CHECK(ia::pref_rm_bwd(a, plan_, ia_stream()));
    adam_launch(a, 1, 1);
    return metrics_;
  }
  // data-parallel pieces: gather (+ block sums -> sums()), forward from the all-reduced
  // sums of n_total rows, backward + slab reduction into grads() (all-reduce them), AdamW
  // gather (+ the column sums -> sums(): all-reduce them before forward(n_total > 0))
  void gather(torch::Tensor idx, bool merge) {
    ia::PrefRmArgs a = args(idx, merge);
    IA_HIP_CHECK(ia::pref_rm_gather(a, ia_stream()));
  }
  // moments from sums() over n_total rows (0: this rank's rows)
  void forward(torch::Tensor idx, bool merge, int n_total) {
    ia::PrefRmArgs a = args(idx, merge);
    IA_HIP_CHECK(ia::pref_rm_fwd(a, plan_, n_total, ia_stream()));
  }
  void backward(torch::Tensor idx, bool merge) {
    ia::PrefRmArgs a = args(idx, merge);
    IA_HIP_CHECK(ia::pref_rm_bwd(a, plan_, ia_stream()));
    adam_launch(a, 1, 0);
  }
  void apply(torch::Tensor idx) {
    ia::PrefRmArgs a = args(idx, false);
    adam_launch(a, 0, 1);
  }
  // One epoch (single rank) in one call -- capturable as ONE graph that is replayed per
  // epoch: minibatch mb takes pairs order[*cursor * P + mb * B, ...) (P pairs, batch B; the
  // last minibatch may be partial), its metrics go to ep[mb * 8 ...]; the epoch end copies
  // ep to all[*cursor] and advances the device cursor.
  void epoch(torch::Tensor order, int P, torch::Tensor cursor, torch::Tensor ep, torch::Tensor all, bool merge) {
    TORCH_CHECK(order.is_cuda() && order.is_contiguous() && order.scalar_type() == torch::kInt64, "order: int64 GPU");
    TORCH_CHECK(cursor.is_cuda() && cursor.scalar_type() == torch::kInt32 && cursor.numel() == 1, "cursor: int32 GPU [1]");
    const int n_mb = (P + B_ - 1) / B_;
    TORCH_CHECK(P > 0 && order.numel() >= P, "order holds fewer than P pairs");
    TORCH_CHECK(ep.is_cuda() && ep.scalar_type() == torch::kFloat32 && ep.numel() >= (int64_t)n_mb * 8, "ep: float32 [n_mb * 8]");
    TORCH_CHECK(all.is_cuda() && all.scalar_type() == torch::kFloat32 && all.numel() % ((int64_t)n_mb * 8) == 0,
                "all: float32 [epochs * n_mb * 8]");
    for (int mb = 0; mb < n_mb; ++mb) {
      ia::PrefRmArgs a = a_;
      a.n = std::min(B_, P - mb * B_);
      TORCH_CHECK(a.n <= cap_, "minibatch above capacity");
      a.idx = order.data_ptr<int64_t>() + (int64_t)mb * B_;
      a.cursor = cursor.data_ptr<int>();
      a.idx_stride = P;
      a.merge = merge ? 1 : 0;
      IA_HIP_CHECK(ia::pref_rm_gather(a, ia_stream()));
      IA_HIP_CHECK(ia::pref_rm_fwd(a, plan_, 0, ia_stream()));
      IA_HIP_CHECK(ia::pref_rm_bwd(a, plan_, ia_stream()));
      adam_launch(a, 1, 1, ep.data_ptr<float>() + (int64_t)mb * 8);
    }
    IA_HIP_CHECK(ia::pref_rm_epoch_end(ep.data_ptr<float>(), all.data_ptr<float>(), n_mb * 8, cursor.data_ptr<int>(),
                                         ia_stream()));
  }

 private:
  ia::PrefRmArgs args(const torch::Tensor& idx, bool merge) {
    TORCH_CHECK(idx.is_cuda() && idx.is_contiguous() && idx.scalar_type() == torch::kInt64 && idx.dim() == 1,
                "idx: int64 GPU vector");
    TORCH_CHECK(idx.numel() > 0 && idx.numel() <= cap_, "minibatch of ", idx.numel(), " pairs (capacity ", cap_, ")");
    ia::PrefRmArgs a = a_;
    a.n = (int)idx.numel();
    a.idx = idx.data_ptr<int64_t>();
    a.merge = merge ? 1 : 0;
    return a;
  }
  void adam_launch(const ia::PrefRmArgs& a, int reduce, int do_adam, float* stats_out = nullptr) {
    ia::DiscAdamArgs d = ad_;
    d.nblk = ia::pref_rm_blocks(a.n, a.L);
    d.stats_nblk = a.n;
    d.stats_scale = 1.f / (float)a.n;
    launch_disc_adam(d, reduce, do_adam, reduce ? (stats_out ? stats_out : metrics_.data_ptr<float>()) : nullptr);
  }
  PlanDict pd_;
  std::vector<torch::Tensor> ws_;
  torch::Tensor sums_, grads_, metrics_;
  ia::PrefRmArgs a_{};
  ia::PrefPlan plan_{};
  ia::DiscAdamArgs ad_{};
  int B_ = 0, cap_ = 0;
};

}  // namespace

void register_pref(py::module& m) {
  py::class_<PrefRmPlan>(m, "PrefRmPlan")
      .def(py::init<py::dict>())
      .def_property_readonly("n_params", &PrefRmPlan::n_params)
      .def_property_readonly("lds_bytes", &PrefRmPlan::lds_bytes)
      .def_property_readonly("sums", &PrefRmPlan::sums)
      .def_property_readonly("grads", &PrefRmPlan::grads)
      .def_property_readonly("metrics", &PrefRmPlan::metrics)
      .def("step", &PrefRmPlan::step, py::arg("idx"), py::arg("merge"))
      .def("gather", &PrefRmPlan::gather, py::arg("idx"), py::arg("merge"))
      .def("forward", &PrefRmPlan::forward, py::arg("idx"), py::arg("merge"), py::arg("n_total"))
      .def("backward", &PrefRmPlan::backward, py::arg("idx"), py::arg("merge"))
      .def("apply", &PrefRmPlan::apply, py::arg("idx"))
      .def("epoch", &PrefRmPlan::epoch, py::arg("order"), py::arg("P"), py::arg("cursor"), py::arg("ep"), py::arg("all"),
           py::arg("merge"));
}
