// The torch-op layer over the C ABI (SURVEY.md §8(b) "torch op wrapper"): the sampling path's objects and
// entry points registered with the dispatcher (TORCH_LIBRARY), so torch-native callers (TorchScript, C++
// frontends, torch.compile graphs) build and drive the sampler without the Python ctypes binding:
//   * torch.classes.chemeleon.Model / Batch / Schedule (torch::CustomClassHolder, reference-counted): the
//     packed decoder weights (chm_model), a crystal batch with its workspace (chm_batch; it holds its Model),
//     and the per-timestep tables (chm_schedule; it holds its tensors). An op takes these objects, never a raw
//     address, so nothing it reads can be freed under it;
//   * every launch goes on the current HIP stream of the batch's device, under a device guard for that
//     device; every tensor must live on that device (checked on the host before any launch);
//   * a Batch is scratch for one stream at a time: an op on another stream than the batch's last one first
//     makes its stream wait for the last one's work (an event) and records the workspace as used on it
//     (record_stream), so uses on several streams are ordered and the caching allocator reuses the
//     workspace only after every stream that used it is done;
//   * outputs and workspaces come from the PyTorch caching allocator (at::empty);
//   * shapes, dtypes and devices are checked on the host, the C ABI checks element counts again, and a
//     failing call raises through TORCH_CHECK with chm_last_error() (RuntimeError in Python).
// The reference interfaces these replace: CSPNet.__init__ / load_state_dict and CSPNet.forward
// (chemeleon/modules/cspnet.py:185-234, 345-405), one reverse step of Chemeleon._sample_generator
// (chemeleon/modules/chemeleon.py:379-466) with its schedule buffers (chemeleon/utils/diff_utils.py:57-185),
// scatter_mean (chemeleon/utils/scatter.py:88-112) and D3PM.p_logits (chemeleon/utils/diff_utils.py:307-329).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/hip/HIPStream.h>
#include <torch/custom_class.h>
#include <torch/library.h>

#include <hip/hip_runtime_api.h>

#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/chemeleon_hip.h"

namespace {

using c10::hip::HIPGuardMasqueradingAsCUDA;

void* stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }

void check(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " failed (code ", rc, "): ", chm_last_error()); }

void need(const at::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, ": chemeleon ops run on a HIP device only (no CPU fallback)");
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": expected a contiguous tensor");
}

void need_on(const at::Tensor& t, const c10::Device& dev, at::ScalarType dt, const char* name) {
  need(t, dt, name);
  TORCH_CHECK(t.device() == dev, name, " is on ", t.device(), ", the batch on ", dev);
}

void need_shape(const at::Tensor& t, at::IntArrayRef shape, const char* name) {
  TORCH_CHECK(t.sizes() == shape, name, ": expected shape ", shape, ", got ", t.sizes());
}

// ---------------------------------------------------------------- objects
struct Model : torch::CustomClassHolder {
  chm_model* m = nullptr;
  chm_dims d{};
  c10::Device device{c10::kCUDA, 0};

  // params: the decoder's state_dict tensors in order (chm_model_create), fp32 contiguous on one HIP device
  Model(std::vector<at::Tensor> params, int64_t hidden_dim, int64_t time_dim, int64_t text_dim, int64_t num_layers,
        int64_t max_atoms, int64_t num_freqs) {
    TORCH_CHECK(!params.empty(), "Model: no parameter tensors");
    device = params[0].device();
    for (size_t i = 0; i < params.size(); ++i) need_on(params[i], device, at::kFloat, "Model parameter");
    d = chm_dims{(int)hidden_dim, (int)time_dim, (int)text_dim, (int)num_layers, (int)max_atoms, (int)num_freqs};
    HIPGuardMasqueradingAsCUDA guard(device);
    std::vector<const float*> ptrs;
    for (auto& p : params) ptrs.push_back(p.data_ptr<float>());
    check(chm_model_create(&d, ptrs.data(), (int)ptrs.size(), stream(), &m), "chm_model_create");
  }
  ~Model() override {
    if (m) chm_model_destroy(m);
  }
  void set_math(const std::string& mode) {
    const int code = mode == "split16" ? CHM_MATH_SPLIT16 : mode == "bf16x3" ? CHM_MATH_BF16X3 : mode == "f32" ? CHM_MATH_F32 : -1;
    TORCH_CHECK(code >= 0, "set_math: 'split16', 'bf16x3' or 'f32', got '", mode, "'");
    check(chm_model_set_math(m, code), "chm_model_set_math");
  }
  std::string get_math() const {
    const int c = chm_model_get_math(m);
    return c == CHM_MATH_SPLIT16 ? "split16" : c == CHM_MATH_BF16X3 ? "bf16x3" : "f32";
  }
  void set_option(const std::string& key, int64_t value) { check(chm_model_set_option(m, key.c_str(), value), "chm_model_set_option"); }
};

struct Batch : torch::CustomClassHolder {
  c10::intrusive_ptr<Model> model;  // the weights outlive every batch built on them
  at::Tensor workspace;             // caller-owned workspace (caching allocator), freed after the batch
  chm_batch* b = nullptr;
  int64_t N = 0, E = 0, B = 0;
  int P = 0, knn = 0;
  std::mutex mu;                    // guards last / ev (ops from several host threads)
  hipStream_t last = nullptr;       // the stream of the last op on this batch (creation: its stream)
  hipEvent_t ev = nullptr;

  // natoms: atoms per crystal; max_pairs 1 (plain decoder calls) or 2 (CFG pairs, sampling); knn: the
  // reference's radius graph instead of fc edges (max_neighbors as CSPNet's)
  Batch(c10::intrusive_ptr<Model> model_, std::vector<int64_t> natoms, int64_t max_pairs, bool knn_edges,
        int64_t max_neighbors)
      : model(std::move(model_)) {
    TORCH_CHECK(!natoms.empty(), "Batch: natoms is empty");
    std::vector<int32_t> nat;
    for (int64_t n : natoms) {
      TORCH_CHECK(n >= 1 && n <= (1 << 20), "Batch: atoms per crystal must be in [1, 2^20], got ", n);
      nat.push_back((int32_t)n);
    }
    chm_batch_options opts{knn_edges ? CHM_EDGES_KNN : CHM_EDGES_FC, (int32_t)max_neighbors, 0, 0};
    const size_t need_b = chm_batch_workspace_bytes_ex(model->m, nat.data(), (int)nat.size(), (int)max_pairs, &opts);
    TORCH_CHECK(need_b > 0, "chm_batch_workspace_bytes_ex failed: ", chm_last_error());
    HIPGuardMasqueradingAsCUDA guard(model->device);
    workspace = at::empty({(int64_t)need_b}, at::TensorOptions().dtype(at::kByte).device(model->device));
    check(chm_batch_create_ex(model->m, nat.data(), (int)nat.size(), (int)max_pairs, &opts, workspace.data_ptr(), need_b,
                              stream(), &b),
          "chm_batch_create_ex");
    chm_dims d;
    check(chm_batch_info(b, &d, &B, &P, &knn), "chm_batch_info");
    TORCH_CHECK(chm_batch_device(b) == model->device.index(), "Batch: the library placed the batch on device ",
                chm_batch_device(b), ", the model is on ", model->device);
    N = chm_batch_num_nodes(b);
    E = chm_batch_num_edges(b);
    last = (hipStream_t)stream();
    TORCH_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess, "Batch: hipEventCreate failed");
  }
  ~Batch() override {
    if (b) chm_batch_destroy(b);
    if (ev) (void)hipEventDestroy(ev);
  }
  // called under the device guard, before an op launches on the current stream: order it behind the work of the
  // batch's last stream and keep the workspace alive for this stream (caching allocator)
  void use_current_stream() {
    // (the CUDA-typed view of the HIP stream: PyTorch-ROCm's caching allocator keys streams as CUDA)
    const c10::hip::HIPStreamMasqueradingAsCUDA cur = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA();
    std::lock_guard<std::mutex> lk(mu);
    if (cur.stream() == last) return;
    TORCH_CHECK(hipEventRecord(ev, last) == hipSuccess && hipStreamWaitEvent(cur.stream(), ev, 0) == hipSuccess,
                "Batch: ordering the batch's previous stream before this one failed");
    workspace.record_stream(cur.unwrap());
    last = cur.stream();
  }
  const chm_dims& dims() const { return model->d; }
  const c10::Device& device() const { return model->device; }
  int64_t num_nodes() const { return N; }
  int64_t num_edges() const { return E; }
  int64_t num_graphs() const { return B; }
};

struct Schedule : torch::CustomClassHolder {
  at::Tensor coef, time_emb, q_one_step, q_mats;  // held: chm_schedule points into them
  chm_schedule s{};

  // coef [T+1, 8], time_emb [T+1, time_dim], q_one_step / q_mats [T+1, A, A] (Chemeleon.schedule_tables)
  Schedule(at::Tensor coef_, at::Tensor time_emb_, at::Tensor q_one_step_, at::Tensor q_mats_)
      : coef(std::move(coef_)), time_emb(std::move(time_emb_)), q_one_step(std::move(q_one_step_)),
        q_mats(std::move(q_mats_)) {
    const c10::Device dev = coef.device();
    need_on(coef, dev, at::kFloat, "coef");
    need_on(time_emb, dev, at::kFloat, "time_emb");
    need_on(q_one_step, dev, at::kFloat, "q_one_step");
    need_on(q_mats, dev, at::kFloat, "q_mats");
    TORCH_CHECK(coef.dim() == 2 && coef.size(1) == 8 && coef.size(0) >= 2, "coef must be [T+1, 8]");
    const int64_t T1 = coef.size(0);
    TORCH_CHECK(time_emb.dim() == 2 && time_emb.size(0) == T1, "time_emb must be [T+1, time_dim]");
    TORCH_CHECK(q_mats.dim() == 3 && q_mats.size(0) == T1 && q_mats.size(1) == q_mats.size(2) &&
                    q_one_step.sizes() == q_mats.sizes(),
                "q_one_step / q_mats must be [T+1, A, A]");
    s.T = (int)(T1 - 1);
    s.num_classes = (int)q_mats.size(1);
    s.time_dim = (int)time_emb.size(1);
    s.d_coef = coef.data_ptr<float>();
    s.d_time_emb = time_emb.data_ptr<float>();
    s.d_q_one_step = q_one_step.data_ptr<float>();
    s.d_q_mats = q_mats.data_ptr<float>();
  }
  int64_t num_timesteps() const { return s.T; }
};

// ---------------------------------------------------------------- ops
void need_state(const Batch& b, const at::Tensor& a, const at::Tensor& x, const at::Tensor& l) {
  need_on(a, b.device(), at::kLong, "atom_types");
  need_on(x, b.device(), at::kFloat, "frac");
  need_on(l, b.device(), at::kFloat, "lattices");
  need_shape(a, {b.N}, "atom_types");
  need_shape(x, {b.N, 3}, "frac");
  need_shape(l, {b.B, 3, 3}, "lattices");
}

const float* fptr_on(const c10::optional<at::Tensor>& t, const Batch& b, const char* name) {
  if (!t.has_value()) return nullptr;
  need_on(*t, b.device(), at::kFloat, name);
  return t->data_ptr<float>();
}

// CSPNet.forward for `pairs` conditionings sharing atoms / coordinates / lattices (pairs = 2: the CFG pair
// of Chemeleon.model_predictions): time_emb [B, >= time_dim] (row stride = its last size), text
// [pairs, B, text_dim] -> (types [pairs,N,max_atoms], lattice [pairs,B,3,3], coords [pairs,N,3],
// node features [pairs,N,hidden_dim])
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> decoder_forward(const c10::intrusive_ptr<Batch>& bp,
                                                                           int64_t pairs, const at::Tensor& atom_types,
                                                                           const at::Tensor& frac,
                                                                           const at::Tensor& lattices,
                                                                           const c10::optional<at::Tensor>& time_emb,
                                                                           const c10::optional<at::Tensor>& text) {
  const Batch& b = *bp;
  const chm_dims& d = b.dims();
  TORCH_CHECK(pairs >= 1 && pairs <= b.P, "pairs must be in [1, ", b.P, "] for this batch");
  need_state(b, atom_types, frac, lattices);
  const bool film = d.time_dim > 0 || d.text_dim > 0;
  int64_t tstride = 0;
  if (film) {
    TORCH_CHECK(time_emb.has_value(), "time_emb is required (the model has a FiLM layer)");
    TORCH_CHECK(time_emb->dim() == 2 && time_emb->size(0) == b.B && time_emb->size(1) >= d.time_dim,
                "time_emb must be [B, >= time_dim]");
    tstride = time_emb->size(1);
  }
  if (d.text_dim > 0) {
    TORCH_CHECK(text.has_value(), "text embeddings are required (text_dim > 0)");
    need_shape(*text, {pairs, b.B, d.text_dim}, "text");
  }
  const float* te = film ? fptr_on(time_emb, b, "time_emb") : nullptr;
  const float* tx = d.text_dim > 0 ? fptr_on(text, b, "text") : nullptr;
  HIPGuardMasqueradingAsCUDA guard(b.device());
  bp->use_current_stream();
  auto o = frac.options();
  at::Tensor types = at::empty({pairs, b.N, d.max_atoms}, o), latt = at::empty({pairs, b.B, 3, 3}, o),
             coords = at::empty({pairs, b.N, 3}, o), nodes = at::empty({pairs, b.N, d.hidden_dim}, o);
  check(chm_decoder_forward(b.b, (int)pairs, atom_types.data_ptr<int64_t>(), frac.data_ptr<float>(),
                            lattices.data_ptr<float>(), te, (int)tstride, tx, types.data_ptr<float>(),
                            latt.data_ptr<float>(), coords.data_ptr<float>(), nodes.data_ptr<float>(), stream()),
        "chm_decoder_forward");
  return {types, latt, coords, nodes};
}

// One reverse step t -> t-1, state updated in place. Noise tensors given: the reference's CPU stream
// (parity mode); absent: device Philox noise keyed by (seed, t, global index).
void sample_step(const c10::intrusive_ptr<Batch>& bp, const c10::intrusive_ptr<Schedule>& sp, int64_t t,
                 double cond_scale, at::Tensor atom_types, at::Tensor frac, at::Tensor lattices,
                 const c10::optional<at::Tensor>& cond, const c10::optional<at::Tensor>& null,
                 const c10::optional<at::Tensor>& rand_a, const c10::optional<at::Tensor>& rand_l,
                 const c10::optional<at::Tensor>& rand_x1, const c10::optional<at::Tensor>& rand_x2, int64_t seed,
                 int64_t node_base, int64_t graph_base) {
  const Batch& b = *bp;
  const Schedule& sc = *sp;
  const chm_dims& d = b.dims();
  TORCH_CHECK(b.P >= 2, "sample_step needs a batch created for 2 pairs (the CFG pair)");
  TORCH_CHECK(sc.coef.device() == b.device(), "schedule is on ", sc.coef.device(), ", the batch on ", b.device());
  TORCH_CHECK(sc.s.num_classes == d.max_atoms && sc.s.time_dim == d.time_dim, "schedule tables (A = ", sc.s.num_classes,
              ", time_dim = ", sc.s.time_dim, ") do not match the model (", d.max_atoms, ", ", d.time_dim, ")");
  TORCH_CHECK(t >= 1 && t <= sc.s.T, "t must be in [1, ", sc.s.T, "]");
  need_state(b, atom_types, frac, lattices);
  const bool guide = d.text_dim > 0;
  TORCH_CHECK(cond.has_value() == guide && null.has_value() == guide,
              guide ? "cond and null text embeddings are required" : "this model takes no text embeddings");
  if (guide) {
    need_shape(*cond, {b.B, d.text_dim}, "cond");
    need_shape(*null, {b.B, d.text_dim}, "null");
  }
  const bool noise = rand_a.has_value();
  TORCH_CHECK(noise == rand_l.has_value() && noise == rand_x1.has_value() && noise == rand_x2.has_value(),
              "pass all four noise tensors (parity mode) or none (device noise)");
  if (noise) {
    need_shape(*rand_a, {b.N, d.max_atoms}, "rand_a");
    need_shape(*rand_l, {b.B, 3, 3}, "rand_l");
    need_shape(*rand_x1, {b.N, 3}, "rand_x1");
    need_shape(*rand_x2, {b.N, 3}, "rand_x2");
  }
  chm_step_io io{};
  io.d_atom_types = atom_types.data_ptr<int64_t>(); io.n_atom_types = atom_types.numel();
  io.d_frac = frac.data_ptr<float>(); io.n_frac = frac.numel();
  io.d_lattices = lattices.data_ptr<float>(); io.n_lattices = lattices.numel();
  io.d_cond = fptr_on(cond, b, "cond"); io.n_cond = guide ? cond->numel() : 0;
  io.d_null = fptr_on(null, b, "null"); io.n_null = guide ? null->numel() : 0;
  io.d_rand_a = fptr_on(rand_a, b, "rand_a"); io.n_rand_a = noise ? rand_a->numel() : 0;
  io.d_rand_l = fptr_on(rand_l, b, "rand_l"); io.n_rand_l = noise ? rand_l->numel() : 0;
  io.d_rand_x1 = fptr_on(rand_x1, b, "rand_x1"); io.n_rand_x1 = noise ? rand_x1->numel() : 0;
  io.d_rand_x2 = fptr_on(rand_x2, b, "rand_x2"); io.n_rand_x2 = noise ? rand_x2->numel() : 0;
  HIPGuardMasqueradingAsCUDA guard(b.device());
  bp->use_current_stream();
  check(chm_sample_step(b.b, &sc.s, (int)t, (float)cond_scale, &io, (uint64_t)seed, node_base, graph_base, stream()),
        "chm_sample_step");
}

// scatter_mean of per-edge messages [pairs,E,hidden_dim] onto their source nodes -> [pairs,N,hidden_dim]
at::Tensor segment_mean(const c10::intrusive_ptr<Batch>& bp, int64_t pairs, const at::Tensor& msg) {
  const Batch& b = *bp;
  TORCH_CHECK(!b.knn, "segment_mean: fc batches only");
  TORCH_CHECK(pairs >= 1, "pairs must be >= 1");
  need_on(msg, b.device(), at::kFloat, "msg");
  need_shape(msg, {pairs, b.E, b.dims().hidden_dim}, "msg");
  HIPGuardMasqueradingAsCUDA guard(b.device());
  bp->use_current_stream();
  at::Tensor agg = at::empty({pairs, b.N, b.dims().hidden_dim}, msg.options());
  check(chm_segment_mean(b.b, (int)pairs, msg.data_ptr<float>(), msg.numel(), agg.data_ptr<float>(), agg.numel(),
                         stream()),
        "chm_segment_mean");
  return agg;
}

// D3PM reverse sampling (Gumbel argmax of the posterior logits) for explicit inputs -> [N] int64. t and x_t are
// range-checked on the device (the call synchronises the stream); an out-of-range index raises.
at::Tensor d3pm_sample(const at::Tensor& logits, const at::Tensor& xt, const at::Tensor& t, const at::Tensor& noise,
                       const at::Tensor& q_one_step, const at::Tensor& q_mats) {
  const c10::Device dev = logits.device();
  need_on(logits, dev, at::kFloat, "logits");
  need_on(xt, dev, at::kLong, "x_t");
  need_on(t, dev, at::kLong, "t");
  need_on(noise, dev, at::kFloat, "noise");
  need_on(q_one_step, dev, at::kFloat, "q_one_step");
  need_on(q_mats, dev, at::kFloat, "q_mats");
  TORCH_CHECK(logits.dim() == 2 && noise.sizes() == logits.sizes(), "logits / noise must be [N, A]");
  const int64_t N = logits.size(0), A = logits.size(1);
  TORCH_CHECK(A >= 1 && A <= 128, "at most 128 classes");
  TORCH_CHECK(xt.numel() == N && t.numel() == N, "x_t / t must have N entries");
  TORCH_CHECK(q_mats.dim() == 3 && q_mats.size(1) == A && q_mats.size(2) == A && q_one_step.sizes() == q_mats.sizes(),
              "q tables must be [T+1, A, A]");
  HIPGuardMasqueradingAsCUDA guard(dev);
  at::Tensor out = at::empty({N}, xt.options());
  check(chm_d3pm_sample((int)N, (int)A, (int)q_mats.size(0) - 1, logits.data_ptr<float>(), xt.data_ptr<int64_t>(),
                        t.data_ptr<int64_t>(), noise.data_ptr<float>(), q_one_step.data_ptr<float>(),
                        q_mats.data_ptr<float>(), out.data_ptr<int64_t>(), stream()),
        "chm_d3pm_sample");
  return out;
}

// ---------------------------------------------------------------- finishing legs
// screen, dedup, cell, symmetry, primitive, match, match_group and match_set share what stands between here and the first of them:
// the checks of a state against its crystal list, the optional exclude / require tensors, and one plan cache.
// A cache keeps the plans of the last 8 (crystal lists, device) keys, evicts the oldest first and lives as long
// as the process (nothing is freed during static destruction, when the HIP runtime may be gone). It hands out
// shared_ptrs: an op holds its entry until its chm_*_run calls have returned, so an entry that another host
// thread evicts meanwhile is destroyed after that, never under the call.
constexpr float kMatchCellSymprec = 0.1f, kMatchCellAngleTolerance = 10.0f;  // the cell pass in front of the matcher

using Lists = std::vector<std::vector<int64_t>>;  // a cache key: natoms (match: natoms, ref_natoms, ref_of)

// a crystal list as the C ABI takes it; `op` and `what` word the refusal ("screen: atoms per crystal ...")
std::vector<int32_t> to_int32(const std::vector<int64_t>& natoms, const char* op, const char* what) {
  std::vector<int32_t> nat;
  for (int64_t n : natoms) {
    TORCH_CHECK(n >= 1 && n <= INT32_MAX, op, ": atoms per ", what, " must be >= 1, got ", n);
    nat.push_back((int32_t)n);
  }
  return nat;
}

// a chm_* handle that is destroyed with its owner (every chm_*_destroy takes NULL)
template <class T, void (*Destroy)(T*)>
struct Handle {
  T* p = nullptr;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() { Destroy(p); }
};
using CellHandle = Handle<chm_cell, chm_cell_destroy>;

// Entry: default-constructible, create(key) builds its handles or raises (what it had built goes with it)
template <class Entry>
std::shared_ptr<Entry> cached_plan(const Lists& key, int device) {
  struct Cache {
    std::mutex mu;
    std::vector<std::tuple<Lists, int, std::shared_ptr<Entry>>> plans;
  };
  static Cache* cache = new Cache;
  std::lock_guard<std::mutex> lk(cache->mu);
  for (auto& e : cache->plans)
    if (std::get<1>(e) == device && std::get<0>(e) == key) return std::get<2>(e);
  auto entry = std::make_shared<Entry>();
  entry->create(key);
  if (cache->plans.size() >= 8) cache->plans.erase(cache->plans.begin());
  cache->plans.emplace_back(key, device, entry);
  return entry;
}

struct Crystals {
  int64_t N, B;
};

// a state's tensors (atom_types may be absent: cell) on `dev`, then their shapes for `natoms`; `pre` = "ref_" for
// the reference lists of match
void need_crystals_on(const c10::Device& dev, const at::Tensor* atom_types, const at::Tensor& frac,
                      const at::Tensor& lattices, const std::string& pre = "") {
  if (atom_types) need_on(*atom_types, dev, at::kLong, (pre + "atom_types").c_str());
  need_on(frac, dev, at::kFloat, (pre + "frac").c_str());
  need_on(lattices, dev, at::kFloat, (pre + "lattices").c_str());
}

Crystals need_crystals_shape(const std::vector<int64_t>& natoms, const at::Tensor* atom_types, const at::Tensor& frac,
                             const at::Tensor& lattices, const std::string& pre = "") {
  int64_t N = 0;
  for (int64_t n : natoms) N += n;
  const int64_t B = (int64_t)natoms.size();
  if (atom_types) need_shape(*atom_types, {N}, (pre + "atom_types").c_str());
  need_shape(frac, {N, 3}, (pre + "frac").c_str());
  need_shape(lattices, {B, 3, 3}, (pre + "lattices").c_str());
  return {N, B};
}

Crystals need_crystals(const c10::Device& dev, const std::vector<int64_t>& natoms, const at::Tensor* atom_types,
                       const at::Tensor& frac, const at::Tensor& lattices) {
  need_crystals_on(dev, atom_types, frac, lattices);
  return need_crystals_shape(natoms, atom_types, frac, lattices);
}

// exclude: a bool / uint8 tensor [B] of crystals that take no part, or None (NULL)
const uint8_t* optional_exclude(const c10::optional<at::Tensor>& exclude, const c10::Device& dev, int64_t B) {
  if (!exclude.has_value()) return nullptr;
  TORCH_CHECK(exclude->scalar_type() == at::kBool || exclude->scalar_type() == at::kByte,
              "exclude: expected bool or uint8, got ", exclude->scalar_type());
  need_on(*exclude, dev, exclude->scalar_type(), "exclude");
  need_shape(*exclude, {B}, "exclude");
  return static_cast<const uint8_t*>(exclude->data_ptr());
}

// require: the wanted system codes, int32 [1] or [B], or None (NULL, 0)
std::pair<const int32_t*, int64_t> optional_require(const c10::optional<at::Tensor>& require, const c10::Device& dev,
                                                    int64_t B) {
  if (!require.has_value()) return {nullptr, 0};
  need_on(*require, dev, at::kInt, "require");
  TORCH_CHECK(require->dim() == 1 && (require->size(0) == 1 || require->size(0) == B),
              "require: expected shape [1] or [", B, "], got ", require->sizes());
  return {require->data_ptr<int32_t>(), require->numel()};
}

// The screen of finished structures (chm_screen_run): cell parameters, the shortest periodic distance, formula
// units and flags per crystal -> (floats [B,8] = a, b, c, alpha, beta, gamma, volume, dmin; ints [B,4] = i_min,
// j_min, formula_units, flags). target: the wanted reduced element counts, int32 [104] or [B,104], or None.
struct ScreenPlan {
  Handle<chm_screen, chm_screen_destroy> screen;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "screen", "crystal");
    check(chm_screen_create(nat.data(), (int)nat.size(), &screen.p), "chm_screen_create");
  }
};

std::tuple<at::Tensor, at::Tensor> screen(const at::Tensor& atom_types, const at::Tensor& frac,
                                          const at::Tensor& lattices, std::vector<int64_t> natoms,
                                          const c10::optional<at::Tensor>& target, double max_length,
                                          double min_distance) {
  TORCH_CHECK(!natoms.empty(), "screen: natoms is empty");
  const c10::Device dev = frac.device();
  const int64_t B = need_crystals(dev, natoms, &atom_types, frac, lattices).B;
  const int32_t* tg = nullptr;
  int64_t n_tg = 0;
  if (target.has_value()) {
    need_on(*target, dev, at::kInt, "target");
    TORCH_CHECK((target->dim() == 1 && target->size(0) == 104) ||
                    (target->dim() == 2 && target->size(0) == B && target->size(1) == 104),
                "target: expected shape [104] or [", B, ", 104], got ", target->sizes());
    tg = target->data_ptr<int32_t>();
    n_tg = target->numel();
  }
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<ScreenPlan>({natoms}, dev.index());
  at::Tensor rec = at::empty({B, 64}, at::TensorOptions().dtype(at::kByte).device(dev));
  check(chm_screen_run(plan->screen.p, atom_types.data_ptr<int64_t>(), atom_types.numel(), frac.data_ptr<float>(),
                       frac.numel(), lattices.data_ptr<float>(), lattices.numel(), tg, n_tg, (float)max_length,
                       (float)min_distance, rec.data_ptr(), (size_t)rec.numel(), stream()),
        "chm_screen_run");
  return {rec.view(at::kFloat).slice(1, 0, 8).contiguous(), rec.view(at::kInt).slice(1, 8, 12).contiguous()};
}

// Grouping of duplicate structures (chm_dedup_fingerprint + chm_dedup_group): the state's fingerprints
// ([B, 2 * bins], include/chemeleon_hip.h) and their groups by the leader rule -> (group [B] int32: the
// representative's index or -1, count [B] int32: the group's size at a representative, fingerprint).
struct DedupPlan {
  Handle<chm_dedup, chm_dedup_destroy> dedup;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "dedup", "crystal");
    check(chm_dedup_create(nat.data(), (int)nat.size(), &dedup.p), "chm_dedup_create");
  }
};

std::tuple<at::Tensor, at::Tensor, at::Tensor> dedup(const at::Tensor& atom_types, const at::Tensor& frac,
                                                     const at::Tensor& lattices, std::vector<int64_t> natoms,
                                                     const c10::optional<at::Tensor>& exclude, double tol,
                                                     double r_cut, double sigma, int64_t bins) {
  TORCH_CHECK(!natoms.empty(), "dedup: natoms is empty");
  TORCH_CHECK(bins >= 8 && bins <= 256, "dedup: bins must be in [8, 256], got ", bins);
  const c10::Device dev = frac.device();
  const int64_t B = need_crystals(dev, natoms, &atom_types, frac, lattices).B;
  const uint8_t* ex = optional_exclude(exclude, dev, B);
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<DedupPlan>({natoms}, dev.index());
  const auto ints = at::TensorOptions().dtype(at::kInt).device(dev);
  at::Tensor fp = at::empty({B, 2 * bins}, frac.options()), counts = at::empty({B, 104}, ints),
             flags = at::empty({B}, ints), group = at::empty({B}, ints), count = at::empty({B}, ints);
  const size_t ws_bytes = chm_dedup_workspace_bytes(B);
  at::Tensor ws = at::empty({(int64_t)ws_bytes}, at::TensorOptions().dtype(at::kByte).device(dev));
  check(chm_dedup_fingerprint(plan->dedup.p, atom_types.data_ptr<int64_t>(), atom_types.numel(),
                              frac.data_ptr<float>(), frac.numel(), lattices.data_ptr<float>(), lattices.numel(),
                              (int)bins, (float)r_cut, (float)sigma, fp.data_ptr<float>(), fp.numel(),
                              counts.data_ptr<int32_t>(), counts.numel(), flags.data_ptr<int32_t>(), flags.numel(),
                              stream()),
        "chm_dedup_fingerprint");
  check(chm_dedup_group(B, (int)bins, fp.data_ptr<float>(), fp.numel(), counts.data_ptr<int32_t>(), counts.numel(),
                        flags.data_ptr<int32_t>(), flags.numel(), ex, ex ? B : 0, (float)tol,
                        group.data_ptr<int32_t>(), group.numel(), count.data_ptr<int32_t>(), count.numel(),
                        ws.data_ptr(), ws_bytes, stream()),
        "chm_dedup_group");
  return {group, count, fp};
}

// Lattice system and reduced cell (chm_cell_run + chm_cell_apply): the state's cell records and the state in the
// reduced cells -> (floats [B,8] = a, b, c, alpha, beta, gamma, volume, 0 of the reduced cell; ints [B,18] = T
// (9, row-major), n_ops, n2, n3, n4, n6, system, halvings, flags, passes; frac [N,3] in the reduced basis;
// lattices [B,3,3] reduced).
struct CellPlan {
  CellHandle cells;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "cell", "crystal");
    check(chm_cell_create(nat.data(), (int)nat.size(), &cells.p), "chm_cell_create");
  }
};

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> cell(const at::Tensor& frac, const at::Tensor& lattices,
                                                                std::vector<int64_t> natoms,
                                                                const c10::optional<at::Tensor>& require,
                                                                double symprec, double angle_tolerance) {
  TORCH_CHECK(!natoms.empty(), "cell: natoms is empty");
  const c10::Device dev = frac.device();
  const int64_t B = need_crystals(dev, natoms, nullptr, frac, lattices).B;
  const auto rq = optional_require(require, dev, B);
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<CellPlan>({natoms}, dev.index());
  at::Tensor rec = at::empty({B, 128}, at::TensorOptions().dtype(at::kByte).device(dev));
  at::Tensor x_out = at::empty_like(frac), lat_out = at::empty_like(lattices);
  check(chm_cell_run(plan->cells.p, lattices.data_ptr<float>(), lattices.numel(), rq.first, rq.second, (float)symprec,
                     (float)angle_tolerance, rec.data_ptr(), (size_t)rec.numel(), stream()),
        "chm_cell_run");
  check(chm_cell_apply(plan->cells.p, rec.data_ptr(), (size_t)rec.numel(), frac.data_ptr<float>(), frac.numel(),
                       lattices.data_ptr<float>(), lattices.numel(), x_out.data_ptr<float>(), x_out.numel(),
                       lat_out.data_ptr<float>(), lat_out.numel(), stream()),
        "chm_cell_apply");
  return {rec.view(at::kFloat).slice(1, 0, 8).contiguous(), rec.view(at::kInt).slice(1, 8, 26).contiguous(), x_out,
          lat_out};
}

// Crystal system with the atoms (chm_cell_run + chm_symm_run on one stream): (records uint8 [B,64] = the
// chm_symm_record of every crystal; operations uint8 [B,48,16] = the slots of (int32 candidate index, float t[3]),
// or [0,48,16] unless `operations`).
struct SymmPlan {
  CellHandle cells;
  Handle<chm_symm, chm_symm_destroy> symm;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "symmetry", "crystal");
    check(chm_symm_create(nat.data(), (int)nat.size(), &symm.p), "chm_symm_create");
    check(chm_cell_create(nat.data(), (int)nat.size(), &cells.p), "chm_cell_create");
  }
};

std::tuple<at::Tensor, at::Tensor> symmetry(const at::Tensor& atom_types, const at::Tensor& frac,
                                            const at::Tensor& lattices, std::vector<int64_t> natoms,
                                            const c10::optional<at::Tensor>& require, double symprec,
                                            double angle_tolerance, bool operations) {
  TORCH_CHECK(!natoms.empty(), "symmetry: natoms is empty");
  const c10::Device dev = frac.device();
  const int64_t B = need_crystals(dev, natoms, &atom_types, frac, lattices).B;
  const auto rq = optional_require(require, dev, B);
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<SymmPlan>({natoms}, dev.index());
  const auto bytes = at::TensorOptions().dtype(at::kByte).device(dev);
  at::Tensor cells = at::empty({B, 128}, bytes), rec = at::empty({B, 64}, bytes);
  at::Tensor ops = at::empty({operations ? B : 0, 48, 16}, bytes);
  check(chm_cell_run(plan->cells.p, lattices.data_ptr<float>(), lattices.numel(), nullptr, 0, (float)symprec,
                     (float)angle_tolerance, cells.data_ptr(), (size_t)cells.numel(), stream()),
        "chm_cell_run");
  check(chm_symm_run(plan->symm.p, cells.data_ptr(), (size_t)cells.numel(), atom_types.data_ptr<int64_t>(),
                     atom_types.numel(), frac.data_ptr<float>(), frac.numel(), lattices.data_ptr<float>(),
                     lattices.numel(), rq.first, rq.second, (float)symprec, (float)angle_tolerance, rec.data_ptr(),
                     (size_t)rec.numel(), operations ? ops.data_ptr() : nullptr, (size_t)ops.numel(), stream()),
        "chm_symm_run");
  return {rec, ops};
}

// Primitive cells (chm_cell_run + chm_prim_run on one stream): (atom_types int64 [N] and frac [N,3], the packed
// primitive cells in their first new_offsets[B] rows and zero after them; lattices [B,3,3]; new_offsets int32
// [B+1]; records uint8 [B,64] = the chm_prim_record of every crystal). Nothing crosses to the host here: the caller
// reads N' from new_offsets.
struct PrimPlan {
  CellHandle cells;
  Handle<chm_prim, chm_prim_destroy> prim;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "primitive", "crystal");
    check(chm_prim_create(nat.data(), (int)nat.size(), &prim.p), "chm_prim_create");
    check(chm_cell_create(nat.data(), (int)nat.size(), &cells.p), "chm_cell_create");
  }
};

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> primitive(
    const at::Tensor& atom_types, const at::Tensor& frac, const at::Tensor& lattices, std::vector<int64_t> natoms,
    double symprec, double angle_tolerance) {
  TORCH_CHECK(!natoms.empty(), "primitive: natoms is empty");
  const c10::Device dev = frac.device();
  const Crystals c = need_crystals(dev, natoms, &atom_types, frac, lattices);
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<PrimPlan>({natoms}, dev.index());
  const auto bytes = at::TensorOptions().dtype(at::kByte).device(dev);
  const auto ints = at::TensorOptions().dtype(at::kInt).device(dev);
  at::Tensor cells = at::empty({c.B, 128}, bytes), rec = at::empty({c.B, 64}, bytes);
  at::Tensor source = at::empty({c.N}, ints), new_off = at::empty({c.B + 1}, ints);
  at::Tensor a_out = at::empty_like(atom_types), x_out = at::empty_like(frac), lat_out = at::empty_like(lattices);
  check(chm_cell_run(plan->cells.p, lattices.data_ptr<float>(), lattices.numel(), nullptr, 0, (float)symprec,
                     (float)angle_tolerance, cells.data_ptr(), (size_t)cells.numel(), stream()),
        "chm_cell_run");
  check(chm_prim_run(plan->prim.p, cells.data_ptr(), (size_t)cells.numel(), atom_types.data_ptr<int64_t>(),
                     atom_types.numel(), frac.data_ptr<float>(), frac.numel(), lattices.data_ptr<float>(),
                     lattices.numel(), (float)symprec, (float)angle_tolerance, rec.data_ptr(), (size_t)rec.numel(),
                     source.data_ptr<int32_t>(), source.numel(), new_off.data_ptr<int32_t>(), new_off.numel(),
                     a_out.data_ptr<int64_t>(), a_out.numel(), x_out.data_ptr<float>(), x_out.numel(),
                     lat_out.data_ptr<float>(), lat_out.numel(), stream()),
        "chm_prim_run");
  return {a_out, x_out, lat_out, new_off, rec};
}

// Matching against references (chm_cell_run on both lists + chm_match_run on one stream): (records uint8 [B,64] =
// the chm_match_record of every crystal; perm int32 [N], or [0] unless `perm`). ref_of: one reference index per
// crystal, -1 for none. The plan's key is (natoms, ref_natoms, ref_of).
struct MatchPlan {
  CellHandle cells, ref_cells;
  Handle<chm_match, chm_match_destroy> match;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "match", "crystal"), rnat = to_int32(key[1], "match", "reference");
    std::vector<int32_t> of;
    for (int64_t r : key[2]) {
      TORCH_CHECK(r >= -1 && r < (int64_t)rnat.size(), "match: ref_of entry ", r, " outside [-1, ", rnat.size(), ")");
      of.push_back((int32_t)r);
    }
    int rc = chm_match_create(nat.data(), (int)nat.size(), rnat.data(), (int)rnat.size(), of.data(), &match.p);
    if (rc == CHM_OK) rc = chm_cell_create(nat.data(), (int)nat.size(), &cells.p);
    if (rc == CHM_OK) rc = chm_cell_create(rnat.data(), (int)rnat.size(), &ref_cells.p);
    check(rc, "chm_match_create");
  }
};

std::tuple<at::Tensor, at::Tensor> match(const at::Tensor& atom_types, const at::Tensor& frac,
                                         const at::Tensor& lattices, std::vector<int64_t> natoms,
                                         const at::Tensor& ref_atom_types, const at::Tensor& ref_frac,
                                         const at::Tensor& ref_lattices, std::vector<int64_t> ref_natoms,
                                         std::vector<int64_t> ref_of, double ltol, double stol, double angle_tol,
                                         bool perm) {
  TORCH_CHECK(!natoms.empty(), "match: natoms is empty");
  TORCH_CHECK(!ref_natoms.empty(), "match: ref_natoms is empty");
  const c10::Device dev = frac.device();
  need_crystals_on(dev, &atom_types, frac, lattices);
  need_crystals_on(dev, &ref_atom_types, ref_frac, ref_lattices, "ref_");
  TORCH_CHECK(ref_of.size() == natoms.size(), "ref_of: expected ", natoms.size(), " entries, got ", ref_of.size());
  const Crystals c = need_crystals_shape(natoms, &atom_types, frac, lattices);
  const int64_t R = need_crystals_shape(ref_natoms, &ref_atom_types, ref_frac, ref_lattices, "ref_").B;
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<MatchPlan>({natoms, ref_natoms, ref_of}, dev.index());
  const auto bytes = at::TensorOptions().dtype(at::kByte).device(dev);
  at::Tensor cells = at::empty({c.B, 128}, bytes), ref_cells = at::empty({R, 128}, bytes),
             rec = at::empty({c.B, 64}, bytes);
  at::Tensor pm = at::empty({perm ? c.N : 0}, at::TensorOptions().dtype(at::kInt).device(dev));
  check(chm_cell_run(plan->cells.p, lattices.data_ptr<float>(), lattices.numel(), nullptr, 0, kMatchCellSymprec,
                     kMatchCellAngleTolerance, cells.data_ptr(), (size_t)cells.numel(), stream()),
        "chm_cell_run");
  check(chm_cell_run(plan->ref_cells.p, ref_lattices.data_ptr<float>(), ref_lattices.numel(), nullptr, 0,
                     kMatchCellSymprec, kMatchCellAngleTolerance, ref_cells.data_ptr(), (size_t)ref_cells.numel(),
                     stream()),
        "chm_cell_run");
  check(chm_match_run(plan->match.p, cells.data_ptr(), (size_t)cells.numel(), atom_types.data_ptr<int64_t>(),
                      atom_types.numel(), frac.data_ptr<float>(), frac.numel(), lattices.data_ptr<float>(),
                      lattices.numel(), ref_cells.data_ptr(), (size_t)ref_cells.numel(),
                      ref_atom_types.data_ptr<int64_t>(), ref_atom_types.numel(), ref_frac.data_ptr<float>(),
                      ref_frac.numel(), ref_lattices.data_ptr<float>(), ref_lattices.numel(), (float)ltol, (float)stol,
                      (float)angle_tol, rec.data_ptr(), (size_t)rec.numel(), perm ? pm.data_ptr<int32_t>() : nullptr,
                      pm.numel(), stream()),
        "chm_match_run");
  return {rec, pm};
}

// Grouping by pairwise matching (chm_cell_run + chm_match_group_run on one stream): (group [B] int32: the
// representative's index or -1, count [B] int32: the group's size at a representative, records uint8 [B,32] = the
// chm_match_group_record of every crystal, pair records uint8 [P,16] in the plan's pair order).
struct MatchGroupPlan {
  CellHandle cells;
  Handle<chm_match_group, chm_match_group_destroy> group;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "match_group", "crystal");
    int rc = chm_match_group_create(nat.data(), (int)nat.size(), &group.p);
    if (rc == CHM_OK) rc = chm_cell_create(nat.data(), (int)nat.size(), &cells.p);
    check(rc, "chm_match_group_create");
  }
};

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> match_group(const at::Tensor& atom_types, const at::Tensor& frac,
                                                                       const at::Tensor& lattices,
                                                                       std::vector<int64_t> natoms,
                                                                       const c10::optional<at::Tensor>& exclude,
                                                                       double ltol, double stol, double angle_tol) {
  TORCH_CHECK(!natoms.empty(), "match_group: natoms is empty");
  const c10::Device dev = frac.device();
  const int64_t B = need_crystals(dev, natoms, &atom_types, frac, lattices).B;
  const uint8_t* ex = optional_exclude(exclude, dev, B);
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<MatchGroupPlan>({natoms}, dev.index());
  const int64_t P = chm_match_group_num_pairs(plan->group.p);
  const size_t ws_bytes = chm_match_group_workspace_bytes(plan->group.p);
  const auto bytes = at::TensorOptions().dtype(at::kByte).device(dev);
  const auto ints = at::TensorOptions().dtype(at::kInt).device(dev);
  at::Tensor cells = at::empty({B, 128}, bytes), rec = at::empty({B, 32}, bytes), pairs = at::empty({P, 16}, bytes),
             ws = at::empty({(int64_t)ws_bytes}, bytes), group = at::empty({B}, ints), count = at::empty({B}, ints);
  check(chm_cell_run(plan->cells.p, lattices.data_ptr<float>(), lattices.numel(), nullptr, 0, kMatchCellSymprec,
                     kMatchCellAngleTolerance, cells.data_ptr(), (size_t)cells.numel(), stream()),
        "chm_cell_run");
  check(chm_match_group_run(plan->group.p, cells.data_ptr(), (size_t)cells.numel(), atom_types.data_ptr<int64_t>(),
                            atom_types.numel(), frac.data_ptr<float>(), frac.numel(), lattices.data_ptr<float>(),
                            lattices.numel(), ex, ex ? B : 0, (float)ltol, (float)stol, (float)angle_tol,
                            group.data_ptr<int32_t>(), group.numel(), count.data_ptr<int32_t>(), count.numel(),
                            rec.data_ptr(), (size_t)rec.numel(), P ? pairs.data_ptr() : nullptr, (size_t)pairs.numel(),
                            ws.data_ptr(), ws_bytes, stream()),
        "chm_match_group_run");
  return {group, count, rec, pairs};
}

// Searching a reference set (chm_cell_run on both lists + chm_match_set_run on one stream): (records uint8 [B,48] =
// the chm_match_set_record of every crystal, pair records uint8 [num_pairs_max,16]: the first sum(n_candidates) are
// this run's, the rest is 0). The references come sorted by (atom count, key, index) with their keys (int64 holding
// the 64 bits) and original indices; the plan's key is (natoms, ref_natoms, ref_keys, ref_index).
struct MatchSetPlan {
  CellHandle cells, ref_cells;
  Handle<chm_match_set, chm_match_set_destroy> set;
  void create(const Lists& key) {
    const auto nat = to_int32(key[0], "match_set", "crystal"), rnat = to_int32(key[1], "match_set", "reference");
    std::vector<uint64_t> keys(key[2].begin(), key[2].end());
    std::vector<int32_t> index(key[3].begin(), key[3].end());
    int rc = chm_match_set_create(nat.data(), (int)nat.size(), rnat.data(), keys.data(), index.data(), (int)rnat.size(),
                                  &set.p);
    if (rc == CHM_OK) rc = chm_cell_create(nat.data(), (int)nat.size(), &cells.p);
    if (rc == CHM_OK) rc = chm_cell_create(rnat.data(), (int)rnat.size(), &ref_cells.p);
    check(rc, "chm_match_set_create");
  }
};

std::tuple<at::Tensor, at::Tensor> match_set(const at::Tensor& atom_types, const at::Tensor& frac,
                                             const at::Tensor& lattices, std::vector<int64_t> natoms,
                                             const at::Tensor& ref_atom_types, const at::Tensor& ref_frac,
                                             const at::Tensor& ref_lattices, std::vector<int64_t> ref_natoms,
                                             std::vector<int64_t> ref_keys, std::vector<int64_t> ref_index,
                                             const c10::optional<at::Tensor>& exclude, double ltol, double stol,
                                             double angle_tol) {
  TORCH_CHECK(!natoms.empty(), "match_set: natoms is empty");
  TORCH_CHECK(!ref_natoms.empty(), "match_set: ref_natoms is empty");
  TORCH_CHECK(ref_keys.size() == ref_natoms.size(), "ref_keys: expected ", ref_natoms.size(), " entries, got ", ref_keys.size());
  TORCH_CHECK(ref_index.size() == ref_natoms.size(), "ref_index: expected ", ref_natoms.size(), " entries, got ",
              ref_index.size());
  const c10::Device dev = frac.device();
  need_crystals_on(dev, &atom_types, frac, lattices);
  need_crystals_on(dev, &ref_atom_types, ref_frac, ref_lattices, "ref_");
  const Crystals c = need_crystals_shape(natoms, &atom_types, frac, lattices);
  const int64_t R = need_crystals_shape(ref_natoms, &ref_atom_types, ref_frac, ref_lattices, "ref_").B;
  const uint8_t* ex = optional_exclude(exclude, dev, c.B);
  HIPGuardMasqueradingAsCUDA guard(dev);
  const auto plan = cached_plan<MatchSetPlan>({natoms, ref_natoms, ref_keys, ref_index}, dev.index());
  const int64_t P = chm_match_set_num_pairs_max(plan->set.p);
  const size_t ws_bytes = chm_match_set_workspace_bytes(plan->set.p);
  const auto bytes = at::TensorOptions().dtype(at::kByte).device(dev);
  at::Tensor cells = at::empty({c.B, 128}, bytes), ref_cells = at::empty({R, 128}, bytes), rec = at::empty({c.B, 48}, bytes),
             pairs = at::zeros({P, 16}, bytes), ws = at::empty({(int64_t)ws_bytes}, bytes);
  check(chm_cell_run(plan->cells.p, lattices.data_ptr<float>(), lattices.numel(), nullptr, 0, kMatchCellSymprec,
                     kMatchCellAngleTolerance, cells.data_ptr(), (size_t)cells.numel(), stream()),
        "chm_cell_run");
  check(chm_cell_run(plan->ref_cells.p, ref_lattices.data_ptr<float>(), ref_lattices.numel(), nullptr, 0,
                     kMatchCellSymprec, kMatchCellAngleTolerance, ref_cells.data_ptr(), (size_t)ref_cells.numel(),
                     stream()),
        "chm_cell_run");
  check(chm_match_set_run(plan->set.p, cells.data_ptr(), (size_t)cells.numel(), atom_types.data_ptr<int64_t>(),
                          atom_types.numel(), frac.data_ptr<float>(), frac.numel(), lattices.data_ptr<float>(),
                          lattices.numel(), ref_cells.data_ptr(), (size_t)ref_cells.numel(),
                          ref_atom_types.data_ptr<int64_t>(), ref_atom_types.numel(), ref_frac.data_ptr<float>(),
                          ref_frac.numel(), ref_lattices.data_ptr<float>(), ref_lattices.numel(), ex, ex ? c.B : 0,
                          (float)ltol, (float)stol, (float)angle_tol, rec.data_ptr(), (size_t)rec.numel(),
                          P ? pairs.data_ptr() : nullptr, (size_t)pairs.numel(), ws.data_ptr(), ws_bytes, stream()),
        "chm_match_set_run");
  return {rec, pairs};
}

}  // namespace

TORCH_LIBRARY(chemeleon, m) {
  m.class_<Model>("Model")
      .def(torch::init<std::vector<at::Tensor>, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>())
      .def("set_math", &Model::set_math)
      .def("get_math", &Model::get_math)
      .def("set_option", &Model::set_option);
  m.class_<Batch>("Batch")
      .def(torch::init<c10::intrusive_ptr<Model>, std::vector<int64_t>, int64_t, bool, int64_t>())
      .def("num_nodes", &Batch::num_nodes)
      .def("num_edges", &Batch::num_edges)
      .def("num_graphs", &Batch::num_graphs);
  m.class_<Schedule>("Schedule")
      .def(torch::init<at::Tensor, at::Tensor, at::Tensor, at::Tensor>())
      .def("num_timesteps", &Schedule::num_timesteps);
  m.def("decoder_forward(__torch__.torch.classes.chemeleon.Batch batch, int pairs, Tensor atom_types, Tensor frac, "
        "Tensor lattices, Tensor? time_emb, Tensor? text) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("sample_step(__torch__.torch.classes.chemeleon.Batch batch, __torch__.torch.classes.chemeleon.Schedule "
        "schedule, int t, float cond_scale, Tensor(a!) atom_types, Tensor(b!) frac, Tensor(c!) lattices, Tensor? cond, "
        "Tensor? null, Tensor? rand_a, Tensor? rand_l, Tensor? rand_x1, Tensor? rand_x2, int seed, int node_base, "
        "int graph_base) -> ()");
  m.def("segment_mean(__torch__.torch.classes.chemeleon.Batch batch, int pairs, Tensor msg) -> Tensor");
  m.def("d3pm_sample(Tensor logits, Tensor x_t, Tensor t, Tensor noise, Tensor q_one_step, Tensor q_mats) -> Tensor");
  m.def("screen(Tensor atom_types, Tensor frac, Tensor lattices, int[] natoms, Tensor? target, float max_length, "
        "float min_distance) -> (Tensor, Tensor)");
  m.def("dedup(Tensor atom_types, Tensor frac, Tensor lattices, int[] natoms, Tensor? exclude, float tol, "
        "float r_cut, float sigma, int bins) -> (Tensor, Tensor, Tensor)");
  m.def("cell(Tensor frac, Tensor lattices, int[] natoms, Tensor? require, float symprec, float angle_tolerance) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("symmetry(Tensor atom_types, Tensor frac, Tensor lattices, int[] natoms, Tensor? require, float symprec, "
        "float angle_tolerance, bool operations) -> (Tensor, Tensor)");
  m.def("primitive(Tensor atom_types, Tensor frac, Tensor lattices, int[] natoms, float symprec, "
        "float angle_tolerance) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("match(Tensor atom_types, Tensor frac, Tensor lattices, int[] natoms, Tensor ref_atom_types, Tensor ref_frac, "
        "Tensor ref_lattices, int[] ref_natoms, int[] ref_of, float ltol, float stol, float angle_tol, bool perm) -> "
        "(Tensor, Tensor)");
  m.def("match_group(Tensor atom_types, Tensor frac, Tensor lattices, int[] natoms, Tensor? exclude, float ltol, "
        "float stol, float angle_tol) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("match_set(Tensor atom_types, Tensor frac, Tensor lattices, int[] natoms, Tensor ref_atom_types, Tensor ref_frac, "
        "Tensor ref_lattices, int[] ref_natoms, int[] ref_keys, int[] ref_index, Tensor? exclude, float ltol, float stol, "
        "float angle_tol) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(chemeleon, CUDA, m) {
  m.impl("decoder_forward", decoder_forward);
  m.impl("sample_step", sample_step);
  m.impl("segment_mean", segment_mean);
  m.impl("d3pm_sample", d3pm_sample);
  m.impl("screen", screen);
  m.impl("dedup", dedup);
  m.impl("cell", cell);
  m.impl("symmetry", symmetry);
  m.impl("primitive", primitive);
  m.impl("match", match);
  m.impl("match_group", match_group);
  m.impl("match_set", match_set);
}
