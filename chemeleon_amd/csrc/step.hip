// The reverse step of the sampler (decoder call, predictor, decoder call, corrector), constrained sampling and the
// training loss: the entry points around run_decoder and the update kernels of kernels.hip / constrain.hip.
#include <cstring>

#include "chm_host.h"

using namespace chm;

// the element counts of a step's buffers against the batch (N nodes, B crystals) and its model
int chm::check_step_io(const chm_batch* b, const chm_step_io* io, bool noise_required, bool noise_allowed,
                       bool text_required) {
  if (!io) return fail(CHM_E_ARG, "io is NULL");
  const long N = b->N, B = b->B, A = b->m->d.max_atoms, X = b->m->d.text_dim;
  auto want = [&](const void* p, int64_t n, long expect, const char* name) -> int {
    if (!p) return fail(CHM_E_ARG, std::string(name) + " is NULL");
    if (n != expect)
      return fail(CHM_E_ARG, std::string(name) + ": " + std::to_string(n) + " elements, the batch needs " +
                                 std::to_string(expect));
    return CHM_OK;
  };
  int rc;
  if ((rc = want(io->d_atom_types, io->n_atom_types, N, "atom_types [N]"))) return rc;
  if ((rc = want(io->d_frac, io->n_frac, 3 * N, "frac [N,3]"))) return rc;
  if ((rc = want(io->d_lattices, io->n_lattices, 9 * B, "lattices [B,3,3]"))) return rc;
  if (X > 0 && text_required) {
    if ((rc = want(io->d_cond, io->n_cond, B * X, "cond [B,text_dim]"))) return rc;
    if ((rc = want(io->d_null, io->n_null, B * X, "null [B,text_dim]"))) return rc;
  }
  const int given = (io->d_rand_a != nullptr) + (io->d_rand_l != nullptr) + (io->d_rand_x1 != nullptr) +
                    (io->d_rand_x2 != nullptr);
  if (given != 0 && given != 4) return fail(CHM_E_ARG, "noise: all four buffers or none");
  if (given && !noise_allowed) return fail(CHM_E_ARG, "this entry point draws device noise: the noise buffers must be NULL");
  if (!given && noise_required) return fail(CHM_E_ARG, "all four noise buffers are required");
  if (given) {
    if ((rc = want(io->d_rand_a, io->n_rand_a, N * A, "rand_a [N,A]"))) return rc;
    if ((rc = want(io->d_rand_l, io->n_rand_l, 9 * B, "rand_l [B,3,3]"))) return rc;
    if ((rc = want(io->d_rand_x1, io->n_rand_x1, 3 * N, "rand_x1 [N,3]"))) return rc;
    if ((rc = want(io->d_rand_x2, io->n_rand_x2, 3 * N, "rand_x2 [N,3]"))) return rc;
  }
  return CHM_OK;
}

// the buffers of a constraint against the batch (N nodes, B crystals, A classes) and the schedule's T
static int check_constraint(const chm_batch* b, const chm_schedule* sc, const chm_constraint* con) {
  if (!con) return fail(CHM_E_ARG, "constraint is NULL");
  const long N = b->N, B = b->B, A = b->m->d.max_atoms;
  auto sized = [&](const void* p, int64_t n, long expect, const char* name) -> int {
    if (p && n != expect)
      return fail(CHM_E_ARG, std::string("constraint ") + name + ": " + std::to_string(n) +
                                 " elements, the batch needs " + std::to_string(expect));
    return CHM_OK;
  };
  auto pair = [&](const void* v, const void* m, const char* name) -> int {
    if ((v != nullptr) != (m != nullptr))
      return fail(CHM_E_ARG, std::string("constraint ") + name + ": known values and mask are given together or not at all");
    return CHM_OK;
  };
  int rc;
  if ((rc = pair(con->d_a0, con->d_type_mask, "a0 / type_mask"))) return rc;
  if ((rc = pair(con->d_x0, con->d_frac_mask, "x0 / frac_mask"))) return rc;
  if ((rc = pair(con->d_l0, con->d_lattice_mask, "l0 / lattice_mask"))) return rc;
  if ((rc = sized(con->d_a0, con->n_a0, N, "a0 [N]"))) return rc;
  if ((rc = sized(con->d_type_mask, con->n_type_mask, N, "type_mask [N]"))) return rc;
  if ((rc = sized(con->d_x0, con->n_x0, 3 * N, "x0 [N,3]"))) return rc;
  if ((rc = sized(con->d_frac_mask, con->n_frac_mask, N, "frac_mask [N]"))) return rc;
  if ((rc = sized(con->d_l0, con->n_l0, 9 * B, "l0 [B,3,3]"))) return rc;
  if ((rc = sized(con->d_lattice_mask, con->n_lattice_mask, B, "lattice_mask [B]"))) return rc;
  if (!con->d_fwd) return fail(CHM_E_ARG, "constraint fwd is NULL");
  if (con->n_fwd != 4L * (sc->T + 1))
    return fail(CHM_E_ARG, "constraint fwd [T+1,4]: " + std::to_string(con->n_fwd) + " elements, the schedule's T = " +
                               std::to_string(sc->T) + " needs " + std::to_string(4L * (sc->T + 1)));
  const int given = (con->d_rand_a != nullptr) + (con->d_rand_l != nullptr) + (con->d_rand_x != nullptr);
  if (given != 0 && given != 3) return fail(CHM_E_ARG, "constraint noise: all three buffers or none");
  if ((rc = sized(con->d_rand_a, con->n_rand_a, N * A, "rand_a [N,A]"))) return rc;
  if ((rc = sized(con->d_rand_l, con->n_rand_l, 9 * B, "rand_l [B,3,3]"))) return rc;
  if ((rc = sized(con->d_rand_x, con->n_rand_x, 3 * N, "rand_x [N,3]"))) return rc;
  return CHM_OK;
}

static ConstrainArgs constrain_args(const chm_batch* b, const chm_schedule* sc, const chm_constraint* con, int level,
                                    const int* d_t, const chm_step_io* io, uint64_t seed, int64_t node_base,
                                    int64_t graph_base) {
  ConstrainArgs c;
  std::memset(&c, 0, sizeof(c));
  c.N = b->N; c.B = b->B; c.A = b->m->d.max_atoms; c.T = sc->T; c.level = level; c.d_t = d_t;
  c.a0 = con->d_a0; c.type_mask = con->d_type_mask; c.x0 = con->d_x0; c.frac_mask = con->d_frac_mask;
  c.l0 = con->d_l0; c.lattice_mask = con->d_lattice_mask; c.fwd = con->d_fwd; c.q_mats = sc->d_q_mats;
  c.a = io->d_atom_types; c.x = io->d_frac; c.l = io->d_lattices;
  c.ra = con->d_rand_a; c.rl = con->d_rand_l; c.rx = con->d_rand_x;
  c.seed = seed; c.node_base = node_base; c.graph_base = graph_base;
  return c;
}

// The update kernels' arguments of one step on the batch's decoder outputs (HO, LAT), for sample_step and
// chm_debug_step_update alike. The guidance weights are formed from the ABI's float cond_scale: the null weight
// is 1 - (double)cond_scale rounded once, which is the reference's fp32(1 - cond_scale) of the Python double only
// where cond_scale is itself a float (2.0, 1.0, 0.0; not 1.3: DESIGN.md "The reverse step's update kernels").
StepArgs chm::step_args(const chm_batch* b, const chm_schedule* sc, int t, const int* d_t, float cond_scale,
                        const chm_step_io* io, uint64_t seed, int64_t node_base, int64_t graph_base) {
  StepArgs sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.t = t; sa.d_t = d_t; sa.T = sc->T; sa.A = b->m->d.max_atoms; sa.N = b->N; sa.B = b->B;
  sa.cs_null = (float)(1.0 - (double)cond_scale); sa.cs_cond = cond_scale;
  sa.coef = sc->d_coef; sa.q_one_step = sc->d_q_one_step; sa.q_mats = sc->d_q_mats;
  sa.HO = b->HO; sa.LAT = b->LAT; sa.a = io->d_atom_types; sa.x = io->d_frac; sa.l = io->d_lattices; sa.n2g = b->n2g;
  if (io->d_rand_a) { sa.ra = io->d_rand_a; sa.rl = io->d_rand_l; sa.rx1 = io->d_rand_x1; sa.rx2 = io->d_rand_x2; }
  sa.seed = seed; sa.node_base = node_base; sa.graph_base = graph_base;
  return sa;
}

// con != null (chm_sample_step_con): the known entries are replaced at level t - 1 between the predictor and the
// corrector's decoder call (stage 1) and the known coordinates again behind the corrector (stage 2, same noise)
static int sample_step(chm_batch* b, const chm_schedule* sc, int t, int* d_t, float cond_scale, const chm_step_io* io,
                       bool noise_required, bool noise_allowed, uint64_t seed, int64_t node_base, int64_t graph_base,
                       hipStream_t s, const chm_constraint* con = nullptr) {
  if (!b || !sc) return fail(CHM_E_ARG, "batch / schedule is NULL");
  if (b->P < 2) return fail(CHM_E_ARG, "sampling needs a batch created with max_pairs = 2");
  if (!b->m->film) return fail(CHM_E_ARG, "sampling needs a time-conditioned decoder (time_dim > 0)");
  if (sc->T < 1) return fail(CHM_E_ARG, "schedule: T must be >= 1");
  if (!d_t && (t < 1 || t > sc->T)) return fail(CHM_E_ARG, "t out of range");
  if (!sc->d_coef || !sc->d_time_emb || !sc->d_q_one_step || !sc->d_q_mats)
    return fail(CHM_E_ARG, "NULL schedule table");
  if (sc->num_classes != b->m->d.max_atoms || sc->time_dim != b->m->d.time_dim)
    return fail(CHM_E_ARG, "schedule: num_classes " + std::to_string(sc->num_classes) + " / time_dim " +
                               std::to_string(sc->time_dim) + " do not match the model's " +
                               std::to_string(b->m->d.max_atoms) + " / " + std::to_string(b->m->d.time_dim));
  int rc = check_step_io(b, io, noise_required, noise_allowed);
  if (rc) return rc;
  if (con && (rc = check_constraint(b, sc, con))) return rc;
  int64_t* d_a = io->d_atom_types;
  float *d_x = io->d_frac, *d_l = io->d_lattices;
  const float *d_cond = b->m->d.text_dim > 0 ? io->d_cond : nullptr, *d_null = b->m->d.text_dim > 0 ? io->d_null : nullptr;
  // time-embedding row: host t -> pointer offset; device t -> offset inside the kernel
  const float* temb = d_t ? sc->d_time_emb : sc->d_time_emb + (size_t)t * TD;
  rc = run_decoder(b, 2, d_a, d_x, d_l, temb, 0, d_t, d_cond, d_null, 3, s);
  if (rc) return rc;
  const StepArgs sa = step_args(b, sc, t, d_t, cond_scale, io, seed, node_base, graph_base);
  HIPCHK(step_predictor(sa, s));
  ConstrainArgs ca;
  if (con) {  // stage 1: the corrector's decoder call sees the known entries at level t - 1
    ca = constrain_args(b, sc, con, t - 1, d_t, io, seed, node_base, graph_base);
    HIPCHK(constrain(ca, 7, s));
  }
  // corrector: same t and text as the predictor, so its FiLM conditioning is reused
  rc = run_decoder(b, 2, d_a, d_x, d_l, temb, 0, d_t, d_cond, d_null, 1, s, true);
  if (rc) return rc;
  HIPCHK(step_corrector(sa, s));
  if (con) HIPCHK(constrain(ca, 4, s));  // stage 2: the corrector's move on the known coordinates is discarded
  if (d_t) HIPCHK(decrement(d_t, s));
  return CHM_OK;
}

extern "C" int chm_sample_step(chm_batch* b, const chm_schedule* sc, int t, float cond_scale, const chm_step_io* io,
                               uint64_t seed, int64_t node_base, int64_t graph_base, void* stream) {
  return sample_step(b, sc, t, nullptr, cond_scale, io, false, true, seed, node_base, graph_base, (hipStream_t)stream);
}

extern "C" int chm_sample_step_dt(chm_batch* b, const chm_schedule* sc, int32_t* d_t, float cond_scale,
                                  const chm_step_io* io, uint64_t seed, int64_t node_base, int64_t graph_base,
                                  void* stream) {
  if (!d_t) return fail(CHM_E_ARG, "d_t is NULL");
  return sample_step(b, sc, 0, d_t, cond_scale, io, false, false, seed, node_base, graph_base, (hipStream_t)stream);
}

extern "C" int chm_sample_step_dt_noise(chm_batch* b, const chm_schedule* sc, int32_t* d_t, float cond_scale,
                                        const chm_step_io* io, void* stream) {
  if (!d_t) return fail(CHM_E_ARG, "d_t is NULL");
  return sample_step(b, sc, 0, d_t, cond_scale, io, true, true, 0, 0, 0, (hipStream_t)stream);
}

extern "C" int chm_sample_step_con(chm_batch* b, const chm_schedule* sc, int t, int32_t* d_t, float cond_scale,
                                   const chm_step_io* io, const chm_constraint* con, uint64_t seed, int64_t node_base,
                                   int64_t graph_base, void* stream) {
  if (!b || !sc) return fail(CHM_E_ARG, "batch / schedule is NULL");
  if (!con) return fail(CHM_E_ARG, "constraint is NULL (chm_sample_step is the unconstrained step)");
  return sample_step(b, sc, d_t ? 0 : t, d_t, cond_scale, io, false, true, seed, node_base, graph_base,
                     (hipStream_t)stream, con);
}

extern "C" int chm_constrain_state(chm_batch* b, const chm_schedule* sc, const chm_constraint* con, int level,
                                   const int32_t* d_t, int what, const chm_step_io* io, uint64_t seed,
                                   int64_t node_base, int64_t graph_base, void* stream) {
  if (!b || !sc) return fail(CHM_E_ARG, "batch / schedule is NULL");
  if (sc->T < 1) return fail(CHM_E_ARG, "schedule: T must be >= 1");
  if (!sc->d_q_mats) return fail(CHM_E_ARG, "NULL schedule table");
  if (sc->num_classes != b->m->d.max_atoms)
    return fail(CHM_E_ARG, "schedule: num_classes " + std::to_string(sc->num_classes) + " does not match the model's " +
                               std::to_string(b->m->d.max_atoms));
  if (!d_t && (level < 0 || level > sc->T))
    return fail(CHM_E_ARG, "level " + std::to_string(level) + " outside [0, " + std::to_string(sc->T) + "]");
  if (what < 1 || what > 7) return fail(CHM_E_ARG, "what " + std::to_string(what) + " outside [1, 7]");
  if (!io) return fail(CHM_E_ARG, "io is NULL");
  const long N = b->N, B = b->B;
  auto want = [&](const void* p, int64_t n, long expect, const char* name) -> int {
    if (!p) return fail(CHM_E_ARG, std::string(name) + " is NULL");
    if (n != expect)
      return fail(CHM_E_ARG, std::string(name) + ": " + std::to_string(n) + " elements, the batch needs " +
                                 std::to_string(expect));
    return CHM_OK;
  };
  int rc;
  if ((rc = want(io->d_atom_types, io->n_atom_types, N, "atom_types [N]"))) return rc;
  if ((rc = want(io->d_frac, io->n_frac, 3 * N, "frac [N,3]"))) return rc;
  if ((rc = want(io->d_lattices, io->n_lattices, 9 * B, "lattices [B,3,3]"))) return rc;
  if ((rc = check_constraint(b, sc, con))) return rc;
  const ConstrainArgs ca = constrain_args(b, sc, con, level, d_t, io, seed, node_base, graph_base);
  HIPCHK(constrain(ca, what, (hipStream_t)stream));
  return CHM_OK;
}

extern "C" int chm_d3pm_sample(int N, int A, int T, const float* logits, const int64_t* xt, const int64_t* tn,
                               const float* noise, const float* q1, const float* qm, int64_t* out, void* stream) {
  if (N < 0 || A < 1 || A > 128 || T < 1) return fail(CHM_E_ARG, "bad sizes");
  if (N == 0) return CHM_OK;
  if (!logits || !xt || !tn || !noise || !q1 || !qm || !out) return fail(CHM_E_ARG, "NULL argument");
  hipStream_t s = (hipStream_t)stream;
  // the device range check: the first node with t outside [1, T] or x_t outside [0, A) (N = none), recorded in
  // one flag word per (host thread, device), allocated on first use; the kernel writes -1 for such a node
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  thread_local std::vector<int*> flag_words;
  if ((int)flag_words.size() <= dev) flag_words.resize(dev + 1, nullptr);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIPCHK(hipStreamIsCapturing(s, &cap));
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (!flag_words[dev]) {
    if (capturing) return fail(CHM_E_UNSUPPORTED, "chm_d3pm_sample: call it once outside capture on this thread first");
    HIPCHK(hipMalloc((void**)&flag_words[dev], sizeof(int)));
  }
  int* d_bad = flag_words[dev];
  int h_bad = N;
  hipError_t e = hipMemsetAsync(d_bad, 0x7f, sizeof(int), s);  // (0x7f7f7f7f: above any node index)
  if (e == hipSuccess)
    e = d3pm_sample(N, A, T, logits, A, nullptr, 1.f, 0.f, xt, tn, 0, nullptr, noise, q1, qm, out, 0, 0, s, d_bad);
  // under stream capture (a graph): no host readback; out-of-range nodes are the ones with out = -1
  if (capturing) {
    if (e != hipSuccess) return fail(CHM_E_HIP, std::string("chm_d3pm_sample: ") + hipGetErrorString(e));
    return CHM_OK;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(CHM_E_HIP, std::string("chm_d3pm_sample: ") + hipGetErrorString(e));
  if (h_bad < N)
    return fail(CHM_E_ARG, "d3pm_sample: node " + std::to_string(h_bad) + " has t outside [1, " + std::to_string(T) +
                               "] or x_t outside [0, " + std::to_string(A) + ")");
  return CHM_OK;
}

// The training kernels' arguments on the batch's decoder outputs (HO, LAT), for chm_training_loss and
// chm_debug_train_update alike. The per-node partials go to Y (decoder scratch, free after the decoder call).
TrainArgs chm::train_args(const chm_batch* b, const chm_train_tables* tt, const int64_t* d_t, const int64_t* a0,
                          const float* x0, const float* l0, const float* rand_a, const float* noise_l,
                          const float* noise_x, float* out, int64_t* a_t, float* x_t, float* l_t, float* target_x) {
  TrainArgs g;
  std::memset(&g, 0, sizeof(g));
  g.N = b->N; g.B = b->B; g.A = b->m->d.max_atoms; g.T = tt->T; g.t = d_t; g.a0 = a0; g.x0 = x0; g.l0 = l0;
  g.rand_a = rand_a; g.noise_l = noise_l; g.noise_x = noise_x; g.coef = tt->d_coef4;
  g.q_one_step = tt->d_q_one_step; g.q_mats = tt->d_q_mats; g.n2g = b->n2g;
  g.a_t = a_t; g.x_t = x_t; g.l_t = l_t; g.target_x = target_x;
  g.hybrid = tt->hybrid_coeff; g.cost_a = tt->cost_atom_types; g.cost_l = tt->cost_lattice; g.cost_x = tt->cost_coords;
  g.HO = b->HO; g.LAT = b->LAT; g.part = b->Y;
  g.out = out;
  return g;
}

extern "C" int chm_training_loss(chm_batch* b, const chm_train_tables* tt, const int64_t* d_t, const int64_t* a0,
                                 const float* x0, const float* l0, const float* temb, const float* text,
                                 const float* rand_a, const float* noise_l, const float* noise_x, float* out,
                                 int64_t* a_t, float* x_t, float* l_t, float* target_x, float* pred_lattice,
                                 float* pred_coords, void* stream) {
  if (!b || !tt || !d_t || !a0 || !x0 || !l0 || !rand_a || !noise_l || !noise_x || !out)
    return fail(CHM_E_ARG, "NULL argument");
  if (!a_t || !x_t || !l_t || !target_x) return fail(CHM_E_ARG, "the noised-state outputs are required");
  if (!tt->d_coef4 || !tt->d_q_one_step || !tt->d_q_mats || tt->T < 1) return fail(CHM_E_ARG, "bad tables");
  const chm_model* m = b->m;
  if (!m->film || !temb) return fail(CHM_E_ARG, "the training forward needs a time-conditioned decoder");
  if (m->d.text_dim > 0 && !text) return fail(CHM_E_ARG, "text embeddings required (text_dim > 0)");
  hipStream_t s = (hipStream_t)stream;
  const long N = b->N;
  const int B = b->B;
  const TrainArgs g = train_args(b, tt, d_t, a0, x0, l0, rand_a, noise_l, noise_x, out, a_t, x_t, l_t, target_x);
  HIPCHK(train_noise(g, s));
  int rc = run_decoder(b, 1, a_t, x_t, l_t, temb, m->d.time_dim, nullptr, text, nullptr, 3, s);
  if (rc) return rc;
  HIPCHK(train_loss(g, s));
  if (pred_lattice) HIPCHK(hipMemcpyAsync(pred_lattice, b->LAT, (size_t)B * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (pred_coords)
    HIPCHK(hipMemcpy2DAsync(pred_coords, 3 * sizeof(float), b->HO + m->d.max_atoms, HEADS_N * sizeof(float),
                            3 * sizeof(float), N, hipMemcpyDeviceToDevice, s));
  return CHM_OK;
}
