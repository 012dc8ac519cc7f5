// chm_model: the weight packer (chm_model_create), the math mode and the option table; and the error string of
// every entry point of the library (chm_last_error, chm::fail).
#include <cstdlib>

#include "chm_host.h"

using namespace chm;

static thread_local std::string g_err;

int chm::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" const char* chm_last_error(void) { return g_err.c_str(); }
extern "C" const char* chm_version(void) { return "chemeleon-mi355x 0.3 (gfx950; split16 / bf16x3 / f32 MFMA)"; }

// (time_dim = text_dim = 0: a CSPNet without FilmLayer, cspnet.py:210-211, e.g. CrystalClip's graph encoder)
static bool film_less(const chm_dims* d) { return d->time_dim == 0 && d->text_dim == 0; }
extern "C" int chm_num_params(const chm_dims* d) { return d ? (film_less(d) ? 1 : 7) + 10 * d->num_layers + 6 : 0; }

static int check_dims(const chm_dims* d) {
  if (!d) return fail(CHM_E_ARG, "dims is NULL");
  if (d->hidden_dim != H) return fail(CHM_E_UNSUPPORTED, "hidden_dim must be 512 in this build");
  if (d->num_freqs != NF) return fail(CHM_E_UNSUPPORTED, "num_freqs must be 128 in this build");
  if (d->time_dim != TD && !film_less(d))
    return fail(CHM_E_UNSUPPORTED, "time_dim must be 128 in this build (or time_dim = text_dim = 0)");
  if (d->text_dim < 0 || (TD + d->text_dim) % 16) return fail(CHM_E_UNSUPPORTED, "time_dim + text_dim must be a multiple of 16");
  if (d->max_atoms < 1 || d->max_atoms + 3 > HEADS_N) return fail(CHM_E_UNSUPPORTED, "max_atoms must be in [1, 125]");
  if (d->num_layers < 1 || d->num_layers > kMaxLayers) return fail(CHM_E_ARG, "num_layers out of range");
  return CHM_OK;
}

// The model's knobs, one row each: chm_model_create reads the rows with an environment variable (unchecked atoi /
// atol, whatever the row's kind and range), chm_model_set_option looks its key up. What a knob does is written at
// its chm_model field (chm_host.h). Beside the table: CHM_MATH (a string), CHM_EDGE_TRACE (a file name), the
// clamp of CHM_EDGE_LAG and the option edge16, in those two functions.
namespace {
struct Field {  // an int, long or unsigned member of chm_model
  int chm_model::*i = nullptr;
  long chm_model::*l = nullptr;
  unsigned chm_model::*u = nullptr;
  constexpr Field(int chm_model::*p) : i(p) {}
  constexpr Field(long chm_model::*p) : l(p) {}
  constexpr Field(unsigned chm_model::*p) : u(p) {}
  void set(chm_model* m, int64_t v) const {
    if (i) m->*i = (int)v;
    else if (l) m->*l = (long)v;
    else m->*u = (unsigned)v;
  }
};
enum Kind { FLAG, INT, BIT };  // set_option stores: value != 0; the value; the field with bit `lo` set or cleared
struct Option {
  const char* key;  // of chm_model_set_option, or null
  const char* env;  // read at chm_model_create, or null
  Field field;
  Kind kind;
  int64_t lo, hi;       // INT: the option's accepted range (BIT: lo = the bit)
  const char* refusal;  // INT: CHM_E_ARG's text outside [lo, hi]; null = every value is taken
};
using M = chm_model;
const Option kOptions[] = {
    {"node_ps", "CHM_NODE_PS", &M::node_ps, FLAG},
    {"edge_rows", "CHM_EDGE_ROWS", &M::edge_rows, FLAG},
    {"edge_layer", "CHM_EDGE_LAYER", &M::edge_layer, FLAG},
    {"edge_pairs", "CHM_EDGE_PAIRS", &M::edge_pairs, FLAG},
    {"edge_pairs_layer", "CHM_EDGE_PAIRS_LAYER", &M::edge_pairs_layer, FLAG},
    {"edge_rows_short", "CHM_EDGE_ROWS_SHORT", &M::edge_rows_short, FLAG},
    {"edge_lag", "CHM_EDGE_LAG", &M::edge_lag, INT, 1, kMaxLag, "edge_lag must be in [1, 1000]"},
    {"edge_layer_min", "CHM_EDGE_LAYER_MIN", &M::edge_layer_min, INT, 1, INT64_MAX, "edge_layer_min must be >= 1"},
    {"xcd_mask", nullptr, &M::xcd_mask, INT},
    {"edge_rows_nowait", nullptr, &M::edge_dbg, BIT, 64},
    {"edge_layer_repair", nullptr, &M::edge_dbg, BIT, 512},
    {"edge_pairs_pq_global", nullptr, &M::edge_dbg, BIT, 1048576},
    {nullptr, "CHM_EDGE_DBG", &M::edge_dbg, INT},
    {nullptr, "CHM_NODE_GLDS", &M::node_glds, INT},
    {nullptr, "CHM_NODE16", &M::node16, INT},
    {nullptr, "CHM_EDGE_STAGGER", &M::edge_stagger, INT},
    {nullptr, "CHM_EDGE_TRACE_LAYER", &M::edge_trace_layer, INT},
    {nullptr, "CHM_REPAIR_GRID", &M::repair_grid, INT},
};
}  // namespace

extern "C" int chm_model_create(const chm_dims* dims, const float* const* p, int n_params, void* stream,
                                chm_model** out) {
  if (!out) return fail(CHM_E_ARG, "out is NULL");
  *out = nullptr;
  int rc = check_dims(dims);
  if (rc) return rc;
  if (n_params != chm_num_params(dims)) return fail(CHM_E_ARG, "wrong number of parameter tensors");
  for (int i = 0; i < n_params; ++i)
    if (!p[i]) return fail(CHM_E_ARG, "parameter pointer " + std::to_string(i) + " is NULL");
  hipStream_t s = (hipStream_t)stream;
  const int A = dims->max_atoms, L = dims->num_layers, X = dims->text_dim;
  const bool film = !film_less(dims);
  const int CIN = film ? TD + X : 0, W1K = 2 * H + 9 + FD;
  const int PL = film ? 7 : 1;  // first layer parameter
  {
    hipError_t e0 = gemm_init();
    if (e0 == hipSuccess) e0 = edge16_init();
    if (e0 == hipSuccess) e0 = node_gemm_init();
    if (e0 != hipSuccess) return fail(CHM_E_HIP, std::string("gemm_init: ") + hipGetErrorString(e0));
  }

  // layout of the packed arena (each piece 256-byte aligned)
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; };
  const size_t o_emb = take((size_t)A * H), o_Wc = take((size_t)2 * H * CIN), o_bc = take(2 * H), o_Wp = take(H * H),
               o_bp = take(H), o_fw = take(H), o_fb = take(H);
  std::vector<size_t> lo(L * 12);
  for (int l = 0; l < L; ++l) {
    lo[l * 12 + 0] = take((size_t)2 * H * H);  // WAB
    lo[l * 12 + 1] = take((size_t)H * 9);      // Wcl
    lo[l * 12 + 2] = take(H);                  // b1
    lo[l * 12 + 3] = take((size_t)H * FD);     // D
    lo[l * 12 + 4] = take((size_t)H * H);      // W2
    lo[l * 12 + 5] = take(H);                  // b2
    lo[l * 12 + 6] = take((size_t)H * 2 * H);  // W3
    lo[l * 12 + 7] = take(H);                  // b3
    lo[l * 12 + 8] = take((size_t)H * H);      // W4
    lo[l * 12 + 9] = take(H);                  // b4
    lo[l * 12 + 10] = take(H);                 // lw
    lo[l * 12 + 11] = take(H);                 // lb
  }
  const size_t o_Wh = take((size_t)HEADS_N * H), o_bh = take(HEADS_N), o_Wl = take(9 * H), o_flw = take(H),
               o_flb = take(H);

  chm_model* m = new chm_model();
  m->d = *dims;
  m->film = film;
  m->mem_floats = off;
  hipError_t e = hipMalloc(&m->mem, off * sizeof(float));
  if (e != hipSuccess) {
    delete m;
    return fail(CHM_E_HIP, std::string("hipMalloc(model): ") + hipGetErrorString(e));
  }
  float* base = m->mem;
  auto cp = [&](size_t o, const float* src, size_t n) {
    return hipMemcpyAsync(base + o, src, n * sizeof(float), hipMemcpyDeviceToDevice, s);
  };
  // 2-D copy of a column block of a row-major [rows][src_ld] matrix
  auto cp2 = [&](size_t o, size_t dst_ld, const float* src, size_t src_ld, size_t col0, size_t cols, size_t rows) {
    return hipMemcpy2DAsync(base + o, dst_ld * sizeof(float), src + col0, src_ld * sizeof(float), cols * sizeof(float),
                            rows, hipMemcpyDeviceToDevice, s);
  };
#define CK(x)                                                                                  \
  do {                                                                                         \
    hipError_t _e = (x);                                                                       \
    if (_e != hipSuccess) {                                                                    \
      (void)hipFree(m->mem);                                                                   \
      delete m;                                                                                \
      return fail(CHM_E_HIP, std::string("weight packing: ") + hipGetErrorString(_e));         \
    }                                                                                          \
  } while (0)
  CK(hipMemsetAsync(base, 0, off * sizeof(float), s));
  CK(cp(o_emb, p[0], (size_t)A * H));
  if (film) {  // (film-less: the FiLM arena stays zero and is never read)
    CK(cp(o_Wc, p[1], (size_t)2 * H * CIN));
    CK(cp(o_bc, p[2], 2 * H));
    CK(cp(o_Wp, p[3], H * H));
    CK(cp(o_bp, p[4], H));
    CK(cp(o_fw, p[5], H));
    CK(cp(o_fb, p[6], H));
  }
  for (int l = 0; l < L; ++l) {
    const float* const* q = p + PL + 10 * l;
    // edge_mlp.0.weight [H][2H+9+FD] -> WAB = [W1[:, 0:H] ; W1[:, H:2H]], Wcl = W1[:, 2H:2H+9], D = W1[:, 2H+9:]
    CK(cp2(lo[l * 12 + 0], H, q[0], W1K, 0, H, H));
    CK(cp2(lo[l * 12 + 0] + (size_t)H * H, H, q[0], W1K, H, H, H));
    CK(cp2(lo[l * 12 + 1], 9, q[0], W1K, 2 * H, 9, H));
    CK(cp2(lo[l * 12 + 3], FD, q[0], W1K, 2 * H + 9, FD, H));
    CK(cp(lo[l * 12 + 2], q[1], H));
    CK(cp(lo[l * 12 + 4], q[2], (size_t)H * H));
    CK(cp(lo[l * 12 + 5], q[3], H));
    CK(cp(lo[l * 12 + 6], q[4], (size_t)H * 2 * H));
    CK(cp(lo[l * 12 + 7], q[5], H));
    CK(cp(lo[l * 12 + 8], q[6], (size_t)H * H));
    CK(cp(lo[l * 12 + 9], q[7], H));
    CK(cp(lo[l * 12 + 10], q[8], H));
    CK(cp(lo[l * 12 + 11], q[9], H));
  }
  const float* const* hq = p + PL + 10 * L;  // coord_out.w, lattice_out.w, type_out.w, type_out.b, final_ln.w, final_ln.b
  CK(cp(o_Wh, hq[2], (size_t)A * H));                 // rows 0..A-1: type_out
  CK(cp(o_Wh + (size_t)A * H, hq[0], (size_t)3 * H)); // rows A..A+2: coord_out
  CK(cp(o_bh, hq[3], A));
  CK(cp(o_Wl, hq[1], 9 * H));
  CK(cp(o_flw, hq[4], H));
  CK(cp(o_flb, hq[5], H));
  CK(hipStreamSynchronize(s));
#undef CK
  m->emb = base + o_emb; m->Wc = base + o_Wc; m->bc = base + o_bc; m->Wp = base + o_Wp; m->bp = base + o_bp;
  m->fw = base + o_fw; m->fb = base + o_fb; m->Whead = base + o_Wh; m->bhead = base + o_bh; m->Wlat = base + o_Wl;
  m->flw = base + o_flw; m->flb = base + o_flb;
  m->layers.resize(L);
  for (int l = 0; l < L; ++l) {
    LayerW& w = m->layers[l];
    const size_t* o = &lo[l * 12];
    w.WAB = base + o[0]; w.Wcl = base + o[1]; w.b1 = base + o[2]; w.D = base + o[3]; w.W2 = base + o[4];
    w.b2 = base + o[5]; w.W3 = base + o[6]; w.b3 = base + o[7]; w.W4 = base + o[8]; w.b4 = base + o[9];
    w.lw = base + o[10]; w.lb = base + o[11];
  }
  // bf16x3 planes of every GEMM weight (fp32-accurate bf16 MFMA path)
  {
    const char* env = getenv("CHM_MATH");
    const std::string mode = env ? env : "";
    m->math = mode == "f32" ? MATH_F32 : mode == "bf16x3" ? MATH_BF16X3 : MATH_SPLIT16;
    m->edge_trace = getenv("CHM_EDGE_TRACE");
    for (const Option& o : kOptions)
      if (const char* v = o.env ? getenv(o.env) : nullptr) o.field.set(m, o.field.l ? atol(v) : atoi(v));
    if (m->edge_lag < 1) m->edge_lag = 1;  // (CHM_EDGE_LAG is clamped; the option refuses such a value)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&m->ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      m->ncu = 0;
    m->device = dev;
    // the pair grid gives each of 8 XCDs a job list of its own: on a device or partition mode with fewer XCDs every
    // launch would end in its repair launches, so it runs only where 8 were seen
    if (m->ncu > 0 && xcd_mask(8 * m->ncu, &m->xcd_mask) != hipSuccess) m->xcd_mask = 0;
    struct Job { const float* src; size_t n; const void** dst; };
    std::vector<Job> jobs;
    jobs.push_back({m->Wc, (size_t)2 * H * CIN, &m->Wc3});
    jobs.push_back({m->Wp, (size_t)H * H, &m->Wp3});
    jobs.push_back({m->Whead, (size_t)HEADS_N * H, &m->Whead3});
    for (auto& w : m->layers) {
      jobs.push_back({w.WAB, (size_t)2 * H * H, &w.WAB3});
      jobs.push_back({w.D, (size_t)H * FD, &w.D3});
      jobs.push_back({w.W2, (size_t)H * H, &w.W23});
      jobs.push_back({w.W3, (size_t)H * 2 * H, &w.W33});
      jobs.push_back({w.W4, (size_t)H * H, &w.W43});
    }
    size_t total = 0;
    for (auto& j : jobs) total += (3 * j.n * 2 + 255) / 256 * 256;
    hipError_t e2 = hipMalloc(&m->mem3, total);
    if (e2 != hipSuccess) {
      (void)hipFree(m->mem);
      delete m;
      return fail(CHM_E_HIP, std::string("hipMalloc(planes): ") + hipGetErrorString(e2));
    }
    char* p3 = (char*)m->mem3;
    for (auto& j : jobs) {
      *j.dst = p3;
      hipError_t e3 = j.n ? split_planes(j.src, (long)j.n, p3, s) : hipSuccess;  // (film-less: no Wc)
      if (e3 != hipSuccess) {
        (void)hipFree(m->mem); (void)hipFree(m->mem3);
        delete m;
        return fail(CHM_E_HIP, std::string("split_planes: ") + hipGetErrorString(e3));
      }
      p3 += (3 * j.n * 2 + 255) / 256 * 256;
    }
    // fp16 hi/lo planes (+ row scales) of the two edge-GEMM weights of every layer
    const size_t per_layer = (2 * (size_t)H * FD * 2 + 2 * (size_t)H * H * 2 + 2 * H * 4 + 1023) / 1024 * 1024;
    e2 = hipMalloc(&m->mem2, per_layer * L);
    for (int l = 0; l < L && e2 == hipSuccess; ++l) {
      char* q = (char*)m->mem2 + per_layer * l;
      LayerW& w = m->layers[l];
      w.D2h = q;
      w.W22h16 = q + 2 * (size_t)H * FD * 2;
      w.Dsc = (float*)(q + 2 * (size_t)H * FD * 2 + 2 * (size_t)H * H * 2);
      w.W2sc = w.Dsc + H;
      e2 = split_rows_h(w.D, H, FD, w.D2h, w.Dsc, 0, s);
      if (e2 == hipSuccess) e2 = split_rows_h(w.W2, H, H, w.W22h16, w.W2sc, 2, s);  // (k_edge16's S layout)
    }
    // fp16 hi/lo rows (16-column chunks, + row scales) of the node-GEMM weights (split16 node GEMMs)
    if (e2 == hipSuccess) {
      struct J16 { const float* src; int n, k; void** dst; float** sc; };
      std::vector<J16> j16;
      void* wp16 = nullptr;
      j16.push_back({m->Wp, H, H, &wp16, &m->Wpsc});
      for (auto& w : m->layers) {
        j16.push_back({w.WAB, 2 * H, H, &w.WAB16, &w.WABsc});
        j16.push_back({w.W3, H, 2 * H, &w.W316, &w.W3sc});
        j16.push_back({w.W4, H, H, &w.W416, &w.W4sc});
      }
      auto sz = [](const J16& j) { return ((size_t)j.n * j.k * 4 + 255) / 256 * 256 + ((size_t)j.n * 4 + 255) / 256 * 256; };
      size_t tot = 0;
      for (auto& j : j16) tot += sz(j);
      e2 = hipMalloc(&m->mem16, tot);
      char* q = (char*)m->mem16;
      for (auto& j : j16) {
        if (e2 != hipSuccess) break;
        *j.dst = q;
        *j.sc = (float*)(q + ((size_t)j.n * j.k * 4 + 255) / 256 * 256);
        e2 = split_rows_h(j.src, j.n, j.k, *j.dst, *j.sc, 0, s, 16);
        q += sz(j);
      }
      m->Wp16 = wp16;
    }
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(s);
    if (e2 != hipSuccess) {
      (void)hipFree(m->mem); (void)hipFree(m->mem3); (void)hipFree(m->mem2); (void)hipFree(m->mem16);
      delete m;
      return fail(CHM_E_HIP, std::string("plane split: ") + hipGetErrorString(e2));
    }
  }
  *out = m;
  return CHM_OK;
}

extern "C" int chm_model_set_math(chm_model* m, int mode) {
  if (!m) return fail(CHM_E_ARG, "model is NULL");
  if (mode != CHM_MATH_BF16X3 && mode != CHM_MATH_F32 && mode != CHM_MATH_SPLIT16)
    return fail(CHM_E_ARG, "unknown math mode");
  m->math = mode;
  return CHM_OK;
}

extern "C" int chm_model_get_math(const chm_model* m) { return m ? m->math : -1; }

extern "C" int chm_model_set_option(chm_model* m, const char* key, int64_t value) {
  if (!m || !key) return fail(CHM_E_ARG, "NULL argument");
  const std::string k = key;
  if (k == "edge16") {  // (no knob any more: the round-1 32x32x16 edge kernels were removed in round 3)
    if (value == 0) return fail(CHM_E_UNSUPPORTED, "edge16 = 0: the 32x32x16 edge kernels were removed");
    return CHM_OK;
  }
  for (const Option& o : kOptions) {
    if (!o.key || k != o.key) continue;
    if (o.kind == INT && o.refusal && (value < o.lo || value > o.hi)) return fail(CHM_E_ARG, o.refusal);
    const int dbg = m->edge_dbg, bit = (int)o.lo;
    o.field.set(m, o.kind == FLAG ? value != 0 : o.kind == BIT ? (value ? (dbg | bit) : (dbg & ~bit)) : value);
    return CHM_OK;
  }
  return fail(CHM_E_ARG, "unknown option: " + k);
}

extern "C" void chm_model_destroy(chm_model* m) {
  if (!m) return;
  (void)hipFree(m->mem);
  (void)hipFree(m->mem3);
  (void)hipFree(m->mem2);
  (void)hipFree(m->mem16);
  delete m;
}
