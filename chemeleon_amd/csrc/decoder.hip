// The decoder driver: the launches of one decoder call on a batch (run_decoder and the pieces it is made of, which
// the test hooks of debug_hooks.hip call as well), the per-kernel profiling records, and the entry points that run
// the decoder or single pieces of it.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "chm_host.h"

using namespace chm;

// ---------------------------------------------------------------- instrumentation
bool chm::g_prof_on = false;
namespace {
struct ProfRec { int id; hipEvent_t a, b; };
std::mutex g_prof_mu;
std::vector<hipEvent_t> g_pool;
std::vector<ProfRec> g_recs;
size_t g_pool_next = 0;
constexpr size_t kPoolPairs = 8192;
}  // namespace

ProfScope::ProfScope(int id_, hipStream_t s_) : id(id_), s(s_) {
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_pool_next + 2 > g_pool.size()) return;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;  // not in graphs
  hipEvent_t a = g_pool[g_pool_next++];
  b = g_pool[g_pool_next++];
  if (hipEventRecord(a, s) != hipSuccess) { b = nullptr; return; }
  g_recs.push_back({id, a, b});
}

extern "C" int chm_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (on && g_pool.empty()) {
    g_pool.resize(2 * kPoolPairs);
    for (auto& e : g_pool)
      if (hipEventCreate(&e) != hipSuccess) return fail(CHM_E_HIP, "hipEventCreate failed");
  }
  g_prof_on = on != 0;
  return CHM_OK;
}

extern "C" int chm_prof_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_recs.clear();
  g_pool_next = 0;
  return CHM_OK;
}

extern "C" int chm_prof_read(int kernel, int64_t* launches, double* total_ms) {
  if (!launches || !total_ms) return fail(CHM_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int64_t n = 0;
  double tot = 0;
  for (const auto& r : g_recs) {
    if (r.id != kernel) continue;
    float ms = 0;
    hipError_t e = hipEventElapsedTime(&ms, r.a, r.b);
    if (e != hipSuccess) return fail(CHM_E_HIP, std::string("hipEventElapsedTime: ") + hipGetErrorString(e));
    ++n;
    tot += ms;
  }
  *launches = n;
  *total_ms = tot;
  return CHM_OK;
}

extern "C" int chm_prof_events(int64_t* out, int n) {
  if (!out || n < 1) return fail(CHM_E_ARG, "NULL argument");
  unsigned long long v[EV_COUNT];
  hipError_t e = edge_events_read(v);
  if (e != hipSuccess) return fail(CHM_E_HIP, std::string("edge_events_read: ") + hipGetErrorString(e));
  for (int k = 0; k < n; ++k) out[k] = k < EV_COUNT ? (int64_t)v[k] : 0;
  return CHM_OK;
}

extern "C" int chm_prof_events_reset(void) {
  hipError_t e = edge_events_reset();
  if (e != hipSuccess) return fail(CHM_E_HIP, std::string("edge_events_reset: ") + hipGetErrorString(e));
  return CHM_OK;
}

static GemmArgs gargs(long M, int N, int K, const float* A, long lda, const float* W, float* C, long ldc) {
  GemmArgs g;
  std::memset(&g, 0, sizeof(g));
  g.M = M; g.N = N; g.K = K; g.A = A; g.lda = lda; g.A2 = A; g.lda2 = lda; g.ksplit = K;
  g.W = W; g.ldw = K; g.C = C; g.ldc = ldc; g.gb_rowmod = 1;
  return g;
}

// W16 / wsc: the split16 node-GEMM rows of the same weight (null: bf16x3 in every mode)
static hipError_t run_gemm(const chm_batch* b, GemmArgs g, int epi, const void* W3, hipStream_t s,
                           const void* W16 = nullptr, const float* wsc = nullptr) {
  if (b->math == MATH_F32) return gemm(g, epi, s);
  if (b->math == MATH_SPLIT16 && W16 && (g.amax || g.aex) && b->m->node16 && b->m->node_glds && epi == EPI_STD) {
    g.Wp3 = W16; g.wscale = wsc;
    return node_gemm(g, s);
  }
  g.Wp3 = W3;
  if (epi == EPI_STD && b->m->node_glds) return node_gemm(g, s);
  return gemm_bf16x3(g, epi, s);
}

// the two edge GEMMs (M = E or P*E rows) in f32 / bf16x3 mode: 256x256 bf16x3 tiles
static hipError_t run_edge_gemm(const chm_batch* b, GemmArgs g, int epi, const void* W3, hipStream_t s) {
  if (b->math == MATH_F32) return gemm(g, epi, s);
  g.Wp3 = W3;
  return gemm_bf16x3_big(g, epi, s);
}

// profiling (CHM_EDGE_TRACE=file, CHM_EDGE_TRACE_LAYER=1, 2 or 4): the 4th eager launch of edge layer
// 1 or 2 (4: of the pair grid) records {hw id, t0, t_mainloop, t_end, ...} per block (s_memrealtime), dumped to the file
template <class F>
static hipError_t traced_edge_launch(const chm_model* m, EdgeArgs& ea, int which, long E, hipStream_t s, F&& launch) {
  static std::atomic<int> traced{0};
  hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
  const bool tr = m->edge_trace && m->edge_trace_layer == which && traced < 4 &&
                  hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusNone && ++traced == 4;
  if (!tr) return launch();
  unsigned long long* tbuf = nullptr;
  // (4, the pair grid: 8 x its longest job list, at most E / 32 jobs)
  const long tblocks = (which == 4 ? E / 4 : 4 * (E / 128 + 1)) + 4096;
  hipError_t e = hipMalloc(&tbuf, tblocks * 48);
  if (e == hipSuccess) e = hipMemsetAsync(tbuf, 0, tblocks * 48, s);
  if (e != hipSuccess) return e;
  ea.trace = tbuf;
  e = launch();
  ea.trace = nullptr;
  std::vector<unsigned long long> h(tblocks * 6);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemcpy(h.data(), tbuf, tblocks * 48, hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    FILE* f = fopen(m->edge_trace, "wb");
    if (f) {
      fwrite(h.data(), 8, h.size(), f);
      fclose(f);
    }
  }
  (void)hipFree(tbuf);
  return e;
}

namespace chm {  // (the functions chm_host.h declares, up to run_decoder)

// knn batches: the radius graph of these coordinates (knn.hip), edges grouped by source node. One
// stream sync reads the out-degrees back to size the launches and build the segment tiles.
int knn_build(chm_batch* b, const float* x, const float* lat, hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return fail(CHM_E_UNSUPPORTED, "knn batches rebuild their edges on the host's schedule: no graph capture");
  const int B = b->B;
  const long N = b->N;
  KnnArgs k;
  std::memset(&k, 0, sizeof(k));
  k.x = x; k.lat = lat; k.natoms = b->natoms; k.node_off = b->node_off; k.cand_off = b->cand_off;
  k.cand_key = b->cand_key; k.cand_d2 = b->cand_d2; k.cand2 = b->cand2; k.atom_cnt = b->atom_cnt;
  k.max_nb = b->knn_max_nb; k.fin_key = b->fin_key; k.fin_fd = b->fin_fd; k.deg = b->deg; k.cryst_fin = b->cryst_fin;
  k.node_estart = b->node_estart; k.ei = b->ei; k.ej = b->ej; k.fd = b->fd;
  HIPCHK(knn_candidates(k, B, s));
  b->h_deg.resize(N);
  HIPCHK(hipMemcpyAsync(b->h_deg.data(), b->deg, N * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  b->h_estart.resize(N);
  b->h_tiles.clear();
  long E = 0, rows = 0;
  int cur0 = 0;
  for (long v = 0; v < N; ++v) {  // segment tiles: runs of whole nodes of <= 256 edge rows (as batch_fill)
    const int d = b->h_deg[v];
    if (d > kTileRows) return fail(CHM_E_UNSUPPORTED, "knn: a node with more than 256 edges");
    b->h_estart[v] = E;
    E += d;
    if (rows + d > kTileRows || v - cur0 >= kTileRows) {  // (<= 256 nodes: isolated atoms add no rows)
      b->h_tiles.push_back(make_int2(cur0, (int)v));
      cur0 = (int)v;
      rows = 0;
    }
    rows += d;
  }
  b->h_tiles.push_back(make_int2(cur0, (int)N));
  if (E > b->E_cap)
    return fail(CHM_E_UNSUPPORTED, "knn: the graph has " + std::to_string(E) + " edges, above the batch capacity " +
                                       std::to_string(b->E_cap) + " (chm_batch_options.knn_edges_per_atom)");
  HIPCHK(hipMemcpyAsync(b->node_estart, b->h_estart.data(), N * sizeof(long), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b->node_n, b->h_deg.data(), N * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b->tiles, b->h_tiles.data(), b->h_tiles.size() * sizeof(int2), hipMemcpyHostToDevice, s));
  HIPCHK(knn_place(k, B, s));
  b->E = E;
  b->ntiles = (int)b->h_tiles.size();
  return CHM_OK;
}

// the EdgePlan (chm_host.h) of a decoder call with P conditionings on this batch
EdgePlan edge_plan(const chm_batch* b, int P) {
  const chm_model* m = b->m;
  EdgePlan p;
  p.n16 = b->math == MATH_SPLIT16 && m->node16 && m->node_glds;
  p.ps = p.n16 && m->node_ps && b->Hs;
  p.pairs = b->math == MATH_SPLIT16 && m->edge_pairs && b->pe && !b->knn && b->E > 0;
  // (edge layer 1 on pairs as two launches, the default below 256 row tiles: no intra-grid waits, nothing to clear;
  // the memsets cost 4.8 us each per call, 0.9% of a 64x20 step)
  p.pair_grid = p.pairs && m->edge_pairs_layer && m->edge_rows && b->rtiles && m->edge_layer && b->psched &&
                P == b->P && b->nrt >= m->edge_layer_min && m->ncu > 0 && m->xcd_mask == 0xffu && b->rt_nbig < 0;
  p.zero_grid = b->xbad && b->math == MATH_SPLIT16 && p.pair_grid;
  return p;
}

// The pair grid's repair requests (layer l: xbad[l]) and per-layer flags (zero_grid) start clear in every call:
// run_decoder's embedding launch clears them; grid_too: this does (chm_debug_edge_layer has no such launch).
int clear_edge_flags(chm_batch* b, const EdgePlan& ep, hipStream_t s, bool grid_too) {
  const int L = b->m->d.num_layers;
  if (grid_too && ep.zero_grid) {
    HIPCHK(hipMemsetAsync(b->xbad, 0, 2 * kMaxLayers * sizeof(unsigned), s));
    HIPCHK(hipMemsetAsync(b->psched, 0, (size_t)L * 8 * b->pplan.npx * sizeof(unsigned), s));
  }
  return CHM_OK;
}

// The Fourier features of the call's edges (pairs: of the (i, j) edges, i <= j) into F, in the math mode's form.
int edge_features(chm_batch* b, const EdgePlan& ep, const float* x, hipStream_t s) {
  const long E = b->E;
  const bool pairs = ep.pairs;
  if (pairs)
    HIPCHK(fourier_h(x, b->pi, b->pj, b->Ep, b->F, s, nullptr));  // (the (i, j) edges' features, i <= j)
  else if (b->math == MATH_SPLIT16)
    HIPCHK(fourier_h(x, b->ei, b->ej, E, b->F, s, b->knn ? b->fd : nullptr));  // fp16 hi/lo split rows
  else
    HIPCHK(fourier(x, b->ei, b->ej, E, b->F, s));
  return CHM_OK;
}

// The message path of CSP layer l on the batch's buffers, every math mode: F (features) and PQ (the per-node halves
// of edge layer 1, P with b1 + the per-graph term) -> agg = mean_j SiLU(SiLU(D f_ij + P[i] + Q[j]) W2^T + b2).
// ps: agg is written as split rows + chunk exponents (aggs / agge) instead of fp32 rows + row maxima.
int edge_block(chm_batch* b, int P, int l, const EdgePlan& ep, bool ps, hipStream_t s) {
  const chm_model* m = b->m;
  const long N = b->N, E = b->E;
  const LayerW& w = m->layers[l];
  const bool pairs = ep.pairs, pair_grid = ep.pair_grid;
  const long RS = (long)b->P * N;
  auto rmx = [&](int k) { return ep.n16 && !ps ? b->rmx + k * RS : nullptr; };
  if (b->math == MATH_SPLIT16 && E == 0) {  // (knn: no atom within any other's radius: every mean is 0)
    HIPCHK(hipMemsetAsync(b->agg, 0, (size_t)P * N * H * sizeof(float), s));
    if (ps) {
      HIPCHK(hipMemsetAsync(b->aggs, 0, (size_t)P * N * H * 4, s));
      HIPCHK(hipMemsetAsync(b->agge, 0, (size_t)P * N * sizeof(int), s));
    }
  } else if (b->math == MATH_SPLIT16) {
    // split16: fp16 hi/lo split rows throughout (edge16.hip). S lives in S's bytes as
    // split rows [P*E][H/32][2][32] plus one packed exponent word per row (rowmax buffer).
    int* sexp = reinterpret_cast<int*>(b->rowmax);
    // edge layer 1: S_c = SiLU(D f_ij + P_c[i] + Q_c[j]), D f shared by the pair
    EdgeArgs e1;
    std::memset(&e1, 0, sizeof(e1));
    e1.M = E; e1.N = H; e1.K = FD; e1.A = b->F; e1.W = w.D2h; e1.wscale = w.Dsc;
    e1.ei = b->ei; e1.ej = b->ej; e1.PQ = b->PQ; e1.nnodes = N; e1.npairs = P; e1.E = E;
    e1.node_off = b->node_off; e1.natoms = b->natoms; e1.n2g = b->n2g;
    e1.S = b->S; e1.sexp = sexp; e1.dbg = m->edge_dbg; e1.stagger = m->edge_stagger;
    // edge layer 2 fused with the aggregation: agg = mean_j SiLU(S W2^T + b2)
    EdgeArgs e2;
    std::memset(&e2, 0, sizeof(e2));
    e2.M = (long)P * E; e2.N = H; e2.K = H; e2.A = b->S; e2.aexp = sexp;
    e2.W = w.W22h16; e2.wscale = w.W2sc; e2.bias = w.b2; e2.tiles = b->tiles;
    e2.ntiles = b->ntiles;
    e2.node_estart = b->node_estart; e2.natoms = b->natoms; e2.n2g = b->n2g; e2.agg = b->agg;
    e2.node_n = b->node_n; e2.agg_max = reinterpret_cast<unsigned*>(rmx(RMX_AGG));
    if (ps) { e2.aggs = b->aggs; e2.agge = b->agge; }
    e2.nnodes = N; e2.npairs = P; e2.E = E; e2.dbg = m->edge_dbg; e2.stagger = m->edge_stagger;
    if (m->edge_rows && b->rtiles) {  // 256-row tiles, cut nodes continued across tiles
      e2.rtiles = b->rtiles; e2.ntiles = (int)b->nrt; e2.sbuf = b->sbuf; e2.msgbuf = b->msgbuf;
      e2.rinfo = b->rinfo; e2.rinfo_n = b->rinfo_n;
      e2.rcnt = b->rcnt; e2.r2tot = b->r2tot;
    }
    // edge layer 2 on the two-launch schedule: one launch, or on a mixed row tiling (short_row_tiles) its 256-row
    // tiles, then its 192-row tiles (k_edge16_short)
    auto layer2 = [&](const EdgeArgs& ga) -> hipError_t {
      if (!ga.rtiles || b->rt_nbig < 0) return edge_gemm16(ga, EPI_SEGMEAN, s);
      if (b->rt_nbig > 0) {
        EdgeArgs gb = ga;
        gb.rt_count = (int)b->rt_nbig;
        if (hipError_t r = edge_gemm16(gb, EPI_SEGMEAN, s); r != hipSuccess) return r;
      }
      EdgeArgs gs = ga;
      gs.rt_first = (int)b->rt_nbig;
      gs.rt_count = (int)(b->nrt - b->rt_nbig);
      gs.rt_h = kShortRows;
      gs.rt_e0 = b->rt_nbig * kTileRows;
      return edge_gemm16(gs, EPI_SEGMEAN, s);
    };
    // (same-box A/B, static grid against two launches: 64x40 8.47 -> 7.77 ms per step, 512x40 54.9 -> 54.8,
    // 64x20 2.95 -> 3.10: 100 row tiles leave each XCD's job list too short to pack; profiles/r5/grid/)
    if (pair_grid) {
      // both edge layers in one grid, layer 1 on pairs (k_edge16_pairs_grid)
      EdgeArgs e1p = e1;
      e1p.M = b->Ep; e1p.Mp = b->Ep; e1p.pi = b->pi; e1p.pj = b->pj; e1p.pe = b->pe; e1p.pnode = b->pnode;
      e1p.xbad = e2.xbad = b->xbad + l;
      PairSched ps;
      ps.jobs = b->pjobs; ps.jstride = b->pplan.jstride;
      ps.npx = b->pplan.npx; ps.pflag = b->psched + (size_t)l * 8 * b->pplan.npx; ps.R = b->nrt;
      ProfScope ps_(CHM_K_EDGE_LAYER, s);
      // (CHM_EDGE_TRACE_LAYER=4: block timelines of this grid, slot = blockIdx)
      HIPCHK(traced_edge_launch(m, e2, 4, E, s, [&] {
        ps.trace = e2.trace;
        e2.trace = nullptr;
        const hipError_t r = edge_gemm16_pairs_layer(e1p, e2, ps, m->repair_grid, s);
        ps.trace = nullptr;
        return r;
      }));
    } else if (pairs) {
      // edge layer 1 on pairs (both directions' S rows per pair), then edge layer 2 on its row tiles
      EdgeArgs e1p = e1;
      e1p.M = b->Ep; e1p.Mp = b->Ep; e1p.pi = b->pi; e1p.pj = b->pj; e1p.pe = b->pe; e1p.pnode = b->pnode;
      {
        ProfScope ps(CHM_K_EDGE_FOURIER, s);
        HIPCHK(edge_gemm16_pairs(e1p, s));
      }
      ProfScope ps(CHM_K_EDGE_MESSAGE, s);
      HIPCHK(layer2(e2));
    } else {
      {
        ProfScope ps(CHM_K_EDGE_FOURIER, s);
        HIPCHK(traced_edge_launch(m, e1, 1, E, s, [&] {
          return edge_gemm16(e1, EPI_EDGE, s);
        }));
      }
      ProfScope ps(CHM_K_EDGE_MESSAGE, s);
      HIPCHK(traced_edge_launch(m, e2, 2, E, s, [&] {
        return layer2(e2);
      }));
    }
  } else {
    {  // edge layer 1: S_c = SiLU(D f_ij + P_c[i] + Q_c[j]), D f shared by the pair
      GemmArgs g = gargs(E, H, FD, b->F, FD, w.D, b->S, H);
      g.ei = b->ei; g.ej = b->ej; g.PQ = b->PQ; g.nnodes = N; g.npairs = P; g.E = E;
      ProfScope ps(CHM_K_EDGE_FOURIER, s);
      HIPCHK(run_edge_gemm(b, g, EPI_EDGE, w.D3, s));
    }
    if (b->math == MATH_F32) {
      {  // edge layer 2: M = SiLU(S W2^T + b2)
        GemmArgs g = gargs((long)P * E, H, H, b->S, H, w.W2, b->M, H);
        g.bias = w.b2; g.act = 1;
        ProfScope ps(CHM_K_EDGE_MESSAGE, s);
        HIPCHK(gemm(g, EPI_STD, s));
      }
      ProfScope ps(CHM_K_SEGMENT_MEAN, s);
      HIPCHK(segment_mean(b->M, b->agg, b->n2g, b->node_off, b->edge_off, b->natoms, N, E, P, s));
    } else {  // edge layer 2 fused with the aggregation: agg = mean_j SiLU(S W2^T + b2), M never stored
      GemmArgs g = gargs((long)P * E, H, H, b->S, H, w.W2, nullptr, H);
      g.bias = w.b2; g.act = 1; g.tiles = b->tiles; g.ntiles = b->ntiles; g.node_estart = b->node_estart;
      g.natoms = b->natoms; g.n2g = b->n2g; g.agg = b->agg; g.nnodes = N; g.npairs = P; g.E = E;
      ProfScope ps(CHM_K_EDGE_MESSAGE, s);
      HIPCHK(run_edge_gemm(b, g, EPI_SEGMEAN, w.W23, s));
    }
  }
  return CHM_OK;
}

// The decoder's node-side glue launches (everything of a decoder call that is neither a GEMM nor the message path),
// each with its arguments built from the batch, the call's EdgePlan and P: run_decoder and chm_debug_node_stage
// call these same functions.
// row k (RMX_*) of the split16 node GEMMs' row-max arrays, null where the plan keeps none
float* rmx_row(const chm_batch* b, const EdgePlan& ep, int k) {
  return ep.n16 && !ep.ps ? b->rmx + k * ((long)b->P * b->N) : nullptr;
}
// cin [P,B,TD+X] = [time embedding | text rows]
int node_cond_in(chm_batch* b, int P, const float* temb, int tstride, const int* d_t, const float* text0,
                 const float* text1, hipStream_t s) {
  HIPCHK(build_cond_in(temb, tstride, d_t, text0, text1, b->m->d.text_dim, b->cin, b->B, P, s));
  return CHM_OK;
}
// the embedding rows and the first kGBLayers layers' per-graph terms of edge layer 1 in one launch
// (the pair grid's repair requests and per-layer flags start clear in every call: zeroed by this launch, two
// memset nodes less per call)
int node_embed(chm_batch* b, const EdgePlan& ep, int P, const int64_t* a, const float* lat, hipStream_t s) {
  const chm_model* m = b->m;
  const int L = m->d.num_layers;
  const bool ps = ep.ps, zero_grid = ep.zero_grid;
  GraphBiasArgs ga0;
  const int nl0 = L < kGBLayers ? L : kGBLayers;
  for (int l = 0; l < nl0; ++l) {
    ga0.Wc[l] = m->layers[l].Wcl;
    ga0.b1[l] = m->layers[l].b1;
  }
  HIPCHK(embed(a, m->emb, b->Hres, b->N, P, s, rmx_row(b, ep, RMX_H), ps ? b->Hs : nullptr, ps ? b->He : nullptr, lat,
               nl0 > 0 ? &ga0 : nullptr, nl0, 9, b->gbias, b->B, zero_grid ? b->xbad : nullptr,
               zero_grid ? 2L * kMaxLayers : 0L, zero_grid ? b->psched : nullptr,
               zero_grid ? (long)L * 8 * b->pplan.npx : 0L));
  return CHM_OK;
}
// the per-graph terms of layers past the first kGBLayers
int node_graph_bias_rest(chm_batch* b, const float* lat, hipStream_t s) {
  const chm_model* m = b->m;
  const int L = m->d.num_layers, B = b->B;
  for (int l0 = kGBLayers; l0 < L; l0 += kGBLayers) {
    GraphBiasArgs ga;
    const int nl = L - l0 < kGBLayers ? L - l0 : kGBLayers;
    for (int l = 0; l < nl; ++l) {
      ga.Wc[l] = m->layers[l0 + l].Wcl;
      ga.b1[l] = m->layers[l0 + l].b1;
    }
    HIPCHK(graph_bias(lat, ga, nl, 9, b->gbias + (size_t)l0 * B * H, B, s));
  }
  return CHM_OK;
}
// FiLM + residual + layer l's LayerNorm (film-less: the LayerNorm only)
int node_film_ln(chm_batch* b, const EdgePlan& ep, int P, int l, hipStream_t s) {
  const chm_model* m = b->m;
  const LayerW& w = m->layers[l];
  const bool ps = ep.ps;
  HIPCHK(film_ln(m->film ? b->Y : nullptr, b->Hres, b->Hl, b->cemb, b->n2g, b->N, b->B, P, m->fw, m->fb, w.lw, w.lb, s,
                 rmx_row(b, ep, 0), (long)b->P * b->N, ps ? b->Hls : nullptr, ps ? b->Hle : nullptr));
  return CHM_OK;
}
int node_final_ln(chm_batch* b, int P, hipStream_t s) {
  HIPCHK(layer_norm(b->Hres, b->Hf, (long)P * b->N, b->m->flw, b->m->flb, s));
  return CHM_OK;
}
int node_graph_heads(chm_batch* b, int P, const float* lat, hipStream_t s) {
  HIPCHK(graph_heads(b->Hf, b->m->Wlat, lat, b->node_off, b->natoms, b->N, b->B, P, b->LAT, s));
  return CHM_OK;
}
int node_split_heads(chm_batch* b, int P, float* types, float* coords, hipStream_t s) {
  HIPCHK(split_heads(b->HO, (long)P * b->N, b->m->d.max_atoms, types, coords, s));
  return CHM_OK;
}

// reuse_cond: the FiLM conditioning (cond_in + the conditioning MLP) of the previous call on this batch
// is still valid (same t and text: the corrector call of a reverse step, chemeleon.py:438-448)
// heads: bit 0 = node heads (types + coords), bit 1 = lattice head
int run_decoder(chm_batch* b, int P, const int64_t* a, const float* x, const float* lat, const float* temb,
                int tstride, const int* d_t, const float* text0, const float* text1, int heads, hipStream_t s,
                bool reuse_cond) {
  const chm_model* m = b->m;
  if (b->knn) {
    const int rc = knn_build(b, x, lat, s);
    if (rc) return rc;
  }
  const int L = m->d.num_layers, X = m->d.text_dim, B = b->B;
  const long N = b->N, R = (long)P * N;
  const int CIN = TD + X;
  ProfScope whole(CHM_K_DECODER, s);
  const EdgePlan ep = edge_plan(b, P);
  const bool ps = ep.ps;
  auto rmx = [&](int k) { return rmx_row(b, ep, k); };
  if (m->film && !reuse_cond) {
    if (const int rc = node_cond_in(b, P, temb, tstride, d_t, text0, text1, s)) return rc;
    GemmArgs g = gargs((long)P * B, 2 * H, CIN, b->cin, CIN, m->Wc, b->cemb, 2 * H);
    g.bias = m->bc; g.act = 1;
    HIPCHK(run_gemm(b, g, EPI_STD, m->Wc3, s));
  }
  if (const int rc = node_embed(b, ep, P, a, lat, s)) return rc;
  if (const int rc = edge_features(b, ep, x, s)) return rc;
  if (const int rc = node_graph_bias_rest(b, lat, s)) return rc;
  if (const int rc = clear_edge_flags(b, ep, s, false)) return rc;
  for (int l = 0; l < L; ++l) {
    const LayerW& w = m->layers[l];
    if (m->film) {  // FiLM projection (cspnet.py:92)
      GemmArgs g = gargs(R, H, H, ps ? (const float*)b->Hs : b->Hres, H, m->Wp, b->Y, H);
      g.bias = m->bp; g.amax = rmx(RMX_H);
      if (ps) g.aex = b->He;
      HIPCHK(run_gemm(b, g, EPI_STD, m->Wp3, s, m->Wp16, m->Wpsc));
    }
    if (const int rc = node_film_ln(b, ep, P, l, s)) return rc;
    {  // per-node halves of the first edge layer: [P | Q] = Hl [A ; Bm]^T, P += b1 + C vec(LL^T)
      GemmArgs g = gargs(R, 2 * H, H, ps ? (const float*)b->Hls : b->Hl, H, w.WAB, b->PQ, 2 * H);
      g.gb = b->gbias + (size_t)l * B * H; g.ldgb = H; g.gb_cols = H; g.row2g = b->n2g; g.gb_rowmod = N;
      g.amax = rmx(RMX_HL);
      if (ps) g.aex = b->Hle;
      HIPCHK(run_gemm(b, g, EPI_STD, w.WAB3, s, w.WAB16, w.WABsc));
    }
    if (const int rc = edge_block(b, P, l, ep, ps, s)) return rc;
    {  // node MLP 1: U = SiLU([Hl | agg] W3^T + b3)
      GemmArgs g = gargs(R, H, 2 * H, b->Hl, H, w.W3, b->Y, H);
      g.A2 = b->agg; g.lda2 = H; g.ksplit = H; g.bias = w.b3; g.act = 1;
      g.amax = rmx(RMX_HL); g.amax2 = rmx(RMX_AGG); g.cmax = reinterpret_cast<unsigned*>(rmx(RMX_U));
      if (ps) {  // U exists only as the next GEMM's split operand
        g.A = (const float*)b->Hls; g.A2 = (const float*)b->aggs; g.aex = b->Hle; g.aex2 = b->agge;
        g.C = nullptr; g.Cs = b->Us; g.cex = b->Ue;
      }
      HIPCHK(run_gemm(b, g, EPI_STD, w.W33, s, w.W316, w.W3sc));
    }
    {  // node MLP 2 + residual: Hres += SiLU(U W4^T + b4)
      GemmArgs g = gargs(R, H, H, b->Y, H, w.W4, b->Hres, H);
      g.bias = w.b4; g.act = 1; g.R = b->Hres; g.ldr = H;
      g.amax = rmx(RMX_U); g.cmax = reinterpret_cast<unsigned*>(rmx(RMX_H));
      if (ps) {  // (and the residual stream split for the next layer's FiLM projection)
        g.A = (const float*)b->Us; g.aex = b->Ue;
        if (l + 1 < L && m->film) { g.Cs = b->Hs; g.cex = b->He; }
      }
      HIPCHK(run_gemm(b, g, EPI_STD, w.W43, s, w.W416, w.W4sc));
    }
  }
  if (const int rc = node_final_ln(b, P, s)) return rc;
  if (heads & 1) {
    GemmArgs g = gargs(R, HEADS_N, H, b->Hf, H, m->Whead, b->HO, HEADS_N);
    g.bias = m->bhead;
    HIPCHK(run_gemm(b, g, EPI_STD, m->Whead3, s));  // (bf16x3: A is LayerNorm output, M small)
  }
  if (heads & 2)
    if (const int rc = node_graph_heads(b, P, lat, s)) return rc;
  return CHM_OK;
}

}  // namespace chm

extern "C" int chm_decoder_forward(chm_batch* b, int pairs, const int64_t* a, const float* x, const float* lat,
                                   const float* temb, int time_stride, const float* text, float* types_out,
                                   float* lattice_out, float* coords_out, float* node_out, void* stream) {
  if (!b) return fail(CHM_E_ARG, "batch is NULL");
  if (pairs < 1 || pairs > b->P) return fail(CHM_E_ARG, "pairs must be in [1, max_pairs]");
  if (!a || !x || !lat || (b->m->film && !temb)) return fail(CHM_E_ARG, "inputs must not be NULL");
  const int X = b->m->d.text_dim;
  if (X > 0 && !text) return fail(CHM_E_ARG, "text embeddings required (text_dim > 0)");
  hipStream_t s = (hipStream_t)stream;
  const float* t0 = text;
  const float* t1 = text ? text + (size_t)b->B * X : nullptr;
  const int heads = ((types_out || coords_out) ? 1 : 0) | (lattice_out ? 2 : 0);
  int rc = run_decoder(b, pairs, a, x, lat, temb, time_stride, nullptr, t0, t1, heads, s);
  if (rc) return rc;
  const long R = (long)pairs * b->N;
  if (heads & 1)
    if (const int rc = node_split_heads(b, pairs, types_out, coords_out, s)) return rc;
  if (lattice_out)
    HIPCHK(hipMemcpyAsync(lattice_out, b->LAT, (size_t)pairs * b->B * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (node_out) HIPCHK(hipMemcpyAsync(node_out, b->Hf, (size_t)R * H * sizeof(float), hipMemcpyDeviceToDevice, s));
  return CHM_OK;
}

extern "C" int chm_segment_mean(chm_batch* b, int pairs, const float* msg, int64_t msg_count, float* agg,
                                int64_t agg_count, void* stream) {
  if (!b || !msg || !agg) return fail(CHM_E_ARG, "NULL argument");
  if (pairs < 1) return fail(CHM_E_ARG, "pairs must be >= 1");
  if (b->knn) return fail(CHM_E_UNSUPPORTED, "segment_mean: the fc edge layout only (knn edges change per call)");
  const long H_ = b->m->d.hidden_dim;
  if (msg_count != (int64_t)pairs * b->E * H_)
    return fail(CHM_E_ARG, "msg: " + std::to_string(msg_count) + " elements, pairs x E x hidden_dim = " +
                               std::to_string((int64_t)pairs * b->E * H_));
  if (agg_count != (int64_t)pairs * b->N * H_)
    return fail(CHM_E_ARG, "agg: " + std::to_string(agg_count) + " elements, pairs x N x hidden_dim = " +
                               std::to_string((int64_t)pairs * b->N * H_));
  HIPCHK(segment_mean(msg, agg, b->n2g, b->node_off, b->edge_off, b->natoms, b->N, b->E, pairs, (hipStream_t)stream));
  return CHM_OK;
}

extern "C" int chm_edge_features(chm_batch* b, const float* x, float* feat, void* stream) {
  if (!b || !x || !feat) return fail(CHM_E_ARG, "NULL argument");
  HIPCHK(fourier(x, b->ei, b->ej, b->E, feat, (hipStream_t)stream));
  return CHM_OK;
}

extern "C" int chm_knn_edges(chm_batch* b, const float* x, const float* lat, int32_t* src, int32_t* dst, float* fd,
                             int64_t capacity, int64_t* n_edges, void* stream) {
  if (!b || !x || !lat || !n_edges) return fail(CHM_E_ARG, "NULL argument");
  if (!b->knn) return fail(CHM_E_ARG, "not a knn batch");
  hipStream_t s = (hipStream_t)stream;
  int rc = knn_build(b, x, lat, s);
  if (rc) return rc;
  *n_edges = b->E;
  if (b->E > capacity) return CHM_OK;
  if (src) HIPCHK(hipMemcpyAsync(src, b->ei, b->E * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (dst) HIPCHK(hipMemcpyAsync(dst, b->ej, b->E * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (fd) HIPCHK(hipMemcpyAsync(fd, b->fd, b->E * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  return CHM_OK;
}

extern "C" int chm_edge_features_split(chm_batch* b, const float* x, void* split, void* stream) {
  if (!b || !x || !split) return fail(CHM_E_ARG, "NULL argument");
  // (knn batches: the features of the graph built by the last decoder call / chm_knn_edges)
  HIPCHK(fourier_h(x, b->ei, b->ej, b->E, split, (hipStream_t)stream, b->knn ? b->fd : nullptr));
  return CHM_OK;
}
