// Internal declarations shared by the host units of the C ABI (include/chemeleon_hip.h): the error plumbing of
// every unit with entry points, and the types and functions model.hip, batch.hip, decoder.hip, step.hip and
// debug_hooks.hip share. The kernel-facing declarations are chm_internal.h's.
//
// chm_model  : packed device copy of the CSPNet decoder weights.
// chm_batch  : one (ragged) batch of crystals: index tables of the implicit
//              fully connected edge layout + the decoder workspace, all
//              allocated once at creation. Decoder calls and sampler steps
//              allocate nothing, synchronise nothing and are capturable.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/chemeleon_hip.h"
#include "chm_internal.h"

namespace chm {

// sets the calling thread's chm_last_error() string (model.hip) and returns code
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return chm::fail(CHM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

struct LayerW {
  const float *WAB, *Wcl, *b1, *D, *W2, *b2, *W3, *b3, *W4, *b4, *lw, *lb;
  const void *WAB3, *D3, *W23, *W33, *W43;  // bf16 hi/mid/lo planes of the GEMM weights
  void* D2h;                                 // fp16 hi/lo split rows of the edge-GEMM weights (row-scaled)
  void* W22h16;                              // W2's split rows with k_edge16's K permutation (perm 2)
  float *Dsc, *W2sc;                         // their per-row power-of-two scales
  void *WAB16, *W316, *W416;                 // split16 node GEMMs: fp16 hi/lo rows, 16-column chunks
  float *WABsc, *W3sc, *W4sc;                // (row-scaled like D2h)
};

enum MathMode { MATH_BF16X3 = 0, MATH_F32 = 1, MATH_SPLIT16 = 2 };
constexpr long kTileRows = 256;  // rows of the edge-GEMM tiles (gemm_bf16x3_big)
// both edge layers in one grid (the pair grid) only from 256 row tiles (32 per XCD) on: at 64x20 (100 row tiles,
// 12-13 per XCD) each XCD's job list is too short to pack (edge_block)
constexpr long kLayerMinTiles = 256;
constexpr int kMaxLag = 1000;  // edge_lag's upper bound (the pair plan's layer-2 lag, in pair tiles)

}  // namespace chm

struct chm_model {
  chm_dims d;
  float* mem = nullptr;
  size_t mem_floats = 0;
  const float *emb, *Wc, *bc, *Wp, *bp, *fw, *fb, *Whead, *bhead, *Wlat, *flw, *flb;
  const void *Wc3, *Wp3, *Whead3;
  void* mem3 = nullptr;  // bf16 planes arena
  void* mem2 = nullptr;  // fp16 planes + scales arena
  void* mem16 = nullptr; // split16 node-GEMM weights arena
  const void* Wp16 = nullptr;
  float* Wpsc = nullptr;
  int math = chm::MATH_SPLIT16;
  int edge_dbg = 0;      // CHM_EDGE_DBG: edge-GEMM ablations for profiling only (wrong results)
  int node_glds = 1;     // CHM_NODE_GLDS=0: node GEMMs on the register-staged k_gemm3 (bit-identical, 2-3% slower)
  int node16 = 1;        // CHM_NODE16=0: split16 mode keeps its node GEMMs on bf16x3
  int node_ps = 0;       // CHM_NODE_PS=1: split16 node GEMMs read their A operands pre-split by the producing
                         // kernels instead of splitting them in the K loop (r4; measured 0.5% slower per step,
                         // DESIGN.md §4 "Node GEMMs")
  int edge_stagger = 0;  // CHM_EDGE_STAGGER: first-round start delay of every other CU (edge16.hip)
  int edge_rows = 1;     // CHM_EDGE_ROWS=0: edge layer 2 on node-aligned segment tiles instead of row tiles
  int edge_layer = 1;    // CHM_EDGE_LAYER=0: edge layers 1 and 2 as two launches (else one grid, k_edge16_pairs_grid)
  int edge_lag = 8;      // CHM_EDGE_LAG: its layer-2 lag behind layer 1, in pair tiles (r6: 8)
  long edge_layer_min = chm::kLayerMinTiles;  // CHM_EDGE_LAYER_MIN: row tiles from which the one-grid kernel runs
  int edge_pairs = 1;    // CHM_EDGE_PAIRS / option edge_pairs: fc edge layer 1 on unordered pairs (k_edge16_pairs:
                         // half its matrix work; both directions' S from one GEMM row), then edge layer 2
  int edge_pairs_layer = 1;  // CHM_EDGE_PAIRS_LAYER / option edge_pairs_layer: both edge layers on pairs in one
                             // static grid (k_edge16_pairs_grid) from edge_layer_min row tiles on; 0 = two launches
  int edge_rows_short = 1;   // CHM_EDGE_ROWS_SHORT / option edge_rows_short: batches below edge_layer_min row tiles whose
                             // last round of 256-row tiles is at most 3/4 full take that round as 192-row tiles
                             // (short_row_tiles, set at batch creation; bit-identical)
  int ncu = 0;          // compute units of the device the model lives on
  int device = 0;        // its HIP device ordinal (the current device at chm_model_create)
  unsigned xcd_mask = 0; // XCC ids a grid's blocks ran on at model creation (the pair grid needs 0xff)
  int repair_grid = 0;   // CHM_REPAIR_GRID: blocks of the edge kernels' repair launches (default: ncu)
  int film = 1;          // 0: time_dim = text_dim = 0 (no FilmLayer: the CrystalClip graph encoder)
  const char* edge_trace = nullptr;  // CHM_EDGE_TRACE=file: one edge-GEMM launch's block timeline
  int edge_trace_layer = 1;          // CHM_EDGE_TRACE_LAYER: 1 or 2 (two-launch schedule), 4 (pair grid)
  std::vector<chm::LayerW> layers;
};

struct chm_batch {
  const chm_model* m;
  int B, P;
  long N, E;
  std::vector<int> h_natoms;
  // index tables
  int *natoms, *node_off, *n2g, *ei, *ej;
  long *edge_off, *node_estart;
  int* node_n;  // atom count of each node's crystal
  // fc: the unordered pairs (i <= j) of every crystal for edge layer 1 on pairs (BatchTables::pi / pj / pe)
  int *pi = nullptr, *pj = nullptr;
  int2* pe = nullptr;
  int2* pnode = nullptr;  // per pair tile: the node range of its P / Q rows (EdgeArgs::pnode)
  long Ep = 0;
  // fc, split16: the job lists of both edge layers in one static grid on pairs (k_edge16_pairs_grid), built for
  // P = max_pairs and the model's edge_lag at creation; per layer 8 npx pair-tile flags (psched)
  chm::PairPlan pplan;
  int4* pjobs = nullptr;  // the pair grid's block records (PairSched::jobs)
  unsigned* psched = nullptr;
  int2* tiles;  // node ranges [x, y) whose edge rows fit one 256-row GEMM tile
  int ntiles;
  // fc batches: edge layer 2 (k_edge16) on row tiles of exactly 256 edge rows, nodes cut at the tile
  // ends (EdgeArgs::rtiles); null for knn batches
  int4* rtiles = nullptr;
  int2* rinfo = nullptr;    // per row tile: its node list (EdgeArgs::rinfo), and its length
  int* rinfo_n = nullptr;
  long nrt = 0, r2tot = 0;  // row tiles; rows of the nodes continued from a previous tile
  // a mixed row tiling (short_row_tiles): tiles [0, rt_nbig) have 256 rows, the rest kShortRows; -1 = all 256
  long rt_nbig = -1;
  float *sbuf = nullptr, *msgbuf = nullptr;
  unsigned* rcnt = nullptr;
  unsigned* xbad = nullptr;    // the pair grid: per layer, raised when its repair launches must run
  int math;     // arithmetic mode fixed at creation (copied from the model)
  // workspace
  float *cin, *cemb, *Hres, *Hl, *Y, *agg, *PQ, *gbias, *F, *S, *M, *Hf, *HO, *LAT;
  float* rmx;        // split16 node GEMMs: the four row-max arrays [4][P*N] (RMX_*)
  // split16 pre-split node GEMMs (node_ps): the node GEMMs' A operands as split rows [P*N][H/16][hi 16 | lo 16]
  // fp16 + per row the packed int8 exponents of its four 128-column chunks: the residual stream (FiLM
  // projection), the layer-normed rows (P / Q halves, node MLP 1), agg (node MLP 1), U (node MLP 2)
  void *Hs, *Hls, *aggs, *Us;
  int *He, *Hle, *agge, *Ue;
  unsigned* rowmax;  // split16: per S row, the packed int8 exponents of its four 128-column chunks, [P][E]
  void* owned = nullptr;  // the library's own allocation (chm_batch_create); null for caller workspaces
  size_t bytes = 0;
  // knn (radius-graph) batches: edges rebuilt every decoder call (knn.hip); E is then the current
  // graph's edge count and E_cap the capacity the edge buffers are sized for
  int knn = 0, knn_max_nb = 20;
  long E_cap = 0, C_cap = 0;
  long* cand_off = nullptr;
  unsigned *cand_key = nullptr, *cand2 = nullptr, *fin_key = nullptr;
  float *cand_d2 = nullptr, *fin_fd = nullptr, *fd = nullptr;
  int *atom_cnt = nullptr, *deg = nullptr, *cryst_fin = nullptr;
  std::vector<int> h_deg, h_fin;
  std::vector<long> h_estart;
  std::vector<int2> h_tiles;
};

namespace chm {

// Host-side index tables of a batch (batch.hip), before they are uploaded into a chm_batch
struct BatchTables {
  std::vector<int> nat, noff, n2g, ei, ej, nn;
  std::vector<long> eoff, estart, coff;
  std::vector<int2> tiles;
  std::vector<int4> rtiles;  // fc: row tiles of edge layer 2 (EdgeArgs::rtiles)
  std::vector<int2> rinfo;   // fc: the row tiles' node lists (EdgeArgs::rinfo, kRowInfo per tile)
  std::vector<int> rinfo_n;
  long nrt = 0, r2tot = 0;
  long rt_nbig = -1;  // fc: 256-row tiles before the kShortRows ones (-1: all 256 rows; set before batch_fill)
  long N = 0, E = 0;  // knn: E = the edge capacity
  // fc: the unordered pairs i <= j of every crystal, row-major (edge layer 1 on pairs, k_edge16_pairs)
  std::vector<int> pi, pj;
  std::vector<int2> pe, pnode;
  long Ep = 0;
  long C = 0;         // knn: candidate scratch entries (sum of n^2 * 27)
  bool knn = false;
};

// The schedule the edge layers of a decoder call with P conditionings take, from the model's options and the
// batch's tables (run_decoder and chm_debug_edge_layer decide it here, once per call).
struct EdgePlan {
  bool n16;        // split16 node GEMMs: row maxima of their A operands, written by the producing kernels
  bool ps;         // pre-split node GEMMs: the producers write the A operands split (no row-max atomics then)
  bool pairs;      // fc edge layer 1 on unordered pairs (option edge_pairs): F holds the pairs' features only
  bool pair_grid;  // both edge layers on pairs in one grid (k_edge16_pairs_grid) for this call
  bool zero_grid;  // the pair grid's repair requests and per-layer flags start clear in every call: zeroed by the
                   // embedding launch
};

// profiling (decoder.hip, chm_prof_*): a pair of events around the launches of a scope, while enabled
extern bool g_prof_on;
struct ProfScope {
  int id; hipStream_t s; hipEvent_t b = nullptr;
  ProfScope(int id_, hipStream_t s_);
  ~ProfScope() { if (b) (void)hipEventRecord(b, s); }
};

// decoder.hip: the pieces of a decoder call, for the entry points of step.hip and the test hooks of debug_hooks.hip
int knn_build(chm_batch* b, const float* x, const float* lat, hipStream_t s);
EdgePlan edge_plan(const chm_batch* b, int P);
int clear_edge_flags(chm_batch* b, const EdgePlan& ep, hipStream_t s, bool grid_too);
int edge_features(chm_batch* b, const EdgePlan& ep, const float* x, hipStream_t s);
int edge_block(chm_batch* b, int P, int l, const EdgePlan& ep, bool ps, hipStream_t s);
float* rmx_row(const chm_batch* b, const EdgePlan& ep, int k);
int node_cond_in(chm_batch* b, int P, const float* temb, int tstride, const int* d_t, const float* text0,
                 const float* text1, hipStream_t s);
int node_embed(chm_batch* b, const EdgePlan& ep, int P, const int64_t* a, const float* lat, hipStream_t s);
int node_graph_bias_rest(chm_batch* b, const float* lat, hipStream_t s);
int node_film_ln(chm_batch* b, const EdgePlan& ep, int P, int l, hipStream_t s);
int node_final_ln(chm_batch* b, int P, hipStream_t s);
int node_graph_heads(chm_batch* b, int P, const float* lat, hipStream_t s);
int node_split_heads(chm_batch* b, int P, float* types, float* coords, hipStream_t s);
int run_decoder(chm_batch* b, int P, const int64_t* a, const float* x, const float* lat, const float* temb,
                int tstride, const int* d_t, const float* text0, const float* text1, int heads, hipStream_t s,
                bool reuse_cond = false);

// step.hip: the argument checks and kernel arguments the update hooks of debug_hooks.hip share with the entry points
int check_step_io(const chm_batch* b, const chm_step_io* io, bool noise_required, bool noise_allowed,
                  bool text_required = true);
StepArgs step_args(const chm_batch* b, const chm_schedule* sc, int t, const int* d_t, float cond_scale,
                   const chm_step_io* io, uint64_t seed, int64_t node_base, int64_t graph_base);
TrainArgs train_args(const chm_batch* b, const chm_train_tables* tt, const int64_t* d_t, const int64_t* a0,
                     const float* x0, const float* l0, const float* rand_a, const float* noise_l,
                     const float* noise_x, float* out, int64_t* a_t, float* x_t, float* l_t, float* target_x);

}  // namespace chm
