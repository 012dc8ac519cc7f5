// The chm_debug_* test hooks that drive device work: single kernels and single pieces of a decoder call or a step on
// caller operands, for the kernel-unit test suites. Beyond the kernel launchers (chm_internal.h) a hook calls only
// what chm_host.h declares, the very functions run_decoder, sample_step and chm_training_loss run: none has a copy
// of its own. (The host-only plan queries are batch.hip's.)
#include <cmath>

#include "chm_host.h"

using namespace chm;

// One GEMM kernel on caller operands (tests/test_gpu_gemm.py). Every argument check runs before the first HIP
// call, so a refused call needs no device.
extern "C" int chm_debug_gemm(const chm_debug_gemm_args* a, void* stream) {
  if (!a) return fail(CHM_E_ARG, "args is NULL");
  const int kind = a->kind;
  auto bad = [&](const char* field, const std::string& why) {
    return fail(CHM_E_ARG, std::string("chm_debug_gemm (kind ") + std::to_string(kind) + "): " + field + " " + why);
  };
  if (kind < 0 || kind > 5) return bad("kind", "must be in [0, 5]");
  const bool node = kind == 3 || kind == 4, edge = kind == 5;
  if (a->M < 1 || a->M > (1L << 24)) return bad("M", "must be in [1, 2^24]");
  if (a->N < 1 || a->K < 1) return bad(a->N < 1 ? "N" : "K", "must be positive");
  if (!a->d_A) return bad("d_A", "is NULL");
  if (!a->d_W) return bad("d_W", "is NULL");
  if (!a->d_C) return bad("d_C", "is NULL");
  if (a->act != 0 && a->act != 1) return bad("act", "must be 0 or 1");
  const int nmult = (kind == 2 || edge) ? 256 : 128;
  if (a->N % nmult) return bad("N", "must be a multiple of " + std::to_string(nmult));
  const int kmult = edge ? 64 : (kind == 0 || kind == 2) ? 16 : 32;
  if (a->K % kmult) return bad("K", "must be a multiple of " + std::to_string(kmult));
  int ksplit = a->ksplit;
  if (!a->d_A2) {
    if (ksplit != 0 && ksplit != a->K) return bad("ksplit", "must be 0 or K without d_A2");
    ksplit = a->K;
  } else {
    if (edge) return bad("d_A2", "is not taken by the edge GEMM");
    if (ksplit < 16 || ksplit >= a->K || ksplit % 16) return bad("ksplit", "must be a multiple of 16 in (0, K)");
    if (a->lda2 < a->K - ksplit || a->lda2 % 4) return bad("lda2", "must be >= K - ksplit and a multiple of 4");
  }
  if (a->lda < ksplit || a->lda % 4) return bad("lda", "must cover the row and be a multiple of 4");
  if (a->ldc < a->N || a->ldc % 4) return bad("ldc", "must be >= N and a multiple of 4");
  if (a->d_R && (a->ldr < a->N || a->ldr % 4)) return bad("ldr", "must be >= N and a multiple of 4");
  if (a->d_gb) {
    if (kind == 2) return bad("d_gb", "is not taken by gemm_bf16x3_big");
    if (!a->d_row2g) return bad("d_row2g", "is NULL");
    if (a->gb_rowmod < 1) return bad("gb_rowmod", "must be >= 1");
    if (a->gb_cols < 4 || a->gb_cols > a->N || a->gb_cols % 4) return bad("gb_cols", "must be a multiple of 4 in (0, N]");
    if (a->ldgb < a->gb_cols || a->ldgb % 4) return bad("ldgb", "must be >= gb_cols and a multiple of 4");
  }
  if (edge && (a->d_bias || a->act || a->d_R || a->d_gb))
    return bad(a->d_bias ? "d_bias" : a->act ? "act" : a->d_R ? "d_R" : "d_gb", "is not taken by the edge GEMM's plain epilogue");
  if (a->chunk_scaled != 0 && a->chunk_scaled != 1) return bad("chunk_scaled", "must be 0 or 1");
  if (a->chunk_scaled && !edge) return bad("chunk_scaled", "is an option of kind 5");
  if (a->chunk_scaled && (a->K % 128 || a->K > 512)) return bad("chunk_scaled", "needs K % 128 == 0 and K <= 512");
  if (a->d_cmax && kind != 4) return bad("d_cmax", "is written by kind 4 only");
  const int tr = a->tile_rows, tc = a->tile_cols, nb = a->blocks_per_cu;
  if (!node && (tr || tc || nb)) return bad(tr ? "tile_rows" : tc ? "tile_cols" : "blocks_per_cu", "is an option of kinds 3 and 4");
  if (tr != 0 && tr != 64 && tr != 128) return bad("tile_rows", "must be 0, 64 or 128");
  if (kind == 3) {
    if (tc != 0 && tc != 128) return bad("tile_cols", "must be 0 or 128 (bf16x3 tiles have 128 columns)");
    if (nb != 0 && nb != 2) return bad("blocks_per_cu", "must be 0 or 2 (bf16x3 tiles run two blocks per CU)");
  } else if (kind == 4) {
    if (tc != 0 && tc != 64 && tc != 128) return bad("tile_cols", "must be 0, 64 or 128");
    if (tc == 64 && tr != 64) return bad("tile_cols", "64 needs tile_rows 64");
    if (nb != 0 && (nb < 2 || nb > 4)) return bad("blocks_per_cu", "must be 0, 2, 3 or 4");
    if (nb && !tr) return bad("blocks_per_cu", "needs tile_rows");
    if (tr == 64 && tc == 64 && nb != 0 && nb != 4) return bad("blocks_per_cu", "must be 0 or 4 on 64x64 tiles");
    if (tr == 64 && tc == 128 && nb == 2) return bad("blocks_per_cu", "must be 0, 3 or 4 on 64-row tiles");
    if (tr == 64 && tc == 0 && nb) return bad("blocks_per_cu", "needs tile_cols on 64-row tiles");
    if (tr == 128 && nb == 4) return bad("blocks_per_cu", "must be 0, 2 or 3 on 128-row tiles");
  }
  for (const void* p : {(const void*)a->d_A, (const void*)a->d_A2, (const void*)a->d_W, (const void*)a->d_bias,
                        (const void*)a->d_R, (const void*)a->d_gb, (const void*)a->d_C})
    if ((uintptr_t)p % 16) return bad("operands", "must be 16-byte aligned");

  hipStream_t s = (hipStream_t)stream;
  const long M = a->M;
  const int N = a->N, K = a->K;
  void* mem = nullptr;  // the packed weights (+ row scales), and kind 5's split A rows (+ chunk exponents)
  const size_t wbytes = ((kind >= 1 && kind <= 3 ? (size_t)3 * N * K * 2 : kind >= 4 ? (size_t)N * K * 4 : 0) + 255) / 256 * 256;
  const size_t scbytes = ((size_t)N * 4 + 255) / 256 * 256;
  const size_t abytes = edge ? (size_t)(M + 256) * K * 4 : 0, ebytes = edge ? ((size_t)M * 4 + 255) / 256 * 256 : 0;
  if (kind != 0) HIPCHK(hipMalloc(&mem, wbytes + scbytes + abytes + ebytes));
  char* base = (char*)mem;
  float* wsc = (float*)(base + wbytes);
  char* As = base + wbytes + scbytes;
  int* aexp = (int*)(As + abytes);
  auto done = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (mem) (void)hipFree(mem);
    return e == hipSuccess ? CHM_OK : fail(CHM_E_HIP, std::string("chm_debug_gemm: ") + what + ": " + hipGetErrorString(e));
  };
  hipError_t e = hipSuccess;
  if (kind >= 1 && kind <= 3) e = split_planes(a->d_W, (long)N * K, base, s);
  if (kind == 4) e = split_rows_h(a->d_W, N, K, base, wsc, 0, s, 16);
  if (edge) e = split_rows_h(a->d_W, N, K, base, wsc, 0, s);
  if (e != hipSuccess) return done(e, "weight packing");

  if (edge) {
    // A as split rows [K/32][hi 32 | lo 32] (edge16.hip): unscaled like the Fourier features, or per (row, 128-column
    // chunk) scaled by 2^-e, e the exponent of the chunk's maximum, like S; 256 readable rows behind the last (NaN:
    // the kernel reads them for a partial tile and must store nothing of them)
    std::vector<float> hA((size_t)M * K);
    e = hipMemcpy2DAsync(hA.data(), (size_t)K * 4, a->d_A, (size_t)a->lda * 4, (size_t)K * 4, M, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return done(e, "A download");
    std::vector<uint16_t> hs((size_t)(M + 256) * K * 2, (uint16_t)0x7e00);
    std::vector<int> he(M, 0);
    for (long r = 0; r < M; ++r) {
      const float* x = hA.data() + (size_t)r * K;
      _Float16* o = reinterpret_cast<_Float16*>(hs.data()) + (size_t)r * 2 * K;
      for (int c0 = 0; c0 < K; c0 += 128) {
        const int cn = K - c0 < 128 ? K - c0 : 128;
        int ex = 0;
        if (a->chunk_scaled) {
          float m = 0.f;
          for (int k = c0; k < c0 + cn; ++k) m = fmaxf(m, fabsf(x[k]));
          if (m > 0.f) frexpf(m, &ex);
          ex = ex < -126 ? -126 : ex > 127 ? 127 : ex;
          he[r] |= (ex & 0xff) << (8 * (c0 / 128));
        }
        const float sc = ldexpf(1.0f, -ex);
        for (int k = c0; k < c0 + cn; ++k) {
          const float v = x[k] * sc;
          const _Float16 hi = (_Float16)v;
          o[(k / 32) * 64 + k % 32] = hi;
          o[(k / 32) * 64 + 32 + k % 32] = (_Float16)(v - (float)hi);
        }
      }
    }
    e = hipMemcpyAsync(As, hs.data(), abytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(aexp, he.data(), (size_t)M * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the host vectors go out of scope)
    if (e != hipSuccess) return done(e, "A upload");
    EdgeArgs g{};
    g.M = M; g.N = N; g.K = K; g.A = As; g.aexp = a->chunk_scaled ? aexp : nullptr;
    g.W = base; g.wscale = wsc; g.C = a->d_C; g.ldc = a->ldc;
    return done(edge_gemm16(g, EPI_STD, s), "edge_gemm16");
  }

  GemmArgs g{};
  g.M = M; g.N = N; g.K = K;
  g.A = a->d_A; g.lda = a->lda;
  g.A2 = a->d_A2 ? a->d_A2 : a->d_A; g.lda2 = a->d_A2 ? a->lda2 : a->lda; g.ksplit = ksplit;
  g.W = a->d_W; g.ldw = K;
  g.C = a->d_C; g.ldc = a->ldc;
  g.bias = a->d_bias; g.act = a->act;
  g.R = a->d_R; g.ldr = a->ldr;
  g.gb = a->d_gb; g.ldgb = a->ldgb; g.gb_cols = a->gb_cols; g.row2g = a->d_row2g; g.gb_rowmod = a->d_gb ? a->gb_rowmod : 1;
  if (kind != 0) g.Wp3 = base;
  if (kind == 4) {
    g.wscale = wsc;
    g.amax = a->d_amax; g.amax2 = a->d_amax ? a->d_amax2 : nullptr; g.cmax = a->d_cmax;
  }
  if (kind == 0) return done(gemm(g, EPI_STD, s), "gemm");
  if (kind == 1) return done(gemm_bf16x3(g, EPI_STD, s), "gemm_bf16x3");
  if (kind == 2) return done(gemm_bf16x3_big(g, EPI_STD, s), "gemm_bf16x3_big");
  const int r0 = g_node_rows, c0 = g_node_cols, b0 = g_node_blocks;
  g_node_rows = tr; g_node_cols = tc; g_node_blocks = nb;
  e = node_gemm(g, s);
  g_node_rows = r0; g_node_cols = c0; g_node_blocks = b0;
  return done(e, "node_gemm");
}

// The argument checks of chm_debug_edge_layer (knn = false; d_agg_split / d_agg_exp are its own) and
// chm_debug_knn_edge_layer (knn = true; d_lat / n_lat are its own), refused under the hook's name: the
// batch-independent ones first, none touches HIP.
static int check_edge_layer_args(const char* hook, bool knn, const chm_batch* b, int pairs, int layer,
                                 const float* d_frac, int64_t n_frac, const float* d_lat, int64_t n_lat,
                                 const float* d_PQ, int64_t n_pq, const float* d_agg, int64_t n_agg,
                                 const void* d_agg_split, const void* d_agg_exp) {
  auto bad = [&](const char* field, const std::string& why) {
    return fail(CHM_E_ARG, std::string(hook) + ": " + field + " " + why);
  };
  if (!d_frac) return bad("d_frac", "is NULL");
  if (knn && !d_lat) return bad("d_lat", "is NULL");
  if (!d_PQ) return bad("d_PQ", "is NULL");
  if (!d_agg) return bad("d_agg", "is NULL");
  if ((d_agg_split == nullptr) != (d_agg_exp == nullptr))
    return bad(d_agg_split ? "d_agg_exp" : "d_agg_split", "is NULL (the split rows and their exponents go together)");
  if (pairs < 1) return bad("pairs", "must be in [1, max_pairs]");
  if (layer < 0) return bad("layer", "must be in [0, num_layers)");
  if (n_frac < 3 || n_frac % 3) return bad("n_frac", "must be 3 N, N >= 1");
  if (knn && (n_lat < 9 || n_lat % 9)) return bad("n_lat", "must be 9 B, B >= 1");
  const int64_t Nc = n_frac / 3;
  if (n_pq != (int64_t)pairs * Nc * 2 * H)
    return bad("n_pq", "is " + std::to_string(n_pq) + ", [pairs, N, 2H] has " + std::to_string((int64_t)pairs * Nc * 2 * H));
  if (n_agg != (int64_t)pairs * Nc * H)
    return bad("n_agg", "is " + std::to_string(n_agg) + ", [pairs, N, H] has " + std::to_string((int64_t)pairs * Nc * H));
  for (const void* p : {(const void*)d_frac, (const void*)d_lat, (const void*)d_PQ, (const void*)d_agg, d_agg_split,
                        d_agg_exp})
    if ((uintptr_t)p % 16) return bad("operands", "must be 16-byte aligned");
  if (!b) return bad("batch", "is NULL");
  const chm_model* m = b->m;
  if ((b->knn != 0) != knn)
    return fail(CHM_E_UNSUPPORTED, std::string(hook) + (knn ? ": batch is an fc batch (knn batches only)"
                                                            : ": batch is a knn batch (fc batches only)"));
  if (Nc != b->N) return bad("n_frac", "is " + std::to_string(n_frac) + ", the batch needs " + std::to_string(3 * b->N));
  if (knn && n_lat != (int64_t)9 * b->B)
    return bad("n_lat", "is " + std::to_string(n_lat) + ", the batch needs " + std::to_string(9 * (int64_t)b->B));
  if (pairs > b->P) return bad("pairs", "must be in [1, max_pairs]");
  if (layer >= m->d.num_layers) return bad("layer", "must be in [0, num_layers)");
  return CHM_OK;
}

// The message path of one CSP layer (edge_block, the code run_decoder runs, on the schedule the model's options and the
// batch give it) on caller operands (tests/test_gpu_edge_layer.py). Every argument check runs before the first HIP
// call, the batch-independent ones first, so a refused call needs no device.
extern "C" int chm_debug_edge_layer(chm_batch* b, int pairs, int layer, const float* d_frac, int64_t n_frac,
                                    const float* d_PQ, int64_t n_pq, float* d_agg, int64_t n_agg, void* d_agg_split,
                                    int32_t* d_agg_exp, void* stream) {
  if (const int rc = check_edge_layer_args("chm_debug_edge_layer", false, b, pairs, layer, d_frac, n_frac, nullptr, 0,
                                           d_PQ, n_pq, d_agg, n_agg, d_agg_split, d_agg_exp))
    return rc;
  const long N = b->N;
  const EdgePlan ep = edge_plan(b, pairs);
  if (d_agg_split && !ep.ps)
    return fail(CHM_E_UNSUPPORTED, "chm_debug_edge_layer: d_agg_split needs a split16 batch created with option node_ps");

  hipStream_t s = (hipStream_t)stream;
  auto run = [&](bool ps) -> int {
    if (const int rc = clear_edge_flags(b, ep, s, true)) return rc;
    if (ep.n16 && !ps)  // (film_ln zeroes agg's row maxima for the layer's atomic maxima)
      HIPCHK(hipMemsetAsync(b->rmx + RMX_AGG * (long)b->P * N, 0, (size_t)b->P * N * sizeof(float), s));
    return edge_block(b, pairs, layer, ep, ps, s);
  };
  if (const int rc = edge_features(b, ep, d_frac, s)) return rc;
  HIPCHK(hipMemcpyAsync(b->PQ, d_PQ, (size_t)n_pq * sizeof(float), hipMemcpyDeviceToDevice, s));
  // fp32 agg: the block without pre-split (a pre-split batch writes agg only as split rows: the block runs once more)
  if (const int rc = run(false)) return rc;
  HIPCHK(hipMemcpyAsync(d_agg, b->agg, (size_t)n_agg * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (d_agg_split) {
    if (const int rc = run(true)) return rc;
    HIPCHK(hipMemcpyAsync(d_agg_split, b->aggs, (size_t)pairs * N * H * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(d_agg_exp, b->agge, (size_t)pairs * N * sizeof(int), hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return CHM_OK;
}

// The same for knn batches (tests/test_gpu_knn_kernels.py): the radius graph of the caller's coordinates and lattices
// (knn_build), then edge_features and edge_block on it as run_decoder runs them. Every argument check runs before the
// first HIP call, the batch-independent ones first. knn_build's own refusals (a node above 256 edges, a graph above
// the batch capacity) are returned as they are: they are decided on the host before anything is placed.
extern "C" int chm_debug_knn_edge_layer(chm_batch* b, int pairs, int layer, const float* d_frac, int64_t n_frac,
                                        const float* d_lat, int64_t n_lat, const float* d_PQ, int64_t n_pq, float* d_agg,
                                        int64_t n_agg, void* stream) {
  if (const int rc = check_edge_layer_args("chm_debug_knn_edge_layer", true, b, pairs, layer, d_frac, n_frac, d_lat,
                                           n_lat, d_PQ, n_pq, d_agg, n_agg, nullptr, nullptr))
    return rc;

  hipStream_t s = (hipStream_t)stream;
  if (const int rc = knn_build(b, d_frac, d_lat, s)) return rc;
  const long N = b->N;
  const EdgePlan ep = edge_plan(b, pairs);  // (after knn_build: the plan reads the call's E)
  if (const int rc = edge_features(b, ep, d_frac, s)) return rc;
  HIPCHK(hipMemcpyAsync(b->PQ, d_PQ, (size_t)n_pq * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (const int rc = clear_edge_flags(b, ep, s, true)) return rc;
  if (ep.n16)  // (film_ln zeroes agg's row maxima for the layer's atomic maxima)
    HIPCHK(hipMemsetAsync(b->rmx + RMX_AGG * (long)b->P * N, 0, (size_t)b->P * N * sizeof(float), s));
  if (const int rc = edge_block(b, pairs, layer, ep, false, s)) return rc;
  HIPCHK(hipMemcpyAsync(d_agg, b->agg, (size_t)n_agg * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return CHM_OK;
}

// The words the embedding launch clears on a pair-grid plan, as chm_debug_node_stage's d_flags holds them: xbad
// [2 kMaxLayers], then the pair grid's per-layer flags [L 8 npx], then the unused words up to the end of that
// buffer's 256-byte-rounded allocation (the guard: no launch may write them). 0: the plan clears nothing.
static long node_flag_words(const chm_batch* b, const EdgePlan& ep, long* n_psched) {
  if (!ep.zero_grid) return 0;
  const long np = (long)b->m->d.num_layers * 8 * b->pplan.npx;
  if (n_psched) *n_psched = np;
  return 2L * kMaxLayers + (np + 63) / 64 * 64;
}
extern "C" int64_t chm_debug_node_flag_words(const chm_batch* b, int pairs, int64_t* n_cleared) {
  if (!b) return fail(CHM_E_ARG, "chm_debug_node_flag_words: batch is NULL");
  if (pairs < 1 || pairs > b->P) return fail(CHM_E_ARG, "chm_debug_node_flag_words: pairs must be in [1, max_pairs]");
  long np = 0;
  const long n = node_flag_words(b, edge_plan(b, pairs), &np);
  if (n_cleared) *n_cleared = n ? 2L * kMaxLayers + np : 0;
  return n;
}

// The decoder's node-side launches alone (the node_* functions run_decoder calls, on the plan a decoder call with
// `pairs` conditionings on this batch takes) on caller operands (tests/test_gpu_node_kernels.py). Every argument
// check runs before the first HIP call, the batch-independent ones first, so a refused call needs no device. The
// batch buffers a stage writes are filled with 0xff bytes (NaNs) first: an output the launch left out shows.
extern "C" int chm_debug_node_stage(chm_batch* b, int pairs, int stage, int layer, const chm_debug_node_io* io,
                                    void* stream) {
  auto bad = [&](const char* field, const std::string& why) {
    return fail(CHM_E_ARG, std::string("chm_debug_node_stage (stage ") + std::to_string(stage) + "): " + field + " " + why);
  };
  auto unsupported = [&](const std::string& why) {
    return fail(CHM_E_UNSUPPORTED, std::string("chm_debug_node_stage (stage ") + std::to_string(stage) + "): " + why);
  };
  if (!io) return bad("io", "is NULL");
  if (stage < 1 || stage > 4) return bad("stage", "must be in [1, 4]");
  if (pairs < 1) return bad("pairs", "must be in [1, max_pairs]");
  if (stage == 3 && layer < 0) return bad("layer", "must be in [0, num_layers)");
  // the pointers each stage needs whatever the batch is
  if (stage == 1) {
    if (!io->d_temb) return bad("d_temb", "is NULL");
    if (!io->d_cin) return bad("d_cin", "is NULL");
    if (!io->d_t && io->tstride < 0) return bad("tstride", "must be >= 0");
  } else if (stage == 2) {
    if (!io->d_a) return bad("d_a", "is NULL");
    if (!io->d_lat) return bad("d_lat", "is NULL");
    if (!io->d_Hres) return bad("d_Hres", "is NULL");
    if (!io->d_gbias) return bad("d_gbias", "is NULL");
  } else if (stage == 3) {
    if (!io->d_Hres) return bad("d_Hres", "is NULL");
    if (!io->d_Hl) return bad("d_Hl", "is NULL");
  } else {
    if (!io->d_Hres) return bad("d_Hres", "is NULL");
    if (!io->d_lat) return bad("d_lat", "is NULL");
    if (!io->d_HO) return bad("d_HO", "is NULL");
    if (!io->d_Hf) return bad("d_Hf", "is NULL");
    if (!io->d_LAT) return bad("d_LAT", "is NULL");
  }
  if (stage == 2 || stage == 3)
    if ((io->d_split == nullptr) != (io->d_exp == nullptr))
      return bad(io->d_split ? "d_exp" : "d_split", "is NULL (the split rows and their exponents go together)");
  if (!b) return bad("batch", "is NULL");
  const chm_model* m = b->m;
  if (pairs > b->P) return bad("pairs", "must be in [1, max_pairs]");
  const int L = m->d.num_layers, X = m->d.text_dim, B = b->B, A = m->d.max_atoms;
  if (stage == 3 && layer >= L) return bad("layer", "must be in [0, num_layers)");
  const long N = b->N, R = (long)pairs * N, RS = (long)b->P * N;
  const EdgePlan ep = edge_plan(b, pairs);
  auto sized = [&](const void* p, int64_t n, long expect, const char* name, const char* shape) -> int {
    if (p && n != expect)
      return bad(name, "has " + std::to_string(n) + " elements, " + shape + " needs " + std::to_string(expect));
    return CHM_OK;
  };
  int rc;
  long n_flags = 0;
  if (stage == 1) {
    if (!m->film) return unsupported("the model has no FilmLayer (time_dim = text_dim = 0): no conditioning input");
    if (io->d_t) {
      if (io->n_t != 1) return bad("n_t", "must be 1 (one device int32)");
      if (io->n_temb < TD || io->n_temb % TD) return bad("n_temb", "must be rows of time_dim = 128 (a table indexed by *d_t)");
    } else if ((rc = sized(io->d_temb, io->n_temb, (long)(B - 1) * io->tstride + TD, "n_temb", "[B] rows tstride apart")))
      return rc;
    if (X > 0 && !io->d_text0) return bad("d_text0", "is NULL (text_dim > 0)");
    if (X > 0 && pairs > 1 && !io->d_text1) return bad("d_text1", "is NULL (text_dim > 0, pairs = 2)");
    if ((rc = sized(io->d_text0, io->n_text0, (long)B * X, "n_text0", "[B,text_dim]"))) return rc;
    if ((rc = sized(io->d_text1, io->n_text1, (long)B * X, "n_text1", "[B,text_dim]"))) return rc;
    if ((rc = sized(io->d_cin, io->n_cin, (long)pairs * B * (TD + X), "n_cin", "[pairs,B,time_dim+text_dim]"))) return rc;
  } else if (stage == 2) {
    if ((rc = sized(io->d_a, io->n_a, N, "n_a", "[N]"))) return rc;
    if ((rc = sized(io->d_lat, io->n_lat, (long)B * 9, "n_lat", "[B,3,3]"))) return rc;
    if ((rc = sized(io->d_Hres, io->n_Hres, R * H, "n_Hres", "[pairs,N,H]"))) return rc;
    if ((rc = sized(io->d_gbias, io->n_gbias, (long)L * B * H, "n_gbias", "[L,B,H]"))) return rc;
    if (io->d_rmax && !rmx_row(b, ep, RMX_H)) return bad("d_rmax", "is not written on this plan (split16 without node_ps only)");
    if ((rc = sized(io->d_rmax, io->n_rmax, R, "n_rmax", "[pairs N]"))) return rc;
    if (io->d_split && !ep.ps) return bad("d_split", "is not written on this plan (split16 with node_ps only)");
    if ((rc = sized(io->d_split, io->n_split, R * 2 * H, "n_split", "[pairs N][H/16][hi 16 | lo 16]"))) return rc;
    if ((rc = sized(io->d_exp, io->n_exp, R, "n_exp", "[pairs N]"))) return rc;
    n_flags = node_flag_words(b, ep, nullptr);
    if (io->d_flags && !n_flags) return bad("d_flags", "is not written on this plan (the pair grid only)");
    if ((rc = sized(io->d_flags, io->n_flags, n_flags, "n_flags", "chm_debug_node_flag_words"))) return rc;
  } else if (stage == 3) {
    if (m->film && !io->d_Y) return bad("d_Y", "is NULL (the model has a FilmLayer)");
    if (m->film && !io->d_cemb) return bad("d_cemb", "is NULL (the model has a FilmLayer)");
    if ((rc = sized(io->d_Y, io->n_Y, R * H, "n_Y", "[pairs,N,H]"))) return rc;
    if ((rc = sized(io->d_cemb, io->n_cemb, (long)pairs * B * 2 * H, "n_cemb", "[pairs,B,2H]"))) return rc;
    if ((rc = sized(io->d_Hres, io->n_Hres, R * H, "n_Hres", "[pairs,N,H]"))) return rc;
    if ((rc = sized(io->d_Hl, io->n_Hl, R * H, "n_Hl", "[pairs,N,H]"))) return rc;
    if (io->d_rmax && !rmx_row(b, ep, 0)) return bad("d_rmax", "is not written on this plan (split16 without node_ps only)");
    if ((rc = sized(io->d_rmax, io->n_rmax, 4 * R, "n_rmax", "[4][pairs N]"))) return rc;
    if (io->d_split && !ep.ps) return bad("d_split", "is not written on this plan (split16 with node_ps only)");
    if ((rc = sized(io->d_split, io->n_split, R * 2 * H, "n_split", "[pairs N][H/16][hi 16 | lo 16]"))) return rc;
    if ((rc = sized(io->d_exp, io->n_exp, R, "n_exp", "[pairs N]"))) return rc;
  } else {
    if ((rc = sized(io->d_Hres, io->n_Hres, R * H, "n_Hres", "[pairs,N,H]"))) return rc;
    if ((rc = sized(io->d_lat, io->n_lat, (long)B * 9, "n_lat", "[B,3,3]"))) return rc;
    if ((rc = sized(io->d_HO, io->n_HO, R * HEADS_N, "n_HO", "[pairs N,128]"))) return rc;
    if ((rc = sized(io->d_Hf, io->n_Hf, R * H, "n_Hf", "[pairs,N,H]"))) return rc;
    if ((rc = sized(io->d_LAT, io->n_LAT, (long)pairs * B * 9, "n_LAT", "[pairs,B,3,3]"))) return rc;
    if ((rc = sized(io->d_types, io->n_types, R * A, "n_types", "[pairs,N,max_atoms]"))) return rc;
    if ((rc = sized(io->d_coords, io->n_coords, R * 3, "n_coords", "[pairs,N,3]"))) return rc;
  }

  hipStream_t s = (hipStream_t)stream;
  const auto D2D = hipMemcpyDeviceToDevice;
  const size_t f4 = sizeof(float);
  if (stage == 1) {
    HIPCHK(hipMemsetAsync(b->cin, 0xff, (size_t)b->P * B * (TD + X) * f4, s));
    if ((rc = node_cond_in(b, pairs, io->d_temb, io->d_t ? 0 : io->tstride, io->d_t, io->d_text0, io->d_text1, s))) return rc;
    HIPCHK(hipMemcpyAsync(io->d_cin, b->cin, (size_t)io->n_cin * f4, D2D, s));
  } else if (stage == 2) {
    HIPCHK(hipMemsetAsync(b->Hres, 0xff, (size_t)RS * H * f4, s));
    HIPCHK(hipMemsetAsync(b->gbias, 0xff, (size_t)L * B * H * f4, s));
    HIPCHK(hipMemsetAsync(b->rmx, 0xff, (size_t)4 * RS * f4, s));
    if (ep.ps) {
      HIPCHK(hipMemsetAsync(b->Hs, 0xff, (size_t)RS * H * 4, s));
      HIPCHK(hipMemsetAsync(b->He, 0xff, (size_t)RS * sizeof(int), s));
    }
    const long nx = 2L * kMaxLayers;
    if (io->d_flags) {
      HIPCHK(hipMemcpyAsync(b->xbad, io->d_flags, nx * sizeof(unsigned), D2D, s));
      HIPCHK(hipMemcpyAsync(b->psched, io->d_flags + nx, (n_flags - nx) * sizeof(unsigned), D2D, s));
    }
    if ((rc = node_embed(b, ep, pairs, io->d_a, io->d_lat, s))) return rc;
    if ((rc = node_graph_bias_rest(b, io->d_lat, s))) return rc;
    HIPCHK(hipMemcpyAsync(io->d_Hres, b->Hres, (size_t)R * H * f4, D2D, s));
    HIPCHK(hipMemcpyAsync(io->d_gbias, b->gbias, (size_t)L * B * H * f4, D2D, s));
    if (io->d_rmax) HIPCHK(hipMemcpyAsync(io->d_rmax, rmx_row(b, ep, RMX_H), (size_t)R * f4, D2D, s));
    if (io->d_split) {
      HIPCHK(hipMemcpyAsync(io->d_split, b->Hs, (size_t)R * H * 4, D2D, s));
      HIPCHK(hipMemcpyAsync(io->d_exp, b->He, (size_t)R * sizeof(int), D2D, s));
    }
    if (io->d_flags) {
      HIPCHK(hipMemcpyAsync(io->d_flags, b->xbad, nx * sizeof(unsigned), D2D, s));
      HIPCHK(hipMemcpyAsync(io->d_flags + nx, b->psched, (n_flags - nx) * sizeof(unsigned), D2D, s));
    }
  } else if (stage == 3) {
    if (m->film) {
      HIPCHK(hipMemcpyAsync(b->Y, io->d_Y, (size_t)R * H * f4, D2D, s));
      HIPCHK(hipMemcpyAsync(b->cemb, io->d_cemb, (size_t)pairs * B * 2 * H * f4, D2D, s));
    }
    HIPCHK(hipMemcpyAsync(b->Hres, io->d_Hres, (size_t)R * H * f4, D2D, s));
    HIPCHK(hipMemsetAsync(b->Hl, 0xff, (size_t)RS * H * f4, s));
    HIPCHK(hipMemsetAsync(b->rmx, 0xff, (size_t)4 * RS * f4, s));
    if (ep.ps) {
      HIPCHK(hipMemsetAsync(b->Hls, 0xff, (size_t)RS * H * 4, s));
      HIPCHK(hipMemsetAsync(b->Hle, 0xff, (size_t)RS * sizeof(int), s));
    }
    if ((rc = node_film_ln(b, ep, pairs, layer, s))) return rc;
    HIPCHK(hipMemcpyAsync(io->d_Hres, b->Hres, (size_t)R * H * f4, D2D, s));
    HIPCHK(hipMemcpyAsync(io->d_Hl, b->Hl, (size_t)R * H * f4, D2D, s));
    if (io->d_rmax)  // (the batch's rows are max_pairs N apart)
      HIPCHK(hipMemcpy2DAsync(io->d_rmax, (size_t)R * f4, b->rmx, (size_t)RS * f4, (size_t)R * f4, 4, D2D, s));
    if (io->d_split) {
      HIPCHK(hipMemcpyAsync(io->d_split, b->Hls, (size_t)R * H * 4, D2D, s));
      HIPCHK(hipMemcpyAsync(io->d_exp, b->Hle, (size_t)R * sizeof(int), D2D, s));
    }
  } else {
    HIPCHK(hipMemcpyAsync(b->Hres, io->d_Hres, (size_t)R * H * f4, D2D, s));
    HIPCHK(hipMemcpyAsync(b->HO, io->d_HO, (size_t)R * HEADS_N * f4, D2D, s));
    HIPCHK(hipMemsetAsync(b->Hf, 0xff, (size_t)RS * H * f4, s));
    HIPCHK(hipMemsetAsync(b->LAT, 0xff, (size_t)b->P * B * 9 * f4, s));
    if ((rc = node_final_ln(b, pairs, s))) return rc;
    if ((rc = node_graph_heads(b, pairs, io->d_lat, s))) return rc;
    if (io->d_types || io->d_coords)
      if ((rc = node_split_heads(b, pairs, io->d_types, io->d_coords, s))) return rc;
    HIPCHK(hipMemcpyAsync(io->d_Hf, b->Hf, (size_t)R * H * f4, D2D, s));
    HIPCHK(hipMemcpyAsync(io->d_LAT, b->LAT, (size_t)pairs * B * 9 * f4, D2D, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return CHM_OK;
}

// The update half of a step on caller-supplied decoder outputs (tests/test_gpu_step_update.py): step_predictor /
// step_corrector with sample_step's StepArgs. Every argument check runs before the first HIP call.
extern "C" int chm_debug_step_update(chm_batch* b, const chm_schedule* sc, int t, const int32_t* d_t, float cond_scale,
                                     const chm_step_io* io, uint64_t seed, int64_t node_base, int64_t graph_base,
                                     const float* d_types, int64_t n_types, const float* d_coords, int64_t n_coords,
                                     const float* d_lattice, int64_t n_lattice, int stage, void* stream) {
  auto bad = [&](const std::string& why) { return fail(CHM_E_ARG, "chm_debug_step_update: " + why); };
  // what needs no batch first, so that those refusals can be tested without a device
  if (!sc) return bad("schedule is NULL");
  if (!io) return bad("io is NULL");
  if (stage != 1 && stage != 2) return bad("stage " + std::to_string(stage) + " outside {1, 2}");
  if (sc->T < 1) return bad("schedule: T must be >= 1");
  if (!d_t && (t < 1 || t > sc->T))
    return bad("t " + std::to_string(t) + " outside [1, " + std::to_string(sc->T) + "]");
  if (!sc->d_coef || !sc->d_q_one_step || !sc->d_q_mats) return bad("NULL schedule table");
  if (!io->d_atom_types || !io->d_frac || !io->d_lattices) return bad("io: a state buffer is NULL");
  const int given = (io->d_rand_a != nullptr) + (io->d_rand_l != nullptr) + (io->d_rand_x1 != nullptr) +
                    (io->d_rand_x2 != nullptr);
  if (given != 0 && given != 4) return bad("noise: all four buffers or none");
  if (!d_coords) return bad("d_coords is NULL");
  if (stage == 1 && !d_types) return bad("d_types is NULL (stage 1)");
  if (stage == 1 && !d_lattice) return bad("d_lattice is NULL (stage 1)");
  if (!b) return bad("batch is NULL");
  if (b->P < 2) return bad("max_pairs: the batch needs 2 (its head buffers hold the cond and the null outputs)");
  if (sc->num_classes != b->m->d.max_atoms || sc->time_dim != b->m->d.time_dim)
    return bad("schedule: num_classes " + std::to_string(sc->num_classes) + " / time_dim " +
               std::to_string(sc->time_dim) + " do not match the model's " + std::to_string(b->m->d.max_atoms) +
               " / " + std::to_string(b->m->d.time_dim));
  int rc = check_step_io(b, io, false, true, false);
  if (rc) return rc;
  const long N = b->N, B = b->B, A = b->m->d.max_atoms;
  auto sized = [&](const void* p, int64_t n, long expect, const char* name) -> int {
    if (p && n != expect)
      return bad(std::string(name) + ": " + std::to_string(n) + " elements, the batch needs " + std::to_string(expect));
    return CHM_OK;
  };
  if ((rc = sized(d_types, n_types, 2 * N * A, "n_types [2,N,A]"))) return rc;
  if ((rc = sized(d_coords, n_coords, 2 * N * 3, "n_coords [2,N,3]"))) return rc;
  if ((rc = sized(d_lattice, n_lattice, 2 * B * 9, "n_lattice [2,B,3,3]"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (d_types) HIPCHK(copy_rows(d_types, A, b->HO, HEADS_N, 2 * N, (int)A, s));
  HIPCHK(copy_rows(d_coords, 3, b->HO + A, HEADS_N, 2 * N, 3, s));
  if (d_lattice)
    HIPCHK(hipMemcpyAsync(b->LAT, d_lattice, (size_t)2 * B * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
  const StepArgs sa = step_args(b, sc, t, d_t, cond_scale, io, seed, node_base, graph_base);
  if (stage == 1) HIPCHK(step_predictor(sa, s));
  else HIPCHK(step_corrector(sa, s));
  HIPCHK(hipStreamSynchronize(s));
  return CHM_OK;
}

// The training kernels on caller-supplied decoder outputs (tests/test_gpu_train_kernels.py): train_noise, then
// train_loss, with chm_training_loss's TrainArgs and no decoder call between them. Every argument check runs before
// the first HIP call, the batch-independent ones first, so a refused call needs no device.
extern "C" int chm_debug_train_update(chm_batch* b, const chm_train_tables* tt, const int64_t* d_t, const int64_t* a0,
                                      const float* x0, const float* l0, const float* rand_a, const float* noise_l,
                                      const float* noise_x, const float* d_types, int64_t n_types,
                                      const float* d_coords, int64_t n_coords, const float* d_lattice,
                                      int64_t n_lattice, float* out, int64_t* a_t, float* x_t, float* l_t,
                                      float* target_x, float* part, void* stream) {
  auto bad = [&](const std::string& why) { return fail(CHM_E_ARG, "chm_debug_train_update: " + why); };
  if (!tt) return bad("tables is NULL");
  if (tt->T < 1) return bad("tables: T must be >= 1");
  if (!tt->d_coef4 || !tt->d_q_one_step || !tt->d_q_mats) return bad("NULL table");
  if (!d_t) return bad("d_t is NULL");
  if (!a0 || !x0 || !l0) return bad(std::string(!a0 ? "d_a0" : !x0 ? "d_x0" : "d_l0") + " is NULL");
  if (!rand_a || !noise_l || !noise_x) return bad("noise: all three buffers are required");
  if (!d_types) return bad("d_types is NULL");
  if (!d_coords) return bad("d_coords is NULL");
  if (!d_lattice) return bad("d_lattice is NULL");
  if (!out) return bad("d_out is NULL");
  if (!a_t || !x_t || !l_t || !target_x) return bad("the noised-state outputs are required");
  if (!part) return bad("d_part is NULL");
  if (!b) return bad("batch is NULL");
  const long N = b->N, B = b->B, A = b->m->d.max_atoms;
  auto sized = [&](int64_t n, long expect, const char* name) -> int {
    if (n != expect)
      return bad(std::string(name) + ": " + std::to_string(n) + " elements, the batch needs " + std::to_string(expect));
    return CHM_OK;
  };
  int rc;
  if ((rc = sized(n_types, N * A, "n_types [N,A]"))) return rc;
  if ((rc = sized(n_coords, N * 3, "n_coords [N,3]"))) return rc;
  if ((rc = sized(n_lattice, B * 9, "n_lattice [B,3,3]"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const TrainArgs g = train_args(b, tt, d_t, a0, x0, l0, rand_a, noise_l, noise_x, out, a_t, x_t, l_t, target_x);
  HIPCHK(train_noise(g, s));
  HIPCHK(copy_rows(d_types, A, b->HO, HEADS_N, N, (int)A, s));
  HIPCHK(copy_rows(d_coords, 3, b->HO + A, HEADS_N, N, 3, s));
  HIPCHK(hipMemcpyAsync(b->LAT, d_lattice, (size_t)B * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(train_loss(g, s));
  HIPCHK(hipMemcpyAsync(part, g.part, (size_t)N * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return CHM_OK;
}

extern "C" int chm_debug_philox(uint64_t seed, int t, int kind, int64_t base, int64_t n, int normal, float* out,
                                void* stream) {
  if (n < 0 || !out || kind < 0 || kind > 6) return fail(CHM_E_ARG, "bad arguments");
  HIPCHK(philox_fill(seed, t, kind, base, n, normal, out, (hipStream_t)stream));
  return CHM_OK;
}

extern "C" int chm_debug_d3pm_philox(int N, int A, int T, const float* logits, const int64_t* xt, const int64_t* tn,
                                     const float* q1, const float* qm, uint64_t seed, int64_t node_base, int64_t* out,
                                     void* stream) {
  if (N < 0 || A < 1 || A > 128 || T < 1) return fail(CHM_E_ARG, "bad sizes");
  if (N == 0) return CHM_OK;
  if (!logits || !xt || !tn || !q1 || !qm || !out) return fail(CHM_E_ARG, "NULL argument");
  HIPCHK(d3pm_sample(N, A, T, logits, A, nullptr, 1.f, 0.f, xt, tn, 0, nullptr, nullptr, q1, qm, out, seed, node_base,
                     (hipStream_t)stream));
  return CHM_OK;
}
