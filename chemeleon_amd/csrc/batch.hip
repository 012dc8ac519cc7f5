// chm_batch: the host-side index tables and plans of a batch, its workspace layout, the batch entry points, and
// the host-only queries that restate the tables and plans for the CPU tests (chm_debug_row_nodes .. _pair_nodes).
#include <algorithm>

#include "chm_host.h"

using namespace chm;

// Host-side index tables of a batch (the implicit fc edge layout) and the byte layout of its
// device memory: index tables first, then the decoder workspace, each piece 256-byte aligned.
// The same carve() sequence sizes the block (base == null) and binds a batch to it.
struct BatchOpts {
  int knn = 0, max_nb = 20, per_atom = 128;
};

static int batch_opts(const chm_batch_options* o, BatchOpts& bo) {
  if (!o) return CHM_OK;
  if (o->edge_style != CHM_EDGES_FC && o->edge_style != CHM_EDGES_KNN) return fail(CHM_E_ARG, "unknown edge_style");
  bo.knn = o->edge_style == CHM_EDGES_KNN;
  bo.max_nb = o->max_neighbors;  // <= 0: no neighbour cap (get_max_neighbors_mask, data_utils.py:341-348)
  if (o->knn_edges_per_atom) bo.per_atom = o->knn_edges_per_atom;
  if (bo.per_atom < 1 || bo.per_atom > 4096) return fail(CHM_E_ARG, "knn_edges_per_atom out of range");
  return CHM_OK;
}

static int batch_tables(const int32_t* h_natoms, int B, BatchTables& t, const BatchOpts& bo = BatchOpts()) {
  t.nat.assign(h_natoms, h_natoms + B);
  t.noff.assign(B + 1, 0);
  t.eoff.assign(B + 1, 0);
  long N = 0, E = 0;
  for (int g = 0; g < B; ++g) {
    if (t.nat[g] < 1) return fail(CHM_E_ARG, "every crystal needs at least one atom");
    if (t.nat[g] > kTileRows) return fail(CHM_E_UNSUPPORTED, "crystals above 256 atoms are not supported");
    t.noff[g] = (int)N;
    t.eoff[g] = E;
    N += t.nat[g];
    E += (long)t.nat[g] * t.nat[g];
    t.Ep += (long)t.nat[g] * (t.nat[g] + 1) / 2;
    if (N > (1L << 30) || E > (1L << 31) - 1) return fail(CHM_E_ARG, "batch too large");
  }
  t.noff[B] = (int)N;
  t.eoff[B] = E;
  t.N = N;
  t.E = E;
  t.knn = bo.knn;
  if (bo.knn) {  // radius graph: candidates n^2 * 27 per crystal, edges up to per_atom per atom
    t.coff.assign(B + 1, 0);
    for (int g = 0; g < B; ++g) t.coff[g + 1] = t.coff[g] + (long)t.nat[g] * t.nat[g] * 27;
    t.C = t.coff[B];
    t.E = N * (long)bo.per_atom;
    if (t.E > (1L << 31) - 1) return fail(CHM_E_ARG, "batch too large");
  }
  return CHM_OK;
}

// Row-tile geometry: tiles [0, nbig) of 256 rows, then tiles of kShortRows (nbig < 0: all 256 rows)
static long rt_count(long E, long nbig) {
  return nbig < 0 ? (E + kTileRows - 1) / kTileRows : nbig + (E - nbig * kTileRows + kShortRows - 1) / kShortRows;
}
static long rt_start(long k, long nbig) {
  return nbig < 0 || k <= nbig ? k * kTileRows : nbig * kTileRows + (k - nbig) * kShortRows;
}

// Row tiles of an fc batch (edge rows grouped by source node; node v's rows [estart, estart + n)):
// tile t = rows [256 t, 256 t + 256) (a mixed tiling: rt_start), {first node starting in it, first node starting
// after it, the node that began in tile t-1 and continues here (-1: none), the offset of those continued rows in
// msgbuf}. Returns the continued rows' total (msgbuf rows per conditioning); out null: sizing only.
static long row_tiles(const BatchTables& t, std::vector<int4>* out) {
  const long E = t.E, nrt = rt_count(E, t.rt_nbig), nb = t.rt_nbig;
  if (out) out->assign(nrt, make_int4((int)t.N, (int)t.N, -1, 0));
  long r2tot = 0, tc = 0, node = 0;
  long prev_end = 0;  // end row of the previous node
  for (size_t g = 0; g < t.nat.size(); ++g)
    for (int i = 0; i < t.nat[g]; ++i, ++node) {
      const long es = t.eoff[g] + (long)i * t.nat[g];
      for (; tc < nrt && rt_start(tc, nb) <= es; ++tc) {  // tiles starting in (previous start, es]
        const long s0 = rt_start(tc, nb);
        int4 r = make_int4((int)node, (int)t.N, -1, 0);
        if (node > 0 && prev_end > s0 && s0 < es) {  // node-1 began before the tile and reaches into it
          r.z = (int)(node - 1);
          r.w = (int)r2tot;
          r2tot += prev_end - s0;
        }
        if (out) (*out)[tc] = r;
      }
      prev_end = es + t.nat[g];
    }
  for (; tc < nrt; ++tc) {  // tiles after the last node start (the last node's rest)
    const long s0 = rt_start(tc, nb);
    int4 r = make_int4((int)t.N, (int)t.N, -1, 0);
    if (prev_end > s0) {
      r.z = (int)(t.N - 1);
      r.w = (int)r2tot;
      r2tot += prev_end - s0;
    }
    if (out) (*out)[tc] = r;
  }
  if (out)
    for (long k = 0; k < nrt; ++k) (*out)[k].y = k + 1 < nrt ? (*out)[k + 1].x : (int)t.N;
  return r2tot;
}

// The node list of every row tile, exactly as edge16.hip's segment-mean epilogue would derive it from
// rtiles / node_estart / node_n: {node, rows in the tile | first row in the tile << 10 | kind << 20},
// kind 0 = a whole node, 1 = the head part of a node cut at the tile end (listed first), 2 = the rest of
// a node begun in the previous tile (listed last). Unused entries are zero.
static void row_tile_nodes(BatchTables& t) {
  const long nrt = (long)t.rtiles.size(), E = t.E;
  t.rinfo.assign((size_t)nrt * kRowInfo, make_int2(0, 0));
  t.rinfo_n.assign(nrt, 0);
  for (long k = 0; k < nrt; ++k) {
    const int4 rt = t.rtiles[k];
    const long e0 = rt_start(k, t.rt_nbig), e1 = std::min<long>(E, rt_start(k + 1, t.rt_nbig));
    const int nreg = rt.y - rt.x;
    const bool head = nreg > 0 && t.estart[rt.y - 1] + t.nn[rt.y - 1] > e1;
    const bool cont = rt.z >= 0;
    const int nn = nreg + (cont ? 1 : 0);
    int2* o = t.rinfo.data() + (size_t)k * kRowInfo;
    for (int i = 0; i < nn; ++i) {
      if (cont && i == nn - 1) {
        o[i] = make_int2(rt.z, (int)(t.estart[rt.z] + t.nn[rt.z] - e0) | (2 << 20));
      } else {
        const int v = rt.x + (head ? (i == 0 ? nreg - 1 : i - 1) : i);
        const long es = t.estart[v], end = es + t.nn[v];
        o[i] = make_int2(v, (int)((end > e1 ? e1 : end) - es) | ((int)(es - e0) << 10) | ((head && i == 0) ? 1 << 20 : 0));
      }
    }
    t.rinfo_n[k] = nn;
  }
}

// fills the per-node / per-edge tables (only when the batch is really built)
static void batch_fill(BatchTables& t) {
  const int B = (int)t.nat.size();
  const long N = t.N, E = t.E;
  t.n2g.resize(N);
  t.nn.resize(N);
  for (int g = 0; g < B; ++g)
    for (int i = 0; i < t.nat[g]; ++i) {
      t.n2g[t.noff[g] + i] = g;
      t.nn[t.noff[g] + i] = t.nat[g];
    }
  if (t.knn) return;  // (edge tables are built per decoder call)
  t.pi.resize(t.Ep);
  t.pj.resize(t.Ep);
  t.pe.resize(t.Ep);
  for (int g = 0, p = 0; g < B; ++g) {
    const int n = t.nat[g], o = t.noff[g];
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j, ++p) {
        t.pi[p] = o + i;
        t.pj[p] = o + j;
        t.pe[p] = make_int2((int)(t.eoff[g] + (long)i * n + j), (int)(t.eoff[g] + (long)j * n + i));
      }
  }
  // the pair tiles' P / Q node ranges: from the first pair's i (pairs are ordered by crystal, then i <= j, so every
  // node of the tile is >= it) to the end of the crystal of the last pair (every j of the tile is below it)
  t.pnode.resize((t.Ep + kPairRows - 1) / kPairRows);
  for (size_t k = 0; k < t.pnode.size(); ++k) {
    const long p0 = (long)k * kPairRows, p1 = std::min<long>(p0 + kPairRows, t.Ep) - 1;
    const int gl = t.n2g[t.pi[p1]];
    t.pnode[k] = make_int2(t.pi[p0], t.noff[gl] + t.nat[gl] - t.pi[p0]);
  }
  t.ei.resize(E);
  t.ej.resize(E);
  t.estart.resize(N);
  for (int g = 0; g < B; ++g) {
    long e = t.eoff[g];
    for (int i = 0; i < t.nat[g]; ++i)
      for (int j = 0; j < t.nat[g]; ++j, ++e) {
        t.ei[e] = t.noff[g] + i;
        t.ej[e] = t.noff[g] + j;
      }
  }
  // segment tiles: runs of whole nodes whose edge rows fit one 256-row GEMM tile
  int cur0 = 0;
  long rows = 0;
  t.tiles.clear();
  for (int g = 0; g < B; ++g)
    for (int i = 0; i < t.nat[g]; ++i) {
      const int node = t.noff[g] + i;
      t.estart[node] = t.eoff[g] + (long)i * t.nat[g];
      if (rows + t.nat[g] > kTileRows) {
        t.tiles.push_back(make_int2(cur0, node));
        cur0 = node;
        rows = 0;
      }
      rows += t.nat[g];
    }
  t.tiles.push_back(make_int2(cur0, (int)N));
  t.r2tot = row_tiles(t, &t.rtiles);
  t.nrt = (long)t.rtiles.size();
  row_tile_nodes(t);
}

// number of segment tiles without building the tables (sizing only)
static long count_tiles(const BatchTables& t) {
  if (t.knn) return t.N + 1;
  long n = 1, rows = 0;
  for (size_t g = 0; g < t.nat.size(); ++g)
    for (int i = 0; i < t.nat[g]; ++i) {
      if (rows + t.nat[g] > kTileRows) {
        ++n;
        rows = 0;
      }
      rows += t.nat[g];
    }
  return n;
}

// A mixed row tiling for edge layer 2 (r6). Below edge_layer_min row tiles edge layer 2 runs on the
// two-launch schedule, where a last round of 256-row tiles may leave CUs idle (64x20: 400 tiles on 256 CUs, the second
// round 56% full). When that round is at most 3/4 full, its rows fit one round of 192-row tiles, which cost ~3/4 of a
// 256-row tile: tiles [0, nbig) fill whole rounds with 256 rows (one launch), the rest run on kShortRows rows
// (k_edge16_short, a second launch). Returns nbig, or -1 for the uniform tiling. A cut node's sum stays one sequential
// sum over its edges across tile ends, so every output is bit-identical to the uniform tiling's.
static long short_row_tiles(const BatchTables& t, int P, long ncu, long layer_min) {
  if (t.knn || t.E <= 0 || ncu <= 0 || P < 1) return -1;
  const long R = (t.E + kTileRows - 1) / kTileRows;
  if (R >= layer_min) return -1;  // (the pair grid takes uniform tiles)
  for (int n : t.nat)
    if (n > kShortRows) return -1;  // (a node then spans at most two tiles)
  const long J = 2L * P, per = ncu / J;  // jobs per row tile (conditionings x column tiles); row tiles per round
  if (per < 1) return -1;
  const long rounds = (R * J + ncu - 1) / ncu;
  const long nbig = (rounds - 1) * per;
  if (rt_count(t.E, nbig) - nbig > per) return -1;  // more than one round of short tiles
  return nbig;
}
static long short_row_tiles(const BatchTables& t, const chm_model* m, int P) {
  if (m->math != MATH_SPLIT16 || !m->edge_rows_short || !m->edge_rows) return -1;
  return short_row_tiles(t, P, m->ncu, m->edge_layer_min);
}

// carves every device buffer of `b` from `base` (null: sizing pass); returns the bytes used
static size_t batch_layout(chm_batch* b, const chm_model* m, char* base, long ntiles) {
  const int P = b->P, L = m->d.num_layers, X = m->d.text_dim, B = b->B;
  const long N = b->N, E = b->E;
  size_t off = 0;
  auto carve = [&](size_t bytes) -> void* {
    const size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return base ? base + o : nullptr;
  };
  auto fl = [&](size_t n) { return (float*)carve(n * sizeof(float)); };
  b->natoms = (int*)carve(B * sizeof(int));
  b->node_off = (int*)carve((B + 1) * sizeof(int));
  b->edge_off = (long*)carve((B + 1) * sizeof(long));
  b->n2g = (int*)carve(N * sizeof(int));
  b->ei = (int*)carve(E * sizeof(int));
  b->ej = (int*)carve(E * sizeof(int));
  b->node_estart = (long*)carve(N * sizeof(long));
  b->node_n = (int*)carve(N * sizeof(int));
  b->tiles = (int2*)carve(ntiles * sizeof(int2));
  if (!b->knn && b->Ep > 0) {  // fc: the pair tables of edge layer 1 on pairs
    b->pi = (int*)carve(b->Ep * sizeof(int));
    b->pj = (int*)carve(b->Ep * sizeof(int));
    b->pe = (int2*)carve(b->Ep * sizeof(int2));
    b->pnode = (int2*)carve((b->Ep + kPairRows - 1) / kPairRows * sizeof(int2));
  }
  if (!b->pplan.jobs.empty()) {  // (and the one-grid pair schedule: job lists, ranges, per-layer words)
    b->pjobs = (int4*)carve(b->pplan.djobs.size() * sizeof(int4));
    b->psched = (unsigned*)carve((size_t)L * 8 * b->pplan.npx * sizeof(unsigned));
  }
  if (b->nrt > 0) {  // fc: row tiles of edge layer 2, the partial sums of cut nodes, the fallback rows
    b->rtiles = (int4*)carve(b->nrt * sizeof(int4));
    b->rinfo = (int2*)carve((size_t)b->nrt * kRowInfo * sizeof(int2));
    b->rinfo_n = (int*)carve(b->nrt * sizeof(int));
    b->sbuf = fl((size_t)P * b->nrt * H);
    b->msgbuf = fl((size_t)P * (b->r2tot + 1) * H);
    b->rcnt = (unsigned*)carve((size_t)P * b->nrt * 8 * sizeof(unsigned));
    b->xbad = (unsigned*)carve(2 * kMaxLayers * sizeof(unsigned));  // layer l: [l] (the second half: unused)
  }
  if (b->knn) {  // (E = the edge capacity E_cap)
    b->cand_off = (long*)carve((B + 1) * sizeof(long));
    b->cand_key = (unsigned*)carve(b->C_cap * sizeof(unsigned));
    b->cand2 = (unsigned*)carve(b->C_cap * sizeof(unsigned));
    b->cand_d2 = (float*)carve(b->C_cap * sizeof(float));
    b->fin_key = (unsigned*)carve(2 * b->C_cap * sizeof(unsigned));
    b->fin_fd = (float*)carve(6 * b->C_cap * sizeof(float));
    b->fd = (float*)carve(3 * E * sizeof(float));
    b->atom_cnt = (int*)carve(N * sizeof(int));
    b->deg = (int*)carve(N * sizeof(int));
    b->cryst_fin = (int*)carve(B * sizeof(int));
  }
  b->cin = fl((size_t)P * B * (TD + X));
  b->cemb = fl((size_t)P * B * 2 * H);
  b->Hres = fl((size_t)P * N * H);
  b->Hl = fl((size_t)P * N * H);
  b->Y = fl((size_t)P * N * H);
  b->agg = fl((size_t)P * N * H);
  b->PQ = fl((size_t)P * N * 2 * H);
  b->gbias = fl((size_t)L * B * H);
  // (F and S carry kTileRows rows of padding: the split16 edge GEMMs read whole 256-row tiles)
  b->F = fl((size_t)(E + kTileRows) * FD);
  b->S = fl(((size_t)P * E + kTileRows) * H);
  b->M = b->math == MATH_F32 ? fl((size_t)P * E * H) : nullptr;
  b->rowmax = b->math == MATH_SPLIT16 ? (unsigned*)fl((size_t)P * E) : nullptr;
  b->rmx = fl((size_t)4 * P * N);
  if (b->math == MATH_SPLIT16 && m->node_ps) {  // (option node_ps at batch creation: ~335 MB at 512x40, P = 2)
    void** sp[4] = {&b->Hs, &b->Hls, &b->aggs, &b->Us};
    int** se[4] = {&b->He, &b->Hle, &b->agge, &b->Ue};
    for (int k = 0; k < 4; ++k) {
      *sp[k] = carve((size_t)P * N * H * 4);
      *se[k] = (int*)carve((size_t)P * N * sizeof(int));
    }
  } else {
    b->Hs = b->Hls = b->aggs = b->Us = nullptr;
    b->He = b->Hle = b->agge = b->Ue = nullptr;
  }
  b->Hf = fl((size_t)P * N * H);
  b->HO = fl((size_t)P * N * HEADS_N);
  b->LAT = fl((size_t)P * B * 9);
  return off;
}

static int batch_build(const chm_model* m, const int32_t* h_natoms, int B, int max_pairs, void* d_ws,
                       size_t ws_bytes, hipStream_t s, chm_batch** out, const BatchOpts& bo = BatchOpts()) {
  if (!out) return fail(CHM_E_ARG, "out is NULL");
  *out = nullptr;
  if (!m || !h_natoms || B < 1) return fail(CHM_E_ARG, "bad batch arguments");
  if (max_pairs < 1 || max_pairs > 2) return fail(CHM_E_ARG, "max_pairs must be 1 or 2");
  if (bo.knn && m->math != MATH_SPLIT16)
    return fail(CHM_E_UNSUPPORTED, "knn edges need the split16 arithmetic (the k_edge16 kernels)");
  BatchTables t;
  int rc = batch_tables(h_natoms, B, t, bo);
  if (rc) return rc;
  t.rt_nbig = short_row_tiles(t, m, max_pairs);
  batch_fill(t);
  chm_batch* b = new chm_batch();
  b->m = m;
  b->math = m->math;
  b->B = B;
  b->P = max_pairs;
  b->N = t.N;
  b->E = t.E;
  b->h_natoms = t.nat;
  b->knn = bo.knn;
  b->knn_max_nb = bo.max_nb;
  b->E_cap = t.E;
  b->C_cap = t.C;
  b->ntiles = t.knn ? (int)(t.N + 1) : (int)t.tiles.size();
  b->nrt = t.knn ? 0 : t.nrt;
  b->r2tot = t.knn ? 0 : t.r2tot;
  b->rt_nbig = t.knn ? -1 : t.rt_nbig;
  b->Ep = t.knn ? 0 : t.Ep;
  if (!t.knn && b->math == MATH_SPLIT16 && t.E > 0 && t.rt_nbig < 0) {  // (the pair grid: uniform row tiles)
    pair_plan(t.nat, t.E, t.Ep, t.nrt, b->P, m->edge_lag, b->pplan);
    if (!pair_plan_ok(b->pplan)) {
      delete b;
      return fail(CHM_E_UNSUPPORTED, "pair grid plan: a flag index outside its list");
    }
  }
  const size_t need = batch_layout(b, m, nullptr, b->ntiles);
  char* base = (char*)d_ws;
  if (!base) {
    if (hipMalloc(&b->owned, need) != hipSuccess) {
      delete b;
      return fail(CHM_E_HIP, "hipMalloc failed for the batch workspace (" + std::to_string(need) + " bytes)");
    }
    base = (char*)b->owned;
  } else if (ws_bytes < need || ((uintptr_t)base & 255)) {
    delete b;
    return fail(CHM_E_ARG, "workspace too small or not 256-byte aligned (need " + std::to_string(need) + " bytes)");
  }
  b->bytes = batch_layout(b, m, base, b->ntiles);
  // index tables (setup only: the host vectors must outlive the copies, so the stream is drained)
  hipError_t e = hipSuccess;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  };
  up(b->natoms, t.nat.data(), B * sizeof(int));
  up(b->node_off, t.noff.data(), (B + 1) * sizeof(int));
  up(b->edge_off, t.eoff.data(), (B + 1) * sizeof(long));
  up(b->n2g, t.n2g.data(), t.N * sizeof(int));
  if (t.knn) {
    up(b->cand_off, t.coff.data(), (B + 1) * sizeof(long));
    b->E = 0;  // no graph yet
    b->ntiles = 0;
  } else {
    up(b->ei, t.ei.data(), t.E * sizeof(int));
    up(b->ej, t.ej.data(), t.E * sizeof(int));
    up(b->node_estart, t.estart.data(), t.N * sizeof(long));
    up(b->node_n, t.nn.data(), t.N * sizeof(int));
    up(b->tiles, t.tiles.data(), t.tiles.size() * sizeof(int2));
    up(b->rtiles, t.rtiles.data(), t.rtiles.size() * sizeof(int4));
    up(b->rinfo, t.rinfo.data(), t.rinfo.size() * sizeof(int2));
    up(b->rinfo_n, t.rinfo_n.data(), t.rinfo_n.size() * sizeof(int));
    up(b->pi, t.pi.data(), t.pi.size() * sizeof(int));
    up(b->pj, t.pj.data(), t.pj.size() * sizeof(int));
    up(b->pe, t.pe.data(), t.pe.size() * sizeof(int2));
    up(b->pnode, t.pnode.data(), t.pnode.size() * sizeof(int2));
    if (b->pjobs) {
      up(b->pjobs, b->pplan.djobs.data(), b->pplan.djobs.size() * sizeof(int4));
    }
    if (e == hipSuccess && b->rcnt)  // (the counters return to 0 at the end of every launch)
      e = hipMemsetAsync(b->rcnt, 0, (size_t)b->P * b->nrt * 8 * sizeof(unsigned), s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    chm_batch_destroy(b);
    return fail(CHM_E_HIP, std::string("index upload: ") + hipGetErrorString(e));
  }
  *out = b;
  return CHM_OK;
}

extern "C" int chm_debug_row_nodes_ex(const int32_t* h_natoms, int B, int64_t nbig, int32_t* out2, int64_t cap2,
                                      int32_t* counts, int64_t cap) {
  if (!h_natoms || B < 1) return fail(CHM_E_ARG, "bad batch arguments");
  BatchTables t;
  int rc = batch_tables(h_natoms, B, t);
  if (rc) return rc;
  if (nbig >= 0 && nbig * kTileRows >= t.E) return fail(CHM_E_ARG, "nbig: no short tile left");
  t.rt_nbig = nbig < 0 ? -1 : nbig;
  batch_fill(t);
  const long R = (long)t.rtiles.size();
  if (out2 && cap2 >= 2 * (int64_t)t.rinfo.size())
    for (size_t k = 0; k < t.rinfo.size(); ++k) {
      out2[2 * k] = t.rinfo[k].x;
      out2[2 * k + 1] = t.rinfo[k].y;
    }
  if (counts && cap >= R)
    for (long k = 0; k < R; ++k) counts[k] = t.rinfo_n[k];
  return (int)R;
}

extern "C" int chm_debug_row_nodes(const int32_t* h_natoms, int B, int32_t* out2, int64_t cap2, int32_t* counts,
                                   int64_t cap) {
  return chm_debug_row_nodes_ex(h_natoms, B, -1, out2, cap2, counts, cap);
}

extern "C" int chm_debug_row_tiles_ex(const int32_t* h_natoms, int B, int64_t nbig, int32_t* out4, int64_t cap4,
                                      int64_t* r2tot) {
  if (!h_natoms || B < 1) return fail(CHM_E_ARG, "bad batch arguments");
  BatchTables t;
  int rc = batch_tables(h_natoms, B, t);
  if (rc) return rc;
  if (nbig >= 0 && nbig * kTileRows >= t.E) return fail(CHM_E_ARG, "nbig: no short tile left");
  t.rt_nbig = nbig < 0 ? -1 : nbig;
  std::vector<int4> rt;
  const long r2 = row_tiles(t, &rt);
  if (r2tot) *r2tot = r2;
  if (out4 && cap4 >= 4 * (int64_t)rt.size())
    for (size_t k = 0; k < rt.size(); ++k) {
      out4[4 * k] = rt[k].x; out4[4 * k + 1] = rt[k].y; out4[4 * k + 2] = rt[k].z; out4[4 * k + 3] = rt[k].w;
    }
  return (int)rt.size();
}

extern "C" int chm_debug_row_tiles(const int32_t* h_natoms, int B, int32_t* out4, int64_t cap4, int64_t* r2tot) {
  return chm_debug_row_tiles_ex(h_natoms, B, -1, out4, cap4, r2tot);
}

// the mixed row tiling short_row_tiles chooses for a batch (256-row tiles before the short ones, -1: uniform)
extern "C" int64_t chm_debug_short_row_tiles(const int32_t* h_natoms, int B, int P, int ncu, int64_t layer_min) {
  if (!h_natoms || B < 1 || P < 1 || P > 2) return fail(CHM_E_ARG, "bad batch arguments");
  BatchTables t;
  int rc = batch_tables(h_natoms, B, t);
  if (rc) return rc;
  return short_row_tiles(t, P, ncu, layer_min);
}

// the row tiling of a batch as it was created (256-row tiles before the short ones, -1: uniform)
extern "C" int64_t chm_batch_short_row_tiles(const chm_batch* b) {
  if (!b) return fail(CHM_E_ARG, "batch is NULL");
  return b->rt_nbig;
}

extern "C" int chm_batch_create(const chm_model* m, const int32_t* h_natoms, int B, int max_pairs, chm_batch** out) {
  return batch_build(m, h_natoms, B, max_pairs, nullptr, 0, nullptr, out);
}

extern "C" size_t chm_batch_workspace_bytes_ex(const chm_model* m, const int32_t* h_natoms, int B, int max_pairs,
                                               const chm_batch_options* opts) {
  if (!m || !h_natoms || B < 1 || max_pairs < 1 || max_pairs > 2) {
    fail(CHM_E_ARG, "bad batch arguments");
    return 0;
  }
  BatchOpts bo;
  if (batch_opts(opts, bo)) return 0;
  BatchTables t;
  if (batch_tables(h_natoms, B, t, bo)) return 0;
  chm_batch b;
  b.m = m;
  b.math = m->math;
  b.B = B;
  b.P = max_pairs;
  b.N = t.N;
  b.E = t.E;
  b.knn = bo.knn;
  b.C_cap = t.C;
  if (!t.knn) {
    t.rt_nbig = short_row_tiles(t, m, max_pairs);
    b.nrt = rt_count(t.E, t.rt_nbig);
    b.r2tot = row_tiles(t, nullptr);
    b.Ep = t.Ep;
    if (b.math == MATH_SPLIT16 && t.E > 0 && t.rt_nbig < 0) pair_plan(t.nat, t.E, t.Ep, b.nrt, b.P, m->edge_lag, b.pplan);
  }
  return batch_layout(&b, m, nullptr, count_tiles(t));
}

extern "C" size_t chm_batch_workspace_bytes(const chm_model* m, const int32_t* h_natoms, int B, int max_pairs) {
  return chm_batch_workspace_bytes_ex(m, h_natoms, B, max_pairs, nullptr);
}

extern "C" int chm_batch_create_ex(const chm_model* m, const int32_t* h_natoms, int B, int max_pairs,
                                   const chm_batch_options* opts, void* d_workspace, size_t workspace_bytes,
                                   void* stream, chm_batch** out) {
  BatchOpts bo;
  const int rc = batch_opts(opts, bo);
  if (rc) return rc;
  return batch_build(m, h_natoms, B, max_pairs, d_workspace, workspace_bytes, (hipStream_t)stream, out, bo);
}

extern "C" int chm_batch_create_with_workspace(const chm_model* m, const int32_t* h_natoms, int B, int max_pairs,
                                               void* d_workspace, size_t workspace_bytes, void* stream,
                                               chm_batch** out) {
  if (!d_workspace) return fail(CHM_E_ARG, "workspace is NULL");
  return batch_build(m, h_natoms, B, max_pairs, d_workspace, workspace_bytes, (hipStream_t)stream, out);
}

extern "C" void chm_batch_destroy(chm_batch* b) {
  if (!b) return;
  if (b->owned) (void)hipFree(b->owned);
  delete b;
}

extern "C" size_t chm_batch_device_bytes(const chm_batch* b) { return b ? b->bytes : 0; }
extern "C" int64_t chm_batch_num_nodes(const chm_batch* b) { return b ? b->N : -1; }
extern "C" int64_t chm_batch_num_edges(const chm_batch* b) { return b ? b->E : -1; }
// (host only, tests) the one-grid pair schedule of an fc batch: see include/chemeleon_hip.h
extern "C" int64_t chm_debug_pair_plan(const int32_t* h_natoms, int B, int P, int lag, int32_t* rng, int64_t cap_rng,
                                       int32_t* pa, int32_t* pb, int32_t* njobs, int32_t* jobs, int64_t cap_jobs) {
  if (!h_natoms || B < 1 || P < 1 || P > 2 || lag < 1) return fail(CHM_E_ARG, "bad arguments");
  BatchTables t;
  if (int rc = batch_tables(h_natoms, B, t)) return rc;
  const long R = (t.E + kTileRows - 1) / kTileRows;
  PairPlan pl;
  pair_plan(t.nat, t.E, t.Ep, R, P, lag, pl);
  if (!pair_plan_ok(pl)) return fail(CHM_E_UNSUPPORTED, "pair grid plan: a flag index outside its list");
  if (rng && cap_rng >= 2 * R)
    for (long k = 0; k < R; ++k) { rng[2 * k] = pl.rng[k].x; rng[2 * k + 1] = pl.rng[k].y; }
  for (int x = 0; x < 8; ++x) {
    if (pa) pa[x] = pl.pa[x];
    if (pb) pb[x] = pl.pb[x];
    if (njobs) njobs[x] = pl.njobs[x];
  }
  if (jobs && cap_jobs >= 2L * 8 * pl.jstride)
    for (size_t k = 0; k < pl.jobs.size(); ++k) { jobs[2 * k] = pl.jobs[k].x; jobs[2 * k + 1] = pl.jobs[k].y; }
  return pl.jstride;
}

// (host only, tests) the pair tiles' P / Q node ranges of an fc batch: see include/chemeleon_hip.h
extern "C" int64_t chm_debug_pair_nodes(const int32_t* h_natoms, int B, int32_t* out, int64_t cap) {
  if (!h_natoms || B < 1) return fail(CHM_E_ARG, "bad arguments");
  BatchTables t;
  if (int rc = batch_tables(h_natoms, B, t)) return rc;
  batch_fill(t);
  const int64_t NP = (int64_t)t.pnode.size();
  if (out && cap >= 2 * NP)
    for (int64_t k = 0; k < NP; ++k) { out[2 * k] = t.pnode[k].x; out[2 * k + 1] = t.pnode[k].y; }
  return NP;
}

extern "C" int chm_batch_device(const chm_batch* b) { return b ? b->m->device : fail(CHM_E_ARG, "batch is NULL"); }
extern "C" int chm_batch_info(const chm_batch* b, chm_dims* dims, int64_t* num_graphs, int* max_pairs, int* knn) {
  if (!b) return fail(CHM_E_ARG, "batch is NULL");
  if (dims) *dims = b->m->d;
  if (num_graphs) *num_graphs = b->B;
  if (max_pairs) *max_pairs = b->P;
  if (knn) *knn = b->knn;
  return CHM_OK;
}
