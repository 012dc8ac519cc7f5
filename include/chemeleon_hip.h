/* chemeleon_hip.h — C ABI of the MI355X (gfx950) sampling path of Chemeleon.
 *
 * The hot path of ryannduma/chemeleon is the reverse-diffusion loop
 * `Chemeleon.sample()` -> `_sample_generator()` -> `model_predictions()` ->
 * `CSPNet.forward()` plus the D3PM / DDPM / VE predictor-corrector updates
 * (chemeleon/modules/chemeleon.py:246-490, chemeleon/modules/cspnet.py:184-405,
 * chemeleon/utils/diff_utils.py:152-329). The reference is pure Python over
 * ATen, so there is no reference C interface to replace; each entry point
 * below names the Python interface whose behaviour it takes over.
 *
 * Conventions
 *  - Every pointer argument named d_* is a DEVICE pointer, caller-owned,
 *    fp32 unless stated; int64 where the reference uses torch.long.
 *  - All work is enqueued on the caller's HIP stream `stream`
 *    (a hipStream_t passed as void*); nothing synchronises the host except
 *    chm_model_create / chm_batch_create (setup).
 *  - No allocation inside chm_decoder_forward / chm_sample_step: the batch
 *    object owns a workspace sized at creation. Calls are graph-capturable.
 *  - Every function returns 0 on success or a negative CHM_E_* code;
 *    chm_last_error() returns a thread-local message for the last failure.
 *  - Conditioning index c: 0 = text ("cond"), 1 = null text ("null").
 */
#ifndef CHEMELEON_HIP_H
#define CHEMELEON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHM_OK 0
#define CHM_E_ARG (-1)      /* bad argument / shape */
#define CHM_E_HIP (-2)      /* HIP runtime error */
#define CHM_E_UNSUPPORTED (-3)

/* Hyper-parameters of the score network; mirrors the CSPNet constructor
 * (chemeleon/modules/cspnet.py:185-202). This build implements
 * hidden_dim = 512, num_freqs = 128, time_dim = 128 (or time_dim = text_dim = 0:
 * no FilmLayer), ln = ip = 1, smooth = 0, act "silu", dis_emb "sin"; other values
 * return CHM_E_UNSUPPORTED from chm_model_create. The edge style ("fc" or
 * "knn") is a property of the batch (chm_batch_options). */
typedef struct {
  int hidden_dim;  /* 512 */
  int time_dim;    /* 128 */
  int text_dim;    /* 512 */
  int num_layers;  /* 6 */
  int max_atoms;   /* 104 classes (103 elements + dummy) */
  int num_freqs;   /* 128 */
} chm_dims;

typedef struct chm_model chm_model;
typedef struct chm_batch chm_batch;

/* Last error message of the calling thread ("" if none). */
const char* chm_last_error(void);

/* Version string of the library build. */
const char* chm_version(void);

/* Number of decoder parameter tensors chm_model_create expects for `dims`
 * (= len(CSPNet.state_dict()) for ln=True, smooth=False). */
int chm_num_params(const chm_dims* dims);

/* Builds the packed device copy of the decoder weights.
 * Replaces: CSPNet.__init__ + load_state_dict (cspnet.py:185-234).
 * d_params[i] points to the i-th state_dict tensor in this order (row-major,
 * contiguous, fp32, nn.Linear layout [out][in]):
 *   node_embedding.weight, film_layer.mlp_cond.0.{weight,bias},
 *   film_layer.proj.{weight,bias}, film_layer.norm.{weight,bias} (not when
 *   time_dim = text_dim = 0),
 *   for l in 0..L-1: csp_layer_l.{edge_mlp.0.weight, edge_mlp.0.bias,
 *     edge_mlp.2.weight, edge_mlp.2.bias, node_mlp.0.weight, node_mlp.0.bias,
 *     node_mlp.2.weight, node_mlp.2.bias, layer_norm.weight, layer_norm.bias},
 *   coord_out.weight, lattice_out.weight, type_out.{weight,bias},
 *   final_layer_norm.{weight,bias}.
 * Synchronises `stream` before returning. */
int chm_model_create(const chm_dims* dims, const float* const* d_params, int n_params, void* stream,
                     chm_model** out);
void chm_model_destroy(chm_model* m);

/* Launch-schedule options (not thread-safe against concurrent steps of the same model):
 *   "edge16" (1): accepted for compatibility (the round-1 32x32x16 kernels were removed; 0 fails).
 *   "edge_rows", "edge_layer", "edge_lag", "edge_layer_min", "edge_rows_short": edge-layer
 *     schedules (bit-identical). A batch plans its pair-grid job lists (and sizes their
 *     buffers) with the edge_lag of its creation: a later change reaches batches created after it only.
 *   "node_ps" (0 / 1): split16 node GEMMs read their A operands pre-split by the producing kernels (not
 *     bit-identical to 0: within fp32 rounding; DESIGN.md §4 "Node GEMMs"); a batch carves their buffers only
 *     when created while the option is set (batches created without it keep the in-loop split).
 *   "edge_pairs" (0 / 1, default 1): fc edge layer 1 computed once per unordered pair of atoms (the reverse
 *     edge's Fourier features are the forward ones with the sine half negated), both directions' messages
 *     from one GEMM row; within fp32 rounding of the directed form (DESIGN.md §4 "Edge layer 1 on pairs").
 *   "edge_pairs_layer" (0 / 1, default 1): with edge_pairs, both edge layers in one static grid from
 *     "edge_layer_min" row tiles on (k_edge16_pairs_grid; bit-identical to two launches).
 *   The one-grid schedule runs only where model creation saw 8 XCDs ("xcd_mask" = 0xff); tests:
 *     "edge_layer_repair" (its layer-2 jobs always request the repair launches), "edge_rows_nowait",
 *     "edge_pairs_pq_global" (the pair epilogue's P / Q rows from global memory instead of LDS).
 * Returns CHM_E_ARG for an unknown key. */
int chm_model_set_option(chm_model* m, const char* key, int64_t value);

/* Arithmetic of the decoder GEMMs (all fp32-accurate, fp32 accumulation):
 *   CHM_MATH_SPLIT16 (default): the two edge GEMMs split each operand into an
 *     fp16 hi/lo pair (three fp16 MFMA products per fp32 product); W rows and
 *     activation rows carry power-of-two scales so every split operand is
 *     <= 1 in magnitude (the Fourier features already are; edge layer 1
 *     records max|S| per row for edge layer 2). Node GEMMs use bf16x3.
 *   CHM_MATH_BF16X3: every GEMM splits each operand into three bf16 parts,
 *     six bf16 MFMA products per fp32 product.
 *   CHM_MATH_F32: v_mfma_f32_32x32x2_f32 (exact fp32 fma chains); standalone
 *     aggregation kernel.
 * In the two split modes the edge message GEMM is fused with scatter_mean.
 * CHM_MATH=f32 / bf16x3 / split16 in the environment selects the mode at
 * creation. A batch keeps the mode its model had when the batch was created. */
#define CHM_MATH_BF16X3 0
#define CHM_MATH_F32 1
#define CHM_MATH_SPLIT16 2
int chm_model_set_math(chm_model* m, int mode);
int chm_model_get_math(const chm_model* m);

/* Describes a (possibly ragged) batch of crystals and owns the workspace of
 * its decoder calls. Replaces: Batch.from_data_list + the fc edge builder
 * (chemeleon.py:335-343, cspnet.py:319-324): node i of crystal g is global
 * node node_off[g] + i; the fully connected edges of crystal g are visited in
 * the reference's row-major (i, j) order, self loops included, but never
 * materialised as a dense N x N matrix. `max_pairs` is 1 (plain decoder
 * calls) or 2 (cond + null classifier-free-guidance pairs). */
int chm_batch_create(const chm_model* m, const int32_t* h_natoms, int num_graphs, int max_pairs, chm_batch** out);
void chm_batch_destroy(chm_batch* b);
/* Device bytes the batch uses (workspace + index tables). */
size_t chm_batch_device_bytes(const chm_batch* b);

/* Caller-owned workspace (SURVEY 8(b) Ownership): chm_batch_workspace_bytes returns the
 * device bytes a batch of these crystals needs with the model's current arithmetic (0 on bad
 * arguments), and chm_batch_create_with_workspace builds the batch inside the caller's
 * allocation d_workspace (>= that many bytes, 256-byte aligned; e.g. a block from the PyTorch
 * caching allocator). The index tables are uploaded on `stream`, which is synchronised before
 * return; the workspace must outlive the batch, and chm_batch_destroy never frees it. A batch
 * is scratch for one stream at a time: samplers that run concurrently on different streams use
 * different batches. */
size_t chm_batch_workspace_bytes(const chm_model* m, const int32_t* h_natoms, int num_graphs, int max_pairs);
int chm_batch_create_with_workspace(const chm_model* m, const int32_t* h_natoms, int num_graphs, int max_pairs,
                                    void* d_workspace, size_t workspace_bytes, void* stream, chm_batch** out);

/* Edge styles (CSPNet(edge_style=...), cspnet.py:319-343). CHM_EDGES_KNN is the reference's radius
 * graph (radius_graph_pbc + neighbour cap + symmetric reorder, data_utils.py:151-398,
 * cspnet.py:236-343; the reference needs torch_scatter's segment ops for it). Its edges depend on the
 * coordinates, so every decoder call of a knn batch rebuilds them on the device and synchronises
 * `stream` once to size the launches: knn batches cannot be captured into a graph. split16
 * arithmetic only. */
#define CHM_EDGES_FC 0
#define CHM_EDGES_KNN 1
typedef struct chm_batch_options {
  int32_t edge_style;          /* CHM_EDGES_FC (default) or CHM_EDGES_KNN */
  int32_t max_neighbors;       /* knn: max_num_neighbors_threshold (CSPNet max_neighbors, 20 in the shipped
                                  config); <= 0 keeps every pair within the radius, as the reference's
                                  get_max_neighbors_mask (data_utils.py:341-348) */
  int32_t knn_edges_per_atom;  /* knn: edge capacity per atom after symmetrisation (default 128); a
                                  decoder call whose graph has more edges fails with CHM_E_UNSUPPORTED */
  int32_t reserved;
} chm_batch_options;
/* chm_batch_workspace_bytes / chm_batch_create_with_workspace with options (NULL = fc defaults);
 * d_workspace NULL: the library allocates (as chm_batch_create). */
size_t chm_batch_workspace_bytes_ex(const chm_model* m, const int32_t* h_natoms, int num_graphs, int max_pairs,
                                    const chm_batch_options* opts);
int chm_batch_create_ex(const chm_model* m, const int32_t* h_natoms, int num_graphs, int max_pairs,
                        const chm_batch_options* opts, void* d_workspace, size_t workspace_bytes, void* stream,
                        chm_batch** out);
/* knn batches: build the edge list of these coordinates now (as a decoder call does) and copy it out,
 * grouped by source node in the reference's order within each node: d_src / d_dst [capacity] int32
 * global node indices, d_frac_diff [capacity, 3]; *n_edges = the edge count (nothing is copied when it
 * exceeds capacity). Any of the output pointers may be NULL. */
int chm_knn_edges(chm_batch* b, const float* d_frac, const float* d_lattices, int32_t* d_src, int32_t* d_dst,
                  float* d_frac_diff, int64_t capacity, int64_t* n_edges, void* stream);

/* One decoder call for `pairs` conditionings that share atom types,
 * coordinates and lattices (pairs = 1: CSPNet.forward, cspnet.py:345-405;
 * pairs = 2: the two calls of Chemeleon.model_predictions, chemeleon.py:258-285).
 *   d_atom_types [N] int64, d_frac [N,3], d_lattices [B,3,3]
 *   d_time_emb   [B,128] rows, row stride time_stride floats (0 = one row for all graphs)
 *   d_text       [pairs,B,text_dim] (row stride text_dim) or NULL if text_dim == 0
 * Outputs (any may be NULL to skip it):
 *   d_types_out [pairs,N,A], d_lattice_out [pairs,B,3,3], d_coords_out [pairs,N,3],
 *   d_node_out  [pairs,N,H] (final-LayerNorm node features). */
/* (A model created with time_dim = text_dim = 0 has no FilmLayer, cspnet.py:210-211: the reference's
 * CrystalClip graph encoder. Its parameter list omits the six film_layer.* tensors, d_time_emb may be
 * NULL, and it cannot sample.) */
int chm_decoder_forward(chm_batch* b, int pairs, const int64_t* d_atom_types, const float* d_frac,
                        const float* d_lattices, const float* d_time_emb, int time_stride, const float* d_text,
                        float* d_types_out, float* d_lattice_out, float* d_coords_out, float* d_node_out,
                        void* stream);

/* Training forward / validation loss (Chemeleon.forward, chemeleon.py:137-244) for a batch created
 * with max_pairs >= 1: q_sample of (d_a0, d_x0, d_l0) at the per-graph timesteps d_t [B] (int64,
 * 1..T) with the caller's noise (d_rand_a [N,A] uniforms, d_noise_l [B,3,3] normals already masked by
 * [[1,0,1],[1,1,1],[0,0,1]], d_noise_x [N,3] normals), one decoder call on the noised state with
 * d_time_emb [B,time_dim] and d_text [B,text_dim] (or NULL), then the D3PM hybrid loss, lattice and
 * coordinate MSEs. Tables (device fp32): d_coef4 [T+1][4] = {sqrt(abar_t), sqrt(1 - abar_t),
 * sigma_t, sigmas_norm_t}, d_q_one_step / d_q_mats [T+1][A][A] as in chm_schedule.
 * Outputs: d_out[6] = {loss, vb_loss, ce_loss, loss_atom_types, loss_lattice, loss_coords};
 * optional (NULL to skip) d_a_t [N] int64, d_x_t [N,3], d_l_t [B,3,3], d_target_x [N,3] (the score
 * target), d_pred_lattice [B,3,3], d_pred_coords [N,3]. */
typedef struct chm_train_tables {
  int T;
  const float* d_coef4;
  const float* d_q_one_step;
  const float* d_q_mats;
  float hybrid_coeff, cost_atom_types, cost_lattice, cost_coords;
} chm_train_tables;
int chm_training_loss(chm_batch* b, const chm_train_tables* tt, const int64_t* d_t, const int64_t* d_a0,
                      const float* d_x0, const float* d_l0, const float* d_time_emb, const float* d_text,
                      const float* d_rand_a, const float* d_noise_l, const float* d_noise_x, float* d_out,
                      int64_t* d_a_t, float* d_x_t, float* d_l_t, float* d_target_x, float* d_pred_lattice,
                      float* d_pred_coords, void* stream);

/* Per-timestep schedule tables (device, fp32), computed once by the host from
 * the reference schedules (diff_utils.py:57-131, chemeleon.py:413-457):
 *   d_coef [T+1][8]: {c0, c1, sigma_l, step_x, std_x, sqrt(sigma_norm),
 *                     step_lr*(sigma_t/sigma_begin)^2, sqrt(2*that)}
 *   d_time_emb [T+1][time_dim]: SinusoidalTimeEmbeddings(t) (cspnet.py:21-35)
 *   d_q_one_step, d_q_mats [T+1][A][A]: D3PM buffers (diff_utils.py:168-185)
 * num_classes (= A) and time_dim describe the tables; a step refuses a schedule
 * whose num_classes / time_dim differ from its batch's model (CHM_E_ARG). */
typedef struct {
  int T;
  int num_classes;
  int time_dim;
  int reserved;
  const float* d_coef;
  const float* d_time_emb;
  const float* d_q_one_step;
  const float* d_q_mats;
} chm_schedule;

/* The device buffers of one reverse step, each with its ELEMENT count. Every count is
 * checked against the batch (N nodes, B crystals) and its model (A = max_atoms classes,
 * text_dim) before anything is enqueued: a mis-sized buffer returns CHM_E_ARG with
 * chm_last_error() naming it, never an out-of-bounds access on the device.
 *   d_atom_types [N] int64, d_frac [N,3], d_lattices [B,3,3]: the state, updated in place;
 *   d_cond, d_null [B,text_dim]: conditioning vectors (NULL / 0 when text_dim = 0);
 *   parity-mode noise, all four or none (NULL: device Philox noise):
 *   d_rand_a [N,A] uniforms, d_rand_l [B,3,3], d_rand_x1 [N,3], d_rand_x2 [N,3] normals. */
typedef struct chm_step_io {
  int64_t* d_atom_types;
  int64_t n_atom_types;
  float* d_frac;
  int64_t n_frac;
  float* d_lattices;
  int64_t n_lattices;
  const float* d_cond;
  int64_t n_cond;
  const float* d_null;
  int64_t n_null;
  const float* d_rand_a;
  int64_t n_rand_a;
  const float* d_rand_l;
  int64_t n_rand_l;
  const float* d_rand_x1;
  int64_t n_rand_x1;
  const float* d_rand_x2;
  int64_t n_rand_x2;
} chm_step_io;

/* One reverse-diffusion step t -> t-1 of Chemeleon._sample_generator
 * (chemeleon.py:379-466): predictor CFG pair, D3PM atom-type sampling
 * (diff_utils.py:307-329), DDPM lattice update (clip at t == T), VE
 * predictor half step, corrector CFG pair, Langevin corrector, wrap to [0,1).
 * Buffers: `io` (state updated in place). With the four noise buffers the
 * host-drawn tensors of the reference's RNG stream are used (parity mode;
 * ignored at t == 1 as in the reference); without them noise comes from a
 * counter-based Philox generator keyed by (seed, t, global node / graph
 * index), so results do not depend on how samples are sharded across GPUs.
 * `node_base`/`graph_base` are the global indices of this batch's first
 * node / graph for that key. */
int chm_sample_step(chm_batch* b, const chm_schedule* sched, int t, float cond_scale, const chm_step_io* io,
                    uint64_t seed, int64_t node_base, int64_t graph_base, void* stream);

/* Graph-capturable form of chm_sample_step: t is read from device memory
 * (*d_t, int32) and decremented by the step's last kernel, so one captured
 * step (hipStreamBeginCapture ... hipGraphLaunch) replayed T times walks
 * t = T .. 1. Noise comes from the counter-based Philox generator only (the
 * noise buffers of `io` must be NULL). */
int chm_sample_step_dt(chm_batch* b, const chm_schedule* sched, int32_t* d_t, float cond_scale, const chm_step_io* io,
                       uint64_t seed, int64_t node_base, int64_t graph_base, void* stream);

/* The same with the noise read from the four fixed device buffers of `io` (required): the
 * caller refills them before every replay (the reference's CPU RNG stream drawn on the host and
 * copied in stream order), so parity-mode sampling also runs as one captured step. At t == 1 the
 * buffers are not read (their stale contents are finite uniforms / normals). */
int chm_sample_step_dt_noise(chm_batch* b, const chm_schedule* sched, int32_t* d_t, float cond_scale,
                             const chm_step_io* io, void* stream);

/* Constrained sampling (RePaint-style conditioning of the reverse loop; the reference has no counterpart: its
 * composition workflow samples freely and discards what does not match, scripts/sample_target_composition.py:57-62).
 * The caller marks atom types (per atom), fractional coordinates (per atom) and lattices (per crystal) as known.
 * After a reverse step t -> t-1 has reached level s = t - 1, the marked entries are replaced by the known clean
 * values forward-noised to level s, the q_sample of the training forward (chemeleon.py:151-180):
 *   types        a = a0 at s = 0, else argmax_d(log(q_mats[s-1][a0][d] + 1e-6) - log(-log(clamp(u[i,d], 1e-6, 1)))),
 *                the first maximum (diff_utils.py:236-256 at time s);
 *   lattices     l = (fwd[s][0] l0 + fwd[s][1] (z_l mask9)) mask9, mask9 = [[1,0,1],[1,1,1],[0,0,1]];
 *   coordinates  x = (x0 + fwd[s][2] z_x) % 1.0;
 * every product and sum rounded to fp32 in this order. All buffers are in node order of the batch, each with its
 * ELEMENT count (checked against the batch's N nodes, B crystals, A classes like chm_step_io's):
 *   d_a0 [N] int64 + d_type_mask [N] uint8 (non-zero = known), d_x0 [N,3] + d_frac_mask [N] uint8,
 *   d_l0 [B,3,3] (the model's lattice representation) + d_lattice_mask [B] uint8: each pair both given or both NULL
 *     (NULL: nothing of that field is held);
 *   d_fwd [T+1][4] = {sqrt(abar_t), sqrt(1 - abar_t), sigma_t, sigmas_norm_t} (chm_train_tables' d_coef4), n_fwd =
 *     4 (T + 1) for the schedule's T;
 *   the replacement's noise, all three or none: d_rand_a [N,A] uniforms, d_rand_l [B,3,3] normals (unmasked),
 *     d_rand_x [N,3] normals. NULL: device Philox streams of kinds 4 (types, index (node_base + i) * 128 + class),
 *     5 (lattices, (graph_base + g) * 9 + q) and 6 (coordinates, (node_base + i) * 3 + k), keyed by (seed, t) with
 *     t = s + 1, the step's t. */
typedef struct chm_constraint {
  const int64_t* d_a0;
  int64_t n_a0;
  const uint8_t* d_type_mask;
  int64_t n_type_mask;
  const float* d_x0;
  int64_t n_x0;
  const uint8_t* d_frac_mask;
  int64_t n_frac_mask;
  const float* d_l0;
  int64_t n_l0;
  const uint8_t* d_lattice_mask;
  int64_t n_lattice_mask;
  const float* d_fwd;
  int64_t n_fwd;
  const float* d_rand_a;
  int64_t n_rand_a;
  const float* d_rand_l;
  int64_t n_rand_l;
  const float* d_rand_x;
  int64_t n_rand_x;
} chm_constraint;

/* The replacement alone, in place on the state buffers of `io` (d_atom_types, d_frac, d_lattices; the other
 * fields of io are not read). `level` = s is used when d_t is NULL; otherwise s = *d_t - 1 is read on the device
 * (int32, the step's t). `what` selects the fields: bit 0 (1) types, bit 1 (2) lattices, bit 2 (4) coordinates.
 * sched supplies T, num_classes and d_q_mats. Allocates nothing and does not synchronise: legal under stream
 * capture. Every check (element counts, the pair and noise all-or-none rules, n_fwd against sched->T, level in
 * [0, T], what in [1, 7]) returns CHM_E_ARG naming the field before the first HIP call. */
int chm_constrain_state(chm_batch* b, const chm_schedule* sched, const chm_constraint* con, int level,
                        const int32_t* d_t, int what, const chm_step_io* io, uint64_t seed, int64_t node_base,
                        int64_t graph_base, void* stream);

/* chm_sample_step with a constraint (con == NULL is refused: the three entry points above are the unconstrained
 * step, unchanged). Host t is used when d_t is NULL; otherwise t is read from *d_t and decremented by the step's
 * last kernel (graph replay). The step's own noise comes from io's four buffers when given, else from Philox.
 * Order inside the step:
 *   1. predictor decoder pair, predictor updates and D3PM sampling, as chm_sample_step;
 *   2. stage 1: types, lattices and coordinates of the known entries replaced at level t - 1 (what = 7);
 *   3. corrector decoder pair, which therefore sees the known atoms where they belong at that level;
 *   4. Langevin corrector, as chm_sample_step;
 *   5. stage 2: the known coordinates written again with the same noise (what = 4), so the corrector's move on
 *      them is discarded; the free atoms keep theirs;
 *   6. decrement of *d_t.
 * A step whose constraint holds nothing of a stage's fields launches nothing for that stage. */
int chm_sample_step_con(chm_batch* b, const chm_schedule* sched, int t, int32_t* d_t, float cond_scale,
                        const chm_step_io* io, const chm_constraint* con, uint64_t seed, int64_t node_base,
                        int64_t graph_base, void* stream);

/* Standalone message-passing aggregation (scatter_mean of edge messages onto
 * their source node; chemeleon/utils/scatter.py:88-112 as called from
 * cspnet.py:155-160) over this batch's fc edge layout:
 *   d_msg [pairs,E,H] (msg_count elements) -> d_agg [pairs,N,H] (agg_count elements),
 *   agg[i] = sum_j msg[(i,j)] / max(n_g,1), H = hidden_dim (512); the counts must be
 * exactly pairs*E*H and pairs*N*H (CHM_E_ARG otherwise); fc batches only
 * (CHM_E_UNSUPPORTED for knn). */
int chm_segment_mean(chm_batch* b, int pairs, const float* d_msg, int64_t msg_count, float* d_agg, int64_t agg_count,
                     void* stream);

/* D3PM reverse sampling for explicit inputs (diff_utils.py:307-329):
 * d_logits [N,A], d_xt [N] int64, d_t [N] int64 per-node timestep,
 * d_noise [N,A] uniform -> d_out [N] int64. Tables as in chm_schedule.
 * Every t must lie in [1, T] and every x_t in [0, A) (the reference indexes its
 * tables with them and raises otherwise): the kernel checks them on the device,
 * and an out-of-range index makes the call return CHM_E_ARG with chm_last_error()
 * naming the first offending node (its d_out entry is -1). The check needs the
 * result, so this entry point synchronises `stream` before returning, except while
 * `stream` is capturing a graph: then nothing is read back and the call returns at
 * once; out-of-range nodes are the d_out entries of -1 (the flag word the check uses
 * is allocated per host thread and device by the first, uncaptured call:
 * CHM_E_UNSUPPORTED if the first call on a thread is captured). */
int chm_d3pm_sample(int N, int A, int T, const float* d_logits, const int64_t* d_xt, const int64_t* d_t,
                    const float* d_noise, const float* d_q_one_step, const float* d_q_mats, int64_t* d_out,
                    void* stream);

/* Test hooks for the perf-mode noise (the device Philox4x32-10 streams the step kernels draw
 * from; the reference draws torch.rand / torch.randn on its CPU generator instead,
 * chemeleon.py:400-404,418,435,455):
 *   chm_debug_philox: d_out[i] = uniform in [0,1) (normal = 0) or standard normal (normal = 1)
 *     of key (seed, t, kind, base + i); kind 0 atom-type uniforms, 1 lattice, 2 / 3 coordinates; 4 / 5 / 6 the
 *     constraint's atom-type uniforms, lattice and coordinate normals (chm_constraint).
 *   chm_debug_d3pm_philox: chm_d3pm_sample with the Gumbel noise drawn from that stream (kind 0,
 *     index (node_base + node) * 128 + class), as the sampler does in perf mode. */
int chm_debug_philox(uint64_t seed, int t, int kind, int64_t base, int64_t n, int normal, float* d_out, void* stream);
int chm_debug_d3pm_philox(int N, int A, int T, const float* d_logits, const int64_t* d_xt, const int64_t* d_t,
                          const float* d_q_one_step, const float* d_q_mats, uint64_t seed, int64_t node_base,
                          int64_t* d_out, void* stream);

/* Test hook: the update half of a reverse step on caller-supplied decoder outputs, by the very code
 * chm_sample_step runs behind its decoder calls (the same kernels, launched with arguments built by the same
 * function). d_types [2,N,A], d_coords [2,N,3], d_lattice [2,B,3,3]: the conditional outputs first, then the
 * null ones, as chm_decoder_forward with pairs = 2 returns them, each with its ELEMENT count; they are packed
 * into the batch's own head buffers (the batch needs max_pairs = 2).
 *   stage 1: the predictor: D3PM atom types (the two logit sets mixed by cond_scale, written in place over
 *            io->d_atom_types), the DDPM lattice update with its clip at t == T, the VE predictor half step;
 *   stage 2: the Langevin corrector and the wrap to [0, 1) on io->d_frac; d_types and d_lattice may be NULL.
 * t is the host value when d_t is NULL, else *d_t (int32) is read on the device; it is not decremented. io: the
 * state in place and the four noise buffers or none (then Philox streams 0-3 keyed by (seed, t): atom-type
 * uniforms at (node_base + i) * 128 + class, lattice normals at (graph_base + g) * 9 + q, the predictor's and
 * the corrector's coordinate normals at (node_base + i) * 3 + k); d_cond / d_null are not read. As in the step,
 * a host t == 1 reads no noise; with d_t the atom-type uniforms are read at t == 1 too and must be finite.
 * For tests only: it synchronises the stream. Every check (NULL pointers, element counts, max_pairs, stage in
 * {1, 2}, host t in [1, T], the noise all-or-none rule, the schedule's num_classes / time_dim) returns
 * CHM_E_ARG naming the field before the first HIP call, without a device. */
int chm_debug_step_update(chm_batch* b, const chm_schedule* sched, int t, const int32_t* d_t, float cond_scale,
                          const chm_step_io* io, uint64_t seed, int64_t node_base, int64_t graph_base,
                          const float* d_types, int64_t n_types, const float* d_coords, int64_t n_coords,
                          const float* d_lattice, int64_t n_lattice, int stage, void* stream);

/* Test hook: the kernels of the training forward on caller-supplied decoder outputs, by the very code
 * chm_training_loss runs around its decoder call (the same kernels, launched with arguments built by the same
 * function) and with no decoder call: q_sample of (d_a0, d_x0, d_l0) at the per-graph d_t [B] (int64, 1..T; d_a0 in
 * [0, A): neither is checked) with the caller's noise, as chm_training_loss takes it (d_noise_l already masked), then
 * the D3PM hybrid loss and the two MSEs on d_types [N,A], d_coords [N,3], d_lattice [B,3,3], each with its ELEMENT
 * count, as chm_decoder_forward with pairs = 1 returns them; they are packed into the batch's own head buffers (any
 * max_pairs). Outputs, all required: d_out[6] as chm_training_loss, d_a_t [N] int64, d_x_t [N,3], d_l_t [B,3,3],
 * d_target_x [N,3], and d_part [N,2] = each node's {KL, cross entropy}, whose means are d_out[1] and d_out[2].
 * For tests only: it synchronises the stream. Every check (NULL pointers, T >= 1, element counts) returns CHM_E_ARG
 * naming the field before the first HIP call, the ones that need no batch first, without a device. */
int chm_debug_train_update(chm_batch* b, const chm_train_tables* tt, const int64_t* d_t, const int64_t* d_a0,
                           const float* d_x0, const float* d_l0, const float* d_rand_a, const float* d_noise_l,
                           const float* d_noise_x, const float* d_types, int64_t n_types, const float* d_coords,
                           int64_t n_coords, const float* d_lattice, int64_t n_lattice, float* d_out, int64_t* d_a_t,
                           float* d_x_t, float* d_l_t, float* d_target_x, float* d_part, void* stream);

/* Test hook: one GEMM kernel of the decoder on caller-supplied fp32 device operands,
 * C[M,N] = epi(A[M,K] . W[N,K]^T), the weights packed exactly as chm_model_create packs them
 * (bf16 planes for kinds 1-3, row-scaled fp16 split rows in 16-column chunks for kind 4, in
 * 32-column chunks for kind 5). For tests only: it allocates, and synchronises the stream.
 *   kind 0 gemm (fp32 MFMA), 1 gemm_bf16x3, 2 gemm_bf16x3_big, 3 node_gemm bf16x3,
 *   4 node_gemm split16, 5 edge_gemm16 with the plain epilogue (main loop + the W-scale undo).
 *   d_A2 / lda2 / ksplit: columns k >= ksplit of A come from d_A2[:, k - ksplit] (NULL: none, and
 *     ksplit is 0 or K). Epilogue: + d_bias[n]; + d_gb[d_row2g[row % gb_rowmod]][n] for n < gb_cols;
 *     act 1 = SiLU; + d_R[row][n] (d_R may equal d_C). Kind 2 takes no gb; kind 5 no A2 and no epilogue.
 *   d_amax / d_amax2 (kind 4 only, ignored elsewhere; NULL = unscaled): per row an upper bound of
 *     max |A[row, :]| / max |A2[row, :]|, whose exponent sets the row's split scale.
 *   d_cmax (kind 4 only; NULL = skip): [M] words the caller zero-fills; receives max |C[row, :]| as float bits.
 *   tile_rows / tile_cols / blocks_per_cu (kinds 3, 4; 0 = the kernel's own choice): the node GEMM's tile
 *     variant, 64 or 128 rows, 64 or 128 columns (64: kind 4 with 64 rows), 2-4 blocks per CU as the variant has.
 *   chunk_scaled (kind 5): A is split per (row, 128-column chunk) scaled by the chunk's exponent, as edge
 *     layer 1 writes S (K % 128 == 0, K <= 512); 0: A is split unscaled, as the Fourier features are (|a| <= 1).
 * Every argument check runs before any HIP call: a shape or option the kind does not accept returns
 * CHM_E_ARG with chm_last_error() naming the field, without a device. */
typedef struct chm_debug_gemm_args {
  int32_t kind, act;
  int64_t M;
  int32_t N, K, ksplit, chunk_scaled;
  const float* d_A; int64_t lda;
  const float* d_A2; int64_t lda2;
  const float* d_W;                 /* [N][K] */
  const float* d_bias;
  const float* d_R; int64_t ldr;
  const float* d_gb; int64_t ldgb;
  const int32_t* d_row2g; int64_t gb_rowmod;
  int32_t gb_cols, tile_rows, tile_cols, blocks_per_cu;
  const float* d_amax; const float* d_amax2;
  float* d_C; int64_t ldc;
  uint32_t* d_cmax;
} chm_debug_gemm_args;
int chm_debug_gemm(const chm_debug_gemm_args* args, void* stream);

/* Test hook: the message path of CSP layer `layer` on caller operands, by the code and on the schedule a decoder
 * call on this fc batch takes (the model's math mode and options, the batch's tables):
 *   agg[c][i] = mean_j SiLU(SiLU(D f_ij + P_c[i] + Q_c[j]) W2^T + b2).
 * d_frac [N,3]: the Fourier features are written from it as the decoder writes them. d_PQ [pairs,N,2H]: per node
 * [P | Q], P already holding b1 + the per-graph term; copied into the batch's buffer. d_agg [pairs,N,H] fp32.
 * d_agg_split / d_agg_exp (both or neither; a split16 batch created with option node_ps only): the layer's output
 * as the pre-split node GEMMs read it, split rows [pairs*N][H/16][hi 16 | lo 16] fp16 (pairs*N*H*4 bytes) and per
 * row the packed int8 exponents of its four 128-column chunks; d_agg then comes from a run of the block without
 * pre-split. Clears the schedule's flag words as a decoder call does, synchronises the stream. Every argument
 * check runs before any HIP call (CHM_E_ARG / CHM_E_UNSUPPORTED naming the field, without a device); knn
 * batches are refused. */
int chm_debug_edge_layer(chm_batch* b, int pairs, int layer, const float* d_frac, int64_t n_frac, const float* d_PQ,
                         int64_t n_pq, float* d_agg, int64_t n_agg, void* d_agg_split, int32_t* d_agg_exp,
                         void* stream);

/* Test hook: the same message path on a knn batch. Builds the radius graph of d_frac [N,3] / d_lat [B,3,3] as a
 * decoder call does (the refusals of that build are returned unchanged: CHM_E_UNSUPPORTED for a node above 256
 * edges or a graph above the batch's edge capacity), writes the features of its edges (frac_diff as built, no
 * wrap), runs the layer's edge block on the node-aligned segment tiles of that graph and copies agg [pairs,N,H]
 * out; a node without edges has an all-zero row. n_lat = 9 B. Every argument check runs before any HIP call
 * (CHM_E_ARG / CHM_E_UNSUPPORTED naming the field, without a device); fc batches are refused. Synchronises the
 * stream. */
int chm_debug_knn_edge_layer(chm_batch* b, int pairs, int layer, const float* d_frac, int64_t n_frac,
                             const float* d_lat, int64_t n_lat, const float* d_PQ, int64_t n_pq, float* d_agg,
                             int64_t n_agg, void* stream);

/* Test hook: the decoder's node-side launches alone (everything of a decoder call that is neither a GEMM nor the
 * message path), by the very functions a decoder call runs them with (arguments built from the batch, its plan for
 * `pairs` conditionings and the layer), on caller operands. Every pointer carries its ELEMENT count; a nullable
 * output is skipped when NULL. fc and knn batches alike (these launches do not depend on the edges).
 *   stage 1, the conditioning input (FiLM models only): d_temb + tstride (row g at d_temb + g tstride, n_temb =
 *     (B-1) tstride + 128), or with d_t (one device int32, n_t = 1) d_temb a table of 128-wide rows read at row *d_t;
 *     d_text0 / d_text1 [B,text_dim] (text_dim > 0; d_text1 for pairs = 2) -> d_cin [pairs,B,128+text_dim].
 *   stage 2, the embedding launch and the per-graph terms: d_a [N] int64 (in [0, max_atoms): not checked), d_lat
 *     [B,3,3] -> d_Hres [pairs,N,H]; d_gbias [L,B,H], all layers (the first 16 from the embedding launch, the rest
 *     from the launches behind it); d_rmax [pairs N], max |row| (split16 batches without option node_ps); d_split
 *     [pairs N][H/16][hi 16 | lo 16] fp16 (n_split = pairs N 2H) with d_exp [pairs N], the packed int8 exponents of
 *     each row's four 128-column chunks (split16 with node_ps; both or neither); d_flags, IN and OUT, on a pair-grid
 *     plan only: the words the launch clears, in the layout and count chm_debug_node_flag_words gives, copied into
 *     the batch's words before the launch and back after it.
 *   stage 3, FiLM + residual + LayerNorm of layer `layer`: d_Y [pairs,N,H] and d_cemb [pairs,B,2H] (FiLM models;
 *     ignored without FilmLayer), d_Hres [pairs,N,H] IN and OUT, copied into the batch's buffers -> d_Hl [pairs,N,H];
 *     d_rmax [4][pairs N], the four row-max arrays (RMX_H, RMX_HL, RMX_AGG, RMX_U); d_split / d_exp: Hl's split rows.
 *   stage 4, the tail: d_Hres [pairs,N,H], d_lat, d_HO [pairs N,128] (the packed head rows) -> d_Hf [pairs,N,H] (the
 *     final LayerNorm), d_LAT [pairs,B,3,3], d_types [pairs,N,max_atoms] and d_coords [pairs,N,3] (each nullable).
 * The batch buffers a stage writes are filled with 0xff bytes before its launches. For tests only: it synchronises
 * the stream. Every check (NULL pointers, stage, pairs, layer, element counts, an output the batch's plan does not
 * write) returns CHM_E_ARG / CHM_E_UNSUPPORTED naming the field before the first HIP call, the ones that need no
 * batch first, without a device. */
typedef struct chm_debug_node_io {
  const float* d_temb; int64_t n_temb;
  const int32_t* d_t; int64_t n_t;
  int32_t tstride, reserved;
  const float* d_text0; int64_t n_text0;
  const float* d_text1; int64_t n_text1;
  float* d_cin; int64_t n_cin;
  const int64_t* d_a; int64_t n_a;
  const float* d_lat; int64_t n_lat;
  const float* d_Y; int64_t n_Y;
  const float* d_cemb; int64_t n_cemb;
  const float* d_HO; int64_t n_HO;
  float* d_Hres; int64_t n_Hres;
  float* d_gbias; int64_t n_gbias;
  float* d_Hl; int64_t n_Hl;
  float* d_rmax; int64_t n_rmax;
  void* d_split; int64_t n_split;
  int32_t* d_exp; int64_t n_exp;
  uint32_t* d_flags; int64_t n_flags;
  float* d_Hf; int64_t n_Hf;
  float* d_LAT; int64_t n_LAT;
  float* d_types; int64_t n_types;
  float* d_coords; int64_t n_coords;
} chm_debug_node_io;
int chm_debug_node_stage(chm_batch* b, int pairs, int stage, int layer, const chm_debug_node_io* io, void* stream);
/* (host only, on a created batch) the words of stage 2's d_flags for `pairs` conditionings: 128 repair-request words,
 * then the pair grid's per-layer flags, then the unused words up to the end of that buffer's allocation (a guard no
 * launch may write). Returns their count (0: the plan clears nothing, d_flags is refused; negative: CHM_E_*) and in
 * *n_cleared how many of them, from the front, the embedding launch zeroes. */
int64_t chm_debug_node_flag_words(const chm_batch* b, int pairs, int64_t* n_cleared);

/* Host-only test hook (no device): the row tiles edge layer 2 runs on for an fc batch of these
 * crystals (EdgeArgs::rtiles; DESIGN.md "Edge layer 2 on row tiles"). Returns the tile count R (or a
 * negative CHM_E_*); if out4 holds >= 4 R int32 it receives per tile {first node starting in the tile,
 * first node starting after it, the node continued from the previous tile or -1, that node's row
 * offset in the continued-rows buffer}, and *r2tot the buffer's rows. */
int chm_debug_row_tiles(const int32_t* h_natoms, int B, int32_t* out4, int64_t cap4, int64_t* r2tot);
/* (host only) the row tiles' node lists (EdgeArgs::rinfo: kRowInfo = 260 {node, packed} pairs per tile) and
 * their lengths, as edge layer 2's segment-mean epilogue reads them; returns the number of row tiles */
int chm_debug_row_nodes(const int32_t* h_natoms, int B, int32_t* out2, int64_t cap2, int32_t* counts, int64_t cap);
/* The same two on a mixed row tiling (r6): tiles [0, nbig) of 256 edge rows, then tiles of 192 rows (nbig < 0: the
 * uniform tiling; CHM_E_ARG when the 256-row tiles leave no row). A batch takes such a tiling at creation when edge
 * layer 2 runs on the two-launch schedule (fewer than the option edge_layer_min row tiles, crystals of at most 192
 * atoms, split16, option edge_rows_short on) and its last round of 256-row tiles would be at most 3/4 full: that
 * round's rows then run as one round of 192-row tiles (k_edge16_short, a launch of their own). Bit-identical.
 * chm_debug_short_row_tiles: the nbig a batch of these crystals takes for P conditionings on a device of ncu CUs with
 * edge_layer_min = layer_min (-1: uniform); chm_batch_short_row_tiles: the one a created batch took. */
int chm_debug_row_tiles_ex(const int32_t* h_natoms, int B, int64_t nbig, int32_t* out4, int64_t cap4, int64_t* r2tot);
int chm_debug_row_nodes_ex(const int32_t* h_natoms, int B, int64_t nbig, int32_t* out2, int64_t cap2, int32_t* counts,
                           int64_t cap);
int64_t chm_debug_short_row_tiles(const int32_t* h_natoms, int B, int P, int ncu, int64_t layer_min);
int64_t chm_batch_short_row_tiles(const chm_batch* b);
/* Host-only test hook: the schedule of both edge layers in one static grid on pairs (k_edge16_pairs_grid; block
 * 8 k + x runs job k of list x) for an fc batch of these crystals, P conditionings and lag `lag` (pair tiles).
 * Returns the job-list stride J (or a negative CHM_E_*); when the buffers are large enough: rng [2 R] = per
 * layer-2 row tile the pair tiles [lo, hi] it reads, pa / pb [8] = list x's pair tiles [pa, pb), njobs [8],
 * jobs [8][J][2] = {kind
 * (1 pair, 2 layer 2), tile index (pair tile * 2 + column tile; (row tile * P + conditioning) * 2 + column
 * tile)}. */
int64_t chm_debug_pair_plan(const int32_t* h_natoms, int B, int P, int lag, int32_t* rng, int64_t cap_rng, int32_t* pa,
                            int32_t* pb, int32_t* njobs, int32_t* jobs, int64_t cap_jobs);
/* Host-only test hook: per pair tile (128 unordered pairs i <= j of an fc batch, crystal-major) the node range
 * [out[2k], out[2k] + out[2k+1]) whose P / Q rows its epilogue stages in LDS (edge layer 1 on pairs). Returns the
 * number of pair tiles (or a negative CHM_E_*); out is filled when cap >= 2 x that number. */
int64_t chm_debug_pair_nodes(const int32_t* h_natoms, int B, int32_t* out, int64_t cap);
/* Fourier edge features of this batch's fc edges (cspnet.py:38-52,324):
 * d_frac [N,3] -> d_feat [E, 6*num_freqs]. */
int chm_edge_features(chm_batch* b, const float* d_frac, float* d_feat, void* stream);
/* The same features in the form the split16 edge GEMM consumes (the sampler's k_fourier_h):
 * d_split [E, 6*num_freqs/32, 2, 32] fp16, per 32-column chunk the hi parts then the lo parts
 * (feature = hi + lo, |lo| <= 2^-11 |hi|); E * 6*num_freqs * 4 bytes. */
int chm_edge_features_split(chm_batch* b, const float* d_frac, void* d_split, void* stream);

/* Bench instrumentation: while enabled, the runtime brackets every launch of
 * the kernels below with HIP events on the launch stream (a pool of 8192
 * pairs; recording stops when it is exhausted). After synchronising the
 * device, chm_prof_read returns the launch count and summed duration.
 * Launches made while the stream is being captured into a graph are not
 * instrumented (time a graph by replaying it; time kernels eagerly).
 *   CHM_K_EDGE_FOURIER  edge layer 1 (Fourier projection + node terms + SiLU)
 *   CHM_K_EDGE_MESSAGE  edge layer 2 (message GEMM + SiLU)
 *   CHM_K_SEGMENT_MEAN  message-passing aggregation (scatter_mean)
 *   CHM_K_DECODER       one whole decoder call (all its kernels)
 *   CHM_K_EDGE_LAYER    both edge layers of a CSP layer in one grid (k_edge16_pairs_grid + its repair pair) */
#define CHM_K_EDGE_FOURIER 0
#define CHM_K_EDGE_MESSAGE 1
#define CHM_K_SEGMENT_MEAN 2
#define CHM_K_DECODER 3
#define CHM_K_EDGE_LAYER 4
int chm_prof_enable(int on);
int chm_prof_reset(void);
int chm_prof_read(int kernel, int64_t* launches, double* total_ms);
/* Health counters of the edge kernels, counted on the device over every launch and graph replay
 * since the last chm_prof_events_reset (synchronous device reads; not while capturing):
 *   out[CHM_EV_LAYER_TIMEOUT]  pair grid: layer-2 jobs whose wait for their pair tiles timed out
 *   out[CHM_EV_LAYER_XCD]      pair grid: layer-2 jobs whose pair tiles ran on another XCD
 *   out[CHM_EV_LAYER_REPAIR]   pair-grid launches recomputed by their repair pair
 *   out[CHM_EV_TAIL_TIMEOUT], out[CHM_EV_TAIL_REPAIR], out[CHM_EV_LAYER_INCOMPLETE]: reserved, always 0 (they
 *                              counted the tail grid and the persistent one-grid kernel, both removed)
 * Results never depend on these (a raised check is repaired before the layer's output is used); a
 * non-zero count means the run paid for the repairs. n <= 8 values are written. */
#define CHM_EV_LAYER_TIMEOUT 0
#define CHM_EV_LAYER_XCD 1
#define CHM_EV_LAYER_REPAIR 2
#define CHM_EV_TAIL_TIMEOUT 3
#define CHM_EV_TAIL_REPAIR 4
#define CHM_EV_LAYER_INCOMPLETE 5
int chm_prof_events(int64_t* out, int n);
int chm_prof_events_reset(void);

/* Host-only (no device): parity-mode atom-type noise for a shard of a sample-parallel run. Continues
 * the MT19937 stream of the CPU torch generator (state[624], left, next as in ATen's
 * mt19937_engine, i.e. the words of torch.Generator.get_state()) over `count` float uniforms, the
 * stream torch.rand(count) draws (chemeleon.py:400-404: one 32-bit output y per element,
 * (y & (2^24 - 1)) * 2^-24), and writes only elements [lo, hi) to out[hi - lo]. state / left / next
 * are advanced in place. Replaces, per rank: torch.rand(N, A)[rows of this shard]. */
int chm_mt19937_uniform(uint32_t* state, int32_t* left, int32_t* next, int64_t count, int64_t lo, int64_t hi,
                        float* out);

/* Snapshot of the sampler state in output order: what schema.step_to_atoms (the reference's
 * TrajectoryContainer.get_atoms, schema.py:57-83) builds per crystal, made on the device so that streaming
 * output copies one packed buffer per step and the host builds the structures by slicing.
 *   numbers: classes outside [0, 103] become 0 (the reference clamps classes above 103; negative classes,
 *     which the sampler never produces and the host path would index from the end of the symbol table, also
 *     become 0);
 *   order: within each crystal the atoms stand in STABLE order of chemical symbol (ase.build.tools.sort).
 *     The key is h_rank[number], a table of n_rank = 104 entries < 104 that the caller derives from its
 *     symbol table (string order, not atomic-number order: H < He, C < Ca < Cl; class 0 is X).
 * The plan holds the crystals' node offsets and the rank table on the current device; it is independent of
 * chm_model / chm_batch, so it also serves a batch gathered from several ranks. Any natoms >= 1 per crystal;
 * more than 2^31 - 1 atoms in all return CHM_E_UNSUPPORTED. Bad arguments (NULL pointers, n_rank != 104,
 * num_graphs <= 0, a natoms entry <= 0) return CHM_E_ARG before the device is touched.
 * Slot layout (N atoms, B crystals; byte offsets):
 *   0            lattices f32 [B*9]
 *   36 B         frac     f32 [N*3], sorted
 *   36 B + 12 N  perm     i32 [N]: the source atom's index inside its crystal, per sorted row
 *   36 B + 16 N  numbers  u8  [N], sorted
 * and the slot's size is 36 B + 17 N rounded up to a multiple of 16 bytes: the plan's slot_bytes (0 for a
 * NULL plan). The run takes every buffer with its element count (the slot with its byte count, which must
 * equal slot_bytes, at a 16-byte aligned address); a mismatch returns CHM_E_ARG naming the buffer and nothing
 * is enqueued. It allocates nothing and does not synchronise: legal under stream capture. */
typedef struct chm_snapshot chm_snapshot;
int chm_snapshot_create(const int32_t* h_natoms, int num_graphs, const uint8_t* h_rank, int n_rank,
                        chm_snapshot** out);
void chm_snapshot_destroy(chm_snapshot* plan);
size_t chm_snapshot_slot_bytes(const chm_snapshot* plan);
int chm_snapshot_run(const chm_snapshot* plan, const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac,
                     int64_t n_frac, const float* d_lattices, int64_t n_lattices, void* d_slot, size_t slot_bytes,
                     void* stream);

/* Screening of finished structures on the device: what the reference's scripts do on the host with pymatgen
 * before anything else looks at a sample (test_valid, scripts/evaluate.py: the longest cell edge at most 60 A
 * and the shortest interatomic distance under periodic boundaries at least 0.5 A; the composition filter of
 * scripts/sample_target_composition.py: the reduced formula is the one asked for). One record per crystal:
 *   a, b, c              lengths of lattice rows 0, 1, 2 (A)
 *   alpha, beta, gamma   angles in degrees between rows 1-2, rows 0-2, rows 0-1 (90 where a row is zero)
 *   volume               |det|
 *   dmin                 the shortest distance (A) over atom pairs i < j and ALL lattice translations; +inf for
 *                        a one-atom crystal
 *   i_min, j_min         indices inside the crystal of a pair that attains dmin (-1, -1 for one atom); ties go
 *                        to the smallest squared distance first, then the smallest i, then the smallest j
 *   formula_units        gcd of the non-zero element counts
 *   flags                CHM_SCREEN_* bits; the structure passes when flags == 0
 * Classes are clamped as in the snapshot (outside [0, 103] -> 0), and class 0 (X) counts as an element of its
 * own, so a crystal that still holds one never matches a target.
 * dmin is exact for any cell, not only over the 27 neighbouring cells: a first pass over the fractional
 * differences wrapped to [-0.5, 0.5] and their 27 images gives an upper bound d0; a closer image lies within
 * |n_k| <= 0.5 + d0 / h_k of the wrapped difference (h_k = volume / |L_{k+1} x L_{k+2}|, the spacing of the
 * lattice planes along axis k), and where that range exceeds 1 on some axis a second pass searches it, up to 4
 * per axis. A crystal that needs more (or whose volume is not > 0) gets CHM_SCREEN_DEGENERATE and dmin holds
 * the capped search's value. Arithmetic is fp32, every product and sum rounded on its own.
 * One deliberate difference from the reference's np.min(dist_mat[dist_mat > 0]): exactly coincident atoms are
 * not ignored, they give dmin = 0 and fail the screen.
 * d_target: the wanted REDUCED element counts (gcd 1), int32: NULL with n_target = 0 (no composition check),
 * [104] for every crystal, or [B*104] per crystal. The plan holds the crystals' node offsets on the current
 * device; create refuses bad arguments (NULL pointers, num_graphs <= 0, a natoms entry <= 0) with CHM_E_ARG
 * before the device is touched. The run takes every buffer with its element count (the records with their
 * byte count, 64 per crystal, at a 16-byte aligned address); a mismatch, or a threshold that is not > 0,
 * returns CHM_E_ARG naming the buffer and nothing is enqueued. It allocates nothing, clears nothing and does
 * not synchronise: legal under stream capture. */
#define CHM_SCREEN_TOO_LONG 1     /* the longest edge > max_length */
#define CHM_SCREEN_TOO_CLOSE 2    /* dmin < min_distance */
#define CHM_SCREEN_COMPOSITION 4  /* reduced counts != target (only with a target) */
#define CHM_SCREEN_DEGENERATE 8   /* image range capped, or volume not > 0 */
#define CHM_SCREEN_NONFINITE 16   /* a non-finite lattice entry or coordinate */
typedef struct {
  float a, b, c;
  float alpha, beta, gamma;
  float volume;
  float dmin;
  int32_t i_min, j_min;
  int32_t formula_units;
  int32_t flags;
  int32_t reserved[4]; /* written as 0 */
} chm_screen_record;   /* 64 bytes */
typedef struct chm_screen chm_screen;
int chm_screen_create(const int32_t* h_natoms, int num_graphs, chm_screen** out);
void chm_screen_destroy(chm_screen* plan);
int chm_screen_run(const chm_screen* plan, const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac,
                   int64_t n_frac, const float* d_lattices, int64_t n_lattices, const int32_t* d_target,
                   int64_t n_target, float max_length, float min_distance, void* d_out, size_t n_out_bytes,
                   void* stream);

/* Grouping of duplicate structures on the device: the third leg of the reference's sample -> validity ->
 * uniqueness workflows (test_unique of scripts/evaluate.py and the grouping of
 * scripts/navigate_chemical_system.py, both StructureMatcher().group_structures on the host). This is NOT a port
 * of pymatgen's StructureMatcher: two crystals are duplicates when their reduced element counts are equal and
 * their fingerprints are close; how that criterion agrees with the matcher has not been measured.
 *
 * The fingerprint of a crystal with n atoms, classes z_i (clamped as in the screen: outside [0, 103] -> 0),
 * fractional coordinates x_i and lattice L (rows are vectors, Cartesian = frac . L) is a smooth radial
 * distribution per atom in C = 2 channels of K bins, bin centres r_k = (k + 0.5) r_cut / K:
 *   F[c][k] = (1/n) sum_i sum_j sum_R  w_c(i,j) exp(-(d - r_k)^2 / (2 sigma^2)) (1/2)(1 + cos(pi d / r_cut))
 *             over every lattice translation R with d = |(x_j - x_i + R) L| <= r_cut, except (i = j, R = 0),
 *             and only into the bins with |d - r_k| <= 6 sigma
 *   w_0 = 1,  w_1 = z_i z_j / zbar^2,  zbar = the crystal's mean class (zbar = 0: channel 1 is all zeros)
 * stored as fp[2K] = channel 0's K bins, then channel 1's. The support of 6 sigma is part of the definition: a
 * dropped term is below exp(-18) = 1.5e-8 of the pair's weight, while the same pair adds at least 0.95 of its
 * weight to its nearest bin at the defaults (K = 64, r_cut = 6.0, sigma = 0.15: the nearest centre is within
 * 0.31 sigma), so what is dropped is less than half an fp32 ulp (2^-24 = 6.0e-8) of what is kept. The taper makes F
 * continuous in the coordinates (a pair that crosses r_cut contributes nothing there). F is intensive and
 * invariant under atom permutation, a common translation, rotation, any unimodular change of the lattice basis
 * and the choice of supercell: the same crystal written with 6 or with 12 atoms has the same fingerprint.
 * Images: the difference x_j - x_i is wrapped to [-0.5, 0.5] and the translations |R_k| <= 0.5 + r_cut / h_k
 * (widened by 1e-5; h_k = volume / |L_{k+1} x L_{k+2}| as in the screen) are searched, at most 8 per axis. A
 * crystal that needs more, or whose volume is not > 0, gets CHM_DEDUP_DEGENERATE; one with a non-finite lattice
 * entry or coordinate CHM_DEDUP_NONFINITE. A flagged crystal's fingerprint is all zeros and it is never grouped.
 * Arithmetic is fp32 with accurate expf / cosf / sqrtf, every product and sum rounded on its own (no
 * contraction): d as in the screen, t = d - r_k, term = (expf(-(t t) / (2 sigma^2)) taper) [z_i z_j], summed
 * per bin in a fixed order that depends on the crystal alone (no float atomics), then channel 0 divided by n
 * and channel 1 multiplied by n / (sum_i z_i)^2. Two runs, and a crystal alone or inside any batch, give the
 * same bits. counts[104] are the crystal's element counts divided by their gcd (the screen's formula
 * reduction); compositions are compared by integer equality only.
 *
 * Grouping takes free-standing fingerprints ([B, 2K], with counts [B,104] and optionally flags [B] and an
 * exclusion mask of B bytes), so the union of several fingerprint calls (several cell sizes) groups as one
 * list. Crystals g < h match when neither is flagged or excluded, their counts are equal and
 *   |F_g - F_h|^2 <= tol^2 max(|F_g|^2, |F_h|^2)         (fp32, each sum over the 2K entries in order)
 * and groups follow the leader rule of group_structures: in index order, g is a representative when it matches
 * no earlier representative, otherwise it joins the earliest representative it matches (not transitive, on
 * purpose). group[g] is the representative's index (g itself for a representative), or -1 for a flagged or
 * excluded crystal; count[g] is the group's size at a representative, 0 elsewhere.
 * The plan holds the crystals' node offsets on the current device (create: as the screen's). Both run calls
 * take every buffer with its element count (the workspace with its byte count, at a 4-byte aligned address);
 * NULL pointers, B <= 0, K outside [8, 256], an r_cut, sigma or tol that is not positive and finite, a
 * mismatched count or a short workspace return CHM_E_ARG naming the argument before the first HIP call, and
 * nothing is enqueued. They allocate nothing and do not synchronise: legal under stream capture.
 * d_flags (n_flags = 0 or B) and d_exclude (n_exclude = 0 or B) may be NULL with a count of 0. */
#define CHM_DEDUP_DEGENERATE 8   /* image range capped, or volume not > 0 */
#define CHM_DEDUP_NONFINITE 16   /* a non-finite lattice entry or coordinate */
typedef struct chm_dedup chm_dedup;
int chm_dedup_create(const int32_t* h_natoms, int num_graphs, chm_dedup** out);
void chm_dedup_destroy(chm_dedup* plan);
int chm_dedup_fingerprint(const chm_dedup* plan, const int64_t* d_atom_types, int64_t n_atom_types,
                          const float* d_frac, int64_t n_frac, const float* d_lattices, int64_t n_lattices, int K,
                          float r_cut, float sigma, float* d_fp, int64_t n_fp, int32_t* d_counts, int64_t n_counts,
                          int32_t* d_flags, int64_t n_flags, void* stream);
size_t chm_dedup_workspace_bytes(int64_t B);
int chm_dedup_group(int64_t B, int K, const float* d_fp, int64_t n_fp, const int32_t* d_counts, int64_t n_counts,
                    const int32_t* d_flags, int64_t n_flags, const uint8_t* d_exclude, int64_t n_exclude, float tol,
                    int32_t* d_group, int64_t n_group, int32_t* d_count, int64_t n_count, void* d_workspace,
                    size_t workspace_bytes, void* stream);

/* Lattice system and reduced cell of finished structures on the device: what test_lattice_system_matching of the
 * reference's scripts/evaluate.py asks of pymatgen / spglib on the host (the structure's atoms replaced by one
 * H, SpacegroupAnalyzer(symprec=0.1, angle_tolerance=10).get_lattice_type()), so a question about the lattice
 * alone. This is NOT a port of spglib: the definition below is this library's own, and how far the two agree
 * on real samples has not been measured. The crystal system with the atoms is chm_symm_*, below.
 * Lattices are row vectors (Cartesian = frac . L).
 *
 * Reduction. Niggli reduction (Krivy-Gruber, steps A1-A8 with the epsilon rules of Grosse-Kunstleve et al.) of
 * each lattice: Lr = T L with T integer and det T = +1 (the handedness is kept). The comparisons are between
 * squared lengths and use eps = 1e-5 V^(2/3). Where an off-diagonal term exceeds its diagonal one (|2 b.c| > b.b
 * + eps in A5, likewise A6, A7) the step subtracts the whole multiple rint(b.c / b.b) at once, so that a cell
 * sheared by k rows takes one pass and not k; on the boundary cases it takes the published unit step. It runs in
 * fp64 on one lane; the rows are recomputed as T L from the input in every pass, each entry (t0 l0 + t1 l1) +
 * t2 l2, so nothing drifts. At most 100 passes, and no entry of T beyond +-32 767 (a step that would exceed it is
 * not taken): a cell that is not finished then keeps what it has and gets CHM_CELL_NOT_REDUCED. Lr is rounded to
 * fp32 once; that fp32 cell is what the record describes, what the search runs on and what chm_cell_apply
 * returns.
 *
 * Search. Every W with entries in {-1, 0, 1} and |det W| = 1 (6 960 of the 3^9 = 19 683 candidates; candidate
 * index = sum_q (W[q] + 1) 3^q over the row-major entries q). With L' = W Lr, W is accepted when every row
 * length of L' differs from Lr's by at most symprec (A) and every inter-row angle by at most angle_tolerance
 * (degrees). fp32, every product and sum rounded on its own, L' entries (w0 l0 + w1 l1) + w2 l2, lengths and
 * angles as in the screen (accurate sqrtf / acosf).
 *
 * Classification. n = the size of the accepted set; among its det = +1 members n2, n3, n4, n6 = the counts with
 * trace -1, 0, 1, 2 (rotations of order 2, 3, 4, 6). (n, n2, n3, n4, n6) =
 *   (2,0,0,0,0) triclinic   (4,1,0,0,0) monoclinic   (8,3,0,0,0) orthorhombic   (16,5,0,2,0) tetragonal
 *   (12,3,2,0,0) rhombohedral   (24,7,2,0,2) hexagonal   (48,9,8,6,0) cubic
 * Any other tuple means that the tolerant set is not a group: both tolerances are halved (exactly, in fp32) and
 * the search runs again, at most 4 halvings; a cell that still matches nothing gets CHM_CELL_AMBIGUOUS and
 * system -1, with the counts of the last level. The counts are integer sums: two runs, and a crystal alone or
 * inside any batch, give the same bytes.
 *
 * Flags. CHM_CELL_NONFINITE: a non-finite lattice entry; CHM_CELL_DEGENERATE: |det L| (fp64) not > 0. Both skip
 * the reduction and the search: system -1, T = identity, counts 0, and the lengths, angles and volume are the
 * input cell's as in the screen (90 degrees where a row is zero). CHM_CELL_NOT_REDUCED skips the search too: the
 * candidates W reach a lattice's symmetries only from a reduced basis, so an unreduced cell gets system -1 and
 * counts 0 rather than a lower system than it has; its record describes T L for the T it reached. CHM_CELL_MISMATCH: a required system was
 * given and the crystal's system (also -1) is another.
 * d_require: the wanted system codes, int32: NULL with n_require = 0 (no requirement), [1] for every crystal,
 * or [B] per crystal.
 *
 * chm_cell_apply writes, for the records of a run, the reduced lattices T L ([B,3,3], the bits the search saw)
 * and per atom x' = frac(x adj(T)) in [0, 1) (adj(T) = T^-1 exactly since det T = 1, formed in 64-bit integers;
 * fp64, rounded once) into
 * caller buffers that must not be the inputs: the sampler's state is never changed in place.
 * The plan holds the crystals' node offsets on the current device (create: as the screen's). run and apply take
 * every buffer with its element count (the records with their byte count, 128 per crystal, 16-byte aligned);
 * a NULL pointer, a mismatched count, symprec outside (0, 1] or angle_tolerance outside (0, 30] returns
 * CHM_E_ARG naming the argument before the first HIP call and nothing is enqueued. They allocate nothing and do
 * not synchronise: legal under stream capture. */
#define CHM_CELL_TRICLINIC 0
#define CHM_CELL_MONOCLINIC 1
#define CHM_CELL_ORTHORHOMBIC 2
#define CHM_CELL_TETRAGONAL 3
#define CHM_CELL_RHOMBOHEDRAL 4
#define CHM_CELL_HEXAGONAL 5
#define CHM_CELL_CUBIC 6
#define CHM_CELL_AMBIGUOUS 1     /* no holohedry matched after 4 halvings */
#define CHM_CELL_MISMATCH 2      /* system != the required one (only with d_require) */
#define CHM_CELL_NOT_REDUCED 4   /* the reduction hit its cap (100 passes, |T| entries 32 767): no system */
#define CHM_CELL_DEGENERATE 8    /* volume not > 0 */
#define CHM_CELL_NONFINITE 16    /* a non-finite lattice entry */
#define CHM_CELL_MAX_SYMPREC 1.0f
#define CHM_CELL_MAX_ANGLE_TOLERANCE 30.0f
typedef struct {
  float a, b, c;              /* lengths of the reduced rows, ascending (A) */
  float alpha, beta, gamma;   /* angles in degrees between rows 1-2, 0-2, 0-1 */
  float volume;               /* |det| of the reduced cell */
  float reserved0;            /* written as 0 */
  int32_t transform[9];       /* T, row-major: Lr = T L */
  int32_t n_ops;              /* n */
  int32_t n2, n3, n4, n6;
  int32_t system;             /* CHM_CELL_TRICLINIC .. CHM_CELL_CUBIC, or -1 */
  int32_t halvings;           /* halvings used, 0..4 */
  int32_t flags;              /* CHM_CELL_* bits */
  int32_t passes;             /* passes of the reduction */
  int32_t reserved[6];        /* written as 0 */
} chm_cell_record;            /* 128 bytes */
typedef struct chm_cell chm_cell;
int chm_cell_create(const int32_t* h_natoms, int num_graphs, chm_cell** out);
void chm_cell_destroy(chm_cell* plan);
int chm_cell_run(const chm_cell* plan, const float* d_lattices, int64_t n_lattices, const int32_t* d_require,
                 int64_t n_require, float symprec, float angle_tolerance, void* d_out, size_t n_out_bytes,
                 void* stream);
int chm_cell_apply(const chm_cell* plan, const void* d_records, size_t n_record_bytes, const float* d_frac,
                   int64_t n_frac, const float* d_lattices, int64_t n_lattices, float* d_frac_out,
                   int64_t n_frac_out, float* d_lattices_out, int64_t n_lattices_out, void* stream);

/* Crystal system with the atoms of finished structures on the device: what test_crystal_system_matching of the
 * reference's scripts/evaluate.py asks of pymatgen / spglib on the host
 * (SpacegroupAnalyzer(st, symprec=0.1, angle_tolerance=10).get_crystal_system()). This is NOT a port of spglib:
 * the definition below is this library's own, and how far the two agree on real samples has not been measured.
 *
 * Input per crystal. The state (atom_types int64 [N], compared as their low 32 bits; frac fp32 [N,3]; lattices
 * fp32 [B,3,3]) and the crystal's chm_cell_record from a run of chm_cell_run on the same lattices with the same
 * symprec and angle_tolerance. The record supplies T, system, halvings, n_ops and flags.
 *
 * Basis. Lr = T L and x' = frac(x adj(T)) are exactly what chm_cell_apply produces, with the same bits (the same
 * device code).
 *
 * Lattice operations. The set {W} is what the cell search accepted at the record's final level: tolerances
 * symprec 2^-halvings and angle_tolerance 2^-halvings of the cell record, the same candidates in the same order,
 * the same fp32 arithmetic (the same device function). A record with system < 0 (flagged or ambiguous), or whose
 * n_ops is not the size of the set found again (a record of other lattices or tolerances), gets
 * CHM_SYMM_NO_LATTICE, system -1, lattice_system -1, counts 0, tol 0.
 *
 * Action. W with L' = W Lr acts on fractional row vectors as x -> x W + t, component k being
 * (x0 W[0][k] + x1 W[1][k]) + x2 W[2][k].
 *
 * Pivot. The pivot species is the atom type with the fewest atoms in the crystal, ties to the smallest type
 * value; the pivot atom p is its first atom in node order. For each W the candidate translations are
 * t_j = x'_j - x'_p W, one for every atom j of the pivot species in node order (n_pivot of them), not wrapped.
 *
 * Acceptance. (W, t_j) is accepted at tolerance tol when every atom i has an atom k of the same type with
 * d = (x'_i W + t_j) - x'_k, d -= rintf(d) per component, c = d Lr with entries (d0 l0 + d1 l1) + d2 l2, and
 * (c0 c0 + c1 c1) + c2 c2 <= tol tol. All fp32, every product and sum rounded on its own, no contraction.
 *
 * Thin cells. One image per component is exact only while 2 tol is below the smallest plane spacing of Lr. With
 * rows a0, a1, a2: c0 = a1 x a2, c1 = a2 x a0, c2 = a0 x a1 (each component u v - w z of two rounded products),
 * V = |(a0[0] c0[0] + a0[1] c0[1]) + a0[2] c0[2]|, spacing_i = V / sqrtf((ci[0] ci[0] + ci[1] ci[1]) + ci[2] ci[2]),
 * all fp32. A crystal where not 2 symprec < fminf(fminf(spacing_0, spacing_1), spacing_2) gets CHM_SYMM_THIN, system -1,
 * counts 0 and tol = symprec: wrong answers on needle cells are worse than none.
 *
 * Counts, from the accepted set: n_sym accepted pairs; n_trans pairs with W = I (>= 1 for finite coordinates);
 * n_pg distinct W with at least one accepted translation; inversion, whether -I is among them; n_proper = m, the
 * number of distinct proper parts det(W) W of those W, and n2, n3, n4, n6 = how many of the proper parts have
 * trace -1, 0, 1, 2. The tuple (m, n2, n3, n4, n6) names the rotation group of the Laue class, hence the system:
 *   (1,0,0,0,0) 1 triclinic      (2,1,0,0,0) 2 monoclinic      (4,3,0,0,0) 222 orthorhombic
 *   (4,1,0,2,0) 4 tetragonal     (8,5,0,2,0) 422 tetragonal    (3,0,2,0,0) 3 trigonal     (6,3,2,0,0) 32 trigonal
 *   (6,1,2,0,2) 6 hexagonal      (12,7,2,0,2) 622 hexagonal    (12,3,8,0,0) 23 cubic      (24,9,8,6,0) 432 cubic
 * The set counts as a group only if the tuple is in the table, n_sym == n_pg n_trans and
 * n_pg == m (1 + inversion). Otherwise tol is halved (exactly, in fp32; it starts at symprec) and the atom search
 * runs again on the same {W}, at most 4 halvings; after the last the crystal gets CHM_SYMM_AMBIGUOUS and system
 * -1, with the last level's counts. The names are pymatgen's: code 4 is "trigonal" here, while the same code of
 * the lattice (CHM_CELL_RHOMBOHEDRAL) is "rhombohedral": a trigonal crystal may sit on a hexagonal lattice.
 * All counts are integer sums: two runs, and a crystal alone or inside any batch, give the same bytes.
 *
 * Deliberately not built: the reduction to a primitive cell. When n_trans > 1 the answer describes the cell as
 * given, so a supercell whose lattice has lower symmetry than the primitive lattice (a 2x1x1 cell of CsCl)
 * reports the lower system (tetragonal); n_trans is in the record so that a caller can tell. The way round it is
 * chm_prim_*, below: run it first and give this run the primitive cells. The space-group number and the point
 * group's name are not built either.
 *
 * CHM_SYMM_MISMATCH and d_require work as in the cell run, with crystal-system codes. The optional second output
 * d_ops (may be NULL with n_ops_bytes = 0) holds CHM_SYMM_MAX_OPS slots of 16 bytes per crystal: int32 candidate
 * index (as in the cell search) and float t[3]; one slot per distinct accepted W of the deciding level, in
 * ascending candidate index, with that W's first accepted translation in pivot order; unused slots hold index -1
 * and zeros. The plan holds the node offsets on the current device (create: as the cell's; a crystal of more than
 * 256 atoms does not fit the staging and is refused with CHM_E_UNSUPPORTED). The run takes every buffer with its
 * count (cell records 128 bytes, out 64 bytes per crystal, both and d_ops 16-byte aligned); a NULL pointer, a
 * mismatched count or tolerances outside the cell run's limits return CHM_E_ARG naming the argument before the
 * first HIP call and nothing is enqueued. It allocates nothing and does not synchronise: legal under stream
 * capture. */
#define CHM_SYMM_TRICLINIC 0
#define CHM_SYMM_MONOCLINIC 1
#define CHM_SYMM_ORTHORHOMBIC 2
#define CHM_SYMM_TETRAGONAL 3
#define CHM_SYMM_TRIGONAL 4
#define CHM_SYMM_HEXAGONAL 5
#define CHM_SYMM_CUBIC 6
#define CHM_SYMM_AMBIGUOUS 1     /* no group matched after 4 halvings */
#define CHM_SYMM_MISMATCH 2      /* system != the required one (only with d_require) */
#define CHM_SYMM_NO_LATTICE 4    /* the cell record has no lattice system (or is not this lattice's) */
#define CHM_SYMM_THIN 8          /* 2 symprec is not below the smallest plane spacing of the reduced cell */
#define CHM_SYMM_MAX_OPS 48
typedef struct {
  int32_t system;             /* CHM_SYMM_TRICLINIC .. CHM_SYMM_CUBIC, or -1 */
  int32_t n_sym;              /* accepted (W, t) pairs */
  int32_t n_trans;            /* pure translations among them */
  int32_t n_pg;               /* distinct W with a translation */
  int32_t n_proper;           /* m */
  int32_t n2, n3, n4, n6;
  int32_t inversion;          /* 1 if -I is in the point group */
  int32_t halvings;           /* halvings of tol used, 0..4 */
  int32_t flags;              /* CHM_SYMM_* bits */
  int32_t n_pivot;            /* atoms of the pivot species */
  int32_t lattice_system;     /* copied from the cell record (-1 with CHM_SYMM_NO_LATTICE) */
  float tol;                  /* the tolerance of the level that decided */
  int32_t reserved;           /* written as 0 */
} chm_symm_record;            /* 64 bytes */
typedef struct chm_symm chm_symm;
int chm_symm_create(const int32_t* h_natoms, int num_graphs, chm_symm** out);
void chm_symm_destroy(chm_symm* plan);
int chm_symm_run(const chm_symm* plan, const void* d_cell_records, size_t n_record_bytes, const int64_t* d_atom_types,
                 int64_t n_atom_types, const float* d_frac, int64_t n_frac, const float* d_lattices,
                 int64_t n_lattices, const int32_t* d_require, int64_t n_require, float symprec,
                 float angle_tolerance, void* d_out, size_t n_out_bytes, void* d_ops, size_t n_ops_bytes,
                 void* stream);

/* Primitive cells of finished structures on the device: the pure translations that chm_symm_* counts as n_trans
 * are used to reduce every crystal to a primitive cell, so that the symmetry, matching and grouping legs can be
 * given primitive cells (a sampler asked for 8 atoms of a 2-atom compound returns supercells routinely). This is
 * NOT a port of spglib's find_primitive: the definition below is this library's own, and how far the two agree
 * on real samples has not been measured.
 *
 * Input per crystal: that of the symmetry run (the state, and the crystal's chm_cell_record from chm_cell_run on
 * the same lattices with the same symprec and angle_tolerance).
 *
 * Basis. Lr = T L and x' = frac(x adj(T)), the bits of chm_cell_apply (the same device code). CHM_PRIM_NO_LATTICE
 * and CHM_PRIM_THIN are set by the rules of CHM_SYMM_NO_LATTICE and CHM_SYMM_THIN, word for word.
 *
 * Pivot and candidates. The pivot atom p is chosen as in chm_symm_* (the first atom of the rarest species, ties to
 * the smallest type); the candidate translations are t_j = x'_j - x'_p, j over that species in node order
 * (n_pivot of them), not wrapped.
 *
 * Acceptance. t_j is accepted at tolerance tol when every atom i has an atom k of its type with
 * d = (x'_i + t_j) - x'_k, d -= rintf(d) per component, c = d Lr, (c0 c0 + c1 c1) + c2 c2 <= tol tol: the
 * acceptance test of chm_symm_* with W = I, the same device function, fp32, every operation rounded on its own.
 * partner(i, j) is the lowest node index k among the atoms of i's type that pass this test.
 *
 * Group, in integers. m = the number of accepted translations. q_j = rintf((float)m t_j) mod m per component (into
 * [0, m)), an integer triple per accepted j. Lambda = the Z-span of all q_j together with m e_0, m e_1, m e_2, and
 * H = Lambda's row Hermite normal form: upper triangular, positive diagonal, 0 <= H[i][k] < H[k][k] for i < k.
 * H is unique, so the order in which the q_j are reduced cannot show. It is computed on one lane in 64-bit
 * integers.
 *
 * Consistency. The accepted set is consistent at tol when (a) m divides every species' atom count, (b)
 * det H == m m (the translations are a group of order m), (c) every t_j lies within tol of q_j / m (the distance
 * test above between t_j and the fp32 quotients (float)q / (float)m), and (d) exactly n / m atoms i have no
 * partner(i, j) < i over the accepted j. Otherwise tol is halved (exactly, in fp32; it starts at symprec) and the
 * search runs again, at most 4 halvings; after the last the crystal gets CHM_PRIM_AMBIGUOUS.
 *
 * Output. A crystal with m == 1, or with any flag, is passed through: its n atoms in node order in the reduced
 * basis (Lr, x'), n_prim = n, H written as the identity. Otherwise Lp = H Lr / m, each entry
 * ((h0 l0 + h1 l1) + h2 l2) / m in fp64, rounded once to fp32; the kept atoms are those of condition (d), in
 * ascending node index, with x_p = frac(x' adj(H) / m), component k being ((x0 a[0][k] + x1 a[1][k]) + x2 a[2][k]) / m
 * with the integer adjugate of H, fp64, rounded once, a value that rounds to 1 written as 0. There is no
 * averaging over an orbit: the representative of an orbit is its member of the lowest node index, with the
 * coordinates it has (a deliberate difference from spglib, which averages). The lattice Lp is a basis of the
 * primitive lattice, not a standardised or reduced one; chm_cell_run reduces it where that is wanted.
 *
 * Buffers. d_out: one chm_prim_record per crystal, 64 bytes each. d_source [N] int32: per input atom its rank among
 * the kept atoms of its crystal, or -1. d_new_offsets [B + 1] int32: the first node of every crystal in the
 * packed output; new_offsets[B] = N', the number of rows written. d_atom_types_out [N], d_frac_out [N,3]: the
 * packed state, crystal g's atoms at rows new_offsets[g] + rank; they are sized for the input's N and cleared
 * first, so the rows from N' on are zero. d_lattices_out [B,3,3]. The outputs must not be the inputs.
 * The plan holds the node offsets on the current device (create: as the symmetry plan's; more than 256 atoms in
 * a crystal is refused with CHM_E_UNSUPPORTED). The run takes every buffer with its count (cell records and out
 * 16-byte aligned); a NULL pointer, a mismatched count or tolerances outside the cell run's limits return
 * CHM_E_ARG naming the argument before the first HIP call and nothing is enqueued. It allocates nothing and does
 * not synchronise: legal under stream capture. All counts are integer sums: two runs, and a crystal alone or
 * inside any batch, give the same bytes per crystal. */
#define CHM_PRIM_AMBIGUOUS 1     /* no consistent set of translations after 4 halvings */
#define CHM_PRIM_NO_LATTICE 4    /* as CHM_SYMM_NO_LATTICE */
#define CHM_PRIM_THIN 8          /* as CHM_SYMM_THIN */
typedef struct {
  int32_t n_prim;             /* atoms written for this crystal: n / m, or n where it is passed through */
  int32_t n_trans;            /* m of the deciding level (0 where no search ran) */
  int32_t n_pivot;            /* atoms of the pivot species */
  int32_t halvings;           /* halvings of tol used, 0..4 */
  int32_t flags;              /* CHM_PRIM_* bits */
  int32_t h[6];               /* H[0][0], H[0][1], H[0][2], H[1][1], H[1][2], H[2][2] */
  float tol;                  /* the tolerance of the level that decided */
  int32_t lattice_system;     /* of the input cell, copied from the cell record (-1 with CHM_PRIM_NO_LATTICE) */
  int32_t reserved[3];        /* written as 0 */
} chm_prim_record;            /* 64 bytes */
typedef struct chm_prim chm_prim;
int chm_prim_create(const int32_t* h_natoms, int num_graphs, chm_prim** out);
void chm_prim_destroy(chm_prim* plan);
int chm_prim_run(const chm_prim* plan, const void* d_cell_records, size_t n_record_bytes, const int64_t* d_atom_types,
                 int64_t n_atom_types, const float* d_frac, int64_t n_frac, const float* d_lattices,
                 int64_t n_lattices, float symprec, float angle_tolerance, void* d_out, size_t n_out_bytes,
                 int32_t* d_source, int64_t n_source, int32_t* d_new_offsets, int64_t n_new_offsets,
                 int64_t* d_atom_types_out, int64_t n_atom_types_out, float* d_frac_out, int64_t n_frac_out,
                 float* d_lattices_out, int64_t n_lattices_out, void* stream);

/* Matching finished structures against reference structures on the device: what test_structure_matching of the
 * reference's scripts/evaluate.py asks of pymatgen on the host (StructureMatcher().fit(ref_st, st), reported as
 * match rate and RMSD). This is NOT a port of pymatgen: the definition below is this library's own, and how far
 * the two agree has not been measured. The parameters take StructureMatcher's defaults: ltol = 0.2 (relative
 * length), stol = 0.3 (fraction of l, below), angle_tol = 5 degrees; scaling is always on.
 *
 * Input. A state of B crystals (atom_types int64 [N], compared as their low 32 bits; frac fp32 [N,3]; lattices
 * fp32 [B,3,3], row vectors), R reference structures packed the same way, ref_of[B] (given at create: crystal g
 * is matched against reference ref_of[g] in [0, R); -1 = no reference: flag CHM_MATCH_NO_REFERENCE, ref -1,
 * everything else 0), and the chm_cell_records of the samples and of the references from chm_cell_run on the
 * same lattices (any tolerances: only T and the flags are read).
 *
 * Preconditions, each a flag, no search, matched = 0. CHM_MATCH_NO_LATTICE: one of the two cell records has
 * CHM_CELL_NOT_REDUCED, CHM_CELL_DEGENERATE or CHM_CELL_NONFINITE, or a reduced volume (below) is not a finite
 * number > 0. CHM_MATCH_SIZE: n != n_ref. CHM_MATCH_COMPOSITION (tested when the sizes are equal): some type's
 * atom count differs, compared as integers. Atom counts must be equal: there is no reduction to a primitive
 * cell, so a supercell sample does not match its primitive reference (a deliberate difference from pymatgen);
 * the way round it is chm_prim_*, above: reduce both to primitive cells first.
 *
 * Reduced frames. Ls = T_s L and x' = frac(x adj(T_s)) for the sample, Lr and xr likewise for the reference,
 * exactly as chm_cell_apply produces them (the same device code). V_s, V_r = |det| of those fp32 cells in fp64,
 * ((l00 (l11 l22 - l12 l21) - l01 (l10 l22 - l12 l20)) + l02 (l10 l21 - l11 l20)). Scale s = cbrt(V_r / V_s) and
 * l = cbrt(V_r / n), both in fp64 on one lane and rounded to fp32 once. Pairing cutoff c = stol l (A), fp32. The
 * scaled sample cell is sLs = s Ls, entry by entry.
 *
 * Lattice mappings. Every integer M with entries in {-1, 0, 1} and |det M| = 1, both signs, so that an
 * enantiomorph matches; index = sum_q (M[q] + 1) 3^q as in the cell search. With L' = M sLs (entries (m0 l0 + m1
 * l1) + m2 l2) M is accepted when every row length l'_i has |l'_i / lr_i - 1| <= ltol and every inter-row angle
 * differs from Lr's by at most angle_tol degrees (lengths, angles as in the cell search: accurate sqrtf / acosf).
 * The accepted M are taken in ascending index; n_mappings counts all of them, the first CHM_MATCH_MAX_MAPPINGS
 * (256) are used and more than that sets CHM_MATCH_MANY_MAPPINGS.
 *
 * Under a mapping. x'' = frac(x' Minv), Minv = det(M) adj(M) in integers, component k = (x0 Minv[0][k] + x1
 * Minv[1][k]) + x2 Minv[2][k], minus its floorf, 0 where that rounds to 1. The metric is G = 0.5 (G(L') + G(Lr)),
 * G(A)[i][j] = row_i . row_j: the mean of the two metric tensors, so no rotation has to be found. The length
 * squared of a fractional vector d is |d|^2 = (u0 d0 + u1 d1) + u2 d2 with u_k = (d0 G[0][k] + d1 G[1][k]) + d2 G[2][k].
 *
 * Anchors. p = the first reference atom of the species with the fewest atoms (ties: the smallest type). For
 * every sample atom j of that species, in node order: t_j = x''_j - xr_p and y_i = x''_i - t_j.
 *
 * Pairing of a candidate (M, j). Each reference atom k, in index order, takes the sample atom i of its own type
 * with the smallest |D|^2, D = (y_i - xr_k) - rintf(y_i - xr_k) per component (one image per component; ties go
 * to the smallest i). The candidate is given up at the first k whose partner has |D|^2 > c^2 (or not <=) or was
 * taken by an earlier k. A candidate that pairs every k survives: the pairing is a type-preserving bijection.
 * This is a nearest-partner rule, not pymatgen's optimal assignment; it is pairing CHM_MATCH_PAIRING_NEAREST, the
 * only one of chm_match_run / chm_match_group_run / chm_match_set_run.
 *
 * Pairing of a candidate (M, j) by assignment (CHM_MATCH_PAIRING_ASSIGNMENT, the *_run_pairing entry points; what
 * pymatgen's _cart_dists does with a linear assignment on the squared distances). Frames, scale, l, mappings,
 * anchors, metric, the thin-cell rule and the arithmetic rule are the ones of this text. (1) Prefilter: the
 * candidate stays alive when every reference atom k has a sample atom of its type with |D|^2 <= c^2; it is given
 * up at the first k with !(best <= c^2), which also removes NaN. n_survivors counts the alive candidates. (2) If
 * the nearest partners of an alive candidate are all different, that pairing is the optimum (the sum of the row
 * minima is a lower bound of every bijection's sum) and it is scored by the code of the nearest rule: its rms has
 * the same bits. (3) Otherwise the pairing is the type-preserving bijection that minimises sum_k |D_k|^2, D the
 * same one-image-per-component vector, over all sample atoms of the type (only the prefilter uses c). It is found
 * per species by shortest augmenting paths in fp32: duals u_k = min_i |D(k, i)|^2 (ties: the smallest i) and v =
 * 0; a column keeps the smallest row that wants it; every other row, in ascending k, grows a tree from reduced
 * costs (|D|^2 - u_k) - v_i, the next column being the one of smallest reduced cost (ties: the smallest i), until
 * a free column is reached. Every loop is bounded by n; a row that finds no column (NaN or Inf) ends the
 * candidate, which then does not count. (4) Score, the rms <= stol test and the winner key are unchanged.
 * At most CHM_MATCH_MAX_ASSIGN (64) collided candidates per crystal are solved, the lowest (mapping position,
 * anchor position) first; more than that sets CHM_MATCH_MANY_ASSIGNMENTS and the others do not count. n_assigned
 * = the number solved: the first reserved word of chm_match_record, bits 16..23 of the flags word of a
 * 16-byte pair record, and of the group / set record that copies it. Under CHM_MATCH_PAIRING_NEAREST those
 * stay 0 and every byte is what the old entry point writes: pairing 0 enqueues exactly the same kernels.
 *
 * Score of a survivor. m = (sum_k D_k) / n (sums in index order), e_k = D_k - m, rms = sqrtf((sum_k |e_k|^2) /
 * n) / l, max_dist = sqrtf(max_k |e_k|^2) (A). The candidate counts if rms <= stol. matched = 1 if any candidate
 * counts; the winner has the smallest rms, ties to the smallest mapping index, then the smallest j: an integer
 * minimum over (rms bits, position in the mapping list, position in the anchor list), so the record does not
 * depend on any order.
 *
 * Thin cells. With the plane spacings of Lr as in chm_symm_*: a crystal where not 2 c < the smallest spacing
 * gets CHM_MATCH_THIN and no search: one image per component would not be exact. Below that bound it is: any
 * image within c has every fractional component under 1/2.
 *
 * All per-candidate arithmetic is fp32, every product and sum rounded on its own. The bytes are the same on
 * every run and for a crystal alone or inside any batch.
 *
 * Record: rms, max_dist, scale, l (0 where not computed), mapping (candidate index of the winner, -1), anchor
 * (the sample atom j of the winner within its crystal, -1), n_mappings, n_candidates (mappings used x anchors),
 * n_survivors, matched, flags, ref, 16 bytes of 0. Optional second output d_perm int32 [N] (NULL with n_perm =
 * 0): at node offset of crystal g, for each reference atom k the sample atom (within the crystal) it is paired
 * with under the winner; -1 everywhere in a crystal that is not matched.
 *
 * The plan holds the node offsets of both lists and ref_of on the current device; a crystal or reference of more
 * than 256 atoms is refused at create with CHM_E_UNSUPPORTED, a ref_of outside [-1, R) with CHM_E_ARG. The run
 * takes every buffer with its count (cell records 128 bytes, out 64 bytes per crystal, 16-byte aligned); a NULL
 * pointer, a mismatched count, ltol or stol outside (0, 1] or angle_tol outside (0, 30] return CHM_E_ARG naming
 * the argument before the first HIP call and nothing is enqueued. It allocates nothing and does not
 * synchronise: legal under stream capture. */
#define CHM_MATCH_NO_REFERENCE 1   /* ref_of = -1 */
#define CHM_MATCH_NO_LATTICE 2     /* a cell record without a reduced cell, or a volume not > 0 */
#define CHM_MATCH_SIZE 4           /* n != n_ref */
#define CHM_MATCH_COMPOSITION 8    /* element counts differ */
#define CHM_MATCH_THIN 16          /* 2 stol l is not below the smallest plane spacing of Lr */
#define CHM_MATCH_MANY_MAPPINGS 32 /* more than CHM_MATCH_MAX_MAPPINGS accepted: the first ones were used */
#define CHM_MATCH_MANY_ASSIGNMENTS 128 /* more than CHM_MATCH_MAX_ASSIGN collided candidates: the lowest were solved */
#define CHM_MATCH_MAX_MAPPINGS 256
#define CHM_MATCH_MAX_ASSIGN 64
#define CHM_MATCH_PAIR_ASSIGNED_SHIFT 16 /* chm_match_pair_record.flags: n_assigned << 16 (assignment pairing only) */
#define CHM_MATCH_PAIRING_NEAREST 0
#define CHM_MATCH_PAIRING_ASSIGNMENT 1
#define CHM_MATCH_MAX_LTOL 1.0f
#define CHM_MATCH_MAX_STOL 1.0f
#define CHM_MATCH_MAX_ANGLE_TOL 30.0f
typedef struct {
  float rms;                  /* of the winner, in units of l */
  float max_dist;             /* of the winner (A) */
  float scale;                /* s */
  float l;                    /* cbrt(V_r / n) (A) */
  int32_t mapping;            /* candidate index of the winner's M, or -1 */
  int32_t anchor;             /* the winner's sample atom j within the crystal, or -1 */
  int32_t n_mappings;         /* accepted M (all of them) */
  int32_t n_candidates;       /* (M, j) tried */
  int32_t n_survivors;        /* candidates that paired every atom */
  int32_t matched;            /* 1 or 0 */
  int32_t flags;              /* CHM_MATCH_* bits */
  int32_t ref;                /* ref_of of the crystal */
  int32_t reserved[4];        /* written as 0; reserved[0] = n_assigned under CHM_MATCH_PAIRING_ASSIGNMENT */
} chm_match_record;           /* 64 bytes */
typedef struct chm_match chm_match;
int chm_match_create(const int32_t* h_natoms, int num_graphs, const int32_t* h_ref_natoms, int num_refs,
                     const int32_t* h_ref_of, chm_match** out);
void chm_match_destroy(chm_match* plan);
int chm_match_run(const chm_match* plan, const void* d_cell_records, size_t n_record_bytes,
                  const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                  const float* d_lattices, int64_t n_lattices, const void* d_ref_cell_records,
                  size_t n_ref_record_bytes, const int64_t* d_ref_atom_types, int64_t n_ref_atom_types,
                  const float* d_ref_frac, int64_t n_ref_frac, const float* d_ref_lattices, int64_t n_ref_lattices,
                  float ltol, float stol, float angle_tol, void* d_out, size_t n_out_bytes, int32_t* d_perm,
                  int64_t n_perm, void* stream);
/* chm_match_run with the pairing chosen: CHM_MATCH_PAIRING_NEAREST (what chm_match_run enqueues, byte for byte) or
 * CHM_MATCH_PAIRING_ASSIGNMENT; any other value returns CHM_E_ARG before any HIP call. d_perm holds the assignment
 * where the winner was a collided candidate. */
int chm_match_run_pairing(const chm_match* plan, const void* d_cell_records, size_t n_record_bytes,
                          const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                          const float* d_lattices, int64_t n_lattices, const void* d_ref_cell_records,
                          size_t n_ref_record_bytes, const int64_t* d_ref_atom_types, int64_t n_ref_atom_types,
                          const float* d_ref_frac, int64_t n_ref_frac, const float* d_ref_lattices,
                          int64_t n_ref_lattices, float ltol, float stol, float angle_tol, void* d_out,
                          size_t n_out_bytes, int32_t* d_perm, int64_t n_perm, void* stream, int pairing);

/* Grouping duplicate structures of one batch by pairwise matching on the device: the uniqueness step of the
 * reference's workflows (StructureMatcher().group_structures in test_unique of scripts/evaluate.py and in
 * scripts/navigate_chemical_system.py) with the match criterion above instead of the fingerprints of chm_dedup_*.
 * This is NOT a port of pymatgen, and how far the groups agree with group_structures has not been measured.
 *
 * Pairs. Every pair (h, g), h < g, of crystals with equal atom counts is one match: crystal h is the reference
 * side (the possible leader), crystal g the sample side, both read from the same state and the same
 * chm_cell_records. The definition of a match is chm_match_*'s, word for word (the reduced frames of both, the
 * volume scaling, the mappings within ltol / angle_tol in ascending index capped at 256, the anchors of the rarest
 * species, nearest-partner pairing within stol l, the mean-removed rms with the smallest winning, and the flags
 * CHM_MATCH_NO_LATTICE, COMPOSITION, THIN and MANY_MAPPINGS): the same device code. Pairs of unequal atom counts
 * can never match (CHM_MATCH_SIZE) and are not launched: there is no reduction to a primitive cell, so a
 * supercell is never grouped with its primitive cell. The pairs are ordered by g, then by h;
 * chm_match_group_num_pairs gives their number P. A pair's record {rms, max_dist, flags, matched} (16 bytes)
 * depends on the two crystals and the tolerances alone, not on the batch, the order of the pairs or the run. A
 * pair with an excluded crystal (d_exclude[g] != 0; NULL with n_exclude = 0: none) has flags
 * CHM_MATCH_EXCLUDED, one with a crystal whose cell record has CHM_CELL_NOT_REDUCED, DEGENERATE or NONFINITE has
 * CHM_MATCH_NO_LATTICE, and neither is searched (everything else 0). The relation is not symmetric in general:
 * THIN and l are taken from the reference side h.
 *
 * Groups: the leader rule of chm_dedup_group on the matrix "h < g and (h, g) matched" (the same kernel). In index
 * order a crystal is a representative when it matches no earlier representative, else it joins the earliest
 * earlier representative it matches; the rule is not transitive, on purpose. group[g] = the representative's
 * index (its own for a representative), count[g] = the group's size at a representative and 0 elsewhere. An
 * excluded crystal or one without a reduced cell gets group -1: it is never a leader and nothing joins it. A
 * leader whose pairs all carry a flag (CHM_MATCH_THIN, say) stays a group of its own.
 *
 * Output per crystal (32 bytes): the record of its pair with its leader and ref = the leader, pair = that pair's
 * position; a leader has rms = max_dist = 0, flags = 0, matched = 0, ref = pair = -1; a crystal of group -1 the
 * same with flags CHM_MATCH_EXCLUDED and / or CHM_MATCH_NO_LATTICE.
 *
 * The plan is built on the host from natoms alone and holds the node offsets and the pair table on the current
 * device; a crystal of more than 256 atoms, or more than 2^31 - 1 pairs (one 1-D grid), is refused at create with
 * CHM_E_UNSUPPORTED. The run takes every buffer with its count (cell records 128, out 32 bytes per crystal, pair
 * records 16 bytes per pair, NULL with 0 bytes when P = 0; all 16-byte aligned; the workspace at least
 * chm_match_group_workspace_bytes); a NULL pointer, a mismatched count or a tolerance outside chm_match_run's
 * ranges return CHM_E_ARG naming the argument before the first HIP call and nothing is enqueued. It enqueues
 * four kernels (the first clears the bit matrix), uses integer atomics only, allocates nothing and does not
 * synchronise: legal under stream capture. */
#define CHM_MATCH_EXCLUDED 64 /* chm_match_group_*: a crystal of the pair (or the crystal) is excluded */
typedef struct {
  float rms;       /* of the winner, in units of l of crystal h */
  float max_dist;  /* of the winner (A) */
  int32_t flags;   /* CHM_MATCH_* bits; bits 16..23 = n_assigned under CHM_MATCH_PAIRING_ASSIGNMENT */
  int32_t matched; /* 1 or 0 */
} chm_match_pair_record; /* 16 bytes */
typedef struct {
  float rms;           /* of the crystal against its leader; 0 for a leader */
  float max_dist;
  int32_t flags;
  int32_t matched;     /* 1 for a member, 0 for a leader and for group -1 */
  int32_t ref;         /* the leader, or -1 */
  int32_t pair;        /* the position of (leader, crystal) among the pairs, or -1 */
  int32_t reserved[2]; /* written as 0 */
} chm_match_group_record; /* 32 bytes */
typedef struct chm_match_group chm_match_group;
int chm_match_group_create(const int32_t* h_natoms, int num_graphs, chm_match_group** out);
void chm_match_group_destroy(chm_match_group* plan);
int64_t chm_match_group_num_pairs(const chm_match_group* plan);
size_t chm_match_group_workspace_bytes(const chm_match_group* plan);
int chm_match_group_run(const chm_match_group* plan, const void* d_cell_records, size_t n_record_bytes,
                        const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                        const float* d_lattices, int64_t n_lattices, const uint8_t* d_exclude, int64_t n_exclude,
                        float ltol, float stol, float angle_tol, int32_t* d_group, int64_t n_group, int32_t* d_count,
                        int64_t n_count, void* d_out, size_t n_out_bytes, void* d_pair_records, size_t n_pair_bytes,
                        void* d_workspace, size_t workspace_bytes, void* stream);
/* chm_match_group_run with the pairing chosen (see chm_match_run_pairing). */
int chm_match_group_run_pairing(const chm_match_group* plan, const void* d_cell_records, size_t n_record_bytes,
                                const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                                const float* d_lattices, int64_t n_lattices, const uint8_t* d_exclude,
                                int64_t n_exclude, float ltol, float stol, float angle_tol, int32_t* d_group,
                                int64_t n_group, int32_t* d_count, int64_t n_count, void* d_out, size_t n_out_bytes,
                                void* d_pair_records, size_t n_pair_bytes, void* d_workspace, size_t workspace_bytes,
                                void* stream, int pairing);

/* Searching a set of reference structures for each finished structure on the device: is this sample any structure
 * of the set (known) or none of them (novel)? It is what the users of the reference's
 * scripts/navigate_chemical_system.py do with its output (strike out the training set, or merge a run into the
 * representatives kept so far) with the match criterion above. This is NOT a port of pymatgen, and how far known /
 * novel agree with StructureMatcher().fit against every structure of the set has not been measured. It inherits
 * every caveat of chm_match_*: atom counts must be equal (no reduction to a primitive cell: chm_prim_* first is the
 * way round it), and the pairing is the nearest-partner rule unless chm_match_set_run_pairing asks for the assignment.
 *
 * Composition key. key = sum_i mix(t_i) over the atoms of a structure, as wrapping 64-bit unsigned addition, where
 * t_i is the atom type's low 32 bits as an unsigned number (what the matcher compares) and mix is the splitmix64
 * finaliser of t + 1: z = t + 1; z = (z ^ (z >> 30)) * CHM_MATCH_SET_MIX_A; z = (z ^ (z >> 27)) *
 * CHM_MATCH_SET_MIX_B; mix = z ^ (z >> 31). The key is exact and does not depend on the order of the atoms; equal
 * compositions have equal keys. Two different compositions of one atom count with equal keys cost one launched
 * pair that ends with CHM_MATCH_COMPOSITION: a collision can never hide a match.
 *
 * Reference set. R structures of at most 256 atoms each, packed like a state and held sorted ascending by (atom
 * count, key, original index); ref_index[k] is the original index of sorted position k. The caller sorts and
 * computes the keys of the references on the host, once; the keys of the samples are computed on the device in
 * every run, from the state's atom types as they are then.
 *
 * Candidates of sample g: the references with its atom count and its key, one contiguous range [lo_g, lo_g + c_g)
 * of sorted positions. An excluded sample (d_exclude[g] != 0; NULL with n_exclude = 0: none) and a sample whose
 * cell record has CHM_CELL_NOT_REDUCED, DEGENERATE or NONFINITE have no candidates (c_g = 0) and the flags
 * CHM_MATCH_EXCLUDED / CHM_MATCH_NO_LATTICE. The pairs of a run are the candidates of sample 0, then of sample 1,
 * ..., each in sorted order: P = sum_g c_g of them, first_g = sum_{h < g} c_h. P is known on the device only; it is
 * at most chm_match_set_num_pairs_max = the sum over the samples of the number of references of that atom count,
 * which the host knows at create and which the pair list can never overflow.
 *
 * Pair match. Each pair is one match in chm_match_*'s definition, word for word (the same device code), the
 * reference being the reference side: l and CHM_MATCH_THIN come from it. Its record is a chm_match_pair_record
 * {rms, max_dist, flags, matched} at its position in the pair list and depends on the two structures and the
 * tolerances alone. A reference without a reduced cell matches nothing (CHM_MATCH_NO_LATTICE on its pairs).
 *
 * Record per sample (48 bytes): n_candidates = c_g; n_matched = how many of them matched; known = n_matched > 0;
 * the winner = the matched candidate with the smallest rms, ties to the smallest original index (an integer
 * minimum over (rms bits, original index), so the answer does not depend on how the set was ordered): ref = its
 * original index, position = its sorted position (both -1 when novel), rms, max_dist and flags of its pair record
 * (rms = max_dist = 0 when novel; flags then hold only CHM_MATCH_EXCLUDED / NO_LATTICE of the sample); key; first
 * = first_g and lo = lo_g, so that the sample's pair records are [first, first + n_candidates) for the sorted
 * positions lo, lo + 1, ...
 *
 * The run enqueues four kernels: the keys (one block per sample: a wave reduction and LDS, integer adds in a fixed
 * order, two binary searches, and the sample's winner word and count cleared), the offsets (one block, an integer
 * scan), the pairs (a grid of fixed size chosen at create, min(num_pairs_max, CHM_MATCH_SET_BLOCKS_PER_CU x the
 * device's compute units) blocks that stride over b < P; one integer atomicAdd and one 64-bit atomicMin per match,
 * no float atomics) and the gather (one thread per sample, blocks of 256). It takes every buffer with its count
 * (cell records 128 bytes per structure, out 48 bytes per sample, pair records 16 bytes x num_pairs_max, NULL with
 * 0 bytes when that is 0; all 16-byte aligned; the workspace at least chm_match_set_workspace_bytes); a NULL
 * pointer, a mismatched count or a tolerance outside chm_match_run's ranges return CHM_E_ARG naming the argument
 * before the first HIP call and nothing is enqueued. Pair records at and after P are left as they were. It
 * allocates nothing and does not synchronise: legal under stream capture, and a replay follows the atom types,
 * coordinates and cell records that the buffers hold then. Create refuses a structure of more than 256 atoms and
 * more than 2^31 - 1 pairs with CHM_E_UNSUPPORTED, a set that is not sorted or a ref_index that is no permutation
 * with CHM_E_ARG. */
#define CHM_MATCH_SET_MIX_A 0xbf58476d1ce4e5b9ull
#define CHM_MATCH_SET_MIX_B 0x94d049bb133111ebull
#define CHM_MATCH_SET_BLOCKS_PER_CU 3 /* what the pair kernel's 144 VGPRs let a CU hold: three blocks of four waves */
typedef struct {
  float rms;            /* of the winner, in units of l of that reference; 0 when novel */
  float max_dist;       /* of the winner (A) */
  int32_t flags;        /* CHM_MATCH_* bits of the winner's pair, or EXCLUDED / NO_LATTICE of the sample */
  int32_t known;        /* 1 or 0 */
  int32_t ref;          /* the winner's original index, or -1 */
  int32_t position;     /* the winner's sorted position, or -1 */
  int32_t n_candidates; /* c_g */
  int32_t n_matched;
  uint64_t key;         /* the sample's composition key */
  int32_t first;        /* the sample's first pair record */
  int32_t lo;           /* the sorted position of its first candidate (where its key would stand if it has none) */
} chm_match_set_record; /* 48 bytes */
typedef struct chm_match_set chm_match_set;
int chm_match_set_create(const int32_t* h_natoms, int num_graphs, const int32_t* h_ref_natoms,
                         const uint64_t* h_ref_keys, const int32_t* h_ref_index, int num_refs, chm_match_set** out);
void chm_match_set_destroy(chm_match_set* plan);
int64_t chm_match_set_num_pairs_max(const chm_match_set* plan);
size_t chm_match_set_workspace_bytes(const chm_match_set* plan);
int chm_match_set_run(const chm_match_set* plan, const void* d_cell_records, size_t n_record_bytes,
                      const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                      const float* d_lattices, int64_t n_lattices, const void* d_ref_cell_records,
                      size_t n_ref_record_bytes, const int64_t* d_ref_atom_types, int64_t n_ref_atom_types,
                      const float* d_ref_frac, int64_t n_ref_frac, const float* d_ref_lattices, int64_t n_ref_lattices,
                      const uint8_t* d_exclude, int64_t n_exclude, float ltol, float stol, float angle_tol, void* d_out,
                      size_t n_out_bytes, void* d_pair_records, size_t n_pair_bytes, void* d_workspace,
                      size_t workspace_bytes, void* stream);
/* chm_match_set_run with the pairing chosen (see chm_match_run_pairing). The grid is the one chosen at create; the
 * assignment kernel's LDS lets a CU hold two of its blocks, the others wait their turn. */
int chm_match_set_run_pairing(const chm_match_set* plan, const void* d_cell_records, size_t n_record_bytes,
                              const int64_t* d_atom_types, int64_t n_atom_types, const float* d_frac, int64_t n_frac,
                              const float* d_lattices, int64_t n_lattices, const void* d_ref_cell_records,
                              size_t n_ref_record_bytes, const int64_t* d_ref_atom_types, int64_t n_ref_atom_types,
                              const float* d_ref_frac, int64_t n_ref_frac, const float* d_ref_lattices,
                              int64_t n_ref_lattices, const uint8_t* d_exclude, int64_t n_exclude, float ltol,
                              float stol, float angle_tol, void* d_out, size_t n_out_bytes, void* d_pair_records,
                              size_t n_pair_bytes, void* d_workspace, size_t workspace_bytes, void* stream, int pairing);

/* Sizes of the batch (for callers that allocate outputs). */
int64_t chm_batch_num_nodes(const chm_batch* b);
int64_t chm_batch_num_edges(const chm_batch* b);

/* The model dimensions behind a batch and its sizes (any pointer may be NULL): *dims = the
 * model's chm_dims, *num_graphs = B, *max_pairs = the pairs it was created for, *knn = 1 for a
 * knn-edge batch. Callers that allocate outputs or validate shapes use it (the torch-op layer,
 * chemeleon_amd/csrc/torch_ops.cpp, checks every tensor against it before a launch). */
int chm_batch_info(const chm_batch* b, chm_dims* dims, int64_t* num_graphs, int* max_pairs, int* knn);
/* The HIP device ordinal the batch (and its model) lives on: every buffer passed with the batch
 * must be memory of that device (the torch-op layer checks each tensor's device against it and
 * launches under a device guard for it). Negative CHM_E_ARG for a NULL batch. */
int chm_batch_device(const chm_batch* b);

#ifdef __cplusplus
}
#endif
#endif /* CHEMELEON_HIP_H */
