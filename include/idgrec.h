/*
 * idgrec.h — C-ABI of libidgrec.so, the MI355X (gfx950) implementation of ID-GRec's
 * LightGCN-style hot path: BPR sampler -> K-layer normalised-adjacency SpMM ->
 * fused gather-BPR loss/grad -> dense Adam, and full-rank scoring + mask + top-K.
 *
 * The reference (BlueGhostYi/ID-GRec) is pure Python; the "FFI" a maintainer binds is
 * ctypes.  Every entry point below names the reference call site
 * (path:line relative to the reference repo) whose arithmetic it replaces.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = error class (IDG_E_*); the message of the
 *     last failure on the calling thread is idg_last_error().
 *   - "host" functions take host pointers and never touch the GPU.
 *   - "device" functions take DEVICE pointers owned by the caller (torch tensors'
 *     data_ptr()), are asynchronous on the hipStream_t passed as `void* stream`
 *     (NULL = the null stream), never allocate, never synchronise.  Scratch memory is
 *     caller-allocated; sizes come from the matching *_workspace_bytes().
 *   - opaque handles (idg_rng, idg_ratings, idg_graph) are owned by the library and
 *     released by the paired *_destroy().
 *   - no C++ exception crosses this boundary.  There is NO CPU fallback for device
 *     entry points: without a gfx950 device they fail with IDG_E_NODEVICE.
 */
#ifndef IDGREC_H
#define IDGREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDG_VERSION 142 /* 0.5.3 (added since, no entry point changed, so the number stays): idg_na_nce_f32 / idg_na_nce_workspace_bytes / idg_reg_rows_f32 (LightCCF's and LightCSCF's neighbour-aggregation loss, and the regulariser without a BPR call); idg_table_nce_f32 / idg_table_nce_workspace_bytes (CGCL's full-table contrastive loss: every batch row against a whole normalised embedding table, forward and backward); 0.5.3: idg_multinomial_nll_f32 / idg_multinomial_nll_workspace_bytes (CVGA's decoder: linear + log-softmax + multinomial NLL over the catalogue, forward and backward), idg_vae_head_fwd_f32 / idg_vae_head_bwd_f32 / idg_vae_head_workspace_bytes (its VAE head); 0.5.2: idg_align_uniform_f32 / idg_align_uniform_workspace_bytes (DirectAU's alignment + uniformity loss); 0.5.1: idg_pack24_f32 / idg_unpack24_f32 / idg_reduce24_f32 / idg_alltoall_f32 (24-bit panel exchange, rank-ordered sum), idg_score_topk_candidate_counts, idg_score_topk_option (the top-K knobs: environment read once), idg_score_topk_info fills info[8], form 3's whole-call fall-back; idg_step_run_f32 takes next_ids_token; idg_step_synchronize also drains the side stream's preparations; 0.5.0: idg_step_* (one library call per training step), idg_adam_rows_f32; 0.4.4: IDG_ADAM_DISCARD_GRAD; 0.4.3: idg_event_synchronize; 0.4.2: idg_infonce_plan / IDG_SSL_PLANNED / idg_infonce_cross_ex_f32 (InfoNCE id lists a batch ahead); 0.4.1: idg_ngcf_layer_fwd_f32 / idg_ngcf_layer_bwd_f32 (one kernel per NGCF layer and direction); 0.4.0: idg_rows_layer_mean_n_f32 (any number of layers), idg_flags_compact_f32 (the touched-item
                           agreement without a host read-back), idg_shard_prepare validates its geometry.
                           133 / 0.3.0: process-wide live-unit registry + idg_graph_live_units_check; idg_spmm_epi_f32 (every
                           epilogue option; out_rows and x_rows combined); round-3 sharded step: idg_rows_gather2 / _scatter /
                           _chain_store2 / _layer_mean, idg_grad_tail_adam_f32, idg_reduce_scatter_f32 */

/* error classes */
#define IDG_OK 0
#define IDG_E_INVALID (-1)  /* bad argument */
#define IDG_E_NODEVICE (-2) /* no HIP device / wrong device */
#define IDG_E_HIP (-3)      /* a HIP runtime call failed */
#define IDG_E_IO (-4)       /* file could not be read / parsed */
#define IDG_E_NOMEM (-5)
#define IDG_E_UNSUPPORTED (-6)

int idg_version(void);
const char* idg_last_error(void);
/* number of visible HIP devices (0 when none). Never fails. */
int idg_device_count(void);

/* ------------------------------------------------------------------------------------
 * HOST: NumPy-legacy MT19937 stream  (replaces the global np.random state the reference
 * seeds in utility/utility_function/tools.py:8-14 and draws from in
 * utility/utility_data/data_loader.py:120 and utility/utility_function/tools.py:42)
 * ---------------------------------------------------------------------------------- */
typedef struct idg_rng idg_rng;

/* np.random.seed(seed) : init_genrand(seed), pos = 624 */
int idg_rng_create(uint32_t seed, idg_rng** out);
int idg_rng_destroy(idg_rng* rng);
/* mirrors np.random.get_state()[1:3] / set_state */
int idg_rng_get_state(const idg_rng* rng, uint32_t key[624], int32_t* pos);
int idg_rng_set_state(idg_rng* rng, const uint32_t key[624], int32_t pos);
/* RandomState.bytes(n): raw little-endian uint32 stream */
int idg_rng_bytes(idg_rng* rng, int64_t nbytes, uint8_t* out);
/* `count` successive scalar np.random.randint(0, high) draws (masked rejection) */
int idg_rng_randint(idg_rng* rng, int64_t high, int64_t count, int64_t* out);

/* Data.sample_data_to_train_all (utility/utility_data/data_loader.py:108-127):
 * for every train edge i in file order emit [train_user[i], train_item[i], neg] with
 * neg = randint(0,num_items) re-drawn while neg is in the user's positive set.
 * pos_indptr[num_users+1] / pos_indices (ascending per user) are the CSR rows of the
 * train matrix (Data.all_positive).  Users with no positives are skipped (:114-115).
 * out_triples is [E,3] row-major int64; *out_count = rows written (<= E). */
int idg_sample_epoch(idg_rng* rng, const int64_t* train_user, const int64_t* train_item, int64_t E,
                     const int64_t* pos_indptr, const int32_t* pos_indices, int64_t num_users,
                     int64_t num_items, int64_t* out_triples, int64_t* out_count);

/* np.random.shuffle(np.arange(n)) (utility/utility_function/tools.py:41-42) */
int idg_shuffle_perm(idg_rng* rng, int64_t n, int64_t* out_perm);

/* random.sample(range(n), k) of Python's `random` module (CPython >= 3.10) on its own MT19937 stream — the
 * draw of SGL's kept edges (utility/utility_function/tools.py:80, never seeded by the reference).  Load the
 * module's state with idg_rng_set_state (random.getstate()[1]: 624 words + index), write it back afterwards.
 * use_pool: the branch random.py takes (n <= 21 + 4 ** ceil(log(3k, 4)) for k > 5), decided by the caller
 * with that very expression.  n < 2^32. */
int idg_py_random_sample(idg_rng* rng, int64_t n, int64_t k, int use_pool, int64_t* out);

/* ------------------------------------------------------------------------------------
 * HOST: rating-file parser and adjacency builder
 * ---------------------------------------------------------------------------------- */
typedef struct idg_ratings idg_ratings;

/* Data.read_ratings (utility/utility_data/data_loader.py:48-70): parse lines
 * "uid i1 i2 ..." (space separated ints).  Lines with no items count in n_lines but emit
 * no edge and do not move the maxima (:59-61).  max_user/max_item are -1 when no edge. */
int idg_ratings_open(const char* path, idg_ratings** out, int64_t* n_edges, int64_t* n_lines,
                     int64_t* max_user, int64_t* max_item);
/* users/items [n_edges] in file order; line_users / line_counts [n_lines] = the user id and
 * the number of items of every line.  Any output may be NULL. */
int idg_ratings_read(const idg_ratings* r, int64_t* users, int64_t* items, int64_t* line_users,
                     int64_t* line_counts);
int idg_ratings_destroy(idg_ratings* r);

/* data_graph.sparse_adjacency_matrix (utility/utility_data/data_graph.py:33-55) and, with
 * self_loops != 0, sparse_adjacency_matrix_with_self (:7-30): the symmetric bipartite
 * adjacency A=[[0,R],[R^T,0]] (+I), duplicate (u,i) pairs summed, normalised
 * D^-1/2 A D^-1/2, as CSR with ascending columns and float32 values.  Arithmetic follows
 * the reference: float32 products (d_i*a)*d_j without self loops; float64 products rounded
 * once to float32 with them (the `+ sp.eye` promotes to float64).
 * dinv (nullable, [U+I]): d^-1/2 per node as the caller computed it (the Python host passes
 * np.power(deg, -0.5), the reference's own expression, whose SIMD rounding cannot be
 * restated portably); NULL = correctly rounded 1/sqrt(deg), 0 for isolated nodes.
 * Two-call protocol: first call with indptr==NULL returns *nnz; second call fills
 * indptr[U+I+1], indices[nnz], values[nnz]. */
int idg_build_norm_adj(int64_t num_users, int64_t num_items, int64_t E, const int64_t* users,
                       const int64_t* items, int self_loops, const double* dinv, int64_t* nnz,
                       int64_t* indptr, int32_t* indices, float* values);

/* ------------------------------------------------------------------------------------
 * DEVICE: sparse graph handle
 * (replaces the coalesced torch sparse COO tensor built in models/LightGCN.py:30-32 via
 *  utility/utility_function/tools.py:95-109)
 * ---------------------------------------------------------------------------------- */
typedef struct idg_graph idg_graph;

#define IDG_GRAPH_SYMMETRIC 1u   /* A == A^T exactly: backward reuses the same CSR */
#define IDG_GRAPH_EXACT_ORDER 2u /* never split a row: every output element is the
                                    sequential CSR-order fmaf chain torch CPU computes */
#define IDG_GRAPH_NO_BALANCED 4u /* do not build the length-balanced second tile schedule of the dense launches
                                    (speed only: same bits either way; IDG_BALANCED_TILES=0 in the environment at
                                    creation does the same for every handle) */

/* CSR arrays are HOST pointers; the handle uploads and owns device copies plus its
 * row-block tile schedule.  split_threshold: rows with more stored entries than this are
 * cut into segments summed in a fixed published order (0 = library default 128; ignored with
 * EXACT_ORDER).  Rows of up to 512 entries are combined inside one workgroup (LDS); longer rows go
 * through one global partial per 512-entry chunk (workspace = n_long_chunks x d floats).  A handle
 * owns the arrival counters of its chunked rows: launches that use one handle must be ordered (one
 * stream, or events between streams); different handles are independent. */
int idg_graph_create(int device, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* indptr,
                     const int32_t* indices, const float* values, uint32_t flags,
                     int64_t split_threshold, idg_graph** out);
/* The same from DEVICE CSR arrays (SURVEY.md 8b's signature: the reference's graph is a coalesced sparse tensor that
 * already lives on the device, models/LightGCN.py:31-32).  The schedule is still built by host code: the arrays are copied
 * to host memory behind `stream` (the one call of this library that synchronises a stream: graph construction is a
 * one-off).  A device-side schedule build is future work. */
int idg_graph_create_from_device(int device, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* d_indptr,
                                 const int32_t* d_indices, const float* d_values, uint32_t flags,
                                 int64_t split_threshold, void* stream, idg_graph** out);
int idg_graph_destroy(idg_graph* g);

/* A copy of `g` whose stored entry (r, c) keeps values[k] / divisor when floor(u + add) != 0 and becomes an explicit
 * zero otherwise, u ~ U[0, 1) drawn by Philox4x32-10 from (seed, stream_id, r, c) — with transpose != 0 from (c, r):
 * for a symmetric `g` that copy is the TRANSPOSE of the first one, which is what the backward of a product with the
 * first one multiplies by.  This is NGCF.node_dropout (models/NGCF.py:56-65: keep where int(rand + (1 - keep_prob))
 * is non-zero, survivors divided by (1 - keep_prob)) with add = divisor = 1 - keep_prob; the zeros stay in the
 * structure (fmaf(0, x, acc) == acc), so the tile schedule, split schedule and summation order are those of `g`.
 * The copy shares g's schedule (g must outlive it) and owns its entry list; destroy it with idg_graph_destroy.
 * The mask is written on `stream`, in order with the products that follow. */
int idg_graph_masked_copy(const idg_graph* g, float add, float divisor, uint64_t seed, uint64_t stream_id,
                          int transpose, void* stream, idg_graph** out);
/* A new draw into an EXISTING copy of g (one made by idg_graph_masked_copy / idg_graph_revalued_copy): no allocation,
 * asynchronous on `stream` — the per-forward form of node dropout. */
int idg_graph_remask(const idg_graph* g, idg_graph* copy, float add, float divisor, uint64_t seed,
                     uint64_t stream_id, int transpose, void* stream);

/* Live work units of a row bitmap (optional accelerator of the row-restricted launches; round 2).  A launch given
 * `out_rows` normally visits every tile to find the few rows wanted.  idg_graph_live_units turns the bitmap into the list
 * of work units behind its rows — on `stream`: meant for the side stream that prepares a batch's index-only work — and
 * registers (schedule, bitmap pointer -> list); from then on every restricted launch on this handle, or on a masked /
 * revalued copy of it (copies share the schedule: no second registration), that names THIS bitmap pointer runs one wave
 * per listed unit and visits no tile.  Results are bit-identical to the tile form.
 * Validity.  A list describes the bitmap's contents at the time of the call.  Every library entry point that writes a row
 * bitmap (idg_bpr_touch_rows, idg_bitmap_clear, the `touched` argument of idg_bpr_backward_f32 / idg_bpr_fused_f32,
 * idg_graph_expand_rows / idg_graph_mark_cols outputs, idg_bpr_pack_rows_f32 / idg_bpr_unpack_rows_f32) drops the lists
 * registered for that pointer before it writes, and launches then fall back to the tile form (always correct) until
 * idg_graph_live_units is called again — so a buffer that was freed and handed out again is harmless once its new owner
 * fills it through the library.  A caller that rewrites a registered bitmap by other means calls
 * idg_graph_forget_live_units first (bitmap = NULL: every list of this handle's schedule); destroying the handle forgets
 * its lists.  The registry is process-wide, holds 64 lists (oldest replaced) and is thread-safe.
 * max_rows: upper bound on the set bits (3 x batch size).  More set bits than that cannot be listed: the list is marked
 * incomplete on the device, launches that use it write NaN into every row they produce, and idg_graph_live_units_check
 * (synchronises `stream`; for tests and debugging) returns IDG_E_INVALID.
 * units_ws: idg_graph_live_units_bytes(g, max_rows) bytes of device memory owned by the caller, alive while registered.
 * idg_graph_bind_live_units registers an existing list under another bitmap pointer / handle of the same schedule. */
size_t idg_graph_live_units_bytes(const idg_graph* g, int64_t max_rows);
int idg_graph_live_units(const idg_graph* g, const uint32_t* bitmap, void* units_ws, int64_t max_rows, void* stream);
int idg_graph_bind_live_units(const idg_graph* g, const uint32_t* bitmap, const void* units_ws, int64_t max_rows);
int idg_graph_forget_live_units(const idg_graph* g, const uint32_t* bitmap);
/* Drop every registered list (unit lists and compacted entry lists, of any handle) that lives in the buffer `ws`: what a
 * caller does before it frees or reuses a list buffer (the registration names the buffer; ADVICE r03: forgetting by bitmap
 * alone drops a NEW registration of the same bitmap when an OLD buffer dies). */
int idg_graph_forget_units_ws(const void* ws);
int idg_graph_live_units_check(const void* units_ws, void* stream);
/* The first backward product of a training step gathers from a panel with <= 3B live rows (d loss / d final: the batch's
 * rows).  Which stored entries point at live rows is index-only work: idg_graph_compact_inputs does it ahead of time (on
 * `stream`, typically the caller's side stream) — per tile the live entries, in their order, a compacted start per virtual
 * row and a live count — and registers the result for `bitmap` exactly as idg_graph_live_units registers a unit list (same
 * validity rules: every library call that writes the bitmap drops it; idg_graph_forget_live_units drops it).  A product
 * naming that bitmap as x_rows (idg_spmm_epi_f32, idg_propagate_mean_bwd*_f32's gout_mask) then walks the compacted
 * lists with the ordinary kernel: bit-identical to the in-kernel compaction and to the dense product.
 * ws: idg_graph_compact_inputs_bytes(g) bytes, 16-byte aligned, owned by the caller while registered. */
size_t idg_graph_compact_inputs_bytes(const idg_graph* g);
int idg_graph_compact_inputs(const idg_graph* g, const uint32_t* bitmap, void* ws, void* stream);

/* The batch's receptive field (no reference counterpart: the reference propagates the whole graph every step,
 * models/LightGCN.py:36-52, although the loss reads the final layer at the batch's rows only).  Layer K is needed at the
 * batch's rows S, layer K - 1 at S and their neighbours, and so on; the gradient flows back through the same sets.  On a
 * graph much larger than the batch's K-hop neighbourhood most of every product is work nobody reads.
 * idg_graph_expand_rows: out_rows = in_rows | {columns of the stored entries of the rows flagged in in_rows} (bitmaps of
 *   n_rows bits, distinct buffers) — one hop.
 * idg_propagate_mean_fields_f32: idg_propagate_mean_f32 with layer k producing the rows of layer_rows[k-1] only (host
 *   array of K device bitmaps; layer_rows[K-1] = the batch's rows; each set must contain the neighbours of the next).
 *   Rows outside the sets keep whatever the buffers held.  Same bits on the produced rows as the full propagation.
 * idg_propagate_mean_bwd_adam_fields_f32: idg_propagate_mean_bwd_adam_f32 where step k's input is known to be zero
 *   outside step_rows[k-1] (step_rows[0] = live rows of gout; NULL = dense; the last step is always dense: it carries
 *   the Adam update of every row).  Same bits as the unrestricted call. */
int idg_graph_expand_rows(const idg_graph* g, const uint32_t* in_rows, uint32_t* out_rows, void* stream);
/* The same hop on a graph of any shape, as float flags over the COLUMNS (caller-zeroed, n_cols floats): col_flags[c] =
 * 1.0f for every column of a stored entry of a row flagged in in_rows (n_rows bits).  The ranks of the sharded step sum
 * these to agree on the item rows a batch's users touch. */
int idg_graph_flag_cols(const idg_graph* g, const uint32_t* in_rows, float* col_flags, void* stream);
/* ... and as a bitmap over the columns (n_cols bits, NOT cleared here: col_bits |= the hop, so the row slices of one
 * matrix can mark into one bitmap).  The sharded step marks the users that reach the touched items this way. */
int idg_graph_mark_cols(const idg_graph* g, const uint32_t* in_rows, uint32_t* col_bits, void* stream);
int idg_propagate_mean_fields_f32(const idg_graph* g, const float* E0, float* out, const uint32_t* const* layer_rows, int K,
                                  int include_layer0, int64_t d, void* ws, void* stream);
int idg_propagate_mean_bwd_adam_fields_f32(const idg_graph* g, const float* gout, const uint32_t* const* step_rows, float* gE0,
                                           int K, int include_layer0, int64_t d, int accumulate, float* param,
                                           float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2,
                                           double eps, int64_t step, void* ws, void* stream);

/* A copy of `g` with NEW VALUES on the same structure and schedule, taken from a DEVICE CSR (indptr int64 [n_rows+1],
 * indices int32 ascending per row, values fp32) that holds every entry of g (it may hold more): entry (r, c) takes the
 * value stored for (r, c) there.  This is how a per-epoch sub-graph gets onto the device without a host-side tile
 * schedule: SGL's edge-dropped views (tools.create_adj_mat, tools.py:67-92; models/SGL.py:130-143) are the full
 * adjacency's handle with dropped interactions as explicit zeros and the kept ones re-normalised.  Same ownership
 * rules as idg_graph_masked_copy; the flags (symmetry) are g's — the caller passes symmetric values. */
int idg_graph_revalued_copy(const idg_graph* g, const int64_t* d_indptr, const int32_t* d_indices,
                            const float* d_values, void* stream, idg_graph** out);

/* values_out[k] = kept(edge_of_entry[k]) ? (dinv[row_of_entry[k]] * 1.0f) * dinv[col_of_entry[k]] : 0 for the nnz
 * entries of a bipartite adjacency in CSR order (all arrays on the device): the float32 arithmetic of
 * degree_matrix.dot(adjacency_matrix).dot(degree_matrix) in tools.create_adj_mat (tools.py:84-90) on the interactions
 * whose bit is set in kept_bits (bit e = interaction e of inter_graph.nonzero()'s order); dinv = d^-1/2 of the kept
 * graph, formed by the caller with the reference's own np.power expression. */
int idg_subgraph_values_f32(int64_t nnz, const int32_t* row_of_entry, const int32_t* col_of_entry,
                            const int32_t* edge_of_entry, const uint32_t* kept_bits, const float* dinv,
                            float* values_out, void* stream);
/* info[0..7] = n_rows, n_cols, nnz, n_tiles, n_long_rows, n_long_chunks, split_threshold, flags.  n_tiles: the workgroups
 * of a dense launch on a cache-resident panel — the tiles of the length-balanced schedule when the handle carries one
 * (idg_graph_schedule_info reports both schedules). */
int idg_graph_info(const idg_graph* g, int64_t info[8]);
/* The handle's two tile schedules: info[0..3] of the one every launch can run on, info[4..7] of the length-balanced one
 * the dense launches take while the gathered panel is cache resident (all 0 when the handle carries none: switched off,
 * a panel that is not cache resident at d = 64, EXACT_ORDER rows longer than a tile, a masked / revalued copy).  Each:
 * tiles, sum of the vrows' rounds (max(1, ceil(entries / 8))), sum over the tiles of 16 x the makespan of the tile's
 * vrows drawn in list order by 16 lane groups (rounds / that = the share of a resident tile's lane groups that work,
 * d = 64), device bytes of the schedule (entry list, vrow tables, tiles, split-row table).  A diagnostic: reads the
 * tables back from the device with blocking copies. */
int idg_graph_schedule_info(const idg_graph* g, int64_t info[8]);
/* The split schedule, so a checker can restate the exact summation order.  Define
 *   SEG(entries, S): cut the entry range into consecutive segments of S stored entries, each a
 *   sequential fmaf chain from +0; combine the segment partials p_0, p_1, ... 4-way strided:
 *   s_q = p_q + p_{q+4} + p_{q+8} + ... (left to right) for q = 0..3, result = ((s_0 + s_1) + s_2) + s_3
 *   (absent s_q skipped).
 * Row long_rows[i] with chunk_len[i] == 0 is SEG(row, seg_len[i]).  With chunk_len[i] = C > 0 the row is
 * first cut into consecutive chunks of C entries, chunk sums c_k = SEG(chunk k, seg_len[i]), and the c_k are
 * combined by the same 4-way strided rule.  Every other row is one sequential chain.
 * The arrays hold n_long_rows (info[4]) elements; any may be NULL. */
int idg_graph_long_rows(const idg_graph* g, int64_t* long_rows, int64_t* seg_len, int64_t* chunk_len);

/* Y = A.X  (torch.sparse.mm(Graph, X): models/LightGCN.py:44, SimGCL.py:48, XSimGCL.py:51,
 * NGCF.py:85, SGL.py:48,50).  X [n_cols, d], Y [n_rows, d] row-major fp32 with leading
 * dimensions ldx/ldy (elements).  If addend != NULL: Y = A.X + addend (addend [n_rows,d],
 * leading dimension ldy) — the autograd chain rule of the layer mean uses this form.
 * ws: idg_spmm_workspace_bytes(g, d) bytes of device scratch (may be NULL when that is 0). */
size_t idg_spmm_workspace_bytes(const idg_graph* g, int64_t d);
int idg_spmm_f32(const idg_graph* g, const float* X, int64_t ldx, float* Y, int64_t ldy,
                 const float* addend, int64_t d, void* ws, void* stream);

/* The same product with the whole fused epilogue exposed, for callers that assemble the layer
 * loop themselves (the user-row-sharded multi-GPU path, where an all-reduce sits between the
 * layers):  t = A.X (+ addend);  Y = t (if Y);  s = (sum_in ? sum_in + t : t) / div;
 * sum_out (+)= s (if sum_out; += when accumulate).  All panels share ldy.  out_rows (nullable):
 * bitmap of the output rows to produce; the others are left untouched.  x_rows (nullable): bitmap of the live rows of
 * X; the others are zero by agreement and are not read. */
int idg_spmm_ex_f32(const idg_graph* g, const float* X, int64_t ldx, float* Y, const float* addend,
                    const float* sum_in, float* sum_out, int64_t ldy, float div, int accumulate,
                    const uint32_t* out_rows, const uint32_t* x_rows, int64_t d, void* ws,
                    void* stream);

/* The same product with EVERY epilogue option as a struct (idg_spmm_ex_f32 is the subset without sum_in2 / sum_in3, mask
 * and Adam).  In order, for each produced row r:
 *   t = (A.X)[r]  (+ addend[r] if live(r));  Y[r] = t (if Y);
 *   s = live(r) && sum_in ? ((sum_in[r] + sum_in2[r]) + sum_in3[r]) + t : t   (absent terms skipped; this is the layer
 *       mean's left-to-right order, models/LightGCN.py:47-48);  s = s / div;
 *   sum_out[r] = accumulate && live(r) ? sum_out[r] + s : s (if sum_out);
 *   adam_param != NULL: the Adam update of row r of (param, exp_avg, exp_avg_sq) with gradient sum_out[r]
 *       (trainer.py:54-56; same arithmetic as idg_adam_step_f32; dense launches only).
 * live(r) = mask == NULL or bit r of mask: rows of addend / sum_in* / the accumulate target whose bit is clear are zero
 * by agreement and are NOT read (they may hold anything).  out_rows: produce only these rows; x_rows: rows of X outside
 * are zero and not read; the two may be combined (a backward product between two small row sets). */
typedef struct idg_epilogue {
  float* Y;
  const float* addend;
  const float* sum_in;
  const float* sum_in2;
  const float* sum_in3;
  float* sum_out;
  int64_t ldy;
  float div;
  int accumulate;
  const uint32_t* mask;
  float* adam_param;
  float* adam_exp_avg;
  float* adam_exp_avg_sq;
  double adam_lr, adam_beta1, adam_beta2, adam_eps;
  int64_t adam_step;
  int adam_discard_grad; /* != 0: the finished gradient feeds the update and is not written to sum_out (which is still
                            READ at live rows when accumulate is set): one [n, d] write less per step */
  /* EGCF's activated layers (models/EGCF.py:46-84: activation_layer(torch.sparse.mm(...)), nn.Tanh) and their backward:
   * applied to t = (A.X)[r] (+ addend[r]) of the rows r < act_rows (0: every row) BEFORE Y / sum_out see it.
   * IDG_ACT_TANH: t = tanh(t).  IDG_ACT_TANH_BWD: t = t * (1 - act_src[r]^2), act_src = the tanh outputs the forward
   * layer saved (torch's tanh_backward).  Not together with Adam; with out_rows or with x_rows, not both. */
  int act;
  const float* act_src;
  int64_t act_rows;
  /* The finished row t (after addend / activation) ALSO — or only: Y may then be NULL — as 24-bit values in idg_pack24_f32's
   * format, three words per four values at y24 + (r * ldy + f) / 4 * 3: the sharded step's packed exchange lets the product
   * write its partial straight into the send buffer (one fp32 write and one pack pass less per exchanged panel).  Dense
   * launches (x_rows allowed, out_rows not), tiled widths, not with Adam. */
  uint32_t* y24;
} idg_epilogue;
#define IDG_ACT_TANH 1
#define IDG_ACT_TANH_BWD 2
int idg_spmm_epi_f32(const idg_graph* g, const float* X, int64_t ldx, int64_t d, const idg_epilogue* epilogue,
                     const uint32_t* out_rows, const uint32_t* x_rows, void* ws, void* stream);
/* out[r, :] = grad[r, :] * (1 - y[r, :]^2) for the rows flagged in `rows` (NULL: every row) of [n, d] panels: the backward
 * of y = tanh(z) where the chain starts — EGCF's summed layer outputs at the batch's rows (models/EGCF.py:60,77).  Other
 * rows of out are left untouched. */
int idg_rows_tanh_bwd_f32(const float* grad, const float* y, const uint32_t* rows, int64_t n, int64_t d, float* out,
                          void* stream);

/* One perturbed layer (models/XSimGCL.py:51-54): Y = A.X;  Y += sign(Y) * normalize(u, dim=-1) * eps,
 * u ~ U[0,1)^d from Philox4x32-10(seed; stream_id, row, feature block).  d in {32,...,512}.
 * out_rows (nullable): bitmap of the rows to produce.  Layer k of idg_propagate_mean_noise_f32(seed, s)
 * draws from stream s * 64 + k: the same layer can be re-produced on its own. */
int idg_spmm_noise_f32(const idg_graph* g, const float* X, int64_t ldx, float* Y, int64_t ldy,
                       const uint32_t* out_rows, int64_t d, float eps, uint64_t seed,
                       uint64_t stream_id, void* ws, void* stream);
/* The perturbation alone, Y[r] = X[r] + sign(X[r]) * normalize(u_r) * eps with the same generator and arithmetic
 * as the epilogue form, for all n rows or the rows of a bitmap (nullable).  Lets passes that share a product
 * (SimGCL: A.E0 feeds the clean pass and both perturbed views) perturb it without multiplying again. */
int idg_perturb_f32(const float* X, float* Y, int64_t n, int64_t d, const uint32_t* rows, float eps,
                    uint64_t seed, uint64_t stream_id, void* stream);

/* SimGCL's encoder passes of one step (models/SimGCL.py:63-65) — the clean layer mean and n_views (1..2)
 * perturbed ones, layer 0 not in the mean — as one call: the first product A.E0 is computed once, each view
 * perturbs its own copy (sub-stream 0 of (seeds[i], stream_ids[i])) and continues with sub-streams 1..K-1 exactly as
 * idg_propagate_mean_noise_f32(X1, K - 1, include_layer0 = 1) would; with out_rows the last layer of ALL passes is ONE
 * launch of a multi-panel row-restricted kernel.  Same values as composing idg_spmm_f32, idg_perturb_f32,
 * idg_propagate_mean_f32 and idg_propagate_mean_noise_f32 by hand.  K >= 2, tiled d.
 * out_views: HOST array of n_views device pointers.  ws: idg_propagate_views_workspace_bytes. */
size_t idg_propagate_views_workspace_bytes(const idg_graph* g, int64_t d, int n_views);
int idg_propagate_views_f32(const idg_graph* g, const float* E0, int K, int64_t d, float eps, int n_views,
                            const uint64_t* seeds, const uint64_t* stream_ids, float* out_clean,
                            float* const* out_views, const uint32_t* out_rows, void* ws, void* stream);

/* LightGCN.aggregate (models/LightGCN.py:36-52) / SimGCL.aggregate(perturbed=False)
 * (models/SimGCL.py:39-60): out = mean over layers of E_k, E_{k+1} = A.E_k, k < K,
 * E_0 included iff include_layer0.  Running sum left-to-right then a true division by the
 * layer count — the order torch.mean(torch.stack(..)) produces on CPU.
 * E0, out: [n, d] contiguous.  ws: idg_propagate_workspace_bytes(g, d). */
size_t idg_propagate_workspace_bytes(const idg_graph* g, int64_t d);
/* out_rows (nullable): bitmap of the rows of `out` the caller will read.  The LAST layer's product
 * feeds nothing but the mean, so with a bitmap it is evaluated for the flagged rows only (bit-
 * identical values there; for K <= 3 every other row of `out` is left untouched, for K > 3 `out`
 * carries the running sum and its other rows hold the sum of the earlier layers).  A training step
 * reads the mean at the <= 3B rows of its batch: idg_bpr_touch_rows builds that bitmap from the indices. */
int idg_propagate_mean_f32(const idg_graph* g, const float* E0, float* out,
                           const uint32_t* out_rows, int K, int include_layer0, int64_t d, void* ws,
                           void* stream);
/* SimGCL.aggregate(perturbed=True) (models/SimGCL.py:47-56): as idg_propagate_mean_f32, but after
 * every product X <- A.X the layer is perturbed in place, X += sign(X) * normalize(u, dim=-1) * eps
 * with u ~ U[0,1)^d, before it enters the running sum and feeds the next layer.  u comes from
 * Philox4x32-10 keyed by (seed, stream_id, layer, row, feature block): reproducible for a given
 * (seed, stream_id), independent of the tile schedule; like the reference's device generator it
 * matches a CPU run statistically, not bit for bit.  d in {32, 64, 128, 256, 512}.  out_rows as in
 * idg_propagate_mean_f32 (a row's noise depends on that row only: the produced rows are the same).
 * The gradient w.r.t. E0 is idg_propagate_mean_bwd_f32's (sign() has zero gradient, u is constant). */
int idg_propagate_mean_noise_f32(const idg_graph* g, const float* E0, float* out,
                                 const uint32_t* out_rows, int K, int include_layer0, int64_t d,
                                 float eps, uint64_t seed, uint64_t stream_id, void* ws, void* stream);

/* Backward of the above for a SYMMETRIC graph: gE0 = (1/cnt)(c0.g + A(g + A(g + ... A g))),
 * the Horner form of autograd's chain through K torch.sparse.mm nodes and the mean.
 * accumulate != 0: gE0 += (the ego-embedding regulariser's gradient is already there). */
/* gout_mask (nullable): bitmap, bit r of word r/32 set iff row r of gout is live.  Rows with a
 * clear bit are taken as zero and never read — a training batch touches <= 3B rows of gout, so
 * the first backward product skips most of its gathers (exact: fmaf(v, 0, acc) == acc) and gout
 * needs no zero-fill.  With accumulate != 0 the same bitmap governs gE0: flagged rows are added
 * to, every other row is overwritten (gE0 needs no zero-fill either).  Produced by
 * idg_bpr_backward_f32's `touched` argument. */
int idg_propagate_mean_bwd_f32(const idg_graph* g, const float* gout, const uint32_t* gout_mask,
                               float* gE0, int K, int include_layer0, int64_t d, int accumulate,
                               void* ws, void* stream);
/* The same backward followed by the dense Adam step on the [n, d] parameter panel E0 the gradient
 * belongs to (loss.backward() + optimizer.step(), utility/utility_train/trainer.py:54-56): each
 * finished gradient row is consumed by its Adam update in the epilogue of the last product instead
 * of being re-read by a second kernel.  gE0 still receives the gradient.  Bit-identical to
 * idg_propagate_mean_bwd_f32 + idg_adam_step_f32 (which is what runs when K < 2 or d is not a tiled
 * width).  Hyper-parameters as idg_adam_step_f32. */
#define IDG_ADAM_DISCARD_GRAD 2 /* OR-ed into `accumulate` of the two calls below: the finished gradient feeds the update and is
                                * NOT written back to gE0 (17.8 MB per step less to store on the yelp2018 shape) */
int idg_propagate_mean_bwd_adam_f32(const idg_graph* g, const float* gout, const uint32_t* gout_mask,
                                    float* gE0, int K, int include_layer0, int64_t d, int accumulate,
                                    float* param, float* exp_avg, float* exp_avg_sq, double lr,
                                    double beta1, double beta2, double eps, int64_t step, void* ws,
                                    void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: fused gather + BPR + L2-reg loss and gradients
 * (LightGCN.forward models/LightGCN.py:54-72; losses.get_bpr_loss / get_reg_loss
 *  utility/utility_function/losses.py:4-21; and their autograd backward)
 * ---------------------------------------------------------------------------------- */
/* final/ego: [n, d] panels, rows [0,num_users) users then items.  users/pos/neg: int64[B]
 * (pos/neg are item ids, NOT offset by num_users).
 * loss[0] = mean_i -log(sigmoid(<f_u,f_p> - <f_u,f_n>) + 1e-7)
 * loss[1] = reg_lambda * sum over the three ego blocks of 0.5*||block||_F^2 / B
 * g_final[n,d] += d loss[0] / d final   (rows scatter-added, duplicates accumulate)
 * g_ego  [n,d] += d loss[1] / d ego
 * touched (nullable, deterministic forms only, g_final != g_ego): a zeroed bitmap of ceil(n/32)
 * words; the rows of g_final AND g_ego this batch reaches (the same rows) are then STORED (not
 * accumulated) and their bits set, every other row of both panels is left untouched and must
 * not be read — hand the bitmap to idg_propagate_mean_bwd_f32, which reads flagged rows only.
 * g_final / g_ego must be zeroed (or hold a gradient to accumulate into) by the caller;
 * either may be NULL to skip that gradient.  final == ego is the MFBPR case
 * (models/MFBPR.py:29-42).  deterministic != 0: duplicate rows are summed in batch order
 * (run-to-run reproducible); 0: float atomics.
 * ws: idg_bpr_workspace_bytes(B, d). */
size_t idg_bpr_workspace_bytes(int64_t B, int64_t d);
int idg_bpr_fused_f32(const float* final_panel, const float* ego_panel, int64_t num_users,
                      int64_t n, const int64_t* users, const int64_t* pos, const int64_t* neg,
                      int64_t B, int64_t d, float reg_lambda, float* loss, float* g_final,
                      float* g_ego, int deterministic, uint32_t* touched, void* ws, void* stream);
/* The same with final rows and ego rows of DIFFERENT widths and an optional item-only regulariser — NGCF (models/NGCF.py:
 * 108-128): the scored rows are the concatenation of the layer outputs ([n, (K+1) d]), the regulariser covers
 * item_embedding(positive) and item_embedding(negative) only (two blocks; reg_users = 0: the user block contributes
 * nothing to loss[1] and a zero row to g_ego).  g_final [n, d_final], g_ego [n, d_ego]; deterministic scatter only
 * (1, or IDG_BPR_PLANNED with the plan in ws). */
int idg_bpr_fused_ex_f32(const float* final_panel, int64_t d_final, const float* ego_panel, int64_t d_ego,
                         int64_t num_users, int64_t n, const int64_t* users, const int64_t* pos, const int64_t* neg,
                         int64_t B, float reg_lambda, int reg_users, float* loss, float* g_final, float* g_ego,
                         int deterministic, uint32_t* touched, void* ws, void* stream);
/* The same computation as two calls, for callers that sit under an autograd engine:
 * forward writes loss[2] and keeps per-triple coefficients in ws; backward (same ws, same
 * inputs) scatters the gradients scaled by upstream[0] (for loss[0]) and upstream[1] (for
 * loss[1]) — a DEVICE pointer to the two incoming gradient scalars, or NULL for 1, 1. */
/* deterministic = IDG_BPR_PLANNED: the sorted (row, slot) plan of THIS batch is already in ws,
 * put there by idg_bpr_plan_f32 (which depends on the indices only, so a caller can run it on
 * a second stream while the forward propagation is still in flight). */
/* bitmap[(r >> 5)] |= 1 << (r & 31) for r in {users[i], num_users + pos[i], num_users + neg[i]}: the
 * panel rows a batch touches.  bitmap: ceil(n/32) words, zeroed by the caller.  Index-only work. */
int idg_bpr_touch_rows(const int64_t* users, const int64_t* pos, const int64_t* neg, int64_t B,
                       int64_t num_users, uint32_t* bitmap, void* stream);
/* Clear a row bitmap of n_bits bits ((n_bits + 31) / 32 words) on `stream`. */
int idg_bitmap_clear(uint32_t* bitmap, int64_t n_bits, void* stream);

/* Gradient rows as a message, for data-parallel replicas (the reference trains on one device,
 * utility/utility_train/trainer.py:42-56 — the replicas reproduce its loss at batch size world x B).
 * After idg_bpr_fused_f32 / idg_bpr_backward_f32 with a touched-row bitmap and the sorted plan in ws, g_final holds
 * one stored row per distinct row of the batch.  idg_bpr_pack_rows_f32 copies them, the sorted row keys of the plan
 * and the two losses into `message` (idg_bpr_rows_message_floats(B, d) floats).  Replicas all-gather their messages;
 * idg_bpr_unpack_rows_f32 then clears `touched` (n bits; unless told it is clear) and merges `world` (<= 64) consecutive messages in ONE launch:
 * the lowest rank naming a row owns it and adds the ranks' rows IN RANK ORDER — g_final rows averaged over ranks,
 * g_ego = the regulariser's gradient (reg_lambda / (world B)) x multiplicity x ego row, loss[2] = mean of the ranks'
 * losses — so that every replica obtains the same bits; at world 1 the panels equal what the scatter left.  The
 * backward propagation then runs on the union bitmap `touched`. */
size_t idg_bpr_rows_message_floats(int64_t B, int64_t d);
/* clear_bitmap (nullable) / clear_bits: a bitmap the pack launch zeroes on the way — hand it the `touched` of the
 * coming merge and pass touched_is_clear = 1 there, and no memset sits between the all-gather and the merge. */
int idg_bpr_pack_rows_f32(const void* ws, int64_t B, int64_t d, const float* g_final, const float* loss,
                          float* message, uint32_t* clear_bitmap, int64_t clear_bits, void* stream);
int idg_bpr_unpack_rows_f32(const float* messages, int world, int64_t B, int64_t d, int64_t n,
                            const float* ego_panel, float reg_lambda, float* g_final, float* g_ego,
                            uint32_t* touched, int touched_is_clear, float* loss, void* stream);
#define IDG_BPR_PLANNED 2
/* OR-ed into `deterministic` together with a `touched` bitmap: the bitmap ALREADY holds exactly the batch's rows
 * (idg_bpr_touch_rows on the same ids) — the scatter stores its rows as with any touched bitmap but does not write the
 * bitmap, so unit / compacted-input lists registered for it stay valid for the backward products that follow. */
#define IDG_BPR_TOUCHED_PRESET 4
int idg_bpr_plan_f32(const int64_t* users, const int64_t* pos, const int64_t* neg, int64_t B,
                     int64_t num_users, int64_t n, void* ws, void* stream);
/* idg_bpr_plan_f32 + idg_bpr_touch_rows in one pass over the ids: the plan's first kernel also sets the batch's bits in
 * `bitmap` (ceil(n / 32) words, zeroed by the caller) — one launch less per step. */
int idg_bpr_plan_rows_f32(const int64_t* users, const int64_t* pos, const int64_t* neg, int64_t B, int64_t num_users,
                          int64_t n, void* ws, uint32_t* bitmap, void* stream);
int idg_bpr_forward_f32(const float* final_panel, const float* ego_panel, int64_t num_users,
                        int64_t n, const int64_t* users, const int64_t* pos, const int64_t* neg,
                        int64_t B, int64_t d, float reg_lambda, float* loss, void* ws,
                        void* stream);
int idg_bpr_backward_f32(const float* final_panel, const float* ego_panel, int64_t num_users,
                         int64_t n, const int64_t* users, const int64_t* pos, const int64_t* neg,
                         int64_t B, int64_t d, float reg_lambda, const float* upstream,
                         float* g_final, float* g_ego, int deterministic, uint32_t* touched, void* ws,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: weight gradient of a thin dense layer  (autograd of torch.matmul(side, W) in NGCF's
 * per-layer transforms, models/NGCF.py:91-99):  w_grad[d1, d2] (+)= X^T . G,  X [n, d1] (leading
 * dimension ldx), G [n, d2] (ldg), row-major fp32.  All reduction (K = n), no output to speak of:
 * rows are cut into slices summed in slice order (deterministic).  ws: *_workspace_bytes.
 * ---------------------------------------------------------------------------------- */
size_t idg_linear_wgrad_workspace_bytes(int64_t n, int64_t d1, int64_t d2);
int idg_linear_wgrad_f32(const float* X, int64_t ldx, const float* G, int64_t ldg, int64_t n,
                         int64_t d1, int64_t d2, float* w_grad, int accumulate, void* ws,
                         void* stream);

/* The four parameter gradients of one NGCF layer in one pass over the rows: out = [g W_gcn (d1 x d2) | g b_gcn (d2) |
 * g W_bi (d1 x d2) | g b_bi (d2)] with g W_gcn = side^T gT, g W_bi = bi^T gT (bi = ego * side as idg_ngcf_transform_f32
 * left it), g b_* = column sums of gT (models/NGCF.py:91-99 under autograd).  d1, d2 multiples of 64; deterministic. */
size_t idg_ngcf_wgrad_workspace_bytes(int64_t d1, int64_t d2);
int idg_ngcf_wgrad_f32(const float* side, const float* bi, const float* gT, int64_t n, int64_t d1, int64_t d2,
                       float* out, void* ws, void* stream);

/* NGCF's two per-layer transforms (models/NGCF.py:88-99: torch.matmul(side, W_gcn) and torch.matmul(ego * side, W_bi))
 * on the fp32 matrix cores in one pass over the rows: S[n, d2] = side . W1 + (ego * side) . W2 (the two bias rows are
 * added by idg_ngcf_tail_f32, which takes S as its S1 with S2 = NULL); BI (nullable) receives ego * side [n, d1], the
 * left operand of W2's weight gradient.  Backward: g_side = gS . W1^T + (gS . W2^T) * ego, g_ego = (gS . W2^T) * side
 * (weight gradients: idg_linear_wgrad_f32 on (side, gS) and (BI, gS)).  W1, W2: [d1, d2] row-major.
 * Forward needs d1 % 64 == 0 and d2 % 32 == 0, backward d2 % 64 == 0 and d1 % 32 == 0, panels 16-byte aligned. */
int idg_ngcf_transform_f32(const float* side, const float* ego, const float* W1, const float* W2, int64_t n,
                           int64_t d1, int64_t d2, float* S, float* BI, void* stream);
int idg_ngcf_transform_bwd_f32(const float* gS, const float* side, const float* ego, const float* W1,
                               const float* W2, int64_t n, int64_t d1, int64_t d2, float* g_side, float* g_ego,
                               void* stream);

/* NGCF's per-layer tail after the two thin GEMMs (models/NGCF.py:95-108), one pass over the rows:
 *   t = (S1 + b1) + (S2 + b2);  a = leaky_relu(t, negative_slope);  E = dropout(a, p);  N = normalize(E, dim=1)
 * (S1 = side.W_gcn, S2 = (ego * side).W_bi, all [n, d] row-major; b1, b2 [d]; S2 = NULL: S1 already holds the sum of
 * the two, as idg_ngcf_transform_f32 produces it).  The dropout mask is a counter-based
 * function of (seed, stream_id, row, feature) — always applied, as in the reference, where nn.Dropout is built
 * inside aggregate() — and regenerated by the backward call, which needs only E:
 *   gT = d loss / d t  given  gE (gradient through E as the next layer's input, nullable) and gN (through N, nullable);
 * then gS1 = gS2 = gT, g b1 = g b2 = column sums of gT. */
int idg_ngcf_tail_f32(const float* S1, const float* S2, const float* b1, const float* b2, int64_t n,
                      int64_t d, float negative_slope, float p, uint64_t seed, uint64_t stream_id,
                      float* E, float* N, void* stream);
int idg_ngcf_tail_bwd_f32(const float* E, const float* gE, const float* gN, int64_t n, int64_t d,
                          float negative_slope, float p, uint64_t seed, uint64_t stream_id, float* gT,
                          void* stream);
/* The forms a fused, autograd-free NGCF step uses (id-grec_amd/ngcf.py): N written with leading dimension ldn — straight
 * into layer l's slot of the concatenated final rows (torch.cat(all_embeddings, dim=1), models/NGCF.py:108); gN read with
 * leading dimension ldgn and only at the rows flagged in gn_rows (NULL: every row) — d loss / d final is stored at the
 * batch's rows only; rows no gradient flows into get gT = 0. */
int idg_ngcf_tail_ex_f32(const float* S1, const float* S2, const float* b1, const float* b2, int64_t n, int64_t d,
                         float negative_slope, float p, uint64_t seed, uint64_t stream_id, float* E, float* N,
                         int64_t ldn, void* stream);
int idg_ngcf_tail_bwd_ex_f32(const float* E, const float* gE, const float* gN, int64_t ldgn, const uint32_t* gn_rows,
                             int64_t n, int64_t d, float negative_slope, float p, uint64_t seed, uint64_t stream_id,
                             float* gT, void* stream);
/* One NGCF layer as ONE kernel per direction, d = 64 (csrc/idg_ngcf.hip; models/NGCF.py:88-108 and its autograd):
 *   forward : E = dropout(leaky_relu(side . W1 + (ego * side) . W2 + b1 + b2)), N = normalize(E)  — N with leading dimension
 *             ldn (layer l's slot of the concatenated final rows); nothing else is stored;
 *   backward: from E, gE (nullable), gN (nullable; ldgn, gn_rows as idg_ngcf_tail_bwd_ex_f32), side and the layer's input
 *             ego: g_side, g_ego [n, 64] and w_grads = [g W1 (64 x 64) | g b1 (64) | g W2 (64 x 64) | g b2 (64)].
 * E, N, g_side, g_ego are bit-identical to idg_ngcf_transform_f32 + idg_ngcf_tail_ex_f32 and their backward forms; the
 * parameter gradients are sums over the rows in a fixed order of their own (slices of rows on persistent workgroups).
 * Any other d: IDG_E_INVALID (use the chain).  ws: idg_ngcf_layer_bwd_workspace_bytes(d). */
int idg_ngcf_layer_fwd_f32(const float* side, const float* ego, const float* W1, const float* W2, const float* b1,
                           const float* b2, int64_t n, int64_t d, float negative_slope, float p, uint64_t seed,
                           uint64_t stream_id, float* E, float* N, int64_t ldn, void* stream);
size_t idg_ngcf_layer_bwd_workspace_bytes(int64_t d);
int idg_ngcf_layer_bwd_f32(const float* E, const float* gE, const float* gN, int64_t ldgn, const uint32_t* gn_rows,
                           const float* side, const float* ego, const float* W1, const float* W2, int64_t n, int64_t d,
                           float negative_slope, float p, uint64_t seed, uint64_t stream_id, float* g_side, float* g_ego,
                           float* w_grads, void* ws, void* stream);
/* One LR-GCCF layer (E = dropout(side . W + b); no bilinear term, no activation, no row norm) as ONE kernel per direction,
 * d = 64 (csrc/idg_gccf.hip).  The mask is idg_ngcf_tail_f32's published function of (seed, stream_id, row, feature).
 *   forward : E[r, 0:d] = keep(r, .) * (side[r, .] . W + b), E written with leading dimension lde (layer l's slot of the
 *             concatenated final rows); bytes outside columns 0 .. d-1 of a row, and rows >= n, are not touched;
 *   backward: gT = keep * ((gE or 0) + (gN at the rows flagged in gn_rows, read with ldgn)); gn_rows = NULL: every row;
 *             what gN holds off the flagged rows is never read; at least one of gE, gN must be given.  No saved activation
 *             is needed.  g_side = gT . W^T [n, 64];  w_grads = [gW (64 x 64) = side^T . gT | gb (64) = column sums of gT].
 * The sums over rows run in a fixed order (slices of rows on persistent workgroups, added in slice order): two runs give
 * the same bits.  Any other d, NULL or misaligned pointers (panels and, in the backward, W: 16 bytes), n <= 0, a leading
 * dimension below d or not a multiple of 4, p outside [0, 1) and outputs that overlap inputs: IDG_E_INVALID before any
 * device work.  ws: as many bytes as idg_gccf_layer_bwd_workspace_bytes returns for d (0 for a width that is not built). */
int idg_gccf_layer_fwd_f32(const float* side, const float* W, const float* b, int64_t n, int64_t d, float p, uint64_t seed,
                           uint64_t stream_id, float* E, int64_t lde, void* stream);
size_t idg_gccf_layer_bwd_workspace_bytes(int64_t d);
int idg_gccf_layer_bwd_f32(const float* gE, const float* gN, int64_t ldgn, const uint32_t* gn_rows, const float* side,
                           const float* W, int64_t n, int64_t d, float p, uint64_t seed, uint64_t stream_id, float* g_side,
                           float* w_grads, void* ws, void* stream);
/* One GCMC layer (models/GCMC.py:73-90) as ONE kernel per direction, d = 64 (csrc/idg_gcmc.hip): two CHAINED products with
 * the activation between them, the mask, and a row normalisation behind the mask.
 *   forward : H = side . Wg + bg;  A = leaky_relu(H);  M = A . Wm + bm;  T = keep * M, written contiguous [n, 64] (the next
 *             layer's product input and the only activation the backward reads);  N = T / max(|T|_2, 1e-12), written with
 *             leading dimension ldn (layer l's slot of the concatenated final rows).  H and A are not stored; nothing is
 *             written outside rows 0 .. n-1 of T and of the slot;
 *   backward: N and its denominator rebuilt from T;  gM = keep * ((gE or 0) + J_normalize(T)^T gN at the rows flagged in
 *             gn_rows) — gn_rows = NULL: every row; what gN holds off the flagged rows is never read; a row below the clamp
 *             has the Jacobian I / 1e-12 (idg_ngcf_tail_bwd_ex_f32's convention); at least one of gE, gN must be given.
 *             H is recomputed from side with the forward's operand order (the forward's bits), the slope applies where
 *             H <= 0.  g_side = ((gM . Wm^T) o leaky_relu'(H)) . Wg^T [n, 64];
 *             w_grads = [gWg (64 x 64) = side^T . gH | gbg (64) | gWm (64 x 64) = A^T . gM | gbm (64)].
 * The sums over rows run in a fixed order (slices of rows on persistent workgroups, added in slice order): two runs give
 * the same bits.  Any other d, NULL or misaligned pointers (panels and, in the backward, Wg and Wm: 16 bytes), n <= 0, a
 * leading dimension below d or not a multiple of 4, p outside [0, 1) and outputs that overlap inputs or each other:
 * IDG_E_INVALID before any device work.  ws: as many bytes as idg_gcmc_layer_bwd_workspace_bytes returns for d (0 for a
 * width that is not built). */
int idg_gcmc_layer_fwd_f32(const float* side, const float* Wg, const float* bg, const float* Wm, const float* bm, int64_t n,
                           int64_t d, float negative_slope, float p, uint64_t seed, uint64_t stream_id, float* T, float* N,
                           int64_t ldn, void* stream);
size_t idg_gcmc_layer_bwd_workspace_bytes(int64_t d);
int idg_gcmc_layer_bwd_f32(const float* T, const float* gE, const float* gN, int64_t ldgn, const uint32_t* gn_rows,
                           const float* side, const float* Wg, const float* bg, const float* Wm, int64_t n, int64_t d,
                           float negative_slope, float p, uint64_t seed, uint64_t stream_id, float* g_side, float* w_grads,
                           void* ws, void* stream);
/* Glue of that step.  idg_copy_cols_f32: dst[r, 0:d] = src[r, 0:d] with leading dimensions ldd / lds.  idg_rows_add2_f32:
 * dst[r] += a[r] (+ b[r]) at the rows flagged in `rows`.  idg_colsum_f32: out[f] (+)= sum over the n rows of X[r, f] — the
 * gradient of a bias row broadcast over n rows (the differentiable layer tail's backward; the fused step gets it from
 * idg_ngcf_wgrad_f32) — slices of rows summed in slice order; ws: idg_colsum_workspace_bytes(d). */
size_t idg_colsum_workspace_bytes(int64_t d);
int idg_colsum_f32(const float* X, int64_t ldx, int64_t n, int64_t d, float* out, int accumulate, void* ws, void* stream);
int idg_copy_cols_f32(float* dst, int64_t ldd, const float* src, int64_t lds, int64_t n, int64_t d, void* stream);
int idg_rows_add2_f32(float* dst, int64_t ldd, const float* a, int64_t lda, const float* b, int64_t ldb,
                      const uint32_t* rows, int64_t n, int64_t d, void* stream);
/* IMP-GCN (models/IMPGCN.py:50-88; csrc/idg_group.hip), d = 64, fp32.
 *
 * idg_group_assign_f32: the group membership of every node, one launch.
 *     temp   = keep1 * leaky_relu((ego + side) . W_fc^T + b_fc)
 *     scores = keep2 * (temp . W_grp^T + b_grp)
 *   W_fc [64, 64], W_grp [G, 64]: nn.Linear's [out, in] layout; 1 <= G <= 8.  keep1 is idg_ngcf_tail_f32's published mask of
 *   (seed, stream_fc, row, feature < 64), keep2 the same function of (seed, stream_grp, row, g < G): 1 / (1 - p) where kept, 0
 *   where dropped; p = 0: no mask.  member[r] (one byte per node) = the bitmask of { g : scores[r, g] == max_g scores[r, :] }
 *   for r < num_users — compared by VALUE, so ties (several scores dropped to 0 over negative survivors; -0.0 against 0.0)
 *   give several bits — and (1 << G) - 1 for r >= num_users.  scores_out (nullable, [n, G]): the masked scores exactly as the
 *   kernel compared them.  temp is never stored; nothing is written outside member[0 .. n-1] and scores_out[0 .. n G - 1].
 *
 * idg_grouped_spmm_f32: one walk of a plain device CSR (indptr int64 [n + 1], indices int32 ascending per row, values fp32;
 *   square, n x n — the arrays idg_graph_revalued_copy takes) for all G sub-graph products A_g = D_g A D_g,
 *   D_g = diag([g in member[r]]):
 *     t_g[r] = sum_k values[k] * [g in member[col_k]] * (X_g[col_k] + V[col_k])            for g in member[r]
 *     Y_g[r] = t_g[r]                                   (Y nullable; group g at Y + g * y_group_stride floats)
 *     S[r]   = (S_in ? S_in[r] : 0) + t_g[r] for g in member[r], ascending      (S nullable; S_in may BE S)
 *   X: one shared [n, 64] panel (x_group_stride = 0) or G panels x_group_stride >= n * 64 floats apart; V (nullable): a
 *   shared [n, 64] addend of the INPUT.  By agreement — the library's x_rows convention — row r of Y_g with g not in
 *   member[r] is NOT written, and row c of a grouped X_g with g not in member[c] is NOT read: it may hold anything.
 *   x_rows (nullable, a SHARED X only) / v_rows (nullable): bitmaps of the rows of X / V that are live; the others count as
 *   zero and are not read.  A row with member 0 contributes nothing and receives nothing (its S is S_in or 0).
 *   The order of every sum is fixed and is no function of the launch: a row's entries in chunks of IDG_GROUP_CHUNK; inside
 *   a chunk four partial sums over the entries k = q (mod 4) in ascending k, added as (q0 + q1) + (q2 + q3); the chunks in
 *   chunk order.  No atomics: two calls give equal bits.  long_rows [n_long] (ascending rows longer than one chunk, ALL of
 *   them) with long_chunk0 [n_long + 1] (running count of their chunks; n_chunks in all) lets each chunk of such a row run on
 *   a wave of its own, through ws (as many bytes as idg_grouped_spmm_workspace_bytes returns) — the same order and bits as
 *   n_long = 0, where one wave walks the row.  Entries of the schedule that name no row or no long row are ignored.
 *
 * idg_group_grad_f32: out[r] = a * S[r] + (r flagged in rows ? b * gF[r] + GE[r] : 0); S nullable (counts as zero), S may BE
 *   out.  The ego gradient of the fused step: (1 / L) * the Horner chain's sum + (G / L) * d loss / d final and the
 *   regulariser's rows, both of which live at the batch's rows only.
 *
 * Any other d, NULL or misaligned pointers (panels, W_fc and ws 16 bytes; indptr 8; the rest 4), n <= 0 or >= 2^31, G outside
 * 1 .. 8, num_users outside 0 .. n, p outside [0, 1), group strides below n * 64 or no multiple of 4, x_rows with a grouped
 * X, v_rows without V, S_in without S, an inconsistent schedule, and outputs that overlap inputs or each other:
 * IDG_E_INVALID before any device work. */
#define IDG_GROUP_CHUNK 512
int idg_group_assign_f32(const float* ego, const float* side, const float* W_fc, const float* b_fc, const float* W_grp,
                         const float* b_grp, int64_t n, int64_t d, int G, int64_t num_users, float negative_slope, float p,
                         uint64_t seed, uint64_t stream_fc, uint64_t stream_grp, uint8_t* member, float* scores_out, void* stream);
int64_t idg_grouped_spmm_chunk(void);
size_t idg_grouped_spmm_workspace_bytes(int64_t n_chunks, int G);
int idg_grouped_spmm_f32(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, const float* values, int64_t d, int G,
                         const uint8_t* member, const float* X, int64_t x_group_stride, const uint32_t* x_rows, const float* V,
                         const uint32_t* v_rows, float* Y, int64_t y_group_stride, const float* S_in, float* S,
                         const int32_t* long_rows, const int32_t* long_chunk0, int64_t n_long, int64_t n_chunks, void* ws,
                         void* stream);
int idg_group_grad_f32(const float* S, float a, const float* gF, float b, const float* GE, const uint32_t* rows, int64_t n, int64_t d,
                       float* out, void* stream);
/* BIGCF's intent layer on rows row0 .. row0 + nrows - 1 of a panel (models/BIGCF.py:62-69; csrc/idg_intent.hip), one kernel
 * per direction, (d, k) = (64, 128), fp32:  S = X . W [., k],  P = softmax(S) (row maximum subtracted),  T = P . W^T,
 * F = X + T o Z.  Every panel, the bitmap and the noise are indexed by the GLOBAL row (the pointers are those of row 0);
 * row0 need not be a multiple of the 64-row tile.  Z = `noise`[row, feature] (a contiguous [., d] panel) when given, else
 * idg_vae_head_fwd_f32's published normal of (seed, stream_id, row, feature); noise_out (nullable, [., d]) receives the Z
 * that was used.  rows_bitmap (nullable = every row): a row whose bit is clear is neither read nor written, a tile with no
 * flagged row is skipped.
 *   backward: gT = (gT_in or 0) + gF o Z [never stored]; gt_rows (nullable = wherever rows_bitmap allows): gT_in is read at
 *             the flagged rows whose bit of gt_rows is set too, and counts as zero at the others (a training step's gT lives
 *             on the user and positive rows, its gF on the negative rows as well);  gP = gT . W;  gS = P o (gP - rowsum(P o gP));
 *             gX = gF + gS . W^T (written at the flagged rows only);  gW [d, k] = X^T . gS + gT^T . P (stored, not added).
 * P is recomputed from X and W and Z regenerated: no activation is saved.  gW is summed in a fixed order (row slices on
 * persistent workgroups, added in slice order): two runs give the same bits.  Any other (d, k), NULL or misaligned pointers
 * (panels and W: 16 bytes), nrows <= 0, row0 < 0, a leading dimension below d or not a multiple of 4 and outputs that
 * overlap inputs or each other: IDG_E_INVALID before any device work.  ws: as many bytes as idg_intent_bwd_workspace_bytes
 * returns for the widths (0 for widths that are not built).  idg_intent_noise_f32: that Z alone, noise_out[row, f] for rows row0 .. row0 + nrows - 1 of
 * a contiguous [., d] panel of ANY width d (the composed path of other widths draws the same noise). */
int idg_intent_noise_f32(int64_t row0, int64_t nrows, int64_t d, uint64_t seed, uint64_t stream_id, float* noise_out, void* stream);
int idg_intent_fwd_f32(const float* X, int64_t ldx, int64_t row0, int64_t nrows, const float* W, int64_t d, int64_t k,
                       const uint32_t* rows_bitmap, const float* noise, uint64_t seed, uint64_t stream_id, float* T, int64_t ldt,
                       float* F, int64_t ldf, float* noise_out, void* stream);
size_t idg_intent_bwd_workspace_bytes(int64_t d, int64_t k);
int idg_intent_bwd_f32(const float* gF, int64_t ldgf, const float* gT_in, int64_t ldgt, const uint32_t* gt_rows,
                       const uint32_t* rows_bitmap, const float* X, int64_t ldx, int64_t row0, int64_t nrows, const float* W, int64_t d, int64_t k, const float* noise,
                       uint64_t seed, uint64_t stream_id, float* gX, int64_t ldgx, float* gW, void* ws, void* stream);
/* HCCF's hypergraph layer on rows row0 .. row0 + nrows - 1 of ONE side of the panel (models/HCCF.py:56-74; csrc/idg_hyper.hip),
 * (d, h) = (64, 64), fp32:  Hb = E0 . W [., h],  H = M o Hb / keep,  L = H^T . X [h, d],  Y = H . L.  H is never stored: every
 * call recomputes it from E0 and W (one product order everywhere: the backward's H has the forward's bits) and regenerates
 * the mask.  Every panel and the mask are indexed by the GLOBAL row (the pointers are those of row 0); row0 need not be a
 * multiple of the 64-row tile.  M[row, c] = `mask`[row * h + c] != 0 (a uint8 panel [., h]) when given, else
 * idg_dropout's published keep function of (seed, stream_id, row, c) at p = 1 - keep; keep >= 1 keeps every element of the
 * generator's.  W, L, gL and gW are contiguous [64, 64].
 *   idg_hyper_latent_f32: L (stored) = sum over the rows of H[r, :]^T . X[r, :]; with gY as X it gives gL.  mask_out
 *     (nullable, uint8 [., h]) receives the mask that was used.
 *   idg_hyper_expand_f32: Y = H . L; with side (and next, which come together): next = side + Y; with total (nullable):
 *     total += next (+= Y without side).
 *   idg_hyper_bwd_f32: gX += H . gL;  gHb = (accumulate ? gHb : 0) + M o (gY . L^T + X . gL^T) / keep  ([., h] panel).
 *   idg_hyper_close_f32: gE0 += gHb . W^T;  gW [d, h] = E0^T . gHb (stored).
 * L, gL and gW are summed in a fixed order (row slices on persistent workgroups, added in slice order): two runs give the
 * same bits.  Any other (d, h), NULL or misaligned pointers (panels, matrices and ws 16 bytes, masks 4), nrows <= 0,
 * row0 < 0, keep <= 0, a leading dimension below 64 or not a multiple of 4, side without next, and outputs that overlap
 * inputs or each other: IDG_E_INVALID before any device work.  ws: as many bytes as the call's *_workspace_bytes returns (0
 * for widths that are not built; both are 512 slices of [64, 64] floats, one per resident workgroup). */
size_t idg_hyper_latent_workspace_bytes(int64_t d, int64_t h);
int idg_hyper_latent_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* X, int64_t ldx, int64_t row0,
                         int64_t nrows, float keep, const uint8_t* mask, uint64_t seed, uint64_t stream_id, float* L, uint8_t* mask_out,
                         void* ws, void* stream);
int idg_hyper_expand_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* L, int64_t row0, int64_t nrows,
                         float keep, const uint8_t* mask, uint64_t seed, uint64_t stream_id, float* Y, int64_t ldy, const float* side,
                         int64_t lds, float* next, int64_t ldn, float* total, int64_t ldtot, void* stream);
int idg_hyper_bwd_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* X, int64_t ldx, const float* gY,
                      int64_t ldgy, const float* L, const float* gL, int64_t row0, int64_t nrows, float keep, const uint8_t* mask,
                      uint64_t seed, uint64_t stream_id, float* gX, int64_t ldgx, float* gHb, int64_t ldgh, int accumulate, void* stream);
size_t idg_hyper_close_workspace_bytes(int64_t d, int64_t h);
int idg_hyper_close_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* gHb, int64_t ldgh, int64_t row0,
                        int64_t nrows, float* gE0, int64_t ldge, float* gW, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: in-batch InfoNCE between two views, forward + backward
 * (utility/utility_function/losses.py:24-35 get_InfoNCE_loss; call sites models/SimGCL.py:79-84,
 *  XSimGCL.py:80-86, SGL.py:96-101: once over unique(batch users), once over unique(batch positive
 *  items), rows gathered from the two [n, d] view panels, users first):
 *     a = normalize(view1[idx]), b = normalize(view2[idx])      (x / max(||x||, 1e-12))
 *     loss = mean_i -log( exp(<a_i,b_i>/t) / sum_k exp(<a_i,b_k>/t) + 1e-5 )
 * loss[0] = the user-set loss, loss[1] = the item-set loss (rows num_users + item id).
 * g1 / g2 (nullable): d(loss[0] + loss[1]) / d view1 / d view2 — the rows of the two sets are
 * STORED, every other row is left untouched (zero-fill the panels first if you need dense
 * gradients), multiplied by grad_scale; with accumulate != 0 they are ADDED to what the rows hold.
 * g1 == g2 is allowed (both views' gradients meet in one panel — a fused training step sums them
 * with the BPR gradient before ONE backward propagation).  The unique id lists never visit the
 * host: launches are shaped by B.
 * dedup = 0 keeps the id lists as they are, duplicates included (models/SGL.py:85-86 indexes its views with
 * the raw batch ids): every occurrence is a row of the in-batch matrix and the gradients of the occurrences
 * of one id are added, in list order, into its panel row.
 * ---------------------------------------------------------------------------------- */
size_t idg_infonce_workspace_bytes(int64_t n, int64_t B, int64_t d);
/* The CROSS form (models/EGCF.py:103: get_InfoNCE_loss(user_embedding, pos_embedding, t) on the RAW batch rows):
 * a_i = normalize(view[users[i]]), b_i = normalize(view[num_users + items[i]]), i < B in batch order, same loss as above
 * in loss[0]; g (nullable): d loss / d view, ADDED (times grad_scale) into the rows of the batch's users and items —
 * the occurrences of one id added in list order.  Same workspace. */
int idg_infonce_cross_f32(const float* view, int64_t n, int64_t d, const int64_t* users, const int64_t* items,
                          int64_t B, int64_t num_users, float temperature, float* loss, float* g, float grad_scale,
                          void* ws, void* stream);
int idg_infonce_pair_f32(const float* view1, const float* view2, int64_t n, int64_t d,
                         const int64_t* users, const int64_t* items, int64_t B, int64_t num_users,
                         int dedup, float temperature, float* loss, float* g1, float* g2,
                         float grad_scale, int accumulate, void* ws, void* stream);
/* The id-list stage of a call on its own — index-only work (unique / raw / cross lists of the batch, the repeat flags and
 * positions of raw lists) that a training loop runs on a side stream one batch ahead, as idg_bpr_plan_f32 does for the
 * scatter plan: idg_infonce_plan(..., mode, ws, stream) with mode 0 = unique ids (dedup = 1), 1 = raw lists (dedup = 0),
 * 2 = the cross form; then the matching call on the SAME workspace with IDG_SSL_PLANNED OR-ed into `dedup`
 * (idg_infonce_pair_f32) or planned != 0 (idg_infonce_cross_ex_f32) skips the stage.  The caller orders the two streams
 * and keeps one workspace per batch in flight. */
#define IDG_SSL_PLANNED 2
int idg_infonce_plan(const int64_t* users, const int64_t* items, int64_t B, int64_t num_users, int64_t n, int64_t d,
                     int mode, void* ws, void* stream);
int idg_infonce_cross_ex_f32(const float* view, int64_t n, int64_t d, const int64_t* users, const int64_t* items,
                             int64_t B, int64_t num_users, float temperature, float* loss, float* g, float grad_scale,
                             int planned, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: alignment + uniformity loss (DirectAU, Wang et al. KDD'22; models/DirectAU.py:59-79 of the reference) and
 * its gradients in one call.  a_i = normalize(final[users[i]]), b_i = normalize(final[num_users + pos[i]]) with
 * normalize(x) = x / max(||x||, 1e-12):
 *   loss[0] = mean_i ||a_i - b_i||^2
 *   loss[1] = gamma (unif(a) + unif(b)) / 2,  unif(x) = log(sum_{i<j} exp(-2 ||x_i - x_j||^2) / (B (B - 1) / 2))
 *             (NaN for B = 1, as torch.pdist's empty mean; the term then contributes no gradient)
 *   loss[2] = reg_lambda (||ego[users]||^2 / 2B + ||ego[num_users + pos]||^2 / 2B)
 * g_final (nullable): d (up[0] loss[0] + up[1] loss[1]) / d final; g_ego (nullable): d (up[2] loss[2]) / d ego, where
 * upstream is a DEVICE pointer to the three incoming gradient scalars up[0..2] or NULL for ones; both the same buffer when
 * final == ego (the MF encoder).  Occurrences of one row are added in batch order (run-to-run reproducible).  Rows the
 * batch touches are ADDED into (accumulate != 0) or STORED (accumulate = 0: the rows of idg_bpr_touch_rows(users, pos,
 * pos), nothing else written).  The B x B pair matrix is never stored: ws is O(B d)
 * (idg_align_uniform_workspace_bytes).  plan_ws: NULL, or a BPR workspace (idg_bpr_workspace_bytes(B, d)) holding
 * idg_bpr_plan_f32(users, pos, pos, ...) of THIS batch — the index-only stage done ahead on another stream.
 * ---------------------------------------------------------------------------------- */
size_t idg_align_uniform_workspace_bytes(int64_t B, int64_t d);
int idg_align_uniform_f32(const float* final_panel, const float* ego_panel, int64_t n, int64_t d,
                          const int64_t* users, const int64_t* pos, int64_t B, int64_t num_users,
                          float gamma, float reg_lambda, float* loss, const float* upstream, float* g_final, float* g_ego,
                          int accumulate, const void* plan_ws, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: SCCF's in-batch second-order contrastive loss (Wu et al. KDD'24; models/SCCF.py:54-81 of the reference) and its
 * gradient in one call.  a_i = normalize(final[users[i]]), b_i = normalize(final[num_users + pos[i]]) with
 * normalize(x) = x / max(||x||, 1e-12), f(s) = exp(s / T) + exp(s^2 / T)  (models/SCCF.py:66-68, 76):
 *   loss[0] = -(1 / B) sum_i log f(a_i.b_i)                                                   (:70, the list's "-up")
 *   loss[1] = log(mean over [Nu, Ni] of f(ah_k.bh_l) cu_k ci_l)                               (:72-78, "down")
 * where ah, bh are the rows of the DISTINCT users and positives of the batch (torch.unique, :60-61) and cu, ci their
 * multiplicities.  cu_k ci_l counts the occurrences of the pair in B x B, so
 *   loss[1] = log(sum_{i<B} sum_{j<B} f(a_i.b_j) / (Nu Ni)):
 * one rectangular Gram problem over the batch rows as they come, and two counts — the run heads of the sorted (row, slot)
 * plan of idg_bpr_plan_f32(users, pos, pos), user rows < num_users <= item rows.  No unique, no host read-back.  The
 * reference's list has no regulariser (reg_lambda is read and never used) and ignores the sampled negatives.
 * With Z = sum sum f every pair's gradient weight is f'(s_ij) / Z, f'(s) = (exp(s / T) + 2 s exp(s^2 / T)) / T: the 128 x 128
 * score tiles (fp32 matrix cores, operands zero-padded to 32 columns, rows and columns >= B masked) are formed ONCE; the pass
 * that sums f also forms tile . b-rows and tile^T . a-rows from f', and 1 / Z is applied per slot afterwards.
 * exp((s - 1) / T) and exp((s^2 - 1) / T) stand for the two exponentials (cosines; 1 / T goes back into the logs).
 * g_final [n, d], nullable (NULL: the losses only, the same bits as with gradients): d (up[0] loss[0] + up[1] loss[1]) /
 * d final (upstream: DEVICE [2], NULL = ones), normalize() differentiated through ((g - <g, h> h) / ||x||, the dot product
 * in double; a row below the floor: g / 1e-12), into the batch's user and positive rows, the occurrences of one row added in
 * batch order by one wave (in double, rounded once: the slots of a repeated id may nearly cancel).  accumulate != 0: ADDED into those rows; accumulate = 0: the rows of idg_bpr_touch_rows(users,
 * pos, pos) are STORED, nothing else written.  g_ego [n, d], nullable, distinct from g_final and given only with it: SCCF
 * has no term on the ego rows — with accumulate = 0 the batch's rows of g_ego are stored as zeros (the engine's "the
 * bitmap's rows of both panels are stored, neither panel is ever filled" without a memset); otherwise untouched.
 * plan_ws: NULL, or a BPR workspace (idg_bpr_workspace_bytes(B, d)) holding idg_bpr_plan_f32(users, pos, pos, ...) of THIS
 * batch; NULL builds the plan in-call, also for the losses alone (the counts come from it).
 * No float atomics, fixed summation orders: the same bits every run.  1 <= d <= 256, 1 <= B < 2^22, T > 0.
 * ws: idg_sccf_workspace_bytes, 256-byte aligned: O(B d) plus the per-tile partial gradient rows, ceil(B / 128) slices of
 * [2, B, d] (16 MiB at B = 2048, d = 64); 0 is returned for sizes not built.
 * ---------------------------------------------------------------------------------- */
size_t idg_sccf_workspace_bytes(int64_t B, int64_t d);
int idg_sccf_loss_f32(const float* final_panel, int64_t n, int64_t d, const int64_t* users, const int64_t* pos, int64_t B,
                      int64_t num_users, float temperature, float* loss /*[2]*/, const float* upstream /*DEVICE [2], NULL = ones*/,
                      float* g_final, float* g_ego, int accumulate, const void* plan_ws, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: the neighbour-aggregation loss of LightCCF (Zhang et al. SIGIR'25; models/LightCCF.py:81-94 of the reference) and
 * LightCSCF (models/LightCSCF.py:93-104) and its gradient in one call.  a_i = normalize(final[users[i]]),
 * b_i = normalize(final[num_users + pos[i]]) with normalize(x) = x / max(||x||, 1e-12), p_i = a_i.b_i:
 *   total_score[i, j] = a_i.b_j + a_i.a_j = a_i.c_j,  c_j = a_j + b_j        (the SUM of the two matrices is inside exp)
 *   T_i = sum_j f(a_i.c_j)  (every j, the diagonal included),   r_i = f(p_i) / T_i
 *   loss[0] = grad_scale (1 / B) sum_i -log(r_i + 1e-5)                                      (the reference's `10e-6`)
 *   margin < 0 (LightCCF):  f(s) = exp(s / T);   0 <= margin <= 2 (LightCSCF):  f(s) = exp(s / T) + exp(relu(s - margin) / T)
 * grad_scale carries ssl_lambda / lambda_gamma.  One rectangular Gram problem A C^T over the batch rows as they come, on
 * 64 x 64 score tiles (operands zero-padded to 32 columns, rows and columns >= B masked), never stored as a [B, B] matrix.
 * The diagonal makes r_i <= exp(-1 / T), the order of the 1e-5 at small T, so row i's gradient carries
 * w_i = r_i / (r_i + 1e-5) and needs T_i complete: the tiles are formed again after a row-sum pass (each partial written by
 * one workgroup, combined in a fixed order), with P_ij = w_i f'(s_ij) / (T_i B), for P . C and for P^T . A.
 * G_c[j] = sum_i P_ij a_i reaches both a_j and b_j; a_i also takes sum_j P_ij c_j and, with b_i, the positive term.  Every
 * exponential carries the fixed shift -2 / T (scores <= 2), which cancels in r_i and in every gradient weight; T >= 0.01.
 * The whole term runs in DOUBLE — normalised rows, scores and both products on v_mfma_f64_16x16x4_f64, exponentials, sums:
 * at a low temperature the diagonal and the columns repeating a row's user hold nearly all of T_i, and the gradient is the rest
 * of parts that cancel, 1e2 ... 1e5 times smaller than they are; float32 operands or tiles leave it wrong by up to percents
 * (csrc/idg_nance.hip).  The inputs and the gradient panel stay float32.
 * g_final [n, d], nullable (NULL: the loss only, the same bits as with gradients): upstream * d loss[0] / d final (upstream:
 * DEVICE [1], NULL = 1), normalize() differentiated through ((g - <g, h> h) / ||x||, in double; a row below the floor:
 * g / 1e-12), into the batch's user and positive rows, the occurrences of one row added in batch order by one wave (in
 * double, rounded once).  accumulate != 0: ADDED into those rows; accumulate = 0: every row of the plan is STORED (a row
 * that only third slots of the plan name: zeros), nothing else written.
 * plan_ws: NULL, or a BPR workspace (idg_bpr_workspace_bytes(B, d)) holding idg_bpr_plan_f32(users, pos, x, ...) of THIS batch
 * (x = the negatives or the positives: third slots carry no term); NULL builds the plan of (users, pos, pos) in-call when a
 * gradient is asked for.  No float atomics, fixed summation orders: the same bits every run.  1 <= d <= 256, 1 <= B < 2^22.
 * ws: idg_na_nce_workspace_bytes, 256-byte aligned: O(B d) doubles, the partial products of at most 8 splits of the tile walk
 * included (43 MiB at B = 4096, d = 64); 0 is returned for sizes not built.
 *
 * idg_reg_rows_f32: the regulariser alone, for a step without a BPR call to carry it (LightCSCF on LightGCN,
 * models/LightCSCF.py:82-89): loss[0] = reg_lambda (1/2) (sum ||e_u||^2 + sum ||e_p||^2 + sum ||e_n||^2) / B over the ego rows
 * of users, positives AND negatives, duplicates counted.  Over the sorted plan of idg_bpr_plan_f32(users, pos, neg, ...)
 * (plan_ws; NULL builds it in-call from the three lists): g_ego (nullable) has the gradient rows STORED (occurrences added
 * in batch order in double, rounded once), g_final (nullable, distinct from g_ego) has zeros STORED to the same rows, so every
 * row of the batch's bitmap is defined before idg_na_nce_f32 ADDS the users' and positives' rows.  ws: a buffer of
 * idg_na_nce_workspace_bytes bytes for this B and d (it may be the one the idg_na_nce_f32 call that follows uses).
 * ---------------------------------------------------------------------------------- */
size_t idg_na_nce_workspace_bytes(int64_t B, int64_t d);
int idg_na_nce_f32(const float* final_panel, int64_t n, int64_t d, const int64_t* users, const int64_t* pos, int64_t B,
                   int64_t num_users, float temperature, float margin /* < 0: none */, float grad_scale, float* loss /*[1]*/,
                   const float* upstream /*DEVICE [1], NULL = 1*/, float* g_final, int accumulate, const void* plan_ws, void* ws,
                   void* stream);
int idg_reg_rows_f32(const float* ego_panel, int64_t n, int64_t d, const int64_t* users, const int64_t* pos, const int64_t* neg,
                     int64_t B, int64_t num_users, float reg_lambda, float* loss /*[1]*/, float* g_ego, float* g_final,
                     const void* plan_ws, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: CVGA's decoder loss and VAE head (Zhang et al. TOIS'23; models/CVGA.py:40-85 and
 * utility/utility_function/losses.py:53-56 of the reference), forward and backward.
 *
 * idg_multinomial_nll_f32: Z [B, d], W [I, d], c [I]; l_bi = <Z[b], W[i]> + c[i]; x_b = row users[b] of the train CSR
 * (indptr int64 [U + 1], items int32 ascending per row, values fp32 — duplicate edges summed; DEVICE pointers, indexed by
 * user id), n_b = sum_i x_bi:
 *   loss[0] = (1 / B) sum_b (n_b log sum_i exp l_bi - sum_i x_bi l_bi)        (-mean(sum(log_softmax(l) * x, -1)))
 * loss nullable.  gZ / gW / gc (all or none): d (up loss) / d Z, W, c with up = *upstream (DEVICE scalar; NULL = 1);
 * gW and gc are WRITTEN for all I rows.  A user with an empty train row contributes 0 to both.  The [B, I] matrix is never
 * stored: a statistics pass (row max and sum-exp over 64-item tiles in up to 256 chunks), then a gradient pass that
 * recomputes each logit tile and forms both products and the column sums from it.  Logit tiles and products on the fp32
 * matrix cores for d % 32 == 0, d <= 256, a SIMT form otherwise.  No float atomics, fixed summation orders: the same bits
 * every run.  ws: idg_multinomial_nll_workspace_bytes (O(chunks B d + B)), 256-byte aligned; it also holds the row
 * statistics: flags IDG_NLL_STATS_READY skips the statistics pass and reuses those of the last call on this ws with the
 * same inputs (the backward of an autograd operator whose forward made them).
 * ---------------------------------------------------------------------------------- */
#define IDG_NLL_STATS_READY 1
size_t idg_multinomial_nll_workspace_bytes(int64_t B, int64_t I, int64_t d);
int idg_multinomial_nll_f32(const float* Z, const float* W, const float* c, int64_t B, int64_t I, int64_t d,
                            const int64_t* users, const int64_t* indptr, const int32_t* items, const float* values,
                            float* loss, const float* upstream, float* gZ, float* gW, float* gc, int flags, void* ws,
                            void* stream);
/* idg_vae_head_fwd_f32: row b of the encoder product is pre[(pre_rows ? pre_rows[b] : b) * ld_pre + 0 .. 2d):
 *   h = keep * (pre_row + bias), mu = h[:d], logvar = h[d:], z[b] = eps * exp(logvar / 2) + mu                [B, d]
 *   *kl = -0.5 / B^2 sum_b sum_j (1 + logvar - mu^2 - exp(logvar))                  (nullable; needs ws then)
 * keep = 1 / (1 - p) or 0 (dropout p, NGCF's counter-based mask of idg_dropout.h over the 2d features of user users[b]);
 * eps = eps_in[b, :] when given, else a standard normal from (seed, stream_id, users[b], feature).  eps_out [B, d] and
 * keep_out [B, 2d] (nullable) receive what was used.  ws: idg_vae_head_workspace_bytes(B).
 * idg_vae_head_bwd_f32: with the same (pre, users, bias, p, seed, stream_id, eps_in) — keep and eps are regenerated —
 * gz = d L / d z (nullable: 0) and up = *upstream_kl (DEVICE scalar d L / d kl, NULL = 1):
 *   gpre row (gpre_rows ? gpre_rows[b] : b) <- keep * (gz + up mu / B^2 | gz eps exp(logvar / 2) / 2 + up (exp(logvar) - 1) / 2B^2)
 *   gbias (nullable) <- the column sums of those rows, in batch order.  With gpre_rows the rows must be distinct. */
size_t idg_vae_head_workspace_bytes(int64_t B);
int idg_vae_head_fwd_f32(const float* pre, int64_t ld_pre, const int64_t* pre_rows, const int64_t* users, int64_t B, int64_t d,
                         const float* bias, float p, uint64_t seed, uint64_t stream_id, const float* eps_in, float* z,
                         float* kl, float* eps_out, float* keep_out, void* ws, void* stream);
int idg_vae_head_bwd_f32(const float* pre, int64_t ld_pre, const int64_t* pre_rows, const int64_t* users, int64_t B, int64_t d,
                         const float* bias, float p, uint64_t seed, uint64_t stream_id, const float* eps_in, const float* gz,
                         const float* upstream_kl, float* gpre, int64_t ld_gpre, const int64_t* gpre_rows, float* gbias,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: full-table contrastive loss (CGCL, He et al. SIGIR'23; models/CGCL.py:95-215 of the reference, the expression of
 * utility/utility_function/losses.py:38-50), forward and backward.
 *
 * Table: rows [row0, row0 + N) of table_panel [*, d], each divided by max(||x||, 1e-12) (F.normalize) -> Th.  nq query
 * blocks (1 .. IDG_TNCE_MAX_QUERY_BLOCKS) share it: block k is the B rows query_panels[k][query_ids[k][b]] (row stride d;
 * any panel, ids may repeat), normalised the same way -> Qh_k.  The positive of query b is table row pos_ids[b] in [0, N)
 * (one list for the call; the caller's contract, as the query ids are).  query_panels / query_ids / g_query_panels / weights
 * are HOST arrays of nq entries; the id lists and panels they name are DEVICE memory.  With s_bj = <Qh_b, Th_j>:
 *   loss[k] = -weights[k] sum_b log( exp(s_b,pos(b) / tau) / sum_{j < N} exp(s_bj / tau) + 1e-7 )
 * loss [nq] nullable.  g_table_panel and g_query_panels (all or none): the gradients of sum_k up[k] loss[k] (upstream: DEVICE
 * [nq], NULL = ones) are ADDED into rows [row0, row0 + N) of g_table_panel (all N rows: the term is dense) and into rows
 * query_ids[k][b] of g_query_panels[k] (repeated ids summed in batch order), both back through the normalisation.  Buffers
 * may coincide (one panel as table and as query panel, one gradient panel for several roles): the additions are made one
 * launch after the other.
 * Scores are cosines, so exp((s - 1) / tau) is used in place of exp(s / tau): the common factor cancels in the ratio, no
 * running maximum is needed and the sums stay finite for any tau > 0, where the reference's exp(1 / tau) overflows fp32
 * for tau below about 0.0113.  The [B, N] matrix is never stored: 128 x 128 score tiles are formed twice (a batch-major pass
 * for the row sums and d Qh, a table-major pass for d Th) on the fp32 matrix cores (v_mfma_f32_32x32x2_f32; the operands are
 * zero-padded to a multiple of 32 columns, so every d <= 256 takes that path).  No float atomics, fixed summation orders:
 * the same bits every run.  ws: idg_table_nce_workspace_bytes (the normalised copies, per-row statistics, and ordered
 * partial sums: O((N + chunks nq B) d), chunks <= 64), 256-byte aligned; 0 is returned for sizes that are not built.
 * ---------------------------------------------------------------------------------- */
#define IDG_TNCE_MAX_QUERY_BLOCKS 4
size_t idg_table_nce_workspace_bytes(int64_t B, int64_t N, int64_t d, int nq);
int idg_table_nce_f32(const float* table_panel, int64_t row0, int64_t N, int64_t d, int nq,
                      const float* const* query_panels, const int64_t* const* query_ids, int64_t B,
                      const int64_t* pos_ids, const float* weights, float temperature, float* loss,
                      const float* upstream, float* g_table_panel, float* const* g_query_panels, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: MixRec's in-batch mixing contrastive terms (Zhang et al. WWW'25; models/MixRec.py:94-154 of the reference: every
 * term is losses.get_InfoNCE_loss_all(e1, e2, e2_all, T) whose positive e2 is NOT a row of its negative set e2_all, and
 * whose operands exist only inside the batch), forward and backward in one call.
 *
 * panel [n, d], users first.  The batch's rows: u_i = panel[users[i]], p_i = panel[num_users + pos[i]],
 * n_i = panel[num_users + neg[i]], i < B (ids may repeat).  user_perm / item_perm: DEVICE int64 [B], permutations of
 * 0 .. B-1 (the caller's contract; an entry outside the batch reads as its own position).  nu: DEVICE float [B].
 * hat(x) = x / max(||x||, 1e-12) (F.normalize: a zero row stays zero).
 *
 * A side with rows x, permutation pi and weight beta — (u, user_perm, user_beta) and (p, item_perm, item_beta):
 *   h = hat(x),   c_i = beta x_i + (1 - beta) x_pi(i),  ch = hat(c),   m = sum_j nu_j x_j,  mh = hat(m)
 *   D_i  = sum_j exp(h_i.h_j / T) + exp(h_i.mh / T)
 *   side = (1/B) sum_i [ -beta log(exp(ch_i.h_i / T) / D_i + 1e-7) - (1 - beta) log(exp(ch_i.h_pi(i) / T) / D_pi(i) + 1e-7) ]
 * which is beta InfoNCE_all(x, c, [x[pi]; m], T) + (1 - beta) InfoNCE_all(x[pi], c, [x; m], T): the first term's
 * denominator sums over a permutation of the rows and the second term's anchors are the permuted rows, so both read one
 * vector of row sums of one symmetric Gram matrix.
 * The rectangular term, T = 1, with Mn_j = item_beta n_j + (1 - item_beta) n_item_perm(j):
 *   rect = (1/B) sum_i -log( exp(hat(u)_i.hat(p)_i) / sum_j exp(hat(u)_i.hat(Mn)_j) + 1e-7 )
 *   loss[0] = (1 - item_beta) rect                         (the reference's second list entry)
 *   loss[1] = ssl_weight (side_users + side_items)         (its fourth)
 * loss [2] nullable.  g_panel [n, d], nullable (NULL: losses only, the same bits as with gradients): the gradient of
 * up[0] loss[0] + up[1] loss[1] (upstream: DEVICE [2], NULL = ones) w.r.t. the panel is ADDED into the batch's rows,
 * repeated ids summed in batch order (users, then positives, then negatives, one launch after the other).  With
 * kappa_k = d side / d D_k the Gram part of d side / d h_k is (1/T)[kappa_k sum_j e_kj h_j + sum_j e_kj kappa_j h_j] +
 * (1/T) kappa_k e_km mh: two passes E.Y over the same symmetric E (Y = H, which also yields the row sums, then
 * Y = kappa o H), no transposed pass; the rectangular term adds one transposed pass for Mn.  The mix row is one dot product
 * per row.  Every normalisation, c, Mn and m are differentiated through (projections with double dot products).
 * exp((s - 1) / T) stands for exp(s / T) (cosines: no running maximum).  The [B, B] matrices are never stored: 128 x 128
 * tiles on the fp32 matrix cores (v_mfma_f32_32x32x2_f32; operands zero-padded to 32 columns: every d <= 256 one path).
 * No float atomics, fixed summation orders: the same bits every run.  1 <= d <= 256, 1 <= B < 2^22, both betas in [0, 1].
 * ws: idg_mix_nce_workspace_bytes, 256-byte aligned (O(chunks B d), chunks <= 64); 0 is returned for sizes not built.
 * ---------------------------------------------------------------------------------- */
size_t idg_mix_nce_workspace_bytes(int64_t B, int64_t d);
int idg_mix_nce_f32(const float* panel, int64_t n, int64_t d, int64_t num_users, const int64_t* users, const int64_t* pos,
                    const int64_t* neg, int64_t B, const int64_t* user_perm, const int64_t* item_perm, const float* nu,
                    float user_beta, float item_beta, float temperature, float ssl_weight, float* loss, const float* upstream,
                    float* g_panel, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: LightGCL's SVD-view contrastive terms (Cai et al. ICLR'23; models/LightGCL.py:58-120 of the reference) and the two
 * rank-q products around them.
 *
 * The reference forms, per layer l, the view g^l = (A S)(A'^T E'^(l-1)) over ALL rows (A, A' [*, q] the two factor panels
 * of one truncated SVD, S its singular values) and sums the layers.  By linearity
 *   G = E^0 + (A S) P,   P = A'^T T',   T = sum_{l < K} E^l = F - E^K     (F the layer sum 0 .. K)
 * so a step needs two projections to [q, d], and only the batch's rows of G are ever read.
 *
 * idg_lowrank_project_f32:  out [q, d] (+)= sum_{r < n} A[a_rows ? a_rows[r] : r, 0:q]^T X[r, 0:d]   (row strides lda, ldx;
 *   a_rows: DEVICE int64 [n], nullable, rows of A, may repeat: the backward's sum over a batch).  A tall reduction: every
 *   workgroup owns a fixed run of at least 64 rows (n / 1024 when that is more), each of its row lanes adds its rows
 *   ascending, the lanes are added in order, and the per-workgroup [q, d] partials meet in the library's one slice reduction.
 *   n >= 1 (tens of millions: 64-bit row arithmetic), 1 <= q <= 16, 1 <= d <= 256.  ws: idg_lowrank_project_workspace_bytes,
 *   256-byte aligned (at most 1024 q d floats).
 * idg_lowrank_expand_f32:   Y[r, 0:d] (+)= scale A[a_rows ? a_rows[r] : r, 0:q] P, r < n, P [q, d] contiguous, k ascending
 *   (row strides lda, ldy; accumulate != 0 adds into Y).  The backward's dense rank-q update gT += A' dP, and the view rows
 *   of the differentiable operator.
 *
 * idg_svd_nce_f32, one side per call (users: row0 = 0, N = num_users; items: row0 = num_users, N = num_items):
 *   F_j = final_panel[row0 + j], j < N (row stride d);  ids: DEVICE int64 [B] in [0, N), may repeat (an id outside reads as
 *   the nearest row of the side);  AS [N, q] contiguous: the side's factor rows times S;  P [q, d] contiguous.
 *   g_b  = ego_panel[row0 + ids[b]] + AS[ids[b]] P
 *   s_bj = <g_b, F_j> / tau                                   RAW dot products: nothing is normalised
 *   loss[0] = (1/B) sum_b log(sum_{j < N} exp(s_bj) + 1e-8)
 *   loss[1] = (1/B) sum_b clamp(<F_ids[b], g_b> / tau, -5, 5)
 * loss [2] nullable.  The log-sum-exp carries a true per-row running maximum, online across the table tiles:
 *   m_b = max_j s_bj,  L_b = m_b + log(sum_j exp(s_bj - m_b) + 1e-8 exp(-m_b))
 * finite and exact where exp(s) overflows fp32 (s > 88), and still log(1e-8 + ..) where every score is far below zero (a
 * norm bound in place of the maximum would lose the sum there).
 * g_final_panel, g_ego_panel [*, d] and dP [q, d] (all or none): with up = upstream (DEVICE [2], NULL = ones) the gradient of
 * up[0] loss[0] + up[1] loss[1] is ADDED
 *   into rows [row0, row0 + N) of g_final_panel: sum_b w_bj g_b, w_bj = up[0] / (B tau) softmax-with-guard weight (all N
 *     rows: the term is dense), and c_b g_b into row row0 + ids[b], c_b = up[1] / (B tau) where -5 <= pos_b <= 5 and
 *     EXACTLY 0 outside (autograd's clamp); occurrences of one id in batch order;
 *   into rows row0 + ids[b] of g_ego_panel: gQ_b = sum_j w_bj F_j + c_b F_ids[b], repeated ids summed in batch order;
 * and dP = sum_b AS[ids[b]]^T gQ_b is STORED (the projection above with the id list).  The panels may coincide: the
 * additions are made one launch after the other.
 * The [B, N] matrix is never stored: 128 x 128 score tiles are formed twice (a batch-major pass for the row statistics and
 * gQ, whose [128, d] accumulator is rescaled in registers when the running maximum moves; a table-major pass for the table
 * gradient from the stored m_b) on the fp32 matrix cores (v_mfma_f32_32x32x2_f32; operands zero-padded to a multiple of 32
 * columns: every d <= 256 one path).  A batch below one tile, B <= 127, takes a direct form instead of the two tile passes: its
 * scores [B, N], row statistics and weights in double (kept in the workspace, 8 B N bytes), one rounding per output — with few
 * rows nothing averages the fp32 rounding of the scores, which 1 / tau multiplies.  No float atomics, fixed summation orders:
 * the same bits every run.
 * Any B >= 1, N >= 1, 1 <= q <= 16.  ws: idg_svd_nce_workspace_bytes, 256-byte aligned (the padded copies, per-chunk
 * statistics and ordered partial sums: O((N + chunks B) d), chunks <= 64); 0 is returned for sizes that are not built.
 * ---------------------------------------------------------------------------------- */
size_t idg_lowrank_project_workspace_bytes(int64_t n, int64_t q, int64_t d);
int idg_lowrank_project_f32(const float* A, int64_t lda, const int64_t* a_rows, const float* X, int64_t ldx, int64_t n,
                            int64_t q, int64_t d, float* out, int accumulate, void* ws, void* stream);
int idg_lowrank_expand_f32(const float* A, int64_t lda, const int64_t* a_rows, const float* P, int64_t n, int64_t q, int64_t d,
                           float scale, int accumulate, float* Y, int64_t ldy, void* stream);
size_t idg_svd_nce_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t q);
int idg_svd_nce_f32(const float* final_panel, const float* ego_panel, int64_t row0, int64_t N, int64_t d, const float* AS,
                    int64_t q, const float* P, const int64_t* ids, int64_t B, float temperature, float* loss,
                    const float* upstream, float* g_final_panel, float* g_ego_panel, float* dP, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: Lloyd's k-means, the E-step of NCL (Lin et al. WWW'22; models/NCL.py:66-81 of the reference: faiss.Kmeans on a
 * host copy of each embedding table, then index.search(x, 1) for the final assignment).
 *
 * X: N rows of d floats, row stride ldx >= d (a panel may be wider than the rows used).  C: [K, d], contiguous.
 * idg_kmeans_assign_f32: assign[i] = argmin_j ||x_i - c_j||^2, evaluated as ||c_j||^2 - 2 <x_i, c_j>, ties to the lowest j;
 *   dist2 (nullable [N]): max(0, ||x_i||^2 + that minimum).  The products run on the fp32 matrix cores
 *   (v_mfma_f32_32x32x2_f32; the operands are zero-padded to a multiple of 32 columns, so every d <= 256 takes one path) in
 *   128 x 128 tiles; the running (min, arg-min) pair stays in registers across the centroid tiles and the [N, K] matrix is
 *   never stored.  With few row tiles K is split over workgroups and the partial minima are combined in chunk order.
 * idg_kmeans_update_f32: C[j] <- the mean of the rows with assign[i] = j, the rows added in ascending row order (brought
 *   together by a stable counting sort of the row ids; integer atomics in its histogram only); counts (nullable [K]): the
 *   rows per cluster.  A cluster without rows keeps the centroid it had, bit for bit (faiss splits its largest cluster
 *   instead: DESIGN.md).  An index outside [0, K) is ignored.
 * idg_kmeans_f32: niter x (assign, update) from the centroids in C, then one more assign against the final centroids;
 *   inertia (nullable [niter + 1]): the sum of dist2 of every assign, the last entry the final one.  Launches on one stream,
 *   no host read-back.
 * No float atomics, fixed summation orders: the same bits every run.  ws: idg_kmeans_workspace_bytes (the padded copies,
 * per-chunk minima and the sorted row ids: O((N + K) d + chunks N), chunks <= 64), 256-byte aligned; 0 is returned for sizes
 * that are not built (d > 256, N or K outside int32).
 * ---------------------------------------------------------------------------------- */
size_t idg_kmeans_workspace_bytes(int64_t N, int64_t K, int64_t d);
int idg_kmeans_assign_f32(const float* X, int64_t ldx, int64_t N, int64_t d, const float* C, int64_t K, int32_t* assign,
                          float* dist2, void* ws, void* stream);
int idg_kmeans_update_f32(const float* X, int64_t ldx, int64_t N, int64_t d, const int32_t* assign, int64_t K, float* C,
                          int32_t* counts, void* ws, void* stream);
int idg_kmeans_f32(const float* X, int64_t ldx, int64_t N, int64_t d, int64_t K, int niter, float* C, int32_t* assign,
                   float* inertia, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: row normalisation of a panel and its backward, the per-layer step of LightGCN++ (Lee et al. RecSys'24;
 * models/LightGCN_pp.py:82-84 of the reference: x / (torch.norm(x, dim=1) + 1e-12)[:, None]).
 *
 * Panels are contiguous fp32 [n, d], 16-byte aligned, 1 <= d <= 512, n < 2^31; norms is [n]; eps > 0.
 * idg_rows_normalize_f32: norms[r] = ||X[r]||_2, Y[r] = X[r] / (norms[r] + eps).  A zero row gives norms[r] = 0 and Y[r] = 0
 *   exactly.
 * idg_rows_normalize_bwd_f32: out[r] = a G[r] + add2[r] + J_r(T[r]); G and add2 may each be NULL (a is then not read).  J is
 *   the backward of the row's normalisation, from the Y and norms the forward call saved: with n = norms[r], e = eps,
 *   y = Y[r]:  J(t) = (t - y <y, t> (n + e) / n) / (n + e) for n > 0, and J(t) = t / e for n == 0 (torch's norm has gradient 0
 *   at the origin; exact: the saved y is 0 there).
 * One row is held by one group of 4 .. 64 lanes in registers between a shuffle reduction and the store (float4 accesses where
 * d % 4 == 0, a scalar path for every other width): every input panel is read once, every output written once; no LDS, no
 * atomics, the same bits every run.
 * Aliasing.  Forward: Y may be X (in place); any other overlap of Y with X, and any overlap of norms with X or Y, is
 * refused.  Backward: out may be T, G or add2 (the same pointer); any other overlap of out with one of them, and any
 * overlap of out with Y or norms, is refused.  The inputs may alias one another freely.
 * Arguments are checked on the host before any device work (IDG_E_INVALID, idg_last_error).
 * ---------------------------------------------------------------------------------- */
int idg_rows_normalize_f32(const float* X, int64_t n, int64_t d, float eps, float* Y, float* norms, void* stream);
int idg_rows_normalize_bwd_f32(const float* T, const float* Y, const float* norms, float eps, const float* G, float a,
                               const float* add2, float* out, int64_t n, int64_t d, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: dense Adam step  (torch.optim.Adam defaults, utility/utility_train/trainer.py:11,56:
 * betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad).  step is 1-based.  The
 * hyper-parameters are doubles because torch forms lr/(1-beta1^t) and sqrt(1-beta2^t) in
 * double on the host before the fp32 kernels see them.
 * ---------------------------------------------------------------------------------- */
int idg_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                      int64_t count, double lr, double beta1, double beta2, double eps,
                      int64_t step, void* stream);

/* out = a*x + b*y over `count` floats (y may be NULL: out = a*x; out may alias x or y).
 * Glue for the sharded path: adding an all-reduced layer into the running sum, the final
 * 1/(K+1) scaling, folding the replicated layer-0 term. */
int idg_lincomb_f32(float* out, const float* x, float a, const float* y, float b, int64_t count,
                    void* stream);

/* Row movers of the user-row-sharded step (no counterpart in the single-device reference): the ranks
 * exchange the batch's user rows through "guest" rows of their panels.
 * idg_rows_gather_f32: dst[t, :] = idx[t] >= 0 ? src[idx[t], :] : 0 for t < count (rows of d floats).
 * idg_rows_chain_add_f32: for every t with idx[t] >= 0, dst[idx[t], :] += src[t, :] + src[next[t], :] + ... following
 * `next` until -1, added in that order by one wave (the caller chains the occurrences of one destination in list
 * order): deterministic, no atomics.  idx / next: int64 device arrays. */
int idg_rows_gather_f32(float* dst, const float* src, const int64_t* idx, int64_t count, int64_t d, void* stream);
int idg_rows_chain_add_f32(float* dst, const float* src, const int64_t* idx, const int64_t* next, int64_t count,
                           int64_t d, void* stream);

/* The same movers in the forms the round-3 step uses (16-byte lanes; d % 4 == 0, panels 16-byte aligned):
 * idg_rows_gather2_f32: idg_rows_gather_f32 for two (dst, src) panel pairs sharing one index list in ONE launch (the
 *   batch users' final and ego rows go to the guest rows together); the second pair may be NULL.
 * idg_rows_scatter_f32: dst[idx[j], :] = src[j, :] (idx distinct, >= 0) — puts an exchanged compact row set back.
 * idg_rows_chain_store2_f32: idg_rows_chain_add_f32 that STORES the chain's sum (dst[idx[t]] = src[t] + src[next[t]] + ...)
 *   for two panel pairs: the destination panels are never zero-filled, their live rows are known by bitmap.
 * idg_rows_layer_mean_f32: out[ids[j], :] = (((a[ids[j]] + b[ids[j]]) + c[ids[j]]) + last[j]) / div with a, b, c nullable
 *   [*, d] panels and `last` a compact [count, d] buffer — LightGCN's layer mean (models/LightGCN.py:47-48, torch.mean of
 *   the stacked layers: left-to-right sum, true division) at the batch's item rows, whose last layer arrives as a
 *   compact exchanged row set.
 * idg_grad_tail_adam_f32: the item-row tail of a sharded step for a block of `rows` rows one rank owns, starting at
 *   global item row row0: s = (include_layer0 && live ? g + t : t) / cnt; s = live ? G + s : s; [G = s if store_grad];
 *   Adam(param, exp_avg, exp_avg_sq; s) — t = the reduced partial sums of the last backward product, g = d loss / d final
 *   and G = the regulariser's gradient, both meaningful only at live rows (bit row0 + r of live_bits; NULL = no live
 *   row).  Pointers address the block's first row.  Same operations in the same order as the last backward epilogue of
 *   the single-device step (autograd of models/LightGCN.py:43-48 + trainer.py:54-56). */
int idg_rows_gather2_f32(float* dst0, const float* src0, float* dst1, const float* src1, const int64_t* idx,
                         int64_t count, int64_t d, void* stream);
int idg_rows_scatter_f32(float* dst, const int64_t* idx, const float* src, int64_t count, int64_t d, void* stream);
int idg_rows_chain_store2_f32(float* dst0, const float* src0, float* dst1, const float* src1, const int64_t* idx,
                              const int64_t* next, int64_t count, int64_t d, void* stream);
int idg_rows_layer_mean_f32(float* out, const int64_t* ids, int64_t count, const float* a, const float* b,
                            const float* c, const float* last, float div, int64_t d, void* stream);
int idg_grad_tail_adam_f32(const float* t, const float* g, float* G, const uint32_t* live_bits, int64_t row0,
                           int64_t rows, int64_t d, int include_layer0, float cnt, int store_grad, float* param,
                           float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                           int64_t step, void* stream);
/* idg_rows_layer_mean_f32 for ANY number of earlier layers (GCN_layer is a free integer: configure/LightGCN.txt:12,
 * models/LightGCN.py:43-48): out[ids[j], :] = ((...(terms[0] + terms[1]) + ...) + terms[n_terms-1])[ids[j]] + last[j]) / div,
 * added left to right as torch.mean(torch.stack(...)) does; terms = HOST array of n_terms <= 15 device panels. */
int idg_rows_layer_mean_n_f32(float* out, const int64_t* ids, int64_t count, const float* const* terms, int n_terms,
                              const float* last, float div, int64_t d, void* stream);
/* ids[0..cap) <- the indices i (ascending) with flags[i] != 0, flags a DEVICE float vector of n entries; slots past the
 * last index repeat it (an empty vector: zeros); *count (device int64, nullable) <- the number of non-zero flags, which
 * may exceed cap (the list then holds the first cap).  Asynchronous, no host read-back: the sharded step agrees on the
 * item rows a batch touches (summed flag vectors) and moves a HOST-bounded number of rows through this
 * list — a repeated row is gathered, reduced and scattered more than once with the same value.
 * ws: idg_flags_compact_workspace_bytes(n). */
size_t idg_flags_compact_workspace_bytes(int64_t n);
int idg_flags_compact_f32(const float* flags, int64_t n, int64_t* ids, int64_t cap, int64_t* count, void* ws, void* stream);

/* The index-only preparation of ONE global batch of the user-row-sharded step as one call (id-grec_amd/sharded/kernels.py
 * HipKernels.prepare did this in twelve: the host cost of a step is its calls).  On `side_stream`, ordered after
 * `main_stream` through ev_fork:  users_bits = bitmap of own_users[0..n_own) (n_local_users bits); items_bits = bitmap
 * of pos[0..B) and neg[0..B) (n_items_padded bits); scatter_bits cleared (n_panel_rows bits: the gradient scatter flags
 * its stored rows there); the live-unit lists of users_bits on user_graph and of each item slice's share of items_bits
 * (bit offset slice_row0[j], a multiple of 32) on slice_graphs[j]; ev_rows recorded; the sorted scatter plan of
 * (guest_ids, pos, neg) over a panel of n_panel_rows rows whose items start at row n_local_users + B_cap
 * (idg_bpr_plan_f32) into plan_ws; ev_plan recorded.  Events are idg_event_create handles (NULL: skipped); unit-list
 * buffers as idg_graph_live_units_bytes(graph, B_cap) / (graph, 2 B_cap) (NULL: no list for that graph). */
typedef struct idg_shard_prep {
  const int64_t* own_users; int64_t n_own;       /* local ids of the owned triples' users */
  const int64_t* pos; const int64_t* neg; const int64_t* guest_ids; int64_t B, B_cap;
  uint32_t* users_bits; int64_t n_local_users;
  uint32_t* items_bits; int64_t n_items_padded;
  uint32_t* scatter_bits; int64_t n_panel_rows;
  const idg_graph* user_graph; void* user_units;
  int n_slices; const idg_graph* const* slice_graphs; const int64_t* slice_row0; void* const* slice_units;
  void* plan_ws;
  void* main_stream; void* side_stream;
  void* ev_fork; void* ev_rows; void* ev_plan;
} idg_shard_prep;
int idg_shard_prepare(const idg_shard_prep* prep);

/* ------------------------------------------------------------------------------------
 * DEVICE: ONE library call per training step
 * (the body of the reference's batch loop, utility/utility_train/trainer.py:42-56 — model(batch) ->
 *  [bpr, reg] (models/LightGCN.py:54-72 / models/MFBPR.py:29-42), backward(), Adam.step() — which this
 *  library's host previously drove as ~8 calls + Python slicing per step: the host was within 10 % of
 *  being the limit of a 0.26 ms step)
 * ---------------------------------------------------------------------------------- */
/* A step plan is built once per model: it names every buffer a step touches (all caller-owned — the library
 * still allocates no device memory) and owns only its events.  idg_step_run_f32 then enqueues, in order:
 *   - on `side_stream`, the index-only preparation of the NEXT batch (row bitmap, live work units, sorted scatter
 *     plan: idg_bpr_touch_rows, idg_graph_live_units, idg_bpr_plan_f32) into one of IDG_STEP_SLOTS slots;
 *   - on `stream`, this batch's step: K forward products with the layer mean at the batch's rows
 *     (idg_propagate_mean_f32 with out_rows), fused BPR + regulariser storing its gradient rows
 *     (idg_bpr_fused_f32, IDG_BPR_PLANNED | IDG_BPR_TOUCHED_PRESET), the backward chain with the Adam update in
 *     its last product's epilogue (idg_propagate_mean_bwd_adam_f32) and the end-of-step event;
 *   graph == NULL (MFBPR: no propagation): fused BPR on the raw tables with stored gradient rows, then
 *     idg_adam_rows_f32 (the dense Adam step reading the gradient at the batch's rows only).
 * Bit-identical to the same chain issued call by call.  IDG_STEP_PACED: the host blocks until the step before the
 * previous one has finished (two steps stay queued), after which a batch prepared a step ahead is complete when its
 * own step is enqueued and the step's stream does not wait for the side stream at all (a barrier packet costs ~4.5 us
 * whether or not its event has fired).
 * ids_token: any value that changes whenever the id arrays' STORAGE changes (a new epoch's triples): the side stream is
 * ordered behind `stream` once per token — the arrays may have been produced there — and 0 means "every call".
 * next_ids_token (idg_step_run_f32): the same for the storage of the NEXT batch's arrays, which need not be this
 * batch's (the first batch of a new epoch, a clone, a gather result). */
#define IDG_STEP_SLOTS 3
#define IDG_STEP_STORE_GRAD 1 /* the finished gradient is also written to `grad` (parity tests read it) */
#define IDG_STEP_PACED 2
typedef struct idg_step idg_step;
typedef struct idg_step_desc {
  const idg_graph* graph;      /* symmetric [n, n] handle, or NULL: no propagation */
  int64_t num_users, n, d;
  int n_layers, include_layer0;
  float reg_lambda;
  float* params;               /* [n, d] E0: users then items */
  float* grad;                 /* [n, d] d loss / d E0 (graph: rows outside the batch's receptive field are overwritten) */
  float* final_panel;          /* [n, d] layer mean (graph != NULL) */
  float* g_final;              /* [n, d] d loss / d final (graph != NULL) */
  float* exp_avg; float* exp_avg_sq;   /* [n, d] Adam moments */
  void* prop_ws;               /* idg_propagate_workspace_bytes(graph, d) (graph != NULL) */
  int64_t batch_capacity;      /* largest B of any call */
  uint32_t* slot_bitmap[IDG_STEP_SLOTS];  /* ceil(n / 32) words each, zeroed once */
  void* slot_units[IDG_STEP_SLOTS];       /* idg_graph_live_units_bytes(graph, 3 * batch_capacity) each (graph != NULL) */
  void* slot_bpr_ws[IDG_STEP_SLOTS];      /* idg_bpr_workspace_bytes(batch_capacity, d) each */
  void* side_stream;
  int flags;
} idg_step_desc;
int idg_step_create(const idg_step_desc* desc, idg_step** out);
int idg_step_destroy(idg_step* plan);
/* Prepare a batch a step ahead without running a step (the first batch of an epoch).  A prepared batch is identified by its
 * three pointers and B and is honoured by the NEXT idg_step_run_f32 only (any other prepared batch is dropped there): keep
 * the id arrays alive and unchanged until that call. */
int idg_step_prefetch(idg_step* plan, const int64_t* users, const int64_t* pos, const int64_t* neg, int64_t B,
                      uint64_t ids_token, void* stream);
/* next_* (nullable, next_B = 0: none): the batch the NEXT call will run.  loss: 2 floats [bpr, reg_lambda * reg].
 * adam_step: 1-based step count of this update; lr / betas / eps as idg_adam_step_f32.  flags: IDG_STEP_STORE_GRAD. */
int idg_step_run_f32(idg_step* plan, const int64_t* users, const int64_t* pos, const int64_t* neg, int64_t B,
                     const int64_t* next_users, const int64_t* next_pos, const int64_t* next_neg, int64_t next_B,
                     uint64_t ids_token, uint64_t next_ids_token, float* loss, int64_t adam_step, double lr, double beta1,
                     double beta2, double eps, int flags, void* stream);
/* The bitmap of the panel rows the LAST idg_step_run_f32 touched (its slot's; valid until that slot is reused two calls on). */
int idg_step_last_bitmap(const idg_step* plan, const uint32_t** out_bitmap);
/* Block the host until every step enqueued through the plan has finished AND every batch preparation it put on the side
 * stream has (a lookahead nobody ran still writes its slot's buffers): after this the plan's buffers may be released. */
int idg_step_synchronize(idg_step* plan);
/* Host-side accounting since the plan was made: out[0] = steps run, out[1] = nanoseconds spent inside idg_step_run_f32,
 * out[2] = of those, nanoseconds BLOCKED in the pacing wait (the device was the limit, not the host), out[3] = steps whose
 * stream did not have to wait for the side stream (the prepared batch was seen complete). */
int idg_step_stats(const idg_step* plan, int64_t out[4]);
/* Dense Adam (idg_adam_step_f32) whose gradient is read at the rows flagged in `rows` only and taken as ZERO elsewhere:
 * the update of a table whose step's gradient lives on the batch's <= 3B rows (MFBPR: no propagation spreads it) —
 * neither a zero-fill of the gradient panel nor its read.  Same arithmetic per element, so bit-identical to
 * idg_adam_step_f32 on a zero-filled panel. */
int idg_adam_rows_f32(float* param, const float* grad, const uint32_t* rows, float* exp_avg, float* exp_avg_sq, int64_t n,
                      int64_t d, double lr, double beta1, double beta2, double eps, int64_t step, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE: full-rank scoring, train-positive masking, top-K
 * (get_rating_for_test models/LightGCN.py:74-80, MFBPR.py:44-49; batch_test.Test
 *  utility/utility_train/batch_test.py:59-68)
 * ---------------------------------------------------------------------------------- */
/* rating[b, i] = act(<user_panel[users[b]], item_panel[i]>), act = sigmoid if apply_sigmoid.
 * rating: [Bt, I] row-major.  The dense matrix the reference's evaluator mutates. */
int idg_score_dense_f32(const float* user_panel, const float* item_panel, const int64_t* users,
                        int64_t Bt, int64_t I, int64_t d, int apply_sigmoid, float* rating,
                        void* stream);

/* Fused: scores go from the MFMA accumulators through an LDS slab into the selection and are never
 * written to global memory.  Entries (b, i) with i in the train row of users[b] (excl_indptr
 * [num_users+1] int64 / excl_items int32 ascending, DEVICE pointers, indexed by user id; NULL = no
 * masking) rank as the value -1 (batch_test.py:62-65).  The k best per row are returned sorted by
 * (raw score descending, item id ascending) — sigmoid is monotone, so this is one of the orders
 * torch.topk may return on the sigmoid values; out_val holds act(score), -1 for masked entries.
 * out_idx int64 [Bt,k], out_val fp32 [Bt,k] (may be NULL).  1 <= k <= min(I, 1024): k <= 64 is one pass;
 * a larger k (torch.topk takes any k <= I, batch_test.py:68) runs one scoring pass per 64 ranks, each admitting only
 * keys strictly below the last one the previous pass emitted (same order, same values as one pass would give).
 * ws: idg_score_topk_workspace_bytes, 16-byte aligned (exact forms: one 64-key list per user and item chunk, 512 B x Bt x
 * chunks; threshold + collect form: up to 1024 candidate keys per user — 8 to 16 KB x Bt — plus the bf16 operand tables,
 * (d / 16 + 1) KiB per 32 items and (d / 16 + 2) x 32 B per user).
 * Throughput wants Bt large — hand over EVERY test user in one call (there is no [Bt, I] matrix to
 * bound; what bounds a call is this workspace): the catalogue is only cut into chunks when Bt/64 workgroups cannot fill
 * the chip. */
size_t idg_score_topk_workspace_bytes(int64_t Bt, int64_t I, int64_t d, int k);
/* Which form a call of this geometry takes, for tests and diagnostics: info[0] = 0 every wave alternates between scoring and
 * selecting, 1 producer / consumer waves on exact fp32 scores, 3 (calls of >= 8 user tiles over >= 32,768 items, d = 64 / 128 /
 * 256, k <= 42; IDG_TOPK_OPT_COLLECT = 0 turns it off) threshold + collect + exact finish on one-sided bf16 bounds of the exact
 * score: a per-user floor from a strided sample of the catalogue scored as LOWER bounds, one pass that appends every item
 * whose UPPER bound reaches the floor to the user's candidate list, exact fp32 re-scoring of the candidates near the top —
 * bit-identical to forms 0 / 1, 3x (d = 64) to 10x (d = 256) as fast.  info[1] = catalogue chunks, info[2] = 1 when
 * chunks start from a floor (form 1).  Form 3 with `ws` the workspace of a FINISHED call on `stream` (synchronises), else -1:
 * info[3] = users redone one by one, exactly, over the whole catalogue (candidate list overflowed or short; a NaN / infinity /
 * a norm beyond 2^60 in the user's row), info[4] = users the finish could not serve (counted up to just past the fall-back
 * threshold: a lower bound when info[5] = 1), info[5] = 1 when the call as a whole
 * was answered by the exact form, whose launches follow every form-3 call and return at once otherwise (more than
 * IDG_TOPK_OPT_FALLBACK_PERMILLE of the users unservable — tables that tie massively — or an irregular ITEM row: decided
 * on the device, no host read; then info[3] = 0), info[6] = 1 when an item row was irregular.  info[7] = 0 (reserved). */
int idg_score_topk_info(int64_t Bt, int64_t I, int64_t d, int k, const void* ws, int64_t info[8], void* stream);
/* Diagnostics of a form-3 call (info[0] == 3) that has been ENQUEUED on `stream` with workspace `ws` and did not fall back:
 * out_counts[b] (device, int32 [Bt]) = the number of candidates the collect pass counted for user b — how many items'
 * upper bounds reached the user's floor (a list beyond its capacity sends the user to the exact pass).  What the
 * candidate capacity and the fall-back threshold are sized by; depends on the tables' norm spread.  Asynchronous. */
int idg_score_topk_candidate_counts(int64_t Bt, int64_t I, int64_t d, int k, const void* ws, int32_t* out_counts, void* stream);
/* Knobs of the form choice, process-wide, for tests and tuning.  Their initial values are read from the environment ONCE,
 * by the first call that needs them (IDG_TOPK_FORM, IDG_TOPK_COLLECT, IDG_TOPK_FLOOR, IDG_TOPK_WGS, IDG_TOPK_CHUNKS,
 * IDG_TOPK_FALLBACK_PERMILLE).  *previous (nullable) receives the old value; value = IDG_TOPK_OPT_KEEP only reads;
 * which = IDG_TOPK_OPT_RESET restores every default.  Not thread-safe against concurrent idg_score_topk_* calls. */
#define IDG_TOPK_OPT_FORM 0               /* -1 (default): by geometry; 0 / 1 / 3: force a kernel (3 where its domain allows) */
#define IDG_TOPK_OPT_COLLECT 1            /* 1; 0: never form 3 */
#define IDG_TOPK_OPT_FLOOR 2              /* 1; 0: many-chunk calls of form 1 without their floor phase */
#define IDG_TOPK_OPT_WGS 3                /* 0; > 0: workgroups wanted per launch */
#define IDG_TOPK_OPT_CHUNKS 4             /* 0; > 0: catalogue chunks */
#define IDG_TOPK_OPT_FALLBACK_PERMILLE 5  /* 20: form 3 hands the whole call to the exact form beyond this share of unservable
                                             users (at least 4); < 0: never (every such user is redone one by one) */
#define IDG_TOPK_OPT_COUNT 6
#define IDG_TOPK_OPT_RESET (-1)
#define IDG_TOPK_OPT_KEEP INT64_MIN
int idg_score_topk_option(int which, int64_t value, int64_t* previous);
int idg_score_topk_f32(const float* user_panel, const float* item_panel, const int64_t* users,
                       int64_t Bt, int64_t I, int64_t d, const int64_t* excl_indptr,
                       const int32_t* excl_items, int k, int apply_sigmoid, int64_t* out_idx,
                       float* out_val, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * DEVICE-LOCAL EVENTS: ordering between the caller's streams on ONE device (the step's stream and the stream that
 * prepares the next batch's index-only work).  Created without timing and WITHOUT the system-scope fence a default
 * HIP event performs when recorded (cache write-back/invalidate for the host's and other devices' benefit: ~7 us on
 * the recording stream); kernel boundaries already order memory at device scope.  Not for host-visible data.
 * ---------------------------------------------------------------------------------- */
int idg_event_create(void** out_event);
int idg_event_destroy(void* event);
int idg_event_record(void* event, void* stream);
int idg_stream_wait_event(void* stream, void* event);
int idg_event_query(void* event, int* done);
/* Block the calling host thread until the recorded work has completed (hipEventSynchronize): the engines use it to stay
 * at most two steps ahead of the device, so that a batch prepared on the side stream is KNOWN to be ready (idg_event_query)
 * when its step is enqueued and the step's stream does not have to wait for it. */
int idg_event_synchronize(void* event);

/* ------------------------------------------------------------------------------------
 * MULTI-GPU: RCCL collectives on the caller's stream (the reference is single-device,
 * utility/utility_train/trainer.py:8-74 — these serve the replicas / user-row shards around its step).
 * One communicator per process (one process per GPU).  Collectives are enqueued on `stream` in order with the
 * kernels around them.  The RCCL library is opened at run time, not linked: idg_comm_load(path) — NULL or "" for
 * the loader's default "librccl.so"; pass the copy the process already uses (PyTorch ships one).  Without it
 * every entry point below fails with IDG_E_UNSUPPORTED.
 * Bootstrap: rank 0 calls idg_comm_unique_id and hands the IDG_COMM_ID_BYTES bytes to every rank by any
 * out-of-band means; then EVERY rank calls idg_comm_create (collective: returns when all ranks have joined).
 * ---------------------------------------------------------------------------------- */
#define IDG_COMM_ID_BYTES 128
typedef struct idg_comm idg_comm;
int idg_comm_load(const char* librccl_path);
int idg_comm_rccl_version(int* version);
int idg_comm_unique_id(void* out_id /* IDG_COMM_ID_BYTES */);
int idg_comm_create(int rank, int world, const void* unique_id, int device, idg_comm** out);
int idg_comm_destroy(idg_comm* comm);
/* buf[0..count) <- sum over ranks (average != 0: mean over ranks), in place. */
int idg_allreduce_f32(idg_comm* comm, float* buf, int64_t count, int average, void* stream);
/* out[r * count .. (r + 1) * count) <- rank r's in[0..count).  In place when in == out + rank * count. */
int idg_allgather_f32(idg_comm* comm, const float* in, float* out, int64_t count, void* stream);
/* out[0..count) <- sum over ranks of their in[rank * count .. (rank + 1) * count): every rank hands in world * count
 * floats and keeps the reduced block it owns (ncclReduceScatter).  In place when out == in + rank * count.  The sharded
 * step ends its last backward exchange with this: each rank finishes the gradient and applies Adam for the item rows it
 * owns, and the updated rows go round by idg_allgather_f32. */
int idg_reduce_scatter_f32(idg_comm* comm, const float* in, float* out, int64_t count, void* stream);

/* ------------------------------------------------------------------------------------
 * MULTI-GPU, opt-in: the step's panel-sized exchanges as 24-bit rows with a rank-ordered sum (id-grec_amd/sharded/packed.py
 * Packed24Comm; SURVEY.md 8e "fix the reduction order (rank order) so k-GPU runs are reproducible run to run").
 * An fp32 value travels as its upper 24 bits (sign, exponent, 15 mantissa bits; the dropped byte rounded to nearest even:
 * 2^-16 relative), four values in three 32-bit words — 3/4 of the bytes of the fp32 exchange.  An all-reduce becomes
 * pack -> idg_alltoall_f32 (block p to rank p) -> idg_reduce24_f32 (the N blocks added in rank order, packed again) ->
 * idg_allgather_f32 of the packed result -> unpack; a reduce-scatter stops after the sum (fp32 out).  Counts `n` are fp32
 * VALUES (multiples of 4); a packed array of n values has 3n/4 words.  Buffers 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
int idg_pack24_f32(const float* src, uint32_t* dst, int64_t n, void* stream);
int idg_unpack24_f32(const uint32_t* src, float* dst, int64_t n, void* stream);
/* out <- blocks[0] + blocks[1] + ... + blocks[n_blocks - 1] in THAT order (block b: the 3n/4 words at blocks + b * 3n/4), as
 * fp32 (out_f32, nullable) and / or packed (out_packed, nullable; may be one of the input blocks' own words: each thread
 * reads its four values of every block before it writes). */
int idg_reduce24_f32(const uint32_t* blocks, int n_blocks, int64_t n, uint32_t* out_packed, float* out_f32, void* stream);
/* The same rank-ordered sum on fp32 blocks of n values each (no packing: `bench.py --reduce-order rank` with 32-bit panels —
 * RCCL's bytes on the links, one fixed sequence of adds).  out may be one of the blocks. */
int idg_reduce_blocks_f32(const float* blocks, int n_blocks, int64_t n, float* out, void* stream);
/* Block p (count floats) of `send` goes to rank p; block p of `recv` receives rank p's block for this rank (grouped
 * ncclSend / ncclRecv: on a fully connected node every peer's block travels over its own link).  Not in place.  The own
 * block is a device copy; flags = IDG_ALLTOALL_OWN_THROUGH_RCCL sends it through RCCL as well (tests on one device). */
#define IDG_ALLTOALL_OWN_THROUGH_RCCL 1
int idg_alltoall_f32(idg_comm* comm, const float* send, float* recv, int64_t count, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IDGREC_H */
