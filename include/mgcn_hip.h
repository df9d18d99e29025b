/*
 * mgcn_hip.h — C ABI of libmgcn_hip.so: the MI355X (gfx950) implementation of the M-GCN hot path.
 *
 * The reference (weilonghu/KGC-GCN) has no FFI of its own: the hot path is Python calling torch /
 * torch_geometric / torch_scatter tensor ops. Each entry point below therefore replaces a span of
 * reference Python, cited as file:line relative to the reference root. The Python host side
 * (kgc-gcn_amd/_native.py) binds these with ctypes; INTEGRATION.md shows the stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - plain C types only; `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - every pointer named *_dev is a BORROWED device pointer (owned by the caller, e.g. a torch
 *     tensor that outlives the call); pointers named *_host are host memory;
 *   - all device work is enqueued asynchronously on `stream`; nothing here allocates, frees or
 *     synchronises the device, so every call may be captured into a hipGraph;
 *   - return value 0 = MGCN_OK; otherwise an MGCN_E* code, and mgcn_last_error() returns a
 *     thread-local, human-readable message;
 *   - no global mutable state besides that thread-local error string (no cached device attributes, no environment
 *     variables); re-entrant per device;
 *   - matrices are row-major f32, indices int32 on the device, int64 on the host side of the feeder.
 */
#ifndef MGCN_HIP_H
#define MGCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGCN_ABI_VERSION 4

enum {
  MGCN_OK = 0,
  MGCN_EINVAL = 1,  /* bad argument: null pointer, negative size, index out of range, misalignment */
  MGCN_ELAUNCH = 2, /* hipGetLastError() after a launch */
  MGCN_EUNSUPPORTED = 3
};

/* One CSR slot = one directed edge in destination order. 16 bytes, read as one dwordx4. */
typedef struct mgcn_edge_rec {
  int32_t src;  /* source node (row of the layer input that is gathered)                          */
  int32_t type; /* row of the relation table [2R+1, D]                                             */
  float norm;   /* deg^-1/2[src] * deg^-1/2[dst], degrees counted by SOURCE within the half (Q2)  */
  int32_t eid;  /* reference edge id (row of the per-edge table in reference order)               */
} mgcn_edge_rec;

int mgcn_abi_version(void);
const char *mgcn_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * (0) Graph ingest on the host (replaces the two Python passes of data_loader.py:61-96 for triple
 * files of 10^7-10^8 lines). mgcn_ingest_open reads the three split files (one `subject relation object` triple per
 * line, any ASCII whitespace between tokens, universal newlines) and assigns entity / relation ids in first-seen
 * order over train, valid, test — per line subject, relation, object — with names lower-cased on insertion
 * (data_loader.py:64-70). Error behaviour follows the reference: a line without exactly three tokens is an error
 * (its tuple unpacking raises ValueError); a token that lower-casing changes is an error naming the token (its raw
 * lookup, data_loader.py:84-86, raises KeyError). A token with a byte >= 0x80 returns MGCN_EUNSUPPORTED (Python's
 * str.lower() is Unicode-aware): use the Python reader for such files.
 * mgcn_ingest_count: what = 0 entities, 1 relations (forward only; reverse relation r + R is implicit), 2 / 3 / 4 =
 * triples of train / valid / test. mgcn_ingest_triples: [n, 3] int64 (s, r, o) ids of a split (0 / 1 / 2).
 * mgcn_ingest_names: the names in id order as one byte string + [n+1] offsets (kind 0 entities, 1 relations).
 */
typedef struct mgcn_ingest mgcn_ingest;
int mgcn_ingest_open(const char *train_path, const char *valid_path, const char *test_path, mgcn_ingest **out);
void mgcn_ingest_close(mgcn_ingest *h);
int64_t mgcn_ingest_count(const mgcn_ingest *h, int32_t what);
int mgcn_ingest_triples(const mgcn_ingest *h, int32_t split, int64_t *triples_host);
int64_t mgcn_ingest_names_bytes(const mgcn_ingest *h, int32_t kind);
int mgcn_ingest_names(const mgcn_ingest *h, int32_t kind, char *bytes_host, int64_t *offsets_host);

/* The loader's known-answer index (data_loader.py:80-96: sr2o over the given triples, both directions — the reverse
 * query of (s, r, o) is (o, r + R, s)) in the form mgcn_filter_mask reads: sorted keys s * 2R + r, CSR pointers,
 * sorted distinct tails. Call with keys_host == NULL to obtain *num_keys / *num_tails, then with buffers of those sizes
 * (keys [num_keys], ptr [num_keys + 1], tails [num_tails]). */
int mgcn_filter_index_build(int64_t num_triples, const int64_t *triples_host, int64_t num_relations, int64_t *keys_host,
                            int64_t *ptr_host, int32_t *tails_host, int64_t *num_keys, int64_t *num_tails);

/* ---------------------------------------------------------------------------------------------
 * (1) Feeder — host side. Replaces data_loader.py:132-157 (`_build_graph`: the bi-directional edge
 * list) as consumed by model.py:88-97 (split into the in-half [0,E) and out-half [E,2E), degree
 * norms per half, `compute_norm` model.py:72-80, hoisted out of the step because the graph is
 * static).
 *   edge_index_host [2, 2E] int64 (row 0 = src, row 1 = dst), edge_type_host [2E] int64.
 * Slot layout produced: [in-half segments by destination | out-half segments by destination | hub segments],
 * every segment in edge-id order (the order a CPU scatter-add visits the edges). A destination with more than
 * hub_threshold slots in a half is a HUB (hub_threshold <= 0: no hubs): its segment moves to the hub region and is
 * cut into chunks of hub_chunk slots, so that no lane group ever walks a long list alone (degree skew);
 * the kernels sum each chunk separately and combine a hub's chunk sums in a fixed order (a strided partition over
 * the lane groups of one workgroup, then the group sums in group order) — still no atomics, still reproducible.
 * Outputs (host, caller-allocated):
 *   rowptr_host [2, N+1] int32   ABSOLUTE slot positions of the non-hub segments (a hub's segment there is empty);
 *   rec_host    [2E]             one record per slot;
 *   perm_host   [2E] int64       slot -> reference edge id (to lay the per-edge table out in slot order once);
 *   hubinfo_host [2, N, 2] int32 (first chunk, chunk count) of destination n in half h, (-1, 0) if not a hub;
 *   chunks_host [max_chunks, 4] int32  {begin, end, first chunk of its hub, chunk count of its hub}: absolute slot
 *                                range [begin, end) of every chunk; *num_chunks_host = chunks in use
 *                                (the three may be NULL when hub_threshold <= 0).
 * Optional outputs for the backward pass (all NULL or all non-NULL):
 *   slot_dst_host [2E] int32     destination node of each slot, bit 31 = half;
 *   mirror_host [2E] int32       slot of the reverse edge ((e + E) mod 2E) of each slot's edge: the edges leaving n
 *                                in half h are the reverses of the edges entering n in half 1-h, so by-SOURCE sums
 *                                walk the destination runs / hub chunks of the other half through this map.
 *                                Needs src[e + E] == dst[e] && dst[e + E] == src[e] for every e < E (the loader's
 *                                list, data_loader.py:143-149); the feeder CHECKS it and, for a list that is not
 *                                mirror-symmetric (the operator seam model.py:82-101 accepts any list), fills mirror
 *                                with -1: everything else stays valid (forward, gee, grel), but gx must not be
 *                                requested from mgcn_aggregate_bwd with such a map (the Python seam raises);
 *   typeptr_host [num_rel_rows+1] int32, typeslots_host [2E] int32
 *                                all slots (ascending) grouped by relation-table row.
 * Fails with MGCN_EINVAL if an endpoint is outside [0,N) or a type outside [0,num_rel_rows-1): the last row of the
 * relation table is the self-loop row (model.py:86), which only the self-loop pass reads.
 */
int mgcn_csr_build_host(int64_t num_nodes, int64_t num_edges_half, int64_t num_rel_rows,
                        const int64_t *edge_index_host, const int64_t *edge_type_host,
                        int64_t hub_threshold, int64_t hub_chunk, int32_t *rowptr_host,
                        mgcn_edge_rec *rec_host, int64_t *perm_host, int32_t *hubinfo_host,
                        int32_t *chunks_host, int64_t max_chunks, int64_t *num_chunks_host,
                        int32_t *slot_dst_host, int32_t *mirror_host, int32_t *typeptr_host,
                        int32_t *typeslots_host);

/* (1v) The LIVE VIEW of the slot layout — host side, graph-static, additive (the canonical arrays above stay as they are).
 * The degrees behind `norm` are counted by SOURCE within a half (Q2), so norm is exactly 0.0f for every slot whose
 * destination never occurs as a source in the same half (leaf entities): a source has degree >= 1, so a destination's
 * run is dead as a whole or live as a whole. Such slots add m * 0 to their sum; the view leaves them out, and the
 * fused forward launched on it (2b, "Live view") never loads their rows.
 *   rowptr_host [2, N+1], rec_host: the canonical arrays of (1) (only the non-hub slots rowptr covers are read).
 *   *num_live_host / *num_dead_host: non-hub slots with norm != 0.0f / == 0.0f. With no dead slot nothing else is
 *     written (the outputs may be NULL): the canonical layout is its own live view, callers build none.
 *   live_rowptr_host [2, N+1] int32: ABSOLUTE positions into live_rec_host, contiguous runs, in-half then out-half
 *     (monotone from 0 to *num_live_host; a hub's run is empty as in rowptr_host);
 *   live_rec_host [max_live >= *num_live_host]: the slots with norm != 0.0f in canonical order, {src, type, norm, row}:
 *     the fourth word is the slot's canonical (absolute) slot index — the row of the slot-ordered per-edge table, minus
 *     the shard offset ee_sub of (2b) — where the canonical record carries the reference edge id.
 * Call with the outputs NULL to size live_rec_host, or pass max_live = the non-hub slot count. */
int mgcn_csr_live_view_host(int64_t num_nodes, const int32_t *rowptr_host, const mgcn_edge_rec *rec_host,
                            int32_t *live_rowptr_host, mgcn_edge_rec *live_rec_host, int64_t max_live,
                            int64_t *num_live_host, int64_t *num_dead_host);

/* ---------------------------------------------------------------------------------------------
 * (2) Aggregation forward. Replaces the gather / message / scatter-add of the three `propagate`
 * calls, model.py:99-101 + 111-118 (+ the identity gathers model.py:29-30), with the weight
 * multiply moved after the sum:
 *   A[n, 0:D)   = sum over in-half  slots p of n:  norm_p * ((x[src_p] * rel[type_p]) * ee_p)
 *   A[n, D:2D)  = same over the out-half
 *   A[n, 2D:3D) = (x[n] * loop_rel) * loop_edge                       (self loop, no norm)
 * The relation table has num_rel_rows rows: rows [0, num_rel_rows-1) at rel_dev, the last (self-loop)
 * row at loop_rel_dev [D] — two pointers so the caller needs no concatenation (model.py:86); they may
 * point into one contiguous [num_rel_rows, D] tensor.
 * Slots of one destination are summed in slot order by one lane group: no atomics, bitwise
 * reproducible. `ee_dev` is the per-edge table: in SLOT order if ee_in_slot_order != 0 (streamed),
 * else in reference edge-id order (gathered through rec.eid); NULL = no per-edge factor.
 *   x_dev [N, D] (ldx floats between rows), rel_dev [num_rel_rows-1, D], loop_edge_dev [D] or NULL
 *   (then the third block is not written and A needs only 2D columns), a_dev [N, lda].
 * Only destinations [node_begin, node_end) are processed (rows of a_dev indexed by global node id): row chunks
 * can be pipelined against (4) on another stream, and a destination partition is one rank's share.
 * Hubs: [chunk_begin, chunk_end) are the chunks of the hubs among [node_begin, node_end) — one run, because the hub
 * region is in node order (all chunks for the whole graph). When it is not empty (hubinfo_dev / chunks_dev from the
 * feeder) ONE pre-pass launch on the same stream writes the chunk sums to partial_dev [chunk_end - chunk_begin, D] and
 * folds every hub's chunk sums into the row of its first chunk (the last lane group to arrive at a hub's counter adds the
 * rows up in row order: a fixed summation tree), and the main launch adds that one row per hub. partial_dev holds
 * mgcn_hub_partial_floats(chunk_end - chunk_begin, D) floats: the rows, then 2 * (chunk_end - chunk_begin) int32 arrival
 * counters which must be ZERO before the first launch that uses the buffer; every completed launch leaves them zero, so a
 * buffer can be reused by later launches on the same stream without clearing (not by launches that may overlap).
 * Table shard (ABI 2): as in the fused launch below, ee_dev may hold only the rows a destination range needs — its
 * in-half slots, its out-half slots, its hub slots, each a contiguous run — with ee_sub_in / ee_sub_out / ee_sub_hub such
 * that the row of (absolute) slot s is s - ee_sub_{region}; all three are 0 with the whole table. This is what lets a
 * rank of the destination partition hold 1/W of a table that does not fit one GPU (configs[4]: 410 GB).
 */
int64_t mgcn_hub_partial_floats(int64_t num_chunks, int32_t dim);
int mgcn_aggregate_fwd(int64_t num_nodes, int64_t num_edges_half, int32_t dim, int32_t num_rel_rows,
                       const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev, const float *x_dev,
                       int64_t ldx, const float *rel_dev, const float *loop_rel_dev, const float *ee_dev,
                       int32_t ee_in_slot_order, const float *loop_edge_dev, float *a_dev, int64_t lda,
                       int64_t node_begin, int64_t node_end, const int32_t *hubinfo_dev, const int32_t *chunks_dev,
                       int64_t chunk_begin, int64_t chunk_end, float *partial_dev, int64_t ee_sub_in, int64_t ee_sub_out,
                       int64_t ee_sub_hub, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (3) Aggregation backward (autograd through (2); driven by main.py:66). Given g = dL/dA [N, lda]
 * (first 2D columns used):
 *   gx[s]   = sum over slots p with src_p = s of norm_p * g[dst_p, half] * rel[type_p] * ee_p
 *   gee[p]  = norm_p * g[dst_p, half] * x[src_p] * rel[type_p]                 (slot order)
 *   grel[t] = sum over slots p with type_p = t of norm_p * g[dst_p, half] * x[src_p] * ee_p
 * gx[s] walks the destination runs of s (rowptr, both halves) and maps every slot to its reverse edge through
 * `mirror` — within a run that is edge-id order, the order of the CPU index_add; hubs are summed per chunk by a
 * pre-pass and folded exactly as in (2) (hubinfo / chunks / num_hub_chunks of the whole graph). grel walks
 * typeptr/typeslots (slots grouped by relation row, long lists cut into fixed chunks whose partial sums are added in
 * chunk order); all from mgcn_csr_build_host. Sums in a fixed order: no float atomics, bitwise reproducible.
 * Any of gx/gee/grel may be NULL. gx [N, D], gee [2E, D] in slot order, grel [num_rel_rows, D]. ee_dev is in slot
 * order. workspace_dev: mgcn_aggregate_bwd_workspace bytes, 16-byte aligned.
 */
int mgcn_aggregate_bwd(int64_t num_nodes, int64_t num_edges_half, int32_t dim, int32_t num_rel_rows,
                       const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev,
                       const int32_t *slot_dst_dev /* bit 31 = half */, const int32_t *mirror_dev,
                       const int32_t *hubinfo_dev, const int32_t *chunks_dev, int64_t num_hub_chunks,
                       const int32_t *typeptr_dev, const int32_t *typeslots_dev, const float *x_dev, int64_t ldx, const float *rel_dev, const float *ee_dev,
                       const float *g_dev, int64_t ldg, float *gx_dev, float *gee_dev, float *grel_dev,
                       float *workspace_dev, size_t workspace_bytes, void *stream);
size_t mgcn_aggregate_bwd_workspace(int64_t num_edges_half, int32_t dim, int32_t num_rel_rows, int64_t num_hub_chunks);

/* (3s) Aggregation backward of ONE destination range [node_begin, node_end) from its table shard — one rank's share of the
 * training step of the destination partition (kgc-gcn_amd/dist.py train_step_sharded). The shard is the table of (2):
 * rows_in in-half rows, then rows_out out-half rows, then rows_hub hub rows, row r of a region at slot r + ee_sub_{region}.
 * g_dev holds the gradient of the range's rows only (row 0 = node_begin, first 2D columns used). Outputs:
 *   gee [rows, D]   = (3)'s gee of the shard's slots, in shard order (bit-identical to (3)'s rows of those slots);
 *   grel [num_rel_rows, D] = (3)'s sum restricted to the shard's slots (a partial: the ranks' grel add up to (3)'s);
 *   gx [N, D] (optional) = for every node, (3)'s by-source sum restricted to the shard's slots (zero rows where the shard has
 *                          none; a partial: the ranks' gx add up to (3)'s).
 * Index lists (built once per graph and range, kgc-gcn_amd/graph.py GraphCSR.shard_backward_index; they only cover the shard's
 * rows, no rank walks the whole graph):
 *   type_ptr [num_rel_rows + 1], type_rows [rows]: the shard's rows grouped by relation row, ascending (slot order);
 *   src_ptr [2N + 1], src_rows [rows]: entries [src_ptr[2s + h], src_ptr[2s + h + 1]) = the rows whose slot lies in half h and
 *     leaves node s, ordered by the slot of the reverse edge (the order in which (3) walks s's destination runs of half 1 - h);
 *   src_chunks [num_hub_chunks][4]: for every hub chunk c of the graph (include (1); hubinfo of the whole graph), {first, end)
 *     entries of src_rows whose reverse slot lies in chunk c, first chunk of its hub, chunk count of its hub}.
 * grel uses (3)'s one-pass gee + by-type chunk sums over type_rows and its final fold; gx walks src_rows per (node, half) and takes
 * a hub's chunk sums through (3)'s fold. Sums in fixed orders, no float atomics. With the whole graph as the range (one rank)
 * every output is bit-identical to (3)'s. workspace: mgcn_aggregate_bwd_shard_workspace bytes, 16-byte aligned. */
size_t mgcn_aggregate_bwd_shard_workspace(int64_t shard_rows, int32_t dim, int32_t num_rel_rows, int64_t num_hub_chunks);
int mgcn_aggregate_bwd_shard(int64_t num_nodes, int64_t num_edges_half, int32_t dim, int32_t num_rel_rows,
                             const mgcn_edge_rec *rec_dev, const int32_t *slot_dst_dev, int64_t node_begin, int64_t node_end,
                             int64_t rows_in, int64_t rows_out, int64_t rows_hub, int64_t ee_sub_in, int64_t ee_sub_out,
                             int64_t ee_sub_hub, const int32_t *src_ptr_dev, const int32_t *src_rows_dev,
                             const int32_t *hubinfo_dev, const int32_t *src_chunks_dev, int64_t num_hub_chunks,
                             const int32_t *type_ptr_dev, const int32_t *type_rows_dev, const float *x_dev, int64_t ldx,
                             const float *rel_dev, const float *ee_dev, const float *g_dev, int64_t ldg, float *gx_dev,
                             float *gee_dev, float *grel_dev, float *workspace_dev, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (4) Dense step + epilogue (f32 MFMA, exact f32). Replaces model.py:116 (moved after the sum) and
 * model.py:103-106 in eval mode:
 *   out = tanh( BN_eval( (A[:,0:D) W_in + A[:,D:2D) W_out + A[:,2D:3D) W_loop) / 3 + bias ) )
 * BN_eval(v) = (v - mean) / sqrt(var + eps) * gamma + beta. bias_dev may be NULL.
 * w_dev [3*dim_in, dim_out] = W_in, W_out, W_loop stacked by rows (one contiguous matrix).
 */
int mgcn_dense_bn_tanh_fwd(int64_t num_nodes, int32_t dim_in, int32_t dim_out, const float *a_dev, int64_t lda,
                           const float *w_dev, const float *bias_dev, const float *bn_mean_dev, const float *bn_var_dev,
                           const float *bn_gamma_dev, const float *bn_beta_dev, float bn_eps,
                           float *out_dev, int64_t ldo, void *stream);

/* (2)+(4) in ONE launch (eval mode): out = tanh(BN_eval((A_in W_in + A_out W_out + A_loop W_loop)/3 + bias)); the
 * aggregates of (2) are built tile by tile in LDS and multiplied there, they never reach HBM. One 1024-thread workgroup
 * per CU owns one contiguous run of destinations; 32-lane groups (16 bytes per lane) sum their destinations' slots in
 * slot order — the sums of (2) —, split each finished row exactly into three bf16 pieces in LDS, and
 * v_mfma_f32_16x16x32_bf16 multiplies them; the epilogue runs on the accumulators. Kernels behind this entry point
 * (mgcn_fused_kernel_generation tells which one a launch takes):
 *   generation 2, dim_in <= 256 and dim_out <= 208  csrc/layer_fused2.hip: eight waves gather, eight multiply; tiles of 80
 *       (or 64) destinations, stages of 128 input columns per mode, two LDS images, one workgroup barrier per stage;
 *   generation 3, otherwise (dim_in <= 1024, dim_out <= 512), and generation 2's shapes when the caller brings row bounds
 *       for a launch short of two tiles per CU  csrc/layer_fused3.hip: one contiguous run of rows per workgroup in tiles of
 *       48-80, stages of 128 input columns (256 through `tune` only), a ring of f32 staging buffers coupled by LDS counters,
 *       13 or 32 column tiles.
 *       Generations 2 and 3 run the same arithmetic (k order, products, and for dim_out > 128 the weight packing): rows
 *       are bit-identical between them.
 * Arguments as in (2) and (4), except that the weights are passed in MFMA fragment order: wp_dev = mgcn_pack_weights() of
 * the stacked [3*dim_in, dim_out] matrix (mgcn_packed_weights_bytes bytes, 16-byte aligned; re-pack whenever a weight
 * changes; the *_gen forms pack for a generation forced through `tune`; 0 = the shape's own, which generations 2 and 3 share for
 * dim_out > 128; for any other `generation` than 0, 2 or 3 the size is 0 and packing returns MGCN_EINVAL). Returns
 * MGCN_EUNSUPPORTED (and does nothing) unless all operands are 16-byte aligned, ee_dev is given in slot order, dim_in % 4 == 0, dim_in <= 1024, dim_out % 4 == 0 and dim_out <= 512 — callers then use (2) followed by (4).
 * NUMERIC CONTRACT. The dense step is not the exact-f32 MFMA of (4): every aggregate a and weight w is split EXACTLY
 * into three bf16 pieces (hi = bf16(v) rounded to nearest, mid = bf16(v - hi), lo = v - hi - mid; hi + mid + lo == v bit
 * for bit) and the six products hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid are accumulated in f32; the dropped terms
 * are below 2^-26 |a||w| per product. For finite inputs |out - exact| <= 4 u B + 2e-7 with u = 2^-24 and
 * B = sum_k |a_k||w_k| * |gamma| / (3 sqrt(var + eps)) (tests/test_gpu_round3.py holds both this launch and (2)+(4) to
 * it on rows with 2^40 of dynamic range; on the benchmark's data both are within 5e-7 of float64). Results are
 * bit-identical across launches of this entry point with `tune` bits 10-11 = 0 (whole graph, any destination range, any
 * table shard, any row bounds, either of generations 2 / 3, any tile geometry) but differ from (2)+(4) in the last bits (<= 2e-6 on a tanh output for
 * dim_in <= 256). A non-finite input (inf / NaN) in a gathered row makes that destination's output row NaN, where
 * (2)+(4) may return +-1; other rows are unaffected.
 * Destination partition: only destinations [node_begin, node_end) are computed; out_dev holds THOSE rows
 * (row 0 = node_begin). A rank may hold only its shard of the slot-ordered per-edge table — the rows of the in-half
 * slots [rowptr_in[node_begin], rowptr_in[node_end]) followed by those of the out-half slots of the same nodes — and
 * then the hub slots [chunks[chunk_begin].begin, chunks[chunk_end - 1].end) of the same nodes — and passes
 * ee_sub_in / ee_sub_out / ee_sub_hub such that the row of (absolute) slot s is s - ee_sub_{region}; with the whole
 * table all three are 0. x_dev is always the whole [N, D] layer input. The kernels carry ee_sub_in / ee_sub_out as int32 (slot
 * indices are below 2^31) and the row stride of x as uint32: an offset outside int32 is MGCN_EINVAL, ldx >= 2^31 is
 * MGCN_EUNSUPPORTED (callers use (2) + (4), whose strides are 64-bit); every address is then formed in 64 bits.
 * Hubs as in (2): hubinfo_dev / chunks_dev / [chunk_begin, chunk_end) / partial_dev [mgcn_hub_partial_floats(chunk_end -
 * chunk_begin, dim_in)] with its counters zero (one pre-pass launch before the layer's launch).
 * rel_out_dev (optional, [num_rel_rows - 1, dim_out]) = rel_dev @ rels_weight_dev [dim_in, dim_out] (model.py:107, the
 * relations the next layer / the scorer read) computed by the same launch after its last gather stage,
 * with the arithmetic of mgcn_matmul_f32's small-matrix kernel (bit-identical results); NULL = not computed.
 * row_bounds_dev (optional; NULL / 0 = equal runs): num_row_bounds + 1 strictly increasing row offsets from node_begin, first 0,
 * last node_end - node_begin: workgroup i takes destinations [b_i, b_i+1) — the caller's work-balanced runs
 * (slots + a constant per row; one run per CU; no run longer than the equal split ceil(rows / runs) rounded up to 16 rows (up to 80) or to 80 rows (past it), which is what the tile
 * height is chosen for), computed once per graph on the host (GraphCSR.workgroup_bounds). Rows do not
 * depend on the runs (fixed k order per row). With bounds given, a generation-2 shape whose tiling would leave the chip short of
 * two tiles per CU takes generation 3 (dim_out > 128); generation 2 itself ignores them. The bounds are read by the launch, not
 * checked: offsets outside the range are the caller's error.
 * tune: 0 = automatic. For A/B runs only (never needed for correctness): bits 0-3 row tiles per tile (3..5); bits 4-7
 * generation 3: staging buffers (1..4); bits 8-9 relation table in LDS (1 = never); bits 10-11 force a generation (2 or 3;
 * wp_dev must then come from mgcn_pack_weights_gen for it; 1 is reserved — it forced the removed generation 4 — and is refused
 * with MGCN_EINVAL before anything is launched); bits 12-13 generation 3: input columns per slot walk (0 or 1 = 128, 2 = 256);
 * bit 14 generations 2 and 3: the legacy column cut (below).
 * Column cut. Generations 2 and 3 (128-column walk) gather a mode's dim_in columns in chunks of at most 128, one slot walk per
 * chunk, every chunk starting on a k-block (32 columns). Rows of the layer input lie 4 * dim_in bytes apart, so the 128-byte
 * lines a chunk touches depend on where it starts. For 128 < dim_in <= 256 the boundary is the multiple of 32 columns (neither
 * chunk above 128) that minimises the mean number of lines per row over the row offsets that stride produces (the multiples
 * of gcd(4 * dim_in, 128)); ties go to the more balanced cut, then to the wider first chunk: dim_in = 200 is cut 96 | 104. Every
 * other width keeps chunks of 128 with the last one short. Where a mode has more than one chunk, lanes past a chunk's width load
 * that chunk's last float4 (and store zeros), so no lane touches a line its pass does not need; a single chunk (dim_in <= 128)
 * keeps them on columns 0-3, which its pass fetches anyway. The legacy cut (`tune` bit 14; MGCN_FUSED_CUT=legacy in the Python
 * binding) is 128 | rest with those lanes on columns 0-3 of the row. The k-blocks, their order and the packed weights do not
 * depend on the cut: rows are bit-identical either way. mgcn_fused_cut reports the cut and its modelled lines.
 * status_dev (optional, one zero-initialised uint32 in device memory): generation 3 couples its roles through LDS counters
 * with BOUNDED spins; a spin that runs out (a wave parked for ~0.1 s by a debugger, a preemption, or a protocol error)
 * lets its wave go on, the rows of that tile are then garbage, and bit 0 of *status_dev is set: callers check the word at
 * their next synchronisation point (kgc-gcn_amd/_native.py check_fused_status). Generation 2 has no spins.
 * Live view. mgcn_layer_fwd_fused_live is the same launch with the main slot walk of generations 2 and 3 on the live view
 * of (1v): live_rowptr_dev / live_rec_dev take the place of rowptr_dev / rec_dev for the partition, the record chunks and
 * the runs, and a slot's per-edge row is its record's fourth word - ee_sub_{region}; rec_dev stays the CANONICAL record
 * array, which the hub pre-pass reads through chunks_dev as before (dead hub slots are still walked there). Same
 * dispatcher, same generation choice, same row bounds, ranges and shards (the row word is an absolute slot index).
 * CONTRACT: for finite inputs the rows are bit-identical to the
 * canonical launch's (s + m * 0 == s, and a run of dead slots only is +0 either way). A non-finite value in an x row or
 * per-edge row that ONLY dead slots read no longer reaches the output: the canonical launch (and the reference) give
 * NaN for that destination, this launch gives the row of the finite terms. */
/* The kernel a launch of (2b) over num_rows destinations takes with `tune` bits 10-11 = 0: 2 (layer_fused2.hip) or 3
 * (layer_fused3.hip). Informational (profiles, benchmarks name the kernel they measured). */
int mgcn_fused_kernel_generation(int32_t dim_in, int32_t dim_out, int64_t num_rows, int32_t with_row_bounds);
/* The column cut of (2b) for dim_in input columns (legacy != 0: the legacy cut), no device work. Returns the number of chunks
 * and writes each chunk's first column and width to col0_out / ncol_out [max_chunks] (either may be NULL) and the modelled mean
 * number of 128-byte lines one input row costs per mode, idle lanes included, to *mean_lines_out (may be NULL); -1 for a width no
 * fused kernel takes or more chunks than max_chunks. */
int mgcn_fused_cut(int32_t dim_in, int32_t legacy, int32_t *col0_out, int32_t *ncol_out, int32_t max_chunks,
                   double *mean_lines_out);
int mgcn_layer_fwd_fused(int64_t num_nodes, int64_t num_edges_half, int32_t dim_in, int32_t dim_out,
                         int32_t num_rel_rows, const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev,
                         const float *x_dev, int64_t ldx, const float *rel_dev, const float *loop_rel_dev,
                         const float *ee_dev, int32_t ee_in_slot_order, const float *loop_edge_dev,
                         const float *wp_dev, const float *bias_dev, const float *bn_mean_dev,
                         const float *bn_var_dev, const float *bn_gamma_dev, const float *bn_beta_dev,
                         float bn_eps, float *out_dev, int64_t ldo, int64_t node_begin, int64_t node_end,
                         int64_t ee_sub_in, int64_t ee_sub_out, int64_t ee_sub_hub, const int32_t *hubinfo_dev,
                         const int32_t *chunks_dev, int64_t chunk_begin, int64_t chunk_end, float *partial_dev,
                         const float *rels_weight_dev, float *rel_out_dev, const int32_t *row_bounds_dev,
                         int32_t num_row_bounds, int32_t tune, uint32_t *status_dev, void *stream);
int mgcn_layer_fwd_fused_live(int64_t num_nodes, int64_t num_edges_half, int32_t dim_in, int32_t dim_out,
                              int32_t num_rel_rows, const int32_t *live_rowptr_dev, const mgcn_edge_rec *live_rec_dev,
                              const mgcn_edge_rec *rec_dev, const float *x_dev, int64_t ldx, const float *rel_dev,
                              const float *loop_rel_dev, const float *ee_dev, int32_t ee_in_slot_order,
                              const float *loop_edge_dev, const float *wp_dev, const float *bias_dev,
                              const float *bn_mean_dev, const float *bn_var_dev, const float *bn_gamma_dev,
                              const float *bn_beta_dev, float bn_eps, float *out_dev, int64_t ldo, int64_t node_begin,
                              int64_t node_end, int64_t ee_sub_in, int64_t ee_sub_out, int64_t ee_sub_hub,
                              const int32_t *hubinfo_dev, const int32_t *chunks_dev, int64_t chunk_begin,
                              int64_t chunk_end, float *partial_dev, const float *rels_weight_dev, float *rel_out_dev,
                              const int32_t *row_bounds_dev, int32_t num_row_bounds, int32_t tune, uint32_t *status_dev,
                              void *stream);
int mgcn_pack_weights(int32_t dim_in, int32_t dim_out, const float *w_dev, float *wp_dev, size_t wp_bytes, void *stream);
size_t mgcn_packed_weights_bytes(int32_t dim_in, int32_t dim_out);
int mgcn_pack_weights_gen(int32_t generation, int32_t dim_in, int32_t dim_out, const float *w_dev, float *wp_dev,
                          size_t wp_bytes, void *stream);
size_t mgcn_packed_weights_bytes_gen(int32_t generation, int32_t dim_in, int32_t dim_out);

/* ---------------------------------------------------------------------------------------------
 * (2e) The forward launches on a bf16 per-edge table — inference only, additive (MGCN_ABI_VERSION stays 4, as with the _dev
 * entry points of (10) and (12)). ee_dev [2E, D] (or a destination range's shard) holds bf16 values as uint16_t, non-NULL;
 * every other argument is that of the f32 sibling of (2) / (2b).
 *   bf16(v)   = the f32 value v rounded to nearest even to 16 bits (torch: tensor.to(torch.bfloat16));
 *   widen(h)  = the f32 whose bit pattern is uint32(h) << 16 (exact).
 * CONTRACT: a launch given the bf16 table T computes exactly what its f32 sibling computes from the f32 table widen(T): the
 * same products in the same order by the same instructions, bit-identical rows. Only the per-edge row's load differs: 2 bytes
 * per element instead of 4, then a shift. Alignment: the vector paths want ee_dev 8-byte aligned (D % 4 == 0 makes every row
 * so); mgcn_aggregate_fwd_ee16 takes a table that is only 2-byte aligned on its element-wise path (as the f32 launch takes a
 * misaligned operand), the fused launches return MGCN_EUNSUPPORTED. Generations 2 and 3 read the bf16 table, on the
 * canonical layout and on the live view. The hub pre-pass
 * reads the same table. There is no backward: (3) and (3s) take f32 tables only (a bf16 table is a deployment form of a
 * trained model). */
int mgcn_aggregate_fwd_ee16(int64_t num_nodes, int64_t num_edges_half, int32_t dim, int32_t num_rel_rows,
                            const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev, const float *x_dev, int64_t ldx,
                            const float *rel_dev, const float *loop_rel_dev, const uint16_t *ee_dev,
                            int32_t ee_in_slot_order, const float *loop_edge_dev, float *a_dev, int64_t lda,
                            int64_t node_begin, int64_t node_end, const int32_t *hubinfo_dev, const int32_t *chunks_dev,
                            int64_t chunk_begin, int64_t chunk_end, float *partial_dev, int64_t ee_sub_in,
                            int64_t ee_sub_out, int64_t ee_sub_hub, void *stream);
int mgcn_layer_fwd_fused_ee16(int64_t num_nodes, int64_t num_edges_half, int32_t dim_in, int32_t dim_out,
                              int32_t num_rel_rows, const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev,
                              const float *x_dev, int64_t ldx, const float *rel_dev, const float *loop_rel_dev,
                              const uint16_t *ee_dev, int32_t ee_in_slot_order, const float *loop_edge_dev,
                              const float *wp_dev, const float *bias_dev, const float *bn_mean_dev,
                              const float *bn_var_dev, const float *bn_gamma_dev, const float *bn_beta_dev,
                              float bn_eps, float *out_dev, int64_t ldo, int64_t node_begin, int64_t node_end,
                              int64_t ee_sub_in, int64_t ee_sub_out, int64_t ee_sub_hub, const int32_t *hubinfo_dev,
                              const int32_t *chunks_dev, int64_t chunk_begin, int64_t chunk_end, float *partial_dev,
                              const float *rels_weight_dev, float *rel_out_dev, const int32_t *row_bounds_dev,
                              int32_t num_row_bounds, int32_t tune, uint32_t *status_dev, void *stream);
int mgcn_layer_fwd_fused_live_ee16(int64_t num_nodes, int64_t num_edges_half, int32_t dim_in, int32_t dim_out,
                                   int32_t num_rel_rows, const int32_t *live_rowptr_dev,
                                   const mgcn_edge_rec *live_rec_dev, const mgcn_edge_rec *rec_dev, const float *x_dev,
                                   int64_t ldx, const float *rel_dev, const float *loop_rel_dev, const uint16_t *ee_dev,
                                   int32_t ee_in_slot_order, const float *loop_edge_dev, const float *wp_dev,
                                   const float *bias_dev, const float *bn_mean_dev, const float *bn_var_dev,
                                   const float *bn_gamma_dev, const float *bn_beta_dev, float bn_eps, float *out_dev,
                                   int64_t ldo, int64_t node_begin, int64_t node_end, int64_t ee_sub_in,
                                   int64_t ee_sub_out, int64_t ee_sub_hub, const int32_t *hubinfo_dev,
                                   const int32_t *chunks_dev, int64_t chunk_begin, int64_t chunk_end, float *partial_dev,
                                   const float *rels_weight_dev, float *rel_out_dev, const int32_t *row_bounds_dev,
                                   int32_t num_row_bounds, int32_t tune, uint32_t *status_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (4t) The layer's epilogue in TRAINING mode and its backward (model.py:103-106 under .train(), driven by main.py:61-66):
 *   z = (u_in + u_out + u_loop) / 3 (+ bias)        u_* [N, O] = the three products of model.py:116, dropout already applied
 *   y = tanh((z - mean) * rstd * gamma + beta)      mean / rstd = BATCH statistics over the N rows (biased variance),
 * running_mean / running_var updated as nn.BatchNorm1d does (momentum, unbiased variance); either both NULL or both given.
 * z, y [N, O] contiguous; save_mean / save_rstd [O] are kept for the backward. Reductions over rows are two-stage with fixed
 * row blocks (bitwise reproducible). workspace: mgcn_bn_tanh_train_workspace(N, O) bytes.
 * Backward: given gy = dL/dy, returns gz = dL/dz [N, O], gu = gz / 3 (= dL/du_* before the dropout masks), ggamma, gbeta [O].
 * Every entry point of (4t) and (4s) returns MGCN_EINVAL, nothing launched, for num_rows * dim_out above 2^37 elements (their
 * launch grids are sized in 32 bits; addresses inside the kernels are 64-bit).
 */
size_t mgcn_bn_tanh_train_workspace(int64_t num_rows, int32_t dim_out);
int mgcn_bn_tanh_train_fwd(int64_t num_rows, int32_t dim_out, const float *u_in_dev, const float *u_out_dev,
                           const float *u_loop_dev, int64_t ldu, const float *bias_dev, const float *gamma_dev,
                           const float *beta_dev, float *running_mean_dev, float *running_var_dev, float momentum, float eps,
                           float *z_dev, float *y_dev, float *save_mean_dev, float *save_rstd_dev, float *workspace_dev,
                           size_t workspace_bytes, void *stream);
int mgcn_bn_tanh_train_bwd(int64_t num_rows, int32_t dim_out, const float *z_dev, const float *y_dev, const float *gy_dev,
                           const float *save_mean_dev, const float *save_rstd_dev, const float *gamma_dev, float *gz_dev,
                           float *gu_dev, float *ggamma_dev, float *gbeta_dev, float *workspace_dev, size_t workspace_bytes,
                           void *stream);

/* (4s) (4t) split into stages around an exchange, for the destination partition's training step: each rank holds num_rows rows of
 * the layer and reduces them in the same fixed 128-row blocks as (4t); between the stages the caller gathers every rank's per-block
 * partials ([ceil(num_rows / 128), O] each) and passes them all, rank after rank, as num_blocks rows; total_rows = the rows of all
 * ranks. The folds add the blocks in the order given, so every rank, a rank without rows included, computes the same bits for mean,
 * rstd, ggamma, gbeta and (from the same starting values) the running statistics. When every rank's first row is a multiple of 128
 * (always with one rank) the blocks are (4t)'s blocks and all results are bit-identical to (4t)'s. At any other cut -- a rank counts
 * its blocks from ITS first row, so a boundary that is no multiple of 128 leaves a short last block on one rank and shifts the blocks
 * of the next -- the sums are associated differently: still the same bits on every rank, and within the float64 bars that hold for
 * (4t) (tests/dense_ref.py: train_bars), but not (4t)'s bits. z is row-local and equals (4t)'s z at every cut.
 * z_dev, y_dev, gy_dev are contiguous [num_rows, O] (there is no leading dimension); every per-column vector has O elements.
 *   stage_sum:    z (as (4t)) and its per-block column sums -> part [nblk, O];
 *   stage_center: mean = (sum of the blocks) / total_rows, then the per-block sums of (z - mean)^2 -> part [nblk, O];
 *   stage_finish: rstd and the running statistics from the blocks of stage_center, then y = tanh(BN(z));
 *   bwd_stage_sums:  per-block sums of g_pre = gy * (1 - y^2) and of g_pre * xhat -> g_part, gx_part [nblk, O];
 *   bwd_stage_apply: gbeta / ggamma = the folds of all ranks' blocks, then gz and gu = gz / 3 for the rank's rows.
 * num_rows may be 0 (a rank without rows contributes no blocks). */
int mgcn_bn_train_stage_sum(int64_t num_rows, int32_t dim_out, const float *u_in_dev, const float *u_out_dev,
                            const float *u_loop_dev, int64_t ldu, const float *bias_dev, float *z_dev, float *part_dev, void *stream);
int mgcn_bn_train_stage_center(int64_t num_rows, int32_t dim_out, const float *z_dev, const float *sum_parts_dev, int64_t num_blocks,
                               int64_t total_rows, float *mean_dev, float *part_dev, void *stream);
int mgcn_bn_train_stage_finish(int64_t num_rows, int32_t dim_out, const float *z_dev, const float *sq_parts_dev, int64_t num_blocks,
                               int64_t total_rows, const float *mean_dev, const float *gamma_dev, const float *beta_dev,
                               float *running_mean_dev, float *running_var_dev, float momentum, float eps, float *rstd_dev,
                               float *y_dev, void *stream);
int mgcn_bn_train_bwd_stage_sums(int64_t num_rows, int32_t dim_out, const float *z_dev, const float *y_dev, const float *gy_dev,
                                 const float *save_mean_dev, const float *save_rstd_dev, float *g_part_dev, float *gx_part_dev,
                                 void *stream);
int mgcn_bn_train_bwd_stage_apply(int64_t num_rows, int32_t dim_out, const float *z_dev, const float *y_dev, const float *gy_dev,
                                  const float *save_mean_dev, const float *save_rstd_dev, const float *gamma_dev,
                                  const float *g_parts_dev, const float *gx_parts_dev, int64_t num_blocks, int64_t total_rows,
                                  float *gz_dev, float *gu_dev, float *ggamma_dev, float *gbeta_dev, void *stream);

/* C[M, N] = A^T B for A [K, M] (lda), B [K, N] (ldb): the weight gradient of model.py:116, dW = aggregate^T g (K = number of
 * nodes). Split over K (fixed ranges, partial products added in range order: reproducible), exact-f32 MFMA. M <= 208, N <= 256,
 * else MGCN_EUNSUPPORTED. workspace: mgcn_matmul_tn_workspace(K, M, N) bytes. */
size_t mgcn_matmul_tn_workspace(int64_t k, int32_t m, int32_t n);
int mgcn_matmul_tn_f32(int64_t k, int32_t m, int32_t n, const float *a_dev, int64_t lda, const float *b_dev, int64_t ldb,
                       float *c_dev, int64_t ldc, float *workspace_dev, size_t workspace_bytes, void *stream);

/* Plain C[M,N] = A[M,K] @ B[K,N] on the same f32 MFMA kernel (model.py:107, the relation projection). */
int mgcn_matmul_f32(int64_t m, int32_t k, int32_t n, const float *a_dev, int64_t lda, const float *b_dev,
                    int64_t ldb, float *c_dev, int64_t ldc, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (5) Full-graph scoring and filtered ranking. Replaces model.py:177-179 and main.py:122-126.
 *   score[b, n] = sigmoid( x[b,:] . ent[n,:] + bias[n] ),  x [B, O], ent [n_local, O].
 * mgcn_score_fwd materialises score [B, n_local] (training / the drop-in forward()).
 * mgcn_score_target computes target[b] = score[b, obj[b]] for the queries whose obj lies in
 *   [ent_row0, ent_row0 + n_local) with the SAME arithmetic as the other two (others untouched).
 * One arithmetic for all three, chosen by shape alone: 16-byte aligned operands with dim % 4 == 0 and dim <= 352 take the
 *   six-product bf16 split on the bf16 MFMA (exact three-way split of both operands, f32 accumulation: the numeric
 *   contract of (2)+(4) in one launch below; 6/16 of the exact-f32 MFMA's time); other shapes the exact-f32 MFMA. A score
 *   is the same f32 value whichever of the three entry points computes it, so counts are exact against a recount over
 *   mgcn_score_fwd's scores.
 * mgcn_score_rank never materialises the scores: for every b it adds to counts[b, 0..2]
 *   gt   = #{n != obj[b], not filtered : score[b,n] >  target[b]}
 *   tl   = #{n != obj[b], not filtered, n <  obj[b] : score[b,n] == target[b]}   (ties_lower)
 *   ties = #{n != obj[b], not filtered : score[b,n] == target[b]}
 * where n is filtered iff label[b, n] != 0 after the reference's label.byte() (f32 rows, stride ldl, the shard's own
 * columns), or — when mask_dev is given instead of label_dev — iff bit (n & 31) of mask[b, n >> 5] is set
 * (uint32 rows, stride ldm words; built on the device by mgcn_filter_mask). Exactly one of label_dev / mask_dev.
 * counts [B,3] int64 must be zeroed by the caller; integer atomics => order independent.
 * rank = 1 + gt (+ tl under the stable tie rule). With an entity shard per GPU the caller sums
 * counts over ranks (RCCL all-reduce); `ent_row0` is the shard's first global entity id.
 */
int mgcn_score_fwd(int32_t batch, int64_t n_local, int32_t dim, const float *x_dev, int64_t ldx,
                   const float *ent_dev, int64_t lde, const float *bias_dev, float *score_dev, int64_t lds,
                   void *stream);
int mgcn_score_target(int32_t batch, int64_t n_local, int64_t ent_row0, int32_t dim, const float *x_dev,
                      int64_t ldx, const float *ent_dev, int64_t lde, const float *bias_dev,
                      const int64_t *obj_dev, float *target_dev, void *stream);
int mgcn_score_rank(int32_t batch, int64_t n_local, int64_t ent_row0, int32_t dim, const float *x_dev,
                    int64_t ldx, const float *ent_dev, int64_t lde, const float *bias_dev,
                    const int64_t *obj_dev, const float *target_dev, const float *label_dev, int64_t ldl,
                    const uint32_t *mask_dev, int64_t ldm, int64_t *counts_dev, void *stream);
/* Training loss fused with the scoring pass (replaces model.py:177-179 + model.py:42-44 and the
 * autograd of both down to the logits, main.py:61-66): for z[b, n] = x[b,:] . ent[n,:] + bias[n], p = sigmoid(z) and
 * targets y[b, n] = hot where bit n of mask[b] is set, cold elsewhere (mgcn_filter_mask over the TRAIN index; hot / cold
 * as in mgcn_label_rows), ONE launch writes
 *   grad_logit_dev [n_local, ldg] (row = entity, column = query): d mean-BCE / d z = (p - y) / max(p(1-p), 1e-12) * p(1-p)
 *                  * inv_count — torch's BCELoss and sigmoid backward formulas multiplied out, inv_count = 1 / (B * N);
 *   loss_partial_dev [mgcn_score_bce_partials(batch, n_local)]: per-workgroup sums of
 *                  (y - 1) * max(log1p(-p), -100) - y * max(log(p), -100), reduced in a fixed order; the loss is their
 *                  sum * inv_count.
 * Neither the scores nor the [B, N] targets are materialised. The caller finishes the backward with plain GEMMs:
 * d ent = G @ x (mgcn_matmul_f32), d x = G^T @ ent, d bias = row sums of G. Returns MGCN_EUNSUPPORTED unless operands
 * are 16-byte aligned, dim % 4 == 0 and batch % 4 == 0 (callers then use mgcn_score_fwd + the framework's loss). */
int64_t mgcn_score_bce_partials(int32_t batch, int64_t n_local);
int mgcn_score_bce_fwd(int32_t batch, int64_t n_local, int32_t dim, const float *x_dev, int64_t ldx, const float *ent_dev,
                       int64_t lde, const float *bias_dev, const uint32_t *mask_dev, int64_t ldm, float hot, float cold,
                       float inv_count, float *grad_logit_dev, int64_t ldg, float *loss_partial_dev, void *stream);

/* Filter bits on the device (replaces building + shipping the dense [B, N] label block of data_loader.py:34-51
 * for evaluation). keys_dev [num_keys] sorted int64 (subject * num_rel_ids + relation), ptr_dev
 * [num_keys+1], tails_dev [ptr[num_keys]] int32: the known tails of each (subject, relation). For query b with key
 * qkey_dev[b] the bits of its tails inside [ent_row0, ent_row0 + n_local) are set in mask_dev[b, :] (zeroed here). */
int mgcn_filter_mask(int32_t batch, const int64_t *qkey_dev, int64_t num_keys, const int64_t *keys_dev,
                     const int64_t *ptr_dev, const int32_t *tails_dev, int64_t ent_row0, int64_t n_local,
                     uint32_t *mask_dev, int64_t ldm, void *stream);

/* Training targets on the device (SURVEY N2 for the train loop; replaces the per-sample dense label rows of
 * data_loader.py:34-51 and their host-to-device copy, main.py:62): out_dev[b, n] = hot if entity ent_row0 + n is a known
 * tail of query b's key, else cold. The caller passes hot = (1 - eps) * 1 + 1/N and cold = (1 - eps) * 0 + 1/N evaluated
 * in f32 as numpy does (data_loader.py:41-43), or 1 and 0 without smoothing. Index arrays as in mgcn_filter_mask
 * (built over the TRAIN split). out_dev [batch, ldo >= n_local]. */
int mgcn_label_rows(int32_t batch, const int64_t *qkey_dev, int64_t num_keys, const int64_t *keys_dev,
                    const int64_t *ptr_dev, const int32_t *tails_dev, int64_t ent_row0, int64_t n_local, float hot,
                    float cold, float *out_dev, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (7) Filtered top-k link prediction: the k most likely tails of each query (h, r, ?), the job of model.py:177-179
 * that the reference leaves to torch.topk over the [B, N] block. Head prediction is the inverse-relation query
 * (t, r + R, ?), as the loader builds it (data_loader.py:80-96).
 * mgcn_score_topk, for x [B, O] against the shard ent [n_local, O] / bias [n_local] whose rows are global ids
 * [ent_row0, ent_row0 + n_local):
 *   score  the f32 value mgcn_score_fwd produces for (b, n), bit for bit (the shard is scored through that launch, in
 *          chunks of at most 2^18 rows into the workspace, so both arithmetic paths of (5) apply as there);
 *   filter entity n is excluded when bit (n & 31) of mask[b, n >> 5] is set (the bits of mgcn_score_rank, built by
 *          mgcn_filter_mask; ldm words per row); mask_dev == NULL excludes nothing;
 *   order  score descending, then global id ascending (compared as f32 values: -0 == +0): the order of a stable
 *          descending sort over the ids in ascending order, the tie rule of the rank counts (rank = 1 + gt + tl);
 *          NaN scores (mgcn_score_fwd gives none for finite operands; a merge may be handed some) are ordered too: a
 *          NaN with the sign bit clear ranks above +inf, a NaN with the sign bit set below -inf, and NaNs among
 *          themselves by bit pattern (IEEE totalOrder with the two zeros merged: the order of an order-preserving
 *          integer key). A returned zero is +0; a returned NaN is a NaN, its payload unspecified;
 *   output out_score [B, ldo >= k] f32 and out_id [B, ldi >= k] int64 in that order; a row with fewer than k unfiltered
 *          entities is padded at its end with score -inf and id -1.
 * The result depends on nothing but the scores: not on the chunking, the launch geometry, the arrival order of the
 * (integer) LDS atomics, or the sharding. Selection: every chunk is cut into segments of 4096 columns; one workgroup per
 * (query, segment) keeps the segment's k best (radix select on an order-preserving 32-bit key with the id below it,
 * bitonic sort of at most 1024 pairs in LDS), and one workgroup per query folds the segments' lists and the running
 * list of the chunks before (the kernel of mgcn_topk_merge). A shard of one segment takes the single launch.
 * Limits: 1 <= k <= 1024; batch, n_local, dim as mgcn_score_fwd; ent_row0 + n_local <= 2^31 - 1 (ids are int32 on
 * the device). workspace_dev: mgcn_score_topk_workspace(batch, n_local, k) bytes, 16-byte aligned; with
 * C = min(n_local, 2^18) rows per chunk and S = ceil(C / 4096) segments, it is
 *   align256(4 B round4(C)) + align256(4 B (S + 1) k) + 8 B (S + 1) k   (align256: up to a multiple of 256)
 * which does not grow with n_local past 2^18 rows (0 is returned for arguments outside the limits).
 * mgcn_topk_merge: the top-k, in the order above, of `lists` candidate lists of k per query: list l of query b is
 * in_score / in_id [b * ld_in + l * k, + k); entries with id < 0 are padding and are skipped, the others have distinct
 * ids in [0, 2^31) (the lists need not be sorted). out [B, k] contiguous, padded as above; it must not overlap the input.
 * Merging the lists of the shards of a table equals mgcn_score_topk over the whole table (dist.sharded_topk).
 */
size_t mgcn_score_topk_workspace(int32_t batch, int64_t n_local, int32_t k);
int mgcn_score_topk(int32_t batch, int64_t n_local, int64_t ent_row0, int32_t dim, const float *x_dev, int64_t ldx,
                    const float *ent_dev, int64_t lde, const float *bias_dev, const uint32_t *mask_dev, int64_t ldm,
                    int32_t k, float *out_score_dev, int64_t ldo, int64_t *out_id_dev, int64_t ldi, void *workspace_dev,
                    size_t workspace_bytes, void *stream);
int mgcn_topk_merge(int32_t batch, int32_t lists, const float *in_score_dev, const int64_t *in_id_dev, int64_t ld_in,
                    int32_t k, float *out_score_dev, int64_t *out_id_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (8) ConvE query trunk, eval mode (model.py:161-175): from the encoder's two tables to the query embeddings x [B, O]
 * that (5) and (7) score. For query b with s = ent[src_index[b]] and r = rel[rel_index[b]] (both [O], O = k_w * k_h):
 *   image [2 k_w, k_h], flat element 2 j = s[j], 2 j + 1 = r[j] (the reference interleaves the two rows);
 *   bn0 (one channel, running statistics); valid kernel_size x kernel_size convolution to num_filter channels of H x W,
 *   H = 2 k_w - kernel_size + 1, W = k_h - kernel_size + 1 (conv bias optional); bn1 per channel; relu; flatten to
 *   f H W + y W + x; fc [O, num_filter H W] + bias; bn2 per output; relu.
 * mgcn_conve_pack folds bn0 / conv bias / bn1 into scaled taps and one constant per filter, fc bias / bn2 into one
 * scale and shift per output (in double, rounded once) and lays fc.weight out in MFMA fragment order:
 * mgcn_conve_packed_bytes bytes (0 for a geometry that is refused), 16-byte aligned. Re-pack whenever one of its inputs
 * changes. conv_w [num_filter, kernel_size^2] and the BN vectors are contiguous; conv_b, fc_b and the BN gamma / beta
 * pointers may be NULL (no bias; gamma 1, beta 0); fc_w rows are ldw floats apart.
 * mgcn_conve_trunk_fwd gathers the rows itself: src_index / rel_index [B] int64, NULL = rows 0 .. B-1 (the table must
 * then have at least B rows); an index outside [0, rows) is clamped to the table. out [B, ldo >= O] f32.
 * Arithmetic: the convolution is an f32 fma chain in tap order, the fc product runs on v_mfma_f32_16x16x4_f32 (exact
 * f32). The [B, num_filter H W] activation is never stored: each activation is formed in the register that feeds the
 * MFMA. Summation order of one output: the K axis is cut into ceil(H W / 4) segments (four positions of every filter),
 * each one accumulation chain in filter order from 0; the segment sums are added in ascending order from 0; then
 * relu(fma(total, scale, shift)). The order is a function of the geometry alone: a query's row has the same bits
 * whatever the batch, its position in it, or the launch form. Up to 8192 queries the segments are spread over workgroups
 * through workspace_dev (mgcn_conve_trunk_workspace(batch, ...) bytes, 16-byte aligned; [segments, B, round16(O)] f32)
 * and a second launch adds them; larger batches walk them inside one wave and need no workspace (0 bytes, NULL allowed).
 * No atomics, no spinning. A non-finite value in a query's rows makes that output row non-finite and leaves all others
 * unchanged.
 * Takes k_w * k_h == O <= 512, 1 <= kernel_size <= min(2 k_w, k_h), num_filter >= 1, a pack below 2^31 floats;
 * MGCN_EINVAL for anything that is not a ConvE geometry, MGCN_EUNSUPPORTED (nothing done) for O > 512 or a larger pack.
 */
size_t mgcn_conve_packed_bytes(int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter, int32_t dim_out);
int mgcn_conve_pack(int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter, int32_t dim_out,
                    const float *conv_w_dev, const float *conv_b_dev, const float *fc_w_dev, int64_t ldw,
                    const float *fc_b_dev, const float *bn0_mean_dev, const float *bn0_var_dev,
                    const float *bn0_gamma_dev, const float *bn0_beta_dev, float bn0_eps, const float *bn1_mean_dev,
                    const float *bn1_var_dev, const float *bn1_gamma_dev, const float *bn1_beta_dev, float bn1_eps,
                    const float *bn2_mean_dev, const float *bn2_var_dev, const float *bn2_gamma_dev,
                    const float *bn2_beta_dev, float bn2_eps, void *packed_dev, size_t packed_bytes, void *stream);
size_t mgcn_conve_trunk_workspace(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                                  int32_t dim_out);
int mgcn_conve_trunk_fwd(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                         int32_t dim_out, const float *ent_dev, int64_t lde, int64_t ent_rows,
                         const int64_t *src_index_dev, const float *rel_dev, int64_t ldr, int64_t rel_rows,
                         const int64_t *rel_index_dev, const void *packed_dev, float *out_dev, int64_t ldo,
                         void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (9) ConvE query trunk, training mode, forward and backward (csrc/conve_train.hip): bn0 -> convolution -> bn1 -> relu ->
 * feature_drop -> fc with BATCH statistics, from the gathered rows s, r [B, O] (rows lds / ldr floats apart) to z [B, ldz >= O].
 * With the image x[b, 2 j] = s[b, j], x[b, 2 j + 1] = r[b, j] of (8), P = H W, K = num_filter P, pi(p, t) the image element
 * under tap t of position p:
 *   bn0 (one channel, n0 = 2 O B): mu0, var0 (biased), xh = (x - mu0) rstd0, x0 = g0 xh + b0
 *   c[b, f, p] = cb[f] + sum_t w[f, t] x0[b, pi(p, t)]            an fma chain in tap order, from cb[f] (0 without a bias)
 *   bn1 (per filter, n1 = B P): mu1, var1, ch = (c - mu1) rstd1, a = g1 ch + b1
 *   h[b, k] = keep[b, k] inv_keep max(a, 0), k = f P + p          keep: one byte per element, NULL = keep all (inv_keep is 1)
 *   z = h fc_w^T + fc_b
 * and for gz [B, ldg >= O]:
 *   d fc_b = sum_b gz;  d fc_w[o, k] = sum_b gz[b, o] h[b, k];  gh = gz fc_w
 *   ga = gh keep inv_keep [a > 0] (0 at a == 0);  d b1[f] = sum_{b, p} ga;  d g1[f] = sum_{b, p} ga ch
 *   gc = g1 rstd1 (ga - d b1 / n1 - ch d g1 / n1)
 *   d cb[f] = sum gc;  d w[f, t] = sum_{b, p} gc[b, f, p] x0[b, pi(p, t)];  gx0[b, i] = sum over pi(p, t) = i of gc[b, f, p] w[f, t]
 *   d b0 = sum gx0;  d g0 = sum gx0 xh;  gx = g0 rstd0 (gx0 - d b0 / n0 - xh d g0 / n0);  ds[b, j] = gx[b, 2 j], dr[b, j] = gx[b, 2 j + 1]
 * Variances are two-pass (mean, then centred squares), rstd = 1 / sqrt(var + eps). The forward writes saved_dev
 * [2 + 2 num_filter] = mu0, rstd0, mu1[...], rstd1[...] and updates the running statistics in place as nn.BatchNorm does
 * (running = (1 - momentum) running + momentum stat, the variance unbiased: n / (n - 1)); num_batches_tracked is the caller's.
 * Arithmetic: exact f32. The three products (h fc_w^T, gz^T h, gz fc_w) run on v_mfma_f32_16x16x4_f32; h is formed from c in the
 * register that feeds the MFMA. Convolution, correlation and tap gradients are fmaf chains.
 * Reductions: no atomics, no spinning, no workgroup waits on another. Every sum over the batch is a multi-launch reduction: one
 * partial per block of rows (bn0: 8 rows; bn1, its backward sums, taps and conv bias: 16 rows; d fc_b: 32 rows; the bn0 backward
 * sums: 1 row, folded in blocks of 16 rows and then across the blocks), each a strided per-thread chain and a halving tree over the workgroup, then the partials added in ascending
 * block order from 0 (up to 128 partials an f32 chain; more -- bn0 past 1024 rows, the 16-row blocks past 2048 -- in a double
 * accumulator, rounded once). h fc_w^T is cut along K into up to 128 splits of whole 16-element units; a split is one MFMA chain in
 * ascending k, the splits are added in ascending order from 0, then the bias. gz^T h is one chain over ascending rows, gz fc_w one
 * over ascending outputs. The launch plan is a function of (batch, geometry) alone: same inputs and mask, same bits.
 * workspace_dev: mgcn_conve_train_workspace(batch, ...) bytes (0 = refused), 16-byte aligned, in floats from its start (each
 * section rounded up to 4): c [B, K] (the forward leaves it there and the backward READS it: pass the same, untouched workspace),
 * ga / gc [B, K], gx0 [B, 2 O], split partials [S, B, O], the (mu1, rstd1, g1, b1) table [num_filter, 4], (mu0, rstd0, g0, b0),
 * then the partials of bn0 (sum, squares), bn1 (sum, squares), bn1 backward, bn0 backward, taps + conv bias, d fc_b.
 * The backward also takes the forward's s, r, weights, mask and saved_dev. A NULL gradient pointer skips that output (and the
 * launches only it needs) and leaves the bits of the others unchanged. conv_w [num_filter, kernel_size^2] contiguous; conv_b,
 * fc_b and keep_dev may be NULL; the BN gamma / beta and running pointers are required.
 * Takes the geometries of (8) (k_w k_h == O <= 512, 1 <= kernel_size <= min(2 k_w, k_h), num_filter >= 1) and 1 <= B <= 4096 with
 * B P >= 2 and B K < 2^31. All checks precede the first launch: MGCN_EINVAL for a null required pointer, a negative size, a
 * leading dimension that is too small, a misaligned or too small workspace, and anything that is not a ConvE geometry;
 * MGCN_EUNSUPPORTED, nothing written, for the rest.
 */
size_t mgcn_conve_train_workspace(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter,
                                  int32_t dim_out);
int mgcn_conve_train_fwd(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter, int32_t dim_out,
                         const float *s_dev, int64_t lds, const float *r_dev, int64_t ldr, const float *conv_w_dev,
                         const float *conv_b_dev, const float *fc_w_dev, int64_t ldw, const float *fc_b_dev,
                         const float *bn0_gamma_dev, const float *bn0_beta_dev, float *bn0_running_mean_dev,
                         float *bn0_running_var_dev, float bn0_momentum, float bn0_eps, const float *bn1_gamma_dev,
                         const float *bn1_beta_dev, float *bn1_running_mean_dev, float *bn1_running_var_dev, float bn1_momentum,
                         float bn1_eps, const uint8_t *keep_dev, float inv_keep, float *z_dev, int64_t ldz, float *saved_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);
int mgcn_conve_train_bwd(int32_t batch, int32_t k_w, int32_t k_h, int32_t kernel_size, int32_t num_filter, int32_t dim_out,
                         const float *s_dev, int64_t lds, const float *r_dev, int64_t ldr, const float *conv_w_dev,
                         const float *fc_w_dev, int64_t ldw, const float *bn0_gamma_dev, const float *bn0_beta_dev,
                         const float *bn1_gamma_dev, const float *bn1_beta_dev, const uint8_t *keep_dev, float inv_keep,
                         const float *saved_dev, const float *gz_dev, int64_t ldg, float *ds_dev, int64_t ldds, float *dr_dev,
                         int64_t lddr, float *d_conv_w_dev, float *d_conv_b_dev, float *d_bn0_gamma_dev, float *d_bn0_beta_dev,
                         float *d_bn1_gamma_dev, float *d_bn1_beta_dev, float *d_fc_w_dev, int64_t lddw, float *d_fc_b_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (10) Global-norm clipping and the Adam update (csrc/optim.hip; replaces main.py:69-70, clip_grad_norm_ followed by
 * torch.optim.Adam.step, amsgrad = False, maximize = False). Three entry points over a LIST of n f32 tensors, given as HOST
 * arrays of device pointers and of int64 element counts; a tensor with a NULL gradient or 0 elements is skipped (its other
 * pointers may be NULL, nothing of it is read or written). Nothing is kept between calls: the pointers travel by value in
 * the kernel arguments, MGCN_ADAM_BATCH tensors per launch, one workgroup per MGCN_ADAM_CHUNK elements of a tensor.
 * mgcn_adam_sq_norms: sq_dev[i] = sum of squares of gradient i (0 for a skipped one), i < n. Order: a workgroup sums its
 *   chunk (256 threads, each four chains over its float4s in ascending order, combined (c0 + c1) + (c2 + c3), then a halving
 *   tree); one wave folds a tensor's chunk partials in double (lane l takes chunks l, l + 64, ... in ascending order, then
 *   a halving tree over the lanes). No atomics: same inputs, same bits. workspace_dev: mgcn_adam_sq_norms_workspace bytes
 *   (one float per chunk of EVERY tensor of the list, 4-byte aligned; NULL allowed when that is 0).
 * mgcn_adam_clip_coef: out_dev[0] = total = sqrt(sum of sq_dev[0 .. n)) (summed in double as above), out_dev[1] = coef =
 *   min(max_norm / (total + 1e-6), 1), clip_grad_norm_'s formulas in f32. A caller that shards tensors over devices
 *   all-reduces those entries of sq_dev between the two calls; the host never reads the norm.
 * mgcn_adam_step, per element, in f32, in this order of operations (torch's single-tensor Adam; no contraction):
 *   g' = coef g;  g' = g' + weight_decay p (only when weight_decay != 0);  m = m + (1 - beta1)(g' - m);
 *   v = v beta2 + ((1 - beta2) g') g';  p = p + (-step_size)(m / (sqrt(v) / bc2_sqrt + eps))
 *   with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) formed by the caller in double; coef is read from
 *   coef_dev (out_dev + 1 of the call above), NULL = 1. Gradients are read, never written. 16-byte accesses when the four
 *   bases of a tensor are 16-byte aligned, scalar accesses otherwise and for the last numel % 4 elements.
 * mgcn_adam_step_dev: mgcn_adam_step with the two scalars that change from step to step read on the device: hyper_dev points to
 *   two floats, step_size and bc2_sqrt (4-byte aligned), which every workgroup loads before it forms -step_size. With the same two
 *   float values in memory every output bit equals mgcn_adam_step's. For a launch that is captured into a hipGraph once and
 *   replayed: the host writes each step's pair (still formed in double and rounded to float) into that memory ahead of the
 *   replay. Pointers, lengths, betas, eps and weight_decay still travel by value; the values in memory are not checked
 *   (MGCN_EINVAL for a NULL or misaligned hyper_dev).
 * All checks precede the first launch and write nothing: MGCN_EINVAL for n < 0, a NULL array, a negative length, a live
 * tensor with a NULL p / m / v, a beta outside [0, 1), eps, weight_decay, max_norm or step_size (a negative lr) below 0 or
 * not a number, bc2_sqrt outside (0, 1], a NULL, misaligned or too small workspace; MGCN_EUNSUPPORTED for more than 2^31
 * chunks in one launch.
 */
#define MGCN_ADAM_CHUNK 8192 /* elements per workgroup */
#define MGCN_ADAM_BATCH 64   /* tensors per launch */
size_t mgcn_adam_sq_norms_workspace(int64_t n, const int64_t *numel_host);
int mgcn_adam_sq_norms(int64_t n, const float *const *grad_host, const int64_t *numel_host, float *sq_dev,
                       void *workspace_dev, size_t workspace_bytes, void *stream);
int mgcn_adam_clip_coef(int64_t n, const float *sq_dev, float max_norm, float *out_dev, void *stream);
int mgcn_adam_step(int64_t n, const float *const *grad_host, float *const *param_host, float *const *exp_avg_host,
                   float *const *exp_avg_sq_host, const int64_t *numel_host, const float *coef_dev, float step_size,
                   float bc2_sqrt, double beta1, double beta2, double eps, double weight_decay, void *stream);
int mgcn_adam_step_dev(int64_t n, const float *const *grad_host, float *const *param_host, float *const *exp_avg_host,
                       float *const *exp_avg_sq_host, const int64_t *numel_host, const float *coef_dev, const float *hyper_dev,
                       double beta1, double beta2, double eps, double weight_decay, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (11) The training step's query path between the encoder and the scorer (csrc/query_train.hip): the backward of the two
 * query-row gathers of MGCN.forward (model.py:35-36, all_ent[src] and all_rel[rel]) and the trunk's tail hidden_drop -> bn2 ->
 * relu (model.py:173-175) with batch statistics, forward and backward. Plain pointers with leading dimensions (every tensor may
 * be a column window of a wider one), all checks before the first launch, a refusal writes nothing. No float atomics, no
 * spinning, no workgroup waits on another: the same inputs give the same bits at every launch.
 *
 * mgcn_query_rows_bwd: out [num_rows, dim] (rows ldo floats apart) is written completely, bit for bit as the sequential f32 loop
 *     out[:] = 0;  for b in 0 .. batch - 1: out[idx[b], :] += d[b, :]
 *   writes it: the addends of a row are added one after another in ascending b, from 0. Rows that no b names are zero; columns
 *   dim .. ldo of a window are not touched. An idx[b] outside [0, num_rows) is never followed and adds nothing. Three launches:
 *   one workgroup sorts the unique 64-bit keys idx[b] << 12 | b in LDS (so the plan is a function of idx alone) and leaves the
 *   sorted (row, b) pairs in the workspace; a fill zeroes the window; a sum gives each run of equal rows to the workgroup of its
 *   first sorted position, whose threads (one per column) walk the run. workspace_dev: mgcn_query_rows_bwd_workspace(batch)
 *   bytes (0 = refused), 16-byte aligned. 1 <= batch <= MGCN_QUERY_MAX_BATCH, dim >= 1, 1 <= num_rows <= 2^50.
 *
 * mgcn_conve_tail_fwd, for z [batch, dim] and the optional byte keep-mask keep [batch, dim] (NULL = keep all, inv_keep is 1; the
 *   convention of (9)), per column:
 *     u = (z keep) inv_keep;  mean = (sum_b u) / B;  res = (sum_b (u - mean)) / B;  c = (u - mean) - res
 *     var = (sum_b c^2) / B;  rstd = 1 / sqrt(var + eps);  x = max((c rstd) gamma + beta, 0)
 *   (res is what the f32 mean leaves of the centred column: rows that nearly coincide cancel in u - mean down to the mean's own
 *   rounding error, which rstd then multiplies; c sums to zero to the accuracy of the differences themselves.)
 *   saved_dev [2, dim] (rows ldsv apart) = mean, rstd; the running statistics are updated in place as nn.BatchNorm1d does
 *   (running = (1 - momentum) running + momentum stat, the variance unbiased: sum / (B - 1)); num_batches_tracked is the caller's.
 * mgcn_conve_tail_bwd, for gx [batch, dim] and the forward's z, keep, x and saved_dev:
 *     ga = gx [x > 0];  d beta = sum_b ga;  d gamma = sum_b ga uh, uh = c rstd with c centred as in the forward
 *     gz = ((gamma rstd ((ga - d beta / B) - uh d gamma / B)) keep) inv_keep
 *   The relu mask is read from the forward's own output. gz_dev, d_gamma_dev and d_beta_dev may each be NULL, which only
 *   removes work and leaves the bits of the others unchanged.
 *   One launch each: a workgroup owns 16 columns over all rows. Every batch sum is a per-thread chain over rows t, t + 16, ...
 *   in ascending order and a halving tree over the 16 chains, so its order depends on B alone and a column's results do not
 *   depend on which other columns are in the call. 2 <= batch <= MGCN_QUERY_MAX_BATCH, dim >= 1.
 * MGCN_EINVAL for a null required pointer, a negative batch, dim < 1, num_rows < 1, a leading dimension below dim, an inv_keep
 * that is negative or not finite, a momentum outside [0, 1], a negative eps, a misaligned or too small workspace;
 * MGCN_EUNSUPPORTED, nothing written, for a batch outside the limits (batch = 1 for the tail: one value per channel has no
 * batch statistics) and for num_rows > 2^50.
 */
#define MGCN_QUERY_MAX_BATCH 4096
size_t mgcn_query_rows_bwd_workspace(int32_t batch);
int mgcn_query_rows_bwd(int32_t batch, int64_t num_rows, int32_t dim, const int64_t *idx_dev, const float *d_dev, int64_t ldd,
                        float *out_dev, int64_t ldo, void *workspace_dev, size_t workspace_bytes, void *stream);
int mgcn_conve_tail_fwd(int32_t batch, int32_t dim, const float *z_dev, int64_t ldz, const uint8_t *keep_dev, int64_t ldk,
                        float inv_keep, const float *gamma_dev, const float *beta_dev, float *running_mean_dev,
                        float *running_var_dev, float momentum, float eps, float *x_dev, int64_t ldx, float *saved_dev,
                        int64_t ldsv, void *stream);
int mgcn_conve_tail_bwd(int32_t batch, int32_t dim, const float *z_dev, int64_t ldz, const uint8_t *keep_dev, int64_t ldk,
                        float inv_keep, const float *x_dev, int64_t ldx, const float *saved_dev, int64_t ldsv,
                        const float *gamma_dev, const float *gx_dev, int64_t ldg, float *gz_dev, int64_t ldgz,
                        float *d_gamma_dev, float *d_beta_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (12) Counter-based dropout (csrc/dropout.hip): the keep bit of an element is a pure function of the seed, the
 * step, the site, the GLOBAL row (an entity id, or a batch row in the trunk) and the column, so a mask does not depend on the
 * launch geometry, on the rank count or on which rank owns the row; the backward recomputes it instead of loading a saved mask.
 *
 * The bit definition. Let sm(x) be one SplitMix64 step (^ is XOR, >> an unsigned shift, all arithmetic mod 2^64):
 *     x += 0x9E3779B97F4A7C15
 *     z = x
 *     z = (z ^ z>>30) * 0xBF58476D1CE4E5B9
 *     z = (z ^ z>>27) * 0x94D049BB133111EB
 *     return z ^ z>>31
 * Then:
 *   - key(seed, step, site) = sm(sm(sm(seed) ^ step) ^ site). The host computes it once per call and passes it by value as a
 *     64-bit kernel argument.
 *   - Words = Philox4x32-10 (the generator of the Random123 library), using that library's standard constants. The multipliers
 *     are 0xD2511F53 and 0xCD9E8D57. The key increments are 0x9E3779B9 and 0xBB67AE85.
 *       Key words are (key & 0xffffffff, key >> 32).
 *       The counter is (row_lo, row_hi, col >> 2, 0), where row is the 64-bit global row row0 + r.
 *       Element (row, col) uses output word col & 3.
 *   - An element is kept iff word < T, where T = min(2^32 - 1, floor((1 - p) * 2^32)), computed in Python doubles.
 *     inv_keep = 1 / (1 - p) is passed as an f32.
 *   - A kept element becomes x * inv_keep (one f32 multiply). A dropped element becomes +0.0f whatever x holds. The backward is
 *     the same operation applied to the gradient.
 *   - Sites with p <= 0 launch nothing. Sites with p >= 1 produce zeros (T = 0 keeps nothing; the caller passes inv_keep = 0).
 *   - Site ids: layer li: 4 li + 0 (in), 4 li + 1 (out), 4 li + 2 (gcn_drop); trunk: 0x1000 (feature, row = batch row, flat_sz
 *     columns) and 0x1001 (hidden, O columns).
 *
 * mgcn_dropout_apply: out [rows, cols] (rows ldo floats apart) = dropout of x [rows, cols] (rows ldx apart) under `key`, row r of
 *   the block being global row row0 + r. out may be x itself (same pointer, same leading dimension); any other overlap is the
 *   caller's error. Columns cols .. ld of a padded row are not touched.
 * mgcn_dropout_apply_pair: the same for two sites over one block in one launch -- the layer's in / out pair: out_a from x_a under
 *   key_a, out_b from x_b under key_b, one row0, threshold and inv_keep. x_a and x_b may be one matrix (the backward reads the
 *   incoming gradient once); each output may be either input as the same matrix; the two outputs are distinct.
 * mgcn_dropout_mask: the keep bytes (1 / 0) [rows, cols], rows ldm bytes apart: the bool masks (9) and (11) take.
 * mgcn_dropout_mask_host: the same bytes on the CPU from the SAME inline function the kernels call. Test infrastructure, like
 *   mgcn_csr_build_host's role for the layout; no model path calls it.
 * mgcn_dropout_apply_dev, mgcn_dropout_apply_pair_dev, mgcn_dropout_mask_dev: the three device entry points above with the last
 *   SplitMix64 step moved into the kernel: in place of each `key` they take the 64-bit site id, and step_key_dev points to ONE
 *   64-bit word in device memory (8-byte aligned) that holds sm(sm(seed) ^ step); every lane forms key = sm(word ^ site). One
 *   word serves all sites of a step. With the word of (seed, step) in memory every output bit equals the by-value entry point
 *   called with key(seed, step, site). For launches captured into a hipGraph: the host rewrites the word ahead of each replay.
 *   MGCN_EINVAL for a NULL or misaligned step_key_dev; everything else as the by-value forms.
 * One lane serves four columns with one Philox call; 16-byte accesses when every base pointer is 16-byte aligned and every leading
 * dimension a multiple of 4 (mask: 4-byte stores under the same rule for 4 bytes), the element-wise path with the same bits
 * otherwise. At most 2048 workgroups of 256 threads stride over the block; index arithmetic is 64-bit; no atomics, no LDS.
 * MGCN_EINVAL, nothing launched: a null pointer, rows < 0 or > 2^40, cols < 1, a leading dimension below cols, rows x ld above
 * 2^60, an inv_keep that is negative or not finite, an output aliasing an input with another leading dimension, out_a == out_b.
 * rows == 0 launches nothing.
 */
int mgcn_dropout_apply(int64_t rows, int32_t cols, const float *x_dev, int64_t ldx, float *out_dev, int64_t ldo, uint64_t key,
                       uint64_t row0, uint32_t threshold, float inv_keep, void *stream);
int mgcn_dropout_apply_pair(int64_t rows, int32_t cols, const float *xa_dev, int64_t ldxa, float *outa_dev, int64_t ldoa,
                            uint64_t key_a, const float *xb_dev, int64_t ldxb, float *outb_dev, int64_t ldob, uint64_t key_b,
                            uint64_t row0, uint32_t threshold, float inv_keep, void *stream);
int mgcn_dropout_mask(int64_t rows, int32_t cols, uint8_t *mask_dev, int64_t ldm, uint64_t key, uint64_t row0, uint32_t threshold,
                      void *stream);
int mgcn_dropout_apply_dev(int64_t rows, int32_t cols, const float *x_dev, int64_t ldx, float *out_dev, int64_t ldo,
                           const uint64_t *step_key_dev, uint64_t site, uint64_t row0, uint32_t threshold, float inv_keep, void *stream);
int mgcn_dropout_apply_pair_dev(int64_t rows, int32_t cols, const float *xa_dev, int64_t ldxa, float *outa_dev, int64_t ldoa,
                                uint64_t site_a, const float *xb_dev, int64_t ldxb, float *outb_dev, int64_t ldob, uint64_t site_b,
                                const uint64_t *step_key_dev, uint64_t row0, uint32_t threshold, float inv_keep, void *stream);
int mgcn_dropout_mask_dev(int64_t rows, int32_t cols, uint8_t *mask_dev, int64_t ldm, const uint64_t *step_key_dev, uint64_t site,
                          uint64_t row0, uint32_t threshold, void *stream);
int mgcn_dropout_mask_host(int64_t rows, int32_t cols, uint8_t *mask_host, int64_t ldm, uint64_t key, uint64_t row0,
                           uint32_t threshold);

/* ---------------------------------------------------------------------------------------------
 * (13) Scores of per-query candidate lists (csrc/dense.hip) — additive, MGCN_ABI_VERSION stays 4. What (5)
 * answers for the whole table, answered for the entities a caller names: the score of a triple, a short list to re-rank,
 * sampled negatives, the ids (7) returned. For query b and list position j, with id = cand[b * ldc + j] and o = id - ent_row0:
 *   0 <= o < n_local   out[b * ldo + j] = sigmoid(ent[o,:] . x[b,:] + bias[o]); with mask_dev given (the bit-packed rows of
 *                      mgcn_filter_mask for the same shard: bit (o & 31) of mask[b, o >> 5], ldm words per row, the layout
 *                      and the ent_row0 of (7)) a candidate whose bit is set gets -inf instead;
 *   any other id       the element of out is LEFT AS IT IS: -1 padding, an id of another shard, any int64 value, negative
 *                      or huge. No value of cand makes the launch read ent, bias or mask outside the shard (the test is one
 *                      unsigned comparison of id - ent_row0 against n_local before any of the three is addressed).
 * Duplicate ids in a row are allowed, each occurrence gets the score. Callers that want (7)'s padding convention pre-fill
 * out with -inf; shards then write disjoint elements of one block (launch per shard, or all-reduce MAX across ranks).
 * CONTRACT: the score is the f32 value mgcn_score_fwd produces for the same (x, ent, bias), bit for bit, hence also the
 * value of mgcn_score_target / mgcn_score_rank / mgcn_score_topk. The arithmetic family is chosen as in (5), by dim and by the
 * alignment and leading dimensions of x and ent alone (never by cand, out, n_cand or batch): 16-byte aligned operands with
 * dim % 4 == 0 and dim <= 352 take the six-product bf16 split in (5)'s product order per 32-wide k-block, everything else
 * the exact-f32 MFMA's k-ordered chain (operands that are not 16-byte aligned or dim % 4 != 0: element-wise guarded loads,
 * the same summation order).
 * Launch: one workgroup of four waves per (query, 64 list positions), grid-stride; a wave's MFMA tile is 16 gathered
 * candidate rows of its query, each row fetched once, the next k-block's loads in flight; no atomics, no workspace.
 * MGCN_EINVAL, nothing launched: a null x / ent / bias / cand / out, ldc < n_cand, ldo < n_cand, ldx < dim, lde < dim,
 * ent_row0 < 0, a negative size, dim < 1, batch / n_cand / n_local at or above 2^31 - 64, mask_dev given with
 * ldm < ceil(n_local / 32). batch == 0, n_cand == 0 or n_local == 0 return MGCN_OK without a launch.
 */
int mgcn_score_candidates(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *x_dev,
                          int64_t ldx, const float *ent_dev, int64_t lde, const float *bias_dev, const int64_t *cand_dev,
                          int64_t ldc, const uint32_t *mask_dev, int64_t ldm, float *out_dev, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (14) Training on per-query candidate lists (csrc/dense.hip: labels and forward; csrc/query_train.hip: backward; DESIGN
 * §4.11) — additive, MGCN_ABI_VERSION stays 4. The mean BCE of (6) over the lists of (13) instead of the table: the true tails
 * plus sampled negatives. Nothing here has a [B, N] or [B, N/32] operand; the work is B n_cand dim. No float atomics, every sum
 * has a fixed order: the same inputs give the same bits.
 * Liveness is that of (13): with id = cand[b * ldc + j] and d = uint64(id) - uint64(ent_row0), position (b, j) is LIVE iff
 * d < n_local, its shard row is o = d. One unsigned comparison, made before any address of ent, bias, d_ent or d_bias is formed:
 * -1, another shard's id, +-2^62 are DEAD and load nothing.
 *
 * mgcn_cand_labels: label[b * ldl + j] (uint8) = 1 iff position (b, j) is live and cand[b, j] is among the known tails of
 *   qkey[b] in the keys / ptr / tails arrays of mgcn_filter_mask (tails ascending within a key), else 0. The key lookup of
 *   mgcn_filter_mask, then a binary search in the key's run. One launch, integers only.
 * mgcn_cand_bce_partials(batch, n_cand) = batch * ceil(n_cand / 64), the length of loss_partial.
 * mgcn_cand_bce_fwd: one launch with the geometry of (13) (a workgroup of four waves per (query, 64 list positions),
 *   grid-stride, a wave's tile 16 gathered rows). For a live (b, j): z = the exact-f32 MFMA's k-ordered chain of (13) -- ALWAYS
 *   that family, never the six-product split, because mgcn_score_bce_fwd always takes it --, p = sigmoid(z + bias[o]),
 *   y = label[b, j] ? hot : cold, and
 *     g[b * ldg + j] = (p - y) / max(p (1 - p), 1e-12) * p (1 - p) * inv_count
 *   with the term (y - 1) max(log1p(-p), -100) - y max(log(p), -100) added to the unit's partial. A dead position writes
 *   g = 0 and adds no term, so g [batch, n_cand] is written completely. loss_partial[b * chunks + ch] is the sum of the unit's
 *   terms in a fixed order (lanes: xor tree; then the four waves in wave order), a function of its own (query, chunk) and of
 *   nothing else in the launch; the loss is the sum of the partials times inv_count.
 *   CONTRACT: for a live position, g[b, j] has the bits of grad_logit[o, b] of mgcn_score_bce_fwd for the same x, ent, bias, hot,
 *   cold, inv_count and a mask whose bit o of row b equals label[b, j] (operands that entry point takes: 16-byte aligned,
 *   dim % 4 == 0, batch % 4 == 0). Other operands take element-wise guarded loads and the same summation order.
 * mgcn_cand_bce_bwd_x: dx [batch, dim] (rows ldx apart), written completely:
 *     dx[b, c] = 0;  for ch = 0 .. chunks - 1:  s = 0;  for the LIVE j of [64 ch, min(64 ch + 64, n_cand)) ascending:
 *     s = s + (g[b, j] * ent[o_j, c]);  then dx[b, c] = dx[b, c] + s
 *   every product and every sum rounded to f32 (no contraction). The order depends on n_cand alone.
 * mgcn_cand_bce_bwd_ent: the caller supplies a plan perm [batch * n_cand] int64: the flat positions b * n_cand + j of the live
 *   entries ordered by (shard row, flat position), then the dead ones; n_live is the length of the live prefix (only the prefix
 *   is read). The kernel recomputes the row of every perm[i] it meets from cand with the liveness test and follows nothing it
 *   has not checked: a perm[i] outside [0, batch * n_cand) or a dead one inside the prefix is skipped and ends the run before
 *   it. A run is a maximal stretch of plan entries with equal rows; the wave of a run's first entry owns it, every other wave
 *   exits. The owner walks the run in plan order and writes
 *     d_ent[o * lde + c] = sum of (g[pos] * x[b(pos), c]),   d_bias[o] = sum of g[pos]
 *   each the sequential f32 loop from 0, products and sums rounded separately. Rows that no live position names are LEFT AS THEY
 *   ARE (the caller zero-fills: the convention of (13)). Either of d_ent_dev / d_bias_dev may be NULL, which only removes work
 *   (with d_ent_dev NULL, x_dev / ldx / lde are not looked at).
 *   A RUN IS WALKED BY ONE WAVE, HOWEVER LONG IT IS: a list in which every query names the same entity is a chain of batch
 *   addends per column on one wave (measured: tools/bench_cand_train.py). With a plan that is not sorted as described, a row
 *   whose entries are not adjacent has several owners and receives the sum of one of its stretches; nothing outside the rows
 *   that live positions name is ever written.
 * All checks precede the first launch; a refusal writes nothing. MGCN_EINVAL: a null required pointer, a negative size, dim < 1,
 * ent_row0 < 0, batch / n_cand / n_local at or above 2^31 - 64, ldc / ldl / ldg < n_cand, ldx / lde < dim, n_live outside
 * [0, batch * n_cand]. batch == 0, n_cand == 0 or n_local == 0 (bwd_ent: also n_live == 0, or both outputs NULL) return MGCN_OK
 * without a launch and write nothing.
 */
int mgcn_cand_labels(int32_t batch, int64_t n_cand, const int64_t *qkey_dev, int64_t num_keys, const int64_t *keys_dev,
                     const int64_t *ptr_dev, const int32_t *tails_dev, int64_t ent_row0, int64_t n_local, const int64_t *cand_dev,
                     int64_t ldc, uint8_t *label_dev, int64_t ldl, void *stream);
int64_t mgcn_cand_bce_partials(int32_t batch, int64_t n_cand);
int mgcn_cand_bce_fwd(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *x_dev,
                      int64_t ldx, const float *ent_dev, int64_t lde, const float *bias_dev, const int64_t *cand_dev, int64_t ldc,
                      const uint8_t *label_dev, int64_t ldl, float hot, float cold, float inv_count, float *g_dev, int64_t ldg,
                      float *loss_partial_dev, void *stream);
int mgcn_cand_bce_bwd_x(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *g_dev,
                        int64_t ldg, const int64_t *cand_dev, int64_t ldc, const float *ent_dev, int64_t lde, float *dx_dev,
                        int64_t ldx, void *stream);
int mgcn_cand_bce_bwd_ent(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *g_dev,
                          int64_t ldg, const int64_t *cand_dev, int64_t ldc, const int64_t *perm_dev, int64_t n_live,
                          const float *x_dev, int64_t ldx, float *d_ent_dev, int64_t lde, float *d_bias_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (15) Counter-drawn candidate lists (csrc/dropout.hip, next to the Philox function it calls) — additive,
 * MGCN_ABI_VERSION stays 4. The lists (14) trains on, one known tail plus sampled negatives per query, as a pure function of
 * (seed, step, global batch row, list position) and of the index: every rank of a sharded step draws the same [B, K] block
 * without an exchange, and a checkpoint restores the stream from (seed, step count). Integers only, so the bits are exact.
 *
 *   - key = sm(sm(sm(seed) ^ step) ^ site) of (12) with the site id 0x2000; the host forms it and passes it by value
 *     (mgcn_cand_draw), or the lanes form its last step from a word in device memory (mgcn_cand_draw_dev, below).
 *   - For list position (b, j), with the 64-bit global batch row row = row0 + b: the words w0..w3 are Philox4x32-10 of (12) with
 *     key words (key & 0xffffffff, key >> 32) and counter (row_lo, row_hi, j >> 1, 0); r = w0 | w1 << 32 for even j,
 *     r = w2 | w3 << 32 for odd j. One Philox call serves two positions.
 *   - j >= 1 (negatives): cand[b * ldc + j] = (r * num_entities) >> 64, the high half of the 128-bit product: an id in
 *     [0, num_entities).
 *   - j == 0 (one known tail): qkey[b] is looked up in keys (the lookup of mgcn_filter_mask); with its run [lo, hi) =
 *     [ptr[i], ptr[i + 1]): cand[b * ldc] = tails[lo + ((r * (hi - lo)) >> 64)]. It is -1 when the key is absent or the run is
 *     empty, reversed or not inside [0, n_tails]: the kernel follows nothing it has not checked. -1 is a dead position of (14):
 *     it contributes zero and counts in the divisor.
 *   - label_dev (optional) [batch, n_cand] uint8, rows ldl bytes apart: 1 iff 0 <= id < num_entities and the id is found in the
 *     query's run by mgcn_cand_labels' binary search (the run the thread already holds; no run: 0), else 0. For an index whose
 *     runs are ascending with tails in [0, num_entities), column 0 is therefore 1 wherever it is not -1, and the block equals
 *     mgcn_cand_labels(..., ent_row0 = 0, n_local = num_entities) of the drawn list bit for bit: the GLOBAL label, valid on any
 *     shard because mgcn_cand_bce_fwd never reads the label of a dead position. label_dev == NULL removes only that work.
 *
 * mgcn_cand_draw: one launch, at most 2048 workgroups of 256 threads grid-striding over (b, j >> 1); no LDS, no atomics, 64-bit
 *   index arithmetic. Columns n_cand .. ldc of a padded row are not touched. ptr holds num_keys + 1 entries, tails n_tails.
 * mgcn_cand_draw_dev: mgcn_cand_draw with the key read from device memory, as the _dev forms of (12): step_key_dev points at ONE
 *   64-bit word in device memory that holds sm(sm(seed) ^ step), `site` is the site id (0x2000), and every thread forms
 *   key = sm(*step_key_dev ^ site) once, ahead of its grid-stride loop, and hands it to the same inline function. The word is read
 *   when the kernel RUNS, not when it is enqueued: a launch captured into a hipGraph draws, on every replay, the lists of the word
 *   it finds (captured.CapturedCandidateStep writes the word ahead of each replay). Same geometry, same checks, same bits as
 *   mgcn_cand_draw under the key of that word. A null step_key_dev, or one not aligned to 8 bytes, is MGCN_EINVAL before any other
 *   check and at batch == 0 too.
 * mgcn_cand_draw_host: the same block on the CPU over host pointers, from the SAME inline function the kernel calls: test
 *   infrastructure, the role mgcn_dropout_mask_host plays in (12).
 * MGCN_EINVAL, nothing launched and nothing written (all checks precede the first HIP call): a null qkey / ptr / cand, a null
 * keys with num_keys > 0 or a null tails with n_tails > 0; batch < 0, n_cand < 1, num_keys < 0, n_tails < 0; num_entities outside
 * [1, 2^40]; batch or n_cand at or above 2^31 - 64; ldc < n_cand, or ldl < n_cand when labels are asked for; batch x leading
 * dimension above 2^60. batch == 0 launches nothing.
 */
int mgcn_cand_draw(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                   const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails, uint64_t key,
                   uint64_t row0, int64_t *cand_dev, int64_t ldc, uint8_t *label_dev, int64_t ldl, void *stream);
int mgcn_cand_draw_dev(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                       const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails,
                       const uint64_t *step_key_dev, uint64_t site, uint64_t row0, int64_t *cand_dev, int64_t ldc, uint8_t *label_dev,
                       int64_t ldl, void *stream);
int mgcn_cand_draw_host(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_host, int64_t num_keys,
                        const int64_t *keys_host, const int64_t *ptr_host, const int32_t *tails_host, int64_t n_tails, uint64_t key,
                        uint64_t row0, int64_t *cand_host, int64_t ldc, uint8_t *label_host, int64_t ldl);

/* ---------------------------------------------------------------------------------------------
 * (16) Softmax cross-entropy over per-query candidate lists (csrc/dense.hip) — additive, MGCN_ABI_VERSION stays 4.
 * The listwise loss (sampled softmax) next to the BCE of (14): the candidates of a query compete, the smoothing is over the list
 * and not over the table. The forward is three kinds of launch, logits -> merge -> finish; the backward is (14)'s
 * mgcn_cand_bce_bwd_x / mgcn_cand_bce_bwd_ent on the g this block leaves, unchanged. Nothing has a [B, N] operand or a workspace
 * of size N, there are no float atomics, every sum has a fixed order: the same inputs give the same bits. No host read.
 * Liveness is that of (13) / (14): with id = cand[b * ldc + j] and d = uint64(id) - uint64(ent_row0), position (b, j) is LIVE iff
 * d < n_local, its shard row is o = d; the one unsigned comparison is made before any address of ent or bias is formed, and a
 * dead position's label is not read. -1, another shard's id, +-2^62 are DEAD.
 *
 * The loss. z[b, j] = ent[o,:] . x[b,:] + bias[o] for a live position. Per row b, over the live positions OF ALL SHARDS:
 *   M = max z,  S = sum exp(z - M),  n_live = their number,  n_pos = the number of them with label != 0.
 *   q[b, j] = (1 - eps) label[b, j] / n_pos + eps / n_live   (eps = lbl_smooth: several known tails of one list share the mass,
 *             duplicates are separate positions, the smoothing mass is spread over the LIST)
 *   lp = (z - M) - log S,  p = exp(lp),  g[b, j] = (p - q) inv_batch,  the position's term is -(q lp);
 *   loss = inv_batch * the sum of all terms (inv_batch = 1 / B for the mean over queries).
 * A dead position has g = 0 and no term. A row with n_pos == 0 (its column 0 is the -1 of mgcn_cand_draw, or nothing of it is
 * live anywhere) has g = 0 everywhere and no term; it still counts in the divisor B: the convention of (14).
 * The loss is a sum of per-position terms: with the GLOBAL statistics of a row in every shard's finish, the shards' losses add up
 * to the loss, the shards' g blocks are disjoint, d ent / d bias are local and complete, d x is a sum of partial sums.
 *
 * A STATISTIC is a record of four 32-bit words: m (f32), s (f32), n_live (int32), n_pos (int32); arrays of them are passed as
 * float pointers, record i at words 4 i .. 4 i + 3. The counts are integers, exact at every list length the entry points take.
 * The empty statistic is (-inf, 0, 0, 0).
 *
 * mgcn_cand_ce_partials(batch, n_cand) = batch * ceil(n_cand / 64): the number of units (query, chunk of 64 list positions), the
 *   records of stat_dev of mgcn_cand_ce_logits and the length of loss_partial of mgcn_cand_ce_finish.
 * mgcn_cand_ce_logits: one launch with the geometry of (13) (a workgroup of four waves per unit, grid-stride, a wave's tile 16
 *   gathered rows, each row fetched once). z is the exact-f32 MFMA's k-ordered chain of (13) plus bias[o] -- ALWAYS that family,
 *   never the six-product split: for a live position, z has the bits of the logit mgcn_cand_bce_fwd feeds its sigmoid
 *   (16-byte aligned operands with dim % 4 == 0: vector loads; anything else element-wise guarded loads, the same order).
 *   z[b * ldz + j] is written for every j < n_cand: the logit, or -inf at a dead position. Record b * chunks + ch of stat_dev is
 *   the unit's statistic: m = the maximum of its live z (-inf without one), s = the sum of exp(z - m) over its live positions
 *   (lanes: xor tree; then the four waves in wave order), the two counts. It is a function of the unit's own (query, chunk) and
 *   of nothing else in the launch.
 * mgcn_cand_ce_merge: out record r (r < batch) = the fold of the `parts` records in[r * row_stride + p * part_stride], p ascending
 *   (strides in records): M = max m_p; S = 0, then S = S + s_p * exp(m_p - M) for p = 0 .. parts - 1, skipping parts with
 *   m_p = -inf (a part with m_p == M takes the factor 1); the counts add (the caller's parts partition one list, so the sums
 *   stay at or below n_cand). parts == 1 copies the record: the identity on bits. A row without a live part gives
 *   (-inf, 0, 0, 0). Used twice: chunks -> row (parts = chunks, row_stride = chunks, part_stride = 1 on the records of
 *   mgcn_cand_ce_logits) and ranks -> global (the all-gathered [W, batch] blocks: parts = W, row_stride = 1,
 *   part_stride = batch). One thread per row. in and out must not be the same block.
 * mgcn_cand_ce_finish: element-wise over [batch, n_cand], a wave per unit: from z (read only where the position is live: liveness
 *   is recomputed from cand, never inferred from z), label, the row's statistic stat_dev[b] (batch records), lbl_smooth and
 *   inv_batch it writes g [batch, n_cand] COMPLETELY (0 at dead positions and in rows with n_pos == 0) and
 *   loss_partial[b * chunks + ch] = the sum of the unit's terms -(q lp), in the order mgcn_cand_bce_fwd adds its partials (within
 *   each sixteen positions the xor tree, then the four sixteens in order): a function of the unit's positions and of its row's
 *   statistic alone. The loss is inv_batch times the sum of the partials.
 * All checks precede the first launch; a refusal writes nothing. MGCN_EINVAL: a null pointer, a negative size, dim < 1,
 * ent_row0 < 0, batch / n_cand / n_local / parts at or above 2^31 - 64, ldc / ldl / ldz / ldg < n_cand, ldx / lde < dim,
 * lbl_smooth outside [0, 1]; merge: parts < 1, a stride < 1 or at or above 2^40, strides under which records of different (row,
 * part) coincide, in == out. batch == 0, n_cand == 0 or n_local == 0 (merge: batch == 0) return MGCN_OK without a launch and
 * write nothing: a rank without entity rows holds z = -inf, the empty statistic and g = 0 by the caller's fill.
 * Domain: finite logits. NOT MEASURED: the kernels' own times (DESIGN §4.13 has the stage's time around device events).
 */
int64_t mgcn_cand_ce_partials(int32_t batch, int64_t n_cand);
int mgcn_cand_ce_logits(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *x_dev,
                        int64_t ldx, const float *ent_dev, int64_t lde, const float *bias_dev, const int64_t *cand_dev, int64_t ldc,
                        const uint8_t *label_dev, int64_t ldl, float *z_dev, int64_t ldz, float *stat_dev, void *stream);
int mgcn_cand_ce_merge(int32_t batch, int64_t parts, const float *stat_in_dev, int64_t row_stride, int64_t part_stride,
                       float *stat_out_dev, void *stream);
int mgcn_cand_ce_finish(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, const float *z_dev, int64_t ldz,
                        const int64_t *cand_dev, int64_t ldc, const uint8_t *label_dev, int64_t ldl, const float *stat_dev,
                        float lbl_smooth, float inv_batch, float *g_dev, int64_t ldg, float *loss_partial_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (17) Weighted candidate lists: negatives drawn by entity weight through an alias table (csrc/csr_build.cpp builds the table,
 * csrc/dropout.hip draws) — additive, MGCN_ABI_VERSION stays 4. The draw of (15) with one more operand: the key,
 * the Philox counter layout (one call per two positions), column 0 (the known tail), the optional labels and every check are
 * those of (15); only the id of a negative changes. Integers only: a pure function of (seed, step, global batch row, list
 * position), of the index and of the table; the same bits on any rank, at any launch geometry, eager or replayed.
 *
 * THE TABLE. table[n] (n < num_entities) is one int64 word, alias[n] << 32 | thr[n]: thr a 32-bit threshold, alias in
 * [0, num_entities). mgcn_alias_build_host builds it on the CPU from int64 weights w[n] in [0, 2^32), W = sum w >= 1, by Vose's
 * method on the integers m[n] = w[n] * num_entities compared against W (64-bit; the threshold's product is 128-bit; no floating
 * point anywhere):
 *   - an entry with m == W is finished: thr = 0xffffffff, alias = n (both branches of the draw return n);
 *   - the smalls (m < W) wait in a FIFO that starts as their ascending ids; the larges (m > W) are taken in ascending id;
 *   - the small s at the head of the FIFO gets thr[s] = floor(m[s] * 2^32 / W) and alias[s] = L, the current large, which loses
 *     exactly W - m[s]; if that leaves m[L] == W it is finished as above, if it leaves m[L] < W it joins the BACK of the FIFO;
 *     in both cases the next large in ascending id becomes current. Sums are exact, so the FIFO and the larges run out together.
 *   The table realises cnt[n] = thr[n] + the sum of (2^32 - thr[m]) over every m with alias[m] == n (m == n included), and
 *   Q(n) = cnt[n] / (num_entities * 2^32), an exact rational: sum cnt = num_entities * 2^32, w[n] == 0 gives cnt[n] == 0, and
 *   |cnt[n] W - w[n] num_entities 2^32| <= (1 + indeg[n]) W. Equal weights give n << 32 | 0xffffffff.
 *   MGCN_EINVAL, nothing written: a null pointer, num_entities outside [1, 2^31 - 1], a weight outside [0, 2^32), W == 0.
 *
 * THE DRAW. For j >= 1, with the r of (15): slot = (r * num_entities) >> 64, the high half of the 128-bit product; u = the upper
 * 32 bits of the LOW half of the same product (the position inside the slot: no second random word is spent); t = table[slot],
 * one 8-byte load; id = u < uint32(t) ? slot : uint64(t) >> 32; an alias at or above num_entities is written as -1 (a dead
 * position of (14) / (16)). slot < num_entities always and the alias is compared before it is written: a corrupt table yields
 * dead positions downstream, never an address. With the equal-weights table the block is that of mgcn_cand_draw, bit for bit.
 * mgcn_cand_draw_alias / _dev / _host are mgcn_cand_draw / _dev / _host with table [num_entities] after n_tails: the same grid
 * rule (at most 2048 workgroups of 256 threads over (b, j >> 1)), no LDS, no atomics, plain vector stores; n_cand == 1 never
 * reads the table. MGCN_EINVAL on top of (15)'s cases, nothing launched and nothing written: a null table, a table not aligned
 * to 8 bytes, num_entities > 2^31 - 1. NOT MEASURED: the kernel's own time (DESIGN §4.15 times the call).
 */
int mgcn_alias_build_host(int64_t num_entities, const int64_t *w_host, int64_t *table_host);
int mgcn_cand_draw_alias(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                         const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails,
                         const int64_t *table_dev, uint64_t key, uint64_t row0, int64_t *cand_dev, int64_t ldc, uint8_t *label_dev,
                         int64_t ldl, void *stream);
int mgcn_cand_draw_alias_dev(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                             const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails,
                             const int64_t *table_dev, const uint64_t *step_key_dev, uint64_t site, uint64_t row0, int64_t *cand_dev,
                             int64_t ldc, uint8_t *label_dev, int64_t ldl, void *stream);
int mgcn_cand_draw_alias_host(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_host, int64_t num_keys,
                              const int64_t *keys_host, const int64_t *ptr_host, const int32_t *tails_host, int64_t n_tails,
                              const int64_t *table_host, uint64_t key, uint64_t row0, int64_t *cand_host, int64_t ldc,
                              uint8_t *label_host, int64_t ldl);

/* ---------------------------------------------------------------------------------------------
 * (18) The list backward with long runs split across waves, in a fixed order (csrc/query_train.hip) — additive,
 * MGCN_ABI_VERSION stays 4. mgcn_cand_bce_bwd_ent of (14) walks a run of plan entries that name one entity with one wave however
 * long it is; on weighted lists a hub entity is named thousands of times. mgcn_cand_bce_bwd_ent_split takes that call's
 * arguments, with the same meaning, checks and optionality (d_ent_dev NULL: bias only), plus
 *   keys_dev [batch * n_cand] int64: the ascending sort keys row * (batch * n_cand) + position the plan perm was sorted by (dead
 *     entries: row = n_local), i.e. keys_dev[i] is the key of perm_dev[i]; run_split = S in [16, 65536]; a workspace of at least
 *     mgcn_cand_bwd_ent_split_workspace bytes, 16-byte aligned, which the call may overwrite completely and reads nothing from
 *     that it has not written itself.
 * THE ORDER (the contract). A run is a maximal stretch of plan entries e_0 .. e_{L-1} with one live row o, as in (14). Piece p
 * holds e_{pS} .. e_{min((p+1)S, L)-1}: the cuts are counted from the run's OWN first entry, not from the plan's. A piece's
 * partial is (14)'s loop over its entries: the sequential f32 sum from +0 of the rounded products g[pos] * x[b(pos), c] (for
 * d_bias: of g[pos]) in plan order. d_ent[o, c] and d_bias[o] are the sequential f32 sum from +0 of the pieces' partials in piece
 * order. Hence a run with L <= S has the bits mgcn_cand_bce_bwd_ent gives it (0 + a = a, and a sum from +0 is never -0), and a
 * row's result depends only on the positions that name it and on S: not on the other ids of the list, on ent_row0 / n_local,
 * on the grid or on scheduling, so a shard's rows equal the same rows of the one-rank call bit for bit. Rows that no live position
 * names are LEFT AS THEY ARE. The dependent chain of a row is S + ceil(L / S) additions instead of L.
 * THE LAUNCHES, all enqueued by the one call (no host read, no allocation, no atomics of any kind, plain vector stores; it may
 * be captured): (a) one thread per plan entry i finds its run's first entry s, the lowest index with keys_dev[s] >=
 * row_i * (batch * n_cand), by galloping backwards from i and bisecting inside [0, i], and marks i as a piece head iff
 * (i - s) % S == 0; (b) one wave per plan entry, a head walks its at most S entries and writes either the row (the run's only
 * piece) or a workspace slot of dim + 1 floats; (c) one wave per window of S plan entries adds the slots of the run of several
 * pieces that begins in that window, if there is one (two cannot: they would be more than S entries apart).
 * SLOTS: head i of a run of several pieces writes slot 2 * (i / S) + (1 if it is the run's first head else 0). Two heads of one
 * run are S apart, so they lie in different windows i / S; two runs with a head in one window are adjacent in the plan, the
 * earlier one's head there is not its first and the later one's is. So no two heads share a slot and 2 * ceil(batch * n_cand / S)
 * slots suffice: the workspace is these slots, one int64 per window (written by one thread each) and one byte per plan entry.
 * keys_dev is only ever COMPARED: the row, the query and every address of g / x / d_ent / d_bias come from cand through the
 * liveness test as in (14), a slot index from the entry's own index i < n_live. Keys that are not the plan's can give wrong sums
 * in the rows the lists name and nothing else.
 * MGCN_EINVAL on top of (14)'s cases, nothing launched and nothing written: a null keys_dev, run_split outside [16, 65536], a
 * null or misaligned workspace or one smaller than mgcn_cand_bwd_ent_split_workspace says, (n_local + 1) * batch * n_cand
 * not below 2^63. mgcn_cand_bwd_ent_split_workspace returns 0 for sizes or a run_split the call refuses.
 * NOT MEASURED: the three kernels' own times (DESIGN §4.16 times the stage).
 */
size_t mgcn_cand_bwd_ent_split_workspace(int32_t batch, int64_t n_cand, int32_t dim, int32_t run_split);
int mgcn_cand_bce_bwd_ent_split(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *g_dev,
                                int64_t ldg, const int64_t *cand_dev, int64_t ldc, const int64_t *perm_dev, int64_t n_live,
                                const float *x_dev, int64_t ldx, float *d_ent_dev, int64_t lde, float *d_bias_dev,
                                const int64_t *keys_dev, int32_t run_split, void *ws_dev, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (19) Edge dropout and own-triple removal: this step's graph as a copy of the slot records (csrc/dropout.hip, the table in
 * csrc/csr_build.cpp) — additive, MGCN_ABI_VERSION stays 4. Every aggregation kernel of (2), (3), (3s) and (4) takes
 * a slot's norm from its record and nothing else, and a slot with norm +0.0f contributes nothing (1v). So a training step that
 * drops edges needs no new layout: it needs rec' [2E], the records with the norms of the kept edge list, which the layers are
 * handed in place of rec. rowptr, slot_dst, mirror, the type lists and the hub chunks stay as (1) built them.
 * THE DEFINITION. E = num_edges_half. Directed edge d in [0, 2E) has the undirected id u = d mod E: an edge and its reverse live
 * and die together. keep(u) is element (row u, column 0) of the mask of (12) under `key` and `threshold`, i.e. byte u of
 * mgcn_dropout_mask_host with rows = E, cols = 1, row0 = 0 (callers use key(seed, step, site 0x3000) and T(p); at p = 0 that is
 * T = 2^32 - 1, so a word of 0xffffffff still drops its edge). forced [E] uint8, optional: kept(u) = keep(u) && !forced[u].
 * For node n and half h, deg_h[n] is the number of kept slots in the destination run of n in half 1 - h — the non-hub run of
 * rowptr, or the hub's segment chunks[first].begin .. chunks[first + count - 1].end — which by mirror symmetry is the kept
 * out-degree of n in half h, the by-SOURCE degree (Q2) of the kept list. Integer counts: no order, no atomics. T[d] is
 * mgcn_edge_drop_table_host's table, the feeder's own expression d ? 1.0f / sqrt(float(d)) : 0.0f evaluated on the host; the
 * device only looks values up. For slot p in half h with source s and destination n:
 *   rec'[p] = {src, type, kept(eid_p mod E) ? T[deg_h[s]] * T[deg_h[n]] : +0.0f, eid},   one f32 multiply, as in the feeder,
 * so a kept slot carries, bit for bit, the norm mgcn_csr_build_host folds for that edge when it is run on the kept edge list alone.
 * An eid outside [0, 2E) or a src / destination outside [0, N) gives norm +0.0f and addresses nothing.
 * The graph must be mirror-symmetric and carry the backward index (slot_dst): callers refuse other graphs (the Python seam raises).
 *   table_dev [table_len] f32 with table_len > max_run, max_run = the longest destination run in either half (hub segments
 *   included); a count at or above table_len (a max_run that was not the graph's) reads nothing and gives 0.
 *   cinv_dev [2, N] f32: workspace, written by the call (T[deg_h[n]]); rec_out_dev [2E]: 16-byte aligned, not rec_dev.
 * mgcn_edge_drop_records: two launches on `stream`, no host read, no allocation, no LDS, no atomics, plain vector stores; it may
 * be captured. (a) eight lanes per (half, node) walk the run, count the kept slots (an integer sum across the lanes) and store
 * T[count]; (b) one lane per slot writes its record with one 16-byte store. The bits do not depend on the grid. threshold = 0
 * (p >= 1): every norm is +0.0f. mgcn_edge_drop_records_dev: the same kernels, instantiated on the key source as (12)'s _dev
 * forms: `site` and the 8-byte aligned step word sm(sm(seed) ^ step) in device memory, read when the launch RUNS.
 * mgcn_edge_drop_records_host: the CPU twin from the same inline functions (test infrastructure); it measures max_run itself.
 * mgcn_edge_drop_table_host: T[0 .. len), len in [1, 2^31).
 * mgcn_edge_flags_from_queries: forced[u] = 1 for every directed edge whose key src * 2R + type equals a query key qkey[b]
 * (the keys of mgcn_filter_index_build), u its undirected id. ekeys_dev [2E] int64 ascending, eund_dev [2E] int32 the undirected
 * id of each sorted entry (an id outside [0, E) is skipped). One wave per query bisects ekeys (mgcn_filter_mask's idiom) and its
 * lanes walk the run of equal keys; racing stores write the same byte. The caller zero-fills forced first; bytes of edges that no
 * query names are left as they are.
 * MGCN_EINVAL, nothing launched and nothing written: a null pointer (forced may be NULL; hubinfo / chunks when num_chunks = 0),
 * a negative size, N, 2E or num_chunks outside int32 slots, records not 16-byte aligned, rec_out_dev == rec_dev, table_len <=
 * max_run, a null or misaligned step_key_dev.
 * NOT MEASURED: the kernels' own times (DESIGN §4.17 times the calls and the step).
 */
int mgcn_edge_drop_table_host(int64_t len, float *table_host);
int mgcn_edge_drop_records(int64_t num_nodes, int64_t num_edges_half, const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev,
                           const int32_t *slot_dst_dev, const int32_t *hubinfo_dev, const int32_t *chunks_dev, int64_t num_chunks,
                           const float *table_dev, int64_t table_len, int64_t max_run, const uint8_t *forced_dev, uint64_t key,
                           uint32_t threshold, float *cinv_dev, mgcn_edge_rec *rec_out_dev, void *stream);
int mgcn_edge_drop_records_dev(int64_t num_nodes, int64_t num_edges_half, const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev,
                               const int32_t *slot_dst_dev, const int32_t *hubinfo_dev, const int32_t *chunks_dev, int64_t num_chunks,
                               const float *table_dev, int64_t table_len, int64_t max_run, const uint8_t *forced_dev,
                               const uint64_t *step_key_dev, uint64_t site, uint32_t threshold, float *cinv_dev,
                               mgcn_edge_rec *rec_out_dev, void *stream);
int mgcn_edge_drop_records_host(int64_t num_nodes, int64_t num_edges_half, const int32_t *rowptr_host, const mgcn_edge_rec *rec_host,
                                const int32_t *slot_dst_host, const int32_t *hubinfo_host, const int32_t *chunks_host, int64_t num_chunks,
                                const float *table_host, int64_t table_len, const uint8_t *forced_host, uint64_t key,
                                uint32_t threshold, float *cinv_host, mgcn_edge_rec *rec_out_host);
int mgcn_edge_flags_from_queries(int32_t batch, const int64_t *qkey_dev, int64_t num_edges_half, const int64_t *ekeys_dev,
                                 const int32_t *eund_dev, uint8_t *forced_dev, void *stream);

/* ---------------------------------------------------------------------------------------------
 * (20) Softmax cross-entropy over the full entity table (csrc/dense.hip) — additive, MGCN_ABI_VERSION stays 4.
 * The listwise loss of (16) with "list position" replaced by "entity": the 1-vs-all softmax next to the BCE of (6). Every entity
 * is live. The forward is logits -> merge over tiles (mgcn_cand_ce_merge of (16), unchanged) -> finish; the backward is (6)'s three
 * products on the g this block leaves. No [B, N] label block, ONE [n_local, batch] block (z, overwritten by g), no float atomics,
 * every sum has a fixed order: the same inputs give the same bits. No host read.
 *
 * The loss. For query b and entity n of the GLOBAL table of N = num_entities entities: z[b, n] = x[b,:] . ent[n,:] + bias[n].
 * Per row b over ALL shards: M = max z, S = sum exp(z - M), n_pos = the number of set mask bits (the known tails of the query).
 *   q[b, n] = (1 - eps) y[b, n] / n_pos + eps / N      (eps = lbl_smooth; y = the mask bit; the smoothing mass is eps / N over
 *             the table, not (6)'s + 1 / N; eps / N is formed once on the host as float(eps) / float(N))
 *   lp = (z - M) - log S,  p = exp(lp),  g = (p - q) inv_batch,  the element's term is -(q lp);
 *   loss = inv_batch * the sum of all terms (inv_batch = 1 / B for the mean over queries).
 * A row with n_pos == 0 has g = 0 everywhere and no term; it still counts in the divisor B: the convention of (14) and (16).
 * With the GLOBAL statistics of a row in every shard's finish the shards' losses add up to the loss, the shards' g blocks are
 * disjoint, d ent / d bias are local and complete, d x is a sum of partial sums.
 *
 * A STATISTIC is (16)'s record (m, s, n_live, n_pos). z, like (6)'s grad_logit, is entity-major: element (n, b) at z[n * ldz + b].
 * mgcn_score_ce_tiles(n_local) = ceil(n_local / 32): the row tiles of a launch. mgcn_score_ce_partials(batch, n_local) =
 *   ceil(n_local / 32) * ceil(batch / 64): the length of loss_partial of mgcn_score_ce_finish.
 * mgcn_score_ce_logits: ONE launch of (6)'s tile kernel with another epilogue: same operands, same acceptance rule (16-byte
 *   aligned x / ent / z, ldx, lde, ldz, dim and batch multiples of 4, else MGCN_EUNSUPPORTED), ALWAYS the exact-f32 family,
 *   never the six-product split. z[n * ldz + b] has the bits of the logit mgcn_score_bce_fwd feeds its sigmoid, which are the
 *   bits of (16)'s z for the list that names entity n. Record t * lds + b of stat_dev (lds >= batch, in records; stat_dev 16-byte
 *   aligned, ceil(n_local / 32) * lds records) is the statistic of (row tile t of 32 entities, query b): m = the maximum of the
 *   tile's rows below n_local, s = the sum from 0 of exp(z - m) over those rows in row order (one thread per query: no lane or
 *   wave order enters), n_live = their number, n_pos = the popcount of the query's mask word t below n_live. A record is a
 *   function of its own tile and query and of nothing else in the launch. mgcn_cand_ce_merge(batch, parts = tiles, in = stat_dev,
 *   row_stride = 1, part_stride = lds) folds them tile by tile into the rows' [batch] records with coalesced reads; the same
 *   entry point folds the all-gathered [W, batch] blocks of the ranks (a rank without rows passes the empty statistic on).
 *   That fold is one thread per query walking every tile: with many tiles fold in two levels through the same strides (as
 *   _native.score_ce_fold does beyond 64 tiles): with G groups of P tiles, lds = batch and the records past `tiles` preset to the
 *   empty statistic, mgcn_cand_ce_merge(batch * G, parts = P, row_stride = 1, part_stride = G * batch) folds tiles g, g + G, ...
 *   into record g * batch + b, and mgcn_cand_ce_merge(batch, parts = G, row_stride = 1, part_stride = batch) folds the groups.
 * mgcn_score_ce_finish: element-wise and IN PLACE over z [n_local, batch], any batch and alignment, every access guarded: from z,
 *   the mask, the rows' GLOBAL statistics stat_dev [batch] (of which m, s and n_pos are read), lbl_smooth, inv_batch and
 *   num_entities it overwrites z with g and writes loss_partial[t * ceil(batch / 64) + qg] = the sum of the terms of (row tile t,
 *   queries 64 qg .. 64 qg + 63): a lane adds its query's eight rows in row order from 0, the 64 lanes fold by xor tree, the four
 *   waves follow in wave order. The loss is inv_batch times the sum of the partials.
 * All checks precede the first launch; a refusal writes nothing. MGCN_EINVAL: a null pointer, a negative size, dim < 1, batch /
 * n_local at or above 2^31 - 64, ldx / lde < dim, ldz / lds < batch, ldm < ceil(n_local / 32), lds at or above 2^40, a stat_dev of
 * mgcn_score_ce_logits that is not 16-byte aligned, lbl_smooth outside [0, 1], num_entities < max(n_local, 1). batch == 0 or
 * n_local == 0 return MGCN_OK without a launch and write nothing.
 * Domain: finite logits. NOT MEASURED: the kernels' own times (DESIGN §4.19 and profiles/bench_table_ce.json have the stage's time
 * around device events, Python's enqueueing included).
 */
int64_t mgcn_score_ce_tiles(int64_t n_local);
int64_t mgcn_score_ce_partials(int32_t batch, int64_t n_local);
int mgcn_score_ce_logits(int32_t batch, int64_t n_local, int32_t dim, const float *x_dev, int64_t ldx, const float *ent_dev,
                         int64_t lde, const float *bias_dev, const uint32_t *mask_dev, int64_t ldm, float *z_dev, int64_t ldz,
                         float *stat_dev, int64_t lds, void *stream);
int mgcn_score_ce_finish(int32_t batch, int64_t n_local, float *z_dev, int64_t ldz, const uint32_t *mask_dev, int64_t ldm,
                         const float *stat_dev, float lbl_smooth, float inv_batch, int64_t num_entities, float *loss_partial_dev,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MGCN_HIP_H */
