/*
 * nrk.h -- C ABI of libnrk.so, the MI355X-native recall + rank hot path.
 *
 * Every entry point:
 *   - takes caller-owned DEVICE buffers (plain pointers + sizes, row-major,
 *     contiguous) and an explicit HIP stream (hipStream_t passed as void*);
 *   - is asynchronous on that stream, performs no hidden allocation, no host
 *     synchronisation and no hipMalloc/hipMemcpy (graph-capturable); scratch
 *     comes from a caller workspace sized by the matching *_bytes() query;
 *   - returns NRK_OK (0) or an error code; nrk_last_error() gives a
 *     thread-local message.  No C++ exception crosses the ABI.
 *
 * The reference (qiqiqicheng/news-recommendation-tc) is pure Python with no
 * FFI of its own; each function below names the reference call site it
 * replaces (paths relative to the reference root).  The Python plugins in
 * news-recommendation-tc_amd/nrk bind these through ctypes; INTEGRATION.md
 * shows the binding a reference maintainer would add.
 */
#ifndef NRK_H
#define NRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nrk_stream_t; /* hipStream_t */

#define NRK_OK 0
#define NRK_EINVAL 1       /* bad argument (shape, null pointer, size)      */
#define NRK_EHIP 2         /* HIP runtime error (launch / device)           */
#define NRK_EUNSUPPORTED 3 /* configuration outside the compiled variants   */

const char* nrk_last_error(void);
/* ABI version 3 (round 5): the round-3 CSR owner protocol
 * (nrk_ip_topk_screen_range, nrk_ip_topk_band_pack, nrk_ip_topk_refine_csr)
 * is gone; config 4 runs shard_screen -> shard_band -> refine_x.
 * Version 2 (round 4): nrk_ip_topk_bound takes k before m (the screen's k, so
 * the bound pass knows the list length); the packed catalog carries a
 * half-block-major fp16 copy after its header (nrk_ip_catalog_bytes grew);
 * nrk_din_remap_index added; DIN item features 1, 2, 4 or 8.  A caller built
 * against an older version must be rebuilt. */
#define NRK_ABI_VERSION 3
int nrk_abi_version(void);

/* ---------------------------------------------------------------------- */
/* YouTubeDNN two-tower forward                                           */
/* ---------------------------------------------------------------------- */

/* User tower, eval mode.  Replaces YoutubeDNN.forward / get_user_embedding
 * (src/recall/youtubednn_recaller.py:129-182) as driven by
 * _extract_embeddings (:425-470), INCLUDING the host-side numpy
 * re-normalisation with zero-norm -> 1 (:467-470):
 *   x   = [E_u[uid] ; sum_{t<len} E_i[hist_t] / (len + 1e-8)]
 *   x   = ReLU(W1 ReLU(W0 x + b0) + b1)          (dropout = identity)
 *   out = renorm(x / max(||x||, 1e-12))
 * dim in {16, 32, 64}; h0 <= 128; h1 == dim.  hist is [n, seq_len]. */
int nrk_tt_user_fwd(const float* user_table, int64_t n_user_rows, const float* item_table,
                    int64_t n_item_rows, int dim, const int32_t* uid, const int32_t* hist,
                    const int32_t* hist_len, int64_t n, int seq_len, const float* w0,
                    const float* b0, int h0, const float* w1, const float* b1, int h1,
                    float* out, nrk_stream_t stream);

/* Users that one wave pass of nrk_tt_user_fwd's kernel handles together at
 * (dim, h0): 4 with h0 <= 64, and 0 where the one-user-per-wave kernel runs
 * (h0 > 64).  No device work.  0 with the error set for a dim or an h0 that
 * nrk_tt_user_fwd rejects. */
int nrk_tt_user_pass_users(int dim, int h0);

/* Item tower.  Replaces get_item_embedding (:184-188) + numpy re-norm
 * (:485-489): out[r] = renorm(normalize(E_i[ids[r]])). */
/* The user tower at any depth (youtubednn_hidden_units of any length,
 * youtubednn_recaller.py:105-112): weights packed per layer as W_l
 * [widths[l], in_l] row-major then b_l [widths[l]] (in_0 = 2 * dim), 1 to 8
 * layers of width <= 256, the last equal to dim.  Same outputs as
 * nrk_tt_user_fwd for two layers. */
int nrk_tt_user_fwd_layers(const float* user_table, int64_t n_user_rows, const float* item_table,
                           int64_t n_item_rows, int dim, const int32_t* uid, const int32_t* hist,
                           const int32_t* hist_len, int64_t n, int seq_len, const float* weights, int n_layers,
                           const int* widths, float* out, nrk_stream_t stream);
int nrk_tt_item_fwd(const float* item_table, int64_t n_item_rows, int dim, const int32_t* ids,
                    int64_t n, float* out, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* YouTubeDNN training (youtubednn_recaller.py:211-423)                   */
/* ---------------------------------------------------------------------- */

/* Shapes as nrk_tt_user_fwd_layers (dim in {16, 32, 64}, 1 to 8 layers of
 * width <= 256, the last equal to dim, seq_len in [1, 64]); batch in
 * [1, 8192].  Weights packed per layer W_l [widths[l], in_l] then b_l.
 *
 * A sample is (user, pos, target, label) over the click log in CSR form
 * (log_off int64 [n_user_rows + 1], log_items int32, each row in time order):
 * its history is log_items[log_off[user] : log_off[user] + min(pos, seq_len)]
 * (collate_fn :43-83), pos >= 1. */
size_t nrk_tt_train_workspace_bytes(int64_t n_user_rows, int64_t n_item_rows, int dim, int n_layers,
                                    const int* widths, int seq_len, int batch);

/* One batch: forward (train mode), mean BCE-with-logits loss and backward.
 *   loss     device float: the mean over the batch
 *   w_grad   dense gradient of the packed weights
 *   u_rows / u_vals / u_count   gradient of the user table as a compact list:
 *            *u_count ascending unique rows, u_vals [*u_count, dim]
 *            (capacity batch rows)
 *   i_rows / i_vals / i_count   the same for the item table (capacity
 *            batch * (seq_len + 1) rows)
 * Dropout (p in [0, 1), every layer, scale 1 / (1 - p)) keeps unit o of
 * layer l for sample b of the batch iff the counter-based generator of
 * nrk_tt_dropout_mask says so for (seed, step, l, b, o); p == 0 draws nothing.
 * Every output is bitwise reproducible: no floating-point atomics, the
 * batch sums and the per-row sums run in a fixed order. */
int nrk_tt_train_grad(const float* user_table, int64_t n_user_rows, const float* item_table,
                      int64_t n_item_rows, int dim, const float* weights, int n_layers, const int* widths,
                      const int64_t* log_off, const int32_t* log_items, const int32_t* s_user,
                      const int32_t* s_pos, const int32_t* s_target, const float* s_label, int batch,
                      int seq_len, float p, uint64_t seed, int64_t step, float* loss, float* w_grad,
                      int32_t* u_rows, float* u_vals, int32_t* u_count, int32_t* i_rows, float* i_vals,
                      int32_t* i_count, void* workspace, size_t workspace_bytes, nrk_stream_t stream);

/* out [batch, width] fp32: 1 where the generator keeps the unit, else 0. */
int nrk_tt_dropout_mask(uint64_t seed, int64_t step, int layer, int batch, int width, float p, float* out,
                        nrk_stream_t stream);

/* One torch.optim.Adam step (no weight decay, no amsgrad) with dense
 * semantics over the packed weights and both tables, in
 * _single_tensor_adam's operation order; t is the 1-based step number.
 * Rows absent from the compact lists have g = 0 and are still updated; a
 * row whose m, v and g are all zero is left untouched.  Moments are fp32
 * buffers of the parameters' shapes, owned by the caller. */
int nrk_tt_adam_step(float* weights, float* w_m, float* w_v, const float* w_grad, int64_t n_weights,
                     float* user_table, float* u_m, float* u_v, int64_t n_user_rows, const int32_t* u_rows,
                     const float* u_vals, const int32_t* u_count, float* item_table, float* i_m, float* i_v,
                     int64_t n_item_rows, const int32_t* i_rows, const float* i_vals, const int32_t* i_count,
                     int dim, double lr, double beta1, double beta2, double eps, int64_t t,
                     nrk_stream_t stream);

/* _prepare_data (:230-300) on the device.  The count query writes pos_off
 * int64 [n_users + 1]: the exclusive prefix of each user's number of training
 * positives (n clicks, n >= 2: positions 1 .. n - max(1, int(0.2 n)) - 1), so
 * pos_off[n_users] is the number of positives.  nrk_tt_make_samples then
 * writes n_pos * (1 + negsample) samples in (user, pos) order: each positive
 * (label 1) followed by its negsample negatives (label 0, same user and pos,
 * target uniform over pool[0 .. n_pool) with replacement). */
int nrk_tt_make_samples_count(const int64_t* log_off, int64_t n_users, int64_t* pos_off, nrk_stream_t stream);
int nrk_tt_make_samples(const int64_t* log_off, const int32_t* log_items, int64_t n_users,
                        const int64_t* pos_off, int64_t n_pos, int negsample, const int32_t* pool,
                        int64_t n_pool, uint64_t seed, int32_t* s_user, int32_t* s_pos, int32_t* s_target,
                        float* s_label, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Brute-force inner-product top-K (replaces faiss.IndexFlatIP)           */
/* ---------------------------------------------------------------------- */

/* Catalog = the "index": an fp16 copy of the item rows (power-of-two scaled)
 * in MFMA-fragment order, a header (max row norm, scale, max rounding error)
 * and, for dim <= 64, a half-block-major fp16 copy read by the refine's
 * prefilter.  Replaces faiss.IndexFlatIP(d).add(items)
 * (youtubednn_recaller.py:493-494).  items stays the fp32 source of truth
 * for exact rescoring and must outlive the catalog. */
size_t nrk_ip_catalog_bytes(int64_t n_items, int dim);
int nrk_ip_catalog_build(const float* items, int64_t n_items, int dim, void* catalog,
                         nrk_stream_t stream);

/* Exact top-k by inner product for every user row.  Replaces
 * faiss_index.search(user_emb, topk + 1) (youtubednn_recaller.py:520) for a
 * whole user batch at once.  Contract (same as IndexFlatIP): exact score
 * (fp64 accumulation of the fp32 products), sorted by score desc, ties ->
 * lower row; fewer than k items -> rows -1 / scores -FLT_MAX.
 * out_rows are catalog rows + row_offset (global rows of a shard).
 * out_exact (nullable) receives the fp64 scores used for ordering (the
 * merge key for catalog-sharded runs).  1 <= k <= 2048 (the fp16 MFMA screen
 * path up to k = 128, an exact radix-select path above); dim <= 256. */
size_t nrk_ip_topk_workspace_bytes(int64_t n_users, int64_t n_items, int dim, int k);
int nrk_ip_topk(const float* users, int64_t n_users, const float* items, const void* catalog,
                int64_t n_items, int dim, int k, int64_t row_offset, float* out_scores,
                int32_t* out_rows, double* out_exact, void* workspace, size_t workspace_bytes,
                nrk_stream_t stream);

/* The two phases of nrk_ip_topk, for callers that pipeline or time them:
 * screen (fp16 MFMA scan -> per user two append lists of half-block maxima,
 * their list bound and eps in the workspace; per-user (cut, eps) reads
 * (-inf, eps) after it) and finish (exact fp64 rescoring + ordering, exact
 * fallback for overflowed users).  finish must follow screen on the same
 * workspace, once.  After a plain screen, finish compacts the candidate band
 * from the append lists itself (every entry >= list bound - 2 eps); after
 * nrk_ip_topk_bound it reads the band that call built.  finish reads the
 * packed catalog (may be NULL) for an fp16 prefilter of the candidate band
 * before the exact fp32-row rescoring. */
int nrk_ip_topk_screen(const float* users, int64_t n_users, const void* catalog, int64_t n_items,
                       int dim, int k, void* workspace, size_t workspace_bytes,
                       nrk_stream_t stream);
/* nrk_ip_topk_screen in its two parts (timing / profiling of the MFMA scan
 * alone): nrk_ip_topk_scan, then nrk_ip_topk_select, same arguments.
 * nrk_ip_topk_select clears the workspace header (overflow counts, "no band
 * built") and, where there is no scan (no items, k > 128), marks the users;
 * it launches no kernel otherwise: the per-user select (theta, the k-th
 * largest appended maximum, and its band) runs in nrk_ip_topk_bound only. */
int nrk_ip_topk_scan(const float* users, int64_t n_users, const void* catalog, int64_t n_items, int dim, int k,
                     void* workspace, size_t workspace_bytes, nrk_stream_t stream);
int nrk_ip_topk_select(const float* users, int64_t n_users, const void* catalog, int64_t n_items, int dim, int k,
                       void* workspace, size_t workspace_bytes, nrk_stream_t stream);
int nrk_ip_topk_finish(const float* users, int64_t n_users, const float* items,
                       const void* catalog, int64_t n_items,
                       int dim, int k, int64_t row_offset, float* out_scores, int32_t* out_rows,
                       double* out_exact, void* workspace, size_t workspace_bytes,
                       nrk_stream_t stream);

/* Catalog-sharded runs, between screen and
 * finish:
 *   nrk_ip_topk_bound (same k as the screen) builds the band of the user's
 *   append lists (every entry >= theta - 2 eps, theta = the k-th largest
 *   appended maximum; finish then reads this band and its cut instead of the
 *   lists) and writes, per user, the m (<= 256) largest exact lower
 *   bounds this shard's screen found, descending, fp32 [n_users, m], -inf
 *   padded: each one bounds a distinct item's exact score from below.
 *   After an all_gather of every shard's [n_users, m] block (layout
 *   [n_lists][n_users][m], n_lists * m <= 512), nrk_ip_topk_apply_bound takes
 *   the k-th largest of the user's n_lists * m values -- a lower bound of
 *   the user's k-th exact score over the WHOLE catalog -- and raises the
 *   shard's refine cut to it, so finish rescores only the candidates that
 *   can still reach the merged top-k (the output then holds the shard's
 *   top-k among items with exact score >= the global bound, -1 padded).
 *   k > n_lists * m leaves the cut unchanged.  New: no reference
 *   counterpart (a Faiss search is single-index). */
int nrk_ip_topk_bound(const float* users, int64_t n_users, const void* catalog, int64_t n_items, int dim,
                      int k, int m, float* out_bound, void* workspace, size_t workspace_bytes,
                      nrk_stream_t stream);
int nrk_ip_topk_apply_bound(int64_t n_users, const float* bounds, int n_lists, int m, int k, void* workspace,
                            size_t workspace_bytes, nrk_stream_t stream);

/* 32-item blocks per screen tile at this dim (one LDS ring slot of the MFMA
 * scan; 8 KB, or 4 blocks = 32 KB at dims 65..128): catalog shard ranges start
 * on a tile.  0 for dim outside [1, 256].  Host-only, no device work.  New: no
 * reference counterpart (Faiss shards are whole indexes). */
int nrk_ip_topk_tile_blocks(int dim);

/* Config 4 (catalog sharded) with owner refine: every rank
 * holds the SAME packed catalog and fp32 rows (nrk_ip_catalog_build over all
 * items) and screens only its block range [blk_lo, blk_hi) (32-item blocks;
 * blk_lo a multiple of nrk_ip_topk_tile_blocks(dim), blk_hi too unless it is
 * the catalog end) for every user; half-block ids stay global.  No per-shard
 * select:
 *   nrk_ip_topk_shard_screen = the scan of [blk_lo, blk_hi) + per user the m
 *   (1..256) largest appended half-block maxima as exact lower bounds
 *   (out_bound [n_users, m] f32, descending, -inf padded; k <= 128);
 *   nrk_ip_topk_shard_band, after the all_gather of every shard's bounds
 *   (bounds [n_lists][n_users][m], n_lists * m <= 512, or NULL): cut =
 *   max(the scan's own list bound - 2 eps, k-th largest bound - eps), the
 *   appended half-blocks >= cut packed as uint32 global half-block ids to
 *   out_ent[u * x_cap + j] (x_cap in [1, 288]; out_cnt -1 when more: the
 *   user then takes the owner's exact path), and ucut written for the refine.
 * The ids and counts of each user block go to its owner in one fixed-size
 * all_to_all (nrk.dist.catalog_sharded_owner, or nrk_rccl_band_alltoall),
 * and the owner runs nrk_ip_topk_refine_x over its users: source s's ids for
 * user u at band[(s * src_users + u) * x_cap + j], j < src_cnt[s * src_users
 * + u]; ucut [n_users, 2] (cut, eps) = the owner's own shard_band values
 * for its user block (every shard's cut bounds the user's k-th exact score
 * over the whole catalog); ovf_in [n_users] (1 = exact path over the full
 * catalog).  Output = the final top-k (no merge).  New: no reference
 * counterpart. */
int nrk_ip_topk_shard_screen(const float* users, int64_t n_users, const void* catalog, int64_t n_items, int dim,
                             int k, int64_t blk_lo, int64_t blk_hi, int m, float* out_bound, void* workspace,
                             size_t workspace_bytes, nrk_stream_t stream);
int nrk_ip_topk_shard_band(int64_t n_users, int64_t n_items, int dim, int k, const float* bounds, int n_lists,
                           int m, int x_cap, void* workspace, size_t workspace_bytes, void* out_ent,
                           int32_t* out_cnt, nrk_stream_t stream);
int nrk_ip_topk_refine_x(const float* users, int64_t n_users, const float* items, const void* catalog,
                         int64_t n_items, int dim, int k, int64_t row_offset, const void* band, int n_src,
                         int64_t src_users, int x_cap, const int32_t* src_cnt, const float* ucut,
                         const int32_t* ovf_in, float* out_scores, int32_t* out_rows, double* out_exact,
                         void* workspace, size_t workspace_bytes, nrk_stream_t stream);

/* Merge n_lists per-shard top-k_in lists (fp64 exact scores + global rows,
 * list l of user u at [l * list_stride + u * k_in]) into the top-k_out by
 * (score desc, row asc).  New: the catalog-sharded multi-GPU merge
 * (SURVEY.md §8e); n_lists * k_in <= 1024. */
int nrk_topk_merge(const double* in_exact, const int32_t* in_rows, int n_lists,
                   int64_t list_stride, int64_t n_users, int k_in, int k_out, float* out_scores,
                   int32_t* out_rows, double* out_exact, nrk_stream_t stream);

/* nrk_ip_topk's contract for a SMALL user batch (the serving case: one
 * faiss_index.search per recall(user_id), youtubednn_recaller.py:520).
 * nrk_ip_topk gives 1,024 users to a workgroup, so a few users run on one
 * compute unit; this path splits the catalog across the chip instead: every
 * workgroup scores its slices of the fp32 rows exactly against a tile of
 * users and keeps a streaming top-k, one workgroup per user merges the lists.
 * No packed catalog is read.  Bit-identical outputs to nrk_ip_topk (rows,
 * fp32 scores, fp64 scores; the -1 / -FLT_MAX / -inf padding past n_items).
 * 1 <= k <= 128 (larger: NRK_EUNSUPPORTED, use nrk_ip_topk), dim <= 256,
 * n_users <= NRK_IP_QUERY_MAX_USERS (the workspace holds one k-entry list per
 * user and catalog workgroup), n_items < 2^30.  users and items must be
 * finite.  New: no reference counterpart.
 *   nrk_ip_query_plan: out = {users per workgroup tile, items per round,
 *   workgroups along the catalog, list capacity} of such a call -- a pure
 *   function of its arguments, no device work. */
#define NRK_IP_QUERY_MAX_USERS 4096
size_t nrk_ip_query_workspace_bytes(int64_t n_users, int64_t n_items, int dim, int k);
int nrk_ip_query_plan(int64_t n_users, int64_t n_items, int dim, int k, int32_t out[4]);
int nrk_ip_query(const float* users, int64_t n_users, const float* items, int64_t n_items, int dim, int k,
                 int64_t row_offset, float* out_scores, int32_t* out_rows, double* out_exact, void* workspace,
                 size_t workspace_bytes, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Embedding similarity (the second Faiss site)                           */
/* ---------------------------------------------------------------------- */

/* out[r] = x[r] / ||x[r]||, bit-identical to numpy's float32
 *   item_emb_np / np.linalg.norm(item_emb_np, axis=1, keepdims=True)
 * (src/similarity/embedding.py:41; pairwise float32 sum of squares, correctly
 * rounded sqrt and division).  norms (nullable) receives ||x[r]||.  The
 * self-search that follows (embedding.py:46-50) is nrk_ip_topk with
 * users == items == out.  dim <= 256; out may not alias x. */
int nrk_row_normalize(const float* x, int64_t n, int dim, float* out, float* norms,
                      nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* ItemCF co-occurrence similarity                                        */
/* ---------------------------------------------------------------------- */

/* Replaces ItemCFSimilarity.calculate (src/similarity/item_cf.py:17-89).
 * Input: user click lists in CSR (users in ascending id order, each list in
 * click-time order = UserFeatureExtractor.get_user_item_time_dict,
 * src/data/extractors.py:10-36), dense item ids, raw ms timestamps, and the
 * MinMax-scaled created time per dense item (float64).
 * Pass 1 (nrk_itemcf_pair_offsets): per-user pair-slot offsets
 * (pair_off[u] = sum_{v<u} L_v^2, pair_off[n_users] = total) -- the caller
 * reads the total to size the workspace and outputs.
 * Pass 2 (nrk_itemcf_sim): one entry per distinct (i, j), sorted by (i, j):
 * normalised similarity (fp64, per-pair weights summed in the reference's
 * order), first-encounter slot (the dict insertion order that the
 * reference's stable sorts use as tie-break) and item_cnt per dense item.
 * *out_n (device int64) receives the number of entries. */
int nrk_itemcf_pair_offsets(const int64_t* offsets, int64_t n_users, int64_t* pair_off,
                            nrk_stream_t stream);
size_t nrk_itemcf_workspace_bytes(int64_t n_pairs, int32_t n_items);
int nrk_itemcf_sim(const int64_t* offsets, int64_t n_users, const int32_t* items,
                   const int64_t* ts, const double* created, int32_t n_items,
                   const int64_t* pair_off, int64_t n_pairs, double loc_alpha,
                   double loc_alpha_rev, double loc_beta, double time_alpha,
                   double created_alpha, int32_t* out_i, int32_t* out_j, double* out_v,
                   int64_t* out_first, int64_t* out_n, int64_t* out_cnt, void* workspace,
                   size_t workspace_bytes, nrk_stream_t stream);

/* Per-row top-n of the similarity CSR by (score desc, first-encounter asc):
 * replaces ItemCFRecaller._precompute_topk_similar_items
 * (src/recall/itemcf_recaller.py:41-54).  row_off has n_rows + 1 entries.
 * Outputs [n_rows, topn] (-1 / 0 padded) and counts. topn <= 64. */
int nrk_itemcf_topn(const int64_t* row_off, int64_t n_rows, const int32_t* cols,
                    const double* vals, const int64_t* first, int topn, int32_t* out_cols,
                    double* out_vals, int32_t* out_cnt, nrk_stream_t stream);

/* Users-sharded ItemCF: each rank owns a contiguous user range
 * and items are owned by contiguous id ranges; one exchange step.
 * nrk_itemcf_pairs: the pair tuples of the rank's users -- key (i << b | j),
 * b = smallest with 2^b > n_items (sentinel for i == j), the pair's GLOBAL
 * slot (slot_base + local slot; the global slot order is the reference's
 * S[i][j] += w order), weight -- as nrk_itemcf_sim computes them, and the
 * rank's click counts (item_cnt += ; caller zeroes).  pair_off from
 * nrk_itemcf_pair_offsets over the rank's users.
 * nrk_itemcf_reduce: the owner's pass over the tuples it received, in global
 * slot order (all_to_all concatenates sources in rank order): one entry per
 * distinct key, (i, j), sum / sqrt(cnt_i cnt_j) with the all-reduced counts,
 * first slot.  Same results as nrk_itemcf_sim on one GPU. */
int nrk_itemcf_pairs(const int64_t* offsets, int64_t n_users, const int32_t* items, const int64_t* ts,
                     const double* created, int32_t n_items, const int64_t* pair_off, int64_t slot_base,
                     double loc_alpha, double loc_alpha_rev, double loc_beta, double time_alpha,
                     double created_alpha, uint64_t* keys, int32_t* slots, double* w, int64_t* item_cnt,
                     nrk_stream_t stream);
size_t nrk_itemcf_reduce_workspace_bytes(int64_t n);
int nrk_itemcf_reduce(const uint64_t* keys, const int32_t* slots, const double* w, int64_t n, int32_t n_items,
                      const int64_t* item_cnt, int32_t* out_i, int32_t* out_j, double* out_v,
                      int64_t* out_first, int64_t* out_n, void* workspace, size_t workspace_bytes,
                      nrk_stream_t stream);

/* CSR row offsets (n_rows + 1) of nrk_itemcf_sim's entries, which are sorted
 * by i: row_off[r] = number of entries with i < r. */
int nrk_itemcf_row_offsets(const int32_t* ei, int64_t n, int64_t n_rows, int64_t* row_off,
                           nrk_stream_t stream);

/* ItemCFRecaller.recall for a batch of query users (replaces the per-user
 * host loop of src/recall/itemcf_recaller.py:56-129).  Dense item ids; the
 * user click lists in CSR (offsets, items; the history order of
 * user_item_time_dict); q_slot[q] = the query's row in that CSR or -1 for an
 * unknown user (cold start, :68-70).  nbr_*: per item its top-n neighbours
 * [n_items, topn] from nrk_itemcf_topn (A9).  emb_* (ke = 0: none): per item
 * up to ke embedding neighbours (EmbeddingSimilarity, the content weight of
 * :98-103).  hot: item_topk_click (dense), the fill order of :116-122.
 * Pass 1 (nrk_itemcf_recall_offsets): cand_off[q] = exclusive prefix of the
 * candidate counts, cand_off[n_query] = n_cand (read it to size the
 * workspace).  Pass 2: per query up to topk (item, score) sorted like
 * sorted(item_rank.items(), key=score, reverse=True)[:topk] -- ties in dict
 * insertion order; out_src = 0 scored candidate, 1 hot fill (-x - 100),
 * 2 cold start (-x), -1 padding.  topk <= 64. */
int nrk_itemcf_recall_offsets(const int64_t* q_slot, int64_t n_query, const int64_t* offsets,
                              const int32_t* items, const int32_t* nbr_cnt, int64_t* cand_off,
                              nrk_stream_t stream);
size_t nrk_itemcf_recall_workspace_bytes(int64_t n_cand);
int nrk_itemcf_recall(const int64_t* q_slot, int64_t n_query, const int64_t* offsets, const int32_t* items,
                      const int32_t* nbr_cols, const double* nbr_vals, const int32_t* nbr_cnt, int topn,
                      const double* created, int32_t n_items, const int32_t* hot, int n_hot,
                      const int32_t* emb_cols, const double* emb_vals, const int32_t* emb_cnt, int ke,
                      double loc_beta, double created_alpha, const int64_t* cand_off, int64_t n_cand,
                      int topk, int32_t* out_items, double* out_scores, int32_t* out_src,
                      int32_t* out_cnt, void* workspace, size_t workspace_bytes, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* UserCF user-to-user similarity and recall                              */
/* ---------------------------------------------------------------------- */

/* Replaces UserCFSimilarity.calculate (src/similarity/user_cf.py:31-66),
 * which the reference ships but comments out of its pipeline
 * (src/recall/recall_pipeline.py:137,151-155): its host loop is
 * O(sum_items n_i^2) and stores every user pair.  Dense user and item ids.
 *   i_off [n_items + 1], i_users [n_clicks]: the item -> user CSR, items in
 *     ascending raw id, entries in the order of
 *     InteractionFeatureExtractor.get_item_user_time_dict
 *     (src/data/extractors.py:200-231);
 *   u_off [n_users + 1], u_items [n_clicks]: every user's clicks sorted by
 *     item, duplicates kept;
 *   act [n_users] the activate degree, pen [n_items] = 1.0 / log(n_i + 1),
 *     both fp64, formed on the host.
 * Row u's value for v is the fp64 sum of (50.0 * (act[u] + act[v])) * pen[i]
 * over the reference's (item, u entry, v entry) order, divided by
 * sqrt(cnt[u] * cnt[v]) -- bit-identical to the reference -- and its first
 * slot is the smallest index into i_users at which v stands in an item that
 * u clicked (the reference's dict insertion order).
 * nrk_usercf_topn: per user the top-n by (value desc, first slot asc), the
 * reference's stable sorted(..., reverse=True)[:topn]: out_cols / out_vals
 * [n_users, topn] (-1 / 0 padded), out_cnt [n_users] click rows, out_nnz
 * [n_users] distinct neighbours.  The u2u matrix is never materialised: the
 * workspace holds a fixed number of dense rows.  topn <= 1024.
 * nrk_usercf_sim: every (v, value, first slot) of every row, row u at
 * row_off[u] (row_off = the exclusive scan of out_nnz, n_entries its total),
 * entries of a row in no particular order (sort by first slot).  Same
 * workspace. */
size_t nrk_usercf_workspace_bytes(int64_t n_users, int64_t n_clicks, int topn);
int nrk_usercf_topn(const int64_t* i_off, int32_t n_items, const int32_t* i_users, const int64_t* u_off,
                    int64_t n_users, const int32_t* u_items, int64_t n_clicks, const double* act, const double* pen,
                    int topn, int32_t* out_cols, double* out_vals, int64_t* out_cnt, int32_t* out_nnz,
                    void* workspace, size_t workspace_bytes, nrk_stream_t stream);
int nrk_usercf_sim(const int64_t* i_off, int32_t n_items, const int32_t* i_users, const int64_t* u_off,
                   int64_t n_users, const int32_t* u_items, int64_t n_clicks, const double* act, const double* pen,
                   const int64_t* row_off, int64_t n_entries, int32_t* out_v, double* out_s, int64_t* out_first,
                   void* workspace, size_t workspace_bytes, nrk_stream_t stream);

/* UserCFRecaller.recall (src/recall/usercf_recaller.py:37-118) for a batch of
 * query users.  offsets / items: the user click lists in history order
 * (user_item_time_dict), dense ids; q_slot[q] = the query's row or -1 (cold
 * start, :48-53).  nbr_* [n_users, topn]: per user its top-n neighbours
 * (dense user rows, nrk_usercf_topn's order); loc_w [n_users] = 1 + sum_loc
 * beta^(L - loc) (:84-86), formed on the host.  Every click i of a
 * neighbour, in (neighbour rank, history position) order and not in the
 * query's history H, adds ((loc_w * content_w) * created_w) * w_uv with
 * content_w = 1 + the emb_* entries of (i, j) and (j, i) and created_w = 1 +
 * sum exp(created_alpha ^ |created_i - created_j|) over j in H (:76-102; the
 * reference passes the literal 0.8).  The per-item sums in walk order, the
 * hot fill and the top-k are those of nrk_itemcf_recall, and so are emb_*,
 * hot, cand_off / n_cand (pass 1: nrk_usercf_recall_offsets), the outputs
 * and the limits. */
int nrk_usercf_recall_offsets(const int64_t* q_slot, int64_t n_query, const int64_t* offsets,
                              const int32_t* nbr_cols, const int32_t* nbr_cnt, int topn, int64_t* cand_off,
                              nrk_stream_t stream);
size_t nrk_usercf_recall_workspace_bytes(int64_t n_cand);
int nrk_usercf_recall(const int64_t* q_slot, int64_t n_query, const int64_t* offsets, const int32_t* items,
                      const int32_t* nbr_cols, const double* nbr_vals, const int32_t* nbr_cnt, int topn,
                      const double* loc_w, const double* created, int32_t n_items, const int32_t* hot, int n_hot,
                      const int32_t* emb_cols, const double* emb_vals, const int32_t* emb_cnt, int ke,
                      double created_alpha, const int64_t* cand_off, int64_t n_cand, int topk, int32_t* out_items,
                      double* out_scores, int32_t* out_src, int32_t* out_cnt, void* workspace,
                      size_t workspace_bytes, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* DIN attention-over-history scorer                                      */
/* ---------------------------------------------------------------------- */

/* DINModel.forward (src/rank/DIN.py:214-286) in eval mode for one batch,
 * as DINRanker.predict drives it (DIN.py:1219-1283).  Dice uses the batch
 * statistics (mean, unbiased std over the batch, DIN.py:39-44), so a batch
 * is the unit of work and the caller batches exactly like the reference.
 *
 * Embedding tables: all per-feature nn.Embedding(vocab, 32) tables
 * concatenated row-wise into one table (fp32: table_dtype 0, bf16: 1);
 * feature f's row r lives at row_base[f] + r.  Feature order: user features
 * [0, n_user), item features [n_user, n_user + n_item) (shared by the
 * candidate and the history), context features after them.
 * Index tensors are int32: user [B, n_user], item [B, n_item],
 * hist [B, T, n_item], ctx [B, n_ctx]; mask [B, T] float (1 valid, 0 pad).
 * Weights (fp32, the state_dict tensors): att_w0 [36, 4*n_item*32],
 * att_b0 [36], att_w1 [36], att_b1 [1]; mlp_w0 [h1, in], mlp_b0 [h1],
 * mlp_w1 [h2, h1], mlp_b1 [h2], mlp_w2 [h2], mlp_b2 [1]
 * with in = 32 * (n_user + n_ctx + 2 * n_item).
 * nrk_din_prepare derives the batch-invariant attention matrices, the
 * power-of-two scales of the split-fp16 attention products (from max|table|),
 * the packed weight fragments and (bf16 tables) an fp16 copy of the table at
 * that scale, once per weight load into prep (nrk_din_prep_bytes(n_item,
 * n_table_rows)); call it again if the table changes.  B >= 2 (B = 1 is NaN in the
 * reference too). */
/* Embedding widths other than 32 (din_embedding_dim, src/utils/config.py:115,
 * read back by DINRanker.load_model, DIN.py:1371-1379): the kernels read
 * 32-wide VIRTUAL features.  The host zero-pads every table to
 * m = ceil(D / 32) * 32 columns, views it as [m * vocab, 32] (feature f's
 * index i -> virtual indices m i + h, h < m), expands att_w0 / mlp_w0 with
 * zero columns at the padded positions, and pads the item features with a
 * shared all-zero row up to 1, 2, 4 or 8.  nrk_din_remap_index maps caller
 * index rows [n_rows, f_in] to the virtual layout [n_rows, f_out]:
 * out[r, j] = map[j] < 0 ? map[2 f_out + j]
 *                        : in[r, map[j]] * map[f_out + j] + map[2 f_out + j]
 * (map: int32 device array, rows src | mul | add).  Identity when D = 32 and
 * the item-feature count is 1, 2, 4 or 8 (no call needed). */
int nrk_din_remap_index(const int32_t* in, int64_t n_rows, int f_in, const int32_t* map, int f_out,
                        int32_t* out, nrk_stream_t stream);
size_t nrk_din_prep_bytes(int n_item, int64_t n_table_rows);
int nrk_din_prepare(const float* att_w0, int n_item, const void* table, int table_dtype,
                    int64_t n_table_rows, void* prep, nrk_stream_t stream);
size_t nrk_din_workspace_bytes(int64_t batch, int seq_len, int n_user, int n_item, int n_ctx,
                               int h1, int h2);
int nrk_din_forward(const void* table, int table_dtype, const int64_t* row_base, int n_user,
                    int n_item, int n_ctx, const int32_t* user_idx, const int32_t* item_idx,
                    const int32_t* hist_idx, const int32_t* ctx_idx, const float* mask,
                    int64_t batch, int seq_len, const void* prep, const float* att_b0,
                    const float* att_w1, const float* att_b1, const float* mlp_w0,
                    const float* mlp_b0, int h1, const float* mlp_w1, const float* mlp_b1,
                    int h2, const float* mlp_w2, const float* mlp_b2, float* out_probs,
                    float* out_logits, void* workspace, size_t workspace_bytes,
                    nrk_stream_t stream);

/* The whole of DINRanker.predict (DIN.py:1245-1283) in one call: n_samples
 * rows scored as consecutive Dice batches of seg_len (the DataLoader's
 * batch_size, shuffle=False), each batch with its own statistics -- the
 * same result as nrk_din_forward once per batch, with every batch's phases
 * in one launch each.  seg_len >= n_samples is one batch (n_samples >= 2);
 * otherwise seg_len must be a multiple of 64.  A trailing batch of a single
 * row has no std (NaN in the reference): its output is unspecified here and
 * the caller marks it NaN.  Index tensors are [n_samples, ...] as above. */
size_t nrk_din_segments_workspace_bytes(int64_t n_samples, int64_t seg_len, int seq_len, int n_user,
                                        int n_item, int n_ctx, int h1, int h2);
int nrk_din_forward_segments(const void* table, int table_dtype, const int64_t* row_base, int n_user,
                             int n_item, int n_ctx, const int32_t* user_idx, const int32_t* item_idx,
                             const int32_t* hist_idx, const int32_t* ctx_idx, const float* mask,
                             int64_t n_samples, int64_t seg_len, int seq_len, const void* prep,
                             const float* att_b0, const float* att_w1, const float* att_b1,
                             const float* mlp_w0, const float* mlp_b0, int h1, const float* mlp_w1,
                             const float* mlp_b1, int h2, const float* mlp_w2, const float* mlp_b2,
                             float* out_probs, float* out_logits, void* workspace,
                             size_t workspace_bytes, nrk_stream_t stream);

/* nrk_din_forward_segments for any DINModel the reference's RankConfig
 * builds: n_layers in [1, 4] hidden layers (din_mlp_hidden_units,
 * src/utils/config.py:117) of widths[n] in [1, 1024], widths[0] = h1, and
 * activation 0 (Dice) or 1 (nn.PReLU(), din_activation, config.py:118,
 * DIN.py:203-206).  Arguments as nrk_din_forward_segments up to mlp_b0, then
 * HOST arrays of n_layers device pointers: mlp_w[n] / mlp_b[n] are the weight
 * [widths[n + 1], widths[n]] and bias of hidden layer n + 2 for
 * n < n_layers - 1, and mlp_w[n_layers - 1] [widths[n_layers - 1]] /
 * mlp_b[n_layers - 1] [1] the output row.  slopes: DEVICE float [n_layers],
 * the one slope of each PReLU (state_dict mlp.{2n+1}.weight); ignored (may be
 * null) under Dice.  The attention unit is Dice under either activation
 * (DIN.py:188), so the batch rules above hold for both.  Two Dice layers run
 * exactly what nrk_din_forward_segments runs.  Other n_layers or widths:
 * NRK_EUNSUPPORTED. */
size_t nrk_din_mlp_workspace_bytes(int64_t n_samples, int64_t seg_len, int seq_len, int n_user, int n_item,
                                   int n_ctx, int n_layers, const int* widths, int activation);
int nrk_din_forward_mlp(const void* table, int table_dtype, const int64_t* row_base, int n_user, int n_item,
                        int n_ctx, const int32_t* user_idx, const int32_t* item_idx, const int32_t* hist_idx,
                        const int32_t* ctx_idx, const float* mask, int64_t n_samples, int64_t seg_len,
                        int seq_len, const void* prep, const float* att_b0, const float* att_w1,
                        const float* att_b1, const float* mlp_w0, const float* mlp_b0, int n_layers,
                        const int* widths, const float* const* mlp_w, const float* const* mlp_b, int activation,
                        const float* slopes, float* out_probs, float* out_logits, void* workspace,
                        size_t workspace_bytes, nrk_stream_t stream);

/* DIN training (DINRanker.train's loop body, src/rank/DIN.py:907-912): one
 * batch of DINModel.forward in train mode, mean BCELoss and the backward,
 * all fp32.  Table, row_base, index tensors and mask as nrk_din_forward;
 * labels [batch] fp32, 0 or 1.  weights is one packed vector in the order
 *   att_w0 [36, 4*n_item*32] | att_b0 [36] | att_w1 [36] | att_b1 [1] |
 *   mlp_w0 [h1, in] | mlp_b0 [h1] | mlp_w1 [h2, h1] | mlp_b1 [h2] |
 *   mlp_w2 [h2] | mlp_b2 [1]
 * and w_grad its dense gradient (the Dice alphas have none).  Built for
 * dim == 32, fp32 tables (table_dtype 0), Dice (activation 0), n_item in
 * {1, 2, 4, 8}, n_user in [1, 64], n_ctx in [0, 64], h1 and h2 in [1, 1024],
 * batch in [2, 8192], seq_len in [1, 128]; anything else is NRK_EUNSUPPORTED
 * before a pointer is touched (the workspace query then returns 0).
 *   loss     device float: the mean over the batch
 *   t_rows / t_vals / t_count   gradient of the concatenated table as a
 *            compact list: *t_count ascending unique rows, t_vals
 *            [*t_count, 32]; capacity min(n_table_rows, batch *
 *            (n_user + n_ctx + n_item * (1 + seq_len))) rows.  Candidate and
 *            history contributions of an item table meet in the same rows.
 * Masked positions carry gradient through the Dice statistics of their
 * columns (into row 0 of every item table among others).  Every output is
 * bitwise reproducible.  No host synchronisation. */
size_t nrk_din_train_workspace_bytes(int64_t n_table_rows, int dim, int table_dtype, int n_user, int n_item,
                                     int n_ctx, int h1, int h2, int activation, int64_t batch, int seq_len);
int nrk_din_train_grad(const float* table, int64_t n_table_rows, int dim, int table_dtype, const int64_t* row_base,
                       int n_user, int n_item, int n_ctx, const float* weights, int h1, int h2, int activation,
                       const int32_t* user_idx, const int32_t* item_idx, const int32_t* hist_idx,
                       const int32_t* ctx_idx, const float* mask, const float* labels, int64_t batch, int seq_len,
                       float* loss, float* w_grad, int32_t* t_rows, float* t_vals, int32_t* t_count, void* workspace,
                       size_t workspace_bytes, nrk_stream_t stream);

/* nrk_din_train_grad for every DINModel nrk_din_forward_mlp serves: n_layers
 * in [1, 4] hidden layers of widths[n] in [1, 1024] (HOST array) and
 * activation 0 (Dice) or 1 (nn.PReLU(): one trained slope per layer,
 * initialised to 0.25 by torch).  Everything else as nrk_din_train_grad, the
 * attention unit (Dice, hidden width 36) and the batch rule included: batch
 * in [2, 8192] under either activation.  Packed weights and w_grad:
 *   att_w0 | att_b0 | att_w1 | att_b1 |
 *   per hidden layer n: w_n [widths[n], k_n] | b_n [widths[n]] |
 *                       (PReLU only) slope_n [1] |         k_0 = in, k_n = widths[n-1]
 *   w_out [widths[n_layers-1]] | b_out [1]
 * nrk_din_train_mlp_n_weights is that vector's length (0 and the last error
 * if the shape is refused).  Two Dice layers give nrk_din_train_grad's layout
 * and run the same device code: the results are bit-equal.  nrk_din_adam_step
 * takes the longer vector as it is; the slopes get their update from the same
 * sweep.  PReLU follows torch at the kink: y = x > 0 ? x : a x,
 * dx = x > 0 ? g : a g, d a = sum (x > 0 ? 0 : x g), the sum in a fixed order
 * in fp64 (bitwise reproducible like every other output).  A null widths or an
 * activation other than 0 / 1 is NRK_EINVAL, any other shape outside the above
 * NRK_EUNSUPPORTED, both before a pointer is touched. */
size_t nrk_din_train_mlp_workspace_bytes(int64_t n_table_rows, int dim, int table_dtype, int n_user, int n_item,
                                         int n_ctx, int n_layers, const int32_t* widths, int activation,
                                         int64_t batch, int seq_len);
int64_t nrk_din_train_mlp_n_weights(int dim, int n_user, int n_item, int n_ctx, int n_layers, const int32_t* widths,
                                    int activation);
int nrk_din_train_grad_mlp(const float* table, int64_t n_table_rows, int dim, int table_dtype, const int64_t* row_base,
                           int n_user, int n_item, int n_ctx, const float* weights, int n_layers,
                           const int32_t* widths, int activation, const int32_t* user_idx, const int32_t* item_idx,
                           const int32_t* hist_idx, const int32_t* ctx_idx, const float* mask, const float* labels,
                           int64_t batch, int seq_len, float* loss, float* w_grad, int32_t* t_rows, float* t_vals,
                           int32_t* t_count, void* workspace, size_t workspace_bytes, nrk_stream_t stream);

/* One torch.optim.Adam step with dense semantics over the packed weights
 * and the whole table (as nrk_tt_adam_step): rows absent from the list have
 * g = 0 and still move; a row with m = v = g = 0 is left untouched. */
int nrk_din_adam_step(float* weights, float* w_m, float* w_v, const float* w_grad, int64_t n_weights, float* table,
                      float* t_m, float* t_v, int64_t n_table_rows, int dim, const int32_t* t_rows,
                      const float* t_vals, const int32_t* t_count, double lr, double beta1, double beta2, double eps,
                      int64_t t, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Recall -> rank hand-off (fused config 5)                               */
/* ---------------------------------------------------------------------- */

/* Builds the DIN index tensors of the recalled pairs of users [u0, u0 + nu)
 * on the device -- the counterpart of the host feature assembly and
 * encoding (src/features/feature_extractor.py:440-723, src/rank/DIN.py:330-520)
 * for the fused pipeline.  rec_rows / rec_scores [n_users, k_in] from
 * nrk_ip_topk; pair p = (u - u0) * k_use + c uses recall column c + skip
 * (skip = 1 drops rank 0 as youtubednn_recaller.py:524 does).  user_feat
 * [n_users, n_user], item_feat [n_items, n_item] table indices; user_hist
 * [n_users, T] item rows (left-aligned, hist_len valid).  Outputs
 * out_user [P, n_user], out_item [P, n_item], out_hist [P, T, n_item]
 * (0 on padding), out_ctx [P, n_ctx] (ctx 0 = recall-score bin + 1, the
 * rest hash bins + 1), out_mask [P, T], out_cand [P] (candidate item row). */
int nrk_din_assemble(const int32_t* rec_rows, const float* rec_scores, int64_t n_users, int k_in, int skip,
                     int k_use, const int32_t* user_feat, int n_user, const int32_t* item_feat,
                     int64_t n_items, int n_item, const int32_t* user_hist, const int32_t* hist_len, int T,
                     int n_ctx, int ctx_bins, float score_lo, float score_hi, uint32_t seed, int64_t u0,
                     int64_t nu, int32_t* out_user, int32_t* out_item, int32_t* out_hist, int32_t* out_ctx,
                     float* out_mask, int32_t* out_cand, nrk_stream_t stream);

/* Row gather of 4-byte words (int32 codes or f32 mask values): out[b] =
 * src[idx[b]] (row_words words per row), zeros when idx[b] is outside
 * [0, n_rows).  The device half of the vectorised DIN encoder
 * (nrk/rank/encode.py): DINDataset.__getitem__ + collate_fn (src/rank/
 * DIN.py:358-520) look every sample's user profile, candidate item features
 * and last-T history up in per-user / per-item dicts; here those lookups
 * become row indices into encoded tables resident in HBM. */
int nrk_gather_rows(const void* src, int64_t n_rows, int row_words, const int32_t* idx, int64_t n, void* out,
                    nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Recall fusion                                                          */
/* ---------------------------------------------------------------------- */

/* RecallFusion.fuse (src/recall/fusion.py:267-342) for every user at once.
 * Entries of all recall methods' lists grouped by user (offsets [n_users+1]),
 * inside a user in method order then list order: item (dense int32 code),
 * raw score (f64), method index, position in its list.  weight [n_methods].
 * strategy: 0 weighted_sum, 1 weighted_avg, 2 max_score, 3 harmonic_mean,
 * 4 diversity_weighted, 5 rrf (:189-265).  norm: 0 local (per list min-max,
 * :71-98), 1 global (gmin / gmax from nrk_fuse_minmax, :100-134), 2 z-score
 * (zmean / zstd per method, :136-187; device exp), 3 pre-normalised (the
 * caller passes the normalised scores: the Python wrapper computes the
 * z-score sigmoid with numpy exactly as the reference does).  Optional
 * seen_off / seen: per-user item codes removed after the merge (:320-326).
 * Output: the top-k items by (merged score desc, first appearance asc) --
 * the reference's stable sort of its insertion-ordered dict -- -1 padded,
 * and the count per user.  nrk_fuse takes users of at most 256 entries: a
 * user with more gets out_cnt = -1 (padded output); nrk_fuse_wide takes any
 * user of at most max_entries (<= 2048) entries, any topk. */
int nrk_fuse_minmax(const double* score, int64_t n, double* out_minmax, nrk_stream_t stream);
int nrk_fuse(const int64_t* offsets, int64_t n_users, const int32_t* item, const double* score,
             const int32_t* method, const int32_t* rank, int n_methods, const double* weight, int strategy,
             int norm, double gmin, double gmax, const double* zmean, const double* zstd, const int64_t* seen_off,
             const int32_t* seen, int topk, int32_t* out_item, double* out_score, int32_t* out_cnt,
             nrk_stream_t stream);
int nrk_fuse_wide(const int64_t* offsets, int64_t n_users, const int32_t* item, const double* score,
                  const int32_t* method, const int32_t* rank, int n_methods, const double* weight, int strategy,
                  int norm, double gmin, double gmax, const double* zmean, const double* zstd,
                  const int64_t* seen_off, const int32_t* seen, int max_entries, int topk, int32_t* out_item,
                  double* out_score, int32_t* out_cnt, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Cold-start recall                                                      */
/* ---------------------------------------------------------------------- */

/* ColdStartRecaller (src/recall/coldstart_recaller.py) over dense ids.
 * Lists: list_off [n_lists + 1], item [n_entries] (row of the item tables, or
 * -1 = missing from one of the three item dicts, :86-91), score [n_entries]
 * f64, in list order; prof [n_lists] = row of the profile tables or -1 (the
 * user is not in user_hist_item_types_dict, :74).  Profile tables: cat_off
 * [n_prof + 1] / cat [n_cat] (every user's distinct category codes,
 * ascending), mean_words, last_created [n_prof] f64.  Item tables [n_items]:
 * item_type int32, item_words / item_created f64, item_clicked uint8.  A pair
 * is kept when (:98-115, in f64 with the reference's operations)
 *   prof >= 0 && item >= 0 && cat contains item_type[item]
 *   && !item_clicked[item] && !(fabs(item_words[item] - mean_words[p]) > words_tol)
 *   && !(fabs(item_created[item] - last_created[p]) > time_tol)
 * so a NaN mean or time keeps the pair, as the reference's `>` does.
 *
 * nrk_coldstart_filter replaces _apply_filtering's loop (:71-120) for every
 * list in one launch: keep [n_entries] uint8 (1 = kept), kept [n_lists] the
 * count per list.  Lists and category sets of any length.
 *
 * nrk_coldstart_recall replaces recall (:139-147) for n_query users in one
 * launch: q [n_query] = list index or -1 (unknown user: empty).  Per query:
 * the filter, then the top-k of the survivors by (score desc, position asc)
 * -- Python's stable sorted(..., reverse=True)[:topk]; -0.0 == +0.0, NaN
 * scores are the caller's to refuse.  out_pos [n_query, topk] = position
 * inside the list (-1 padded), out_score [n_query, topk] (0 padded), out_cnt
 * [n_query].  cap in [1, 2048] is the survivor capacity per user (LDS slots):
 * a user with more survivors gets out_cnt = -1 and padded rows.  topk in
 * [1, 2048].  No workspace, no allocation, no host sync. */
int nrk_coldstart_filter(const int64_t* list_off, int64_t n_lists, const int32_t* item, int64_t n_entries,
                         const int32_t* prof, const int64_t* cat_off, const int32_t* cat, int64_t n_cat,
                         const double* mean_words, const double* last_created, int64_t n_prof,
                         const int32_t* item_type, const double* item_words, const double* item_created,
                         const uint8_t* item_clicked, int64_t n_items, double words_tol, double time_tol,
                         uint8_t* keep, int32_t* kept, nrk_stream_t stream);
int nrk_coldstart_recall(const int64_t* q, int64_t n_query, const int64_t* list_off, int64_t n_lists,
                         const int32_t* item, const double* score, int64_t n_entries, const int32_t* prof,
                         const int64_t* cat_off, const int32_t* cat, int64_t n_cat, const double* mean_words,
                         const double* last_created, int64_t n_prof, const int32_t* item_type,
                         const double* item_words, const double* item_created, const uint8_t* item_clicked,
                         int64_t n_items, double words_tol, double time_tol, int cap, int topk, int32_t* out_pos,
                         double* out_score, int32_t* out_cnt, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* User profiles, item popularity, labels                                 */
/* ---------------------------------------------------------------------- */

/* FeatureExtractor._extract_user_profile_features / _extract_item_features /
 * _add_labels (src/features/feature_extractor.py:296-438, :752-836) over
 * dense ids.  The click log is a CSR by user row: u_off [n_users + 1]; inside
 * a user the clicks in frame order: item (row of the item tables; a row
 * outside [0, n_items) is an article without a words entry), ts
 * (click_timestamp), dev_code (dense device-group code in [0, n_codes),
 * ascending in the raw value).  sorted_item [n_clicks] is the same CSR with
 * every user's item rows ascending (the caller's key sort); words [n_items]
 * the word count per item row.
 *
 * nrk_profile_user, per user (a user without clicks: zeros, mode and last
 * item -1):
 *   out_count    clicks
 *   out_gap      (double)(max ts - min ts) / (double)(n - 1), 0.0 at n = 1
 *   out_mean_ts  pandas' groupby mean: the Kahan sum of the float64-cast
 *                timestamps in frame order / n; (double)sum / n when no
 *                timestamp is negative and the exact sum is below 2^53, where
 *                the two agree
 *   out_mode     x.mode()[0]: the smallest of the most frequent codes
 *   out_words    (double)(sum of words over the distinct items) / n_distinct
 *   out_last     item of the maximal timestamp, ties to the later position
 * n_codes > 64 is NRK_EUNSUPPORTED.
 *
 * nrk_profile_item_count: clicks per item row (integer atomics), rows outside
 * [0, n_items) ignored.
 *
 * nrk_profile_scale: sklearn's MinMaxScaler of one column with minmax [2] =
 * {min, max} on the device (nrk_fuse_minmax): scale = 1 / range (a range
 * below 10 eps counts as 1), min_ = 0 - min * scale, out = x * scale + min_
 * as two rounded operations.  skip_zero = 1 leaves entries equal to 0 at 0.0
 * (the popularity of an unclicked item).
 *
 * nrk_profile_labels: out[i] = 1 when last_item[user[i]] == item[i], else 0
 * (a user or item row of -1: 0); offline = 0 writes -1 everywhere and reads
 * no input.  No workspace, no allocation, no host sync in any of the four. */
int nrk_profile_user(const int64_t* u_off, int64_t n_users, const int32_t* item, const int64_t* ts,
                     const int32_t* dev_code, int64_t n_clicks, int n_codes, const int32_t* sorted_item,
                     const int64_t* words, int64_t n_items, int64_t* out_count, double* out_gap,
                     double* out_mean_ts, int32_t* out_mode, double* out_words, int32_t* out_last,
                     nrk_stream_t stream);
int nrk_profile_item_count(const int32_t* item, int64_t n_clicks, int64_t n_items, int64_t* out_count,
                           nrk_stream_t stream);
int nrk_profile_scale(const double* x, int64_t n, const double* minmax, int skip_zero, double* out,
                      nrk_stream_t stream);
int nrk_profile_labels(const int32_t* user, const int32_t* item, int64_t n_pairs, const int32_t* last_item,
                       int64_t n_users, int offline, int32_t* out, nrk_stream_t stream);

/* ---------------------------------------------------------------------- */
/* Ranker context features                                                */
/* ---------------------------------------------------------------------- */

/* FeatureExtractor._extract_context_features
 * (src/features/feature_extractor.py:440-723) for every (user, recalled
 * item) row, then the fitted binning (_apply_binning :838-898) and context
 * LabelEncoder codes (src/rank/DIN.py:330-353, :560-617).  Features per row,
 * F = 1 + 3 * last_n + 6 (16 at last_n = 3), in feature_lists order:
 *   score, (sim_i, time_diff_i, word_diff_i) i = 1..last_n, sim_max,
 *   sim_mean, sim_min, sim_std, item_user_sim, recall_in_user_cat.
 * Rows are processed in user groups (group_off / pair_pos); tables are
 * indexed by dense user / item rows.  Outputs (either may be NULL):
 * out_raw [n_rows, F] f64 (the reference's column values: float32 features
 * exactly representable, NaN where the reference leaves NaN) and out_codes
 * [n_rows, code_stride] int32 (spec[f] applied to feature f). */
typedef struct {
    int64_t n_groups;           /* user groups                                      */
    const int64_t* group_off;   /* [n_groups + 1] into the grouped pair order       */
    const int32_t* group_user;  /* [n_groups] user row (-1: no such user)           */
    const int64_t* pair_pos;    /* [n_pairs] output row of grouped pair q (NULL: q) */
    const int32_t* pair_item;   /* [n_rows] item row of output row (-1: unknown)    */
    const double* pair_score;   /* [n_rows] recall score                            */
    int32_t last_n;             /* history items used (config.last_N = 3), <= 4     */
    int32_t code_stride;        /* row stride of out_codes (>= F)                   */
    const int32_t* hist_last;   /* [n_users, last_n] last items, oldest first, -1 = unknown item */
    const int32_t* hist_n;      /* [n_users] min(len, last_n); -1 = no history entry */
    const int64_t* ucat_off;    /* [n_users + 1] */
    const int32_t* ucat;        /* distinct categories of each user's whole history */
    const float* user_yt;       /* [n_users, dy] YouTubeDNN user vectors, or NULL   */
    const uint8_t* user_yt_ok;  /* [n_users] */
    int64_t n_items;
    const float* w2v;           /* [n_items, dw] article-id Word2Vec vectors        */
    const uint8_t* w2v_ok;      /* [n_items] */
    int32_t dw;
    const double* content;      /* [n_items, dc] content embeddings (float64)       */
    const uint8_t* content_flags; /* bit 0 row present, bit 1 f32 row not all zero */
    int32_t dc;
    const double* created;      /* [n_items] MinMax created time, NaN = missing     */
    const int32_t* category;    /* [n_items] category, -1 = missing                 */
    const float* item_yt;       /* [n_items, dy] YouTubeDNN item vectors            */
    const uint8_t* item_yt_ok;  /* [n_items] */
    int32_t dy;
} nrk_ctx_tables;

/* One feature's fitted encoding.  kind 0 (KBins-binned): NaN -> fill, bin =
 * #(edges[k] <= value) over the inner edges, code = lut[bin] (0 past n_lut).
 * kind 1 (unbinned): code = codes[k] where vals[k] == value, else 0. */
typedef struct {
    int32_t kind, n_edges, n_lut, n_vals;
    double fill;
    double edges[16];
    double vals[32];
    int32_t lut[32];
    int32_t codes[32];
} nrk_ctx_spec;

int nrk_ctx_features(const nrk_ctx_tables* tables, const nrk_ctx_spec* spec, double* out_raw, int32_t* out_codes,
                     nrk_stream_t stream);

/* The order statistics a context spec is fitted from (_apply_binning's
 * nunique / median / fillna and the ranks np.percentile interpolates between),
 * of n_cols columns of the raw feature matrix nrk_ctx_features writes.  Every
 * requested column is turned into order-preserving u64 keys (-0.0 = +0.0, NaN
 * last), sorted (keys-only LSD radix sort, one segment per column) and
 * summarised; the interpolation of the edges is the caller's (nrk/features.py
 * _finish_edges).  No host sync, no allocation; the result depends only on the
 * multiset of each column's values.
 *   raw        device, row-major [n_rows, ld] f64
 *   cols       HOST [n_cols] column indices (any order, < ld)
 *   col_kind   HOST [n_cols] 0 = f64, 1 = f32, 2 = integer-valued: the dtype the
 *              even-count median is formed in ((a + b) / 2 in f32 for kind 1);
 *              a valid value that kind 1 / 2 cannot hold sets `inexact`
 *   ranks      HOST [n_ranks] ascending ranks in [0, n_rows) into the FILLED
 *              sorted column: the sorted valid values with the n_rows - n_valid
 *              NaN rows replaced by `fill` at its place; n_ranks <= 64
 *   out_stats  device [n_cols]
 *   out_picks  device [n_cols, n_ranks] the filled column's value at each rank
 * n_rows == 0 is NRK_OK with nothing launched; n_rows >= 2^31 is
 * NRK_EUNSUPPORTED; n_cols is in [1, 64]. */
typedef struct {
    int64_t n_valid;      /* rows that are not NaN                                   */
    int64_t n_distinct;   /* distinct valid values                                   */
    double vmin, vmax;    /* of the valid values (0 when there is none)              */
    double mid_lo, mid_hi; /* the two middle valid values (equal when n_valid is odd) */
    double fill;          /* the median in the column's kind; 0 when n_valid == 0    */
    int64_t n_lt_fill;    /* valid values below fill                                 */
    int64_t n_eq_fill;    /* valid values equal to fill                              */
    double small[21];     /* the min(n_distinct, 21) smallest distinct values, ascending; then 0 */
    int64_t inexact;      /* 1: some valid value is not representable in the kind    */
} nrk_ctx_fit_col;

size_t nrk_ctx_fit_workspace_bytes(int64_t n_rows, int32_t n_cols); /* 0: arguments out of range */
int32_t nrk_ctx_fit_tile(void);                                     /* keys per sort tile */
int nrk_ctx_fit_stats(const double* raw, int64_t n_rows, int32_t ld, const int32_t* cols, const int32_t* col_kind,
                      int32_t n_cols, const int64_t* ranks, int32_t n_ranks, nrk_ctx_fit_col* out_stats,
                      double* out_picks, void* workspace, size_t workspace_bytes, nrk_stream_t stream);
/* After nrk_ctx_fit_stats, on the workspace it left (same n_rows, n_cols, not
 * written since): out_counts[c, p] = valid values of column c below
 * probes[c, p] (device [n_cols, n_probes] each, n_probes <= 64; a NaN probe
 * counts 0).  With the candidate bin edges as probes the differences say which
 * bins hold a row, i.e. the classes the reference's LabelEncoder sees. */
int nrk_ctx_fit_count_below(int64_t n_rows, int32_t n_cols, const double* probes, int32_t n_probes,
                            int64_t* out_counts, const void* workspace, size_t workspace_bytes,
                            nrk_stream_t stream);

/* ---- multi-GPU exchanges over RCCL --------
 * For a caller binding the C ABI without torch.distributed: one process per
 * GPU; rank 0 makes a unique id (nrk_rccl_unique_id_bytes() bytes), the
 * caller sends it to every rank, each rank calls nrk_rccl_comm_init with its
 * device current.  Communicators are opaque (void*).
 * nrk_rccl_topk_allgather: the merge protocol -- all-gather every shard's
 *   top-k_in of every user (fp64 + global row) into the caller's
 *   gather_exact / gather_rows [n_ranks][n_users][k_in], then nrk_topk_merge.
 *   Replaces: nothing (a Faiss search is single-index).
 * nrk_rccl_bound_allgather / nrk_rccl_band_alltoall: the owner protocol's
 *   two exchanges (bounds [n_users, m] f32; counts [n_ranks * per] and
 *   x_cap ids per user, user block o to rank o), around
 *   nrk_ip_topk_shard_screen / _shard_band / _refine_x. */
int nrk_rccl_unique_id_bytes(void);
int nrk_rccl_get_unique_id(void* out_id);
int nrk_rccl_comm_init(void** out_comm, int n_ranks, const void* id, int rank);
int nrk_rccl_comm_destroy(void* comm);
int nrk_rccl_topk_allgather(void* comm, const double* in_exact, const int32_t* in_rows, int64_t n_users, int k_in,
                            int k_out, double* gather_exact, int32_t* gather_rows, float* out_scores,
                            int32_t* out_rows, double* out_exact, nrk_stream_t stream);
int nrk_rccl_bound_allgather(void* comm, const float* bounds, int64_t n_users, int m, float* out,
                             nrk_stream_t stream);
int nrk_rccl_band_alltoall(void* comm, const int32_t* cnt, const int32_t* ids, int64_t per, int x_cap,
                           int32_t* out_cnt, int32_t* out_ids, nrk_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NRK_H */
