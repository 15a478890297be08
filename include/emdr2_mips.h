/*
 * include/emdr2_mips.h -- C ABI of the MI355X-native MIPS path (libemdr2_hip.so).
 *
 * Drop-in boundary for the reference's evidence search.  The reference has no native ABI for
 * this path (it is torch.matmul + torch.topk driven from Python); these entry points are what a
 * ctypes/cffi binding added next to megatron/data/emdr2_index.py would call:
 *
 *   emdr2_mips_pack_rows      replaces  DistributedBruteForceIndex.add_embed_data   emdr2_index.py:241-266
 *                                       (dense fp16 [N,768] upload; here: upload + stripe-tiling)
 *   emdr2_mips_search         replaces  DistributedBruteForceIndex.search_mips_index emdr2_index.py:268-305
 *                                       (fp16 Q*E^T, dense C[Q,N], torch.topk, id_map loop)
 *   emdr2_mips_search_exact   same contract, slow all-exact path for queries the fast path flags
 *   emdr2_mips_merge          replaces  the gather of per-device partial results     emdr2_index.py:284-295
 *                                       and the two broadcasts                       emdr2_model.py:451-452
 *                                       (here: k-way merge of per-shard top-k after ONE all-gather)
 *   emdr2_mips_unpack_rows    inverse of pack_rows (reconstruct / store export)
 *   emdr2_mips_gather_rows    the same by GLOBAL row, zero rows outside the shard (search_and_reconstruct over a sharded index;
 *                             the retrieved passages' embeddings for --context-embeddings-from-index)
 *   emdr2_mips_audit          no counterpart in the reference: re-checks, on the image in HBM, the stored bounds the search's proof rests on
 *
 * Conventions: raw device pointers + sizes + hipStream_t; the caller (torch) owns every buffer;
 * nothing is allocated inside; every function returns 0 on success or a negative EMDR2_E_* code
 * (no exceptions cross the ABI; the Python side raises).  All kernels are enqueued on `stream`
 * and the call returns without synchronising.
 *
 * Numerics contract: score(q,r) = RNE_fp16(exact sum_d q[d]*E[r][d]);
 * results ordered by (score desc, row asc); rows are positions in the store's insertion order.
 */
#ifndef EMDR2_MIPS_H
#define EMDR2_MIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMDR2_ABI_VERSION 4

#define EMDR2_OK 0
#define EMDR2_E_BADARG (-1)      /* bad size / alignment / null pointer */
#define EMDR2_E_WORKSPACE (-2)   /* workspace too small */
#define EMDR2_E_LAUNCH (-3)      /* HIP launch / runtime error */
#define EMDR2_E_UNSUPPORTED (-4) /* shape outside the supported envelope */

/* per-query flag bits written by emdr2_mips_search */
#define EMDR2_FLAG_AMBIGUOUS 1u /* fast path could not prove its top-k canonical: rerun with _search_exact */
#define EMDR2_FLAG_OVERFLOW 2u  /* candidate buffer overflowed (adversarial row order): rerun with _search_exact */

#define EMDR2_STRIPE_ROWS 128 /* rows per HBM stripe */
#define EMDR2_CHUNK_K 32      /* k-elements per stripe chunk */
#define EMDR2_MAX_TOPK 120    /* k <= 120 (candidate lists hold 64 or 128 rows) */
#define EMDR2_MAX_QUERIES_PER_PASS 512

typedef void *emdr2_stream_t; /* hipStream_t */

int emdr2_abi_version(void);

/* number of compute units of the current device (grid sizing, reported by bench.py) */
int emdr2_device_cu_count(void);

/* Bytes of the stripe-tiled index image for n_rows x dim fp16 (dim % 32 == 0, dim >= 64).
 * Rows are padded with zeros up to a multiple of 512. */
int emdr2_mips_layout_bytes(int64_t n_rows, int dim, size_t *bytes);

/* Re-layout rows [row_offset, row_offset + n_chunk) of the shard from row-major fp16 (device
 * pointer rows_rm, n_chunk x dim) into the stripe-tiled image `tiled` (device, layout_bytes,
 * zero-initialised by the caller before the first chunk).  Also folds max_r ||E[r]||_2^2 of the
 * chunk into *emax_sq (device float, caller initialises to 0). */
int emdr2_mips_pack_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset,
                         int64_t n_rows_total, void *tiled, float *emax_sq, emdr2_stream_t stream);

/* Gather rows back: rows_rm[i] = E[row_ids[i]] (row-major fp16), row_ids device int64 (local rows).  An id outside [0, n_rows_total)
 * yields a zero row (it is _gather_rows with row_base 0). */
int emdr2_mips_unpack_rows(const void *tiled, int64_t n_rows_total, int dim, const int64_t *row_ids,
                           int64_t n_out, void *rows_rm, emdr2_stream_t stream);

/* Gather by GLOBAL row (search results: out_row / last_search_rows): rows_rm (device fp16 [n_out, dim], row-major, 16-byte aligned)
 * row i receives image row global_rows[i] - row_base, bit for bit, when that row lies in [0, n_rows); otherwise all zero bytes -- -1 (an
 * empty slot), a row of another rank's shard, a row in the zero padding.  So every rank can be handed the same merged row list and the
 * buffers of the ranks have exactly one non-zero contributor per row.  One launch of 16-byte segment copies on `stream`; nothing is
 * allocated, no host synchronisation.  n_out == 0 is a no-op returning 0; EMDR2_E_BADARG for null pointers, row_base < 0 or a dim
 * outside the layout's envelope. */
int emdr2_mips_gather_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const int64_t *global_rows, int64_t n_out,
                           void *rows_rm, emdr2_stream_t stream);

/*
 * Index snapshots: a contiguous row range of a shard image back out of HBM, and its digest.
 *   _export_rows  the inverse of _pack_rows for image rows [row_offset, row_offset + n_chunk): rows_rm (device fp16 [n_chunk, dim],
 *                 row-major) receives them.  No row-id array, nothing allocated.
 *   _digest_rows  adds into digest[0] (wrap-around sum) and XORs into digest[1] the 64-bit hash g(r) of every row r of the range
 *                 (device uint64[2], zeroed by the caller before the first range).  All arithmetic on uint64, mod 2^64:
 *                     mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *                     w[j]   = the j-th little-endian 32-bit word of the row's dim * 2 bytes (element 2j in the low half), j < dim / 2
 *                     acc(r) = sum over j of mix( w[j] | ((j + 1) << 32) )
 *                     g(r)   = mix( acc(r) ^ ((row_base + r + 1) * 0x9E3779B97F4A7C15) )
 *                 Bits are hashed, not values.  A sum and an XOR over rows: the digest of a shard does not depend on how it is cut into
 *                 ranges or ranks (row_base = the global number of image row 0), and integer atomics give the same bits in any order.
 *                 The zero padding past n_rows_total never enters.
 * Both: n_chunk == 0 is a no-op returning 0; EMDR2_E_BADARG for null pointers, a dim outside the layout's envelope, or a range outside
 * [0, n_rows_total].
 */
int emdr2_mips_export_rows(const void *tiled, int64_t n_rows_total, int dim, int64_t row_offset, int64_t n_chunk, void *rows_rm,
                           emdr2_stream_t stream);
int emdr2_mips_digest_rows(const void *tiled, int64_t n_rows_total, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base,
                           uint64_t *digest, emdr2_stream_t stream);

/* Workspace bytes for emdr2_mips_search with up to n_q queries (per call) and this k. */
int emdr2_mips_workspace_bytes(int n_q, int dim, int k, size_t *bytes);

/*
 * Canonical top-k of one row shard.
 *   tiled     stripe-tiled shard image (emdr2_mips_pack_rows), n_rows valid rows, row_base = global
 *             row number of the shard's first row
 *   emax_sq   device float: upper bound of max_r ||E[r]||^2 (from pack_rows)
 *   queries   device fp16 [n_q, dim] row-major;  n_q >= 1 (internally processed 512 per pass)
 *   ids       optional device int32 [n_rows]: row -> doc id (reference id_map, emdr2_index.py:258-260);
 *             NULL: out_idx = global row number
 *   out_dist  device fp16  [n_q, k]   canonical scores, descending
 *   out_idx   device int32 [n_q, k]   doc ids (or rows)
 *   out_row   device int64 [n_q, k]   global row numbers (tie-break key for emdr2_mips_merge)
 *   out_flags device uint32 [n_q]     EMDR2_FLAG_* (0 = proven canonical)
 * Slots beyond the shard's row count are filled with dist = -inf, idx = -1, row = -1.
 */
int emdr2_mips_search(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq,
                      const void *queries, int n_q, int k, const int32_t *ids,
                      void *out_dist, int32_t *out_idx, int64_t *out_row, uint32_t *out_flags,
                      void *workspace, size_t workspace_bytes, emdr2_stream_t stream);

/* Workspace bytes for emdr2_mips_search_exact (n_sel queries at once). */
int emdr2_mips_exact_workspace_bytes(int64_t n_rows, int n_sel, size_t *bytes);

/*
 * All-exact search (integer arithmetic for every row) for the n_sel queries listed in
 * sel (device int32 [n_sel], indices into queries); overwrites rows sel[i] of the outputs and
 * clears their flags.  Slow (full index pass in integer arithmetic per 8 queries); correctness net.
 */
int emdr2_mips_search_exact(const void *tiled, int64_t n_rows, int dim, int64_t row_base,
                            const void *queries, int n_q, const int32_t *sel, int n_sel, int k,
                            const int32_t *ids, void *out_dist, int32_t *out_idx, int64_t *out_row,
                            uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                            emdr2_stream_t stream);

/*
 * Merge per-shard results after an all-gather: inputs are [n_shards, n_q, k] (shard-major),
 * outputs [n_q, k], ordered by (score desc, global row asc).  Deterministic and independent of
 * the number of shards.
 */
int emdr2_mips_merge(const void *dist_in, const int32_t *idx_in, const int64_t *row_in, int n_shards,
                     int n_q, int k, void *out_dist, int32_t *out_idx, int64_t *out_row,
                     emdr2_stream_t stream);

/*
 * FaissMIPSIndex-style twins (reference: megatron/data/emdr2_index.py:103-197 -- faiss.IndexFlatIP over fp16-stored vectors searched
 * with float32 queries that hold fp16 values, evaluate.py:49,123): score = RNE_fp32(exact dot), order (fp32 score desc, row asc).
 * Same pipeline, same validity proof in the fp32 key domain, fp32 distances out.  faiss itself is absent from /root/reference and
 * unpinned (docker/Dockerfile:26-28): parity is against the exact-arithmetic restatement oracle/mips_oracle.c:emdr2_oracle_topk_f32.
 */
int emdr2_mips_search_f32(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq,
                          const void *queries, int n_q, int k, const int32_t *ids,
                          float *out_dist, int32_t *out_idx, int64_t *out_row, uint32_t *out_flags,
                          void *workspace, size_t workspace_bytes, emdr2_stream_t stream);
int emdr2_mips_exact_workspace_bytes_f32(int64_t n_rows, int n_sel, size_t *bytes);
int emdr2_mips_search_exact_f32(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const void *queries, int n_q,
                                const int32_t *sel, int n_sel, int k, const int32_t *ids, float *out_dist, int32_t *out_idx,
                                int64_t *out_row, uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                                emdr2_stream_t stream);
int emdr2_mips_merge_f32(const float *dist_in, const int32_t *idx_in, const int64_t *row_in, int n_shards, int n_q, int k,
                         float *out_dist, int32_t *out_idx, int64_t *out_row, emdr2_stream_t stream);


/*
 * The sharded search's exchange format (replaces the reference's gather of per-device partial results + two broadcasts,
 * emdr2_index.py:284-295, emdr2_model.py:451-452): ONE 16-byte little-endian record per (query, slot),
 *     { int64 global row | int32 doc id | uint32 score bits (fp16 in the low half; fp32 when f32 != 0) },   row = id = -1 in empty slots.
 * emdr2_mips_search_records = emdr2_mips_search / _search_f32 whose last kernel writes records [n_q, k] -- i.e. straight into the send
 * buffer of the ONE all-gather of a search; emdr2_mips_merge_records = emdr2_mips_merge / _merge_f32 reading the gathered buffer
 * [n_shards, n_q, k] as it arrived; emdr2_mips_pack_records overwrites records rows sel[i] from (dist, idx, row) arrays (queries that the
 * all-exact path re-did).  records pointers are 16-byte aligned.
 */
int emdr2_mips_search_records(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq, const void *queries, int n_q,
                              int k, const int32_t *ids, int f32, void *out_records, uint32_t *out_flags, void *workspace,
                              size_t workspace_bytes, emdr2_stream_t stream);
int emdr2_mips_merge_records(const void *records_in, int n_shards, int n_q, int k, int f32, void *out_dist, int32_t *out_idx, int64_t *out_row,
                             emdr2_stream_t stream);
int emdr2_mips_pack_records(const void *dist, const int32_t *idx, const int64_t *row, const int32_t *sel, int n_sel, int k, int f32,
                            void *records, emdr2_stream_t stream);

/*
 * int8 shadow image: a second, int8 image of the shard in the stripe-tiled geometry plus three floats per 256-row
 * block, from which the long filter segments of a 129..512-query search run at the int8 MFMA rate behind a rigorous per-block error bound;
 * survivors are re-scored from the fp16 image before anything else sees them, so results are those of emdr2_mips_search bit for bit.
 *   _shadow_bytes     sizes of the image and of the block table (dim % 256 == 0)
 *   _seal_shadow      builds both from the FINISHED fp16 image (call again whenever the fp16 image changed); *nonfinite (device uint32,
 *                     caller zeroes) is set to 1 if the image holds an inf / NaN -- such a shard must not be searched with its shadow
 *   _search_shadow    emdr2_mips_search (f32 = 0), _search_f32 (f32 != 0) or, with out_records != NULL, _search_records, with filter segments
 *                     of at least shadow_min_rows rows taken on the shadow image
 *   _shadow_launches  number of int8 scan launches so far in this process (tests assert that the path really ran)
 */
int emdr2_mips_shadow_bytes(int64_t n_rows, int dim, size_t *image_bytes, size_t *table_bytes);
int emdr2_mips_seal_shadow(const void *tiled, int64_t n_rows, int dim, void *shadow, void *table, uint32_t *nonfinite, emdr2_stream_t stream);
int emdr2_mips_search_shadow(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq, const void *shadow,
                             const void *table, int64_t shadow_min_rows, const void *queries, int n_q, int k, const int32_t *ids, int f32,
                             void *out_dist, int32_t *out_idx, int64_t *out_row, void *out_records, uint32_t *out_flags, void *workspace,
                             size_t workspace_bytes, emdr2_stream_t stream);
int emdr2_mips_shadow_launches(void);

/*
 * The segment schedule of one search pass, read-only (host arithmetic alone: no launch, no GPU needed): what emdr2_mips_search and its
 * siblings would run for n_q queries (1..EMDR2_MAX_QUERIES_PER_PASS: one pass) over n_rows rows, as planned by csrc/mips_plan.h with the
 * library's built-in knobs.  shadow_min_rows < 0: a shard without a shadow image, else the argument of _search_shadow.  cus: the compute
 * units to plan for, 0 = those of the current device.  Segment i covers rows [row_end[i-1], row_end[i]) (from 0; the last ends at n_rows)
 * on engine[i], select_after[i] != 0: a select launch follows it, prog_slot[i]: the set of pair-progress counters a persistent launch
 * uses, or -1.  *pack_q8 != 0: the int8 query image is packed, i.e. the shard needs its shadow image.  n_rows == 0: no segments.
 * EMDR2_E_BADARG, with nothing written: a null output, a shape no search takes, cus < 0, or more segments than max_segments (32 always do).
 */
#define EMDR2_SCAN_DENSE 0           /* the first segment: every score written */
#define EMDR2_SCAN_LOCKSTEP 1        /* the filter scan of mips_scan.hip */
#define EMDR2_SCAN_PERSISTENT_F16 2  /* the persistent filter scan (mips_scan8.hip) */
#define EMDR2_SCAN_PERSISTENT_I8 3   /* ... on the int8 shadow image (mips_scan8i.hip) */
int emdr2_mips_search_plan(int64_t n_rows, int n_q, int dim, int k, int64_t shadow_min_rows, int cus, int max_segments, int *n_segments,
                           int64_t *row_end, int32_t *engine, int32_t *select_after, int32_t *prog_slot, int *pack_q8);

/*
 * In-place row updates of a FINISHED shard (the device counterpart of the reference store's add_block_data(..., allow_overwrite=True)):
 * every derived structure is left exactly as a fresh build of the same rows would leave it.
 *   _block_norm_bytes  size of the block-norm table: one float per 256-row block of the padded image
 *   _block_norms       (re)builds entries [first_block, first_block + n_blocks) from the image: entry b = max over the block's rows of
 *                      ||E[r]||_2^2 (rows past n_rows are zero).  Called once over the whole table before the first update.
 *   _update_rows       writes rows_rm (device fp16 [n_chunk, dim]) into image rows [row_offset, row_offset + n_chunk), rewrites the table
 *                      entries of the blocks they touch, sets *emax_sq to the maximum of the WHOLE table -- bit for bit what _pack_rows
 *                      leaves after a fresh build of the same rows, so it falls when the row that held the maximum is overwritten -- and,
 *                      with shadow != NULL, re-seals exactly the touched blocks of the int8 shadow image and its table with the arithmetic
 *                      of _seal_shadow, OR-ing 1 into *nonfinite (device uint32) if one of them holds an inf / NaN.  A few small launches
 *                      on `stream`; nothing allocated, no host synchronisation.  The caller orders it against searches of the shard.
 *                      n_chunk == 0 is a no-op.  shadow == NULL: table and nonfinite are ignored.
 *   _update_rows_scattered  the same update addressed by a LIST of rows (add_block_data takes a list of ids, not a range): rows_rm is device
 *                      fp16 [n_upd, dim], row_ids device int64 [n_upd], local rows in any order; entry i writes rows_rm[i] into image row
 *                      row_ids[i].  An entry whose id is outside [0, n_rows_total) is SKIPPED -- negative ids, ids past the end, ids that
 *                      fall into the zero padding up to the next multiple of 512 -- so a rank can be handed a gathered list that also names
 *                      rows of other shards without compacting it on the host.  The valid ids must be distinct; that is the caller's duty,
 *                      as ordering against searches is.  Otherwise the row holds a mix of the 16-byte segments of its sources (each segment
 *                      is one store of one source; which source wins a segment is not defined), and the derived structures describe
 *                      whatever mix was stored.  Afterwards the image, the touched entries of block_norm_sq, *emax_sq (the maximum of the
 *                      whole table, so it can fall) and, with shadow != NULL, the touched 256-row blocks of the int8 image and its table
 *                      are bit for bit what _pack_rows + _seal_shadow leave after a fresh build of the same rows; *nonfinite gets 1 OR-ed in
 *                      if a touched block holds an inf / NaN.  The norm and seal arithmetic is that of _update_rows, run over a device-side
 *                      list of the touched blocks instead of a range.  Nothing is allocated, no host synchronisation; one memset and at
 *                      most four launches on `stream`, whatever the list holds.  workspace: device memory, 16-byte aligned, at least
 *                      _scatter_workspace_bytes(n_rows_total, n_upd) bytes (one claim word per 256-row block of the padded image, a
 *                      counter, a block list of min(n_upd, blocks) entries); its contents need not be kept between calls.
 *                      n_upd == 0 is a no-op returning 0.  EMDR2_E_BADARG: null pointers, a bad dim, a misaligned table or workspace,
 *                      shadow without table / nonfinite; EMDR2_E_WORKSPACE: workspace_bytes too small.
 */
int emdr2_mips_block_norm_bytes(int64_t n_rows, size_t *bytes);
int emdr2_mips_block_norms(const void *tiled, int64_t n_rows, int dim, int64_t first_block, int64_t n_blocks, float *block_norm_sq,
                           emdr2_stream_t stream);
int emdr2_mips_update_rows(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, int64_t n_rows_total, void *tiled,
                           float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite, emdr2_stream_t stream);
int emdr2_mips_scatter_workspace_bytes(int64_t n_rows_total, int64_t n_upd, size_t *bytes);
int emdr2_mips_update_rows_scattered(const void *rows_rm, const int64_t *row_ids, int64_t n_upd, int dim, int64_t n_rows_total,
                                     void *tiled, float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite,
                                     void *workspace, size_t workspace_bytes, emdr2_stream_t stream);

/*
 * Generation stamps: one uint32 per local row of a shard, owned by the caller (device memory, n_rows_total words, 4-byte aligned) -- the
 * GENERATION of a row is the number of optimizer steps the weights that produced its embedding had taken; values are below 2^31.  The
 * library keeps no stamps of its own: a shard without them uses the entry points above, which are unchanged.
 *   _update_rows_stamped, _update_rows_scattered_stamped   _update_rows / _update_rows_scattered with four more arguments in front of the
 *                      stream: generation (the stamp array), gen, newest_wins, n_kept_newer (a device uint32 counter, or NULL).  For
 *                      every destination row r -- of the range; of the list, invalid ids skipped as above and never counted --
 *                        newest_wins == 0:  the row is written and generation[r] = gen;
 *                        newest_wins != 0:  the row is written and stamped gen iff generation[r] <= gen; otherwise neither the image
 *                                           row nor its stamp changes and *n_kept_newer, when given, goes up by one.
 *                      Ties write: two writers of one generation keep "the last one wins".  The rule is non-strict on purpose: the row
 *                      writers have one thread per 16-byte segment, and only under <= do all threads of a row take the same decision
 *                      whether they read the stamp before or after the segment-0 thread has stored gen (csrc/mips_aux.hip).
 *                      Everything behind the row write is the code of the unstamped forms over the same range / touched-block list
 *                      (a block of the list form whose rows were all left alone is not listed): block norms, *emax_sq as the maximum of the
 *                      whole table, the re-seal of the touched 256-row blocks, *nonfinite -- all recomputed from the image, so the
 *                      contract stands: afterwards the shard is byte for byte a fresh build of the rows it now holds.  The same
 *                      launches as the unstamped forms, nothing allocated, no host synchronisation; the counter is only ever added to
 *                      (the caller clears and reads it).  EMDR2_E_BADARG in addition: a null or misaligned generation, a misaligned
 *                      counter, gen >= 2^31.
 *   _generation_stats  one pass over stamps, report = device uint64[EMDR2_GEN_WORDS], 8-byte aligned, cleared by the call itself.
 *                      global_rows == NULL: all n_rows stamps (n_sel is ignored).  Otherwise the n_sel entries of global_rows (device
 *                      int64) that fall into [row_base, row_base + n_rows): other entries -- negative ones, rows of other shards -- are not
 *                      counted, a row named twice counts twice.  age = now - generation[r], taken as 0 where the stamp exceeds now.
 *                         0  count         rows covered
 *                         1  sum_age       sum of the ages
 *                         2  min_age       ~0 when count == 0
 *                         3  max_age
 *                         4  from_future   stamps > now (should be 0: such a row claims weights that do not exist yet)
 *                         5..36  histogram bin b = word 5 + b: bin 0 holds age 0, bin b ages in [2^(b-1), 2^b)
 *                      Integer atomics behind per-workgroup LDS tallies: the report does not depend on the order of the visit.  Two
 *                      launches on `stream`, nothing allocated, no host synchronisation.  n_rows == 0 or n_sel == 0: count 0, min_age ~0,
 *                      the rest 0, nothing is read.  EMDR2_E_BADARG: a null or misaligned report, a null generation with n_rows > 0,
 *                      n_rows < 0, row_base < 0, n_sel < 0 with a list.
 */
#define EMDR2_GEN_WORDS 37
int emdr2_mips_update_rows_stamped(const void *rows_rm, int64_t n_chunk, int dim, int64_t row_offset, int64_t n_rows_total, void *tiled,
                                   float *block_norm_sq, float *emax_sq, void *shadow, void *table, uint32_t *nonfinite,
                                   uint32_t *generation, uint32_t gen, int newest_wins, uint32_t *n_kept_newer, emdr2_stream_t stream);
int emdr2_mips_update_rows_scattered_stamped(const void *rows_rm, const int64_t *row_ids, int64_t n_upd, int dim, int64_t n_rows_total,
                                             void *tiled, float *block_norm_sq, float *emax_sq, void *shadow, void *table,
                                             uint32_t *nonfinite, void *workspace, size_t workspace_bytes, uint32_t *generation,
                                             uint32_t gen, int newest_wins, uint32_t *n_kept_newer, emdr2_stream_t stream);
int emdr2_mips_generation_stats(const uint32_t *generation, int64_t n_rows, int64_t row_base, const int64_t *global_rows, int64_t n_sel,
                                uint32_t now, uint64_t *report, emdr2_stream_t stream);

/*
 * Oldest rows: which rows of a shard a refresher should embed next, chosen on the device from the stamps alone.
 *   _oldest_rows       generation: the n_rows stamps of the shard.  A local row r is ELIGIBLE when generation[r] < below (below = the
 *                      generation of the weights about to embed it: a row that is not older than they are gains nothing).  The eligible
 *                      rows are ordered by (stamp ascending, row ascending), a total order; the SELECTED SET is the first
 *                      min(n_want, n_eligible) rows of it: the oldest stamps, and among the rows that share the cut stamp the
 *                      lowest-numbered ones.
 *                        out_rows   device int64[n_want], 8-byte aligned: the selected set as GLOBAL rows, row_base + r, in ASCENDING ROW
 *                                   order (the scattered writer's touched-block list stays short; with uniform stamps the list is the
 *                                   range row_base .. row_base + n_want - 1); every slot behind the set receives -1, which
 *                                   _update_rows_scattered skips
 *                        out_info   device uint64[4], 8-byte aligned, cleared by the call itself:
 *                                     0  n_selected
 *                                     1  n_eligible
 *                                     2  the largest stamp selected, ~0 when nothing was selected
 *                                     3  0
 *                      A radix select over the stamps (per-workgroup LDS histograms, integer atomics) and an ordered compaction over
 *                      per-workgroup slabs of consecutive rows: the result is a function of the stamps alone, not of the order the
 *                      workgroups run in nor of the grid.  No workgroup waits on another: the phases are separate launches, six at most,
 *                      on `stream`; nothing allocated, no host synchronisation.  The caller orders the call against writers of the
 *                      stamps.  workspace: device memory, 16-byte aligned, at least _oldest_rows_workspace_bytes(n_rows) bytes; its
 *                      contents need not be kept, nor cleared, between calls.
 *                      n_want == 0: the report only, out_rows may be NULL.  n_rows == 0: words 0, 1, 3 are 0 and word 2 is ~0, nothing
 *                      is read.  below == 0: nothing is eligible.  EMDR2_E_BADARG: a null or misaligned out_info, workspace or out_rows
 *                      (null only with n_want > 0), a misaligned generation or a null one with n_rows > 0, n_rows < 0 or >= 2^31,
 *                      row_base < 0, n_want < 0, n_want > n_rows; EMDR2_E_WORKSPACE: workspace_bytes too small.
 */
int emdr2_mips_oldest_rows_workspace_bytes(int64_t n_rows, size_t *bytes);
int emdr2_mips_oldest_rows(const uint32_t *generation, int64_t n_rows, int64_t row_base, uint32_t below, int64_t n_want,
                           int64_t *out_rows, uint64_t *out_info, void *workspace, size_t workspace_bytes, emdr2_stream_t stream);

/*
 * Index snapshots with stamps: the digest of the generation stamps of a row range, the companion of _digest_rows.
 *   _digest_stamps     generation: the n_rows_total stamps of the shard (4-byte aligned, nothing more is assumed).  For every local row r in
 *                      [row_offset, row_offset + n_chunk), with mix as for _digest_rows and all arithmetic on uint64, mod 2^64:
 *                          h(r) = mix( mix( generation[r] | (0x47454E53 << 32) ) ^ ((row_base + r + 1) * 0x9E3779B97F4A7C15) )
 *                      digest[0] += h(r) (wrap-around), digest[1] ^= h(r); digest is a device uint64[2], 8-byte aligned, zeroed by the
 *                      caller before the first range.  The tag keeps a stamp word apart from every row word of _digest_rows.  Bits are
 *                      hashed, not values.  A sum and an XOR over rows: the digest of a shard's stamps does not depend on how it is cut
 *                      into ranges or ranks (row_base = the global number of local row 0), and integer atomics give the same bits in
 *                      any order.  One launch on `stream` (scalar head and tail around 16-byte vector loads, grid-stride under a
 *                      workgroup cap, one 64-bit add and one 64-bit xor per workgroup); nothing allocated, no host synchronisation.  The
 *                      caller orders the call against writers of the stamps: on one stream, between the same two neighbours as the
 *                      _export_rows / _digest_rows of the same range, it hashes the stamps that belong to exactly the exported rows.
 *                      n_chunk == 0 is a no-op returning 0.  EMDR2_E_BADARG: a null or misaligned digest, a misaligned generation or a
 *                      null one with n_chunk > 0, a range outside [0, n_rows_total], row_base < 0.
 */
int emdr2_mips_digest_stamps(const uint32_t *generation, int64_t n_rows_total, int64_t row_offset, int64_t n_chunk, int64_t row_base,
                             uint64_t *digest, emdr2_stream_t stream);

/*
 * Incremental index snapshots: which rows of a shard differ from the rows a base snapshot holds, found from per-row keys.
 *   key(r) = g(r)                       on a shard without stamps (generation == NULL)
 *   key(r) = g(r) + h(r)  mod 2^64      on one with stamps
 * g is the row hash of _digest_rows and h the stamp hash of _digest_stamps, both numbered row_base + r: a row is CHANGED exactly when its
 * key differs from the key it had in the base, whoever wrote it -- a re-write of the same bits under a newer stamp included.  An
 * "unchanged" verdict is wrong only on a 64-bit collision.
 *   _row_keys          keys: device uint64[n_rows_total], 8-byte aligned; the slots [row_offset, row_offset + n_chunk) receive the keys of
 *                      those local rows, every other slot is left alone.  One launch on `stream`.  On one stream, between the same two
 *                      neighbours as the _export_rows / _digest_rows (/ _digest_stamps) of the same range, the keys are those of exactly
 *                      the exported bits.  n_chunk == 0 is a no-op returning 0.
 *   _changed_rows      ONE pass over the live image (it streams the shard once, like _digest_rows), then two small launches.
 *                        base_keys  device uint64[n_rows], 8-byte aligned: read, never written
 *                        out_rows   device int64[cap], 8-byte aligned: the GLOBAL rows row_base + r with key(r) != base_keys[r], in
 *                                   ASCENDING row order, the first min(n_changed, cap) of them; every slot behind receives -1
 *                        out_info   device uint64[8], 8-byte aligned; every word is written by the call:
 *                                     0     n_changed
 *                                     1     n_stored = min(n_changed, cap)
 *                                     2, 3  sum and xor of g(r) over ALL rows of the shard as they stand: the bits _digest_rows gives for
 *                                           the whole shard at the same stream point
 *                                     4, 5  the same for h(r) (_digest_stamps); 0 without stamps
 *                                     6     the smallest changed global row, ~0 when none
 *                                     7     0
 *                      The pass leaves per 128-row stripe a changed mask, a count and its digest words in the workspace; per-slab sums and
 *                      an ordered expansion of the masks at their global ranks follow.  Every workspace word a launch reads was stored by
 *                      one workgroup of the launch before: no atomics on global memory, nothing to clear, no workgroup waits on another,
 *                      and the output is a function of the image, the stamps and the keys alone -- not of the grid nor of the order the
 *                      workgroups run in.  Nothing allocated, no host synchronisation; the caller orders the call against writers of the
 *                      shard.  The zero padding past n_rows is read and never counted.  workspace: device memory, 16-byte aligned, at
 *                      least _changed_rows_workspace_bytes(n_rows) bytes; its contents need not be kept, nor cleared, between calls.
 *                      cap == 0: the report only, out_rows may be NULL.  n_rows == 0: zeros, word 6 is ~0, nothing is read.
 * EMDR2_E_BADARG: null or misaligned pointers (generation may be NULL: no stamps), a dim outside the layout's envelope, a range outside
 * the shard, row_base < 0, n_rows >= 2^31, cap < 0 or cap > n_rows; EMDR2_E_WORKSPACE: workspace_bytes too small.
 */
int emdr2_mips_row_keys(const void *tiled, int64_t n_rows_total, int dim, int64_t row_offset, int64_t n_chunk, int64_t row_base,
                        const uint32_t *generation, uint64_t *keys, emdr2_stream_t stream);
int emdr2_mips_changed_rows_workspace_bytes(int64_t n_rows, size_t *bytes);
int emdr2_mips_changed_rows(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const uint32_t *generation,
                            const uint64_t *base_keys, int64_t cap, int64_t *out_rows, uint64_t *out_info, void *workspace,
                            size_t workspace_bytes, emdr2_stream_t stream);

/*
 * Index audit: one streaming pass over a shard's LIVE images that re-checks the premises of the search's
 * proof from the stored bits and, separately, the "bit for bit a fresh build" contract of the derived structures -- emax_sq, the
 * block-norm table, the int8 shadow image and its {s_b, N_b, D_b} table, which pack_rows, seal_shadow, update_rows, update_rows_scattered
 * and an image swap all maintain.  It repairs nothing.
 *   tiled, n_rows, dim, row_base, emax_sq   as for _search
 *   block_norm_sq   the block-norm table of _block_norms, or NULL (words 4 and 5 stay 0)
 *   shadow, table   the int8 image and its table as _search_shadow takes them, or both NULL (words 7..11 stay 0)
 *   report          device uint64[EMDR2_AUDIT_WORDS], 8-byte aligned; the call clears it itself
 * Enqueued on `stream` (three launches), nothing allocated, no host synchronisation; the caller orders it against updates of the shard like
 * a search.  n_rows == 0: every counter 0 and both first-offender words ~0, nothing is read.  EMDR2_E_BADARG: null tiled, emax_sq or report,
 * a dim outside the layout's envelope, row_base < 0, shadow without table or table without shadow, a shadow with dim % 256 != 0.
 *
 * Report words.  SOUND words: a non-zero count means a search of this image may return a wrong top-k with flags == 0.  They are evaluated
 * in float64 from the stored bits -- the fp16 value widened exactly, the int8 byte as stored, s_b the stored float widened exactly -- and
 * share no arithmetic with the seal or the norm routine.  NO tolerance is added: the square of an fp16 value is exact in float64 and the
 * float64 sum of 8,192 of them is off by ~1e-12 relative, nine orders below the 0.1 % slack that every stored bound carries.  CANONICAL
 * words: the structure differs in bits from what the project's own routine gives for this image (the audit runs that routine -- the code of
 * _block_norms / _seal_shadow itself -- and compares instead of storing); the proof may still hold.  b = the 256-row block of row r.
 *    0  rows_checked               n_rows
 *    1  pad_rows_nonzero           rows of the fp16 image's zero padding (n_rows up to the next multiple of 512) with any bit set
 *    2  nonfinite_rows             rows holding an inf / NaN (a shard searched through its shadow must hold none); excluded from 3, 4, 8, 9
 *    3  rows_over_emax             sound: ||e_r||_2 > sqrtf(*emax_sq) * 1.001f, the bound formed in float exactly as the search's proof forms it
 *    4  block_norm_low             sound, with block_norm_sq: ||e_r||_2^2 > block_norm_sq[b] * 1.001^2 (the same slack: the table feeds emax_sq)
 *    5  block_norm_noncanonical    canonical, with block_norm_sq: blocks whose entry differs from _block_norms' value
 *    6  emax_noncanonical          canonical: 1 if *emax_sq differs from the maximum over the image's blocks of that value
 *    7  shadow_pad_rows_nonzero    rows past n_rows of the last sealed block of the int8 image (the seal covers ceil(n_rows / 256) blocks)
 *                                  with any byte set
 *    8  shadow_norm_low            sound: rows with ||e_r||_2 > N_b
 *    9  shadow_resid_low           sound: rows with ||e_r - s_b e8_r||_2 > D_b, e8_r = the stored bytes
 *   10  shadow_rows_noncanonical   canonical: rows of the sealed blocks whose int8 bytes differ from a fresh seal of the block
 *   11  shadow_table_noncanonical  canonical: blocks whose {s_b, N_b, D_b} differ from a fresh seal
 *   12  first_bad_row              the smallest GLOBAL row (row_base + local) counted in any of 1..4, 7..10; ~0 if none
 *   13  first_bad_block            the smallest local 256-row block counted in 5 or 11; ~0 if none
 *   14, 15  reserved, 0
 * Counters are integer atomics: the report does not depend on the order the blocks are visited in.
 */
#define EMDR2_AUDIT_WORDS 16
int emdr2_mips_audit(const void *tiled, int64_t n_rows, int dim, int64_t row_base, const float *emax_sq, const float *block_norm_sq,
                     const void *shadow, const void *table, uint64_t *report, emdr2_stream_t stream);

/* Diagnostics for tests: fp32 MFMA scores S~[n_q, n_rows] (row-major float) of the scan kernel's
 * arithmetic, for measuring |S~ - exact| against the bound used by the validity check. */
int emdr2_mips_debug_scores(const void *tiled, int64_t n_rows, int dim, const void *queries, int n_q,
                            float *out_scores, void *workspace, size_t workspace_bytes,
                            emdr2_stream_t stream);

/* Scan-kernel timing for bench.py's roofline: while enabled, emdr2_mips_search records a hipEvent
 * pair on `stream` around every scan launch (pool of 2048 pairs).  _set_timing(on/off) also resets
 * the pool; _timing_collect synchronises on the recorded events, returns per-launch
 * (milliseconds, index rows scanned by that launch) in launch order and resets the pool. */
int emdr2_mips_set_timing(int enabled);
int emdr2_mips_timing_collect(float *ms, int64_t *rows, int max_n, int *n_out);

#ifdef __cplusplus
}
#endif
#endif
