/*
 * vsearch_hip.h -- C ABI of libvsearch_hip.so: the MI355X (gfx950) implementation of vsearch's
 * vocabulary-space retrieval hot path.
 *
 * The reference (jzhoubu/vsearch @ 2024-12-18) is pure Python and has no FFI layer; the boundary it
 * offers is its Python API (src/ir/retriever/index.py, retriever.py, src/ir/utils/sparse.py,
 * src/ir/encoder/vdr.py).  This header is the boundary *below* that API: each entry point names the
 * reference call site (file:line under the reference root) whose arithmetic it replaces.  The
 * Python facade in vsearch_amd/ir/ (same class / method names as src/ir) binds these symbols
 * through ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - Plain C: pointers + explicit sizes, no C++ or torch types.  Returns 0 (VS_OK) or a negative
 *     VS_E* code; vs_last_error() gives the thread-local message.
 *   - Data pointers may be host or device (HIP) pointers; the library detects which
 *     (hipPointerGetAttributes).  Device pointers must belong to the index's device.
 *   - `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).  NULL = the
 *     device's null stream AND a blocking call: it returns after the work has completed.  With a
 *     non-NULL stream (hipStreamLegacy = (hipStream_t)1 names the null stream without blocking) and
 *     device pointers for every input and output, vs_index_search on the blocked-postings filter
 *     path (vs_index_info_t.last_path == 3: the default for large sparse / bag-of-token indexes)
 *     only enqueues kernels: tile plan, candidate proof and the exact pass for unproven queries are
 *     decided on the device.  The other paths (8-query CSR scan, fp64 walk, one-query scan)
 *     synchronise once per call to read the tile plan; host pointers are copied and block.
 *     vs_index_info() reads device-side statistics of the last search and therefore synchronises.
 *   - ONE search at a time per vs_index handle, from ONE host thread, on ONE stream at a time: the
 *     handle and a few per-device buffers (vs_merge_topk, the sparsify entry points) own grow-only
 *     scratch memory that consecutive calls re-use in stream order.  Calls on a different stream
 *     must be ordered after the previous call's work by the caller (event / synchronise).
 *   - Top-k order is canonical: score descending, then id ascending (torch.topk leaves ties
 *     unspecified, index.py:92).  fp32 accumulation order differs from MKL/cuSPARSE: scores agree to
 *     ~1e-6 relative; on binary index x dyadic query weights they are bit-exact.
 */
#ifndef VSEARCH_HIP_H
#define VSEARCH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_API __attribute__((visibility("default")))

/* error codes */
#define VS_OK            0
#define VS_EINVAL       -1   /* bad argument (Python facade: ValueError / TypeError)                   */
#define VS_ERANGE       -2   /* k > number of rows: torch.topk's RuntimeError (index.py:92)           */
#define VS_ENOMEM       -3   /* host or device allocation failed                                      */
#define VS_EHIP         -4   /* HIP runtime error (message has the hipError string)                   */
#define VS_EUNSUPPORTED -5   /* e.g. n_cols > 65535                                                   */
#define VS_ENODEVICE    -6   /* no usable gfx950 device: the product path never falls back to the CPU */

/* element types */
#define VS_F32   0
#define VS_F16   1
#define VS_I32   2
#define VS_I64   3
#define VS_U16   4
#define VS_U8    5
#define VS_NONE -1           /* "no values": binary (bag-of-token) index                              */

/* index kinds (IndexType, index.py:20-23) */
#define VS_KIND_DENSE 0
#define VS_KIND_CSR   1      /* SparseIndex / BoTIndex                                                */

typedef struct vs_index vs_index;

typedef struct vs_index_info_t {
    int32_t kind;            /* VS_KIND_*                                                             */
    int32_t store_dtype;     /* VS_F32 | VS_F16 | VS_NONE (binary)                                    */
    int64_t n_rows;
    int32_t n_cols;
    int32_t device;
    int64_t nnz;             /* logical non-zeros (CSR) or n_rows*n_cols (dense)                      */
    int64_t n_packets;       /* CSR device format: 8-nnz packets incl. row padding                    */
    int64_t device_bytes;    /* bytes of the device-resident index                                    */
    int64_t bytes_per_pass;  /* algorithmic HBM bytes one scoring pass streams      */
    int32_t lanes_per_row;   /* CSR scan geometry                                                     */
    int32_t queries_per_pass;/* Qt of the most recent search() (the planned default before any search)   */
    int64_t last_scan_bytes; /* bytes the scan kernels of the most recent search() had to read: passes x
                              * bytes_per_pass on the CSR paths; on the blocked-postings path the posting lists of
                              * the queries' columns (document ids + values) + their directory entries            */
    int64_t aux_bytes;       /* bytes of the blocked-postings copy (0 when absent)                      */
    int32_t last_path;       /* most recent search(): 0 = one query per pass, 1 = 8-query CSR scan, 2 = blocked postings
                              * (fp64 walk), 3 = blocked postings, fixed-point filter walk + exact refine               */
    int32_t last_fallbacks;  /* path 3: queries of the most recent search() whose top k the refine step could not prove from
                              * the filter's candidates and that were re-run on the exact walk (reading it synchronises)  */
    int64_t last_walk_postings; /* score terms (query weight x document value) the most recent walk accumulated: scatter-adds
                              * of posting lists + multiply-adds on the dense head strips                                 */
    int32_t head_columns;    /* columns of the blocked-postings copy kept as dense strips (option "postings_head")         */
    int32_t postings_state;  /* the blocked-postings copy: 0 = not attempted yet, 1 = built, 2 = NOT built: no room in HBM (sparse
                              * queries take the ~10x slower CSR scan), 3 = NOT built: a block holds more records than a directory
                              * word addresses, 4 = not wanted (small / short-row index, or option "blocked_postings" = 0)          */
    int32_t postings_walk;   /* which walk serves the filter on the copy that was built: 0 = list walk over 8-posting records,
                              * 4 = quad walk over 64-cell chunks (the default of a valued index), 5 = bag-of-token walk;
                              * -1 = no copy                                                                                     */
    int32_t last_packed_tiles; /* path 3 on bag-of-token chunks: query tiles of the most recent search() that took the packed walk (four slots
                              * on 16-bit sums, option "postings_packed"); the other tiles ran two int32 slots each                     */
    int64_t n_live;          /* rows not deleted (vs_index_delete_rows): n_rows on a handle without tombstones.  The count lives on the device:
                              * reading it synchronises once the handle has tombstones                                                     */
} vs_index_info_t;

/* ---- library ------------------------------------------------------------------------------- */
VS_API int          vs_version(void);
VS_API const char*  vs_last_error(void);
VS_API int          vs_device_count(int32_t* out);

/* ---- index containers: Index / SparseIndex / BoTIndex (index.py:25-218) ---------------------- */

/* Builds the device-resident CSR index from a torch/scipy-style CSR (what SparseIndex.init_index
 * assembles at index.py:163-179 and build_index at retriever.py:299-312).  Inputs are copied; the
 * library owns its own device format (row-padded 8-nnz packets: uint16 column ids, fp32/fp16/no
 * values, uint32 packet row pointers).
 *   rowptr_dtype, col_dtype: VS_I32 | VS_I64.   val_dtype: VS_F32 | VS_F16; values == NULL -> binary.
 *   store_dtype: VS_F32 | VS_F16 | VS_NONE -- dtype streamed by search (fp16 = the reference's
 *   `fp16=True` load default, index.py:135,176; VS_NONE asserts every value == 1).              */
VS_API int vs_index_create_csr(const void* rowptr, int rowptr_dtype, const void* colidx, int col_dtype,
                               const void* values, int val_dtype, int store_dtype,
                               int64_t n_rows, int32_t n_cols, int device, vs_index** out);

/* Shard-by-shard construction: what SparseIndex.init_index does with `vstack(shards)` (index.py:172-175),
 * without ever holding the concatenation on the host.  Reserve capacity (rows, 8-nnz packets: a row of
 * `len` entries takes ceil(len / 8)), then append CSR row blocks in order; rows become searchable as they
 * are appended.                                                                                       */
VS_API int vs_index_create_reserved(int64_t rows_cap, int64_t packets_cap, int32_t n_cols, int store_dtype, int device, vs_index** out);
VS_API int vs_index_append_csr(vs_index* index, const void* rowptr, int rowptr_dtype, const void* colidx, int col_dtype,
                               const void* values, int val_dtype, int64_t n_rows);

/* Row-range sharding ("per-shard npz or row ranges"): rows [row0, row0 + n_rows) of a CSR index as a NEW
 * index on GPU `device` -- the packets are copied device to device (a peer copy across GPUs).  The reference joins its shard files
 * with vstack (index.py:172-175) and keeps ONE matrix on one device; SparseIndex(index_file=<one file>, devices=N) and
 * Retriever.build_index(..., devices=N) deal that one matrix out in contiguous row ranges with this call.                      */
VS_API int vs_index_slice_rows(const vs_index* index, int64_t row0, int64_t n_rows, int device, vs_index** out);

/* Native shard files (".vsx"): the device format written / read verbatim.  SparseIndex.init_index re-parses,
 * slices and vstacks scipy .npz shards on every load (index.py:172-176); a .vsx file is a header + the three
 * device arrays, so a 97 GB index loads at storage speed.                                                */
/* scipy.sparse.save_npz shards read natively (SparseIndex.init_index: load_npz(f)[:, shift:] per shard, then
 * vstack, index.py:172-175).  A .npz is a ZIP archive (stored or deflated members, ZIP64 for members beyond 4 GB) of .npy arrays
 * indptr / indices / data / shape / format; only format "csr" is read (anything else: VS_EUNSUPPORTED -- the Python facade then
 * falls back to scipy).  No GPU is touched by vs_npz_inspect.
 *   vs_npz_inspect: shape of the shard and what remains after the column shift -- columns below `shift` are dropped, n_cols
 *     is reported after the shift; `packets` = 8-nnz packets of the device format (what vs_index_create_reserved needs).
 *   vs_index_append_npz: appends the shard's rows to a reserved CSR index (columns shifted and sorted within a row; a binary
 *     index -- store VS_NONE -- requires every stored value == 1).                                                            */
VS_API int vs_npz_inspect(const char* path, int32_t shift, int64_t* n_rows, int64_t* n_cols, int64_t* nnz, int64_t* packets);
VS_API int vs_index_append_npz(vs_index* index, const char* path, int32_t shift);
/* SparseIndex.save (index.py:181-202): the index as a scipy.sparse.save_npz file that scipy.sparse.load_npz reads back -- CSR,
 * int64 indptr / indices (the reference's torch CSR has int64 ids), fp32 data (all 1 for a binary index).  compressed = 0:
 * stored members; 1: deflate (level 1).  ZIP64 records are written where a member or an offset passes 4 GB.                  */
VS_API int vs_index_save_npz(const vs_index* index, const char* path, int compressed);
VS_API int vs_index_save_native(const vs_index* index, const char* path);
VS_API int vs_index_load_native(const char* path, int device, vs_index** out);

/* Dense index (Index.vector = [n_rows, n_cols], index.py:25-44, retriever.py:292-297). */
VS_API int vs_index_create_dense(const void* mat, int dtype, int store_dtype, int64_t n_rows, int32_t n_cols,
                                 int64_t ld, int device, vs_index** out);

/* Sparsity-aware variant: when the matrix density is <= max_density (a dense index of VDR embeddings holds
 * <= 768 non-zeros per 29 523-wide row) the rows are stored as CSR packets and searched by the CSR scan --
 * identical dot products, ~2.6 % of the bytes, none of the dense flops.  vs_index_info still reports
 * VS_KIND_DENSE and vs_index_export_dense works.  max_density <= 0 == vs_index_create_dense.             */
VS_API int vs_index_create_dense_auto(const void* mat, int dtype, int store_dtype, int64_t n_rows, int32_t n_cols,
                                      int64_t ld, double max_density, int device, vs_index** out);

/* Synthetic corpus generated straight into the device format (bench / tests; no reference
 * counterpart).  Rows are the pure function of (seed, global row id) defined in
 * vsearch_amd/synth.py; this shard holds rows [row0, row0 + n_rows).
 *   kind: 0 = fixed `nnz` per row with values, uniform columns; 1 = bag-of-token lengths (binary);
 *         2 = fixed `nnz`, column popularity ~ 1 / rank (Zipf s = 1, the most popular ~127 columns in every row).  */
VS_API int vs_index_create_synthetic(uint64_t seed, int64_t row0, int64_t n_rows, int32_t n_cols, int32_t nnz,
                                     int kind, int val_law, int store_dtype, int device, vs_index** out);

/* Index.search (index.py:88-94):  q.to(device).type(vector.dtype); matmul(q, vector.t()); topk(k).
 *   q: dense [B, n_cols] row-major with leading dimension ldq (elements), q_dtype VS_F32 | VS_F16.
 *   out_ids [B,k] int64 (row ids + id_offset), out_scores [B,k] fp32, descending.
 *   Returns VS_ERANGE when k > n_rows (the reference raises RuntimeError there).                 */
VS_API int vs_index_search(vs_index* index, const void* q, int q_dtype, int64_t ldq, int32_t B, int32_t k,
                           int64_t id_offset, int64_t* out_ids, float* out_scores, void* stream);

/* Filtered search (no reference counterpart: the reference can only search a larger k and drop hits): what vs_index_search returns over
 * the index that holds only the ALLOWED rows, bit for bit, with ids mapped back to the full index (+ id_offset), in the canonical order.
 *   filter: a bitmap of uint32 words -- bit i is bit i & 31 of word i >> 5; row r is allowed for query b iff bit filter_bit0 + r of the
 *   bitmap at filter + b * filter_ld is set.  filter_ld = 0: one bitmap for the whole batch; else >= the (filter_bit0 + n_rows + 31) / 32
 *   words a bitmap spans.  Host pointer, or device pointer on the index's device (as q).  filter == NULL: exactly vs_index_search.
 *   Fewer than k allowed rows: the positions behind them hold id -1, score -inf (an empty filter returns only those).  k > n_rows is
 *   still VS_ERANGE.  Every path gates candidate admission inside its kernels (k does not grow); with device pointers and a non-NULL
 *   stream the blocked-postings filter path (last_path == 3) only enqueues work, as vs_index_search does.                        */
VS_API int vs_index_search_filtered(vs_index* index, const void* q, int q_dtype, int64_t ldq, int32_t B, int32_t k,
                                    const uint32_t* filter, int64_t filter_bit0, int64_t filter_ld,
                                    int64_t id_offset, int64_t* out_ids, float* out_scores, void* stream);

/* Range search (no reference counterpart: the reference only has topk): every document scoring at least a threshold, counted.
 * For query b a row r MATCHES iff it is live (not deleted), the filter allows it, and score(b, r) >= thr[b] compared as fp32 floats (-0.0 and
 * +0.0 are equal).  score is the library's exact numerics and nothing else, whichever kernel serves the call: q rounded to the index dtype
 * as in vs_index_search, score = fl32(sum over the row's columns of fp64(fl32(q[c] * v[c]))), v = 1 on a binary index -- bit-identical to
 * vs_index_explain's score of the pair and independent of the summation order; an empty row scores +0.0 (it matches thr <= 0).  A dense
 * index on the matrix cores uses its own fp32 search score instead (what vs_index_search returns for the pair).
 *   thr [B] fp32.  -inf matches every live, allowed row; +inf none.  NaN: VS_EINVAL for a host array; on the device it matches no row.
 *   out_count [B] int64 (may be NULL): the number of matching rows -- exact whatever max_hits is.
 *   out_ids / out_scores [B, max_hits]: the first max_hits matches in the canonical order (score descending, id ascending; ids + id_offset):
 *     the complete match set when count <= max_hits, else its top max_hits; id -1 / score -inf behind the matches; every slot is written.
 *     max_hits in 0..VS_RANGE_MAX_HITS (VS_EINVAL beyond); max_hits > n_rows is allowed (this is no top-k: no VS_ERANGE); max_hits = 0 is
 *     count-only / bitmap-only, and the two pointers may then be NULL.
 *   out_words [B, ld_words] uint32 (may be NULL): the match bitmap in the layout of vs_index_search_filtered -- bit r of query b's row is set
 *     iff row r matches; words [0, (n_rows + 31) / 32) of each row are written whole, bits past n_rows are 0, ld_words >= that many words.
 *     The uncapped result: it can be passed back as a filter.
 *   filter / filter_bit0 / filter_ld: as vs_index_search_filtered; NULL = every live row.
 * Pointers: all host (staged; the call blocks), or all device on the index's device (VS_EINVAL for a mix).  With device pointers and a
 * non-NULL stream the one-query scan and the dense index only enqueue; the tile scan reads its tile plan back first, as vs_index_search does.
 * A CSR-packet index is served by the 8-queries-a-pass tile scan when the batch qualifies for tiles (as in vs_index_search; option
 * queries_per_pass = 1 turns it off) and max_hits <= 512, else by a one-query scan, one wave per row; both give identical bits.  The blocked
 * postings are never used.  A CSR-packet index wider than the LDS query image (n_cols > 32763): VS_EUNSUPPORTED.                          */
#define VS_RANGE_MAX_HITS 2048
VS_API int vs_index_search_range(vs_index* index, const void* q, int q_dtype, int64_t ldq, int32_t B, const float* thr, int32_t max_hits,
                                 const uint32_t* filter, int64_t filter_bit0, int64_t filter_ld, int64_t id_offset, int64_t* out_ids,
                                 float* out_scores, int64_t* out_count, uint32_t* out_words, int64_t ld_words, void* stream);

/* The scan plan the most recent vs_index_search_range took on this handle (its last sub-batch): the row chunks a query's (or a tile's)
 * scan was cut into and the rows of a chunk -- the last chunk holds the rest.  0 / 0 before the first range search; 1 chunk on a dense index. */
VS_API int vs_index_last_range_plan(const vs_index* index, int32_t* out_chunks, int64_t* out_rows_per_chunk);

/* Boosted search (no reference counterpart: the reference only has topk): vs_index_search_range with a BOOSTED score in the place of the
 * score -- relevance plus (or times) a weighted sum of up to VS_BOOST_MAX_FIELDS numeric fields, exact: every live, allowed row is scored, so
 * with thr = -inf and max_hits = k the list is the exact top k by boosted score, not a rescore window of a deeper top-k.
 * One numerics, reproducible bit for bit (csrc/boost_check.h: boost_apply).  For query b and row r:
 *   S    = the fp64 sum vs_index_search_range holds before its rounding: sum over the row's columns of fp64(fl32(q[c] * v[c])), q rounded to the
 *          index dtype, v = 1 on a binary index (fl32(S) is that call's score); a row without packets has S = +0.0.  A dense index on the
 *          matrix cores: S = fp64(its own fp32 search score).
 *   t_j  = +0.0 if weights[b, j] == 0 or row r has no value in field j (NaN / INT32_MIN), else fp64(weights[b, j]) * fp64(fields[j][r]) --
 *          exact in fp64.
 *   VS_BOOST_ADD: x = (((S + t_0) + t_1) + ...), fp64 additions in field order.   VS_BOOST_MUL: u = (((1.0 + t_0) + t_1) + ...), x = S * u.
 *   boosted(b, r) = fl32(x), -0.0 read as +0.0.  x NaN (an infinite value met its opposite, or S = 0): the row matches nothing for query b.
 * With every weight 0 the call is vs_index_search_range bit for bit in both modes, whatever the fields hold; a missing value is neutral.
 *   fields [n_fields]: HOST table of pointers to the value arrays [n_rows] (fp32 or int32, the layout of vs_value_*); field_dtypes [n_fields]:
 *     HOST array of VS_VAL_F32 | VS_VAL_I32; n_fields in 1..VS_BOOST_MAX_FIELDS; weights fp32 [B, n_fields]; mode VS_BOOST_ADD | VS_BOOST_MUL.
 *   thr [B] is a floor on the boosted score (NULL: -inf, every live, allowed row whose boosted score is not NaN).  out_count, out_ids /
 *     out_scores (the boosted scores; canonical order: boosted descending, id ascending), max_hits, out_words, filter, id_offset: as
 *     vs_index_search_range.
 * Pointers: q, thr, filter, the outputs, the value arrays and weights are all host or all device on the index's device.  Host weights must be
 * finite and a host thr not NaN (VS_EINVAL); on the device a NaN weight or a NaN thr makes its query match nothing, other non-finite weights go
 * through the arithmetic as written.  n_fields outside 1..4, an unknown mode or dtype, a NULL field pointer: VS_EINVAL before any device work;
 * a CSR-packet index with n_cols > 32763: VS_EUNSUPPORTED.  Routing as vs_index_search_range (tile scan when the batch qualifies and max_hits
 * <= 512, else the one-query scan; identical bits); a disallowed or deleted row loads no value.  vs_index_last_range_plan reports its plan.
 * Not covered: the blocked postings (their filter proves a top k of q.p, not of a boosted score: every call is an exact scan, one index pass
 * per 8 queries), boosts in the grouped / diverse / fused searches and in vs_index_set_scores, decay functions (derive the field and store
 * it), 64-bit values, more than 4 fields.                                                                                                    */
#define VS_BOOST_ADD 0
#define VS_BOOST_MUL 1
#define VS_BOOST_MAX_FIELDS 4
VS_API int vs_index_search_boosted(vs_index* index, const void* q, int q_dtype, int64_t ldq, int32_t B, const float* thr, int32_t max_hits,
                                   const uint32_t* filter, int64_t filter_bit0, int64_t filter_ld, int64_t id_offset, int64_t* out_ids,
                                   float* out_scores, int64_t* out_count, uint32_t* out_words, int64_t ld_words, const void* const* fields,
                                   const int32_t* field_dtypes, int32_t n_fields, const float* weights, int mode, void* stream);

/* ---- facet counts: how a document set spreads over per-row integer labels (no reference counterpart: the reference only has topk) ----------
 * The set of query b is a bitmap in the layout of vs_index_search_filtered: bit bit0 + r of the bitmap at words + b * ld_words stands for row
 * r (ld_words = 0: one bitmap for all queries, and then B must be 1; else ld_words >= the (bit0 + n_rows + 31) / 32 words a bitmap spans).
 * words == NULL: every row is set (B must be 1).  and_words (may be NULL): a second bitmap shared by all queries, at the same bit0.  Row r is
 * IN for query b iff its bit is set in words and in and_words; bits at or past bit0 + n_rows are ignored, whatever they hold.
 *   labels [n_rows] int32, n_labels >= 1.  total [b] = rows in; counts [b, l] = rows in with labels[r] == l, 0 <= l < n_labels; other [b] =
 *   rows in whose label is outside [0, n_labels) (-1 = "no label", anything too large): no label value causes an out-of-range access, and
 *   sum over l of counts [b, l] + other [b] == total [b] always.  counts [B, ld_counts] (ld_counts >= n_labels; elements [b, 0 .. n_labels)
 *   are written), total [B], other [B]: int64, every element written.  n_rows in 1 .. 2^32 - 1 (a count fits 32 bits).
 * A workgroup owns a chunk of rows and a tile of qt queries; it reads the bitmap words coalesced, skips all-zero spans without touching the
 * labels and loads a row's label once for the tile.  Two regimes (vs_facet_plan): qt x n_labels <= VS_FACET_LDS_BINS -- one uint32 histogram
 * per query of the tile in LDS, non-zero bins added to counts at the end of the chunk (qt the largest of 8, 4, 2, 1 that fits; 1 for a
 * shared bitmap); n_labels > VS_FACET_LDS_BINS -- 64-bit atomic adds straight into counts (qt = 8, or 1 for a shared bitmap).
 * vs_facet_plan: the launch of vs_facet_counts for these arguments -- pure host arithmetic, no device needed.  regime 0 = LDS, 1 = global;
 *   chunks x rows_per_chunk >= n_rows > (chunks - 1) x rows_per_chunk.  rows_per_chunk = 0: automatic; any other value must be a positive
 *   multiple of 64 and is taken as given (a tuning knob; the result does not depend on it).  vs_facet_counts / vs_index_facet_counts take the
 *   same argument and launch exactly this plan.
 * vs_index_facet_counts: vs_facet_counts over the index's rows with its tombstones as and_words: deleted rows never count.  words == NULL: the
 *   label distribution of the live index.
 * vs_facet_topn: per query the n labels with the largest counts [B, ld_counts] -- count descending, then label ascending; only labels with
 *   count >= max(min_count, 1); unused slots hold label -1 / count 0, every slot of out_labels int32 [B, n] / out_counts int64 [B, n] is
 *   written.  n in 1..VS_FACET_MAX_TOPN, n > n_labels is allowed; counts are below 2^32 (what vs_facet_counts writes).  One workgroup per query.
 * Errors: NULL labels or outputs, n_labels < 1, n out of range, rows_per_chunk no multiple of 64, B > 1 with ld_words = 0, ld_words too short:
 * VS_EINVAL -- checked before the device is touched (without a GPU a bad argument is VS_EINVAL, a good one VS_ENODEVICE).  Pointers: all
 * host (staged; the call blocks), or all device pointers on `device` / the index's device (VS_EINVAL for a mix); device pointers and a
 * non-NULL stream only enqueue.
 * Not covered: no index file stores labels, and a shard group has no entry point of its own (every shard counts its rows with its slice of
 * the labels and its bit range of the bitmap; the counts are summed, and the top-n taken after the sum); the one-process-per-GPU RCCL path
 * has none.                                                                                                                              */
#define VS_FACET_LDS_BINS 16384      /* uint32 bins of a workgroup's LDS histograms (64 KiB: two workgroups a CU) */
#define VS_FACET_MAX_TOPN 1024       /* labels vs_facet_topn lists per query at most */
VS_API int vs_facet_plan(int64_t n_rows, int32_t B, int32_t n_labels, int per_query, int64_t rows_per_chunk, int32_t* out_regime,
                         int32_t* out_qt, int64_t* out_chunks, int64_t* out_rows_per_chunk);
VS_API int vs_facet_counts(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const int32_t* labels,
                           int64_t n_rows, int32_t n_labels, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* total,
                           int64_t* other, int device, void* stream);
VS_API int vs_index_facet_counts(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                 int32_t n_labels, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* total, int64_t* other,
                                 void* stream);
VS_API int vs_facet_topn(const int64_t* counts, int64_t ld_counts, int32_t B, int32_t n_labels, int32_t n, int64_t min_count,
                         int32_t* out_labels, int64_t* out_counts, int device, void* stream);

/* ---- term aggregations: what a document set is about (no reference counterpart: the reference only has topk) ---------------------------------
 * For any set of rows of a CSR-packet index: how many of them HAVE each vocabulary column (vs_index_term_counts, vs_index_term_counts_ids), and
 * which columns are over-represented in the set against a background (vs_term_topn: "significant terms").
 * A row has column c under the definition of the term constraints (vs_index_term_bitmaps): it stores c with a non-zero value.  An fp16 store widens exactly; a
 * binary index stores 1, so every stored cell counts; a stored +0.0 or -0.0 does not count; the packets' padding column n_cols never counts.
 *   counts [B, ld_counts] int64, ld_counts >= n_cols: counts [b, c] = rows of query b's set that have column c.  Every element of
 *   counts [:, 0 .. n_cols) is written, columns [n_cols, ld_counts) are not touched.  total [B] int64: the rows of the set, every element written.
 * vs_index_term_counts (bitmap driven): row membership is exactly that of vs_index_facet_counts -- bit bit0 + r of the bitmap at words + b *
 *   ld_words stands for row r; ld_words = 0: one shared bitmap, and then B must be 1 (else ld_words >= the (bit0 + n_rows + 31) / 32 words a
 *   bitmap spans); words == NULL: every row is set (B must be 1); the handle's live bitmap is ANDed in at bit 0 whatever bit0 is (deleted rows
 *   never count); bits at or past bit0 + n_rows are ignored whatever they hold.  words == NULL is the document frequency of all columns over the
 *   live index in one pass.
 * vs_index_term_counts_ids (id-list driven): ids [B, ld] int64 with m entries a query (ld >= m), row = id - id_offset: the terms of a hit list
 *   without a bitmap.  Id -1 is skipped; a deleted row is skipped; AN ID LISTED TWICE COUNTS TWICE; total [b] = the entries counted.  An id
 *   outside the index (row outside [0, n_rows)): strict = 1 -- VS_EINVAL for a host list, the entry is skipped for a device list (device ids
 *   are not read on the host); strict = 0 -- skipped silently (what a shard passes for ids it does not own).
 * A workgroup owns a chunk of rows (a slice of a list) and one query; it walks the bitmap in 2048-row spans, leaves an all-zero span at once,
 * skips a 64-row step with no bit set, and streams the packets of the set rows: a lane takes one 16-byte packet of 8 column ids and reads the
 * values only where the store has them.  Two regimes (vs_term_plan): n_cols <= VS_TERM_LDS_COLS -- one uint32 histogram of all columns in the
 * workgroup's LDS (the 29 523 columns of the BERT vocabulary are 118 KB of a CU's 160 KiB), non-zero bins added to counts at the end of the chunk;
 * wider (up to the 65 535 columns a packet can name) -- 64-bit atomic adds straight into counts.
 * vs_term_plan: the launch of the two calls for these arguments -- pure host arithmetic, no device needed.  n_rows: the index's rows (for the
 *   id-list call: the m entries of a query, with per_query = 1 and rows_per_chunk = 0).  regime 0 = LDS, 1 = global; chunks x rows_per_chunk >=
 *   n_rows > (chunks - 1) x rows_per_chunk.  rows_per_chunk = 0: automatic (B x chunks ~ 4 workgroups a CU, a chunk at least 2048 rows); any
 *   other value must be a positive multiple of 64 and is taken as given (a tuning knob: the result never depends on the plan).
 * vs_term_topn: per query the n most significant columns of counts [B, ld_counts] / total [B] against the background bg [n_cols] int64 (shared
 *   by the batch) / bg_total.  Column c is a candidate iff fg = counts [b, c] >= max(min_count, 1), bg [c] > 0, total [b] > 0 and bg_total > 0.
 *   In fp64, each operation rounded once (no contraction): fgp = double(fg) / double(total [b]), bgp = double(bg [c]) / double(bg_total);
 *     VS_TERM_LIFT: s = fgp / bgp;     VS_TERM_JLH: a candidate only if fgp > bgp, s = (fgp - bgp) * (fgp / bgp).
 *   Order: float(s) descending, then column ascending -- two columns whose scores round to the same fp32 are ordered by the column.  out_cols
 *   int32 / out_score fp32 / out_fg int64 / out_bg int64, all [B, n], every slot written: -1 / -inf / 0 / 0 behind the last candidate.  n in
 *   1..VS_TERM_MAX_TOPN, n > n_cols is allowed.  One workgroup per query.  Ordering by the raw count is no method here (an fp32 score cannot
 *   order counts above 2^24 exactly): vs_facet_topn over counts does that on the exact integers.
 * Errors: NULL handle or outputs, B < 1, rows_per_chunk no multiple of 64, B > 1 with ld_words = 0, ld_words / ld / ld_counts too short, m < 1,
 * n or method out of range, chunks x B beyond 2^31 - 1 work items: VS_EINVAL -- checked before the device is touched (without a GPU a bad argument is VS_EINVAL, a good one
 * VS_ENODEVICE).  Pointers: all host (staged; the call blocks), or all device pointers on the index's device / `device` (VS_EINVAL for a mix);
 * device pointers and a non-NULL stream only enqueue.  A dense index on the matrix cores keeps no packets: VS_EUNSUPPORTED.
 * Weight sums and centroids per column: vs_index_term_sums below (column tiles of 64-bit bins).  Not covered: the dense
 * matrix kind; a shard group has no entry point of its own (every shard counts its bit range of the bitmap, or the ids with strict = 0 and its
 * id_offset; counts and total are summed, and the top-n taken after the sum) and the one-process-per-GPU RCCL path has none; a cached
 * background; scores that need a logarithm (PMI, tf-idf): they would not be bit-reproducible.                                               */
#define VS_TERM_LDS_COLS 36864       /* columns of a workgroup's LDS histogram (144 KiB of uint32 bins; the rest of the 160 KiB: counters) */
#define VS_TERM_MAX_TOPN 1024        /* columns vs_term_topn lists per query at most */
#define VS_TERM_LIFT 0
#define VS_TERM_JLH 1
VS_API int vs_term_plan(int64_t n_rows, int32_t B, int32_t n_cols, int per_query, int64_t rows_per_chunk, int32_t* out_regime,
                        int64_t* out_chunks, int64_t* out_rows_per_chunk);
VS_API int vs_index_term_counts(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, int64_t rows_per_chunk,
                                int64_t* counts, int64_t ld_counts, int64_t* total, void* stream);
VS_API int vs_index_term_counts_ids(vs_index* index, const int64_t* ids, int32_t B, int64_t m, int64_t ld, int64_t id_offset, int strict,
                                    int64_t* counts, int64_t ld_counts, int64_t* total, void* stream);
VS_API int vs_term_topn(const int64_t* counts, int64_t ld_counts, const int64_t* total, int32_t B, int32_t n_cols, const int64_t* bg,
                        int64_t bg_total, int method, int32_t n, int64_t min_count, int32_t* out_cols, float* out_score, int64_t* out_fg,
                        int64_t* out_bg, int device, void* stream);

/* ---- term sums: how much weight a document set puts on each column -- its centroid in vocabulary space (no reference counterpart) ----------------
 * For any set of rows of a CSR-packet index: the sum of the stored values of each vocabulary column over the set (vs_index_term_sums,
 * vs_index_term_sums_ids), and the columns with the largest mean weight (vs_term_sum_topn).  Integers throughout, so that a sum spread over many
 * workgroups does not depend on the order of its additions and every result compares exactly.
 * Per cell: a stored cell of value v (fp16 widened exactly; a binary index stores 1) contributes
 *     fx(v) = llrint(double(clamp(v, -2^VS_TERM_FX_CLAMP_LOG2, +2^VS_TERM_FX_CLAMP_LOG2)) * 2^VS_TERM_FX_SHIFT)
 *   rounded to nearest even; NaN contributes 0; +-inf clamp like any large value.  Every fp16 value, subnormals included, is a multiple of 2^-24:
 *   fp16 and binary stores are summed exactly, an fp32 value is rounded to 2^-24 absolute.  A cell is at most 2^44 in magnitude, so at least 2^19
 *   saturated rows fit before an int64 wraps; SUMS WRAP MODULO 2^64 (two's complement, as numpy's int64 does).
 *   sums [B, ld_sums] int64, ld_sums >= n_cols: sums [b, c] = the sum of fx(v) over the stored cells (r, c) of the rows r of query b's set.  The
 *   packets' padding column n_cols never contributes; a stored +0.0 or -0.0 contributes 0.  Every element of sums [:, 0 .. n_cols) is written,
 *   columns [n_cols, ld_sums) are not touched.  total [B] int64: the rows of the set, every element written.  sums * 2^-24 / total is the centroid.
 * vs_index_term_sums (bitmap driven): row membership is exactly that of vs_index_term_counts -- bit bit0 + r of the bitmap at words + b *
 *   ld_words stands for row r; ld_words = 0: one shared bitmap, and then B must be 1 (else ld_words >= the (bit0 + n_rows + 31) / 32 words a
 *   bitmap spans); words == NULL: every row is set (B must be 1); the handle's live bitmap is ANDed in at bit 0 whatever bit0 is (deleted rows
 *   never contribute); bits at or past bit0 + n_rows are ignored whatever they hold.
 * vs_index_term_sums_ids (id-list driven): ids [B, ld] int64 with m entries a query (ld >= m), row = id - id_offset.  Id -1 is skipped; a deleted
 *   row is skipped; AN ID LISTED TWICE COUNTS TWICE; total [b] = the entries counted.  An id outside the index (row outside [0, n_rows)): strict = 1
 *   -- VS_EINVAL for a host list, the entry is skipped for a device list (device ids are not read on the host); strict = 0 -- skipped silently
 *   (what a shard passes for ids it does not own).
 * A 64-bit image of the vocabulary does not fit a CU's LDS, so the columns are cut into tiles: a workgroup owns a chunk of rows (a slice of a
 * list), one query and one column tile of at most VS_TERM_SUM_TILE_COLS 64-bit bins.  It walks the bitmap as vs_index_term_counts does, streams the
 * packets of the set rows, and for a cell of column c adds fx(v) to bin c - tile0 when that is inside the tile -- one unsigned compare, which also
 * drops the padding id; a lane whose 8 column ids all miss the tile does not read the packet's values.  Non-zero bins are added to sums at the end
 * of the chunk (64-bit atomic adds); only the workgroups of tile 0 add to total.
 * vs_term_sum_plan: the launch of the two calls for these arguments -- pure host arithmetic, no device needed.  n_rows: the index's rows (for the
 *   id-list call: the m entries of a query, with per_query = 1 and rows_per_chunk = 0).  tile_cols = 0: automatic -- tiles = ceil(n_cols /
 *   VS_TERM_SUM_TILE_COLS), tile_cols = ceil(n_cols / tiles) (29 523 columns: two tiles of 14 762); any other value must lie in
 *   1..VS_TERM_SUM_TILE_COLS and is taken as given, tiles = ceil(n_cols / tile_cols).  rows_per_chunk = 0: automatic (chunks x B x tiles ~ 4
 *   workgroups a CU, a chunk at least 2048 rows); any other value must be a positive multiple of 64 and is taken as given.  chunks x rows_per_chunk
 *   >= n_rows > (chunks - 1) x rows_per_chunk.  Work item i: tile i % tiles of query (i / tiles) % B of chunk i / (tiles x B).  Both are tuning
 *   knobs: THE RESULT NEVER DEPENDS ON THE PLAN.
 * vs_term_sum_topn: per query the n columns with the largest mean weight, from sums [B, ld_sums] / total [B] and, when counts != NULL, counts
 *   [B, ld_counts] (vs_index_term_counts of the same set).  Column c is a candidate iff sums [b, c] > 0, total [b] > 0 and (counts == NULL or
 *   counts [b, c] >= min_count); without counts min_count is not looked at.  In fp64, each operation rounded once (no contraction):
 *     s = (double(sums [b, c]) * 2^-24) / double(total [b]),  score = float(s).
 *   Order: score descending, then column ascending -- two columns whose scores round to the same fp32 are ordered by the column.  out_cols int32 /
 *   out_score fp32 / out_sums int64, all [B, n], every slot written: -1 / -inf / 0 behind the last candidate.  n in 1..VS_TERM_MAX_TOPN, n > n_cols
 *   is allowed.  One workgroup per query; the order is that of the fp32 score, not of a saturating integer key (sums above 2^32 order correctly).
 * Errors: NULL handle or outputs, B < 1, rows_per_chunk no multiple of 64, tile_cols outside 0..VS_TERM_SUM_TILE_COLS, B > 1 with ld_words = 0,
 * ld_words / ld / ld_sums / ld_counts too short, m < 1, n out of range, chunks x B x tiles beyond 2^31 - 1 work items: VS_EINVAL -- checked before
 * the device is touched (without a GPU a bad argument is VS_EINVAL, a good one VS_ENODEVICE).  Pointers: all host (staged; the call blocks), or all
 * device pointers on the index's device / `device` (VS_EINVAL for a mix); device pointers and a non-NULL stream only enqueue.  A dense index on the
 * matrix cores keeps no packets: VS_EUNSUPPORTED.
 * Not covered: per-entry weights on id lists (fixed point would no longer be exact); the dense matrix kind; a shard group has no entry point of its
 * own (every shard sums its bit range of the bitmap, or the ids with strict = 0 and its id_offset; sums and total are added -- integers, so the
 * result is exactly the unsharded one -- and the top-n taken after the sum) and the one-process-per-GPU RCCL path has none; k-means itself; a
 * combined counts + sums pass.                                                                                                                  */
#define VS_TERM_FX_SHIFT 24          /* a cell contributes its value times 2^24, rounded to nearest even */
#define VS_TERM_FX_CLAMP_LOG2 20     /* ... after a clamp to +-2^20 */
#define VS_TERM_SUM_TILE_COLS 18432  /* columns of a workgroup's tile (144 KiB of 64-bit bins; the rest of the 160 KiB: counters) */
VS_API int vs_term_sum_plan(int64_t n_rows, int32_t B, int32_t n_cols, int per_query, int64_t rows_per_chunk, int32_t tile_cols,
                            int32_t* out_tiles, int32_t* out_tile_cols, int64_t* out_chunks, int64_t* out_rows_per_chunk);
VS_API int vs_index_term_sums(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, int64_t rows_per_chunk,
                              int32_t tile_cols, int64_t* sums, int64_t ld_sums, int64_t* total, void* stream);
VS_API int vs_index_term_sums_ids(vs_index* index, const int64_t* ids, int32_t B, int64_t m, int64_t ld, int64_t id_offset, int strict,
                                  int32_t tile_cols, int64_t* sums, int64_t ld_sums, int64_t* total, void* stream);
VS_API int vs_term_sum_topn(const int64_t* sums, int64_t ld_sums, const int64_t* total, const int64_t* counts, int64_t ld_counts, int32_t B,
                            int32_t n_cols, int32_t n, int64_t min_count, int32_t* out_cols, float* out_score, int64_t* out_sums, int device,
                            void* stream);

/* ---- clustering: the nearest of K centroids for every row (no reference counterpart: the reference only has topk) ----------------------------
 * The transposed question of a search: not "the best rows for this query" but "the best of these K queries for every row", without a [K, N]
 * score matrix.  centroids fp32 [K, ldc] (ldc >= n_cols), c'_j = centroid j rounded to the index dtype as vs_index_search rounds a query (fp16
 * store: to fp16, nearest even, widened again; fp32 and binary stores: as given).  For a row r with stored cells (col_t, v_t) in STORED order (v =
 * 1 on a binary index; cells carrying the padding id n_cols are skipped):
 *     S(j, r)     = the fp64 sum, starting at +0.0, taken in the row's stored cell order, of double(float(c'_j[col_t] * v_t))   (no fma)
 *     value(j, r) = float(S)  when bias == NULL,  float(S + double(bias[j]))  otherwise;  a NaN value counts -- and is reported -- as -inf
 *     label(r)    = the lowest j whose value is largest, values compared as floats (-0.0 == +0.0)
 * The order is fixed -- one lane owns a centroid and adds its products one after the other -- so a plain loop over the cells reproduces the sum bit
 * for bit; where every product and partial sum is exact, value equals vs_index_explain's score of (centroid label(r), row r).  A row that is deleted
 * or not allowed by the filter gets label -1 / value -inf; an empty row has S = +0.0 (label 0 without a bias, the argmax of the bias with one).
 * out_labels int32 [n_rows] and out_values fp32 [n_rows] (may be NULL): slots [0, n_rows) are all written, nothing behind them.
 * filter: ONE bitmap in the layout of vs_index_search_filtered, read from bit filter_bit0 on (bit filter_bit0 + r = row r: a shard passes the
 * group's bitmap and its first row); NULL = every live row.  Tombstones are ANDed in at bit 0.
 *
 * vs_centroid_half_norms: hn[j] = float(0.5 * T_j) for centroids c fp32 [K, ldc], rounded to fp16 first when round_f16 != 0:
 *     x[t] = fp64 sum over columns c = t, t + 256, t + 512, ... (ascending) of double(float(c'_j[c] * c'_j[c])),   t in 0..255
 *     for h = 128, 64, ..., 1:  x[t] += x[t + h] for t < h;   T_j = x[0]
 * With bias = -hn, the argmax of value is the argmin of ||x_r - c'_j||^2: the assignment step of Lloyd's k-means.
 *
 * vs_label_bitmaps: labels int32 [n_rows] and B values -> B bitmaps, bit bit0 + r of row b set iff labels[r] == values[b].  Words [0, (bit0 +
 * n_rows + 31) / 32) of each row of out_words [B, ld_words] are written whole (bits below bit0 and past the rows: 0).  The per-label filters of a
 * drill-down, and the K cluster sets vs_index_term_sums takes.  B in 1..VS_LABEL_MAX_VALUES.
 *
 * Kernels (assign.hip): a prep kernel transposes and rounds the centroids into a slab Ct [n_cols + 1][Kp] (Kp = K rounded up to the slice width W;
 * row n_cols -- the padding id -- and slots j >= K are zero; device scratch of slab_bytes, freed before the call returns).  The assign kernel gives
 * a wave a row: lane l holds packet p0 + l in registers, the cells are broadcast in stored order and every lane loads its W / 64 centroids' weights of
 * the cell's column -- one coalesced read of W * 4 bytes -- and adds the product to its fp64 accumulators; K > W takes Kp / W slices over the same
 * registers.  vs_assign_plan is the launch for these arguments -- pure host arithmetic, no device needed: W = 64 (K <= 64), 128 (K <= 128) or 256;
 * rows_per_chunk = 0: automatic, else a positive multiple of 64 taken as given (a tuning knob: the result does not depend on it).
 * Errors: NULL handle / centroids / out_labels, K outside 1..VS_ASSIGN_MAX_K, ldc < n_cols, filter_bit0 < 0, rows_per_chunk no multiple of 64,
 * host centroids or bias that are not finite: VS_EINVAL -- checked before the device is touched.  Pointers: all host (staged; the call blocks) or all
 * device pointers on the index's device / `device` (VS_EINVAL for a mix); device pointers and a non-NULL stream only enqueue (the slab is freed
 * behind a stream synchronisation either way).  A dense index on the matrix cores keeps no packets: VS_EUNSUPPORTED.
 * Not covered: the top-m nearest centroids and soft assignment; the dense matrix kind; a shard group has no entry point of its own (every shard
 * assigns its rows with its bit range of the filter: a row's value depends on nothing but the row) and the one-process-per-GPU RCCL path has none.
 * (The k-means update takes the sums of all K clusters from one vs_index_label_term_sums call, below.)                                          */
#define VS_ASSIGN_MAX_K 4096         /* centroids of one vs_index_assign call */
#define VS_LABEL_MAX_VALUES 4096     /* bitmaps of one vs_label_bitmaps call */
VS_API int vs_assign_plan(int64_t n_rows, int32_t K, int32_t n_cols, int64_t rows_per_chunk, int32_t* out_slice_w, int32_t* out_slices,
                          int64_t* out_chunks, int64_t* out_rows_per_chunk, int64_t* out_slab_bytes);
VS_API int vs_centroid_half_norms(const float* c, int64_t ldc, int32_t K, int32_t n_cols, int round_f16, float* out, int device, void* stream);
VS_API int vs_index_assign(vs_index* index, const float* centroids, int64_t ldc, int32_t K, const float* bias, const uint32_t* filter,
                           int64_t filter_bit0, int64_t rows_per_chunk, int32_t* out_labels, float* out_values, void* stream);
VS_API int vs_label_bitmaps(const int32_t* labels, int64_t n_rows, const int32_t* values, int32_t B, int64_t bit0, uint32_t* out_words,
                            int64_t ld_words, int device, void* stream);

/* ---- per-label term aggregations: the term sums / term counts of every label's rows in one pass (no reference counterpart) -------------------
 * The "x facet label" product of vs_index_term_sums and vs_index_term_counts: the centroid of every cluster, category or article at once.  Every
 * row has one label, so the work is one visit per stored cell whatever the number of labels; the answers are the integers of the calls above, so
 * row l equals, bit for bit, vs_index_term_sums / vs_index_term_counts on the set "label == l AND set".
 * Inputs: a CSR-packet index; labels int32 [n_rows]; n_labels in 1..VS_LABEL_TERM_MAX_LABELS; ONE document set -- bit bit0 + r of `words` stands
 * for row r, words == NULL: every row; the handle's live bitmap is ANDed in at bit 0 whatever bit0 is; bits at or past bit0 + n_rows are ignored.
 * vs_index_label_term_sums: sums [n_labels, ld_sums] int64 (ld_sums >= n_cols): sums [l, c] = the sum of fx(v) -- the fixed point of the term sums,
 *   unchanged: a binary store, the padding column, stored +-0, NaN and the wrap modulo 2^64 as there -- over the stored cells (r, c) of the set
 *   rows with labels [r] == l.  total [n_labels] int64: the set rows of each label.  other [1] int64: the set rows whose label is outside [0,
 *   n_labels) (-1 = "no label" included); they contribute nowhere.  total.sum() + other [0] = vs_set_count of the same set.  Every element
 *   of sums [:, 0 .. n_cols), of total and of other is written; columns [n_cols, ld_sums) are not touched.
 * vs_index_label_term_counts: the same shape; counts [l, c] = the set rows of label l that HAVE column c (stored with a non-zero value: the
 *   definition of vs_index_term_counts).  A binary index's sums are its counts x 2^24.
 * vs_label_order: the set rows grouped by label, the first stage of the two calls, public so that it can be pinned: ptr int64 [n_labels + 1],
 *   the exclusive bases of the per-label set-row counts (ptr [n_labels] = the rows listed); rows uint32 [n_rows], of which the first ptr [n_labels]
 *   are written: rows [ptr [l] .. ptr [l + 1]) are the set rows of label l in NO SPECIFIED ORDER (compare them sorted); other [1] as above.  Any
 *   index kind.  Up to VS_FACET_LDS_BINS labels a workgroup counts and ranks its chunk's rows in an LDS histogram and reserves a label's range with
 *   one global atomic; above, every set row takes one global atomic.
 * Kernels (label_terms.hip): the label order (count, one-workgroup scan, place), a small kernel that cuts every label's segment into items of at
 * most rows_per_item rows -- sum over labels of ceil(cnt / rows_per_item) of them --, and one 1024-thread workgroup per (item, column tile) that
 * zeroes a tile of 64-bit (sums) or 32-bit (counts) LDS bins, streams the packets of the item's rows and flushes the non-zero bins with 64-bit
 * atomics into row `label`.  The grid is sized by the bound max_items = ceil(n_rows / rows_per_item) + n_labels; items past the real count exit
 * at once -- nothing is read back to the host between the stages.  The scratch (4 bytes a row, 16 an item, 24 a label) is kept by the handle.
 * vs_label_term_plan: the launch for these arguments -- pure host arithmetic, no device needed.  tile_cols as in vs_term_sum_plan (0 = automatic,
 *   else 1..VS_TERM_SUM_TILE_COLS taken as given).  rows_per_item = 0: automatic -- the chunk rule of the term aggregations over `tiles` work
 *   items (~ 1024 / tiles items over the rows, at least 2048 rows each); any other value must be a positive multiple of 64 and is taken as given.
 *   Both are tuning knobs: NO OUTPUT DEPENDS ON THE PLAN.
 * Errors: NULL handle, labels or outputs, n_labels outside 1..VS_LABEL_TERM_MAX_LABELS, bit0 < 0, rows_per_item no multiple of 64, tile_cols outside
 * 0..VS_TERM_SUM_TILE_COLS, ld too short, n_labels x ld beyond VS_LABEL_TERM_MAX_CELLS (1 GiB of int64: 4546 labels at 29 523 columns), max_items x
 * tiles beyond VS_LABEL_TERM_MAX_WORK_ITEMS (a launch of 1024-thread workgroups holds fewer than 2^32 threads): VS_EINVAL -- checked before the device is
 * touched.  Pointers: all host (staged; the call blocks) or all
 * device pointers on the index's device (VS_EINVAL for a mix); device pointers and a non-NULL stream only enqueue.  A dense index on the matrix
 * cores keeps no packets: VS_EUNSUPPORTED (vs_label_order serves it).
 * Not covered: B > 1 sets in one call; two label arrays crossed; a sorted order inside a label; id-list driven sets; the dense matrix kind; a
 * shard group has no entry point of its own (every shard takes its slice of the labels and its bit range of the set; the integer outputs are
 * added, any top-n taken after the sum) and the one-process-per-GPU RCCL path has none.                                                          */
#define VS_LABEL_TERM_MAX_LABELS 65536      /* labels of one call */
#define VS_LABEL_TERM_MAX_CELLS (1ll << 27) /* n_labels x ld of one call: 1 GiB of int64 */
#define VS_LABEL_TERM_MAX_WORK_ITEMS 4194303 /* max_items x tiles of one call: (2^32 - 1) / 1024 workgroups of 1024 threads */
VS_API int vs_label_term_plan(int64_t n_rows, int32_t n_labels, int32_t n_cols, int64_t rows_per_item, int32_t tile_cols, int32_t* out_tiles,
                              int32_t* out_tile_cols, int64_t* out_rows_per_item, int64_t* out_max_items);
VS_API int vs_label_order(vs_index* index, const uint32_t* words, int64_t bit0, const int32_t* labels, int32_t n_labels, int64_t* ptr,
                          uint32_t* rows, int64_t* other, void* stream);
VS_API int vs_index_label_term_sums(vs_index* index, const uint32_t* words, int64_t bit0, const int32_t* labels, int32_t n_labels,
                                    int64_t rows_per_item, int32_t tile_cols, int64_t* sums, int64_t ld_sums, int64_t* total, int64_t* other,
                                    void* stream);
VS_API int vs_index_label_term_counts(vs_index* index, const uint32_t* words, int64_t bit0, const int32_t* labels, int32_t n_labels,
                                      int64_t rows_per_item, int32_t tile_cols, int64_t* counts, int64_t ld_counts, int64_t* total, int64_t* other,
                                      void* stream);

/* ---- numeric fields: range filters, stats, histograms and sort by value over a per-row quantity (no reference counterpart) ------------------
 * A field is one 32-bit value per row: values [n_rows] of dtype VS_VAL_F32 (fp32) or VS_VAL_I32 (int32).  A row may have NO value: the missing
 * sentinel is NaN (any NaN pattern) for fp32 and INT32_MIN for int32.  Everything is decided on one ORDER KEY, a uint32:
 *     fp32:  key = flip(canon_zero(v)) -- -0.0 and +0.0 share a key, -inf < finite < +inf, the smallest key is -inf's, 0x007FFFFF;
 *     int32: key = uint32(v) ^ 0x80000000;       missing: key 0 (no value of either type has it).
 * All comparisons are unsigned compares of keys, so every result is exact and bit-reproducible whatever the launch.
 * A set of rows is given exactly as for vs_facet_counts: bit bit0 + r of the bitmap at words + b * ld_words stands for row r (ld_words = 0: one
 * bitmap, and then B must be 1; else ld_words >= the (bit0 + n_rows + 31) / 32 words a bitmap spans); words == NULL: every row (B must be 1);
 * and_words (may be NULL): a second bitmap shared by all queries, at the same bit0; bits at or past bit0 + n_rows are ignored whatever they hold.
 * The vs_index_* variants run over the index's rows with its tombstones ANDed in (at bit 0 whatever bit0 is): deleted rows never count.
 *
 * vs_value_range_bitmaps: lo / hi [B] in the field's type -> B bitmaps; bit bit0 + r of row b is set iff row r has a value and lo[b] <= v <= hi[b],
 *   both ends inclusive (compared on keys: a bound of -0.0 is +0.0).  lo > hi is the empty set; fp32 bounds may be +-inf (an open end; for int32
 *   INT32_MIN + 1 and INT32_MAX).  A missing bound (NaN / INT32_MIN): VS_EINVAL for host arrays; on the device it matches nothing.  Words [0,
 *   (bit0 + n_rows + 31) / 32) of each row of out_words [B, ld_words] are written whole, bits below bit0 and past the rows 0 -- the convention of
 *   vs_label_bitmaps.  B in 1..VS_VALUE_MAX_RANGES.  A wave owns 64 bits of every bitmap: it loads its rows' keys once and forms each word pair
 *   with a ballot; plain stores, no atomics.
 * vs_value_plan: the launch of vs_value_stats / vs_value_histogram for these arguments -- pure host arithmetic, no device needed, the rule of
 *   vs_facet_plan: qt = queries a workgroup serves (8 for per-query bitmaps, 1 for a shared one); chunks x rows_per_chunk >= n_rows > (chunks - 1)
 *   x rows_per_chunk.  n_bins: the LDS bins a query takes (n_edges + 2 for a histogram, 0 for stats; 0..VS_VALUE_MAX_EDGES + 2).  rows_per_chunk
 *   = 0: automatic; any other value must be a positive multiple of 64 and is taken as given (a tuning knob: no result depends on it).
 *   vs_value_topk cuts its chunks by the same rule with per_query = 1 and n_bins = 0, one query a workgroup.
 * vs_value_stats: per query b, count [b] = set rows that have a value, missing [b] = set rows without one (count + missing = the size of the set,
 *   vs_facet_counts' total); out_min [b] / out_max [b]: raw 32-bit values of the field's type (of -0.0 and +0.0 the answer is +0.0; count = 0:
 *   the missing sentinel, NaN 0x7FC00000 / INT32_MIN); sum [b] int64: int32 field -- the exact integer sum; fp32 field -- the sum of fx(v) of
 *   the term sums above (clamped to +-2^VS_TERM_FX_CLAMP_LOG2, times 2^VS_TERM_FX_SHIFT, rounded to nearest even); sums wrap modulo 2^64.
 *   count, missing, sum int64 [B]; every element of the five outputs is written.
 * vs_value_histogram: edges [n_edges] in the field's type, strictly ascending (on keys: -0.0 next to +0.0 is not), none missing, n_edges in
 *   2..VS_VALUE_MAX_EDGES -- a host array that breaks this is VS_EINVAL, a device array is not read on the host (the bin sum identity still
 *   holds, the bins are whatever the search gives).  Bin i holds edges[i] <= v < edges[i + 1]; below [b]: v < edges[0]; above [b]: v >=
 *   edges[n_edges - 1]; missing [b] as above.  counts [B, ld_counts] int64, ld_counts >= n_edges - 1; columns [n_edges - 1, ld_counts) are not
 *   touched; below / above / missing int64 [B].  counts [b].sum() + below [b] + above [b] + missing [b] == the size of the set, always.
 * vs_value_topk: per query the k set rows that have a value, in value order: descending != 0 -- value descending, else ascending; then id
 *   ascending (-0.0 and +0.0 tie).  out_ids int64 [B, k] (row + id_offset), out_values [B, k] the rows' 32-bit values as stored (a -0.0 stays -0.0); unused slots hold id
 *   -1 and the missing sentinel; every slot is written.  k in 1..VS_VALUE_MAX_TOPK, k > n_rows is allowed.
 * Kernels (values.hip).  Stats and histogram: a workgroup owns a chunk of rows and a tile of qt queries; it walks the bitmaps in 2048-row spans,
 * leaves a span whose words are all zero without touching the values, and loads a row's value once for the tile.  Histogram: the edges sit in LDS
 * as keys, the bin is a branch-free binary search (<= 11 steps), one uint32 LDS histogram of n_edges + 2 bins per query of the tile (33 KB at 8
 * queries and 1025 edges: one regime); non-zero bins are added to the outputs with 64-bit atomics at the end of the chunk.  Stats: min / max key
 * and sum per lane, reduced per wave, then per workgroup in LDS, then one atomic per (workgroup, query) on keys / int64; a finishing kernel
 * turns keys into raw values.  Top-k: a workgroup owns a chunk and one query and streams (key or ~key) << 32 | ~row through a 4096-key LDS
 * buffer, sorted and cut to k when more than 2048 are in -- afterwards only keys above the k-th are admitted; per-chunk lists go to device
 * scratch (freed behind a stream synchronisation before the call returns) and one workgroup per query merges them.
 * Errors: NULL values or outputs, dtype not VS_VAL_*, n_rows outside 1..2^32 - 1, B < 1 (B > VS_VALUE_MAX_RANGES for the range bitmaps), bit0 < 0,
 * B > 1 with ld_words = 0, ld_words / ld_counts too short, rows_per_chunk no multiple of 64, n_edges or k out of range, chunks x B x k beyond
 * 2^27 scratch keys, host edges / bounds as above: VS_EINVAL -- checked before the device is touched (without a GPU a bad argument is VS_EINVAL,
 * a good one VS_ENODEVICE).  Pointers: all host (staged; the call blocks), or all device pointers on `device` / the index's device (VS_EINVAL
 * for a mix); device pointers and a non-NULL stream only enqueue (vs_value_topk synchronises either way).
 * Not covered: no index file stores values; 64-bit and fp64 values; sort by several keys; k > 1024; a shard
 * group has no entry point of its own (every shard works on its slice of the values and its bit range of the bitmap: counts, sums and bins are
 * added, min / max combined on keys, the top-k lists merged by (key, id)) and the one-process-per-GPU RCCL path has none.                       */
#define VS_VAL_F32 0
#define VS_VAL_I32 1
#define VS_VALUE_MAX_RANGES 4096     /* bitmaps of one vs_value_range_bitmaps call */
#define VS_VALUE_MAX_EDGES 1025      /* edges of a histogram: up to 1024 bins */
#define VS_VALUE_MAX_TOPK 1024       /* rows vs_value_topk lists per query at most */
VS_API int vs_value_range_bitmaps(const void* values, int dtype, int64_t n_rows, const void* lo, const void* hi, int32_t B, int64_t bit0,
                                  uint32_t* out_words, int64_t ld_words, int device, void* stream);
VS_API int vs_value_plan(int64_t n_rows, int32_t B, int32_t n_bins, int per_query, int64_t rows_per_chunk, int32_t* out_qt, int64_t* out_chunks,
                         int64_t* out_rows_per_chunk);
VS_API int vs_value_stats(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                          int dtype, int64_t n_rows, int64_t rows_per_chunk, int64_t* count, int64_t* missing, void* out_min, void* out_max,
                          int64_t* sum, int device, void* stream);
VS_API int vs_index_value_stats(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values, int dtype,
                                int64_t rows_per_chunk, int64_t* count, int64_t* missing, void* out_min, void* out_max, int64_t* sum,
                                void* stream);
VS_API int vs_value_histogram(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                              int dtype, int64_t n_rows, const void* edges, int32_t n_edges, int64_t rows_per_chunk, int64_t* counts,
                              int64_t ld_counts, int64_t* below, int64_t* above, int64_t* missing, int device, void* stream);
VS_API int vs_index_value_histogram(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values,
                                    int dtype, const void* edges, int32_t n_edges, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts,
                                    int64_t* below, int64_t* above, int64_t* missing, void* stream);
VS_API int vs_value_topk(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                         int dtype, int64_t n_rows, int32_t k, int descending, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids,
                         void* out_values, int device, void* stream);
VS_API int vs_index_value_topk(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values, int dtype,
                               int32_t k, int descending, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, void* out_values,
                               void* stream);

/* ---- percentiles: exact order statistics of a numeric field over any document set (no reference counterpart) ---------------------------------
 * For query b let K_b be the ascending multiset of the order keys (above) of the rows that are in the set (bitmap bit set, and_words bit set,
 * live for the vs_index_* variant) and carry a value (key != 0): count [b] = |K_b|, missing [b] = the set rows with key 0.  The ORDER STATISTIC
 * of rank r (0-based, ascending) is value_unkey(K_b[r]): a raw 32-bit value of the field's type, +0.0 of -0.0 / +0.0 as vs_value_stats' min and
 * max.  A rank outside 0..count - 1 (any rank when count = 0) gives the missing sentinel (NaN 0x7FC00000 / INT32_MIN) and a resolved rank of -1.
 * QUANTILE -> RANK: pos = q * double(count - 1), ONE fp64 multiplication, q in [0, 1]; VS_QUANTILE_LOWER: floor(pos), VS_QUANTILE_HIGHER:
 * ceil(pos), VS_QUANTILE_NEAREST: rint(pos), half to even.  No call interpolates (the Python facade's "linear" selects floor and ceil exactly).
 * The selection is a most-significant-digit radix select on the keys, VS_VALUE_RADIX_LEVELS = 3 levels: level 0 = bits 31..21, level 1 = bits
 * 20..10 (VS_VALUE_RADIX_BINS = 2048 bins each), level 2 = bits 9..0 (1024 bins): three passes over bitmaps and values.  Every count is an
 * integer, so shards ADD their counts between the levels and a row-sharded index gives the unsharded answer bit for bit.
 *
 * vs_value_quantiles / vs_index_value_quantiles: all three levels on one device.  The set arguments are vs_value_stats'.  R in
 *   1..VS_VALUE_MAX_RANKS ranks per query, given either as q double [R] (shared by the queries) with `method`, or -- q == NULL -- as ranks
 *   int64 [B, R].  out_values [B, R] raw 32-bit, out_ranks int64 [B, R] the resolved ranks (-1: no answer), count / missing int64 [B]; every
 *   element is written.  The call is the composition of the level calls below, bit for bit, and synchronises either way (its counts are device
 *   scratch, B x R x 2048 int64, at most 2^27 of them).
 * vs_value_radix_counts / vs_index_value_radix_counts: one level's digit counts.  counts int64 [B, S, bins], S = 1 at level 0 and R at levels 1
 *   and 2, bins = 2048 / 2048 / 1024, written whole.  Level 0 counts the top digit of every set row with a value and writes missing [B]; levels
 *   1 and 2 read the step's state -- slot_prefix uint32 [B, R], n_slots int32 [B] -- and count, for slot s < n_slots[b], the level's digit of the
 *   rows whose higher digits equal slot_prefix [b, s]; rows of no slot cost no atomic; slots >= n_slots[b] stay 0.  missing / slot_prefix /
 *   n_slots may be NULL where the level does not use them.  Pointers all host or all device, as vs_value_stats.
 * vs_value_radix_step: the step between two levels, on DEVICE buffers only (one workgroup a query).  State arrays, all [B, R] but n_slots [B]:
 *     rank_res    int64   in (levels 1, 2) / out: each rank's residual rank inside its slot; -1 = no answer
 *     rank_slot   int32   in (levels 1, 2) / out: the slot of the NEXT level the rank fell into; -1 = no answer
 *     rank_prefix uint32  out: the rank's digits so far, right-aligned (11, 22, 32 bits: after level 2 the key itself)
 *     slot_prefix uint32  in (levels 1, 2) / out: the next level's slots: the distinct rank_prefix values, ascending; 0xFFFFFFFF behind the last
 *     n_slots     int32   out: how many; equal ranks, and ranks that fell into one bin, share a slot
 *   Level 0 reads counts [B, 1, 2048] and q [R] with method or ranks [B, R] (device arrays; a q outside [0, 1] or NaN, or a rank outside
 *   0..count - 1, resolves to -1), and also writes count [B] = the sum of the bins and out_ranks [B, R].  Levels 1 and 2 read counts [B, R,
 *   bins]: per slot a prefix scan of the bins, per rank the bin d with cum <= r < cum + counts[d]; the residual becomes r - cum.  Level 2 also
 *   writes out_values [B, R] = value_unkey(rank_prefix) (the sentinel for -1); out_values may be NULL at the other levels, q / ranks / count /
 *   out_ranks at levels 1 and 2.
 * vs_value_quantile_plan: the launch of the counting kernel -- pure host arithmetic on R: per-query bitmaps R = 1..2 -> qt = 8, 3..4 -> 4, 5..8
 *   -> 2, 9..16 -> 1; a shared bitmap qt = 1; chunks and rows_per_chunk by vs_value_plan's rule with n_bins = 0.  LDS = qt x S x bins x 4 bytes,
 *   128 KiB at most.
 * Kernels (quantiles.hip).  Counting: the shape of the histogram kernel above -- a workgroup owns a chunk and a tile of qt queries, walks the
 * bitmaps in 2048-row spans, loads a row's value once for the tile; a row's slot is found by a branch-free search (4 steps and a compare) over the
 * query's sorted slot prefixes in LDS; when every row of a 64-row step falls into one bin one lane adds the popcount; non-zero bins are flushed
 * with 64-bit atomics.  Integer arithmetic throughout.
 * Errors (VS_EINVAL before the device is touched; a good call without a GPU is VS_ENODEVICE): everything vs_value_stats refuses, R outside
 * 1..VS_VALUE_MAX_RANKS, an unknown method or level, a host q outside [0, 1] or NaN, a negative host rank, B x R x 2048 beyond 2^27, a NULL
 * array the level needs, host pointers to vs_value_radix_step.
 * Not covered: weighted quantiles; skipping levels by the set's common key prefix; 64-bit values; the one-process-per-GPU RCCL path
 * (per-label quantiles: vs_facet_value_quantiles below).                                                                                        */
#define VS_VALUE_RADIX_BINS 2048
#define VS_VALUE_RADIX_LEVELS 3
#define VS_VALUE_MAX_RANKS 16
#define VS_QUANTILE_LOWER 0
#define VS_QUANTILE_HIGHER 1
#define VS_QUANTILE_NEAREST 2
VS_API int vs_value_quantile_plan(int64_t n_rows, int32_t B, int32_t R, int per_query, int64_t rows_per_chunk, int32_t* out_qt, int64_t* out_chunks,
                                  int64_t* out_rows_per_chunk);
VS_API int vs_value_quantiles(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                              int dtype, int64_t n_rows, const double* q, int method, const int64_t* ranks, int32_t R, int64_t rows_per_chunk,
                              void* out_values, int64_t* out_ranks, int64_t* count, int64_t* missing, int device, void* stream);
VS_API int vs_index_value_quantiles(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values, int dtype,
                                    const double* q, int method, const int64_t* ranks, int32_t R, int64_t rows_per_chunk, void* out_values,
                                    int64_t* out_ranks, int64_t* count, int64_t* missing, void* stream);
VS_API int vs_value_radix_counts(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                                 int dtype, int64_t n_rows, int level, int32_t R, const uint32_t* slot_prefix, const int32_t* n_slots,
                                 int64_t rows_per_chunk, int64_t* counts, int64_t* missing, int device, void* stream);
VS_API int vs_index_value_radix_counts(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values,
                                       int dtype, int level, int32_t R, const uint32_t* slot_prefix, const int32_t* n_slots, int64_t rows_per_chunk,
                                       int64_t* counts, int64_t* missing, void* stream);
VS_API int vs_value_radix_step(int level, const int64_t* counts, int32_t B, int32_t R, const double* q, int method, const int64_t* ranks,
                               int64_t* rank_res, int32_t* rank_slot, uint32_t* rank_prefix, uint32_t* slot_prefix, int32_t* n_slots,
                               int64_t* count, int64_t* out_ranks, void* out_values, int dtype, int device, void* stream);

/* ---- breakdowns: a numeric field's stats and histogram per facet label, in one pass (no reference counterpart) -------------------------------
 * The product of the facet counts and the numeric fields above: labels int32 [n_rows] as for vs_facet_counts, values [n_rows] of dtype
 * VS_VAL_F32 / VS_VAL_I32 as for vs_value_stats, the set of rows given exactly as there (words, bit0, ld_words, and_words; the vs_index_*
 * variants AND the index's tombstones in at bit 0).  Everything is decided on the order keys above: every output is an integer or a 32-bit
 * pattern, exact, independent of the launch, and bit-identical on a row-sharded index.  For a row of query b's set:
 *   its label is outside [0, n_labels), -1 included: other [b] += 1 and nothing else, whether or not it has a value;
 *   its label is l and it has a value (key != 0): count [b, l] += 1, min / max [b, l] are taken on the key, sum [b, l] adds what vs_value_stats
 *     adds (the integer itself for int32, fx(v) of the term sums for fp32; int64 wrapping modulo 2^64);
 *   its label is l and it has no value (NaN, INT32_MIN): missing [b, l] += 1;
 *   total [b] is the size of the set: count [b].sum() + missing [b].sum() + other [b] == total [b], and count + missing is vs_facet_counts'
 *   counts [b, l].
 * vs_facet_value_plan: the launch of either call -- pure host arithmetic, no device needed.  n_slots = 0: stats, a query takes n_labels
 *   24-byte records; n_slots = n_edges + 2: histogram, a query takes n_labels x n_slots uint32 bins.  regime 0: the records / bins of qt
 *   queries sit in a workgroup's LDS (qt x records <= VS_FACET_VALUE_LDS_RECORDS, qt x bins <= VS_FACET_LDS_BINS; per-query bitmaps start at
 *   qt = 8 and halve until that holds, a shared bitmap has qt = 1); regime 1: atomics straight into the outputs (qt = 8 or 1: the tile only
 *   shares the loads).  chunks and rows_per_chunk by vs_value_plan's rule with a floor of 16 x the LDS records / bins of a query.
 * vs_facet_value_stats: count, missing, sum int64 [B, ld_out]; out_min / out_max [B, ld_out] raw 32-bit values of the field's type (a cell with
 *   count = 0: the missing sentinel, NaN 0x7FC00000 / INT32_MIN; of -0.0 and +0.0 the answer is +0.0); total, other int64 [B].  ld_out >=
 *   n_labels; columns [n_labels, ld_out) of the five matrices are never written, every other element is.
 * vs_facet_value_histogram: edges as for vs_value_histogram (checked the same way); counts int64 [B, n_labels, ld_counts]: bin i of (b, l)
 *   holds the rows with label l and edges[i] <= v < edges[i + 1]; below / above / missing int64 [B, n_labels]; total, other int64 [B].
 *   ld_counts >= n_edges - 1; columns [n_edges - 1, ld_counts) are never written.  counts [b].sum() + below [b].sum() + above [b].sum() +
 *   missing [b].sum() + other [b] == total [b], always; the slots of (b, l) add up to vs_facet_counts' counts [b, l].
 * Kernels (facet_values.hip): a workgroup owns a chunk of rows and a tile of qt queries and walks the bitmaps as the kernels above do; a lane
 * whose row is in some query's set loads its label and its value once for the tile.  A step whose in-range rows of a query all carry one label
 * (32 of them at least; one slot, for the histogram, any number) is reduced across the wave and added by one lane; otherwise every lane adds for itself.  Stats keep the min /
 * max KEYS in out_min / out_max (preset to 0xFFFFFFFF / 0) until a finishing kernel turns them into values.
 * Errors: as for vs_value_stats / vs_value_histogram, and n_labels < 1, n_labels x (n_edges + 2) > VS_FACET_VALUE_MAX_CELLS, B x n_labels >
 * 2^31 - 1, ld_out < n_labels: VS_EINVAL, checked before the device is touched.  Pointers: all host (staged; the call blocks) or all device.
 * Not covered: top-n labels by a statistic; two facet fields crossed; 64-bit values; the one-process-per-GPU RCCL path. */
/* (query, label) records of a workgroup's LDS in the stats kernel: 24 bytes each, 48 KiB, so three workgroups fit a CU's 160 KiB.  A design
 * choice: the occupancy it leaves has not been measured against a smaller or a larger cap. */
#define VS_FACET_VALUE_LDS_RECORDS 2048
#define VS_FACET_VALUE_MAX_CELLS 4194304 /* n_labels x (n_edges + 2) of a histogram call: 2^22 cells a query */
VS_API int vs_facet_value_plan(int64_t n_rows, int32_t B, int32_t n_labels, int32_t n_slots, int per_query, int64_t rows_per_chunk,
                               int32_t* out_regime, int32_t* out_qt, int64_t* out_chunks, int64_t* out_rows_per_chunk);
VS_API int vs_facet_value_stats(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const int32_t* labels,
                                int32_t n_labels, const void* values, int dtype, int64_t n_rows, int64_t rows_per_chunk, int64_t* count,
                                int64_t* missing, void* out_min, void* out_max, int64_t* sum, int64_t ld_out, int64_t* total, int64_t* other,
                                int device, void* stream);
VS_API int vs_index_facet_value_stats(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                      int32_t n_labels, const void* values, int dtype, int64_t rows_per_chunk, int64_t* count, int64_t* missing,
                                      void* out_min, void* out_max, int64_t* sum, int64_t ld_out, int64_t* total, int64_t* other, void* stream);
VS_API int vs_facet_value_histogram(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B,
                                    const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t n_rows, const void* edges,
                                    int32_t n_edges, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* below, int64_t* above,
                                    int64_t* missing, int64_t* total, int64_t* other, int device, void* stream);
VS_API int vs_index_facet_value_histogram(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                          int32_t n_labels, const void* values, int dtype, const void* edges, int32_t n_edges,
                                          int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* below, int64_t* above,
                                          int64_t* missing, int64_t* total, int64_t* other, void* stream);

/* ---- per-label percentiles: exact order statistics of a numeric field per facet label, one pass a radix level (no reference counterpart) ------
 * The product of the percentiles and the breakdowns above.  The set arguments, the dtypes, the pointer rule and the error order are
 * vs_facet_value_stats'; the digits, the ranks and the sentinels vs_value_quantiles'.  For query b and label l in [0, n_labels) let K[b, l] be
 * the ascending multiset of the order keys of the rows that are in the set, carry label l and have a value (key != 0): count [b, l] = |K[b, l]|,
 * missing [b, l] = the set rows of label l with key 0; a set row whose label is outside [0, n_labels), -1 included, adds to other [b] and
 * nothing else; total [b] is the size of the set: count [b].sum() + missing [b].sum() + other [b] == total [b], always, and count + missing is
 * vs_facet_counts' counts [b, l].  The order statistic of rank r is value_unkey(K[b, l][r]); a rank outside 0..count - 1 gives the missing
 * sentinel and a resolved rank of -1; quantile -> rank is the rule above applied to count [b, l].
 *
 * vs_facet_value_radix_counts / vs_index_facet_value_radix_counts: one level's digit counts per (query, label).  counts int64 [B, n_labels, S,
 *   bins], S = 1 at level 0 and R at levels 1 and 2, bins = 2048 / 2048 / 1024, written whole.  Level 0 also writes missing [B, n_labels], total
 *   [B] and other [B].  Levels 1 and 2 read slot_prefix uint32 [B, n_labels, R] and n_slots int32 [B, n_labels]: exactly the state
 *   vs_value_radix_step produces when called with B' = B x n_labels.  A row of no slot costs no atomic; slots >= n_slots stay 0.  The arrays a
 *   level does not use may be NULL.
 * vs_facet_value_quantiles / vs_index_facet_value_quantiles: all three levels on one device.  Ranks as q double [R] with `method` or -- q ==
 *   NULL -- as ranks int64 [B, n_labels, R].  out_values [B, n_labels, R] raw 32-bit, out_ranks int64 [B, n_labels, R], count, missing int64
 *   [B, n_labels], total, other int64 [B]; every element is written.  The call is, bit for bit, the composition of the level call and
 *   vs_value_radix_step over B x n_labels cells, and synchronises either way (its counts are device scratch).
 * vs_facet_value_quantile_plan: the launch of the counting kernel at `level` -- pure host arithmetic.  cap = the (query, label) cells whose
 *   histograms fit 128 KiB of LDS: 16 at level 0, 16 / R at level 1, 32 / R at level 2.  regime 0 (LDS): a workgroup serves qt queries x
 *   tile_labels labels, qt x tile_labels <= cap, label_tiles = ceil(n_labels / tile_labels) tiles in the grid's z dimension; qt is the power of
 *   two in 1..8 (1 for a shared bitmap) with the fewest passes ceil(B / qt) x label_tiles, tile_labels = min(n_labels, cap / qt), among those
 *   with label_tiles <= VS_FACET_QUANTILE_MAX_LABEL_TILES; of equal ones the smallest qt.  None: regime 1 (global atomics), qt = 8 or 1,
 *   tile_labels = n_labels, label_tiles = 1.  chunks and rows_per_chunk by vs_value_plan's rule over ceil(B / qt) x label_tiles items.
 * Kernel (facet_quantiles.hip): the shape of the percentiles' counting kernel.  A lane whose row is in some query's set loads its label once
 * for the tile; LDS regime: one unsigned compare label - tile0 < tile_labels picks the tile's rows, only those load their value; the tile's
 * slot prefixes sit in LDS; only slots in use are zeroed and flushed (64-bit atomics on non-zero bins); total and other are counted by the
 * first label tile, a label's missing rows by the tile that owns the label.  Global regime: 64-bit atomics straight into counts, a cell's slot
 * prefixes read from global memory.  A 64-row step whose counted rows all fall into one (label, slot, bin) is added once.
 * Errors (VS_EINVAL before the device is touched; a good call without a GPU is VS_ENODEVICE): everything vs_facet_value_stats and
 * vs_value_quantiles refuse, n_labels < 1, R outside 1..VS_VALUE_MAX_RANKS, B x n_labels x R x 2048 beyond 2^27 counts.
 * Not covered: weighted quantiles; more than 65536 labels through the Python facade; two facet fields crossed; the one-process-per-GPU RCCL
 * path.                                                                                                                                         */
/* Label tiles a level of the LDS regime takes at most.  Measured, not chosen: on builds of either regime at 21 M rows a tile pass costs 0.06
 * ms and the regimes meet at 8 tiles a level on a uniform float32 field and at 16 on a field of years. */
#define VS_FACET_QUANTILE_MAX_LABEL_TILES 16
VS_API int vs_facet_value_quantile_plan(int64_t n_rows, int32_t B, int32_t n_labels, int32_t R, int level, int per_query, int64_t rows_per_chunk,
                                        int32_t* out_regime, int32_t* out_qt, int32_t* out_tile_labels, int32_t* out_label_tiles,
                                        int64_t* out_chunks, int64_t* out_rows_per_chunk);
VS_API int vs_facet_value_quantiles(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B,
                                    const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t n_rows, const double* q,
                                    int method, const int64_t* ranks, int32_t R, int64_t rows_per_chunk, void* out_values, int64_t* out_ranks,
                                    int64_t* count, int64_t* missing, int64_t* total, int64_t* other, int device, void* stream);
VS_API int vs_index_facet_value_quantiles(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                          int32_t n_labels, const void* values, int dtype, const double* q, int method, const int64_t* ranks,
                                          int32_t R, int64_t rows_per_chunk, void* out_values, int64_t* out_ranks, int64_t* count,
                                          int64_t* missing, int64_t* total, int64_t* other, void* stream);
VS_API int vs_facet_value_radix_counts(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B,
                                       const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t n_rows, int level, int32_t R,
                                       const uint32_t* slot_prefix, const int32_t* n_slots, int64_t rows_per_chunk, int64_t* counts,
                                       int64_t* missing, int64_t* total, int64_t* other, int device, void* stream);
VS_API int vs_index_facet_value_radix_counts(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B,
                                             const int32_t* labels, int32_t n_labels, const void* values, int dtype, int level, int32_t R,
                                             const uint32_t* slot_prefix, const int32_t* n_slots, int64_t rows_per_chunk, int64_t* counts,
                                             int64_t* missing, int64_t* total, int64_t* other, void* stream);

/* ---- scores as a field: the exact score of every row of a document set, as a value array (no reference counterpart) -----------------------------
 * vs_index_set_scores: for query b and row r, out_scores [b * ld_scores + r] holds the library's exact score when r is live (not deleted) and in
 *   the set, and the missing sentinel of the numeric fields, NaN 0x7FC00000, for every other row.  The result is a VS_VAL_F32 field of its own:
 *   vs_index_value_stats / _histogram / _topk / _quantiles and the breakdowns take row b of it as `values` unchanged, which gives the stats,
 *   histograms, percentiles and per-label breakdowns of SCORES under the very keys every other field is decided on.
 *   The set: bit bit0 + r of the bitmap at words + b * ld_words, the layout of vs_index_value_stats -- but here ld_words = 0 is one bitmap SHARED by
 *   the batch and words == NULL every live row, for any B (the queries differ, not the sets); else ld_words >= the (bit0 + n_rows + 31) / 32 words
 *   a bitmap spans.  Bits at or past bit0 + n_rows are ignored.  The index's tombstones are ANDed in at bit 0 whatever bit0 is.
 *   The score is the one of vs_index_search_range and vs_index_explain, bit for bit: q (fp32 | fp16 [B, ldq]) is rounded to the index dtype as in
 *   vs_index_search; score = fl32(sum of fp64(fl32(q[c] * v[c])) over the row's stored cells), v = 1 on a binary index; a row without cells
 *   scores +0.0.  A score that is itself NaN (non-finite stored data or query) cannot be told from "not in the set": it reads as missing.
 *   Every element [b, 0 .. n_rows) is written; columns [n_rows, ld_scores) are not touched; ld_scores >= n_rows.
 * vs_set_score_plan: the launch for these arguments -- pure host arithmetic, no device needed.  A work item is (query, chunk of rows): chunks x
 *   rows_per_chunk >= n_rows > (chunks - 1) x rows_per_chunk.  rows_per_chunk = 0: automatic (about 1024 work items over the batch, a multiple
 *   of 64 rows, 2048 at least); any other value must be a positive multiple of 64 and is taken as given (a tuning knob: no result depends
 *   on it).  per_query is accepted for symmetry with the other plans; the rule does not depend on it.
 * Kernel (set_scores.hip): 1024 threads, one workgroup a CU; the query's dense fp32 image (4 x (n_cols + 1) bytes) sits in LDS and is loaded when
 *   a workgroup's query changes.  The set is walked in 2048-row spans, every wave on the same words; a span whose set words or live words are all
 *   zero is left at once.  The set rows of a span are compacted through LDS into a list (8 KB) and dealt to the 16 waves, one wave a row, so a
 *   sparse set costs its rows and the bitmap walk, not a scan.  The queries of a chunk run side by side on one XCD and share its L2.  Plain stores
 *   only; the sentinel is a 32-bit memset on the stream ahead of the kernel.
 * Errors: NULL q or out_scores, q_dtype not VS_F32 / VS_F16, B < 1, bit0 < 0, ld_words < 0 or too short, rows_per_chunk no multiple of 64, a NULL
 *   index, ldq < n_cols, ld_scores < n_rows, chunks x B beyond 2^31 - 1: VS_EINVAL, checked on the host before the device is touched.  A dense index
 *   on the matrix cores, and a CSR index wider than the LDS image (n_cols > 32763): VS_EUNSUPPORTED.  Pointers: all host (staged; the call blocks)
 *   or all device pointers on the index's device (VS_EINVAL for a mix); device pointers and a non-NULL stream only enqueue.
 * Not covered: a dense index; wide indexes; the one-process-per-GPU RCCL path; an 8-queries-a-pass tile variant of the scorer; a values stride in
 *   the value calls, which would make a batch of score rows one call (today: one value call a query); weighted aggregations.                    */
VS_API int vs_set_score_plan(int64_t n_rows, int32_t B, int32_t n_cols, int per_query, int64_t rows_per_chunk, int64_t* out_chunks,
                             int64_t* out_rows_per_chunk);
VS_API int vs_index_set_scores(vs_index* index, const void* q, int q_dtype, int64_t ldq, int32_t B, const uint32_t* words, int64_t bit0,
                               int64_t ld_words, int64_t rows_per_chunk, float* out_scores, int64_t ld_scores, void* stream);

/* ---- set egress: the size, the members, a page and a sample of any document set, and id lists back to bitmaps (no reference counterpart) ------
 * The way out of a bitmap.  A set of rows is given exactly as for vs_value_stats: bit bit0 + r of the bitmap at words + b * ld_words stands for
 * row r (ld_words = 0: one bitmap, and then B must be 1; else ld_words >= the (bit0 + n_rows + 31) / 32 words a bitmap spans); words == NULL:
 * every row (B must be 1); and_words (may be NULL): a second bitmap shared by all queries, at the same bit0; bits below bit0 and at or past
 * bit0 + n_rows are ignored whatever they hold.  The vs_index_* variants run over the index's rows with its tombstones ANDed in (at bit 0
 * whatever bit0 is): deleted rows are never counted, listed or sampled.  No float and no position-deciding atomic is involved: every result is
 * exact and independent of the launch.
 *
 * vs_set_list_plan: the launch for these arguments -- pure host arithmetic, no device needed.  A work item is (query, chunk of rows): chunks x
 *   rows_per_chunk >= n_rows > (chunks - 1) x rows_per_chunk; spans = the 2048-row spans of a query, (n_rows + 2047) / 2048.  rows_per_chunk = 0:
 *   automatic (about 1024 work items over the batch, 8192 rows at least); any other value must be a positive multiple of 64 and is rounded up
 *   to whole spans (a tuning knob: no result depends on it).
 * vs_set_count: out_counts int64 [B] receives the number of set rows.
 * vs_set_ids: per query the set's rows IN ASCENDING ORDER, ranks [offsets[b], offsets[b] + limit) of that list, as row + id_offset in out_ids
 *   int64 [B, limit]; slots behind the last member hold -1; every slot is written.  out_counts [b] is the full size of the set whatever the
 *   window.  offsets int64 [B] or NULL (0); a negative host offset is VS_EINVAL, a negative device one reads as 0; an offset at or past the
 *   count gives all -1.  limit = 0 is count-only (out_ids may be NULL).  B x limit <= 2^27 (VS_SET_MAX_OUT_IDS).
 * vs_set_sample: per query the n set rows with the smallest (h, id), listed in that order -- a uniform sample without replacement, the same for
 *   the same seed, and the same whether the rows are one index or the shards of one (id = row + id_offset, the GLOBAL id, is what is hashed).
 *   All arithmetic modulo 2^64:
 *       mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31      (the splitmix64 finaliser)
 *       k = mix(seeds[b] + 0x9E3779B97F4A7C15);   h = uint32(mix(k ^ (0x9E3779B97F4A7C15 * (id + 1))) >> 32)
 *   (seed, id) -> h: (0, 0) 0x0397ab29, (0, 1) 0xc0737b7c, (1, 0) 0xddc1ed05, (12345, 21015323) 0xfa680e94, (2^64 - 1, 2^32 - 2) 0x29fc86af;
 *   vs_set_sample_hash computes it on the host.  seeds uint64 [B]; out_ids int64 [B, n]; out_hash uint32 [B, n] or NULL: the members' hashes
 *   (what a merge of shards' lists orders by); unused slots hold id -1 and hash 0xFFFFFFFF; every slot is written.  out_counts [b]: the size of
 *   the set.  n in 1..VS_SET_MAX_SAMPLE, n > count is allowed; chunks x B x n <= 2^27 scratch keys, the rule of vs_value_topk.
 * vs_set_from_ids: the inverse of vs_set_ids.  ids int64 [B, ld_ids], m entries a query (m = 0: ids may be NULL) -> out_words [B, ld_words]:
 *   words [0, (bit0 + n_rows + 31) / 32) of each row are written whole, bits below bit0 and past the rows 0 -- the convention of
 *   vs_label_bitmaps.  Bit bit0 + id is set for every listed id in [0, n_rows); ids below 0 are padding and ignored; duplicates are harmless.
 *   An id at or above n_rows: VS_EINVAL in a host array; on the device it is ignored and never written anywhere.  allow = 0 gives the
 *   complement within the rows.  B in 1..65535, bit0 in 0..2^32.
 * Kernels (set_list.hip).  Count: a wave owns a 2048-row span of one query; lane s forms the 64 rows of step s from the two bitmaps' words
 *   (shifted and masked at both ends) and the wave adds the popcounts into span_count uint32 [B, spans].  Scan: one workgroup per query turns
 *   them into exclusive int64 bases and the total.  Write: a wave per span; a span whose ranks [base, base + count) miss the window, or that is
 *   empty, is left WITHOUT READING THE BITMAP; otherwise a wave-exclusive scan of the steps' popcounts gives the step bases, a row's rank is
 *   base + step base + popc(step & lanes below), and rows inside the window are stored at rank - offset with plain stores; a fourth launch
 *   writes the -1 tail.  Sample: the shape of vs_value_topk with the key computed, not loaded -- (~h << 32 | ~row) through the 4096-key LDS
 *   stream per (chunk, query), per-chunk lists and counts in scratch, one workgroup per query merges.  From ids: a clear, a scatter with a
 *   32-bit atomicOr per id, and an invert pass when allow = 0.
 * Errors: NULL outputs (or seeds), n_rows outside 1..2^32 - 1, B < 1, bit0 < 0, B > 1 with ld_words = 0, ld_words too short, rows_per_chunk no
 *   multiple of 64, limit < 0 or B x limit > 2^27, n out of range or too many scratch keys, spans x B > 2^27, host offsets / ids as above:
 *   VS_EINVAL -- checked before the device is touched (without a GPU a bad argument is VS_EINVAL, a good one VS_ENODEVICE).  Pointers: all
 *   host (staged; the call blocks), or all device pointers on `device` / the index's device (VS_EINVAL for a mix).  vs_set_from_ids with device
 *   pointers and a non-NULL stream only enqueues; the others hold device scratch and synchronise the stream before they return.
 * Not covered: payloads gathered with the ids (scores: vs_index_set_scores; values: the caller's array); weighted, stratified or
 *   with-replacement sampling; a rank -> row select call; more than 2^32 - 1 rows; a shard group has no entry point of its own (counts add; a
 *   shard lists its local window [offset - C, offset - C + limit) clipped at 0, C the count of the shards before it, with id_offset = its first
 *   row; samples merge by (h, id)) and the one-process-per-GPU RCCL path has none.                                                          */
#define VS_SET_MAX_SAMPLE 1024        /* rows vs_set_sample lists per query at most */
#define VS_SET_MAX_OUT_IDS 134217728  /* B x limit of one vs_set_ids call: 2^27 */
VS_API uint32_t vs_set_sample_hash(uint64_t seed, int64_t id);
VS_API int vs_set_list_plan(int64_t n_rows, int32_t B, int per_query, int64_t rows_per_chunk, int64_t* out_chunks, int64_t* out_rows_per_chunk,
                            int64_t* out_spans);
VS_API int vs_set_count(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, int64_t n_rows,
                        int64_t rows_per_chunk, int64_t* out_counts, int device, void* stream);
VS_API int vs_index_set_count(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, int64_t rows_per_chunk,
                              int64_t* out_counts, void* stream);
VS_API int vs_set_ids(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, int64_t n_rows,
                      const int64_t* offsets, int64_t limit, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, int64_t* out_counts,
                      int device, void* stream);
VS_API int vs_index_set_ids(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int64_t* offsets,
                            int64_t limit, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, int64_t* out_counts, void* stream);
VS_API int vs_set_sample(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, int64_t n_rows,
                         const uint64_t* seeds, int32_t n, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, uint32_t* out_hash,
                         int64_t* out_counts, int device, void* stream);
VS_API int vs_index_set_sample(vs_index* index, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const uint64_t* seeds, int32_t n,
                               int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, uint32_t* out_hash, int64_t* out_counts,
                               void* stream);
VS_API int vs_set_from_ids(const int64_t* ids, int32_t B, int64_t m, int64_t ld_ids, int64_t n_rows, int64_t bit0, int allow,
                           uint32_t* out_words, int64_t ld_words, int device, void* stream);

/* bool / uint8 mask [B, n] (row stride ld_mask bytes; non-zero = allowed) -> the bitmap words [B, ld_words] vs_index_search_filtered
 * reads (bits past n of a row's last word are 0).  mask and words: host pointers or device pointers on `device` (VS_EINVAL otherwise).  stream as in
 * vs_index_search (host buffers block).                                                                                          */
VS_API int vs_filter_pack(const uint8_t* mask, int32_t B, int64_t n, int64_t ld_mask, uint32_t* words, int64_t ld_words,
                          int device, void* stream);

/* Explain given (query, document id) pairs (no reference call site: what ir.explain(q, p) reports, biencoder.py:111-123, read from the
 * index rows instead of re-embedded texts).  For pair (b, j) with id = ids[b * ld_ids + j]:
 *   out_scores [B, k] fp32: the pair's score.  A CSR-packet index scores the row with the library's exact numerics (fp32 products summed
 *     in fp64, the row summation of the refine step and the exact passes): bit-identical to the score those search paths return for the
 *     pair.  A dense index on the matrix cores: the fp64 sum of the products, equal to its search score to within fp32 rounding.
 *   out_matched [B, k] int32: terms whose product fl32(q[c] * v) is non-zero (> topn: the list below is truncated).
 *   out_cols [B, k, topn] int32 / out_contrib [B, k, topn] fp32: the columns of the topn largest products, contribution descending
 *     then column ascending; unused slots -1 / 0.  May be NULL when topn == 0 (score only).  topn in 0..1024.
 *   id == -1 (a filtered search's padding): cols -1, contrib 0, score -inf, matched 0.  An id whose row id - id_offset is outside the
 *   index: out_matched = -1 and nothing else written for the pair ("not mine": row-sharded callers pick each pair's owner by it).
 *   q == NULL: disentangle mode -- each listed row's own stored values are ranked (contrib = value, 1 for a binary index), the score is
 *   the fp64 sum of the values and out_matched the row's non-zeros.
 *   q: as vs_index_search (rounded to the index dtype).  Host or device pointers (all outputs of one kind); device pointers must live
 *   on the index's device (VS_EINVAL).  With a non-NULL stream and device pointers throughout, a CSR index only enqueues the work.   */
VS_API int vs_index_explain(vs_index* index, const void* q, int q_dtype, int64_t ldq, int32_t B, const int64_t* ids, int64_t ld_ids,
                            int32_t k, int64_t id_offset, int32_t topn, int32_t* out_cols, float* out_contrib, float* out_scores,
                            int32_t* out_matched, void* stream);

/* Query by example (no reference call site: what index.vector[ids] gives the reference, without exporting the index).
 * vs_index_get_rows: the stored rows of ids [n] (row = id - id_offset) as a compact CSR -- out_rowptr int64 [n + 1], out_cols int32 and
 *   out_vals fp32 [out_rowptr[n]]: columns ascending as stored, fp16 values widened exactly, 1 for a binary index, the non-zeros of a dense
 *   (MFMA) row.  Id -1 gives an empty row; any other id outside the index: VS_EINVAL.  Two calls, like vs_index_export_csr: out_cols ==
 *   out_vals == NULL fills out_rowptr only (sizes the others).  Host or device pointers (outputs all of one kind; device pointers on the
 *   index's device).  Blocking.                                                                                                          */
VS_API int vs_index_get_rows(vs_index* index, const int64_t* ids, int64_t n, int64_t id_offset, int64_t* out_rowptr, int32_t* out_cols,
                             float* out_vals, void* stream);
/* vs_index_queries_from_rows: dense fp32 query rows out_q [B, ldo] built from stored rows, with these numerics (fl32 = fp32 rounding):
 *     acc[c] = fl32(alpha * q[b, c])            (0 without q; an fp16 q is widened first)
 *     for j = 0 .. m-1, skipping id -1:  for every stored column c of row ids[b * ld_ids + j]:  acc[c] = fl32(acc[c] + fl32(w[b, j] * v))
 *   weights [B, ldw] fp32 or NULL (all 1); q [B, ldq] VS_F32 | VS_F16 or NULL; m >= 1, ldq and ldo >= n_cols.  Host ids outside [-1, n_rows):
 *   VS_EINVAL (device ids are not read on the host: such rows are skipped).  Host or device pointers; device pointers on the index's device.
 *   With device pointers throughout and a non-NULL stream the call only enqueues the work.                                             */
VS_API int vs_index_queries_from_rows(vs_index* index, const int64_t* ids, int32_t B, int32_t m, int64_t ld_ids, const float* weights,
                                      int64_t ldw, const void* q, int q_dtype, int64_t ldq, float alpha, float* out_q, int64_t ldo,
                                      void* stream);
/* vs_topk_exclude: per query b, its top list ids / scores [B, ld] (kk entries, canonical order) without the ids excl[b * ld_excl + 0 .. m)
 *   (-1 in excl is no id) -> the first k survivors in out_ids / out_scores [B, k]; fewer than k survivors: id -1, score -inf behind them.
 *   Padding (id -1) of a filtered search stays last.  Searching kk = min(k + m, N) and excluding is exact: under the canonical order the top
 *   k of "all rows minus E" lies inside the top k + |E|.  m in 1..16384.  Host or device pointers (device ones on `device`); stream as in
 *   vs_topk_mask.                                                                                                                        */
VS_API int vs_topk_exclude(const int64_t* ids, const float* scores, int32_t B, int32_t kk, int64_t ld, const int64_t* excl, int32_t m,
                           int64_t ld_excl, int32_t k, int64_t* out_ids, float* out_scores, int device, void* stream);

/* ---- mutable index: delete, restore, compact (no reference counterpart: the reference rebuilds its tensor, index.py:163-179) -------------
 * Deletion state lives IN THE HANDLE: a bitmap of live rows (uint32 words, the bit layout of vs_index_search_filtered), allocated by the first
 * deletion and covering the handle's row capacity.
 *   - A handle on which nothing was ever deleted (or whose rows were all restored with ids == NULL) behaves exactly as before: the same
 *     kernels, the same results, the same .vsx bytes.
 *   - With tombstones, vs_index_search / vs_index_search_filtered / vs_shard_group_search* return what vs_index_search_filtered returns for
 *     the bitmap (live AND the caller's filter): bit for bit, canonical order, id -1 / score -inf behind fewer than k live (and allowed)
 *     rows.  No score changes: deletion only gates candidate admission.  k > n_rows (STORED rows) stays VS_ERANGE.  Without a caller's filter
 *     the kernels read the live bitmap itself; with one, a kernel in front of the search, on the same stream, writes live & filter into
 *     scratch of the handle (B x n_rows / 8 bytes for a per-query filter: VS_ENOMEM when that does not fit).
 *   - Row ids do not move.  vs_index_explain, vs_index_get_rows, vs_index_queries_from_rows, vs_index_export_csr, vs_index_scores still read a
 *     deleted row: it stays stored until vs_index_compact, and vs_index_restore_rows depends on that.
 *   - vs_index_append_csr after deletions: the new rows are live.  vs_index_slice_rows carries the slice's bits over.
 *   - vs_index_save_native writes the bitmap behind the three arrays (flagged in the header) when rows are deleted, vs_index_load_native reads
 *     it back; a handle without deleted rows writes the file it always wrote.  vs_index_save_npz of a handle with deleted rows: VS_EINVAL
 *     ("compact first") -- an .npz cannot record them and a reload would resurrect the rows.
 * vs_index_delete_rows: clears the live bits of ids [n] (row = id - id_offset).  Id -1 is ignored; any other id outside the index: VS_EINVAL for
 *   host ids, skipped for device ids (they are not read on the host, as in vs_index_queries_from_rows).  Deleting a row twice -- in one call
 *   or in two -- counts once.  Host or device ids (device ids on the index's device).  stream as in vs_index_search: NULL blocks; device ids
 *   and a non-NULL stream only enqueue (the live count stays on the device).
 * vs_index_restore_rows: sets them again; ids == NULL restores every row.
 * vs_index_live_rows: rows not deleted; synchronises the device.
 * vs_index_live_bitmap: the live bits of rows [0, n_rows) into out_words [n_words >= (n_rows + 31) / 32] (host, or device on the index's
 *   device; bits and words past n_rows are 0): what a caller ANDs with or inspects.  Blocking.                                         */
VS_API int vs_index_delete_rows(vs_index* index, const int64_t* ids, int64_t n, int64_t id_offset, void* stream);
VS_API int vs_index_restore_rows(vs_index* index, const int64_t* ids, int64_t n, int64_t id_offset, void* stream);
VS_API int vs_index_live_rows(const vs_index* index, int64_t* out);
VS_API int vs_index_live_bitmap(const vs_index* index, uint32_t* out_words, int64_t n_words);
/* vs_index_compact: a NEW index on GPU `device` holding the live rows of `src` in order, with room for rows_extra more rows and packets_extra
 *   more 8-nnz packets (vs_index_append_csr).  out_old_ids [live rows] int64 (host, or device on src's device; may be NULL): the row of `src`
 *   that new row j was.  Packets are copied whole on the device -- stored values and their order inside a row do not change, so scores do
 *   not either; nnz is recounted.  fp32 / fp16 / binary stores, a dense index stored as packets (still reported VS_KIND_DENSE), and the dense
 *   matrix kind (row gather; no spare capacity, same device only).  A source without tombstones compacts to a copy with the spare capacity:
 *   that is how an index without reserved room grows.  `src` is untouched and stays the caller's to destroy; the result has no tombstones
 *   and no postings copy yet (vs_index_prepare).  Source and new index are both resident during the call: VS_ENOMEM (the message names the
 *   bytes needed) when HBM cannot hold them -- setting option "blocked_postings" to 0 on `src` releases its postings copy.  Blocking.  */
VS_API int vs_index_compact(const vs_index* src, int64_t rows_extra, int64_t packets_extra, int device, vs_index** out, int64_t* out_old_ids);

/* ---- index pruning: re-sparsify a stored index to its top-m cells (embed(..., topk = m), encoder/vdr.py:102-168: mask = bow_mask | topk_mask) -----
 * The reference fixes a document's sparsity when it embeds it.  For m <= the topk an index was built with, the m largest entries of a row's
 * full embedding are among its stored ones, and a lexical cell outside them is not larger than the smallest: the index built with topk = m is
 * a function of the stored index and of the bag-of-token rows (the protect index).  vs_index_prune makes it on the GPU: a NEW index holding,
 * for every row of a CSR index, a subset of its stored cells.  Rows keep their ids; the source is untouched.
 * For row r with stored cells (col_t, v_t), t = 0..n-1 in STORED ORDER (the order vs_index_export_csr returns; padding cells are not cells):
 *   - eligible_t = col_keep[col_t] and, if min_value is given (not NaN), v_t >= min_value -- compared on the fp32-widened stored value; a NaN
 *     value is never >=.
 *   - key_t = the order key of the numeric fields on the fp32-widened stored value (value_key_f32 of the library's value_check.h): -0.0 and
 *     +0.0 tie, -inf < finite < +inf, a NaN has key 0 and ranks last.  fp16 -> fp32 is monotone: a fp16 store ranks as its halves do.
 *   - rank: among eligible cells, by (key descending, t ascending); top_t = rank < topk.  topk = 0: no cut (every eligible cell is top).
 *   - protected_t = row r of `protect` stores col_t.  protect: a binary or valued CSR index with the same n_rows and n_cols on the same
 *     device (any stored cell counts, whatever its value), or NULL.
 *   - kept_t = eligible_t && (top_t || protected_t): the reference's logical_or(bow_mask, topk_mask) -- the top m is taken over all eligible
 *     cells, protected cells are added and do not count against m.
 *   - the new row = the kept cells in stored order, 8 to a packet, the last packet padded with column id n_cols and value 0; a row with no
 *     kept cell has 0 packets.  Values move as stored bits.
 *   - rows are 1:1 with the source, deleted rows included; the new handle carries the source's tombstones (vs_index_restore_rows brings a
 *     deleted row back pruned).  It has no postings copy yet (vs_index_prepare).
 *   - a binary index (VS_NONE): topk > 0 or a min_value is VS_EINVAL (every value is 1); col_keep alone is allowed.  A dense matrix index:
 *     VS_EUNSUPPORTED; a dense index stored as packets is pruned like any CSR index and stays reported VS_KIND_DENSE.
 * col_keep: uint32 bitmap of n_cols bits (bit c & 31 of word c >> 5), host or device on src's device; NULL: every column.  out_kept: int32
 * [n_rows] kept cells per row, host or device on src's device, may be NULL; col_keep and out_kept together are both host or both device
 * pointers.  topk in 0..65535.  rows_extra / packets_extra / device as in vs_index_compact: spare capacity for vs_index_append_csr, the same
 * 2^32 limits, VS_ENOMEM naming the bytes when HBM cannot hold source and result, the result moved to GPU `device` by peer copies.  nnz = the
 * sum of out_kept.  Three steps on src's GPU: select (a wave a row: rows of up to reg_cells cells are read once and held in registers, longer
 * rows are re-read every pass; an exact radix select on the 32-bit keys; one keep byte a source packet), scan, pack.  Blocking.
 * vs_prune_plan: pure host arithmetic, no device -- reg_cells (the register path's longest row, a constant of the build), the scratch the
 * call allocates next to both indexes (a keep byte a source packet + 4 bytes a row + the scan's block sums: 2 GB at 21 M rows x 96 packets)
 * and the LDS of a select workgroup.  Any output may be NULL.  The shape and rule errors of vs_index_prune: n_cols > 65535 VS_EUNSUPPORTED,
 * topk outside 0..65535 or topk > 0 on VS_NONE: VS_EINVAL.                                                                                  */
VS_API int vs_prune_plan(int64_t n_rows, int64_t n_packets, int32_t n_cols, int store_dtype, int32_t topk, int has_protect, int32_t* out_reg_cells,
                         int64_t* out_scratch_bytes, int32_t* out_lds_bytes);
VS_API int vs_index_prune(const vs_index* src, int32_t topk, float min_value, const uint32_t* col_keep, const vs_index* protect, int64_t rows_extra,
                          int64_t packets_extra, int device, vs_index** out, int32_t* out_kept);

/* ---- sub-index: any rows, in any order, as a new index (no reference counterpart: the reference indexes its tensor, index.py:163-179) ----------
 * vs_index_slice_rows takes a contiguous range, vs_index_compact the live rows in order, vs_index_prune all rows thinner; vs_index_select_rows
 * takes "these rows, in this order": a NEW index on GPU `device` whose row j is row ids[j] - id_offset of `src`.
 *   - Packets are copied whole on the device: column ids, value bits, the order inside a row and the padding of a row's last packet do not
 *     change, so a row scores bit for bit what it scored in `src`.  nnz is recounted, lanes_per_row picked for the new shape, a dense index
 *     stored as packets stays reported VS_KIND_DENSE.  `src` is untouched; the result has no postings copy yet (vs_index_prepare).
 *   - ids [n] int64: any order, repeats allowed (oversampling, a bootstrap); host pointers, or device pointers on src's device.  Every id has
 *     to name a stored row: an id outside [id_offset, id_offset + n_rows) -- -1 included -- is VS_EINVAL and no handle is made.  Host ids are
 *     checked on the host; device ids by the first kernel, whose flag is read back with the totals.  n == 0: VS_EINVAL ("empty selection").
 *   - Tombstones travel with the rows: with deletions on `src`, new row j is deleted iff its source row is (the live count is right, and
 *     vs_index_restore_rows on the result brings the row back).  A source without tombstones, or a selection without a deleted row, gives a handle without a live bitmap: it
 *     behaves, and is written to .vsx, as an index built from the same CSR.
 *   - fp32 / fp16 / binary stores.  The dense matrix kind: a row gather of the padded matrix, rows_extra == packets_extra == 0 and the same
 *     device only, as in vs_index_compact.
 *   - rows_extra / packets_extra / device, the 2^32 row and packet limits (repeats can select more packets than `src` stores: the sum is taken
 *     in 64 bits) and the VS_ENOMEM naming the bytes are vs_index_compact's.  Blocking.
 * Four steps on src's GPU: stat (a thread an id: the range check and the source row's packets, summed over blocks of 4096 ids), the scan of
 * the block sums and map (the new row pointers; with tombstones the live words of the new rows, two whole words a wave from a ballot), gather
 * (a wave takes 64 new rows -- one contiguous packet range of the new index -- and issues the loads of four 64-packet steps, held in registers,
 * before it stores),
 * the recount of the non-zeros.
 * vs_select_plan: pure host arithmetic, no device -- the scratch the call allocates next to both indexes: 8 bytes an id (host ids are staged
 *   on the device), the block sums, the totals.  n outside 1..2^32 - 2: VS_EINVAL.  The output may be NULL.
 * vs_select_split: pure host arithmetic -- how a selection of GLOBAL ids is dealt to the shards of a row-sharded index.  Shard s holds the
 *   rows [cuts[s], cuts[s + 1]) (cuts [n_shards + 1] int64, ascending from 0); the ids are dealt IN THE ORDER GIVEN, out_begin [n_shards + 1]:
 *   positions [out_begin[s], out_begin[s + 1]) of ids belong to shard s.  The shards side by side are the unsharded selection exactly when
 *   the shard of ids[i] never decreases along i; a list that goes back to an earlier shard would move a row across shards: VS_EINVAL, as is
 *   an id outside [0, cuts[n_shards]).  Host pointers only.                                                                                 */
VS_API int vs_select_plan(int64_t n_ids, int64_t* out_scratch_bytes);
VS_API int vs_select_split(const int64_t* ids, int64_t n, const int64_t* cuts, int32_t n_shards, int64_t* out_begin);
VS_API int vs_index_select_rows(const vs_index* src, const int64_t* ids, int64_t n, int64_t id_offset, int64_t rows_extra, int64_t packets_extra,
                                int device, vs_index** out);

/* ---- reweighted index: row statistics, and cells rescaled by row and column (no reference counterpart: the reference multiplies its tensor) ------
 * Every call above moves stored cells without changing a value.  vs_index_row_stats reads a row's magnitude, vs_index_rescale makes a NEW
 * index with the source's sparsity and new values.  Row r has stored cells (col_t, v_t), t = 0..n-1 in STORED ORDER (the order
 * vs_index_export_csr returns; padding cells are not cells); w_t is v_t widened to fp32, and 1 on a binary index (VS_NONE).
 * vs_index_row_stats: n_rows entries each, any output may be NULL, the non-NULL ones all host pointers or all device pointers on src's device.
 *   - cells[r]   = n, the stored cells.
 *   - nonzero[r] = the cells with w_t != 0 (+0.0 and -0.0 are zero): the term constraints' "has a column".
 *   - l1[r]      = the sum of fp64(|w_t|);  sumsq[r] = the sum of fp64(w_t) * fp64(w_t), each product exact in fp64.  Both are fp64 sums in
 *     ONE pinned order, the order of the exact scores: lane l of the row's wave (l = 0..63) adds the cells of packets p0 + l, p0 + l + 64, ...
 *     cell by cell from +0.0 (a packet holds 8 consecutive cells; p0 is the row's first packet), then for o = 32, 16, .. 1 every lane adds the sum
 *     of lane l xor o to its own.  A loop on the host reproduces them bit for bit whatever the magnitudes (a NaN cell gives some NaN).  No
 *     square root is taken: that keeps every output reproducible.
 *   - max[r]     = the largest w_t as fp32; a NaN cell is skipped, a zero maximum is +0.0 whatever the signs of the zeros, a row with no
 *     non-NaN cell gives NaN (0x7FC00000), the numeric fields' "no value".
 *   An empty row has 0 / 0 / +0.0 / +0.0 / NaN.  Deleted rows are stored rows and get their statistics.  A dense matrix index: VS_EUNSUPPORTED;
 *   a dense index stored as packets is a CSR index here.  One wave a row, 64 consecutive rows a wave, 256 a workgroup: the outputs are written
 *   as runs.  Blocking.
 * vs_index_rescale: a NEW index on GPU `device` with src's row pointers, src's packets' column ids bit for bit (padding included), src's
 *   tombstones (as vs_index_prune carries them: vs_index_restore_rows brings a deleted row back rescaled), src's nnz, and no postings copy yet
 *   (vs_index_prepare).  `src` is untouched.  row_scale [n_rows], col_scale [n_cols]: float32, each a host pointer or a device pointer on src's
 *   device, each may be NULL = a scale of 1 that is not multiplied in.  out_dtype: VS_F32 or VS_F16 (VS_NONE: VS_EINVAL, binarising is not covered).
 *   - a real cell: x = fl64(fl64(fp64(w) * fp64(row_scale[r])) * fp64(col_scale[col])), products left to right, a NULL scale skipped; the stored
 *     value is fl32(x), for a fp16 result fl16(fl32(x)), both roundings to nearest even.  With one scale the fp64 product is exact: the fp32
 *     value is the correctly rounded fp32 product w * s.  With no scale and out_dtype == src's dtype the value bits are copied.
 *   - scales are data and are not checked: zero, negative, infinite and NaN scales give the IEEE result (a NaN result is any NaN); subnormal
 *     results are kept, never flushed.
 *   - a padding cell keeps id n_cols and value +0 whatever the scales are (an infinite scale does not turn it into a NaN): no scale applies to it.
 *   - a binary source has w = 1 in every real cell and becomes a valued index.  A dense matrix index: VS_EUNSUPPORTED.
 *   - rows_extra / packets_extra / device, the 2^32 row and packet limits and the VS_ENOMEM naming the bytes are vs_index_compact's.  Blocking.
 *   One kernel on src's GPU: a wave takes 64 consecutive rows (one contiguous packet range), a lane a packet -- it finds the packet's row among
 *   the run's row pointers (only with a row scale), reads ids and values once and writes ids and values once, four 64-packet steps in flight.
 * vs_rescale_plan: pure host arithmetic, no device -- the scratch the call allocates next to both indexes when the scales given are host
 *   pointers (4 bytes a row, 4 a column), the LDS of a workgroup, and out_col_route: 0 = no column scales, 1 = the column scales are held as an
 *   LDS image (n_cols <= 40 960: the image fits the 160 KB of a CU), 2 = they are read from memory.  Any output may be NULL.  n_cols > 65535:
 *   VS_EUNSUPPORTED; a bad dtype, out_dtype VS_NONE, a negative count: VS_EINVAL.                                                            */
VS_API int vs_index_row_stats(const vs_index* src, int32_t* out_cells, int32_t* out_nonzero, double* out_l1, double* out_sumsq, float* out_max);
VS_API int vs_rescale_plan(int64_t n_rows, int64_t n_packets, int32_t n_cols, int src_dtype, int out_dtype, int has_row_scale, int has_col_scale,
                           int64_t* out_scratch_bytes, int32_t* out_lds_bytes, int32_t* out_col_route);
VS_API int vs_index_rescale(const vs_index* src, const float* row_scale, const float* col_scale, int out_dtype, int64_t rows_extra,
                            int64_t packets_extra, int device, vs_index** out);

/* ---- combined index: the weighted cell-wise sum of two indexes of the same rows (no reference counterpart: the reference adds its tensors) ---------
 * Every index-to-index call above keeps or shrinks the source's sparsity.  vs_index_combine makes a NEW index on GPU `device` whose row r is
 * wa * (row r of a) + wb * (row r of b), cell by cell.  A score is linear in the stored cells -- q . (wa A + wb B)^T = wa q . A^T + wb q . B^T --, so
 * a search of the result ranks by the weighted sum of the two scores, over the whole corpus.  `a` and `b` are untouched.
 *   - sources: CSR-kind indexes (fp32, fp16 or binary store, independently) on the same GPU with equal n_rows and equal n_cols; a == b is
 *     allowed.  A dense matrix index: VS_EUNSUPPORTED; a dense index stored as packets is combined like any other (the result is reported
 *     VS_KIND_DENSE when both sources are).  Unequal shapes, different devices, NULL handles, out_dtype outside {VS_F32, VS_F16}: VS_EINVAL
 *     (VS_NONE: binarising is not covered).
 *   - the columns of result row r: the set of columns either source row stores, each once, in ASCENDING column order, 8 to a packet, the last
 *     packet padded with column id n_cols and value +0; a row with no cell has 0 packets.  The sparsity is the union of the STORED cells: an
 *     explicitly stored zero is a cell, and a sum that cancels to zero stays a cell.  The stored order inside the source rows is arbitrary
 *     and does not enter.
 *   - a source row that stores one column twice would make the sum depend on the order: VS_EINVAL naming the source and the lowest such row
 *     (index a before index b at the same row).  The count step finds it on the device; nothing is allocated for the result.
 *   - values: w = the stored value widened to fp32 (1 for a binary source); a column in both rows gets x = fp64(wa) * fp64(w_a) + fp64(wb) *
 *     fp64(w_b), a column in one row the one product, in fp64 -- each product is exact there, the sum is rounded once.  The stored value is
 *     fl32(x), for a fp16 result fl16(fl32(x)), both roundings to nearest even: numpy's np.float32(np.float64(wa) * a + np.float64(wb) * b)
 *     reproduces every bit.  Weights are data: 0, negative, infinite and NaN weights give the IEEE result (a NaN result is any NaN);
 *     subnormal results are kept, never flushed.
 *   - tombstones: cells come from the stored rows whether or not a row is deleted; the result's deleted rows are a's OR b's, and
 *     vs_index_restore_rows brings them back combined.  The result has no postings copy yet (vs_index_prepare).
 *   - rows_extra / packets_extra / device, the 2^32 row and packet limits and the VS_ENOMEM naming the bytes are vs_index_prune's; nnz = the
 *     union cells; lanes_per_row is picked for the new shape.  Blocking.
 * Three steps on the sources' GPU.  count: a wave a row sets the row's columns in two per-wave LDS bitmaps of n_cols bits (LDS atomicOr; a
 *   bit found set already is the repeated column), counts b's cells whose bit a's bitmap lacks -- the union is a's cells plus those -- and
 *   clears the words it set by walking the packets again.  scan: the new row pointers, the non-zeros summed on the way.  fill: the same
 *   bitmaps plus a per-word exclusive popcount prefix of the union; a cell's place in the result row is prefix[word] + popc(union bits below
 *   it) -- no sort and no atomic decides a place.  The row is staged in LDS, one 32-bit slot a union cell: a's lanes store the final bits of
 *   the columns b lacks and the raw value of the shared ones, b's lanes then finish the shared columns and their own; ids (from the union's
 *   set bits) and values leave as 16-byte stores.  Rows with cells_a + cells_b <= wave_cells (2048) are filled a wave a row, four waves a
 *   workgroup (a row of up to 1024 cells a side is read once and held in registers, a longer one is read again by every pass); a longer row by one 1024-thread
 *   workgroup, whose slots hold a union of up to group_cells (32 768) cells.  A larger union is
 *   possible only beyond 32 768 columns: VS_EUNSUPPORTED from the count step, naming the row.
 * vs_combine_plan: pure host arithmetic, no device -- the limits of the two routes, the LDS of a fill workgroup of either route, and the
 *   scratch the call allocates next to the three indexes (4 bytes a row, the list of long rows, the scan's block sums).  Any output may be
 *   NULL.  n_cols > 65535: VS_EUNSUPPORTED; a bad dtype, out_dtype VS_NONE, a negative count: VS_EINVAL.                                    */
VS_API int vs_combine_plan(int64_t n_rows, int64_t packets_a, int64_t packets_b, int32_t n_cols, int dtype_a, int dtype_b, int out_dtype,
                           int32_t* out_wave_cells, int32_t* out_group_cells, int32_t* out_wave_lds_bytes, int32_t* out_group_lds_bytes,
                           int64_t* out_scratch_bytes);
VS_API int vs_index_combine(const vs_index* a, const vs_index* b, float wa, float wb, int out_dtype, int64_t rows_extra, int64_t packets_extra,
                            int device, vs_index** out);

/* ---- joined index: the rows of several indexes, one source behind the other, as a new index (reference: vstack(shards), index.py:172-175) --------
 * vs_index_select_rows picks rows of ONE index, vs_index_combine unions the cells of two indexes of the same rows; vs_index_concat puts the
 * rows of srcs[1] behind those of srcs[0], and so on: a NEW index on GPU `device`.  The sources are untouched.
 *   - sources: n_src in 1..256 CSR-kind handles on one GPU with equal n_cols; fp32, fp16 and binary stores may be mixed freely, the same handle
 *     may appear more than once, a source with 0 rows contributes nothing.  A total of 0 rows: VS_EINVAL ("empty join").  A dense matrix index:
 *     VS_EUNSUPPORTED; a dense index stored as packets joins like any other (the result is reported VS_KIND_DENSE only when every source is).
 *     A NULL handle, unequal widths, sources on different GPUs, n_src outside 1..256, negative extras: VS_EINVAL.
 *   - out_dtype: VS_F32 or VS_F16; VS_NONE only when every source is binary -- the result is then binary --, otherwise VS_EINVAL (binarising
 *     is not covered).
 *   - row pointers: with R_s and P_s the rows and the packets of the sources before source s, new row pointer R_s + r is src_pk_s[r] + P_s;
 *     the last pointer is the packet total.
 *   - packets move whole: the 16 bytes of column ids, padding included, are copied bit for bit.  A source whose store equals out_dtype has its
 *     value bits copied; a source of another store is converted cell by cell under vs_index_rescale's rule with no scale: fp16 -> fp32 is
 *     exact, fp32 -> fp16 rounds once to nearest even (overflow to +-inf, subnormals kept, a NaN stays a NaN), a binary source's real cell
 *     becomes 1.0, and a padding cell keeps id n_cols and value +0 whatever the source store was.  A row therefore scores bit for bit what
 *     it scored in a source of the result's dtype.
 *   - tombstones travel with the rows: a result row is deleted iff its source row is.  When no source row is deleted the handle has no live
 *     bitmap: it behaves, and is written to .vsx, as an index built from the joined CSR.  Bits past the last row stay set.
 *   - nnz is the sum of the sources' nnz, lanes_per_row is picked for the new shape, the result has no postings copy yet (vs_index_prepare).
 *   - rows_extra / packets_extra / device, the 2^32 row and packet limits, the VS_ENOMEM naming the bytes and the move to another GPU are
 *     vs_index_select_rows's.  Blocking.
 * Two launches on the sources' GPU whatever n_src is.  A device table of per-source entries (row base, packet base, the four array pointers,
 * the store, the live words or NULL) is read into LDS once by every workgroup.  map: a thread a result row finds its source by a branch-free
 * search over the row bases and writes the rebased pointer; with tombstones on any source the live words of the new rows, two whole words a
 * wave from a ballot, and the dead count.  copy: a wave takes 256 contiguous result packets, a lane a packet of each 64-packet step; a step
 * whose first and last packet fall into one source takes that source for all lanes (decided wave-uniformly), a step across a boundary
 * searches a lane at a time; the loads of four steps, 16 bytes each, are in flight before the first store, values are converted in registers.
 * vs_concat_plan: pure host arithmetic, no device -- rows [n_src], packets [n_src], dtypes [n_src] of the sources -> the totals, the scratch
 *   the call allocates next to the indexes (48 bytes a source for the table + the counters) and the LDS of a workgroup.  Any output may be
 *   NULL.  The shape errors of the call; n_cols > 65535 and totals of 2^32 - 1 rows or 2^32 packets and more: VS_EUNSUPPORTED.              */
VS_API int vs_concat_plan(int32_t n_src, const int64_t* rows, const int64_t* packets, int32_t n_cols, const int* dtypes, int out_dtype,
                          int64_t* out_rows, int64_t* out_packets, int64_t* out_scratch_bytes, int32_t* out_lds_bytes);
VS_API int vs_index_concat(const vs_index* const* srcs, int32_t n_src, int out_dtype, int64_t rows_extra, int64_t packets_extra,
                           int device, vs_index** out);

/* ---- term constraints: must / must-not / should filters built from the index's own columns (no reference counterpart) --------------------
 * A row HAS term c (a column id in [0, n_cols)) iff it stores column c with a non-zero value; under a threshold thr, iff the stored value
 * v satisfies v >= thr (an fp16 store widens exactly, as vs_index_get_rows; a binary index stores 1; a stored zero counts under thr <= 0).
 * The packets' padding column never matches; a dense index on the matrix cores stores its non-zero elements (vs_index_get_rows).  Tombstones do not enter: a deleted row still reports its terms (the search ANDs the live
 * bitmap itself).  A program (must, must_not, should, min_should) allows row r iff r has every must term, no must_not term and at least
 * min_should of the should terms: empty lists constrain nothing, min_should <= 0 constrains nothing, min_should above the number of should
 * terms allows no row.  Bitmaps have the layout of vs_index_search_filtered (row r = bit r & 31 of word r >> 5).
 * vs_index_term_bitmaps: out_words [T, ld_words] (ld_words >= W = (n_rows + 31) / 32): bitmap t holds the rows that have cols[t] (under
 *   thr[t] when thr != NULL; a NaN thr[t] = no threshold for that term).  Words [0, W) of every bitmap are written whole, the bits past
 *   n_rows are 0; words [W, ld_words) are not touched.  T in 1..4096; duplicate terms give identical bitmaps; a column outside [0, n_cols):
 *   VS_EINVAL.  out_df [T] int64 (may be NULL): the set bits of every bitmap -- of its live rows only when live_only != 0.
 *   One pass over the packets' column ids serves up to VS_TERM_FILTER_SLOTS distinct terms (more: further passes); values are read only for
 *   the entries whose column is a term.  cols / thr: host arrays (control data; device arrays are copied back first, which synchronises
 *   the stream).  out_words / out_df: host pointers, or device pointers on the index's device: with those and a non-NULL stream a CSR-packet
 *   index only enqueues work.
 * vs_term_filter_combine: out_words [B, out_ld] from T term bitmaps term_words [T, ld_words] of n_rows rows.  must / must_not / should:
 *   [B, n_*] indices into the T bitmaps, padded with -1, each at most VS_TERM_FILTER_LIST wide (NULL with n_* = 0); min_should [B] (NULL: 0).
 *   B = 1 is a program shared by the batch.  Words [0, W) of every output bitmap are written (bits past n_rows 0); when out_ld is a multiple
 *   of 4 words and out_words is 16-byte aligned, so are the zero words up to the next multiple of 4.  An index outside [-1, T): VS_EINVAL for
 *   host lists, ignored for device lists.  All pointers host, or all device pointers on `device`; with device pointers and a non-NULL stream
 *   the call only enqueues work.                                                                                                          */
#define VS_TERM_FILTER_SLOTS 255     /* distinct terms one pass of the scan serves */
#define VS_TERM_FILTER_TERMS 4096    /* terms a call takes at most */
#define VS_TERM_FILTER_LIST  64      /* entries of a must / must_not / should list at most */
VS_API int vs_index_term_bitmaps(vs_index* index, const int32_t* cols, const float* thr, int32_t T, uint32_t* out_words, int64_t ld_words,
                                 int64_t* out_df, int live_only, void* stream);
VS_API int vs_term_filter_combine(const uint32_t* term_words, int64_t ld_words, int64_t n_rows, int32_t T, const int32_t* must, int32_t n_must,
                                  const int32_t* must_not, int32_t n_must_not, const int32_t* should, int32_t n_should,
                                  const int32_t* min_should, int32_t B, uint32_t* out_words, int64_t out_ld, int device, void* stream);

/* ---- grouped search: the top k GROUPS of a ranking, each with its best m rows (field collapsing; no reference counterpart) ----------------
 * groups [n_rows] int32, every value >= 0: rows with equal values form a group (a row with a negative value is never kept).  For a query
 * let L be the canonical ranking (score descending, id ascending) of its live, allowed rows.  L is walked in order with a set of OPEN groups:
 * a row whose group is open and holds fewer than m kept rows is kept as that group's next member; a row whose group is not open opens it,
 * and is kept as its first member, iff fewer than k groups are open; every other row is skipped.  The result: the open groups in opening
 * order (the order of their best rows), each with its kept rows in keep order.  The walk runs in ROUNDS: a search to some depth under a
 * filter, vs_topk_collapse over its list, and -- for the queries the list did not complete -- vs_group_filter for the next, deeper search.
 * The state between the rounds is the result itself:
 *   out_group [B, k] int32 (-1: unused slot), out_count [B, k] int32 (rows kept of the slot), out_ids [B, k, m] int64 / out_scores [B, k, m]
 *   fp32 (unused member slots: id -1, score -inf; scores are copied from the lists bit for bit), out_status [B] int32 (1 = complete).
 * vs_topk_collapse: continues the walk of query qmap[i] (qmap == NULL: query i) over list i of ids / scores [Bp, ld] (kk entries, canonical
 *   order) for i = 0 .. Bp-1; a query must be listed once at most.  init != 0: the listed queries start from the empty state and their unused
 *   slots are padded; init == 0: they go on from their state (a query whose status is 1 is left as it is).  A list ends at its first id -1
 *   (the padding of a filtered search).  A query is complete when its list ended inside the kk entries, when exhausted_hint != 0 (the
 *   caller searched kk == n_rows: nothing ranks behind the list), or when k groups are open and all hold m rows.  *out_incomplete (int32 [1]) =
 *   the listed queries left incomplete.  k in 1..1024, m in 1..64, k * m <= 8192, kk in 1..16384; anything else: VS_EINVAL.  An id outside
 *   [-1, n_rows): VS_EINVAL for host lists; a device list ends there (it is not read on the host).  One wave per query, the open groups in an
 *   LDS table; no thread walks a list serially.
 * vs_group_filter: the rows the next round of the Bp listed queries has to rank, as bitmaps out_words [Bp, ld_words] in the layout of
 *   vs_index_search_filtered: row r is allowed for list i (query b = qmap[i]) iff the caller's filter allows it (filter + b * filter_ld;
 *   filter_ld = 0: one bitmap for the batch; filter == NULL: none), r is not a kept row of b, r's group is not full, and r's group is open or
 *   fewer than k groups are.  Every row outside it is kept already or would be skipped whatever comes later, so the next list ranks wholly behind
 *   this one.  Words [0, (n_rows + 31) / 32) of every bitmap are written whole, bits past n_rows 0.  Tombstones do not enter: the search ANDs
 *   the live bitmap itself.  The bitmaps cost what any per-query filter costs (Bp x n_rows / 8 bytes): VS_ENOMEM, with the size in the message,
 *   when a host caller's do not fit on the device.
 * Both: all buffers host pointers, or all device pointers on `device` (VS_EINVAL for a mix); host buffers are staged and the call blocks; device
 * pointers and a non-NULL stream only enqueue, as vs_topk_exclude.
 * Not covered: `groups` is the caller's array -- no index file (.vsx, .npz) stores it, and vs_index_compact does not remap it (the Python
 * facade does both sides of that: Index.compact / add(groups=)); a shard group has no entry point of its own -- its rounds are
 * vs_shard_group_search_filtered with global groups and bitmaps on the first shard's device; the one-process-per-GPU RCCL path has none.   */
VS_API int vs_topk_collapse(const int64_t* ids, const float* scores, int32_t Bp, int32_t kk, int64_t ld, const int32_t* qmap,
                            const int32_t* groups, int64_t n_rows, int32_t B, int32_t k, int32_t m, int32_t* out_group, int32_t* out_count,
                            int64_t* out_ids, float* out_scores, int32_t* out_status, int32_t* out_incomplete, int init, int exhausted_hint,
                            int device, void* stream);
VS_API int vs_group_filter(const int32_t* groups, int64_t n_rows, int32_t Bp, const int32_t* qmap, int32_t B, int32_t k, int32_t m,
                           const int32_t* state_group, const int32_t* state_count, const int64_t* state_ids, const uint32_t* filter,
                           int64_t filter_ld, uint32_t* out_words, int64_t ld_words, int device, void* stream);

/* ---- diversified search: Maximal Marginal Relevance over a hit list (Carbonell & Goldstein 1998; no reference counterpart) -----------------
 * vs_mmr_select_csr picks k of each query's kk candidates greedily, every pick trading relevance against similarity to the picks before it.
 * Query b's candidates are ids / scores [b * ld, b * ld + kk) in the search's canonical order; candidate j's stored row is row b * kk + j of
 * the compact CSR (rowptr [B * kk + 1] int64, cols int32, vals fp32 -- what vs_index_get_rows / vs_shard_group_get_rows write for the
 * flattened ids; columns of a row distinct).  The n candidates of a query are the entries before its first id -1; the rest is ignored.
 *   g(i, j) = fl32(sum over shared columns of fp64(fl32(v_i[c] * v_j[c])))      (the library's score numerics; the sum's order is free)
 *   VS_MMR_COSINE: rel_j = fl32(s_j / s_0) when s_0 > 0, else s_j;  sim(i, j) = fl32(fp64(g(i, j)) / sqrt(fp64(g(i, i)) * fp64(g(j, j)))),
 *                  sqrt and division in fp64; 0 when either diagonal is 0
 *   VS_MMR_DOT:    rel_j = s_j;  sim(i, j) = g(i, j)
 *   pen_j = 0; after a pick p every unpicked j takes pen_j = sim(p, j) where that is larger; an unpicked j is worth
 *   val_j = fl32(fl32(lam_b * rel_j) - fl32(mu_b * pen_j)), mu_b = fl32(1 - lam_b), no fused multiply-add; the largest val is picked, the lower
 *   list position on a tie; min(k, n) picks.  Scores are expected finite (no NaN).
 * Outputs, all [B, k]: out_ids int64, out_scores fp32 (the list's own score bits), out_pos int32 (position in the list), out_mmr fp32 (val at
 * pick time), out_pen fp32 (pen at pick time); unused slots: id -1, score -inf, pos -1, mmr -inf, pen 0.  Every slot is written.  lam [B] fp32.
 * Limits: kk and k in 1..VS_MMR_MAX_DEPTH (else VS_EINVAL); n_cols <= 32768, the LDS image (VS_EUNSUPPORTED beyond it: no column tiles).
 * All buffers host pointers, or all device pointers on `device` (VS_EINVAL for a mix).  Host arrays are checked (rowptr monotone, columns
 * in [0, n_cols), lam in [0, 1]: VS_EINVAL, nothing written), staged, and the call blocks.  Device arrays are not read on the host: rowptr is
 * trusted, a column outside [0, n_cols) is skipped as if the cell were absent; with a non-NULL stream the call only enqueues.
 * One workgroup per query: an fp32 LDS image of the last pick's row, one wave per candidate; no float atomics, so results are deterministic. */
#define VS_MMR_COSINE 0
#define VS_MMR_DOT    1
#define VS_MMR_MAX_DEPTH 1024
VS_API int vs_mmr_select_csr(const int64_t* rowptr, const int32_t* cols, const float* vals, const int64_t* ids, const float* scores, int32_t B,
                             int32_t kk, int64_t ld, int32_t n_cols, const float* lam, int32_t k, int mode, int64_t* out_ids, float* out_scores,
                             int32_t* out_pos, float* out_mmr, float* out_pen, int device, void* stream);

/* ---- fused search: rank and score fusion of hit lists (reciprocal rank fusion: Cormack, Clarke & Buettcher 2009; CombSUM / CombMNZ: Fox &
 * Shaw 1994; no reference counterpart) ---------------------------------------------------------------------------------------------------
 * vs_fuse_topk merges L hit lists per query into one: the union of their ids, every id given a fused value from its rank or score in each
 * list, the top k of them.  List l of query b is ids / scores [l * list_stride + b * ld, + kk) (int64 / fp32).  A list ends at its first id -1
 * (a filtered search's padding); what stands behind it is ignored.  An id may stand in several lists; an id twice in ONE list counts at its
 * lowest position, the later entries are ignored (they still take part in mx_l / mn_l below).
 * Contribution c_l of list l to document d at 0-based position r with score s (fl32 = rounded to fp32, never a fused multiply-add):
 *   VS_FUSE_RRF: fl32(w_l / fl32(rrf_c + (float)(r + 1))); scores are not read for it (NaN / inf scores are harmless); absent from l: +0
 *   VS_FUSE_SUM: fl32(w_l * n), n = fl32(fl32(s - mn_l) / fl32(mx_l - mn_l)), mx_l / mn_l the largest / smallest score among the entries of
 *                list l of this query (-0.0 ordered below +0.0), n = 1 when mx_l == mn_l (weighted CombSUM, min-max normalised); absent: +0
 *   VS_FUSE_MNZ: as VS_FUSE_SUM
 *   VS_FUSE_RAW: fl32(w_l * s); absent: fl32(w_l * fill[b * ldf + l]), 0 without fill (fill is read in this mode only)
 *   fused(d) = fl32(...fl32(fl32(c_0 + c_1) + c_2)... + c_{L-1}), in list order; VS_FUSE_MNZ then multiplies once: fl32(fused * (float)m), m the
 *   number of lists holding d.  The lists need not be sorted for the score modes; RRF reads the position as the rank, so its callers pass
 *   lists in the search's canonical order.  Scores are expected finite in the three score modes.
 * weights fp32: ldw == 0 -> [L] for the batch, else [B, ldw] (w_l of query b = weights[b * ldw + l]); NULL = all 1.
 * Result: fused descending, compared as floats (-0.0 and +0.0 tie), then id ascending; min(k, out_n[b]) results.  out_ids [B, k] int64,
 * out_fused [B, k] fp32, out_ranks [B, k, L] int32 (0-based position in list l, -1 = not in it), out_scores [B, k, L] fp32 (list l's own score
 * bits, -inf where absent), out_n [B] int32 (the size of the union, whatever k is).  Unused slots: id -1, fused -inf, ranks -1, scores -inf.
 * Every slot is written.
 * Limits (VS_EINVAL beyond them): L in 1..VS_FUSE_MAX_LISTS, kk and k in 1..VS_FUSE_MAX_DEPTH, L * kk <= VS_FUSE_MAX_ENTRIES, ld >= kk,
 * list_stride >= (B - 1) * ld + kk when L > 1, ldw 0 or >= L, ldf >= L, a valid mode, finite rrf_c >= 0 (conventionally 60), ids in
 * [-1, 2^32 - 1): the keys hold 32-bit ids, as in vs_merge_topk.
 * All buffers host pointers, or all device pointers on `device` (VS_EINVAL for a mix).  Host arrays are checked (ids in range in front of a
 * list's first -1, weights and fill finite: VS_EINVAL, nothing written), staged, and the call blocks.  Device arrays are not read on the host:
 * an id outside the range ends its list there, as in vs_topk_collapse; with a non-NULL stream the call only enqueues.
 * One workgroup per query: the L * kk entries sorted once as 64-bit keys (id : list : position) in LDS, so that a document's entries are
 * adjacent and its first entry of a list is its lowest position; the documents ranked by a second sort of (fused, position of the run).  No
 * float atomics, so results are deterministic.
 * Not covered: z-score normalisation; more than 8 lists or L * kk > 4096; the one-process-per-GPU RCCL path has no entry of its own (its
 * lists after vs_merge_topk are ordinary lists).                                                                                       */
#define VS_FUSE_RRF 0
#define VS_FUSE_SUM 1
#define VS_FUSE_MNZ 2
#define VS_FUSE_RAW 3
#define VS_FUSE_MAX_LISTS   8
#define VS_FUSE_MAX_DEPTH   1024
#define VS_FUSE_MAX_ENTRIES 4096
VS_API int vs_fuse_topk(const int64_t* ids, const float* scores, int32_t L, int32_t B, int32_t kk, int64_t ld, int64_t list_stride,
                        const float* weights, int64_t ldw, const float* fill, int64_t ldf, int mode, float rrf_c, int32_t k, int64_t* out_ids,
                        float* out_fused, int32_t* out_ranks, float* out_scores, int32_t* out_n, int device, void* stream);

/* Dense score matrix [B, n_rows] fp32 -- the intermediate index.py:91 materialises.  Used by the
 * parity tests to check every score, not just the top-k.                                         */
VS_API int vs_index_scores(vs_index* index, const void* q, int q_dtype, int64_t ldq, int32_t B,
                           float* out_scores, void* stream);

VS_API int  vs_index_info(const vs_index* index, vs_index_info_t* out);

/* Scan selection (tuning / tests; no reference counterpart): 0 = auto -- score tiles of 8 sparse queries
 * per pass over the index when every query is sparse enough for the LDS tile tables (512 ranks per
 * pass; larger k takes several passes), else one query per pass with a dense fp32 query image;
 * 1 = always the latter.                                                                          */
VS_API int  vs_index_set_queries_per_pass(vs_index* index, int qt);

/* Builds NOW what the first sparse search would otherwise build inside the call (the blocked-postings copy: 0.5 s at 21 M docs):
 * Index.move_to_device / load_index / build_index of the Python facade call it, so a user's first retrieve() pays nothing extra.
 * Idempotent; indexes that get no copy return at once.  vs_index_info_t.postings_state tells what happened.  stream as in
 * vs_index_search (NULL = blocking).                                                                                           */
VS_API int  vs_index_prepare(vs_index* index, void* stream);

/* Tuning / test options by name (no reference counterpart):
 *   "queries_per_pass"  as above
 *   "blocked_postings"  -1 = auto (long-row valued indexes, when HBM has room for the second copy), 0 = off, 1 = on:
 *                       sparse queries are scored from a row-blocked, column-grouped copy of the index that is built on
 *                       first use -- a query tile reads only the posting lists of its own columns
 *   "postings_rows"     0 = auto (a column's list in a block averages ~50 postings, at most 2048 documents; the bag-of-token chunks of a
 *                       binary index: ~18 postings, at most 8192), else documents per block of the copy (a multiple of 64 in 256..8192,
 *                       clipped to what the index's walk holds)
 *   "postings_chunks"   0 = auto, else the number of block runs the postings scan cuts the index into (work items = tiles x runs)
 *   "postings_filter"   1 (default) = the postings walk accumulates int32 fixed-point sums (3.4x the LDS atomic rate of fp64 on
 *                       MI355X) and returns k + max(28, k/4) candidates per query, which are re-scored with the exact numerics
 *                       and PROVEN to contain the top k; unproven queries re-run on the exact one-query scan of the CSR packets
 *                       (exact_scan_topk_kernel).  Results are identical to 0 = fp64 walk only
 *   "postings_quant"    1 (default) = an fp32 index keeps fp16-rounded values in the postings copy (the filter only ranks
 *                       candidates; the refine step re-scores them from the fp32 CSR), 0 = fp32 values there too
 *   "postings_walk"     which copy / kernel serves the filter: -1 = auto -- a valued index gets QUAD CHUNKS (bp_quad.h: 256-byte chunks of 64
 *                       postings per (block, column), walked by a generated asm loop) while they stay within 3 x the CSR bytes, else the
 *                       list walk over records; a binary index gets BAG-OF-TOKEN CHUNKS (bp_bq.h: 64-byte chunks of 32 document ids);
 *                       0 = the list walk over records (bp_walk.h: a list per 8-lane group), 4 = quad chunks whatever their size,
 *                       5 = the record walk of a binary index (bp_bin.h), 6 = bag-of-token chunks; 1 - 3 = the experimental walks of round 3,
 *                       removed (VS_EUNSUPPORTED; their measurements: docs/EXPERIMENTS.md).  A copy that does
 *                       not fit HBM falls back to the records, then to the CSR scan.  All return identical results; a change rebuilds the copy.
 *   "postings_head_gemm" -1 / 1 = the head columns' part of the filter sums comes from the head pre-pass (bp_head.h: one MFMA product per
 *                       pass of query tiles, columns in >= 1/8 of the documents, up to 1024; from 1 M documents on, HBM permitting: >= 1/16, up to 1536), 0 = multiplied inside the walk (round 4)
 *   "postings_head_tiles" 0 = auto, else query tiles per pass of the head pre-pass (its scratch: 32 KB per tile and block)
 *   "postings_head_product" the pre-pass's kernel: 1 = workgroups of 2 x 2 waves share a k-step's operands through an LDS ring (LDS-DMA,
 *                       four k-steps in flight), 0 = every wave loads its own, -1 = auto (the ring from 32 tiles a pass on).  Identical results
 *   "postings_packed"   -1 / 1 = the bag-of-token chunk walk puts FOUR query slots on the two sum planes of a tile (16-bit sums, two to a dword)
 *                       for the queries whose weights allow it (integer at a small power-of-two scale, longest row x largest weight < 65 536:
 *                       checked per query on the device); 0 = two int32 slots a tile.  Identical results
 *   "postings_pace"     lock-step window of the walk's work items in blocks (-1 / 0 = free running, the default)
 *   "postings_arrange"  1 = bank-aware order inside each posting list at build time (off by default: no measured gain)
 *   "postings_lanes"    0 = auto; valued index: lanes per posting list (4 | 8, auto 8); binary index: records in flight per lane (4 | 8, auto 8)
 *   "postings_align"    1 = posting lists start on whole 128-byte lines (16 % more bytes, ~2 % less walk time); 0 / -1 = packed
 *   "postings_head"     -1 = auto (4), 0 = off, N in 2..64: columns present in >= 1/N of the documents (at most 512, the most
 *                       frequent first) leave the posting lists and are kept as dense fp16 strips [block][column][document];
 *                       a query tile scores them with multiply-adds in registers (skewed vocabularies: a Zipf corpus has
 *                       3/4 of its non-zeros there).  Valued, non-negative indexes with the filter search; results unchanged
 *   "mq_variant"        -1 = auto (from the batch's query overlap), 0 = plain, 1 = shared-column variant of the 8-query scan */
VS_API int  vs_index_set_option(vs_index* index, const char* name, int value);

/* ---- row-sharded search in one process: one vs_index per GPU (the reference searches one index on one device,
 * its only sharding precedent is the per-shard index build, examples/inference_sparse/README.md:90-107, index.py:172-175) -----
 * `shards` are consecutive row ranges of one corpus (shard i holds rows [sum of n_rows of the shards before it, ...)), each on
 * its own device; the group does not own them.  vs_shard_group_search scores the batch on every GPU concurrently, moves the
 * B * k (id, score) pairs of each shard to the first shard's device with peer copies (xGMI), and merges there: the result is
 * identical to searching the unsharded index (global ids, canonical order).  q: host pointer or device pointer on any GPU;
 * outputs: host pointers or device pointers on the first shard's device.  Blocking.  The shards run on streams of the group: with a
 * device-resident q (or device outputs) the call first synchronises that device, so that work the caller has queued on ANY of its
 * streams (the encoder writing q, a kernel still reading a recycled output buffer) is done before the shards touch the buffers.
 * Fewer than 2^32 - 1 documents in total.
 * (One process per GPU with torch.distributed / RCCL uses vs_index_search's id_offset + vs_merge_topk instead:
 * vsearch_amd/distributed.py.)                                                                                                */
typedef struct vs_shard_group vs_shard_group;
VS_API int  vs_shard_group_create(vs_index* const* shards, int32_t n_shards, vs_shard_group** out);
VS_API int  vs_shard_group_search(vs_shard_group* group, const void* q, int q_dtype, int64_t ldq, int32_t B, int32_t k,
                                  int64_t* out_ids, float* out_scores);
/* vs_shard_group_search under a document filter over the GROUP's rows (global ids): shard i reads the bitmap from bit = its first global
 * row on (vs_index_search_filtered's filter_bit0; generally not a multiple of 32), on its own device -- a host bitmap or one on another
 * GPU is copied there as q is.  filter_ld = 0: one bitmap for the batch, else >= (total rows + 31) / 32 words a query.  Padding (fewer
 * than k allowed rows) comes out of the merge as id -1, score -inf.  filter == NULL: exactly vs_shard_group_search.              */
VS_API int  vs_shard_group_search_filtered(vs_shard_group* group, const void* q, int q_dtype, int64_t ldq, int32_t B, int32_t k,
                                           const uint32_t* filter, int64_t filter_ld, int64_t* out_ids, float* out_scores);
/* vs_index_explain over the group's rows: ids are global; every shard explains the pairs of its row range on its own device, the first
 * shard's device gathers each pair from its owner.  The result equals vs_index_explain of the unsharded index bit for bit.  q may be
 * NULL (disentangle mode).  Inputs and outputs as in vs_shard_group_search (outputs on the first shard's device); blocking.        */
VS_API int  vs_shard_group_explain(vs_shard_group* group, const void* q, int q_dtype, int64_t ldq, int32_t B, const int64_t* ids,
                                   int64_t ld_ids, int32_t k, int32_t topn, int32_t* out_cols, float* out_contrib, float* out_scores,
                                   int32_t* out_matched);
/* vs_index_get_rows / vs_index_queries_from_rows over the group's rows: ids are global.  Every shard extracts the rows it owns on its own
 * device, the first shard's device stitches them (and accumulates the queries from the stitched rows: the same fl32 operations in the same
 * order).  The results equal the unsharded calls bit for bit.  Inputs: host or device pointers on any GPU; outputs: host pointers or device
 * pointers on the first shard's device.  An id outside [-1, total rows): VS_EINVAL.  Blocking.                                          */
VS_API int  vs_shard_group_get_rows(vs_shard_group* group, const int64_t* ids, int64_t n, int64_t* out_rowptr, int32_t* out_cols,
                                    float* out_vals);
VS_API int  vs_shard_group_queries_from_rows(vs_shard_group* group, const int64_t* ids, int32_t B, int32_t m, int64_t ld_ids,
                                             const float* weights, int64_t ldw, const void* q, int q_dtype, int64_t ldq, float alpha,
                                             float* out_q, int64_t ldo);
/* vs_index_delete_rows / vs_index_restore_rows over the group's rows: ids [n] are global, every shard clears / sets the bits of the rows it
 * owns.  Id -1 ignored; another id outside [0, total rows): VS_EINVAL for host ids, skipped for device ids (any GPU; they are copied to the
 * host).  vs_shard_group_restore_rows with ids == NULL restores every row.  Blocking.                                                  */
VS_API int  vs_shard_group_delete_rows(vs_shard_group* group, const int64_t* ids, int64_t n);
VS_API int  vs_shard_group_restore_rows(vs_shard_group* group, const int64_t* ids, int64_t n);
/* vs_index_term_bitmaps over the group's rows: every shard scans its rows on its own GPU; the first shard's device re-bases each shard's
 * words to the shard's first global row (generally not a multiple of 32: the seam words take bits of two shards) and ORs them into the
 * global bitmaps; document frequencies are summed.  Equal to the unsharded call bit for bit.  out_words [T, ld_words >= (total rows + 31)
 * / 32] / out_df: host pointers or device pointers on the first shard's device.  Blocking.                                              */
VS_API int  vs_shard_group_term_bitmaps(vs_shard_group* group, const int32_t* cols, const float* thr, int32_t T, uint32_t* out_words,
                                        int64_t ld_words, int64_t* out_df, int live_only);
VS_API void vs_shard_group_destroy(vs_shard_group* group);

/* SparseIndex.save (index.py:181-202) needs crow/col/values back: int64 rowptr [n_rows+1], int64
 * colidx [nnz], values [nnz] as val_dtype (VS_F32 | VS_F16).  Pass NULL colidx/values to get rowptr
 * only (to size the other two).                                                                  */
VS_API int  vs_index_export_csr(const vs_index* index, int64_t* rowptr, int64_t* colidx, void* values, int val_dtype);
/* vs_index_export_dense: the stored matrix as dtype (VS_F32 | VS_F16) into mat [n_rows, ld], ld >= n_cols, host or device pointer.  Only
 * the n_cols columns of every row are written: what the caller keeps in the ld - n_cols elements behind them stays.              */
VS_API int  vs_index_export_dense(const vs_index* index, void* mat, int dtype, int64_t ld);
VS_API void vs_index_destroy(vs_index* index);

/* Row-sharded search, merge step (new in this build): candidates gathered from
 * all shards ([B, n_cand] global ids + scores, e.g. after an RCCL all-gather) -> canonical top-k. */
/* (ids must be in [0, 2^32 - 1): the merge keys hold 32-bit ids; a candidate outside that range -- the id -1 padding of a filtered
 *  search among them -- is dropped, never aliased; fewer than k candidates left: id -1, score -inf behind them)                     */
/* (order: score descending, id ascending, scores compared as floats: -0.0 and +0.0 tie -- the id decides -- and both come back as
 *  +0.0; a real candidate that scores -inf precedes the pads; NaN scores are not ordered)                                         */
VS_API int vs_merge_topk(const int64_t* cand_ids, const float* cand_scores, int32_t B, int64_t n_cand, int32_t k,
                         int64_t* out_ids, float* out_scores, int device, void* stream);

/* ---- sparsify: src/ir/utils/sparse.py + the tail of VDREncoder.embed (vdr.py:152-169) -------- */

/* Selection rule of every top-k mask below (vs_topk_mask, vs_embed_mask, vs_embed_mask_to_csr): a row's k largest ORDER KEYS, ties at
 * the k-th key: lower column wins.  The order key of an fp32 value is its bit pattern with the sign bit set (non-negative values) or
 * with all bits inverted (negative values), compared as an unsigned integer.  That is the float order on all values that compare,
 * and beyond it: +0.0 ranks above -0.0 (for the row [-0.0, +0.0, -1.0] and k = 1 column 1 is selected, not column 0), and NaNs rank by
 * bit pattern: positive NaNs above +inf, negative NaNs below -inf.  Only vs_topk_mask's bytes can show which of two zeros was taken:
 * a kept and a dropped zero are the same bits in vs_embed_mask's output, and the CSR holds neither.
 * (tests/_sparsify_ref.py restates this rule; tests/test_gpu_sparsify_edges.py pins the kernels to it)                              */

/* build_topk_mask (sparse.py:8-14): mask[b, c] = 1 iff x[b, c] is among the k largest of row b by the rule above
 * (ties at the k-th key: lower column wins).  x: [B, V] fp32 device/host, mask: [B, V] uint8.    */
VS_API int vs_topk_mask(const float* x, int32_t B, int32_t V, int64_t ld, int32_t k, uint8_t* mask, int device, void* stream);

/* build_bow_mask (sparse.py:21-29): multi-hot of token ids over `vocab`, first `shift` columns
 * dropped, optional L2 row norm.  ids: [B, L] int64; out: [B, vocab - shift] fp32.               */
VS_API int vs_bow_mask(const int64_t* ids, int32_t B, int32_t L, int32_t vocab, int32_t shift, int norm,
                       float* out, int device, void* stream);

/* embed()'s mask stage (vdr.py:152-169), in place on emb [B, V = vocab - shift] (leading dim ld):
 *   bow != 0          -> emb = bow_mask(ids)
 *   topk == 0         -> keep only lexical dims;  topk < 0 -> keep all;  else keep top-k
 *   activate_lexical  -> mask |= bow_mask(ids)                                                   */
VS_API int vs_embed_mask(float* emb, int64_t ld, const int64_t* ids, int32_t B, int32_t L, int32_t vocab, int32_t shift,
                         int32_t topk, int activate_lexical, int bow, int device, void* stream);

/* The mask stage of VDREncoder.embed FUSED with Tensor.to_sparse_csr() (vdr.py:152-169 + retriever.py:304; SURVEY.md 8(f1) "write CSR
 * rows directly"): x [B, V] fp32 (device; NOT modified) -> the CSR of x * (topk_mask | lexical_mask): int64 rowptr [B + 1], int32 cols /
 * fp32 vals [cap] (device; cap >= B * (topk + L) always suffices; nnz = rowptr[B]).  One read of [B, V] instead of the five passes of
 * vs_embed_mask + vs_dense_to_csr.  VS_EUNSUPPORTED outside the fused kernel's range (topk <= 0, V > 32 Ki, min(V, topk + L) > 8192):
 * use those two.
 * What is stored: the KEPT elements that are not +-0.0, in column order (a kept NaN or +-inf is stored as it is).  The fused call
 * expects finite input: an unselected NaN or +-inf is dropped, where vs_embed_mask + vs_dense_to_csr (and torch) store the NaN that
 * x * 0 makes of it.  On finite input the two paths give the same CSR bit for bit.                                                  */
VS_API int vs_embed_mask_to_csr(const float* x, int64_t ld, const int64_t* ids, int32_t B, int32_t L, int32_t vocab, int32_t shift,
                                int32_t topk, int activate_lexical, int64_t* rowptr, int32_t* cols, float* vals, int64_t cap,
                                int device, void* stream);

/* Tensor.to_sparse_csr() (retriever.py:304): non-zeros of dense x [B, V] as CSR -- int64 rowptr
 * [B+1], int32 cols / fp32 vals.  Two-call protocol: (1) cols == vals == NULL: rowptr is WRITTEN
 * (sizes the outputs: nnz = rowptr[B]); (2) cols / vals with cap >= nnz: the same rowptr is READ and
 * the non-zeros are written in column order.  build_index emits CSR batch by batch this way and
 * never holds the dense [N, V] matrix (retriever.py:281).                                        */
VS_API int vs_dense_to_csr(const float* x, int32_t B, int32_t V, int64_t ld, int64_t* rowptr, int32_t* cols, float* vals,
                           int64_t cap, int device, void* stream);

/* Encoder head tail (vdr.py:73-75): elu1p then max over L of logits [B, L, V] -> out [B, V]
 * (computed as elu1p(max) -- elu1p is monotone; pad positions are pooled like the reference).    */
VS_API int vs_head_pool(const float* logits, int32_t B, int32_t L, int32_t V, float* out, int device, void* stream);

/* Encoder head, fused (vdr.py:72-75): out[b, v] = elu1p(max_l hidden[b, l, :] . W[v, :]) on the fp32 matrix cores;
 * hidden [B, L, H] (LayerNorm'ed), W [V, H] (= word_embeddings[shift:]), out [B, V]: device pointers, H % 32 == 0.
 * The reference's [B, L, V] logits tensor is never materialised.                                          */
VS_API int vs_head_project_pool(const float* hidden, const float* W, int32_t B, int32_t L, int32_t H, int32_t V, float* out,
                                int device, void* stream);

/* VDREncoder.forward with pooling = "mean" and pooling_topk = t (vdr.py:76-79):
 * out[b, c] = mean over the t largest elu1p(logits[b, l, c]), l < L.  logits [B, L, V], out [B, V]: device pointers, t <= 32. */
VS_API int vs_head_pool_mean_topk(const float* logits, int32_t B, int32_t L, int32_t V, int32_t topk, float* out, int device, void* stream);

/* ---- rerank of bag-of-token hits: Retriever.retrieve(rerank=True) (retriever.py:137-147) --------
 * The reference re-embeds the B * k hit texts with encoder_p into a dense [B * k, V] tensor, takes torch.bmm against the query
 * embeddings, and topk(k) re-sorts every row.  Here the two steps are separate entry points so that the re-embedding can be
 * streamed in batches (the dense tensor is 12 GB at B = 1024, k = 100): vs_rerank_scores fills scores[row0 .. row0 + n_rows) of
 * the flat [B * k] score array from one batch of passage embeddings (row r of the batch is hit (row0 + r) % k of query
 * (row0 + r) / k; fp32 products, fp64 sums), vs_rerank_topk then orders every query's k hits by (score descending,
 * first-stage rank ascending) and gathers their ids.  Device pointers only; k <= 2048.
 * vs_rerank_scores: a zero passage element (+0.0 or -0.0) contributes nothing whatever the query holds (inf, NaN); a call writes
 * scores[row0 .. row0 + n_rows) and nothing else (n_rows = 0: nothing).  vs_rerank_topk compares scores as floats: -0.0 and +0.0
 * tie -- the first-stage rank decides -- and both come back as +0.0; -inf (the padding of a filtered first stage, id -1) stays
 * last in its first-stage order; 64-bit ids pass through unchanged.                                                          */
VS_API int vs_rerank_scores(const void* p_emb, int p_dtype, int64_t ldp, int64_t n_rows, int64_t row0, const float* q, int64_t ldq, int32_t B,
                            int32_t k, int32_t n_cols, float* scores, int device, void* stream);
VS_API int vs_rerank_topk(const float* scores, const int64_t* hit_ids, int32_t B, int32_t k, int64_t* out_ids, float* out_scores, int device,
                          void* stream);

/* elu1p (sparse.py:6) elementwise. */
VS_API int vs_elu1p(const float* x, int64_t n, float* out, int device, void* stream);

/* ---- bag-of-token builder: Retriever._build_bot_vectors (retriever.py:208-253) --------------- */
/* tokens: flat int32 token ids of all docs (already truncated by the tokenizer), offsets [n_docs+1].
 * Per doc: first-`max_token`-unique cap (0 = off; counts every id incl. [CLS], index_utils.py:11-21),
 * multi-hot, drop ids < shift, sorted columns.  Two-call protocol: out_cols == NULL fills only
 * out_rowptr (int64 [n_docs+1]).  Host pointers only (tokenisation is host work in the reference). */
VS_API int vs_bot_build(const int32_t* tokens, const int64_t* offsets, int64_t n_docs, int32_t vocab, int32_t shift,
                        int32_t max_token, int64_t* out_rowptr, int32_t* out_cols);

/* ---- measurement hooks (bench.py) ----------------------------------------------------------- */
/* When enabled, every launch of the scoring kernels is bracketed by hipEvents on the launch
 * stream; vs_profile_read returns accumulated device time and launch count per kernel name.      */
VS_API int vs_profile_enable(int on);
VS_API int vs_profile_reset(void);
VS_API int vs_profile_read(const char* kernel, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* VSEARCH_HIP_H */
