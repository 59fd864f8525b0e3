/*
 * archi_knn.h -- C ABI of libarchi_hip.so, the MI355X (gfx950) embedding +
 * retrieval backend that drops in behind archi's embedding-provider /
 * vector-store plugin surface.
 *
 * The reference (archi-physics/archi) is pure Python and has NO FFI for this
 * path: its two engines are reached through
 *   - psycopg2 + SQL (pgvector operators)      src/data_manager/vectorstore/postgres_vectorstore.py:317-335
 *   - LangChain Embeddings.embed_documents     src/data_manager/vectorstore/manager.py:373
 * so every entry point below cites the reference call it REPLACES. The binding
 * a maintainer adds is a ctypes stub; signatures use only
 * plain pointers and sizes.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; ak_last_error() gives a
 *     thread-local message. Nothing falls back to the CPU.
 *   - the caller allocates all outputs; the library never frees caller memory;
 *     pointers are only valid for the duration of the call.
 *   - "dev" pointers are HIP device pointers on the device chosen by ak_init
 *     (one process per GPU); `stream` is a hipStream_t passed as void* (NULL =
 *     the default stream). torch users pass torch.cuda.current_stream().cuda_stream.
 *   - search entry points are re-entrant (Flask request threads call them
 *     concurrently, src/interfaces/chat_app/app.py:1554); add/remove assume a
 *     single writer (src/bin/service_data_manager.py:38,62-73) and are
 *     serialised against searches by a per-index lock.
 */
#ifndef ARCHI_KNN_H
#define ARCHI_KNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* storage dtype of the corpus matrix in HBM */
#define AK_DTYPE_F32 0
#define AK_DTYPE_BF16 1
#define AK_DTYPE_F16 2

/* distance metric == pgvector operator chosen at postgres_vectorstore.py:74-82 */
#define AK_METRIC_COSINE 0 /* "<=>" */
#define AK_METRIC_L2 1     /* "<->" */
#define AK_METRIC_IP 2     /* "<#>" (negative inner product) */

/* search mode */
#define AK_SEARCH_AUTO 0  /* MFMA candidate scan + exact re-rank + certification, exact fallback */
#define AK_SEARCH_EXACT 1 /* exact-arithmetic scan only (slow, reference arithmetic for every row) */
#define AK_SEARCH_FAST_ONLY 2 /* AUTO without the fallback: uncertified queries are reported, not re-run */

/* distinct error code of the search entry points: the row_filter was built for another layout of the index (see
 * ak_index_slots); nothing of it was read; rebuild it and retry */
#define AK_ERR_STALE_FILTER (-11)

/* ak_index_search_sharded_dev on a communicator that an earlier call left at a point the other ranks could not follow (the HIP
 * runtime or RCCL refused a step of the exchange itself): destroy the communicator and create a new one on every rank */
#define AK_ERR_COMM_BROKEN (-13)

/* encoder pooling (sentence-transformers Pooling module [upstream]) */
#define AK_POOL_MEAN 0 /* all-MiniLM-L6-v2 */
#define AK_POOL_CLS 1  /* bge-base-en */
#define AK_POOL_LAST 2 /* e5-mistral-7b-instruct: the last valid token (ak_llama_ / ak_qwen2_forward_lens only) */

typedef void *ak_index_t;
typedef void *ak_encoder_t;

/* ABI version: bumped whenever a signature in this header changes (3: filter_len / filter_epoch on the search entry points,
 * a fourth out-pointer on ak_index_slots -- round 4; ak_abi_version / ak_debug_set / ak_encoder_forward_lens -- round 5;
 * 4: the sharded exchange's payload carries a status word per rank (wire format of ak_index_search_sharded_dev / ak_merge_shards_dev
 * callers), AK_ERR_COMM_BROKEN and the ak_shard_* helpers, AkBertConfig.precision 2 -- round 6; 5: the ak_decoder_* entry points).
 * A binding checks ak_abi_version() == AK_ABI_VERSION right after loading the library (archi_amd/_lib.py does) instead of
 * passing arguments to a function whose parameter list has moved. */
#define AK_ABI_VERSION 5

/* ---- library ---------------------------------------------------------- */
const char *ak_last_error(void);
const char *ak_version(void);
int ak_abi_version(void);
/* Measurement / test hook (no reference counterpart): sets one of the A-B switches of DESIGN.md section 7 for this process, as if
 * the environment variable `name` had held `value` at start-up (NULL or "" = the default). The library reads its switches from
 * the environment ONCE; nothing on the request path calls getenv. Returns -1 for an unknown name -- and, in libarchi_hip.so, for
 * the stage-skipping switches that produce wrong results: those exist only in libarchi_hip_dbg.so. */
int ak_debug_set(const char *name, const char *value);
/* Bind this process to one GPU (one process per GPU). */
int ak_init(int device);
int ak_device_info(char *name_out, int name_cap, int *cu_count, int64_t *hbm_bytes);
int ak_sync(void *stream);

/* ---- index: replaces the document_chunks.embedding column + pgvector --- */
/* src/cli/templates/init.sql:256-274 (vector(D) column), exact branch :290-292 */
int ak_index_create(int64_t capacity, int dim, int dtype, int metric, ak_index_t *out);
int ak_index_destroy(ak_index_t h);

/* INSERT ... %s::vector   (postgres_vectorstore.py:168-180, manager.py:414-422)
 * rows: [n][dim] float32, host (is_device=0) or device (is_device=1) memory.
 * ids : [n] int64 host array (document_chunks.id), unique (-6 on a repeat inside the batch or against a live row);
 *        NULL -> consecutive from one above the largest id ever stored.
 * normalise != 0 applies x / max(||x||, 1e-12) before storing (a3).            */
int ak_index_add(ak_index_t h, const float *rows, int is_device, int64_t n, const int64_t *ids,
                 int normalise);

/* Synthetic corpus generated on device (bench / large parity tests): the
 * counter-based generator specified in oracle/knn_oracle.c (ako_gen_rows).
 * Appends rows [row0, row0+n) of stream `stream`; ids = id0 + i.              */
int ak_index_generate(ak_index_t h, uint64_t seed, uint32_t stream, uint64_t row0, int64_t n,
                      int normalise, int64_t id0);

/* DELETE FROM document_chunks WHERE ... (postgres_vectorstore.py:516-529).
 * Unknown ids are ignored; *n_removed (may be NULL) gets the number deleted. */
int ak_index_remove(ak_index_t h, const int64_t *ids, int64_t n, int64_t *n_removed);

/* SELECT COUNT(*) (postgres_vectorstore.py:570-585): live rows. */
int ak_index_count(ak_index_t h, int64_t *out);
/* Row slots in use (live + tombstones: the length of a row_filter), the current capacity and the LAYOUT EPOCH. The index
 * grows by itself (ak_index_create's capacity is only the first reservation) and reclaims tombstones when an add would
 * otherwise not fit: the reference's table has no capacity and update_vectorstore deletes and re-adds changed files
 * (manager.py:192-211). The epoch changes with every add (the slot count grows) and every reclaim (slot numbers change);
 * a delete alone leaves it (a mask that lets a deleted row pass is harmless). A row_filter is valid for exactly one
 * (slots, epoch) pair, read here in ONE call, and the search entry points take that pair with the mask: the reference
 * evaluates WHERE, distance, ORDER BY and LIMIT in one SQL statement = one snapshot (postgres_vectorstore.py:296-332),
 * and this is how a caller that builds its mask outside the library's lock gets the same guarantee. Any pointer may be NULL. */
int ak_index_slots(ak_index_t h, int64_t *out_slots, int64_t *out_capacity, uint64_t *out_epoch);
/* Reclaim every tombstone now (VACUUM; manager.py:103-153 runs VACUUM FULL at reset). *n_reclaimed may be NULL. */
int ak_index_compact(ak_index_t h, int64_t *n_reclaimed);

/* Copy stored rows back as float32 (values exactly as stored). rows: row slots. */
int ak_index_fetch(ak_index_t h, const int64_t *row_slots, int64_t n, float *out_host);
/* id -> row slot (-1 when absent). */
int ak_index_lookup(ak_index_t h, const int64_t *ids, int64_t n, int64_t *out_slots);
/* Semantic leg of the hybrid query: `1.0 - (c.embedding <op> %s::vector) AS semantic_score` for the rows a
 * BM25 match returns (postgres_vectorstore.py:435-457). Distances of ONE query [dim] float32 (host) to the
 * listed ids, in the search's exact arithmetic; out_dist[i] = NaN and out_found[i] = 0 (out_found may be
 * NULL) for ids that are absent or deleted. */
int ak_index_distances(ak_index_t h, const float *query, const int64_t *ids, int64_t n, double *out_dist,
                       uint8_t *out_found);

/* ---- lexical store + the hybrid query: replaces the pg_textsearch BM25 index and hybrid_search's SQL ------------------
 * init.sql:294-300 (CREATE INDEX ... USING bm25 on document_chunks.chunk_text) and postgres_vectorstore.py:366-491. The index
 * keeps, per row, a list of (term id, tf) entries ascending in term id and the row's length in tokens, in HBM next to the
 * embedding; the caller owns the tokeniser and the term dictionary (archi_amd/lexical.py). 8 bytes per entry (uint32 term id,
 * uint32 tf): any term id below 2^31 and any tf are held exactly. A delete is ak_index_remove's tombstone; growth, reclaim and
 * ak_index_compact move the lists with their rows (a compaction drops the dead rows' entries).
 *
 * ak_index_lex_attach: the INSERT's effect on the bm25 index (postgres_vectorstore.py:168-180 with init.sql:294-300). Lists for
 *   n LIVE rows by document_chunks.id, CSR: row i holds terms / tfs [row_offsets[i], row_offsets[i+1]), doc_len[i] tokens. An id
 *   that is unknown or dead, listed twice, a list that does not ascend, a tf < 1 or a `generation` other than the store's is an
 *   error and NOTHING is attached. Takes the index's writer lock; the layout epoch does not move. A row attached again gets the
 *   new list.
 * ak_index_lex_clear: DROP + CREATE of that index (a changed text_config / REINDEX): every list and the arena go, and the store
 *   belongs to `new_generation` -- the owner's mark, so that a scorer notices lists it did not write.
 * ak_index_lex_info: any pointer may be NULL. rows_attached: live rows with a list; entries: their entries (a dead row's stay
 *   counted until a compaction drops them); arena_bytes: bytes of the arena up to its append position. */
int ak_index_lex_attach(ak_index_t h, const int64_t *ids, int64_t n, const int64_t *row_offsets, const int32_t *terms,
                        const int32_t *tfs, const int32_t *doc_len, uint64_t generation);
int ak_index_lex_clear(ak_index_t h, uint64_t new_generation);
int ak_index_lex_info(ak_index_t h, uint64_t *generation, int64_t *rows_attached, int64_t *entries, int64_t *arena_bytes);
/* `chunk_text <@> to_bm25query(...)` for every row (postgres_vectorstore.py:421-433, the bm25_scores CTE): Okapi BM25 of one
 * query over the LIVE rows, in float64 with one rounding per operation, in the order of the scalar formulation:
 *   n = live rows, avg = sum of their lengths / n, df_t = live rows holding term t, idf_t = log(1.0 + (n - df_t + 0.5) / (df_t + 0.5))
 *   (the host C library's log); terms with df_t = 0 drop out; per row, terms in the query's first-occurrence order from acc = 0.0:
 *   acc = acc + ((idf * tf) * (k1 + 1.0)) / (tf + k1 * ((1.0 - b) + (b * len) / avg))   [avg == 0: tf + k1 * (1.0 - b)];  bm = sign * acc
 * terms [T]: the query's term ids (repeats are dropped; any T). out_bm / out_hit: [slots] float64 / bytes on the HOST indexed by
 * row slot (ak_index_slots, ak_index_lookup): out_hit = 1 and out_bm = the score for live rows holding a query term, 0 elsewhere.
 * out_info: NULL or int64[4] = {n, sum of lengths, matching rows, terms with df > 0}. */
int ak_index_lex_scores(ak_index_t h, const int32_t *terms, int T, double k1, double b, double sign, double *out_bm,
                        uint8_t *out_hit, int64_t *out_info);
/* The hybrid query (postgres_vectorstore.py:420-457) as ONE call under the index's reader lock:
 *   combined = (1.0 - distance) * w_s + COALESCE(bm25, 0) * w_b ... ORDER BY combined DESC LIMIT k
 * evaluated as two legs whose union holds the answer (w_s >= 0): the HIT leg -- rows holding a query term and the rows listed in
 * also_ids [n_also] (ids whose distance can be NaN; unknown ids are ignored), restricted to live rows that pass row_filter: their
 * exact distances in the search's arithmetic, BM25 as ak_index_lex_scores (+0.0 for an also-row without a match), the best k by
 * (NaN first, combined descending, id ascending) -- and the SCAN leg: ak_index_search (AUTO) of the other rows that pass row_filter.
 *   query      : [dim] float32, host
 *   row_filter : NULL or [filter_len] bytes on the host with (filter_len, filter_epoch) as for ak_index_search: AK_ERR_STALE_FILTER
 *                when the index has moved on, nothing read
 *   out_hit_ids / out_hit_combined [k], *n_hit; out_scan_ids / out_scan_dist [k] (float8 distance), *n_scan: the two lists; the
 *                caller merges the <= 2 k entries (the scan rows' combined = (1.0 - d) * w_s + 0 * w_b)
 *   out_info   : NULL or int64[12] = {n, sum of lengths, matching rows that pass the filter, rows of the hit leg, terms with
 *                df > 0, arena entries streamed per pass, then -- when ak_index_profile is on -- nanoseconds of the statistics
 *                pass, the score pass (with the host's idf step), the hit leg and the scan leg, 0, 0}
 * Workspace comes from the index (grown on first use); evaluations on one index are serialised, and concurrent calls are
 * coalesced into batch evaluations (see ak_index_hybrid_search_batch). */
int ak_index_hybrid_search(ak_index_t h, const float *query, const int32_t *terms, int T, double k1, double b, double sign,
                           double w_s, double w_b, const int64_t *also_ids, int64_t n_also, const uint8_t *row_filter,
                           int64_t filter_len, uint64_t filter_epoch, int k, int64_t *out_hit_ids, double *out_hit_combined,
                           int *n_hit, int64_t *out_scan_ids, double *out_scan_dist, int *n_scan, int64_t *out_info);
/* ak_index_hybrid_search for a BATCH of queries: one pass over the lists for the statistics, one host step (idf), one score pass and
 * ONE scan for up to 32 queries. The scan takes one mask for all its queries, so the batch is evaluated the way also_ids rows are:
 *   U = the live rows that pass row_filter and hold a term of ANY query of the batch, plus the also rows;
 *   HIT leg, per query q: the exact distance of EVERY row of U, bm_q = the query's BM25 exactly as ak_index_lex_scores computes it for
 *   rows holding a term of q and +0.0 for the rest of U, combined = (1.0 - d) * w_s + bm_q * w_b, the best k by (NaN first, combined
 *   descending, id ascending); SCAN leg: one ak_index_search (AUTO) of all queries over the rows that pass row_filter and are not in U.
 * A row of U without a term of q scores (1.0 - d) * w_s + 0.0 * w_b, the expression the caller evaluates for a scan row, so the
 * MERGED top k of query q -- ids and float64 score bits -- equals that of ak_index_hybrid_search for q alone; the two lists
 * themselves differ (rows move from the scan list to the hit list). Known cost: the hit leg computes nq * |U| exact distances where
 * nq single calls compute the sum of their own hit counts; with frequent words U approaches the whole collection.
 *   queries      : [nq][dim] float32, host; 1 <= nq
 *   term_offsets : [nq + 1], terms: query q's term ids are terms[term_offsets[q], term_offsets[q + 1]) (CSR). A query with no terms,
 *                  with only unknown terms, with repeated terms, and identical queries are all fine.
 *   k1 / b / sign / w_s / w_b / k, also_ids [n_also], row_filter with (filter_len, filter_epoch): ONE of each for the batch, as for
 *                  the single call (AK_ERR_STALE_FILTER when the index has moved on, nothing read)
 *   out_hit_ids / out_hit_combined [nq][k], n_hit [nq]; out_scan_ids / out_scan_dist [nq][k], n_scan [nq]
 *   out_info     : NULL or int64[16] = {n, sum of lengths, |U| without the also rows, rows of the hit leg, union terms with df > 0,
 *                  arena entries streamed per statistics pass, then -- when ak_index_profile is on -- nanoseconds of the statistics
 *                  pass, the score pass (with the host's idf step), the hit leg and the scan leg; [10] statistics passes run,
 *                  [11] score passes run, [12] scans run, [13] sub-batches, [14] the sum over queries of their own matching rows
 *                  (what nq single calls would re-rank), [15] (query, row) pairs the hit leg evaluated}; [2]-[4] and [6]-[15] are
 *                  summed over the sub-batches
 * Limits: 32 queries (one bit each in a uint32 per row) and 2048 distinct terms (the kernels' LDS table) per sub-batch; more of
 * either runs as consecutive sub-batches INSIDE the call, under one reader lock = one state of the index. A single query with more
 * than 2048 distinct terms goes through the single-query passes. The [queries][rows of U] arrays of the hit leg (48 bytes per pair)
 * are allocated after the host has read |U| and hold at most AK_LEX_BATCH_PAIRS pairs (ak_debug_set; default 2^24, about 0.8 GB):
 * beyond it the hit leg runs in query groups, each with its own score pass over U's lists; the statistics pass over the whole arena
 * and the scan stay shared. AK_LEX_BATCH_TERMS lowers the term limit (tests). One host synchronisation between the statistics and
 * the score pass per sub-batch, as in the single call.
 *
 * Concurrent ak_index_hybrid_search calls on one index are coalesced (AK_COALESCE=0 turns it off): a call on an idle index runs at
 * once; calls that arrive while one is running queue up and are then served together, per group of equal (k, k1, b, sign, w_s,
 * w_b, row_filter pointer, filter_len, filter_epoch), by ONE batch evaluation with their also lists united. Each caller gets its own
 * rows; its out_info [0..9] then describes the SHARED evaluation (|U| of the group, its times) and out_info[10] is the number of
 * calls it served (0: the call ran alone). An error of the shared evaluation reaches every caller of the group with its message. */
int ak_index_hybrid_search_batch(ak_index_t h, const float *queries, int nq, const int64_t *term_offsets, const int32_t *terms,
                                 double k1, double b, double sign, double w_s, double w_b, const int64_t *also_ids, int64_t n_also,
                                 const uint8_t *row_filter, int64_t filter_len, uint64_t filter_epoch, int k, int64_t *out_hit_ids,
                                 double *out_hit_combined, int *n_hit, int64_t *out_scan_ids, double *out_scan_dist, int *n_scan,
                                 int64_t *out_info);

/* SELECT ... embedding <op> %s::vector AS distance ... WHERE ... ORDER BY distance
 * ASC LIMIT k   (postgres_vectorstore.py:317-332).
 *   queries   : [nq][dim] float32, host memory
 *   row_filter: NULL, or [filter_len] bytes on the HOST indexed by row slot (see
 *               ak_index_lookup): rows with 0 fail the WHERE clause (:296-310).
 *               filter_len / filter_epoch: the (slots, epoch) pair ak_index_slots returned
 *               when the mask was built; if the index has moved on since (a concurrent
 *               add or reclaim), the call returns AK_ERR_STALE_FILTER without reading the
 *               mask. Both are ignored when row_filter is NULL.
 *   out_ids   : [nq][k] int64; out_dist: [nq][k] float64 (pgvector float8
 *               distance; the caller computes score = 1 - distance for cosine,
 *               :361). Unused tail slots: id -1, distance NaN.
 *   out_counts: [nq] rows returned per query (NULL allowed)
 *   out_stats : NULL or int64[4] = {queries certified by the fast path (either scan),
 *               queries re-run exactly, candidates re-ranked, queries certified
 *               only by the second, widest-candidate-list scan}
 * Re-entrant: the reference runs one such SELECT per request thread
 * (src/interfaces/chat_app/app.py:1554 -> postgres_vectorstore.py:227-248). Calls
 * with nq <= 16 that arrive while another call's search is in flight are COALESCED:
 * they wait for it, then one of them searches for all that carry the same k, mode
 * and row_filter POINTER (+ length and epoch) in one launch (a scan costs the same for 1 query as for 64);
 * each caller gets its own rows back (out_stats then describes the shared launch).
 * Nobody waits when the index is idle. AK_COALESCE=0 turns it off.            */
int ak_index_search(ak_index_t h, const float *queries, int nq, int k, int mode,
                    const uint8_t *row_filter, int64_t filter_len, uint64_t filter_epoch,
                    int64_t *out_ids, double *out_dist, int *out_counts, int64_t *out_stats);

/* Max-marginal-relevance search. NO COUNTERPART in the reference's store (PostgresVectorStore has no MMR read): the method follows
 * LangChain's VectorStore contract, max_marginal_relevance_search(query, k, fetch_k, lambda_mult) [upstream, not in tree], which
 * as_retriever(search_type="mmr") calls. Cosine indexes only (LangChain's helper is cosine-only too); an l2 / ip index is refused
 * by name before any GPU work. Requires 1 <= k <= fetch_k <= 128 and 0 <= lambda_mult <= 1.
 *   1. Candidates: the first fetch_k rows of ak_index_search for this query, mask and mode, in its order (distance ascending, ties
 *      by id, NaN last); m <= fetch_k of them. Rank r = position in that list, dq[r] its float64 distance, sq[r] = 1.0 - dq[r].
 *   2. Pair distances, ranks i < j: d(i,j) = the cosine distance of the two STORED rows in the search's exact arithmetic (float32
 *      chain in element order, one rounding per multiply and per add, the index's stored row norms, float64 finish);
 *      s(i,j) = s(j,i) = 1.0 - d(i,j).
 *   3. Greedy pick, float64, no contraction: the first pick is rank 0. red[r] starts at -inf; after a pick p every unpicked r gets
 *      red[r] = s(r,p) if s(r,p) > red[r] (a NaN never updates). The next pick is the unpicked r with the largest
 *      score[r] = lambda_mult * sq[r] - (1.0 - lambda_mult) * red[r], (1.0 - lambda_mult) computed once; strict > scanning ranks
 *      upward (the lowest rank wins a tie); a NaN score never wins, and when every remaining score is NaN the lowest remaining
 *      rank is picked. min(k, m) picks.
 *   out_ids / out_dist [nq][k]: the picks in pick order with dq of each pick; out_rank [nq][k] (NULL allowed): each pick's rank;
 *   out_counts [nq] (NULL allowed) = min(k, m). Unused tail: id -1, distance NaN, rank -1.
 *   out_stats: NULL or int64[4], that of the candidate search. row_filter / filter_len / filter_epoch: as ak_index_search,
 *   AK_ERR_STALE_FILTER included.
 * With lambda_mult = 1 the result is the first k rows of ak_index_search. The candidate search and the selection run under ONE hold
 * of the index's reader lock. Re-entrant like ak_index_search; not coalesced. A refused call launches nothing and leaves the
 * outputs untouched. */
int ak_index_mmr_search(ak_index_t h, const float *queries, int nq, int k, int fetch_k, double lambda_mult, int mode,
                        const uint8_t *row_filter, int64_t filter_len, uint64_t filter_epoch,
                        int64_t *out_ids, double *out_dist, int *out_rank, int *out_counts, int64_t *out_stats);

/* Grouped search: the k nearest GROUPS of rows (documents) and the best group_size rows (chunks) of each. NO COUNTERPART in the
 * reference's store: its callers collapse the retriever's k chunks by document on the host (ChatWrapper.get_top_sources,
 * src/interfaces/chat_app/app.py:442-484 there); this is the "group by" / "collapse" read of other vector stores.
 *   row_group [filter_len] int32 on the host, REQUIRED, indexed by row slot: a key >= 0 names the row's group, a negative key means
 *   "this row is a group by itself". It is valid for exactly the (filter_len, filter_epoch) pair ak_index_slots returned;
 *   row_filter (NULL allowed) is under the same contract and has the same length. A stale pair returns AK_ERR_STALE_FILTER with
 *   nothing read and the outputs untouched. Every metric. mode: AK_SEARCH_AUTO or AK_SEARCH_EXACT (FAST_ONLY is refused by name).
 *   1 <= k <= 32 and 1 <= group_size <= 8, refused by name outside them before any GPU work; any nq >= 0.
 * Definition:
 *   1. Let L(q) be the complete result list of ak_index_search for query q with this mask and k = every live row that passes the
 *      mask: distance ascending, ties by id ascending, NaN distances last; distances are the float8 values of the exact arithmetic.
 *   2. Walk L(q) from the front.
 *   3. A group is ranked by the position of its first row.
 *   4. A group's members are its rows in list order.
 * Result: the first min(k, number of groups) groups. For each: its first min(group_size, members) rows in out_ids / out_dist
 * [nq][k][group_size], its key as given (so negative for a single-row group) in out_group [nq][k], the number of members returned
 * in out_sizes [nq][k]; out_counts [nq] (NULL allowed) = groups returned. Padding: id -1, distance NaN, out_group -1, out_sizes 0.
 * It follows that (a) every key negative and group_size = 1 gives the first k rows of ak_index_search, and (b) every row in one
 * group gives one group whose members are the first group_size rows of ak_index_search, both bit for bit.
 *   out_stats: NULL or int64[8] = {certified, exact re-runs, re-ranked, certified by the second scan (these four: the FIRST
 *   round's search, as ak_index_search reports them), search rounds run summed over queries, queries that needed more than one
 *   round, rows matched by the member pass, searches launched}.
 * How: a certified search returns exactly the first k' rows of L(q), so the distinct groups among them, in order of first
 * appearance, are the first groups of the ranking. Round 1 fetches k' = clamp(4 k, 16, 128) rows for all queries (AK_GROUP_FETCH,
 * ak_debug_set, 1 .. 128, overrides k'); a query that then holds fewer than k groups although its round came back full runs
 * further rounds alone, each with the groups found so far masked out, until it has k groups or a round comes back short. With
 * group_size > 1 one pass over the row slots per query lists the members of the winning groups, whose distances are computed in
 * the search's exact arithmetic; nothing is truncated, whatever a group's size. All rounds of one call run under ONE hold of the
 * index's reader lock. Re-entrant; not coalesced. A refused or failed call leaves the outputs untouched. */
int ak_index_group_search(ak_index_t h, const float *queries, int nq, int k, int group_size, int mode,
                          const int32_t *row_group, const uint8_t *row_filter, int64_t filter_len, uint64_t filter_epoch,
                          int64_t *out_ids, double *out_dist, int32_t *out_group, int *out_sizes, int *out_counts,
                          int64_t *out_stats);

/* Same query, everything resident in HBM (bench path and the row-sharded multi-GPU path: inputs already on the device
 * when the timed region starts; `stream` orders the work).
 *   mode AK_SEARCH_FAST_ONLY: asynchronous, nothing synchronises with the host. out_cert_dev [nq] int32 receives 1 for
 *        every query whose top-k is PROVEN identical to the exact path; the rows of a query with 0 may differ and must be
 *        re-run by the caller (archi_amd/sharded.py reduces the flags over the ranks and re-runs them with AUTO).
 *   mode AK_SEARCH_AUTO: the same, then the flags are read back (one host synchronisation) and open queries are re-run
 *        on the device -- second scan with the widest candidate lists, then the exact path -- so that on return every row
 *        is the reference's ORDER BY distance LIMIT k and every flag is 1.
 *   mode AK_SEARCH_EXACT: reference arithmetic for every row (asynchronous).
 *   Shapes the MFMA scan does not take (fewer than 4096 rows, an empty shard, dim % 64 != 0, k > 128) run the exact path
 *   in every mode and report 1.
 *   row_filter_dev: NULL or [filter_len] bytes on the DEVICE (the WHERE clause, as ak_index_search's row_filter, with the
 *        same (filter_len, filter_epoch) contract and AK_ERR_STALE_FILTER).
 *   out_cert_dev may be NULL (AUTO / EXACT).
 * Workspace comes from the index (grown on first use). Calls on one index are serialised; a call on another stream
 * waits on the device for the previous call's kernels, and ak_index_add / remove / compact wait for them on the host. */
int ak_index_search_dev(ak_index_t h, const float *queries_dev, int nq, int k, int mode,
                        const uint8_t *row_filter_dev, int64_t filter_len, uint64_t filter_epoch,
                        int64_t *out_ids_dev, double *out_dist_dev, int *out_cert_dev, void *stream);

/* How a search of this shape would run: out8 = {fast path usable, tile config id, k', corpus
 * slices, query groups, seed-pass slices, seed-pass rows, queries per workgroup}. The main scan
 * launch covers rows [seed_rows, count).                                                      */
int ak_index_scan_plan(ak_index_t h, int nq, int k, int64_t *out8);
/* int8 shadow of a 16-bit corpus (AK_SCAN_I8): out4 = {rows covered, full builds so far, searches that ran the int8 plan,
 * largest relative rounding error of a row in units of 1e-9} */
int ak_index_i8_info(ak_index_t h, int64_t *out4);

/* Developer aid: per-wave phase cycle counters of the last search's two scan launches (seed pass at
 * [0,65536), main pass at [65536,131072), 8 int64 per wave: k-loop, filter, sync, compaction, final,
 * slow-path entries, compactions, tiles). Filled only when the search ran with AK_SCAN_DBG=1.    */
int ak_index_debug_read(ak_index_t h, int64_t *out, int n);

/* Per-launch timing of the dominant kernel (the MFMA candidate scan): when
 * enabled every search records a HIP event pair around that kernel on the
 * launch stream. Read (after synchronising the stream) returns the durations in
 * ms in launch order and clears the log. Used by bench.py's roofline object.  */
int ak_index_profile(ak_index_t h, int enable);
int ak_index_profile_read(ak_index_t h, float *out_ms, int cap, int *n_out);

/* Cross-shard k-way merge: parts [g][nq][k] on device (after the
 * RCCL all-gather) -> [nq][k], comparator (distance asc, NaN last, id asc).  */
int ak_merge_topk_dev(int g, int nq, int k, const int64_t *part_ids_dev, const double *part_dist_dev,
                      int64_t *out_ids_dev, double *out_dist_dev, void *stream);

/* The row-sharded search's exchange step in one call (archi_amd/sharded.py). payload_dev: the all-gathered buffer, per
 * rank [ids nq*k int64 | float8 distance bits nq*k int64 | certificate flags nq int32, padded to a whole int64] -- what
 * ak_index_search_dev writes when its three outputs point into ONE buffer, so the local search fills the payload in
 * place --, ranks `stride` int64 elements apart (stride >= 2*nq*k + (nq+1)/2). Merges like
 * ak_merge_topk_dev and reduces the flags: out_open_dev [nq + 1] int32 = 1 for every query SOME shard could not certify
 * (the caller re-runs those on every shard with AK_SEARCH_AUTO), their count at [nq].                                */
int ak_merge_shards_dev(int g, int nq, int k, const int64_t *payload_dev, int64_t stride, int64_t *out_ids_dev,
                        double *out_dist_dev, int *out_open_dev, void *stream);

/* ---- the row-sharded search with its exchange step inside the library -------------------------------
 * One process per GPU, every rank holds one row shard in an ak_index_t. The reference has no counterpart (one Postgres
 * backend scans the whole table, postgres_vectorstore.py:317-332); these calls are what a maintainer binds -- with ctypes
 * alone, no torch.distributed -- to run that statement over the 8 GPUs of a node:
 *   rank 0:      ak_comm_unique_id(id)           128 bytes, handed to the other ranks by any channel (file, socket, MPI ...)
 *   every rank:  ak_comm_create(id, rank, world, &comm)     ncclCommInitRank on ak_init's device (RCCL over xGMI)
 *   every rank:  ak_index_search_sharded_dev(shard, comm, ...)   the same queries on every rank, the same result on every rank
 * RCCL is looked up when the first of these is called (the librccl.so already mapped into the process, else ROCm's
 * librccl.so.1); they return -12 where it is missing, the rest of the library does not need it. */
typedef void *ak_comm_t;
#define AK_COMM_ID_BYTES 128
int ak_comm_unique_id(void *out_id128);
int ak_comm_create(const void *unique_id128, int rank, int world, ak_comm_t *out);
int ak_comm_destroy(ak_comm_t c);
/* ak_index_search_dev(FAST_ONLY) on the local shard -> ONE ncclAllGather of [ids | float8 distance bits | certificate flags]
 * (nq * (16 k + 4) bytes per rank) -> ak_merge_shards_dev, all on `stream`; the flags are then read (one host synchronisation)
 * and the queries ANY shard could not certify are re-run on EVERY shard with AK_SEARCH_AUTO, exchanged and merged again --
 * every rank reads the same gathered flags and takes the same branch. On return out_ids_dev / out_dist_dev [nq][k] hold the
 * exact ORDER BY distance LIMIT k over all shards, identical on every rank; *out_rerun (may be NULL) = queries re-run.
 * queries_dev must hold the same rows on every rank; row_filter_dev / filter_len / filter_epoch describe the LOCAL shard (as
 * for ak_index_search_dev). Calls on one communicator are serialised; every rank must issue them in the same order. */
int ak_index_search_sharded_dev(ak_index_t shard, ak_comm_t comm, const float *queries_dev, int nq, int k,
                                const uint8_t *row_filter_dev, int64_t filter_len, uint64_t filter_epoch,
                                int64_t *out_ids_dev, double *out_dist_dev, int64_t *out_rerun, void *stream);

/* Failure contract of ak_index_search_sharded_dev ("one statement succeeds or fails as a whole", postgres_vectorstore.py:317-332):
 *   - a rank whose LOCAL scan fails (stale row_filter, workspace ...) still enters the all-gather, with empty rows and its code in
 *     the payload's status word: every rank returns that code after the collective;
 *   - a rank whose first MERGE fails reads the gathered flag / status words itself and joins the second all-gather whenever the
 *     others enter it (empty rows + its code: every rank returns it); if no query is open only that rank returns the error;
 *   - a failure of the exchange itself -- its buffers, a HIP copy / memset / launch / synchronise on `stream`, an RCCL error --
 *     is FATAL TO THE COMMUNICATOR: the rank returns, and every later call on that communicator returns AK_ERR_COMM_BROKEN at
 *     once instead of pairing with the wrong collective; the other ranks' collective ends by RCCL's own abort / timeout, as after
 *     the loss of a process. Destroy and re-create the communicator on every rank.
 * AK_RCCL_PATH in the environment at load names the communicator library (default: the librccl.so already mapped, else ROCm's).
 *
 * The exchange's small device steps, exported for a caller that drives the same exchange over another transport
 * (archi_amd/sharded.py over torch.distributed): no torch kernel is then needed between the local search and the result.
 *   ak_shard_payload_begin_dev   zero the flag padding and the status word of a payload [2 nq k + (nq+1)/2 + 1] int64 before the
 *                                local ak_index_search_dev writes ids / float8 bits / flags into it
 *   ak_shard_fail_payload_dev    the payload of a rank whose local search failed: no rows (id -1, NaN), every flag "certified"
 *                                (it asks for no re-run), `status` in the last word
 *   ak_shard_status_dev          out_status_dev[r] = (int) last word of rank r's payload, r < g <= 1024, payloads `stride` apart
 *   ak_shard_gather_rows_dev     out[j] = rows[idx[j]] (the open queries of a batch, [m][dim] float32)
 *   ak_shard_scatter_topk_dev    out_ids[idx[j]] = sub_ids[j], out_dist[idx[j]] = sub_dist[j] (rows of k): the re-run's rows back */
int ak_shard_payload_begin_dev(int64_t *payload_dev, int nq, int k, void *stream);
int ak_shard_fail_payload_dev(int64_t *payload_dev, int nq, int k, int status, void *stream);
int ak_shard_status_dev(int g, const int64_t *gathered_dev, int64_t stride, int *out_status_dev, void *stream);
int ak_shard_gather_rows_dev(const float *rows_dev, const int *idx_dev, int m, int dim, float *out_dev, void *stream);
int ak_shard_scatter_topk_dev(const int *idx_dev, int m, int k, const int64_t *sub_ids_dev, const double *sub_dist_dev,
                              int64_t *out_ids_dev, double *out_dist_dev, void *stream);

/* ---- L2 normalise (a3) ------------------------------------------------- */
/* encode_kwargs.normalize_embeddings (src/cli/templates/base-config.yaml:149-150) */
int ak_l2_normalize_dev(float *rows_dev, int64_t n, int dim, void *stream);

/* ---- encoder: replaces Embeddings.embed_documents / embed_query -------- */
/* manager.py:373, postgres_vectorstore.py:143,245,390 */
typedef struct AkBertConfig {
    int vocab_size;     /* 30522 */
    int hidden;         /* 384 (MiniLM-L6) / 768 (bge-base) */
    int layers;         /* 6 / 12 */
    int heads;          /* 12 */
    int intermediate;   /* 1536 / 3072 */
    int max_position;   /* 512 */
    int type_vocab;     /* 2 */
    float ln_eps;       /* 1e-12 */
    int residual_bf16;  /* 0: fp32 residual stream between layers (reference-like); 1: the residual stream is kept
                         * in bf16 only (hidden 384 path): 60% less epilogue traffic, +~1e-6 cosine deviation from
                         * the fp32 reference on top of the bf16 GEMM inputs */
    int precision;      /* 0: bf16 MFMA GEMMs (the measured path). 1: fp32 PARITY MODE -- every matrix in `weights_dev` is then
                         * float32 (same order and shapes) and all arithmetic is float32: GEMMs and attention on
                         * v_mfma_f32_32x32x2_f32 (csrc/encoder_f32.hip; 0.70 / 0.77 of the 157 TFLOP/s float32 matrix roof),
                         * exact erf GELU, fp32 LayerNorm / softmax: the reference's CPU embedder (torch fp32, manager.py:373)
                         * to ~1e-6, at ~1/9 of the bf16 rate. 2: SPLIT-bf16 PARITY MODE ("bf16x3") -- float32 weights as for 1;
                         * every GEMM operand is split x = hi + lo (two bf16 values, lo = bf16(x - hi)) and every product runs
                         * as hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 with one fp32 accumulator (~2^-16 per
                         * product), everything between the GEMMs in fp32 as for 1: fp32-grade embeddings at ~1/3 of the bf16
                         * rate. Batches of >= 16 384 tokens (hidden >= 512; 20 480 below) run on the bf16 path's GEMM tiles (csrc/gemm.hip MODE 5 / 6: the
                         * activations travel as bf16 [hi | lo] rows, the K-loop walks 3 K; GELU by a cubic table of the normal
                         * CDF, max error 5e-7), smaller ones on csrc/encoder_f32.hip's k3_gemm; both held to 1e-5 by the tests. */
} AkBertConfig;

/* Weight order (all device pointers, bf16 matrices (float32 when cfg->precision == 1) row-major [out][in] exactly
 * as torch.nn.Linear.weight, fp32 vectors):
 *   0 word_emb [vocab][H] bf16, 1 pos_emb [max_pos][H] bf16, 2 type_emb [type][H] bf16,
 *   3 emb_ln_g [H] f32, 4 emb_ln_b [H] f32,
 *   per layer l (base 5 + 16*l):
 *     +0 wq +1 bq +2 wk +3 bk +4 wv +5 bv +6 wo +7 bo +8 ln1_g +9 ln1_b
 *     +10 w1 [I][H] +11 b1 [I] +12 w2 [H][I] +13 b2 [H] +14 ln2_g +15 ln2_b      */
int ak_encoder_create(const AkBertConfig *cfg, const void *const *weights_dev, int n_weights,
                      ak_encoder_t *out);
int ak_encoder_destroy(ak_encoder_t h);
/* ids/mask: [B][S] int32 on device; out: [B][H] float32 on device. Asynchronous on `stream`, with one exception: under
 * AK_QUERY_FUSED=1 (opt-in, hidden 384, B * S <= 64) the forward pass runs as ONE launch confined to one XCD (csrc/query_forward.hip)
 * whose every wait is bounded; the call then synchronises `stream` to read its failure word and, had a wait given up, re-runs the
 * pass through the ordinary launches -- same rows bit for bit either way. Measured slower than the ordinary launches on MI355X
 * (DESIGN.md section 4), hence opt-in. */
int ak_encoder_forward(ak_encoder_t h, const int32_t *ids_dev, const int32_t *mask_dev, int B, int S,
                       int pooling, int normalise, float *out_dev, void *stream);
/* The same forward pass for RIGHT-PADDED rows given by their lengths -- what a tokenizer emits and what the provider's
 * length-sorted tiles hold (replaces the per-tile mask assembly the Python side did with torch kernels; round-4 review):
 *   ids_dev   [B] rows of S token ids, `ld_ids` int32 apart (>= S); whatever lies past a row's length is ignored
 *   lens_dev  one int32 per row, `lens_stride` int32 apart (the tiles carry it as column S of the id rows: ld_ids = S + 1,
 *             lens_dev = ids_dev + S, lens_stride = S + 1); clamped to [0, S]; a row of length 0 embeds to zeros
 *   out_dev   [B][H] float32: the caller passes the address of the tile's first row inside ONE result buffer.
 * The library lays the 0 / 1 mask out itself (one small launch) and runs ak_encoder_forward's kernels on it: results are
 * bit-identical to ak_encoder_forward on the explicit mask. S a multiple of 32, <= 512. */
int ak_encoder_forward_lens(ak_encoder_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                            int pooling, int normalise, float *out_dev, void *stream);

/* Relative-position bias (MPNet: sentence-transformers/all-mpnet-base-v2 and its family, the default model of
 * HuggingFaceEmbeddings behind manager.py:373): an additive per-head term bias[h][key - query] in every attention layer, added after
 * the 1 / sqrt(head size) scaling and before the softmax, as HF MPNet adds compute_position_bias's output.
 *   bias_dev  [heads][2 n_rel - 1] float32 on device, natural-log domain: entry [h][d + n_rel - 1] is the bias of distance
 *             d = key - query, |d| < n_rel (one value per distance: any bucketing scheme is resolved by the caller)
 *   heads     must equal cfg->heads; 1 <= n_rel <= 1023
 * The library copies the table at the call (bias_dev may be freed afterwards). Call it once, before the first forward pass; a
 * forward pass with S > n_rel then fails. Served in every precision; the single-launch query forward (AK_QUERY_FUSED) is not
 * taken by such an encoder. The rest of MPNet needs no entry point of its own: its RoBERTa-style positions are pos_emb offset by
 * padding_idx + 1 rows with max_position = max_position_embeddings - padding_idx - 1, and its missing token types one zero
 * type_emb row with type_vocab = 1. */
int ak_encoder_set_rel_bias(ak_encoder_t h, const float *bias_dev, int heads, int n_rel);

/* Positions from the ids (RoBERTa / XLM-R: BAAI/bge-m3, intfloat/multilingual-e5-*, paraphrase-multilingual-mpnet-base-v2, the
 * multilingual embedders an archi deployment names behind manager.py:373), as HF's create_position_ids_from_input_ids computes them:
 * a token inside the row (mask != 0, or before the row's length) whose id is not padding_idx sits at position padding_idx + the number
 * of such tokens up to and including it; every other token at padding_idx. A text holding a literal <pad> thus shifts the positions of
 * the tokens behind it, as in HF. (HF looks at the ids alone; here a token outside the mask never counts, so that ids past a row's
 * length are ignored. The two agree on right-padded rows; they differ only for a mask with zeros on non-pad ids before real tokens.) pos_emb is then the FULL position table (max_position = max_position_embeddings rows, the
 * padding_idx row included) and type_emb the model's one token-type row (type_vocab = 1).
 *   padding_idx  >= 0; the model's pad id
 *   max_seq      the longest row (S) the encoder then accepts: 1 <= max_seq <= 8192 and padding_idx + 1 + max_seq <= max_position;
 *                above 512 only in precision bf16 at head size 64 (hidden != 384): tiles with S > 512 run the long-row flash attention
 *                (csrc/attn_long.hip), tiles with S <= 512 the kernels they ran before
 * Call it once, after ak_encoder_create and before the first forward pass; it applies to ak_encoder_forward and
 * ak_encoder_forward_lens in every precision. Not combined with ak_encoder_set_rel_bias (either call fails once the other was made);
 * the single-launch query forward (AK_QUERY_FUSED) is not taken by such an encoder. An encoder on which it is not called keeps
 * position = token index. */
int ak_encoder_set_positions_from_ids(ak_encoder_t h, int padding_idx, int max_seq);

/* The 8192-entry bf16 table the fused hidden-384 layer kernel and the wide FFN-up tile read their GELU from (csrc/gelu_table.h):
 * entry i = bf16(gelu(v)), v = the MIDPOINT of the IEEE half bit patterns [8 i, 8 i + 8) (sign, 5 exponent bits, 7 mantissa bits;
 * the lookup truncates, so the midpoint halves its error), exact erf GELU
 * (the activation of the reference's default embedder, all-MiniLM-L6-v2, inside Embeddings.embed_documents, manager.py:373).
 * Host only -- no GPU work; exported so that the CPU suite can hold the table to the exact function. */
int ak_encoder_gelu_table(uint16_t *out8192);

/* ---- decoder: Qwen3-Embedding (0.6B / 4B / 8B), the instruction-aware embedders of the reference's retrievers -------- */
/* retrievers/utils.py:7-11, semantic_retriever.py:31-38. The forward pass of HF Qwen3Model (RMSNorm, per-head q / k RMSNorm, rotate_half
 * RoPE, grouped-query causal attention at head dim 128, SwiGLU MLP), then the final norm of each row's LAST valid token and L2
 * normalisation (sentence-transformers' lasttoken Pooling + Normalize). bf16 MFMA GEMMs, float32 residual stream.
 * One of three ABIs over one implementation, the head-128 decoder stack (csrc/decoder128.hip; ak_llama_* and ak_qwen2_* below are the
 * others): Qwen3 is the Mistral / Llama layer plus the per-head q / k norm, causal without a window, last-token pooling only. */
typedef void *ak_decoder_t;
typedef struct AkDecoderConfig {
    int vocab_size;     /* 151669 */
    int hidden;         /* 1024 / 2560 / 4096; a multiple of 128 */
    int layers;         /* 28 / 36 / 36 */
    int q_heads;        /* 16 / 32 / 32 */
    int kv_heads;       /* 8; q_heads % kv_heads == 0, at most 4 query heads per kv head */
    int head_dim;       /* 128 (the only head size implemented) */
    int intermediate;   /* 3072 / 9728 / 12288; a multiple of 64 */
    int max_position;   /* 32768 (sequences are limited to min(max_position, 8192) tokens) */
    float rms_eps;      /* 1e-6 */
    float rope_theta;   /* 1e6 (default RoPE only: no rope scaling) */
} AkDecoderConfig;
/* Weight order (device pointers; matrices bf16 row-major [out][in] exactly as torch.nn.Linear.weight, vectors float32):
 *   0 embed_tokens [vocab][H] bf16, 1 final norm [H],
 *   per layer l (base 2 + 11 * l):
 *     +0 wq [q_heads 128][H] +1 wk [kv_heads 128][H] +2 wv [kv_heads 128][H] +3 q_norm [128] +4 k_norm [128]
 *     +5 wo [H][q_heads 128] +6 ln_in [H] (input_layernorm) +7 ln_post [H] (post_attention_layernorm)
 *     +8 w_gate [I][H] +9 w_up [I][H] +10 w_down [H][I]
 * The library copies wq | wk | wv into one matrix and interleaves the gate and up rows at create; the other pointers must stay valid
 * until ak_decoder_destroy. Refused (non-zero, message naming the field in the last-error string) by the stack's one config check,
 * as ak_llama_create refuses it: head_dim != 128, q_heads % kv_heads, more than 4 query heads per kv head, hidden % 128,
 * intermediate % 64, a non-positive size (hidden and intermediate among them), rms_eps or rope_theta, a weight count other than
 * 2 + 11 * layers, a NULL pointer. */
int ak_decoder_create(const AkDecoderConfig *cfg, const void *const *weights_dev, int n_weights, ak_decoder_t *out);
int ak_decoder_destroy(ak_decoder_t h);
/* The tile layout of ak_encoder_forward_lens: B right-padded rows of S token ids `ld_ids` int32 apart, lengths `lens_stride` apart
 * (clamped to [0, S]; ids past a row's length are ignored; a row of length 0 embeds to zeros); out_dev [B][H] float32, the final norm
 * of token len - 1 of each row, L2-normalised when `normalise` != 0. S a multiple of 32, <= 8192 and <= max_position. Positions are
 * 0 .. len - 1 (RoPE is relative, so this equals a left-padded batch up to rounding). Asynchronous on `stream`. */
int ak_decoder_forward_lens(ak_decoder_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                            int normalise, float *out_dev, void *stream);
/* The RoPE table the decoder uploads at create: cos_out / sin_out [n_pos][head_dim / 2] float32, angle = float(pos) * inv_freq[i],
 * inv_freq[i] = 1 / theta^(2 i / head_dim) (HF's default rotary embedding; its cos / sin are these rows twice). Host only -- no GPU
 * work; exported so that the CPU suite can hold the table to HF's. */
int ak_decoder_rope_table(float theta, int head_dim, int n_pos, float *cos_out, float *sin_out);
/* The same table from GIVEN inverse frequencies inv_freq[half] (the second half of the routine above): angle = float(pos) * inv_freq[i].
 * For a caller that holds the model's own inv_freq buffer: torch's vectorised float32 pow, from which HF's buffer comes, is 1 ulp off
 * the correctly rounded 1 / theta^(2 i / head_dim) at one frequency in 128 (head_dim 256), and a binding can hand over HF's bits. */
int ak_decoder_rope_table_inv(const float *inv_freq, int half, int n_pos, float *cos_out, float *sin_out);

/* ---- ModernBERT encoders (nomic-ai/modernbert-embed-base, Alibaba-NLP/gte-modernbert-base, lightonai/modernbert-embed-large) ---- */
/* The forward pass of HF ModernBertModel: token embedding + LayerNorm, pre-norm layers (fused Wqkv, rotate_half RoPE at head size 64
 * with one theta for the global and one for the sliding-window layers, bidirectional attention -- in a sliding layer key k is visible
 * to query q iff |q - k| <= half_window --, GeGLU MLP), the final LayerNorm, then mean / cls pooling over the valid tokens and L2
 * normalisation. No bias anywhere, LayerNorms carry a weight only. bf16 MFMA GEMMs, float32 residual stream / norms / softmax. */
typedef void *ak_mbert_t;
#define AK_MBERT_MAX_LAYERS 64
typedef struct AkModernBertConfig {
    int vocab_size;     /* 50368 */
    int hidden;         /* 768 / 1024; a multiple of 128, <= 1024 */
    int layers;         /* 22 / 28; <= AK_MBERT_MAX_LAYERS */
    int heads;          /* 12 / 16; hidden / heads must be 64 */
    int intermediate;   /* 1152 / 2624; a multiple of 64 */
    int max_position;   /* 8192 (rows are limited to min(max_position, 8192) tokens) */
    float norm_eps;     /* 1e-5 */
    float global_rope_theta;   /* 160000: layers with layer_global[l] != 0 */
    float local_rope_theta;    /* 10000: the sliding-window layers */
    int half_window;    /* local_attention / 2 = 64; >= 1 */
    int layer_global[AK_MBERT_MAX_LAYERS];   /* per layer: != 0 full attention, 0 sliding window */
} AkModernBertConfig;
/* Weight order (device pointers; matrices bf16 row-major [out][in] as torch.nn.Linear.weight, vectors float32):
 *   0 tok_embeddings [vocab][H] bf16, 1 embeddings.norm [H], 2 final_norm [H],
 *   per layer l (base 3 + 6 * l):
 *     +0 attn_norm [H] (layer 0: the identity in the model -- the pointer is not read, pass any valid one) +1 Wqkv [3 H][H]
 *     +2 attn.Wo [H][H] +3 mlp_norm [H] +4 mlp.Wi [2 I][H] +5 mlp.Wo [H][I]
 * The library interleaves the two halves of Wi at create (row 2 j = Wi row j, row 2 j + 1 = Wi row I + j; when 2 I is not a multiple
 * of 256 it also pads Wi with zero rows and copies mlp.Wo with zero columns to match); the other pointers must stay valid until the
 * handle is destroyed. Refused (non-zero, message in the last-error string): head size != 64, hidden % 128 or > 1024,
 * intermediate % 64, half_window < 1, layers > AK_MBERT_MAX_LAYERS, a weight count other than 3 + 6 * layers. */
int ak_mbert_create(const AkModernBertConfig *cfg, const void *const *weights_dev, int n_weights, ak_mbert_t *out);
int ak_mbert_destroy(ak_mbert_t h);
/* The tile layout of the other forward_lens calls: B right-padded rows of S token ids `ld_ids` int32 apart, lengths `lens_stride`
 * apart (clamped to [0, S]; ids past a row's length are ignored; a row of length 0 embeds to zeros). pooling: AK_POOL_MEAN /
 * AK_POOL_CLS over the final norm of the valid tokens; out_dev [B][H] float32, L2-normalised when `normalise` != 0. S a multiple of
 * 32, <= 8192 and <= max_position. Asynchronous on `stream`. */
int ak_mbert_forward_lens(ak_mbert_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                          int pooling, int normalise, float *out_dev, void *stream);

/* ---- EmbeddingGemma encoders (google/embeddinggemma-300m) ---- */
/* The forward pass of HF Gemma3TextModel run bidirectionally (use_bidirectional_attention): token embedding times sqrt(hidden), layers
 * with four RMSNorms each (x rsqrt(mean(x^2) + eps) (1 + w): before and after both sub-layers), per-head q / k RMSNorm, rotate_half RoPE
 * at head size 256 with one theta for the full and one for the sliding-window layers, grouped-query attention (query head h reads kv
 * head h / (q_heads / kv_heads)) scaled by query_pre_attn_scalar^-0.5 -- in a sliding layer key k is visible to query q iff
 * |q - k| <= half_window --, a GeGLU MLP with the tanh GELU, the final norm; then the sentence-transformers tail: mean pooling over the
 * valid tokens, 0 - 2 Dense matrices (no bias, identity activation) in float32, L2 normalisation. No bias anywhere. bf16 MFMA GEMMs,
 * float32 residual stream / norms / softmax. */
typedef void *ak_gemma_t;
#define AK_GEMMA_MAX_LAYERS 64
typedef struct AkGemmaConfig {
    int vocab_size;     /* 262144 */
    int hidden;         /* 768; a multiple of 128, <= 1024 */
    int layers;         /* 24; <= AK_GEMMA_MAX_LAYERS */
    int q_heads;        /* 3 */
    int kv_heads;       /* 1; q_heads a multiple of it, q_heads / kv_heads <= 4 */
    int head_dim;       /* 256 (the only head size the attention kernel takes) */
    int intermediate;   /* 1152; a multiple of 64 */
    int max_position;   /* 2048 (rows are limited to min(max_position, 2048) tokens) */
    float rms_eps;      /* 1e-6 */
    float global_rope_theta;      /* 1e6: layers with layer_global[l] != 0 */
    float local_rope_theta;       /* 1e4: the sliding-window layers */
    float query_pre_attn_scalar;  /* 256: scores are scaled by its inverse square root, not by head_dim's */
    int half_window;    /* sliding_window / 2 = 256 (what the bidirectional config leaves a query to each side); >= 1 */
    float attn_softcap; /* attn_logit_softcapping: must be 0 (none) */
    float final_softcap;/* final_logit_softcapping: must be 0 (none) */
    int rope_type;      /* 0 = default; anything else is refused */
    int activation;     /* 0 = gelu_pytorch_tanh; anything else is refused */
    int attention_bias; /* must be 0 */
    int n_dense;        /* Dense modules behind the pooling: 0, 1 or 2 */
    int dense_out[2];   /* their output widths (3072, 768); the input width of the first is hidden, of the second dense_out[0] */
    int layer_global[AK_GEMMA_MAX_LAYERS];   /* per layer: != 0 full attention, 0 sliding window */
} AkGemmaConfig;
/* Weight order (device pointers; matrices bf16 row-major [out][in] as torch.nn.Linear.weight, norm vectors float32 AS STORED -- the
 * library adds the 1 --, Dense matrices float32):
 *   0 embed_tokens [vocab][H] bf16, 1 norm [H],
 *   per layer l (base 2 + 13 * l):
 *     +0 input_layernorm [H] +1 q_proj [q_heads 256][H] +2 k_proj [kv_heads 256][H] +3 v_proj [kv_heads 256][H] +4 q_norm [256]
 *     +5 k_norm [256] +6 o_proj [H][q_heads 256] +7 post_attention_layernorm [H] +8 pre_feedforward_layernorm [H] +9 gate_proj [I][H]
 *     +10 up_proj [I][H] +11 down_proj [H][I] +12 post_feedforward_layernorm [H]
 *   then n_dense Dense matrices [dense_out[i]][in] float32.
 * The library concatenates q / k / v_proj, interleaves gate / up_proj (row 2 j = gate row j, row 2 j + 1 = up row j; padded with zero
 * rows when 2 I is not a multiple of 256, down_proj with zero columns to match) and folds 1 + w into copies of the norm vectors at
 * create; embed_tokens, o_proj, down_proj and the Dense matrices must stay valid until the handle is destroyed. Refused (non-zero,
 * message naming the field in the last-error string): head_dim != 256, q_heads % kv_heads, a group > 4, hidden % 128 or > 1024,
 * intermediate % 64, a soft-cap, rope_type / activation / attention_bias != 0, half_window < 1, layers > AK_GEMMA_MAX_LAYERS, a
 * weight count other than 2 + 13 * layers + n_dense. */
int ak_gemma_create(const AkGemmaConfig *cfg, const void *const *weights_dev, int n_weights, ak_gemma_t *out);
int ak_gemma_destroy(ak_gemma_t h);
/* Replace the two rotary tables ak_gemma_create built from the thetas (ak_decoder_rope_table at head size 256) by the tables of GIVEN
 * inverse frequencies (ak_decoder_rope_table_inv): global_inv / local_inv, 128 host floats each -- the full-attention and the
 * sliding-attention layers' inv_freq buffers of the HF model. Optional; archi_amd.gemma.HipGemma calls it with the frequencies of HF's
 * own torch expression, so that the tables are HF's to the bit of every frequency. Waits for the handle's work in flight. */
int ak_gemma_set_rope_inv_freq(ak_gemma_t h, const float *global_inv, const float *local_inv);
/* The tile layout of ak_mbert_forward_lens. pooling: AK_POOL_MEAN only; out_dev [B][D] float32, D = the last Dense module's width (hidden
 * without one), L2-normalised when `normalise` != 0. S a multiple of 32, <= 2048 and <= max_position. Asynchronous on `stream`. */
int ak_gemma_forward_lens(ak_gemma_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                          int pooling, int normalise, float *out_dev, void *stream);

/* ---- NomicBERT encoders (nomic-ai/nomic-embed-text-v1 / -v1.5 / -v1-unsupervised, Snowflake/snowflake-arctic-embed-m-long) ---- */
/* The forward pass of HF NomicBertModel, the model behind Embeddings.embed_documents (manager.py:373) when embedding_class_map names a
 * NomicBERT checkpoint: word embedding + token-type row 0 + LayerNorm (no position table), POST-norm layers -- x = LayerNorm(x +
 * sub-layer(x)): the residual stream is the LayerNorm output -- with separate q / k / v projections, rotate_half RoPE at head size 64
 * with one theta over the whole head, bidirectional attention scaled by 1 / 8, a SwiGLU MLP (silu(gate) * up); no final norm; then
 * mean / cls pooling over the valid tokens and L2 normalisation. No bias in any Linear; every LayerNorm carries a weight and a bias.
 * bf16 MFMA GEMMs, float32 residual stream / norms / softmax. */
typedef void *ak_nomic_t;
typedef struct AkNomicBertConfig {
    int vocab_size;     /* 30528 */
    int hidden;         /* 768; a multiple of 128, <= 1024 */
    int layers;         /* 12; <= AK_MBERT_MAX_LAYERS */
    int heads;          /* 12; hidden / heads must be 64 */
    int intermediate;   /* 3072; a multiple of 64 */
    int type_vocab;     /* 2: rows of the token-type table (row 0 is the one read) */
    int max_position;   /* 8192 (rows are limited to min(max_position, 8192) tokens) */
    float ln_eps;       /* 1e-12 */
    float rope_theta;   /* 1000 (default RoPE: a dynamic-NTK checkpoint equals it up to its trained length, which max_position states) */
} AkNomicBertConfig;
/* Weight order (device pointers; matrices bf16 row-major [out][in] as torch.nn.Linear.weight, vectors float32):
 *   0 word_emb [vocab][H] bf16, 1 type_emb [type_vocab][H] float32, 2 emb_ln_g [H], 3 emb_ln_b [H],
 *   per layer l (base 4 + 11 * l):
 *     +0 wq [H][H] +1 wk [H][H] +2 wv [H][H] +3 wo [H][H] +4 ln1_g [H] +5 ln1_b [H] (post_attention_layernorm)
 *     +6 w_gate [I][H] +7 w_up [I][H] +8 w_down [H][I] +9 ln2_g [H] +10 ln2_b [H] (post_mlp_layernorm)
 * The library copies wq | wk | wv into one matrix and interleaves the gate and up rows at create (row 2 j = gate row j, row 2 j + 1 =
 * up row j; when 2 I is not a multiple of 256 it also pads them with zero rows and copies w_down with zero columns to match); the
 * other pointers must stay valid until the handle is destroyed. Refused (non-zero, message in the last-error string): head size != 64,
 * hidden % 128 or > 1024, intermediate % 64, layers > AK_MBERT_MAX_LAYERS, a non-positive size, ln_eps or rope_theta, a weight count
 * other than 4 + 11 * layers. */
int ak_nomic_create(const AkNomicBertConfig *cfg, const void *const *weights_dev, int n_weights, ak_nomic_t *out);
int ak_nomic_destroy(ak_nomic_t h);
/* One tile of the embedding step of manager.py:373, in the tile layout of ak_encoder_forward_lens: B right-padded rows of S token ids
 * `ld_ids` int32 apart, lengths `lens_stride` apart (clamped to [0, S]; ids past a row's length are ignored; a row of length 0 embeds
 * to zeros). pooling: AK_POOL_MEAN / AK_POOL_CLS over the last layer's rows of the valid tokens; out_dev [B][H] float32, L2-normalised
 * when `normalise` != 0. S a multiple of 32, <= 8192 and <= max_position. Asynchronous on `stream`. */
int ak_nomic_forward_lens(ak_nomic_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                          int pooling, int normalise, float *out_dev, void *stream);

/* ---- T5 encoders (sentence-transformers/gtr-t5-base / -large, sentence-t5-base / -large, GTR-initialised instructor models) ---- */
/* The forward pass of HF T5EncoderModel: the shared embedding (no scale, no position table), pre-norm layers with T5LayerNorm
 * (x * rsqrt(mean(x^2) + eps) * w, float32), separate q / k / v projections, bidirectional attention WITHOUT a 1 / sqrt(d) scale whose
 * only position signal is the learned per-head bias of the T5 bucket of key - query (one table for all layers), an un-gated ReLU
 * feed-forward (T5 v1.0) or the gated gelu_new one (T5 v1.1); the final_layer_norm per token; mean / cls pooling over the valid
 * tokens; the 0 - 2 bias-free Dense matrices of the sentence-transformers tail in float32; L2 normalisation. No bias in any Linear.
 * bf16 MFMA GEMMs, float32 residual stream / norms / softmax. */
typedef void *ak_t5_t;
typedef struct AkT5Config {
    int vocab_size;     /* 32128 */
    int hidden;         /* d_model 768 / 1024; a multiple of 128, <= 1024 */
    int layers;         /* 12 / 24; <= AK_MBERT_MAX_LAYERS */
    int heads;          /* 12 / 16; heads * 64 == hidden */
    int head_dim;       /* d_kv; 64 */
    int d_ff;           /* 3072 / 4096 (relu), 2048 / 2816 (gated-gelu); a multiple of 64 */
    int gated;          /* 0: wo(relu(wi(x))); 1: wo(gelu_new(wi_0(x)) * wi_1(x)) */
    int max_distance;   /* relative_attention_max_distance D (128): the bias table holds 2 D + 1 floats per head; 1 .. 4096 */
    float ln_eps;       /* layer_norm_epsilon 1e-6 */
    int n_dense;        /* Dense modules behind the pool: 0, 1 or 2 */
    int dense_out[2];   /* their output widths: multiples of 4, <= 4096 */
} AkT5Config;
/* Weight order (device pointers; matrices bf16 row-major [out][in] as torch.nn.Linear.weight, vectors float32):
 *   0 shared [vocab][H] bf16,
 *   1 rel_table [heads][2 D + 1] float32: entry [h][clamp(key - query, -D, D) + D] = block 0's relative_attention_bias weight at the
 *     T5 bucket of that distance, TIMES log2(e) (the softmax runs in base 2). The bidirectional bucket saturates at D on either
 *     side, so the clamped table is the whole bias at any row length; the caller builds it (archi_amd.t5.t5_rel_table evaluates
 *     HF's own float32 expression for the bucket) -- the library does not derive buckets,
 *   2 final_layer_norm [H],
 *   per layer l (base 3 + (8 + gated) * l):
 *     +0 ln0 [H] (layer.0.layer_norm), +1 wq, +2 wk, +3 wv, +4 wo [H][H], +5 ln1 [H] (layer.1.layer_norm),
 *     gated == 0: +6 wi [d_ff][H], +7 wo_ff [H][d_ff];   gated == 1: +6 wi_0 [d_ff][H], +7 wi_1 [d_ff][H], +8 wo_ff [H][d_ff],
 *   then the n_dense Dense matrices, float32 [out][in].
 * The library copies what it re-lays out (QKV concatenated, wi_0 / wi_1 interleaved, d_ff padded to the GEMM tile); every other
 * pointer must stay valid until the handle is destroyed. Refused (non-zero, message in the last-error string): head_dim != 64,
 * heads * 64 != hidden, hidden % 128 or > 1024, d_ff % 64, layers > AK_MBERT_MAX_LAYERS, a non-positive size, max_distance < 1 or
 * > 4096, ln_eps <= 0, gated other than 0 / 1, a Dense width out of range, a weight count other than 3 + (8 + gated) * layers + n_dense. */
int ak_t5_create(const AkT5Config *cfg, const void *const *weights_dev, int n_weights, ak_t5_t *out);
int ak_t5_destroy(ak_t5_t h);
/* One tile in the layout of ak_nomic_forward_lens. pooling: AK_POOL_MEAN / AK_POOL_CLS over the final_layer_norm rows of the valid
 * tokens; out_dev [B][out_dim] float32 (out_dim = the last Dense width, or hidden), L2-normalised when `normalise` != 0. S a multiple
 * of 32, <= 8192 (the model has no position limit of its own). Asynchronous on `stream`. */
int ak_t5_forward_lens(ak_t5_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                       int pooling, int normalise, float *out_dev, void *stream);

/* ---- Mistral / Llama decoder embedders (intfloat/e5-mistral-7b-instruct, Salesforce/SFR-Embedding-Mistral,
 * Linq-AI-Research/Linq-Embed-Mistral, the Llama-3.1-8B based embedders) ---- */
/* The other instruction-aware embedders the reference's retrievers single out (retrievers/utils.py:7-19), loaded by name through
 * HuggingFaceEmbeddings. The forward pass of HF MistralModel / LlamaModel: RMSNorm, rotate_half RoPE at head dim 128 WITHOUT a per-head
 * q / k norm, grouped-query causal attention -- with sliding_window = w > 0 key k is visible to query q iff k <= q and q - k <= w - 1
 * (HF's sliding_window_overlay), or bidirectional attention for the embedders trained without the causal mask --, SwiGLU MLP; then the
 * final norm of each row's LAST valid token, or the mean of the final norm over the valid tokens, and L2 normalisation
 * (sentence-transformers' lasttoken / mean Pooling + Normalize). No bias anywhere. bf16 MFMA GEMMs, float32 residual stream / norms / softmax.
 * The plain layer of the head-128 decoder stack (csrc/decoder128.hip): ak_decoder_* adds the per-head norm to it, ak_qwen2_* the biases. */
typedef void *ak_llama_t;
typedef struct AkLlamaConfig {
    int vocab_size;     /* 32000 (Mistral) / 128256 (Llama 3.1) */
    int hidden;         /* 4096; a multiple of 128 */
    int layers;         /* 32 */
    int q_heads;        /* 32 */
    int kv_heads;       /* 8; q_heads % kv_heads == 0, at most 4 query heads per kv head */
    int head_dim;       /* 128 (the only head size implemented) */
    int intermediate;   /* 14336; a multiple of 64 */
    int max_position;   /* 32768 / 131072 (rows are limited to min(max_position, 8192) tokens) */
    float rms_eps;      /* 1e-5 */
    float rope_theta;   /* 1e4 / 5e5: the default rotary table (ak_llama_set_rope_inv_freq replaces it, e.g. for rope_type llama3) */
    int sliding_window; /* 4096 (Mistral-7B-v0.1); 0 = none; < 0 is refused */
    int bidirectional;  /* 0 = causal (with the window); 1 = every key below the row's length for every query below it, the window ignored */
} AkLlamaConfig;
/* Weight order (device pointers; matrices bf16 row-major [out][in] exactly as torch.nn.Linear.weight, vectors float32):
 *   0 embed_tokens [vocab][H] bf16, 1 final norm [H],
 *   per layer l (base 2 + 9 * l):
 *     +0 wq [q_heads 128][H] +1 wk [kv_heads 128][H] +2 wv [kv_heads 128][H] +3 wo [H][q_heads 128]
 *     +4 ln_in [H] (input_layernorm) +5 ln_post [H] (post_attention_layernorm) +6 w_gate [I][H] +7 w_up [I][H] +8 w_down [H][I]
 * The library copies wq | wk | wv into one matrix and interleaves the gate and up rows at create; the other pointers must stay valid
 * until ak_llama_destroy. Refused (non-zero, message naming the field in the last-error string): head_dim != 128, q_heads % kv_heads,
 * more than 4 query heads per kv head, hidden % 128, intermediate % 64, sliding_window < 0, bidirectional other than 0 / 1, a non-positive size,
 * rms_eps or rope_theta, a weight count other than 2 + 9 * layers, a NULL pointer. */
int ak_llama_create(const AkLlamaConfig *cfg, const void *const *weights_dev, int n_weights, ak_llama_t *out);
int ak_llama_destroy(ak_llama_t h);
/* Replace the rotary table ak_llama_create built from rope_theta by the table of GIVEN inverse frequencies (ak_decoder_rope_table_inv):
 * inv_freq, 64 host floats -- the HF model's own inv_freq buffer (archi_amd.llama.rope_inv_freq restates HF's float32 expressions for
 * the default and the llama3 rope types). Waits for the handle's work in flight. */
int ak_llama_set_rope_inv_freq(ak_llama_t h, const float *inv_freq);
/* The tile layout and the argument checks of ak_decoder_forward_lens. pooling: AK_POOL_LAST (the final norm of token len - 1 of each
 * row) or AK_POOL_MEAN (the mean over t < len of the final norm of token t: the norm per token, before the mean; what the embedders
 * trained without the causal mask pair with bidirectional = 1); anything else is refused. out_dev [B][H] float32, L2-normalised when
 * `normalise` != 0. S a multiple of 32, <= 8192 and <= max_position. Asynchronous on `stream`. */
int ak_llama_forward_lens(ak_llama_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                          int pooling, int normalise, float *out_dev, void *stream);

/* ---- Qwen2 / Qwen2.5 decoder embedders (Alibaba-NLP/gte-Qwen2-1.5B-instruct, gte-Qwen2-7B-instruct, gte-Qwen1.5-7B-instruct,
 * infly/inf-retriever-v1 and -1.5b) ---- */
/* Instruction-aware embedders of the kind the reference's retrievers single out (retrievers/utils.py:7-19), loaded by name through
 * HuggingFaceEmbeddings. The forward pass of HF Qwen2Model: the Mistral / Llama layer above (RMSNorm, rotate_half RoPE at head dim 128,
 * grouped-query attention, SwiGLU MLP) WITH a bias on the q, k and v projections -- added in float32 to the projection's accumulator
 * before its bf16 store -- and with up to 8 query heads per kv head (Qwen2-1.5B: 6, Qwen2-7B: 7, Qwen2.5-3B: 8, Qwen2.5-14B: 5). Causal
 * attention without a window, or bidirectional attention for the embedders trained without the causal mask; then the final norm of
 * each row's LAST valid token, or the mean of the final norm over the valid tokens, and L2 normalisation (sentence-transformers'
 * lasttoken / mean Pooling + Normalize). bf16 MFMA GEMMs, float32 residual stream / norms / softmax / biases. The same handle, create
 * and layer loop as ak_llama_* (csrc/decoder128.hip); with all-zero biases the two give the same bits. */
typedef void *ak_qwen2_t;
typedef struct AkQwen2Config {
    int vocab_size;     /* 151646 (gte-Qwen2) */
    int hidden;         /* 1536 / 3584; a multiple of 128 */
    int layers;         /* 28 */
    int q_heads;        /* 12 / 28 */
    int kv_heads;       /* 2 / 4; q_heads % kv_heads == 0, at most 8 query heads per kv head */
    int head_dim;       /* 128 (the only head size implemented) */
    int intermediate;   /* 8960 / 18944; a multiple of 64 */
    int max_position;   /* 131072 (rows are limited to min(max_position, 8192) tokens) */
    float rms_eps;      /* 1e-6 */
    float rope_theta;   /* 1e6: the default rotary table (ak_qwen2_set_rope_inv_freq replaces it) */
    int bidirectional;  /* 0 = causal; 1 = every key below the row's length for every query below it */
} AkQwen2Config;
/* Weight order (device pointers; matrices bf16 row-major [out][in] exactly as torch.nn.Linear.weight, vectors and biases float32):
 *   0 embed_tokens [vocab][H] bf16, 1 final norm [H],
 *   per layer l (base 2 + 12 * l):
 *     +0 wq [q_heads 128][H] +1 wk [kv_heads 128][H] +2 wv [kv_heads 128][H] +3 bq [q_heads 128] +4 bk [kv_heads 128] +5 bv [kv_heads 128]
 *     +6 wo [H][q_heads 128] +7 ln_in [H] (input_layernorm) +8 ln_post [H] (post_attention_layernorm) +9 w_gate [I][H] +10 w_up [I][H]
 *     +11 w_down [H][I]
 * The library copies wq | wk | wv into one matrix and bq | bk | bv into one vector and interleaves the gate and up rows at create; the
 * other pointers must stay valid until ak_qwen2_destroy. Refused (non-zero, message naming the field in the last-error string):
 * head_dim != 128, q_heads % kv_heads, more than 8 query heads per kv head, hidden % 128, intermediate % 64, bidirectional other than
 * 0 / 1, a non-positive size, rms_eps or rope_theta, a weight count other than 2 + 12 * layers, a NULL pointer. */
int ak_qwen2_create(const AkQwen2Config *cfg, const void *const *weights_dev, int n_weights, ak_qwen2_t *out);
int ak_qwen2_destroy(ak_qwen2_t h);
/* ak_llama_set_rope_inv_freq for a Qwen2 handle: the rotary table of GIVEN inverse frequencies (64 host floats; rope_type llama3). */
int ak_qwen2_set_rope_inv_freq(ak_qwen2_t h, const float *inv_freq);
/* The tile layout, the argument checks and the poolings (AK_POOL_LAST / AK_POOL_MEAN) of ak_llama_forward_lens. out_dev [B][H] float32,
 * L2-normalised when `normalise` != 0. S a multiple of 32, <= 8192 and <= max_position. Asynchronous on `stream`. */
int ak_qwen2_forward_lens(ak_qwen2_t h, const int32_t *ids_dev, int ld_ids, const int32_t *lens_dev, int lens_stride, int B, int S,
                          int pooling, int normalise, float *out_dev, void *stream);

/* ---- host tokenizer: the tokenisation step inside Embeddings.embed_documents -------- */
/* manager.py:373 -> HuggingFaceEmbeddings -> sentence-transformers' BERT WordPiece tokenizer [upstream]. Pure host
 * code (no GPU work): multi-threaded, so that text -> token ids keeps up with ak_encoder_forward at ingestion.
 * vocab_path: the checkpoint's vocab.txt (one token per line, id = line number; needs [CLS] [SEP] [UNK]). */
typedef void *ak_wordpiece_t;
int ak_wordpiece_create(const char *vocab_path, int lowercase, ak_wordpiece_t *out);
/* The same tokenizer with the model's own special tokens (MPNet: cls "<s>", sep "</s>", unk "[UNK]"): cls / sep / unk are
 * emitted by name (each must be in the vocabulary), and a text that holds any of the n_specials strings `specials` literally
 * gets length -1 from ak_wordpiece_encode (the full tokenizer matches them in the raw text). ak_wordpiece_create is this with
 * "[CLS]", "[SEP]", "[UNK]" and the specials [CLS] [SEP] [UNK] [PAD] [MASK]. */
int ak_wordpiece_create_ex(const char *vocab_path, int lowercase, const char *cls, const char *sep, const char *unk,
                           const char *const *specials, int n_specials, ak_wordpiece_t *out);
int ak_wordpiece_destroy(ak_wordpiece_t h);
/* n texts as one UTF-8 blob, text i = blob[offsets[i] : offsets[i+1]]. out_ids: [n][max_len] int32, zero padded;
 * out_len[i] = ids of text i including [CLS] and [SEP], truncated to max_len (the last kept id is [SEP]), or -1 when
 * the text holds a byte >= 0x80 or a literal special token such as "[SEP]": those need the full Unicode tokenizer
 * and are left to the caller. threads <= 0: all host cores. */
int ak_wordpiece_encode(ak_wordpiece_t h, const char *blob, const int64_t *offsets, int64_t n, int max_len,
                        int threads, int32_t *out_ids, int32_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* ARCHI_KNN_H */
