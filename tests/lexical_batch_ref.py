"""Reference for the BATCH hybrid query (csrc/lexical_batch.hip), TESTS ONLY: the two-leg evaluation of a batch of queries that
share ONE scan mask, stated in numpy over all rows, next to the formula it has to reproduce.

  all-rows formula (what the statement computes, tests/test_lexical_gpu.py's Brute):
      combined = (1.0 - distance) * w_s + COALESCE(bm25, 0) * w_b over the live rows that pass the WHERE mask,
      ORDER BY combined DESC (NaN first), id ASC, LIMIT k
  two-leg batch scheme:
      U        = live rows that pass the mask and hold a term of ANY query, plus the also rows (live, pass the mask, not in U yet)
      hit leg  : per query q every row of U: bm_q = the query's BM25 where the row holds a term of q, +0.0 for the rest of U;
                 combined = (1.0 - d) * w_s + bm_q * w_b; the best k by (NaN first, combined descending, id ascending)
      scan leg : per query the k nearest rows (distance ascending, id ascending) among live, passing, NOT in U -- one mask for all
      merge    : the caller's: scan rows get (1.0 - d) * w_s + 0 * w_b, then the same ordering over the <= 2 k candidates

BM25 itself is tests/lexical_ref.py's doc-major statement (held to HostBm25 bit for bit by test_lexical_cpu.py).
"""
import numpy as np

from tests import lexical_ref as lr


def bm25_rows(ro, terms, tfs, dl, alive, query_terms, k1=1.2, b=0.75, sign=1.0):
    """-> (bm [R] float64, +0.0 where the row holds no query term; hit [R] bool)."""
    rows, sc = lr.doc_major_scores(ro, terms, tfs, dl, alive, query_terms, k1, b, sign)
    bm = np.zeros(len(dl), np.float64)
    hit = np.zeros(len(dl), bool)
    bm[rows] = sc
    hit[rows] = True
    return bm, hit


def best(ids, comb, k):
    """The statement's ordering: NaN first, combined descending, id ascending -> (ids [<= k], combined [<= k])."""
    ids = np.asarray(ids, np.int64)
    comb = np.asarray(comb, np.float64)
    nan = comb != comb
    o = np.lexsort((ids, -np.where(nan, 0.0, comb), ~nan))[:k]
    return ids[o], comb[o]


def all_rows_topk(dist_q, bm_q, live, allowed, k, w_s, w_b):
    ids = np.flatnonzero(live & allowed)
    comb = (1.0 - dist_q[ids]) * w_s + bm_q[ids] * w_b
    return best(ids, comb, k)


def union_rows(hits, live, allowed, also):
    """U as a bool mask over the rows; hits [Q][R] bool."""
    ok = live & allowed
    U = ok & np.any(hits, axis=0)
    for s in also:
        if 0 <= s < len(U) and ok[s]:
            U[s] = True
    return U


def two_leg_batch(dist, bms, hits, live, allowed, also, k, w_s, w_b):
    """dist / bms / hits: [Q][R]. -> (U, per query ((hit ids, hit combined), (scan ids, scan distances)))."""
    U = union_rows(hits, live, allowed, also)
    u_ids = np.flatnonzero(U)
    rest = np.flatnonzero(live & allowed & ~U)
    legs = []
    for q in range(len(dist)):
        bm_q = np.where(hits[q][u_ids], bms[q][u_ids], 0.0)          # +0.0 for a row of U without a term of q
        comb = (1.0 - dist[q][u_ids]) * w_s + bm_q * w_b
        hit_leg = best(u_ids, comb, k)
        d = dist[q][rest]
        num = rest[d == d]                                              # a top-k scan never returns a NaN distance
        o = np.lexsort((num, dist[q][num]))[:k]
        legs.append((hit_leg, (num[o], dist[q][num[o]])))
    return U, legs


def merge(hit_leg, scan_leg, k, w_s, w_b):
    """ArchiHipHybridVectorStore's merge of the two lists -> (ids, combined)."""
    (hi, hc), (si, sd) = hit_leg, scan_leg
    c = np.concatenate([hc, (1.0 - sd.astype(np.float64)) * w_s + 0 * w_b])
    return best(np.concatenate([hi, si]), c, k)
