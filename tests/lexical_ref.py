"""Reference for the device BM25 passes (csrc/lexical.hip), TESTS ONLY: a doc-major, row-by-row statement of what the two list
passes compute, one Python float (IEEE double, one rounding per operation) at a time.

  statistics pass over all live rows: n, sum_len, df per query term; a row matches when it holds at least one query term
  host step: avg = sum_len / n, idf_t = math.log(1.0 + (n - df_t + 0.5) / (df_t + 0.5)); terms with df_t = 0 drop out
  score pass per matching row: terms in the query's first-occurrence order, acc from 0.0,
      acc = acc + ((idf * tf) * (k1 + 1.0)) / (tf + k1 * ((1.0 - b) + (b * len) / avg))      [avg == 0: tf + k1 * (1.0 - b)]
      bm = sign * acc

test_lexical_cpu.py holds it to HostBm25.scores_arrays (posting-major, numpy) bit for bit, so the order of operations the kernels
restate is pinned before a kernel is involved.
"""
import math

import numpy as np


def doc_major_scores(row_offsets, terms, tfs, doc_len, alive, query_terms, k1=1.2, b=0.75, sign=1.0):
    """CSR lists of R rows (a row's term ids ascending), alive [R] bool, query_terms: term ids in query order (repeats allowed).
    -> (rows with at least one match, ascending [m] int64; their scores [m] float64)."""
    R = len(doc_len)
    q = list(dict.fromkeys(int(t) for t in query_terms))
    qset = set(q)
    n, sum_len = 0, 0
    df = dict.fromkeys(q, 0)
    matched = []                                   # (row, {term: tf}) of the live rows holding a query term
    for r in range(R):
        if not alive[r]:
            continue
        n += 1
        sum_len += int(doc_len[r])
        found = {}
        for e in range(int(row_offsets[r]), int(row_offsets[r + 1])):
            t = int(terms[e])
            if t in qset:
                found[t] = int(tfs[e])
                df[t] += 1
        if found:
            matched.append((r, found))
    if n == 0 or not matched:
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    avg = sum_len / n
    used = [t for t in q if df[t] > 0]
    idf = {t: math.log(1.0 + (n - df[t] + 0.5) / (df[t] + 0.5)) for t in used}
    rows, scores = [], []
    for r, found in matched:
        acc = 0.0
        dl = float(int(doc_len[r]))
        for t in used:
            if t not in found:
                continue
            tf = float(found[t])
            if avg > 0:
                norm = tf + k1 * ((1.0 - b) + (b * dl) / avg)
            else:
                norm = tf + k1 * (1.0 - b)
            acc = acc + ((idf[t] * tf) * (k1 + 1.0)) / norm
        rows.append(r)
        scores.append(sign * acc)
    return np.asarray(rows, np.int64), np.asarray(scores, np.float64)
