"""CPU restatement of ak_index_mmr_search's contract (include/archi_knn.h), TESTS ONLY: the candidate list from the oracle's
exact search, pair distances from the oracle's scalar cosine distance on the stored rows, the greedy pick in Python floats
(IEEE float64, one rounding per operation). What the HIP kernels are held to bit for bit."""
import math

import numpy as np

from oracle import knn_oracle as ko
from tests.fake_index import OracleIndex


def mmr_select(rows, dq, k, lam, cache=None, keys=None):
    """Rules 2-3. rows [m, dim] float32: the candidates' STORED rows in rank order; dq [m]: their float64 distances to the query.
    Returns the picked ranks, min(k, m) of them. cache / keys: optional dict of pair distances shared between calls, keyed by
    (keys[i], keys[j]) -- a pair's distance depends on the two rows only."""
    m = len(rows)
    lam = float(lam)
    oml = 1.0 - lam
    sq = [1.0 - float(d) for d in dq]
    red = [-math.inf] * m

    def s(i, j):
        i, j = (i, j) if i < j else (j, i)
        if cache is None:
            return 1.0 - ko.distance("cosine", rows[i], rows[j])
        key = (keys[i], keys[j])
        if key not in cache:
            cache[key] = ko.distance("cosine", rows[i], rows[j])
        return 1.0 - cache[key]

    picked, left = [], list(range(m))
    while len(picked) < min(k, m):
        p = left[0]                                   # the first pick is rank 0; later: the fallback when every score is NaN
        if picked:
            best, best_score = None, None
            for r in left:                            # ranks upward, strict >: the lowest rank wins a tie
                score = lam * sq[r] - oml * red[r]
                if score != score:                    # a NaN never wins
                    continue
                if best is None or score > best_score:
                    best, best_score = r, score
            if best is not None:
                p = best
        picked.append(p)
        left.remove(p)
        for r in left:
            v = s(r, p)
            if v > red[r]:                            # a NaN never updates
                red[r] = v
    return picked


def mmr_search_ref(rows, ids, alive, queries, k, fetch_k, lam, dtype=None, cache=None):
    """rows [n, dim]: the index's rows by slot (as fetch returns them, or raw values with the storage dtype to round them
    through), ids [n], alive [n] (None: all; a WHERE mask is and-ed in by the caller). Returns (ids [Q,k], dist [Q,k], counts [Q],
    ranks [Q,k]) padded with -1 / NaN / -1 like the library."""
    rows = np.ascontiguousarray(rows, np.float32)
    if dtype is not None:
        rows = ko.round_through(rows, dtype)
    ids = np.asarray(ids, np.int64)
    q = np.asarray(queries, np.float32)
    q = q[None] if q.ndim == 1 else q
    nq = len(q)
    out_i = np.full((nq, k), -1, np.int64)
    out_d = np.full((nq, k), np.nan, np.float64)
    out_r = np.full((nq, k), -1, np.int32)
    cnt = np.zeros(nq, np.int32)
    if len(rows) == 0:
        return out_i, out_d, cnt, out_r
    ci, cd, cc = ko.search(rows, q, fetch_k, "cosine", ids=ids, alive=alive)
    slot_of = {int(i): s for s, i in enumerate(ids) if alive is None or alive[s]}
    for qi in range(nq):
        m = int(cc[qi])
        slots = [slot_of[int(i)] for i in ci[qi, :m]]
        picks = mmr_select(rows[slots], cd[qi, :m], k, lam, cache=cache, keys=slots)
        cnt[qi] = len(picks)
        for t, r in enumerate(picks):
            out_i[qi, t], out_d[qi, t], out_r[qi, t] = ci[qi, r], cd[qi, r], r
    return out_i, out_d, cnt, out_r


class MmrOracleIndex(OracleIndex):
    """OracleIndex + HipIndex.mmr_search, for the store's host logic."""

    def mmr_search(self, queries, k, fetch_k=20, lambda_mult=0.5, mode="auto", row_filter=None, filter_epoch=None,
                   return_rank=False):
        if self.metric != "cosine":
            from archi_amd import HipBackendError
            raise HipBackendError("ak_index_mmr_search: cosine indexes only")
        if row_filter is not None:
            self.search(queries, 1, row_filter=row_filter, filter_epoch=filter_epoch)      # raises StaleFilterError like the library
        alive = self.alive if row_filter is None else (self.alive & np.asarray(row_filter, np.uint8))
        i, d, c, r = mmr_search_ref(self.rows, self.ids, alive, queries, k, fetch_k, lambda_mult)
        return (i, d, c, r) if return_rank else (i, d, c)
