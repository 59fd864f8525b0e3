"""CPU restatement of ak_index_group_search's contract (include/archi_knn.h), TESTS ONLY: the complete ranking from the oracle's
exact search (k = every row), then the walk of the definition in plain Python. What the HIP kernels are held to bit for bit."""
import numpy as np

from oracle import knn_oracle as ko
from tests.fake_index import OracleIndex


def group_walk(ids, dist, slots, groups, k, group_size):
    """Steps 2-4 for one query. ids / dist / slots: the complete list in order; groups: key per row slot. Returns
    [(key, [(id, dist), ...])]: the first k groups by the position of their first row, each with its first group_size rows."""
    order, members = [], {}
    for i, d, s in zip(ids, dist, slots):
        key = int(groups[s])
        name = ("g", key) if key >= 0 else ("row", int(s))          # a negative key: the row is a group by itself
        if name not in members:
            members[name] = (key, [])
            order.append(name)
        if len(members[name][1]) < group_size:
            members[name][1].append((int(i), float(d)))
    return [members[name] for name in order[:k]]


def group_search_ref(rows, ids, alive, groups, queries, k, group_size, metric="cosine", dtype=None):
    """rows [n, dim]: the index's rows by slot (as fetch returns them, or raw values with the storage dtype to round them through),
    ids [n], alive [n] (None: all; a WHERE mask is and-ed in by the caller), groups [n] int32 keys by slot. Returns (ids [Q,k,g],
    dist [Q,k,g], keys [Q,k], sizes [Q,k], counts [Q]) padded with -1 / NaN / -1 / 0 like the library."""
    rows = np.ascontiguousarray(rows, np.float32)
    if dtype is not None:
        rows = ko.round_through(rows, dtype)
    ids = np.asarray(ids, np.int64)
    q = np.asarray(queries, np.float32)
    q = q[None] if q.ndim == 1 else q
    nq, g = len(q), group_size
    out_i = np.full((nq, k, g), -1, np.int64)
    out_d = np.full((nq, k, g), np.nan, np.float64)
    out_g = np.full((nq, k), -1, np.int32)
    out_s = np.zeros((nq, k), np.int32)
    cnt = np.zeros(nq, np.int32)
    n = len(rows)
    if n == 0 or nq == 0:
        return out_i, out_d, out_g, out_s, cnt
    li, ld, lc = ko.search(rows, q, n, metric, ids=ids, alive=alive)
    slot_of = {int(i): s for s, i in enumerate(ids) if alive is None or alive[s]}
    for qi in range(nq):
        m = int(lc[qi])
        slots = [slot_of[int(i)] for i in li[qi, :m]]
        won = group_walk(li[qi, :m], ld[qi, :m], slots, groups, k, g)
        cnt[qi] = len(won)
        for w, (key, mem) in enumerate(won):
            out_g[qi, w], out_s[qi, w] = key, len(mem)
            for j, (i, d) in enumerate(mem):
                out_i[qi, w, j], out_d[qi, w, j] = i, d
    return out_i, out_d, out_g, out_s, cnt


class GroupOracleIndex(OracleIndex):
    """OracleIndex + HipIndex.group_search, for the store's host logic."""

    GROUP_MAX_K = 32
    GROUP_MAX_SIZE = 8

    def group_search(self, queries, k, group_size=1, *, row_group, row_filter=None, filter_epoch=None, mode="auto",
                     return_stats=False):
        from archi_amd import HipBackendError
        if not 1 <= k <= self.GROUP_MAX_K:
            raise HipBackendError("ak_index_group_search: k must be in 1 .. 32")
        if not 1 <= group_size <= self.GROUP_MAX_SIZE:
            raise HipBackendError("ak_index_group_search: group_size must be in 1 .. 8")
        row_group = np.asarray(row_group, np.int32)
        # the keys are under the mask's contract: a stale (length, epoch) pair raises StaleFilterError like the library
        if (filter_epoch is not None and filter_epoch != self.epoch) or len(row_group) != self.slots or \
                (row_filter is not None and len(row_filter) != self.slots):
            from archi_amd import StaleFilterError
            raise StaleFilterError("stale row_group")
        alive = self.alive if row_filter is None else (self.alive & np.asarray(row_filter, np.uint8))
        return group_search_ref(self.rows, self.ids, alive, row_group, queries, k, group_size, self.metric)
