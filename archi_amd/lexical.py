"""DeviceBm25 -- the BM25 scorer of hybrid_search with its index in HBM (csrc/lexical.hip).

Stands where the reference's pg_textsearch index stands (src/cli/templates/init.sql:294-300, queried at
src/data_manager/vectorstore/postgres_vectorstore.py:421-457). HostBm25 (vectorstore.py) keeps posting lists on the host and
scores them in numpy; this scorer keeps only the term dictionary and the tokeniser on the host. The lists live inside the
HipIndex, one sorted (term id, tf) list per row, and the whole hybrid query -- statistics, BM25, the hits' exact distances, the
combine, both top-k -- is one library call (HipIndex.hybrid_search). Same arithmetic in the same order as HostBm25.scores_arrays:
the two return the same float64 bits.
"""
from __future__ import annotations

import re
import secrets
from typing import Any, Dict, List, Tuple

import numpy as np

from ._lib import HipBackendError
from .chunktable import ChunkTable

_TOK = re.compile(r"\w+")           # HostBm25's tokeniser: \w+ on text.lower(), Python's Unicode semantics
ATTACH_ROWS = 65536                 # rows per ak_index_lex_attach call


def tokenize(text: str) -> List[str]:
    return _TOK.findall(text.lower())


def encode_rows(table: ChunkTable, lo: int, hi: int, terms: Dict[str, int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """CSR encoding of the live table positions [lo, hi): (row ids [m], row_offsets [m + 1], term ids, tfs, doc_len [m]). A row's
    term ids ascend; new words get the next id in `terms` in order of appearance (HostBm25's numbering). Positions that are dead
    are left out: a row dead on arrival is never scored. Caller holds the table lock."""
    alive = table._alive
    rids: List[int] = []
    offsets: List[int] = [0]
    flat_t: List[int] = []
    flat_f: List[int] = []
    dlen: List[int] = []
    get = terms.get
    for p in range(lo, hi):
        if not alive[p]:
            continue
        toks = _TOK.findall(table.text_at(p).lower())
        counts: Dict[int, int] = {}
        for w in toks:
            tid = get(w)
            if tid is None:
                tid = terms[w] = len(terms)
            counts[tid] = counts.get(tid, 0) + 1
        for tid in sorted(counts):
            flat_t.append(tid)
            flat_f.append(counts[tid])
        rids.append(int(table._ids[p]))
        offsets.append(len(flat_t))
        dlen.append(len(toks))
    return (np.asarray(rids, np.int64), np.asarray(offsets, np.int64), np.asarray(flat_t, np.int32), np.asarray(flat_f, np.int32),
            np.asarray(dlen, np.int32))


class DeviceBm25:
    """Okapi BM25 over the chunk texts of a ChunkTable with the index in HBM. A plug-in scorer like HostBm25
    (`scores(query, table)`, `scores_arrays(query, table)`), and -- what ArchiHipHybridVectorStore.hybrid_search looks for --
    `device_query`, which hands the store the query's term ids after bringing the device lists up to date. It needs a HipIndex:
    on an index without the lexical entry points (ShardedHipIndex, a test stand-in) it raises; use HostBm25 there.
    `sign=-1` reproduces the `<@>` operator's convention of returning negated scores."""

    def __init__(self, k1: float = 1.2, b: float = 0.75, sign: float = 1.0):
        self.k1, self.b, self.sign = float(k1), float(b), float(sign)
        self._terms: Dict[str, int] = {}
        self._index: Any = None
        self._table_key = None
        self._upto = 0
        self._gen = secrets.randbits(62) | 1          # this scorer's mark on the index's lists; moves on with every fresh start

    # -- which index ---------------------------------------------------------
    def use_index(self, index: Any) -> None:
        if not all(callable(getattr(index, m, None)) for m in ("lex_attach", "lex_clear", "lex_generation", "lex_scores", "hybrid_search")):
            raise HipBackendError(f"DeviceBm25 needs a HipIndex with the lexical entry points (lex_attach, hybrid_search); "
                                  f"{type(index).__name__} has none -- use HostBm25 with this store")
        if index is not self._index:
            self._index = index
            self._table_key = None                    # another index: its lists are not ours

    def _need_index(self) -> Any:
        if self._index is None:
            raise HipBackendError("DeviceBm25 has no index yet: the store hands it over (use_index) -- or use HostBm25")
        return self._index

    # -- sync ------------------------------------------------------------------
    def _sync(self, table: ChunkTable, index: Any) -> None:
        """Attach the lists of the positions appended since the last call. The table is append-only between vacuums and a delete
        is the index's own tombstone, so nothing is ever rewritten; a text changed in place or a vacuum (`text_epoch`), another
        table, or lists on the index that are not this scorer's (the generation) start over: clear, attach everything."""
        self.use_index(index)
        with table.lock:
            key = (id(table), table.text_epoch)
            if self._table_key != key or index.lex_generation() != self._gen:
                self._gen = (self._gen + 2) & ((1 << 63) - 1)
                index.lex_clear(self._gen)
                self._terms = {}
                self._upto = 0
                self._table_key = key
            n = table.positions
            for lo in range(self._upto, n, ATTACH_ROWS):
                hi = min(n, lo + ATTACH_ROWS)
                rids, ro, te, tf, dl = encode_rows(table, lo, hi, self._terms)
                if len(rids):
                    index.lex_attach(rids, ro, te, tf, dl, self._gen)
                self._upto = hi

    def term_ids(self, query: str) -> np.ndarray:
        """The query's known words as term ids, in first-occurrence order (an unknown word matches no row)."""
        ids = [self._terms[w] for w in dict.fromkeys(tokenize(query)) if w in self._terms]
        return np.asarray(ids, np.int32)

    def device_query(self, query: str, table: ChunkTable, index: Any) -> np.ndarray:
        """Bring the device lists up to date and return the query's term ids. Caller holds the table lock."""
        self._sync(table, index)
        return self.term_ids(query)

    # -- the plug-in scorer protocol ---------------------------------------------
    def scores_arrays(self, query: str, table: ChunkTable) -> Tuple[np.ndarray, np.ndarray]:
        """(table positions, scores) of the live rows matching at least one query term, positions ascending: HostBm25's
        contract, computed by the device passes (ak_index_lex_scores)."""
        index = self._need_index()
        with table.lock:
            self._sync(table, index)
            bm, hit, _ = index.lex_scores(self.term_ids(query), self.k1, self.b, self.sign)
            pos = np.flatnonzero(table._alive[: table.positions])
            if not len(pos) or not hit.any():
                return np.zeros(0, np.int64), np.zeros(0, np.float64)
            slots = index.lookup(table.rids_at(pos))
            ok = slots >= 0
            pos, slots = pos[ok], slots[ok]
            m = hit[slots] != 0
            return pos[m].astype(np.int64), bm[slots[m]]

    def scores(self, query: str, table: ChunkTable) -> Dict[int, float]:
        with table.lock:
            pos, sc = self.scores_arrays(query, table)
            return dict(zip(table.rids_at(pos).tolist(), sc.tolist()))
