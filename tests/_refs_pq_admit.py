"""The packed PQ graph walk with an admitted-result list (annlite_graph_search_packed_admit, graph_admit.hip), restated for one query
and for both expansion widths -- shared by tests/test_graph_pq_admit_restated.py (which checks it, without a GPU) and
tests/test_graph_packed_admit.py (which pins the kernel to it).  Not a conftest, no pytest setting.

Two sorted lists:

  * C, the routing list: ``tests/test_graph_pair.py::walk_restated``'s list at ``ef = ef_route`` -- seeds offered flat in rounds of 64,
    then ``width`` nodes expanded per step (the best unexpanded entries among the ``cap`` live ones), a step's unseen neighbours
    tested against C's worst entry before any of them is inserted; 1 / 2 / 3 / 4 registers per lane as there (3: the pair walk's
    list for 128 < ef <= 192).  ``admit`` never touches it.
  * R, the result list of ``ef`` places (``ResultList``; ``tests/_refs_admit.py`` is this walk at width 1).  Every batch C is offered R is
    offered too, restricted to admitted nodes; of those, the ones that beat R's worst entry AS IT IS NOW and are not in R already
    (nor came earlier in the same batch) are merged in.

R never acts on the walk, so one walk can carry several result lists (``walk_pq_restated``: the tests' five filters ride one walk).
Sums are the caller's: ``keys`` u64 [N] = ``_refs.f32_key`` of hnswlib::PQLookup (``oracle.adc_gather_c``) of the query's table over
every row; both lists are ordered by (key, node id)."""
import numpy as np

from _refs import f32_key, key_to_bits

INF_BITS = 0x7f800000
_NONE = (1 << 40, 1 << 40)  # behind every (key, id)


def regs(ef, width):
    """registers per lane of a list of ``ef`` places in the walk of that width"""
    return 1 if ef <= 64 else 2 if ef <= 128 else 3 if (ef <= 192 and width == 2) else 4


def pq_keys(oracle, lut, codes):
    """u64 [N]: the list key of the query's PQLookup sum to every row (``lut`` f32 [M, Ks], ``codes`` u8 [N, M])"""
    return f32_key(oracle.adc_gather_c(lut, codes, np.arange(codes.shape[0], dtype=np.int64)))


class ResultList:
    """R: ``ef`` live places out of 64 * regs slots, admitted nodes only.  ``offered``: node -> how often it was offered."""

    def __init__(self, ef, admit, width=1):
        self.ef, self.admit = ef, admit
        self.slots, self.cap = 64 * regs(ef, width), min(ef, 64 * regs(ef, width))
        self.res = []  # sorted [(key, node)]
        self.offered = {}

    def offer(self, nodes, keys):
        res, cap = self.res, self.cap
        worst = res[cap - 1] if len(res) >= cap else _NONE  # as it is NOW: before any node of this batch is merged
        have = set(res)
        for v in nodes:
            if not self.admit[v]:
                continue
            self.offered[int(v)] = self.offered.get(int(v), 0) + 1
            kv = (int(keys[v]), int(v))
            if kv < worst and kv not in have:
                have.add(kv)
                res.append(kv)
        res.sort()
        del res[self.slots:]

    def output(self):
        """(ids i64 [ef], distance bits u32 [ef]): ascending, (-1, +inf) at the tail"""
        ids = np.full(self.ef, -1, np.int64)
        bits_ = np.full(self.ef, INF_BITS, np.uint32)
        for i, (k, v) in enumerate(self.res[:self.cap]):
            ids[i] = v
            bits_[i] = key_to_bits(k)
        return ids, bits_


def walk_pq_restated(links, seeds, keys, ef_route, results, width=1, table=None, stats=None):
    """One query's walk.  ``links`` u32 [N, L+1] (count, ids), ``keys`` u64 [N]; ``results``: the ``ResultList``s that are offered what
    C is offered.  ``table``: None = a visited table that holds every node; a number = one that records at most that many nodes and
    reports every other node as new each time it is met (Beam::visit once its buckets are full).  ``stats`` receives ``expansions``,
    ``evals``, ``route_worst_bits`` (the sum at C's last place, +inf while C is not full) and ``routing`` (C's first ``cap`` entries as
    (ids i64 [ef_route], bits u32 [ef_route]))."""
    n = keys.shape[0]
    slots, cap = 64 * regs(ef_route, width), min(ef_route, 64 * regs(ef_route, width))
    lst = []  # C: sorted [(key, node, expanded)]
    seen = set()
    n_expand = n_eval = 0

    def visit(v):  # True: not seen before, as far as the table knows
        if v in seen:
            return False
        if table is None or len(seen) < table:
            seen.add(v)
        return True

    def offer(nodes):
        if not len(nodes):
            return
        worst = (lst[cap - 1][0], lst[cap - 1][1]) if len(lst) >= cap else _NONE
        have = {(t[0], t[1]) for t in lst}
        for v in nodes:
            kv = (int(keys[v]), int(v))
            if kv < worst and kv not in have:
                have.add(kv)
                lst.append((kv[0], kv[1], False))
        lst.sort(key=lambda t: (t[0], t[1]))
        del lst[slots:]
        for r in results:  # the same lanes, restricted to admitted nodes, under the same rule against R's own worst entry
            r.offer(nodes, keys)

    seeds = [int(s) for s in seeds]
    for s0 in range(0, len(seeds), 64):
        rnd = [s for s in seeds[s0:s0 + 64] if s < n]
        n_eval += len(rnd)
        offer(rnd)
    for t in list(lst):
        visit(t[1])
    while True:
        pick = [i for i, t in enumerate(lst[:cap]) if not t[2]][:width]
        if not pick:
            break
        for i in pick:
            lst[i] = (lst[i][0], lst[i][1], True)
        n_expand += len(pick)
        fresh = []
        for i in pick:  # (a neighbour of both nodes passes the table once -- while the table still records)
            row = links[lst[i][1]]
            fresh += [int(nb) for nb in row[1:1 + int(row[0])] if int(nb) < n and visit(int(nb))]
        n_eval += len(fresh)
        offer(fresh)
    if stats is not None:
        c_ids = np.full(ef_route, -1, np.int64)
        c_bits = np.full(ef_route, INF_BITS, np.uint32)
        for i, t in enumerate(lst[:cap]):
            c_ids[i], c_bits[i] = t[1], key_to_bits(t[0])
        stats.update(expansions=n_expand, evals=n_eval, routing=(c_ids, c_bits),
                     route_worst_bits=key_to_bits(lst[cap - 1][0]) if len(lst) >= cap else INF_BITS)


def walk_pq_admit_restated(links, seeds, keys, ef_route, ef, admit, width=1, table=None, stats=None):
    """The walk with ONE filter ``admit`` bool [N]: (ids i64 [ef], distance bits u32 [ef]) of R.  ``stats`` also receives
    ``admitted_evaluated``, the set of admitted nodes ever offered."""
    r = ResultList(ef, admit, width)
    walk_pq_restated(links, seeds, keys, ef_route, [r], width=width, table=table, stats=stats)
    if stats is not None:
        stats['admitted_evaluated'] = set(r.offered)
    return r.output()
