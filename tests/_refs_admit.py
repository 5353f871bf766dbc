"""The float graph walk with an admitted-result list (annlite_graph_f32_search_admit), restated -- shared by
tests/test_graph_f32_admit_restated.py (which checks it, without a GPU) and tests/test_graph_f32_admit_walk.py (which pins the kernel
to it).  It IS ``_refs_pq_admit``'s walk one node at a time: the float kernel and the PQ kernel share the routing list C and the result
list R (graph_beam.h's AdmitList) and differ in the keys the caller hands in.  Not a conftest, no pytest setting."""
from _refs_pq_admit import walk_pq_admit_restated


def walk_admit_restated(links, seeds, keys, ef_route, ef, admit, table=None, stats=None):
    """One query.  ``links`` u32 [N, L+1] (count, ids), ``keys`` u64 [N] (``f32_key`` of the query's distance to every row), ``admit``
    bool [N]; ``table``: None = a visited table that holds every node, a number = one that records at most that many.  Returns (ids i64
    [ef], distance bits u32 [ef]): R ascending, (-1, +inf) at the tail.  ``stats`` receives ``expansions``, ``evals``,
    ``admitted_evaluated`` (the set of admitted nodes that were ever offered) and ``route_worst_bits``."""
    return walk_pq_admit_restated(links, seeds, keys, ef_route, ef, admit, width=1, table=table, stats=stats)
