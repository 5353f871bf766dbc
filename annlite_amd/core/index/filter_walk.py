"""``FilterWalkMixin`` -- ``filter_search='graph'`` of the two HNSW indexes, ONE COPY of the policy: when a search that carries a
filter (``indices=``) is answered by the filtered walk (``graph_beam.h``'s admitted-result list beside the routing list) and when by
the parent's exact search, how wide the routing list is, and which queries the exact search answers again.

The index puts the mixin before its parent class and supplies ``MAX_EF``, ``FILTER_WALK_MIN_FRACTION`` and two hooks:

  * ``_filter_walk(q, ef_route, ef, admit, reach) -> cand, cand_d``: the walk (``reach`` f32 [B] receives the routing list's last place);
  * ``_filter_rank(x, q, cand, cand_d, k, ef, admit) -> d, i, depth``: the answer from the walk's list, and how far into the list
    (``depth`` places) it reaches.
"""
from typing import Optional

import torch

from .row_store import empty_answer, like_input


def routing_places(ef: int, n_rows: int, n_adm: int, max_ef: int) -> int:
    """Places of the routing list: with ``s = n_adm / n_rows`` the admitted share of the rows it gets ``ef / s`` of them (rounded up,
    at most ``max_ef``), so that about ``ef`` of the rows it keeps are admitted ones."""
    return min(max_ef, max(ef, -(-ef * n_rows // n_adm)))


def queries_to_reanswer(cand: torch.Tensor, cand_d: torch.Tensor, reach: torch.Tensor, depth: int) -> torch.Tensor:
    """i64 [n]: the queries whose list the exact search has to answer again, both on the walk's own distances.  Completeness: a list
    with fewer than ``depth`` rows.  Convergence: a list whose ``depth``-th row lies beyond ``reach``, the routing list's last place --
    inside that distance the walk looked as closely as the plain walk at ef_route does, beyond it the list only holds the admitted rows
    met on the way (a filter that admits nothing near the query: hnswlib walks on there, bounded by its admitted results; this walk
    is bounded by ef_route)."""
    return torch.nonzero((cand[:, depth - 1] < 0) | (cand_d[:, depth - 1] > reach)).reshape(-1)


class FilterWalkMixin:
    FILTER_SEARCH = ('exact', 'graph')

    def _check_filter_search(self, filter_search: Optional[str], exact_is: Optional[str] = None):
        """``exact_is``: the constructor's words for what 'exact' is; None: a call's value, which may be None (the constructor's holds)."""
        if filter_search is None and exact_is is None:
            return
        if filter_search not in self.FILTER_SEARCH:
            words = "'exact' or 'graph'" if exact_is is None else f"'exact' ({exact_is}) or 'graph' (the filtered walk)"
            raise ValueError(f'filter_search={filter_search!r}: {words}')

    def _init_filter_search(self, filter_search: str):
        self.filter_search = filter_search
        self.last_filter_path = None     # 'graph' / 'exact': how the last search that carried `indices` was answered
        self.last_filter_reanswered = 0  # ... and how many of its queries the exact search answered again

    def _filtered_answer(self, x, k: int, ef: int, indices, filter_search: Optional[str], walk_ok: bool):
        """The answer of a search that carries ``indices``, or None where the parent's exact search is to give it.  ``filter_search``:
        this call's (an order) or None (the constructor's: a rule, with a floor on the admitted share)."""
        self.last_filter_path, self.last_filter_reanswered = 'exact', 0
        if walk_ok and (filter_search or self.filter_search) == 'graph':
            return self._search_filtered_on_graph(x, k, ef, indices, forced=filter_search == 'graph')
        return None

    def _search_filtered_on_graph(self, x, k: int, ef: int, indices, forced: bool):
        """The filtered walk, or None where the exact search is to answer (no admitted row; the rule's selectivity floor).
        ``admit = valid & filter``; the routing list gets ``routing_places``, the result list ``ef``."""
        admit = self._filter_bits(indices)
        n_rows = self._n_rows
        n_adm = int(self._unpack_bits(admit, n_rows).sum().item())
        if n_adm == 0 or (not forced and n_adm < self.FILTER_WALK_MIN_FRACTION * n_rows):
            return None
        is_np = not isinstance(x, torch.Tensor)
        q = self._pre(x)
        B = q.shape[0]
        self.last_filter_path = 'graph'
        if B == 0:
            return like_input(is_np, *empty_answer(B, k, q.device))
        reach = torch.empty((B,), dtype=torch.float32, device=q.device)
        cand, cand_d = self._filter_walk(q, routing_places(ef, n_rows, n_adm, self.MAX_EF), ef, admit, reach)
        d, i, depth = self._filter_rank(x, q, cand, cand_d, k, ef, admit)
        short = queries_to_reanswer(cand, cand_d, reach, min(depth, n_adm))
        self.last_filter_reanswered = int(short.numel())  # (the one host look)
        if self.last_filter_reanswered:  # (from the caller's own rows: pre-processing them twice would not be the exact search's bits)
            xs = x.reshape(1, -1) if x.ndim == 1 else x
            ed, ei = super().search_batch(xs[short.to(xs.device) if isinstance(xs, torch.Tensor) else short.cpu().numpy()], limit=k,
                                          indices=indices)
            d[short], i[short] = self._to_dev(ed), self._to_dev(ei)
        return like_input(is_np, d, i)
