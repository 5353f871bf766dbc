"""Functional wrappers over the C ABI on torch device tensors.

Every function takes/returns ``torch`` tensors living on the current HIP device and launches the
hand-written gfx950 kernels of ``libannlite_hip.so`` on torch's current stream.  No function here
computes anything on the CPU; without a GPU they raise ``RuntimeError`` (``_capi.require_gpu``).
"""
from typing import List, Optional, Tuple

import numpy as np
import ctypes

import torch

from . import _capi
from ._capi import (CODES_PLAIN, CODES_SKEWED, LAYOUT_BMK, LAYOUT_TILED, LUT_IP, LUT_IPDIST, LUT_L2,
                    check, lib, scan_plan, stream_ptr)

_CODE_TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32}  # torch has no uint16/32 arithmetic; bits are what matter


def device() -> torch.device:
    _capi.require_gpu()
    return torch.device('cuda', torch.cuda.current_device())


def to_dev(a, dtype=None, dev=None) -> torch.Tensor:
    """numpy / torch (any device) -> contiguous tensor on the current HIP device (or on ``dev``)."""
    if dev is None:
        dev = device()
    if isinstance(a, np.ndarray):
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        elif a.dtype == np.uint64:
            a = a.view(np.int64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    else:
        t = a
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.to(dev, non_blocking=True).contiguous()


def code_bytes_of(t: torch.Tensor) -> int:
    return t.element_size()


def codes_to_numpy(t: torch.Tensor) -> np.ndarray:
    a = t.cpu().numpy()
    if a.dtype.kind != 'i' or a.dtype.itemsize == 1:
        return a
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])  # (same width: any row length)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- LUT
def lut_build(queries: torch.Tensor, codebooks: torch.Tensor, kind: int, layout: int = LAYOUT_BMK,
              qi: int = 4) -> torch.Tensor:
    """f32 [B,D] x f32 [M,Ks,dsub] -> LUT.  BMK: [B,M,Ks]; TILED: flat padded buffer (see header)."""
    assert queries.dtype == torch.float32 and codebooks.dtype == torch.float32
    assert queries.ndim == 2 and codebooks.ndim == 3
    B, D = queries.shape
    M, Ks, dsub = codebooks.shape
    assert D == M * dsub, 'input dimension must be Ds * M'
    if layout == LAYOUT_BMK:
        out = torch.empty((B, M, Ks), dtype=torch.float32, device=queries.device)
    else:
        out = torch.empty((((B + 15) // 16) * 16 * M * Ks,), dtype=torch.float32, device=queries.device)
    check(lib().annlite_lut_build(kind, queries.data_ptr(), B, D, codebooks.data_ptr(), M, Ks, out.data_ptr(),
                                  layout, qi, stream_ptr()), 'lut_build')
    return out


def lut_retile(lut_bmk: torch.Tensor, qi: int) -> torch.Tensor:
    B, M, Ks = lut_bmk.shape
    out = torch.empty((((B + 15) // 16) * 16 * M * Ks,), dtype=torch.float32, device=lut_bmk.device)
    check(lib().annlite_lut_retile(lut_bmk.data_ptr(), B, M, Ks, out.data_ptr(), qi, stream_ptr()), 'lut_retile')
    return out


# ---------------------------------------------------------------------------------------------- ADC
def adc_dist(adtable: torch.Tensor, codes: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pq_bind.dist_pqcodes_to_codebooks on device: f32 [M,Ks], codes [N,M] -> f32 [N] (into ``out`` when given)."""
    assert adtable.ndim == 2 and codes.ndim == 2 and adtable.dtype == torch.float32
    M, Ks = adtable.shape
    N = codes.shape[0]
    assert codes.shape[1] == M
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=codes.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == N and out.device == codes.device
    check(lib().annlite_adc_dist(adtable.data_ptr(), M, Ks, codes.data_ptr(), code_bytes_of(codes), N,
                                 out.data_ptr(), stream_ptr()), 'adc_dist')
    return out


def adc_gather(lut_bmk: torch.Tensor, codes: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    B, M, Ks = lut_bmk.shape
    assert cand.dtype == torch.int64 and cand.shape[0] == B
    R = cand.shape[1]
    out = torch.empty((B, R), dtype=torch.float32, device=codes.device)
    check(lib().annlite_adc_gather(lut_bmk.data_ptr(), B, M, Ks, codes.data_ptr(), code_bytes_of(codes),
                                   codes.shape[0], cand.data_ptr(), R, out.data_ptr(), stream_ptr()), 'adc_gather')
    return out


def graph_search(links: torch.Tensor, seeds: torch.Tensor, codes: torch.Tensor, lut_bmk: torch.Tensor, ef: int,
                 valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """GPU beam search over exported HNSW level-0 lists (``annlite_graph_search``): ``links`` i32 [N, L+1]
    (count, ids), ``seeds`` i32 [S], PLAIN ``codes`` u8 [N, M], L2 tables f32 [B, M, Ks].  Returns
    (ids i64 [B, ef] ascending by PQ distance, -1 padded; dist f32 [B, ef])."""
    B, M, Ks = lut_bmk.shape
    N = codes.shape[0] if n_rows is None else n_rows
    out_i = torch.empty((B, ef), dtype=torch.int64, device=codes.device)
    out_d = torch.empty((B, ef), dtype=torch.float32, device=codes.device)
    check(lib().annlite_graph_search(links.data_ptr(), links.shape[1] - 1, seeds.data_ptr(), seeds.numel(), codes.data_ptr(),
                                     N, M, Ks, _ptr(valid_bits), lut_bmk.data_ptr(), B, int(ef), out_i.data_ptr(),
                                     out_d.data_ptr(), stream_ptr()), 'graph_search')
    return out_i, out_d


def graph_pack(links: torch.Tensor, codes: torch.Tensor, n_rows: Optional[int] = None) -> torch.Tensor:
    """Packed node records (``annlite_graph_pack``): u8 [N, record_bytes] = every node's neighbours' code rows + its link
    list, from the exported lists ``links`` i32 [N, L+1] and the PLAIN ``codes`` u8 [N, M]."""
    import ctypes

    N = codes.shape[0] if n_rows is None else n_rows
    L, M = links.shape[1] - 1, codes.shape[1]
    nb = ctypes.c_int64(0)
    check(lib().annlite_graph_record_bytes(L, M, ctypes.byref(nb)), 'graph_record_bytes')
    out = torch.empty((max(N, 1), int(nb.value)), dtype=torch.uint8, device=codes.device)
    check(lib().annlite_graph_pack(links.data_ptr(), L, codes.data_ptr(), N, M, out.data_ptr(), stream_ptr()), 'graph_pack')
    return out


def graph_search_packed(packed: torch.Tensor, links_per_node: int, seeds: torch.Tensor, codes: torch.Tensor, lut_bmk: torch.Tensor,
                        ef: int, valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, expand_width: int = 1
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``graph_search`` over packed node records (``annlite_graph_search_packed``): one contiguous read per expansion, the
    next record prefetched; candidate lists bit-equal to ``graph_search``'s.  ``expand_width=2``
    (``annlite_graph_search_packed_ex``): the pair walk -- the two best unexpanded entries per step, half as many dependent steps;
    its own (pinned) expansion order."""
    B, M, Ks = lut_bmk.shape
    N = codes.shape[0] if n_rows is None else n_rows
    out_i = torch.empty((B, ef), dtype=torch.int64, device=codes.device)
    out_d = torch.empty((B, ef), dtype=torch.float32, device=codes.device)
    if int(expand_width) != 1:
        check(lib().annlite_graph_search_packed_ex(packed.data_ptr(), int(links_per_node), seeds.data_ptr(), seeds.numel(),
                                                   codes.data_ptr(), N, M, Ks, _ptr(valid_bits), lut_bmk.data_ptr(), B, int(ef),
                                                   int(expand_width), out_i.data_ptr(), out_d.data_ptr(), stream_ptr()),
              'graph_search_packed_ex')
        return out_i, out_d
    check(lib().annlite_graph_search_packed(packed.data_ptr(), int(links_per_node), seeds.data_ptr(), seeds.numel(), codes.data_ptr(),
                                            N, M, Ks, _ptr(valid_bits), lut_bmk.data_ptr(), B, int(ef), out_i.data_ptr(),
                                            out_d.data_ptr(), stream_ptr()), 'graph_search_packed')
    return out_i, out_d


def _admit_walk_outputs(B: int, ef: int, N: int, admit_bits: Optional[torch.Tensor], route_worst: Optional[torch.Tensor],
                        device) -> Tuple[torch.Tensor, torch.Tensor]:
    """What the two filtered walks ask of ``admit_bits`` and ``route_worst``, and their (ids i64 [B, ef], dist f32 [B, ef]) outputs."""
    assert route_worst is None or (route_worst.dtype == torch.float32 and route_worst.is_contiguous() and route_worst.numel() == B
                                   and route_worst.device == device)
    # (None goes to the library, which refuses it)
    assert admit_bits is None or (admit_bits.is_contiguous() and admit_bits.element_size() == 4 and admit_bits.numel() * 32 >= N)
    return torch.empty((B, ef), dtype=torch.int64, device=device), torch.empty((B, ef), dtype=torch.float32, device=device)


def graph_search_packed_admit(packed: torch.Tensor, links_per_node: int, seeds: torch.Tensor, codes: torch.Tensor, lut_bmk: torch.Tensor,
                              ef_route: int, ef: int, admit_bits: torch.Tensor, n_rows: Optional[int] = None, expand_width: int = 1,
                              route_worst: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_graph_search_packed_admit``: ``graph_search_packed`` at ``ef = ef_route`` -- same expansions, same rows evaluated --
    that keeps, beside the routing list, the ``ef <= ef_route`` best rows set in the bitmap ``admit_bits`` (i32 words over the rows;
    required) among everything it evaluates.  Returns (ids i64 [B, ef] ascending by (PQLookup sum, id), admitted rows only, -1 at the
    tail; dist f32 [B, ef], +inf there).  ``route_worst`` f32 [B], when given, receives the sum at the routing list's last place (+inf
    while that list is not full): how far the walk reached."""
    assert codes.dtype == torch.uint8 and codes.is_contiguous() and packed.is_contiguous() and lut_bmk.is_contiguous()
    assert lut_bmk.dtype == torch.float32 and seeds.is_contiguous() and seeds.element_size() == 4
    B, M, Ks = lut_bmk.shape
    assert codes.shape[1] == M
    N = codes.shape[0] if n_rows is None else int(n_rows)
    assert N <= codes.shape[0] and N <= packed.shape[0]
    out_i, out_d = _admit_walk_outputs(B, ef, N, admit_bits, route_worst, codes.device)
    check(lib().annlite_graph_search_packed_admit(packed.data_ptr(), int(links_per_node), seeds.data_ptr(), seeds.numel(),
                                                  codes.data_ptr(), N, M, Ks, _ptr(admit_bits), lut_bmk.data_ptr(), B, int(ef_route),
                                                  int(ef), int(expand_width), out_i.data_ptr(), out_d.data_ptr(), _ptr(route_worst),
                                                  stream_ptr()), 'graph_search_packed_admit')
    return out_i, out_d


def graph_record_bytes(links_per_node: int, M: int) -> int:
    import ctypes

    nb = ctypes.c_int64(0)
    check(lib().annlite_graph_record_bytes(int(links_per_node), int(M), ctypes.byref(nb)), 'graph_record_bytes')
    return int(nb.value)


def graph_build_sdc(codebooks: torch.Tensor) -> torch.Tensor:
    """Symmetric code-to-code L2 table f32 [M, Ks, Ks] of the GPU graph build (``annlite_graph_build_sdc``)."""
    M, Ks, dsub = codebooks.shape
    out = torch.empty((M, Ks, Ks), dtype=torch.float32, device=codebooks.device)
    check(lib().annlite_graph_build_sdc(codebooks.data_ptr(), M, Ks, dsub, out.data_ptr(), stream_ptr()), 'graph_build_sdc')
    return out


def graph_build_select(cand: torch.Tensor, base0: int, codes: torch.Tensor, sdc: torch.Tensor, max_keep: int,
                       links: torch.Tensor) -> torch.Tensor:
    """``annlite_graph_build_select``: the lists of the batch's points (nodes ``base0 + i``) from their candidate lists ``cand``
    i64 [b, ef]; writes ``links`` rows in place, returns the (target << 32 | source) pairs i64 [b, max_keep] (INT64_MAX = none)."""
    b, ef = cand.shape
    M, Ks = codes.shape[1], sdc.shape[1]
    pairs = torch.empty((b, int(max_keep)), dtype=torch.int64, device=codes.device)
    check(lib().annlite_graph_build_select(cand.data_ptr(), int(ef), b, int(base0), codes.data_ptr(), M, Ks, sdc.data_ptr(),
                                           int(max_keep), links.data_ptr(), links.shape[1] - 1, pairs.data_ptr(), stream_ptr()),
          'graph_build_select')
    return pairs


def graph_build_reverse(keys_sorted: torch.Tensor, seg: torch.Tensor, codes: torch.Tensor, sdc: torch.Tensor, links: torch.Tensor):
    """``annlite_graph_build_reverse``: reverse links for the sorted pairs; ``seg`` i64 [S + 1] bounds the runs of equal target."""
    M, Ks = codes.shape[1], sdc.shape[1]
    check(lib().annlite_graph_build_reverse(keys_sorted.data_ptr(), seg.data_ptr(), seg.numel() - 1, codes.data_ptr(), M, Ks,
                                            sdc.data_ptr(), links.data_ptr(), links.shape[1] - 1, stream_ptr()), 'graph_build_reverse')


def graph_pack_nodes(links: torch.Tensor, codes: torch.Tensor, nodes: torch.Tensor, packed: torch.Tensor, n_rows: int):
    """``annlite_graph_pack_nodes``: re-pack the records of ``nodes`` i64 [n] in place."""
    check(lib().annlite_graph_pack_nodes(links.data_ptr(), links.shape[1] - 1, codes.data_ptr(), int(n_rows), codes.shape[1],
                                         nodes.data_ptr(), nodes.numel(), packed.data_ptr(), stream_ptr()), 'graph_pack_nodes')


# ---------------------------------------------------------------------------------------------- float graph (graph_f32.hip)
def graph_f32_search(metric: int, queries: torch.Tensor, vectors: torch.Tensor, links: torch.Tensor, seeds: torch.Tensor, ef: int,
                     valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_graph_f32_search``: the beam walk over the level-0 lists ``links`` i32 [N, L+1] (count, ids) with exact distances on
    the float rows ``vectors`` f32 [N, D] (``exact_gather_dist``'s bits).  Returns (ids i64 [B, ef] ascending by (distance, id), rows
    cleared in ``valid_bits`` blanked in place to -1; dist f32 [B, ef], +inf there)."""
    assert queries.dtype == torch.float32 and vectors.dtype == torch.float32 and queries.is_contiguous() and vectors.is_contiguous()
    assert links.is_contiguous() and seeds.is_contiguous() and links.element_size() == 4 and seeds.element_size() == 4
    B, D = queries.shape
    assert vectors.shape[1] == D
    N = vectors.shape[0] if n_rows is None else int(n_rows)
    assert N <= vectors.shape[0] and N <= links.shape[0]
    out_i = torch.empty((B, ef), dtype=torch.int64, device=vectors.device)
    out_d = torch.empty((B, ef), dtype=torch.float32, device=vectors.device)
    check(lib().annlite_graph_f32_search(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), N, links.data_ptr(), links.shape[1] - 1,
                                         seeds.data_ptr(), seeds.numel(), _ptr(valid_bits), int(ef), out_i.data_ptr(), out_d.data_ptr(),
                                         stream_ptr()), 'graph_f32_search')
    return out_i, out_d


def graph_f32_search_admit(metric: int, queries: torch.Tensor, vectors: torch.Tensor, links: torch.Tensor, seeds: torch.Tensor,
                           ef_route: int, ef: int, admit_bits: torch.Tensor, n_rows: Optional[int] = None,
                           route_worst: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_graph_f32_search_admit``: ``graph_f32_search`` at ``ef = ef_route`` -- same expansions, same rows evaluated -- that
    keeps, beside the routing list, the ``ef <= ef_route`` best rows set in the bitmap ``admit_bits`` (i32 words over the rows; required)
    among everything it evaluates.  Returns (ids i64 [B, ef] ascending by (distance, id), admitted rows only, -1 at the tail; dist f32
    [B, ef], +inf there).  ``route_worst`` f32 [B], when given, receives the distance of the routing list's last place (+inf while that
    list is not full): how far the walk reached."""
    assert queries.dtype == torch.float32 and vectors.dtype == torch.float32 and queries.is_contiguous() and vectors.is_contiguous()
    assert links.is_contiguous() and seeds.is_contiguous() and links.element_size() == 4 and seeds.element_size() == 4
    B, D = queries.shape
    assert vectors.shape[1] == D
    N = vectors.shape[0] if n_rows is None else int(n_rows)
    assert N <= vectors.shape[0] and N <= links.shape[0]
    out_i, out_d = _admit_walk_outputs(B, ef, N, admit_bits, route_worst, vectors.device)
    check(lib().annlite_graph_f32_search_admit(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), N, links.data_ptr(),
                                               links.shape[1] - 1, seeds.data_ptr(), seeds.numel(), _ptr(admit_bits), int(ef_route),
                                               int(ef), out_i.data_ptr(), out_d.data_ptr(), _ptr(route_worst), stream_ptr()),
          'graph_f32_search_admit')
    return out_i, out_d


def graph_f32_search_stats() -> Tuple[int, int]:
    """(expansions, rows evaluated) of the last float graph walk, with or without an admit list (ANNLITE_DEBUG_COUNTERS=1)."""
    out = (ctypes.c_uint64 * 2)()
    check(lib().annlite_graph_f32_search_stats(out), 'graph_f32_search_stats')
    return int(out[0]), int(out[1])


def graph_f32_build_select(metric: int, cand: torch.Tensor, base0: int, vectors: torch.Tensor, max_keep: int, links: torch.Tensor,
                           n_rows: Optional[int] = None) -> torch.Tensor:
    """``annlite_graph_f32_build_select``: ``graph_build_select`` with the float distance between the rows of ``vectors``."""
    assert cand.dtype == torch.int64 and cand.is_contiguous() and vectors.dtype == torch.float32 and vectors.is_contiguous()
    b, ef = cand.shape
    N = vectors.shape[0] if n_rows is None else int(n_rows)
    assert N <= vectors.shape[0] and N <= links.shape[0] and links.is_contiguous() and links.element_size() == 4
    pairs = torch.empty((b, int(max_keep)), dtype=torch.int64, device=vectors.device)
    check(lib().annlite_graph_f32_build_select(int(metric), cand.data_ptr(), int(ef), b, int(base0), vectors.data_ptr(), N, vectors.shape[1],
                                               int(max_keep), links.data_ptr(), links.shape[1] - 1, pairs.data_ptr(), stream_ptr()),
          'graph_f32_build_select')
    return pairs


def graph_f32_build_reverse(metric: int, keys_sorted: torch.Tensor, seg: torch.Tensor, vectors: torch.Tensor, links: torch.Tensor,
                            n_rows: Optional[int] = None):
    """``annlite_graph_f32_build_reverse``: ``graph_build_reverse`` with the float distance between the rows of ``vectors``."""
    assert keys_sorted.dtype == torch.int64 and seg.dtype == torch.int64 and keys_sorted.is_contiguous() and seg.is_contiguous()
    assert vectors.dtype == torch.float32 and vectors.is_contiguous() and links.is_contiguous() and links.element_size() == 4
    N = vectors.shape[0] if n_rows is None else int(n_rows)
    assert N <= vectors.shape[0] and N <= links.shape[0]
    check(lib().annlite_graph_f32_build_reverse(int(metric), keys_sorted.data_ptr(), seg.data_ptr(), seg.numel() - 1, vectors.data_ptr(), N,
                                                vectors.shape[1], links.data_ptr(), links.shape[1] - 1, stream_ptr()),
          'graph_f32_build_reverse')


class ScanWorkspace:
    """Re-usable device scratch for the scan (avoids an allocation per search call).  One buffer PER STREAM:
    batches issued on different streams run concurrently (the next batch's kernels fill the CUs the previous
    scan's tail leaves idle) and must not share scratch."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, dev) -> torch.Tensor:
        key = stream_ptr()
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes or buf.device != dev:
            buf = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev)
            self.bufs[key] = buf
        return buf


def adc_scan_topk(codes: torch.Tensor, lut: torch.Tensor, B: int, k: int, M: int, Ks: int,
                  valid_bits: Optional[torch.Tensor] = None, row_base: int = 0, n_rows: Optional[int] = None,
                  codes_layout: int = CODES_PLAIN, workspace: Optional[ScanWorkspace] = None,
                  out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batched flat ADC scan + exact top-k.  ``lut`` must be in the plan's layout (TILED when
    ``scan_plan(...).fast`` else BMK).  Returns (f32 [B,k], i64 [B,k]) ascending by (dist, id)."""
    N = codes.shape[0] if n_rows is None else n_rows
    cb = code_bytes_of(codes)
    plan = scan_plan(N, M, Ks, cb, B, k)
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(plan.workspace_bytes), dev)
    if out is None:
        od = torch.empty((B, k), dtype=torch.float32, device=dev)
        oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    else:
        od, oi = out
    check(lib().annlite_adc_scan_topk(codes.data_ptr(), cb, codes_layout, N, M, Ks, _ptr(valid_bits), lut.data_ptr(), B, k,
                                      row_base, od.data_ptr(), oi.data_ptr(), ws.data_ptr(), ws.numel(),
                                      stream_ptr()), 'adc_scan_topk')
    return od, oi


def adc_scan_topk_packed(codes: torch.Tensor, lut: torch.Tensor, B: int, k: int, M: int, Ks: int,
                         valid_bits: Optional[torch.Tensor] = None, row_base: int = 0, n_rows: Optional[int] = None,
                         codes_layout: int = CODES_PLAIN, workspace: Optional[ScanWorkspace] = None) -> torch.Tensor:
    """``adc_scan_topk`` with the result in ONE i64 tensor [B, k, 2] = (global id, f32 distance bits): the
    buffer a rank contributes to the single all-gather of the row-sharded search."""
    N = codes.shape[0] if n_rows is None else n_rows
    cb = code_bytes_of(codes)
    plan = scan_plan(N, M, Ks, cb, B, k)
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(plan.workspace_bytes), dev)
    out = torch.empty((B, k, 2), dtype=torch.int64, device=dev)
    check(lib().annlite_adc_scan_topk_packed(codes.data_ptr(), cb, codes_layout, N, M, Ks, _ptr(valid_bits),
                                             lut.data_ptr(), B, k, row_base, out.data_ptr(), ws.data_ptr(),
                                             ws.numel(), stream_ptr()), 'adc_scan_topk_packed')
    return out


def pq_search_topk(lut_kind: int, queries: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, k: int, M: int,
                   Ks: int, valid_bits: Optional[torch.Tensor] = None, row_base: int = 0, n_rows: Optional[int] = None,
                   codes_layout: int = CODES_PLAIN, workspace: Optional[ScanWorkspace] = None, packed: bool = False,
                   sqrt: bool = False, state=None):
    """LUT build + scan + top-k in one C call (``annlite_pq_search_topk_ex``).  ``queries`` f32 [B, D] already
    pre-processed (normalised for cosine).  Returns (f32 [B,k], i64 [B,k]) or, with ``packed``, i64 [B,k,2].
    ``state``: the table's ``_capi.ScanState`` (the library's kernel choice remembers what earlier launches measured)."""
    N = codes.shape[0] if n_rows is None else n_rows
    B, D = queries.shape
    cb = code_bytes_of(codes)
    need = ctypes.c_int64(0)
    check(lib().annlite_pq_search_workspace_bytes(N, M, Ks, cb, B, k, ctypes.byref(need)), 'pq_search_workspace_bytes')
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(need.value), dev)
    od = oi = op = None
    if packed:
        op = torch.empty((B, k, 2), dtype=torch.int64, device=dev)
    else:
        od = torch.empty((B, k), dtype=torch.float32, device=dev)
        oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    check(lib().annlite_pq_search_topk_ex(lut_kind, queries.data_ptr(), B, D, codebooks.data_ptr(), codes.data_ptr(), cb,
                                          codes_layout, N, M, Ks, _ptr(valid_bits), k, row_base, _ptr(od), _ptr(oi), _ptr(op),
                                          1 if sqrt else 0, ws.data_ptr(), ws.numel(), stream_ptr(),
                                          state.ptr if state is not None else None), 'pq_search_topk')
    return op if packed else (od, oi)


def debug_seed_candidates(queries: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, seed_rows: int,
                          valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                          codes_layout: int = CODES_PLAIN) -> Optional[torch.Tensor]:
    """Test hook (``annlite_debug_seed_candidates``): the rows the MFMA launch nominates for the seed bound, int64 [B, 512]
    (-1 = none); ``None`` where the launch does not apply (not M = 16 / 128-d, seed_rows not a multiple of 8192 ...)."""
    N = codes.shape[0] if n_rows is None else n_rows
    B, D = queries.shape
    M, Ks = codebooks.shape[0], codebooks.shape[1]
    out = torch.empty((B, 512), dtype=torch.int32, device=codes.device)
    rc = lib().annlite_debug_seed_candidates(queries.data_ptr(), B, D, codebooks.data_ptr(), codes.data_ptr(), codes_layout, N, M, Ks,
                                             _ptr(valid_bits), int(seed_rows), out.data_ptr(), stream_ptr())
    from ._capi import NOT_APPLICABLE

    if rc == NOT_APPLICABLE:
        return None
    check(rc, 'debug_seed_candidates')
    o = out.to(torch.int64)
    return torch.where(o < 0, o + (1 << 32), o).masked_fill(out == -1, -1)


def pq_search_split(phase: int, lut_kind: int, queries: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, k: int, M: int,
                    Ks: int, state, workspace: ScanWorkspace, valid_bits: Optional[torch.Tensor] = None, row_base: int = 0,
                    n_rows: Optional[int] = None, codes_layout: int = CODES_PLAIN, seed_rows: int = 0,
                    seed_keys: Optional[torch.Tensor] = None):
    """One half of the row-sharded search with a seed exchange (``annlite_pq_search_split``).
    ``PHASE_PREPARE`` -> the rank's seed keys i64 [B, SEED_KEYS], or None when the split does not apply to this batch (nothing
    was launched: make the plain call); ``PHASE_SCAN`` -> the packed result i64 [B, k, 2] of the prepared batch (same
    arguments, same workspace object, same stream)."""
    from ._capi import NOT_APPLICABLE, PHASE_PREPARE, SEED_KEYS

    N = codes.shape[0] if n_rows is None else n_rows
    B, D = queries.shape
    cb = code_bytes_of(codes)
    need = ctypes.c_int64(0)
    check(lib().annlite_pq_search_workspace_bytes(N, M, Ks, cb, B, k, ctypes.byref(need)), 'pq_search_workspace_bytes')
    dev = codes.device
    ws = workspace.get(int(need.value), dev)
    op = None
    if phase == PHASE_PREPARE:
        seed_keys = torch.empty((B, SEED_KEYS), dtype=torch.int64, device=dev) if seed_keys is None else seed_keys
    else:
        op = torch.empty((B, k, 2), dtype=torch.int64, device=dev)
    rc = lib().annlite_pq_search_split(phase, int(seed_rows), lut_kind, queries.data_ptr(), B, D, codebooks.data_ptr(), codes.data_ptr(),
                                       cb, codes_layout, N, M, Ks, _ptr(valid_bits), k, row_base, None, None, _ptr(op), 0,
                                       ws.data_ptr(), ws.numel(), stream_ptr(), state.ptr, _ptr(seed_keys))
    if rc == NOT_APPLICABLE:
        return None
    check(rc, 'pq_search_split')
    return seed_keys if phase == PHASE_PREPARE else op


def pq_search_seed_union(all_keys: torch.Tensor, codes: torch.Tensor, B: int, k: int, M: int, Ks: int, workspace: ScanWorkspace,
                         n_rows: Optional[int] = None) -> None:
    """``all_keys`` i64 [G, B, SEED_KEYS] (the all-gathered seed keys of the G ranks): tighten the prepared batch's bounds to the
    k-th smallest of every query's G * k keys (``annlite_pq_search_seed_union``; between the two halves of ``pq_search_split``)."""
    N = codes.shape[0] if n_rows is None else n_rows
    cb = code_bytes_of(codes)
    need = ctypes.c_int64(0)
    check(lib().annlite_pq_search_workspace_bytes(N, M, Ks, cb, B, k, ctypes.byref(need)), 'pq_search_workspace_bytes')
    ws = workspace.get(int(need.value), codes.device)
    assert all_keys.dtype == torch.int64 and all_keys.is_contiguous() and all_keys.shape[1] == B
    check(lib().annlite_pq_search_seed_union(all_keys.data_ptr(), all_keys.shape[0], N, M, Ks, cb, B, k, ws.data_ptr(), ws.numel(),
                                             stream_ptr()), 'pq_search_seed_union')


def ivf_select_cells(kind: int, queries: torch.Tensor, centroids: torch.Tensor, n_probe: int) -> torch.Tensor:
    """The ``n_probe`` nearest cells of every query, i32 [B, P] ascending in (distance, cell)
    (``AnnLite._cell_selection``, annlite/index.py:458-466).  kind 0: squared L2, 1: negative inner product."""
    B, D = queries.shape
    C = centroids.shape[0]
    cells = torch.empty((B, n_probe), dtype=torch.int32, device=queries.device)
    check(lib().annlite_ivf_select_cells(kind, queries.data_ptr(), B, D, centroids.data_ptr(), C, n_probe,
                                         cells.data_ptr(), stream_ptr()), 'ivf_select_cells')
    return cells


def ivf_max_tiles(B: int, P: int, C: int, qt: int) -> int:
    return int(lib().annlite_ivf_max_tiles(B, P, C, qt))


def ivf_plan(cells: torch.Tensor, n_cells: int, qt: int, cell_rows: torch.Tensor, cell_order: torch.Tensor):
    """(query, cell) pairs -> query tiles of ``qt`` slots probing one cell each.  Returns
    ``(vmap i32 [T*qt], slot_of i32 [B, P], tile_rows i64 [T, 2], n_tiles_used i32 [1])``."""
    B, P = cells.shape
    T = ivf_max_tiles(B, P, n_cells, qt)
    dev = cells.device
    vmap = torch.empty((T * qt,), dtype=torch.int32, device=dev)
    slot_of = torch.empty((B, P), dtype=torch.int32, device=dev)
    tile_rows = torch.empty((T, 2), dtype=torch.int64, device=dev)
    used = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib().annlite_ivf_plan(cells.data_ptr(), B, P, n_cells, qt, cell_rows.data_ptr(), cell_order.data_ptr(), T,
                                 vmap.data_ptr(), slot_of.data_ptr(), tile_rows.data_ptr(), used.data_ptr(),
                                 stream_ptr()), 'ivf_plan')
    return vmap, slot_of, tile_rows, used


def ivf_max_tiles_first(B: int, P: int, C: int, qt: int) -> int:
    return int(lib().annlite_ivf_max_tiles_first(B, P, C, qt))


def ivf_plan_first(cells: torch.Tensor, n_cells: int, qt: int, cell_rows: torch.Tensor, cell_order: torch.Tensor, n_first: int):
    """``ivf_plan`` with the pairs of every query's ``n_first`` nearest cells in tiles of their own, which come first
    (``annlite_ivf_plan_first``; ``n_first`` 0 or >= P: one class of cells, ``ivf_plan``'s tiles)."""
    B, P = cells.shape
    T = ivf_max_tiles_first(B, P, n_cells, qt) if 0 < n_first < P else ivf_max_tiles(B, P, n_cells, qt)
    dev = cells.device
    vmap = torch.empty((T * qt,), dtype=torch.int32, device=dev)
    slot_of = torch.empty((B, P), dtype=torch.int32, device=dev)
    tile_rows = torch.empty((T, 2), dtype=torch.int64, device=dev)
    used = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib().annlite_ivf_plan_first(cells.data_ptr(), B, P, n_cells, qt, cell_rows.data_ptr(), cell_order.data_ptr(), T,
                                       vmap.data_ptr(), slot_of.data_ptr(), tile_rows.data_ptr(), used.data_ptr(), int(n_first),
                                       stream_ptr()), 'ivf_plan_first')
    return vmap, slot_of, tile_rows, used


def ivf_merge_lists(lists: torch.Tensor, slot_of: torch.Tensor, k: int, row_ids: Optional[torch.Tensor] = None,
                    id_base: int = 0, sqrt: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_ivf_merge_lists``: the per-slot lists ``lists`` i64 [V, k] of keys ``(ordered(sum) << 32) | table row``
    (ascending, all-ones = none) of every query's P slots -> ([B,k] f32, [B,k] i64) under (distance, external id)."""
    B, P = slot_of.shape
    assert lists.dtype == torch.int64 and lists.is_contiguous() and lists.shape[1] == k
    od = torch.empty((B, k), dtype=torch.float32, device=lists.device)
    oi = torch.empty((B, k), dtype=torch.int64, device=lists.device)
    check(lib().annlite_ivf_merge_lists(lists.data_ptr(), k, slot_of.data_ptr(), B, P, _ptr(row_ids), id_base, od.data_ptr(),
                                        oi.data_ptr(), 1 if sqrt else 0, stream_ptr()), 'ivf_merge_lists')
    return od, oi


def pq_search_tiles(lut_kind: int, queries: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, k: int,
                    M: int, Ks: int, tile_rows: torch.Tensor, vmap: torch.Tensor,
                    valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                    codes_layout: int = CODES_PLAIN, workspace: Optional[ScanWorkspace] = None, cand_cap: int = 256
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_pq_search_tiles``: REAL queries f32 [B, D] (their tables are built once); slot s of the V =
    ``vmap.numel()`` slots scans rows ``tile_rows[s // qt]`` with the tables of query ``vmap[s]``, integer sums only.
    Returns the per-slot candidate lists ``(cand i32 [V, cand_cap] table rows, count i32 [V])`` (count -1: overflow,
    re-score the whole cell)."""
    N = codes.shape[0] if n_rows is None else n_rows
    B, D = queries.shape
    V = vmap.numel()
    cb = code_bytes_of(codes)
    need = ctypes.c_int64(0)
    check(lib().annlite_pq_search_tiles_workspace_bytes(N, M, Ks, cb, V, k, ctypes.byref(need)),
          'pq_search_tiles_workspace_bytes')
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(need.value), dev)
    cand = torch.empty((V, cand_cap), dtype=torch.int32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    check(lib().annlite_pq_search_tiles(lut_kind, queries.data_ptr(), B, D, codebooks.data_ptr(), codes.data_ptr(),
                                        cb, codes_layout, N, M, Ks, _ptr(valid_bits), k, V, tile_rows.data_ptr(),
                                        vmap.data_ptr(), cand.data_ptr(), cand_cap, count.data_ptr(), ws.data_ptr(),
                                        ws.numel(), stream_ptr()), 'pq_search_tiles')
    return cand, count


def ivf_rescore(lut_bmk: torch.Tensor, codes_plain: torch.Tensor, cand: torch.Tensor, count: torch.Tensor,
                slot_of: torch.Tensor, tile_rows: torch.Tensor, qt: int, k: int, row_ids: Optional[torch.Tensor] = None,
                valid_bits: Optional[torch.Tensor] = None, id_base: int = 0, sqrt: bool = False
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact distances of every query's candidate rows + top-k: ``lut_bmk`` f32 [B, M, Ks] (``get_dist_mat``),
    ``codes_plain`` u8 [N, M] (cell-sorted, PLAIN).  Returns ([B,k] f32, [B,k] i64 ids)."""
    B, M, Ks = lut_bmk.shape
    P = slot_of.shape[1]
    od = torch.empty((B, k), dtype=torch.float32, device=lut_bmk.device)
    oi = torch.empty((B, k), dtype=torch.int64, device=lut_bmk.device)
    check(lib().annlite_ivf_rescore(lut_bmk.data_ptr(), B, M, Ks, codes_plain.data_ptr(), codes_plain.shape[0],
                                    _ptr(valid_bits), cand.data_ptr(), cand.shape[1], count.data_ptr(), slot_of.data_ptr(),
                                    P, tile_rows.data_ptr(), qt, _ptr(row_ids), id_base, k, od.data_ptr(), oi.data_ptr(),
                                    1 if sqrt else 0, stream_ptr()), 'ivf_rescore')
    return od, oi


def ivf_candidate_ids(cand: torch.Tensor, count: torch.Tensor, slot_of: torch.Tensor, R: int,
                      row_ids: Optional[torch.Tensor] = None, id_base: int = 0) -> torch.Tensor:
    """Every query's candidate lists as one dense i64 row [B, R] of external ids, padded with -1."""
    B, P = slot_of.shape
    out = torch.empty((B, R), dtype=torch.int64, device=cand.device)
    check(lib().annlite_ivf_candidate_ids(cand.data_ptr(), cand.shape[1], count.data_ptr(), slot_of.data_ptr(), B, P,
                                          _ptr(row_ids), id_base, out.data_ptr(), R, stream_ptr()), 'ivf_candidate_ids')
    return out


def ivf_search_topk(lut_kind: int, queries: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, cells: torch.Tensor, n_cells: int,
                    cell_rows: torch.Tensor, cell_order: torch.Tensor, k: int, M: int, Ks: int,
                    row_ids: Optional[torch.Tensor] = None, valid_bits: Optional[torch.Tensor] = None,
                    n_rows: Optional[int] = None, codes_layout: int = CODES_PLAIN, id_base: int = 0, sqrt: bool = False,
                    workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_ivf_search_topk``: the pruned search over cells on the byte-table kernel in one call -- plan, preparation
    launch (tables, per-cell seed bounds, per-query byte tables), scan in cell tiles with exact sums, merge of the per-cell
    lists.  ``queries`` f32 [B, D] (the tables of ``lut_kind`` -- LUT_L2 or LUT_IPDIST -- are built from them and ``codebooks`` [M, Ks, D/M]), ``codes`` the
    CELL-SORTED table, ``cells`` i32 [B, P] nearest first.  M = 16, Ks <= 256, k <= 16.  Returns ([B,k] f32, [B,k] i64)."""
    N = codes.shape[0] if n_rows is None else n_rows
    B, D = queries.shape
    P = cells.shape[1]
    need = ctypes.c_int64(0)
    check(lib().annlite_ivf_search_topk_workspace_bytes(B, P, n_cells, M, Ks, k, ctypes.byref(need)), 'ivf_search_topk_workspace_bytes')
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(need.value), dev)
    od = torch.empty((B, k), dtype=torch.float32, device=dev)
    oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    check(lib().annlite_ivf_search_topk(lut_kind, queries.data_ptr(), B, D, codebooks.data_ptr(), M, Ks, codes.data_ptr(), codes_layout, N,
                                        _ptr(valid_bits), cells.data_ptr(), P, n_cells, cell_rows.data_ptr(), cell_order.data_ptr(),
                                        _ptr(row_ids), id_base, k, od.data_ptr(), oi.data_ptr(), 1 if sqrt else 0, ws.data_ptr(),
                                        ws.numel(), stream_ptr()), 'ivf_search_topk')
    return od, oi


def ivf_search_candidates(lut_kind: int, queries: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, cells: torch.Tensor,
                          n_cells: int, cell_rows: torch.Tensor, cell_order: torch.Tensor, k: int, M: int, Ks: int,
                          row_ids: Optional[torch.Tensor] = None, valid_bits: Optional[torch.Tensor] = None,
                          n_rows: Optional[int] = None, codes_layout: int = CODES_PLAIN, id_base: int = 0,
                          workspace: Optional[ScanWorkspace] = None, bound_rank: int = 1,
                          seed_cells: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``annlite_ivf_search_candidates``: the pruned search's pipeline as the candidate generator of an exact re-rank -- every
    (query, probed cell) list on its own (the cell's best <= k rows at or below the query's first bound, the
    ``min(bound_rank * k, 64)``-th smallest seed sum of its nearest cell -- of entry ``seed_cells[b]`` (i32 [B]) of the cell table when given).
    Returns i64 [B, P * k] external ids, -1 = none."""
    N = codes.shape[0] if n_rows is None else n_rows
    B, D = queries.shape
    P = cells.shape[1]
    need = ctypes.c_int64(0)
    check(lib().annlite_ivf_search_topk_workspace_bytes(B, P, n_cells, M, Ks, k, ctypes.byref(need)), 'ivf_search_topk_workspace_bytes')
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(need.value), dev)
    out = torch.empty((B, P * k), dtype=torch.int64, device=dev)
    check(lib().annlite_ivf_search_candidates(lut_kind, queries.data_ptr(), B, D, codebooks.data_ptr(), M, Ks, codes.data_ptr(), codes_layout,
                                              N, _ptr(valid_bits), cells.data_ptr(), P, n_cells, cell_rows.data_ptr(), cell_order.data_ptr(),
                                              _ptr(row_ids), id_base, k, bound_rank, _ptr(seed_cells), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              stream_ptr()),
          'ivf_search_candidates')
    return out


def topk_merge_packed(packed: torch.Tensor, sqrt: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """[G,B,k,2] i64 (id, distance bits) -> ([B,k] f32, [B,k] i64), same order rule as ``topk_merge``."""
    G, B, k, _ = packed.shape
    od = torch.empty((B, k), dtype=torch.float32, device=packed.device)
    oi = torch.empty((B, k), dtype=torch.int64, device=packed.device)
    check(lib().annlite_topk_merge_packed(packed.contiguous().data_ptr(), G, B, k, od.data_ptr(), oi.data_ptr(),
                                          1 if sqrt else 0, stream_ptr()), 'topk_merge_packed')
    return od, oi


def adc_scan_candidates(codes: torch.Tensor, lut: torch.Tensor, B: int, k: int, M: int, Ks: int,
                        valid_bits: Optional[torch.Tensor] = None, row_base: int = 0, n_rows: Optional[int] = None,
                        codes_layout: int = CODES_PLAIN, workspace: Optional[ScanWorkspace] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Unmerged per-slice top-k lists: (f32 [B, n_slices*k], i64 [B, n_slices*k]); superset of the top-k."""
    N = codes.shape[0] if n_rows is None else n_rows
    cb = code_bytes_of(codes)
    plan = scan_plan(N, M, Ks, cb, B, k)
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(plan.workspace_bytes), dev)
    R = plan.n_slices * k
    od = torch.empty((B, R), dtype=torch.float32, device=dev)
    oi = torch.empty((B, R), dtype=torch.int64, device=dev)
    check(lib().annlite_adc_scan_candidates(codes.data_ptr(), cb, codes_layout, N, M, Ks, _ptr(valid_bits),
                                            lut.data_ptr(), B, k, row_base, od.data_ptr(), oi.data_ptr(),
                                            ws.data_ptr(), ws.numel(), stream_ptr()), 'adc_scan_candidates')
    return od, oi


def pq_search_candidates(lut_kind: int, queries: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, k: int, M: int, Ks: int,
                         valid_bits: Optional[torch.Tensor] = None, row_base: int = 0, n_rows: Optional[int] = None,
                         codes_layout: int = CODES_PLAIN, workspace: Optional[ScanWorkspace] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_pq_search_candidates``: table build + candidate generator in one C call -- (f32 [B, n_slices*k], i64 [B, n_slices*k]),
    every slice's k best rows at or below the table-wide first bound (a superset of the table's top-k; -1 / +inf padded)."""
    N = codes.shape[0] if n_rows is None else n_rows
    B, D = queries.shape
    cb = code_bytes_of(codes)
    plan = scan_plan(N, M, Ks, cb, B, k)
    need = ctypes.c_int64(0)
    check(lib().annlite_pq_search_workspace_bytes(N, M, Ks, cb, B, k, ctypes.byref(need)), 'pq_search_workspace_bytes')
    dev = codes.device
    ws = (workspace or ScanWorkspace()).get(int(need.value), dev)
    R = plan.n_slices * k
    od = torch.empty((B, R), dtype=torch.float32, device=dev)
    oi = torch.empty((B, R), dtype=torch.int64, device=dev)
    check(lib().annlite_pq_search_candidates(lut_kind, queries.data_ptr(), B, D, codebooks.data_ptr(), codes.data_ptr(), cb, codes_layout,
                                             N, M, Ks, _ptr(valid_bits), k, row_base, od.data_ptr(), oi.data_ptr(), ws.data_ptr(),
                                             ws.numel(), stream_ptr()), 'pq_search_candidates')
    return od, oi


def topk_merge(dist: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[G,B,k] x2 -> [B,k] x2 (the merge after the RCCL all-gather of per-shard top-k)."""
    G, B, k = dist.shape
    od = torch.empty((B, k), dtype=torch.float32, device=dist.device)
    oi = torch.empty((B, k), dtype=torch.int64, device=dist.device)
    check(lib().annlite_topk_merge(dist.data_ptr(), ids.data_ptr(), G, B, k, od.data_ptr(), oi.data_ptr(),
                                   stream_ptr()), 'topk_merge')
    return od, oi


def topk_rows(values: torch.Tensor, k: int, id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    B, N = values.shape
    od = torch.empty((B, k), dtype=torch.float32, device=values.device)
    oi = torch.empty((B, k), dtype=torch.int64, device=values.device)
    check(lib().annlite_topk_rows(values.data_ptr(), B, N, k, id_base, od.data_ptr(), oi.data_ptr(), stream_ptr()),
          'topk_rows')
    return od, oi


def codes_skew(codes: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0,
               out: Optional[torch.Tensor] = None, inverse: bool = False) -> torch.Tensor:
    """PLAIN rows -> SKEWED table rows (scatter by ids) or back (inverse gather)."""
    assert codes.dtype == torch.uint8
    if inverse:
        n = ids.shape[0] if ids is not None else codes.shape[0]
        M = codes.shape[1]
        out = torch.empty((n, M), dtype=torch.uint8, device=codes.device) if out is None else out
    else:
        n, M = codes.shape
        out = torch.empty_like(codes) if out is None else out
    check(lib().annlite_codes_skew(codes.data_ptr(), n, M, _ptr(ids), id_base, out.data_ptr(), int(inverse),
                                   stream_ptr()), 'codes_skew')
    return out


# -------------------------------------------------------------------------------------------- codec
def pq_encode(x: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    N, D = x.shape
    M, Ks, dsub = codebooks.shape
    assert D == M * dsub, 'input dimension must be Ds * M'
    cb = 1 if Ks <= 256 else (2 if Ks <= 65536 else 4)
    out = torch.empty((N, M), dtype=_CODE_TORCH[cb], device=x.device)
    check(lib().annlite_pq_encode(x.data_ptr(), N, D, codebooks.data_ptr(), M, Ks, out.data_ptr(), cb, stream_ptr()),
          'pq_encode')
    return out


def pq_decode(codes: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    N, M = codes.shape
    Mc, Ks, dsub = codebooks.shape
    assert M == Mc
    out = torch.empty((N, M * dsub), dtype=torch.float32, device=codes.device)
    check(lib().annlite_pq_decode(codes.data_ptr(), code_bytes_of(codes), N, M, Ks, codebooks.data_ptr(), dsub,
                                  out.data_ptr(), stream_ptr()), 'pq_decode')
    return out


def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    N, D = x.shape
    out = torch.empty_like(x)
    check(lib().annlite_l2_normalize(x.data_ptr(), N, D, out.data_ptr(), stream_ptr()), 'l2_normalize')
    return out


def kmeans_assign_accumulate(x, codebooks, sums, counts, inertia=None):
    N, D = x.shape
    M, Ks, dsub = codebooks.shape
    check(lib().annlite_kmeans_assign_accumulate(x.data_ptr(), N, D, codebooks.data_ptr(), M, Ks, sums.data_ptr(),
                                                 counts.data_ptr(), _ptr(inertia), stream_ptr()),
          'kmeans_assign_accumulate')


def kmeans_update(sums, counts, codebooks):
    M, Ks, dsub = codebooks.shape
    check(lib().annlite_kmeans_update(sums.data_ptr(), counts.data_ptr(), M, Ks, dsub, codebooks.data_ptr(),
                                      stream_ptr()), 'kmeans_update')


def exact_gather_dist(metric: int, queries: torch.Tensor, vectors: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    B, D = queries.shape
    N = vectors.shape[0]
    R = cand.shape[1]
    out = torch.empty((B, R), dtype=torch.float32, device=queries.device)
    check(lib().annlite_exact_gather_dist(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), N,
                                          cand.data_ptr(), R, out.data_ptr(), stream_ptr()), 'exact_gather_dist')
    return out


def rerank_topk(metric: int, queries: torch.Tensor, vectors: torch.Tensor, cand: torch.Tensor, k: int,
                valid_bits: Optional[torch.Tensor] = None, sqrt: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_rerank_topk``: exact distances of the candidate lists ``cand`` i64 [B, R] fused with the top-k (k <= 64):
    ``(dist f32 [B, k], ids i64 [B, k])`` in (distance, list position) order, (+inf, -1) padded."""
    B, D = queries.shape
    R = cand.shape[1]
    out_d = torch.empty((B, k), dtype=torch.float32, device=queries.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=queries.device)
    check(lib().annlite_rerank_topk(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), vectors.shape[0], cand.data_ptr(), R,
                                    _ptr(valid_bits), int(k), 1 if sqrt else 0, out_d.data_ptr(), out_i.data_ptr(),
                                    stream_ptr()), 'rerank_topk')
    return out_d, out_i


# ---------------------------------------------------------------------------------------------- exact float32 search
def flat_row_norms(vectors: torch.Tensor, ids: Optional[torch.Tensor] = None, n: Optional[int] = None, id_base: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``annlite_flat_row_norms``: ``out[row] = |vectors[row]|^2`` for the rows ``ids`` (i64) or ``id_base .. id_base + n``."""
    cap, D = vectors.shape
    if out is None:
        out = torch.zeros((cap,), dtype=torch.float32, device=vectors.device)
    cnt = ids.numel() if ids is not None else (cap - id_base if n is None else n)
    check(lib().annlite_flat_row_norms(vectors.data_ptr(), cap, D, _ptr(ids), cnt, id_base, out.data_ptr(), stream_ptr()), 'flat_row_norms')
    return out


def flat_list_capacity() -> int:
    return int(lib().annlite_flat_list_capacity())


def _flat_slack(entry: str, metric: int, dim: int) -> Tuple[np.float32, np.float32]:
    """the ``(c_rel, c_abs)`` pair of the C entry ``annlite_<entry>``"""
    c_rel, c_abs = ctypes.c_float(0), ctypes.c_float(0)
    check(getattr(lib(), 'annlite_' + entry)(int(metric), int(dim), ctypes.byref(c_rel), ctypes.byref(c_abs)), entry)
    return np.float32(c_rel.value), np.float32(c_abs.value)


def _flat_workspace(entry: str, shape: Tuple[int, ...], dev, workspace: Optional[ScanWorkspace]) -> torch.Tensor:
    """this stream's buffer of ``workspace`` (of a throw-away one without), sized by the C entry ``annlite_<entry>(*shape, &bytes)``"""
    need = ctypes.c_int64(0)
    check(getattr(lib(), 'annlite_' + entry)(*shape, ctypes.byref(need)), entry)
    return (workspace or ScanWorkspace()).get(int(need.value), dev)


def _flat_topk_outputs(B: int, k: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    return torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev)


def _flat_lists(B: int, dev, score_cols: Optional[int] = None):
    """``(cand i32 [B, cap], count i32 [B] of zeros, scores)`` -- scores f32 [B, score_cols] of NaN, or None without ``score_cols``"""
    cand = torch.empty((B, flat_list_capacity()), dtype=torch.int32, device=dev)
    count = torch.zeros((B,), dtype=torch.int32, device=dev)
    sc = None if score_cols is None else torch.full((B, score_cols), float('nan'), dtype=torch.float32, device=dev)
    return cand, count, sc


def _flat_filter_stage(entry: str, ws_entry: str, metric: int, queries, vectors, norms, bounds, valid_bits, n_rows, stride: int, scores: bool,
                       workspace, n_query_outputs: int, after_vectors=(), after_count=()):
    """One filter stage over the table through ``annlite_<entry>``: ``(cand, count, *per-query f32 [B] outputs[, scores])``.  The
    entries differ in what follows the vectors (int8: the scale), in how many per-query outputs they have and in what follows the
    count (split: the centre)."""
    B, D = queries.shape
    N = vectors.shape[0] if n_rows is None else n_rows
    dev = queries.device
    ws = _flat_workspace(ws_entry, (N, D, B, 1), dev, workspace)
    cand, count, sc = _flat_lists(B, dev, (N + stride - 1) // stride if scores else None)
    outs = [torch.empty((B,), dtype=torch.float32, device=dev) for _ in range(n_query_outputs)]
    check(getattr(lib(), 'annlite_' + entry)(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), *after_vectors, norms.data_ptr(), N, stride,
                                             _ptr(valid_bits), *[o.data_ptr() for o in outs], bounds.data_ptr(), cand.data_ptr(),
                                             count.data_ptr(), *after_count, _ptr(sc), ws.data_ptr(), ws.numel(), stream_ptr()), entry)
    return (cand, count, *outs, sc) if scores else (cand, count, *outs)


def _flat_search(entry: str, ws_entry: str, metric: int, queries, vectors, norms, k: int, valid_bits, n_rows, sqrt: bool, workspace,
                 after_vectors=(), after_valid=()) -> Tuple[torch.Tensor, torch.Tensor]:
    """A search over the table through ``annlite_<entry>``; the entries differ in what follows the vectors (int8: the scale) and the
    bitmap (split: the centre)."""
    B, D = queries.shape
    N = vectors.shape[0] if n_rows is None else n_rows
    dev = queries.device
    ws = _flat_workspace(ws_entry, (N, D, B, k), dev, workspace)
    od, oi = _flat_topk_outputs(B, k, dev)
    check(getattr(lib(), 'annlite_' + entry)(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), *after_vectors, norms.data_ptr(), N,
                                             _ptr(valid_bits), *after_valid, int(k), 1 if sqrt else 0, od.data_ptr(), oi.data_ptr(),
                                             ws.data_ptr(), ws.numel(), stream_ptr()), entry)
    return od, oi


def flat_slack(metric: int, dim: int) -> Tuple[np.float32, np.float32]:
    """``annlite_flat_slack``: the ``(c_rel, c_abs)`` the filter kernel is launched with (host only, needs no GPU)."""
    return _flat_slack('flat_slack', metric, dim)


def flat_filter(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, bounds: torch.Tensor,
                valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, stride: int = 1,
                query_norms: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_flat_filter``: ``(cand i32 [B, cap], count i32 [B])`` -- the rows (in no particular order) that may lie within
    ``bounds`` f32 [B] of each query; ``count > cap`` marks an overflowed list."""
    B, D = queries.shape
    N = vectors.shape[0] if n_rows is None else n_rows
    if query_norms is None:
        query_norms = flat_row_norms(queries)
    cand, count, _ = _flat_lists(B, queries.device)
    check(lib().annlite_flat_filter(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), norms.data_ptr(), N, stride, _ptr(valid_bits),
                                    query_norms.data_ptr(), bounds.data_ptr(), cand.data_ptr(), count.data_ptr(), stream_ptr()), 'flat_filter')
    return cand, count


def flat_search_topk(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, k: int,
                     valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, sqrt: bool = False,
                     workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_flat_search_topk``: exact k nearest rows (k <= 64), ``(dist f32 [B, k], ids i64 [B, k])`` ascending by
    (distance, id), (+inf, -1) padded.  ``flat_overflow_count(workspace)`` reads the call's overflow counter afterwards."""
    return _flat_search('flat_search_topk', 'flat_search_workspace_bytes', metric, queries, vectors, norms, k, valid_bits, n_rows, sqrt, workspace)


def flat_overflow_count(workspace: ScanWorkspace) -> int:
    """Queries of the last ``flat_search_topk`` on this stream's workspace buffer that took the all-rows route."""
    buf = workspace.bufs.get(stream_ptr())
    if buf is None:
        return 0
    n = ctypes.c_int64(0)
    check(lib().annlite_flat_overflow_count(buf.data_ptr(), stream_ptr(), ctypes.byref(n)), 'flat_overflow_count')
    return int(n.value)


def flat_list_counts(workspace: ScanWorkspace, B: int) -> torch.Tensor:
    """``annlite_flat_list_counts``: i32 [B], the rows the last filter stage of the last ``flat_search_topk`` /
    ``ivf_flat_search_topk`` of ``B`` queries on this stream's workspace buffer offered each list (measurement scripts)."""
    buf = workspace.bufs[stream_ptr()]
    out = torch.empty((B,), dtype=torch.int32, device=buf.device)
    check(lib().annlite_flat_list_counts(buf.data_ptr(), B, out.data_ptr(), stream_ptr()), 'flat_list_counts')
    return out


def flat_split_slack(metric: int, dim: int) -> Tuple[np.float32, np.float32]:
    """``annlite_flat_split_slack``: the ``(c_rel, c_abs)`` the split filter kernel is launched with (host only, needs no GPU)."""
    return _flat_slack('flat_split_slack', metric, dim)


def flat_centred_norms(vectors: torch.Tensor, centre: torch.Tensor, ids: Optional[torch.Tensor] = None, n: Optional[int] = None,
                       id_base: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``annlite_flat_centred_norms``: ``out[row] = |fl(vectors[row] - centre)|^2`` for the rows ``ids`` (i64) or
    ``id_base .. id_base + n``."""
    cap, D = vectors.shape
    assert centre.dtype == torch.float32 and centre.numel() == D and centre.is_contiguous()
    if out is None:
        out = torch.zeros((cap,), dtype=torch.float32, device=vectors.device)
    cnt = ids.numel() if ids is not None else (cap - id_base if n is None else n)
    check(lib().annlite_flat_centred_norms(vectors.data_ptr(), cap, D, _ptr(ids), cnt, id_base, centre.data_ptr(), out.data_ptr(),
                                           stream_ptr()), 'flat_centred_norms')
    return out


def flat_filter_split(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, bounds: torch.Tensor,
                      centre: Optional[torch.Tensor] = None, valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                      stride: int = 1, scores: bool = False, workspace: Optional[ScanWorkspace] = None):
    """``annlite_flat_filter_split``: ``flat_filter`` with the split-bf16 filter over ``fl(x - centre)``; ``norms`` are
    ``flat_centred_norms`` with the same centre (``flat_row_norms`` without one).  ``(cand i32 [B, cap], count i32 [B],
    query_norms f32 [B])`` -- the last as the filter used them -- and, with ``scores=True``, the filter's score of every
    (query, stage row) pair, f32 [B, ceil(N / stride)]."""
    return _flat_filter_stage('flat_filter_split', 'flat_search_split_workspace_bytes', metric, queries, vectors, norms, bounds, valid_bits,
                              n_rows, stride, scores, workspace, 1, after_count=(_ptr(centre),))


def flat_search_topk_split(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, k: int,
                           centre: Optional[torch.Tensor] = None, valid_bits: Optional[torch.Tensor] = None,
                           n_rows: Optional[int] = None, sqrt: bool = False,
                           workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_flat_search_topk_split``: ``flat_search_topk`` with the split-bf16 filter (``norms``: see ``flat_filter_split``);
    the same answer, bit for bit.  ``flat_overflow_count`` / ``flat_list_counts`` read this workspace too."""
    return _flat_search('flat_search_topk_split', 'flat_search_split_workspace_bytes', metric, queries, vectors, norms, k, valid_bits, n_rows,
                        sqrt, workspace, after_valid=(_ptr(centre),))


# ---------------------------------------------------------------------------------------------- exact search over f16 rows
def exact_gather_dist_f16(metric: int, queries: torch.Tensor, vectors: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """``annlite_exact_gather_dist_f16``: ``exact_gather_dist`` over ``vectors`` f16 [N, D], the bits of the widened rows."""
    assert vectors.dtype == torch.float16
    B, D = queries.shape
    N = vectors.shape[0]
    R = cand.shape[1]
    out = torch.empty((B, R), dtype=torch.float32, device=queries.device)
    check(lib().annlite_exact_gather_dist_f16(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), N,
                                              cand.data_ptr(), R, out.data_ptr(), stream_ptr()), 'exact_gather_dist_f16')
    return out


def flat_row_norms_f16(vectors: torch.Tensor, ids: Optional[torch.Tensor] = None, n: Optional[int] = None, id_base: int = 0,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``annlite_flat_row_norms_f16``: ``flat_row_norms`` over ``vectors`` f16 [capacity, D]."""
    assert vectors.dtype == torch.float16
    cap, D = vectors.shape
    if out is None:
        out = torch.zeros((cap,), dtype=torch.float32, device=vectors.device)
    cnt = ids.numel() if ids is not None else (cap - id_base if n is None else n)
    check(lib().annlite_flat_row_norms_f16(vectors.data_ptr(), cap, D, _ptr(ids), cnt, id_base, out.data_ptr(), stream_ptr()),
          'flat_row_norms_f16')
    return out


def flat_f16_slack(metric: int, dim: int) -> Tuple[np.float32, np.float32]:
    """``annlite_flat_f16_slack``: the ``(c_rel, c_abs)`` the f16 filter kernel is launched with (host only, needs no GPU)."""
    return _flat_slack('flat_f16_slack', metric, dim)


def flat_filter_f16(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, bounds: torch.Tensor,
                    valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, stride: int = 1, scores: bool = False,
                    workspace: Optional[ScanWorkspace] = None):
    """``annlite_flat_filter_f16``: ``flat_filter`` over ``vectors`` f16 [N, D]; ``norms`` are ``flat_row_norms_f16``.
    ``(cand i32 [B, cap], count i32 [B], query_norms f32 [B], query_flush f32 [B])`` -- the last two as the filter used them:
    ``|q|^2`` and the per-query term of the slack -- and, with ``scores=True``, the filter's score of every (query, stage row)
    pair, f32 [B, ceil(N / stride)]."""
    assert vectors.dtype == torch.float16
    return _flat_filter_stage('flat_filter_f16', 'flat_search_f16_workspace_bytes', metric, queries, vectors, norms, bounds, valid_bits, n_rows,
                              stride, scores, workspace, 2)


def flat_search_topk_f16(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, k: int,
                         valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, sqrt: bool = False,
                         workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_flat_search_topk_f16``: ``flat_search_topk`` over ``vectors`` f16 [N, D] (``norms``: ``flat_row_norms_f16``): the
    answer of ``flat_search_topk`` over the widened rows, bit for bit.  ``flat_overflow_count`` / ``flat_list_counts`` read this
    workspace too."""
    assert vectors.dtype == torch.float16
    return _flat_search('flat_search_topk_f16', 'flat_search_f16_workspace_bytes', metric, queries, vectors, norms, k, valid_bits, n_rows, sqrt,
                        workspace)


# ---------------------------------------------------------------------------------------------- exact search over int8 rows
def exact_gather_dist_i8(metric: int, queries: torch.Tensor, vectors: torch.Tensor, cand: torch.Tensor, scale: float) -> torch.Tensor:
    """``annlite_exact_gather_dist_i8``: ``exact_gather_dist`` over ``vectors`` int8 [N, D], the bits of the rows ``scale * c``."""
    assert vectors.dtype == torch.int8
    B, D = queries.shape
    N = vectors.shape[0]
    R = cand.shape[1]
    out = torch.empty((B, R), dtype=torch.float32, device=queries.device)
    check(lib().annlite_exact_gather_dist_i8(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), float(scale), N,
                                             cand.data_ptr(), R, out.data_ptr(), stream_ptr()), 'exact_gather_dist_i8')
    return out


def flat_row_norms_i8(vectors: torch.Tensor, scale: float, ids: Optional[torch.Tensor] = None, n: Optional[int] = None,
                      id_base: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``annlite_flat_row_norms_i8``: ``flat_row_norms`` over ``vectors`` int8 [capacity, D] read as ``scale * c``."""
    assert vectors.dtype == torch.int8
    cap, D = vectors.shape
    if out is None:
        out = torch.zeros((cap,), dtype=torch.float32, device=vectors.device)
    cnt = ids.numel() if ids is not None else (cap - id_base if n is None else n)
    check(lib().annlite_flat_row_norms_i8(vectors.data_ptr(), float(scale), cap, D, _ptr(ids), cnt, id_base, out.data_ptr(), stream_ptr()),
          'flat_row_norms_i8')
    return out


def flat_i8_slack(metric: int, dim: int) -> Tuple[np.float32, np.float32]:
    """``annlite_flat_i8_slack``: the ``(c_rel, c_abs)`` the int8 filter kernel is launched with (host only, needs no GPU)."""
    return _flat_slack('flat_i8_slack', metric, dim)


def flat_filter_i8(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, bounds: torch.Tensor, scale: float,
                   valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, stride: int = 1, scores: bool = False,
                   workspace: Optional[ScanWorkspace] = None):
    """``annlite_flat_filter_i8``: ``flat_filter`` over ``vectors`` int8 [N, D] read as ``scale * c``; ``norms`` are
    ``flat_row_norms_i8`` with the same scale.  ``(cand i32 [B, cap], count i32 [B], query_norms f32 [B], query_slack f32 [B])`` --
    the last two as the filter used them: ``|q|^2`` and the per-query term of the slack -- and, with ``scores=True``, the filter's
    score of every (query, stage row) pair, f32 [B, ceil(N / stride)]."""
    assert vectors.dtype == torch.int8
    return _flat_filter_stage('flat_filter_i8', 'flat_search_i8_workspace_bytes', metric, queries, vectors, norms, bounds, valid_bits, n_rows,
                              stride, scores, workspace, 2, after_vectors=(float(scale),))


def flat_search_topk_i8(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, k: int, scale: float,
                        valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, sqrt: bool = False,
                        workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_flat_search_topk_i8``: ``flat_search_topk`` over ``vectors`` int8 [N, D] read as ``scale * c`` (``norms``:
    ``flat_row_norms_i8``): the answer of ``flat_search_topk`` over those f32 rows, bit for bit.  ``flat_overflow_count`` /
    ``flat_list_counts`` read this workspace too."""
    assert vectors.dtype == torch.int8
    return _flat_search('flat_search_topk_i8', 'flat_search_i8_workspace_bytes', metric, queries, vectors, norms, k, valid_bits, n_rows, sqrt,
                        workspace, after_vectors=(float(scale),))


# ---------------------------------------------------------------------------------------------- cells over float vectors
def ivf_flat_stages(max_probed_rows: int) -> List[int]:
    """``annlite_ivf_flat_stages``: the strides ``ivf_flat_search_topk`` uses for queries that probe at most ``max_probed_rows``
    rows -- the first exact sample's, then the filter stages' down to 1; empty: exact sums over all probed rows (host only,
    needs no GPU)."""
    strides, n = (ctypes.c_int64 * 16)(), ctypes.c_int(0)
    check(lib().annlite_ivf_flat_stages(int(max_probed_rows), strides, ctypes.byref(n)), 'ivf_flat_stages')
    return [int(strides[i]) for i in range(n.value)]


def ivf_flat_search_topk(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, cells: torch.Tensor,
                         n_cells: int, perm: torch.Tensor, cell_rows: torch.Tensor, cell_order: torch.Tensor, max_cell_rows: int,
                         max_probed_rows: int, k: int, valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                         sqrt: bool = False, workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_ivf_flat_search_topk``: exact k nearest (k <= 64) among the rows of each query's probed ``cells`` i32 [B, P] --
    ``perm`` i32 = the live offsets grouped by cell, ``cell_rows`` i64 [C, 2] their ranges, ``cell_order`` i32 [C] cells by
    descending size.  ``(dist f32 [B, k], ids i64 [B, k])`` ascending by (distance, id), (+inf, -1) padded;
    ``flat_overflow_count(workspace)`` reads the call's overflow counter afterwards."""
    B, D = queries.shape
    P = cells.shape[1]
    N = vectors.shape[0] if n_rows is None else n_rows
    dev = queries.device
    ws = _flat_workspace('ivf_flat_search_workspace_bytes', (B, P, n_cells, k), dev, workspace)
    od, oi = _flat_topk_outputs(B, k, dev)
    check(lib().annlite_ivf_flat_search_topk(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), norms.data_ptr(), N, _ptr(valid_bits),
                                             cells.data_ptr(), P, int(n_cells), perm.data_ptr(), perm.numel(), cell_rows.data_ptr(),
                                             cell_order.data_ptr(), int(max_cell_rows), int(max_probed_rows), int(k), 1 if sqrt else 0,
                                             od.data_ptr(), oi.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), 'ivf_flat_search_topk')
    return od, oi


def ivf_flat_centred_norms(vectors: torch.Tensor, centres: torch.Tensor, cell_of: torch.Tensor, ids: Optional[torch.Tensor] = None,
                           n: Optional[int] = None, id_base: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``annlite_ivf_flat_centred_norms``: ``out[row] = |fl(vectors[row] - centres[cell_of[row]])|^2`` for the rows ``ids`` (i64) or
    ``id_base .. id_base + n``: ``flat_centred_norms`` with the centre chosen per row (``centres`` f32 [C, D], ``cell_of`` i32
    [capacity])."""
    cap, D = vectors.shape
    assert centres.dtype == torch.float32 and centres.ndim == 2 and centres.shape[1] == D and centres.is_contiguous()
    assert cell_of.dtype == torch.int32 and cell_of.numel() >= cap and cell_of.is_contiguous()
    if out is None:
        out = torch.zeros((cap,), dtype=torch.float32, device=vectors.device)
    cnt = ids.numel() if ids is not None else (cap - id_base if n is None else n)
    check(lib().annlite_ivf_flat_centred_norms(vectors.data_ptr(), cap, D, _ptr(ids), cnt, id_base, centres.data_ptr(), centres.shape[0],
                                               cell_of.data_ptr(), out.data_ptr(), stream_ptr()), 'ivf_flat_centred_norms')
    return out


def ivf_flat_filter_split(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, bounds: torch.Tensor,
                          cells: torch.Tensor, n_cells: int, perm: torch.Tensor, cell_rows: torch.Tensor, cell_order: torch.Tensor,
                          max_cell_rows: int, centres: Optional[torch.Tensor] = None, cell_of: Optional[torch.Tensor] = None,
                          valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, stride: int = 1, scores: bool = False,
                          workspace: Optional[ScanWorkspace] = None):
    """``annlite_ivf_flat_filter_split``: the split-bf16 filter stage over the (cell, queries) tiles alone -- ``flat_filter_split`` of the
    cells.  ``norms`` are ``ivf_flat_centred_norms`` with the same ``centres`` (``flat_row_norms`` without).  ``(cand i32 [B, cap],
    count i32 [B], pair_norms f32 [B, P])`` -- the last as the filter used them -- and, with ``scores=True``, the filter's score by
    (query, row offset), f32 [B, N]: NaN where the filter evaluated nothing (cell not probed, row not valid)."""
    B, D = queries.shape
    P = cells.shape[1]
    N = vectors.shape[0] if n_rows is None else n_rows
    dev = queries.device
    ws = _flat_workspace('ivf_flat_search_split_workspace_bytes', (B, P, n_cells, D, 1), dev, workspace)
    cand, count, sc = _flat_lists(B, dev, N if scores else None)
    pn = torch.empty((B, P), dtype=torch.float32, device=dev)
    check(lib().annlite_ivf_flat_filter_split(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), norms.data_ptr(), N, _ptr(valid_bits),
                                              cells.data_ptr(), P, int(n_cells), perm.data_ptr(), perm.numel(), cell_rows.data_ptr(),
                                              cell_order.data_ptr(), int(max_cell_rows), int(stride), _ptr(centres), _ptr(cell_of),
                                              bounds.data_ptr(), cand.data_ptr(), count.data_ptr(), pn.data_ptr(), _ptr(sc),
                                              ws.data_ptr(), ws.numel(), stream_ptr()), 'ivf_flat_filter_split')
    return (cand, count, pn, sc) if scores else (cand, count, pn)


def ivf_flat_search_topk_split(metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, cells: torch.Tensor,
                               n_cells: int, perm: torch.Tensor, cell_rows: torch.Tensor, cell_order: torch.Tensor, max_cell_rows: int,
                               max_probed_rows: int, k: int, centres: Optional[torch.Tensor] = None,
                               cell_of: Optional[torch.Tensor] = None, valid_bits: Optional[torch.Tensor] = None,
                               n_rows: Optional[int] = None, sqrt: bool = False,
                               workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_ivf_flat_search_topk_split``: ``ivf_flat_search_topk`` with the split-bf16 filter over the cell tiles, every tile
    centred on its cell's row of ``centres`` f32 [C, D] (``norms``: see ``ivf_flat_filter_split``); the same answer, bit for bit.
    ``flat_overflow_count`` / ``flat_list_counts`` read this workspace too."""
    B, D = queries.shape
    P = cells.shape[1]
    N = vectors.shape[0] if n_rows is None else n_rows
    dev = queries.device
    ws = _flat_workspace('ivf_flat_search_split_workspace_bytes', (B, P, n_cells, D, k), dev, workspace)
    od, oi = _flat_topk_outputs(B, k, dev)
    check(lib().annlite_ivf_flat_search_topk_split(int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), norms.data_ptr(), N,
                                                   _ptr(valid_bits), cells.data_ptr(), P, int(n_cells), perm.data_ptr(), perm.numel(),
                                                   cell_rows.data_ptr(), cell_order.data_ptr(), int(max_cell_rows), int(max_probed_rows),
                                                   _ptr(centres), _ptr(cell_of), int(k), 1 if sqrt else 0, od.data_ptr(), oi.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), stream_ptr()), 'ivf_flat_search_topk_split')
    return od, oi


# ---------------------------------------------------------------------------------------------- PCA projector
def _row_stride(t: torch.Tensor, what: str) -> int:
    assert t.dim() == 2 and t.dtype == torch.float32, f'{what} must be a 2-D float32 tensor'
    assert t.shape[1] == 1 or t.stride(1) == 1, f'{what}: the rows must be contiguous'
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    assert ld >= t.shape[1], f'{what}: overlapping rows'
    return int(ld)


def affine_rows(x: torch.Tensor, M: torch.Tensor, sub: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``annlite_affine_rows``: ``out[r] = (x[r] - sub) @ M.T + add`` on f32 MFMA -- ``x`` f32 [n, Din] and ``out`` f32 [n, Dout] may be
    row-strided views (contiguous rows), ``M`` f32 [Dout, Din] contiguous, ``sub`` [Din] / ``add`` [Dout] optional."""
    n, Din = x.shape
    Dout, Dm = M.shape
    assert Dm == Din, 'M must be [Dout, Din]'
    assert M.is_contiguous() and M.dtype == torch.float32
    assert sub is None or (sub.numel() == Din and sub.is_contiguous() and sub.dtype == torch.float32)
    assert add is None or (add.numel() == Dout and add.is_contiguous() and add.dtype == torch.float32)
    if out is None:
        out = torch.empty((n, Dout), dtype=torch.float32, device=x.device)
    assert out.shape == (n, Dout)
    check(lib().annlite_affine_rows(x.data_ptr(), n, Din, _row_stride(x, 'x'), M.data_ptr(), Dout, _ptr(sub), _ptr(add), out.data_ptr(),
                                    _row_stride(out, 'out'), stream_ptr()), 'affine_rows')
    return out


def pca_accumulate(x: torch.Tensor, shift: torch.Tensor, sum64: torch.Tensor, gram64: torch.Tensor,
                   workspace: Optional[ScanWorkspace] = None) -> None:
    """``annlite_pca_accumulate``: ``sum64 (f64 [D]) += sum (x - shift)`` and ``gram64 (f64 [D, D]) += sum (x - shift)(x - shift)^T`` over
    the rows of ``x`` f32 [n, D], in place; chunked f32 MFMA products folded in f64 in a fixed order (the same bits on every run)."""
    n, D = x.shape
    assert shift.numel() == D and shift.dtype == torch.float32 and shift.is_contiguous()
    assert sum64.dtype == torch.float64 and sum64.numel() == D and sum64.is_contiguous()
    assert gram64.dtype == torch.float64 and gram64.shape == (D, D) and gram64.is_contiguous()
    need = ctypes.c_int64(0)
    check(lib().annlite_pca_accumulate_workspace_bytes(n, D, ctypes.byref(need)), 'pca_accumulate_workspace_bytes')
    ws = (workspace or ScanWorkspace()).get(int(need.value), x.device)
    check(lib().annlite_pca_accumulate(x.data_ptr(), n, D, _row_stride(x, 'x'), shift.data_ptr(), sum64.data_ptr(), gram64.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream_ptr()), 'pca_accumulate')


def pca_chunk_rows() -> int:
    """Rows of one partial product of ``pca_accumulate`` (a compile-time constant of the library)."""
    return 512


# ---------------------------------------------------------------------------------------------- filterable columns
def filter_eval(program: '_capi.FilterProgram', n_rows: int, n_words: int, and_bits: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None, max_blocks: int = 0,
                dev: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_filter_eval``: the program (``_capi.FilterProgram``, its pointers device arrays over ``n_rows`` rows) evaluated into
    ``out`` i32 [n_words] -- bit r = row r passes, ANDed with ``and_bits`` i32 [n_words] where given, every word behind the rows 0 --
    and the number of set bits ADDED to ``count`` i64 [1] (a fresh zero by default).  Returns ``(out, count)``."""
    _capi.require_gpu()
    if dev is None:
        dev = and_bits.device if and_bits is not None else out.device if out is not None else device()
    if out is None:
        out = torch.empty((n_words,), dtype=torch.int32, device=dev)
    if count is None:
        count = torch.zeros((1,), dtype=torch.int64, device=dev)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == n_words
    assert count.dtype == torch.int64 and count.numel() == 1
    assert and_bits is None or (and_bits.dtype == torch.int32 and and_bits.is_contiguous() and and_bits.numel() >= n_words)
    check(lib().annlite_filter_eval(ctypes.byref(program), n_rows, _ptr(and_bits), out.data_ptr(), n_words, count.data_ptr(), max_blocks,
                                    stream_ptr()), 'filter_eval')
    return out, count


def _page_out(count: int, out: Optional[torch.Tensor], dev) -> torch.Tensor:
    """i32 [count + 1]: the page's rows and, behind them, their number -- one buffer, so that one copy brings both to the host"""
    if out is None:
        out = torch.empty((count + 1,), dtype=torch.int32, device=dev)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == count + 1
    return out


def _page_workspace(workspace: Optional[ScanWorkspace], dev) -> torch.Tensor:
    need = ctypes.c_int64(0)
    check(lib().annlite_page_workspace_bytes(ctypes.byref(need)), 'page_workspace_bytes')
    return (workspace or ScanWorkspace()).get(int(need.value), dev)


def _bitmap(t: Optional[torch.Tensor], n_words: int, name: str):
    assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n_words), f'{name}: i32 [>= {n_words}], contiguous'


def order_page(mask: Optional[torch.Tensor], rows: torch.Tensor, values: torch.Tensor, kind: int, present: torch.Tensor, n_rows: int,
               n_words: int, descending: bool, first: int, count: int, rank: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, workspace: Optional[ScanWorkspace] = None,
               max_blocks: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_order_page``: of the rows set in ``mask & rows`` (i32 [n_words] each; ``mask`` None: every row of ``rows``, the
    row-present words) the ones of rank ``[first, first + count)`` in the listing's order by the column -- ``values`` (i64 / f64 / i32
    codes, [>= n_rows]) of ``kind`` (``_capi.COL_*``), ``present`` i32 [n_words], for a str column ``rank`` i32 [dictionary]: code ->
    position in the sorted dictionary.  Rows without a value come first ascending, last descending; equal values stay in ascending
    row.  ``out`` i32 [count + 1] (made here by default) takes the rows and, behind them, their number.  Returns ``(out[:count],
    out[count:])``: the rows -- valid up to the number -- and the number, both still on the device."""
    _capi.require_gpu()
    out = _page_out(count, out, rows.device)
    for t, name in ((mask, 'mask'), (rows, 'rows'), (present, 'present')):
        _bitmap(t, n_words, name)
    want = {_capi.COL_I64: torch.int64, _capi.COL_F64: torch.float64, _capi.COL_CODE: torch.int32}.get(kind)
    assert want is None or (values.dtype == want and values.is_contiguous() and values.numel() >= n_rows), 'values: the kind\'s type, [>= n_rows]'
    assert rank is None or (rank.dtype == torch.int32 and rank.is_contiguous())
    ws = _page_workspace(workspace, rows.device)
    check(lib().annlite_order_page(_ptr(mask), rows.data_ptr(), values.data_ptr(), kind, present.data_ptr(), _ptr(rank),
                                   0 if rank is None else rank.numel(), n_rows, n_words, int(bool(descending)), first, count, out.data_ptr(),
                                   out.data_ptr() + 4 * count, ws.data_ptr(), ws.numel(), max_blocks, stream_ptr()), 'order_page')
    return out[:count], out[count:]


def bitmap_page(bits: torch.Tensor, n_rows: int, n_words: int, first: int, count: int, and_bits: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, workspace: Optional[ScanWorkspace] = None,
                max_blocks: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_bitmap_page``: the rows ``< n_rows`` set in ``bits`` (``& and_bits`` where given; i32 [n_words] each) of rank
    ``[first, first + count)``, ascending.  ``out`` and the return value as ``order_page``'s."""
    _capi.require_gpu()
    out = _page_out(count, out, bits.device)
    _bitmap(bits, n_words, 'bits')
    _bitmap(and_bits, n_words, 'and_bits')
    ws = _page_workspace(workspace, bits.device)
    check(lib().annlite_bitmap_page(bits.data_ptr(), _ptr(and_bits), n_rows, n_words, first, count, out.data_ptr(), out.data_ptr() + 4 * count,
                                    ws.data_ptr(), ws.numel(), max_blocks, stream_ptr()), 'bitmap_page')
    return out[:count], out[count:]


# ---------------------------------------------------------------------------------------------- selected rows
def bitmap_rows(words: torch.Tensor, and_words: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                out: Optional[torch.Tensor] = None, workspace: Optional[ScanWorkspace] = None, sync: bool = True):
    """``annlite_bitmap_rows``: the rows ``< n_rows`` (default: every bit of ``words``) set in ``words`` (``& and_words`` where given;
    i32 words) as ascending offsets in ``out`` i32 (made here by default, ``n_rows`` entries; a shorter one takes the first
    ``out.numel()``).  Returns ``(rows, n)``: ``n`` the number of such rows -- also where ``out`` is shorter -- and ``rows =
    out[:min(n, out.numel())]``.  Reading ``n`` synchronises; ``sync=False`` returns ``(out, count i64 [1] on the device)`` instead."""
    _capi.require_gpu()
    n_words = words.numel()
    N = n_words * 32 if n_rows is None else int(n_rows)
    _bitmap(words, (N + 31) // 32, 'words')
    _bitmap(and_words, (N + 31) // 32, 'and_words')
    dev = words.device
    if out is None:
        out = torch.empty((N,), dtype=torch.int32, device=dev)
    assert out.dtype == torch.int32 and out.is_contiguous()
    need = ctypes.c_int64(0)
    check(lib().annlite_bitmap_rows_workspace_bytes(N, ctypes.byref(need)), 'bitmap_rows_workspace_bytes')
    # (the count behind the block counts, 8-byte aligned: one buffer)
    ws = (workspace or ScanWorkspace()).get(int(need.value) + 8, dev)
    count = ws[int(need.value):int(need.value) + 8].view(torch.int64)
    check(lib().annlite_bitmap_rows(words.data_ptr(), _ptr(and_words), N, n_words, out.data_ptr(), out.numel(), count.data_ptr(), ws.data_ptr(),
                                    int(need.value), stream_ptr()), 'bitmap_rows')
    if not sync:
        return out, count
    n = int(count.item())
    return out[:min(n, out.numel())], n


def _flat_row_set_call(kind: str, flat_filter: str, metric: int, queries, vectors, norms, n_rows, row_set, centre, scale, workspace,
                       k: Optional[int] = None, sqrt: bool = False, bounds=None, stride: int = 1, scores: bool = False):
    """A search (``k``) or one filter stage (``bounds``) of the ``flat_filter`` filter over a row set, through ``annlite_flat_search_topk_<kind>``
    or ``annlite_flat_filter_<kind>``.  The two kinds differ in ``row_set(B, N) -> (n_set, args)`` alone: the rows of the set, which size the
    workspace and the scores, and what the entry takes behind N (``'rows'``: the list and n_sel; ``'grouped'``: the bitmaps)."""
    B, D = queries.shape
    N = vectors.shape[0] if n_rows is None else n_rows
    dev = queries.device
    code = _capi.FLAT_FILTER[flat_filter]
    n_set, set_args = row_set(B, N)
    ws = _flat_workspace(f'flat_search_{kind}_workspace_bytes', (code, n_set, D, B, 1 if k is None else k), dev, workspace)
    if k is not None:
        entry, out = f'flat_search_topk_{kind}', _flat_topk_outputs(B, k, dev)
        job = (int(k), 1 if sqrt else 0, out[0].data_ptr(), out[1].data_ptr())
    else:
        entry, out = f'flat_filter_{kind}', _flat_lists(B, dev, (n_set + stride - 1) // stride if scores else None)
        job = (stride, bounds.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), _ptr(out[2]))
        out = out if scores else out[:2]
    check(getattr(lib(), 'annlite_' + entry)(code, int(metric), queries.data_ptr(), B, D, vectors.data_ptr(), float(scale), norms.data_ptr(),
                                             _ptr(centre), N, *set_args, *job, ws.data_ptr(), ws.numel(), stream_ptr()), entry)
    return out


def _listed_rows(rows: torch.Tensor, n_sel: Optional[int]):
    """the ``row_set`` of the selected-rows entries: the first ``n_sel`` (default: all) of the ascending offsets ``rows`` i32"""
    n_sel = rows.numel() if n_sel is None else int(n_sel)
    assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() >= n_sel
    return lambda B, N: (n_sel, (rows.data_ptr(), n_sel))


def _grouped_rows(valid_bits: Optional[torch.Tensor], masks: torch.Tensor, group: torch.Tensor):
    """the ``row_set`` of the grouped entries: the table under the live bitmap, i32 [G, mask_ld] bitmaps and i32 [B] group ids"""
    def row_set(B: int, N: int):
        assert masks.dtype == torch.int32 and masks.ndim == 2 and masks.is_contiguous() and masks.shape[1] * 32 >= N
        assert group.dtype == torch.int32 and group.is_contiguous() and group.numel() == B
        return N, (_ptr(valid_bits), masks.data_ptr(), masks.shape[1], masks.shape[0], group.data_ptr())
    return row_set


def flat_search_topk_rows(flat_filter: str, metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, rows: torch.Tensor,
                          k: int, n_sel: Optional[int] = None, n_rows: Optional[int] = None, centre: Optional[torch.Tensor] = None,
                          scale: float = 1.0, sqrt: bool = False, workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_flat_search_topk_rows``: ``flat_search_topk`` (``flat_filter`` ``'f32'``), ``_split`` (``'bf16x3'``), ``_f16``
    (``'f16x2'``) or ``_i8`` (``'i8x3'``) over the ``n_sel`` (default: all) ascending offsets ``rows`` i32 instead of the table: the answer
    of that search with the list's rows as its bitmap, bit for bit.  ``flat_overflow_count`` / ``flat_list_counts`` read this workspace
    too."""
    return _flat_row_set_call('rows', flat_filter, metric, queries, vectors, norms, n_rows, _listed_rows(rows, n_sel), centre, scale, workspace,
                              k=k, sqrt=sqrt)


def flat_filter_rows(flat_filter: str, metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, bounds: torch.Tensor,
                     rows: torch.Tensor, n_sel: Optional[int] = None, n_rows: Optional[int] = None, centre: Optional[torch.Tensor] = None,
                     scale: float = 1.0, stride: int = 1, scores: bool = False, workspace: Optional[ScanWorkspace] = None):
    """``annlite_flat_filter_rows``: one stage of the ``flat_filter`` filter over every ``stride``-th of the ``n_sel`` offsets ``rows``:
    ``(cand i32 [B, cap] -- offsets --, count i32 [B])`` and, with ``scores=True`` (not ``'f32'``), the filter's score of every
    (query, stage row) pair by LIST POSITION, f32 [B, ceil(n_sel / stride)]."""
    return _flat_row_set_call('rows', flat_filter, metric, queries, vectors, norms, n_rows, _listed_rows(rows, n_sel), centre, scale, workspace,
                              bounds=bounds, stride=stride, scores=scores)


# ---------------------------------------------------------------------------------------------- a filter per query
def flat_search_topk_grouped(flat_filter: str, metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, masks: torch.Tensor,
                             group: torch.Tensor, k: int, valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                             centre: Optional[torch.Tensor] = None, scale: float = 1.0, sqrt: bool = False,
                             workspace: Optional[ScanWorkspace] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``annlite_flat_search_topk_grouped``: ``flat_search_topk`` (``flat_filter`` ``'f32'``), ``_split`` (``'bf16x3'``), ``_f16``
    (``'f16x2'``) or ``_i8`` (``'i8x3'``) with a bitmap per query: ``masks`` i32 [G, n_words] (each ANDed with the live bitmap by the
    caller), ``group`` i32 [B] in ``[0, G)`` -- an id outside selects nothing.  Row b of the answer is that search's for query b with
    ``masks[group[b]]`` as its bitmap, bit for bit.  ``valid_bits``: the live bitmap (which rows are scored at all).
    ``flat_overflow_count`` / ``flat_list_counts`` read this workspace too."""
    return _flat_row_set_call('grouped', flat_filter, metric, queries, vectors, norms, n_rows, _grouped_rows(valid_bits, masks, group), centre,
                              scale, workspace, k=k, sqrt=sqrt)


def flat_filter_grouped(flat_filter: str, metric: int, queries: torch.Tensor, vectors: torch.Tensor, norms: torch.Tensor, bounds: torch.Tensor,
                        masks: torch.Tensor, group: torch.Tensor, valid_bits: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                        centre: Optional[torch.Tensor] = None, scale: float = 1.0, stride: int = 1, scores: bool = False,
                        workspace: Optional[ScanWorkspace] = None):
    """``annlite_flat_filter_grouped``: one stage of the ``flat_filter`` filter over every ``stride``-th row of the table with a bitmap
    per query (``masks`` / ``group`` as ``flat_search_topk_grouped``): ``(cand i32 [B, cap], count i32 [B])`` and, with ``scores=True``
    (not ``'f32'``), the filter's score of every (query, stage row) pair, f32 [B, ceil(N / stride)]."""
    return _flat_row_set_call('grouped', flat_filter, metric, queries, vectors, norms, n_rows, _grouped_rows(valid_bits, masks, group), centre,
                              scale, workspace, bounds=bounds, stride=stride, scores=scores)
