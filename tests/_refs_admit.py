"""The float graph walk with an admitted-result list (annlite_graph_f32_search_admit), restated on ``_refs``'s rule -- shared by
tests/test_graph_f32_admit_restated.py (which checks it, without a GPU) and tests/test_graph_f32_admit_walk.py (which pins the kernel
to it).  Not a conftest, no pytest setting."""
import numpy as np

from _refs import key_to_bits


def _regs(ef):
    return 1 if ef <= 64 else 2 if ef <= 128 else 4  # registers per lane of a list of `ef` places


def walk_admit_restated(links, seeds, keys, ef_route, ef, admit, table=None, stats=None):
    """One query.  ``links`` u32 [N, L+1] (count, ids), ``keys`` u64 [N] (``f32_key`` of the query's distance to every row), ``admit``
    bool [N].  Two sorted lists:

      * C, the routing list: ``_refs.walk_restated``'s at ``ef = ef_route`` (``_refs.walk_forgetful``'s when ``table`` is not None: a
        visited table that records at most ``table`` nodes).  ``admit`` never touches it.
      * R, the result list of ``ef`` places: every batch C is offered (a seed round, an expansion's unseen neighbours) R is offered
        too, restricted to admitted nodes; of those, the ones that beat R's worst entry AS IT IS NOW and are not in R already (nor came
        earlier in the same batch) are merged in.

    Returns (ids i64 [ef], distance bits u32 [ef]): R ascending, (-1, +inf) at the tail.  ``stats`` receives the expansions, the rows
    evaluated, ``admitted_evaluated`` (the set of admitted nodes that were ever offered) and ``route_worst_bits``."""
    n = keys.shape[0]
    slots, cap = 64 * _regs(ef_route), min(ef_route, 64 * _regs(ef_route))
    r_slots, r_cap = 64 * _regs(ef), min(ef, 64 * _regs(ef))
    lst, res = [], []  # C: sorted [(key, node, expanded)]; R: sorted [(key, node)]
    seen = set()
    offered = set()
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
        worst = (lst[cap - 1][0], lst[cap - 1][1]) if len(lst) >= cap else (1 << 40, 1 << 40)
        have = {(t[0], t[1]) for t in lst}
        for v in nodes:
            kv = (int(keys[v]), int(v))
            if kv < worst and kv not in have:
                have.add(kv)
                lst.append((kv[0], kv[1], False))
        lst.sort(key=lambda t: (t[0], t[1]))
        del lst[slots:]
        # ---- R: the same lanes restricted to admitted nodes, the same rule against R's own worst entry ----
        r_worst = res[r_cap - 1] if len(res) >= r_cap else (1 << 40, 1 << 40)
        r_have = set(res)
        for v in nodes:
            if not admit[v]:
                continue
            offered.add(int(v))
            kv = (int(keys[v]), int(v))
            if kv < r_worst and kv not in r_have:
                r_have.add(kv)
                res.append(kv)
        res.sort()
        del res[r_slots:]

    seeds = [int(s) for s in seeds]
    for s0 in range(0, len(seeds), 64):
        rnd = [s for s in seeds[s0:s0 + 64] if s < n]
        n_eval += len(rnd)
        offer(rnd)
    for t in list(lst):
        visit(t[1])
    while True:
        pick = [i for i, t in enumerate(lst[:cap]) if not t[2]][:1]
        if not pick:
            break
        i = pick[0]
        lst[i] = (lst[i][0], lst[i][1], True)
        n_expand += 1
        row = links[lst[i][1]]
        fresh = [int(nb) for nb in row[1:1 + int(row[0])] if int(nb) < n and visit(int(nb))]
        n_eval += len(fresh)
        offer(fresh)
    if stats is not None:
        # (route_worst_bits: the distance of C's last place, +inf while C is not full -- the kernel's out_route_worst)
        stats.update(expansions=n_expand, evals=n_eval, admitted_evaluated=offered,
                     route_worst_bits=key_to_bits(lst[cap - 1][0]) if len(lst) >= cap else 0x7f800000)
    ids = np.full(ef, -1, np.int64)
    bits_ = np.full(ef, np.float32(np.inf).view(np.uint32), np.uint32)
    for i, (k, v) in enumerate(res[:r_cap]):
        ids[i] = v
        bits_[i] = key_to_bits(k)
    return ids, bits_
