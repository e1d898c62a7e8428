"""numpy / plain Python references for the liveness tests (tests/test_live_host.py, tests/test_gpu_live.py): fixpoints
over plain edge arrays, sharing no code with the library's kernels or with tests/golden/make_golden_live.py."""
import hashlib

import numpy as np

UNSET = 0xFFFFFFFF


def _no_self(src, dst):
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    keep = src != dst
    return src[keep], dst[keep]


def np_within(n, src, dst, target):
    """u32 per state.  Iterates "a state with a non-self edge out, all of whose non-self successors are set, gets 1 +
    their maximum" from within = 0 on `target` until nothing changes (n rounds at most); UNSET = an avoider."""
    src, dst = _no_self(src, dst)
    out = np.bincount(src, minlength=n)
    w = np.where(np.asarray(target, dtype=bool), np.int64(0), np.int64(-1))
    while True:
        ok = w[dst] >= 0
        n_set = np.bincount(src[ok], minlength=n)
        mx = np.full(n, -1, dtype=np.int64)
        np.maximum.at(mx, src[ok], w[dst[ok]])
        new = (w < 0) & (out > 0) & (n_set == out)
        if not new.any():
            break
        w[new] = mx[new] + 1
    return np.where(w < 0, UNSET, w).astype(np.uint32)


def next_avoid(n, src, dst, within):
    """per state the smallest non-self successor that is an avoider (UNSET: none), for the avoiders"""
    src, dst = _no_self(src, dst)
    both = (within[src] == UNSET) & (within[dst] == UNSET)
    nx = np.full(n, UNSET, dtype=np.int64)
    np.minimum.at(nx, src[both], dst[both])
    return nx


def avoid_walk(nx, gid):
    """(gids, loop_at): follow nx from gid; loop_at = the index on the path the last state steps back to, or None when
    the walk ends in a state without a non-self edge out"""
    gids, at = [int(gid)], {int(gid): 0}
    while True:
        d = int(nx[gids[-1]])
        if d == UNSET:
            return gids, None
        if d in at:
            return gids, at[d]
        at[d] = len(gids)
        gids.append(d)


def np_scc(n, src, dst):
    """u32 per state: the smallest gid of its strongly connected component (self-edges ignored).  Forward and backward
    closures intersected, state after state among those not labelled yet."""
    src, dst = _no_self(src, dst)
    order = np.argsort(src, kind="stable")
    f_row = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
    f_col = dst[order]
    order = np.argsort(dst, kind="stable")
    b_row = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    b_col = src[order]
    label = np.full(n, -1, dtype=np.int64)

    def closure(row, col, g):
        seen = {g}
        todo = [g]
        while todo:
            v = todo.pop()
            for d in col[row[v]:row[v + 1]].tolist():
                if d not in seen and label[d] < 0:
                    seen.add(d)
                    todo.append(d)
        return seen

    # a state without a non-self edge from, or without one into, a state still present is alone: these go first
    present = np.ones(n, dtype=bool)
    while True:
        live = present[src] & present[dst]
        nxt = present & (np.bincount(src[live], minlength=n) > 0) & (np.bincount(dst[live], minlength=n) > 0)
        if np.array_equal(nxt, present):
            break
        present = nxt
    alone = np.flatnonzero(~present)
    label[alone] = alone
    for g in range(n):
        if label[g] >= 0:
            continue
        both = closure(f_row, f_col, g) & closure(b_row, b_col, g)
        label[list(both)] = g  # (g is the smallest unlabelled gid, so the smallest of its component)
    return label.astype(np.uint32)


def scc_summary(label):
    _, size = np.unique(label, return_counts=True)
    big = size[size >= 2]
    return dict(components=int(len(size)), nontrivial=int(len(big)), nontrivial_states=int(big.sum()),
                largest=int(size.max()))


def np_live_query(n, src, dst, target, lv=None, source=None):
    """The fields of a live.json query entry (make_golden_live.py's format) from the numpy fixpoint, and within."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    within = np_within(n, src, dst, target)
    avoid = np.flatnonzero(within == UNSET)
    lv = np.zeros(n, dtype=np.int64) if lv is None else lv
    nl = int(lv.max()) + 1
    s_ns, _ = _no_self(src, dst)
    out_ns = np.bincount(s_ns, minlength=n)
    nx = next_avoid(n, src, dst, within)

    def path(g):
        gids, at = avoid_walk(nx, g)
        return dict(gids=gids, loop_at=at)

    q = dict(targets=int(np.asarray(target).sum()), must=n - len(avoid), avoiders=len(avoid),
             avoid_terminal=int((out_ns[avoid] == 0).sum()), first_avoid=int(avoid[0]) if len(avoid) else None,
             first_avoid_level=int(lv[avoid[0]]) + 1 if len(avoid) else None,
             max_within=int(within[within != UNSET].max()) if (within != UNSET).any() else 0,
             init_within=None if within[0] == UNSET else int(within[0]),
             levels=[[int(a), int(b)] for a, b in zip(np.bincount(lv[within != UNSET], minlength=nl),
                                                      np.bincount(lv[within == UNSET], minlength=nl))],
             within_sha256=hashlib.sha256(within.astype("<u4").tobytes()).hexdigest(),
             avoid_path=path(avoid[0]) if len(avoid) else None)
    if source is not None:
        sav = np.flatnonzero(np.asarray(source, dtype=bool) & (within == UNSET))
        q.update(sources=int(np.asarray(source).sum()), source_avoiders=len(sav),
                 first_source_avoid=int(sav[0]) if len(sav) else None,
                 first_source_avoid_level=int(lv[sav[0]]) + 1 if len(sav) else None,
                 source_path=path(sav[0]) if len(sav) else None)
    return q, within


def live_fields(mc, r, levels):
    """A raftmc.LiveResult, graph_eventually_levels() and the avoid paths in the same format (without the digest)."""
    def path(g):
        if g is None:
            return None
        gids, at = mc.graph_avoid_path(g)
        return dict(gids=gids, loop_at=at)

    q = dict(targets=r.targets, must=r.must, avoiders=r.avoiders, avoid_terminal=r.avoid_terminal,
             first_avoid=r.first_avoid, first_avoid_level=r.first_avoid_level, max_within=r.max_within,
             init_within=r.init_within, levels=[[int(a), int(b)] for a, b in levels], avoid_path=path(r.first_avoid))
    if r.source is not None:
        q.update(sources=r.sources, source_avoiders=r.source_avoiders, first_source_avoid=r.first_source_avoid,
                 first_source_avoid_level=r.first_source_avoid_level, source_path=path(r.first_source_avoid))
    return q
