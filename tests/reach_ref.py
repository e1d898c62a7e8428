"""numpy references for the reachability tests (tests/test_reach_host.py, tests/test_gpu_reach.py): fixpoints over
plain edge arrays, sharing no code with the library's kernels or with tests/golden/make_golden_reach.py."""
import hashlib

import numpy as np

UNSET = 0xFFFFFFFF


def targets_of(inv, bit, value):
    """bool per state: invariant `bit` evaluated to `value` (an evaluation error is in neither set)"""
    inv = np.asarray(inv, dtype=np.uint32)
    return (((inv >> (8 + bit)) & 1) == 0) & (((inv >> bit) & 1) == (1 if value else 0))


def np_dist(n, src, dst, target):
    """u32 per state: the fewest edges to a state of `target`, UNSET if there is no path.  Relaxes every edge per
    round until nothing changes (dist[src] = min(dist[src], dist[dst] + 1)): n rounds at most."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    big = np.int64(1) << 40
    d = np.where(np.asarray(target, dtype=bool), np.int64(0), big)
    while True:
        cand = d[dst] + 1
        new = d.copy()
        np.minimum.at(new, src, cand)
        if np.array_equal(new, d):
            break
        d = new
    return np.where(d >= big, UNSET, d).astype(np.uint32)


def np_cyclic(n, src, dst):
    """states left after repeatedly removing every state with no non-self edge into a state still present"""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    present = np.ones(n, dtype=bool)
    while True:
        live = present[src] & present[dst]
        out = np.bincount(src[live], minlength=n)
        nxt = present & (out > 0)
        if np.array_equal(nxt, present):
            return int(present.sum())
        present = nxt


def np_shape(n, src, dst):
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    ind, outd = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    return dict(states=n, edges=len(src), self_edges=int((src == dst).sum()), back_edges=int((dst < src).sum()),
                sinks=int((outd == 0).sum()), max_in=int(ind.max()) if n else 0, max_out=int(outd.max()) if n else 0,
                cyclic_states=np_cyclic(n, src, dst),
                in_hist=np.bincount(np.minimum(ind, 63), minlength=64).tolist(),
                out_hist=np.bincount(np.minimum(outd, 63), minlength=64).tolist())


def np_levels(n, src, dst):
    """BFS level (0 = Init's) per gid of a graph in discovery order: one below the source of the first edge in"""
    lv = np.full(n, -1, dtype=np.int64)
    lv[0] = 0
    for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if lv[d] < 0:
            lv[d] = lv[s] + 1
    return lv


def np_query(n, src, dst, target, lv=None):
    """The fields of a reach.json query entry (make_golden_reach.py's format) from the numpy fixpoint."""
    dist = np_dist(n, src, dst, target)
    cannot = np.flatnonzero(dist == UNSET)
    lv = np.zeros(n, dtype=np.int64) if lv is None else lv
    nl = int(lv.max()) + 1
    can_l = np.bincount(lv[dist != UNSET], minlength=nl)
    cannot_l = np.bincount(lv[dist == UNSET], minlength=nl)
    return dict(targets=int(np.asarray(target).sum()), can_reach=n - len(cannot), cannot_reach=len(cannot),
                first_cannot=int(cannot[0]) if len(cannot) else None,
                first_cannot_level=int(lv[cannot[0]]) + 1 if len(cannot) else None,
                max_distance=int(dist[dist != UNSET].max()) if (dist != UNSET).any() else 0,
                init_distance=None if dist[0] == UNSET else int(dist[0]),
                levels=[[int(a), int(b)] for a, b in zip(can_l, cannot_l)],
                dist_sha256=hashlib.sha256(dist.astype("<u4").tobytes()).hexdigest()), dist


def result_fields(r, levels):
    """A raftmc.ReachResult and graph_reach_levels() in the same format (without the digest)."""
    return dict(targets=r.targets, can_reach=r.can_reach, cannot_reach=r.cannot_reach, first_cannot=r.first_cannot,
                first_cannot_level=r.first_cannot_level, max_distance=r.max_distance, init_distance=r.init_distance,
                levels=[[int(a), int(b)] for a, b in levels])
