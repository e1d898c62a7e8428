#!/usr/bin/env python3
"""Golden fixture of the reachability queries (rmc_set_graph_keep / rmc_graph_reach / rmc_graph_shape):
reach.json, from the Python oracle (oracle/raft_ref.py) alone.

The graph of a configuration is make_golden_graph.graph_bfs's: states in TLC -workers 1 discovery order
(Init = gid 0), every generated successor an edge (src, dst), duplicates and self-edges included; an
error-stopped search keeps the states and edges up to TLC's stopping point.  Per configuration:
  states, edges, self_edges, back_edges (dst < src), sinks (no edge out at all), max_in, max_out (every edge
  counts), level_starts (gid of the first state of each BFS level; the level an error stops in included)
  cyclic_states   states left after repeatedly removing every state with no non-self edge into a state still
                  present (0: no cycle other than self-edges)
  inv_sha256      sha256 of the u16 per state, little-endian, in gid order: bit b = invariant b of
                  raftmc.INVARIANT_BY_BIT is TRUE, bit 8 + b = it raised the evaluation error
  queries["NAME=TRUE" | "NAME=FALSE"] for each of the seven invariants: the target set is the states on which
  it evaluated to that value (an evaluation error: neither);
      targets, can_reach (targets included), cannot_reach, first_cannot (smallest gid, null if none),
      first_cannot_level (1 = Init's level, null if none), max_distance, init_distance (null: Init cannot),
      levels ([can, cannot] per BFS level), dist_sha256 (the fewest edges from each state to a target as
      little-endian u32, 0xFFFFFFFF where there is no path, in gid order)
Everything is digests and counts: the file stays small.

Usage: python tests/golden/make_golden_reach.py        (n3_v1_e2_r3 and its seeded twin take a few minutes each)
"""
import hashlib
import json
import os
import struct
import sys
from collections import deque
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import raft_ref as R  # noqa: E402
from make_golden_graph import CONFIGS as GRAPH_CONFIGS, SPOT as GRAPH_SPOT, graph_bfs  # noqa: E402

NAMES = ("n3_v1_e1_r3", "n2_v1_e2_r3", "nosym_n3_v1_e1_r3", "n3_v1_e2_r3", "seeded_n3_v1_e2_r3")
# raftmc.INVARIANT_BY_BIT: bit index -> name
INV_BY_BIT = ("Inv", "NoSplitVote", "RaftCanCommt", "FollowerCanCommit", "CommitAll", "NoAllCommit",
              "ExistLeaderAndCandidate")
UNSET = 0xFFFFFFFF

# spot values computed on the CPU when the feature was specified; RaftCanCommt = TRUE:
# states, targets, can_reach, cannot_reach, first_cannot, max_distance
SPOT = {
    "n3_v1_e1_r3": (545, 300, 408, 137, 10, 9),
    "n2_v1_e2_r3": (1061, 706, 924, 137, 3, 6),
}
CYCLIC_SPOT = {"n3_v1_e1_r3": 0, "n2_v1_e2_r3": 0}


def inv_value(cfg, st):
    v = 0
    for b, name in enumerate(INV_BY_BIT):
        try:
            if R.INV_FUNCS[name](cfg, st):
                v |= 1 << b
        except R.EvalError:
            v |= 1 << (8 + b)
    return v


def levels_of(n_states, edges):
    """level (0 = Init's) per gid: a state is one level below the source of the first edge that reaches it"""
    lv = [-1] * n_states
    lv[0] = 0
    for s, d in edges:
        if lv[d] < 0:
            lv[d] = lv[s] + 1
    assert min(lv) >= 0 and all(lv[i] <= lv[i + 1] for i in range(n_states - 1))
    return lv


def shape(n, edges):
    indeg, outdeg = [0] * n, [0] * n
    for s, d in edges:
        outdeg[s] += 1
        indeg[d] += 1
    return dict(self_edges=sum(1 for s, d in edges if s == d), back_edges=sum(1 for s, d in edges if d < s),
                sinks=sum(1 for x in outdeg if x == 0), max_in=max(indeg), max_out=max(outdeg))


def cyclic_states(n, edges, pred):
    out = [0] * n
    for s, d in edges:
        if s != d:
            out[s] += 1
    todo = deque(g for g in range(n) if out[g] == 0)
    gone = 0
    while todo:
        v = todo.popleft()
        gone += 1
        for p in pred[v]:
            out[p] -= 1
            if out[p] == 0:
                todo.append(p)
    return n - gone


def backward(n, pred, targets):
    dist = [UNSET] * n
    todo = deque()
    for g in targets:
        dist[g] = 0
        todo.append(g)
    while todo:
        v = todo.popleft()
        for p in pred[v]:
            if dist[p] == UNSET:
                dist[p] = dist[v] + 1
                todo.append(p)
    return dist


def query(n, pred, lv, n_levels, targets):
    dist = backward(n, pred, targets)
    cannot = [g for g in range(n) if dist[g] == UNSET]
    levels = [[0, 0] for _ in range(n_levels)]
    for g in range(n):
        levels[lv[g]][1 if dist[g] == UNSET else 0] += 1
    return dict(targets=len(targets), can_reach=n - len(cannot), cannot_reach=len(cannot),
                first_cannot=cannot[0] if cannot else None, first_cannot_level=lv[cannot[0]] + 1 if cannot else None,
                max_distance=max((d for d in dist if d != UNSET), default=0),
                init_distance=None if dist[0] == UNSET else dist[0], levels=levels,
                dist_sha256=hashlib.sha256(struct.pack("<%dI" % n, *dist)).hexdigest())


def entry(name):
    _src, kw = GRAPH_CONFIGS[name]
    cfg = R.Config(max_restart=3, **kw)
    verdict, states, edges3, _per_level = graph_bfs(cfg)
    n = len(states)
    edges = [(s, d) for s, _k, d in edges3]
    assert all(d < n for _s, d in edges)
    lv = levels_of(n, edges)
    n_levels = lv[-1] + 1
    pred = [[] for _ in range(n)]
    for s, d in edges:
        if s != d:
            pred[d].append(s)
    inv = [inv_value(cfg, st) for st in states]
    e = dict(verdict=verdict, states=n, edges=len(edges), **shape(n, edges),
             level_starts=[lv.index(k) for k in range(n_levels)], cyclic_states=cyclic_states(n, edges, pred),
             inv_sha256=hashlib.sha256(struct.pack("<%dH" % n, *inv)).hexdigest(), queries={})
    for b, inv_name in enumerate(INV_BY_BIT):
        for value in (1, 0):
            targets = [g for g in range(n) if not (inv[g] >> (8 + b)) & 1 and (inv[g] >> b) & 1 == value]
            e["queries"]["%s=%s" % (inv_name, "TRUE" if value else "FALSE")] = query(n, pred, lv, n_levels, targets)
    if name in GRAPH_SPOT:  # the shape numbers make_golden_graph.py holds
        w = GRAPH_SPOT[name]
        got = (n, len(edges), e["self_edges"], e["back_edges"] if w[3] is not None else None, e["max_in"], e["max_out"],
               e["sinks"])
        assert got == w[:7], (name, got, w)
    if name in SPOT:
        q = e["queries"]["RaftCanCommt=TRUE"]
        got = (n, q["targets"], q["can_reach"], q["cannot_reach"], q["first_cannot"], q["max_distance"])
        assert got == SPOT[name], (name, got, SPOT[name])
        assert e["cyclic_states"] == CYCLIC_SPOT[name]
    return name, e


def main():
    with ProcessPoolExecutor(max_workers=min(len(NAMES), os.cpu_count() or 1)) as ex:
        out = dict(ex.map(entry, NAMES))
    for name in NAMES:
        e = out[name]
        print(name, e["verdict"], e["states"], e["edges"], "cyclic", e["cyclic_states"],
              {k: e["queries"]["RaftCanCommt=TRUE"][k] for k in ("targets", "can_reach", "cannot_reach", "first_cannot",
                                                                 "first_cannot_level", "max_distance", "init_distance")},
              flush=True)
    with open(os.path.join(HERE, "reach.json"), "w") as f:
        json.dump({name: out[name] for name in NAMES}, f, indent=1)


if __name__ == "__main__":
    main()
