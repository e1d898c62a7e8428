#!/usr/bin/env python3
"""Golden fixture of the liveness queries (rmc_graph_eventually / rmc_graph_avoid_path / rmc_graph_scc): live.json,
from the Python oracle (oracle/raft_ref.py) alone, over the graphs make_golden_reach.py uses (make_golden_graph.graph_bfs:
states in TLC -workers 1 discovery order, every generated successor an edge, duplicates and self-edges included; an
error-stopped search keeps the states and edges up to TLC's stopping point).

Semantics (include/rmc.h): self-edges are ignored; a fair behaviour is a maximal path; `must` is the least fixpoint of
X = T u {s : s has a non-self edge out and every non-self edge out of s ends in X}; within = 0 on T, 1 + max over the
non-self successors elsewhere in `must`, 0xFFFFFFFF on an avoider.  Per configuration:
  states, edges, level_starts, inv_sha256 (as reach.json)
  scc: components, nontrivial (two states or more), nontrivial_states, largest
  queries[KEY]: KEY is "NAME=TRUE" for each of the seven invariants, two "NAME=FALSE", and two leads-to pairs
  "Q=TRUE~>P=TRUE" (Q the source set):
      targets, must, avoiders, avoid_terminal (avoiders with no non-self edge out), first_avoid (smallest gid, null if
      none), first_avoid_level (1 = Init's level), max_within, init_within (null: Init is an avoider), levels ([must,
      avoid] per BFS level), within_sha256 (little-endian u32 per state in gid order), avoid_path: the walk from
      first_avoid along the smallest successor that is an avoider -- {gids, loop_at} (loop_at null: it ends in a state
      with no non-self edge out; else the index on the path its last state steps back to), null without an avoider;
      a leads-to also has sources, source_avoiders, first_source_avoid, first_source_avoid_level and source_path (the
      walk from first_source_avoid).
The attractor here is counter-based with a work list and Tarjan's algorithm finds the components; tests/live_ref.py
recomputes both another way.

Usage: python tests/golden/make_golden_live.py        (n3_v1_e2_r3 and its seeded twin take a few minutes each)
"""
import hashlib
import json
import os
import struct
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import raft_ref as R  # noqa: E402
from make_golden_graph import CONFIGS as GRAPH_CONFIGS, graph_bfs  # noqa: E402
from make_golden_reach import INV_BY_BIT, NAMES, inv_value, levels_of  # noqa: E402

UNSET = 0xFFFFFFFF
# (target name, value, source name or None, source value)
QUERIES = [(name, 1, None, 1) for name in INV_BY_BIT] + [
    ("RaftCanCommt", 0, None, 1), ("CommitAll", 0, None, 1),
    ("RaftCanCommt", 1, "ExistLeaderAndCandidate", 1), ("CommitAll", 1, "RaftCanCommt", 1)]


def qkey(name, value, source=None, source_value=1):
    k = "%s=%s" % (name, "TRUE" if value else "FALSE")
    return k if source is None else "%s=%s~>%s" % (source, "TRUE" if source_value else "FALSE", k)


def members(inv, name, value):
    b = INV_BY_BIT.index(name)
    return [g for g in range(len(inv)) if not (inv[g] >> (8 + b)) & 1 and (inv[g] >> b) & 1 == value]


def attractor(n, succ, pred, targets):
    """within per state: counters of non-self out-edges, a work list from the targets"""
    within = [UNSET] * n
    left = [len(succ[g]) for g in range(n)]
    todo = list(targets)
    for g in targets:
        within[g] = 0
    while todo:
        nxt = []
        for v in todo:
            for p in pred[v]:
                left[p] -= 1
                if left[p] == 0 and within[p] == UNSET:
                    within[p] = 1 + max(within[d] for d in succ[p])
                    nxt.append(p)
        todo = nxt
    return within


def walk(succ, within, g):
    gids, at = [g], {g: 0}
    while True:
        nx = [d for d in succ[gids[-1]] if within[d] == UNSET]
        if not nx:
            return dict(gids=gids, loop_at=None)
        d = min(nx)
        if d in at:
            return dict(gids=gids, loop_at=at[d])
        at[d] = len(gids)
        gids.append(d)


def tarjan(n, succ):
    """label (smallest gid of the component) per state; iterative"""
    index, low, on, label = [-1] * n, [0] * n, [False] * n, [-1] * n
    stack, k = [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                index[v] = low[v] = k
                k += 1
                stack.append(v)
                on[v] = True
            if i < len(succ[v]):
                work.append((v, i + 1))
                w = succ[v][i]
                if index[w] < 0:
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], index[w])
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                for w in comp:
                    label[w] = min(comp)
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
    return label


def scc_summary(label):
    size = {}
    for c in label:
        size[c] = size.get(c, 0) + 1
    big = [s for s in size.values() if s >= 2]
    return dict(components=len(size), nontrivial=len(big), nontrivial_states=sum(big), largest=max(size.values()))


def query(n, succ, pred, lv, n_levels, inv, name, value, source, source_value):
    within = attractor(n, succ, pred, members(inv, name, value))
    avoid = [g for g in range(n) if within[g] == UNSET]
    levels = [[0, 0] for _ in range(n_levels)]
    for g in range(n):
        levels[lv[g]][1 if within[g] == UNSET else 0] += 1
    q = dict(targets=sum(1 for w in within if w == 0), must=n - len(avoid), avoiders=len(avoid),
             avoid_terminal=sum(1 for g in avoid if not succ[g]), first_avoid=avoid[0] if avoid else None,
             first_avoid_level=lv[avoid[0]] + 1 if avoid else None,
             max_within=max((w for w in within if w != UNSET), default=0),
             init_within=None if within[0] == UNSET else within[0], levels=levels,
             within_sha256=hashlib.sha256(struct.pack("<%dI" % n, *within)).hexdigest(),
             avoid_path=walk(succ, within, avoid[0]) if avoid else None)
    if source is not None:
        src = members(inv, source, source_value)
        sav = [g for g in src if within[g] == UNSET]
        q.update(sources=len(src), source_avoiders=len(sav), first_source_avoid=sav[0] if sav else None,
                 first_source_avoid_level=lv[sav[0]] + 1 if sav else None,
                 source_path=walk(succ, within, sav[0]) if sav else None)
    return q


def entry(name):
    _src, kw = GRAPH_CONFIGS[name]
    cfg = R.Config(max_restart=3, **kw)
    verdict, states, edges3, _per_level = graph_bfs(cfg)
    n = len(states)
    edges = [(s, d) for s, _k, d in edges3]
    lv = levels_of(n, edges)
    n_levels = lv[-1] + 1
    succ, pred = [[] for _ in range(n)], [[] for _ in range(n)]
    for s, d in edges:  # (duplicates stay: the counters count them)
        if s != d:
            succ[s].append(d)
            pred[d].append(s)
    inv = [inv_value(cfg, st) for st in states]
    e = dict(verdict=verdict, states=n, edges=len(edges), level_starts=[lv.index(k) for k in range(n_levels)],
             inv_sha256=hashlib.sha256(struct.pack("<%dH" % n, *inv)).hexdigest(), scc=scc_summary(tarjan(n, succ)),
             queries={})
    for q in QUERIES:
        e["queries"][qkey(*q)] = query(n, succ, pred, lv, n_levels, inv, *q)
    return name, e


def main():
    with ProcessPoolExecutor(max_workers=min(len(NAMES), os.cpu_count() or 1)) as ex:
        out = dict(ex.map(entry, NAMES))
    for name in NAMES:
        e = out[name]
        q = e["queries"]["RaftCanCommt=TRUE"]
        print(name, e["verdict"], e["states"], e["edges"], e["scc"],
              {k: q[k] for k in ("targets", "must", "avoiders", "avoid_terminal", "first_avoid", "max_within", "init_within")},
              flush=True)
    with open(os.path.join(HERE, "live.json"), "w") as f:
        json.dump({name: out[name] for name in NAMES}, f, indent=1)


if __name__ == "__main__":
    main()
