#!/usr/bin/env python3
"""Golden fixture of graph mode (rmc_set_graph; TLC's -dump): graph.json and graph_full.json.gz, from the
Python oracle (oracle/raft_ref.py) alone.

graph_bfs is raft_ref.bfs's search (TLC -workers 1 order) that also resolves every successor: states get
global ids in discovery order (Init = 0), and every generated successor -- duplicates and self-loops
included, Next's order -- is an edge (src gid, key, dst gid), key = server << 24 | action << 16 | witness, dst
the id of the successor's SYMMETRY/VIEW class (raft_ref.canonical).  The search stops where raft_ref.bfs
stops: at an invariant violation or evaluation error right behind the erring successor's edge, at
UpdateTerm's Assert before the failing sub-action's batch, at a deadlock with no edge of that parent.

Per entry of graph.json: the verdict, the numbers of states and edges, the cumulative edge count after each
level (the level an error stops in included), the edges per action id, and two digests:
  edges_sha256   over the edges packed little-endian as (u64 src, u32 key, u64 dst), in order
  states_sha256  over json.dumps(raft_ref.state_to_json(state), sort_keys=True) + "\\n" per state, in gid order
  states_sample_sha256  the same over the states with gid % 64 == 0
graph_full.json.gz holds the whole edge and state lists of the two smallest configurations.  The entries are
the twelve of coverage.json plus seeded_n3_v1_e2_r3 without invariants (what -continue searches).

Usage: python tests/golden/make_golden_graph.py        (n5_v1_e1_r3 takes ~8 min, noinv_seeded_n3_v1_e2_r3 ~8 min)
"""
import gzip
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
from make_golden_coverage import CONFIGS as COVERAGE_CONFIGS  # noqa: E402

NACT = len(R.ACTIONS)

# name -> (levels file holding the same configuration or None, Config keywords)
CONFIGS = dict(COVERAGE_CONFIGS)
CONFIGS["noinv_seeded_n3_v1_e2_r3"] = (None, dict(n=3, V=1, max_election=2, seeded=True, invariants=()))
FULL = ("n2_v1_e2_r3", "n3_v1_e1_r3")
SAMPLE = 64  # states_sample_sha256: the states with gid % SAMPLE == 0 (what a test of a large run can afford to render)

# spot values computed on the CPU when the feature was specified:
# states, edges, dst == src, dst < src (None: not recorded), max in-degree, max out-degree, states without an
# edge out, first 16 hex digits of edges_sha256
SPOT = {
    "n2_v1_e2_r3": (1061, 2058, 696, 7, 5, 5, 94, "b1d08da200988cb0"),
    "n3_v1_e1_r3": (545, 2028, 946, 0, 7, 6, 2, "f67499a64d9ff63f"),
    "nosym_n3_v1_e1_r3": (3172, 11859, 5532, None, 7, 6, 6, "11d17c2658236094"),
    "n4_v1_e1_r3": (3323, 17318, 9168, None, 9, 8, 2, "a378f84244923b40"),
}


def edge_key(s, a, w):
    return (s << 24) | (a << 16) | w


def graph_bfs(cfg):
    """Returns (verdict, states, edges, edges_per_level): states in gid order, edges as (src, key, dst) in
    TLC -workers 1 order, edges_per_level[k] = edges delivered once level k + 1 was expanded (or stopped in)."""
    def bad(st):
        try:
            return "invariant" if any(not R.INV_FUNCS[i](cfg, st) for i in cfg.invariants) else None
        except R.EvalError:
            return "eval_error"

    s0 = R.init_state(cfg)
    gid = {R.canonical(cfg, s0): 0}
    states, edges, per_level = [s0], [], []
    if bad(s0):
        return bad(s0), states, edges, per_level
    level = [0]
    while level:
        nxt = []

        def stop(verdict):
            per_level.append(len(edges))
            return verdict, states, edges, per_level

        for src in level:
            st, n_succ = states[src], 0
            try:
                for s, a, batch in R.successor_batches(cfg, st):
                    n_succ += len(batch)
                    for w, t in batch:
                        c = R.canonical(cfg, t)
                        d = gid.get(c)
                        new = d is None
                        if new:
                            d = gid[c] = len(states)
                            states.append(t)
                        edges.append((src, edge_key(s, a, w), d))
                        if new:
                            if bad(t):
                                return stop(bad(t))
                            nxt.append(d)
            except R.AssertionFailure:  # raised before the failing sub-action's batch is yielded
                return stop("assert")
            if n_succ == 0 and cfg.check_deadlock:
                return stop("deadlock")
        per_level.append(len(edges))
        level = nxt
    return "ok", states, edges, per_level


def edges_digest(edges):
    h = hashlib.sha256()
    for src, key, dst in edges:
        h.update(struct.pack("<QIQ", src, key, dst))
    return h.hexdigest()


def state_line(d):
    return json.dumps(d, sort_keys=True) + "\n"


def states_digest(dicts):
    h = hashlib.sha256()
    for d in dicts:
        h.update(state_line(d).encode())
    return h.hexdigest()


def shape(n_states, edges):
    """(dst == src, dst < src, max in-degree, max out-degree, states without an edge out)"""
    indeg, outdeg = [0] * n_states, [0] * n_states
    for src, _k, dst in edges:
        outdeg[src] += 1
        indeg[dst] += 1
    return (sum(1 for s, _k, d in edges if s == d), sum(1 for s, _k, d in edges if d < s), max(indeg), max(outdeg),
            sum(1 for x in outdeg if x == 0))


def entry(name):
    src, kw = CONFIGS[name]
    cfg = R.Config(max_restart=3, **kw)
    verdict, states, edges, per_level = graph_bfs(cfg)
    by_action = [0] * NACT
    for _s, k, _d in edges:
        by_action[(k >> 16) & 0xFF] += 1
    dicts = [R.state_to_json(st) for st in states]
    e = dict(levels_file=src, verdict=verdict, states=len(states), edges=len(edges), edges_per_level=per_level,
             by_action=by_action, edges_sha256=edges_digest(edges), states_sha256=states_digest(dicts),
             states_sample_sha256=states_digest(dicts[::SAMPLE]))
    if name in SPOT:
        loops, back, max_in, max_out, sinks = shape(len(states), edges)
        want = SPOT[name]
        got = (len(states), len(edges), loops, back if want[3] is not None else None, max_in, max_out, sinks,
               e["edges_sha256"][:16])
        assert got == want, (name, got, want)
    full = dict(edges=[list(x) for x in edges], states=dicts) if name in FULL else None
    return name, e, full


def main():
    with ProcessPoolExecutor(max_workers=min(len(CONFIGS), os.cpu_count() or 1)) as ex:
        res = {name: (e, full) for name, e, full in ex.map(entry, CONFIGS)}
    out = {name: res[name][0] for name in CONFIGS}
    for name, e in out.items():
        print(name, e["verdict"], e["states"], e["edges"], flush=True)
    with open(os.path.join(HERE, "graph.json"), "w") as f:
        json.dump(out, f, indent=1)
    # (mtime 0: the same bytes from every run)
    with open(os.path.join(HERE, "graph_full.json.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(json.dumps({name: res[name][1] for name in FULL}, separators=(",", ":")).encode())


if __name__ == "__main__":
    main()
