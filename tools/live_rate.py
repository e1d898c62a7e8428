"""What the liveness queries (ModelChecker.graph_eventually / graph_scc) cost, beside the passes of the same shape.

For BASELINE configs[1] (3 servers, 1 value, MaxElection 2: 223,437 states, 936,729 edges) and 3 servers, 2 values,
MaxElection 2 (18.5 M states, 108 M edges, reach_rate.py's larger graph): one checker with keep exhausts the state
space, and on the kept graph, in this one process, after a first query that builds the reverse CSR:
  the backward pass of "RaftCanCommt = TRUE" (graph_reach: a CAS per predecessor entry)       -- predates this tool
  the attractor of "RaftCanCommt = TRUE" and of "CommitAll = TRUE" (graph_eventually: an atomicSub per entry)
  graph_shape (degree histograms and Kahn peeling)                                             -- predates this tool
  graph_scc (the peeling, the in-edge trimming, and on a graph with cycles the colouring)
  graph_avoid_path from the first avoider (the edge-parallel next_avoid pass and the copy of its array)
each three times, the best.  Recorded (profiles/live_rate.txt), not gated: nothing comparable exists to hold them to.

usage: python tools/live_rate.py [--out profiles/live_rate.txt] [--only c2|n3v2e2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import raftmc  # noqa: E402
from graph_rate import CONFIGS  # noqa: E402

QUERIES = ("RaftCanCommt", "CommitAll")
REPEAT = 3


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def measure(kw):
    with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
        mc.set_timing(0)
        mc.set_graph_keep()
        res = mc.run()
        assert res.status == "done", res.status
        first = mc.graph_reach(QUERIES[0])  # (builds the CSR)
        back = [mc.graph_reach(QUERIES[0]) for _ in range(REPEAT)]
        live = {q: [mc.graph_eventually(q) for _ in range(REPEAT)] for q in QUERIES}
        shape = [timed(mc.graph_shape) for _ in range(REPEAT)]
        scc = [timed(mc.graph_scc) for _ in range(REPEAT)]
        walks = []
        r = mc.graph_eventually(QUERIES[0])
        if r.first_avoid is not None:
            for _ in range(REPEAT):
                mc.graph_eventually(QUERIES[0])  # (a new query: the next_avoid pass runs again)
                walks.append(timed(lambda: mc.graph_avoid_path(r.first_avoid)))
    return res, first, back, live, shape, scc, walks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_rate.txt"))
    ap.add_argument("--only", choices=sorted(CONFIGS))
    a = ap.parse_args()
    lines = ["liveness queries: python tools/live_rate.py -- per configuration one checker with keep; on the kept graph, after "
             f"the CSR build, each pass {REPEAT} times (the best): the backward pass and graph_shape (both older) beside the "
             "attractor and graph_scc, then the avoid walk from the first avoider"]
    for key, (name, kw) in CONFIGS.items():
        if a.only and a.only != key:
            continue
        try:
            res, first, back, live, shape, scc, walks = measure(kw)
        except raftmc.RmcError as e:
            lines += ["", f"{name}: not measured: {e}"]
            continue
        edges = first.edges
        rate = lambda s: f"{edges / max(s, 1e-9):,.0f} edges/s"  # noqa: E731
        lines.append("")
        lines.append(f"{name}: {res.distinct:,} distinct, {edges:,} edges ({first.self_edges:,} self-edges); reverse CSR build "
                     f"{first.csr_seconds * 1e3:.2f} ms")
        b = min(x.seconds for x in back)
        lines.append(f"  backward pass of {QUERIES[0]} = TRUE ({back[0].rounds} rounds): best {b * 1e3:.2f} ms: {rate(b)}; "
                     f"{back[0].can_reach:,} can reach one, {back[0].cannot_reach:,} cannot")
        for q in QUERIES:
            rs = live[q]
            t = min(x.seconds for x in rs)
            r = rs[0]
            lines.append(f"  attractor of {q} = TRUE ({r.rounds} rounds): best {t * 1e3:.2f} ms: {rate(t)}; {r.targets:,} satisfy it, "
                         f"{r.must:,} must reach one (latest {r.max_within}, Init {r.init_within}), {r.avoiders:,} can avoid it "
                         f"({r.avoid_terminal:,} terminal; first gid {r.first_avoid}, level {r.first_avoid_level})")
        sh, t = min(shape, key=lambda x: x[1])
        lines.append(f"  graph_shape: best {t * 1e3:.2f} ms; cyclic_states {sh['cyclic_states']:,}")
        s, t = min(scc, key=lambda x: x[1])
        lines.append(f"  graph_scc: best {t * 1e3:.2f} ms wall, {s.seconds * 1e3:.2f} ms inside ({s.rounds} rounds read by the host); "
                     f"{s.components:,} components, {s.nontrivial:,} of more than one state ({s.nontrivial_states:,} states, "
                     f"largest {s.largest:,}), trimmed {s.trimmed:,}")
        if walks:
            (gids, at), t = min(walks, key=lambda x: x[1])
            lines.append(f"  graph_avoid_path from the first avoider: best {t * 1e3:.2f} ms; {len(gids)} states, "
                         + ("ends where no step leads out" if at is None else f"back to index {at}"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
