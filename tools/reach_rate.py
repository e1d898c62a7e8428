"""What the reachability queries (ModelChecker.set_graph_keep / graph_reach / graph_shape) cost.

For BASELINE configs[1] (3 servers, 1 value, MaxElection 2: 223,437 states, 936,729 edges) and 3 servers, 2 values,
MaxElection 2 (18.5 M states, 108 M edges, the largest graph_rate.py measures): on one checker, after untimed
exhaustions that grow the buffers, the state space is exhausted in plain graph mode (edges only, the sink discards
them: graph_rate.py's "on") and with keep (no sink), alternating, twice each: the cost of keep over plain graph
mode.  Then on the kept graph: the reverse CSR's build (edges/s; rmc_reach_result.csr_seconds, measured by dropping
the CSR with a reset and a new run before each query), the backward pass of "RaftCanCommt = TRUE" (edges/s over
every edge of the graph, three queries, the best), and graph_shape (degrees and Kahn peeling).  Recorded
(profiles/reach_rate.txt), not gated: nothing comparable exists to hold them to.

usage: python tools/reach_rate.py [--out profiles/reach_rate.txt] [--only c2|n3v2e2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import raftmc  # noqa: E402
from graph_rate import CONFIGS, Count  # noqa: E402

QUERY = "RaftCanCommt"


def exhaust(mc, keep):
    """keep: the kept graph, no sink; otherwise plain graph mode, edges delivered and discarded"""
    mc.reset()
    if keep:
        mc.clear_graph()
    else:
        mc.set_graph(states=False, on_edges=Count())
    t0 = time.perf_counter()
    res = mc.run()
    dt = time.perf_counter() - t0
    assert res.status == "done", res.status
    return res, dt


def measure(kw):
    # plain graph mode on a checker of its own (keep can only be switched before init, and stays)
    with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
        mc.set_timing(0)
        mc.run()
        exhaust(mc, False)
        plain = [exhaust(mc, False)[1] for _ in range(2)]
    with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
        mc.set_timing(0)
        mc.set_graph_keep()
        first = mc.run()
        kept, csr, back, rounds = [], [], [], 0
        r = None
        for _ in range(2):
            res, dt = exhaust(mc, True)
            assert (res.generated, res.distinct) == (first.generated, first.distinct)
            kept.append(dt)
            r = mc.graph_reach(QUERY)  # (the first query on a kept graph builds the CSR)
            csr.append(r.csr_seconds)
            back.append(r.seconds)
            for _ in range(2):
                back.append(mc.graph_reach(QUERY).seconds)
            rounds = r.rounds
        t0 = time.perf_counter()
        sh = mc.graph_shape()
        shape_s = time.perf_counter() - t0
        assert r.edges == first.generated - 1 == sh["edges"]
    return first, plain, kept, csr, back, rounds, r, sh, shape_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_rate.txt"))
    ap.add_argument("--only", choices=sorted(CONFIGS))
    a = ap.parse_args()
    lines = ["reachability queries: python tools/reach_rate.py -- per configuration two warm checkers: exhaustions in plain "
             "graph mode (edges only, discarded) and with keep (no sink), twice each; then on the kept graph the reverse CSR "
             f"build, the backward pass of {QUERY} = TRUE (best of 6) and graph_shape"]
    for key, (name, kw) in CONFIGS.items():
        if a.only and a.only != key:
            continue
        try:
            first, plain, kept, csr, back, rounds, r, sh, shape_s = measure(kw)
        except raftmc.RmcError as e:
            lines += ["", f"{name}: not measured: {e}"]
            continue
        edges = r.edges
        lines.append("")
        lines.append(f"{name}: {first.distinct:,} distinct, {edges:,} edges ({r.self_edges:,} self-edges)")
        lines.append("  plain graph mode: " + ", ".join(f"{t:.3f} s" for t in plain) + "   keep: " +
                     ", ".join(f"{t:.3f} s" for t in kept) + f"   keep/plain (best of each): {min(kept) / min(plain):.3f}")
        lines.append(f"  reverse CSR build: " + ", ".join(f"{t * 1e3:.2f} ms" for t in csr) +
                     f": {edges / max(min(csr), 1e-9):,.0f} edges/s")
        lines.append(f"  backward pass ({rounds} rounds): best {min(back) * 1e3:.2f} ms of {len(back)}: "
                     f"{edges / max(min(back), 1e-9):,.0f} edges/s")
        lines.append(f"  {QUERY} = TRUE: {r.targets:,} satisfy it, {r.can_reach:,} can reach one (farthest {r.max_distance}, "
                     f"Init {r.init_distance}), {r.cannot_reach:,} cannot (first gid {r.first_cannot}, level {r.first_cannot_level})")
        lines.append(f"  graph_shape: {shape_s * 1e3:.2f} ms; cyclic_states {sh['cyclic_states']:,}, back edges {sh['back_edges']:,}, "
                     f"sinks {sh['sinks']:,}, max in {sh['max_in']}, max out {sh['max_out']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
