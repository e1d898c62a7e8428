"""What graph mode (ModelChecker.set_graph, TLC's -dump) costs: edges per second of the edge pass.

For BASELINE configs[1] (3 servers, 1 value, MaxElection 2: 223,437 states, 936,729 edges) and the largest
configuration that stays below graph mode's limit within about a minute (3 servers, 2 values, MaxElection 2): on
one checker, after an untimed exhaustion without and one with graph mode (they grow the buffers and the gid map,
which stay with the checker while graph mode is switched off), the state space is exhausted with graph mode off
and on, alternating, twice each.  On: edges only, the sink discards them (states=False, a callback that
counts).  The edge count must be generated - 1.  edges/s = edges / (on - off), the time the graph pass adds;
the on/off ratio is recorded too (profiles/graph_rate.txt), not gated.

usage: python tools/graph_rate.py [--out profiles/graph_rate.txt] [--only c2|n3v2e2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))

import raftmc  # noqa: E402

CONFIGS = {
    "c2": ("configs[1] (n=3, V=1, E=2, R=3)", dict(n_servers=3, n_vals=1, max_election=2, max_restart=3)),
    # (the seen set keeps its full slots up to 2^30 of them: the engine sizes it on each chunk's successor bound,
    # which passes the default 2^27 at this configuration's widest levels, and graph mode cannot follow it to the
    # compact table)
    "n3v2e2": ("n=3, V=2, E=2, R=3, compact_log2=30", dict(n_servers=3, n_vals=2, max_election=2, max_restart=3,
                                                          compact_log2=30)),
}


class Count:
    def __init__(self):
        self.edges = 0

    def __call__(self, src, key, dst):
        self.edges += len(src)
        return 0


def exhaust(mc, on):
    mc.reset()
    sink = Count()
    if on:
        mc.set_graph(states=False, on_edges=sink)
    else:
        mc.clear_graph()
    t0 = time.perf_counter()
    res = mc.run()
    dt = time.perf_counter() - t0
    assert res.status == "done", res.status
    return res, dt, sink.edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_rate.txt"))
    ap.add_argument("--only", choices=sorted(CONFIGS))
    a = ap.parse_args()
    lines = ["graph mode: exhaustions with graph mode off / on (edges only, discarded), alternating, twice each on one "
             "warm checker"]
    for key, (name, kw) in CONFIGS.items():
        if a.only and a.only != key:
            continue
        try:
            with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
                mc.set_timing(0)
                first = mc.run()  # (untimed: allocation and buffer growth)
                exhaust(mc, True)  # (untimed: the gid map grown to its size, the edge buffers; clear_graph keeps them)
                times, edges = {False: [], True: []}, None
                for on in (False, True, False, True):
                    res, dt, n = exhaust(mc, on)
                    assert (res.generated, res.distinct) == (first.generated, first.distinct)
                    times[on].append(dt)
                    if on:
                        assert n == res.generated - 1, (n, res.generated)
                        edges = n
        except raftmc.RmcError as e:
            lines += ["", f"{name}: not measured: {e}"]
            continue
        off, onn = min(times[False]), min(times[True])
        lines.append("")
        lines.append(f"{name}: {first.distinct:,} distinct, {first.generated:,} generated, {edges:,} edges")
        lines.append("  off: " + ", ".join(f"{t:.3f} s" for t in times[False]) +
                     "   on: " + ", ".join(f"{t:.3f} s" for t in times[True]) +
                     f"   on/off (best of each): {onn / off:.3f}")
        lines.append(f"  the graph pass adds {onn - off:.3f} s: {edges / max(onn - off, 1e-9):,.0f} edges/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
