"""What action coverage (ModelChecker.set_coverage, TLC's -coverage) costs, and its table at scale.

For Raft.cfg (3 servers, 2 values, MaxElection 3: 10.9 G states) and BASELINE configs[1] (3 servers, 1
value, MaxElection 2): on one checker, after an untimed exhaustion that grows the buffers, the state space
is exhausted with coverage off and on, alternating, twice each.  The counts must add up to the run's
counters (for Raft.cfg: the known totals), and every covered run must give the same table.  The on/off
ratio is recorded (profiles/coverage_rate.txt), not gated: TLC's own -coverage overhead cannot be run
beside it.

usage: python tools/coverage_rate.py [--out profiles/coverage_rate.txt] [--only raftcfg|c2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))

import raftmc  # noqa: E402

CONFIGS = {
    "raftcfg": ("Raft.cfg (n=3, V=2, E=3, R=3)", dict(n_servers=3, n_vals=2, max_election=3, max_restart=3),
                (56936653204, 10946499503)),
    "c2": ("configs[1] (n=3, V=1, E=2, R=3)", dict(n_servers=3, n_vals=1, max_election=2, max_restart=3),
           (936730, 223437)),
}


def exhaust(mc, on):
    mc.reset()
    mc.set_coverage(on)
    t0 = time.perf_counter()
    res = mc.run()
    dt = time.perf_counter() - t0
    assert res.status == "done", res.status
    return res, dt, (mc.coverage() if on else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage_rate.txt"))
    ap.add_argument("--only", choices=sorted(CONFIGS))
    a = ap.parse_args()
    lines = ["action coverage: exhaustions with coverage off / on, alternating, twice each on one warm checker"]
    for key, (name, kw, (gen, dist)) in CONFIGS.items():
        if a.only and a.only != key:
            continue
        with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
            mc.set_timing(0)
            mc.run()  # (untimed: allocation and buffer growth)
            times, table = {False: [], True: []}, None
            for on in (False, True, False, True):
                res, dt, cov = exhaust(mc, on)
                assert (res.generated, res.distinct) == (gen, dist), (res.generated, res.distinct)
                times[on].append(dt)
                if on:
                    assert 1 + sum(g for k, (d, g) in cov.items() if k != "Init") == gen
                    assert 1 + sum(d for k, (d, g) in cov.items() if k != "Init") == dist
                    assert table is None or table == cov
                    table = cov
        off, onn = min(times[False]), min(times[True])
        lines.append("")
        lines.append(f"{name}: {dist:,} distinct, {gen:,} generated")
        lines.append("  off: " + ", ".join(f"{t:.3f} s" for t in times[False]) +
                     "   on: " + ", ".join(f"{t:.3f} s" for t in times[True]) +
                     f"   on/off (best of each): {onn / off:.3f}")
        lines.append(f"  {'action':<22}{'distinct':>16}{'generated':>18}{'% of generated':>16}")
        for act, (d, g) in table.items():
            if act in ("FollowerAppendEntry", "BecomeFollower"):
                continue  # not in this spec's Next
            lines.append(f"  {act:<22}{d:>16,}{g:>18,}{100.0 * g / gen:>15.2f}%")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
