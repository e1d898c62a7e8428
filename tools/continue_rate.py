"""What continuation (ModelChecker.set_continue, TLC's -continue) costs, at both ends.

Raft.cfg with INVARIANT Inv (3 servers, 2 values, MaxElection 3: 10.9 G states, none violates) and
n3_v1_e3_r3 with INVARIANT ExistLeaderAndCandidate (3 servers, 1 value, MaxElection 3: 60.2 M states, nearly
every one violates), and configs[1] with Inv (223,437 states, a run of a few milliseconds inside the device-driven
level loop).  The off run of n3_v1_e3_r3 checks Inv instead: with ExistLeaderAndCandidate and continuation off the
search ends at Init, so that ratio also holds the difference between evaluating the two invariants.  On one checker per case, after an untimed exhaustion that grows
the buffers, the state space is exhausted with continuation off and on, alternating, twice each; the counters
must be the known totals in every run and the violation counts the same in every run that counts.  The on/off
ratios are recorded (profiles/continue_rate.txt), not gated.

usage: python tools/continue_rate.py [--out profiles/continue_rate.txt] [--only raftcfg|c2|e3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))

import raftmc  # noqa: E402

# key -> (title, ModelConfig keywords, invariants of the on run, of the off run, (generated, distinct))
CONFIGS = {
    "raftcfg": ("Raft.cfg (n=3, V=2, E=3, R=3), INVARIANT Inv", dict(n_servers=3, n_vals=2, max_election=3, max_restart=3),
                ("Inv",), ("Inv",), (56936653204, 10946499503)),
    "c2": ("configs[1] (n=3, V=1, E=2, R=3), INVARIANT Inv", dict(n_servers=3, n_vals=1, max_election=2, max_restart=3),
           ("Inv",), ("Inv",), (936730, 223437)),
    "e3": ("n3_v1_e3_r3 (n=3, V=1, E=3, R=3), INVARIANT ExistLeaderAndCandidate",
           dict(n_servers=3, n_vals=1, max_election=3, max_restart=3), ("ExistLeaderAndCandidate",), ("Inv",), (248221155, 60230324)),
}


def exhaust(mc, on):
    mc.reset()
    mc.set_continue(on)
    t0 = time.perf_counter()
    res = mc.run()
    dt = time.perf_counter() - t0
    assert res.status == "done", res.status
    return res, dt, (mc.violations() if on else None)


def measure(kw, inv, on, totals):
    """An untimed exhaustion, then two timed ones, on one checker."""
    gen, dist = totals
    times, viol = [], None
    with raftmc.ModelChecker(raftmc.ModelConfig(invariants=inv, **kw)) as mc:
        mc.set_timing(0)
        mc.set_continue(on)
        mc.run()  # (untimed: allocation and buffer growth)
        for _ in range(2):
            res, dt, v = exhaust(mc, on)
            assert res.distinct == dist and (gen is None or res.generated == gen), (res.generated, res.distinct)
            assert viol is None or viol == v
            times.append(dt)
            viol = v
    return times, viol, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continue_rate.txt"))
    ap.add_argument("--only", choices=sorted(CONFIGS))
    a = ap.parse_args()
    lines = ["continuation: exhaustions with continuation off / on, two timed each after an untimed one, one warm "
             "checker per setting"]
    for key, (name, kw, inv_on, inv_off, totals) in CONFIGS.items():
        if a.only and a.only != key:
            continue
        if inv_on == inv_off:  # one checker, alternating
            gen, dist = totals
            times, viol = {False: [], True: []}, None
            with raftmc.ModelChecker(raftmc.ModelConfig(invariants=inv_on, **kw)) as mc:
                mc.set_timing(0)
                mc.run()
                for on in (False, True, False, True):
                    res, dt, v = exhaust(mc, on)
                    assert (res.generated, res.distinct) == (gen, dist), (res.generated, res.distinct)
                    times[on].append(dt)
                    if on:
                        assert viol is None or viol == v
                        viol = v
            t_off, t_on = times[False], times[True]
        else:
            t_off, _, r_off = measure(kw, inv_off, False, totals)
            t_on, viol, res = measure(kw, inv_on, True, totals)
            assert (res.generated, res.distinct, res.depth) == (r_off.generated, r_off.distinct, r_off.depth)
        lines.append("")
        lines.append(f"{name}: {res.distinct:,} distinct, {res.generated:,} generated, depth {res.depth}")
        lines.append("  off: " + ", ".join(f"{t:.3f} s" for t in t_off) + "   on: " + ", ".join(f"{t:.3f} s" for t in t_on) +
                     f"   on/off (best of each): {min(t_on) / min(t_off):.3f}")
        for nm, (count, first) in viol.items():
            lines.append(f"  {nm}: violated by {count:,} states" + (f", first at depth {first}" if first else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
