"""Walk steps per second of simulation mode (ModelChecker.simulate, TLC's -simulate).

For Raft.cfg (3 servers, 2 values, MaxElection 3) and configs[3] (5 servers, 1 value, MaxElection 3):
2^20 walks of depth 100, seed 1, auto batch, called twice on one checker; the figure is the second
(warm) call's states / seconds -- the states the walks checked over the library's wall time of the
call, host side included.  Nothing comparable exists to hold it to (there is no TLC to run beside it and
the C oracle has no walker), so the number is recorded (profiles/sim_rate.txt), not gated.

usage: python tools/sim_rate.py [--walks N] [--depth D] [--seed S]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))

import raftmc  # noqa: E402

CONFIGS = [("Raft.cfg (n=3, V=2, E=3, R=3)", dict(n_servers=3, n_vals=2, max_election=3, max_restart=3)),
           ("configs[3] (n=5, V=1, E=3, R=3)", dict(n_servers=5, n_vals=1, max_election=3, max_restart=3))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    print(f"simulate: {a.walks} walks, depth {a.depth}, seed {a.seed}, auto batch; second call of two")
    for name, kw in CONFIGS:
        with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
            cold = mc.simulate(a.walks, depth=a.depth, seed=a.seed)
            r = mc.simulate(a.walks, depth=a.depth, seed=a.seed)
        assert (cold.status, cold.states, cold.generated) == (r.status, r.states, r.generated)
        print(f"{name}: {r.states / r.seconds:,.0f} walk steps/s  ({r.states:,} states checked, "
              f"{r.generated:,} generated, {r.seconds:.3f} s warm, {cold.seconds:.3f} s cold; status {r.status}, "
              f"longest {r.longest}, {r.ended_early:,} of {r.walks:,} walks ended without successors)")


if __name__ == "__main__":
    main()
