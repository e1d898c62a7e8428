#!/usr/bin/env python3
"""Golden fixture of the action coverage (rmc_set_coverage; TLC's -coverage): coverage.json, from the
Python oracle (oracle/raft_ref.py) alone.

Per configuration: the verdict, TLC's counters, and per action id (raft_ref.ACTIONS / raftmc.ACTIONS,
13 of them) `generated` -- the successors of that action among those "states generated" counts, self-loops
and duplicates included -- and `distinct` -- the states first found through it.  Init is apart (1:1), so
    1 + sum(generated) == generated total        1 + sum(distinct) == distinct total
in every outcome: cover_bfs adds a sub-action's whole batch to its action before it fingerprints any of it
and returns at the first error, exactly where raft_ref.bfs stops its counters.  n3_v1_e1_r3 also carries the
cumulative arrays after each level.  Every entry names the levels*.json entry of the same configuration,
whose totals the tests compare (tests/test_coverage_host.py).

Usage: python tests/golden/make_golden_coverage.py        (n5_v1_e1_r3 takes ~7 min, n3_v1_e2_r3 ~3 min)
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import raft_ref as R  # noqa: E402

NACT = len(R.ACTIONS)

# name -> (levels file holding the same configuration, Config keywords)
CONFIGS = {
    "n2_v1_e2_r3": ("levels.json", dict(n=2, V=1, max_election=2)),
    "n3_v1_e1_r3": ("levels.json", dict(n=3, V=1, max_election=1)),
    "n3_v2_e1_r3": ("levels.json", dict(n=3, V=2, max_election=1)),
    "n4_v1_e1_r3": ("levels.json", dict(n=4, V=1, max_election=1)),
    "n5_v1_e1_r3": ("levels.json", dict(n=5, V=1, max_election=1)),
    "n3_v1_e2_r3": ("levels.json", dict(n=3, V=1, max_election=2)),
    "bf_n3_v1_e1_r3": ("levels_bf.json", dict(n=3, V=1, max_election=1, become_follower=True)),
    "nosym_n3_v1_e1_r3": ("levels_variants.json", dict(n=3, V=1, max_election=1, symmetry=False)),
    "seeded_n3_v1_e2_r3": ("levels.json", dict(n=3, V=1, max_election=2, seeded=True)),
    "sb_n3_v1_e2_r3": ("levels_errors.json", dict(n=3, V=1, max_election=2, split_brain=True)),
    "deadlock_n3_v1_e1_r3": ("levels.json", dict(n=3, V=1, max_election=1, check_deadlock=True)),
    "cpl_n3_v2_e1_r3": ("levels_errors.json", dict(n=3, V=2, max_election=1, commit_past_log=True)),
}
PER_LEVEL = ("n3_v1_e1_r3",)

# spot values computed independently when the feature was specified
SPOT = {
    "n2_v1_e2_r3": dict(generated=[77, 75, 41, 41, 30, 124, 949, 26, 90, 134, 471, 0, 0],
                        distinct=[66, 50, 41, 36, 22, 118, 171, 26, 76, 86, 368, 0, 0]),
    "sb_n3_v1_e2_r3": dict(generated=[92, 244, 59, 53, 34, 84, 7, 0, 0, 0, 61, 0, 0],
                           distinct=[51, 129, 41, 22, 7, 14, 7, 0, 0, 0, 17, 0, 0]),
    "deadlock_n3_v1_e1_r3": dict(generated=[3, 44, 19, 3, 14, 30, 30, 0, 1, 0, 31, 0, 0]),
}


def cover_bfs(cfg):
    """raft_ref.bfs's search (TLC -workers 1 order) with the two per-action counters.  Returns (verdict,
    generated[NACT], distinct[NACT], per_level): per_level[k] = the cumulative pair after level k + 1 was
    expanded whole (no entry for a level an error stops in)."""
    gen, dist, per_level = [0] * NACT, [0] * NACT, []
    s0 = R.init_state(cfg)
    seen = {R.canonical(cfg, s0)}
    level = [s0]

    def bad(st):
        try:
            return "invariant" if any(not R.INV_FUNCS[i](cfg, st) for i in cfg.invariants) else None
        except R.EvalError:
            return "eval_error"

    if bad(s0):
        return bad(s0), gen, dist, per_level
    while level:
        nxt = []
        for st in level:
            n_succ = 0
            try:
                for _s, a, batch in R.successor_batches(cfg, st):
                    gen[a] += len(batch)  # the whole batch, before any of it is fingerprinted
                    n_succ += len(batch)
                    for _w, t in batch:
                        c = R.canonical(cfg, t)
                        if c in seen:
                            continue
                        seen.add(c)
                        dist[a] += 1
                        if bad(t):
                            return bad(t), gen, dist, per_level
                        nxt.append(t)
            except R.AssertionFailure:  # raised before the failing sub-action's batch is yielded
                return "assert", gen, dist, per_level
            if n_succ == 0 and cfg.check_deadlock:
                return "deadlock", gen, dist, per_level
        per_level.append(dict(generated=list(gen), distinct=list(dist)))
        level = nxt
    return "ok", gen, dist, per_level


def entry(name):
    src, kw = CONFIGS[name]
    cfg = R.Config(max_restart=3, **kw)
    verdict, gen, dist, per_level = cover_bfs(cfg)
    e = dict(levels_file=src, verdict=verdict, total_generated=1 + sum(gen), total_distinct=1 + sum(dist),
             generated=gen, distinct=dist)
    if name in PER_LEVEL:
        e["per_level"] = per_level
    for k, v in SPOT.get(name, {}).items():
        assert e[k] == v, (name, k, e[k], v)
    return name, e


def main():
    with ProcessPoolExecutor(max_workers=min(len(CONFIGS), os.cpu_count() or 1)) as ex:
        out = dict(ex.map(entry, CONFIGS))
    out = {name: out[name] for name in CONFIGS}
    for name, e in out.items():
        print(name, e["verdict"], e["total_generated"], e["total_distinct"], flush=True)
    with open(os.path.join(HERE, "coverage.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
