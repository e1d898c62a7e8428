#!/usr/bin/env python3
"""Golden fixture of the whole-state search (ModelConfig(view=False), rmc_set_full_state; raftmc
-fullstate): fullstate.json, from the Python oracle alone through tests/fullstate_ref.py, whose identity
is the whole state (its SYMMETRY orbit minimum, pendingResponse permuted on both indices).

Per entry: the configuration, levels, generated per level, depth, verdict, the counters at an error and
the counterexample (levels.json's / traces.json's fields), `view`: the same run under the cfg's VIEW
(raft_ref.bfs unchanged) -- every entry differs from its twin --, and for a finished run `view_classes`:
how many VIEW classes its states fall into (equal to the twin's distinct count when the VIEW hid no
class).  The deadlock and BecomeFollower entries are the first of CANDIDATES whose whole-state run differs
from its VIEW twin.  On the smallest entry also: per-action coverage (make_golden_coverage.cover_bfs), the
whole-state graph's edges with RaftCanCommt per state; on the seeded configuration the per-invariant
counts of a run that continues past violations (make_golden_continue.cont_bfs).

Usage: python tests/golden/make_golden_fullstate.py        (about six minutes on 8 cores)
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import fullstate_ref as F  # noqa: E402
import raft_ref as R  # noqa: E402
from make_golden_continue import cont_bfs  # noqa: E402
from make_golden_coverage import cover_bfs  # noqa: E402

# name -> Config keywords (max_restart included)
CONFIGS = {
    "sym_n2_v1_e2_r2": dict(n=2, V=1, max_election=2, max_restart=2),
    "sym_n2_v2_e2_r2": dict(n=2, V=2, max_election=2, max_restart=2),
    "nosym_n2_v1_e2_r2": dict(n=2, V=1, max_election=2, max_restart=2, symmetry=False),
    "nosym_n2_v2_e2_r2": dict(n=2, V=2, max_election=2, max_restart=2, symmetry=False),
    "sym_n3_v1_e2_r1": dict(n=3, V=1, max_election=2, max_restart=1),
    "seeded_n3_v1_e2_r1": dict(n=3, V=1, max_election=2, max_restart=1, seeded=True),
}
# smallest first: (n, V, E, R)
CANDIDATES = [(2, 1, 2, 1), (2, 1, 2, 2), (2, 2, 2, 1), (2, 2, 2, 2), (2, 1, 3, 1), (2, 1, 3, 2), (3, 1, 2, 1)]
SMALL = "sym_n2_v1_e2_r2"
SEEDED = "seeded_n3_v1_e2_r1"


def summary(r):
    out = dict(verdict=r.verdict, generated=r.generated, distinct=r.distinct, depth=r.depth, levels=r.levels,
               gen_per_level=r.generated_per_level, trace_len=len(r.trace) if r.trace else 0,
               queue_left=r.queue_left)
    if r.verdict == "invariant":
        out["violated"] = r.violated
    return out


def run(kw):
    """The whole-state run and its VIEW twin as one entry."""
    cfg = R.Config(view=False, **kw)
    vcfg = R.Config(view=True, **kw)
    r = F.bfs(cfg, keep_states=True)
    e = summary(r)
    e.update(n=cfg.n, V=cfg.V, E=cfg.max_election, R=cfg.max_restart, seeded=cfg.seeded,
             become_follower=cfg.become_follower, symmetry=cfg.symmetry, invariants=list(cfg.invariants),
             check_deadlock=cfg.check_deadlock)
    if r.trace:
        e["steps"] = [dict(key=list(k) if k else None, state=R.state_to_json(st)) for k, st in r.trace]
    e["view"] = summary(R.bfs(vcfg))
    if r.verdict == "ok":
        e["view_classes"] = F.view_classes(cfg, r.states)
    return e, (cfg, r)


def differs(e):
    v = e["view"]
    return (e["generated"], e["distinct"], e["levels"]) != (v["generated"], v["distinct"], v["levels"])


def entry(name):
    e, (cfg, r) = run(CONFIGS[name])
    if name == SMALL:
        with F._identity():
            verdict, gen, dist, _ = cover_bfs(cfg)
        assert verdict == "ok" and 1 + sum(gen) == e["generated"] and 1 + sum(dist) == e["distinct"]
        e["coverage"] = dict(generated=gen, distinct=dist)
        gid = {F.canonical(cfg, st): i for i, st in enumerate(r.states)}
        src, dst = [], []
        for i, st in enumerate(r.states):
            for _, t in R.successors(cfg, st):
                src.append(i)
                dst.append(gid[F.canonical(cfg, t)])
        assert len(src) == e["generated"] - 1
        e["graph"] = dict(states=len(r.states), edges=len(src), self_edges=sum(a == b for a, b in zip(src, dst)),
                          src=src, dst=dst,
                          raft_can_commit=[int(R.INV_FUNCS["RaftCanCommt"](cfg, st)) for st in r.states])
    if name == SEEDED:
        with F._identity():
            verdict, generated, distinct, depth, viol, _, _ = cont_bfs(cfg)
        e["continue"] = dict(verdict=verdict, generated=generated, distinct=distinct, depth=depth,
                             violations={nm: dict(count=v["count"], first_level=v["first_level"])
                                         for nm, v in viol.items()})
    return name, e


def first_that_differs(tag):
    """The smallest of CANDIDATES whose whole-state run differs from its VIEW twin, with deadlock checking
    on (tag "deadlock") or BecomeFollower uncommented (tag "bf")."""
    extra = dict(check_deadlock=True) if tag == "deadlock" else dict(become_follower=True)
    for n, V, E, Rr in CANDIDATES:
        e, _ = run(dict(n=n, V=V, max_election=E, max_restart=Rr, **extra))
        if differs(e):
            return f"{tag}_n{n}_v{V}_e{E}_r{Rr}", e
    raise AssertionError(f"no candidate differs from its VIEW twin ({tag})")


def job(name):
    return first_that_differs(name) if name in ("deadlock", "bf") else entry(name)


def main():
    names = list(CONFIGS) + ["deadlock", "bf"]
    with ProcessPoolExecutor(max_workers=min(len(names), os.cpu_count() or 1)) as ex:
        out = dict(ex.map(job, names))
    for name, e in out.items():
        assert differs(e), name
        v = e["view"]
        print(name, e["verdict"], f"{e['distinct']} / {e['generated']} / {e['depth']}",
              f"VIEW {v['distinct']} / {v['generated']} / {v['depth']}", "view classes", e.get("view_classes"),
              flush=True)
    with open(os.path.join(HERE, "fullstate.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
