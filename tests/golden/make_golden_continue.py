#!/usr/bin/env python3
"""Golden fixture of continuation (rmc_set_continue; TLC's -continue): continue.json, from the Python
oracle (oracle/raft_ref.py) alone.

cont_bfs is raft_ref.bfs's loop (TLC -workers 1 order) with the break-and-go-on rule: per new state the
invariants are evaluated in cfg order up to the first FALSE one, the state is attributed to that invariant
and is enqueued like any other; an invariant after a FALSE one is not evaluated on that state.  Init is
checked the same way.  An evaluation error, UpdateTerm's Assert and a deadlock (deadlock checking on) stop
the search where raft_ref.bfs stops it, and the violation counts then cover exactly the states found up to
there (global ids below `distinct`).

Per entry: the verdict, generated, distinct, depth, and per invariant the count, the counts per level
(depth of them; [0] is Init's level), and the first violating state's global id, level and path from Init
as (server, action, witness) keys.  seeded_n3_v1_e2_r3 also carries its per-action coverage arrays (as
make_golden_coverage.py defines them).  `levels_file` names the levels*.json that holds a full exhaustion of
the same configuration, where there is one (tests/test_continue_host.py compares the counters).

Usage: python tests/golden/make_golden_continue.py        (seeded_n3_v1_e2_r3 takes ~5 min)
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

# name -> (levels file with a full exhaustion of the configuration or None, its key there, Config keywords)
CONFIGS = {
    "n2_v1_e2_r3": ("levels.json", "n2_v1_e2_r3",
                    dict(n=2, V=1, max_election=2, invariants=("RaftCanCommt", "FollowerCanCommit", "CommitAll"))),
    "n3_v1_e2_r3": ("levels.json", "n3_v1_e2_r3",
                    dict(n=3, V=1, max_election=2, invariants=("RaftCanCommt", "FollowerCanCommit", "Inv"))),
    "n3_v1_e2_r3_b": ("levels.json", "n3_v1_e2_r3",
                      dict(n=3, V=1, max_election=2, invariants=("Inv", "NoSplitVote", "ExistLeaderAndCandidate"))),
    "n4_v1_e1_r3": ("levels.json", "n4_v1_e1_r3",
                    dict(n=4, V=1, max_election=1, invariants=("FollowerCanCommit", "NoAllCommit"))),
    "n3_v2_e1_r3": ("levels.json", "n3_v2_e1_r3",
                    dict(n=3, V=2, max_election=1,
                         invariants=("NoSplitVote", "RaftCanCommt", "NoAllCommit", "CommitAll"))),
    "bf_n3_v1_e1_r3": ("levels_bf.json", "bf_n3_v1_e1_r3",
                       dict(n=3, V=1, max_election=1, become_follower=True,
                            invariants=("RaftCanCommt", "FollowerCanCommit"))),
    "seeded_n3_v1_e2_r3": (None, None, dict(n=3, V=1, max_election=2, seeded=True, invariants=("Inv",))),
    "sb_n3_v1_e3_r3": (None, None, dict(n=3, V=1, max_election=3, split_brain=True, invariants=("Inv", "NoSplitVote"))),
    "cpl_n3_v2_e1_r3": (None, None, dict(n=3, V=2, max_election=1, commit_past_log=True,
                                         invariants=("RaftCanCommt", "Inv"))),
    "deadlock_n3_v1_e1_r3": (None, None, dict(n=3, V=1, max_election=1, check_deadlock=True,
                                              invariants=("FollowerCanCommit",))),
    # (not in the issue's table: a stopping entry whose counted invariant reads msgs, for the cut on the sharded paths)
    "cpl_nac_n3_v2_e1_r3": (None, None, dict(n=3, V=2, max_election=1, commit_past_log=True,
                                             invariants=("Inv", "NoAllCommit"))),
}
COVERAGE = ("seeded_n3_v1_e2_r3",)

# spot values computed independently when the feature was specified:
# (verdict, generated, distinct, depth), {invariant: (count, first global id or None, first level or None)}
SPOT = {
    "n2_v1_e2_r3": (("ok", 2059, 1061, 23),
                    {"RaftCanCommt": (355, 0, 1), "FollowerCanCommit": (210, 28, 7), "CommitAll": (496, 52, 8)}),
    "n3_v1_e2_r3": (("ok", 936730, 223437, 37),
                    {"RaftCanCommt": (54113, 0, 1), "FollowerCanCommit": (27166, 686, 10), "Inv": (0, None, None)}),
    "n3_v1_e2_r3_b": (("ok", 936730, 223437, 37),
                      {"Inv": (0, None, None), "NoSplitVote": (0, None, None),
                       "ExistLeaderAndCandidate": (221961, 0, 1)}),
    "n4_v1_e1_r3": (("ok", 17319, 3323, 27), {"FollowerCanCommit": (1303, 0, 1), "NoAllCommit": (2020, 240, 13)}),
    "n3_v2_e1_r3": (("ok", 54433, 10501, 28),
                    {"NoSplitVote": (0, None, None), "RaftCanCommt": (1321, 0, 1), "NoAllCommit": (9180, 203, 10),
                     "CommitAll": (0, None, None)}),
    "bf_n3_v1_e1_r3": (("ok", 2177, 545, 20), {"RaftCanCommt": (245, 0, 1), "FollowerCanCommit": (81, 97, 10)}),
    "seeded_n3_v1_e2_r3": (("ok", 1871481, 456319, 37), {"Inv": (1125, 3455, 12)}),
    "sb_n3_v1_e3_r3": (("assert", 1219, 541, 7), {"Inv": (0, None, None), "NoSplitVote": (16, 55, 5)}),
    "cpl_n3_v2_e1_r3": (("eval_error", 8435, 2615, 17), {"RaftCanCommt": (1086, 0, 1), "Inv": (0, None, None)}),
    "deadlock_n3_v1_e1_r3": (("deadlock", 176, 88, 9), {"FollowerCanCommit": (88, 0, 1)}),
}


def cont_bfs(cfg):
    """Returns (verdict, generated, distinct, depth, viol, gen[NACT], dist[NACT]); viol[name] = dict(count,
    per_level (one entry per level that holds a state), first_gid, first_level, first_path)."""
    names = list(cfg.invariants)
    parent, keys, level_of = [-1], [None], [1]
    viol = {nm: dict(count=0, per_level=[], first_gid=None, first_level=None) for nm in names}
    gen, dist = [0] * NACT, [0] * NACT

    def check(st, gid, lvl):
        """The first FALSE invariant in cfg order is counted (the later ones are not evaluated); raises
        R.EvalError as the invariant does."""
        for nm in names:
            if not R.INV_FUNCS[nm](cfg, st):
                v = viol[nm]
                v["count"] += 1
                while len(v["per_level"]) < lvl:
                    v["per_level"].append(0)
                v["per_level"][lvl - 1] += 1
                if v["first_gid"] is None:
                    v["first_gid"], v["first_level"] = gid, lvl
                return

    def finish(verdict, generated, depth):
        for v in viol.values():
            v["per_level"] += [0] * (depth - len(v["per_level"]))
            assert len(v["per_level"]) == depth and sum(v["per_level"]) == v["count"]
            path, i = [], v["first_gid"]
            while i is not None and parent[i] >= 0:
                path.append(list(keys[i]))
                i = parent[i]
            v["first_path"] = list(reversed(path)) if v["first_gid"] is not None else None
        return verdict, generated, len(parent), depth, viol, gen, dist

    s0 = R.init_state(cfg)
    seen = {R.canonical(cfg, s0)}
    generated = 1
    try:
        check(s0, 0, 1)
    except R.EvalError:
        return finish("eval_error", generated, 1)
    level, lvl = [(0, s0)], 1
    while level:
        nxt = []
        for i, st in level:
            n_succ = 0
            try:
                for s, a, batch in R.successor_batches(cfg, st):
                    generated += len(batch)  # the whole batch, before any of it is fingerprinted
                    gen[a] += len(batch)
                    n_succ += len(batch)
                    for w, t in batch:
                        c = R.canonical(cfg, t)
                        if c in seen:
                            continue
                        seen.add(c)
                        j = len(parent)
                        parent.append(i)
                        keys.append((s, a, w))
                        level_of.append(lvl + 1)
                        dist[a] += 1
                        try:
                            check(t, j, lvl + 1)
                        except R.EvalError:
                            return finish("eval_error", generated, lvl + 1)
                        nxt.append((j, t))
            except R.AssertionFailure:  # raised before the failing sub-action's batch is yielded
                return finish("assert", generated, max(level_of))
            if n_succ == 0 and cfg.check_deadlock:
                return finish("deadlock", generated, max(level_of))
        level = nxt
        lvl += 1
    return finish("ok", generated, max(level_of))


def entry(name):
    src, key, kw = CONFIGS[name]
    cfg = R.Config(max_restart=3, **kw)
    verdict, generated, distinct, depth, viol, gen, dist = cont_bfs(cfg)
    e = dict(levels_file=src, levels_key=key, config={k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()},
             invariants=list(cfg.invariants), verdict=verdict, generated=generated, distinct=distinct, depth=depth,
             violations=viol)
    if name in COVERAGE:
        e["coverage"] = dict(generated=gen, distinct=dist)
    assert 1 + sum(gen) == generated and 1 + sum(dist) == distinct
    if name not in SPOT:
        return name, e
    head, per_inv = SPOT[name]
    assert (verdict, generated, distinct, depth) == head, (name, verdict, generated, distinct, depth, head)
    for nm, want in per_inv.items():
        v = viol[nm]
        assert (v["count"], v["first_gid"], v["first_level"]) == want, (name, nm, v["count"], v["first_gid"],
                                                                         v["first_level"], want)
    return name, e


def main():
    with ProcessPoolExecutor(max_workers=min(len(CONFIGS), os.cpu_count() or 1)) as ex:
        out = dict(ex.map(entry, CONFIGS))
    out = {name: out[name] for name in CONFIGS}
    for name, e in out.items():
        print(name, e["verdict"], e["generated"], e["distinct"], e["depth"],
              {nm: (v["count"], v["first_gid"], v["first_level"]) for nm, v in e["violations"].items()}, flush=True)
    with open(os.path.join(HERE, "continue.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
