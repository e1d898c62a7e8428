#!/usr/bin/env python3
"""Golden fixture for counting the VIEW's classes among the states of a whole-state search (DESIGN.md section 18:
does the cfg's VIEW lose a class, and is each class found at its shortest depth): viewclasses.json, from the
Python oracle alone through tests/fullstate_ref.py.  It is the reference a count on the device is to be held to.

Per run: the whole-state search's states grouped by their VIEW class (raft_ref.canonical under the run's
SYMMETRY setting) -- `classes`, `class_levels` (the classes first met at each level), `size_hist` (32 bins:
[k], k < 31, the classes of k + 1 states, [31] the larger ones), `largest`, `states` -- and `sample`: about 50
states with their class's `members` and `first_level`.

A: fullstate.json's finished runs at 2 servers, Init as the root (the entry's name is fullstate.json's).
B, C: the smallest of them from two roots, [Init with restartCount = MaxRestart, Init] and [Init with
electionCount = MaxElection, Init], through a seeded search of this file's own: the first root of each
identity in argument order is kept, as rmc_init_from defines, then raft_ref.bfs's order.  The VIEW search
keeps the spent copy alone; `view` holds its counters and levels, `roots` the root states, `absent` a
state of no reached class.

Usage: python tests/golden/make_golden_viewclasses.py        (under a minute on 8 cores)
"""
import json
import os
import random
import sys
from collections import deque
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fullstate_ref as F  # noqa: E402
import raft_ref as R  # noqa: E402

BINS = 32
SAMPLE = 50
SMALL = dict(n=2, V=1, max_election=2, max_restart=2)


def seeded_bfs(cfg, roots):
    """(states, level of each, generated): breadth-first from the kept roots (the first of each identity under
    cfg, in argument order), successors in raft_ref's order, first discovery wins.  `generated` counts every
    given root and every successor, as the engine's counter does."""
    seen, states, level = set(), [], []
    for st in roots:
        c = F.canonical(cfg, st)
        if c not in seen:
            seen.add(c)
            states.append(st)
            level.append(1)
    generated = len(roots)
    queue = deque(range(len(states)))
    while queue:
        i = queue.popleft()
        for _, t in R.successors(cfg, states[i]):
            generated += 1
            c = F.canonical(cfg, t)
            if c not in seen:
                seen.add(c)
                states.append(t)
                level.append(level[i] + 1)
                queue.append(len(states) - 1)
    return states, level, generated


def levels_of(level):
    out = [0] * max(level)
    for lv in level:
        out[lv - 1] += 1
    return out


def classes_of(cfg, states, level, seed):
    """The fixture's fields for a whole-state run's states (BFS order) and their levels."""
    vcfg = R.Config(**{**cfg.__dict__, "view": True})
    members, first = {}, {}
    keys = [R.canonical(vcfg, st) for st in states]
    for k, lv in zip(keys, level):
        members[k] = members.get(k, 0) + 1
        first.setdefault(k, lv)  # (BFS order: the first member met has the smallest level)
    assert all(first[k] <= lv for k, lv in zip(keys, level))
    class_levels = [0] * max(level)
    for lv in first.values():
        class_levels[lv - 1] += 1
    hist = [0] * BINS
    for m in members.values():
        hist[min(m, BINS) - 1] += 1
    rng = random.Random(seed)
    idx = sorted(set([0, len(states) - 1] + rng.sample(range(len(states)), min(SAMPLE, len(states)))))
    # (among them a member of a largest class)
    big = max(members.values())
    idx = sorted(set(idx + [next(i for i, k in enumerate(keys) if members[k] == big)]))
    sample = [dict(state=R.state_to_json(states[i]), members=members[keys[i]], first_level=first[keys[i]]) for i in idx]
    out = dict(states=len(states), classes=len(members), class_levels=class_levels, size_hist=hist, largest=big,
               levels=levels_of(level), sample=sample)
    assert sum(hist) == out["classes"] == sum(class_levels) and sum(members.values()) == out["states"]
    return out, set(members)


def run_a(item):
    name, g = item
    kw = dict(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"], symmetry=g["symmetry"],
              become_follower=g["become_follower"])
    cfg = R.Config(view=False, **kw)
    r = F.bfs(cfg, keep_states=True)
    assert r.verdict == "ok" and (r.distinct, r.generated, r.levels) == (g["distinct"], g["generated"], g["levels"])
    level = [lv + 1 for lv, k in enumerate(r.levels) for _ in range(k)]
    e, _ = classes_of(cfg, r.states, level, seed=7)
    assert e["classes"] == g["view_classes"]
    e["config"] = kw
    return name, e


def run_roots(tag):
    cfg, vcfg = R.Config(view=False, **SMALL), R.Config(view=True, **SMALL)
    init = R.init_state(cfg)
    spent = (R.State(**{**init.__dict__, "restartCount": cfg.max_restart}) if tag == "B" else
             R.State(**{**init.__dict__, "electionCount": cfg.max_election}))
    roots = [spent, init]
    states, level, generated = seeded_bfs(cfg, roots)
    e, keys = classes_of(cfg, states, level, seed=13)
    vs, vl, vg = seeded_bfs(vcfg, roots)
    e["generated"] = generated
    e["view"] = dict(distinct=len(vs), generated=vg, levels=levels_of(vl))
    e["config"] = SMALL
    e["roots"] = [R.state_to_json(st) for st in roots]
    # a state of no reached class: Init with every commitIndex one past its log's only entry
    ghost = R.State(**{**init.__dict__, "commitIndex": tuple(c + 1 for c in init.commitIndex)})
    assert R.canonical(vcfg, ghost) not in keys
    e["absent"] = R.state_to_json(ghost)
    return tag, e


def main():
    with open(os.path.join(HERE, "fullstate.json")) as f:
        full = json.load(f)
    a_items = [(k, g) for k, g in sorted(full.items()) if g["verdict"] == "ok" and g["n"] == 2]
    with ProcessPoolExecutor(max_workers=min(len(a_items) + 2, os.cpu_count() or 1)) as ex:
        fa = ex.map(run_a, a_items)
        fr = ex.map(run_roots, ["B", "C"])
        out = dict(A=dict(fa), **dict(fr))
    for name, e in list(out["A"].items()) + [("B", out["B"]), ("C", out["C"])]:
        print(name, f"{e['states']} states in {e['classes']} classes, largest {e['largest']},",
              "sizes", [x for x in e["size_hist"] if x], "firsts", e["class_levels"][:10],
              ("VIEW " + str(e["view"]["distinct"]) + " / " + str(e["view"]["generated"]) + " levels " +
               str(e["view"]["levels"][:10]) + f", generated {e['generated']}") if "view" in e else "", flush=True)
    with open(os.path.join(HERE, "viewclasses.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
