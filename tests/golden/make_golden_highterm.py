#!/usr/bin/env python3
"""High-term fixtures: MaxElection 4..7, MaxRestart up to 7 (and 0), MaxElection 0.

The packed codec, the message info word and the 16-bit message ids are sized for MaxElection 0..7 and
MaxRestart 0..15 (rmc_spec.h: the 3-bit currentTerm / electionCount / log-entry term, the 4-bit
restartCount, the 4-bit message term fields), but every other fixture stays at MaxElection <= 3 and
MaxRestart <= 3.  This script writes, from oracle/ alone:

* levels_highterm.json           per-level distinct / generated counts, depth and verdict (the format of
                                 levels.json), exhausted where the oracles can (`exhausted`), otherwise the
                                 levels the C oracle completes within `max_states` (the format of
                                 levels_prefix.json).  Small configurations by BOTH oracle/raft_ref.py and
                                 oracle/raft_oracle.c, which must agree; the rest by the C restatement.
* successors_highterm.json.gz    sampled walk states in successors_deep.json.gz's record format
                                 (make_golden_deep.state_record): successors in TLC order by both oracles, a
                                 server-permuted copy, canonical classes, the seven invariants.

The walk is make_golden_deep.walk with its weights turned around: that one spends elections late to
pile up messages, this one spends them, and Restart, early, so that terms, electionCount and
restartCount reach the top of their ranges; once a leader of term >= 4 exists, replication steps are
favoured so that log entries, prevLogTerm and lastLogTerm of term >= 4 appear.  Restart needs a Leader,
so restartCount <= electionCount <= 7: MaxRestart above 7 never binds, which is why these stop at 7.
Kept states are chosen by the coverage properties first (COVER), then at random; the conditions are
asserted here and the counts recorded in the fixture (tests/test_highterm_fixtures.py recomputes them).

Usage: python tests/golden/make_golden_highterm.py   (a few minutes; both files are reproduced byte for byte)
"""
import gzip
import json
import os
import random
import sys
import zlib
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import R, run_c, run_py  # noqa: E402
from make_golden_deep import c_lib, state_record, walk  # noqa: E402
from make_golden_prefix import run_prefix  # noqa: E402

# ---- levels_highterm.json -------------------------------------------------------------------------
BOTH = [(2, 1, 4, 3), (2, 1, 2, 0), (3, 1, 1, 0), (3, 2, 1, 0)]
E0 = [(2, 1, 0, 3), (3, 1, 0, 15)]          # empty message universe: Init alone, without and with deadlock checking
C_ONLY = [(2, 1, 5, 5)]
# the largest MaxElection each compiled (servers, values) pair admits under the 16-bit message ids
PREFIXES = [(2, 1, 7, 7, 400_000), (2, 2, 6, 3, 400_000), (3, 1, 7, 7, 400_000), (3, 2, 6, 3, 400_000),
            (3, 3, 4, 3, 400_000), (4, 1, 7, 3, 400_000), (4, 2, 5, 3, 300_000), (5, 1, 7, 3, 150_000),
            (5, 2, 4, 3, 100_000)]


def exhausted(spec):
    n, V, E, Rr, deadlock, both = spec
    c = run_c(n, V, E, Rr, deadlock=deadlock)
    src = "c"
    if both:
        _, p = run_py(n, V, E, Rr, deadlock=deadlock)
        assert (p.verdict, p.generated, p.distinct, p.depth, p.levels, p.generated_per_level) == (
            c["verdict"], c["generated"], c["distinct"], c["depth"], c["levels"], c["gen_per_level"]), spec
        assert (len(p.trace) if p.trace else 0) == c["trace_len"], spec
        src = "python+c"
        c.update(queue_left=p.queue_left, violated=p.violated)
    c.update(n=n, V=V, E=E, R=Rr, seeded=False, invariants=["Inv"], check_deadlock=deadlock, source=src,
             exhausted=True)
    return ("deadlock_" if deadlock else "") + f"n{n}_v{V}_e{E}_r{Rr}", c


def prefix(spec):
    n, V, E, Rr, max_states = spec
    r = run_prefix(n, V, E, Rr, max_states)
    del r["oracle_seconds"]  # (a time: the fixture is reproducible byte for byte)
    assert not r["exhausted"] and len(r["levels"]) >= 8
    return f"n{n}_v{V}_e{E}_r{Rr}", r


# ---- successors_highterm.json.gz ------------------------------------------------------------------
# (name, n, V, E, R, BecomeFollower variant, walk states kept, message lanes of the GPU layout)
CONFIGS = [
    ("n3_v1_e7_r7", 3, 1, 7, 7, False, 60, 64),
    ("n3_v2_e6_r6", 3, 2, 6, 6, False, 60, 64),
    ("n2_v2_e7_r7", 2, 2, 7, 7, False, 60, 64),
    ("n4_v1_e7_r7", 4, 1, 7, 7, False, 30, 128),
    ("n5_v1_e7_r7", 5, 1, 7, 7, False, 30, 128),
    ("bf_n3_v1_e7_r7", 3, 1, 7, 7, True, 60, 64),
]
WALKS = 150
STEPS = {2: 120, 3: 120, 4: 240, 5: 240}  # by servers: an election takes more steps with more voters
# property -> least number of kept states that must have it, for every configuration with E >= 6
COVER = [("append_req_prev_log_term_ge4", 1), ("vote_req_last_log_term_ge4", 1), ("restart_count_ge4", 5),
         ("current_term_top", 10), ("election_count_top", 10), ("log_term_ge4", 10), ("msg_term_ge4", 10)]


def properties(d, E):
    """The coverage properties of a state (JSON form, raft_ref.state_to_json)."""
    return dict(
        current_term_top=max(d["currentTerm"]) == E,
        election_count_top=d["electionCount"] == E,
        log_term_ge4=any(e[0] >= 4 for log in d["logs"] for e in log),
        restart_count_ge4=d["restartCount"] >= 4,
        msg_term_ge4=any(m["term"] >= 4 for m in d["msgs"]),
        append_req_prev_log_term_ge4=any(m["type"] == "AppendReq" and m["prevLogTerm"] >= 4 for m in d["msgs"]),
        vote_req_last_log_term_ge4=any(m["type"] == "VoteReq" and m["lastLogTerm"] >= 4 for m in d["msgs"]))


def coverage_counts(states, E):
    out = {name: 0 for name, _ in COVER}
    for d in states:
        for name, on in properties(d, E).items():
            out[name] += bool(on)
    out.update(max_current_term=max(max(d["currentTerm"]) for d in states),
               max_election_count=max(d["electionCount"] for d in states),
               max_restart_count=max(d["restartCount"] for d in states),
               max_log_term=max(e[0] for d in states for log in d["logs"] for e in log),
               max_msg_term=max([m["term"] for d in states for m in d["msgs"]] or [0]))
    return out


def weight(st, key, t):
    """BecomeCandidate 0.3 and Restart 2.0 against 1.0: elections and restarts are spent, not saved.
    Under a term >= 4 the replication steps weigh 3.0 (ClientReq, LeaderAppendEntry, FollowerAcceptEntry,
    HandleAppendResp), which is what puts term >= 4 into logs, prevLogTerm and lastLogTerm.  At 4 and 5
    servers a state has several times the successors, so Restart weighs 6.0 and BecomeLeader 3.0 there:
    without that no walk reaches restartCount 4."""
    a = key[1]
    many = len(st["currentTerm"]) >= 4
    if a == R.A_RS:
        return 6.0 if many else 2.0
    if a == R.A_BC:
        return 0.3
    if a == R.A_BL and many:
        return 3.0
    if max(st["currentTerm"]) >= 4 and a in (R.A_CR, R.A_LAE, R.A_FAE, R.A_HAR):
        return 3.0
    return 1.0


def one_config(spec):
    name, n, V, E, Rr, bf, keep, mcap = spec
    cfg = R.Config(n=n, V=V, max_election=E, max_restart=Rr, become_follower=bf)
    flags = 2 if bf else 0
    rng = random.Random(zlib.crc32(name.encode()) ^ 20261021)
    lib = c_lib()
    init = [R.state_to_json(R.init_state(cfg))]
    pool = [(k, d) for _ in range(WALKS)
            for k, d in enumerate(walk(lib, cfg, rng, init, STEPS[n], None, mcap, weight=weight, flags=flags)) if k]
    picked, seen = [], set()

    def take(k, d):
        c = R.canonical(cfg, R.state_from_json(d))
        if c in seen:
            return False
        seen.add(c)
        picked.append((k, d))
        return True

    # by the coverage properties first (the rarest first), then at random
    for prop, least in COVER:
        have = [x for x in pool if properties(x[1], E)[prop]]
        rng.shuffle(have)
        for k, d in have:
            if sum(1 for _, p in picked if properties(p, E)[prop]) >= least or len(picked) >= keep:
                break
            take(k, d)
    tries = 0
    while len(picked) < keep and tries < 50 * keep:
        tries += 1
        take(*rng.choice(pool))
    items, canon_ids, c_of_py = [], {}, {}
    for k, d in picked:
        items.append(state_record(lib, cfg, name, rng, k, R.state_from_json(d), canon_ids, c_of_py, flags=flags))
    cov = coverage_counts([it["state"] for it in items], E)
    if E >= 6:
        for prop, least in COVER:
            assert cov[prop] >= least, (name, prop, cov[prop], least)
    nm = [it["nmsgs"] for it in items]
    cov.update(states=len(items), successors=sum(len(it.get("successors", [])) for it in items),
               assert_states=sum(1 for it in items if it["assert_fails"]), min_msgs=min(nm), max_msgs=max(nm),
               max_depth=max(it["depth"] for it in items), pool_states=len(pool),
               become_follower_successors=sum(1 for it in items for s in it.get("successors", [])
                                              if s["key"][1] == R.A_BF),
               generator="tests/golden/make_golden_highterm.py (raft_ref.py + raft_oracle.c agree)")
    out = dict(n=n, V=V, E=E, R=Rr, become_follower=bf, msg_cap=mcap, items=items, coverage=cov)
    print(name, json.dumps(cov), flush=True)
    return name, out


def main():
    specs = [(n, V, E, Rr, False, True) for n, V, E, Rr in BOTH]
    specs += [(n, V, E, Rr, dl, True) for n, V, E, Rr in E0 for dl in (False, True)]
    specs += [(n, V, E, Rr, False, False) for n, V, E, Rr in C_ONLY]
    with ProcessPoolExecutor(max_workers=8) as ex:
        fl = [ex.submit(exhausted, s) for s in specs] + [ex.submit(prefix, s) for s in PREFIXES]
        fs = [ex.submit(one_config, s) for s in CONFIGS]
        levels = dict(f.result() for f in fl)
        succ = dict(f.result() for f in fs)
    for name, g in levels.items():
        print(name, "exhausted" if g["exhausted"] else f"prefix(max_states {g['max_states']})", "levels",
              len(g["levels"]), "states", sum(g["levels"]), g.get("verdict", ""), g["source"], flush=True)
    with open(os.path.join(HERE, "levels_highterm.json"), "w") as f:
        json.dump(levels, f, indent=1)
    # (no file name or time in the gzip header: the same bytes every run)
    with open(os.path.join(HERE, "successors_highterm.json.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(json.dumps(succ, separators=(",", ":")).encode())


if __name__ == "__main__":
    main()
