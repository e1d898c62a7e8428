#!/usr/bin/env python3
"""Golden fixtures for the kernel variants the Raft.cfg family of fixtures never launches
(tests/test_gpu_variants.py), from the oracles as make_golden.py / make_golden_bf.py do:

* levels_variants.json
    nosym_*          a cfg without the SYMMETRY line (Raft.cfg:24 removed; rmc_config.no_symmetry): the
                     canonical form is the view under the identity permutation alone.  Computed by BOTH
                     oracle/raft_ref.py (Config(symmetry=False)) and oracle/raft_oracle.c
                     (orc_set_symmetry(h, 0)), which must agree level by level.
    n4_v2_e1_r3      two values at four servers, exhausted by the C oracle;
    n5_v2_e1_r3      two values at five servers: the levels oracle/raft_mt.c completes up to the first
                     level boundary past PREFIX_STATES states (make_golden_prefix.run_prefix_mt);
    bf_n4_v2_e1_r3, bf_n5_v2_e1_r3
                     their BecomeFollower twins (Raft.tla:420 uncommented): the complete levels of a
                     C-oracle run stopped at PREFIX_STATES states.
* traces_variants.json      counterexamples of the nosym_* error runs (Python oracle; the C oracle's
                            trace length must agree).
* successors_variants.json.gz  (4,2) and (5,2): states sampled from a Python BFS capped at a state budget
                            (random ones plus the last few), their successors in TLC order -- Python and
                            C (orc_successors) agreeing --, a server-permuted copy, canonical class ids.

Usage: python tests/golden/make_golden_variants.py   (about five minutes on 8 cores)
"""
import ctypes
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import INV_BIT, R, VERDICTS, c_oracle  # noqa: E402
from make_golden_deep import c_lib, c_successors  # noqa: E402
from make_golden_prefix import run_prefix_mt  # noqa: E402

PREFIX_STATES = 200_000
MT_THREADS = 16
# the totals the Python oracle gives without SYMMETRY (distinct, generated, depth): the generator must
# reproduce them
NOSYM_TOTALS = {
    "nosym_n3_v1_e1_r3": (3172, 11860, 20),
    "nosym_n2_v1_e2_r3": (2120, 4115, 23),
    "nosym_n3_v2_e1_r3": (62434, 323836, 28),
    "nosym_n4_v1_e1_r3": (71333, 373045, 27),
}


def run_c(n, V, E, Rr, flags=0, invs=("Inv",), deadlock=False, symmetry=True, max_states=0):
    """oracle/raft_oracle.c; flags: bit 0 RaftSeeded, bit 1 BecomeFollower.  With max_states the run
    stops inside a level: only the complete levels are kept (as make_golden_prefix.run_prefix)."""
    lib = c_oracle()
    lib.orc_set_symmetry.argtypes = [ctypes.c_void_p, ctypes.c_int]
    mask = 0
    for i in invs:
        mask |= 1 << INV_BIT[i]
    h = lib.orc_create(n, V, E, Rr, flags, int(deadlock), mask, 0 if max_states else 1)
    lib.orc_set_symmetry(h, int(symmetry))
    v = lib.orc_run(h, max_states)
    d = (ctypes.c_uint64 * 1024)()
    g = (ctypes.c_uint64 * 1024)()
    L = lib.orc_levels(h, d, g, 1024)
    if max_states and v != 0:
        assert v == 5, v  # V_LIMIT: levels 1..L-1 discovered, 1..L-2 expanded
        out = dict(prefix=True, max_states=max_states, stopped_at_distinct=lib.orc_distinct(h),
                   levels=list(d[:L - 1]), gen_per_level=list(g[:L - 2]), max_msgs=lib.orc_max_msgs(h))
    else:
        out = dict(verdict=VERDICTS[v], generated=lib.orc_generated(h), distinct=lib.orc_distinct(h),
                   depth=lib.orc_depth(h), levels=list(d[:L]), gen_per_level=list(g[:L]),
                   max_msgs=lib.orc_max_msgs(h), trace_len=lib.orc_trace_len(h), queue_left=lib.orc_queue_left(h))
    lib.orc_destroy(h)
    return out


def permuted_copy(rng, st, n):
    """A concrete state of st's symmetry class under a random server permutation (hidden variables too)."""
    perm = list(range(n))
    rng.shuffle(perm)
    pv = R.permute_view(st.view(), perm)
    inv = [0] * n
    for a in range(n):
        inv[perm[a]] = a
    return R.State(votedFor=pv[0], currentTerm=pv[1], logs=pv[2], matchIndex=pv[3], nextIndex=pv[4],
                   commitIndex=pv[5], msgs=frozenset(pv[6]), role=pv[7], electionCount=st.electionCount,
                   restartCount=st.restartCount,
                   pendingResponse=tuple(tuple(st.pendingResponse[inv[a]][inv[b]] for b in range(n))
                                         for a in range(n)),
                   valSent=st.valSent)


def capped_bfs(cfg, max_states):
    """raft_ref's BFS (TLC order, first discovery wins) stopped at max_states distinct states."""
    s0 = R.init_state(cfg)
    seen = {R.canonical(cfg, s0)}
    states, lvls, head = [s0], [1], 0
    while head < len(states) and len(states) < max_states:
        st, lv = states[head], lvls[head]
        head += 1
        for _, t in R.successors(cfg, st):
            c = R.canonical(cfg, t)
            if c not in seen:
                seen.add(c)
                states.append(t)
                lvls.append(lv + 1)
    return states, lvls


def main():
    levels, traces = {}, {}

    # ------------------------------------------------------------ no SYMMETRY
    nosym = [("nosym_n3_v1_e1_r3", (3, 1, 1, 3), {}), ("nosym_n2_v1_e2_r3", (2, 1, 2, 3), {}),
             ("nosym_n3_v2_e1_r3", (3, 2, 1, 3), {}), ("nosym_n4_v1_e1_r3", (4, 1, 1, 3), {}),
             ("nosym_seeded_n3_v2_e2_r3", (3, 2, 2, 3), dict(seeded=True)),
             ("nosym_deadlock_n3_v1_e1_r3", (3, 1, 1, 3), dict(deadlock=True))]
    for name, (n, V, E, Rr), kw in nosym:
        seeded, deadlock = kw.get("seeded", False), kw.get("deadlock", False)
        c = run_c(n, V, E, Rr, flags=int(seeded), deadlock=deadlock, symmetry=False)
        p = R.bfs(R.Config(n=n, V=V, max_election=E, max_restart=Rr, seeded=seeded, check_deadlock=deadlock,
                           symmetry=False))
        assert (p.verdict, p.generated, p.distinct, p.depth) == (c["verdict"], c["generated"], c["distinct"],
                                                                 c["depth"]), name
        if p.verdict == "ok":
            assert (p.levels, p.generated_per_level) == (c["levels"], c["gen_per_level"]), name
            assert (p.distinct, p.generated, p.depth) == NOSYM_TOTALS[name], name
        else:
            assert p.levels[:-1] == c["levels"][:len(p.levels) - 1], name
        assert (len(p.trace) if p.trace else 0) == c["trace_len"], name
        c.update(n=n, V=V, E=E, R=Rr, seeded=seeded, symmetry=False, invariants=["Inv"], check_deadlock=deadlock,
                 source="python+c", queue_left=p.queue_left, violated=p.violated)
        if p.trace:
            traces[name] = dict(verdict=p.verdict, violated=p.violated,
                                steps=[dict(key=list(k) if k else None, state=R.state_to_json(s))
                                       for k, s in p.trace])
        levels[name] = c
        print(name, c["verdict"], c["distinct"], c["generated"], c["depth"], flush=True)

    # ------------------------------------------------------------ two values at 4 and 5 servers
    c = run_c(4, 2, 1, 3)
    c.update(n=4, V=2, E=1, R=3, seeded=False, invariants=["Inv"], check_deadlock=False, source="c")
    levels["n4_v2_e1_r3"] = c
    print("n4_v2_e1_r3", c["verdict"], c["distinct"], c["generated"], c["depth"], c["max_msgs"], flush=True)
    r = run_prefix_mt(5, 2, 1, 3, PREFIX_STATES, MT_THREADS)
    del r["oracle_seconds"]
    r.update(prefix=True, seeded=False)
    levels["n5_v2_e1_r3"] = r
    print("n5_v2_e1_r3 prefix", len(r["levels"]), sum(r["levels"]), flush=True)
    for n in (4, 5):
        name = f"bf_n{n}_v2_e1_r3"
        c = run_c(n, 2, 1, 3, flags=2, max_states=PREFIX_STATES)
        c.update(n=n, V=2, E=1, R=3, seeded=False, become_follower=True, invariants=["Inv"], check_deadlock=False,
                 source="c")
        levels[name] = c
        print(name, "prefix" if c.get("prefix") else c["verdict"], len(c["levels"]), sum(c["levels"]), flush=True)
    # the symmetric prefix of n5_v2 by the single-threaded oracle too: the two C drivers must agree
    c = run_c(5, 2, 1, 3, max_states=PREFIX_STATES)
    k = min(len(c["levels"]), len(r["levels"]))
    assert c["levels"][:k] == r["levels"][:k] and k >= len(r["levels"]) - 1
    k = min(len(c["gen_per_level"]), len(r["gen_per_level"]))
    assert c["gen_per_level"][:k] == r["gen_per_level"][:k]

    with open(os.path.join(HERE, "levels_variants.json"), "w") as f:  # a configuration per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in levels.items()) + "\n}\n")
    with open(os.path.join(HERE, "traces_variants.json"), "w") as f:
        json.dump(traces, f)

    # ------------------------------------------------------------ successor samples at (4,2), (5,2)
    rng = random.Random(20261020)
    lib = c_lib()
    samples = {}
    for (n, V, E, Rr, budget, k) in [(4, 2, 1, 3, 4000, 20), (5, 2, 1, 3, 2500, 20)]:
        cfg = R.Config(n=n, V=V, max_election=E, max_restart=Rr)
        states, lvls = capped_bfs(cfg, budget)
        picks = rng.sample(range(len(states) - 5), k) + list(range(len(states) - 5, len(states)))
        items = []
        for i in picks:
            st = states[i]
            succ = R.successors(cfg, st)
            cnt, csucc = c_successors(lib, cfg, R.state_to_json(st))
            assert cnt == len(succ), (n, V, i)
            assert [(list(kk), R.state_to_json(t)) for kk, t in succ] == [(kk, t) for kk, t in csucc], (n, V, i)
            pst = permuted_copy(rng, st, n)
            assert R.canonical(cfg, pst) == R.canonical(cfg, st)
            items.append(dict(level=lvls[i], state=R.state_to_json(st), permuted=R.state_to_json(pst),
                              successors=[dict(key=list(kk), state=R.state_to_json(t)) for kk, t in succ]))
        canon_ids = {}
        for it in items:
            for sc in it["successors"]:
                c = R.canonical(cfg, R.state_from_json(sc["state"]))
                sc["canon"] = canon_ids.setdefault(c, len(canon_ids))
        samples[f"n{n}_v{V}_e{E}_r{Rr}"] = dict(n=n, V=V, E=E, R=Rr, bfs_states=len(states), items=items)
        print("samples", n, V, len(items), sum(len(it["successors"]) for it in items),
              max(len(it["state"]["msgs"]) for it in items), flush=True)
    # gzipped like successors_deep.json.gz: ~600 KB of JSON on one line otherwise
    with gzip.GzipFile(os.path.join(HERE, "successors_variants.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(samples, separators=(",", ":")).encode())


if __name__ == "__main__":
    main()
