"""Simulation mode (rmc_simulate, TLC's -simulate) against the oracle: every walk is replayed at test
time on oracle/raft_ref.py with R.successors, R.INV_FUNCS and raftmc.sim_choice, so lengths, step keys,
counters, the error reported and its behaviour must match bit for bit."""
import functools
import json
import os
import subprocess

import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

VARIANT = {"seeded": raftmc.SPEC_SEEDED, "split_brain": raftmc.SPEC_SPLIT_BRAIN,
           "become_follower": raftmc.SPEC_BECOME_FOLLOWER}
STATUS = {"invariant": "invariant", "eval_error": "eval_error", "assert": "assert", "deadlock": "deadlock"}


def oracle_walks(cfg, num_walks, depth, seed, stop_at_error=True):
    """include/rmc.h's semantics on the CPU oracle.  Returns (walks, err): walks[w] = dict(len, gen, keys,
    end, states) with end one of "depth", "stuck", or an error ("deadlock", "assert", ("invariant", name),
    ("eval_error", name)); err = index of the first erring walk or None.  With stop_at_error the walks
    after it are not run."""
    def check(st):
        for name in cfg.invariants:
            try:
                if not R.INV_FUNCS[name](cfg, st):
                    return ("invariant", name)
            except R.EvalError:
                return ("eval_error", name)
        return None

    init = R.init_state(cfg)
    bad = check(init)
    if bad:  # an error at Init is walk 0, length 1
        return [dict(len=1, gen=0, keys=[], end=bad, states=[init])], 0
    walks, err = [], None
    for w in range(num_walks):
        st, keys, gen, end, states = init, [], 0, "depth", [init]
        while len(states) < depth:
            try:
                succ = R.successors(cfg, st)
            except R.AssertionFailure:
                end = "assert"
                break
            if not succ:
                end = "deadlock" if cfg.check_deadlock else "stuck"
                break
            gen += len(succ)
            key, st = succ[raftmc.sim_choice(seed, w, len(states) - 1, len(succ))]
            keys.append(key)
            states.append(st)
            bad = check(st)
            if bad:
                end = bad
                break
        walks.append(dict(len=len(states), gen=gen, keys=keys, end=end, states=states))
        if end not in ("depth", "stuck") and err is None:
            err = w
            if stop_at_error:
                break
    return walks, err


def make(n, V, E, Rr, variant=None, invariants=("Inv",), check_deadlock=False, **kw):
    """The oracle's Config and a checker of the same model."""
    ocfg = R.Config(n=n, V=V, max_election=E, max_restart=Rr, invariants=tuple(invariants),
                    check_deadlock=check_deadlock, **({variant: True} if variant else {}))
    mc = raftmc.ModelChecker(raftmc.ModelConfig(n_servers=n, n_vals=V, max_election=E, max_restart=Rr,
                                                invariants=tuple(invariants), check_deadlock=check_deadlock,
                                                spec_variant=VARIANT.get(variant, raftmc.SPEC_RAFT), **kw))
    return ocfg, mc


# name -> (make() arguments, walks, depth, seed)
PARITY = {
    "n3_v1_e2_r3": (dict(n=3, V=1, E=2, Rr=3), 200, 100, 1),
    "raftcfg_n3_v2_e3_r3": (dict(n=3, V=2, E=3, Rr=3), 200, 100, 1),
    "n2_v1_e1_r1": (dict(n=2, V=1, E=1, Rr=1), 200, 100, 1),
    "n3_v3_e3_r3": (dict(n=3, V=3, E=3, Rr=3), 200, 100, 1),
    "n3_v1_e2_r3_cap128": (dict(n=3, V=1, E=2, Rr=3, msg_cap=128), 200, 100, 1),
    "bf_n4_v1_e1_r3": (dict(n=4, V=1, E=1, Rr=3, variant="become_follower"), 50, 100, 1),
    "n5_v1_e3_r3": (dict(n=5, V=1, E=3, Rr=3), 60, 200, 1),
    "bf_n5_v2_e3_r3": (dict(n=5, V=2, E=3, Rr=3, variant="become_follower"), 30, 200, 1),
    # MaxElection / MaxRestart past 3: terms, election and restart counters up to 7 inside k_walk
    "n3_v1_e7_r7": (dict(n=3, V=1, E=7, Rr=7), 200, 100, 1),
    "n3_v2_e6_r6": (dict(n=3, V=2, E=6, Rr=6), 200, 100, 1),
    "n5_v1_e7_r7": (dict(n=5, V=1, E=7, Rr=7), 200, 100, 1),
    "bf_n3_v1_e7_r7": (dict(n=3, V=1, E=7, Rr=7, variant="become_follower"), 200, 100, 1),
}


@functools.lru_cache(maxsize=None)
def parity_oracle(name):
    kw, walks, depth, seed = PARITY[name]
    kw = {k: v for k, v in kw.items() if k != "msg_cap"}
    ocfg = R.Config(n=kw["n"], V=kw["V"], max_election=kw["E"], max_restart=kw["Rr"],
                    **({kw["variant"]: True} if kw.get("variant") else {}))
    return oracle_walks(ocfg, walks, depth, seed)


def assert_accounted(res, walks, upto=None):
    """res's lengths, keys and counters against the oracle's walks 0 .. upto (all of them: None)."""
    acc = walks if upto is None else walks[:upto + 1]
    if res.lengths is not None:
        assert res.lengths[:len(acc)] == [w["len"] for w in acc]
        for i, w in enumerate(acc):
            assert [tuple(k) for k in res.keys[i]] == [tuple(k) for k in w["keys"]], i
        assert all(n == 0 for n in res.lengths[len(acc):])  # walks past the error are not accounted
    assert res.walks == len(acc)
    assert res.states == sum(w["len"] for w in acc)
    assert res.generated == sum(w["gen"] for w in acc)
    assert res.longest == max(w["len"] for w in acc)
    assert res.ended_early == sum(1 for w in acc if w["end"] in ("stuck", "deadlock"))


@pytest.mark.parametrize("batch", [64, 0])
@pytest.mark.parametrize("name", sorted(PARITY))
def test_walks_match_oracle(name, batch):
    """Lengths and every key of every walk, the accounted sums and the status.  batch_walks 64 does
    not divide the walk counts, so the last batch is a short one; auto runs them in one launch."""
    kw, n, depth, seed = PARITY[name]
    walks, err = parity_oracle(name)
    assert err is None and len(walks) == n
    _, mc = make(**kw)
    with mc:
        res = mc.simulate(n, depth=depth, seed=seed, batch_walks=batch, keep_walks=True)
    assert res.status == "done" and res.violated is None and res.err_walk is None
    assert_accounted(res, walks)


def test_parity_walks_reach_both_exits():
    """Neither exit is vacuous: the oracle's walks hit the depth bound and end in states without
    successors, in every parity configuration whose space allows both."""
    ends = {name: [w["end"] for w in parity_oracle(name)[0]] for name in PARITY}
    for name, e in ends.items():
        assert set(e) <= {"depth", "stuck"}
    assert any("depth" in e and "stuck" in e for e in ends.values())
    assert sum(e.count("depth") for e in ends.values()) > 0 and sum(e.count("stuck") for e in ends.values()) > 0
    print({name: (e.count("depth"), e.count("stuck")) for name, e in ends.items()})


BASE = dict(n=3, V=1, E=2, Rr=3)


def test_edge_shapes():
    ocfg, mc = make(**BASE)
    with mc:
        r = mc.simulate(70, depth=1, seed=3, keep_walks=True)
        assert r.status == "done" and r.lengths == [1] * 70 and r.generated == 0 and r.states == 70
        assert r.keys == [[]] * 70 and r.longest == 1 and r.ended_early == 0
        for n, depth, batch in [(70, 2, 0), (1, 100, 0), (65, 100, 64)]:
            walks, err = oracle_walks(ocfg, n, depth, 3)
            assert err is None
            r = mc.simulate(n, depth=depth, seed=3, batch_walks=batch, keep_walks=True)
            assert r.status == "done"
            assert_accounted(r, walks)
            if depth == 2:
                assert r.lengths == [2] * n and r.generated == n * len(R.successors(ocfg, R.init_state(ocfg)))


def test_deterministic_across_batches():
    """The same call twice, and batch_walks 1 (a launch per walk), 7 (a tail batch), 64 and auto."""
    _, mc = make(**BASE)
    with mc:
        runs = [mc.simulate(130, depth=60, seed=9, batch_walks=b, keep_walks=True) for b in (0, 0, 1, 7, 64)]
    key = lambda r: (r.status, r.walks, r.states, r.generated, r.longest, r.ended_early, r.lengths, r.keys)
    assert all(key(r) == key(runs[0]) for r in runs[1:])
    assert runs[0].states > 130


def test_persistent_loop_takes_several_walks_per_wave():
    """8,300 walks in one batch: more walks than the launch has waves (8,192 at most), so some waves
    take a second walk; depth 4 keeps the oracle's replay short."""
    ocfg, mc = make(**BASE)
    walks, err = oracle_walks(ocfg, 8300, 4, 5)
    assert err is None
    with mc:
        r = mc.simulate(8300, depth=4, seed=5, batch_walks=8300, keep_walks=True)
    assert r.status == "done"
    assert_accounted(r, walks)


# name -> (make() arguments, walks, depth, seed, expected oracle facts)
ERRORS = {
    "seeded_inv": (dict(BASE, variant="seeded"), 400, 100, 1),
    "split_brain_assert": (dict(BASE, variant="split_brain"), 64, 100, 2),
    "deadlock": (dict(BASE, check_deadlock=True), 64, 100, 4),
    "seven_invariants": (dict(BASE, invariants=("Inv", "NoSplitVote", "RaftCanCommt", "FollowerCanCommit", "CommitAll",
                                                "NoAllCommit", "ExistLeaderAndCandidate")), 64, 100, 1),
    # (not in the list above: an invariant other than the first of the cfg, violated inside a walk)
    "split_brain_no_split_vote": (dict(BASE, variant="split_brain", invariants=("Inv", "NoSplitVote")), 64, 100, 2),
}


@functools.lru_cache(maxsize=None)
def error_oracle(name):
    kw, n, depth, seed = ERRORS[name]
    ocfg = R.Config(n=kw["n"], V=kw["V"], max_election=kw["E"], max_restart=kw["Rr"],
                    invariants=tuple(kw.get("invariants", ("Inv",))), check_deadlock=kw.get("check_deadlock", False),
                    **({kw["variant"]: True} if kw.get("variant") else {}))
    return oracle_walks(ocfg, n, depth, seed, stop_at_error=False)


@pytest.mark.parametrize("batch", [64, "all"])
@pytest.mark.parametrize("name", sorted(ERRORS))
def test_smallest_erring_walk_wins(name, batch):
    """err_walk, err_len, status, violated, the accounted counters and the behaviour, with batches of
    64 and with every walk in one launch (later erring walks run beside the first)."""
    kw, n, depth, seed = ERRORS[name]
    walks, err = error_oracle(name)
    assert err is not None
    erring = [i for i, w in enumerate(walks) if w["end"] not in ("depth", "stuck")]
    if name == "seeded_inv":
        assert err >= 64 and len(erring) >= 2 and walks[err]["end"] == ("invariant", "Inv")
    if name == "split_brain_assert":
        assert walks[err]["end"] == "assert" and len(erring) >= 2
    if name == "deadlock":
        assert walks[err]["end"] == "deadlock"
    if name == "seven_invariants":  # (RaftCanCommt is FALSE at Init already: the error is Init's, length 1)
        assert err == 0 and walks[0]["end"] == ("invariant", "RaftCanCommt")
    if name == "split_brain_no_split_vote":
        assert walks[err]["end"] == ("invariant", "NoSplitVote") and walks[err]["len"] > 1
    print(name, "first error: walk", err, "length", walks[err]["len"], walks[err]["end"], "erring walks:", len(erring))
    _, mc = make(**kw)
    with mc:
        res = mc.simulate(n, depth=depth, seed=seed, batch_walks=n if batch == "all" else batch, keep_walks=True)
        trace = mc.trace()
    w = walks[err]
    kind = w["end"] if isinstance(w["end"], str) else w["end"][0]
    assert res.status == STATUS[kind]
    assert res.violated == (None if isinstance(w["end"], str) else w["end"][1])
    assert (res.err_walk, res.err_len) == (err, w["len"])
    assert_accounted(res, walks, upto=err)
    assert [st for _, st in trace] == [R.state_to_json(s) for s in w["states"]]
    assert [k for k, _ in trace] == [None] + [tuple(k) for k in w["keys"]]


def golden_levels(name):
    with open(os.path.join(GOLDEN, "levels.json")) as f:
        return json.load(f)[name]


def assert_golden_run(res, g):
    assert res.status == "done"
    assert (res.distinct, res.generated, res.depth) == (g["distinct"], g["generated"], g["depth"])
    assert [ls.new_states for ls in res.levels if ls.new_states] == g["levels"]


CONFIGS1 = "n3_v1_e2_r3"  # configs[1]: 223,437 distinct states at depth 37


def test_bfs_untouched_by_simulate():
    g = golden_levels(CONFIGS1)
    assert (g["distinct"], g["depth"]) == (223437, 37)
    ocfg, fresh = make(**BASE)
    with fresh:
        ref = fresh.simulate(100, depth=50, seed=6, keep_walks=True)
    # (a) simulate on a fresh checker, then run()
    _, mc = make(**BASE)
    with mc:
        a = mc.simulate(100, depth=50, seed=6, keep_walks=True)
        assert_golden_run(mc.run(), g)
        # (b) after a finished run(), simulate gives what it gives on a fresh checker
        b = mc.simulate(100, depth=50, seed=6, keep_walks=True)
        assert mc.result().distinct == g["distinct"] and mc.trace() == []
    for r in (a, b):
        assert (r.status, r.states, r.generated, r.lengths, r.keys) == \
               (ref.status, ref.states, ref.generated, ref.lengths, ref.keys)
    # (c) a simulate that ends in an error, then reset() + run(): the seeded spec's golden counterexample
    gs = golden_levels("seeded_n3_v1_e2_r3")
    with open(os.path.join(GOLDEN, "traces.json")) as f:
        ts = json.load(f)["seeded_n3_v1_e2_r3"]
    _, mc = make(**dict(BASE, variant="seeded"))
    with mc:
        e = mc.simulate(400, depth=100, seed=1)
        assert e.status == "invariant" and len(mc.trace()) == e.err_len
        mc.reset()
        assert mc.trace() == []
        res = mc.run()
        trace = mc.trace()
    assert (res.status, res.violated) == ("invariant", gs["violated"])
    assert (res.generated, res.distinct, res.queue, res.trace_len) == \
           (gs["generated"], gs["distinct"], gs["queue_left"], gs["trace_len"])
    assert [st for _, st in trace] == [step["state"] for step in ts["steps"]]


def test_simulate_between_bfs_steps():
    g = golden_levels(CONFIGS1)
    _, mc = make(**BASE)
    with mc:
        mc.init()
        for _ in range(5):
            mc.step()
        r = mc.simulate(65, depth=40, seed=2, batch_walks=64)
        assert r.status == "done"
        res = mc.run()
    assert (res.status, res.distinct, res.generated, res.depth) == ("done", g["distinct"], g["generated"], g["depth"])


def test_refusals():
    _, mc = make(**BASE)
    with mc:
        for kw in (dict(num_walks=10, depth=0), dict(num_walks=0, depth=10)):
            with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
                mc.simulate(**kw)
    _, mc = make(**dict(BASE, virtual_shards=2))
    with mc:
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
            mc.simulate(10)


def test_simulate_after_release_device_is_refused():
    _, mc = make(**BASE)
    with mc:
        assert mc.simulate(3, depth=5).status == "done"
        assert mc.lib.rmc_release_device(mc.h) == raftmc.RMC_OK
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.simulate(3, depth=5)


def _state_blocks(out):
    blocks, cur = [], None
    for line in out:
        if line.startswith("State "):
            cur = [line]
            blocks.append(cur)
        elif cur is not None and line.startswith("/\\ "):
            cur.append(line)
        elif cur is not None and line.startswith("   ["):
            cur[-1] += " " + line.strip()
        elif cur is not None and not line.strip():
            cur = None
    return blocks


def test_launcher_simulate(tmp_path):
    """raftmc -simulate on the seeded spec: exit 12, the seed named, the State k blocks equal to the
    oracle's behaviour; on the plain spec with -deadlock: exit 0 and the accounted totals."""
    from test_host import LAUNCHER, cfg_text
    from tla_render import render_state
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    (tmp_path / "RaftSeeded.cfg").write_text(cfg_text(E=2, R=3, vals="v1"))
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=2, R=3, vals="v1"))
    args = ["-simulate", "num=400", "-depth", "100", "-seed", "1"]
    r = subprocess.run([LAUNCHER] + args + ["-deadlock", "-config", str(tmp_path / "RaftSeeded.cfg"),
                                            str(tmp_path / "RaftSeeded.tla")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 12, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert any("Simulation" in ln and "seed 1" in ln for ln in out)
    assert "Error: Invariant Inv is violated." in out and "Error: The behavior up to this point is:" in out
    walks, err = error_oracle("seeded_inv")
    w = walks[err]
    blocks = _state_blocks(out)
    assert len(blocks) == w["len"]
    for k, (blk, key, st) in enumerate(zip(blocks, [None] + w["keys"], w["states"])):
        if key is None:
            assert blk[0] == f"State {k + 1}: <Initial predicate>"
        else:
            assert blk[0] == f"State {k + 1}: <{raftmc.ACTIONS[key[1]]}(s{key[0] + 1})>", blk[0]
        want = render_state(R.state_to_json(st), ["s1", "s2", "s3"], ["v1"])
        assert [l.replace(",  [", ", [") for l in blk[1:]] == want, (k, blk[1:], want)
    acc = walks[:err + 1]
    assert f"{sum(x['len'] for x in acc)} states checked, {sum(x['gen'] for x in acc)} states generated." in out
    assert any(f"behaviour {err} " in ln for ln in out)

    r = subprocess.run([LAUNCHER] + args + ["-deadlock", "-config", str(tmp_path / "Raft.cfg"), str(tmp_path / "Raft.tla")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ocfg = R.Config(n=3, V=1, max_election=2, max_restart=3)
    walks, err = oracle_walks(ocfg, 400, 100, 1)
    assert err is None
    assert f"{sum(x['len'] for x in walks)} states checked, {sum(x['gen'] for x in walks)} states generated." in r.stdout
    assert "400 behaviours checked" in r.stdout and "No error has been found" in r.stdout
    assert sum(1 for ln in r.stdout.splitlines() if ln.startswith("State ")) == 0
