"""GPU parity tests of the compiled kernel variants the Raft.cfg family of fixtures never launches
(fixtures: tests/golden/make_golden_variants.py, from the oracles only):

* a cfg without SYMMETRY (rmc_config.no_symmetry): the fingerprint's coset is the identity at all
  three sites (single state, hash pass, fused expansion);
* two values at four and five servers -- Layout<4,2> / Layout<5,2>, and with BecomeFollower the
  largest successor stride of all;
* msg_cap = 128 at three servers (MR = 2: (3,1,2), (3,2,2) and their BecomeFollower twins);
* the capacity error (RMC_E_CAPACITY) of the single-state hooks.

The bar is test_gpu.py's: identical successor lists, classes, invariant values, per-level counts,
depth, verdict, counters at an error and counterexamples."""
import gzip
import json
import os

import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN
from test_gpu import DEEP, INV_NAMES, LEVELS, LEVELS_BF, SAMPLES, TRACES, check_levels, checker, run_cfg

pytestmark = pytest.mark.gpu


def load(name):
    with (gzip.open if name.endswith(".gz") else open)(os.path.join(GOLDEN, name), "rt") as f:
        return json.load(f)


LEVELS_V = load("levels_variants.json")
TRACES_V = load("traces_variants.json")
SAMPLES_V = load("successors_variants.json.gz")
NOSYM = sorted(k for k in LEVELS_V if k.startswith("nosym_"))
PREFIXES = sorted(k for k, g in LEVELS_V.items() if g.get("prefix"))


def trace_matches(mc, t):
    assert [(list(k) if k else None, st) for k, st in mc.trace()] == [(e["key"], e["state"]) for e in t["steps"]]


def mode_kw(mode, g, monkeypatch):
    """The execution modes of test_gpu.py: the device loop, host-driven levels, every chunk split, two
    virtual shards (rounds of a few dozen parents; `_split`: every round a split one), a one-rank RCCL
    communicator."""
    if mode.endswith("split"):
        monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    size = g.get("distinct") or sum(g["levels"])
    chunk = 3000 if size < 100000 else 40000  # rounds of 20-40 parents; a few hundred at the 2 * 10^5-state runs
    if mode == "default":
        return {}
    if mode in ("host_levels", "split"):
        return dict(device_levels=1)
    if mode.startswith("virtual2"):
        return dict(virtual_shards=2, chunk_successors=chunk, shard_min_states=1)
    assert mode == "rccl1"
    return dict(world_size=1, rank=0, comm_unique_id=raftmc.comm_unique_id(), chunk_successors=chunk,
                shard_min_states=1)


# ---- 1. no SYMMETRY: BFS parity -----------------------------------------------------------------
def test_nosym_fixtures_are_the_issue_configurations():
    assert NOSYM == sorted(["nosym_n3_v1_e1_r3", "nosym_n2_v1_e2_r3", "nosym_n3_v2_e1_r3", "nosym_n4_v1_e1_r3",
                            "nosym_seeded_n3_v2_e2_r3", "nosym_deadlock_n3_v1_e1_r3"])
    assert sorted(TRACES_V) == ["nosym_deadlock_n3_v1_e1_r3", "nosym_seeded_n3_v2_e2_r3"]
    assert LEVELS_V["nosym_seeded_n3_v2_e2_r3"]["verdict"] == "invariant"
    assert LEVELS_V["nosym_deadlock_n3_v1_e1_r3"]["verdict"] == "deadlock"


@pytest.mark.parametrize("mode", ["default", "host_levels", "split", "virtual2", "rccl1"])
@pytest.mark.parametrize("name", NOSYM)
def test_nosym_bfs_matches_golden_levels(name, mode, monkeypatch):
    """A cfg without SYMMETRY: every view is its own class (both oracles, symmetry off) -- levels,
    generated per level, depth, verdict, counters at the error and the counterexample."""
    g = LEVELS_V[name]
    mc, res = run_cfg(g, symmetry=False, **mode_kw(mode, g, monkeypatch))
    check_levels(g, res)
    if name in TRACES_V:
        trace_matches(mc, TRACES_V[name])
    mc.close()


@pytest.mark.parametrize("device_levels", [0, 1])
@pytest.mark.parametrize("name", ["nosym_n3_v1_e1_r3", "nosym_n3_v2_e1_r3"])
def test_nosym_compact_seen_set_matches_golden(name, device_levels):
    """The large-run storage (8-B seen-set slots after 2^10, a frontier ring at ~60 % of the peak) as
    test_compact_seen_set_and_fixed_ring_match_golden runs it, without SYMMETRY."""
    g = LEVELS_V[name]
    probe, res0 = run_cfg(g, symmetry=False, chunk_successors=6000, device_levels=1)
    peak = res0.frontier_peak_bytes
    probe.close()
    slots = 1 << max(12, (int(g["distinct"] / 0.6)).bit_length())
    ring = int(0.6 * peak) + 4 * 6000 * 36 + 4096
    mc, res = run_cfg(g, symmetry=False, chunk_successors=6000, device_levels=device_levels, compact_log2=10,
                      seen_log2=8, seen_mem_bytes=8 * slots, frontier_mem_bytes=ring)
    check_levels(g, res)
    assert res.seen_slot_bytes == 8 and res.seen_slots == slots
    mc.close()


def _nosym_cfg(g, symmetry=False):
    return raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
                              symmetry=symmetry)


def test_nosym_checkpoint_resume_matches_uninterrupted(tmp_path):
    g = LEVELS_V["nosym_n3_v1_e1_r3"]
    path = str(tmp_path / "run.ckpt")
    with raftmc.ModelChecker(_nosym_cfg(g)) as a, raftmc.ModelChecker(_nosym_cfg(g)) as b:
        a.init()
        for _ in range(6):
            assert a.step().status == "ok"
        a.checkpoint(path)
        done = len(a.levels)
        res_a = a.run()
        b.resume(path)
        res_b = b.run()
        check_levels(g, res_a)
        for f in ("status", "generated", "distinct", "depth", "queue"):
            assert getattr(res_b, f) == getattr(res_a, f), f
        assert [ls.new_states for ls in res_b.levels if ls.new_states] == g["levels"][done:]


@pytest.mark.parametrize("writer", [False, True])
def test_resume_rejects_the_other_symmetry_setting(writer, tmp_path):
    """A checkpoint's seen set holds the fingerprints of one symmetry setting only."""
    g = LEVELS_V["nosym_n3_v1_e1_r3"]
    path = str(tmp_path / "run.ckpt")
    with raftmc.ModelChecker(_nosym_cfg(g, symmetry=writer)) as a:
        a.init()
        a.step()
        a.checkpoint(path)
    with raftmc.ModelChecker(_nosym_cfg(g, symmetry=not writer)) as b:
        with pytest.raises(raftmc.RmcError, match="not a checkpoint of this configuration"):
            b.resume(path)
    with raftmc.ModelChecker(_nosym_cfg(g, symmetry=writer)) as c:
        c.resume(path)


# ---- 2. no SYMMETRY: single states ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_nosym_fingerprint_is_exact_view_equality(name):
    """symmetry=False on the samples of successors.json: a state and its server-permuted copy have one
    fingerprint exactly when their views coincide; over all successors of all samples and of their
    permuted copies the fingerprint partition is exact view equality (raft_ref.canonical, symmetry off)
    in both directions; and the successor lists -- keys and states -- are the symmetric checker's (the
    fixture's, and the oracle's for the permuted copies)."""
    g = SAMPLES[name]
    sym = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"])
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"], symmetry=False)
    view = lambda d: R.canonical(cfg, R.state_from_json(d))
    mc = checker(g["n"], g["V"], g["E"], g["R"], symmetry=False)
    fp_of_view, view_of_fp, classes = {}, {}, set()
    differ = 0
    for it in g["items"]:
        same = view(it["state"]) == view(it["permuted"])
        assert (mc.fingerprint(it["state"]) == mc.fingerprint(it["permuted"])) == same
        differ += not same
        permuted = [dict(key=list(k), state=R.state_to_json(t))
                    for k, t in R.successors(sym, R.state_from_json(it["permuted"]))]
        for src, exp in ((it["state"], it["successors"]), (it["permuted"], permuted)):
            got = mc.successors(src)
            assert [list(k) for k, _, _ in got] == [e["key"] for e in exp]
            for (k, st, fp), e in zip(got, exp):
                assert st == e["state"], (k, src)
                assert mc.fingerprint(st) == fp
                v = view(st)
                assert fp_of_view.setdefault(v, fp) == fp
                assert view_of_fp.setdefault(fp, v) == v
                classes.add(R.canonical(sym, R.state_from_json(st)))
    assert differ > 0
    # the identity coset splits classes that the symmetric fingerprint merges
    assert len(fp_of_view) > len(classes)


# ---- 3. two values at four and five servers ---------------------------------------------------------
def successors_match(mc, g):
    for it in g["items"]:
        got = mc.successors(it["state"])
        assert [list(k) for k, _, _ in got] == [e["key"] for e in it["successors"]]
        for (k, st, _), e in zip(got, it["successors"]):
            assert st == e["state"], (k, it["state"])


def classes_match(mc, g):
    fp_of_canon, canon_of_fp = {}, {}
    for it in g["items"]:
        assert mc.fingerprint(it["state"]) == mc.fingerprint(it["permuted"])
        for (k, st, fp), e in zip(mc.successors(it["state"]), it["successors"]):
            assert mc.fingerprint(st) == fp
            assert fp_of_canon.setdefault(e["canon"], fp) == fp
            assert canon_of_fp.setdefault(fp, e["canon"]) == e["canon"]
    assert len(fp_of_canon) == len({e["canon"] for it in g["items"] for e in it["successors"]})


def invariants_match(mc, g):
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"])
    for it in g["items"]:
        for sc in [it] + it["successors"][:4]:
            st = R.state_from_json(sc["state"])
            for nm in INV_NAMES:
                try:
                    exp = R.INV_FUNCS[nm](cfg, st)
                except R.EvalError:
                    exp = None
                assert mc.eval_invariant(sc["state"], nm) == exp, nm


@pytest.mark.parametrize("check", [successors_match, classes_match, invariants_match])
@pytest.mark.parametrize("name", sorted(SAMPLES_V))
def test_two_values_samples_match_oracle(name, check):
    """The three single-state tests of test_gpu.py on the (4,2) and (5,2) samples: successor lists,
    fingerprint classes (the permuted copy included), all seven invariants."""
    g = SAMPLES_V[name]
    check(checker(g["n"], g["V"], g["E"], g["R"]), g)


def maxsucc(g):
    """Successor slots per state (rmc_kernels.hip Launch::MX = Spec::MAXS + MCAP with BecomeFollower):
    the message lanes, SLOTS_PER_SERVER = 4 + V + (N - 1) per server, a BecomeFollower candidate per lane."""
    n = g["n"]
    msg_cap = 64 if n <= 3 else 128
    return msg_cap + n * (4 + g["V"] + n - 1) + (msg_cap if g.get("become_follower") else 0)


def test_bf_n5_v2_has_the_largest_successor_stride():
    """What the BecomeFollower cases below add: a stride past every other fixture's (301 at (5,1))."""
    top = maxsucc(LEVELS_V["bf_n5_v2_e1_r3"])
    assert LEVELS_V["bf_n5_v2_e1_r3"]["become_follower"] and LEVELS_V["bf_n4_v2_e1_r3"]["become_follower"]
    assert top == 128 + 5 * (4 + 2 + 4) + 128
    assert top > max(maxsucc(g) for g in list(LEVELS_BF.values()) + list(LEVELS.values()))
    assert top > maxsucc(LEVELS_V["bf_n4_v2_e1_r3"]) > maxsucc(LEVELS_BF["bf_n4_v1_e1_r3"])
    assert top <= 1024  # the sharded election key's 10-bit rank


# virtual2 beside virtual2_split: rounds below the split size fingerprint in the routed expansion, a site
# of its own (a wrong parent content matrix there at (5,2) passes the four other modes)
MODES_V2 = ["default", "host_levels", "split", "virtual2_split", "virtual2"]


@pytest.mark.parametrize("mode", MODES_V2)
def test_n4_v2_bfs_matches_golden_levels(mode, monkeypatch):
    """(4,2,2) exhausted: the C oracle's 212187 states level by level."""
    g = LEVELS_V["n4_v2_e1_r3"]
    assert not g.get("prefix") and g["verdict"] == "ok"
    mc, res = run_cfg(g, **mode_kw(mode, g, monkeypatch))
    check_levels(g, res)
    mc.close()


@pytest.mark.parametrize("mode", MODES_V2)
@pytest.mark.parametrize("name", PREFIXES)
def test_two_values_prefix_matches_c_oracle(name, mode, monkeypatch):
    """(5,2,2) and the BecomeFollower twins at (4,2,2) / (5,2,2): the levels the C oracle completes,
    level by level as test_configs3_prefix_matches_c_oracle steps them (the device loop two levels a
    batch, so that it stops within a level of the prefix)."""
    g = LEVELS_V[name]
    want = len(g["levels"])
    assert len(g["gen_per_level"]) == want - 1
    kw = mode_kw(mode, g, monkeypatch)
    if mode == "default":
        kw["device_levels"] = 2
    spec = raftmc.SPEC_BECOME_FOLLOWER if g.get("become_follower") else raftmc.SPEC_RAFT
    with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"],
                                                max_restart=g["R"], spec_variant=spec, **kw)) as mc:
        mc.init()
        while len(mc.levels) < want:
            last = mc.steps()[-1] if mode == "default" else mc.step()
            assert last.status == "ok"
        assert [ls.new_states for ls in mc.levels[:want]] == g["levels"]
        assert [ls.generated for ls in mc.levels[1:want]] == g["gen_per_level"]


def test_prefix_fixtures_are_the_issue_configurations():
    assert PREFIXES == ["bf_n4_v2_e1_r3", "bf_n5_v2_e1_r3", "n5_v2_e1_r3"]
    for name in PREFIXES:
        assert sum(LEVELS_V[name]["levels"]) >= 100_000, name


# ---- 4. msg_cap = 128 at three servers (MR = 2) --------------------------------------------------------
CAP128 = [("n3_v1_e2_r3", LEVELS, TRACES), ("n3_v2_e1_r3", LEVELS, TRACES), ("seeded_n3_v2_e2_r3", LEVELS, TRACES),
          ("bf_n3_v1_e2_r3", LEVELS_BF, {})]


@pytest.mark.parametrize("mode", ["default", "split", "virtual2"])
@pytest.mark.parametrize("name,levels,traces", CAP128, ids=[c[0] for c in CAP128])
def test_msg_cap_128_at_three_servers_matches_golden(name, levels, traces, mode, monkeypatch):
    """128 message lanes at 3 servers -- another MAXS, and 128 + 3 * SLOTS_PER_SERVER items a parent in
    the items kernel -- give the golden levels of the 64-lane runs."""
    g = levels[name]
    mc, res = run_cfg(g, msg_cap=128, **mode_kw(mode, g, monkeypatch))
    check_levels(g, res)
    if name in traces:
        trace_matches(mc, traces[name])
    mc.close()


@pytest.mark.parametrize("check", [successors_match, classes_match, invariants_match])
@pytest.mark.parametrize("name", ["n3_v1_e2_r3", "n3_v2_e1_r3"])
def test_msg_cap_128_samples_match_oracle(name, check):
    g = SAMPLES[name]
    mc = checker(g["n"], g["V"], g["E"], g["R"], msg_cap=128)
    check(mc, g)
    mc64 = checker(g["n"], g["V"], g["E"], g["R"])
    assert all(mc.fingerprint(it["state"]) == mc64.fingerprint(it["state"]) for it in g["items"])


def test_msg_cap_128_deep_states_match_oracle_and_the_64_lane_fingerprints():
    """The message-heavy Raft.cfg states (up to 64 messages) under the 128-lane checker: the oracle's
    successor lists and classes, and the fingerprints of the 64-lane checker bit for bit."""
    g = DEEP["raftcfg_n3_v2_e3_r3"]
    mc = checker(g["n"], g["V"], g["E"], g["R"], msg_cap=128)
    mc64 = checker(g["n"], g["V"], g["E"], g["R"])
    fp_of_canon, canon_of_fp = {}, {}
    heavy = 0
    for it in g["items"]:
        if it["assert_fails"]:
            with pytest.raises(AssertionError, match="split brain"):
                mc.successors(it["state"])
            continue
        assert mc.fingerprint(it["state"]) == mc.fingerprint(it["permuted"]) == mc64.fingerprint(it["state"])
        got = mc.successors(it["state"])
        assert [list(k) for k, _, _ in got] == [e["key"] for e in it["successors"]], it["nmsgs"]
        for (k, st, fp), e, (_, _, fp64) in zip(got, it["successors"], mc64.successors(it["state"])):
            assert st == e["state"], (k, it["nmsgs"])
            assert fp == fp64 == mc.fingerprint(st)
            assert fp_of_canon.setdefault(e["canon"], fp) == fp
            assert canon_of_fp.setdefault(fp, e["canon"]) == e["canon"]
            heavy += len(st["msgs"]) == 64
        for tag, vals in it["invariants"].items():
            st = it["state"] if tag == "state" else it["successors"][int(tag[4:])]["state"]
            assert [mc.eval_invariant(st, nm) for nm in INV_NAMES] == vals, (tag, it["nmsgs"])
    assert heavy > 0


# ---- 5. capacity ------------------------------------------------------------------------------------
def _state_at_the_cap():
    """A 3-server state of the deep fixture with exactly 64 messages of which the oracle's successor list
    holds one with 65: (state, oracle successors)."""
    g = DEEP["raftcfg_n3_v2_e3_r3"]
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"])
    for it in g["items"]:
        for sc in [it] + it.get("successors", []):
            if len(sc["state"]["msgs"]) != 64:
                continue
            try:
                succ = R.successors(cfg, R.state_from_json(sc["state"]))
            except R.AssertionFailure:
                continue
            if max(len(t.msgs) for _, t in succ) == 65:
                return g, sc["state"], succ
    raise AssertionError("the deep fixture has no 64-message state with a 65-message successor")


def test_successor_past_msg_cap_is_a_capacity_error():
    """A successor with 65 messages under the default cap of 64: RMC_E_CAPACITY, not a dropped message;
    msg_cap=128 returns the oracle's list; a 65-message state handed in under cap 64 is refused."""
    g, state, succ = _state_at_the_cap()
    mc64 = checker(g["n"], g["V"], g["E"], g["R"])
    mc128 = checker(g["n"], g["V"], g["E"], g["R"], msg_cap=128)
    mc64.fingerprint(state)  # 64 messages fit
    with pytest.raises(raftmc.RmcError, match="RMC_E_CAPACITY"):
        mc64.successors(state)
    got = mc128.successors(state)
    assert [list(k) for k, _, _ in got] == [list(k) for k, _ in succ]
    assert [st for _, st, _ in got] == [R.state_to_json(t) for _, t in succ]
    big = next(R.state_to_json(t) for _, t in succ if len(t.msgs) == 65)
    for call in (mc64.fingerprint, mc64.successors, lambda s: mc64.eval_invariant(s, "Inv")):
        with pytest.raises(raftmc.RmcError, match="RMC_E_CAPACITY"):
            call(big)
    assert mc128.fingerprint(big) == next(fp for _, st, fp in got if len(st["msgs"]) == 65)
    # the context is still usable after the refusals
    assert mc64.fingerprint(state) == mc128.fingerprint(state)


def test_msg_cap_below_64_is_rounded_up_to_64():
    """msg_cap selects the message rounds (MR = 1 up to 64, 2 above): msg_cap=8 is the 64-lane layout."""
    g, state, _ = _state_at_the_cap()
    mc8 = checker(g["n"], g["V"], g["E"], g["R"], msg_cap=8)
    assert mc8.fingerprint(state) == checker(g["n"], g["V"], g["E"], g["R"]).fingerprint(state)
    with pytest.raises(raftmc.RmcError, match="RMC_E_CAPACITY"):
        mc8.successors(state)
    small = LEVELS["n3_v1_e1_r3"]
    mc, res = run_cfg(small, msg_cap=8)
    check_levels(small, res)
    mc.close()


# ---- 7. launcher ----------------------------------------------------------------------------------------
def test_launcher_without_symmetry_line_prints_the_nosym_counts(tmp_path):
    """raftmc -deadlock -config on a cfg without the SYMMETRY line: TLC's closing lines carry the
    no-symmetry counts."""
    import subprocess
    from test_host import LAUNCHER, cfg_text
    g = LEVELS_V["nosym_n3_v1_e1_r3"]
    text = cfg_text(E=g["E"], R=g["R"], vals="v1")
    assert "SYMMETRY symmServers\n" in text
    (tmp_path / "Raft.cfg").write_text(text.replace("SYMMETRY symmServers\n", ""))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    r = subprocess.run([LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg"), str(tmp_path / "Raft.tla")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{g['generated']} states generated, {g['distinct']} distinct states found, 0 states left on queue." \
        in r.stdout
    assert f"The depth of the complete state graph search is {g['depth']}." in r.stdout
    assert g["distinct"] != LEVELS["n3_v1_e1_r3"]["distinct"]
