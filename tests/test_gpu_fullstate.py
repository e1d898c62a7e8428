"""GPU tests of the whole-state search (rmc_set_full_state, ModelConfig(view=False), raftmc -fullstate)
against tests/fullstate_ref.py and its fixture tests/golden/fullstate.json (make_golden_fullstate.py):

1. single states: every hidden component (each pendingResponse bit, electionCount, restartCount, valSent)
   reaches the fingerprint, at every site and under both SYMMETRY settings; with the setting off none does;
2. search parity with the reference in the five execution modes, and a VIEW twin that differs;
3. the compact seen set, checkpoint / resume, the refusals;
4. graph mode, coverage, continuation and graph_reach on whole states;
5. tools/view_gap.py's counts;
6. the launcher's -fullstate."""
import gzip
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import fullstate_ref as F
import raft_ref as R
import raftmc
import reach_ref
from conftest import GOLDEN, ROOT
from test_gpu import check_levels, checker, run_cfg
from test_gpu_variants import mode_kw

sys.path.insert(0, os.path.join(ROOT, "tools"))
import view_gap  # noqa: E402

pytestmark = pytest.mark.gpu


def load(name):
    with (gzip.open if name.endswith(".gz") else open)(os.path.join(GOLDEN, name), "rt") as f:
        return json.load(f)


FULL = load("fullstate.json")
SMALL = "sym_n2_v1_e2_r2"
SEEDED = "seeded_n3_v1_e2_r1"

# (fixture file, entry, ModelConfig extras): 2, 3, 4 and 5 servers, 64 and 128 message lanes
GROUPS = [
    ("successors.json", "n2_v2_e2_r3", {}),
    ("successors.json", "n3_v1_e2_r3", {}),
    ("successors.json", "n3_v1_e2_r3", dict(msg_cap=128)),
    ("successors.json", "n4_v1_e1_r3", {}),
    ("successors_variants.json.gz", "n4_v2_e1_r3", {}),
    ("successors_variants.json.gz", "n5_v2_e1_r3", {}),
    ("successors_deep.json.gz", "raftcfg_n3_v2_e3_r3", {}),
    ("successors_deep.json.gz", "raftcfg_n3_v2_e3_r3", dict(msg_cap=128)),
    ("successors_deep.json.gz", "c4_n5_v1_e3_r3", {}),
]
_files = {}


def group(fname, key):
    if fname not in _files:
        _files[fname] = load(fname)
    return _files[fname][key]


def fps_of(mc, dicts):
    """One rmc_fingerprints launch over state dicts -> [(x, y)]."""
    n, V = mc.cfg.n_servers, mc.cfg.n_vals
    rows = [raftmc.state_to_unpacked(d, n, V) for d in dicts]
    arr = np.zeros((len(rows), max(len(r) for r in rows)), dtype=np.int32)
    for i, r in enumerate(rows):
        arr[i, :len(r)] = r
    return [tuple(int(w) for w in f) for f in mc.fingerprints_array(arr)]


def sample(g, k=6, seed=11):
    """k states of the group (fixed choice), the first and the last among them; under 64 lanes only those
    that fit."""
    items = g["items"]
    rng = random.Random(seed)
    idx = sorted(set([0, len(items) - 1] + rng.sample(range(len(items)), min(k, len(items)))))
    return [items[i]["state"] for i in idx]


# ---- 1. single states ---------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetry", [True, False], ids=["sym", "nosym"])
@pytest.mark.parametrize("fname,key,extra", GROUPS, ids=[f"{k}{'_cap128' if e else ''}" for _, k, e in GROUPS])
def test_every_hidden_component_reaches_the_fingerprint(fname, key, extra, symmetry):
    g = group(fname, key)
    n, V = g["n"], g["V"]
    cap = extra.get("msg_cap", 64 if n <= 3 else 128)
    mc = checker(n, V, g["E"], g["R"], symmetry=symmetry, view=False, **extra)
    rcfg = R.Config(n=n, V=V, max_election=g["E"], max_restart=g["R"], symmetry=symmetry, view=False)
    rng = random.Random(5)
    perms = [p for p in ([1, 0] + list(range(2, n)), list(range(1, n)) + [0], rng.sample(range(n), n))]
    used = 0
    for d in sample(g):
        if len(d["msgs"]) > cap:
            continue
        used += 1
        st = R.state_from_json(d)
        copies = F.hidden_copies(st)
        labels = [c[0] for c in copies]
        assert sum(x.startswith("pend") for x in labels) == n * (n - 1) + 1
        assert all(any(x.startswith(p) for x in labels) for p in ("valSent", "electionCount", "restartCount"))
        base = [st] + [c[1] for c in copies]
        images = [(i, F.permute_state(s, pi)) for i, s in enumerate(base) for pi in perms]
        fps = fps_of(mc, [R.state_to_json(s) for s in base + [im for _, im in images]])
        fb, fi = fps[:len(base)], fps[len(base):]
        # whole state on: every copy differs from the state (one bit or one count more or less: never the
        # state's orbit), and from every other copy -- but for two copies that are one class under SYMMETRY
        # (pendingResponse[0][1] and [0][2] flipped where servers 1 and 2 are alike): equal fingerprints only there
        assert all(f != fb[0] for f in fb[1:]), [x for x, f in zip(labels, fb[1:]) if f == fb[0]]
        for i in range(1, len(base)):
            for j in range(i + 1, len(base)):
                if fb[i] == fb[j]:
                    assert symmetry and F.canonical(rcfg, base[i]) == F.canonical(rcfg, base[j]), (labels[i - 1], labels[j - 1])
        if not symmetry:
            assert len(set(fb)) == len(base)
        for (i, im), f in zip(images, fi):
            if symmetry:  # a server permutation, pendingResponse permuted on both indices, keeps the fingerprint
                assert f == fb[i], (["state"] + labels)[i]
            else:  # equal exactly when the whole states are
                assert (f == fb[i]) == (F.whole(im) == F.whole(base[i])), (["state"] + labels)[i]
        # the single-state hook and the successor hook (the fused expansion's site) agree with the batch
        assert mc.fingerprint(R.state_to_json(base[0])) == fb[0]
        assert mc.fingerprint(R.state_to_json(base[1])) == fb[1]
        # the setting off, on the same checker: no hidden component is seen (the default, test_gpu_deep.py)
        try:
            mc.reset()
            mc.set_full_state(False)
            off = fps_of(mc, [R.state_to_json(s) for s in base])
            assert len(set(off)) == 1, [x for x, f in zip(labels, off[1:]) if f != off[0]]
        finally:
            mc.reset()
            mc.set_full_state(True)
        assert fps_of(mc, [R.state_to_json(base[0])])[0] == fb[0]
    assert used >= 3


def test_setting_off_is_the_default_fingerprint():
    """A checker with the setting toggled on and off again gives the fingerprints of one that never had it."""
    g = group("successors.json", "n3_v1_e2_r3")
    states = sample(g)
    plain = checker(g["n"], g["V"], g["E"], g["R"])
    with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"],
                                                max_restart=g["R"], view=False)) as mc:
        on = fps_of(mc, states)
        mc.set_full_state(False)
        assert fps_of(mc, states) == fps_of(plain, states) != on


@pytest.mark.parametrize("mode", ["default", "split"])
@pytest.mark.parametrize("name", [SMALL, "nosym_n2_v1_e2_r2", "sym_n3_v1_e2_r1"])
def test_every_site_gives_one_fingerprint(name, mode, monkeypatch):
    """The level kernels (a fused level / a split chunk's hash pass) against the hooks: after a finished run, a
    breadth-first walk through rmc_successors from Init finds every successor's fingerprint in the seen set,
    equal to rmc_fingerprint's and rmc_fingerprints', and the walk's distinct fingerprints are the run's states."""
    g = FULL[name]
    kw = mode_kw(mode, g, monkeypatch)
    mc, res = run_cfg(g, view=False, symmetry=g["symmetry"], **kw)
    check_levels(g, res)
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"])
    limit = 400 if g["distinct"] > 5000 else g["distinct"]
    init = R.state_to_json(R.init_state(cfg))
    seen, order, head = {mc.fingerprint(init): init}, [mc.fingerprint(init)], 0
    while head < len(order) and head < limit:
        got = mc.successors(seen[order[head]])
        head += 1
        fps = [fp for _, _, fp in got]
        assert fps_of(mc, [st for _, st, _ in got]) == fps if got else True
        assert all(mc.seen_contains(fps)) if got else True
        for _, st, fp in got:
            if fp not in seen:
                seen[fp] = st
                order.append(fp)
    assert mc.fingerprint(seen[order[-1]]) == order[-1]
    if limit == g["distinct"]:
        assert len(order) == g["distinct"]
    mc.close()


# ---- 2. search parity -----------------------------------------------------------------------------------
def trace_matches(mc, g):
    assert [(list(k) if k else None, st) for k, st in mc.trace()] == [(e["key"], e["state"]) for e in g["steps"]]


@pytest.mark.parametrize("mode", ["default", "host_levels", "split", "virtual2", "rccl1"])
@pytest.mark.parametrize("name", sorted(FULL))
def test_whole_state_bfs_matches_the_reference(name, mode, monkeypatch):
    g = FULL[name]
    mc, res = run_cfg(g, view=False, symmetry=g["symmetry"], **mode_kw(mode, g, monkeypatch))
    check_levels(g, res)
    if "steps" in g:
        trace_matches(mc, g)
    mc.close()


@pytest.mark.parametrize("name", sorted(FULL))
def test_view_twin_differs(name):
    """The same configuration under the VIEW gives the fixture's VIEW counts, which are not the whole-state
    ones: a setting that silently does nothing fails here (and above)."""
    g = FULL[name]
    twin = {**g, **g["view"]}
    mc, res = run_cfg(twin, symmetry=g["symmetry"])
    check_levels(twin, res)
    assert (res.generated, res.distinct) != (g["generated"], g["distinct"])
    mc.close()


# ---- 3. storage and resume ------------------------------------------------------------------------------
@pytest.mark.parametrize("device_levels", [0, 1])
def test_compact_seen_set_and_fixed_ring(device_levels):
    """The large-run storage as test_nosym_compact_seen_set_matches_golden runs it, on the whole state."""
    g = FULL["sym_n2_v2_e2_r2"]
    probe, res0 = run_cfg(g, view=False, chunk_successors=6000, device_levels=1)
    peak = res0.frontier_peak_bytes
    probe.close()
    slots = 1 << max(12, (int(g["distinct"] / 0.6)).bit_length())
    ring = int(0.6 * peak) + 4 * 6000 * 36 + 4096
    mc, res = run_cfg(g, view=False, chunk_successors=6000, device_levels=device_levels, compact_log2=10,
                      seen_log2=8, seen_mem_bytes=8 * slots, frontier_mem_bytes=ring)
    check_levels(g, res)
    assert res.seen_slot_bytes == 8 and res.seen_slots == slots
    mc.close()


def _cfg(g, view):
    return raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
                              symmetry=g["symmetry"], view=view)


def test_checkpoint_resume_matches_uninterrupted(tmp_path):
    g = FULL[SMALL]
    path = str(tmp_path / "run.ckpt")
    with raftmc.ModelChecker(_cfg(g, False)) as a, raftmc.ModelChecker(_cfg(g, False)) as b:
        a.init()
        for _ in range(8):
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


@pytest.mark.parametrize("writer", [False, True], ids=["view_writer", "whole_writer"])
def test_resume_rejects_the_other_setting(writer, tmp_path):
    g = FULL[SMALL]
    path = str(tmp_path / "run.ckpt")
    with raftmc.ModelChecker(_cfg(g, not writer)) as a:
        a.init()
        a.step()
        a.checkpoint(path)
    with raftmc.ModelChecker(_cfg(g, writer)) as b:
        with pytest.raises(raftmc.RmcError, match="not a checkpoint of this configuration"):
            b.resume(path)
    with raftmc.ModelChecker(_cfg(g, not writer)) as c:
        c.resume(path)


def test_setter_state_rules_and_reset_keeps_the_setting():
    g = FULL[SMALL]
    with raftmc.ModelChecker(_cfg(g, True)) as mc:
        mc.set_full_state(True)
        mc.init()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.set_full_state(False)
        res = mc.run()
        check_levels(g, res)
        mc.reset()  # the setting stays
        check_levels(g, mc.run())
        mc.reset()
        mc.set_full_state(False)
        res = mc.run()
        assert (res.generated, res.distinct) == (g["view"]["generated"], g["view"]["distinct"])


# ---- 4. the modes on top --------------------------------------------------------------------------------
def test_graph_mode_edges_are_the_whole_state_graph():
    g = FULL[SMALL]
    with raftmc.ModelChecker(_cfg(g, False)) as mc:
        mc.set_graph(states=False)
        res = mc.run()
        check_levels(g, res)
        src, _, dst = mc.graph_edges()
    gg = g["graph"]
    assert (res.distinct, len(src), int((src == dst).sum())) == (gg["states"], gg["edges"], gg["self_edges"])
    assert src.tolist() == gg["src"] and dst.tolist() == gg["dst"]


def test_coverage_counts_whole_states():
    g = FULL[SMALL]
    with raftmc.ModelChecker(_cfg(g, False)) as mc:
        mc.set_coverage()
        check_levels(g, mc.run())
        cov = mc.coverage()
    assert cov["Init"] == (1, 1)
    assert [cov[a] for a in raftmc.ACTIONS] == list(zip(g["coverage"]["distinct"], g["coverage"]["generated"]))
    assert 1 + sum(cov[a][0] for a in raftmc.ACTIONS) == g["distinct"] != g["view"]["distinct"]


def test_continuation_counts_whole_states():
    g = FULL[SEEDED]
    c = g["continue"]
    mc = raftmc.ModelChecker(raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"],
                                                max_restart=g["R"], spec_variant=raftmc.SPEC_SEEDED, view=False))
    with mc:
        mc.set_continue()
        res = mc.run()
        assert (res.generated, res.distinct, res.depth) == (c["generated"], c["distinct"], c["depth"])
        assert mc.violations() == {nm: (v["count"], v["first_level"]) for nm, v in c["violations"].items()}
    assert c["violations"]["Inv"]["count"] > 0


def test_graph_reach_on_the_whole_state_graph():
    g = FULL[SMALL]
    gg = g["graph"]
    n, src, dst = gg["states"], np.array(gg["src"]), np.array(gg["dst"])
    exp, _ = reach_ref.np_query(n, src, dst, np.array(gg["raft_can_commit"], dtype=bool),
                                reach_ref.np_levels(n, src, dst))
    del exp["dist_sha256"]
    with raftmc.ModelChecker(_cfg(g, False)) as mc:
        mc.set_graph_keep()
        check_levels(g, mc.run())
        r = mc.graph_reach("RaftCanCommt")
        assert reach_ref.result_fields(r, mc.graph_reach_levels()) == exp
    assert 0 < exp["targets"] < n


# ---- 5. view gap ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bf_n2_v1_e2_r1", SMALL, "nosym_n2_v1_e2_r2"])
def test_view_gap_counts(name):
    g = FULL[name]
    kw = dict(n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"], symmetry=g["symmetry"],
              spec_variant=raftmc.SPEC_BECOME_FOLLOWER if g["become_follower"] else raftmc.SPEC_RAFT)
    r = view_gap.view_gap(kw, raftmc)
    v = g["view"]
    assert r["view"] == (v["distinct"], v["generated"], v["depth"])
    assert r["full"] == (g["distinct"], g["generated"], g["depth"])
    assert r["view_classes"] == g["view_classes"]
    assert view_gap.verdict(r) == "the VIEW run missed no class"


# ---- 6. launcher ----------------------------------------------------------------------------------------
def test_launcher_fullstate_on_the_seeded_cfg(tmp_path):
    from test_host import LAUNCHER, cfg_text
    g = FULL[SEEDED]
    v = g["view"]
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=g["E"], R=g["R"], vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    base = [LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg"), str(tmp_path / "RaftSeeded.tla")]
    full = subprocess.run(base[:1] + ["-fullstate"] + base[1:], capture_output=True, text=True, env=env, timeout=120)
    view = subprocess.run(base, capture_output=True, text=True, env=env, timeout=120)
    line = "Fingerprinting the whole state: the cfg's VIEW view is not applied."
    assert full.returncode == view.returncode == 12, full.stdout + full.stderr
    fl, vl = full.stdout.splitlines(), view.stdout.splitlines()
    assert fl.count(line) == 1 and fl[[i for i, x in enumerate(fl) if x.startswith("Starting... (")][0] + 1] == line
    assert line not in vl
    assert f"{g['generated']} states generated, {g['distinct']} distinct states found, {g['queue_left']} states left" \
        in full.stdout
    assert f"{v['generated']} states generated, {v['distinct']} distinct states found, {v['queue_left']} states left" \
        in view.stdout
    assert "Error: Invariant Inv is violated." in full.stdout and f"State {g['trace_len']}:" in full.stdout
    # without the flag: the launcher's stdout of before the flag existed, byte for byte but for the lines that
    # carry a time, a rate or the spec's path (tests/golden/launcher_seeded_n3_v1_e2_r1_view.txt, recorded from
    # the build without rmc_set_full_state on this cfg); with it: the same lines but the new one, the counters
    # and the whole-state behaviour
    want = open(os.path.join(GOLDEN, "launcher_seeded_n3_v1_e2_r1_view.txt")).read()
    assert mask_times(view.stdout) == want
    assert mask_times(full.stdout) != want
    assert [x for x in mask_times(full.stdout).splitlines() if x != line][:len(PRE)] == want.splitlines()[:len(PRE)]


# the lines of the launcher's stdout that hold a time, a rate or a path, cut after their fixed beginning
TIMED = ("Parsing file ", "Starting... (", "Finished computing initial states", "Progress(", "Finished in ", "GPU: ")
PRE = ("raftmc (", "Running breadth-first", "Parsing file ", "Semantic processing", "Starting... (", "Computing initial")


def mask_times(text):
    out = []
    for ln in text.splitlines():
        cut = next((t for t in TIMED if ln.startswith(t)), None)
        out.append(cut if cut else ln)
    return "\n".join(out) + "\n"
