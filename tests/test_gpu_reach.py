"""Reachability queries on the GPU (rmc_set_graph_keep / rmc_graph_reach / rmc_graph_shape; raftmc -canreach): the
kept graph of a run against tests/golden/reach.json (the Python oracle, tests/golden/make_golden_reach.py), and the
analyses' kernels on imported graphs against numpy fixpoints written in tests/reach_ref.py.  Integers and digests:
every comparison is exact.  Every test fails without the feature (the entry points do not exist)."""
import gzip
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import raftmc
from conftest import GOLDEN
from reach_ref import UNSET, np_dist, np_levels, np_query, np_shape, result_fields, targets_of
from test_gpu_coverage import cfg_kw
from test_reach_host import FULL_KW, QUERIES, inv_values, qkey
from tla_render import render_state

import raft_ref as R

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "reach.json")) as _f:
    REACH = json.load(_f)
with gzip.open(os.path.join(GOLDEN, "graph_full.json.gz")) as _f:
    FULL = json.load(_f)
SHAPE_KEYS = ("states", "edges", "self_edges", "back_edges", "sinks", "max_in", "max_out", "cyclic_states")
BIG = "n3_v1_e2_r3"


def make(name, **kw):
    return raftmc.ModelChecker(raftmc.ModelConfig(**cfg_kw(name, **kw)))


def sha(a, t):
    return hashlib.sha256(np.asarray(a).astype(t).tobytes()).hexdigest()


def check_against_golden(mc, e, dists=None):
    """Shape, invariant values and all 14 queries of the kept graph against a reach.json entry."""
    sh = mc.graph_shape()
    assert {k: sh[k] for k in SHAPE_KEYS} == {k: e[k] for k in SHAPE_KEYS}
    assert sum(sh["in_hist"]) == sum(sh["out_hist"]) == e["states"] and sh["out_hist"][0] == e["sinks"]
    inv = mc.graph_inv_values()
    assert inv.dtype == np.uint16 and sha(inv, "<u2") == e["inv_sha256"]
    for _b, inv_name, value in QUERIES:
        want = dict(e["queries"][qkey(inv_name, value)])
        r = mc.graph_reach(inv_name, value, want_dist=True)
        got = result_fields(r, mc.graph_reach_levels())
        got["dist_sha256"] = sha(r.dist, "<u4")
        assert got == want, (inv_name, value)
        assert (r.states, r.edges, r.self_edges) == (e["states"], e["edges"], e["self_edges"])
        assert r.dist.dtype == np.uint32 and r.rounds == (r.max_distance + 1 if r.targets else 0)
        if dists is not None:
            dists[(inv_name, value)] = r.dist
    return inv


# ---- 1. runs against the fixture ------------------------------------------------------------------------------
@pytest.mark.parametrize("sink", [False, True], ids=["nosink", "sink"])
@pytest.mark.parametrize("chunk", [97, 0], ids=["chunk97", "auto"])
@pytest.mark.parametrize("name", list(REACH))
def test_run_equals_the_fixture(name, chunk, sink):
    """All 14 queries, the shape and the invariant values, whatever the edge chunking and with or without a sink; on
    configs[1] the distances also against the numpy fixpoint over the delivered edges and the library's values."""
    e = REACH[name]
    with make(name) as mc:
        mc.set_graph_keep()
        delivered = [0, 0, True]
        e_src, e_dst = [], []
        if sink:
            collect = name == BIG and chunk == 0

            def on_edges(s, k, d):
                delivered[1] += len(s)
                delivered[2] = delivered[2] and (len(d) == 0 or int(d.max()) < e["states"])
                if collect:
                    e_src.append(s.copy())
                    e_dst.append(d.copy())
                return 0

            def on_states(gid0, a):
                delivered[0] += len(a)
                return 0

            mc.set_graph(chunk_parents=chunk, on_states=on_states, on_edges=on_edges)
        elif chunk:
            # (no sink: the chunk size of the pass comes from a sink that is installed and removed again)
            mc.set_graph(states=False, chunk_parents=chunk)
            mc.clear_graph()
        res = mc.run()
        assert res.status == ("done" if e["verdict"] == "ok" else e["verdict"]) and res.distinct == e["states"]
        dists = {} if name == BIG and sink and chunk == 0 else None
        inv = check_against_golden(mc, e, dists)
        if sink:  # the error-stopped run too: totals equal the delivered states and edges, every dst < distinct
            assert (delivered[0], delivered[1]) == (e["states"], e["edges"]) and delivered[2]
        if dists is not None:  # independent of the new kernels: graph mode's edges, numpy's fixpoint
            src, dst = np.concatenate(e_src), np.concatenate(e_dst)
            assert len(src) == e["edges"]
            for b, inv_name, value in QUERIES[:6]:
                assert np.array_equal(np_dist(e["states"], src, dst, targets_of(inv, b, value)), dists[(inv_name, value)])


def test_error_stopped_run_keeps_what_graph_mode_delivers():
    name = "seeded_n3_v1_e2_r3"
    e = REACH[name]
    with make(name) as mc:
        mc.set_graph_keep()
        mc.set_graph(states=False)
        res = mc.run()
        assert res.status == "invariant"
        src, _key, dst = mc.graph_edges()
        sh = mc.graph_shape()
        assert (sh["states"], sh["edges"]) == (res.distinct, len(src)) == (e["states"], e["edges"])
        assert int(dst.max()) < res.distinct and int(src.max()) < res.distinct
        want = np_shape(res.distinct, src, dst)
        assert sh == want
        r = mc.graph_reach("Inv", False, want_dist=True)  # the violating state is the only target
        assert r.targets == 1 and r.dist[res.distinct - 1] == 0
        assert np.array_equal(r.dist, np_dist(res.distinct, src, dst, targets_of(mc.graph_inv_values(), 0, False)))


def test_keep_composes_with_coverage_and_continuation():
    """As graph mode does: the search that does not stop at the seeded spec's violation keeps the whole graph (what
    graph.json records without invariants), the coverage and the violation counts are those of that search."""
    from test_gpu_coverage import as_cov
    with open(os.path.join(GOLDEN, "graph.json")) as f:
        twin = json.load(f)["noinv_seeded_n3_v1_e2_r3"]
    with open(os.path.join(GOLDEN, "continue.json")) as f:
        cont = json.load(f)["seeded_n3_v1_e2_r3"]
    with make("seeded_n3_v1_e2_r3") as mc:
        mc.set_graph_keep()
        mc.set_continue()
        mc.set_coverage()
        res = mc.run()
        assert (res.status, res.distinct, res.generated) == ("done", cont["distinct"], cont["generated"])
        sh = mc.graph_shape()
        assert (sh["states"], sh["edges"]) == (twin["states"], twin["edges"]) == (res.distinct, res.generated - 1)
        assert mc.coverage() == as_cov(cont["coverage"]["generated"], cont["coverage"]["distinct"])
        r = mc.graph_reach("Inv", False)  # the states that violate Inv are the ones continuation counts
        assert r.targets == mc.violations()["Inv"][0] == cont["violations"]["Inv"]["count"]
        assert r.cannot_reach > 0 and r.first_cannot is not None
        inv = mc.graph_inv_values()
        assert int(((inv & 1) == 0).sum()) == r.targets and not (inv >> 8).any()


# ---- 2. between steps ------------------------------------------------------------------------------------------
def test_query_between_steps_is_that_of_the_truncated_graph():
    name, k = "n3_v1_e1_r3", 6
    e = REACH[name]
    ls = e["level_starts"]
    n = ls[k + 1]  # init() + k steps: levels 1 .. k + 1 stand, the parents of levels 1 .. k have their edges
    edges = np.array([x for x in FULL[name]["edges"] if x[0] < ls[k]], dtype=np.int64)
    src, dst = edges[:, 0], edges[:, 2]
    assert int(dst.max()) < n
    inv = inv_values(R.Config(max_restart=3, **FULL_KW[name]), FULL[name]["states"][:n])
    lv = np_levels(n, src, dst)
    with make(name) as mc:
        mc.set_graph_keep()
        mc.init()
        for _ in range(k):
            mc.step()
        assert np.array_equal(mc.graph_inv_values(), inv)
        for b, inv_name, value in QUERIES:
            want, dist = np_query(n, src, dst, targets_of(inv, b, value), lv)
            r = mc.graph_reach(inv_name, value, want_dist=True)
            got = result_fields(r, mc.graph_reach_levels())
            got["dist_sha256"] = sha(r.dist, "<u4")
            assert got == want and np.array_equal(r.dist, dist)
        assert mc.graph_shape() == np_shape(n, src, dst)
        res = mc.run()  # the run goes on; the CSR is rebuilt for the grown graph
        assert res.status == "done"
        check_against_golden(mc, e)
        mc.reset()  # the store is emptied, the setting stays
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_shape()
        mc.run()
        check_against_golden(mc, e)


# ---- 3. ordering -----------------------------------------------------------------------------------------------
def test_ordering_and_limits():
    name = "n3_v1_e1_r3"
    calls = [lambda m: m.graph_reach("RaftCanCommt"), lambda m: m.graph_reach_levels(), lambda m: m.graph_shape(),
             lambda m: m.graph_inv_values(), lambda m: m.graph_import(1, [], [], [1])]
    with make(name) as mc:  # keep off
        mc.run()
        for f in calls:
            with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
                f(mc)
    with make(name) as mc:
        mc.set_graph_keep()
        for f in calls[:4]:  # on, nothing kept yet
            with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
                f(mc)
        mc.init()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.set_graph_keep()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_import(1, [], [], [1])  # mid-run
        mc.graph_reach("RaftCanCommt")  # Init alone is a graph
        mc.run()
        mc.graph_shape()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_reach_levels()  # the graph has grown since the last query
    with make(name, virtual_shards=2) as mc:
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
            mc.set_graph_keep()


@pytest.mark.parametrize("name", ["n3_v1_e1_r3", "seeded_n3_v1_e2_r3"])
def test_bfs_is_untouched_by_keep(name):
    """Levels, counters and the trace of a keep run equal the plain run's."""
    def run(keep):
        with make(name) as mc:
            if keep:
                mc.set_graph_keep()
            res = mc.run()
            lv = [(l.level, l.status, l.expanded, l.generated, l.new_states, l.total_generated, l.total_distinct, l.queue,
                   l.self_loops) for l in res.levels]
            tr = mc.trace() if res.status != "done" else None
            return (res.status, res.depth, res.generated, res.distinct, res.queue, res.violated, res.trace_len), lv, tr
    plain, kept = run(False), run(True)
    assert kept == plain


# ---- 4. imported graphs against the numpy fixpoints ------------------------------------------------------------
@pytest.fixture(scope="module")
def imc():
    with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=2, n_vals=1, max_election=1, max_restart=1)) as mc:
        mc.set_graph_keep()
        yield mc


def check_import(mc, n, src, dst, inv, queries=((0, True), (0, False), (2, True))):
    src, dst, inv = np.asarray(src, dtype=np.uint32), np.asarray(dst, dtype=np.uint32), np.asarray(inv, dtype=np.uint16)
    mc.graph_import(n, src, dst, inv)
    assert np.array_equal(mc.graph_inv_values(), inv)
    sh = mc.graph_shape()
    assert sh == np_shape(n, src, dst)
    out = {}
    for b, value in queries:
        name = raftmc.INVARIANT_BY_BIT[b]
        want, dist = np_query(n, src, dst, targets_of(inv, b, value))
        r = mc.graph_reach(name, value, want_dist=True)
        got = result_fields(r, mc.graph_reach_levels())
        assert got == {k: v for k, v in want.items() if k != "dist_sha256"}, (b, value)
        assert np.array_equal(r.dist, dist)
        assert (r.states, r.edges, r.self_edges) == (n, len(src), sh["self_edges"])
        out[(b, value)] = r
    return sh, out


def test_import_one_state_no_edge(imc):
    sh, q = check_import(imc, 1, [], [], [1])
    assert sh["sinks"] == 1 and sh["cyclic_states"] == 0
    assert (q[(0, True)].can_reach, q[(0, True)].init_distance, q[(0, True)].first_cannot) == (1, 0, None)
    assert (q[(0, False)].cannot_reach, q[(0, False)].first_cannot, q[(0, False)].first_cannot_level) == (1, 0, 1)


def test_import_only_self_edges(imc):
    n = 5
    sh, q = check_import(imc, n, list(range(n)) + [2], list(range(n)) + [2], [1, 0, 1, 0, 0])
    assert (sh["self_edges"], sh["sinks"], sh["cyclic_states"], sh["max_in"]) == (6, 0, 0, 2)
    assert (q[(0, True)].can_reach, q[(0, True)].max_distance, q[(0, True)].first_cannot) == (2, 0, 1)


def test_import_chain_of_1000(imc):
    """1,000 rounds of one-state frontiers."""
    n = 1000
    inv = np.zeros(n, dtype=np.uint16)
    inv[n - 1] = 1
    sh, q = check_import(imc, n, np.arange(n - 1), np.arange(1, n), inv, queries=((0, True),))
    r = q[(0, True)]
    assert np.array_equal(r.dist, np.arange(n - 1, -1, -1, dtype=np.uint32))
    assert (r.rounds, r.max_distance, r.init_distance, r.can_reach) == (1000, 999, 999, 1000)
    assert (sh["cyclic_states"], sh["sinks"], sh["back_edges"]) == (0, 1, 0)


def test_import_hub_with_duplicate_edges(imc):
    n = 2501
    src = np.concatenate([np.arange(1, n), np.arange(1, n)])  # every spoke twice: in-degree 5,000
    inv = np.zeros(n, dtype=np.uint16)
    inv[0] = 1
    sh, q = check_import(imc, n, src, np.zeros_like(src), inv)
    assert (sh["max_in"], sh["in_hist"][63], sh["max_out"], sh["back_edges"]) == (5000, 1, 2, 5000)
    assert (q[(0, True)].can_reach, q[(0, True)].max_distance, q[(0, True)].rounds) == (n, 1, 2)


def test_import_two_disjoint_cycles(imc):
    src = [0, 1, 2, 2, 3, 4, 5, 5]
    dst = [1, 2, 0, 6, 4, 5, 3, 7]
    sh, q = check_import(imc, 8, src, dst, [0, 0, 0, 0, 0, 0, 1, 0])
    assert sh["cyclic_states"] == 6 and sh["sinks"] == 2
    r = q[(0, True)]
    assert r.dist.tolist() == [3, 2, 1, UNSET, UNSET, UNSET, 0, UNSET]
    assert (r.can_reach, r.cannot_reach, r.first_cannot, r.init_distance) == (4, 4, 3, 3)


def test_import_random_graph_empty_and_full_target_sets(imc):
    rng = np.random.default_rng(20250411)
    n, m = 4096, 20000
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    inv = (rng.integers(0, 2, n) | (rng.integers(0, 16, n) == 0) << 2).astype(np.uint16)  # bit 0: half; bit 2: 1/16
    err = rng.integers(0, 8, n) == 0  # an eighth raise the evaluation error of invariant 0: in neither of its sets
    inv[err] = (inv[err] & ~np.uint16(1)) | np.uint16(1 << 8)
    # bit 1 is never set: "NoSplitVote = TRUE" is empty and "= FALSE" is everything
    sh, q = check_import(imc, n, src, dst, inv, queries=((0, True), (0, False), (2, True), (1, True), (1, False)))
    assert q[(0, True)].targets + q[(0, False)].targets == n - int(err.sum())
    e = q[(1, True)]
    assert (e.targets, e.can_reach, e.cannot_reach, e.first_cannot, e.rounds, e.init_distance) == (0, 0, n, 0, 0, None)
    f = q[(1, False)]
    assert (f.targets, f.can_reach, f.first_cannot, f.max_distance) == (n, n, None, 0)
    assert sh["cyclic_states"] > 0
    with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
        imc.graph_import(4, [0, 4], [1, 2], [0, 0, 0, 0])  # an edge past n_states


# ---- 5. launcher -----------------------------------------------------------------------------------------------
def _normal(out):
    out = re.sub(r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d", "<time>", out)
    out = re.sub(r"\(\d+ d?s/min\)", "(<rate>)", out)
    out = re.sub(r"Finished in [\d.]+s", "Finished in <s>", out)
    return re.sub(r"(?m)^GPU: .*$", "GPU: <rate>", out)


def test_launcher_canreach(tmp_path):
    from test_host import LAUNCHER, cfg_text
    name = "n3_v1_e1_r3"
    e = REACH[name]
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=1, R=3, servers="s1, s2, s3", vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    base = [LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg")]
    tla = str(tmp_path / "Raft.tla")
    plain = subprocess.run(base + [tla], capture_output=True, text=True, env=env, timeout=120)
    r = subprocess.run(base + ["-canreach", "RaftCanCommt", "-canreach", "CommitAll=FALSE", tla], capture_output=True, text=True,
                       env=env, timeout=120)
    assert plain.returncode == r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("Reachability of ")]
    end = [i for i, l in enumerate(lines) if l.startswith("The state graph has ")]
    assert len(at) == 2 and len(end) == 1 and at[0] < at[1] < end[0]
    q = e["queries"]["RaftCanCommt=TRUE"]
    assert lines[at[0]] == (
        f"Reachability of RaftCanCommt = TRUE: {q['targets']} of {e['states']} distinct states satisfy it, {q['can_reach']} can "
        f"reach one (farthest: {q['max_distance']} steps, Init: {q['init_distance']} steps), {q['cannot_reach']} cannot (first at "
        f"depth {q['first_cannot_level']}).")
    assert (q["targets"], q["can_reach"], q["cannot_reach"], q["first_cannot"]) == (300, 408, 137, 10)
    q2 = e["queries"]["CommitAll=FALSE"]
    assert lines[at[1]].startswith(f"Reachability of CommitAll = FALSE: {q2['targets']} of {e['states']} distinct states satisfy "
                                   f"it, {q2['can_reach']} can reach one")
    assert lines[end[0]] == "The state graph has no cycle other than self-loops."
    # the behaviour from Init to gid 10: as many states as its level, the last one the fixture's state 10
    block = lines[at[0] + 1:at[1]]
    assert block[0] == "The behavior up to the first state that cannot is:"
    heads = [i for i, l in enumerate(block) if re.match(r"State \d+: <", l)]
    assert len(heads) == q["first_cannot_level"] and block[heads[0]] == "State 1: <Initial predicate>"
    want = render_state(FULL[name]["states"][10], ["s1", "s2", "s3"], ["v1"])
    last = []  # (the trace printer wraps msgs: its continuation lines "   [..]" belong to the msgs line)
    for l in block[heads[-1] + 1:]:
        if l.startswith("   ["):
            last[-1] += " " + l.strip()
        elif l:
            last.append(l)
    assert [l.replace(",  [", ", [") for l in last] == want
    # without the flag: the parent's output; with it, the same lines around the new ones
    rest = lines[:at[0]] + lines[end[0] + 1:]
    assert _normal("\n".join(rest)) == _normal("\n".join(plain.stdout.splitlines()))
    assert "Reachability" not in plain.stdout and "The state graph has" not in plain.stdout
