"""Graph mode on the GPU (rmc_set_graph; raftmc -dump): the states a run finds and every resolved edge, against
tests/golden/graph.json and graph_full.json.gz (the Python oracle, tests/golden/make_golden_graph.py).  Integers
and text: every comparison is exact.

The entries cover every compiled kernel variant (n = 2..5, V = 1..2, BecomeFollower, no SYMMETRY, 128 message
lanes) and the four error kinds, whose cut a wrong stopping point would fail.  Every entry is checked by its
counts, its per-level edge counts, the edge digest and the digest over all of its states (and, as an extra, the
digest of the states with gid % 64 == 0).  The state digest is updated inside the states callback, piece by piece
(graph_render.StatesDigest: a state's JSON line from the texts of its variables, each rendered by json.dumps once
per distinct value), so the largest runs are checked whole in a few seconds; where a run has at most 25,000
states every line is also compared with the plain json.dumps(unpacked_to_state(row)) rendering."""
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
from graph_render import StatesDigest, dot_text, dump_text, edges_sha256
from test_gpu import check_levels
from test_gpu_coverage import cfg_kw, golden

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "graph.json")) as _f:
    GRAPH = json.load(_f)
with gzip.open(os.path.join(GOLDEN, "graph_full.json.gz")) as _f:
    FULL = json.load(_f)
TWIN = "noinv_seeded_n3_v1_e2_r3"
ERRORS = ["seeded_n3_v1_e2_r3", "sb_n3_v1_e2_r3", "deadlock_n3_v1_e1_r3", "cpl_n3_v2_e1_r3"]
ALL_STATES_MAX = 25000
SAMPLE = 64


def make(name, **kw):
    if name == TWIN:
        c = cfg_kw("seeded_n3_v1_e2_r3", **kw)
        c["invariants"] = ()
    else:
        c = cfg_kw(name, **kw)
    return raftmc.ModelChecker(raftmc.ModelConfig(**c))


def states_sha256(dicts):
    h = hashlib.sha256()
    for d in dicts:
        h.update((json.dumps(d, sort_keys=True) + "\n").encode())
    return h.hexdigest()


def run_graph(name, want=None, stepwise=True, cont=False, cov=False, **kw):
    """A run of `name` with graph mode on; returns (result, edge arrays, (StatesDigest of every delivered state, kept
    rows or None), per-level edge counts, coverage or None); `want`: the fixture entry the run is expected to equal,
    if not its own.  graph keywords (chunk_parents, map_log2) go to set_graph, the others to the configuration."""
    gkw = {k: kw.pop(k) for k in ("chunk_parents", "map_log2") if k in kw}
    e = GRAPH[want or name]
    with make(name, **kw) as mc:
        keep = e["states"] <= ALL_STATES_MAX
        digest = StatesDigest(mc.cfg.n_servers, mc.cfg.n_vals, keep=keep)
        rows = [] if keep else None

        def on_states(gid0, a):
            digest.update(gid0, a)  # (asserts ascending gids without a gap)
            if keep:
                rows.append(a.copy())
            return 0

        src, key, dst = [], [], []

        def on_edges(s, k, d):
            src.append(s.copy())
            key.append(k.copy())
            dst.append(d.copy())
            return 0

        mc.set_graph(on_states=on_states, on_edges=on_edges, **gkw)
        if cont:
            mc.set_continue()
        if cov:
            mc.set_coverage()
        per_level = []
        if stepwise:
            ls = mc.init()
            assert digest.count == 1 and not src  # Init is delivered by init(), no edge yet
            while ls.status == "ok":
                ls = mc.step()
                per_level.append(sum(len(x) for x in src))
            res = mc.result()
        else:
            res = mc.run()
        coverage = mc.coverage() if cov else None
        n, V = mc.cfg.n_servers, mc.cfg.n_vals
        dicts = [raftmc.unpacked_to_state(r.tolist(), n, V) for part in rows for r in part] if keep else None
    cat = lambda parts, t: np.concatenate(parts) if parts else np.zeros(0, dtype=t)  # noqa: E731
    return res, (cat(src, np.uint64), cat(key, np.uint32), cat(dst, np.uint64)), (digest, dicts), per_level, coverage


def check_entry(name, want=None, **kw):
    e = GRAPH[want or name]
    res, (src, key, dst), (digest, dicts), per_level, _ = run_graph(name, want=want, **kw)
    assert (digest.count, len(src)) == (e["states"], e["edges"])
    assert res.distinct == e["states"]
    if e["verdict"] == "ok":
        assert len(src) == res.generated - 1
    if per_level:
        assert per_level == e["edges_per_level"]
    assert edges_sha256(src, key, dst) == e["edges_sha256"]
    assert len(src) == 0 or int(dst.max()) < e["states"]
    assert np.all(src[1:] >= src[:-1])  # ascending src
    assert digest.hexdigest() == e["states_sha256"]
    assert digest.sample_hexdigest() == e["states_sample_sha256"]
    if dicts is not None:  # the plain rendering, line by line and as digests
        assert [(json.dumps(d, sort_keys=True) + "\n").encode() for d in dicts] == digest.lines
        assert states_sha256(dicts) == e["states_sha256"]
        assert states_sha256(dicts[::SAMPLE]) == e["states_sample_sha256"]
    return res


# ---- 1. exact lists, default settings -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FULL))
def test_edges_and_states_equal_the_fixture_element_for_element(name):
    """The binding's own collection, default settings, rmc_run_levels: fails without the feature."""
    with make(name) as mc:
        mc.set_graph()
        res = mc.run()
        check_levels(golden(name), res)
        src, key, dst = mc.graph_edges()
        states = mc.graph_states()
    assert src.dtype == np.uint64 and key.dtype == np.uint32 and dst.dtype == np.uint64
    assert [list(map(int, x)) for x in zip(src, key, dst)] == FULL[name]["edges"]
    assert states == FULL[name]["states"]
    assert len(src) == res.generated - 1 and len(states) == res.distinct


# ---- 2. every kernel variant -------------------------------------------------------------------------------
def test_fixture_covers_the_kernel_variants_and_every_verdict():
    names = [n for n in GRAPH if n != TWIN]
    assert len(names) == 12 and TWIN in GRAPH
    g = {n: golden(n) for n in names}
    assert {g[n]["n"] for n in names} == {2, 3, 4, 5} and {g[n]["V"] for n in names} == {1, 2}
    assert golden("bf_n3_v1_e1_r3").get("become_follower") and "nosym_n3_v1_e1_r3" in names
    assert {GRAPH[n]["verdict"] for n in ERRORS} == {"invariant", "assert", "deadlock", "eval_error"}


@pytest.mark.parametrize("name", list(GRAPH))
def test_counts_levels_and_digests_match_the_fixture(name):
    res = check_entry(name)
    if name != TWIN:
        check_levels(golden(name), res)


# ---- 3. chunk and growth edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(chunk_parents=1), dict(chunk_parents=7), dict(chunk_parents=64), dict(map_log2=4),
                                dict(device_levels=0, stepwise=False), dict(device_levels=4, stepwise=False)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
@pytest.mark.parametrize("name", ["n3_v1_e1_r3", "n4_v1_e1_r3"])
def test_chunk_boundaries_map_growth_and_device_levels(name, kw):
    check_entry(name, **kw)


@pytest.mark.parametrize("name", ["n3_v1_e1_r3", "n4_v1_e1_r3"])
def test_search_on_split_chunks(name, monkeypatch):
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    check_entry(name, chunk_successors=6000, device_levels=1)


# ---- 4. error cuts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_parents", [0, 7])
@pytest.mark.parametrize("name", ERRORS)
def test_error_cuts_equal_the_fixture(name, chunk_parents):
    res = check_entry(name, chunk_parents=chunk_parents)
    assert res.status == GRAPH[name]["verdict"] != "ok"


# ---- 5. composition -----------------------------------------------------------------------------------------
def test_continue_gives_the_graph_of_the_search_that_did_not_stop():
    res = check_entry("seeded_n3_v1_e2_r3", want=TWIN, stepwise=False, cont=True)
    assert res.status == "done"


@pytest.mark.parametrize("name", ["n3_v1_e1_r3", "bf_n3_v1_e1_r3"])
def test_edges_per_action_equal_coverage_generated(name):
    _, (_src, key, _dst), _, _, cov = run_graph(name, cov=True)
    by_action = np.bincount((key >> 16) & 0xFF, minlength=len(raftmc.ACTIONS)).tolist()
    assert by_action == [cov[a][1] for a in raftmc.ACTIONS] == GRAPH[name]["by_action"]


# ---- 6. refusals and limits ---------------------------------------------------------------------------------
def test_refusals():
    with make("n3_v1_e1_r3", virtual_shards=2, chunk_successors=3000, shard_min_states=1) as mc:
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
            mc.set_graph()
    with make("n3_v1_e1_r3") as mc:
        mc.init()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.set_graph()


def test_the_step_that_would_migrate_fails_and_leaves_a_prefix():
    name = "n2_v1_e2_r3"
    with make(name, compact_log2=10, seen_log2=8) as mc:
        mc.set_graph()
        ls = mc.init()
        with pytest.raises(raftmc.RmcError, match="RMC_E_MEMORY") as ei:
            while ls.status == "ok":
                ls = mc.step()
        msg = str(ei.value)
        assert "graph mode keeps both levels resident" in msg and "2^10" in msg and "compact_log2" in msg
        src, key, dst = mc.graph_edges()
        states = mc.graph_states()
    assert 0 < len(states) < GRAPH[name]["states"]
    assert [list(map(int, x)) for x in zip(src, key, dst)] == FULL[name]["edges"][:len(src)]
    assert states == FULL[name]["states"][:len(states)]


def test_a_failing_sink_ends_the_run_and_the_context_is_destroyed_cleanly():
    calls = [0]

    def on_edges(s, k, d):
        calls[0] += 1
        return calls[0] == 2

    mc = make("n3_v1_e1_r3")
    mc.set_graph(states=False, on_edges=on_edges)
    ls = mc.init()
    with pytest.raises(raftmc.RmcError, match="RMC_E_SINK"):
        while ls.status == "ok":
            ls = mc.step()
    assert calls[0] == 2
    mc.close()
    assert mc.h is None


def test_a_sink_that_fails_on_init_ends_the_run():
    mc = make("n3_v1_e1_r3")
    mc.set_graph(on_states=lambda gid0, a: 1)
    with pytest.raises(raftmc.RmcError, match="RMC_E_SINK"):
        mc.init()
    with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
        mc.init()
    with pytest.raises(raftmc.RmcError, match="RMC_E_SINK"):
        mc.step()
    mc.close()
    assert mc.h is None


def test_switching_graph_mode_off_and_on_again_on_one_checker():
    """clear_graph keeps the buffers; the next graph run starts from an empty map."""
    name = "n3_v1_e1_r3"
    with make(name) as mc:
        for _ in range(2):
            mc.reset()
            mc.set_graph(states=False)
            res = mc.run()
            src, key, dst = mc.graph_edges()
            assert len(src) == res.generated - 1 and edges_sha256(src, key, dst) == GRAPH[name]["edges_sha256"]
            mc.reset()
            mc.clear_graph()
            check_levels(golden(name), mc.run())


# ---- 7. off path ---------------------------------------------------------------------------------------------
def test_off_by_default():
    with make("n3_v1_e1_r3") as mc:
        res = mc.run()
        check_levels(golden("n3_v1_e1_r3"), res)
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_edges()


# ---- 8. launcher ---------------------------------------------------------------------------------------------
def _normal(out):
    out = re.sub(r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d", "<time>", out)
    out = re.sub(r"\(\d+ d?s/min\)", "(<rate>)", out)
    out = re.sub(r"Finished in [\d.]+s", "Finished in <s>", out)
    return re.sub(r"(?m)^GPU: .*$", "GPU: <rate>", out)


def test_launcher_dump_and_dot(tmp_path):
    from test_host import LAUNCHER, cfg_text
    name = "n2_v1_e2_r3"
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=2, R=3, servers="s1, s2", vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    base = [LAUNCHER, "-deadlock", "-workers", "4", "-config", str(tmp_path / "Raft.cfg")]
    tla = str(tmp_path / "Raft.tla")
    runs = [subprocess.run(base + extra + [tla], capture_output=True, text=True, env=env, timeout=120)
            for extra in ([], ["-dump", str(tmp_path / "g")], ["-dump", "dot,actionlabels", str(tmp_path / "g")])]
    for r in runs:
        assert r.returncode == runs[0].returncode == 0, r.stdout + r.stderr
        assert _normal(r.stdout) == _normal(runs[0].stdout)
    states, edges = FULL[name]["states"], FULL[name]["edges"]
    assert (tmp_path / "g.dump").read_text() == dump_text(states, ["s1", "s2"], ["v1"])
    assert (tmp_path / "g.dot").read_text() == dot_text(states, edges, ["s1", "s2"], ["v1"], True)
