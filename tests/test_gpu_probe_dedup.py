"""The probe pass's table of recent fingerprints (RMC_PROBE_DEDUP, rmc_kernels.hip k_hash_probe): in a
single-GPU split chunk each wave drops the successors whose fingerprint an earlier successor of its own
has, before the seen-set probe and the election -- their verdict, "not a winner", is the one they would
get there.  Nothing a run reports may change: counts per level, TLC's order (the counterexamples) and the
error precedence.

As tests/test_gpu_lookahead.py, every case splits every chunk (RMC_SPLIT_MIN=1) and drives the levels from
the host (device_levels=1); most take chunks of 6000 successor slots.  RMC_PROBE_DEDUP=8 leaves a wave
eight entries, so nearly every round has two fingerprints on one entry and evicts; RMC_PROBE_RUN makes a
wave take several groups of 64 parents in a row, its table carrying over."""
import json
import os
import re

import pytest

import raftmc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


LEVELS = load("levels.json")
TRACES = load("traces.json")
LEVELS_BF = load("levels_bf.json")
LEVELS_ERR = load("levels_errors.json")
TRACES_ERR = load("traces_errors.json")

CHUNK = 6000
KW = dict(device_levels=1, chunk_successors=CHUNK)


# the helpers of tests/test_gpu_lookahead.py
def spec_of(g):
    if g.get("become_follower"):
        return raftmc.SPEC_BECOME_FOLLOWER
    if g.get("variant"):
        return {"split_brain": raftmc.SPEC_SPLIT_BRAIN, "commit_past_log": raftmc.SPEC_COMMIT_PAST_LOG}[g["variant"]]
    return raftmc.SPEC_SEEDED if g["seeded"] else raftmc.SPEC_RAFT


def run_cfg(g, **kw):
    mc = raftmc.ModelChecker(raftmc.ModelConfig(
        n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
        invariants=tuple(g["invariants"]), check_deadlock=g["check_deadlock"],
        spec_variant=spec_of(g), **kw))
    res = mc.run()
    return mc, res


def check_levels(g, res):
    assert res.status == {"ok": "done"}.get(g["verdict"], g["verdict"])
    assert res.generated == g["generated"] and res.distinct == g["distinct"]
    if g["verdict"] == "ok":
        assert res.depth == g["depth"]
        assert [ls.new_states for ls in res.levels if ls.new_states] == g["levels"]
        assert [ls.generated for ls in res.levels[1:]] == g["gen_per_level"]
        assert res.queue == 0
    else:
        assert res.trace_len == g["trace_len"]
        assert res.queue == g["queue_left"]
        if g["verdict"] == "invariant":
            assert res.violated == g["violated"]


def trace_of(mc):
    return [(list(k) if k else None, st) for k, st in mc.trace()]


def golden_trace(t):
    return [(e["key"], e["state"]) for e in t["steps"]]


def level_counts(res):
    return [(ls.expanded, ls.generated, ls.new_states, ls.self_loops, ls.new_bytes) for ls in res.levels]


LOG_LINE = re.compile(r"rmc probe_dedup: level (\d+) fingerprinted (\d+) dropped (\d+)")


def dropped_per_level(err):
    """[(level, fingerprinted, dropped)] from the engine's RMC_PROBE_DEDUP_LOG lines."""
    return [tuple(int(v) for v in m.groups()) for m in LOG_LINE.finditer(err)]


@pytest.fixture
def split_all(monkeypatch):
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    monkeypatch.delenv("RMC_PROBE_RUN", raising=False)
    monkeypatch.delenv("RMC_PROBE_DEDUP", raising=False)
    return monkeypatch


@pytest.mark.parametrize("name", ["n3_v2_e1_r3", "n3_v1_e2_r3", "n4_v1_e1_r3", "seeded_n3_v2_e2_r3"])
def test_dedup_counts_and_traces_equal_plain_probe(name, split_all):
    """The table at its compiled size, off, and at eight entries: each the golden run, per-level counters
    equal between the three, and the golden counterexample where there is one (it changes if a successor
    that is not the first in TLC order wins)."""
    g = LEVELS[name]
    per_mode = {}
    for mode in ("1", "0", "8"):
        split_all.setenv("RMC_PROBE_DEDUP", mode)
        mc, res = run_cfg(g, **KW)
        check_levels(g, res)
        per_mode[mode] = level_counts(res)
        if name in TRACES:
            assert trace_of(mc) == golden_trace(TRACES[name])
        mc.close()
    assert per_mode["1"] == per_mode["0"] == per_mode["8"]


@pytest.mark.parametrize("run,entries", [("16", "1"), ("3", "8"), ("1", "1")])
def test_dedup_one_chunk_per_level(run, entries, split_all):
    """The default chunk size: the widest level (20,503 parents) is one chunk.  With runs of 16 groups a
    wave keeps its table over 1024 parents in a row; runs of 3 do not divide the level's groups."""
    split_all.setenv("RMC_PROBE_DEDUP", entries)
    split_all.setenv("RMC_PROBE_RUN", run)
    g = LEVELS["n3_v1_e2_r3"]
    mc, res = run_cfg(g, device_levels=1)
    check_levels(g, res)
    mc.close()


@pytest.mark.parametrize("name", ["bf_n3_v1_e2_r3", "bf_n4_v1_e1_r3"])
def test_dedup_sparse_layout(name, split_all):
    """The chunks whose winners the items commit does not take (k_insert_winners + k_commit_split on
    the sparse slot layout, LS_SEEN = not a candidate): the BecomeFollower variant."""
    split_all.setenv("RMC_PROBE_DEDUP", "1")
    g = LEVELS_BF[name]
    mc, res = run_cfg(g, **KW)
    check_levels(g, res)
    mc.close()


@pytest.mark.parametrize("name", ["sb_n3_v1_e3_r3", "sb_n3_v2_e2_r3"])
def test_dedup_errors(name, split_all):
    """An invariant violation and an Assert with the table on: TLC's verdict, the counters at the error
    and the counterexample."""
    split_all.setenv("RMC_PROBE_DEDUP", "1")
    g = LEVELS_ERR[name]
    mc, res = run_cfg(g, **KW)
    check_levels(g, res)
    assert [ls.new_states for ls in res.levels if ls.new_states][:len(g["levels"]) - 1] == g["levels"][:-1]
    assert trace_of(mc) == golden_trace(TRACES_ERR[name])
    mc.close()


def test_dedup_drops_repeats(split_all, capfd):
    """The table does drop: with it on, the dropped successors of n3_v2_e1_r3 are more than none and at
    most the fingerprinted successors that are not new states (generated - self-loops - distinct), level by
    level too; with it off, none."""
    g = LEVELS["n3_v2_e1_r3"]
    split_all.setenv("RMC_PROBE_DEDUP_LOG", "1")
    dropped = {}
    for mode in ("1", "8", "0"):
        split_all.setenv("RMC_PROBE_DEDUP", mode)
        capfd.readouterr()
        mc, res = run_cfg(g, **KW)
        check_levels(g, res)
        mc.close()
        rows = dropped_per_level(capfd.readouterr().err)
        stats = {ls.level: ls for ls in res.levels}
        assert len(rows) == len(res.levels) - 1  # every level but Init's
        for level, fingerprinted, drop in rows:
            ls = stats[level]
            assert fingerprinted == ls.generated - ls.self_loops
            assert drop <= fingerprinted - ls.new_states
        dropped[mode] = sum(r[2] for r in rows)
    print(f"dropped of {res.generated - 1 - sum(ls.self_loops for ls in res.levels)} fingerprinted: {dropped}")
    self_loops = sum(ls.self_loops for ls in res.levels)
    for mode in ("1", "8"):
        assert 0 < dropped[mode] <= res.generated - self_loops - res.distinct
    assert dropped["0"] == 0
