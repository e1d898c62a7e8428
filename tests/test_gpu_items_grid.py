"""Grids of a split chunk's expansion and items commit (RMC_ITEMS_GRID, rmc_engine.hip size_items_grids):
both kernels' blocks stride over batches of 64 parents (b0 += gridDim.x * PB), and the grid is a few resident
generations of blocks, so a block of a large chunk takes several batches.

Every case splits every chunk (RMC_SPLIT_MIN=1), drives the levels from the host (device_levels=1) and
takes chunks of 40000 successor slots: 454-470 parents at n = 3 (8 batches, the last partial), 231-250 at
n = 4 and 5 (4 batches).  With RMC_ITEMS_GRID=1 one block walks all the batches of a chunk, with 3 the blocks
take uneven shares, unset the residency-derived grid exceeds the batches and every block takes one.  The
results must be the golden ones (tests/golden/, from oracle/) and equal across the grids."""
import json
import os

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

CHUNK = 40000
KW = dict(device_levels=1, chunk_successors=CHUNK)
GRIDS = ("1", "3", None)


# the helpers of tests/test_gpu.py
def spec_of(g):
    if g.get("become_follower"):
        return raftmc.SPEC_BECOME_FOLLOWER
    return raftmc.SPEC_SEEDED if g["seeded"] else raftmc.SPEC_RAFT


def run_cfg(g, **kw):
    mc = raftmc.ModelChecker(raftmc.ModelConfig(
        n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
        invariants=tuple(g["invariants"]), check_deadlock=g["check_deadlock"],
        spec_variant=spec_of(g), **kw))
    res = mc.run()
    return mc, res


def check_levels(g, res):
    assert g["verdict"] == "ok"
    assert res.status == "done"
    assert res.generated == g["generated"] and res.distinct == g["distinct"]
    assert res.depth == g["depth"]
    assert [ls.new_states for ls in res.levels if ls.new_states] == g["levels"]
    assert [ls.generated for ls in res.levels[1:]] == g["gen_per_level"]
    assert res.queue == 0


def trace_of(mc):
    return [(list(k) if k else None, st) for k, st in mc.trace()]


def golden_trace(t):
    return [(e["key"], e["state"]) for e in t["steps"]]


def level_counts(res):
    return [(ls.expanded, ls.generated, ls.new_states, ls.self_loops, ls.new_bytes) for ls in res.levels]


def chunk_parents(g):
    """Parents per chunk (rmc_engine.hip setup: Gcap / maxsucc; maxsucc = Spec::MAXS of one message round
    for n <= 3, two above, and msg_cap more under BecomeFollower)."""
    n = g["n"]
    cap = 64 if n <= 3 else 128
    maxsucc = cap + n * (4 + g["V"] + n - 1) + (cap if g.get("become_follower") else 0)
    return max(CHUNK, 64 * maxsucc) // maxsucc


def set_grid(mp, grid):
    if grid is None:
        mp.delenv("RMC_ITEMS_GRID", raising=False)
    else:
        mp.setenv("RMC_ITEMS_GRID", grid)


@pytest.fixture
def split_all(monkeypatch):
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    return monkeypatch


def across_grids(g, name, mp, batches):
    """The golden run at every grid, the golden trace where there is one; returns the per-level counters,
    which must not depend on the grid."""
    cp = chunk_parents(g)
    assert -(-cp // 64) == batches and max(g["levels"]) >= cp  # some chunk has that many batches
    counts = []
    for grid in GRIDS:
        set_grid(mp, grid)
        mc, res = run_cfg(g, **KW)
        check_levels(g, res)
        counts.append(level_counts(res))
        if name in TRACES:
            assert trace_of(mc) == golden_trace(TRACES[name])
        mc.close()
    assert counts[0] == counts[1] == counts[2]
    return counts[0]


@pytest.mark.parametrize("name", ["n3_v2_e1_r3", "n3_v1_e2_r3"])
def test_items_grid_n3(name, split_all):
    """Eight batches per chunk, the last partial: one block for all of them, three blocks with shares of
    3, 3 and 2, and a block each -- with the next chunk's expansion looked ahead and in series."""
    g = LEVELS[name]
    per_mode = []
    for mode in ("1", "0"):
        split_all.setenv("RMC_LOOKAHEAD", mode)
        per_mode.append(across_grids(g, name, split_all, 8))
    assert per_mode[0] == per_mode[1]


@pytest.mark.parametrize("name", ["n4_v1_e1_r3", "n5_v1_e1_r3"])
def test_items_grid_wide_cores(name, split_all):
    """The wider cores and the 48-B staging rows of n = 4 and 5: four batches per chunk."""
    across_grids(LEVELS[name], name, split_all, 4)


@pytest.mark.parametrize("name", ["bf_n3_v1_e2_r3", "bf_n4_v1_e1_r3"])
def test_items_grid_become_follower(name, split_all):
    """The BecomeFollower variant's kernels (two candidates per message item).  At n = 3 a parent's 149
    slots still fit the items commit; at n = 4 (288 slots) the chunks keep the sparse slot layout and
    commit through k_insert_winners and k_commit_split, whose grids the knob does not set -- their
    expansion's it does."""
    g = LEVELS_BF[name]
    across_grids(g, name, split_all, -(-chunk_parents(g) // 64))


def test_items_grid_single_chunk_levels(split_all):
    """A chunk per level and the grid unset: the narrow levels have fewer batches than the residency-derived
    grid (from one parent up), none has more -- the launch takes min(batches, grid) blocks, never 0."""
    name = "n3_v1_e2_r3"
    g = LEVELS[name]
    set_grid(split_all, None)
    mc, res = run_cfg(g, device_levels=1, chunk_successors=1 << 26)
    check_levels(g, res)
    assert g["levels"][0] == 1 and max(g["levels"]) <= 64 * 2048  # the default grid has at least 2048 blocks
    if name in TRACES:
        assert trace_of(mc) == golden_trace(TRACES[name])
    mc.close()
