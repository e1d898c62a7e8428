"""The search from given root states (rmc_init_from) on the GPU, against tests/golden/roots.json.gz (the C oracle,
tests/golden/make_golden_roots.py).  Integers and digests: every comparison is exact.

The suite's other searches start at Init, and msgs only grows (Raft.tla:43-45): none of them gets to a state with
more than 26 messages at 4-5 servers or more than 44 at 3.  Here a level of 200-260 roots with up to 126 messages
(45-64 on the 64-lane kernels) stands in Init's place and the ordinary search runs two levels from it, so the
batch kernels' second message round (ids 64..127) -- the cross-round ranks of write_ids, the per-round ballots of
the item kernels, the split probe's fingerprint rebuilt from the parent's core, the LDS-staged commit of records
with 65..128 ids, the outbox and regrouping of such records in a sharded round -- and the capacity error of a
level run inside a search, on every execution path.

Timing of this file on an MI355X is in the pull request that added it; each case is one entry on one path."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN
from graph_render import StatesDigest, edges_sha256
from test_gpu import LEVELS, LEVELS_BF, check_levels

pytestmark = pytest.mark.gpu

with gzip.open(os.path.join(GOLDEN, "roots.json.gz"), "rt") as _f:
    ROOTS = json.load(_f)
COUNTING = ["n5_v1", "n4_v1", "n5_v2", "bf_n5_v1", "n3_v2"]
ALL7 = tuple(raftmc.INVARIANT_BY_BIT)

# path -> (environment, configuration keywords, how a level is driven).  "steps": rmc_steps with room for one
# level, i.e. a one-level batch of the device-driven loop; "step": rmc_step, the host drives the level.
SPLIT = {"RMC_SPLIT_MIN": "1"}
PATHS = {
    "device_loop": ({}, {}, "steps"),
    "host": ({}, dict(device_levels=1), "step"),
    "split_nolookahead": ({**SPLIT, "RMC_LOOKAHEAD": "0"}, dict(device_levels=1), "step"),
    "split_lookahead": ({**SPLIT, "RMC_LOOKAHEAD": "1"}, dict(device_levels=1), "step"),
    "split_nodedup": ({**SPLIT, "RMC_PROBE_DEDUP": "0"}, dict(device_levels=1), "step"),
    "split_dedup_small": ({**SPLIT, "RMC_PROBE_DEDUP": "4"}, dict(device_levels=1), "step"),
    # the smallest chunk the engine takes, 64 parents: the levels are cut into several chunks (and with split
    # chunks the next one is expanded while the current one commits)
    "chunks": ({}, dict(device_levels=1, chunk_successors=1), "step"),
    "chunks_split": (SPLIT, dict(device_levels=1, chunk_successors=1), "step"),
    # (a small chunk: the move to the compact table first grows the chunk buffers to their full size)
    "compact": ({}, dict(device_levels=1, compact_log2=10, seen_log2=8, seen_mem_bytes=8 << 22,
                         frontier_mem_bytes=512 << 20, chunk_successors=100000), "step"),
    "virtual2": ({}, dict(virtual_shards=2, chunk_successors=20000), "step"),
    "virtual3": ({}, dict(virtual_shards=3, chunk_successors=20000), "step"),
    "virtual2_split": (SPLIT, dict(virtual_shards=2, chunk_successors=20000), "step"),
    "virtual3_split": (SPLIT, dict(virtual_shards=3, chunk_successors=20000), "step"),
}


def make(e, env, monkeypatch, **kw):
    for k, v in env.items():  # (the library reads them when a checker is created)
        monkeypatch.setenv(k, v)
    if kw.get("virtual_shards"):
        kw.setdefault("shard_min_states", e["m"] + 1)
    return raftmc.ModelChecker(raftmc.ModelConfig(
        n_servers=e["n"], n_vals=e["V"], max_election=e["E"], max_restart=e["R"],
        spec_variant=raftmc.SPEC_BECOME_FOLLOWER if e["bf"] else raftmc.SPEC_RAFT, **kw))


def rows_of(e, lanes=None):
    stride = raftmc.unpacked_len(e["n"], e["V"], lanes or e["lanes"])
    a = np.zeros((len(e["roots"]), stride), dtype=np.int32)
    for i, r in enumerate(e["roots"]):
        a[i, :len(r)] = r
    return a


def root_state(e, gid):
    """The kept root with global id gid, as a state dict (the first root of each class, argument order)."""
    cfg = R.Config(n=e["n"], V=e["V"], max_election=e["E"], max_restart=e["R"], become_follower=e["bf"])
    seen = {}
    for r in e["roots"]:
        d = raftmc.unpacked_to_state(r, e["n"], e["V"])
        c = R.canonical(cfg, R.state_from_json(d))
        if c not in seen:
            if len(seen) == gid:
                return d
            seen[c] = 1
    raise AssertionError(gid)


def key(ls):
    return dict(level=ls.level, expanded=ls.expanded, generated=ls.generated, new_states=ls.new_states,
                self_loops=ls.self_loops, total_generated=ls.total_generated, total_distinct=ls.total_distinct,
                queue=ls.queue)


def seed(mc, e, lanes=None):
    ls = mc.init_from(rows_of(e, lanes))
    assert (ls.level, ls.status, ls.expanded, ls.new_states, ls.total_generated, ls.total_distinct, ls.queue) == \
           (1, "ok", 0, e["m"], e["n_given"], e["m"], e["m"])
    return ls


def expand(mc, how):
    if how == "step":
        return mc.step()
    out = mc.steps(cap=2)
    assert len(out) == 1
    return out[0]


def want(e, k):
    return {x: e["levels"][k][x] for x in ("level", "expanded", "generated", "new_states", "self_loops",
                                           "total_generated", "total_distinct", "queue")}


def check_counting(e, path, monkeypatch, lanes=None, **extra):
    env, kw, how = PATHS[path]
    with make(e, env, monkeypatch, **kw, **extra) as mc:
        seed(mc, e, lanes)
        for k in range(2):
            ls = expand(mc, how)
            print(path, key(ls))
            assert ls.status == "ok" and key(ls) == want(e, k)
            res = mc.result()
            assert (res.depth, res.queue, res.generated, res.distinct) == \
                   (k + 2, e["levels"][k]["queue"], e["levels"][k]["total_generated"], e["levels"][k]["total_distinct"])
        if path == "compact":
            assert res.seen_slot_bytes == 8
        # a state of level 3 leads back to a root in two steps
        keys, gids = mc.state_path(e["states"] - 1)
        assert len(keys) == 2 and len(gids) == 3 and gids[0] < e["m"] <= gids[1] < e["levels"][0]["total_distinct"]


# ---- 1. the counting entries, level by level, on every path ------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", COUNTING)
def test_levels_from_roots(name, path, monkeypatch):
    check_counting(ROOTS[name], path, monkeypatch)


@pytest.mark.parametrize("path", ["device_loop", "host", "split_lookahead", "chunks_split", "virtual2", "virtual2_split"])
def test_n3_v2_on_128_lanes_gives_the_same_numbers(path, monkeypatch):
    """The 64-lane entry on the 128-lane kernels of (3, 2): roots of 45..64 messages, the first round full."""
    check_counting(ROOTS["n3_v2"], path, monkeypatch, lanes=128, msg_cap=128)


# ---- 2. graph mode: the whole seeded graph -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "split", "chunk16", "chunk50"])
@pytest.mark.parametrize("name", COUNTING)
def test_graph_from_roots(name, mode, monkeypatch):
    e = ROOTS[name]
    env = SPLIT if mode == "split" else {}
    gkw = dict(chunk_parents=int(mode[5:])) if mode.startswith("chunk") else {}
    with make(e, env, monkeypatch, device_levels=1) as mc:
        digest = StatesDigest(e["n"], e["V"])
        src, k32, dst, per_level = [], [], [], []

        def on_states(gid0, a):
            digest.update(gid0, a)
            return 0

        def on_edges(s, k, d):
            src.append(s.copy()); k32.append(k.copy()); dst.append(d.copy())
            return 0

        mc.set_graph(on_states=on_states, on_edges=on_edges, **gkw)
        seed(mc, e)
        assert digest.count == e["m"] and not src  # the roots are level 1, without edges
        for k in range(2):
            ls = mc.step()
            assert key(ls) == want(e, k)
            per_level.append(sum(len(x) for x in src))
    assert per_level == e["edges_per_level"] and digest.count == e["states"]
    src, k32, dst = np.concatenate(src), np.concatenate(k32), np.concatenate(dst)
    assert len(src) == e["edges"] == e["levels"][1]["total_generated"] - e["n_given"]
    assert np.all(src[1:] >= src[:-1]) and int(dst.max()) < e["states"]
    assert edges_sha256(src, k32, dst) == e["edges_sha256"]
    assert digest.hexdigest() == e["states_sha256"]


def test_keep_delivers_the_roots_as_level_1(monkeypatch):
    e = ROOTS["n4_v1"]
    with make(e, {}, monkeypatch, device_levels=1) as mc:
        mc.set_graph_keep()
        seed(mc, e)
        mc.step()
        sh = mc.graph_shape()
        assert (sh["states"], sh["edges"]) == (e["levels"][0]["total_distinct"], e["levels"][0]["generated"])
        assert len(mc.graph_inv_values()) == sh["states"]


# ---- 3. coverage --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "split", "virtual2"])
@pytest.mark.parametrize("name", COUNTING)
def test_coverage_from_roots(name, mode, monkeypatch):
    e = ROOTS[name]
    kw = dict(virtual_shards=2, chunk_successors=20000) if mode == "virtual2" else {}
    with make(e, SPLIT if mode == "split" else {}, monkeypatch, **kw) as mc:
        mc.set_coverage()
        seed(mc, e)
        for k in range(2):
            assert key(mc.step()) == want(e, k)
        cov = mc.coverage()
    exp = {"Init": (e["m"], e["n_given"])}
    for a, act in enumerate(raftmc.ACTIONS):
        exp[act] = (e["coverage"]["distinct"][a], e["coverage"]["generated"][a])
    assert cov == exp


# ---- 4. continuation: all seven invariants, counted per level ---------------------------------------------
@pytest.mark.parametrize("path", ["host", "device_loop", "split_lookahead", "virtual2"])
@pytest.mark.parametrize("name", COUNTING)
def test_continuation_from_roots(name, path, monkeypatch):
    e = ROOTS[name]
    env, kw, how = PATHS[path]
    with make(e, env, monkeypatch, invariants=ALL7, **kw) as mc:
        mc.set_continue()
        seed(mc, e)
        for k in range(2):
            ls = expand(mc, how)
            assert ls.status == "ok" and key(ls) == want(e, k)
        got = {nm: mc.violation_levels(nm) for nm in ALL7}
        viol = mc.violations()
    assert got == e["continuation"]
    for nm in ALL7:
        lv = e["continuation"][nm]
        assert viol[nm] == (sum(lv), next((i + 1 for i, c in enumerate(lv) if c), None))


# ---- 5. the error entries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "device_loop", "split_lookahead", "virtual2", "virtual2_split"])
@pytest.mark.parametrize("name", ["cap_n5_v1", "cap_n3_v2"])
def test_capacity_error_of_a_level(name, path, monkeypatch):
    """A state of level 2 has a successor one message past the lanes: level 1 expands with the recorded
    numbers, the expansion of level 2 fails with RMC_E_CAPACITY (the chunk flag's read-back in the fused and
    split chunks, in the device loop and in a sharded round)."""
    e = ROOTS[name]
    env, kw, how = PATHS[path]
    assert e["stop"] == dict(status="capacity", level=2, parent_gid=e["stop"]["parent_gid"])
    with make(e, env, monkeypatch, **kw) as mc:
        seed(mc, e)
        ls = expand(mc, how)
        assert ls.status == "ok" and key(ls) == want(e, 0)
        with pytest.raises(raftmc.RmcError, match="RMC_E_CAPACITY.*exceeds msg_cap = %d" % e["lanes"]):
            expand(mc, how)


def test_a_root_past_the_lanes_is_refused(monkeypatch):
    e = ROOTS["n3_v2"]
    with make(e, {}, monkeypatch) as mc:
        a = rows_of(e, lanes=72)
        col = raftmc.unpacked_len(e["n"], e["V"], 0) - 1
        i, was = int(np.argmax(a[:, col])), int(a[:, col].max())
        a[i, col] = 65  # (the slots past its messages hold zeros; they are never looked at: the count is checked first)
        with pytest.raises(raftmc.RmcError, match="RMC_E_CAPACITY"):
            mc.init_from(a)
        a[i, col] = was
        a[3, 0] = 7  # votedFor out of range
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG.*votedFor"):
            mc.init_from(a)
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
            mc.init_from(a[:0])
        a[3, 0] = -1  # nothing was seeded by the refused calls: the same checker takes the repaired rows
        seed(mc, e, lanes=72)


@pytest.mark.parametrize("path", ["host", "device_loop", "split_lookahead", "virtual2"])
def test_assert_at_a_root(path, monkeypatch):
    """The expansion of a root in the middle of level 1 hits UpdateTerm's Assert: verdict, counters at the stop,
    queue and the one-state trace are the oracle's, and the trace ends at that root -- not at gid 0."""
    e = ROOTS["assert_n5_v1"]
    s = e["stop"]
    env, kw, how = PATHS[path]
    with make(e, env, monkeypatch, **kw) as mc:
        seed(mc, e)
        ls = expand(mc, how)
        assert (ls.status, ls.level, ls.generated, ls.new_states, ls.total_generated, ls.total_distinct, ls.queue) == \
               ("assert", 1, s["level_generated"], s["level_new"], s["generated"], s["distinct"], s["queue"])
        res = mc.result()
        assert (res.status, res.depth, res.generated, res.distinct, res.queue, res.violated) == \
               ("assert", s["depth"], s["generated"], s["distinct"], s["queue"], None)
        assert s["parent_gid"] != 0
        assert mc.trace() == [(None, root_state(e, s["parent_gid"]))]
        assert mc.state_path(s["parent_gid"]) == ([], [s["parent_gid"]])
        keys, gids = mc.state_path(s["distinct"] - 1)  # the last state found before the stop
        assert len(keys) == 1 and gids[0] <= s["parent_gid"] and gids[1] == s["distinct"] - 1


@pytest.mark.parametrize("shards", [0, 2])
def test_invariant_false_at_a_root(shards, monkeypatch):
    """Inv is FALSE on a root behind clean ones, and an earlier root has a server-permuted twin (n > m): the
    verdict is Init's, the trace holds that root alone."""
    e = ROOTS["invroot_n3_v2"]
    s = e["stop"]
    with make(e, {}, monkeypatch, **(dict(virtual_shards=shards) if shards else {})) as mc:
        ls = mc.init_from(rows_of(e))
        assert (ls.status, ls.level, ls.new_states, ls.total_generated, ls.total_distinct, ls.queue) == \
               ("invariant", 1, e["m"], e["n_given"], e["m"], 0)
        res = mc.result()
        assert (res.status, res.violated, res.depth, res.generated, res.distinct, res.queue) == \
               ("invariant", "Inv", 1, s["generated"], s["distinct"], 0)
        assert s["root_gid"] != 0 and e["n_given"] == e["m"] + 1
        assert mc.trace() == [(None, root_state(e, s["root_gid"]))]
        assert mc.state_path(s["root_gid"]) == ([], [s["root_gid"]])


def test_continuation_counts_a_violating_root_at_level_1(monkeypatch):
    e = ROOTS["invroot_n3_v2"]
    with make(e, {}, monkeypatch, device_levels=1) as mc:
        mc.set_continue()
        ls = mc.init_from(rows_of(e))
        assert ls.status == "ok" and ls.queue == e["m"]
        assert mc.violations() == {"Inv": (1, 1)} and mc.violation_levels("Inv") == [1]
        assert mc.violation_trace("Inv") == [(None, root_state(e, e["stop"]["root_gid"]))]


# ---- 6. the hook itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,levels", [("n3_v2_e1_r3", LEVELS), ("bf_n3_v1_e1_r3", LEVELS_BF)])
def test_seeded_run_then_reset_and_the_plain_run(name, levels, monkeypatch):
    """Seeded with Init's successors the search finds every state but Init (terms only grow: Init is not
    reached again), twice in a row; then reset() + init() + run() is the plain run: Init's cached record,
    fingerprint and verdicts were not overwritten."""
    g = levels[name]
    bf = bool(g.get("become_follower"))
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"], become_follower=bf)
    succ = [R.state_to_json(t) for _, t in R.successors(cfg, R.init_state(cfg))]
    classes = {R.canonical(cfg, R.state_from_json(d)) for d in succ}
    kw = dict(n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
              spec_variant=raftmc.SPEC_BECOME_FOLLOWER if bf else raftmc.SPEC_RAFT)
    with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
        plain = mc.run()  # first the plain run, so that Init is cached before the seeded ones
        check_levels(g, plain)
        for _ in range(2):
            mc.reset()
            ls = mc.init_from(succ)
            assert (ls.new_states, ls.total_generated, ls.total_distinct) == (len(classes), len(succ), len(classes))
            res = mc.run()
            assert (res.status, res.generated, res.distinct, res.depth) == \
                   ("done", g["generated"] - 1, g["distinct"] - 1, g["depth"] - 1)
            assert [l.new_states for l in res.levels if l.new_states] == g["levels"][1:]
        mc.reset()
        mc.init()
        check_levels(g, mc.run())


def test_seeding_twice_gives_the_same_levels(monkeypatch):
    e = ROOTS["n4_v1"]
    with make(e, {}, monkeypatch, device_levels=1) as mc:
        for _ in range(2):
            seed(mc, e)
            assert [key(mc.step()) for _ in range(2)] == [want(e, 0), want(e, 1)]
            with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
                mc.init_from(rows_of(e))  # the run has begun
            mc.reset()


def test_refusals(monkeypatch, tmp_path):
    e = ROOTS["cap_n3_v2"]
    # shard_min_states <= m: the roots would have to enter the sharded layout at once
    for sm in (1, e["m"]):
        with make(e, {}, monkeypatch, virtual_shards=2, shard_min_states=sm) as mc:
            with pytest.raises(raftmc.RmcError, match="RMC_E_STATE.*shard_min_states"):
                mc.init_from(rows_of(e))
    # checkpoint of a seeded run: the file format has no place for the roots
    with make(e, {}, monkeypatch, device_levels=1) as mc:
        seed(mc, e)
        mc.step()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE.*rmc_init_from"):
            mc.checkpoint(str(tmp_path / "seeded.ckpt"))
        assert not os.path.exists(tmp_path / "seeded.ckpt")


def test_refused_on_an_rccl_rank(monkeypatch):
    e = ROOTS["cap_n3_v2"]
    with make(e, {}, monkeypatch, world_size=1, rank=0, comm_unique_id=raftmc.comm_unique_id()) as mc:
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE.*RCCL"):
            mc.init_from(rows_of(e))


def test_refused_on_the_host_staged_transport(monkeypatch):
    """A rank of the host-staged transport (world_size > 1 without a communicator): callbacks that stand for a
    world of one are enough to create the context; the hook refuses before it calls any."""
    e = ROOTS["cap_n3_v2"]

    def allreduce(_u, _v, _n, _is_max):
        return 0

    def allgather(_u, row, k, out):
        for q in range(2):
            for i in range(k):
                out[q * k + i] = row[i]
        return 0

    def alltoallv(*_a):
        return 0

    t = raftmc._Transport(None, raftmc._ALLREDUCE(allreduce), raftmc._ALLGATHER(allgather), raftmc._ALLTOALLV(alltoallv))
    lib = raftmc.load_library()
    assert lib.rmc_set_transport(ctypes.byref(t)) == 0
    try:
        with make(e, {}, monkeypatch, world_size=2, rank=0) as mc:
            with pytest.raises(raftmc.RmcError, match="RMC_E_STATE.*host-staged"):
                mc.init_from(rows_of(e))
    finally:
        lib.rmc_set_transport(None)
