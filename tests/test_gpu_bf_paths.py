"""The BecomeFollower variant (Raft.tla:420 uncommented) on the engine paths of its own.

At 4 and 5 servers a BecomeFollower state has 288 / 301 successor slots (msg_cap 128, the servers' slots
and a BecomeFollower candidate per message lane), past the 256 lanes of the items commit
(k_commit_items).  These instantiations keep the sparse slot layout (no hoff), insert a split chunk's
winners in k_insert_winners and commit them in k_commit_split on one GPU, and in a sharded round decide
the shard's own candidates in k_local_flags whether or not the round is split (rmc_engine.hip
step_sharded: round_commit_decides).  Every case here runs one of those paths -- split sharded rounds
(virtual shards, the owner-table rebid, a one-rank RCCL communicator), reset and rerun, split chunks with
and without look-ahead, host-driven fused levels and the device loop, self-loops per level, checkpoint
and resume -- against the oracle's fixtures (tests/golden/levels_bf.json, traces_bf.json), with a
3-server configuration (at most 152 slots: the items commit) as the control."""
import functools
import json
import os

import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


LEVELS_BF = load("levels_bf.json")
TRACES_BF = load("traces_bf.json")

PH_DEDUP, PH_OTHER = 2, 5  # rmc_engine.hip Phase: winner count (+ k_insert_winners); a split chunk's probe pass


# the helpers of tests/test_gpu.py
def spec_of(g):
    if g.get("become_follower"):
        return raftmc.SPEC_BECOME_FOLLOWER
    if g.get("variant"):
        return {"split_brain": raftmc.SPEC_SPLIT_BRAIN, "commit_past_log": raftmc.SPEC_COMMIT_PAST_LOG}[g["variant"]]
    return raftmc.SPEC_SEEDED if g["seeded"] else raftmc.SPEC_RAFT


def model_config(g, **kw):
    return raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
                              invariants=tuple(g["invariants"]), check_deadlock=g["check_deadlock"],
                              spec_variant=spec_of(g), **kw)


def run_cfg(g, **kw):
    mc = raftmc.ModelChecker(model_config(g, **kw))
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


def check_trace(name, mc):
    if name in TRACES_BF:
        assert [(list(k) if k else None, st) for k, st in mc.trace()] == \
               [(e["key"], e["state"]) for e in TRACES_BF[name]["steps"]]


def maxsucc(g):
    """Successor slots per state (rmc_kernels.hip Launch::MX): the message lanes (msg_cap: 64 up to 3 servers,
    128 above), the servers' slots, and a BecomeFollower candidate per message lane."""
    n = g["n"]
    msg_cap = 64 if n <= 3 else 128
    return msg_cap + n * (4 + g["V"] + n - 1) + msg_cap


def test_fixtures_reach_past_the_items_commit():
    """What the cases below rely on: 288 / 301 slots at 4 / 5 servers, the control below 256."""
    assert maxsucc(LEVELS_BF["bf_n4_v1_e1_r3"]) == 288
    assert maxsucc(LEVELS_BF["bf_n5_v1_e1_r3"]) == 301
    assert maxsucc(LEVELS_BF["bf_n3_v2_e1_r3"]) == 152
    assert all(g["become_follower"] for g in LEVELS_BF.values())


# ---- (a) sharded rounds that split ------------------------------------------------------------
SHARDED_SPLIT = ["bf_n4_v1_e1_r3", "bf_n5_v1_e1_r3", "bf_n3_v2_e1_r3", "bf_deadlock_n3_v1_e1_r3",
                 "bf_exist_lc_n3_v1_e2_r3"]


def sharded_kw(mode, monkeypatch, shard_min=1):
    """The layouts of test_sharded_commit_list_matches_golden_levels (64 parents a round and shard)."""
    kw = dict(chunk_successors=3000, shard_min_states=shard_min)
    if mode == "rccl1":
        kw.update(world_size=1, rank=0, comm_unique_id=raftmc.comm_unique_id())
    elif mode == "virtual3_rebid":
        monkeypatch.setenv("RMC_OWNER_LXY", "2")
        kw.update(virtual_shards=3)
    else:
        kw.update(virtual_shards=int(mode[len("virtual"):]))
    return kw


@pytest.mark.parametrize("name,mode", [(n, m) for n in SHARDED_SPLIT for m in ("virtual2", "virtual3_rebid", "rccl1")] +
                         [("bf_n5_v1_e1_r3", "virtual4")])
def test_sharded_split_rounds_match_golden(name, mode, monkeypatch):
    """Every sharded round split (RMC_SPLIT_MIN=1): k_hash_probe bids the shard's own successors in its
    election table (virtual3_rebid: the bids always redone in the owner table), and at 288 / 301 slots the
    commit is k_commit_split, which takes LS_WIN verdicts only -- so k_local_flags must have decided the own
    candidates, inserted the winners and counted them.  An own winner left undecided is a state never
    committed nor inserted: the level sizes fall short of the golden ones.  virtual4 at 5 servers: ranks up
    to 300 in the election key's 10 bits beside four owners."""
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    g = LEVELS_BF[name]
    mc, res = run_cfg(g, **sharded_kw(mode, monkeypatch))
    check_levels(g, res)
    check_trace(name, mc)
    mc.close()


# ---- (b) sharded split, reset, rerun ----------------------------------------------------------
@pytest.mark.parametrize("mode", ["virtual2", "rccl1"])
def test_sharded_split_run_then_reset_reruns_golden(mode, monkeypatch):
    """As test_sharded_run_then_reset_reruns_golden at 288 slots: the first levels replicated (the fused
    election in E), the split sharded rounds after them with their own bids in E under owner keys, reset,
    and twice more: a summary word (SUM_INS_COMMIT) or an owner key left over from a run shows as
    another count."""
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    g = LEVELS_BF["bf_n4_v1_e1_r3"]
    mc, res = run_cfg(g, **sharded_kw(mode, monkeypatch, shard_min=40))
    check_levels(g, res)
    for _ in range(2):
        mc.reset()
        check_levels(g, mc.run())
    mc.close()


# ---- (c) single-GPU split chunks, with and without look-ahead -----------------------------------
CHUNK = 6000
SPLIT_KW = dict(device_levels=1, chunk_successors=CHUNK)
SPLIT_CASES = ["bf_n4_v1_e1_r3", "bf_n5_v1_e1_r3", "bf_n3_v2_e1_r3"]


def chunk_parents(g):
    """Parents per chunk (rmc_engine.hip: max(chunk_successors, 64 maxsucc) / maxsucc)."""
    return max(CHUNK, 64 * maxsucc(g)) // maxsucc(g)


def level_counts(res):
    return [(ls.expanded, ls.generated, ls.new_states, ls.self_loops, ls.new_bytes) for ls in res.levels]


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_split_chunks_with_and_without_lookahead(name, monkeypatch):
    """Every chunk split, host-driven levels: k_insert_winners + k_commit_split on the sparse layout at
    288 / 301 slots (the control: k_commit_items on the dense one), the next chunk expanded ahead or not --
    both the golden run, level by level equal to each other."""
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    g = LEVELS_BF[name]
    assert max(g["levels"]) >= 3 * chunk_parents(g)  # the widest level has at least 3 chunks
    per_mode = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("RMC_LOOKAHEAD", mode)
        mc, res = run_cfg(g, **SPLIT_KW)
        check_levels(g, res)
        per_mode[mode] = level_counts(res)
        mc.close()
    assert per_mode["1"] == per_mode["0"]


@pytest.mark.parametrize("name", ["bf_n4_v1_e1_r3", "bf_n3_v2_e1_r3"])
def test_split_chunks_insert_pass_only_above_256_slots(name, monkeypatch):
    """Which path a split chunk took, from the timed sections per level: one probe pass a chunk (PH_OTHER)
    shows the chunk was split; the winner count's phase (PH_DEDUP) has a second section a chunk, the
    k_insert_winners pass, exactly where the items commit cannot take a parent's slots."""
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    monkeypatch.setenv("RMC_LOOKAHEAD", "0")
    g = LEVELS_BF[name]
    mc, res = run_cfg(g, timing_phases=(1 << PH_DEDUP) | (1 << PH_OTHER), **SPLIT_KW)
    check_levels(g, res)
    cp, per_chunk = chunk_parents(g), 2 if maxsucc(g) > 256 else 1
    for ls in res.levels[1:]:
        chunks = -(-ls.expanded // cp)
        assert ls.kernel_launches[PH_OTHER] == chunks, ls
        assert ls.kernel_launches[PH_DEDUP] == per_chunk * chunks, ls
    mc.close()


# ---- (d) host-driven fused levels and the device loop -------------------------------------------
@pytest.mark.parametrize("name,device_levels", [("bf_n4_v1_e1_r3", 1), ("bf_n5_v1_e1_r3", 1), ("bf_n4_v1_e1_r3", 2),
                                                ("bf_n4_v1_e1_r3", 5)])
def test_fused_levels_match_golden(name, device_levels, monkeypatch):
    """No chunk split (the default split size is far above these levels): the fused expansion and the
    wave-per-parent k_commit at 288 / 301 slots, a level per host round trip (1) or in device-driven
    batches of 2 and 5 levels (odd and even frontier swaps, a batch boundary every few levels)."""
    monkeypatch.delenv("RMC_SPLIT_MIN", raising=False)
    g = LEVELS_BF[name]
    mc, res = run_cfg(g, device_levels=device_levels)
    check_levels(g, res)
    mc.close()


# ---- (e) self-loops per level --------------------------------------------------------------------
SELF_LOOP_CASES = ["bf_n4_v1_e1_r3", "bf_n3_v1_e1_r3"]


@functools.lru_cache(maxsize=None)
def oracle_self_loops(name):
    """Per expanded level, the oracle's successors identical to their parent (as test_gpu.py's
    _oracle_self_loops, with BecomeFollower in Next)."""
    g = LEVELS_BF[name]
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"], become_follower=True)
    ref = R.bfs(cfg, keep_states=True)
    want = [0] * max(ref.state_levels)
    for st, lv in zip(ref.states, ref.state_levels):
        want[lv - 1] += sum(1 for _, t in R.successors(cfg, st) if t == st)
    return want


@pytest.mark.parametrize("mode", ["device_loop", "host_fused", "split", "virtual2", "virtual2_split", "rccl1_split"])
@pytest.mark.parametrize("name", SELF_LOOP_CASES)
def test_self_loops_per_level_match_oracle(name, mode, monkeypatch):
    """rmc_level_stats.self_loops of the BecomeFollower kernels: counted by the fused expansion (device
    loop, host-driven levels, sharded rounds below the split size) or set apart by a split chunk's / split
    round's expansion and counted by its winner count -- equal, level by level, the oracle's successors
    identical to their parent (oracle/raft_ref.py, exact state equality)."""
    g = LEVELS_BF[name]
    want = oracle_self_loops(name)
    assert sum(want) > 0
    if mode.endswith("split"):
        monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    else:
        monkeypatch.delenv("RMC_SPLIT_MIN", raising=False)
    base = mode[:-len("_split")] if mode.endswith("_split") else mode
    kw = sharded_kw(base, monkeypatch) if base in ("virtual2", "rccl1") else {}
    if base in ("host_fused", "split"):
        kw["device_levels"] = 1
    mc, res = run_cfg(g, **kw)
    check_levels(g, res)
    got = [ls.self_loops for ls in res.levels[1:]]
    assert got == want[:len(got)] and sum(got) == sum(want), (got, want)
    mc.close()


# ---- (f) checkpoint / resume ---------------------------------------------------------------------
CKPT_MODES = {
    "single": dict(),
    "single_split": dict(device_levels=1, chunk_successors=CHUNK),
    "virtual2_split": dict(virtual_shards=2, chunk_successors=3000, shard_min_states=1),
}


@pytest.mark.parametrize("mode", sorted(CKPT_MODES))
def test_checkpoint_resume_matches_golden(mode, tmp_path, monkeypatch):
    """Stopped after 12 of 27 levels (near the widest), checkpointed, then finished twice: in the same
    checker and in a fresh one resumed from the file.  Both end with the golden totals and the golden
    sizes and successor counts of the remaining levels -- on one GPU, on one GPU with every chunk split,
    and on two virtual shards with every round split."""
    if mode.endswith("split"):
        monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    else:
        monkeypatch.delenv("RMC_SPLIT_MIN", raising=False)
    g = LEVELS_BF["bf_n4_v1_e1_r3"]
    path = str(tmp_path / "run.ckpt")
    a = raftmc.ModelChecker(model_config(g, **CKPT_MODES[mode]))
    a.init()
    k = 0
    while k < 12 and a.step().status == "ok":
        k += 1
    assert k == 12, "the configuration must run past the checkpoint level"
    a.checkpoint(path)
    done = len(a.levels)
    assert done == 13
    res_a = a.run()
    check_levels(g, res_a)
    b = raftmc.ModelChecker(model_config(g, **CKPT_MODES[mode]))
    b.resume(path)
    res_b = b.run()
    assert (res_b.status, res_b.distinct, res_b.generated, res_b.depth, res_b.queue) == \
           ("done", g["distinct"], g["generated"], g["depth"], 0)
    assert [ls.new_states for ls in res_b.levels if ls.new_states] == g["levels"][done:]
    assert [ls.generated for ls in res_b.levels] == g["gen_per_level"][done - 1:]
    a.close()
    b.close()


def test_resume_rejects_another_spec_variant(tmp_path):
    """The header's spec_variant: a BecomeFollower checkpoint is no checkpoint of Raft.tla as shipped at the
    same servers, values, MaxElection and MaxRestart."""
    g = LEVELS_BF["bf_n4_v1_e1_r3"]
    path = str(tmp_path / "run.ckpt")
    with raftmc.ModelChecker(model_config(g)) as a:
        a.init()
        a.step()
        a.checkpoint(path)
    shipped = dict(g, become_follower=False)
    assert spec_of(shipped) == raftmc.SPEC_RAFT
    with raftmc.ModelChecker(model_config(shipped)) as b:
        with pytest.raises(raftmc.RmcError, match="not a checkpoint of this configuration"):
            b.resume(path)
