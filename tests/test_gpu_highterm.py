"""MaxElection 4..7, MaxRestart up to 7 (and 0), MaxElection 0 through the kernels.

rmc_config takes max_election 0..7 and max_restart 0..15, and the packed codec (3-bit currentTerm,
electionCount and log-entry term, 4-bit restartCount), the message info word (4-bit term fields) and the
16-bit message ids are sized for that, but every other fixture stays at MaxElection <= 3, MaxRestart <= 3.
These run the high corner (tests/golden/make_golden_highterm.py, from oracle/ alone) through
rmc_successors, the fingerprint, the invariants, the frontier codec, the BFS in its execution modes and the
message-universe limit.  Every comparison is exact."""
import gzip
import json
import os
import time

import numpy as np
import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN
from test_gpu import (check_deep_fingerprint_classes, check_deep_invariants, check_deep_successors, check_levels,
                      checker, mode_kwargs, run_cfg)
from test_gpu_deep import check_sampled_levels

pytestmark = pytest.mark.gpu

with gzip.open(os.path.join(GOLDEN, "successors_highterm.json.gz"), "rt") as _f:
    HIGH = json.load(_f)
with open(os.path.join(GOLDEN, "levels_highterm.json")) as _f:
    LEVELS = json.load(_f)
EXHAUSTED = sorted(k for k, g in LEVELS.items() if g["exhausted"])
PREFIXES = sorted(k for k, g in LEVELS.items() if not g["exhausted"])


def high_checker(g):
    kw = dict(spec_variant=raftmc.SPEC_BECOME_FOLLOWER) if g["become_follower"] else {}
    return checker(g["n"], g["V"], g["E"], g["R"], **kw)


# ---- single states ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HIGH))
def test_highterm_successors_match_oracle(name):
    """Successor lists, keys and states bit for bit in TLC order, of states with terms, electionCount and
    log-entry terms up to 7, restartCount up to 5 and messages of term up to 7."""
    check_deep_successors(HIGH[name], high_checker(HIGH[name]))


@pytest.mark.parametrize("name", sorted(HIGH))
def test_highterm_fingerprint_classes_match_oracle(name):
    check_deep_fingerprint_classes(HIGH[name], high_checker(HIGH[name]))


@pytest.mark.parametrize("name", sorted(HIGH))
def test_highterm_invariants_match_oracle(name):
    check_deep_invariants(HIGH[name], high_checker(HIGH[name]))


@pytest.mark.parametrize("name", sorted(HIGH))
def test_fingerprint_ignores_everything_outside_the_view(name):
    """rmc_fingerprint of every fixture state is that of its copies with electionCount 0..7 x restartCount
    0..15 (the whole range of both fields, 128 copies) and pendingResponse / valSent changed: the variables
    outside the VIEW (Raft.tla:29,34,38).  A counter bit leaking into the fingerprint splits classes only
    where the counters pass 3."""
    g = HIGH[name]
    n, V = g["n"], g["V"]
    mc = high_checker(g)
    stride = raftmc.unpacked_len(n, V, g["msg_cap"])
    pend = 5 * n + n * (V + 1) * 2 + 2 * n * n  # include/rmc.h: the unpacked layout
    ec, rc, vs = pend + n * n, pend + n * n + 1, pend + n * n + 2
    rows, owner, base = [], [], []
    for k, it in enumerate(g["items"]):
        u = raftmc.state_to_unpacked(it["state"], n, V)
        assert (u[ec], u[rc]) == (it["state"]["electionCount"], it["state"]["restartCount"])
        u = np.asarray(u + [0] * (stride - len(u)), dtype=np.int32)
        base.append(u)
        for e in range(8):
            for r in range(16):
                c = u.copy()
                c[ec], c[rc] = e, r
                if (e + r) % 2:  # every other copy: pendingResponse complemented, valSent toggled
                    c[pend:pend + n * n] = 1 - c[pend:pend + n * n]
                    c[vs:vs + V] = np.where(c[vs:vs + V] == -1, 0, -1)
                rows.append(c)
                owner.append(k)
    fps = mc.fingerprints_unpacked(np.ascontiguousarray(np.stack(base)), stride, len(base))
    assert fps == [mc.fingerprint(it["state"]) for it in g["items"]]
    got = mc.fingerprints_unpacked(np.ascontiguousarray(np.stack(rows)), stride, len(rows))
    apart = sum(1 for k, f in enumerate(got) if f != fps[owner[k]])
    assert apart == 0, f"{apart} of {len(rows)} non-VIEW copies fingerprint apart from their states"
    assert len(set(fps)) == len(fps)  # (the kept states are distinct classes: the check is not vacuous)


# ---- BFS ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "host_levels", "virtual2"])
@pytest.mark.parametrize("name", EXHAUSTED)
def test_exhausted_levels_match_golden(name, mode, monkeypatch):
    """MaxElection 4 and 5 at 2 servers, MaxRestart 0 (Restart never enabled) and MaxElection 0 (no message,
    no successor: Init alone) to the end: levels, generated counts, depth, verdict."""
    g = LEVELS[name]
    mc, res = run_cfg(g, **mode_kwargs(mode, monkeypatch))
    check_levels(g, res)
    if g["E"] == 0:
        assert (res.distinct, res.generated, res.depth) == (1, 1, 1)
        assert res.status == ("deadlock" if g["check_deadlock"] else "done")
        init = R.state_to_json(R.init_state(R.Config(n=g["n"], V=g["V"], max_election=0, max_restart=g["R"])))
        assert mc.trace() == ([(None, init)] if g["check_deadlock"] else [])
        assert mc.successors(init) == []
    mc.close()


@pytest.mark.parametrize("mode", ["default", "host_levels", "split", "virtual2", "rccl1"])
@pytest.mark.parametrize("name", PREFIXES)
def test_prefix_levels_match_golden(name, mode, monkeypatch):
    """The largest MaxElection of every compiled (servers, values) pair, exactly as deep as the C oracle has
    complete levels (level 8 on holds states of term and electionCount 7): distinct and generated per
    level.  `default` takes the levels in device-driven batches (rmc_steps), the others one rmc_step each."""
    g = LEVELS[name]
    L = len(g["levels"])
    with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"],
                                                max_restart=g["R"], **mode_kwargs(mode, monkeypatch))) as mc:
        mc.init()
        while len(mc.levels) < L:
            got = mc.steps(cap=L - len(mc.levels)) if mode == "default" else [mc.step()]
            assert all(ls.status == "ok" for ls in got)
        assert len(mc.levels) == L
        assert [ls.new_states for ls in mc.levels] == g["levels"]
        assert [ls.generated for ls in mc.levels[1:]] == g["gen_per_level"]
        assert mc.levels[-1].total_distinct == sum(g["levels"])
        assert mc.levels[-1].total_generated == 1 + sum(g["gen_per_level"])


def test_e4_compact_seen_set_and_fixed_ring():
    """n2_v1_e4_r3 on the large-run storage (8-B seen-set slots after 2^10, a frontier ring at ~60 % of the
    peak): the frontier codec's round trip of records with terms up to 4 through the ring."""
    g = LEVELS["n2_v1_e4_r3"]
    probe, res0 = run_cfg(g, chunk_successors=6000, device_levels=1)
    peak = res0.frontier_peak_bytes
    probe.close()
    slots = 1 << max(12, (int(g["distinct"] / 0.6)).bit_length())
    ring = int(0.6 * peak) + 4 * 6000 * 36 + 4096
    mc, res = run_cfg(g, chunk_successors=6000, compact_log2=10, seen_log2=8, seen_mem_bytes=8 * slots,
                      frontier_mem_bytes=ring)
    check_levels(g, res)
    assert res.seen_slot_bytes == 8 and res.seen_slots == slots
    mc.close()


def test_e4_checkpoint_resume_at_the_middle_level(tmp_path):
    g = LEVELS["n2_v1_e4_r3"]
    cfg = raftmc.ModelConfig(n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"])
    path = str(tmp_path / "run.ckpt")
    with raftmc.ModelChecker(cfg) as a:
        a.init()
        for _ in range(g["depth"] // 2):
            assert a.step().status == "ok"
        a.checkpoint(path)
        done = len(a.levels)
        res_a = a.run()
        check_levels(g, res_a)
    with raftmc.ModelChecker(cfg) as b:
        b.resume(path)
        res_b = b.run()
        assert (res_b.status, res_b.generated, res_b.distinct, res_b.depth, res_b.queue) == \
               ("done", g["generated"], g["distinct"], g["depth"], 0)
        assert [ls.new_states for ls in res_b.levels if ls.new_states] == g["levels"][done:]
        assert [ls.generated for ls in res_b.levels] == g["gen_per_level"][done - 1:]


# ---- closure at depth, without a golden ------------------------------------------------------------------
def _closure(n, V, E, Rr):
    """Exhaust (n, V, E, Rr) and apply tests/test_gpu_deep.py's checks (i)-(vi) to 2,000 seeded samples drawn
    evenly from the deeper half of the levels, with the C oracle as the checker."""
    with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=n, n_vals=V, max_election=E, max_restart=Rr)) as mc:
        t0 = time.time()
        res = mc.run()
        dt = time.time() - t0
        assert res.status == "done" and res.queue == 0
        lo = res.depth // 2 + 1
        picks, n_succ, n_images = check_sampled_levels(mc, res, n, V, E, Rr, lo, res.depth, 2000, 20261021)
    print(f"closure n{n}_v{V}_e{E}_r{Rr}: {res.distinct} distinct states, {res.generated} generated, depth {res.depth}, "
          f"exhausted in {dt:.1f} s; {picks} states over levels {lo}-{res.depth}, {n_succ} oracle successors in the "
          f"seen set, {n_images} images with their state's fingerprint")
    assert picks == 2000
    return res


def test_closure_at_depth_n2_v1_e7_r7():
    """No oracle exhausts this one: 336,584,785 distinct states at depth 68 (601,201,862 generated), 6.6 s of
    GPU time on an MI355X -- the whole of 2 servers at the top of both counters' useful range."""
    res = _closure(2, 1, 7, 7)
    # (this checker's own totals, pinned so that a change of them is seen; parity is what _closure checks)
    assert (res.distinct, res.generated, res.depth) == (336584785, 601201862, 68)


# ---- the message-universe limit ---------------------------------------------------------------------------
def test_create_refuses_oversized_universes_and_leaves_nothing_behind():
    """(3,2,E7), (3,3,E5), (4,2,E6), (5,2,E5) have 0xFFFF message records or more: RMC_E_ARG naming the pair's
    largest MaxElection, before the device is touched -- then a run in the same process, and the one-lower
    neighbours create."""
    for (n, V, E), lim in {(3, 2, 7): 6, (3, 3, 5): 4, (4, 2, 6): 5, (5, 2, 5): 4}.items():
        with pytest.raises(raftmc.RmcError, match=rf"RMC_E_ARG: .*max_election is at most {lim} for this pair"):
            raftmc.ModelChecker(raftmc.ModelConfig(n_servers=n, n_vals=V, max_election=E, max_restart=3))
    with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=3, n_vals=1, max_election=1, max_restart=3)) as mc:
        res = mc.run()
        assert (res.status, res.distinct) == ("done", 545)
    for n, V, E in [(3, 2, 6), (3, 3, 4), (4, 2, 5), (5, 2, 4)]:
        with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=n, n_vals=V, max_election=E, max_restart=3)) as mc:
            assert mc.init().new_states == 1
