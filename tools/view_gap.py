"""Does the cfg's VIEW lose a class?  The VIEW (Raft.tla:38) leaves out four variables that guard actions, so a
VIEW run keeps the first-found member of each class and never expands the others.  Per configuration this tool

1. exhausts the state space under the VIEW and on the whole state (ModelConfig(view=False));
2. streams the whole-state run's states (set_graph(states=True, on_states=...), in chunks);
3. fingerprints each chunk with a second checker that applies the VIEW (fingerprints_array);
4. counts the distinct VIEW fingerprints (ClassCounter).

Every state a VIEW run keeps is reachable, so the whole-state run meets every class the VIEW run found: equal
counts mean the VIEW run missed no class, a larger count is the number of classes the VIEW hid.  Streaming
copies every state to the host in the unpacked layout (kilobytes a state), so it may be given a time budget:
past it the sink ends the run and the report says how many states had been streamed and counted by then.
Raft.cfg itself is too large to stream: --raftcfg runs it on the whole state alone and records how far it got.
The report file is rewritten after every configuration.

usage: python tools/view_gap.py [--out profiles/view_gap.txt] [--only c2,n3v2e2,n3v1e3] [--raftcfg] [--budget SECONDS]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))

CONFIGS = {
    "c2": ("configs[1] (n=3, V=1, E=2, R=3)", dict(n_servers=3, n_vals=1, max_election=2, max_restart=3)),
    # (graph mode keeps the full seen-set slots: compact_log2 raised as tools/graph_rate.py does)
    "n3v2e2": ("n=3, V=2, E=2, R=3, compact_log2=30", dict(n_servers=3, n_vals=2, max_election=2, max_restart=3,
                                                          compact_log2=30)),
    "n3v1e3": ("n=3, V=1, E=3, R=3, compact_log2=31", dict(n_servers=3, n_vals=1, max_election=3, max_restart=3,
                                                          compact_log2=31)),
}
RAFT_CFG = dict(n_servers=3, n_vals=2, max_election=3, max_restart=3)


class ClassCounter:
    """Distinct 128-bit fingerprints among those added, chunk by chunk ((n, 2) uint64 arrays)."""

    def __init__(self):
        self.parts = []
        self.total = 0

    def add(self, fps):
        fps = np.asarray(fps, dtype=np.uint64).reshape(-1, 2)
        # a chunk's own repeats go at once: what is kept is at most the number of classes per chunk
        self.parts.append(self._unique(fps))
        self.total += len(fps)
        if len(self.parts) >= 64:
            self.parts = [self._unique(np.concatenate(self.parts))]

    @staticmethod
    def _unique(fps):
        if len(fps) < 2:
            return fps.copy()
        order = np.lexsort((fps[:, 1], fps[:, 0]))
        s = fps[order]
        keep = np.ones(len(s), dtype=bool)
        keep[1:] = (s[1:, 0] != s[:-1, 0]) | (s[1:, 1] != s[:-1, 1])
        return s[keep]

    def count(self):
        if not self.parts:
            return 0
        self.parts = [self._unique(np.concatenate(self.parts))]
        return len(self.parts[0])


def view_gap(kw, raftmc=None, budget=None):
    """The measurement for one configuration (ModelConfig keywords): a dict with the VIEW run's and the
    whole-state run's counters, `view_classes` among the whole-state run's states, and the times.  With a
    budget (seconds) the streaming pass may end early: `streamed` < the run's distinct states, `stopped` set."""
    if raftmc is None:
        import raftmc
    out = {}
    with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as view:
        t0 = time.perf_counter()
        rv = view.run()
        out["view_seconds"] = time.perf_counter() - t0
        assert rv.status == "done", rv.status
        out["view"] = (rv.distinct, rv.generated, rv.depth)
    # (that checker is closed: its seen set and rings are freed.  The fingerprint hook needs no search, so the
    # checker that applies the VIEW below is a fresh one, which has allocated no level buffers)
    with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as view:
        counter = ClassCounter()
        streamed = [0]
        t_stream = [0.0]

        def on_states(gid0, a):
            assert gid0 == streamed[0]
            if budget is not None and time.perf_counter() - t_stream[0] > budget:
                return 1  # over the budget: the sink ends the run (RMC_E_SINK)
            counter.add(view.fingerprints_array(np.ascontiguousarray(a)))
            streamed[0] += len(a)
            return 0

        with raftmc.ModelChecker(raftmc.ModelConfig(view=False, **kw)) as full:
            t0 = time.perf_counter()
            rf = full.run()
            out["full_seconds"] = time.perf_counter() - t0
            assert rf.status == "done", rf.status
            out["full"] = (rf.distinct, rf.generated, rf.depth)
            full.reset()
            full.set_graph(states=True, on_states=on_states, on_edges=lambda s, k, d: 0)
            t_stream[0] = t0 = time.perf_counter()
            try:
                rg = full.run()
                assert (rg.distinct, rg.generated) == (rf.distinct, rf.generated) and streamed[0] == rf.distinct
            except raftmc.RmcError as e:
                out["stopped"] = str(e)
            out["stream_seconds"] = time.perf_counter() - t0
    out["streamed"] = streamed[0]
    out["view_classes"] = counter.count()
    return out


def verdict(r):
    if r.get("stopped"):
        return (f"not decided: {r['streamed']:,} of {r['full'][0]:,} states streamed when the pass stopped "
                f"({r['stopped']})")
    hid = r["view_classes"] - r["view"][0]
    assert hid >= 0, "the whole-state run reaches every state a VIEW run keeps"
    return "the VIEW run missed no class" if hid == 0 else f"the VIEW hid {hid:,} classes"


def main():
    import raftmc
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_gap.txt"))
    ap.add_argument("--only", default=",".join(CONFIGS))
    ap.add_argument("--raftcfg", action="store_true")
    ap.add_argument("--budget", type=float, default=None, help="seconds a configuration's streaming pass may take")
    a = ap.parse_args()

    def save(lines):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    lines = ["view gap: per configuration the state space exhausted under the VIEW and on the whole state (one cold run "
             "each), then the whole-state run again with its states streamed and fingerprinted under the VIEW"]
    for key in [k for k in a.only.split(",") if k]:
        name, kw = CONFIGS[key]
        lines.append("")
        try:
            r = view_gap(kw, raftmc, a.budget)
        except raftmc.RmcError as e:
            lines.append(f"{name}: stopped: {e}")
            print(lines[-1], flush=True)
            save(lines)
            continue
        lines.append(f"{name}:")
        lines.append("  VIEW        {:,} distinct / {:,} generated / depth {}   {:.3f} s ({:,.0f} states/s)".format(
            *r["view"], r["view_seconds"], r["view"][0] / r["view_seconds"]))
        lines.append("  whole state {:,} distinct / {:,} generated / depth {}   {:.3f} s ({:,.0f} states/s)".format(
            *r["full"], r["full_seconds"], r["full"][0] / r["full_seconds"]))
        lines.append(f"  view classes among the whole-state run's states: {r['view_classes']:,}: {verdict(r)} "
                     f"(streamed and counted in {r['stream_seconds']:.1f} s)")
        print("\n".join(lines[-4:]), flush=True)
        save(lines)
    if a.raftcfg:
        lines.append("")
        with raftmc.ModelChecker(raftmc.ModelConfig(view=False, **RAFT_CFG)) as mc:
            t0 = time.perf_counter()
            mc.init()
            stop = "finished"
            try:
                batch = mc.steps()
                while batch and batch[-1].status == "ok":
                    batch = mc.steps()
            except raftmc.RmcError as e:
                stop = f"stopped by: {e}"
            dt = time.perf_counter() - t0
            lv = [ls for ls in mc.levels if ls.new_states]
            lines.append(f"Raft.cfg on the whole state: {sum(ls.new_states for ls in lv):,} distinct states over "
                         f"{len(lv)} complete levels in {dt:.1f} s "
                         f"({sum(ls.new_states for ls in lv) / dt:,.0f} states/s); {stop}")
        print(lines[-1], flush=True)
    save(lines)


if __name__ == "__main__":
    main()
