"""One rank of a two-process sharded run with continuation on, over the host-staged transport (test helper
beside coverage_worker.py).

usage: python continue_worker.py SPEC_JSON -- SPEC = {"rank", "world", "port", "cfg": ModelConfig keywords,
"out": result path}.  The ranks meet in a torch.distributed gloo group on 127.0.0.1, install
raftmc.HostTransport and run the configuration with world_size = W on device 0; each writes the run's
counters and its own violations() and violation_levels() -- the global totals on every rank -- and the keys
of every first violating behaviour (violation_trace walks the distributed trace: both ranks call it)."""
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tla-raft_amd"))

import torch.distributed as dist  # noqa: E402

import raftmc  # noqa: E402


def main():
    spec = json.loads(sys.argv[1])
    r, W = spec["rank"], spec["world"]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{spec['port']}", rank=r, world_size=W,
                            timeout=datetime.timedelta(seconds=spec.get("timeout", 120)))
    raftmc.HostTransport().install()
    out = {"rank": r}
    try:
        mc = raftmc.ModelChecker(raftmc.ModelConfig(rank=r, world_size=W, device=0, **spec["cfg"]))
        try:
            mc.set_continue()
            res = mc.run()
            viol = mc.violations()
            out.update(status=res.status, generated=res.generated, distinct=res.distinct, depth=res.depth,
                       violations={k: list(v) for k, v in viol.items()},
                       levels={k: mc.violation_levels(k) for k in viol},
                       paths={k: [list(key) for key, _ in mc.violation_trace(k)[1:]] for k, v in viol.items() if v[0]})
        finally:
            mc.close()
    except raftmc.RmcError as e:
        out["error"] = str(e)
    with open(spec["out"], "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
