"""One rank of a two-process sharded run with action coverage on, over the host-staged transport (test
helper beside hostx_worker.py).

usage: python coverage_worker.py SPEC_JSON -- SPEC = {"rank", "world", "port", "cfg": ModelConfig keywords,
"out": result path}.  The ranks meet in a torch.distributed gloo group on 127.0.0.1, install
raftmc.HostTransport and run the configuration with world_size = W on device 0; each writes the run's
counters and its own coverage() -- the global totals on every rank."""
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
            mc.set_coverage()
            res = mc.run()
            out.update(status=res.status, generated=res.generated, distinct=res.distinct,
                       coverage={k: list(v) for k, v in mc.coverage().items()})
        finally:
            mc.close()
    except raftmc.RmcError as e:
        out["error"] = str(e)
    with open(spec["out"], "w") as f:
        json.dump(out, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
