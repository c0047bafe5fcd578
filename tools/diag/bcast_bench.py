"""Time ovs_chord_broadcast_batch on a large converged ring and the emulation it replaces.

  python tools/diag/bcast_bench.py [--log2n 20] [--nb 64] [--reps 3] [--out FILE]

The broadcast: nb broadcasts at once, device pointers, records written (and once more with
statistics only).  The call returns when its last level is done, so its wall time is the batch time
(level launches, the per-level read-back of the queue length, the statistics reduction).
The emulation: before the broadcast call, the only way to get a hop count from an initiator to every
node was ovs_route_batch with n lookups per initiator, each for a node's own key -- O(n log n) line
reads per initiator instead of n - 1 tree edges.  Both run in this process on the same ring.
Model traffic of the broadcast: 64 B per edge read (the finger entry) + 16 B per record written.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--nb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from oversim_amd import KbrEngine, Params, ROUTE_OUT_DTYPE, workload as W

    dev = torch.device("cuda:0")
    n, nb = 1 << a.log2n, a.nb
    ids_t, xy_t = W.device_population(n, 0xB0CA, dev)
    init = torch.from_numpy(np.random.default_rng(1).integers(0, n, nb).astype(np.int32)).to(dev)
    init_h = init.cpu().tolist()
    recs = torch.empty(nb * n * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    res = dict(n=n, nb=nb, reps=a.reps, edges=nb * (n - 1))
    with KbrEngine(0) as eng:
        eng.set_params(Params.chord())
        eng.chord_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)

        def timed(nodes_ptr):
            eng.chord_broadcast_device(init.data_ptr(), nb, 100, 0, nodes_ptr)       # warm-up: scratch, code
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = eng.chord_broadcast_device(init.data_ptr(), nb, 100, 0, nodes_ptr)
                ts.append(time.perf_counter() - t0)
            return ts, st

        ts, st = timed(recs.data_ptr())
        ts0, _ = timed(None)
        assert all(s["actual"] == n and s["expired"] == 0 for s in st)
        best = min(ts)
        res.update(broadcast_ms=[t * 1e3 for t in ts], broadcast_stats_only_ms=[t * 1e3 for t in ts0],
                   edges_per_s=res["edges"] / best,
                   model_bytes=64 * res["edges"] + 16 * nb * n,
                   model_GBs=(64 * res["edges"] + 16 * nb * n) / best / 1e9,
                   levels=int(max(s["hop_count"]["max"] for s in st)),
                   mean_hops=float(np.mean([s["hop_count"]["mean"] for s in st])))

        # the emulation: n lookups of the nodes' own keys from each initiator
        out = torch.empty(n * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        src = torch.empty(n, dtype=torch.int32, device=dev)
        te = []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(nb):
                src.fill_(init_h[b])
                eng.lookup_device(ids_t.data_ptr(), src.data_ptr(), n, out.data_ptr(), 0)
            torch.cuda.synchronize()
            if rep:
                te.append(time.perf_counter() - t0)
        o = out.cpu().numpy().view(ROUTE_OUT_DTYPE)
        res.update(emulation_ms=[t * 1e3 for t in te], emulation_last_mean_hops=float(o["hops"].mean()),
                   emulation_lookups=nb * n, speedup=min(te) / best)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
