"""Time ovs_pastry_broadcast_batch beside ovs_chord_broadcast_batch on the same ids.

  python tools/diag/pastry_bcast_bench.py [--log2n 20] [--nb 64] [--reps 5] [--out FILE]

Two contexts on one population: the rule's Pastry tables (defaults: bitsPerDigit 4, numberOfLeaves 16) and the
converged Chord ring.  nb broadcasts at once from the same initiators, ttl 100, device pointers, records written.
Each call returns when its last level is done, so its wall time is the batch time.  After a warm-up of each the
two calls alternate repetition by repetition; the figure is the median.

Requested bytes per edge of the Pastry call, from what the kernels ask for (not from counters): per reached node
its 24 B item (read twice: expansion, statistics) and its 64 B record, 4 B of every slot it scans (the slot's
node index; the lane-per-node form scans twice, which this count leaves out); per child 16 B of coordinates, the
24 B item and the 16 B record written.  The slots scanned are counted on the host from the records of broadcast
0: a node forwards from the row after the one its request came from, up to its last non-empty row.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def _shared_digits(a, b, bits):
    """Digits of `bits` bits two uint64 key heads share (64 where equal)."""
    import numpy as np
    x = a ^ b
    lead = np.zeros(len(x), dtype=np.int64)
    alive = np.ones(len(x), dtype=bool)
    for k in range(64):
        alive &= ((x >> np.uint64(63 - k)) & np.uint64(1)) == 0
        lead += alive
    return lead // bits


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--nb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from oversim_amd import BCAST_NODE_DTYPE, KbrEngine, Params, PastryParams, workload as W

    dev = torch.device("cuda:0")
    n, nb = 1 << a.log2n, a.nb
    ids_t, xy_t = W.device_population(n, 0xB0CA, dev)
    init = torch.from_numpy(np.random.default_rng(1).integers(0, n, nb).astype(np.int32)).to(dev)
    recs = torch.empty(nb * n * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    res = dict(n=n, nb=nb, reps=a.reps, edges=nb * (n - 1))
    with KbrEngine(0) as pe, KbrEngine(0) as ce:
        pe.set_params(Params.pastry())
        pe.pastry_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, PastryParams.default())
        ce.set_params(Params.chord())
        ce.chord_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)
        calls = dict(pastry=pe.pastry_broadcast_device, chord=ce.chord_broadcast_device)
        ts = dict(pastry=[], chord=[])
        st = {}
        for name, call in calls.items():                              # warm-up: scratch, code objects
            call(init.data_ptr(), nb, 100, 0, recs.data_ptr())
        for _ in range(a.reps):
            for name, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st[name] = call(init.data_ptr(), nb, 100, 0, recs.data_ptr())
                ts[name].append(time.perf_counter() - t0)
        # the records left in `recs` are the Chord call's (the last to run): take Pastry's once more for the count
        pe.pastry_broadcast_device(init.data_ptr(), nb, 100, 0, recs.data_ptr())
        r0 = recs[: n * 16].cpu().numpy().view(BCAST_NODE_DTYPE)
        rows = int(pe._L.ovs_pastry_num_rows(pe._h))
    for name in calls:
        assert all(s["actual"] == n and s["expired"] == 0 for s in st[name]), name
        med = statistics.median(ts[name])
        res[name] = dict(ms=[t * 1e3 for t in ts[name]], median_ms=med * 1e3, spread_ms=(max(ts[name]) - min(ts[name])) * 1e3,
                         levels=int(max(s["hop_count"]["max"] for s in st[name])),
                         mean_hops=float(np.mean([s["hop_count"]["mean"] for s in st[name]])),
                         edges_per_s=res["edges"] / med)
    # slots scanned in broadcast 0
    ids = ids_t.cpu().numpy().view(np.uint32).reshape(n, 5)
    head = (ids[:, 4].astype(np.uint64) << np.uint64(32)) | ids[:, 3].astype(np.uint64)
    nbr = np.maximum(_shared_digits(head, np.roll(head, 1), 4), _shared_digits(head, np.roll(head, -1), 4))
    nrows = np.minimum(nbr + 1, rows)                                 # rows up to the last non-empty one
    par = r0["parent"].astype(np.int64)
    kid = par != 0xFFFFFFFF
    first = np.zeros(n, dtype=np.int64)
    first[kid] = _shared_digits(head[kid], head[par[kid]], 4) + 1
    slots = int((np.maximum(nrows - first, 0) * 16).sum())
    per_edge = (n * (2 * 24 + 64) + 4 * slots + (n - 1) * (16 + 24 + 16)) / (n - 1)
    res["pastry"].update(table_rows=rows, slots_scanned_per_node=slots / n, requested_bytes_per_edge=per_edge,
                         requested_GBs=per_edge * res["pastry"]["edges_per_s"] / 1e9)
    res["pastry_over_chord"] = res["pastry"]["median_ms"] / res["chord"]["median_ms"]
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
