"""Time ovs_scribe_build and ovs_scribe_multicast_batch on a large converged network.

  python tools/diag/scribe_bench.py [--overlay chord|pastry|both] [--log2n 20] [--groups 1024] [--members 1024]
                                    [--reps 5] [--out FILE]

The build: groups x members memberships (device pointers), semi-recursive routing.  The baseline is
what the engine could do with the same pairs before: route every member to its group key with the
hops recorded (ovs_route_batch / ovs_pastry_route_batch with hop_seq) -- the raw material of the same
trees, without the deduplication, the child lists or the roots.  The build evaluates fewer findNodes (a
chain stops at the first node already in the tree) but synchronises once per level and sorts twice.
The multicast: one publish per group from a random node, delivery records written.
--overlay both holds a Chord and a Pastry context on the same ids and alternates them repetition by
repetition, after one warm-up of each; every figure is reported as all its wall times, their median and
their minimum, in ms.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--overlay", choices=("chord", "pastry", "both"), default="chord")
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--members", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from oversim_amd import (DEVICE_PTRS, KbrEngine, Params, PastryParams, ROUTE_OUT_DTYPE, SCRIBE_DELIVERY_DTYPE,
                             SCRIBE_MSG_DTYPE, workload as W)

    dev = torch.device("cuda:0")
    n, G, m = 1 << a.log2n, a.groups, a.groups * a.members
    ids_t, xy_t = W.device_population(n, 0x5C81, dev)
    rng = np.random.default_rng(2)
    gk = rng.integers(0, 1 << 32, (G, 5), dtype=np.uint64).astype(np.uint32)
    mg = np.repeat(np.arange(G, dtype=np.uint32), a.members)
    mn = rng.integers(0, n, m).astype(np.uint32)
    t_gk, t_mg, t_mn = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (gk, mg, mn))
    t_keys = torch.from_numpy(gk[mg].view(np.int32)).to(dev)
    pg = torch.arange(G, dtype=torch.int32, device=dev)
    ps = torch.from_numpy(rng.integers(0, n, G).astype(np.int32)).to(dev)
    pf = torch.zeros(G, dtype=torch.uint8, device=dev)
    po = torch.empty(G * SCRIBE_MSG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    pd = torch.empty(m * SCRIBE_DELIVERY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    overlays = ("chord", "pastry") if a.overlay == "both" else (a.overlay,)
    res = dict(n=n, groups=G, memberships=m, reps=a.reps, overlays=list(overlays))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def alternate(fns):
        """one warm-up of each, then reps rounds that run every overlay's call in turn"""
        for fn in fns.values():
            fn()
        ts = {o: [] for o in fns}
        for _ in range(a.reps):
            for o, fn in fns.items():
                ts[o].append(timed(fn))
        return ts

    engines = {}
    try:
        for o in overlays:
            eng = engines[o] = KbrEngine(0)
            if o == "chord":
                p = Params.chord().replace(routingType=1)
                eng.set_params(p)
                eng.chord_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)
            else:
                p = Params.pastry()
                eng.set_params(p)
                eng.pastry_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, PastryParams.default(routeMsgAcks=0))
        H = max(p.hopCountMax, 1)
        out = torch.empty(m * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        hop = torch.empty(m * H, dtype=torch.int32, device=dev)

        def route(o):
            eng = engines[o]
            if o == "chord":
                eng._chk(eng._L.ovs_route_batch(eng._h, C.c_void_p(t_keys.data_ptr()), C.c_void_p(t_mn.data_ptr()), m,
                                                C.c_void_p(out.data_ptr()), C.c_void_p(hop.data_ptr()), None, DEVICE_PTRS, None),
                         "ovs_route_batch")
            else:
                eng._chk(eng._L.ovs_pastry_route_batch(eng._h, C.c_void_p(t_keys.data_ptr()), C.c_void_p(t_mn.data_ptr()), m,
                                                       C.c_void_p(out.data_ptr()), C.c_void_p(hop.data_ptr()), DEVICE_PTRS, None),
                         "ovs_pastry_route_batch")

        def report(name, ts):
            for o, t in ts.items():
                res[f"{o}_{name}_ms"] = dict(all=[round(x, 3) for x in t], median=round(statistics.median(t), 3),
                                             min=round(min(t), 3))

        report("route_record_hops", alternate({o: (lambda o=o: route(o)) for o in overlays}))
        cap = {}
        for o in overlays:
            route(o)
            hops = out.cpu().numpy().view(ROUTE_OUT_DTYPE)["hops"]
            res[f"{o}_route_findnodes"] = int(hops.sum()) + m
            cap[o] = int(hops.sum()) + m + G
        report("build", alternate({o: (lambda o=o: engines[o].scribe_build_device(
            t_gk.data_ptr(), G, t_mg.data_ptr(), t_mn.data_ptr(), m, cap[o])) for o in overlays}))
        for o in overlays:
            nodes, edges, rooted = engines[o].scribe_count()
            res[f"{o}_forest"] = dict(tree_nodes=nodes, edges=edges, rooted_groups=rooted, max_depth=int(
                engines[o].scribe_export()["depth"].max()))
        cnt = {}

        def publish(o):
            cnt[o] = engines[o].scribe_multicast_device(pg.data_ptr(), ps.data_ptr(), pf.data_ptr(), G, 100, po.data_ptr(),
                                                        pd.data_ptr(), m)

        report("multicast", alternate({o: (lambda o=o: publish(o)) for o in overlays}))
        for o in overlays:
            res[f"{o}_deliveries"] = cnt[o]
            res[f"{o}_deliveries_per_s"] = cnt[o] / (res[f"{o}_multicast_ms"]["median"] * 1e-3)
            res[f"{o}_build_over_route"] = res[f"{o}_build_ms"]["median"] / res[f"{o}_route_record_hops_ms"]["median"]
    finally:
        for eng in engines.values():
            eng.close()
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
