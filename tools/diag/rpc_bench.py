"""Time ovs_rpc_batch against the one-way ovs_route_batch it builds on, at config C's shape.

  python tools/diag/rpc_bench.py [--log2n 20] [--rpcs 10000000] [--reps 5] [--out FILE]

A converged Chord ring of 2^log2n nodes, `rpcs` (key, source) pairs with node-ID keys, device pointers.
For routingType 0 (iterative) and 2 (full-recursive) the two calls are alternated -- route, rpc, route,
rpc ... -- after one warm-up of each, un-profiled, each timed from launch to the stream's
synchronisation.  The RPC call is the route plus the finish pass (one 16 B record read, two 16 B
coordinate gathers, one 32 B record written per RPC); under routingType 2 it is two routes plus the
finish and fold passes.  Writes medians, spread (max - min) and the overhead to --out as text.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rpcs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from oversim_amd import KbrEngine, Params, ROUTE_OUT_DTYPE, RPC_OUT_DTYPE, workload as W

    dev = torch.device("cuda:0")
    n, m = 1 << a.log2n, a.rpcs
    ids_t, xy_t = W.device_population(n, 0xC0C0, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    src = torch.randint(0, n, (m,), dtype=torch.int32, device=dev, generator=g)
    keys = ids_t[torch.randint(0, n, (m,), device=dev, generator=g)].contiguous()        # lookupNodeIds = true
    rout = torch.empty(m * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    pout = torch.empty(m * RPC_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    lines = [f"rpc_bench: n = 2^{a.log2n} nodes, {m} RPCs, device pointers, {a.reps} alternated repetitions, ms"]
    with KbrEngine(0) as eng:
        for rt in (0, 2):
            eng.set_params(Params.chord().replace(routingType=rt))
            eng.chord_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)

            def route():
                eng.lookup_device(keys.data_ptr(), src.data_ptr(), m, rout.data_ptr())

            def rpc():
                eng.rpc_device(keys.data_ptr(), src.data_ptr(), m, pout.data_ptr())

            def timed(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            timed(route), timed(rpc)                     # warm-up: code objects, cached buffers
            tr, tp = [], []
            for _ in range(a.reps):
                tr.append(timed(route))
                tp.append(timed(rpc))
            o = pout.cpu().numpy().view(RPC_OUT_DTYPE)
            mr, mp = statistics.median(tr), statistics.median(tp)
            lines += [f"routingType {rt}:",
                      f"  ovs_route_batch  median {mr:9.3f}  spread {max(tr) - min(tr):7.3f}  all {' '.join(f'{t:.3f}' for t in tr)}",
                      f"  ovs_rpc_batch    median {mp:9.3f}  spread {max(tp) - min(tp):7.3f}  all {' '.join(f'{t:.3f}' for t in tp)}",
                      f"  rpc / route = {mp / mr:.4f}  (rpc - {2 if rt == 2 else 1} x route = {mp - (2 if rt == 2 else 1) * mr:+.3f} ms)",
                      f"  answered {(o['outcome'] == 0).sum()} of {m}, mean RPC hop count {o['hop_count'][o['outcome'] == 0].mean():.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
