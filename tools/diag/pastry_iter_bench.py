"""Time Pastry's iterative lookup kernel beside its semi-recursive route kernel on the same tables and batch.

  python tools/diag/pastry_iter_bench.py [--log2n 20] [--lookups 10000000] [--reps 5] [--out FILE]

Converged Pastry tables of 2^log2n nodes at the defaults (bitsPerDigit 4, numberOfLeaves 16); `lookups` random keys
from random sources on device pointers.  Two contexts on the same ids: one with routingType iterative
(LookupCalls with num_siblings 1, ovs_pastry_lookup_batch), one semi-recursive (recNumRedundantNodes 3,
ovs_pastry_route_batch).  After one warm-up of each the two are alternated -- iterative, semi-recursive, iterative
... -- un-profiled, each timed from launch to the stream's synchronisation.  Writes medians, spread (max - min),
lookups/s, FindNodeCalls/s, mean hops and the bytes a responder visit asks for to --out as text.  Bytes per visit
are what the layout makes a visit request, not a counter: 64 B record + 24 B x numberOfLeaves leaf row + one 24 B
table slot; the source's own findNode asks for the same and, for the first target of a numberOfLeaves-node
answer under useRegularNextHop, nothing more.
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
    ap.add_argument("--lookups", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from oversim_amd import KbrEngine, LOOKUP_OUT_DTYPE, Params, PastryParams, ROUTE_OUT_DTYPE, workload as W

    dev = torch.device("cuda:0")
    n, m = 1 << a.log2n, a.lookups
    ids_t, xy_t = W.device_population(n, 0xB300, dev)
    keys, src = W.device_lookups(n, m, 0xB301, dev)
    out = torch.empty(m * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    lout = torch.empty(m * LOOKUP_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    sib = torch.empty(m, dtype=torch.int32, device=dev)
    rpcs = torch.empty(m, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def med(ts):
        return f"median {statistics.median(ts):10.3f}  spread {max(ts) - min(ts):8.3f}  all {' '.join(f'{t:.3f}' for t in ts)}"

    lines = [f"pastry_iter_bench: n = 2^{a.log2n} nodes, {m} lookups, device pointers, {a.reps} alternated repetitions, ms"]
    with KbrEngine(0) as ei, KbrEngine(0) as er:
        pp = PastryParams.default(routeMsgAcks=0)
        ei.set_params(Params.pastry().replace(routingType=0))
        ei.pastry_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, pp)
        er.set_params(Params.pastry())
        er.pastry_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, pp)

        def iterative():
            ei.pastry_lookup_call_device(keys.data_ptr(), src.data_ptr(), m, 1, lout.data_ptr(), sib.data_ptr(),
                                         rpcs_ptr=rpcs.data_ptr())

        def semirec():
            er.pastry_lookup_device(keys.data_ptr(), src.data_ptr(), m, out.data_ptr())

        timed(iterative)
        o = lout.cpu().numpy().view(LOOKUP_OUT_DTYPE)
        oki, hi, ci = int((o["status"] == 0).sum()), float(o["hops"].mean()), float(rpcs.cpu().numpy().mean())
        timed(semirec)
        o = out.cpu().numpy().view(ROUTE_OUT_DTYPE)
        okr, hr = int((o["status"] == 0).sum()), float(o["hops"].mean())
        ti, tr = [], []
        for _ in range(a.reps):
            ti.append(timed(iterative))
            tr.append(timed(semirec))
        mi, mr = statistics.median(ti), statistics.median(tr)
        bp = 64 + 24 * pp.numberOfLeaves + 24
        # a responder visit: every FindNodeCall's responder plus the source's own findNode; a route: every node
        # that holds the message, the source included
        vi, vr = ci + 1, hr + 1
        lines += [f"  iterative LookupCall, num_siblings 1 (rows {ei._L.ovs_pastry_num_rows(ei._h)})  {med(ti)}",
                  f"    valid {oki} of {m}, mean hops {hi:.3f}, {m / mi / 1e3:.1f} M lookups/s, {ci * m / mi / 1e3:.1f} M FindNodeCalls/s,"
                  f" {bp} B requested per RPC (+ the source's {bp} B a lookup)",
                  f"  semi-recursive route  {med(tr)}",
                  f"    delivered {okr} of {m}, mean hops {hr:.3f}, {hr * m / mr / 1e3:.1f} M hops/s",
                  f"  iterative / semi-recursive: time {mi / mr:.3f}, time per findNode visit {(mi / vi) / (mr / vr):.3f}"
                  f" ({vi:.3f} and {vr:.3f} visits a lookup)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
