"""Time Broose's snapshot build and route kernel (K4) beside Koorde's K3 at the same shape.

  python tools/diag/broose_bench.py [--log2n 20] [--lookups 10000000] [--reps 5] [--out FILE]

An ideal Broose snapshot of 2^log2n nodes at the defaults (bucketSize = rBucketSize = 8, shiftingBits 2) and
a converged Koorde ring of the same ids with shiftingBits 2; `lookups` random keys from random sources, device
pointers, direction flags alternating.  After one warm-up of each the two routes are alternated -- Broose,
Koorde, Broose, Koorde ... -- un-profiled, each timed from launch to the stream's synchronisation; the build is
timed `reps` times the same way.  FindNodeCalls come from the calls' rpcs output (+ 1 local findNode a lookup).
Writes medians, spread (max - min), hops/s and the time per findNode to --out as text.
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
    from oversim_amd import BrooseParams, KbrEngine, Params, ROUTE_OUT_DTYPE, workload as W

    dev = torch.device("cuda:0")
    n, m = 1 << a.log2n, a.lookups
    ids_t, xy_t = W.device_population(n, 0xB200, dev)
    keys, src = W.device_lookups(n, m, 0xB201, dev)
    right = (torch.arange(m, device=dev) & 1).to(torch.uint8)
    out = torch.empty(m * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
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

    lines = [f"broose_bench: n = 2^{a.log2n} nodes, {m} lookups, device pointers, {a.reps} alternated repetitions, ms"]
    with KbrEngine(0) as eb, KbrEngine(0) as ek:
        eb.set_params(Params.broose())
        bp = BrooseParams.default()
        load = lambda: eb.broose_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, bp)
        timed(load)
        tb = [timed(load) for _ in range(a.reps)]
        ek.set_params(Params.koorde().replace(shiftingBits=2))
        ek.koorde_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)

        def broose():
            eb.broose_lookup_device(keys.data_ptr(), src.data_ptr(), right.data_ptr(), m, out.data_ptr(), rpcs_ptr=rpcs.data_ptr())

        def koorde():
            ek.lookup_device(keys.data_ptr(), src.data_ptr(), m, out.data_ptr(), rpcs_ptr=rpcs.data_ptr())

        def census():
            o = out.cpu().numpy().view(ROUTE_OUT_DTYPE)
            return int((o["status"] == 0).sum()), float(o["hops"].mean()), int(rpcs.sum().item()) + m

        timed(broose)
        okb, hb, fb = census()
        timed(koorde)
        okk, hk, fk = census()
        rb, rk = [], []
        for _ in range(a.reps):
            rb.append(timed(broose))
            rk.append(timed(koorde))
        mb, mk = statistics.median(rb), statistics.median(rk)
        lines += [f"  broose snapshot build (upload, rows, records)  {med(tb)}",
                  f"  broose route K4   {med(rb)}",
                  f"    delivered {okb} of {m}, mean hops {hb:.3f}, findNodes per lookup {fb / m:.3f}, "
                  f"{hb * m / mb / 1e3:.1f} M hops/s, {mb * 1e6 / fb:.2f} ns per findNode",
                  f"  koorde route K3 (shiftingBits 2)  {med(rk)}",
                  f"    delivered {okk} of {m}, mean hops {hk:.3f}, findNodes per lookup {fk / m:.3f}, "
                  f"{hk * m / mk / 1e3:.1f} M hops/s, {mk * 1e6 / fk:.2f} ns per findNode",
                  f"  broose / koorde: time {mb / mk:.3f}, time per findNode {(mb / fb) / (mk / fk):.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
