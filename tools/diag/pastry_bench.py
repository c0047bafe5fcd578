"""Time Pastry's table build and semi-recursive route kernel beside Chord's semi-recursive route on the same ids
and batch.

  python tools/diag/pastry_bench.py [--log2n 20] [--lookups 10000000] [--reps 5] [--out FILE]

Converged Pastry tables of 2^log2n nodes at the defaults (bitsPerDigit 4, numberOfLeaves 16, recNumRedundantNodes 3)
and a converged Chord ring of the same ids with routingType semi-recursive; `lookups` random keys from random
sources on device pointers.  After one warm-up of each the two routes are alternated -- Pastry, Chord, Pastry,
Chord ... -- un-profiled, each timed from launch to the stream's synchronisation; the build is timed `reps`
times the same way.  Writes medians, spread (max - min), hops/s and the bytes a hop asks for to --out as text.
Bytes per hop are what the layout makes a hop request, not a counter: Pastry 64 B record + 24 B x numberOfLeaves leaf
row + one 24 B table slot; Chord 64 B per hop + 104 B per lookup.
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
    from oversim_amd import KbrEngine, Params, PastryParams, ROUTE_OUT_DTYPE, workload as W

    dev = torch.device("cuda:0")
    n, m = 1 << a.log2n, a.lookups
    ids_t, xy_t = W.device_population(n, 0xB300, dev)
    keys, src = W.device_lookups(n, m, 0xB301, dev)
    out = torch.empty(m * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def med(ts):
        return f"median {statistics.median(ts):10.3f}  spread {max(ts) - min(ts):8.3f}  all {' '.join(f'{t:.3f}' for t in ts)}"

    lines = [f"pastry_bench: n = 2^{a.log2n} nodes, {m} routes, device pointers, {a.reps} alternated repetitions, ms"]
    with KbrEngine(0) as ep, KbrEngine(0) as ec:
        ep.set_params(Params.pastry())
        pp = PastryParams.default(routeMsgAcks=0)
        load = lambda: ep.pastry_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, pp)
        timed(load)
        tb = [timed(load) for _ in range(a.reps)]
        ec.set_params(Params.chord().replace(routingType=1))
        ec.chord_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)

        def pastry():
            ep.pastry_lookup_device(keys.data_ptr(), src.data_ptr(), m, out.data_ptr())

        def chord():
            ec.lookup_device(keys.data_ptr(), src.data_ptr(), m, out.data_ptr())

        def census():
            o = out.cpu().numpy().view(ROUTE_OUT_DTYPE)
            return int((o["status"] == 0).sum()), float(o["hops"].mean())

        timed(pastry)
        okp, hp = census()
        timed(chord)
        okc, hc = census()
        rp, rc = [], []
        for _ in range(a.reps):
            rp.append(timed(pastry))
            rc.append(timed(chord))
        mp, mc = statistics.median(rp), statistics.median(rc)
        bp = 64 + 24 * pp.numberOfLeaves + 24
        lines += [f"  pastry table build (upload, leaf sets, table, records)  {med(tb)}",
                  f"  pastry route (rows {ep._L.ovs_pastry_num_rows(ep._h)})  {med(rp)}",
                  f"    delivered {okp} of {m}, mean hops {hp:.3f}, {hp * m / mp / 1e3:.1f} M hops/s, {bp} B requested per hop"
                  f" (+ the source's {bp} B a route)",
                  f"  chord semi-recursive route  {med(rc)}",
                  f"    delivered {okc} of {m}, mean hops {hc:.3f}, {hc * m / mc / 1e3:.1f} M hops/s, 64 B per hop + 104 B per route",
                  f"  pastry / chord: time {mp / mc:.3f}, time per hop {(mp / max(hp, 1e-9)) / (mc / max(hc, 1e-9)):.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
