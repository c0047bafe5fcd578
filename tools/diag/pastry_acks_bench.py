"""Time Pastry's acked route and RPC test beside the plain route on the same tables and batch.

  python tools/diag/pastry_acks_bench.py [--log2n 20] [--lookups 10000000] [--reps 5] [--out FILE]

Converged Pastry tables of 2^log2n nodes at the defaults (bitsPerDigit 4, numberOfLeaves 16, recNumRedundantNodes 3),
loaded once without acks and once with them (routeMsgAcks is a property of the context); `lookups` random keys from
random sources on device pointers.  After one warm-up of each, every repetition alternates three calls un-profiled,
each timed from launch to the stream's synchronisation:

  plain   ovs_pastry_route_batch, routeMsgAcks = 0        (k_pastry_route<false>)
  acked   ovs_pastry_acked_route_batch with ack records    (k_pastry_route<true>)
  rpc     ovs_pastry_rpc_batch, routeMsgAcks = 1           (k_pastry_route<true> without ack records + k_rpc_finish)

Writes medians, spread (max - min), hops/s and the ratios to --out as text.  The acked instantiation reads the same bytes a
hop as the plain one (64 B record + 24 B x numberOfLeaves leaf row + one 24 B slot); it writes 16 B more a route.
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
    from oversim_amd.kbr import PASTRY_ACK_OUT_DTYPE, RPC_OUT_DTYPE

    dev = torch.device("cuda:0")
    n, m = 1 << a.log2n, a.lookups
    ids_t, xy_t = W.device_population(n, 0xB300, dev)
    keys, src = W.device_lookups(n, m, 0xB301, dev)
    out = torch.empty(m * ROUTE_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ack = torch.empty(m * PASTRY_ACK_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rpc = torch.empty(m * RPC_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def med(ts):
        return f"median {statistics.median(ts):10.3f}  spread {max(ts) - min(ts):8.3f}  all {' '.join(f'{t:.3f}' for t in ts)}"

    lines = [f"pastry_acks_bench: n = 2^{a.log2n} nodes, {m} routes, device pointers, {a.reps} alternated repetitions, ms"]
    with KbrEngine(0) as e0, KbrEngine(0) as e1:
        for e, flag in ((e0, 0), (e1, 1)):
            e.set_params(Params.pastry())
            e.pastry_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, PastryParams.default(routeMsgAcks=flag))

        def plain():
            e0.pastry_lookup_device(keys.data_ptr(), src.data_ptr(), m, out.data_ptr())

        def acked():
            e1.pastry_acked_lookup_device(keys.data_ptr(), src.data_ptr(), m, out.data_ptr(), ack.data_ptr())

        def rpcs():
            e1.pastry_rpc_device(keys.data_ptr(), src.data_ptr(), m, rpc.data_ptr())

        def census():
            o = out.cpu().numpy().view(ROUTE_OUT_DTYPE)
            return int((o["status"] == 0).sum()), float(o["hops"].mean())

        timed(plain)
        ok0, h0 = census()
        timed(acked)
        ok1, h1 = census()
        ao = ack.cpu().numpy().view(PASTRY_ACK_OUT_DTYPE)
        timed(rpcs)
        ro = rpc.cpu().numpy().view(RPC_OUT_DTYPE)
        answered = int((ro["outcome"] == 0).sum())
        tp, ta, tr = [], [], []
        for _ in range(a.reps):
            tp.append(timed(plain))
            ta.append(timed(acked))
            tr.append(timed(rpcs))
        mp, ma, mr = (statistics.median(t) for t in (tp, ta, tr))
        lines += [f"  plain route (routeMsgAcks = 0)   {med(tp)}",
                  f"    delivered {ok0} of {m}, mean hops {h0:.3f}, {h0 * m / mp / 1e3:.1f} M hops/s",
                  f"  acked route with ack records     {med(ta)}",
                  f"    delivered {ok1} of {m}, mean hops {h1:.3f}, {h1 * m / ma / 1e3:.1f} M hops/s, mean acks {ao['acks'].mean():.3f}, "
                  f"largest ack round trip {int(ao['max_ack_rtt_ns'].max())} ns, ack timeouts {int((ao['timeout_hop'] != 0xFF).sum())}",
                  f"  RPC test (routeMsgAcks = 1)      {med(tr)}",
                  f"    answered {answered} of {m}, {h1 * m / mr / 1e3:.1f} M call hops/s",
                  f"  acked / plain: {ma / mp:.4f}   rpc / acked: {mr / ma:.4f}   rpc / plain: {mr / mp:.4f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
