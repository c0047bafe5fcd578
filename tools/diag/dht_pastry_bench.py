"""Time the DHT calls on a Pastry context beside the bare Pastry LookupCall and beside the same DHT calls on Chord.

  python tools/diag/dht_pastry_bench.py [--log2n 20] [--log2ops 20] [--reps 5] [--out FILE]

Converged tables of 2^log2n nodes on the same ids and coordinates: Pastry at the defaults (bitsPerDigit 4,
numberOfLeaves 16, routingType iterative) and a Chord ring (successorListSize 8).  2^log2ops operations with random
keys from random sources, numReplica = numGetRequests = 4, 100 B values, device pointers.  After one warm-up
repetition each repetition clears the stores and times, from launch to the stream's synchronisation and alternated
between the overlays,
  ovs_dht_put_batch, ovs_dht_get_batch            on Pastry and on Chord
  ovs_pastry_lookup_batch with num_siblings 4     the DHT calls' lookup phase on Pastry, alone
  ovs_lookup_batch with num_siblings 4            the same on Chord
The replica phase of a DHT call is the call minus the bare lookup: on both overlays it is the same kernels of
dht.hip on the same number of pairs, so it should cost about the same.  Writes medians and spread (max - min) in ms
to --out as text; without a GPU it writes a line saying that nothing was measured.
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def write(text: str, out: str) -> None:
    print(text, end="")
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(text)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--log2ops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from oversim_amd import (DHT_GET_DTYPE, DHT_OP_DTYPE, DHT_PUT_DTYPE, LOOKUP_OUT_DTYPE, DhtParams, KbrEngine, Params,
                             PastryParams, workload as W)
    from oversim_amd.kbr import DEVICE_PTRS

    R = 4
    head = f"dht_pastry_bench: n = 2^{a.log2n} nodes, 2^{a.log2ops} operations, numReplica {R}, numGetRequests {R}"
    if not torch.cuda.is_available():
        write(head + "\nUNMEASURED: no GPU in this process\n", a.out)
        return 0
    dev = torch.device("cuda:0")
    n, m = 1 << a.log2n, 1 << a.log2ops
    ids_t, xy_t = W.device_population(n, 0xD47, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    src = torch.randint(0, n, (m,), dtype=torch.int32, device=dev, generator=g)
    keys_h = np.random.default_rng(5).integers(0, 2**32, (m, 5), dtype=np.uint32)
    ops_h = np.zeros(m, dtype=DHT_OP_DTYPE)
    ops_h["token"], ops_h["kind"], ops_h["id"], ops_h["vlen"], ops_h["ttl"] = np.arange(m) + 1, 1, 1, 100, 0
    gops_h = ops_h.copy()
    gops_h["t0_ns"] = 100 * 10**9

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    keys, ops, gops = up(keys_h), up(ops_h), up(gops_h)
    pout = torch.empty(m * DHT_PUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    gout = torch.empty(m * DHT_GET_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    lout = torch.empty(m * LOOKUP_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    sib = torch.empty(m * R, dtype=torch.int32, device=dev)
    dp = DhtParams.default().replace(numReplica=R, numGetRequests=R)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    with KbrEngine(0) as ep, KbrEngine(0) as ec:
        ep.set_params(Params.pastry().replace(routingType=0))
        ep.pastry_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n, PastryParams.default())
        ec.set_params(Params.chord())
        ec.chord_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)
        for e in (ep, ec):
            e.dht_store_create(1 << (a.log2ops + 4))          # 16 slots an operation for 4 entries: load factor 1/4

        def put(e):
            return lambda: e.dht_put_device(keys.data_ptr(), src.data_ptr(), ops.data_ptr(), m, pout.data_ptr(), dp)

        def get(e):
            return lambda: e.dht_get_device(keys.data_ptr(), src.data_ptr(), gops.data_ptr(), m, gout.data_ptr(), dp)

        def pastry_lookup():
            ep.pastry_lookup_call_device(keys.data_ptr(), src.data_ptr(), m, R, lout.data_ptr(), sib.data_ptr())

        def chord_lookup():
            ec._chk(ec._L.ovs_lookup_batch(ec._h, C.c_void_p(keys.data_ptr()), C.c_void_p(src.data_ptr()), m, R,
                                           C.c_void_p(lout.data_ptr()), C.c_void_p(sib.data_ptr()), DEVICE_PTRS, None),
                    "ovs_lookup_batch")

        names = ("pastry put", "pastry get", "pastry lookup", "chord put", "chord get", "chord lookup")
        t = {k: [] for k in names}
        facts = {}
        for rep in range(a.reps + 1):                         # repetition 0 is the warm-up
            ep.dht_store_clear()
            ec.dht_store_clear()
            row = []
            for tag, e, look in (("pastry", ep, pastry_lookup), ("chord", ec, chord_lookup)):
                row.append(timed(put(e)))
                po = pout.cpu().numpy().view(DHT_PUT_DTYPE)
                row.append(timed(get(e)))
                go = gout.cpu().numpy().view(DHT_GET_DTYPE)
                row.append(timed(look))
                lo = lout.cpu().numpy().view(LOOKUP_OUT_DTYPE)
                facts[tag] = (int((po["outcome"] == 0).sum()), int((go["result_count"] == 1).sum()), float(lo["hops"].mean()),
                              int((lo["status"] == 0).sum()), e.dht_store_count())
            if rep:
                for k, v in zip(names, row):
                    t[k].append(v)
        med = {k: statistics.median(v) for k, v in t.items()}
        lines = [head + f", device pointers, {a.reps} repetitions after one warm-up, ms"]
        for k, call in zip(names, ("ovs_dht_put_batch", "ovs_dht_get_batch", f"ovs_pastry_lookup_batch ns={R}",
                                   "ovs_dht_put_batch", "ovs_dht_get_batch", f"ovs_lookup_batch ns={R}")):
            v = t[k]
            lines.append(f"  {k.split()[0]:6s} {call:30s} median {med[k]:9.3f}  spread {max(v) - min(v):7.3f}  "
                         f"all {' '.join(f'{x:.3f}' for x in v)}")
        for tag in ("pastry", "chord"):
            ok, found, hops, valid, cnt = facts[tag]
            lines.append(f"  {tag}: replica phase (DHT call - bare lookup) put {med[tag + ' put'] - med[tag + ' lookup']:.3f}, "
                         f"get {med[tag + ' get'] - med[tag + ' lookup']:.3f}; puts succeeded {ok} of {m}, gets with a value {found}, "
                         f"lookups valid {valid}, mean hops {hops:.3f}, store (slots, refused) {cnt}")
        lines.append(f"  pastry / chord: put {med['pastry put'] / med['chord put']:.3f}, get {med['pastry get'] / med['chord get']:.3f}, "
                     f"lookup {med['pastry lookup'] / med['chord lookup']:.3f}")
    write("\n".join(lines) + "\n", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
