"""Time the replica-team DHT calls against T plain DHT calls on the team keys, same library, same process.

  python tools/diag/dht_teams_bench.py [--log2n 20] [--log2ops 20] [--teams 4] [--reps 3] [--out FILE]

A converged Chord ring of 2^log2n nodes, 2^log2ops operations with random keys, symmetric teams, numReplica 8,
device pointers.  Each repetition clears the store and times, from launch to the stream's synchronisation,
  ovs_dht_team_put_batch, ovs_dht_team_get_batch                 (numReplica 8, T teams)
then clears it again and times
  T x ovs_dht_put_batch, T x ovs_dht_get_batch on key_j          (numReplica 8 / T each)
after one warm-up of each.  The team calls do strictly more work per operation: they record every chain's
responders (n * T * hopCountMax words) and replay all of an operation's messages in one lane; the plain calls
ignore the coupling between the teams, so their records are not the same.  Writes medians and spread (max - min)
in ms to --out as text; without a GPU it writes a line saying that nothing was measured.
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--teams", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from oversim_amd import (DHT_GET_DTYPE, DHT_OP_DTYPE, DHT_PUT_DTYPE, DhtParams, DhtTeamParams, KbrEngine, Params,
                             workload as W)

    head = f"dht_teams_bench: n = 2^{a.log2n} nodes, 2^{a.log2ops} operations, symmetric, numReplica 8, T = {a.teams}"
    if not torch.cuda.is_available():
        write(head + "\nUNMEASURED: no GPU in this process\n", a.out)
        return 0
    dev = torch.device("cuda:0")
    n, m, T = 1 << a.log2n, 1 << a.log2ops, a.teams
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

    tp, dp8, dpt = DhtTeamParams.symmetric(T), DhtParams.default().replace(numReplica=8), DhtParams.default().replace(numReplica=8 // T)
    with KbrEngine(0) as eng:
        eng.set_params(Params.chord())
        eng.chord_load_device(ids_t.data_ptr(), xy_t.data_ptr(), n)
        eng.dht_store_create(1 << (a.log2ops + 5))          # 32 slots an operation for 8 entries: load factor 1/4
        tk_h = eng.dht_team_keys(keys_h, tp)
        keys, ops, gops = up(keys_h), up(ops_h), up(gops_h)
        tkeys = [up(tk_h[:, j]) for j in range(T)]
        pout = torch.empty(m * DHT_PUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        gout = torch.empty(m * DHT_GET_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        ptm = torch.empty(m * T * DHT_PUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        gtm = torch.empty(m * T * DHT_GET_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        win = torch.empty(m, dtype=torch.int32, device=dev)

        def team_put():
            eng.dht_team_device(True, keys.data_ptr(), src.data_ptr(), ops.data_ptr(), m, pout.data_ptr(), ptm.data_ptr(),
                                win.data_ptr(), tp, dp8)

        def team_get():
            eng.dht_team_device(False, keys.data_ptr(), src.data_ptr(), gops.data_ptr(), m, gout.data_ptr(), gtm.data_ptr(),
                                win.data_ptr(), tp, dp8)

        def plain_put():
            for k in tkeys:
                eng.dht_put_device(k.data_ptr(), src.data_ptr(), ops.data_ptr(), m, pout.data_ptr(), dpt)

        def plain_get():
            for k in tkeys:
                eng.dht_get_device(k.data_ptr(), src.data_ptr(), gops.data_ptr(), m, gout.data_ptr(), dpt)

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        t = {k: [] for k in ("team_put", "team_get", "plain_put", "plain_get")}
        for rep in range(a.reps + 1):                         # repetition 0 is the warm-up
            eng.dht_store_clear()
            a1, a2 = timed(team_put), timed(team_get)
            go = gout.cpu().numpy().view(DHT_GET_DTYPE)
            po = pout.cpu().numpy().view(DHT_PUT_DTYPE)
            found_team, ok_team = int((go["result_count"] == 1).sum()), int((po["outcome"] == 0).sum())
            refused = eng.dht_store_count()[1]
            eng.dht_store_clear()
            b1, b2 = timed(plain_put), timed(plain_get)
            found_plain = int((gout.cpu().numpy().view(DHT_GET_DTYPE)["result_count"] == 1).sum())
            if rep:
                for k, v in zip(t, (a1, a2, b1, b2)):
                    t[k].append(v)
        lines = [head + f", device pointers, {a.reps} repetitions after one warm-up, ms"]
        for k, v in t.items():
            calls = f"{T} x ovs_dht_{k[6:]}_batch" if k.startswith("plain") else f"ovs_dht_team_{k[5:]}_batch"
            lines.append(f"  {calls:28s} median {statistics.median(v):9.3f}  spread {max(v) - min(v):7.3f}  all {' '.join(f'{x:.3f}' for x in v)}")
        lines.append(f"  team / plain: put {statistics.median(t['team_put']) / statistics.median(t['plain_put']):.3f}, "
                     f"get {statistics.median(t['team_get']) / statistics.median(t['plain_get']):.3f}")
        lines.append(f"  team puts accepted as success {ok_team} of {m}, team gets with a value {found_team}, "
                     f"last plain get batch with a value {found_plain}, put batches refused {refused}")
    write("\n".join(lines) + "\n", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
