"""Regenerates tests/golden/dht_chord_n1000.npz from the replay (tests/refmodel_dht.py) with the CPU oracle's
LookupCalls: a put batch, a get batch, an overwrite batch and a get batch after the first TTLs ran out on a
1000-node Chord ring, 500 operations each.  Run from the repository root: python tests/golden/make_golden_dht.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import refmodel_dht as D  # noqa: E402
from oracle_lib import OracleNet, chord_params  # noqa: E402
from oversim_amd import workload as W  # noqa: E402

SEC = 10**9


def main():
    m = 500
    net = W.population(1000, 0x444854)
    rng = np.random.default_rng(2026)
    k1, s1 = W.lookups(net.ids, m // 2, 61, node_ids=True)
    k2, s2 = W.lookups(net.ids, m - m // 2, 62, node_ids=False)
    keys, src = np.ascontiguousarray(np.concatenate([k1, k2])), np.ascontiguousarray(np.concatenate([s1, s2]))
    keys[:16] = keys[16]
    put = D.make_ops(m, t0_ns=rng.integers(0, 5 * SEC, m), token=np.arange(m) + 1, vlen=rng.integers(1, 200, m),
                     ttl=np.where(np.arange(m) % 2, 60, 0), id=1 + np.arange(m) % 3)
    get1 = put.copy()
    get1["t0_ns"] = 20 * SEC + rng.integers(0, SEC, m)
    over = put[:m // 2].copy()
    over["t0_ns"] = 30 * SEC + rng.integers(0, SEC, m // 2)
    over["token"] += 10**6
    over["vlen"] = np.where(np.arange(m // 2) % 7 == 3, 0, over["vlen"])
    over["ttl"] = 0
    get2 = put.copy()
    get2["t0_ns"] = 100 * SEC
    o = OracleNet("chord", net.ids, net.xy, chord_params(simtimeRound=1))
    M = D.DhtModel(net.xy, D.oracle_lookup(o, 4), True)
    res = dict(ids=net.ids, xy=net.xy, keys=keys, src=src, put=put, get1=get1, over=over, get2=get2,
               put_out=M.put_batch(keys, src, put), get1_out=M.get_batch(keys, src, get1),
               over_out=M.put_batch(keys[:m // 2], src[:m // 2], over), get2_out=M.get_batch(keys, src, get2))
    np.savez_compressed(ROOT / "tests" / "golden" / "dht_chord_n1000.npz", **res)
    print({k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main()
