"""Writes tests/golden/rpc_chord_n1000.npz: a 1000-node converged Chord ring, 600 KbrTestCalls and the
reference's records (tests/refmodel_rpc.py over the CPU oracle's routes) for routingType 0 and 2, with
hopCountMax = 6 and rpcKeyTimeout = 0.9 s so that answered RPCs, dropped calls, dropped responses and
timeouts all occur.  Inputs come from seeded numpy generators (oversim_amd/workload.py).

    python tests/golden/make_golden_rpc.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import refmodel_rpc as R                                   # noqa: E402
from oracle_lib import OracleNet, chord_params             # noqa: E402
from oversim_amd import workload as W                      # noqa: E402

N, M, SEED, RND, HCM, TIMEOUT = 1000, 600, 0x52504331, 1, 6, 0.9


def main() -> int:
    net = W.population(N, SEED)
    k1, s1 = W.lookups(net.ids, M // 2, SEED + 1, node_ids=True)
    k2, s2 = W.lookups(net.ids, M - M // 2, SEED + 2, node_ids=False)
    keys, src = np.concatenate([k1, k2]), np.concatenate([s1, s2])
    keys[:4] = net.ids[src[:4]]
    d = dict(ids=net.ids, xy=net.xy, keys=keys, src=src, simtime_round=RND, hop_count_max=HCM, rpc_key_timeout=TIMEOUT)
    for rt in (0, 2):
        o = OracleNet("chord", net.ids, net.xy, chord_params(routingType=rt, simtimeRound=RND, hopCountMax=HCM))
        ref = R.rpc_batch(net.ids, net.xy, keys, src, R.oracle_leg(o), rt, bool(RND), rpc_key_timeout=TIMEOUT)
        print(f"routingType {rt}: answered {(ref['outcome'] == 0).sum()}, timed out {(ref['outcome'] == 1).sum()}, "
              f"calls dropped {(ref['status'] != 0).sum()}, responses dropped "
              f"{((ref['status'] == 0) & (ref['resp_status'] != 0)).sum()}")
        for f in R.FIELDS:
            d[f"rt{rt}_{f}"] = ref[f]
    out = HERE / "rpc_chord_n1000.npz"
    np.savez_compressed(out, **d)
    print(out, out.stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
