"""Writes tests/golden/dht_teams_n1000.npz: one symmetric (T = 4) and one repeated-hashing (T = 2) put batch
and get batch on the golden 1000-node ring, from the event-heap model tests/refmodel_dht_teams.py alone.  The
file is written only after both anchors hold (T = 1 equals the plain DHT model; without serialisation times
every team equals a single-team operation).

    python tests/golden/make_dht_teams_golden.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import dht_teams_cases as K          # noqa: E402
import refmodel_dht as D             # noqa: E402
import refmodel_dht_teams as TM      # noqa: E402

N_OPS = 384


def build() -> dict:
    keys, src, put, get1, _, _, _ = K.batches(1000, N_OPS, 2024)
    out = dict(keys=keys, src=src, put_ops=put.view(np.uint8), get_ops=get1.view(np.uint8))
    for name, mode, T in (("sym", TM.SYMMETRIC, 4), ("rh", TM.REPEATED_HASHING, 2)):
        M = K.model(1000, mode, T)
        out[name + "_team_keys"] = TM.team_keys(keys, mode, T)
        for what, res in (("put", M.put_batch(keys, src, put)), ("get", M.get_batch(keys, src, get1))):
            out[f"{name}_{what}_out"] = res[0].view(np.uint8)
            out[f"{name}_{what}_team"] = res[1].reshape(-1).view(np.uint8)
            out[f"{name}_{what}_winner"] = res[2]
    return out


def main() -> int:
    for n in (9, 1000):
        K.anchor_one_team(n)
    K.anchor_no_coupling(1000, TM.SYMMETRIC, 4)
    K.anchor_no_coupling(1000, TM.REPEATED_HASHING, 2)
    np.savez_compressed(HERE / "dht_teams_n1000.npz", **build())
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
