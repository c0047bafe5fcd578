"""The Pastry struct as a C compiler sees it: tests/abi_layout_pastry.c, built with gcc -std=c99 against
include/ovs_kbr.h alone, prints its sizeof/offsetof; each must match the Python mirror in oversim_amd/kbr.py."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from pathlib import Path

import pytest

from oversim_amd import kbr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = tmp_path_factory.mktemp("abi") / "abi_layout_pastry"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_pastry.c"), "-o", str(exe)], check=True)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)


def test_overlay_id(layout):
    assert layout["overlay"] == kbr.OVERLAY_PASTRY == 6
    assert layout["abi"] == 12


def test_params_mirror(layout):
    want = layout["ovs_pastry_params"]
    assert C.sizeof(kbr.PastryParams) == want["size"] == 24
    assert [f for f, _ in kbr.PastryParams._fields_] == list(want["fields"])
    for f, off in want["fields"].items():
        assert getattr(kbr.PastryParams, f).offset == off, f


def test_defaults_are_default_ini():
    p = kbr.PastryParams.default()
    assert (p.bitsPerDigit, p.numberOfLeaves, p.numberOfNeighbors, p.optimizeLookup, p.useRegularNextHop,
            p.routeMsgAcks) == (4, 16, 0, 0, 1, 1)                                        # default.ini:226-245
    q = kbr.Params.pastry()
    assert q.overlay == kbr.OVERLAY_PASTRY and q.routingType == 1 and q.recNumRedundantNodes == 3


def test_from_ini():
    ini = """
[General]
**.overlay*.pastry.bitsPerDigit = 2
**.overlay*.pastry.routeMsgAcks = false
**.overlay*.pastry.joinTimeout = 20s
[Config Thin]
**.overlay*.pastry.numberOfLeaves = 8
**.overlay*.pastry.optimizeLookup = true
[Config Iter]
**.overlay*.pastry.routingType = "iterative"
[Config Leafs]
**.overlay*.pastry.enableNewLeafs = true
"""
    p = kbr.PastryParams.from_ini(ini)
    assert (p.bitsPerDigit, p.numberOfLeaves, p.optimizeLookup, p.routeMsgAcks) == (2, 16, 0, 0)
    p = kbr.PastryParams.from_ini(ini, "Thin")
    assert (p.bitsPerDigit, p.numberOfLeaves, p.optimizeLookup) == (2, 8, 1)
    with pytest.raises(kbr.KbrError, match="routingType"):
        kbr.PastryParams.from_ini(ini, "Iter")
    with pytest.raises(kbr.KbrError, match="enableNewLeafs"):
        kbr.PastryParams.from_ini(ini, "Leafs")
