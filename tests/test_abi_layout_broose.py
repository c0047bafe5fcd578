"""The Broose structs as a C compiler sees them: tests/abi_layout_broose.c, built with gcc -std=c99 against
include/ovs_kbr.h alone, prints their sizeof/offsetof; each must match the Python mirrors in oversim_amd/kbr.py."""
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
    exe = tmp_path_factory.mktemp("abi") / "abi_layout_broose"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_broose.c"), "-o", str(exe)], check=True)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)


def test_overlay_id(layout):
    assert layout["overlay"] == kbr.OVERLAY_BROOSE == 5
    assert layout["abi"] == 12


def test_params_mirror(layout):
    want = layout["ovs_broose_params"]
    assert C.sizeof(kbr.BrooseParams) == want["size"] == 16
    assert [f for f, _ in kbr.BrooseParams._fields_] == list(want["fields"])
    for f, off in want["fields"].items():
        assert getattr(kbr.BrooseParams, f).offset == off, f


def test_ext_mirror(layout):
    want = layout["ovs_broose_ext"]
    dt = kbr.BROOSE_EXT_DTYPE
    assert dt.itemsize == want["size"] == 32
    assert list(dt.names) == list(want["fields"])
    for f, off in want["fields"].items():
        assert dt.fields[f][1] == off, f


def test_defaults_are_default_ini():
    p = kbr.BrooseParams.default()
    assert (p.bucketSize, p.rBucketSize, p.userDist, p.shiftingBits) == (8, 8, 0, 2)     # default.ini:295-298
    assert p.num_rows() == 6 and [p.row_cap(r) for r in range(6)] == [8, 8, 8, 8, 32, 56]
    assert kbr.BrooseParams.default(shiftingBits=5).num_rows() == -1
    q = kbr.Params.broose()
    assert q.overlay == kbr.OVERLAY_BROOSE and q.lookupRedundantNodes == 1 and q.lookupParallelRpcs == 1
