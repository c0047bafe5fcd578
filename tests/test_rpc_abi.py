"""The C ABI of the KBRTestApp RPC test: the struct layouts a plain C compiler derives from
include/ovs_kbr.h alone equal the numpy / ctypes mirrors in oversim_amd/kbr.py and the reference
model's record, the library exports the two entry points, and the ABI version is unchanged."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _layout(tmp_path):
    exe = tmp_path / "abi_layout_rpc"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "abi_layout_rpc.c"), "-o", str(exe)], check=True)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)


def test_rpc_struct_layout(tmp_path):
    from oversim_amd import kbr
    import refmodel_rpc
    lay = _layout(tmp_path)
    assert lay["abi"] == 12
    assert (lay["answered"], lay["timeout"]) == (kbr.RPC_ANSWERED, kbr.RPC_TIMEOUT) == (refmodel_rpc.ANSWERED, refmodel_rpc.TIMEOUT)
    rec = lay["ovs_rpc_out"]
    for dt in (kbr.RPC_OUT_DTYPE, refmodel_rpc.RPC_DTYPE):
        assert dt.itemsize == rec["size"] == 32 and list(dt.names) == list(rec["fields"])
        for f, off in rec["fields"].items():
            assert dt.fields[f][1] == off, f
    st, cls = lay["ovs_kbrtest_rpc_stats"], kbr.KbrTestRpcStats
    assert C.sizeof(cls) == st["size"] and [f for f, _ in cls._fields_] == list(st["fields"])
    for f, off in st["fields"].items():
        assert getattr(cls, f).offset == off, f


def test_library_exports_the_rpc_test():
    import oversim_amd
    L = oversim_amd.lib()
    assert hasattr(L, "ovs_rpc_batch") and hasattr(L, "ovs_kbrtest_rpc_stats_batch")
    assert L.ovs_abi_version() == 12
    assert oversim_amd.RPC_OUT_DTYPE.itemsize == 32
    for name in ("rpcCall", "rpc_device", "kbrtest_rpc_stats"):
        assert callable(getattr(oversim_amd.KbrEngine, name))
