"""ASan + UBSan build of the CPU restatement (oracle/ovs_oracle.c) and the host-side .ini binder
(oversim_amd/csrc/ovs_ini.cpp), compiled with -Wall -Wextra -Werror and run on small networks
through every oracle entry point (tests/sanitize_driver.cpp).  SURVEY.md §5: sanitizers run on the
host code; GPU code is checked by the parity tests.  CPU only."""
from __future__ import annotations

import math
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
WARN = ["-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None, reason="needs gcc/g++")
def test_oracle_and_ini_binder_clean_under_asan_ubsan(tmp_path):
    objs = []
    cmds = [
        ["gcc", "-std=gnu11", "-fopenmp", "-ffp-contract=off", *SAN, *WARN, "-c", str(ROOT / "oracle" / "ovs_oracle.c"),
         "-o", str(tmp_path / "oracle.o")],
        ["g++", "-std=c++17", *SAN, *WARN, "-c", str(ROOT / "oversim_amd" / "csrc" / "ovs_ini.cpp"),
         "-o", str(tmp_path / "ini.o")],
        ["g++", "-std=c++17", *SAN, *WARN, "-c", str(ROOT / "tests" / "sanitize_driver.cpp"),
         "-o", str(tmp_path / "driver.o")],
    ]
    for c in cmds:
        r = subprocess.run(c, capture_output=True, text=True)
        assert r.returncode == 0, f"{' '.join(c)}\n{r.stdout}{r.stderr}"
        objs.append(c[-1])
    exe = tmp_path / "sanitize_driver"
    r = subprocess.run(["g++", "-fopenmp", *SAN, *objs, "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the environment is passed through unchanged (a preloaded library may precede the ASan runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1",
               OMP_NUM_THREADS="2")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_table_bookkeeping_clean_under_asan_ubsan(tmp_path):
    """The C ABI's host-side table code (oversim_amd/csrc/host_tables.cpp: explicit Chord tables, the
    fixfingers and stabilize rounds' updates, EpiChord snapshot validation and ordering) built with
    plain g++ under ASan/UBSan -Werror and driven through a converging ring and broken inputs
    (tests/host_tables_driver.cpp)."""
    inc = ["-I", str(ROOT / "oversim_amd" / "csrc")]
    objs = []
    for src, o in ((ROOT / "oversim_amd" / "csrc" / "host_tables.cpp", "ht.o"),
                   (ROOT / "tests" / "host_tables_driver.cpp", "drv.o")):
        c = ["g++", "-std=c++17", *SAN, *WARN, *inc, "-c", str(src), "-o", str(tmp_path / o)]
        r = subprocess.run(c, capture_output=True, text=True)
        assert r.returncode == 0, f"{' '.join(c)}\n{r.stdout}{r.stderr}"
        objs.append(str(tmp_path / o))
    exe = tmp_path / "host_tables_driver"
    r = subprocess.run(["g++", *SAN, *objs, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_call_frame_clean_under_asan_ubsan(tmp_path):
    """The C ABI's per-call device memory (oversim_amd/csrc/call_frame.hpp: the call frame, the
    event-ordered cached buffer and the counter slots) built with plain g++ under ASan/UBSan -Werror
    against a fake HIP runtime whose every call is made to fail in turn: each failure is reported,
    nothing leaks, every lease records its event, and a device-pointer frame calls nothing
    (tests/call_frame_driver.cpp).  No HIP library is linked."""
    exe = tmp_path / "call_frame_driver"
    c = ["g++", "-std=c++17", *SAN, *WARN, "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
         "-I", str(ROOT / "oversim_amd" / "csrc"), str(ROOT / "tests" / "call_frame_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(c, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(c)}\n{r.stdout}{r.stderr}"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_persist_plan_clean_under_asan_ubsan(tmp_path):
    """The persistent-slice scheduler's host plan (oversim_amd/csrc/persist.hpp: static slices, block
    count and dynamic split of K1, K2, K2x and K3) built with plain g++ under ASan/UBSan -Werror: the
    slices and the dynamic region partition every batch, a replay of waves claiming chunks in an
    arbitrary interleaving visits every index once, and each kernel's numbers equal literal values
    worked out from its former launcher's formulas (tests/persist_plan_driver.cpp).  No HIP compiler
    and no HIP library."""
    exe = tmp_path / "persist_plan_driver"
    c = ["g++", "-std=c++17", *SAN, *WARN, "-I", str(ROOT / "oversim_amd" / "csrc"),
         str(ROOT / "tests" / "persist_plan_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(c, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(c)}\n{r.stdout}{r.stderr}"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


def _cstddev(values=None, sums=None):
    """cStdDev as cstddev.hpp finishes it, in Python floats (IEEE doubles, no contraction) in the same
    operation order: (count, mean, stddev, min, max); an empty one stays zeroed."""
    if sums is None:
        cnt, s, sq, mn, mx = 0, 0.0, 0.0, math.inf, -math.inf
        for v in values:
            s += v
            sq += v * v
            mn = v if v < mn else mn
            mx = v if v > mx else mx
            cnt += 1
    else:
        cnt, s, sq, mn, mx = sums
    if not cnt:
        return (0, 0.0, 0.0, 0.0, 0.0)
    var = 0.0
    if cnt > 1:
        var = (sq - s * s / float(cnt)) / float(cnt - 1)
        if var < 0:
            var = 0.0
    return (cnt, s / float(cnt), math.sqrt(var), mn, mx)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cstddev_clean_and_exact_under_asan_ubsan(tmp_path):
    """The statistics calls' one accumulator (oversim_amd/csrc/cstddev.hpp) built with plain g++ under
    ASan/UBSan -Werror and -ffp-contract=off (tests/cstddev_driver.cpp): an empty accumulator, one and two
    values, a variance that rounds below zero and clamps, exact integer sums against collect() over the
    same samples, and a row in the device layout -- each compared bit for bit with the same operations
    in Python floats.  No HIP compiler and no HIP library."""
    exe = tmp_path / "cstddev_driver"
    c = ["g++", "-std=c++17", "-ffp-contract=off", *SAN, *WARN, "-I", str(ROOT / "oversim_amd" / "csrc"),
         str(ROOT / "tests" / "cstddev_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(c, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(c)}\n{r.stdout}{r.stderr}"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) == 6:
            got[f[0]] = (int(f[1]),) + tuple(float.fromhex(x) for x in f[2:])
    samples = [3, 7, 7, 12, 1, 30]
    want = {
        "empty": _cstddev([]),
        "one": _cstddev([2.5]),
        "two": _cstddev([1.0, 4.0]),
        "clamp": _cstddev([0.1, 0.1, 0.1]),
        "collect": _cstddev([float(v) for v in samples]),
        "sums": _cstddev(sums=(len(samples), float(sum(samples)), float(sum(v * v for v in samples)),
                               float(min(samples)), float(max(samples)))),
        "row": _cstddev(sums=(4, 10.5, 40.25, 0.5, 6.0)),
        "empty_row": _cstddev([]),
    }
    assert set(got) == set(want), sorted(got)
    for name, w in want.items():
        g = got[name]
        assert g[0] == w[0] and all(a.hex() == b.hex() for a, b in zip(g[1:], w[1:])), (name, g, w)
    # the cases are what they claim to be
    s = 0.1 + 0.1 + 0.1
    sq = 0.1 * 0.1 + 0.1 * 0.1 + 0.1 * 0.1
    assert sq - s * s / 3.0 < 0 and got["clamp"][2] == 0.0, "three times 0.1 must round to a negative variance and clamp"
    assert got["one"] == (1, 2.5, 0.0, 2.5, 2.5)
    assert got["two"][:2] == (2, 2.5) and got["two"][2] == math.sqrt(4.5)
    assert got["sums"] == got["collect"], "from_sums over exact integer sums must equal collect() over the samples"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_checks_clean_under_asan_ubsan(tmp_path):
    """The entry points' refusals that depend on plain values only (oversim_amd/csrc/host_checks.hpp: the
    shard steps' arc map, the shapes of Kademlia tables and routingBucketSize, the table builders' bad
    codes, the refresh lookups' parameters, node-index ranges) built with plain g++ under ASan/UBSan
    -Werror: every case's status and literal message (tests/host_checks_driver.cpp).  No HIP compiler and
    no HIP library."""
    exe = tmp_path / "host_checks_driver"
    c = ["g++", "-std=c++17", *SAN, *WARN, "-I", str(ROOT / "oversim_amd" / "csrc"),
         str(ROOT / "tests" / "host_checks_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(c, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(c)}\n{r.stdout}{r.stderr}"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
