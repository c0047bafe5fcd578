"""Host-side mirror of OverSim's KBR lookup interface over the C ABI (include/ovs_kbr.h).

Names follow the reference so a test reads like OverSim code:

  KbrEngine.lookupCall(keys, src, numSiblings)
        -> BaseOverlay::lookupRpc for a batch of KBRTestApp LookupCalls
           (KBRTestApp.cc:190-206, BaseOverlay.cc:1938-1968, 1272-1300)
  KbrEngine.findNode(node, key, numRedundantNodes, numSiblings)
        -> BaseOverlay::findNode (BaseOverlay.h:693-696; Chord.cc:548-599,
           Kademlia.cc:1101-1246), evaluated at `node`
  KbrEngine.isSiblingFor(node, key, numSiblings)
        -> BaseOverlay::isSiblingFor (BaseOverlay.h:417-418), node == thisNode
  KbrEngine.lookup(keys, src)
        -> AbstractLookup::lookup + LookupListener::lookupFinished for a batch
           of KBRTestApp one-way tests (IterativeLookup.cc:695-723,
           BaseOverlay.cc:1241-1307)

Errors raised by the engine become KbrError (the reference throws
cRuntimeError).  There is no CPU fallback: importing this module without the
built HIP library raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np

# OVS_LIB selects an experimental build of the same engine (tools/build_alt_src.sh); default: the in-tree build
_LIB_PATH = Path(os.environ.get("OVS_LIB") or Path(__file__).resolve().parent / "libovs_kbr.so")

OVERLAY_CHORD = 1
OVERLAY_KADEMLIA = 2
OVERLAY_KOORDE = 3
OVERLAY_EPICHORD = 4
OVERLAY_BROOSE = 5
OVERLAY_PASTRY = 6
DEVICE_PTRS = 0x1
NONE = 0xFFFFFFFF

STATUS = {0: "OK", 1: "EINVAL", 2: "ENOMEM", 3: "EDEVICE", 4: "ESTATE", 5: "ENOTSUP"}
LOOKUP_STATUS = {0: "OK", 1: "TIMEOUT", 2: "RPC_TIMEOUT", 3: "HOPMAX", 4: "NO_NEXT", 5: "BROKEN", 6: "INVALID"}


class KbrError(RuntimeError):
    """cRuntimeError equivalent raised from an ovs_status != OVS_OK."""


class Params(C.Structure):
    """ovs_params; field names are the NED/.ini parameter names."""

    _fields_ = [
        ("overlay", C.c_int32), ("keyLength", C.c_int32), ("hopCountMax", C.c_int32),
        ("successorListSize", C.c_int32), ("extendedFingerTable", C.c_int32),
        ("numFingerCandidates", C.c_int32), ("k", C.c_int32), ("s", C.c_int32), ("b", C.c_int32),
        ("lookupRedundantNodes", C.c_int32), ("lookupParallelPaths", C.c_int32),
        ("lookupParallelRpcs", C.c_int32), ("lookupMerge", C.c_int32),
        ("lookupStrictParallelRpcs", C.c_int32), ("lookupVisitOnlyOnce", C.c_int32),
        ("lookupAcceptLateSiblings", C.c_int32), ("lookupUseAllParallelResponses", C.c_int32),
        ("lookupNewRpcOnEveryTimeout", C.c_int32), ("lookupNewRpcOnEveryResponse", C.c_int32),
        ("lookupFinishOnFirstUnchanged", C.c_int32), ("lookupVerifySiblings", C.c_int32),
        ("lookupMajoritySiblings", C.c_int32), ("routingType", C.c_int32), ("numSiblings", C.c_int32),
        ("useCoordinateBasedDelay", C.c_int32), ("simtimeRound", C.c_int32), ("testMsgSize", C.c_int32),
        ("recNumRedundantNodes", C.c_int32), ("rpcUdpTimeout", C.c_double), ("lookupTimeout", C.c_double),
        ("jitter", C.c_double), ("constantDelay", C.c_double), ("datarate", C.c_double),
        ("accessDelay", C.c_double), ("kadSeed", C.c_uint64),
        ("shiftingBits", C.c_int32), ("deBruijnListSize", C.c_int32), ("useOtherLookup", C.c_int32),
        ("useSucList", C.c_int32), ("bucketType", C.c_int32), ("cacheTTL", C.c_double),
        ("globalNodeLimit", C.c_int32), ("extraNodesFinalBucket", C.c_int32), ("rpcKeyTimeout", C.c_double),
        ("measureAuthBlock", C.c_int32),
    ]

    @classmethod
    def default(cls, overlay: int = OVERLAY_CHORD) -> "Params":
        p = cls()
        lib().ovs_params_default(overlay, C.byref(p))
        return p

    @classmethod
    def chord(cls) -> "Params":
        return cls.default(OVERLAY_CHORD)

    @classmethod
    def kademlia(cls) -> "Params":
        return cls.default(OVERLAY_KADEMLIA)

    @classmethod
    def koorde(cls) -> "Params":
        return cls.default(OVERLAY_KOORDE)

    @classmethod
    def epichord(cls) -> "Params":
        return cls.default(OVERLAY_EPICHORD)

    @classmethod
    def broose(cls) -> "Params":
        """The overlay-independent parameters for a Broose context; Broose's own are BrooseParams."""
        return cls.default(OVERLAY_BROOSE)

    @classmethod
    def pastry(cls) -> "Params":
        """The overlay-independent parameters for a Pastry context: Pastry's routingType is semi-recursive
        (default.ini:246); Pastry's own parameters are PastryParams."""
        return cls.default(OVERLAY_PASTRY).replace(routingType=1)

    @classmethod
    def from_ini(cls, text: str, config: str | None = None, overlay: int = OVERLAY_CHORD,
                 base: "Params | None" = None) -> "Params":
        p = cls()
        C.memmove(C.byref(p), C.byref(base), C.sizeof(cls)) if base is not None else lib().ovs_params_default(overlay, C.byref(p))
        err = C.create_string_buffer(512)
        st = lib().ovs_params_from_ini(C.byref(p), text.encode(), config.encode() if config else None, err, 512)
        if st != 0:
            raise KbrError(f"ovs_params_from_ini: {STATUS.get(st, st)}: {err.value.decode()}")
        return p

    @classmethod
    def from_ini_file(cls, path, config: str | None = None, overlay: int = OVERLAY_CHORD) -> "Params":
        """Like from_ini, reading the file and its `include` lines as Cmdenv does."""
        p = cls()
        lib().ovs_params_default(overlay, C.byref(p))
        err = C.create_string_buffer(512)
        st = lib().ovs_params_from_ini_file(C.byref(p), str(path).encode(), config.encode() if config else None, err, 512)
        if st != 0:
            raise KbrError(f"ovs_params_from_ini_file: {STATUS.get(st, st)}: {err.value.decode()}")
        return p

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_ if not f.startswith("_")}

    def replace(self, **kw) -> "Params":
        p = Params()
        C.memmove(C.byref(p), C.byref(self), C.sizeof(Params))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


ROUTE_OUT_DTYPE = np.dtype([("responsible", "<u4"), ("hops", "<u2"), ("status", "u1"),
                            ("one_way_hops", "u1"), ("latency_ns", "<i8")])
assert ROUTE_OUT_DTYPE.itemsize == 16
KOORDE_EXT_DTYPE = np.dtype([("route_key", "<u4", 5), ("step", "<i4"), ("has_route_key", "<i4")])
assert KOORDE_EXT_DTYPE.itemsize == 28
BROOSE_EXT_DTYPE = np.dtype([("route_key", "<u4", 5), ("step", "<i4"), ("has_ext", "u1"), ("right_shifting", "u1"),
                             ("pad", "u1", 2), ("last_node", "<u4")])
assert BROOSE_EXT_DTYPE.itemsize == 32
LOOKUP_OUT_DTYPE = np.dtype([("num_siblings", "<u4"), ("hops", "<u2"), ("status", "u1"),
                             ("is_valid", "u1"), ("latency_ns", "<i8")])
assert LOOKUP_OUT_DTYPE.itemsize == 16
BCAST_NODE_DTYPE = np.dtype([("arrival_ns", "<i8"), ("parent", "<u4"), ("hops", "<u2"), ("rank", "<u2")])
assert BCAST_NODE_DTYPE.itemsize == 16
RPC_OUT_DTYPE = np.dtype([("responder", "<u4"), ("hop_count", "<u2"), ("call_hops", "u1"), ("status", "u1"),
                          ("outcome", "u1"), ("resp_status", "u1"), ("pad", "u1", 6), ("rtt_ns", "<i8"),
                          ("call_latency_ns", "<i8")])
assert RPC_OUT_DTYPE.itemsize == 32
RPC_ANSWERED, RPC_TIMEOUT = 0, 1
PASTRY_ACK_OUT_DTYPE = np.dtype([("max_ack_rtt_ns", "<i8"), ("acks", "<u2"), ("timeout_hop", "u1"), ("pad", "u1", 5)])
assert PASTRY_ACK_OUT_DTYPE.itemsize == 16
PASTRY_NO_TIMEOUT_HOP = 0xFF
DHT_OP_DTYPE = np.dtype([("t0_ns", "<i8"), ("token", "<u8"), ("kind", "<u4"), ("id", "<u4"), ("vlen", "<u4"),
                         ("ttl", "<i4")])
assert DHT_OP_DTYPE.itemsize == 32
DHT_PUT_DTYPE = np.dtype([("latency_ns", "<i8"), ("bytes", "<u4"), ("hop_count", "<u2"), ("messages", "<u2"),
                          ("outcome", "u1"), ("status", "u1"), ("num_sent", "u1"), ("num_responses", "u1"),
                          ("pad", "u1", 4)])
assert DHT_PUT_DTYPE.itemsize == 24
DHT_GET_DTYPE = np.dtype([("latency_ns", "<i8"), ("bytes", "<u4"), ("hop_count", "<u2"), ("messages", "<u2"),
                          ("outcome", "u1"), ("status", "u1"), ("num_sent", "u1"), ("num_responses", "u1"),
                          ("result_count", "<u4"), ("value_token", "<u8"), ("value_len", "<u4"), ("server", "<u4")])
assert DHT_GET_DTYPE.itemsize == 40
DHT_ENTRY_DTYPE = np.dtype([("key", "<u4", 5), ("kind", "<u4"), ("id", "<u4"), ("vlen", "<u4"), ("token", "<u8"),
                            ("expiry_ns", "<i8")])
assert DHT_ENTRY_DTYPE.itemsize == 48
DHT_SUCCESS, DHT_FAILED, DHT_LOOKUP_FAILED = 0, 1, 2
DHT_EXPECT_DTYPE = np.dtype([("token", "<u8"), ("endtime_ns", "<i8"), ("known", "<u4"), ("pad", "<u4")])
assert DHT_EXPECT_DTYPE.itemsize == 24


SCRIBE_NODE_DTYPE = np.dtype([("group", "<u4"), ("node", "<u4"), ("parent", "<u4"), ("depth", "<u2"), ("flags", "<u2")])
SCRIBE_MSG_DTYPE = np.dtype([("response_ns", "<i8"), ("last_delivery_ns", "<i8"), ("receivers", "<u4"),
                             ("forwarded", "<u4"), ("publish_hops", "<u2"), ("depth", "<u2"), ("status", "u1"),
                             ("pad", "u1", 3)])
SCRIBE_DELIVERY_DTYPE = np.dtype([("msg", "<u4"), ("node", "<u4"), ("hops", "<u4"), ("pad", "<u4"), ("arrival_ns", "<i8")])
SCRIBE_SUBSCRIBER, SCRIBE_ROOT, SCRIBE_FORWARDER = 1, 2, 4
SCRIBE_STATUS = {0: "OK", 1: "WRONG_ROOT", 2: "ROUTE_FAILED"}


class ScribeParams:
    """What ALMTest sets for a publish: almTest.messageLength (default.ini:81), the ALM payload in bytes."""

    def __init__(self, messageLength: int = 100):
        self.messageLength = int(messageLength)

    @classmethod
    def from_ini(cls, text: str, config: str | None = None) -> "ScribeParams":
        """Reads `**.almTest.messageLength` from ini text: the [General] section, then `config`'s, the
        last assignment winning; units are not accepted (the key is a plain int)."""
        out = cls()
        section = "General"
        for raw in text.splitlines():
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            if line.startswith("[") and line.endswith("]"):
                section = line[1:-1].strip()
                section = section[len("Config "):].strip() if section.startswith("Config ") else section
                continue
            if section != "General" and section != config:
                continue
            key, sep, val = line.partition("=")
            if sep and key.strip().endswith("almTest.messageLength"):
                out.messageLength = int(val.strip())
        if out.messageLength < 0:
            raise ValueError("almTest.messageLength must be >= 0")
        return out


class BrooseParams(C.Structure):
    """ovs_broose_params: **.broose.bucketSize / rBucketSize / userDist and **.brooseShiftingBits."""

    _fields_ = [("bucketSize", C.c_int32), ("rBucketSize", C.c_int32), ("userDist", C.c_int32),
                ("shiftingBits", C.c_int32)]

    @classmethod
    def default(cls, **kw) -> "BrooseParams":
        p = cls()
        lib().ovs_broose_params_default(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    def num_rows(self) -> int:
        """rows per node: rBucket[0 .. 2^shiftingBits - 1], lBucket, bBucket"""
        return int(lib().ovs_broose_num_rows(C.byref(self)))

    def row_cap(self, row: int) -> int:
        return int(lib().ovs_broose_row_cap(C.byref(self), row))


class PastryParams(C.Structure):
    """ovs_pastry_params: the **.pastry.* parameters a route over fixed tables reads (default.ini:226-245)."""

    _fields_ = [("bitsPerDigit", C.c_int32), ("numberOfLeaves", C.c_int32), ("numberOfNeighbors", C.c_int32),
                ("optimizeLookup", C.c_int32), ("useRegularNextHop", C.c_int32), ("routeMsgAcks", C.c_int32)]

    @classmethod
    def default(cls, **kw) -> "PastryParams":
        """default.ini's values.  routeMsgAcks = true among them runs through pastry_acked_lookup and pastry_rpc; the
        calls that send no acks (pastry_lookup, pastry_iterative_lookup, Scribe) take routeMsgAcks=0."""
        p = cls()
        lib().ovs_pastry_params_default(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    @classmethod
    def from_ini(cls, text: str, config: str | None = None, base: "PastryParams | None" = None) -> "PastryParams":
        p = cls.default()
        if base is not None:
            C.memmove(C.byref(p), C.byref(base), C.sizeof(cls))
        err = C.create_string_buffer(512)
        st = lib().ovs_pastry_params_from_ini(C.byref(p), text.encode(), config.encode() if config else None, err, 512)
        if st != 0:
            raise KbrError(f"ovs_pastry_params_from_ini: {STATUS.get(st, st)}: {err.value.decode()}")
        return p


class DhtParams(C.Structure):
    """ovs_dht_params: the **.tier1*.dht.* parameters (DHT.cc:65-70)."""

    _fields_ = [("numReplica", C.c_int32), ("numGetRequests", C.c_int32), ("ratioIdentical", C.c_double),
                ("secureMaintenance", C.c_int32), ("invalidDataAttack", C.c_int32), ("maintenanceAttack", C.c_int32),
                ("pad", C.c_int32)]

    @classmethod
    def default(cls) -> "DhtParams":
        p = cls()
        lib().ovs_dht_params_default(C.byref(p))
        return p

    @classmethod
    def from_ini(cls, ini_text: str, config: str | None = None, base: "DhtParams | None" = None):
        """(DhtParams, testTtl or None) from .ini text: the `**.tier1*.dht.*` keys and
        `**.tier2*.dhtTestApp.testTtl`, starting from `base` (default: the defaults)."""
        return cls._ini(lib().ovs_dht_params_from_ini, ini_text.encode(), config, base)

    @classmethod
    def from_ini_file(cls, path, config: str | None = None, base: "DhtParams | None" = None):
        return cls._ini(lib().ovs_dht_params_from_ini_file, str(path).encode(), config, base)

    @classmethod
    def _ini(cls, fn, arg, config, base):
        p = base.replace() if base is not None else cls.default()
        ttl = C.c_int32(-1)
        err = C.create_string_buffer(512)
        st = fn(C.byref(p), C.byref(ttl), arg, config.encode() if config else None, err, len(err))
        if st != 0:
            raise KbrError(f"ovs_dht_params_from_ini: {STATUS.get(st, st)}: {err.value.decode()}")
        return p, (ttl.value if ttl.value >= 0 else None)

    def replace(self, **kw) -> "DhtParams":
        q = DhtParams.from_buffer_copy(self)
        for k, v in kw.items():
            if not hasattr(q, k):
                raise AttributeError(k)
            setattr(q, k, v)
        return q

DHT_TEAMS_SYMMETRIC, DHT_TEAMS_REPEATED_HASHING = 0, 1


class DhtTeamParams(C.Structure):
    """ovs_dht_team_params: which replica-team DHT (SymmetricDHT.cc / RepeatedHashingDHT.cc) and numReplicaTeams."""

    _fields_ = [("mode", C.c_int32), ("numReplicaTeams", C.c_int32)]

    @classmethod
    def default(cls) -> "DhtTeamParams":
        p = cls()
        lib().ovs_dht_team_params_default(C.byref(p))
        return p

    @classmethod
    def symmetric(cls, teams: int) -> "DhtTeamParams":
        return cls(DHT_TEAMS_SYMMETRIC, teams)

    @classmethod
    def repeated_hashing(cls, teams: int) -> "DhtTeamParams":
        return cls(DHT_TEAMS_REPEATED_HASHING, teams)

    @classmethod
    def from_ini(cls, ini_text: str, config: str | None = None, base: "DhtTeamParams | None" = None) -> "DhtTeamParams":
        """From .ini text: the mode from `**.tier1Type`, the teams from `**.tier1*.dht.numReplicaTeams`."""
        return cls._ini(lib().ovs_dht_team_params_from_ini, ini_text.encode(), config, base)

    @classmethod
    def from_ini_file(cls, path, config: str | None = None, base: "DhtTeamParams | None" = None) -> "DhtTeamParams":
        return cls._ini(lib().ovs_dht_team_params_from_ini_file, str(path).encode(), config, base)

    @classmethod
    def _ini(cls, fn, arg, config, base):
        p = cls.from_buffer_copy(base) if base is not None else cls.default()
        err = C.create_string_buffer(512)
        st = fn(C.byref(p), arg, config.encode() if config else None, err, len(err))
        if st != 0:
            raise KbrError(f"ovs_dht_team_params_from_ini: {STATUS.get(st, st)}: {err.value.decode()}")
        return p

    def check(self, dp: "DhtParams") -> None:
        """The checks of initializeDHT (numReplica a multiple of the teams) and of the team calls' sizes."""
        err = C.create_string_buffer(512)
        st = lib().ovs_dht_team_params_check(C.byref(dp), C.byref(self), err, len(err))
        if st != 0:
            raise KbrError(f"ovs_dht_team_params_check: {STATUS.get(st, st)}: {err.value.decode()}")

    @staticmethod
    def offset(teams: int) -> int:
        """SymmetricDHT's overlayKeyOffset = OverlayKey::getMax() / numReplicaTeams."""
        w = (C.c_uint32 * 5)()
        if lib().ovs_dht_team_offset(int(teams), w) != 0:
            raise KbrError("ovs_dht_team_offset: numReplicaTeams outside 1..8")
        return sum(int(w[i]) << (32 * i) for i in range(5))


class StdDev(C.Structure):
    """ovs_stddev: one cStdDev summary (GlobalStatistics::addStdDev)."""

    _fields_ = [("count", C.c_uint64), ("mean", C.c_double), ("stddev", C.c_double),
                ("min", C.c_double), ("max", C.c_double)]


class KbrTestStats(C.Structure):
    """ovs_kbrtest_stats: KBRTestApp one-way statistics of a batch (KBRTestApp.cc:380-520)."""

    _fields_ = [
        ("num_sent", C.c_uint64), ("num_delivered", C.c_uint64), ("num_dropped", C.c_uint64),
        ("num_lookup_failed", C.c_uint64), ("bytes_sent", C.c_uint64), ("bytes_delivered", C.c_uint64),
        ("bytes_dropped", C.c_uint64), ("hop_count_sum", C.c_uint64), ("latency_sum_ns", C.c_int64),
        ("hop_count_min", C.c_uint32), ("hop_count_max", C.c_uint32),
        ("latency_min_ns", C.c_int64), ("latency_max_ns", C.c_int64),
        ("hop_count_mean", C.c_double), ("latency_mean_s", C.c_double),
        ("status_count", C.c_uint64 * 8), ("hop_hist", C.c_uint64 * 64),
        ("delivered_msgs_per_s", StdDev), ("delivered_bytes_per_s", StdDev),
        ("dropped_msgs_per_s", StdDev), ("dropped_bytes_per_s", StdDev), ("delivery_ratio", StdDev),
    ]

    STDDEV_NAMES = {
        "delivered_msgs_per_s": "KBRTestApp: One-way Delivered Messages/s",
        "delivered_bytes_per_s": "KBRTestApp: One-way Delivered Bytes/s",
        "dropped_msgs_per_s": "KBRTestApp: One-way Dropped Messages/s",
        "dropped_bytes_per_s": "KBRTestApp: One-way Dropped Bytes/s",
        "delivery_ratio": "KBRTestApp: One-way Delivery Ratio",
    }


class BcastStats(C.Structure):
    """ovs_bcast_stats: one broadcast (GlobalStatistics::bcastSearch and BroadcastTestApp's RECORD_STATS)."""

    _fields_ = [("expected", C.c_uint64), ("actual", C.c_uint64), ("expired", C.c_uint64),
                ("messages", C.c_uint64), ("bytes", C.c_uint64), ("last_arrival_ns", C.c_int64),
                ("hop_count", StdDev)]


_lib = None


def lib() -> C.CDLL:
    """Load libovs_kbr.so; raises if the HIP engine was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise ImportError(f"{_LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the MI355X engine has no CPU fallback)")
    # One HIP runtime per process: PyTorch ships its own libamdhip64 / libhsa-runtime64 (same
    # SONAMEs as /opt/rocm's).  Loaded after torch, the engine binds to torch's copies; loaded
    # before it, torch would map a second runtime and whichever initialises second finds no GPU
    # (tools/diag/runtime_order.py).  So torch, when installed, is imported first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(str(_LIB_PATH))
    L.ovs_build_id.argtypes = []
    L.ovs_build_id.restype = C.c_char_p
    if not os.environ.get("OVS_LIB"):
        # the library must be the build of the sources it ships with (oversim_amd/build.py)
        from .build import source_hash
        built, want = L.ovs_build_id().decode(), source_hash()
        if built != want:
            raise ImportError(f"{_LIB_PATH} is stale (build id {built}, sources {want}): rebuild with "
                              "`python -m oversim_amd.build`")
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32
    sigs = {
        "ovs_abi_version": ([], C.c_int),
        "ovs_params_default": ([i32, vp], None),
        "ovs_params_from_ini": ([vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int], C.c_int),
        "ovs_params_from_ini_file": ([vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int], C.c_int),
        "ovs_ctx_create": ([C.c_int, C.POINTER(vp)], C.c_int),
        "ovs_ctx_destroy": ([vp], None),
        "ovs_last_error": ([vp], C.c_char_p),
        "ovs_set_params": ([vp, vp], C.c_int),
        "ovs_get_params": ([vp, vp], C.c_int),
        "ovs_chord_load": ([vp, vp, u64, vp, u32], C.c_int),
        "ovs_chord_load_tables": ([vp, vp, u64, vp, vp, vp, vp, vp, vp, u32], C.c_int),
        "ovs_kad_load": ([vp, vp, u64, vp, u32], C.c_int),
        "ovs_koorde_load": ([vp, vp, u64, vp, u32], C.c_int),
        "ovs_koorde_export": ([vp, vp, vp, vp], C.c_int),
        "ovs_koorde_find_node_batch": ([vp, vp, vp, vp, vp, u64], C.c_int),
        "ovs_kad_load_tables": ([vp, vp, u64, vp, vp, vp, vp, u32], C.c_int),
        "ovs_kad_num_buckets": ([vp], i32),
        "ovs_kad_load_tables_csr": ([vp, vp, u64, vp, vp, vp, vp, u32], C.c_int),
        "ovs_kad_export_csr": ([vp, vp, vp, vp, u64, C.POINTER(u64)], C.c_int),
        "ovs_epichord_load": ([vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32], C.c_int),
        "ovs_epichord_find_node_batch": ([vp, vp, vp, vp, vp, u64, i32, vp, vp, u32, vp, vp, u32, vp], C.c_int),
        "ovs_kad_export": ([vp, vp, vp, vp], C.c_int),
        "ovs_chord_export_fingers": ([vp, vp], C.c_int),
        "ovs_route_batch": ([vp, vp, vp, u64, vp, vp, vp, u32, vp], C.c_int),
        "ovs_find_node_batch": ([vp, vp, vp, u64, i32, i32, vp, u32, vp, vp, u32, vp], C.c_int),
        "ovs_delay_batch": ([vp, vp, vp, vp, u64, vp, u32, vp], C.c_int),
        "ovs_sync": ([vp], C.c_int),
        "ovs_chord_broadcast_batch": ([vp, vp, u64, i32, i32, vp, vp, u32, vp], C.c_int),
        "ovs_pastry_broadcast_batch": ([vp, vp, u64, i32, i32, vp, vp, u32, vp], C.c_int),
        "ovs_kbrtest_stats_batch": ([vp, vp, vp, vp, u64, C.c_double, i32, vp, u32, vp], C.c_int),
        "ovs_chord_fix_fingers": ([vp, vp, u64, vp], C.c_int),
        "ovs_lookup_batch": ([vp, vp, vp, u64, i32, vp, vp, u32, vp], C.c_int),
        "ovs_chord_stabilize": ([vp, vp, u64, vp], C.c_int),
        "ovs_chord_export_tables": ([vp, vp, vp, vp], C.c_int),
        "ovs_kad_refresh_batch": ([vp, vp, vp, u64, i32, vp, vp, vp, vp, vp, u32, vp], C.c_int),
        "ovs_kad_refresh_keys": ([vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), u32, vp], C.c_int),
        "ovs_kad_maintenance_round": ([vp, vp, u64, vp, vp, vp], C.c_int),
        "ovs_kbrtest_lookup_stats_batch": ([vp, vp, vp, i32, vp, vp, u64, C.c_double, i32, C.c_double, vp, u32, vp],
                                           C.c_int),
        "ovs_rpc_batch": ([vp, vp, vp, u64, vp, u32, vp], C.c_int),
        "ovs_dht_params_default": ([vp], None),
        "ovs_dht_store_create": ([vp, u64], C.c_int),
        "ovs_dht_store_clear": ([vp], C.c_int),
        "ovs_dht_store_count": ([vp, vp, vp, vp], C.c_int),
        "ovs_dht_params_from_ini": ([vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int], C.c_int),
        "ovs_dht_params_from_ini_file": ([vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int], C.c_int),
        "ovs_dhttest_stats_batch": ([vp, vp, vp, u64, vp, vp, vp, vp, u64, C.c_double, vp, u32, vp], C.c_int),
        "ovs_dht_put_batch": ([vp, vp, vp, vp, vp, u64, vp, u32, vp], C.c_int),
        "ovs_dht_get_batch": ([vp, vp, vp, vp, vp, u64, vp, u32, vp], C.c_int),
        "ovs_dht_dump_node": ([vp, u32, C.c_int64, vp, u64, vp], C.c_int),
        "ovs_dht_team_params_default": ([vp], None),
        "ovs_dht_team_params_from_ini": ([vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int], C.c_int),
        "ovs_dht_team_params_from_ini_file": ([vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int], C.c_int),
        "ovs_dht_team_params_check": ([vp, vp, C.c_char_p, C.c_int], C.c_int),
        "ovs_dht_team_offset": ([C.c_int32, vp], C.c_int),
        "ovs_dht_team_keys": ([vp, vp, vp, u64, vp, u32, vp], C.c_int),
        "ovs_dht_team_put_batch": ([vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, u32, vp], C.c_int),
        "ovs_dht_team_get_batch": ([vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, u32, vp], C.c_int),
        "ovs_dhttest_team_stats_batch": ([vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, C.c_double, vp, u32, vp], C.c_int),
        "ovs_kbrtest_rpc_stats_batch": ([vp, vp, vp, vp, u64, C.c_double, i32, C.c_double, vp, u32, vp], C.c_int),
        "ovs_scribe_build": ([vp, vp, u64, vp, vp, u64, u64, u32, vp], C.c_int),
        "ovs_scribe_clear": ([vp], C.c_int),
        "ovs_scribe_count": ([vp, vp, vp, vp], C.c_int),
        "ovs_scribe_export": ([vp, vp, u32, vp], C.c_int),
        "ovs_scribe_multicast_batch": ([vp, vp, vp, vp, u64, i32, vp, vp, u64, vp, u32, vp], C.c_int),
        "ovs_broose_params_default": ([vp], None),
        "ovs_broose_num_rows": ([vp], i32),
        "ovs_broose_row_cap": ([vp, i32], i32),
        "ovs_broose_load": ([vp, vp, vp, u64, vp, u32], C.c_int),
        "ovs_broose_load_tables": ([vp, vp, vp, u64, vp, vp, vp, u32], C.c_int),
        "ovs_broose_export": ([vp, vp, vp, u64, C.POINTER(u64)], C.c_int),
        "ovs_broose_find_node_batch": ([vp, vp, vp, vp, vp, u64, i32, i32, vp, u32, vp, vp, vp], C.c_int),
        "ovs_broose_route_batch": ([vp, vp, vp, vp, u64, vp, vp, vp, u32, vp], C.c_int),
        "ovs_pastry_params_default": ([vp], None),
        "ovs_pastry_params_from_ini": ([vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int], C.c_int),
        "ovs_pastry_load": ([vp, vp, vp, u64, vp, u32], C.c_int),
        "ovs_pastry_num_rows": ([vp], i32),
        "ovs_pastry_load_tables": ([vp, vp, vp, u64, vp, vp, vp, i32, u32], C.c_int),
        "ovs_pastry_export": ([vp, vp, vp], C.c_int),
        "ovs_pastry_find_node_batch": ([vp, vp, vp, u64, i32, i32, vp, u32, vp, vp, vp], C.c_int),
        "ovs_pastry_route_batch": ([vp, vp, vp, u64, vp, vp, u32, vp], C.c_int),
        "ovs_pastry_lookup_batch": ([vp, vp, vp, u64, i32, vp, vp, vp, vp, u32, vp], C.c_int),
        "ovs_pastry_iterative_route_batch": ([vp, vp, vp, u64, vp, vp, u32, vp], C.c_int),
        "ovs_pastry_acked_route_batch": ([vp, vp, vp, u64, vp, vp, vp, u32, vp], C.c_int),
        "ovs_pastry_rpc_batch": ([vp, vp, vp, u64, vp, u32, vp], C.c_int),
    }
    for name, (args, res) in sigs.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def keys_array(keys) -> np.ndarray:
    """(n,5) uint32 little-endian 32-bit words, w[0] least significant."""
    a = np.ascontiguousarray(keys, dtype=np.uint32)
    if a.ndim != 2 or a.shape[1] != 5:
        raise ValueError("keys must have shape (n, 5) uint32")
    return a


def key_from_int(x: int) -> np.ndarray:
    x &= (1 << 160) - 1
    return np.array([(x >> (32 * i)) & 0xFFFFFFFF for i in range(5)], dtype=np.uint32)


def key_to_int(w) -> int:
    return sum(int(w[i]) << (32 * i) for i in range(5))


class FixFingersStats(C.Structure):
    """ovs_fixfingers_stats: one fixfingers round (ovs_chord_fix_fingers)."""

    _fields_ = [("lookups", C.c_uint64), ("ok", C.c_uint64), ("changed", C.c_uint64), ("hops", C.c_uint64)]


class StabilizeStats(C.Structure):
    """ovs_stabilize_stats: one stabilize round (ovs_chord_stabilize)."""

    _fields_ = [("nodes", C.c_uint64), ("succ_changed", C.c_uint64), ("lists_changed", C.c_uint64),
                ("pred_changed", C.c_uint64)]


class KadRoundStats(C.Structure):
    """ovs_kad_round_stats: one Kademlia maintenance round (ovs_kad_maintenance_round)."""

    _fields_ = [(f, C.c_uint64) for f in ("lookups", "failed", "responses", "sib_changes", "bucket_changes", "lost",
                                           "replacement", "refreshed")]


class KbrTestLookupStats(C.Structure):
    """ovs_kbrtest_lookup_stats: KBRTestApp lookup-test statistics of a batch (KBRTestApp.cc:331-371, 546-557)."""

    _fields_ = [
        ("num_sent", C.c_uint64), ("num_success", C.c_uint64), ("num_failed", C.c_uint64),
        ("num_invalid", C.c_uint64), ("hop_count_sum", C.c_uint64), ("failed_hop_count_sum", C.c_uint64),
        ("success_latency_sum_ns", C.c_int64), ("hop_count_min", C.c_uint32), ("hop_count_max", C.c_uint32),
        ("success_latency_min_ns", C.c_int64), ("success_latency_max_ns", C.c_int64),
        ("hop_count_mean", C.c_double), ("failed_hop_count_mean", C.c_double),
        ("success_latency_mean_s", C.c_double), ("total_latency_mean_s", C.c_double),
        ("status_count", C.c_uint64 * 8), ("hop_hist", C.c_uint64 * 64),
        ("successful_lookups_per_s", StdDev), ("failed_lookups_per_s", StdDev), ("success_ratio", StdDev),
    ]

    STDDEV_NAMES = {
        "successful_lookups_per_s": "KBRTestApp: Successful Lookups/s",
        "failed_lookups_per_s": "KBRTestApp: Failed Lookups/s",
        "success_ratio": "KBRTestApp: Lookup Success Ratio",
    }


class KbrTestRpcStats(C.Structure):
    """ovs_kbrtest_rpc_stats: KBRTestApp RPC-test statistics of a batch (KBRTestApp.cc:251-314, 519-545)."""

    _fields_ = [
        ("num_sent", C.c_uint64), ("num_delivered", C.c_uint64), ("num_dropped", C.c_uint64),
        ("num_timeout", C.c_uint64), ("bytes_sent", C.c_uint64), ("bytes_delivered", C.c_uint64),
        ("bytes_dropped", C.c_uint64), ("hop_count_sum", C.c_uint64), ("success_latency_sum_ns", C.c_int64),
        ("hop_count_min", C.c_uint32), ("hop_count_max", C.c_uint32),
        ("success_latency_min_ns", C.c_int64), ("success_latency_max_ns", C.c_int64),
        ("hop_count_mean", C.c_double), ("success_latency_mean_s", C.c_double), ("total_latency_mean_s", C.c_double),
        ("status_count", C.c_uint64 * 8), ("hop_hist", C.c_uint64 * 64),
        ("delivered_msgs_per_s", StdDev), ("delivered_bytes_per_s", StdDev),
        ("dropped_msgs_per_s", StdDev), ("dropped_bytes_per_s", StdDev), ("delivery_ratio", StdDev),
    ]

    STDDEV_NAMES = {
        "delivered_msgs_per_s": "KBRTestApp: RPC Delivered Messages/s",
        "delivered_bytes_per_s": "KBRTestApp: RPC Delivered Bytes/s",
        "dropped_msgs_per_s": "KBRTestApp: RPC Dropped Messages/s",
        "dropped_bytes_per_s": "KBRTestApp: RPC Dropped Bytes/s",
        "delivery_ratio": "KBRTestApp: RPC Delivery Ratio",
    }


class DhtTestStats(C.Structure):
    """ovs_dhttest_stats: DHTTestApp statistics of a put and a get batch (DHTTestApp.cc:147-234, 439-467)."""

    _fields_ = [
        ("num_put_success", C.c_uint64), ("num_put_error", C.c_uint64), ("num_get_success", C.c_uint64),
        ("num_get_error", C.c_uint64), ("put_latency_sum_ns", C.c_uint64), ("put_latency_sumsq_lo", C.c_uint64),
        ("put_latency_sumsq_hi", C.c_uint64), ("get_latency_sum_ns", C.c_uint64), ("get_latency_sumsq_lo", C.c_uint64),
        ("get_latency_sumsq_hi", C.c_uint64), ("put_latency_min_ns", C.c_int64), ("put_latency_max_ns", C.c_int64),
        ("get_latency_min_ns", C.c_int64), ("get_latency_max_ns", C.c_int64), ("get_latency_count", C.c_uint64),
        ("put_hop_count", C.c_uint64), ("put_hop_sum", C.c_uint64), ("get_hop_count", C.c_uint64),
        ("get_hop_sum", C.c_uint64), ("normal_messages", C.c_uint64), ("num_bytes_normal", C.c_uint64),
        ("put_latency_s", StdDev), ("get_latency_s", StdDev), ("put_success_per_s", StdDev),
        ("put_error_per_s", StdDev), ("get_success_per_s", StdDev), ("get_error_per_s", StdDev),
        ("get_success_ratio", StdDev),
    ]

    STDDEV_NAMES = {
        "put_latency_s": "DHTTestApp: PUT Latency (s)", "get_latency_s": "DHTTestApp: GET Latency (s)",
        "put_success_per_s": "DHTTestApp: Successful PUT Requests/s", "put_error_per_s": "DHTTestApp: Failed PUT Requests/s",
        "get_success_per_s": "DHTTestApp: Successful GET Requests/s", "get_error_per_s": "DHTTestApp: Failed GET Requests/s",
        "get_success_ratio": "DHTTestApp: GET Success Ratio",
    }


def bcast_stats_dict(st: BcastStats) -> dict:
    d = {f: getattr(st, f) for f, _ in BcastStats._fields_ if f != "hop_count"}
    d["hop_count"] = {f: getattr(st.hop_count, f) for f, _ in StdDev._fields_}
    return d


class KbrEngine:
    """One engine context per HIP device (ovs_ctx)."""

    def __init__(self, device: int = 0, params: Params | None = None):
        self._L = lib()
        h = C.c_void_p()
        st = self._L.ovs_ctx_create(device, C.byref(h))
        if st != 0:
            raise KbrError(f"ovs_ctx_create(device={device}) failed: {STATUS.get(st, st)}")
        self._h = h
        self.n = 0
        self.overlay = 0
        if params is not None:
            self.set_params(params)

    # -- plumbing
    def _chk(self, st: int, what: str):
        if st != 0:
            msg = self._L.ovs_last_error(self._h)
            raise KbrError(f"{what}: {STATUS.get(st, st)}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.ovs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self) -> int:
        return self._h.value

    # -- parameters
    def set_params(self, p: Params):
        self._chk(self._L.ovs_set_params(self._h, C.byref(p)), "ovs_set_params")

    def get_params(self) -> Params:
        p = Params()
        self._chk(self._L.ovs_get_params(self._h, C.byref(p)), "ovs_get_params")
        return p

    # -- networks
    def chord_load(self, ids, xy):
        ids = keys_array(ids)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        self._chk(self._L.ovs_chord_load(self._h, _ptr(ids), len(ids), _ptr(xy), 0), "ovs_chord_load")
        self.n, self.overlay = len(ids), OVERLAY_CHORD

    def chord_load_device(self, ids_ptr: int, xy_ptr: int, n: int):
        """Load a Chord ring whose sorted ids / coordinates already live on this device."""
        self._chk(self._L.ovs_chord_load(self._h, C.c_void_p(ids_ptr), n, C.c_void_p(xy_ptr), DEVICE_PTRS),
                  "ovs_chord_load")
        self.n, self.overlay = n, OVERLAY_CHORD

    def koorde_load(self, ids, xy):
        """Converged Koorde ring (ovs_koorde_load); params.overlay must be OVERLAY_KOORDE."""
        ids = keys_array(ids)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        self._chk(self._L.ovs_koorde_load(self._h, _ptr(ids), len(ids), _ptr(xy), 0), "ovs_koorde_load")
        self.n, self.overlay = len(ids), OVERLAY_KOORDE

    def koorde_load_device(self, ids_ptr: int, xy_ptr: int, n: int):
        self._chk(self._L.ovs_koorde_load(self._h, C.c_void_p(ids_ptr), n, C.c_void_p(xy_ptr), DEVICE_PTRS),
                  "ovs_koorde_load")
        self.n, self.overlay = n, OVERLAY_KOORDE

    def koorde_state(self):
        """(deBruijnNode, first node of the deBruijnNodes list, list length) per node."""
        db = np.empty(self.n, dtype=np.uint32)
        start = np.empty(self.n, dtype=np.uint32)
        num = np.empty(self.n, dtype=np.uint8)
        self._chk(self._L.ovs_koorde_export(self._h, _ptr(db), _ptr(start), _ptr(num)), "ovs_koorde_export")
        return db, start, num

    def koorde_find_node(self, node, keys, ext=None):
        """Koorde::findNode at node[i] for keys[i]; ext = KOORDE_EXT_DTYPE records (None: fresh,
        unspecified route key, step 1) are advanced in place.  Returns (next hop, NONE where the
        reference throws; the extensions the responses carry)."""
        node = np.ascontiguousarray(node, dtype=np.uint32)
        keys = keys_array(keys)
        n = len(node)
        if ext is None:
            ext = np.zeros(n, dtype=KOORDE_EXT_DTYPE)
            ext["step"] = 1
        ext = np.ascontiguousarray(ext, dtype=KOORDE_EXT_DTYPE).copy()
        nxt = np.empty(n, dtype=np.uint32)
        self._chk(self._L.ovs_koorde_find_node_batch(self._h, _ptr(node), _ptr(keys), _ptr(ext), _ptr(nxt), n),
                  "ovs_koorde_find_node_batch")
        return nxt, ext

    # -- Broose
    def broose_load(self, ids, xy, bp: "BrooseParams | None" = None):
        """The ideal Broose snapshot (ovs_broose_load): every bucket holds the nodes XOR-closest to its key.
        params.overlay must be OVERLAY_BROOSE."""
        ids = keys_array(ids)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        bp = bp if bp is not None else BrooseParams.default()
        self._chk(self._L.ovs_broose_load(self._h, C.byref(bp), _ptr(ids), len(ids), _ptr(xy), 0), "ovs_broose_load")
        self._bp, self.n, self.overlay = bp, len(ids), OVERLAY_BROOSE      # a refused load leaves the loaded shape

    def broose_load_device(self, ids_ptr: int, xy_ptr: int, n: int, bp: "BrooseParams | None" = None):
        bp = bp if bp is not None else BrooseParams.default()
        self._chk(self._L.ovs_broose_load(self._h, C.byref(bp), C.c_void_p(ids_ptr), n, C.c_void_p(xy_ptr),
                                          DEVICE_PTRS), "ovs_broose_load")
        self._bp, self.n, self.overlay = bp, n, OVERLAY_BROOSE

    def broose_load_tables(self, ids, xy, row_off, row_nodes, bp: "BrooseParams | None" = None):
        """Explicit Broose buckets in CSR form (ovs_broose_load_tables): row r of node v =
        row_nodes[row_off[v * rows + r] : row_off[v * rows + r + 1]], closest to the bucket key first."""
        ids = keys_array(ids)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        off = np.ascontiguousarray(row_off, dtype=np.uint64)
        nd = np.ascontiguousarray(row_nodes, dtype=np.uint32)
        bp = bp if bp is not None else BrooseParams.default()
        if len(off) != len(ids) * bp.num_rows() + 1:
            raise ValueError("row_off must have n * rows + 1 entries")
        if len(nd) < int(off[-1]):
            raise ValueError("row_nodes is shorter than row_off[-1]")
        self._chk(self._L.ovs_broose_load_tables(self._h, C.byref(bp), _ptr(ids), len(ids), _ptr(xy), _ptr(off),
                                                 _ptr(nd) if len(nd) else None, 0), "ovs_broose_load_tables")
        self._bp, self.n, self.overlay = bp, len(ids), OVERLAY_BROOSE

    def broose_export(self):
        """(row_off (n * rows + 1), row_nodes) of the loaded Broose buckets."""
        off = np.empty(self.n * self._bp.num_rows() + 1, dtype=np.uint64)
        tot = C.c_uint64(0)
        self._chk(self._L.ovs_broose_export(self._h, _ptr(off), None, 0, C.byref(tot)), "ovs_broose_export")
        nodes = np.empty(max(int(tot.value), 1), dtype=np.uint32)
        self._chk(self._L.ovs_broose_export(self._h, _ptr(off), _ptr(nodes), len(nodes), C.byref(tot)), "ovs_broose_export")
        return off, nodes[:int(tot.value)]

    def broose_find_node(self, node, keys, right, ext=None, numRedundantNodes: int = 1, numSiblings: int = 1,
                         max_out: int | None = None):
        """Broose::findNode at node[i] for keys[i] (ovs_broose_find_node_batch).  ext = BROOSE_EXT_DTYPE records
        (None: calls without an extension); right[i] = the direction of an extension created in call i.
        Returns (nodes (n, max_out) NONE padded, count, sibling flag, status (1 = the reference errors),
        the extensions the responses carry)."""
        node = np.ascontiguousarray(node, dtype=np.uint32)
        keys = keys_array(keys)
        n = len(node)
        right = np.ascontiguousarray(np.broadcast_to(right, (n,)), dtype=np.uint8)
        ext = np.zeros(n, dtype=BROOSE_EXT_DTYPE) if ext is None else np.ascontiguousarray(ext, dtype=BROOSE_EXT_DTYPE).copy()
        mo = max_out or max(numRedundantNodes, numSiblings, 1)
        out = np.empty((n, mo), dtype=np.uint32)
        cnt = np.empty(n, dtype=np.uint8)
        sib = np.empty(n, dtype=np.uint8)
        st = np.empty(n, dtype=np.uint8)
        self._chk(self._L.ovs_broose_find_node_batch(self._h, _ptr(node), _ptr(keys), _ptr(ext), _ptr(right), n,
                                                     numRedundantNodes, numSiblings, _ptr(out), mo, _ptr(cnt), _ptr(sib),
                                                     _ptr(st)), "ovs_broose_find_node_batch")
        return out, cnt, sib, st, ext

    def broose_directions(self, keys, src, parity=None):
        """The per-lookup direction flags Broose's chooseLookup++ (Broose.cc:643) gives a batch that runs in
        order: a lookup turns right iff its source created an odd number of extensions before it, and a
        lookup creates one unless its source is a sibling of its key.  parity: chooseLookup per node before
        the batch (None: 0).  Returns (right flags uint8, chooseLookup per node after the batch)."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        par = np.zeros(self.n, dtype=np.int64) if parity is None else np.array(parity, dtype=np.int64)
        if len(src) == 0:
            return np.zeros(0, dtype=np.uint8), par
        _, _, sib, _, _ = self.broose_find_node(src, keys, 0)
        creates = (sib == 0).astype(np.int64)
        order = np.argsort(src, kind="stable")
        s, cr = src[order], creates[order]
        csum = np.cumsum(cr) - cr                           # extensions created before, over the sorted batch
        first = np.r_[0, np.flatnonzero(s[1:] != s[:-1]) + 1]
        before = csum - np.repeat(csum[first], np.diff(np.r_[first, len(s)]))
        right = np.empty(len(src), dtype=np.uint8)
        right[order] = ((par[s] + before) % 2).astype(np.uint8)
        np.add.at(par, src, creates)
        return right, par

    def broose_lookup(self, keys, src, right, record_hops: bool = False, count_rpcs: bool = False) -> dict:
        """Batched KBRTestApp one-way lookups on a Broose context (ovs_broose_route_batch); right[i] = lookup
        i's direction flag (broose_directions).  Returns numpy arrays by field, as lookup()."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        n = len(keys)
        if len(src) != n:
            raise ValueError("keys and src differ in length")
        right = np.ascontiguousarray(np.broadcast_to(right, (n,)), dtype=np.uint8)
        out = np.empty(n, dtype=ROUTE_OUT_DTYPE)
        H = max(self.get_params().hopCountMax, 1)
        hop = np.empty((n, H), dtype=np.uint32) if record_hops else None
        rpcs = np.empty(n, dtype=np.uint32) if count_rpcs else None
        self._chk(self._L.ovs_broose_route_batch(self._h, _ptr(keys), _ptr(src), _ptr(right), n, _ptr(out), _ptr(hop),
                                                 _ptr(rpcs), 0, None), "ovs_broose_route_batch")
        res = {f: out[f].copy() for f in ROUTE_OUT_DTYPE.names}
        if hop is not None:
            res["hop_seq"] = hop
        if rpcs is not None:
            res["rpcs"] = rpcs
        return res

    def broose_lookup_device(self, keys_ptr: int, src_ptr: int, right_ptr: int, n: int, out_ptr: int,
                             stream: int | None = None, rpcs_ptr: int | None = None):
        """Device-resident batch (async on `stream`)."""
        self._chk(self._L.ovs_broose_route_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), C.c_void_p(right_ptr), n,
                                                 C.c_void_p(out_ptr), None, C.c_void_p(rpcs_ptr) if rpcs_ptr else None,
                                                 DEVICE_PTRS, C.c_void_p(stream) if stream else None),
                  "ovs_broose_route_batch")

    # -- Pastry
    def pastry_load(self, ids, xy, pp: "PastryParams | None" = None):
        """The converged Pastry tables (ovs_pastry_load), built on the device by the rule of DESIGN.md §4.
        params.overlay must be OVERLAY_PASTRY."""
        ids = keys_array(ids)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        self._pp = pp if pp is not None else PastryParams.default(routeMsgAcks=0)
        self._chk(self._L.ovs_pastry_load(self._h, C.byref(self._pp), _ptr(ids), len(ids), _ptr(xy), 0), "ovs_pastry_load")
        self.n, self.overlay = len(ids), OVERLAY_PASTRY

    def pastry_load_device(self, ids_ptr: int, xy_ptr: int, n: int, pp: "PastryParams | None" = None):
        self._pp = pp if pp is not None else PastryParams.default(routeMsgAcks=0)
        self._chk(self._L.ovs_pastry_load(self._h, C.byref(self._pp), C.c_void_p(ids_ptr), n, C.c_void_p(xy_ptr),
                                          DEVICE_PTRS), "ovs_pastry_load")
        self.n, self.overlay = n, OVERLAY_PASTRY

    def pastry_load_tables(self, ids, xy, leaf, table, pp: "PastryParams | None" = None):
        """Explicit Pastry tables as node indices, NONE = unspecified (ovs_pastry_load_tables): leaf (n, L) in
        the reference's slot order, table (n, rows, 2^bitsPerDigit)."""
        ids = keys_array(ids)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        leaf = np.ascontiguousarray(leaf, dtype=np.uint32)
        table = np.ascontiguousarray(table, dtype=np.uint32)
        pp = pp if pp is not None else PastryParams.default(routeMsgAcks=0)
        n = len(ids)
        if leaf.shape != (n, pp.numberOfLeaves):
            raise ValueError("leaf must be (n, numberOfLeaves)")
        if table.ndim != 3 or table.shape[0] != n or table.shape[2] != 1 << pp.bitsPerDigit:
            raise ValueError("table must be (n, rows, 2^bitsPerDigit)")
        self._chk(self._L.ovs_pastry_load_tables(self._h, C.byref(pp), _ptr(ids), n, _ptr(xy), _ptr(leaf), _ptr(table),
                                                 table.shape[1], 0), "ovs_pastry_load_tables")
        self._pp = pp
        self.n, self.overlay = n, OVERLAY_PASTRY

    def pastry_export(self):
        """(leaf (n, L), table (n, rows, 2^bitsPerDigit)) of the loaded Pastry tables, NONE = unspecified."""
        rows = int(self._L.ovs_pastry_num_rows(self._h))
        if rows < 0:
            raise KbrError("ovs_pastry_export: ESTATE: no Pastry network loaded")
        leaf = np.empty((self.n, self._pp.numberOfLeaves), dtype=np.uint32)
        table = np.empty((self.n, rows, 1 << self._pp.bitsPerDigit), dtype=np.uint32)
        self._chk(self._L.ovs_pastry_export(self._h, _ptr(leaf), _ptr(table)), "ovs_pastry_export")
        return leaf, table

    def pastry_find_node(self, node, keys, numRedundantNodes: int = 1, numSiblings: int = 1, max_out: int | None = None):
        """BasePastry::findNode at node[i] for keys[i] (ovs_pastry_find_node_batch).  Returns (nodes (n, max_out)
        NONE padded, count, sibling flag, status: bit 0 isSiblingFor's err, bit 1 the reference throws)."""
        node = np.ascontiguousarray(node, dtype=np.uint32)
        keys = keys_array(keys)
        n = len(node)
        mo = max_out or max(numRedundantNodes + 1, numSiblings, 1)
        out = np.empty((n, mo), dtype=np.uint32)
        cnt = np.empty(n, dtype=np.uint8)
        sib = np.empty(n, dtype=np.uint8)
        st = np.empty(n, dtype=np.uint8)
        self._chk(self._L.ovs_pastry_find_node_batch(self._h, _ptr(node), _ptr(keys), n, numRedundantNodes, numSiblings,
                                                     _ptr(out), mo, _ptr(cnt), _ptr(sib), _ptr(st)),
                  "ovs_pastry_find_node_batch")
        return out, cnt, sib, st

    def _pastry_one_way(self, name: str, takes: tuple, keys, src, record_hops: bool = False, ack_records: bool = False,
                        out_dtype=ROUTE_OUT_DTYPE) -> dict:
        """What the Pastry one-way wrappers share: keys and src as arrays of one length, the out records, the
        optional ack records and hop rows, the call `name`, which takes the buffers `takes` names in that order,
        and the records unpacked by field."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        n = len(keys)
        if len(src) != n:
            raise ValueError("keys and src differ in length")
        out = np.empty(n, dtype=out_dtype)
        ack = np.empty(n, dtype=PASTRY_ACK_OUT_DTYPE) if ack_records else None
        hop = np.empty((n, max(self.get_params().hopCountMax, 1)), dtype=np.uint32) if record_hops else None
        bufs = {"out": out, "ack": ack, "hop": hop}
        self._chk(getattr(self._L, name)(self._h, _ptr(keys), _ptr(src), n, *(_ptr(bufs[b]) for b in takes), 0, None), name)
        res = {f: out[f].copy() for f in out_dtype.names}
        if ack is not None:
            res.update({f: ack[f].copy() for f in PASTRY_ACK_OUT_DTYPE.names})
        if hop is not None:
            res["hop_seq"] = hop
        return res

    def pastry_lookup(self, keys, src, record_hops: bool = False) -> dict:
        """Batched semi-recursive one-way routes on a Pastry context (ovs_pastry_route_batch).  Returns numpy
        arrays by field, as lookup()."""
        return self._pastry_one_way("ovs_pastry_route_batch", ("out", "hop"), keys, src, record_hops)

    def pastry_lookup_device(self, keys_ptr: int, src_ptr: int, n: int, out_ptr: int, stream: int | None = None):
        """Device-resident batch (async on `stream`)."""
        self._chk(self._L.ovs_pastry_route_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n, C.c_void_p(out_ptr),
                                                 None, DEVICE_PTRS, C.c_void_p(stream) if stream else None),
                  "ovs_pastry_route_batch")

    def pastry_lookup_call(self, keys, src, num_siblings: int = 1, record_hops: bool = False) -> dict:
        """Batched iterative LookupCalls on a Pastry context (ovs_pastry_lookup_batch; params.routingType = 0).
        num_siblings = -1 is getMaxNumSiblings() = numberOfLeaves / 2.  Returns num_siblings, hops, status,
        is_valid, latency_ns and rpcs per lookup and `siblings` (n, num_siblings), NONE padded; with record_hops
        the responders in order as hop_seq (n, hopCountMax)."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        n = len(keys)
        if len(src) != n:
            raise ValueError("keys and src differ in length")
        ns = num_siblings if num_siblings >= 0 else self._pp.numberOfLeaves // 2
        out = np.empty(n, dtype=LOOKUP_OUT_DTYPE)
        sib = np.empty((n, max(ns, 1)), dtype=np.uint32)
        hop = np.empty((n, max(self.get_params().hopCountMax, 1)), dtype=np.uint32) if record_hops else None
        rpcs = np.empty(n, dtype=np.uint32)
        self._chk(self._L.ovs_pastry_lookup_batch(self._h, _ptr(keys), _ptr(src), n, num_siblings, _ptr(out), _ptr(sib),
                                                  _ptr(hop), _ptr(rpcs), 0, None), "ovs_pastry_lookup_batch")
        res = {f: out[f].copy() for f in LOOKUP_OUT_DTYPE.names}
        res["siblings"] = sib
        res["rpcs"] = rpcs
        if hop is not None:
            res["hop_seq"] = hop
        return res

    def pastry_lookup_call_device(self, keys_ptr: int, src_ptr: int, n: int, num_siblings: int, out_ptr: int,
                                  siblings_ptr: int, stream: int | None = None, rpcs_ptr: int | None = None):
        """Device-resident batch (async on `stream`): out n ovs_lookup_out, siblings n * num_siblings uint32."""
        self._chk(self._L.ovs_pastry_lookup_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n, num_siblings,
                                                  C.c_void_p(out_ptr), C.c_void_p(siblings_ptr), None,
                                                  C.c_void_p(rpcs_ptr) if rpcs_ptr else None, DEVICE_PTRS,
                                                  C.c_void_p(stream) if stream else None), "ovs_pastry_lookup_batch")

    def pastry_iterative_lookup(self, keys, src, record_hops: bool = False) -> dict:
        """Batched KBRTestApp one-way routes under iterative routing on a Pastry context
        (ovs_pastry_iterative_route_batch; params.routingType = 0).  Returns numpy arrays by field, as lookup()."""
        return self._pastry_one_way("ovs_pastry_iterative_route_batch", ("out", "hop"), keys, src, record_hops)

    def pastry_iterative_lookup_device(self, keys_ptr: int, src_ptr: int, n: int, out_ptr: int, stream: int | None = None):
        """Device-resident batch (async on `stream`)."""
        self._chk(self._L.ovs_pastry_iterative_route_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n,
                                                           C.c_void_p(out_ptr), None, DEVICE_PTRS,
                                                           C.c_void_p(stream) if stream else None),
                  "ovs_pastry_iterative_route_batch")

    def pastry_acked_lookup(self, keys, src, record_hops: bool = False, ack_records: bool = True) -> dict:
        """Batched KBRTestApp one-way routes on a Pastry context under its routeMsgAcks
        (ovs_pastry_acked_route_batch): semi-recursive, or with params.routingType = 0 the iterative lookup whose
        final message goes as one NextHopCall.  Returns the route fields as lookup() and, per route, acks (the
        NextHopCalls sent), max_ack_rtt_ns (-1 without one) and timeout_hop (the first hop whose ack round trip
        reached rpcUdpTimeout, 0xFF = none); ack_records=False passes no ack buffer."""
        return self._pastry_one_way("ovs_pastry_acked_route_batch", ("out", "ack", "hop"), keys, src, record_hops, ack_records)

    def pastry_acked_lookup_device(self, keys_ptr: int, src_ptr: int, n: int, out_ptr: int, ack_out_ptr: int | None = None,
                                   stream: int | None = None):
        """Device-resident batch (async on `stream`): out n ovs_route_out, ack_out n ovs_pastry_ack_out or None."""
        self._chk(self._L.ovs_pastry_acked_route_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n,
                                                       C.c_void_p(out_ptr), C.c_void_p(ack_out_ptr) if ack_out_ptr else None,
                                                       None, DEVICE_PTRS, C.c_void_p(stream) if stream else None),
                  "ovs_pastry_acked_route_batch")

    def pastry_rpc(self, keys, src) -> dict:
        """Batched routed KbrTestCall round trips on a Pastry context (ovs_pastry_rpc_batch; KBRTestApp with
        kbrRpcTest, semi-recursive routing, either routeMsgAcks).  Returns the ovs_rpc_out fields as rpcCall()."""
        return self._pastry_one_way("ovs_pastry_rpc_batch", ("out",), keys, src, out_dtype=RPC_OUT_DTYPE)

    def pastry_rpc_device(self, keys_ptr: int, src_ptr: int, n: int, out_ptr: int, stream: int | None = None):
        """Device-resident RPC batch (async on `stream`): out n ovs_rpc_out."""
        self._chk(self._L.ovs_pastry_rpc_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n, C.c_void_p(out_ptr),
                                               DEVICE_PTRS, C.c_void_p(stream) if stream else None), "ovs_pastry_rpc_batch")

    def epichord_load(self, ids, xy, succ, nsucc, pred, npred, lists_full, cache_off, cache_node, cache_last_ns,
                      cache_ttl_ns):
        """One EpiChord routing snapshot (ovs_epichord_load): successor / predecessor lists (n, L) closest
        first with their lengths and isFull() bits, the live finger caches as CSR rows (node, lastUpdate,
        ttl in ns).  params.overlay must be OVERLAY_EPICHORD."""
        ids = keys_array(ids)
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((xy, np.float64), (succ, np.uint32), (nsucc, np.uint8), (pred, np.uint32), (npred, np.uint8),
                 (lists_full, np.uint8), (cache_off, np.uint64), (cache_node, np.uint32),
                 (cache_last_ns, np.int64), (cache_ttl_ns, np.int64))]
        self._chk(self._L.ovs_epichord_load(self._h, _ptr(ids), len(ids), *[_ptr(a) for a in arrs], 0),
                  "ovs_epichord_load")
        self.n, self.overlay = len(ids), OVERLAY_EPICHORD

    def epichord_find_node(self, node, keys, src, now_ns, numRedundantNodes: int, max_out: int | None = None):
        """EpiChord::findNode per call (ovs_epichord_find_node_batch): src NONE = a local call.  Returns
        (nodes (n, max_out), lastUpdates (n, max_out), count, status)."""
        node = np.ascontiguousarray(node, dtype=np.uint32)
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        now = np.ascontiguousarray(now_ns, dtype=np.int64)
        n = len(node)
        mo = max_out or max(3, 1 + numRedundantNodes)
        out = np.empty((n, mo), dtype=np.uint32)
        last = np.empty((n, mo), dtype=np.int64)
        cnt = np.empty(n, dtype=np.uint8)
        st = np.empty(n, dtype=np.uint8)
        self._chk(self._L.ovs_epichord_find_node_batch(self._h, _ptr(node), _ptr(keys), _ptr(src), _ptr(now), n,
                                                       numRedundantNodes, _ptr(out), _ptr(last), mo, _ptr(cnt),
                                                       _ptr(st), 0, None), "ovs_epichord_find_node_batch")
        return out, last, cnt, st

    def kad_load_device(self, ids_ptr: int, xy_ptr: int, n: int):
        self._chk(self._L.ovs_kad_load(self._h, C.c_void_p(ids_ptr), n, C.c_void_p(xy_ptr), DEVICE_PTRS),
                  "ovs_kad_load")
        self.n, self.overlay = n, OVERLAY_KADEMLIA

    def chord_load_tables(self, ids, xy, pred, succ, nsucc, fingers, deque_size):
        ids = keys_array(ids)
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((xy, np.float64), (pred, np.uint32), (succ, np.uint32), (nsucc, np.uint8),
                 (fingers, np.uint32), (deque_size, np.uint8))]
        self._chk(self._L.ovs_chord_load_tables(self._h, _ptr(ids), len(ids), *[_ptr(a) for a in arrs], 0),
                  "ovs_chord_load_tables")
        self.n, self.overlay = len(ids), OVERLAY_CHORD

    def kad_load(self, ids, xy):
        ids = keys_array(ids)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        self._chk(self._L.ovs_kad_load(self._h, _ptr(ids), len(ids), _ptr(xy), 0), "ovs_kad_load")
        self.n, self.overlay = len(ids), OVERLAY_KADEMLIA

    def kad_load_tables(self, ids, xy, siblings, bucket_count, bucket_nodes):
        """Explicit Kademlia tables (ovs_kad_load_tables): siblings (n, 5s), bucket_count (n, 160),
        bucket_nodes (n, 160, k), 0xFFFFFFFF padded -- the k-buckets a running OverSim node holds."""
        ids = keys_array(ids)
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((xy, np.float64), (siblings, np.uint32), (bucket_count, np.uint8), (bucket_nodes, np.uint32))]
        self._chk(self._L.ovs_kad_load_tables(self._h, _ptr(ids), len(ids), *[_ptr(a) for a in arrs], 0),
                  "ovs_kad_load_tables")
        self.n, self.overlay = len(ids), OVERLAY_KADEMLIA

    def kad_load_tables_csr(self, ids, xy, siblings, bucket_off, bucket_nodes):
        """Kademlia tables in CSR form (ovs_kad_load_tables_csr): any b / bucketType of the current
        params -- siblings (n, 5s), bucket_off (n * numBuckets + 1) uint64, bucket_nodes (LRU order)."""
        ids = keys_array(ids)
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in
                ((xy, np.float64), (siblings, np.uint32), (bucket_off, np.uint64), (bucket_nodes, np.uint32))]
        self._chk(self._L.ovs_kad_load_tables_csr(self._h, _ptr(ids), len(ids), *[_ptr(a) for a in arrs], 0),
                  "ovs_kad_load_tables_csr")
        self.n, self.overlay = len(ids), OVERLAY_KADEMLIA

    def kad_num_buckets(self) -> int:
        p = self.get_params()
        return int(self._L.ovs_kad_num_buckets(C.byref(p)))

    def kad_tables_csr(self):
        """(siblings (n, 5s), bucket_off (n * numBuckets + 1), bucket_nodes) of the loaded tables."""
        p = self.get_params()
        nb = self.kad_num_buckets()
        sib = np.empty((self.n, 5 * p.s), dtype=np.uint32)
        off = np.empty(self.n * nb + 1, dtype=np.uint64)
        tot = C.c_uint64(0)
        self._chk(self._L.ovs_kad_export_csr(self._h, _ptr(sib), _ptr(off), None, 0, C.byref(tot)), "ovs_kad_export_csr")
        nodes = np.empty(max(int(tot.value), 1), dtype=np.uint32)
        self._chk(self._L.ovs_kad_export_csr(self._h, _ptr(sib), _ptr(off), _ptr(nodes), len(nodes), C.byref(tot)),
                  "ovs_kad_export_csr")
        return sib, off, nodes[:int(tot.value)]

    def chord_fingers(self) -> np.ndarray:
        out = np.empty((self.n, 160), dtype=np.uint32)
        self._chk(self._L.ovs_chord_export_fingers(self._h, _ptr(out)), "ovs_chord_export_fingers")
        return out

    def chord_fix_fingers(self, nodes=None) -> dict:
        """One synchronous fixfingers round on an explicit-table ring (ovs_chord_fix_fingers):
        the batched maintenance lookups of Chord::handleFixFingersTimerExpired."""
        nodes = np.arange(self.n, dtype=np.uint32) if nodes is None else np.ascontiguousarray(nodes, np.uint32)
        st = FixFingersStats()
        self._chk(self._L.ovs_chord_fix_fingers(self._h, _ptr(nodes), len(nodes), C.cast(C.byref(st), C.c_void_p)),
                  "ovs_chord_fix_fingers")
        return {f: getattr(st, f) for f, _ in FixFingersStats._fields_}

    def chord_stabilize(self, nodes=None) -> dict:
        """One synchronous stabilize round on an explicit-table ring (ovs_chord_stabilize): successor's
        predecessor, notify, successor-list update (Chord.cc:793-842, 1055-1225)."""
        nodes = np.arange(self.n, dtype=np.uint32) if nodes is None else np.ascontiguousarray(nodes, np.uint32)
        st = StabilizeStats()
        self._chk(self._L.ovs_chord_stabilize(self._h, _ptr(nodes), len(nodes), C.cast(C.byref(st), C.c_void_p)),
                  "ovs_chord_stabilize")
        return {f: getattr(st, f) for f, _ in StabilizeStats._fields_}

    def kad_maintenance_round(self, nodes=None, flags=None, stale=None) -> dict:
        """One synchronous Kademlia maintenance round (ovs_kad_maintenance_round): the listed nodes'
        refresh lookups on the device (flags bit 0 sibling refresh, bit 1 bucket refreshes; None =
        both), then Kademlia::routingAdd for every call and response on the host; returns the counters
        plus "changes" (membership changes)."""
        nodes = np.arange(self.n, dtype=np.uint32) if nodes is None else np.ascontiguousarray(nodes, np.uint32)
        fl = None if flags is None else np.ascontiguousarray(np.broadcast_to(flags, nodes.shape), dtype=np.uint8)
        stl = None if stale is None else np.ascontiguousarray(stale, dtype=np.uint32)
        st = KadRoundStats()
        self._chk(self._L.ovs_kad_maintenance_round(self._h, _ptr(nodes), len(nodes), _ptr(fl), _ptr(stl),
                                                    C.cast(C.byref(st), C.c_void_p)), "ovs_kad_maintenance_round")
        d = {f: getattr(st, f) for f, _ in KadRoundStats._fields_}
        d["changes"] = d["sib_changes"] + d["bucket_changes"] + d["lost"]
        return d

    def chord_tables(self):
        """(pred, succ (n, successorListSize), nsucc) of an explicit-table ring as they now stand."""
        sls = self.get_params().successorListSize
        pred = np.empty(self.n, dtype=np.uint32)
        succ = np.empty((self.n, sls), dtype=np.uint32)
        nsucc = np.empty(self.n, dtype=np.uint8)
        self._chk(self._L.ovs_chord_export_tables(self._h, _ptr(pred), _ptr(succ), _ptr(nsucc)),
                  "ovs_chord_export_tables")
        return pred, succ, nsucc

    def kad_tables(self):
        p = self.get_params()
        sib = np.empty((self.n, 5 * p.s), dtype=np.uint32)
        cnt = np.empty((self.n, 160), dtype=np.uint8)
        nodes = np.empty((self.n, 160, p.k), dtype=np.uint32)
        self._chk(self._L.ovs_kad_export(self._h, _ptr(sib), _ptr(cnt), _ptr(nodes)), "ovs_kad_export")
        return sib, cnt, nodes

    # -- the hot path
    def lookup(self, keys, src, record_hops: bool = False, count_rpcs: bool = False) -> dict:
        """Batched KBRTestApp one-way lookups; returns numpy arrays by field."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        n = len(keys)
        if len(src) != n:
            raise ValueError("keys and src differ in length")
        out = np.empty(n, dtype=ROUTE_OUT_DTYPE)
        H = max(self.get_params().hopCountMax, 1)
        hop = np.empty((n, H), dtype=np.uint32) if record_hops else None
        rpcs = np.empty(n, dtype=np.uint32) if count_rpcs else None
        self._chk(self._L.ovs_route_batch(self._h, _ptr(keys), _ptr(src), n, _ptr(out), _ptr(hop), _ptr(rpcs), 0,
                                          None), "ovs_route_batch")
        res = {f: out[f].copy() for f in ROUTE_OUT_DTYPE.names}
        if hop is not None:
            res["hop_seq"] = hop
        if rpcs is not None:
            res["rpcs"] = rpcs
        return res

    def lookupCall(self, keys, src, numSiblings: int = -1) -> dict:
        """Batched LookupCalls (KBRTestApp lookup test; BaseOverlay::lookupRpc, BaseOverlay.cc:1938-1968,
        answered by SendToKeyListener::lookupFinished, 1272-1300).  numSiblings = -1 is
        getMaxNumSiblings(), as KBRTestApp sends it.  Returns num_siblings, hops, status, is_valid,
        latency_ns per lookup and `siblings` (n, numSiblings), NONE padded."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        n = len(keys)
        if len(src) != n:
            raise ValueError("keys and src differ in length")
        p = self.get_params()
        ns = numSiblings if numSiblings >= 0 else (p.successorListSize if p.overlay == OVERLAY_CHORD else p.s)
        out = np.empty(n, dtype=LOOKUP_OUT_DTYPE)
        sib = np.empty((n, max(ns, 1)), dtype=np.uint32)
        self._chk(self._L.ovs_lookup_batch(self._h, _ptr(keys), _ptr(src), n, numSiblings, _ptr(out), _ptr(sib), 0,
                                           None), "ovs_lookup_batch")
        res = {f: out[f].copy() for f in LOOKUP_OUT_DTYPE.names}
        res["siblings"] = sib
        return res

    def kad_refresh(self, keys, src, redundantNodes: int, record: bool = True) -> dict:
        """Kademlia refresh lookups (ovs_kad_refresh_batch): exhaustive-iterative lookups of keys[i] from
        src[i] with config.redundantNodes = numSiblings = redundantNodes (Kademlia.cc:1591-1686).
        Returns the LookupCall fields, `siblings` (n, R), `rpcs`, and with record the responders
        (n, hopCountMax) and their RTTs in ns, in the order the responses arrived."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        n = len(keys)
        if len(src) != n:
            raise ValueError("keys and src differ in length")
        R = int(redundantNodes)
        H = max(self.get_params().hopCountMax, 1)
        out = np.empty(n, dtype=LOOKUP_OUT_DTYPE)
        sib = np.empty((n, max(R, 1)), dtype=np.uint32)
        resp = np.empty((n, H), dtype=np.uint32) if record else None
        rtt = np.empty((n, H), dtype=np.int64) if record else None
        rpcs = np.empty(n, dtype=np.uint32)
        self._chk(self._L.ovs_kad_refresh_batch(self._h, _ptr(keys), _ptr(src), n, R, _ptr(out), _ptr(sib), _ptr(resp),
                                                _ptr(rtt), _ptr(rpcs), 0, None), "ovs_kad_refresh_batch")
        res = {f: out[f].copy() for f in LOOKUP_OUT_DTYPE.names}
        res["siblings"] = sib
        res["rpcs"] = rpcs
        if record:
            res["responders"] = resp
            res["rtt_ns"] = rtt
        return res

    def kad_refresh_device(self, keys_ptr: int, src_ptr: int, n: int, redundantNodes: int, out_ptr: int,
                           sib_ptr: int, rpcs_ptr: int | None = None, stream: int | None = None):
        """Device-resident refresh batch (no responder record)."""
        self._chk(self._L.ovs_kad_refresh_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n, redundantNodes,
                                                C.c_void_p(out_ptr), C.c_void_p(sib_ptr), None, None,
                                                C.c_void_p(rpcs_ptr) if rpcs_ptr else None, DEVICE_PTRS,
                                                C.c_void_p(stream) if stream else None), "ovs_kad_refresh_batch")

    def kad_refresh_keys(self, nodes=None, stale=None):
        """The bucket-refresh (keys, src) of Kademlia::handleBucketRefreshTimerExpired for `nodes`
        (default: all); stale = (m, 5) uint32 bit masks of the buckets due (None: all)."""
        nodes = np.arange(self.n, dtype=np.uint32) if nodes is None else np.ascontiguousarray(nodes, np.uint32)
        st = None if stale is None else np.ascontiguousarray(stale, dtype=np.uint32)
        cnt = C.c_uint64(0)
        self._chk(self._L.ovs_kad_refresh_keys(self._h, _ptr(nodes), len(nodes), _ptr(st), None, None, 0,
                                               C.byref(cnt), 0, None), "ovs_kad_refresh_keys")
        total = cnt.value
        keys = np.zeros((max(total, 1), 5), dtype=np.uint32)
        src = np.zeros(max(total, 1), dtype=np.uint32)
        self._chk(self._L.ovs_kad_refresh_keys(self._h, _ptr(nodes), len(nodes), _ptr(st), _ptr(keys), _ptr(src),
                                               total, C.byref(cnt), 0, None), "ovs_kad_refresh_keys")
        return keys[:total], src[:total]

    def lookup_device(self, keys_ptr: int, src_ptr: int, n: int, out_ptr: int, stream: int | None = None,
                      hop_ptr: int | None = None, rpcs_ptr: int | None = None):
        """Device-resident batch (pointers on this context's device, async on `stream`, 0 = default stream)."""
        self._chk(self._L.ovs_route_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n,
                                          C.c_void_p(out_ptr), C.c_void_p(hop_ptr) if hop_ptr else None,
                                          C.c_void_p(rpcs_ptr) if rpcs_ptr else None,
                                          DEVICE_PTRS, C.c_void_p(stream) if stream else None), "ovs_route_batch")

    def findNode(self, node, keys, numRedundantNodes: int, numSiblings: int, max_out: int = 16):
        keys = keys_array(keys)
        node = np.ascontiguousarray(node, dtype=np.uint32)
        n = len(keys)
        nodes = np.empty((n, max_out), dtype=np.uint32)
        cnt = np.empty(n, dtype=np.uint8)
        sib = np.empty(n, dtype=np.uint8)
        self._chk(self._L.ovs_find_node_batch(self._h, _ptr(node), _ptr(keys), n, numRedundantNodes, numSiblings,
                                              _ptr(nodes), max_out, _ptr(cnt), _ptr(sib), 0, None),
                  "ovs_find_node_batch")
        return nodes, cnt, sib

    def isSiblingFor(self, node, keys, numSiblings: int = 1) -> np.ndarray:
        _, _, sib = self.findNode(node, keys, 1, numSiblings, max_out=1)
        return sib.astype(bool)

    def delay_ns(self, a, b, nbytes) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint32)
        nbytes = np.ascontiguousarray(nbytes, dtype=np.int32)
        out = np.empty(len(a), dtype=np.int64)
        self._chk(self._L.ovs_delay_batch(self._h, _ptr(a), _ptr(b), _ptr(nbytes), len(a), _ptr(out), 0, None),
                  "ovs_delay_batch")
        return out

    def _broadcast(self, call: str, initiators, ttl: int, query_bytes: int, nodes: bool):
        init = np.ascontiguousarray(initiators, dtype=np.uint32)
        nb = len(init)
        rec = np.empty((nb, self.n), dtype=BCAST_NODE_DTYPE) if nodes else None
        st = (BcastStats * max(nb, 1))()
        self._chk(getattr(self._L, call)(self._h, _ptr(init), nb, int(ttl), int(query_bytes), _ptr(rec),
                                         C.cast(st, C.c_void_p), 0, None), call)
        return rec, [bcast_stats_dict(st[b]) for b in range(nb)]

    def _broadcast_device(self, call: str, init_ptr: int, nb: int, ttl: int, query_bytes: int, nodes_ptr: int | None,
                          stream: int | None):
        st = (BcastStats * max(nb, 1))()
        self._chk(getattr(self._L, call)(self._h, C.c_void_p(init_ptr), nb, int(ttl), int(query_bytes),
                                         C.c_void_p(nodes_ptr) if nodes_ptr else None, C.cast(st, C.c_void_p), DEVICE_PTRS,
                                         C.c_void_p(stream) if stream else None), call)
        return [bcast_stats_dict(st[b]) for b in range(nb)]

    def chord_broadcast(self, initiators, ttl: int = 100, query_bytes: int = 0, nodes: bool = True):
        """Batched overlay broadcasts on a converged Chord ring (ovs_chord_broadcast_batch:
        BroadcastTestApp::rpcBroadcastRequest over Chord::forwardBroadcast, Chord.cc:1410-1445), one
        from each initiator.  Returns (records, stats): records (nb, n) of BCAST_NODE_DTYPE (None with
        nodes=False) and one dict per broadcast (ovs_bcast_stats; hop_count = the cStdDev fields)."""
        return self._broadcast("ovs_chord_broadcast_batch", initiators, ttl, query_bytes, nodes)

    def chord_broadcast_device(self, init_ptr: int, nb: int, ttl: int, query_bytes: int, nodes_ptr: int | None,
                               stream: int | None = None):
        """The same for device-resident initiators / records (the call completes on `stream`); returns the stats."""
        return self._broadcast_device("ovs_chord_broadcast_batch", init_ptr, nb, ttl, query_bytes, nodes_ptr, stream)

    def pastry_broadcast(self, initiators, ttl: int = 100, query_bytes: int = 0, nodes: bool = True):
        """Batched overlay broadcasts on a Pastry context from either loader (ovs_pastry_broadcast_batch:
        BroadcastTestApp::rpcBroadcastRequest over Pastry::forwardBroadcast, Pastry.cc:1343-1390), one from
        each initiator.  Returns what chord_broadcast returns; on explicit tables with empty slots the nodes
        behind them stay unreached (arrival_ns -1)."""
        return self._broadcast("ovs_pastry_broadcast_batch", initiators, ttl, query_bytes, nodes)

    def pastry_broadcast_device(self, init_ptr: int, nb: int, ttl: int, query_bytes: int, nodes_ptr: int | None,
                                stream: int | None = None):
        """The same for device-resident initiators / records (the call completes on `stream`); returns the stats."""
        return self._broadcast_device("ovs_pastry_broadcast_batch", init_ptr, nb, ttl, query_bytes, nodes_ptr, stream)

    # -- Scribe
    def scribe_build(self, group_keys, member_group, member_node, capacity: int | None = None):
        """Build the Scribe forest of all groups (ovs_scribe_build) on a converged Chord ring (chord_load) or
        converged Pastry tables (pastry_load): member_node[i] subscribes to group member_group[i] (an index
        into group_keys).  capacity = the most tree nodes the forest may hold
        (default: memberships * 64 + groups, far above a Chord path's length).  Returns (tree nodes,
        edges, groups with a root)."""
        gk = keys_array(group_keys) if len(group_keys) else np.zeros((0, 5), np.uint32)
        mg = np.ascontiguousarray(member_group, dtype=np.uint32)
        mn = np.ascontiguousarray(member_node, dtype=np.uint32)
        if len(mg) != len(mn):
            raise ValueError("member_group and member_node differ in length")
        if capacity is None:
            capacity = len(mg) * 64 + len(gk)
        self._chk(self._L.ovs_scribe_build(self._h, _ptr(gk), len(gk), _ptr(mg), _ptr(mn), len(mg), int(capacity), 0, None),
                  "ovs_scribe_build")
        return self.scribe_count()

    def scribe_build_device(self, gk_ptr: int, n_groups: int, mg_ptr: int, mn_ptr: int, n_members: int, capacity: int,
                            stream: int | None = None):
        self._chk(self._L.ovs_scribe_build(self._h, C.c_void_p(gk_ptr), n_groups, C.c_void_p(mg_ptr), C.c_void_p(mn_ptr),
                                           n_members, int(capacity), DEVICE_PTRS, C.c_void_p(stream) if stream else None),
                  "ovs_scribe_build")
        return self.scribe_count()

    def scribe_clear(self):
        self._chk(self._L.ovs_scribe_clear(self._h), "ovs_scribe_clear")

    def scribe_count(self) -> tuple[int, int, int]:
        a, b, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._L.ovs_scribe_count(self._h, C.byref(a), C.byref(b), C.byref(r)), "ovs_scribe_count")
        return a.value, b.value, r.value

    def scribe_export(self) -> np.ndarray:
        """The forest as SCRIBE_NODE_DTYPE records sorted by (group, node)."""
        out = np.empty(self.scribe_count()[0], dtype=SCRIBE_NODE_DTYPE)
        self._chk(self._L.ovs_scribe_export(self._h, _ptr(out), 0, None), "ovs_scribe_export")
        return out

    def scribe_multicast(self, msg_group, msg_src, known_rp=None, payload_bytes: int = 100, deliveries: bool = True):
        """Publish message i from node msg_src[i] to group msg_group[i] (ovs_scribe_multicast_batch);
        known_rp[i]: the sender has the rendezvous point cached.  Returns (out, deliveries): SCRIBE_MSG_DTYPE
        per message and the SCRIBE_DELIVERY_DTYPE records sorted by (msg, node) (None with deliveries=False)."""
        mg = np.ascontiguousarray(msg_group, dtype=np.uint32)
        ms = np.ascontiguousarray(msg_src, dtype=np.uint32)
        mf = np.zeros(len(mg), np.uint8) if known_rp is None else np.ascontiguousarray(known_rp, dtype=np.uint8)
        if not (len(mg) == len(ms) == len(mf)):
            raise ValueError("msg_group, msg_src and known_rp differ in length")
        out = np.zeros(len(mg), dtype=SCRIBE_MSG_DTYPE)
        cnt = C.c_uint64()
        call = lambda d, cap: self._chk(self._L.ovs_scribe_multicast_batch(
            self._h, _ptr(mg), _ptr(ms), _ptr(mf), len(mg), int(payload_bytes), _ptr(out), _ptr(d), cap, C.byref(cnt), 0,
            None), "ovs_scribe_multicast_batch")
        if not deliveries:
            call(None, 0)
            return out, None
        # every subscriber of the message's group at most
        sub = self.scribe_export()
        per_group = np.bincount(sub["group"][(sub["flags"] & SCRIBE_SUBSCRIBER) != 0], minlength=1)
        cap = int(per_group[mg[mg < len(per_group)]].sum()) if len(mg) else 0
        d = np.zeros(max(cap, 1), dtype=SCRIBE_DELIVERY_DTYPE)
        call(d, cap)
        d = d[:min(cnt.value, cap)]
        return out, d[np.lexsort((d["node"], d["msg"]))]

    def scribe_multicast_device(self, mg_ptr: int, ms_ptr: int, mf_ptr: int, n: int, payload_bytes: int, out_ptr: int,
                                deliv_ptr: int | None = None, deliv_cap: int = 0, stream: int | None = None) -> int:
        """The same for device-resident arrays; returns the number of delivery records there are."""
        cnt = C.c_uint64()
        self._chk(self._L.ovs_scribe_multicast_batch(
            self._h, C.c_void_p(mg_ptr), C.c_void_p(ms_ptr), C.c_void_p(mf_ptr), n, int(payload_bytes), C.c_void_p(out_ptr),
            C.c_void_p(deliv_ptr) if deliv_ptr else None, deliv_cap, C.byref(cnt), DEVICE_PTRS,
            C.c_void_p(stream) if stream else None), "ovs_scribe_multicast_batch")
        return cnt.value

    def sync(self):
        self._chk(self._L.ovs_sync(self._h), "ovs_sync")

    # -- KBRTestApp statistics
    def kbrtest_stats(self, result: dict | np.ndarray, keys, src, measured_time_s: float,
                      lookupNodeIds: bool = True) -> KbrTestStats:
        """Reduce lookup() results to the KBRTestApp one-way statistics on the device."""
        if isinstance(result, dict):
            out = np.empty(len(result["responsible"]), dtype=ROUTE_OUT_DTYPE)
            for f in ROUTE_OUT_DTYPE.names:
                out[f] = result[f]
        else:
            out = np.ascontiguousarray(result, dtype=ROUTE_OUT_DTYPE)
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        if not (len(out) == len(keys) == len(src)):
            raise ValueError("result, keys and src differ in length")
        st = KbrTestStats()
        self._chk(self._L.ovs_kbrtest_stats_batch(self._h, _ptr(out), _ptr(keys), _ptr(src), len(out),
                                                  float(measured_time_s), int(bool(lookupNodeIds)), C.byref(st),
                                                  0, None), "ovs_kbrtest_stats_batch")
        return st

    def kbrtest_lookup_stats(self, result: dict, keys, src, measured_time_s: float, lookupNodeIds: bool = True,
                             failureLatency: float = 10.0) -> KbrTestLookupStats:
        """Reduce lookupCall() results to the KBRTestApp lookup-test statistics on the device."""
        out = np.empty(len(result["hops"]), dtype=LOOKUP_OUT_DTYPE)
        for f in LOOKUP_OUT_DTYPE.names:
            out[f] = result[f]
        sib = np.ascontiguousarray(result["siblings"], dtype=np.uint32)
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        st = KbrTestLookupStats()
        self._chk(self._L.ovs_kbrtest_lookup_stats_batch(self._h, _ptr(out), _ptr(sib), sib.shape[1], _ptr(keys),
                                                         _ptr(src), len(out), float(measured_time_s),
                                                         int(bool(lookupNodeIds)), float(failureLatency),
                                                         C.byref(st), 0, None), "ovs_kbrtest_lookup_stats_batch")
        return st

    # -- KBRTestApp RPC test
    def rpcCall(self, keys, src) -> dict:
        """Batched routed KbrTestCall round trips (KBRTestApp with kbrRpcTest; KBRTestApp.cc:172-189,
        230-329): RPC i from node src[i] to keys[i].  Returns the ovs_rpc_out fields as arrays."""
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        n = len(keys)
        if len(src) != n:
            raise ValueError("keys and src differ in length")
        out = np.empty(n, dtype=RPC_OUT_DTYPE)
        self._chk(self._L.ovs_rpc_batch(self._h, _ptr(keys), _ptr(src), n, _ptr(out), 0, None), "ovs_rpc_batch")
        return {f: out[f].copy() for f in RPC_OUT_DTYPE.names}

    def rpc_device(self, keys_ptr: int, src_ptr: int, n: int, out_ptr: int, stream: int | None = None):
        """Device-resident RPC batch (pointers on this context's device, async on `stream`, 0 = default stream)."""
        self._chk(self._L.ovs_rpc_batch(self._h, C.c_void_p(keys_ptr), C.c_void_p(src_ptr), n, C.c_void_p(out_ptr),
                                        DEVICE_PTRS, C.c_void_p(stream) if stream else None), "ovs_rpc_batch")

    def kbrtest_rpc_stats(self, result: dict | np.ndarray, keys, src, measured_time_s: float,
                          lookupNodeIds: bool = True, failureLatency: float = 10.0) -> KbrTestRpcStats:
        """Reduce rpcCall() results to the KBRTestApp RPC-test statistics on the device."""
        if isinstance(result, dict):
            out = np.zeros(len(result["responder"]), dtype=RPC_OUT_DTYPE)
            for f in RPC_OUT_DTYPE.names:
                if f in result:
                    out[f] = result[f]
        else:
            out = np.ascontiguousarray(result, dtype=RPC_OUT_DTYPE)
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        if not (len(out) == len(keys) == len(src)):
            raise ValueError("result, keys and src differ in length")
        st = KbrTestRpcStats()
        self._chk(self._L.ovs_kbrtest_rpc_stats_batch(self._h, _ptr(out), _ptr(keys), _ptr(src), len(out),
                                                      float(measured_time_s), int(bool(lookupNodeIds)),
                                                      float(failureLatency), C.byref(st), 0, None),
                  "ovs_kbrtest_rpc_stats_batch")
        return st

    # -- DHT tier
    def dht_store_create(self, capacity: int):
        """The context's DHT data storage: an open-addressing table of `capacity` slots on the device."""
        self._chk(self._L.ovs_dht_store_create(self._h, int(capacity)), "ovs_dht_store_create")

    def dht_store_clear(self):
        self._chk(self._L.ovs_dht_store_clear(self._h), "ovs_dht_store_clear")

    def dht_store_count(self) -> tuple[int, int]:
        """(claimed slots, device-pointer put batches refused for lack of room)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self._L.ovs_dht_store_count(self._h, C.byref(a), C.byref(b), None), "ovs_dht_store_count")
        return a.value, b.value

    def dhttest_stats(self, put_out, put_src, get_out, get_ops, get_src, expect, measured_time_s: float) -> DhtTestStats:
        """DHTTestApp statistics of one put batch and one get batch (either may be empty); `expect`
        (DHT_EXPECT_DTYPE) is the caller's GlobalDhtTestMap entry for each get."""
        po = np.ascontiguousarray(put_out, dtype=DHT_PUT_DTYPE)
        ps = np.ascontiguousarray(put_src, dtype=np.uint32)
        go = np.ascontiguousarray(get_out, dtype=DHT_GET_DTYPE)
        gp = np.ascontiguousarray(get_ops, dtype=DHT_OP_DTYPE)
        gs = np.ascontiguousarray(get_src, dtype=np.uint32)
        ex = np.ascontiguousarray(expect, dtype=DHT_EXPECT_DTYPE)
        if len(po) != len(ps) or not (len(go) == len(gp) == len(gs) == len(ex)):
            raise ValueError("records, sources and expectations differ in length")
        st = DhtTestStats()
        self._chk(self._L.ovs_dhttest_stats_batch(self._h, _ptr(po), _ptr(ps), len(po), _ptr(go), _ptr(gp), _ptr(gs),
                                                  _ptr(ex), len(go), float(measured_time_s), C.byref(st), 0, None),
                  "ovs_dhttest_stats_batch")
        return st

    def _dht(self, fn, name, dtype, keys, src, ops, dp):
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        ops = np.ascontiguousarray(ops, dtype=DHT_OP_DTYPE)
        n = len(keys)
        if not (len(src) == len(ops) == n):
            raise ValueError("keys, src and ops differ in length")
        dp = dp if dp is not None else DhtParams.default()
        out = np.zeros(n, dtype=dtype)
        self._chk(fn(self._h, C.byref(dp), _ptr(keys), _ptr(src), _ptr(ops), n, _ptr(out), 0, None), name)
        return out

    def dht_put(self, keys, src, ops, dp: "DhtParams | None" = None) -> np.ndarray:
        """Batched DHT puts (DHT.cc:499-516, 832-897): put i from node src[i] stores ops[i] (DHT_OP_DTYPE) under
        keys[i].  Returns DHT_PUT_DTYPE records."""
        return self._dht(self._L.ovs_dht_put_batch, "ovs_dht_put_batch", DHT_PUT_DTYPE, keys, src, ops, dp)

    def dht_get(self, keys, src, ops, dp: "DhtParams | None" = None) -> np.ndarray:
        """Batched DHT gets (DHT.cc:518-535, 898-957, 577-715).  Returns DHT_GET_DTYPE records."""
        return self._dht(self._L.ovs_dht_get_batch, "ovs_dht_get_batch", DHT_GET_DTYPE, keys, src, ops, dp)

    def dht_put_device(self, keys_ptr: int, src_ptr: int, ops_ptr: int, n: int, out_ptr: int,
                       dp: "DhtParams | None" = None, stream: int | None = None):
        """Device-resident put batch (async on `stream`; a batch that does not fit is counted by dht_store_count)."""
        dp = dp if dp is not None else DhtParams.default()
        self._chk(self._L.ovs_dht_put_batch(self._h, C.byref(dp), C.c_void_p(keys_ptr), C.c_void_p(src_ptr),
                                            C.c_void_p(ops_ptr), n, C.c_void_p(out_ptr), DEVICE_PTRS,
                                            C.c_void_p(stream) if stream else None), "ovs_dht_put_batch")

    def dht_get_device(self, keys_ptr: int, src_ptr: int, ops_ptr: int, n: int, out_ptr: int,
                       dp: "DhtParams | None" = None, stream: int | None = None):
        dp = dp if dp is not None else DhtParams.default()
        self._chk(self._L.ovs_dht_get_batch(self._h, C.byref(dp), C.c_void_p(keys_ptr), C.c_void_p(src_ptr),
                                            C.c_void_p(ops_ptr), n, C.c_void_p(out_ptr), DEVICE_PTRS,
                                            C.c_void_p(stream) if stream else None), "ovs_dht_get_batch")

    def dht_dump(self, node: int, now_ns: int) -> np.ndarray:
        """DHTdumpCall: the node's entries live at now_ns in insertion order (DHT_ENTRY_DTYPE)."""
        cnt = C.c_uint64()
        self._chk(self._L.ovs_dht_dump_node(self._h, int(node), int(now_ns), None, 0, C.byref(cnt)), "ovs_dht_dump_node")
        out = np.zeros(cnt.value, dtype=DHT_ENTRY_DTYPE)
        if cnt.value:
            self._chk(self._L.ovs_dht_dump_node(self._h, int(node), int(now_ns), _ptr(out), cnt.value, C.byref(cnt)),
                      "ovs_dht_dump_node")
        return out

    # -- replica-team DHTs (SymmetricDHT.cc / RepeatedHashingDHT.cc)
    def dht_team_keys(self, keys, tp: DhtTeamParams) -> np.ndarray:
        """The derived keys, (n, T, 5) uint32: key_0 = key, then + offset (symmetric) or SHA-1 of the hex string."""
        keys = keys_array(keys)
        out = np.zeros((len(keys), tp.numReplicaTeams, 5), dtype=np.uint32)
        self._chk(self._L.ovs_dht_team_keys(self._h, C.byref(tp), _ptr(keys), len(keys), _ptr(out), 0, None),
                  "ovs_dht_team_keys")
        return out

    def _dht_team(self, fn, name, dtype, keys, src, ops, tp, dp):
        keys = keys_array(keys)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        ops = np.ascontiguousarray(ops, dtype=DHT_OP_DTYPE)
        n = len(keys)
        if not (len(src) == len(ops) == n):
            raise ValueError("keys, src and ops differ in length")
        dp = dp if dp is not None else DhtParams.default()
        T = max(int(tp.numReplicaTeams), 1)
        out, team, win = np.zeros(n, dtype=dtype), np.zeros((n, T), dtype=dtype), np.zeros(n, dtype=np.int32)
        self._chk(fn(self._h, C.byref(dp), C.byref(tp), _ptr(keys), _ptr(src), _ptr(ops), n, _ptr(out), _ptr(team), _ptr(win),
                     0, None), name)
        return out, team, win

    def dht_team_put(self, keys, src, ops, tp: DhtTeamParams, dp: "DhtParams | None" = None):
        """Batched puts of a replica-team DHT: (out[n], team_out[n, T], winner[n]); `out` is the record of the team
        whose DHTputCAPIResponse tier 2 accepts.  dp.numReplica is the value before initializeDHT divides it."""
        return self._dht_team(self._L.ovs_dht_team_put_batch, "ovs_dht_team_put_batch", DHT_PUT_DTYPE, keys, src, ops, tp, dp)

    def dht_team_get(self, keys, src, ops, tp: DhtTeamParams, dp: "DhtParams | None" = None):
        """Batched gets of a replica-team DHT: (out[n], team_out[n, T], winner[n])."""
        return self._dht_team(self._L.ovs_dht_team_get_batch, "ovs_dht_team_get_batch", DHT_GET_DTYPE, keys, src, ops, tp, dp)

    def dht_team_device(self, is_put: bool, keys_ptr: int, src_ptr: int, ops_ptr: int, n: int, out_ptr: int, team_out_ptr: int,
                        winner_ptr: int, tp: DhtTeamParams, dp: "DhtParams | None" = None, stream: int | None = None):
        """Device-resident team batch (async on `stream`; a put batch that does not fit is counted by dht_store_count)."""
        dp = dp if dp is not None else DhtParams.default()
        fn = self._L.ovs_dht_team_put_batch if is_put else self._L.ovs_dht_team_get_batch
        self._chk(fn(self._h, C.byref(dp), C.byref(tp), C.c_void_p(keys_ptr), C.c_void_p(src_ptr), C.c_void_p(ops_ptr), n,
                     C.c_void_p(out_ptr), C.c_void_p(team_out_ptr), C.c_void_p(winner_ptr), DEVICE_PTRS,
                     C.c_void_p(stream) if stream else None), "ovs_dht_team_put_batch" if is_put else "ovs_dht_team_get_batch")

    def dhttest_team_stats(self, tp: DhtTeamParams, put_out, put_team_out, put_src, get_out, get_team_out, get_ops, get_src,
                           expect, measured_time_s: float) -> DhtTestStats:
        """DHTTestApp statistics of a team put batch and a team get batch: outcomes and latencies from the `out`
        records, hop counts, messages and bytes from the team records."""
        po = np.ascontiguousarray(put_out, dtype=DHT_PUT_DTYPE)
        pt = np.ascontiguousarray(put_team_out, dtype=DHT_PUT_DTYPE).reshape(-1)
        ps = np.ascontiguousarray(put_src, dtype=np.uint32)
        go = np.ascontiguousarray(get_out, dtype=DHT_GET_DTYPE)
        gt = np.ascontiguousarray(get_team_out, dtype=DHT_GET_DTYPE).reshape(-1)
        gp = np.ascontiguousarray(get_ops, dtype=DHT_OP_DTYPE)
        gs = np.ascontiguousarray(get_src, dtype=np.uint32)
        ex = np.ascontiguousarray(expect, dtype=DHT_EXPECT_DTYPE)
        T = int(tp.numReplicaTeams)
        if len(po) != len(ps) or len(pt) != len(po) * T or not (len(go) == len(gp) == len(gs) == len(ex)) or len(gt) != len(go) * T:
            raise ValueError("records, sources and expectations differ in length")
        st = DhtTestStats()
        self._chk(self._L.ovs_dhttest_team_stats_batch(self._h, C.byref(tp), _ptr(po), _ptr(pt), _ptr(ps), len(po), _ptr(go),
                                                       _ptr(gt), _ptr(gp), _ptr(gs), _ptr(ex), len(go),
                                                       float(measured_time_s), C.byref(st), 0, None),
                  "ovs_dhttest_team_stats_batch")
        return st

    def kbrtest_stats_device(self, out_ptr: int, keys_ptr: int, src_ptr: int, n: int, measured_time_s: float,
                             lookupNodeIds: bool = True, stream: int | None = None) -> KbrTestStats:
        """Same as kbrtest_stats for a device-resident batch (synchronises `stream`)."""
        st = KbrTestStats()
        self._chk(self._L.ovs_kbrtest_stats_batch(self._h, C.c_void_p(out_ptr), C.c_void_p(keys_ptr),
                                                  C.c_void_p(src_ptr), n, float(measured_time_s),
                                                  int(bool(lookupNodeIds)), C.byref(st), DEVICE_PTRS,
                                                  C.c_void_p(stream) if stream else None),
                  "ovs_kbrtest_stats_batch")
        return st


@dataclass
class Network:
    """A generated overlay population: sorted unique ids + SimpleUnderlay coordinates."""

    ids: np.ndarray   # (n,5) uint32
    xy: np.ndarray    # (n,2) float64

    @property
    def n(self) -> int:
        return len(self.ids)
