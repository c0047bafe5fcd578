"""oversim_amd -- MI355X-native batched KBR lookup routing for OverSim's Chord and Kademlia.

The product is the C-ABI library libovs_kbr.so (include/ovs_kbr.h) built from
the HIP sources in oversim_amd/csrc; this package is its host-side mirror of
the reference's BaseOverlay / AbstractLookup interface (kbr.py) plus workload
generation (workload.py).
"""
from .kbr import (BCAST_NODE_DTYPE, DEVICE_PTRS, LOOKUP_OUT_DTYPE, LOOKUP_STATUS, NONE, OVERLAY_CHORD,  # noqa: F401
                  OVERLAY_KADEMLIA, ROUTE_OUT_DTYPE, RPC_OUT_DTYPE, BcastStats, KbrEngine, KbrError, KbrTestRpcStats, Network, Params,
                  key_from_int, key_to_int, keys_array, lib)
from .kbr import DHT_ENTRY_DTYPE, DHT_EXPECT_DTYPE, DHT_GET_DTYPE, DHT_OP_DTYPE, DHT_PUT_DTYPE, DhtParams, DhtTestStats  # noqa: F401
from .kbr import DHT_TEAMS_REPEATED_HASHING, DHT_TEAMS_SYMMETRIC, DhtTeamParams  # noqa: F401
from .kbr import SCRIBE_DELIVERY_DTYPE, SCRIBE_MSG_DTYPE, SCRIBE_NODE_DTYPE, SCRIBE_STATUS, ScribeParams  # noqa: F401
from .kbr import BROOSE_EXT_DTYPE, OVERLAY_BROOSE, BrooseParams  # noqa: F401
from .kbr import OVERLAY_PASTRY, PastryParams  # noqa: F401

__all__ = ["PastryParams", "OVERLAY_PASTRY", "BrooseParams", "BROOSE_EXT_DTYPE", "OVERLAY_BROOSE","KbrEngine", "KbrError", "Params", "Network", "lib", "keys_array", "key_from_int", "key_to_int",
           "OVERLAY_CHORD", "OVERLAY_KADEMLIA", "ROUTE_OUT_DTYPE", "LOOKUP_OUT_DTYPE", "LOOKUP_STATUS", "NONE", "DEVICE_PTRS",
           "BCAST_NODE_DTYPE", "BcastStats", "RPC_OUT_DTYPE", "KbrTestRpcStats",
           "DhtParams", "DHT_OP_DTYPE", "DHT_PUT_DTYPE", "DHT_GET_DTYPE", "DHT_ENTRY_DTYPE", "DHT_EXPECT_DTYPE",
           "DhtTestStats", "DhtTeamParams", "DHT_TEAMS_SYMMETRIC", "DHT_TEAMS_REPEATED_HASHING", "ScribeParams", "SCRIBE_NODE_DTYPE", "SCRIBE_MSG_DTYPE", "SCRIBE_DELIVERY_DTYPE", "SCRIBE_STATUS"]
