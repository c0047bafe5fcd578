// team_params.hpp -- the host pieces of the replica-team DHTs that need no device: the checks of
// SymmetricDHT / RepeatedHashingDHT::initializeDHT and SymmetricDHT's overlayKeyOffset.  Plain C++ against
// include/ovs_kbr.h alone (tests/dht_teams_driver.cpp builds it with g++ under sanitizers).
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ovs_kbr.h"

namespace ovs {

// SymmetricDHT.cc:40-43 / RepeatedHashingDHT.cc:40-43 and the sizes the replay is built for
inline ovs_status team_params_check(const ovs_dht_params* dp, const ovs_dht_team_params* tp, std::string* msg)
{
    if (!dp || !tp) { *msg = "null argument"; return OVS_EINVAL; }
    if (tp->mode != OVS_DHT_TEAMS_SYMMETRIC && tp->mode != OVS_DHT_TEAMS_REPEATED_HASHING) {
        *msg = "team mode: symmetric or repeated hashing";
        return OVS_ENOTSUP;
    }
    const int32_t T = tp->numReplicaTeams;
    if (T < 1 || T > 8) { *msg = "dht.numReplicaTeams outside 1..8"; return OVS_ENOTSUP; }
    if (dp->numReplica % T != 0) {
        *msg = "initializeDHT(): numReplica must be a multiple of numReplicaTeams.";
        return OVS_EINVAL;
    }
    // the replay holds 8 put RPCs, or 8 hash and 8 value RPCs, per operation across all its teams
    if (dp->numReplica < 1 || dp->numReplica > 8) {
        *msg = "replica teams: dht.numReplica (all teams together) outside 1..8";
        return OVS_ENOTSUP;
    }
    return OVS_OK;
}

// OverlayKey::getMax() / T: mpn_divrem_1 of the 160-bit all-ones number by one limb (OverlayKey.cc:274-279),
// the quotient floor((2^160 - 1) / T) as five 32-bit words, least significant first.  T >= 1.
inline void team_offset(int32_t T, uint32_t w[5])
{
    uint64_t rem = 0;
    for (int i = 4; i >= 0; --i) {
        const uint64_t cur = (rem << 32) | 0xFFFFFFFFull;
        w[i] = (uint32_t)(cur / (uint64_t)T);
        rem = cur % (uint64_t)T;
    }
}

}  // namespace ovs
