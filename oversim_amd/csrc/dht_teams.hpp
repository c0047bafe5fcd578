// dht_teams.hpp -- replica-team DHTs (SymmetricDHT.cc, RepeatedHashingDHT.cc): the team keys and the
// time-ordered replay of one operation's teams through shared transmit queues (internal).
#pragma once
#include "dht.hpp"

namespace ovs {

constexpr int TEAMS_MAX = 8;         // numReplicaTeams <= 8
constexpr int TEAM_HCM_MAX = 1000;   // the replay numbers an operation's events in 16 bits

// per-launch constants of the replay (host: ovs_dht_team_put_batch / ovs_dht_team_get_batch)
struct TeamConsts {
    DhtConsts D;            // R = numReplica / T, the siblings of one team
    int64_t lookupTimeout;  // T(LOOKUP_TIMEOUT)
    int32_t T;              // numReplicaTeams
    int32_t hcm;            // hopCountMax = the stride of the recorded chains
    int32_t m;              // NodeHandles the responsible node answers: min(R, 1 + successors)
    int32_t respBase;       // a FindNodeResponse without NodeHandles on the wire: 61 B, 161 B with measureAuthBlock
};

// team_keys[i * T + j] = key_j of keys[i]; team_src / team_ops (both or neither): src[i] (a source outside
// the network becomes node 0, as the DHT kernels read it) and ops[i] once per team
hipError_t launch_team_keys(int mode, int T, const K160& offset, uint32_t nnodes, const K160* keys, const uint32_t* src,
                            const ovs_dht_op* ops, uint64_t n, K160* team_keys, uint32_t* team_src, ovs_dht_op* team_ops,
                            hipStream_t s);
// route[n * T], hopseq[n * T * hcm]: the team keys routed one-way without timeouts, responders recorded.
// put: pair_t / pair_node [n * T * R]: each DHTPutCall's arrival (-1: none) and replica; adds the pairs without
// a slot to the store's need counter, like launch_dht_put_plan
hipError_t launch_team_put(const DhtStore& st, const TeamConsts& C, const ovs_route_out* route, const uint32_t* hopseq,
                           const K160* team_keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                           ovs_dht_put_out* team_out, ovs_dht_put_out* out, int32_t* winner, long long* pair_t,
                           uint32_t* pair_node, hipStream_t s);
hipError_t launch_team_get(const DhtStore& st, const TeamConsts& C, const ovs_route_out* route, const uint32_t* hopseq,
                           const K160* team_keys, const uint32_t* src, const ovs_dht_op* ops, const double2* xy, uint64_t n,
                           ovs_dht_get_out* team_out, ovs_dht_get_out* out, int32_t* winner, hipStream_t s);

}  // namespace ovs
