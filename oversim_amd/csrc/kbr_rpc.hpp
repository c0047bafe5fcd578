// kbr_rpc.hpp -- KBRTestApp RPC test: response leg and timeout rule (internal; its statistics: stats.hpp).
#pragma once
#include "engine.hpp"

namespace ovs {

// per-launch constants of the response leg (host: ovs_rpc_batch)
struct RpcConsts {
    int64_t timeout;     // T(rpcKeyTimeout): rtt >= timeout is a timeout
    int64_t respMsg;     // 2*T(L*8/datarate) + 2*T(accessDelay) of the direct KbrTestResponse
    int32_t round;       // SimTime(double) rounding rule
    int32_t full;        // full-recursive routing: the response is a second route
    uint32_t nnodes;
    int64_t respQueue;   // what the responder's transmit queue holds ahead of the response: 0, or on Pastry under
                         // routeMsgAcks T(L*8/datarate) of the NextHopResponse it has just sent (ovs_pastry_rpc_batch)
};

// Pass 1 over the call routes: writes out[i]; full-recursive routing: also the return route's inputs
// rkeys[i] = ids[src[i]], rsrc[i] = the responder (an unanswered call: src[i], a self-route).
hipError_t launch_rpc_finish(const ovs_route_out* route, const uint32_t* src, const KeyRec* recs, const double2* xy,
                             const RpcConsts& RC, uint64_t n, ovs_rpc_out* out, K160* rkeys, uint32_t* rsrc,
                             int num_cu, hipStream_t s);
// Pass 2 (full-recursive routing): folds the return routes into out
hipError_t launch_rpc_fold(const ovs_route_out* ret, const uint32_t* src, const RpcConsts& RC, uint64_t n,
                           ovs_rpc_out* out, int num_cu, hipStream_t s);

}  // namespace ovs
