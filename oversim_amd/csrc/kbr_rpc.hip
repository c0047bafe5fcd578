// kbr_rpc.hip -- KBRTestApp RPC test (kbrRpcTest): the response leg of a batch of routed KbrTestCalls
// and the timeout rule.  The call leg is a one-way route (ovs_route_batch's kernels); the statistics are
// stats.hip's k_stats_lookups over these records.
//
// Reference: KBRTestApp::kbrTestCall / handleRpcResponse / handleRpcTimeout / finishApp
// (KBRTestApp.cc:230-329, 519-545), BaseApp::internalSendRpcResponse (BaseApp.cc:572-611),
// BaseRpc::sendRpcResponse (BaseRpc.cc:531-596), BaseRpc::sendRpcCall's timeout (BaseRpc.cc:202-205,
// 257-258), BaseOverlay::route (BaseOverlay.cc:1310-1359), the UDP hop count (BaseOverlay.cc:747-751),
// SimpleNodeEntry::calcDelay (SimpleNodeEntry.cc:155-195).
//
// k_rpc_finish: one lane per RPC, grid-stride.  Reads the 16 B route record and src[i], gathers the two
// 16 B coordinate pairs and evaluates the direct response's delay (iterative / semi-recursive
// routing), applies rtt >= rpcKeyTimeout and writes the 32 B record.  Full-recursive routing: it writes
// the return route's inputs instead (key = ids[src], source = responder); a call nobody answered gets
// the harmless self-route src -> ids[src] (0 hops, no table walk), whose result k_rpc_fold ignores,
// so the route kernel never sees a bad source index and nothing is compacted.  k_rpc_fold adds the
// return route.  No lane waits for another wave; every loop is bounded by n.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "kbr_rpc.hpp"
#include "tier_dev.hpp"

namespace ovs {

namespace {

__global__ __launch_bounds__(256) void k_rpc_finish(const ovs_route_out* __restrict__ route,
                                                    const uint32_t* __restrict__ src,
                                                    const KeyRec* __restrict__ recs,
                                                    const double2* __restrict__ xy, RpcConsts RC, uint64_t n,
                                                    ovs_rpc_out* __restrict__ out, K160* __restrict__ rkeys,
                                                    uint32_t* __restrict__ rsrc)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const ovs_route_out r = route[i];
        // device-pointer calls do not check sources (ovs_kbr.h): this pass still reads inside the tables
        const uint32_t s = src[i] < RC.nnodes ? src[i] : 0u;
        const bool answered = r.status == OVS_LOOKUP_OK && r.responsible < RC.nnodes;
        ovs_rpc_out o{};
        o.responder = answered ? r.responsible : NONE;
        o.call_hops = answered ? r.one_way_hops : (uint8_t)0;   // callHopCount (BaseRpc.cc:570)
        o.status = r.status;
        o.outcome = OVS_RPC_TIMEOUT;
        o.rtt_ns = -1;
        o.call_latency_ns = answered ? r.latency_ns : -1;
        if (RC.full) {
            // BaseApp.cc:595-599: destKey = the caller's key, routed from the responder
            const KeyRec k = load_rec(recs, s);
            K160 rk;
#pragma unroll
            for (int j = 0; j < 5; ++j) rk.w[j] = k.w[j];
            rkeys[i] = rk;
            rsrc[i] = answered ? r.responsible : s;
        } else if (answered) {
            // BaseOverlay.cc:1340-1341: one UDP message; to the node itself no delay (SimpleUDP.cc:322) and
            // the hop count stays 0 (BaseOverlay.cc:747-751)
            int64_t d = 0;
            uint32_t rh = 0;
            if (r.responsible != s) {
                const double2 a = xy[r.responsible], b = xy[s];
                d = RC.respQueue + RC.respMsg + coord_ns(a.x, a.y, b.x, b.y, RC.round);
                rh = 1;
            }
            const int64_t rtt = r.latency_ns + d;
            if (rtt < RC.timeout) {                 // the timeout event precedes a response at the same instant
                o.outcome = OVS_RPC_ANSWERED;
                o.rtt_ns = rtt;
                o.hop_count = (uint16_t)(o.call_hops + rh);
            }
        }
        out[i] = o;
    }
}

__global__ __launch_bounds__(256) void k_rpc_fold(const ovs_route_out* __restrict__ ret,
                                                  const uint32_t* __restrict__ src, RpcConsts RC, uint64_t n,
                                                  ovs_rpc_out* __restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        ovs_rpc_out o = out[i];
        if (o.responder == NONE) continue;          // the self-route of an unanswered call: ignored
        const ovs_route_out r = ret[i];
        o.resp_status = r.status;
        // a response that ends at another node finds no pending call there and is dropped
        if (r.status == OVS_LOOKUP_OK && r.responsible == src[i]) {
            const int64_t rtt = o.call_latency_ns + r.latency_ns;
            if (rtt < RC.timeout) {
                o.outcome = OVS_RPC_ANSWERED;
                o.rtt_ns = rtt;
                o.hop_count = (uint16_t)((uint32_t)o.call_hops + r.one_way_hops);
            }
        }
        out[i] = o;
    }
}

}  // namespace

hipError_t launch_rpc_finish(const ovs_route_out* route, const uint32_t* src, const KeyRec* recs, const double2* xy,
                             const RpcConsts& RC, uint64_t n, ovs_rpc_out* out, K160* rkeys, uint32_t* rsrc,
                             int num_cu, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (RC.nnodes == 0 || (RC.full && (!rkeys || !rsrc))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rpc_finish, dim3(capped_grid(n, 256, num_cu, 8)), dim3(256), 0, s, route, src, recs, xy, RC, n, out,
                       rkeys, rsrc);
    return hipGetLastError();
}

hipError_t launch_rpc_fold(const ovs_route_out* ret, const uint32_t* src, const RpcConsts& RC, uint64_t n,
                           ovs_rpc_out* out, int num_cu, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rpc_fold, dim3(capped_grid(n, 256, num_cu, 8)), dim3(256), 0, s, ret, src, RC, n, out);
    return hipGetLastError();
}

}  // namespace ovs
