// kbr_rpc.hip -- KBRTestApp RPC test (kbrRpcTest): the response leg of a batch of routed KbrTestCalls,
// the timeout rule and the statistics.  The call leg is a one-way route (ovs_route_batch's kernels).
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
// return route.  k_kbrtest_rpc_stats: integer sums in registers -> wave reduction -> one global atomic
// per wave at the end; status and hop histograms in LDS; per-node counters by global atomics whose
// value is never read back in the kernel.  No lane waits for another wave; every loop is bounded by n.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "kbr_rpc.hpp"

namespace ovs {

namespace {

__device__ __forceinline__ uint64_t wsum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint64_t wmin(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t wmax(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

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
                d = RC.respMsg + coord_ns(a.x, a.y, b.x, b.y, RC.round);
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

__global__ __launch_bounds__(256) void k_kbrtest_rpc_stats(const ovs_rpc_out* __restrict__ out,
                                                           const K160* __restrict__ keys,
                                                           const uint32_t* __restrict__ src,
                                                           const KeyRec* __restrict__ recs, uint64_t n,
                                                           uint32_t nnodes, int lookup_node_ids,
                                                           RpcStatsDev* __restrict__ S,
                                                           uint32_t* __restrict__ node_sent,
                                                           uint32_t* __restrict__ node_deliv,
                                                           uint32_t* __restrict__ node_drop)
{
    __shared__ uint32_t hist[64];
    __shared__ uint32_t stat[8];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    if (threadIdx.x < 8) stat[threadIdx.x] = 0;
    __syncthreads();

    uint64_t deliv = 0, drop = 0, tmo = 0, hops = 0, lat = 0;
    uint64_t hmin = ~0ull, hmax = 0, lmin = ~0ull, lmax = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const ovs_rpc_out o = out[i];
        const uint32_t s = src[i];
        const bool valid_src = s < nnodes;
        atomicAdd(&stat[o.status & 7], 1u);
        if (valid_src) atomicAdd(&node_sent[s], 1u);
        bool ok = o.outcome == OVS_RPC_ANSWERED;
        tmo += ok ? 0 : 1;
        if (ok && lookup_node_ids) {
            // KBRTestApp.cc:254-256: destKey == srcNode.getKey() && destAddr == srcNode (unique IDs)
            if (o.responder < nnodes) {
                const KeyRec r = load_rec(recs, o.responder);
                const K160 k = keys[i];
                ok = r.w[0] == k.w[0] && r.w[1] == k.w[1] && r.w[2] == k.w[2] && r.w[3] == k.w[3] && r.w[4] == k.w[4];
            } else {
                ok = false;
            }
        }
        if (!ok) {
            ++drop;
            if (valid_src) atomicAdd(&node_drop[s], 1u);
            continue;
        }
        ++deliv;
        if (valid_src) atomicAdd(&node_deliv[s], 1u);
        const uint64_t h = o.hop_count;             // "RPC Hop Count"
        const uint64_t l = (uint64_t)o.rtt_ns;      // "RPC Success Latency"
        hops += h;
        lat += l;
        hmin = h < hmin ? h : hmin;
        hmax = h > hmax ? h : hmax;
        lmin = l < lmin ? l : lmin;
        lmax = l > lmax ? l : lmax;
        atomicAdd(&hist[h < 63 ? h : 63], 1u);
    }
    deliv = wsum(deliv);
    drop = wsum(drop);
    tmo = wsum(tmo);
    hops = wsum(hops);
    lat = wsum(lat);
    hmin = wmin(hmin);
    hmax = wmax(hmax);
    lmin = wmin(lmin);
    lmax = wmax(lmax);
    if ((threadIdx.x & 63) == 0) {
        if (deliv) atomicAdd(&S->delivered, deliv);
        if (drop) atomicAdd(&S->dropped, drop);
        if (tmo) atomicAdd(&S->timeout, tmo);
        if (hops) atomicAdd(&S->hop_sum, hops);
        if (lat) atomicAdd(&S->lat_sum, lat);
        if (hmin != ~0ull) {
            atomicMin(&S->hop_min, hmin);
            atomicMax(&S->hop_max, hmax);
            atomicMin(&S->lat_min, lmin);
            atomicMax(&S->lat_max, lmax);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && hist[threadIdx.x]) atomicAdd(&S->hist[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
    if (threadIdx.x < 8 && stat[threadIdx.x]) atomicAdd(&S->status[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
}

// a grid-stride launch: enough blocks for n items, at most 8 per CU
unsigned rpc_blocks(uint64_t n, int num_cu)
{
    uint64_t blocks = (n + 255) / 256;
    const uint64_t cap = (uint64_t)(num_cu > 0 ? num_cu : 1) * 8;
    return (unsigned)(blocks > cap ? cap : blocks);
}

}  // namespace

hipError_t launch_rpc_finish(const ovs_route_out* route, const uint32_t* src, const KeyRec* recs, const double2* xy,
                             const RpcConsts& RC, uint64_t n, ovs_rpc_out* out, K160* rkeys, uint32_t* rsrc,
                             int num_cu, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (RC.nnodes == 0 || (RC.full && (!rkeys || !rsrc))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rpc_finish, dim3(rpc_blocks(n, num_cu)), dim3(256), 0, s, route, src, recs, xy, RC, n, out,
                       rkeys, rsrc);
    return hipGetLastError();
}

hipError_t launch_rpc_fold(const ovs_route_out* ret, const uint32_t* src, const RpcConsts& RC, uint64_t n,
                           ovs_rpc_out* out, int num_cu, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rpc_fold, dim3(rpc_blocks(n, num_cu)), dim3(256), 0, s, ret, src, RC, n, out);
    return hipGetLastError();
}

hipError_t launch_rpc_stats(const ovs_rpc_out* out, const K160* keys, const uint32_t* src, const KeyRec* recs,
                            uint64_t n, uint32_t nnodes, int lookup_node_ids, RpcStatsDev* S, uint32_t* node_counts,
                            int num_cu, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(node_counts, 0, sizeof(uint32_t) * 3 * (uint64_t)nnodes, s);
    if (e != hipSuccess) return e;
    RpcStatsDev init{};
    init.hop_min = ~0ull;
    init.lat_min = ~0ull;
    e = hipMemcpyAsync(S, &init, sizeof init, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_kbrtest_rpc_stats, dim3(rpc_blocks(n, num_cu)), dim3(256), 0, s, out, keys, src, recs, n,
                       nnodes, lookup_node_ids, S, node_counts, node_counts + nnodes,
                       node_counts + 2 * (uint64_t)nnodes);
    return hipGetLastError();
}

}  // namespace ovs
