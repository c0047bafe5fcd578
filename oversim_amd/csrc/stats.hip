// stats.hip -- KBRTestApp statistics over a batch of results of the one-way, lookup or RPC test.
//
// Reference: KBRTestApp::deliver / evaluateData / finishApp (KBRTestApp.cc:380-520),
// handleRpcResponse / handleRpcTimeout / handleLookupResponse (KBRTestApp.cc:237-371),
// SendToKeyListener::lookupFinished failure branch (BaseOverlay.cc:1258-1270),
// GlobalStatistics::addStdDev / recordOutVector / finalizeStatistics
// (GlobalStatistics.cc:103-200).  OMNeT++'s cStdDev is not in the image; its
// published accumulator (count, sum, sum of squares, min, max) is restated here.
//
// Pass 1 (k_stats_lookups<Reader>): one thread per record, grid-stride.  Integer
// counters only, so the result is independent of scheduling: register
// accumulation -> wave reduction -> one global atomic per wave; per-node
// sent/delivered/dropped counts by global atomics; hop histogram in LDS.  The
// one-way, lookup and RPC tests differ in the record they read (the readers below).
// Pass 2 (k_stats_nodes): per-node rates folded into cStdDev accumulators in
// a FIXED order (fixed grid, fixed stride, fixed tree), so the fp64 sums are
// deterministic run to run.  Pass 3 (k_stats_final): one block folds the
// per-block partials in index order.  The RPC test takes pass 1 alone.
// All passes are HBM-streaming (20 B per lookup + 12 B per node) and tiny
// next to the route kernels.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "stats.hpp"
#include "tier_dev.hpp"

namespace ovs {

namespace {

// what pass 1 counts of one record
struct StatsRec {
    uint32_t status;    // the lookup status byte
    bool early;         // one-way test: a failed lookup, nothing else is counted
    bool ok;            // delivered, as far as the record says (before the key check)
    uint32_t node;      // lookupNodeIds: the node whose key must equal the destination key
    uint64_t hops, lat; // what a delivered record adds to the sums
    uint64_t extra;     // what any record adds to StatsDev::failed
};

// One-way test over ovs_route_out: delivered / dropped / failed lookups.  A failed lookup is
// SendToKeyListener::lookupFinished's failure branch (BaseOverlay.cc:1258-1270); the key check is
// KBRTestApp::deliver: getThisNode().getKey() == destKey (KBRTestApp.cc:407).
struct OneWayReader {
    static constexpr bool FAILED_HOPS = false;
    const ovs_route_out* __restrict__ out;
    __device__ __forceinline__ StatsRec read(uint64_t i, int) const
    {
        const ovs_route_out o = out[i];
        const bool failed = o.status != OVS_LOOKUP_OK;
        return {o.status, failed, true, o.responsible, o.one_way_hops, (uint64_t)o.latency_ns, failed ? 1u : 0u};
    }
};

// Lookup test over ovs_lookup_out and the first column of the sibling vectors: delivered =
// numLookupSuccess, dropped = numLookupFailed, failed = the !isValid part of it (KBRTestApp.cc:331-371).
// KBRTestApp::handleLookupResponse: isValid && (!lookupNodeIds || (siblings non-empty,
// siblings[0].key == key, siblings[0] == destAddr)) -- unique IDs: the node owning key.  hops is the
// "Lookup Hop Count" (a failed lookup's: "Failed Lookup Hop Count"), lat the "Lookup Success Latency".
struct LookupReader {
    static constexpr bool FAILED_HOPS = true;
    const ovs_lookup_out* __restrict__ out;
    const uint32_t* __restrict__ first;
    uint64_t first_stride;
    __device__ __forceinline__ StatsRec read(uint64_t i, int lookup_node_ids) const
    {
        const ovs_lookup_out o = out[i];
        const bool valid = o.is_valid != 0;
        const uint32_t f = valid && lookup_node_ids && o.num_siblings > 0 ? first[i * first_stride] : NONE;
        return {o.status, false, valid, f, o.hops, (uint64_t)o.latency_ns, valid ? 0u : 1u};
    }
};

// RPC test over ovs_rpc_out: failed counts the timeouts (handleRpcTimeout, KBRTestApp.cc:294-329), the key
// check is KBRTestApp.cc:254-256: destKey == srcNode.getKey() && destAddr == srcNode (unique IDs); hops
// is the "RPC Hop Count", lat the "RPC Success Latency".
struct RpcReader {
    static constexpr bool FAILED_HOPS = false;
    const ovs_rpc_out* __restrict__ out;
    __device__ __forceinline__ StatsRec read(uint64_t i, int) const
    {
        const ovs_rpc_out o = out[i];
        const bool answered = o.outcome == OVS_RPC_ANSWERED;
        return {o.status, false, answered, o.responder, o.hop_count, (uint64_t)o.rtt_ns, answered ? 0u : 1u};
    }
};

// a lane's sums of pass 1
struct StatsAcc {
    uint64_t deliv = 0, drop = 0, failed = 0, hops = 0, lat = 0, fhops = 0;
    uint64_t hmin = ~0ull, hmax = 0, lmin = ~0ull, lmax = 0;
};

// the end of pass 1, called by the whole block: the lanes' sums reduced per wave and added by one
// lane (minima and maxima only from a wave that delivered something), then the block's LDS counters
__device__ __forceinline__ void stats_flush(StatsAcc a, const uint32_t* hist, const uint32_t* stat, StatsDev* __restrict__ S)
{
    a.deliv = wave_sum_u64(a.deliv);
    a.drop = wave_sum_u64(a.drop);
    a.failed = wave_sum_u64(a.failed);
    a.hops = wave_sum_u64(a.hops);
    a.lat = wave_sum_u64(a.lat);
    a.fhops = wave_sum_u64(a.fhops);
    a.hmin = wave_min_u64(a.hmin);
    a.hmax = wave_max_u64(a.hmax);
    a.lmin = wave_min_u64(a.lmin);
    a.lmax = wave_max_u64(a.lmax);
    if ((threadIdx.x & 63) == 0) {
        if (a.deliv) atomicAdd(&S->delivered, a.deliv);
        if (a.drop) atomicAdd(&S->dropped, a.drop);
        if (a.failed) atomicAdd(&S->failed, a.failed);
        if (a.hops) atomicAdd(&S->hop_sum, a.hops);
        if (a.lat) atomicAdd(&S->lat_sum, a.lat);
        if (a.fhops) atomicAdd(&S->fhop_sum, a.fhops);
        if (a.hmin != ~0ull) {
            atomicMin(&S->hop_min, a.hmin);
            atomicMax(&S->hop_max, a.hmax);
            atomicMin(&S->lat_min, a.lmin);
            atomicMax(&S->lat_max, a.lmax);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && hist[threadIdx.x]) atomicAdd(&S->hist[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
    if (threadIdx.x < 8 && stat[threadIdx.x]) atomicAdd(&S->status[threadIdx.x], (unsigned long long)stat[threadIdx.x]);
}

template <class Reader>
__global__ __launch_bounds__(256) void k_stats_lookups(Reader rd, const K160* __restrict__ keys,
                                                       const uint32_t* __restrict__ src,
                                                       const KeyRec* __restrict__ recs, uint64_t n, uint32_t nnodes,
                                                       int lookup_node_ids, StatsDev* __restrict__ S,
                                                       uint32_t* __restrict__ node_sent,
                                                       uint32_t* __restrict__ node_deliv,
                                                       uint32_t* __restrict__ node_drop)
{
    __shared__ uint32_t hist[64];
    __shared__ uint32_t stat[8];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    if (threadIdx.x < 8) stat[threadIdx.x] = 0;
    __syncthreads();

    StatsAcc a;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const StatsRec r = rd.read(i, lookup_node_ids);
        const uint32_t s = src[i];
        const bool valid_src = s < nnodes;     // device-pointer calls do not check sources: counted in the sums only
        atomicAdd(&stat[r.status & 7], 1u);
        if (valid_src) atomicAdd(&node_sent[s], 1u);
        a.failed += r.extra;
        if (r.early) continue;
        bool ok = r.ok;
        if (ok && lookup_node_ids) ok = r.node < nnodes && rec_is_key(load_rec(recs, r.node), keys[i]);
        if (!ok) {
            ++a.drop;
            if constexpr (Reader::FAILED_HOPS) a.fhops += r.hops;
            if (valid_src) atomicAdd(&node_drop[s], 1u);
            continue;
        }
        ++a.deliv;
        if (valid_src) atomicAdd(&node_deliv[s], 1u);
        const uint64_t h = r.hops, l = r.lat;
        a.hops += h;
        a.lat += l;
        a.hmin = h < a.hmin ? h : a.hmin;
        a.hmax = h > a.hmax ? h : a.hmax;
        a.lmin = l < a.lmin ? l : a.lmin;
        a.lmax = l > a.lmax ? l : a.lmax;
        atomicAdd(&hist[h < 63 ? h : 63], 1u);
    }
    stats_flush(a, hist, stat, S);
}

// cStdDev accumulator (OMNeT++ cStdDev::collect: n, sum, sqrsum, min, max)
struct Acc {
    double sum, sq, mn, mx;
    uint64_t n;
};

__device__ __forceinline__ void acc_init(Acc& a)
{
    a.sum = 0; a.sq = 0; a.mn = __longlong_as_double(0x7FF0000000000000ll); a.mx = -a.mn; a.n = 0;
}

__device__ __forceinline__ void acc_add(Acc& a, double v)
{
    a.sum = __dadd_rn(a.sum, v);
    a.sq = __dadd_rn(a.sq, __dmul_rn(v, v));
    a.mn = v < a.mn ? v : a.mn;
    a.mx = v > a.mx ? v : a.mx;
    ++a.n;
}

__device__ __forceinline__ void acc_merge(Acc& a, const Acc& b)
{
    a.sum = __dadd_rn(a.sum, b.sum);
    a.sq = __dadd_rn(a.sq, b.sq);
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.n += b.n;
}

__device__ __forceinline__ void acc_store(double* p, const Acc& a)
{
    p[0] = a.sum; p[1] = a.sq; p[2] = a.mn; p[3] = a.mx; p[4] = __longlong_as_double((long long)a.n);
}

__device__ __forceinline__ void acc_load(const double* p, Acc& a)
{
    a.sum = p[0]; a.sq = p[1]; a.mn = p[2]; a.mx = p[3]; a.n = (uint64_t)__double_as_longlong(p[4]);
}

// fixed-shape tree reduction of NSTAT accumulators over a 256-thread block
__device__ void block_reduce_store(Acc (&a)[NSTAT], double* __restrict__ dst)
{
    __shared__ double sh[NSTAT * 5][256];
#pragma unroll
    for (int k = 0; k < NSTAT; ++k) {
        sh[k * 5 + 0][threadIdx.x] = a[k].sum;
        sh[k * 5 + 1][threadIdx.x] = a[k].sq;
        sh[k * 5 + 2][threadIdx.x] = a[k].mn;
        sh[k * 5 + 3][threadIdx.x] = a[k].mx;
        sh[k * 5 + 4][threadIdx.x] = __longlong_as_double((long long)a[k].n);
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < NSTAT; ++k) {
                Acc x, y;
                x.sum = sh[k * 5 + 0][threadIdx.x]; y.sum = sh[k * 5 + 0][threadIdx.x + w];
                x.sq = sh[k * 5 + 1][threadIdx.x]; y.sq = sh[k * 5 + 1][threadIdx.x + w];
                x.mn = sh[k * 5 + 2][threadIdx.x]; y.mn = sh[k * 5 + 2][threadIdx.x + w];
                x.mx = sh[k * 5 + 3][threadIdx.x]; y.mx = sh[k * 5 + 3][threadIdx.x + w];
                x.n = (uint64_t)__double_as_longlong(sh[k * 5 + 4][threadIdx.x]);
                y.n = (uint64_t)__double_as_longlong(sh[k * 5 + 4][threadIdx.x + w]);
                acc_merge(x, y);
                sh[k * 5 + 0][threadIdx.x] = x.sum;
                sh[k * 5 + 1][threadIdx.x] = x.sq;
                sh[k * 5 + 2][threadIdx.x] = x.mn;
                sh[k * 5 + 3][threadIdx.x] = x.mx;
                sh[k * 5 + 4][threadIdx.x] = __longlong_as_double((long long)x.n);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < NSTAT * 5) dst[threadIdx.x] = sh[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void k_stats_nodes(const uint32_t* __restrict__ node_sent,
                                                     const uint32_t* __restrict__ node_deliv,
                                                     const uint32_t* __restrict__ node_drop, uint32_t nnodes,
                                                     double time_s, uint64_t msg_bytes, int rates, int lk,
                                                     double* __restrict__ partial)
{
    Acc a[NSTAT];
#pragma unroll
    for (int k = 0; k < NSTAT; ++k) acc_init(a[k]);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nnodes; i += stride) {
        const uint32_t s = node_sent[i], d = node_deliv[i], r = node_drop[i];
        if (rates && lk) {
            // KBRTestApp::finishApp, kbrLookupTest (KBRTestApp.cc:546-557): Successful Lookups/s,
            // Failed Lookups/s, Lookup Success Ratio
            acc_add(a[0], __ddiv_rn((double)d, time_s));
            acc_add(a[2], __ddiv_rn((double)r, time_s));
            if (s > 0) acc_add(a[4], (double)__fdiv_rn((float)d, (float)s));
        } else if (rates) {
            // KBRTestApp::finishApp (KBRTestApp.cc:503-512): numDelivered / time etc.
            // (the reference divides long / simtime_t; as doubles here)
            acc_add(a[0], __ddiv_rn((double)d, time_s));
            acc_add(a[1], __ddiv_rn((double)((uint64_t)d * msg_bytes), time_s));
            acc_add(a[2], __ddiv_rn((double)r, time_s));
            acc_add(a[3], __ddiv_rn((double)((uint64_t)r * msg_bytes), time_s));
            if (s > 0) acc_add(a[4], (double)__fdiv_rn((float)d, (float)s));
        }
    }
    block_reduce_store(a, partial + (uint64_t)blockIdx.x * NSTAT * 5);
}

__global__ __launch_bounds__(256) void k_stats_final(const double* __restrict__ partial, int nblocks,
                                                     double* __restrict__ result)
{
    Acc a[NSTAT];
#pragma unroll
    for (int k = 0; k < NSTAT; ++k) acc_init(a[k]);
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
#pragma unroll
        for (int k = 0; k < NSTAT; ++k) {
            Acc x;
            acc_load(partial + ((uint64_t)b * NSTAT + k) * 5, x);
            acc_merge(a[k], x);
        }
    }
    block_reduce_store(a, result);
}

// pass 1 of any of the three tests: the counters initialised (both minima at ~0), then the kernel
template <class Reader>
hipError_t launch_lookups(Reader rd, const K160* keys, const uint32_t* src, const KeyRec* recs, uint64_t n,
                          uint32_t nnodes, int lookup_node_ids, StatsDev* S, uint32_t* node_counts, int num_cu,
                          hipStream_t st)
{
    StatsDev init{};
    init.hop_min = ~0ull;
    init.lat_min = ~0ull;
    const hipError_t e = stats_prelude(node_counts, 3, nnodes, S, init, st);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(k_stats_lookups<Reader>, dim3(capped_grid(n, 256, num_cu, 8)), dim3(256), 0, st, rd, keys, src,
                       recs, n, nnodes, lookup_node_ids, S, node_counts, node_counts + nnodes,
                       node_counts + 2 * (uint64_t)nnodes);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_stats(const ovs_route_out* out, const K160* keys, const uint32_t* src, const KeyRec* recs,
                        uint64_t n, uint32_t nnodes, int lookup_node_ids, double time_s, uint64_t msg_bytes,
                        int rates, StatsDev* S, uint32_t* node_counts, double* partial, double* result,
                        int num_cu, hipStream_t st, const uint32_t* first, uint64_t first_stride)
{
    const bool lk = first != nullptr;
    hipError_t e =
        lk ? launch_lookups(LookupReader{reinterpret_cast<const ovs_lookup_out*>(out), first, first_stride}, keys, src,
                            recs, n, nnodes, lookup_node_ids, S, node_counts, num_cu, st)
           : launch_lookups(OneWayReader{out}, keys, src, recs, n, nnodes, lookup_node_ids, S, node_counts, num_cu, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_stats_nodes, dim3(STATS_NODE_BLOCKS), dim3(256), 0, st, node_counts, node_counts + nnodes,
                       node_counts + 2 * (uint64_t)nnodes, nnodes, time_s, msg_bytes, rates, lk ? 1 : 0, partial);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_stats_final, dim3(1), dim3(256), 0, st, partial, STATS_NODE_BLOCKS, result);
    return hipGetLastError();
}

hipError_t launch_rpc_stats(const ovs_rpc_out* out, const K160* keys, const uint32_t* src, const KeyRec* recs,
                            uint64_t n, uint32_t nnodes, int lookup_node_ids, StatsDev* S, uint32_t* node_counts,
                            int num_cu, hipStream_t s)
{
    return launch_lookups(RpcReader{out}, keys, src, recs, n, nnodes, lookup_node_ids, S, node_counts, num_cu, s);
}

}  // namespace ovs
