// app_kbrtest.cpp -- KBRTestApp on the route seam: its three statistics calls and the RPC test.
#include <cstring>
#include <new>

#include "cstddev.hpp"
#include "ctx.hpp"
#include "kbr_rpc.hpp"
#include "stats.hpp"

using namespace ovs;

namespace ovs {

ovs_status stats_begin(ovs_ctx* c, double measured_time_s, double failure_latency_s, uint32_t flags, void* stream,
                       bool* dev, hipStream_t* s)
{
    if (!c->overlay) return fail(c, OVS_ESTATE, "no network loaded");
    if (!(measured_time_s >= 0)) return fail(c, OVS_EINVAL, "measured_time_s must be >= 0");
    if (!(failure_latency_s >= 0)) return fail(c, OVS_EINVAL, "failure_latency_s must be >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    *dev = flags & OVS_DEVICE_PTRS;
    *s = *dev ? (hipStream_t)stream : c->stream;   // NULL = the default stream
    return OVS_OK;
}

ovs_status stats_read(ovs_ctx* c, hipStream_t s, hipError_t e, void* sums, const void* dsums, size_t sums_bytes,
                      void* rows, const void* drows, size_t rows_bytes, const char* what)
{
    if (e == hipSuccess) e = hipMemcpyAsync(sums, dsums, sums_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(rows, drows, rows_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, what);
    return OVS_OK;
}

ovs_status node_counters(ovs_ctx* c, int rows, std::vector<uint32_t>& nc)
{
    try {
        nc.resize((uint64_t)rows * c->n);
    } catch (const std::bad_alloc&) {
        return fail(c, OVS_ENOMEM, "per-node counters");
    }
    return OVS_OK;
}

}  // namespace ovs

namespace {

// The statistics kernels over one staged batch: the scratch they reduce in, the launch, and the sums
// (h) and per-node reductions (r, NSTAT rows in CStdDev::from_row's layout) read back.
ovs_status run_stats(ovs_ctx* c, CallFrame& F, hipStream_t s, const ovs_route_out* dout, const K160* dk, const uint32_t* ds,
                     uint64_t n, int32_t lookup_node_ids, double measured_time_s, uint64_t msg_bytes, const uint32_t* dsib,
                     uint64_t sib_stride, StatsDev* h, double* r)
{
    StatsDev* S = F.scratch<StatsDev>(1);
    uint32_t* counts = F.scratch<uint32_t>(3 * c->n);
    double* partial = F.scratch<double>(STATS_NODE_BLOCKS * NSTAT * 5);
    double* result = F.scratch<double>(NSTAT * 5);
    if (!F.ok()) return frame_fail(c, F);
    // GlobalStatistics::MIN_MEASURED = 0.1 s (GlobalStatistics.cc:32, KBRTestApp.cc:502)
    const int rates = measured_time_s >= 0.1;
    const hipError_t e = launch_stats(dout, dk, ds, c->recs, n, (uint32_t)c->n, lookup_node_ids, measured_time_s, msg_bytes,
                                      rates, S, counts, partial, result, c->num_cu, s, dsib, sib_stride);
    return stats_read(c, s, e, h, S, sizeof *h, r, result, sizeof(double) * NSTAT * 5, "statistics kernels");
}

}  // namespace

extern "C" {

ovs_status ovs_kbrtest_stats_batch(ovs_ctx* c, const ovs_route_out* out, const ovs_key160* keys, const uint32_t* src,
                                   uint64_t n, double measured_time_s, int32_t lookup_node_ids,
                                   ovs_kbrtest_stats* stats, uint32_t flags, void* stream)
{
    if (!c || !stats || (n && (!out || !src || (lookup_node_ids && !keys)))) return OVS_EINVAL;
    bool dev;
    hipStream_t s;
    ovs_status st = stats_begin(c, measured_time_s, 0.0, flags, stream, &dev, &s);
    if (st != OVS_OK) return st;
    CallFrame F(dev || n == 0, s);                            // an empty batch has nothing to stage
    const ovs_route_out* dout = F.in(out, n);
    const uint32_t* ds = F.in(src, n);
    const K160* dk = dev || lookup_node_ids ? F.in(reinterpret_cast<const K160*>(keys), n) : nullptr;
    StatsDev h{};
    double r[NSTAT * 5];
    st = run_stats(c, F, s, dout, dk, ds, n, lookup_node_ids, measured_time_s, (uint64_t)c->P.testMsgSize, nullptr, 0, &h, r);
    if (st != OVS_OK) return st;

    ovs_kbrtest_stats& o = *stats;
    std::memset(&o, 0, sizeof o);
    const uint64_t B = (uint64_t)c->P.testMsgSize;
    o.num_sent = n;
    o.num_delivered = h.delivered;
    o.num_dropped = h.dropped;
    o.num_lookup_failed = h.failed;
    o.bytes_sent = n * B;
    o.bytes_delivered = h.delivered * B;
    o.bytes_dropped = h.dropped * B;
    o.hop_count_sum = h.hop_sum;
    o.latency_sum_ns = (int64_t)h.lat_sum;
    if (h.delivered) {
        o.hop_count_min = (uint32_t)h.hop_min;
        o.hop_count_max = (uint32_t)h.hop_max;
        o.latency_min_ns = (int64_t)h.lat_min;
        o.latency_max_ns = (int64_t)h.lat_max;
        // GlobalStatistics::finalizeStatistics: OutVector value / count (GlobalStatistics.cc:134-139);
        // latency values are SIMTIME_DBL(latency), summed here exactly in ns
        o.hop_count_mean = (double)h.hop_sum / (double)h.delivered;
        o.latency_mean_s = ((double)h.lat_sum / (double)h.delivered) * 1e-9;
    }
    for (int i = 0; i < 8; ++i) o.status_count[i] = h.status[i];
    for (int i = 0; i < 64; ++i) o.hop_hist[i] = h.hist[i];
    ovs_stddev* sd[NSTAT] = {&o.delivered_msgs_per_s, &o.delivered_bytes_per_s, &o.dropped_msgs_per_s,
                             &o.dropped_bytes_per_s, &o.delivery_ratio};
    for (int k = 0; k < NSTAT; ++k) CStdDev::from_row(r + 5 * k).finish(*sd[k]);
    return OVS_OK;
}

ovs_status ovs_kbrtest_lookup_stats_batch(ovs_ctx* c, const ovs_lookup_out* out, const uint32_t* siblings,
                                          int32_t siblings_stride, const ovs_key160* keys, const uint32_t* src,
                                          uint64_t n, double measured_time_s, int32_t lookup_node_ids,
                                          double failure_latency_s, ovs_kbrtest_lookup_stats* stats, uint32_t flags,
                                          void* stream)
{
    if (!c || !stats || siblings_stride < 1 || (n && (!out || !src || !siblings || (lookup_node_ids && !keys))))
        return OVS_EINVAL;
    bool dev;
    hipStream_t s;
    ovs_status st = stats_begin(c, measured_time_s, 0.0, flags, stream, &dev, &s);   // failure_latency_s: any value
    if (st != OVS_OK) return st;
    CallFrame F(dev || n == 0, s);                            // an empty batch has nothing to stage
    const ovs_route_out* dout = F.in(reinterpret_cast<const ovs_route_out*>(out), n);
    const uint32_t* ds = F.in(src, n);
    const uint32_t* dsib = F.in(siblings, n * (uint64_t)siblings_stride);
    const K160* dk = dev || lookup_node_ids ? F.in(reinterpret_cast<const K160*>(keys), n) : nullptr;
    StatsDev h{};
    double r[NSTAT * 5];
    st = run_stats(c, F, s, dout, dk, ds, n, lookup_node_ids, measured_time_s, 0, dsib ? dsib : src,
                   (uint64_t)siblings_stride, &h, r);
    if (st != OVS_OK) return st;

    ovs_kbrtest_lookup_stats& o = *stats;
    std::memset(&o, 0, sizeof o);
    o.num_sent = n;
    o.num_success = h.delivered;
    o.num_failed = h.dropped;
    o.num_invalid = h.failed;
    o.hop_count_sum = h.hop_sum;
    o.failed_hop_count_sum = h.fhop_sum;
    o.success_latency_sum_ns = (int64_t)h.lat_sum;
    if (h.delivered) {
        o.hop_count_min = (uint32_t)h.hop_min;
        o.hop_count_max = (uint32_t)h.hop_max;
        o.success_latency_min_ns = (int64_t)h.lat_min;
        o.success_latency_max_ns = (int64_t)h.lat_max;
        o.hop_count_mean = (double)h.hop_sum / (double)h.delivered;
        o.success_latency_mean_s = ((double)h.lat_sum / (double)h.delivered) * 1e-9;
    }
    if (h.dropped) o.failed_hop_count_mean = (double)h.fhop_sum / (double)h.dropped;
    if (n) o.total_latency_mean_s = ((double)h.lat_sum * 1e-9 + (double)h.dropped * failure_latency_s) / (double)n;
    for (int i = 0; i < 8; ++i) o.status_count[i] = h.status[i];
    for (int i = 0; i < 64; ++i) o.hop_hist[i] = h.hist[i];
    CStdDev::from_row(r + 5 * 0).finish(o.successful_lookups_per_s);
    CStdDev::from_row(r + 5 * 2).finish(o.failed_lookups_per_s);
    CStdDev::from_row(r + 5 * 4).finish(o.success_ratio);
    return OVS_OK;
}

// KBRTestApp RPC test (KBRTestApp.cc:172-189, 230-329): the call leg is the one-way route on this call's
// staged copies, so the route's refusals come first; k_rpc_finish adds the response leg and the timeout
// rule; full-recursive routing routes the responses back (BaseApp.cc:595-599) and folds them in.
// Everything is queued on one stream with no host synchronisation in between.
ovs_status ovs_rpc_batch(ovs_ctx* c, const ovs_key160* keys, const uint32_t* src, uint64_t n, ovs_rpc_out* out,
                         uint32_t flags, void* stream)
{
    static_assert(sizeof(ovs_rpc_out) == 32, "ovs_rpc_out is 32 B");
    if (!c || (!keys && n) || (!src && n) || (!out && n)) return OVS_EINVAL;
    const ovs_params& P = c->P;
    const bool dev = flags & OVS_DEVICE_PTRS;
    hipStream_t s = dev ? (hipStream_t)stream : c->stream;
    // the route's own refusals (no network, EpiChord, an arc of a sharded network, parameters), before
    // anything is staged
    ovs_status st = route_check(c, P, s);
    if (st != OVS_OK) return st;
    if (P.routingType == 4)
        return fail(c, OVS_ENOTSUP, "KbrTestCall under source-routing-recursive routing: the response follows the "
                                    "call's recorded hops back (BaseRpc.cc:576-584), which is not implemented");
    if (P.routingType < 0 || P.routingType > 2)
        return fail(c, OVS_ENOTSUP, "KbrTestCall is implemented for routingType iterative / semi-recursive / full-recursive");
    if (!(P.rpcKeyTimeout >= 0)) return fail(c, OVS_EINVAL, "rpcKeyTimeout must be >= 0");
    if (n == 0) return OVS_OK;
    st = check_sources(c, src, n, dev);
    if (st != OVS_OK) return st;
    const bool full = P.routingType == 2;
    CallFrame F(dev, s);
    const K160* dk = F.in(reinterpret_cast<const K160*>(keys), n);
    const uint32_t* ds = F.in(src, n);
    ovs_rpc_out* dout = F.out(out, n);
    if (!F.ok()) return frame_fail(c, F);
    // route records (16 B), and for the return route its keys (20 B) and sources (4 B), each part 256 B aligned
    const uint64_t o_keys = up256(sizeof(ovs_route_out) * n);
    const uint64_t o_src = o_keys + up256(sizeof(K160) * n);
    CachedBuf::Lease buf = c->rpcb.acquire(full ? o_src + sizeof(uint32_t) * n : o_keys, s);
    if (!buf) return lease_fail(c, "RPC buffers", buf);
    ovs_route_out* droute = reinterpret_cast<ovs_route_out*>(buf.data());
    K160* rkeys = full ? reinterpret_cast<K160*>(buf.data() + o_keys) : nullptr;
    uint32_t* rsrc = full ? reinterpret_cast<uint32_t*>(buf.data() + o_src) : nullptr;
    st = route_device(c, P, F, dk, ds, n, droute, nullptr, nullptr, s);
    if (st != OVS_OK) return st;
    RpcConsts RC{};
    const DelayConsts DC = delay_consts(P);
    RC.timeout = simtime_host(P.rpcKeyTimeout, P.simtimeRound);
    // KbrTestResponse in a BaseAppDataMessage straight over UDP: payload + BASEAPPDATA_L 40 bits + UDP/IP 28 B
    // (BaseOverlay.cc:1340-1341, CommonMessages.msg:68, SimpleUDP.cc:291)
    RC.respMsg = 2 * simtime_host((double)((int64_t)(P.testMsgSize + 5 + 28) * 8) / P.datarate, P.simtimeRound) + DC.access2;
    RC.round = P.simtimeRound;
    RC.full = full;
    RC.nnodes = (uint32_t)c->n;
    hipError_t e = launch_rpc_finish(droute, ds, c->recs, c->xy, RC, n, dout, rkeys, rsrc, c->num_cu, s);
    if (e != hipSuccess) return hip_fail(c, e, "RPC finish kernel");
    if (full) {
        // the return routes overwrite the call routes: what the fold needs of those is in dout
        st = route_device(c, P, F, rkeys, rsrc, n, droute, nullptr, nullptr, s);
        if (st != OVS_OK) return st;
        e = launch_rpc_fold(droute, ds, RC, n, dout, c->num_cu, s);
        if (e != hipSuccess) return hip_fail(c, e, "RPC fold kernel");
    }
    buf.release();
    if (F.finish() != hipSuccess) return frame_fail(c, F);
    return OVS_OK;
}

ovs_status ovs_kbrtest_rpc_stats_batch(ovs_ctx* c, const ovs_rpc_out* out, const ovs_key160* keys, const uint32_t* src,
                                       uint64_t n, double measured_time_s, int32_t lookup_node_ids,
                                       double failure_latency_s, ovs_kbrtest_rpc_stats* stats, uint32_t flags,
                                       void* stream)
{
    if (!c || !stats || (n && (!out || !src || (lookup_node_ids && !keys)))) return OVS_EINVAL;
    bool dev;
    hipStream_t s;
    ovs_status st = stats_begin(c, measured_time_s, failure_latency_s, flags, stream, &dev, &s);
    if (st != OVS_OK) return st;
    CallFrame F(dev || n == 0, s);                            // an empty batch has nothing to stage
    const ovs_rpc_out* dout = F.in(out, n);
    const uint32_t* ds = F.in(src, n);
    const K160* dk = dev || lookup_node_ids ? F.in(reinterpret_cast<const K160*>(keys), n) : nullptr;
    StatsDev* S = F.scratch<StatsDev>(1);
    uint32_t* counts = F.scratch<uint32_t>(3 * c->n);
    if (!F.ok()) return frame_fail(c, F);
    StatsDev h{};
    std::vector<uint32_t> nc;
    if ((st = node_counters(c, 3, nc)) != OVS_OK) return st;
    const hipError_t e = launch_rpc_stats(dout, dk, ds, c->recs, n, (uint32_t)c->n, lookup_node_ids, S, counts, c->num_cu, s);
    st = stats_read(c, s, e, &h, S, sizeof h, nc.data(), counts, sizeof(uint32_t) * nc.size(), "RPC statistics kernel");
    if (st != OVS_OK) return st;

    ovs_kbrtest_rpc_stats& o = *stats;
    std::memset(&o, 0, sizeof o);
    const uint64_t B = (uint64_t)c->P.testMsgSize;
    o.num_sent = n;
    o.num_delivered = h.delivered;
    o.num_dropped = h.dropped;
    o.num_timeout = h.failed;
    o.bytes_sent = n * B;
    o.bytes_delivered = h.delivered * B;
    o.bytes_dropped = h.dropped * B;
    o.hop_count_sum = h.hop_sum;
    o.success_latency_sum_ns = (int64_t)h.lat_sum;
    if (h.delivered) {
        o.hop_count_min = (uint32_t)h.hop_min;
        o.hop_count_max = (uint32_t)h.hop_max;
        o.success_latency_min_ns = (int64_t)h.lat_min;
        o.success_latency_max_ns = (int64_t)h.lat_max;
        o.hop_count_mean = (double)h.hop_sum / (double)h.delivered;
        o.success_latency_mean_s = ((double)h.lat_sum / (double)h.delivered) * 1e-9;
    }
    // "RPC Total Latency": rtt for delivered RPCs, failureLatency for the others (KBRTestApp.cc:262-263, 281-285, 306-310)
    if (n) o.total_latency_mean_s = ((double)h.lat_sum * 1e-9 + (double)h.dropped * failure_latency_s) / (double)n;
    for (int i = 0; i < 8; ++i) o.status_count[i] = h.status[i];
    for (int i = 0; i < 64; ++i) o.hop_hist[i] = h.hist[i];
    // KBRTestApp::finishApp (KBRTestApp.cc:519-545) at every node, in node order; only from
    // GlobalStatistics::MIN_MEASURED = 0.1 s on (502)
    if (measured_time_s >= 0.1) {
        CStdDev a[NSTAT];
        const uint64_t N = c->n;
        for (uint64_t v = 0; v < N; ++v) {
            const uint32_t sent = nc[v], d = nc[N + v], dr = nc[2 * N + v];
            a[0].collect((double)d / measured_time_s);
            a[1].collect((double)((uint64_t)d * B) / measured_time_s);
            a[2].collect((double)dr / measured_time_s);
            a[3].collect((double)((uint64_t)dr * B) / measured_time_s);
            if (sent > 0) a[4].collect((double)((float)d / (float)sent));
        }
        ovs_stddev* sd[NSTAT] = {&o.delivered_msgs_per_s, &o.delivered_bytes_per_s, &o.dropped_msgs_per_s,
                                 &o.dropped_bytes_per_s, &o.delivery_ratio};
        for (int k = 0; k < NSTAT; ++k) a[k].finish(*sd[k]);
    }
    return OVS_OK;
}

}  // extern "C"
