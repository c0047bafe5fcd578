// host_checks.hpp -- the entry points' refusals that depend on plain values only (internal).  No HIP and no
// context: a check returns the call's status and leaves the message in *err for fail(c, st, err); the
// engine's limits come in as arguments.  tests/host_checks_driver.cpp pins every status and message.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/ovs_kbr.h"

namespace ovs {

inline ovs_status refusal(ovs_status st, const char* msg, std::string* err)
{
    *err = msg;
    return st;
}

// The arc map of a shard step: nshards + 1 non-decreasing bounds covering [0, n), one of whose arcs is the
// context's [lo, hi).  Copies the bounds out and leaves that arc's index in *me.
inline ovs_status check_arc_map(const uint64_t* shard_lo, uint32_t nshards, uint64_t n, uint64_t lo, uint64_t hi,
                                uint64_t* bounds, int* me, std::string* err)
{
    for (uint32_t r = 0; r <= nshards; ++r) {
        bounds[r] = shard_lo[r];
        if (r > 0 && shard_lo[r] < shard_lo[r - 1]) return refusal(OVS_EINVAL, "shard_lo must be non-decreasing", err);
    }
    if (shard_lo[0] != 0 || shard_lo[nshards] != n) return refusal(OVS_EINVAL, "shard_lo must cover [0, n)", err);
    *me = -1;
    for (uint32_t r = 0; r < nshards; ++r)
        if (shard_lo[r] == lo && shard_lo[r + 1] == hi) *me = (int)r;
    return *me < 0 ? refusal(OVS_EINVAL, "this context's arc is not one of shard_lo's arcs", err) : OVS_OK;
}

// The shapes of Kademlia tables a loader takes (kmax: the largest k the kernels implement).  b1: the refusal of
// a loader that takes b = 1 kademlia buckets only; nullptr: the CSR loader, which takes every b and bucketType.
inline ovs_status check_kad_shape(const ovs_params& P, const char* b1, int kmax, std::string* err)
{
    const bool ks_bad = P.k < 1 || P.k > kmax || P.s < 1 || 5 * P.s > 64;
    if (b1) {
        if (P.b != 1 || P.bucketType != 0) return refusal(OVS_ENOTSUP, b1, err);
        return ks_bad ? refusal(OVS_ENOTSUP, "Kademlia k must be 1..16 (two 96 B bucket blocks) and 5*s <= 64", err) : OVS_OK;
    }
    if (P.b < 1 || P.b > 5) return refusal(OVS_ENOTSUP, "Kademlia b must be 1..5 (numBuckets <= 992)", err);
    if (P.bucketType < 0 || P.bucketType > 2) return refusal(OVS_EINVAL, "bucketType must be 0..2 (kademlia, nkademlia, nr128)", err);
    // routingBucketSize counts indices as if b = 1 (Kademlia.cc:400-406): for b > 1 the indices past
    // 159 get sizes 2^8 .. 2^30 and then (int)pow(2, >= 31) -- undefined, not followed
    if (P.bucketType == 2 && P.b != 1) return refusal(OVS_ENOTSUP, "nr128 buckets need b = 1", err);
    if (P.bucketType == 2 && (P.extraNodesFinalBucket < 0 || P.extraNodesFinalBucket > 511))
        return refusal(OVS_ENOTSUP, "nr128: extraNodesFinalBucket must be 0..511", err);
    return ks_bad ? refusal(OVS_ENOTSUP, "Kademlia k must be 1..16 and 5*s <= 64", err) : OVS_OK;
}

// Kademlia::routingBucketSize (Kademlia.cc:384-411) for keys of keybits bits; 0 = no maximum (nkademlia)
inline int kad_bucket_size_host(const ovs_params& P, int index, int keybits)
{
    if (P.bucketType == 1) return 0;
    if (P.bucketType == 2) {
        const int extra = P.extraNodesFinalBucket == 0 ? keybits : P.extraNodesFinalBucket;   // 146-148
        const int offset = (int)(std::log((double)extra) / std::log(2.0)) - (keybits - (index + 1));
        if (offset > 0 && (1 << offset) > P.k) return 1 << offset;
    }
    return P.k;
}

// what a table builder's bad code says of `node` (kad_build_explicit; csr: kad_build_general, whose buckets
// follow routingBucketSize / routingBucketIndex)
inline std::string kad_table_error(bool csr, uint32_t node, uint32_t code)
{
    static const char* const why[8] = {"", "sibling index out of range or the node itself", "sibling listed twice",
                                       "bucket holds more than k entries", "bucket member out of range or the node itself",
                                       "bucket member in the wrong bucket (msb(member ^ node) != bucket index)",
                                       "bucket member listed twice", "node is both sibling and bucket member"};
    const char* w = code >= 8 ? "?" : why[code];
    if (csr && code == 3) w = "bucket holds more than routingBucketSize(i) entries";
    if (csr && code == 5) w = "bucket member in the wrong bucket (routingBucketIndex(member) != bucket index)";
    return std::string(csr ? "CSR" : "explicit") + " Kademlia tables of node " + std::to_string(node) + ": " + w;
}

// refresh lookups (ovs_kad_refresh_batch, ovs_kad_maintenance_round); a round bounds its redundancies above only
inline ovs_status check_refresh_redundant(int R, bool lower, std::string* err)
{
    return (lower && R < 1) || R > 64 ? refusal(OVS_ENOTSUP, "refresh lookups implement redundantNodes 1..64", err) : OVS_OK;
}

inline ovs_status check_refresh_params(const ovs_params& P, int max_alpha, std::string* err)
{
    if (P.hopCountMax < 1) return refusal(OVS_ENOTSUP, "refresh lookups need hopCountMax >= 1", err);
    if (!P.lookupMerge || !P.lookupStrictParallelRpcs || P.lookupParallelRpcs < 1 || P.lookupParallelRpcs > max_alpha)
        return refusal(OVS_ENOTSUP, "refresh lookups implement lookupMerge, strictParallelRpcs, parallelRpcs 1..8", err);
    if (P.lookupParallelPaths != 1 || P.lookupVerifySiblings || P.lookupMajoritySiblings || P.jitter != 0.0)
        return refusal(OVS_ENOTSUP, "parallelPaths 1, no verify/majority siblings, jitter 0", err);
    return OVS_OK;
}

// a host array of node indices: every one below n; *pos (if given) is the first that is not
inline ovs_status check_node_indices(const uint32_t* node, uint64_t m, uint64_t n, std::string* err, uint64_t* pos = nullptr)
{
    for (uint64_t i = 0; i < m; ++i)
        if (node[i] >= n) {
            if (pos) *pos = i;
            return refusal(OVS_EINVAL, "node index out of range", err);
        }
    return OVS_OK;
}

}  // namespace ovs
