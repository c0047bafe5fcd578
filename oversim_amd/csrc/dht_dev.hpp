// dht_dev.hpp -- what the DHT kernels (dht.hip, dht_teams.hip) share on the device: the message lengths of
// DHTMessage.msg:30-41, the storage's tag and read-only probe, and the sender's side of
// SimpleNodeEntry::calcDelay.  Every function is forced inline or a plain device function without state.
#pragma once
#include "dht.hpp"
#include "tier_dev.hpp"

namespace ovs {

constexpr int64_t DHT_NEVER = INT64_MAX;
constexpr int BASERPC_BITS = 256;      // BASERPC_L (CommonMessages.msg:69-70)
constexpr int ENTRY_BITS = 608;        // KEY_L + KIND_L + ID_L + SEQNO_L + TTL_L + KEY_L + PUBKEY_L (DHTMessage.msg:30-37)
constexpr int GETCALL_BITS = BASERPC_BITS + 160 + 32 + 32 + 1;   // GETCALL_L (DHTMessage.msg:38)
constexpr int HASH_BITS = 20;          // a SHA-1 BinaryValue's size(), added as bits (DHTMessage.msg:40)

__device__ __forceinline__ int bits_bytes(int bits) { return (bits + 7) >> 3; }            // cPacket::getByteLength
__device__ __forceinline__ int wire_bytes(int bits) { return bits_bytes(28 * 8 + 40 + bits); }   // + UDP/IP + BASEAPPDATA_L

__device__ __forceinline__ uint64_t entry_tag(uint32_t node, const K160& k, uint32_t kind, uint32_t id)
{
    uint64_t h = mix64(((uint64_t)node << 32 | k.w[0]) + 0x9e3779b97f4a7c15ull);
    h = mix64(h ^ ((uint64_t)k.w[1] << 32 | k.w[2]));
    h = mix64(h ^ ((uint64_t)k.w[3] << 32 | k.w[4]));
    h = mix64(h ^ ((uint64_t)kind << 32 | id));
    return h ? h : 1;
}

__device__ __forceinline__ bool slot_is(const DhtSlot* s, uint32_t node, const K160& k, uint32_t kind, uint32_t id)
{
    return s->node == node && s->kind == kind && s->id == id && words_are_key(s->key, k);
}

// read-only probe: the entry's slot, or NONE
__device__ inline uint32_t dht_find(const DhtStore& st, uint64_t tag)
{
    uint64_t p = tag % st.cap;
    for (uint64_t step = 0; step < st.cap; ++step) {
        const unsigned long long t = st.slots[p].tag;
        if (t == tag) return (uint32_t)p;
        if (t == 0) return NONE;
        p = p + 1 == st.cap ? 0 : p + 1;
    }
    return NONE;
}

// the sender's side of SimpleNodeEntry::calcDelay: txfin is the sender's tx.finished (SimpleNodeEntry.cc:164-194)
__device__ __forceinline__ int64_t dht_send(int64_t& txfin, uint32_t a, uint32_t b, int wire, int64_t now,
                                            const double2* __restrict__ xy, const DhtConsts& C)
{
    if (a == b) return now;                                   // SimpleUDP.cc:322
    const int64_t bw = bw_ns(wire, C.datarate, C.round);
    txfin = (txfin > now ? txfin : now) + bw;
    const double2 pa = xy[a], pb = xy[b];
    return txfin + C.access + coord_ns(pa.x, pa.y, pb.x, pb.y, C.round) + bw + C.access;
}

}  // namespace ovs
