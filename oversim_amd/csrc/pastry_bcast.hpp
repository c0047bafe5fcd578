// pastry_bcast.hpp -- host launcher of the Pastry broadcast level kernels (pastry_bcast.hip; internal).  The
// queue, its items, the control words, the fill / init / statistics launches are the Chord broadcast's
// (chord_bcast.hpp): only the level differs.
#pragma once
#include "chord_bcast.hpp"
#include "pastry.hpp"

namespace ovs {

// one level: Pastry::forwardBroadcast at queue[lo .. hi), children appended at ctl[0].  An item's `limit` is the
// first routing-table row it forwards from (an initiator, hops 0, forwards from row 0 whatever its limit holds).
// wave_per_item: a wave shares one node's slots (few nodes, up to hundreds of children each); else one lane per
// node.  xy: the coordinates of the t.n nodes.
hipError_t launch_pastry_bcast_level(const PastryTables& t, const double2* xy, const BcastConsts& BC, BcastItem* queue,
                                     uint64_t lo, uint64_t hi, uint64_t cap, ovs_bcast_node* nodes, unsigned long long* ctl,
                                     bool wave_per_item, hipStream_t s);

}  // namespace ovs
