// app_dht.hpp -- what the DHT tier's translation units (app_dht.cpp, app_dht_teams.cpp) share on the host (internal).
#pragma once
#include <vector>

#include "ctx.hpp"

namespace ovs {

// the DHT tier's own refusals, then the LookupCall's (lookup_check) for dp->numReplica siblings
ovs_status dht_check(ovs_ctx* c, const ovs_dht_params* dp, hipStream_t s);
DhtConsts dht_consts(const ovs_ctx* c, const ovs_dht_params* dp);

// One launch of the DHTTestApp statistics kernel over device records (F: the call's frame): the integer sums
// and, with node_rows, the four per-node counter rows (without them the sources are read but never counted).
ovs_status dhttest_sums(ovs_ctx* c, CallFrame& F, const ovs_dht_put_out* dpo, const uint32_t* dps, uint64_t n_put,
                        const ovs_dht_get_out* dgo, const ovs_dht_op* dgp, const uint32_t* dgs, const ovs_dhttest_expect* dex,
                        uint64_t n_get, bool node_rows, hipStream_t s, DhtStatsDev* h, std::vector<uint32_t>* nc);
// the cStdDevs finished on the host, the per-node ones over N nodes in node order
void dhttest_finish(const DhtStatsDev& h, const std::vector<uint32_t>& nc, uint64_t N, double measured_time_s,
                    ovs_dhttest_stats* stats);

}  // namespace ovs
