/* Prints the layout of the DHT structs of include/ovs_kbr.h as JSON, compiled by a plain C compiler
 * against the header alone (tests/test_dht_model.py compares it with the Python mirrors in
 * oversim_amd/kbr.py), in the style of tests/abi_layout_rpc.c. */
#include <stddef.h>
#include <stdio.h>

#include "ovs_kbr.h"

#ifndef OVS_HAS_DHT
#error "include/ovs_kbr.h does not declare the DHT calls"
#endif

#define F(T, f) printf("%s\"%s\": %zu", first++ ? ", " : "", #f, offsetof(T, f))
#define OPEN(T) first = 0, printf(", \"" #T "\": {\"size\": %zu, \"fields\": {", sizeof(T))

int main(void)
{
    int first = 0;
    printf("{\"abi\": %d, \"outcomes\": [%d, %d, %d]", OVS_ABI_VERSION, (int)OVS_DHT_SUCCESS, (int)OVS_DHT_FAILED,
           (int)OVS_DHT_LOOKUP_FAILED);
    OPEN(ovs_dht_params);
    F(ovs_dht_params, numReplica); F(ovs_dht_params, numGetRequests); F(ovs_dht_params, ratioIdentical);
    F(ovs_dht_params, secureMaintenance); F(ovs_dht_params, invalidDataAttack); F(ovs_dht_params, maintenanceAttack);
    F(ovs_dht_params, pad);
    printf("}}");
    OPEN(ovs_dht_op);
    F(ovs_dht_op, t0_ns); F(ovs_dht_op, token); F(ovs_dht_op, kind); F(ovs_dht_op, id); F(ovs_dht_op, vlen);
    F(ovs_dht_op, ttl);
    printf("}}");
    OPEN(ovs_dht_put_out);
    F(ovs_dht_put_out, latency_ns); F(ovs_dht_put_out, bytes); F(ovs_dht_put_out, hop_count);
    F(ovs_dht_put_out, messages); F(ovs_dht_put_out, outcome); F(ovs_dht_put_out, status);
    F(ovs_dht_put_out, num_sent); F(ovs_dht_put_out, num_responses); F(ovs_dht_put_out, pad);
    printf("}}");
    OPEN(ovs_dht_get_out);
    F(ovs_dht_get_out, latency_ns); F(ovs_dht_get_out, bytes); F(ovs_dht_get_out, hop_count);
    F(ovs_dht_get_out, messages); F(ovs_dht_get_out, outcome); F(ovs_dht_get_out, status);
    F(ovs_dht_get_out, num_sent); F(ovs_dht_get_out, num_responses); F(ovs_dht_get_out, result_count);
    F(ovs_dht_get_out, value_token); F(ovs_dht_get_out, value_len); F(ovs_dht_get_out, server);
    printf("}}");
    OPEN(ovs_dht_entry);
    F(ovs_dht_entry, key); F(ovs_dht_entry, kind); F(ovs_dht_entry, id); F(ovs_dht_entry, vlen);
    F(ovs_dht_entry, token); F(ovs_dht_entry, expiry_ns);
    printf("}}");
    OPEN(ovs_dhttest_expect);
    F(ovs_dhttest_expect, token); F(ovs_dhttest_expect, endtime_ns); F(ovs_dhttest_expect, known); F(ovs_dhttest_expect, pad);
    printf("}}");
    OPEN(ovs_dhttest_stats);
    F(ovs_dhttest_stats, num_put_success); F(ovs_dhttest_stats, num_put_error); F(ovs_dhttest_stats, num_get_success);
    F(ovs_dhttest_stats, num_get_error); F(ovs_dhttest_stats, put_latency_sum_ns); F(ovs_dhttest_stats, put_latency_sumsq_lo);
    F(ovs_dhttest_stats, put_latency_sumsq_hi); F(ovs_dhttest_stats, get_latency_sum_ns); F(ovs_dhttest_stats, get_latency_sumsq_lo);
    F(ovs_dhttest_stats, get_latency_sumsq_hi); F(ovs_dhttest_stats, put_latency_min_ns); F(ovs_dhttest_stats, put_latency_max_ns);
    F(ovs_dhttest_stats, get_latency_min_ns); F(ovs_dhttest_stats, get_latency_max_ns); F(ovs_dhttest_stats, get_latency_count);
    F(ovs_dhttest_stats, put_hop_count); F(ovs_dhttest_stats, put_hop_sum); F(ovs_dhttest_stats, get_hop_count);
    F(ovs_dhttest_stats, get_hop_sum); F(ovs_dhttest_stats, normal_messages); F(ovs_dhttest_stats, num_bytes_normal);
    F(ovs_dhttest_stats, put_latency_s); F(ovs_dhttest_stats, get_latency_s); F(ovs_dhttest_stats, put_success_per_s);
    F(ovs_dhttest_stats, put_error_per_s); F(ovs_dhttest_stats, get_success_per_s); F(ovs_dhttest_stats, get_error_per_s);
    F(ovs_dhttest_stats, get_success_ratio);
    printf("}}}\n");
    return 0;
}
