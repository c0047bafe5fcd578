/* Prints the layout of the KBRTestApp RPC-test structs of include/ovs_kbr.h as JSON, compiled by a plain
 * C compiler against the header alone (tests/test_rpc_abi.py compares it with the Python mirrors in
 * oversim_amd/kbr.py), in the style of tests/abi_layout_broadcast.c. */
#include <stddef.h>
#include <stdio.h>

#include "ovs_kbr.h"

#ifndef OVS_HAS_KBR_RPC_TEST
#error "include/ovs_kbr.h does not declare the KBRTestApp RPC test"
#endif

#define F(T, f) printf("%s\"%s\": %zu", first++ ? ", " : "", #f, offsetof(T, f))

int main(void)
{
    int first = 0;
    printf("{\"abi\": %d, \"answered\": %d, \"timeout\": %d, \"ovs_rpc_out\": {\"size\": %zu, \"fields\": {",
           OVS_ABI_VERSION, (int)OVS_RPC_ANSWERED, (int)OVS_RPC_TIMEOUT, sizeof(ovs_rpc_out));
    F(ovs_rpc_out, responder); F(ovs_rpc_out, hop_count); F(ovs_rpc_out, call_hops); F(ovs_rpc_out, status);
    F(ovs_rpc_out, outcome); F(ovs_rpc_out, resp_status); F(ovs_rpc_out, pad); F(ovs_rpc_out, rtt_ns);
    F(ovs_rpc_out, call_latency_ns);
    first = 0;
    printf("}}, \"ovs_kbrtest_rpc_stats\": {\"size\": %zu, \"fields\": {", sizeof(ovs_kbrtest_rpc_stats));
    F(ovs_kbrtest_rpc_stats, num_sent); F(ovs_kbrtest_rpc_stats, num_delivered); F(ovs_kbrtest_rpc_stats, num_dropped);
    F(ovs_kbrtest_rpc_stats, num_timeout); F(ovs_kbrtest_rpc_stats, bytes_sent); F(ovs_kbrtest_rpc_stats, bytes_delivered);
    F(ovs_kbrtest_rpc_stats, bytes_dropped); F(ovs_kbrtest_rpc_stats, hop_count_sum);
    F(ovs_kbrtest_rpc_stats, success_latency_sum_ns); F(ovs_kbrtest_rpc_stats, hop_count_min);
    F(ovs_kbrtest_rpc_stats, hop_count_max); F(ovs_kbrtest_rpc_stats, success_latency_min_ns);
    F(ovs_kbrtest_rpc_stats, success_latency_max_ns); F(ovs_kbrtest_rpc_stats, hop_count_mean);
    F(ovs_kbrtest_rpc_stats, success_latency_mean_s); F(ovs_kbrtest_rpc_stats, total_latency_mean_s);
    F(ovs_kbrtest_rpc_stats, status_count); F(ovs_kbrtest_rpc_stats, hop_hist);
    F(ovs_kbrtest_rpc_stats, delivered_msgs_per_s); F(ovs_kbrtest_rpc_stats, delivered_bytes_per_s);
    F(ovs_kbrtest_rpc_stats, dropped_msgs_per_s); F(ovs_kbrtest_rpc_stats, dropped_bytes_per_s);
    F(ovs_kbrtest_rpc_stats, delivery_ratio);
    printf("}}}\n");
    return 0;
}
