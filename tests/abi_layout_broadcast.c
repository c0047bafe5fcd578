/* Prints the layout of the broadcast structs of include/ovs_kbr.h as JSON, compiled by a plain C
 * compiler against the header alone (tests/test_broadcast_model.py compares it with the Python
 * mirrors in oversim_amd/kbr.py), in the style of tests/abi_layout.c. */
#include <stddef.h>
#include <stdio.h>

#include "ovs_kbr.h"

#ifndef OVS_HAS_CHORD_BROADCAST
#error "include/ovs_kbr.h does not declare the Chord broadcast"
#endif

#define F(T, f) printf("%s\"%s\": %zu", first++ ? ", " : "", #f, offsetof(T, f))

int main(void)
{
    int first = 0;
    printf("{\"abi\": %d, \"ovs_bcast_node\": {\"size\": %zu, \"fields\": {", OVS_ABI_VERSION, sizeof(ovs_bcast_node));
    F(ovs_bcast_node, arrival_ns); F(ovs_bcast_node, parent); F(ovs_bcast_node, hops); F(ovs_bcast_node, rank);
    first = 0;
    printf("}}, \"ovs_bcast_stats\": {\"size\": %zu, \"fields\": {", sizeof(ovs_bcast_stats));
    F(ovs_bcast_stats, expected); F(ovs_bcast_stats, actual); F(ovs_bcast_stats, expired);
    F(ovs_bcast_stats, messages); F(ovs_bcast_stats, bytes); F(ovs_bcast_stats, last_arrival_ns);
    F(ovs_bcast_stats, hop_count);
    printf("}}}\n");
    return 0;
}
