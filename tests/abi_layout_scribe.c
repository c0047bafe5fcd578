/* Prints the layout of the Scribe structs of include/ovs_kbr.h as JSON, compiled by a plain C compiler
 * against the header alone (tests/test_scribe_model.py compares it with the Python mirrors in
 * oversim_amd/kbr.py), in the style of tests/abi_layout_dht.c. */
#include <stddef.h>
#include <stdio.h>

#include "ovs_kbr.h"

#ifndef OVS_HAS_SCRIBE
#error "include/ovs_kbr.h does not declare the Scribe calls"
#endif

#define F(T, f) printf("%s\"%s\": %zu", first++ ? ", " : "", #f, offsetof(T, f))
#define OPEN(T) first = 0, printf(", \"" #T "\": {\"size\": %zu, \"fields\": {", sizeof(T))

int main(void)
{
    int first = 0;
    printf("{\"abi\": %d, \"status\": [%d, %d, %d], \"flags\": [%u, %u, %u]", OVS_ABI_VERSION, (int)OVS_SCRIBE_OK,
           (int)OVS_SCRIBE_WRONG_ROOT, (int)OVS_SCRIBE_ROUTE_FAILED, OVS_SCRIBE_SUBSCRIBER, OVS_SCRIBE_ROOT,
           OVS_SCRIBE_FORWARDER);
    OPEN(ovs_scribe_node);
    F(ovs_scribe_node, group); F(ovs_scribe_node, node); F(ovs_scribe_node, parent); F(ovs_scribe_node, depth);
    F(ovs_scribe_node, flags);
    printf("}}");
    OPEN(ovs_scribe_msg_out);
    F(ovs_scribe_msg_out, response_ns); F(ovs_scribe_msg_out, last_delivery_ns); F(ovs_scribe_msg_out, receivers);
    F(ovs_scribe_msg_out, forwarded); F(ovs_scribe_msg_out, publish_hops); F(ovs_scribe_msg_out, depth);
    F(ovs_scribe_msg_out, status); F(ovs_scribe_msg_out, pad);
    printf("}}");
    OPEN(ovs_scribe_delivery);
    F(ovs_scribe_delivery, msg); F(ovs_scribe_delivery, node); F(ovs_scribe_delivery, hops); F(ovs_scribe_delivery, pad);
    F(ovs_scribe_delivery, arrival_ns);
    printf("}}}\n");
    return 0;
}
