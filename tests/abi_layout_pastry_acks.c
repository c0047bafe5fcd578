/* Prints the layout of the ack record of include/ovs_kbr.h as JSON, compiled by a plain C compiler against the
 * header alone (tests/test_pastry_acks_model.py compares it with the numpy mirror in oversim_amd/kbr.py), in the
 * style of tests/abi_layout_pastry.c. */
#include <stddef.h>
#include <stdio.h>

#include "ovs_kbr.h"

#if !defined(OVS_HAS_PASTRY_ACKS) || !defined(OVS_HAS_PASTRY_RPC)
#error "include/ovs_kbr.h does not declare the acked Pastry calls"
#endif

#define F(T, f) printf("%s\"%s\": %zu", first++ ? ", " : "", #f, offsetof(T, f))
#define OPEN(T) first = 0, printf(", \"" #T "\": {\"size\": %zu, \"fields\": {", sizeof(T))

int main(void)
{
    int first = 0;
    printf("{\"abi\": %d, \"has_acks\": %d, \"has_rpc\": %d, \"ovs_pastry_params_size\": %zu", OVS_ABI_VERSION,
           OVS_HAS_PASTRY_ACKS, OVS_HAS_PASTRY_RPC, sizeof(ovs_pastry_params));
    OPEN(ovs_pastry_ack_out);
    F(ovs_pastry_ack_out, max_ack_rtt_ns); F(ovs_pastry_ack_out, acks); F(ovs_pastry_ack_out, timeout_hop);
    F(ovs_pastry_ack_out, pad);
    printf("}}}\n");
    return 0;
}
