/* Prints the layout of the Broose structs of include/ovs_kbr.h as JSON, compiled by a plain C compiler
 * against the header alone (tests/test_abi_layout_broose.py compares it with the Python mirrors in
 * oversim_amd/kbr.py), in the style of tests/abi_layout_dht.c. */
#include <stddef.h>
#include <stdio.h>

#include "ovs_kbr.h"

#ifndef OVS_HAS_BROOSE
#error "include/ovs_kbr.h does not declare the Broose calls"
#endif

#define F(T, f) printf("%s\"%s\": %zu", first++ ? ", " : "", #f, offsetof(T, f))
#define OPEN(T) first = 0, printf(", \"" #T "\": {\"size\": %zu, \"fields\": {", sizeof(T))

int main(void)
{
    int first = 0;
    printf("{\"abi\": %d, \"overlay\": %d", OVS_ABI_VERSION, (int)OVS_OVERLAY_BROOSE);
    OPEN(ovs_broose_params);
    F(ovs_broose_params, bucketSize); F(ovs_broose_params, rBucketSize); F(ovs_broose_params, userDist);
    F(ovs_broose_params, shiftingBits);
    printf("}}");
    OPEN(ovs_broose_ext);
    F(ovs_broose_ext, route_key); F(ovs_broose_ext, step); F(ovs_broose_ext, has_ext); F(ovs_broose_ext, right_shifting);
    F(ovs_broose_ext, pad); F(ovs_broose_ext, last_node);
    printf("}}}\n");
    return 0;
}
