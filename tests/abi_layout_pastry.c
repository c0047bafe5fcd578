/* Prints the layout of the Pastry struct of include/ovs_kbr.h as JSON, compiled by a plain C compiler against
 * the header alone (tests/test_abi_layout_pastry.py compares it with the Python mirror in oversim_amd/kbr.py),
 * in the style of tests/abi_layout_broose.c. */
#include <stddef.h>
#include <stdio.h>

#include "ovs_kbr.h"

#ifndef OVS_HAS_PASTRY
#error "include/ovs_kbr.h does not declare the Pastry calls"
#endif

#define F(T, f) printf("%s\"%s\": %zu", first++ ? ", " : "", #f, offsetof(T, f))
#define OPEN(T) first = 0, printf(", \"" #T "\": {\"size\": %zu, \"fields\": {", sizeof(T))

int main(void)
{
    int first = 0;
    printf("{\"abi\": %d, \"overlay\": %d", OVS_ABI_VERSION, (int)OVS_OVERLAY_PASTRY);
    OPEN(ovs_pastry_params);
    F(ovs_pastry_params, bitsPerDigit); F(ovs_pastry_params, numberOfLeaves); F(ovs_pastry_params, numberOfNeighbors);
    F(ovs_pastry_params, optimizeLookup); F(ovs_pastry_params, useRegularNextHop); F(ovs_pastry_params, routeMsgAcks);
    printf("}}}\n");
    return 0;
}
