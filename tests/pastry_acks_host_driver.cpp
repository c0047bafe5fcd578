// Stand-alone driver for the host-only logic of Pastry's acked routes, built with -fsanitize=address,undefined
// by tests/test_pastry_acks_model.py: pastry_acked_refusal and the wire lengths of the NextHopCall, the
// NextHopResponse and the KbrTestResponse (oversim_amd/csrc/pastry_host.hpp).  Prints the lengths for the test
// to compare with the model, then "ok".
#include <cstdio>
#include <cstring>
#include <string>

#include "pastry_host.hpp"

using namespace ovs;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static bool names(const char* why, const char* word) { return why && std::string(why).find(word) != std::string::npos; }

int main()
{
    ovs_pastry_params bp{4, 16, 0, 0, 1, 1};
    ovs_params P;
    std::memset(&P, 0, sizeof P);
    P.routingType = 1; P.numSiblings = 1; P.recNumRedundantNodes = 3; P.testMsgSize = 100; P.hopCountMax = 50;
    P.lookupRedundantNodes = P.lookupParallelRpcs = P.lookupParallelPaths = 1; P.lookupVisitOnlyOnce = 1;

    std::printf("len call %lld\nlen ack %lld\n", (long long)pastry_nexthop_call_bytes(P), (long long)pastry_nexthop_ack_bytes(P));
    P.measureAuthBlock = 1;
    std::printf("len ack_auth %lld\nlen resp %lld\n", (long long)pastry_nexthop_ack_bytes(P), (long long)pastry_rpc_response_bytes(P));
    P.measureAuthBlock = 0;

    // the shipped flags run, with and without acks, and the plain calls still refuse the flag
    for (int rpc = 0; rpc < 2; ++rpc)
        for (int acks = 0; acks < 2; ++acks) {
            bp.routeMsgAcks = acks;
            CHECK(pastry_acked_refusal(P, bp, rpc) == nullptr);
        }
    bp.routeMsgAcks = 1;
    CHECK(names(pastry_route_refusal(P, bp), "routeMsgAcks"));
    CHECK(bp.routeMsgAcks == 1);                                  // the refusal works on a copy

    // routing types: iterative runs the one-way message only
    P.routingType = 0;
    CHECK(pastry_acked_refusal(P, bp, false) == nullptr);
    CHECK(names(pastry_acked_refusal(P, bp, true), "semi-recursive"));
    CHECK(names(pastry_iterative_refusal(P, bp, true), "routeMsgAcks"));
    P.lookupMerge = 1;
    CHECK(names(pastry_acked_refusal(P, bp, false), "lookupMerge"));
    P.lookupMerge = 0;
    P.hopCountMax = 0;
    CHECK(names(pastry_acked_refusal(P, bp, false), "hopCountMax"));
    P.hopCountMax = 50;
    for (int rt : {2, 3, 4, 7})
        for (int rpc = 0; rpc < 2; ++rpc) { P.routingType = rt; CHECK(pastry_acked_refusal(P, bp, rpc) != nullptr); }
    P.routingType = 2;
    CHECK(names(pastry_acked_refusal(P, bp, false), "full-recursive"));
    P.routingType = 4;
    CHECK(names(pastry_acked_refusal(P, bp, false), "source-routing"));
    P.routingType = 1;

    // what the plain route refuses apart from the flag
    P.numSiblings = 2;
    CHECK(names(pastry_acked_refusal(P, bp, false), "numSiblings"));
    P.numSiblings = 1;
    for (int r : {0, 9}) { P.recNumRedundantNodes = r; CHECK(names(pastry_acked_refusal(P, bp, true), "recNumRedundantNodes")); }
    P.recNumRedundantNodes = 3;
    bp.bitsPerDigit = 5;
    CHECK(names(pastry_acked_refusal(P, bp, false), "bitsPerDigit"));
    bp.bitsPerDigit = 4;
    bp.numberOfNeighbors = 2;
    CHECK(names(pastry_acked_refusal(P, bp, false), "numberOfNeighbors"));
    bp.numberOfNeighbors = 0;

    // the transmit queue: ack 60 B + call (testMsgSize + 118) B against 10^6 B, on the byte
    P.testMsgSize = (int32_t)(PASTRY_SEND_QUEUE_BYTES - 60 - 118);
    CHECK(pastry_acked_refusal(P, bp, false) == nullptr && pastry_acked_refusal(P, bp, true) == nullptr);
    P.testMsgSize += 1;
    CHECK(names(pastry_acked_refusal(P, bp, false), "sendQueueLength") && names(pastry_acked_refusal(P, bp, true), "sendQueueLength"));
    bp.routeMsgAcks = 0;
    CHECK(pastry_acked_refusal(P, bp, false) == nullptr);         // no ack, no second packet in the queue
    bp.routeMsgAcks = 1;
    P.testMsgSize -= 101;
    P.measureAuthBlock = 1;                                       // the ack grows by AUTHBLOCK_L
    CHECK(pastry_acked_refusal(P, bp, false) == nullptr);
    P.testMsgSize += 1;
    CHECK(names(pastry_acked_refusal(P, bp, false), "sendQueueLength"));
    P.testMsgSize = -1;
    CHECK(names(pastry_acked_refusal(P, bp, false), "testMsgSize"));

    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
