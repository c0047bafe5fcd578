// dht_teams_driver.cpp -- the host pieces of the replica-team DHTs that need no GPU, as a stand-alone program
// for -fsanitize=address,undefined (tests/test_dht_teams_model.py): SymmetricDHT's offset division, the checks
// of initializeDHT and the .ini binder additions (linked with oversim_amd/csrc/ovs_ini.cpp).
#include <cstdio>
#include <cstring>
#include <string>

#include "../oversim_amd/csrc/team_params.hpp"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static const char* INI =
    "[General]\n**.tier1.dht.numReplica = 4\n"
    "[Config ChordBroadcast]\n"
    "**.lifetimeMean = ${200s, 400s}\n"
    "**.tier1Type = \"oversim.applications.dht.SymmetricDHTModules\"\n"
    "**.tier1.dht.numReplica = 8\n"
    "**.tier1.dht.numReplicaTeams = 4\n"
    "[Config Rh]\n"
    "**.tier1Type = \"oversim.applications.dht.RepeatedHashingDHTModules\"\n"
    "**.tier1.dht.numReplicaTeams = 2\n"
    "[Config Plain]\n"
    "**.tier1Type = \"oversim.applications.dht.DHTModules\"\n"
    "**.tier1.dht.numReplicaTeams = 2\n"
    "[Config Bad]\n"
    "**.tier1.dht.numReplicaTeams = four\n"
    "[Config Other]\n"
    "**.tier1Type = \"oversim.applications.kbrtestapp.KBRTestAppModules\"\n";

int main()
{
    // offset * T + remainder = 2^160 - 1 with remainder < T, limb by limb
    for (int T = 1; T <= 8; ++T) {
        uint32_t w[5];
        ovs::team_offset(T, w);
        uint64_t carry = 0;
        uint32_t p[5];
        for (int i = 0; i < 5; ++i) {
            const uint64_t v = (uint64_t)w[i] * (uint64_t)T + carry;
            p[i] = (uint32_t)v;
            carry = v >> 32;
        }
        CHECK(carry == 0);
        for (int i = 1; i < 5; ++i) CHECK(p[i] == 0xFFFFFFFFu);
        CHECK(0xFFFFFFFFu - p[0] < (uint32_t)T);
    }
    ovs_dht_params dp;
    std::memset(&dp, 0, sizeof dp);
    dp.numReplica = 8;
    std::string msg;
    ovs_dht_team_params tp = {OVS_DHT_TEAMS_SYMMETRIC, 4};
    CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_OK);
    tp.numReplicaTeams = 3;
    CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_EINVAL && msg.find("multiple") != std::string::npos);
    tp.numReplicaTeams = 0;
    CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_ENOTSUP);
    tp.numReplicaTeams = 9;
    CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_ENOTSUP);
    tp.numReplicaTeams = 1;
    dp.numReplica = 16;
    CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_ENOTSUP);
    for (int T : {2, 4, 8}) {            // 16 replicas in all: more RPCs than an operation's replay holds
        tp.numReplicaTeams = T;
        CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_ENOTSUP && msg.find("numReplica") != std::string::npos);
    }
    dp.numReplica = 0;
    CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_ENOTSUP);
    dp.numReplica = 16;
    tp.numReplicaTeams = 1;
    tp.mode = 7;
    CHECK(ovs::team_params_check(&dp, &tp, &msg) == OVS_ENOTSUP);
    CHECK(ovs::team_params_check(nullptr, &tp, &msg) == OVS_EINVAL);

    char err[8];        // shorter than the messages: they must be cut, not overrun
    ovs_dht_team_params b = {OVS_DHT_TEAMS_REPEATED_HASHING, 1};
    CHECK(ovs_dht_team_params_from_ini(&b, INI, "ChordBroadcast", err, sizeof err) == OVS_OK);
    CHECK(b.mode == OVS_DHT_TEAMS_SYMMETRIC && b.numReplicaTeams == 4);
    int32_t ttl = -1;
    CHECK(ovs_dht_params_from_ini(&dp, &ttl, INI, "ChordBroadcast", err, sizeof err) == OVS_OK && dp.numReplica == 8);
    CHECK(ovs_dht_team_params_from_ini(&b, INI, "Rh", err, sizeof err) == OVS_OK);
    CHECK(b.mode == OVS_DHT_TEAMS_REPEATED_HASHING && b.numReplicaTeams == 2);
    CHECK(ovs_dht_team_params_from_ini(&b, INI, "Plain", err, sizeof err) == OVS_OK && b.numReplicaTeams == 1);
    CHECK(ovs_dht_team_params_from_ini(&b, INI, "Bad", err, sizeof err) == OVS_EINVAL);
    CHECK(ovs_dht_team_params_from_ini(&b, INI, "Other", err, sizeof err) == OVS_ENOTSUP);
    CHECK(ovs_dht_team_params_from_ini(&b, INI, nullptr, nullptr, 0) == OVS_OK);
    CHECK(ovs_dht_team_params_from_ini(nullptr, INI, nullptr, err, sizeof err) == OVS_EINVAL);
    CHECK(ovs_dht_team_params_from_ini_file(&b, "/nonexistent/omnetpp.ini", nullptr, err, sizeof err) == OVS_EINVAL);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
