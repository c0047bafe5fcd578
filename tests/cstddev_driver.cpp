// cstddev_driver.cpp -- oversim_amd/csrc/cstddev.hpp under ASan/UBSan (tests/test_sanitizers.py).
// Prints, per case, the five fields finish() leaves in a zeroed ovs_stddev: the count and the four
// doubles as hex floats.  The test recomputes every line in the same operation order.
#include <cstdio>
#include <cstring>

#include "cstddev.hpp"

using ovs::CStdDev;

static void show(const char* name, const CStdDev& a)
{
    ovs_stddev d;
    std::memset(&d, 0, sizeof d);
    a.finish(d);
    std::printf("%s %llu %a %a %a %a\n", name, (unsigned long long)d.count, d.mean, d.stddev, d.min, d.max);
}

int main()
{
    show("empty", CStdDev{});

    CStdDev one;
    one.collect(2.5);
    show("one", one);

    CStdDev two;
    two.collect(1.0);
    two.collect(4.0);
    show("two", two);

    // 0.1 three times: sqsum - sum * sum / 3 rounds below zero, the variance clamps to 0
    CStdDev clamp;
    for (int i = 0; i < 3; ++i) clamp.collect(0.1);
    show("clamp", clamp);

    // exact integer sums against collect() over the same samples
    const unsigned samples[] = {3, 7, 7, 12, 1, 30};
    CStdDev col;
    unsigned long long n = 0, sum = 0, sq = 0, mn = ~0ull, mx = 0;
    for (unsigned v : samples) {
        col.collect((double)v);
        ++n; sum += v; sq += (unsigned long long)v * v;
        if (v < mn) mn = v;
        if (v > mx) mx = v;
    }
    show("collect", col);
    show("sums", CStdDev::from_sums(n, (double)sum, (double)sq, (double)mn, (double)mx));

    // a row as the statistics kernels write it: the count's bits in the fifth double
    double row[5] = {10.5, 40.25, 0.5, 6.0, 0.0};
    const unsigned long long cnt = 4;
    std::memcpy(&row[4], &cnt, sizeof cnt);
    show("row", CStdDev::from_row(row));
    double empty_row[5] = {0.0, 0.0, INFINITY, -INFINITY, 0.0};
    show("empty_row", CStdDev::from_row(empty_row));

    std::printf("clean\n");
    return 0;
}
