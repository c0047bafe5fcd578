// cstddev.hpp -- OMNeT++ 4.x cStdDev as the statistics calls finish it (host only, plain C++).
//
// collect() keeps count, sum, sum of squares, min and max in the order the values come; finish() is
// cStdDev::getMean / getVariance: the sample variance, 0 below two values or if rounding made it
// negative.  The per-node statistics collect in node order; exact integer sums go through from_sums.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/ovs_kbr.h"

namespace ovs {

struct CStdDev {
    uint64_t count = 0;
    double sum = 0, sqsum = 0, min = INFINITY, max = -INFINITY;

    void collect(double v)
    {
        sum += v;
        sqsum += v * v;
        if (v < min) min = v;
        if (v > max) max = v;
        ++count;
    }

    static CStdDev from_sums(uint64_t count, double sum, double sqsum, double min, double max)
    {
        CStdDev a;
        a.count = count; a.sum = sum; a.sqsum = sqsum; a.min = min; a.max = max;
        return a;
    }

    // a row of the statistics kernels' reductions (stats.hpp): sum, sum of squares, min, max, and the
    // count's 64 bits in the fifth double
    static CStdDev from_row(const double* r)
    {
        uint64_t cnt;
        std::memcpy(&cnt, &r[4], sizeof cnt);
        return from_sums(cnt, r[0], r[1], r[2], r[3]);
    }

    // an empty accumulator leaves d (zeroed by the caller) as it is
    void finish(ovs_stddev& d) const
    {
        d.count = count;
        if (!count) return;
        d.mean = sum / (double)count;
        double var = 0.0;
        if (count > 1) {
            var = (sqsum - sum * sum / (double)count) / (double)(count - 1);
            if (var < 0) var = 0;
        }
        d.stddev = std::sqrt(var);
        d.min = min;
        d.max = max;
    }
};

}  // namespace ovs
