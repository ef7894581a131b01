// The genome-pair table K16 (divergence.hip) and K17 (ingroup.hip) share: what orthofilter.gd_table makes of global_differences - the one
// transcendental of checkDiv / distances / determineGroup, exp, depends on the genome pair alone - as keys g1 << 32 | g2 (g1 <= g2, strictly
// increasing) and three doubles per key (gd0, gd0 * exp(gd1 * sqrt(allowed_sigma)), gd0 * exp(gd1 * allowed_sigma)), the default of a missing
// pair behind the last row.  Here: the device view, its binary search and the host check of the caller's table.  What a pair of rows of ONE
// genome gets differs between the two kernels and stays with them.
#pragma once
#include <cmath>
#include <stdint.h>
#include <string>

struct GdTable {
    const uint64_t *key;            // [n] sorted
    const double *val;              // [n + 1][3]: gd0, denX, den; row n = the default
    uint64_t n;
    double self_id;
};

// the row of val for two DIFFERENT genomes: the pair's own, or n (the default) when the table lacks it
__device__ __forceinline__ uint64_t gd_row(const GdTable &T, uint32_t ga, uint32_t gb)
{
    const uint64_t key = ga < gb ? ((uint64_t)ga << 32 | gb) : ((uint64_t)gb << 32 | ga);
    uint64_t lo = 0, hi = T.n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (T.key[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < T.n && T.key[lo] == key) ? lo : T.n;
}

inline bool gd_good(double v) { return std::isfinite(v) && v > 0.; }

// the check of the caller's table, on the host: the text of a PEP_ERR_ARG, or empty
inline std::string gd_table_fault(const uint64_t *gd_key, const double *gd_val, uint64_t n_gd, const double *gd_default)
{
    for (uint64_t i = 0; i < n_gd; ++i) {
        if ((gd_key[i] >> 32) > (gd_key[i] & 0xFFFFFFFFull)) return "gd_key " + std::to_string(i) + " has g1 > g2";
        if (i && gd_key[i] <= gd_key[i - 1]) return "gd_key must be strictly increasing (entry " + std::to_string(i) + ")";
    }
    for (uint64_t i = 0; i <= n_gd; ++i) {
        const double *v = i < n_gd ? gd_val + 3 * i : gd_default;
        if (!gd_good(v[0]) || !gd_good(v[1]) || !gd_good(v[2]))
            return (i < n_gd ? "gd_val row " + std::to_string(i) : std::string("gd_default")) + " must be finite and > 0 in all three columns";
    }
    return std::string();
}
