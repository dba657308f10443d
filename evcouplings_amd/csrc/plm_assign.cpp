// plm_assign.cpp -- exact rectangular linear assignment per group of a block-structured score table (host code, no
// device): the matching step behind plm_cross_energies (DESIGN_NEXT_ROWS.md 9.23).  Shortest augmenting paths with
// potentials (the Hungarian method in its O(n^2 m) form, n <= m): one row enters at a time, a Dijkstra-like scan over the
// columns finds the cheapest augmenting path, and the potentials keep every reduced cost non-negative.
#include "../../include/plm_hip.h"
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

int plm_fail(int code, const char *fmt, ...);   // plm_host.cpp

namespace {

// cost(r, c) for r < n, c < m with n <= m; row_of_col[c] = the row assigned to column c, or -1
template <typename Cost> void assign_rows(int64_t n, int64_t m, Cost cost, std::vector<int64_t> *row_of_col) {
    const double inf = std::numeric_limits<double>::infinity();
    // 1-based as in the classical formulation; column 0 is the virtual start
    std::vector<double> u((size_t)n + 1, 0.0), v((size_t)m + 1, 0.0), minv((size_t)m + 1);
    std::vector<int64_t> p((size_t)m + 1, 0), way((size_t)m + 1, 0);
    std::vector<char> used((size_t)m + 1);
    for (int64_t r = 1; r <= n; r++) {
        p[0] = r;
        int64_t j0 = 0;
        std::fill(minv.begin(), minv.end(), inf);
        std::fill(used.begin(), used.end(), 0);
        do {
            used[(size_t)j0] = 1;
            const int64_t i0 = p[(size_t)j0];
            double delta = inf;
            int64_t j1 = 0;
            for (int64_t j = 1; j <= m; j++) {
                if (used[(size_t)j]) continue;
                const double cur = cost(i0 - 1, j - 1) - u[(size_t)i0] - v[(size_t)j];
                if (cur < minv[(size_t)j]) {
                    minv[(size_t)j] = cur;
                    way[(size_t)j] = j0;
                }
                if (minv[(size_t)j] < delta) {
                    delta = minv[(size_t)j];
                    j1 = j;
                }
            }
            for (int64_t j = 0; j <= m; j++) {
                if (used[(size_t)j]) {
                    u[(size_t)p[(size_t)j]] += delta;
                    v[(size_t)j] -= delta;
                } else {
                    minv[(size_t)j] -= delta;
                }
            }
            j0 = j1;
        } while (p[(size_t)j0] != 0);
        do {
            const int64_t j1 = way[(size_t)j0];
            p[(size_t)j0] = p[(size_t)j1];
            j0 = j1;
        } while (j0);
    }
    row_of_col->assign((size_t)m, -1);
    for (int64_t j = 1; j <= m; j++)
        if (p[(size_t)j]) (*row_of_col)[(size_t)j - 1] = p[(size_t)j] - 1;
}

}  // namespace

int plm_group_assignment(const double *scores, int64_t n_groups, const int64_t *a_offsets, const int64_t *b_offsets,
                         int32_t maximize, int64_t *partner_of_a, double *totals) {
    if (!a_offsets || !b_offsets) return plm_fail(PLM_EINVAL, "NULL offsets");
    if (n_groups < 0) return plm_fail(PLM_EINVAL, "negative count");
    if (a_offsets[0] != 0 || b_offsets[0] != 0) return plm_fail(PLM_EINVAL, "offsets must start at 0");
    double n_scores = 0.0;
    for (int64_t g = 0; g < n_groups; g++) {
        if (a_offsets[g + 1] < a_offsets[g] || b_offsets[g + 1] < b_offsets[g])
            return plm_fail(PLM_EINVAL, "offsets decrease at group %lld", (long long)g);
        n_scores += (double)(a_offsets[g + 1] - a_offsets[g]) * (double)(b_offsets[g + 1] - b_offsets[g]);
    }
    if (n_scores >= 9.2e18) return plm_fail(PLM_EINVAL, "2^63 scores or more");
    const int64_t n_a = a_offsets[n_groups];
    if ((n_scores > 0 && !scores) || (n_a > 0 && !partner_of_a)) return plm_fail(PLM_EINVAL, "NULL argument");
    for (int64_t k = 0; k < (int64_t)n_scores; k++)
        if (!std::isfinite(scores[k])) return plm_fail(PLM_EINVAL, "scores[%lld] is not finite", (long long)k);
    const double sign = maximize ? -1.0 : 1.0;
    std::vector<int64_t> row_of_col;
    const double *blk = scores;
    for (int64_t g = 0; g < n_groups; g++) {
        const int64_t a0 = a_offsets[g], b0 = b_offsets[g], na = a_offsets[g + 1] - a0, nb = b_offsets[g + 1] - b0;
        for (int64_t s = 0; s < na; s++) partner_of_a[a0 + s] = -1;
        if (na > 0 && nb > 0) {
            if (na <= nb) {                  // the a-rows enter, every one gets a partner
                assign_rows(na, nb, [&](int64_t r, int64_t c) { return sign * blk[r * nb + c]; }, &row_of_col);
                for (int64_t c = 0; c < nb; c++)
                    if (row_of_col[(size_t)c] >= 0) partner_of_a[a0 + row_of_col[(size_t)c]] = b0 + c;
            } else {                         // the b-rows enter
                assign_rows(nb, na, [&](int64_t r, int64_t c) { return sign * blk[c * nb + r]; }, &row_of_col);
                for (int64_t c = 0; c < na; c++)
                    if (row_of_col[(size_t)c] >= 0) partner_of_a[a0 + c] = b0 + row_of_col[(size_t)c];
            }
        }
        if (totals) {
            double sum = 0.0;                // over the a-rows in order
            for (int64_t s = 0; s < na; s++)
                if (partner_of_a[a0 + s] >= 0) sum += blk[s * nb + (partner_of_a[a0 + s] - b0)];
            totals[g] = sum;
        }
        blk += na * nb;
    }
    return PLM_OK;
}
