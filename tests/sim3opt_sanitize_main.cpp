// Stand-alone driver of sindh_sim3_optimize for an AddressSanitizer / UBSan build (tests/test_sim3opt_cpu.py builds it with csrc/host/sim3_opt.cpp and runs it as its
// own process).  Input: a file of items written by the test: int32 count, then per item int32 n, int32 fix_scale, float th2, s12, K1[4], K2[4], R12[9], t12[3], and
// the arrays x3Dc1 [n][3], x3Dc2 [n][3], obs1 [n][2], obs2 [n][2], inv_sigma2_1 [n], inv_sigma2_2 [n].  Every item runs twice, with and without the diagnostics.
// Output: per item one line "n_inliers n_bad n_stages removed-count bits-of-s".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sind_hip.h"

extern "C" int sindh_sim3_optimize(const sind_sim3opt_item* items, int B, float th2, int fix_scale);

template <class T> static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (!get(f, &count, 1)) return 2;
    for (int k = 0; k < count; k++) {
        int32_t n = 0, fix = 0; float th2 = 0, s12 = 0, K1[4], K2[4], R12[9], t12[3];
        if (!get(f, &n, 1) || !get(f, &fix, 1) || !get(f, &th2, 1) || !get(f, &s12, 1) || !get(f, K1, 4) || !get(f, K2, 4) || !get(f, R12, 9) || !get(f, t12, 3)) return 2;
        std::vector<float> x1(3 * n), x2(3 * n), o1(2 * n), o2(2 * n), i1(n), i2(n);                     // exactly n entries: a read past the end is a report
        if (!get(f, x1.data(), x1.size()) || !get(f, x2.data(), x2.size()) || !get(f, o1.data(), o1.size()) || !get(f, o2.data(), o2.size()) || !get(f, i1.data(), i1.size()) || !get(f, i2.data(), i2.size())) return 2;
        for (int diag = 0; diag < 2; diag++) {
            std::vector<uint8_t> removed(n);
            double q[4], t[3], s; int nIn = -1, nBad = -1, stages = -1, iters[2]; double chi2[2], lambda[2];
            sind_sim3opt_item it;
            std::memset(&it, 0, sizeof(it));
            it.n = n; it.s12 = s12; it.x3Dc1 = n ? x1.data() : nullptr; it.x3Dc2 = n ? x2.data() : nullptr; it.obs1_xy = n ? o1.data() : nullptr; it.obs2_xy = n ? o2.data() : nullptr;
            it.inv_sigma2_1 = n ? i1.data() : nullptr; it.inv_sigma2_2 = n ? i2.data() : nullptr; it.K1 = K1; it.K2 = K2; it.R12 = R12; it.t12 = t12;
            it.q_out = q; it.t_out = t; it.s_out = &s; it.removed = n ? removed.data() : nullptr; it.n_inliers = &nIn;
            if (diag) { it.n_bad = &nBad; it.n_stages = &stages; it.stage_iters = iters; it.stage_chi2 = chi2; it.stage_lambda = lambda; }
            if (sindh_sim3_optimize(&it, 1, th2, fix) != 0) return 3;
            if (diag) {
                int rem = 0; for (int i = 0; i < n; i++) rem += removed[i];
                uint64_t sb; std::memcpy(&sb, &s, 8);
                printf("%d %d %d %d %llu\n", nIn, nBad, stages, rem, (unsigned long long)sb);
            }
        }
    }
    fclose(f);
    return 0;
}
