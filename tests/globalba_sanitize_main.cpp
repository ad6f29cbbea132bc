// Stand-alone driver of sindh_global_ba for an AddressSanitizer / UBSan build (tests/test_globalba_cpu.py builds it with csrc/host/global_ba.cpp and runs it as its own
// process).  Input: a file of items written by the test: float K5[5], int32 count, then per item int32 n_kf, n_mp, n_obs, iterations, robust, expected return code, and
// the arrays kf_id i64 [n_kf], Tcw [n_kf][16], mp_id i64 [n_mp], x3Dw [n_mp][3], obs_start i32 [n_mp + 1], obs_kf i32 [n_obs], obs_xy [n_obs][2], u_right [n_obs],
// inv_sigma2 [n_obs].  Every item runs twice, with and without the diagnostics.
// Output: per item one line "return-code n_iters n_active_poses included-count env_entries bits-of-chi2 bits-of-the-last-float-of-Tcw_out-row-0".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sind_hip.h"

template <class T> static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    float K5[5]; int32_t count = 0;
    if (!get(f, K5, 5) || !get(f, &count, 1)) return 2;
    for (int k = 0; k < count; k++) {
        int32_t h[6];
        if (!get(f, h, 6)) return 2;
        const int nKf = h[0], nMp = h[1], nObs = h[2];
        std::vector<int64_t> kfId(nKf), mpId(nMp); std::vector<float> Tcw(16 * nKf), X(3 * nMp), xy(2 * nObs), ur(nObs), s2(nObs);      // exactly as many entries: a read past the end is a report
        std::vector<int32_t> start(nMp + 1), okf(nObs);
        if (!get(f, kfId.data(), kfId.size()) || !get(f, Tcw.data(), Tcw.size()) || !get(f, mpId.data(), mpId.size()) || !get(f, X.data(), X.size()) ||
            !get(f, start.data(), start.size()) || !get(f, okf.data(), okf.size()) || !get(f, xy.data(), xy.size()) || !get(f, ur.data(), ur.size()) || !get(f, s2.data(), s2.size())) return 2;
        for (int diag = 0; diag < 2; diag++) {
            std::vector<float> To(16 * nKf + 16), Xo(3 * nMp); std::vector<uint8_t> inc(nMp);
            int iters = -7, act = -7, fail = -7; double chi2 = 0, lambda = 0; long long env = -7, dense = -7;
            sind_globalba_item it;
            std::memset(&it, 0, sizeof(it));
            it.n_kf = nKf; it.kf_id = nKf ? kfId.data() : nullptr; it.Tcw = nKf ? Tcw.data() : nullptr;
            it.n_mp = nMp; it.mp_id = nMp ? mpId.data() : nullptr; it.x3Dw = nMp ? X.data() : nullptr; it.obs_start = nMp ? start.data() : nullptr;
            it.obs_kf = nObs ? okf.data() : nullptr; it.obs_xy = nObs ? xy.data() : nullptr; it.u_right = nObs ? ur.data() : nullptr; it.inv_sigma2 = nObs ? s2.data() : nullptr;
            it.Tcw_out = nKf ? To.data() : nullptr; it.x3Dw_out = nMp ? Xo.data() : nullptr; it.included = nMp ? inc.data() : nullptr;
            if (diag) { it.n_iters = &iters; it.chi2 = &chi2; it.lambda = &lambda; it.n_active_poses = &act; it.solver_fail = &fail; it.env_entries = &env; it.env_dense_entries = &dense; }
            const int rc = sindh_global_ba(&it, 1, h[3], h[4], K5);
            if (rc != h[5]) return 3;
            if (diag) {
                int in = 0; for (int i = 0; i < nMp; i++) in += inc[i];
                uint64_t cb; std::memcpy(&cb, &chi2, 8);
                uint32_t tb; std::memcpy(&tb, &To[11], 4);
                printf("%d %d %d %d %lld %llu %u\n", rc, iters, act, in, env, (unsigned long long)cb, tb);
            }
        }
    }
    fclose(f);
    return 0;
}
