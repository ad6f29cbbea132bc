// Stand-alone driver of sindh_local_ba for an AddressSanitizer / UBSan build (tests/test_localba_cpu.py builds it with csrc/host/local_ba.cpp and runs it as its own
// process).  Input: a file of items written by the test: float K5[5], int32 count, then per item int32 n_kf, n_mp, n_obs, do_more, expected return code, and the arrays
// kf_id i64 [n_kf], kf_kind u8 [n_kf], Tcw [n_kf][16], mp_id i64 [n_mp], x3Dw [n_mp][3], obs_start i32 [n_mp + 1], obs_kf i32 [n_obs], obs_xy [n_obs][2], u_right
// [n_obs], inv_sigma2 [n_obs].  Every item runs twice, with and without the diagnostics.
// Output: per item one line "return-code n_stages n_level1 erase-count bits-of-stage_chi2[1]".
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
        int32_t h[5];
        if (!get(f, h, 5)) return 2;
        const int nKf = h[0], nMp = h[1], nObs = h[2];
        std::vector<int64_t> kfId(nKf), mpId(nMp); std::vector<uint8_t> kind(nKf); std::vector<float> Tcw(16 * nKf), X(3 * nMp), xy(2 * nObs), ur(nObs), s2(nObs);      // exactly as many entries: a read past the end is a report
        std::vector<int32_t> start(nMp + 1), okf(nObs);
        if (!get(f, kfId.data(), kfId.size()) || !get(f, kind.data(), kind.size()) || !get(f, Tcw.data(), Tcw.size()) || !get(f, mpId.data(), mpId.size()) || !get(f, X.data(), X.size()) ||
            !get(f, start.data(), start.size()) || !get(f, okf.data(), okf.size()) || !get(f, xy.data(), xy.size()) || !get(f, ur.data(), ur.size()) || !get(f, s2.data(), s2.size())) return 2;
        for (int diag = 0; diag < 2; diag++) {
            std::vector<float> To(16 * nKf), Xo(3 * nMp); std::vector<uint8_t> erase(nObs);
            int stages = -1, iters[2], level1 = -1; double chi2[2] = {0, 0}, lambda[2];
            sind_localba_item it;
            std::memset(&it, 0, sizeof(it));
            it.n_kf = nKf; it.kf_id = nKf ? kfId.data() : nullptr; it.kf_kind = nKf ? kind.data() : nullptr; it.Tcw = nKf ? Tcw.data() : nullptr;
            it.n_mp = nMp; it.mp_id = nMp ? mpId.data() : nullptr; it.x3Dw = nMp ? X.data() : nullptr; it.obs_start = nMp ? start.data() : nullptr;
            it.obs_kf = nObs ? okf.data() : nullptr; it.obs_xy = nObs ? xy.data() : nullptr; it.u_right = nObs ? ur.data() : nullptr; it.inv_sigma2 = nObs ? s2.data() : nullptr;
            it.do_more = h[3]; it.Tcw_out = nKf ? To.data() : nullptr; it.x3Dw_out = nMp ? Xo.data() : nullptr; it.erase = nObs ? erase.data() : nullptr;
            if (diag) { it.n_stages = &stages; it.stage_iters = iters; it.n_level1 = &level1; it.stage_chi2 = chi2; it.stage_lambda = lambda; }
            const int rc = sindh_local_ba(&it, 1, K5);
            if (rc != h[4]) return 3;
            if (diag) {
                int er = 0; for (int i = 0; i < nObs; i++) er += erase[i];
                uint64_t cb; std::memcpy(&cb, &chi2[1], 8);
                printf("%d %d %d %d %llu\n", rc, stages, level1, er, (unsigned long long)cb);
            }
        }
    }
    fclose(f);
    return 0;
}
