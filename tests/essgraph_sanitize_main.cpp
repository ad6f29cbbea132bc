// Stand-alone driver of sindh_essential_graph for an AddressSanitizer / UBSan build (tests/test_essgraph_cpu.py builds it with csrc/host/essential_graph.cpp and runs it
// as its own process).  Input: a file of items written by the test: int32 count, then per item int32 n_kf, n_edges, n_mp, fixed_kf, fix_scale, expected return code, a tweak
// applied to the item after it is filled (0 none, 1 edge_i = NULL, 2 x3Dw = NULL, 3 n_mp = -1, 4 n_edges = -1), and the arrays kf_id i64 [n_kf], Tcw [n_kf][16], has_corrected u8 [n_kf], corrected f64 [n_kf][8], has_noncorrected u8 [n_kf], noncorrected f64 [n_kf][8], edge_i i32
// [n_edges], edge_j i32 [n_edges], edge_kind u8 [n_edges], x3Dw [n_mp][3], mp_ref i32 [n_mp].  Every item runs twice, with and without the diagnostics.
// Output: per item one line "return-code n_iters n_active solver_fail bits-of-chi2 bits-of-the-last-Siw_out-entry".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sind_hip.h"

template <class T> static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (!get(f, &count, 1)) return 2;
    for (int k = 0; k < count; k++) {
        int32_t h[7];
        if (!get(f, h, 7)) return 2;
        const int nKf = h[0], nE = h[1], nMp = h[2];
        std::vector<int64_t> kfId(nKf); std::vector<float> Tcw(16 * nKf), X(3 * nMp); std::vector<uint8_t> hasC(nKf), hasN(nKf), kind(nE);      // exactly as many entries: a read past the end is a report
        std::vector<double> corr(8 * nKf), ncorr(8 * nKf); std::vector<int32_t> ei(nE), ej(nE), ref(nMp);
        if (!get(f, kfId.data(), kfId.size()) || !get(f, Tcw.data(), Tcw.size()) || !get(f, hasC.data(), hasC.size()) || !get(f, corr.data(), corr.size()) || !get(f, hasN.data(), hasN.size()) ||
            !get(f, ncorr.data(), ncorr.size()) || !get(f, ei.data(), ei.size()) || !get(f, ej.data(), ej.size()) || !get(f, kind.data(), kind.size()) || !get(f, X.data(), X.size()) ||
            !get(f, ref.data(), ref.size())) return 2;
        for (int diag = 0; diag < 2; diag++) {
            std::vector<double> Siw(8 * nKf); std::vector<float> Tiw(16 * nKf), Xo(3 * nMp);
            int iters = -7, nAct = -7, fail = -7; double chi2 = 0, lambda = 0;
            sind_essgraph_item it;
            std::memset(&it, 0, sizeof(it));
            it.n_kf = nKf; it.kf_id = ptr(kfId); it.Tcw = ptr(Tcw); it.has_corrected = ptr(hasC); it.corrected = ptr(corr); it.has_noncorrected = ptr(hasN); it.noncorrected = ptr(ncorr);
            it.fixed_kf = h[3]; it.n_edges = nE; it.edge_i = ptr(ei); it.edge_j = ptr(ej); it.edge_kind = ptr(kind); it.n_mp = nMp; it.x3Dw = ptr(X); it.mp_ref = ptr(ref);
            it.Siw_out = ptr(Siw); it.Tiw_out = ptr(Tiw); it.x3Dw_out = ptr(Xo);
            if (h[6] == 1) it.edge_i = nullptr; else if (h[6] == 2) it.x3Dw = nullptr; else if (h[6] == 3) it.n_mp = -1; else if (h[6] == 4) it.n_edges = -1;
            if (diag) { it.n_iters = &iters; it.chi2 = &chi2; it.lambda = &lambda; it.n_active = &nAct; it.solver_fail = &fail; }
            const int rc = sindh_essential_graph(&it, 1, h[4]);
            if (rc != h[5]) return 3;
            if (diag) {
                uint64_t cb, sb = 0; std::memcpy(&cb, &chi2, 8);
                if (nKf) std::memcpy(&sb, &Siw[8 * nKf - 1], 8);
                printf("%d %d %d %d %llu %llu\n", rc, iters, nAct, fail, (unsigned long long)cb, (unsigned long long)sb);
            }
        }
    }
    fclose(f);
    return 0;
}
