// Stand-alone driver of sindh_triangulate and sindh_update_points for an AddressSanitizer / UBSan build (tests/test_mappoints_cpu.py builds it with
// csrc/host/map_points.cpp and runs it as its own process).  Input: a file written by the test: float K5[5], int32 nlevels, float scale[nlevels], int32 count, then per
// record int32 kind (0 a pair, 1 an item) and the expected return code, and
//   a pair: int32 n1, n2; Tcw1, Twc1, Tcw2, Twc2 [16] each; per side xy [n][2], un_xy [n][2], octave i32 [n], u_right [n], depth [n]; match12 i32 [n1]
//   an item: int32 n_kf, n_mp, n_obs, do_descriptor, do_normal; Ow [n_kf][3], x3Dw [n_mp][3], obs_start i32 [n_mp + 1], obs_kf i32 [n_obs], obs_bad u8 [n_obs],
//            obs_octave i32 [n_obs], obs_desc u8 [n_obs][32], ref_obs i32 [n_mp]
// Every array has exactly as many entries as the call may read: a read past the end is a report.
// Output: per record one line: a pair "return-code nnew sum-of-status bits-of-x3D-xor"; an item "return-code sum-of-best_obs sum-of-updated bits-of-max_dist-xor".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sind_hip.h"

template <class T> static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

struct Side { std::vector<float> xy, un, ur, dp; std::vector<int32_t> oct; };
static bool get_side(FILE* f, int n, Side& s) {
    s.xy.resize(2 * n); s.un.resize(2 * n); s.oct.resize(n); s.ur.resize(n); s.dp.resize(n);
    return get(f, s.xy.data(), s.xy.size()) && get(f, s.un.data(), s.un.size()) && get(f, s.oct.data(), s.oct.size()) && get(f, s.ur.data(), s.ur.size()) && get(f, s.dp.data(), s.dp.size());
}
static sind_tri_side side_of(Side& s, int n) { return sind_tri_side{n, ptr(s.xy), ptr(s.un), ptr(s.oct), ptr(s.ur), ptr(s.dp)}; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    float K5[5]; int32_t nlevels = 0, count = 0;
    if (!get(f, K5, 5) || !get(f, &nlevels, 1) || nlevels < 1 || nlevels > 16) return 2;
    std::vector<float> scale(nlevels);
    if (!get(f, scale.data(), scale.size()) || !get(f, &count, 1)) return 2;
    for (int k = 0; k < count; k++) {
        int32_t kind[2];
        if (!get(f, kind, 2)) return 2;
        if (kind[0] == 0) {
            int32_t n[2]; float T[4][16]; Side s1, s2;
            if (!get(f, n, 2) || !get(f, &T[0][0], 64) || !get_side(f, n[0], s1) || !get_side(f, n[1], s2)) return 2;
            std::vector<int32_t> m12(n[0]), how(n[0], 77), status(n[0], 77); std::vector<float> X(3 * n[0], 7.f); int nnew = 77;
            if (!get(f, m12.data(), m12.size())) return 2;
            sind_tri_pair p{T[0], T[1], T[2], T[3], side_of(s1, n[0]), side_of(s2, n[1]), ptr(m12), ptr(X), ptr(how), ptr(status), &nnew};
            const int rc = sindh_triangulate(&p, 1, K5, scale.data(), nlevels);
            if (rc != kind[1]) return 3;
            long long ss = 0; uint32_t x = 0;
            for (int i = 0; i < n[0]; i++) ss += status[i];
            for (float v : X) { uint32_t b; std::memcpy(&b, &v, 4); x ^= b; }
            printf("%d %d %lld %u\n", rc, nnew, ss, x);
        } else {
            int32_t h[5];
            if (!get(f, h, 5)) return 2;
            const int nKf = h[0], nMp = h[1], nObs = h[2];
            std::vector<float> Ow(3 * nKf), X(3 * nMp); std::vector<int32_t> start(nMp + 1), okf(nObs), ooct(nObs), ref(nMp); std::vector<uint8_t> obad(nObs), odesc(32 * (size_t)nObs);
            if (!get(f, Ow.data(), Ow.size()) || !get(f, X.data(), X.size()) || !get(f, start.data(), start.size()) || !get(f, okf.data(), okf.size()) || !get(f, obad.data(), obad.size()) ||
                !get(f, ooct.data(), ooct.size()) || !get(f, odesc.data(), odesc.size()) || !get(f, ref.data(), ref.size())) return 2;
            std::vector<uint8_t> desc(32 * (size_t)nMp, 0xAB), updated(nMp, 7); std::vector<int32_t> best(nMp, 77); std::vector<float> normal(3 * nMp, 7.f), maxd(nMp, 7.f), mind(nMp, 7.f);
            sind_mappoints_item it{nKf, ptr(Ow), nMp, ptr(X), start.data(), ptr(okf), ptr(obad), ptr(ooct), ptr(odesc), ptr(ref), h[3], h[4], ptr(desc), ptr(best), ptr(normal), ptr(maxd), ptr(mind), ptr(updated)};
            if (!nMp) it.obs_start = nullptr;
            const int rc = sindh_update_points(&it, 1, scale.data(), nlevels);
            if (rc != kind[1]) return 3;
            long long sb = 0, su = 0; uint32_t x = 0;
            for (int j = 0; j < nMp; j++) { sb += best[j]; su += updated[j]; uint32_t b; std::memcpy(&b, &maxd[j], 4); x ^= b; }
            printf("%d %lld %lld %u\n", rc, sb, su, x);
        }
    }
    fclose(f);
    return 0;
}
