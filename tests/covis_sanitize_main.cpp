// Stand-alone driver of sindh_covis_* for an AddressSanitizer / UBSan build (tests/test_covis_cpu.py builds it with csrc/host/covis.cpp and runs it as its own
// process).  Input: a file written by the test: int32 cap_kf, cap_feat, cap_points, nlevels, count, then per record int32 kind and the expected return code, and
//   kind 0, apply: int32 n; ops [n][5]
//   kind 1, count: int32 self_kf, n; points i32 [n]
//   kind 2, cull:  int32 kf, n; points i32 [n], octave u8 [n], close u8 [n]
// Every array has exactly as many entries as the call may read: a read past the end is a report.
// Output: per record one line.  apply: "return-code sum-of-n_obs sum-of-hist[l]*(l+1) sum-of-all-cells" (the state, also after a rejected call); count: "return-code
// sum-of-count sum-of-count[k]*(k+1)"; cull: "return-code n_mps n_redundant sum-of-redundant"; a rejected count or cull: the return code alone.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sind_hip.h"

template <class T> static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[5];
    if (!get(f, h, 5)) return 2;
    const int capKf = h[0], capFeat = h[1], capPoints = h[2], nlevels = h[3], count = h[4];
    sindh_covis* c = nullptr;
    if (sindh_covis_create(capKf, capFeat, capPoints, nlevels, 1, 0, &c) != SIND_OK) return 2;
    for (int k = 0; k < count; k++) {
        int32_t kind[2];
        if (!get(f, kind, 2)) return 2;
        if (kind[0] == 0) {
            int32_t n;
            if (!get(f, &n, 1)) return 2;
            std::vector<sind_covis_op> ops(n);
            if (!get(f, ops.data(), ops.size())) return 2;
            const int rc = sindh_covis_apply(c, ptr(ops), n);
            if (rc != kind[1]) return 3;
            std::vector<int> ids(capPoints), nObs(capPoints), hist((size_t)capPoints * nlevels), point(capFeat); std::vector<uint8_t> octave(capFeat), stereo(capFeat);
            for (int p = 0; p < capPoints; p++) ids[p] = p;
            if (sindh_covis_read_points(c, ids.data(), capPoints, nObs.data(), hist.data()) != SIND_OK) return 3;
            long long so = 0, sh = 0, sc = 0;
            for (int p = 0; p < capPoints; p++) { so += nObs[p]; for (int l = 0; l < nlevels; l++) sh += (long long)hist[(size_t)p * nlevels + l] * (l + 1); }
            for (int kf = 0; kf < capKf; kf++) {
                if (sindh_covis_read_row(c, kf, point.data(), octave.data(), stereo.data()) != SIND_OK) return 3;
                for (int i = 0; i < capFeat; i++) sc += point[i];
            }
            printf("%d %lld %lld %lld\n", rc, so, sh, sc);
        } else if (kind[0] == 1) {
            int32_t a[2];
            if (!get(f, a, 2)) return 2;
            std::vector<int32_t> points(a[1]), out(capKf, 77);
            if (!get(f, points.data(), points.size())) return 2;
            sind_covis_query q{a[0], a[1], ptr(points), out.data()};
            const int rc = sindh_covis_count(c, &q, 1);
            if (rc != kind[1]) return 3;
            if (rc != SIND_OK) { for (int v : out) if (v != 77) return 4; printf("%d\n", rc); continue; }
            long long s = 0, sw = 0;
            for (int kf = 0; kf < capKf; kf++) { s += out[kf]; sw += (long long)out[kf] * (kf + 1); }
            printf("%d %lld %lld\n", rc, s, sw);
        } else {
            int32_t a[2];
            if (!get(f, a, 2)) return 2;
            const int n = a[1] > 0 ? a[1] : 0;
            std::vector<int32_t> points(n); std::vector<uint8_t> octave(n), close(n), red(n, 77); int nMps = 77, nRed = 77;
            if (!get(f, points.data(), points.size()) || !get(f, octave.data(), octave.size()) || !get(f, close.data(), close.size())) return 2;
            sind_covis_cull_item it{a[0], a[1], ptr(points), ptr(octave), ptr(close), &nMps, &nRed, ptr(red)};
            const int rc = sindh_covis_cull(c, &it, 1, 3);
            if (rc != kind[1]) return 3;
            if (rc != SIND_OK) { if (nMps != 77 || nRed != 77) return 4; printf("%d\n", rc); continue; }
            long long s = 0;
            for (uint8_t v : red) s += v;
            printf("%d %d %d %lld\n", rc, nMps, nRed, s);
        }
    }
    sindh_covis_destroy(c);
    fclose(f);
    return 0;
}
