// Stand-alone driver of sindh_cloud_filter_outliers for an AddressSanitizer / UBSan build (tests/test_cloud_filter_cpu.py builds it with csrc/host/cloud_filter.cpp
// and runs it as its own process).  Input: a file written by the test: int32 count, then per record int32 B, stride, mean_k, out_cap, the expected return code; float64
// stddev_mul; n_points i32 [B]; points [B][stride] of 16 bytes.  Every array has exactly as many entries as the call may touch: an access past the end is a report.
// Output: per record one line "return-code" and per cloud " n_out valid degenerate xor-of-distance-bits sum-of-kept-colour-bytes".
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
    int32_t count;
    if (!get(f, &count, 1)) return 2;
    for (int k = 0; k < count; k++) {
        int32_t h[5]; double mul;
        if (!get(f, h, 5) || !get(f, &mul, 1)) return 2;
        const int B = h[0], stride = h[1], meanK = h[2], outCap = h[3];
        std::vector<int32_t> n(B), nOut(B > 0 ? B : 1, 77); std::vector<sind_cloud_point> pts((size_t)B * stride), out((size_t)B * outCap);
        std::vector<float> dist((size_t)B * stride); std::vector<sind_cloud_filter_stats> st(B);
        if (!get(f, n.data(), n.size()) || !get(f, pts.data(), pts.size())) return 2;
        const int rc = sindh_cloud_filter_outliers(B, ptr(pts), stride, ptr(n), meanK, mul, ptr(out), outCap, nOut.data(), ptr(dist), ptr(st));
        if (rc != h[4]) return 3;
        printf("%d", rc);
        if (rc == SIND_E_ARG) { if (nOut[0] != 77) return 4; printf("\n"); continue; }
        for (int b = 0; b < B; b++) {
            uint32_t x = 0; long long s = 0;
            for (int i = 0; i < n[b]; i++) { union { float f; uint32_t u; } v; v.f = dist[(size_t)b * stride + i]; x ^= v.u * (uint32_t)(i + 1); }
            for (int i = 0; i < nOut[b] && i < outCap; i++) { const sind_cloud_point& p = out[(size_t)b * outCap + i]; s += (long long)(p.b + 2 * p.g + 3 * p.r) * (i + 1); }
            printf(" %d %d %d %u %lld", nOut[b], st[b].valid, st[b].degenerate, x, s);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
