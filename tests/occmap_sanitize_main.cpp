// Stand-alone driver of sindh_occmap_* for an AddressSanitizer / UBSan build (tests/test_occmap_cpu.py builds it with csrc/host/occmap.cpp and runs it as its own
// process).  Input: a file written by the test: int32 count, then per record float64 resolution; int32 max_voxels, max_points, calls; per call int32 B, stride, the
// expected return code; n_points i32 [B]; origins f32 [B][3]; points [B][stride] of 16 bytes.  Every array has exactly as many entries as the call may touch: an
// access past the end is a report.  Output: per record one line: per call " return-code" and the sums of the five stats over its key frames, then the map's size, the
// number of occupied voxels, the xor of (their x, y, z bits * (i + 1)) and the sum of (b + 2 g + 3 r) * (i + 1) over them.
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
    int32_t count;
    if (!get(f, &count, 1)) return 2;
    for (int k = 0; k < count; k++) {
        double res; int32_t h[3];
        if (!get(f, &res, 1) || !get(f, h, 3)) return 2;
        sindh_occmap* m = nullptr;
        if (sindh_occmap_create(res, 0.7, 0.4, 0.1192, 0.971, 0.7, h[0], h[1], &m) != SIND_OK) return 3;
        for (int c = 0; c < h[2]; c++) {
            int32_t g[3];
            if (!get(f, g, 3)) return 2;
            const int B = g[0], stride = g[1];
            std::vector<int32_t> n(B); std::vector<float> org((size_t)B * 3); std::vector<sind_cloud_point> pts((size_t)B * stride); std::vector<sind_occmap_stats> st(B);
            if (!get(f, n.data(), n.size()) || !get(f, org.data(), org.size()) || !get(f, pts.data(), pts.size())) return 2;
            const int rc = sindh_occmap_insert(m, B, ptr(pts), stride, ptr(n), ptr(org), ptr(st));
            if (rc != g[2]) return 4;
            long long s[5] = {0, 0, 0, 0, 0};
            for (int b = 0; b < B; b++) { s[0] += st[b].n_rays; s[1] += st[b].n_skipped; s[2] += st[b].n_coloured; s[3] += st[b].n_miss_updates; s[4] += st[b].n_new_voxels; }
            printf(" %d %lld %lld %lld %lld %lld", rc, s[0], s[1], s[2], s[3], s[4]);
        }
        int nOcc = 0;
        if (sindh_occmap_occupied(m, nullptr, 0, &nOcc) != SIND_OK) return 5;
        std::vector<sind_cloud_point> occ(nOcc);
        if (sindh_occmap_occupied(m, ptr(occ), nOcc, &nOcc) != SIND_OK) return 5;
        if (nOcc > 0 && sindh_occmap_occupied(m, ptr(occ), nOcc - 1, &nOcc) != SIND_E_CAPACITY) return 6;
        uint32_t x = 0; long long s = 0;
        for (int i = 0; i < nOcc; i++) {
            uint32_t u[3]; std::memcpy(u, &occ[i].x, 12);
            x ^= (u[0] ^ (u[1] * 3u) ^ (u[2] * 5u)) * (uint32_t)(i + 1); s += (long long)(occ[i].b + 2 * occ[i].g + 3 * occ[i].r) * (i + 1);
        }
        std::vector<uint16_t> keys(3 * (size_t)nOcc, 32768); std::vector<uint8_t> known(nOcc), rgb(3 * (size_t)nOcc); std::vector<uint32_t> lo(nOcc);
        if (sindh_occmap_read(m, ptr(keys), nOcc, ptr(known), ptr(lo), ptr(rgb)) != SIND_OK) return 7;
        printf(" %d %d %u %lld\n", sindh_occmap_size(m), nOcc, x, s);
        sindh_occmap_clear(m);
        if (sindh_occmap_size(m) != 0) return 8;
        sindh_occmap_destroy(m);
    }
    fclose(f);
    return 0;
}
