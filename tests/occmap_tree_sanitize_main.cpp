// Stand-alone driver of sindh_occmap_tree / sindh_occmap_write_ot for an AddressSanitizer / UBSan build (tests/test_occmap_tree_cpu.py builds it with
// csrc/host/occmap.cpp and csrc/host/occmap_tree.cpp and runs it as its own process).  Input: the file format of tests/occmap_sanitize_main.cpp (int32 count, then per
// record float64 resolution; int32 max_voxels, max_points, calls; per call int32 B, stride, the expected return code; n_points i32 [B]; origins f32 [B][3]; points
// [B][stride] of 16 bytes).  After a record's inserts, for every (prune, inner_colour, occupied_only): the counts with NULL outputs, then the outputs into arrays of
// EXACTLY the reported sizes (an access past the end is a report), then capacities one short.  Output: per record and setting one line: the stats, the number of listed
// leaves, an FNV-1a hash of the stream, of the leaves and of their depths; then the size of the .ot file written to argv[2].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "sind_hip.h"

template <class T> static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T> static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
static uint64_t fnv(const void* p, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; i++) { h ^= ((const uint8_t*)p)[i]; h *= 1099511628211ull; } return h; }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
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
            std::vector<int32_t> n(B); std::vector<float> org((size_t)B * 3); std::vector<sind_cloud_point> pts((size_t)B * stride);
            if (!get(f, n.data(), n.size()) || !get(f, org.data(), org.size()) || !get(f, pts.data(), pts.size())) return 2;
            if (sindh_occmap_insert(m, B, ptr(pts), stride, ptr(n), ptr(org), nullptr) != g[2]) return 4;
        }
        for (int flags = 0; flags < 8; flags++) {
            const int prune = flags & 1, colour = (flags >> 1) & 1, occ = (flags >> 2) & 1;
            sind_occmap_tree_stats st, st2; int nl = -1, nl2 = -1;
            if (sindh_occmap_tree(m, prune, colour, occ, nullptr, 0, nullptr, nullptr, 0, &nl, &st) != SIND_OK) return 5;
            std::vector<uint8_t> data((size_t)st.n_nodes * 8), depth(nl); std::vector<sind_cloud_point> leaves(nl);
            // an empty vector's data() may be NULL, which would mean "not wanted": give the call a valid address and a capacity of zero instead
            uint8_t none8 = 0; sind_cloud_point noneP{};
            if (sindh_occmap_tree(m, prune, colour, occ, data.empty() ? &none8 : data.data(), data.size(), leaves.empty() ? &noneP : leaves.data(), depth.empty() ? &none8 : depth.data(), nl, &nl2, &st2) != SIND_OK) return 6;
            if (nl2 != nl || std::memcmp(&st, &st2, sizeof(st)) != 0 || none8 != 0) return 7;
            if (st.n_nodes > 0 && sindh_occmap_tree(m, prune, colour, occ, data.data(), data.size() - 1, nullptr, nullptr, 0, nullptr, &st2) != SIND_E_CAPACITY) return 8;
            if (nl > 0 && sindh_occmap_tree(m, prune, colour, occ, nullptr, 0, leaves.data(), depth.data(), nl - 1, &nl2, &st2) != SIND_E_CAPACITY) return 8;
            if (std::memcmp(&st, &st2, sizeof(st)) != 0) return 9;    // the counts are filled on SIND_E_CAPACITY too
            printf("%d %d %d %d %d", st.n_nodes, st.n_inner, st.n_leaves, st.n_pruned, st.n_occupied_leaves);
            for (int d = 0; d < 17; d++) printf(" %d", st.leaves_at_depth[d]);
            printf(" %d %llu %llu %llu\n", nl, (unsigned long long)fnv(data.data(), data.size()), (unsigned long long)fnv(leaves.data(), leaves.size() * sizeof(sind_cloud_point)),
                   (unsigned long long)fnv(depth.data(), depth.size()));
        }
        if (sindh_occmap_write_ot(m, 1, 0, argv[2]) != SIND_OK) return 10;
        FILE* o = fopen(argv[2], "rb");
        if (!o) return 10;
        fseek(o, 0, SEEK_END); printf("%ld\n", ftell(o)); fclose(o);
        sindh_occmap_destroy(m);
    }
    fclose(f);
    return 0;
}
