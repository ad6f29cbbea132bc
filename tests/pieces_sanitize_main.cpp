// Stand-alone sanitizer program over the host twin of the piece extraction (sindh_find_contours, sindh_seg_pieces of csrc/host/host_capi.cpp): reads one frame written by
// tests/test_pieces_cpu.py (w, h, k, depth scale as int32; k cluster planes, occ1, labelForSegEdge as bit planes; the u16 depth) and prints the piece count, a byte
// checksum of every output and the number of external contours of the cluster planes.  Built with -fsanitize=address,undefined; nothing is loaded into python.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int sindh_find_contours(const uint8_t* src, int w, int h, int external_only, int* pts_xy, int cap_pts, int* lens, int cap_contours);
int sindh_seg_pieces(const uint64_t* planes, int k, const uint64_t* occ1, const uint64_t* label_edge, const uint16_t* depth, int w, int h, float depth_scale, int cap,
                     int* recs, float* vals, uint64_t* piece_planes, uint64_t* conn_planes, uint8_t* piece_of);
}

template <class T> static unsigned long long bytesum(const T* p, size_t n) { const uint8_t* b = reinterpret_cast<const uint8_t*>(p); unsigned long long s = 0; for (size_t i = 0; i < n * sizeof(T); i++) s += b[i]; return s; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb"); if (!f) return 2;
    int hd[4]; if (std::fread(hd, 4, 4, f) != 4) return 2;
    const int w = hd[0], h = hd[1], k = hd[2], wpr = (w + 63) / 64; const size_t pw = (size_t)h * wpr, N = (size_t)w * h;
    std::vector<uint64_t> planes(k * pw), occ1(pw), edge(pw); std::vector<uint16_t> depth(N);
    if (std::fread(planes.data(), 8, planes.size(), f) != planes.size() || std::fread(occ1.data(), 8, pw, f) != pw || std::fread(edge.data(), 8, pw, f) != pw || std::fread(depth.data(), 2, N, f) != N) return 2;
    std::fclose(f);
    const int cap = 64;
    std::vector<int> recs((size_t)cap * 12, -7); std::vector<float> vals((size_t)cap * 2, -7.f); std::vector<uint64_t> pl(cap * pw, 0), cn(cap * pw, 0); std::vector<uint8_t> po(N, 251);
    const int n = sindh_seg_pieces(planes.data(), k, occ1.data(), edge.data(), depth.data(), w, h, (float)hd[3], cap, recs.data(), vals.data(), pl.data(), cn.data(), po.data());
    if (n < 0 || n > cap) return 3;
    int ncont = 0;
    for (int i = 0; i < k; i++) {
        std::vector<uint8_t> img(N);
        for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) img[(size_t)y * w + x] = ((planes[i * pw + (size_t)y * wpr + (x >> 6)] >> (x & 63)) & 1) ? 255 : 0;
        std::vector<int> pts(N * 8), lens(N);
        ncont += sindh_find_contours(img.data(), w, h, 1, pts.data(), (int)(N * 4), lens.data(), (int)N);
    }
    std::printf("%d %llu %llu %llu %llu %llu %d\n", n, bytesum(recs.data(), (size_t)n * 12), bytesum(vals.data(), (size_t)n * 2), bytesum(pl.data(), n * pw), bytesum(cn.data(), n * pw), bytesum(po.data(), N), ncont);
    return 0;
}
