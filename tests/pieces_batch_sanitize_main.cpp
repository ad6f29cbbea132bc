// Stand-alone sanitizer program over the host step of the batched piece stage (sindh_seg_pieces_order of csrc/host/host_capi.cpp: records -> ranked order table): reads the
// frames written by tests/test_pieces_batch_cpu.py (per frame: C as int32, then C records of 16 int32 in PieceRecDev's layout) and prints, per frame, the return value and
// the order, has_conn and score tables it filled.  The tables have exactly the documented 255 entries, so a write past them is seen.  Built with
// -fsanitize=address,undefined; nothing is loaded into python.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int sindh_seg_pieces_order(const int* recs, int C, int* order, int* has_conn, float* score);

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb"); if (!f) return 2;
    int C = 0;
    while (std::fread(&C, 4, 1, f) == 1) {
        if (C < 0 || C > 4096) return 2;
        std::vector<int> recs((size_t)C * 16);
        if (C > 0 && std::fread(recs.data(), 64, (size_t)C, f) != (size_t)C) return 2;
        std::vector<int> order(255, -7), conn(255, -7); std::vector<float> score(255, -7.f);
        const int n = sindh_seg_pieces_order(C > 0 ? recs.data() : nullptr, C, order.data(), conn.data(), score.data());
        std::printf("%d", n);
        for (int r = 0; r < (n > 0 ? n : 0); r++) { uint32_t bits; std::memcpy(&bits, &score[r], 4); std::printf(" %d %d %u", order[r], conn[r], bits); }
        for (int r = (n > 0 ? n : 0); r < 255; r++) if (order[r] != -7 || conn[r] != -7 || score[r] != -7.f) return 3;      // nothing behind the frame's pieces is touched
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
