// The covisibility table (include/sind_hip.h, "sind_covis_*"): the per-element steps of the three walks over MapPoint::mObservations -- KeyFrame::UpdateConnections
// (reference src/KeyFrame.cc:289-320), Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1268-1288), LocalMapping::KeyFrameCulling (src/LocalMapping.cc:645-691) -- on a
// key-frame-major table of cells.  ONE source for the host (covis.cpp: sindh_covis_*) and the device (../covis_kernels.hip), as map_points.hpp is.  Everything is
// integer arithmetic, so the two sides agree in any order of evaluation; the only difference between them is HOW an aggregate is moved (a plain add on the host, an
// integer atomic on the device: the Add parameter of covis_exchange) and how a row's tags are summed (bit by bit on the host, by ballot and popcount on the device).
//   cell (kf, idx)       point (-1: empty) and meta = octave | stereo << 7
//   n_obs[point]         the reference's nObs: 2 per stereo cell, 1 per monocular one (MapPoint.cc:105-108, :119-122)
//   hist[point][octave]  the point's cells by octave: the count of `scaleLeveli <= scaleLevel + 1` (LocalMapping.cc:677) is a prefix of it
//   tag[word][point]     64 query bits per word: bit b of a count call is bit b & 63 of word b >> 6
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "peac_fit.hpp"                                              // SIND_HD
#include "sind_hip.h"

namespace sind {

struct CovisTable {                                                  // host or device pointers
    int* cellPoint; uint8_t* cellMeta;                               // [capKf][capFeat]
    int* nObs; int* hist;                                            // [capPoints], [capPoints][nlevels]
    int capKf, capFeat, capPoints, nlevels;
};

SIND_HD inline uint8_t covis_meta(int octave, int stereo) { return (uint8_t)(octave | (stereo ? 0x80 : 0)); }
SIND_HD inline int covis_octave(uint8_t meta) { return meta & 0x7f; }
SIND_HD inline int covis_stereo(uint8_t meta) { return meta >> 7; }
SIND_HD inline int covis_weight(uint8_t meta) { return (meta & 0x80) ? 2 : 1; }

// One op: the cell takes its new content, the old point loses the cell in its two aggregates and the new one gains it.  No two ops of a call name the same cell, so
// the cell itself is read and written by one lane alone; the aggregates of a point are moved by many and go through add(address, delta).
template <class Add>
SIND_HD inline void covis_exchange(const CovisTable& t, const ::sind_covis_op& op, Add add) {
    const size_t c = (size_t)op.kf * t.capFeat + op.idx;
    const int old = t.cellPoint[c];
    if (old >= 0) {
        const uint8_t m = t.cellMeta[c];
        add(&t.nObs[old], -covis_weight(m)); add(&t.hist[(size_t)old * t.nlevels + covis_octave(m)], -1);
    }
    if (op.point >= 0) {
        const uint8_t m = covis_meta(op.octave, op.stereo);
        t.cellPoint[c] = op.point; t.cellMeta[c] = m;
        add(&t.nObs[op.point], covis_weight(m)); add(&t.hist[(size_t)op.point * t.nlevels + op.octave], 1);
    } else if (old >= 0) {
        t.cellPoint[c] = -1; t.cellMeta[c] = 0;
    }
}

// where bit b of a count call lives
SIND_HD inline int covis_tag_word(int bit) { return bit >> 6; }
SIND_HD inline unsigned long long covis_tag_mask(int bit) { return 1ull << (bit & 63); }

// the tags of the point in cell idx of a row, for one word of 64 bits; an empty cell has none
SIND_HD inline unsigned long long covis_cell_tags(const int* rowPoint, int idx, const unsigned long long* tagWord) {
    const int p = rowPoint[idx];
    return p >= 0 ? tagWord[p] : 0ull;
}

// Entry i of a cull item for key frame kf: `point` seen at `octave`.  -> 1 if the reference's inner loop reaches thObs (LocalMapping.cc:665-687).
SIND_HD inline int covis_cull_entry(const CovisTable& t, int kf, int i, int point, int octave, int thObs) {
    if (!(t.nObs[point] > thObs)) return 0;                          // pMP->Observations() > thObs
    const int* h = t.hist + (size_t)point * t.nlevels;
    const int top = octave + 1 < t.nlevels - 1 ? octave + 1 : t.nlevels - 1;
    int others = 0;
    for (int l = 0; l <= top; l++) others += h[l];
    const int* row = t.cellPoint + (size_t)kf * t.capFeat;
    int own = -1;                                                    // pKFi == pKF: the point's own cell in this key frame does not count
    if (i < t.capFeat && row[i] == point) own = i;
    else for (int j = 0; j < t.capFeat; j++) if (row[j] == point) { own = j; break; }
    if (own >= 0 && covis_octave(t.cellMeta[(size_t)kf * t.capFeat + own]) <= octave + 1) others--;
    return others >= thObs;
}

// ---- what the entry points of both libraries share (covis.cpp) ----
struct CovisDims { int capKf, capFeat, capPoints, nlevels; };
extern const char* const covis_check_text[];
// 0, or an index into covis_check_text (all of them SIND_E_ARG).  stamp: [capKf * capFeat] scratch, epoch its running counter.
int covis_check_ops(const ::sind_covis_op* ops, int n, const CovisDims& d, std::vector<unsigned>& stamp, unsigned& epoch);
int covis_check_queries(const ::sind_covis_query* q, int Q, const CovisDims& d);
int covis_check_cull(const ::sind_covis_cull_item* items, int B, const CovisDims& d);
// The entries of Q lists without the -1s, each with its tag bit: query j owns bits base[j] .. base[j] + mult[j] - 1, mult[j] = how often its list names one point at
// most, and the (t + 1)-th naming of a point gets bit base[j] + t.  occ / occStamp: [capPoints] scratch.  -> the number of bits
int covis_assign_bits(const ::sind_covis_query* q, int Q, std::vector<int>& occ, std::vector<unsigned>& occStamp, unsigned& epoch, std::vector<int>& entPoint,
                      std::vector<int>& entBit, std::vector<int>& base, std::vector<int>& mult);
// count[k] of query j from the per-bit counts perBit[bit * stride + k], k < rows; the rows above are 0
void covis_sum_bits(const ::sind_covis_query& q, int base, int mult, const int* perBit, size_t stride, int rows, int capKf);

}  // namespace sind
