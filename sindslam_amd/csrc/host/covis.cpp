// Host twins of sind_covis_* (reference src/KeyFrame.cc:289-320, src/Tracking.cc:1268-1288, src/LocalMapping.cc:645-691): covis.hpp run op after op, cell after cell
// and entry after entry on a table in host memory, and what the entry points of both libraries share: the argument checks, the tag bits of a count call and the sum
// over a query's bits.  Compiled into libsind_hip.so (capi_covis.cpp calls the shared part) and into libsind_host.so.
#include <algorithm>
#include <cstring>
#include <vector>
#include "covis.hpp"
#include "sind_hip.h"

namespace sind {

const char* const covis_check_text[] = {"", "negative count", "null array", "a key frame is out of range", "a feature index is out of range", "a point is out of range",
                                        "an octave is out of range", "two ops on one cell", "null output"};

static unsigned next_epoch(std::vector<unsigned>& stamp, unsigned& epoch) {
    if (++epoch == 0) { std::fill(stamp.begin(), stamp.end(), 0u); epoch = 1; }
    return epoch;
}

int covis_check_ops(const ::sind_covis_op* ops, int n, const CovisDims& d, std::vector<unsigned>& stamp, unsigned& epoch) {
    if (n < 0) return 1;
    if (n && !ops) return 2;
    for (int i = 0; i < n; i++) {
        const ::sind_covis_op& o = ops[i];
        if (o.kf < 0 || o.kf >= d.capKf) return 3;
        if (o.idx < 0 || o.idx >= d.capFeat) return 4;
        if (o.point < -1 || o.point >= d.capPoints) return 5;
        if (o.point >= 0 && (o.octave < 0 || o.octave >= d.nlevels)) return 6;
    }
    const unsigned e = next_epoch(stamp, epoch);
    for (int i = 0; i < n; i++) {
        unsigned& s = stamp[(size_t)ops[i].kf * d.capFeat + ops[i].idx];
        if (s == e) return 7;
        s = e;
    }
    return 0;
}

int covis_check_queries(const ::sind_covis_query* q, int Q, const CovisDims& d) {
    if (Q < 0) return 1;
    if (Q && !q) return 2;
    for (int j = 0; j < Q; j++) {
        if (q[j].n < 0) return 1;
        if (q[j].n && !q[j].points) return 2;
        if (!q[j].count) return 8;
        if (q[j].self_kf < -1 || q[j].self_kf >= d.capKf) return 3;
        for (int i = 0; i < q[j].n; i++) if (q[j].points[i] < -1 || q[j].points[i] >= d.capPoints) return 5;
    }
    return 0;
}

int covis_check_cull(const ::sind_covis_cull_item* items, int B, const CovisDims& d) {
    if (B < 0) return 1;
    if (B && !items) return 2;
    for (int b = 0; b < B; b++) {
        const ::sind_covis_cull_item& it = items[b];
        if (it.n < 0) return 1;
        if (it.n && (!it.points || !it.octave || !it.close)) return 2;
        if (!it.n_mps || !it.n_redundant) return 8;
        if (it.kf < 0 || it.kf >= d.capKf) return 3;
        for (int i = 0; i < it.n; i++) {
            if (it.points[i] < -1 || it.points[i] >= d.capPoints) return 5;
            if (it.points[i] >= 0 && it.close[i] && it.octave[i] >= d.nlevels) return 6;
        }
    }
    return 0;
}

int covis_assign_bits(const ::sind_covis_query* q, int Q, std::vector<int>& occ, std::vector<unsigned>& occStamp, unsigned& epoch, std::vector<int>& entPoint,
                      std::vector<int>& entBit, std::vector<int>& base, std::vector<int>& mult) {
    entPoint.clear(); entBit.clear(); base.assign(Q, 0); mult.assign(Q, 0);
    int bits = 0;
    for (int j = 0; j < Q; j++) {
        const unsigned e = next_epoch(occStamp, epoch);
        base[j] = bits;
        for (int i = 0; i < q[j].n; i++) {
            const int p = q[j].points[i];
            if (p < 0) continue;
            if (occStamp[p] != e) { occStamp[p] = e; occ[p] = 0; }
            const int t = occ[p]++;
            entPoint.push_back(p); entBit.push_back(bits + t);
            mult[j] = std::max(mult[j], t + 1);
        }
        bits += mult[j];
    }
    return bits;
}

void covis_sum_bits(const ::sind_covis_query& q, int base, int mult, const int* perBit, size_t stride, int rows, int capKf) {
    for (int k = 0; k < capKf; k++) {
        int c = 0;
        if (k < rows && k != q.self_kf) for (int t = 0; t < mult; t++) c += perBit[(size_t)(base + t) * stride + k];
        q.count[k] = c;
    }
}

}  // namespace sind

using namespace sind;

struct sindh_covis {
    CovisDims d{}; int rows = 0;                                      // rows: the highest key frame ever set + 1
    std::vector<int> cellPoint, nObs, hist, occ; std::vector<uint8_t> cellMeta; std::vector<unsigned long long> tag;      // tag: [words][capPoints], grows with the calls
    std::vector<unsigned> stamp, occStamp; unsigned epoch = 0, occEpoch = 0;
    CovisTable table() { return CovisTable{cellPoint.data(), cellMeta.data(), nObs.data(), hist.data(), d.capKf, d.capFeat, d.capPoints, d.nlevels}; }
};

namespace {
struct PlainAdd { void operator()(int* p, int v) const { *p += v; } };
}

extern "C" {

int sindh_covis_create(int cap_kf, int cap_feat, int cap_points, int nlevels, int, int, sindh_covis** out) {
    if (!out || cap_kf < 1 || cap_feat < 1 || cap_points < 1 || nlevels < 1) return SIND_E_ARG;
    if (nlevels > 16) return SIND_E_CAPACITY;
    sindh_covis* c = new sindh_covis(); c->d = CovisDims{cap_kf, cap_feat, cap_points, nlevels};
    const size_t cells = (size_t)cap_kf * cap_feat;
    c->cellPoint.assign(cells, -1); c->cellMeta.assign(cells, 0); c->stamp.assign(cells, 0u);
    c->nObs.assign(cap_points, 0); c->hist.assign((size_t)cap_points * nlevels, 0); c->occ.assign(cap_points, 0); c->occStamp.assign(cap_points, 0u);
    *out = c; return SIND_OK;
}

int sindh_covis_destroy(sindh_covis* c) { delete c; return SIND_OK; }

int sindh_covis_clear(sindh_covis* c) {
    if (!c) return SIND_E_ARG;
    std::fill(c->cellPoint.begin(), c->cellPoint.end(), -1); std::fill(c->cellMeta.begin(), c->cellMeta.end(), (uint8_t)0);
    std::fill(c->nObs.begin(), c->nObs.end(), 0); std::fill(c->hist.begin(), c->hist.end(), 0); c->rows = 0;
    return SIND_OK;
}

int sindh_covis_apply(sindh_covis* c, const sind_covis_op* ops, int n) {
    if (!c) return SIND_E_ARG;
    if (covis_check_ops(ops, n, c->d, c->stamp, c->epoch)) return SIND_E_ARG;
    const CovisTable t = c->table();
    for (int i = 0; i < n; i++) { covis_exchange(t, ops[i], PlainAdd()); if (ops[i].point >= 0) c->rows = std::max(c->rows, ops[i].kf + 1); }
    return SIND_OK;
}

int sindh_covis_read_row(sindh_covis* c, int kf, int* point, uint8_t* octave, uint8_t* stereo) {
    if (!c || !point || !octave || !stereo || kf < 0 || kf >= c->d.capKf) return SIND_E_ARG;
    const size_t o = (size_t)kf * c->d.capFeat;
    for (int i = 0; i < c->d.capFeat; i++) { point[i] = c->cellPoint[o + i]; octave[i] = (uint8_t)covis_octave(c->cellMeta[o + i]); stereo[i] = (uint8_t)covis_stereo(c->cellMeta[o + i]); }
    return SIND_OK;
}

int sindh_covis_read_points(sindh_covis* c, const int* points, int n, int* n_obs, int* hist) {
    if (!c || n < 0 || (n && (!points || !n_obs || !hist))) return SIND_E_ARG;
    for (int i = 0; i < n; i++) if (points[i] < 0 || points[i] >= c->d.capPoints) return SIND_E_ARG;
    const int L = c->d.nlevels;
    for (int i = 0; i < n; i++) { n_obs[i] = c->nObs[points[i]]; std::memcpy(hist + (size_t)i * L, &c->hist[(size_t)points[i] * L], L * sizeof(int)); }
    return SIND_OK;
}

int sindh_covis_count(sindh_covis* c, const sind_covis_query* q, int Q) {
    if (!c) return SIND_E_ARG;
    if (covis_check_queries(q, Q, c->d)) return SIND_E_ARG;
    std::vector<int> entPoint, entBit, base, mult;
    const int bits = covis_assign_bits(q, Q, c->occ, c->occStamp, c->occEpoch, entPoint, entBit, base, mult);
    const int words = (bits + 63) / 64, rows = c->rows; const size_t P = c->d.capPoints;
    if (c->tag.size() < words * P) c->tag.resize(words * P, 0ull);
    for (size_t e = 0; e < entPoint.size(); e++) c->tag[covis_tag_word(entBit[e]) * P + entPoint[e]] |= covis_tag_mask(entBit[e]);
    std::vector<int> perBit((size_t)bits * std::max(rows, 1), 0);
    for (int w = 0; w < words; w++)
        for (int k = 0; k < rows; k++) {
            const int* row = &c->cellPoint[(size_t)k * c->d.capFeat];
            for (int i = 0; i < c->d.capFeat; i++)
                for (unsigned long long m = covis_cell_tags(row, i, &c->tag[w * P]); m; m &= m - 1) perBit[(size_t)(w * 64 + __builtin_ctzll(m)) * rows + k]++;
        }
    for (size_t e = 0; e < entPoint.size(); e++) c->tag[covis_tag_word(entBit[e]) * P + entPoint[e]] &= ~covis_tag_mask(entBit[e]);
    for (int j = 0; j < Q; j++) covis_sum_bits(q[j], base[j], mult[j], perBit.data(), rows, rows, c->d.capKf);
    return SIND_OK;
}

int sindh_covis_cull(sindh_covis* c, const sind_covis_cull_item* items, int B, int th_obs) {
    if (!c) return SIND_E_ARG;
    if (covis_check_cull(items, B, c->d)) return SIND_E_ARG;
    const CovisTable t = c->table();
    for (int b = 0; b < B; b++) {
        const sind_covis_cull_item& it = items[b]; int mps = 0, red = 0;
        for (int i = 0; i < it.n; i++) {
            int r = 0;
            if (it.points[i] >= 0 && it.close[i]) { mps++; r = covis_cull_entry(t, it.kf, i, it.points[i], it.octave[i], th_obs); red += r; }
            if (it.redundant) it.redundant[i] = (uint8_t)r;
        }
        *it.n_mps = mps; *it.n_redundant = red;
    }
    return SIND_OK;
}

}  // extern "C"
