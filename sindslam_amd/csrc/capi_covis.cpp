// C ABI: the covisibility table (include/sind_hip.h, "sind_covis_*").  The argument checks, the tag bits and the sum over a query's bits are host/covis.cpp's, shared
// with the host twin; here: the capacities, the staging and the launches.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/sind_hip.h"
#include "covis_dev.hpp"

using namespace sind;

struct sind_covis {
    int device = 0, maxQ = 0, maxBits = 0, rows = 0; CovisDims d{}; hipStream_t stream = nullptr;      // rows: the highest key frame ever set + 1
    DevBuf<int> cellPoint, nObs, hist; DevBuf<uint8_t> cellMeta; DevBuf<unsigned long long> tag;       // tag: [maxBits / 64][capPoints], zero between the calls
    Staged<::sind_covis_op> ops;                                     // grows to the largest apply seen
    Staged<int> entPoint, entBit, itemStart, itemKf, counts, perBit; Staged<uint8_t> entOctave, entClose, redundant;      // [maxQ * capFeat] per entry, [maxQ (+ 1)] per item, [maxBits][capKf]
    std::vector<int> hNObs, hHist, hRowPoint; std::vector<uint8_t> hRowMeta;      // read-backs
    std::vector<unsigned> stamp, occStamp; std::vector<int> occ, ePoint, eBit, base, mult; unsigned epoch = 0, occEpoch = 0;
    CovisTable table() const { return CovisTable{cellPoint.p, cellMeta.p, nObs.p, hist.p, d.capKf, d.capFeat, d.capPoints, d.nlevels}; }
};

namespace {
int reset_state(sind_covis* c) {
    const size_t cells = (size_t)c->d.capKf * c->d.capFeat, P = c->d.capPoints;
    HIP_TRY(hipMemsetAsync(c->cellPoint.p, 0xFF, cells * sizeof(int), c->stream)); HIP_TRY(hipMemsetAsync(c->cellMeta.p, 0, cells, c->stream));
    HIP_TRY(hipMemsetAsync(c->nObs.p, 0, P * sizeof(int), c->stream)); HIP_TRY(hipMemsetAsync(c->hist.p, 0, P * c->d.nlevels * sizeof(int), c->stream));
    HIP_TRY(hipMemsetAsync(c->tag.p, 0, (size_t)(c->maxBits / 64) * P * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->rows = 0;
    return SIND_OK;
}
int arg_error(const char* who, int code) { sind_set_error("%s: %s", who, covis_check_text[code]); return SIND_E_ARG; }
}  // namespace

extern "C" {

int sind_covis_create(int cap_kf, int cap_feat, int cap_points, int nlevels, int max_queries, int device, sind_covis** out) {
    if (!out || cap_kf < 1 || cap_feat < 1 || cap_points < 1 || nlevels < 1 || max_queries < 1) { sind_set_error("sind_covis_create: bad arguments"); return SIND_E_ARG; }
    if ((long long)cap_kf * cap_feat > (1ll << 28) || cap_points > (1 << 24) || nlevels > 16 || max_queries > 4096) {
        sind_set_error("sind_covis_create: beyond the limits (cap_kf * cap_feat <= 2^28, cap_points <= 2^24, nlevels <= 16, max_queries <= 4096)"); return SIND_E_CAPACITY; }
    HIP_TRY(hipSetDevice(device));
    sind_covis* c = new sind_covis(); c->device = device; c->d = CovisDims{cap_kf, cap_feat, cap_points, nlevels}; c->maxQ = max_queries; c->maxBits = 64 * divup(max_queries, 64);
    const size_t cells = (size_t)cap_kf * cap_feat, P = cap_points, ne = (size_t)max_queries * cap_feat;
    int r = SIND_OK;
    if ((r = c->cellPoint.alloc(cells)) || (r = c->cellMeta.alloc(cells)) || (r = c->nObs.alloc(P)) || (r = c->hist.alloc(P * nlevels)) || (r = c->tag.alloc((size_t)(c->maxBits / 64) * P)) ||
        (r = c->entPoint.alloc(ne)) || (r = c->entBit.alloc(ne)) || (r = c->entOctave.alloc(ne)) || (r = c->entClose.alloc(ne)) || (r = c->redundant.alloc(ne)) ||
        (r = c->itemStart.alloc(max_queries + 1)) || (r = c->itemKf.alloc(max_queries)) || (r = c->counts.alloc(2 * (size_t)max_queries)) || (r = c->perBit.alloc((size_t)c->maxBits * cap_kf))) { delete c; return r; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; sind_set_error("sind_covis_create: stream creation failed"); return SIND_E_HIP; }
    c->stamp.assign(cells, 0u); c->occStamp.assign(P, 0u); c->occ.assign(P, 0);
    if ((r = reset_state(c)) != SIND_OK) { sind_covis_destroy(c); return r; }
    *out = c; return SIND_OK;
}

int sind_covis_destroy(sind_covis* c) {
    if (!c) return SIND_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    hipStream_t s = c->stream; delete c; if (s) (void)hipStreamDestroy(s);
    return SIND_OK;
}

int sind_covis_clear(sind_covis* c) {
    if (!c) { sind_set_error("sind_covis_clear: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    return reset_state(c);
}

int sind_covis_apply(sind_covis* c, const sind_covis_op* ops, int n) {
    if (!c) { sind_set_error("sind_covis_apply: bad arguments"); return SIND_E_ARG; }
    if (const int e = covis_check_ops(ops, n, c->d, c->stamp, c->epoch)) return arg_error("sind_covis_apply", e);
    if (!n) return SIND_OK;
    HIP_TRY(hipSetDevice(c->device));
    SIND_TRY(c->ops.alloc(n));
    std::memcpy(c->ops.h.data(), ops, (size_t)n * sizeof(sind_covis_op));
    SIND_TRY(c->ops.up(n, c->stream));
    SIND_TRY(launch_covis_apply(c->table(), c->ops.d.p, n, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) if (ops[i].point >= 0) c->rows = std::max(c->rows, ops[i].kf + 1);
    return SIND_OK;
}

int sind_covis_read_row(sind_covis* c, int kf, int* point, uint8_t* octave, uint8_t* stereo) {
    if (!c || !point || !octave || !stereo || kf < 0 || kf >= c->d.capKf) { sind_set_error("sind_covis_read_row: bad arguments (key frame %d of %d)", kf, c ? c->d.capKf : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t F = c->d.capFeat, o = (size_t)kf * F;
    c->hRowPoint.resize(F); c->hRowMeta.resize(F);
    HIP_TRY(hipMemcpyAsync(c->hRowPoint.data(), c->cellPoint.p + o, F * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->hRowMeta.data(), c->cellMeta.p + o, F, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < F; i++) { point[i] = c->hRowPoint[i]; octave[i] = (uint8_t)covis_octave(c->hRowMeta[i]); stereo[i] = (uint8_t)covis_stereo(c->hRowMeta[i]); }
    return SIND_OK;
}

int sind_covis_read_points(sind_covis* c, const int* points, int n, int* n_obs, int* hist) {
    if (!c || n < 0 || (n && (!points || !n_obs || !hist))) { sind_set_error("sind_covis_read_points: bad arguments"); return SIND_E_ARG; }
    for (int i = 0; i < n; i++) if (points[i] < 0 || points[i] >= c->d.capPoints) { sind_set_error("sind_covis_read_points: point %d of %d", points[i], c->d.capPoints); return SIND_E_ARG; }
    if (!n) return SIND_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t P = c->d.capPoints, L = c->d.nlevels;
    c->hNObs.resize(P); c->hHist.resize(P * L);
    HIP_TRY(hipMemcpyAsync(c->hNObs.data(), c->nObs.p, P * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->hHist.data(), c->hist.p, P * L * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) { n_obs[i] = c->hNObs[points[i]]; std::memcpy(hist + (size_t)i * L, &c->hHist[(size_t)points[i] * L], L * sizeof(int)); }
    return SIND_OK;
}

int sind_covis_count(sind_covis* c, const sind_covis_query* q, int Q) {
    if (!c) { sind_set_error("sind_covis_count: bad arguments"); return SIND_E_ARG; }
    if (const int e = covis_check_queries(q, Q, c->d)) return arg_error("sind_covis_count", e);
    if (Q > c->maxQ) { sind_set_error("sind_covis_count: Q=%d, max_queries %d", Q, c->maxQ); return SIND_E_CAPACITY; }
    for (int j = 0; j < Q; j++) if (q[j].n > c->d.capFeat) { sind_set_error("sind_covis_count: a list of %d entries, cap_feat %d", q[j].n, c->d.capFeat); return SIND_E_CAPACITY; }
    const int bits = covis_assign_bits(q, Q, c->occ, c->occStamp, c->occEpoch, c->ePoint, c->eBit, c->base, c->mult);
    if (bits > c->maxBits) { sind_set_error("sind_covis_count: %d tag bits, %d reserved", bits, c->maxBits); return SIND_E_CAPACITY; }
    const int n = (int)c->ePoint.size(), rows = c->rows;
    if (n && rows) {
        HIP_TRY(hipSetDevice(c->device));
        std::memcpy(c->entPoint.h.data(), c->ePoint.data(), n * sizeof(int)); std::memcpy(c->entBit.h.data(), c->eBit.data(), n * sizeof(int));
        hipStream_t s = c->stream;
        SIND_TRY(c->entPoint.up(n, s)); SIND_TRY(c->entBit.up(n, s));
        SIND_TRY(launch_covis_tag(c->tag.p, c->entPoint.d.p, c->entBit.d.p, n, c->d.capPoints, true, s));
        SIND_TRY(launch_covis_count(c->table(), c->tag.p, c->perBit.d.p, rows, bits, s));
        SIND_TRY(launch_covis_tag(c->tag.p, c->entPoint.d.p, c->entBit.d.p, n, c->d.capPoints, false, s));
        SIND_TRY(c->perBit.down((size_t)bits * rows, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int j = 0; j < Q; j++) covis_sum_bits(q[j], c->base[j], (n && rows) ? c->mult[j] : 0, c->perBit.h.data(), rows, rows, c->d.capKf);
    return SIND_OK;
}

int sind_covis_cull(sind_covis* c, const sind_covis_cull_item* items, int B, int th_obs) {
    if (!c) { sind_set_error("sind_covis_cull: bad arguments"); return SIND_E_ARG; }
    if (const int e = covis_check_cull(items, B, c->d)) return arg_error("sind_covis_cull", e);
    if (B > c->maxQ) { sind_set_error("sind_covis_cull: B=%d, max_queries %d", B, c->maxQ); return SIND_E_CAPACITY; }
    for (int b = 0; b < B; b++) if (items[b].n > c->d.capFeat) { sind_set_error("sind_covis_cull: an item of %d entries, cap_feat %d", items[b].n, c->d.capFeat); return SIND_E_CAPACITY; }
    int n = 0;
    for (int b = 0; b < B; b++) {
        const sind_covis_cull_item& it = items[b];
        c->itemStart.h[b] = n; c->itemKf.h[b] = it.kf; c->counts.h[2 * b] = c->counts.h[2 * b + 1] = 0;
        if (it.n) { std::memcpy(&c->entPoint.h[n], it.points, it.n * sizeof(int)); std::memcpy(&c->entOctave.h[n], it.octave, it.n); std::memcpy(&c->entClose.h[n], it.close, it.n); }
        n += it.n;
    }
    if (n) {
        c->itemStart.h[B] = n;
        HIP_TRY(hipSetDevice(c->device));
        hipStream_t s = c->stream;
        SIND_TRY(c->itemStart.up(B + 1, s)); SIND_TRY(c->itemKf.up(B, s)); SIND_TRY(c->counts.up(2 * (size_t)B, s));
        SIND_TRY(c->entPoint.up(n, s)); SIND_TRY(c->entOctave.up(n, s)); SIND_TRY(c->entClose.up(n, s));
        SIND_TRY(launch_covis_cull(c->table(), c->itemStart.d.p, c->itemKf.d.p, B, c->entPoint.d.p, c->entOctave.d.p, c->entClose.d.p, n, th_obs, c->counts.d.p, c->redundant.d.p, s));
        SIND_TRY(c->counts.down(2 * (size_t)B, s)); SIND_TRY(c->redundant.down(n, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int b = 0; b < B; b++) {
        const sind_covis_cull_item& it = items[b];
        *it.n_mps = c->counts.h[2 * b]; *it.n_redundant = c->counts.h[2 * b + 1];
        if (it.redundant && it.n) std::memcpy(it.redundant, &c->redundant.h[c->itemStart.h[b]], it.n);
    }
    return SIND_OK;
}

}  // extern "C"
