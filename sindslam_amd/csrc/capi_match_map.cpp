// C ABI: map-point upkeep on the matcher handle: the triangulation loop of LocalMapping::CreateNewMapPoints, MapPoint::ComputeDistinctiveDescriptors and
// MapPoint::UpdateNormalAndDepth (include/sind_hip.h, "sind_match_triangulate", "sind_match_update_points").
#include "match_handle.hpp"

namespace {

// the workspaces grow in powers of two, so that a run of slightly larger calls does not reallocate every time
size_t grown(size_t n) { size_t c = 1024; while (c < n) c *= 2; return c; }

}  // namespace

extern "C" {

// check, list the matches of all pairs with their stereo cosines (host/map_points.cpp), one launch, scatter
int sind_match_triangulate(sind_match* m, const sind_tri_pair* pairs, int B) {
    const char* who = "sind_match_triangulate: pair";
    SIND_TRY(solver_prologue("sind_match_triangulate", m, pairs, B));
    const sind::MatchParams& c = m->prm;
    for (int b = 0; b < B; b++) {
        const sind_tri_pair& q = pairs[b];
        if (q.kf1.n > c.capLast || q.kf2.n > c.capCur) { sind_set_error("%s %d has %d / %d keypoints, capacity %d / %d", who, b, q.kf1.n, q.kf2.n, c.capLast, c.capCur); return SIND_E_CAPACITY; }
        if (const int bad = sind::tri_check(q, c.nlevels)) { sind_set_error("%s %d: %s", who, b, sind::tri_check_text[bad]); return SIND_E_ARG; }
    }
    if (!B) return SIND_OK;
    sind_match::TriSide& w = m->tri;
    w.list.clear();
    for (int b = 0; b < B; b++) sind::tri_collect(pairs[b], b, m->mb, w.list);
    const size_t n = w.list.size();
    if (n) {
        HIP_TRY(hipSetDevice(m->device));
        SIND_TRY(w.pair.alloc((size_t)m->maxB)); SIND_TRY(w.match.alloc(grown(n))); SIND_TRY(w.out.alloc(grown(n)));
        for (int b = 0; b < B; b++) sind::tri_pair(pairs[b], w.pair.h[b]);
        cpy(w.match.h.data(), w.list.data(), n * sizeof(sind::TriMatch));
        const float K5[5] = {c.fx, c.fy, c.cx, c.cy, c.bf};
        sind::TriCam cam; sind::tri_cam(K5, c.scale, c.nlevels, cam);
        hipStream_t s = m->stream;
        SIND_TRY(w.pair.up(B, s)); SIND_TRY(w.match.up(n, s));
        SIND_TRY(sind::launch_tri_points(cam, w.pair.d.p, w.match.d.p, w.out.d.p, (int)n, s));
        SIND_TRY(w.out.down(n, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (int b = 0; b < B; b++) sind::tri_store(pairs[b], b, w.list.data(), w.out.h.data(), n);
    return SIND_OK;
}

// check, flatten the items one after the other (host/map_points.cpp), two launches on the handle's stream, one wait, store
int sind_match_update_points(sind_match* m, const sind_mappoints_item* items, int B) {
    const char* who = "sind_match_update_points: item";
    SIND_TRY(solver_prologue("sind_match_update_points", m, items, B));
    const sind::MatchParams& c = m->prm;
    bool desc = false, normal = false;
    for (int b = 0; b < B; b++) {
        const sind_mappoints_item& q = items[b];
        int bad = sind::mpu_check(q, c.nlevels, false);                 // counts, NULL arrays, obs_start: what the limits read
        if (bad) { sind_set_error("%s %d: %s", who, b, sind::mpu_check_text[bad]); return SIND_E_ARG; }
        if (sind::mpu_over_limit(q)) { sind_set_error("%s %d is beyond a limit: %d key frames, %d points, %d observations", who, b, MPU_MAX_KF, MPU_MAX_MP, MPU_MAX_OBS); return SIND_E_CAPACITY; }
        if ((bad = sind::mpu_check(q, c.nlevels, true))) { sind_set_error("%s %d: %s", who, b, sind::mpu_check_text[bad]); return SIND_E_ARG; }
        desc = desc || (q.do_descriptor && q.n_mp); normal = normal || (q.do_normal && q.n_mp);
    }
    size_t nKf, nPts, nObs; sind::mpu_totals(items, B, nKf, nPts, nObs);
    if (nObs > (size_t)1 << 28 || nKf > (size_t)1 << 28) { sind_set_error("sind_match_update_points: %zu observations in one call", nObs); return SIND_E_CAPACITY; }
    if (!nPts || (!desc && !normal)) return SIND_OK;
    HIP_TRY(hipSetDevice(m->device));
    sind_match::MapSide& w = m->mapPts;
    SIND_TRY(w.reserve(grown(nKf), grown(nPts), grown(nObs)));
    sind::mpu_fill(items, B, sind::MpFill{w.obsFirst.h.data(), w.obsCount.h.data(), w.todo.h.data(), w.x3Dw.h.data(), w.refObs.h.data(), w.obsKf.h.data(), w.obsBad.h.data(), w.obsOctave.h.data(),
                                          w.obsDesc.h.data(), w.Ow.h.data()});
    hipStream_t s = m->stream;
    SIND_TRY(w.obsFirst.up(nPts, s)); SIND_TRY(w.obsCount.up(nPts, s)); SIND_TRY(w.todo.up(nPts, s)); SIND_TRY(w.x3Dw.up(3 * nPts, s)); SIND_TRY(w.refObs.up(nPts, s));
    if (nObs) { SIND_TRY(w.obsKf.up(nObs, s)); SIND_TRY(w.obsBad.up(nObs, s)); SIND_TRY(w.obsOctave.up(nObs, s)); SIND_TRY(w.obsDesc.up(DESC_WORDS * nObs, s)); }
    if (nKf) SIND_TRY(w.Ow.up(3 * nKf, s));
    const sind::MpArrays d{w.obsFirst.d.p, w.obsCount.d.p, w.todo.d.p, w.x3Dw.d.p, w.refObs.d.p, w.obsKf.d.p, w.obsBad.d.p, w.obsOctave.d.p, w.obsDesc.d.p, w.Ow.d.p,
                           w.descOut.d.p, w.bestObs.d.p, w.normal.d.p, w.maxDist.d.p, w.minDist.d.p, w.updated.d.p};
    sind::MpCam cam{}; for (int l = 0; l < 16; l++) cam.scale[l] = c.scale[l]; cam.nlevels = c.nlevels;
    if (desc) { SIND_TRY(sind::launch_mp_descriptor(d, (int)nPts, s)); SIND_TRY(w.descOut.down(DESC_WORDS * nPts, s)); SIND_TRY(w.bestObs.down(nPts, s)); }
    if (normal) { SIND_TRY(sind::launch_mp_normal(cam, d, (int)nPts, s)); SIND_TRY(w.normal.down(3 * nPts, s)); SIND_TRY(w.maxDist.down(nPts, s)); SIND_TRY(w.minDist.down(nPts, s)); SIND_TRY(w.updated.down(nPts, s)); }
    HIP_TRY(hipStreamSynchronize(s));
    const sind::MpArrays h{w.obsFirst.h.data(), w.obsCount.h.data(), w.todo.h.data(), w.x3Dw.h.data(), w.refObs.h.data(), w.obsKf.h.data(), w.obsBad.h.data(), w.obsOctave.h.data(), w.obsDesc.h.data(),
                           w.Ow.h.data(), w.descOut.h.data(), w.bestObs.h.data(), w.normal.h.data(), w.maxDist.h.data(), w.minDist.h.data(), w.updated.h.data()};
    sind::mpu_store(items, B, h);
    return SIND_OK;
}

}  // extern "C"
