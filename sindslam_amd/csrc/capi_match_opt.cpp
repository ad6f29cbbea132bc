// C ABI: the optimizers on the matcher handle: PoseOptimization, OptimizeSim3, LocalBundleAdjustment, OptimizeEssentialGraph, BundleAdjustment (include/sind_hip.h, "sind_match_*").
#include "match_handle.hpp"
#include "host/pose_opt.hpp"
#include "host/sim3_opt.hpp"

extern "C" {

int sind_match_pose_optimize(sind_match* m, const sind_poseopt_item* items, int B) {
    const char* who = "sind_match_pose_optimize: item";
    SIND_TRY(solver_prologue("sind_match_pose_optimize", m, items, B));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_poseopt_item& q = items[b];
        if (q.n > cs) { sind_set_error("%s %d has %d correspondences, capacity %d", who, b, q.n, cs); return SIND_E_CAPACITY; }
        static const char* const what[] = {"", "negative count", "null array", "an inv_sigma2 is not a finite non-negative number", "the pose is not finite"};
        if (const int bad = sind::poseopt_check(q)) { sind_set_error("%s %d: %s", who, b, what[bad]); return SIND_E_ARG; }
        maxN = std::max(maxN, q.n);
    }
    if (!B) return SIND_OK;
    static_assert(sizeof(sind::PoseOptResult) == sizeof(sind::PoseOptOut), "PoseOptResult is PoseOptOut");
    if (maxN < 3) {                                                                                     // the reference's `return 0` for every item: nothing to launch
        for (int b = 0; b < B; b++) { *items[b].n_good = 0; *items[b].n_rounds = 0; }
        return SIND_OK;
    }
    HIP_TRY(hipSetDevice(m->device));
    sind_match::PoseSide& w = m->poseopt;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::MatchParams& c = m->prm;
    const sind::PoseOptParams p{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, (double)c.bf, cs};
    for (int b = 0; b < B; b++) {
        const sind_poseopt_item& q = items[b];
        float4* pt = &w.pts.h[(size_t)b * cs]; float4* ob = &w.obs.h[(size_t)b * cs];
        for (int i = 0; i < q.n; i++) { pt[i] = make_float4(q.x3Dw[3 * i], q.x3Dw[3 * i + 1], q.x3Dw[3 * i + 2], q.inv_sigma2[i]); ob[i] = make_float4(q.obs_xy[2 * i], q.obs_xy[2 * i + 1], q.u_right[i], 0.f); }
        w.n.h[b] = q.n; cpy(&w.Tcw.h[(size_t)b * 16], q.Tcw, 16 * sizeof(float));
    }
    hipStream_t s = m->stream; const size_t k = (size_t)B * cs;
    sind::PoseOptArrays a{w.n.d.p, w.Tcw.d.p, w.pts.d.p, w.obs.d.p, w.outlier.d.p, w.res.d.p};
    SIND_TRY(w.n.up(B, s)); SIND_TRY(w.Tcw.up((size_t)B * 16, s)); SIND_TRY(w.pts.up(k, s)); SIND_TRY(w.obs.up(k, s));
    SIND_TRY(sind::launch_pose_optimize(p, a, B, s));
    SIND_TRY(w.outlier.down(k, s)); SIND_TRY(w.res.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        sind::PoseOptOut o; std::memcpy(&o, &w.res.h[b], sizeof(o));
        sind::poseopt_store(items[b], o, &w.outlier.h[(size_t)b * cs]);
    }
    return SIND_OK;
}

int sind_match_sim3_optimize(sind_match* m, const sind_sim3opt_item* items, int B, float th2, int fix_scale) {
    const char* who = "sind_match_sim3_optimize: item";
    SIND_TRY(solver_prologue("sind_match_sim3_optimize", m, items, B, std::isfinite(th2) && th2 >= 0));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_sim3opt_item& q = items[b];
        if (q.n > cs) { sind_set_error("%s %d has %d pairs, capacity %d", who, b, q.n, cs); return SIND_E_CAPACITY; }
        static const char* const what[] = {"", "negative count", "null array", "an inv_sigma2 is not a finite non-negative number", "the input Sim3 or an intrinsic is not finite"};
        if (const int bad = sind::sim3opt_check(q)) { sind_set_error("%s %d: %s", who, b, what[bad]); return SIND_E_ARG; }
        maxN = std::max(maxN, q.n);
    }
    if (!B) return SIND_OK;
    static_assert(sizeof(sind::Sim3OptResult) == sizeof(sind::Sim3OptOut), "Sim3OptResult is Sim3OptOut");
    if (maxN < 1) {                                                                                     // every graph is empty: the reference's `return 0`, nothing to launch
        for (int b = 0; b < B; b++) {
            sind::Sim3Q S0; sind::s3_from_input(items[b].s12, items[b].R12, items[b].t12, S0);
            sind::Sim3OptOut o{}; std::memcpy(o.q, S0.q, sizeof(o.q)); std::memcpy(o.t, S0.t, sizeof(o.t)); o.s = S0.s;
            sind::sim3opt_store(items[b], o, nullptr);
        }
        return SIND_OK;
    }
    HIP_TRY(hipSetDevice(m->device));
    sind_match::Sim3OptSide& w = m->sim3opt;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::Sim3OptParams p{th2, fix_scale != 0, cs};
    for (int b = 0; b < B; b++) {
        const sind_sim3opt_item& q = items[b];
        float4* p1 = &w.p1.h[(size_t)b * cs]; float4* p2 = &w.p2.h[(size_t)b * cs]; float4* ob = &w.ob.h[(size_t)b * cs];
        for (int i = 0; i < q.n; i++) {
            p1[i] = make_float4(q.x3Dc1[3 * i], q.x3Dc1[3 * i + 1], q.x3Dc1[3 * i + 2], q.inv_sigma2_1[i]);
            p2[i] = make_float4(q.x3Dc2[3 * i], q.x3Dc2[3 * i + 1], q.x3Dc2[3 * i + 2], q.inv_sigma2_2[i]);
            ob[i] = make_float4(q.obs1_xy[2 * i], q.obs1_xy[2 * i + 1], q.obs2_xy[2 * i], q.obs2_xy[2 * i + 1]);
        }
        sind::Sim3OptHead& h = w.head.h[b];
        cpy(h.K1, q.K1, 4 * sizeof(float)); cpy(h.K2, q.K2, 4 * sizeof(float)); h.s12 = q.s12; cpy(h.R12, q.R12, 9 * sizeof(float)); cpy(h.t12, q.t12, 3 * sizeof(float)); h.n = q.n;
    }
    hipStream_t s = m->stream; const size_t k = (size_t)B * cs;
    sind::Sim3OptArrays a{w.head.d.p, w.p1.d.p, w.p2.d.p, w.ob.d.p, w.removed.d.p, w.res.d.p};
    SIND_TRY(w.head.up(B, s)); SIND_TRY(w.p1.up(k, s)); SIND_TRY(w.p2.up(k, s)); SIND_TRY(w.ob.up(k, s));
    SIND_TRY(sind::launch_sim3_optimize(p, a, B, s));
    SIND_TRY(w.removed.down(k, s)); SIND_TRY(w.res.down(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        sind::Sim3OptOut o; std::memcpy(&o, &w.res.h[b], sizeof(o));
        sind::sim3opt_store(items[b], o, &w.removed.h[(size_t)b * cs]);
    }
    return SIND_OK;
}

// local BA and the essential graph: check, plan, pack (match_handle.hpp: PackedItems), launch, unpack
int sind_match_local_ba(sind_match* m, const sind_localba_item* items, int B) {
    const char* who = "sind_match_local_ba: item";
    SIND_TRY(solver_prologue("sind_match_local_ba", m, items, B));
    for (int b = 0; b < B; b++) if (const int bad = sind::lba_check(items[b])) { sind_set_error("%s %d: %s", who, b, sind::lba_check_text[bad]); return SIND_E_ARG; }
    if (!B) return SIND_OK;
    auto& w = m->localba;
    w.plan.resize((size_t)m->maxB);
    for (int b = 0; b < B; b++) if (sind::lba_plan(items[b], w.plan[b])) {
        sind_set_error("%s %d is beyond a limit: %d key frames of kind 0, %d key frames, %d points, %d observations, %d co-observation entries", who, b, LBA_MAX_POSES, LBA_MAX_KF, LBA_MAX_MP, LBA_MAX_OBS, LBA_MAX_PAIRS);
        return SIND_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(m->device));
    SIND_TRY(w.reserve(B, (size_t)m->maxB));
    const sind::MatchParams& c = m->prm;
    const sind::PoseOptCam K{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, (double)c.bf};
    for (int b = 0; b < B; b++) { sind::ba_fill(sind::ba_item(items[b]), w.host(b)); sind::lba_bind(w.plan[b], items[b].do_more, K, w.dev(b), w.views.h[b]); }
    hipStream_t s = m->stream;
    SIND_TRY(w.upload(B, s));
    SIND_TRY(sind::launch_local_ba(w.views.d.p, B, s));
    SIND_TRY(w.download(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) sind::lba_store(items[b], w.plan[b], w.host(b));
    return SIND_OK;
}

int sind_match_essential_graph(sind_match* m, const sind_essgraph_item* items, int B, int fix_scale) {
    const char* who = "sind_match_essential_graph: item";
    SIND_TRY(solver_prologue("sind_match_essential_graph", m, items, B));
    for (int b = 0; b < B; b++) if (const int bad = sind::ess_check(items[b])) { sind_set_error("%s %d: %s", who, b, sind::ess_check_text[bad]); return SIND_E_ARG; }
    if (!B) return SIND_OK;
    auto& w = m->ess;
    w.plan.resize((size_t)m->maxB);
    int maxMp = 0;
    for (int b = 0; b < B; b++) {
        if (sind::ess_plan(items[b], w.plan[b])) {
            sind_set_error("%s %d is beyond a limit: %d key frames, %d edges, %d points, %d entries of the factor's envelope", who, b, ESS_MAX_KF, ESS_MAX_EDGES, ESS_MAX_MP, ESS_MAX_ENV);
            return SIND_E_CAPACITY;
        }
        maxMp = std::max(maxMp, w.plan[b].nMp);
    }
    HIP_TRY(hipSetDevice(m->device));
    SIND_TRY(w.reserve(B, (size_t)m->maxB));
    for (int b = 0; b < B; b++) { sind::ess_fill(items[b], w.host(b)); sind::ess_bind(w.plan[b], fix_scale, w.dev(b), w.views.h[b]); }
    hipStream_t s = m->stream;
    SIND_TRY(w.upload(B, s));
    SIND_TRY(sind::launch_essential_graph(w.views.d.p, B, maxMp, s));
    SIND_TRY(w.download(B, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) sind::ess_store(items[b], w.plan[b], w.host(b));
    return SIND_OK;
}

// global BA: check, plan, pack, then item after item: the phases of host/global_ba.hpp as launches over the whole grid, the Levenberg-Marquardt driver here on the host
int sind_match_global_ba(sind_match* m, const sind_globalba_item* items, int B, int iterations, int robust) {
    const char* who = "sind_match_global_ba: item";
    SIND_TRY(solver_prologue("sind_match_global_ba", m, items, B, iterations >= 0));
    for (int b = 0; b < B; b++) if (const int bad = sind::gba_check(items[b])) { sind_set_error("%s %d: %s", who, b, sind::gba_check_text[bad]); return SIND_E_ARG; }
    if (!B) return SIND_OK;
    auto& w = m->globalba;
    w.plan.resize((size_t)m->maxB);
    for (int b = 0; b < B; b++) if (sind::gba_plan(items[b], w.plan[b])) {
        sind_set_error("%s %d is beyond a limit: %d key frames, %d points, %d observations, %d co-observation entries, %d entries of the factor's envelope", who, b, GBA_MAX_KF, GBA_MAX_MP, GBA_MAX_OBS, GBA_MAX_PAIRS, GBA_MAX_ENV);
        return SIND_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(m->device));
    SIND_TRY(w.reserve(B, (size_t)m->maxB)); SIND_TRY(m->gbaSc.alloc(sind::BA_SC_N));
    const sind::MatchParams& c = m->prm;
    const sind::PoseOptCam K{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, (double)c.bf};
    for (int b = 0; b < B; b++) { sind::ba_fill(sind::ba_item(items[b]), w.host(b)); sind::gba_bind(w.plan[b], K, w.dev(b), w.views.h[b]); }
    hipStream_t s = m->stream;
    SIND_TRY(w.I.up(w.at[B].ints, s)); SIND_TRY(w.Fin.up(w.at[B].floatsIn, s));
    std::vector<sind::GbaDiag> dg((size_t)B);
    m->gbaCount = sind::GbaCounters{};
    for (int b = 0; b < B; b++) SIND_TRY(sind::launch_global_ba(w.views.h[b], w.plan[b].cs.data(), iterations, robust != 0, m->gbaSc.p, s, dg[b], m->gbaCount));
    SIND_TRY(w.Fout.down(w.at[B].floatsOut, s));
    HIP_TRY(hipStreamSynchronize(s)); m->gbaCount.waits++;
    for (int b = 0; b < B; b++) sind::gba_store(items[b], w.plan[b], w.host(b), dg[b]);
    return SIND_OK;
}

// the launches and host waits of the last sind_match_global_ba on the handle (profiles/match_global_ba_timing.py)
int sind_match_global_ba_counts(sind_match* m, long long* launches, long long* waits) {
    if (!m || !launches || !waits) return SIND_E_ARG;
    *launches = m->gbaCount.launches; *waits = m->gbaCount.waits;
    return SIND_OK;
}

}  // extern "C"
