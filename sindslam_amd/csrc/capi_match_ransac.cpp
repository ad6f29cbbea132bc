// C ABI: Sim3Solver and PnPsolver on the matcher handle (include/sind_hip.h, "sind_match_sim3_ransac", "sind_match_pnp_ransac"; match_sim3.hip, match_pnp.hip).
#include "match_handle.hpp"
#include "host/pnp.hpp"

extern "C" {

int sind_match_sim3_ransac(sind_match* m, const sind_sim3_item* items, int B, int fix_scale) {
    const char* who = "sind_match_sim3_ransac: item";
    SIND_TRY(solver_prologue("sind_match_sim3_ransac", m, items, B));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int its = 0, maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_sim3_item& q = items[b];
        if (q.n < 0 || q.n_its < 0) { sind_set_error("%s %d: negative count", who, b); return SIND_E_ARG; }
        if (q.n > cs || q.n_its > SIM3_MAX_ITS) { sind_set_error("%s %d has %d correspondences / %d iterations, capacity %d / %d", who, b, q.n, q.n_its, cs, SIM3_MAX_ITS); return SIND_E_CAPACITY; }
        if ((q.n && (!q.T1w || !q.T2w || !q.x3Dw1 || !q.x3Dw2 || !q.sigma2_1 || !q.sigma2_2)) || (q.n_its && (!q.triple || !q.count || !q.s12 || !q.R12 || !q.t12 || (q.n && !q.inlier_bits)))) {
            sind_set_error("%s %d: null array", who, b); return SIND_E_ARG;
        }
        for (int i = 0; i < q.n; i++) if (!(q.sigma2_1[i] >= 0 && q.sigma2_2[i] >= 0 && std::isfinite(q.sigma2_1[i]) && std::isfinite(q.sigma2_2[i]))) { sind_set_error("%s %d: sigma2 %d is not a finite non-negative number", who, b, i); return SIND_E_ARG; }
        for (int k = 0; k < 3 * q.n_its; k++) if (q.triple[k] < 0 || q.triple[k] >= q.n) { sind_set_error("%s %d: triple index %d outside [0,%d)", who, b, q.triple[k], q.n); return SIND_E_ARG; }
        its = std::max(its, q.n_its); maxN = std::max(maxN, q.n);
    }
    if (!its) return SIND_OK;                                                                          // nothing to evaluate, nothing to write
    HIP_TRY(hipSetDevice(m->device));
    sind_match::RansacSide& w = m->ransac;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::MatchParams& c = m->prm;
    const sind::Sim3Params p{c.fx, c.fy, c.cx, c.cy, cs, its, std::max(1, divup(maxN, 64))};
    for (int b = 0; b < B; b++) {
        const sind_sim3_item& q = items[b];
        float4* c1 = &w.corr.h[(size_t)b * 3 * cs]; float4* c2 = c1 + cs; float4* im = c2 + cs;
        for (int i = 0; i < q.n; i++) {                                                                // the constructor (:84-109)
            float x1[3], x2[3], p1[2], p2[2];
            sind::sim3_to_camera(q.T1w, q.x3Dw1 + 3 * i, x1); sind::sim3_to_camera(q.T2w, q.x3Dw2 + 3 * i, x2);
            sind::sim3_to_image(c.fx, c.fy, c.cx, c.cy, x1, p1); sind::sim3_to_image(c.fx, c.fy, c.cx, c.cy, x2, p2);
            c1[i] = make_float4(x1[0], x1[1], x1[2], sind::sim3_max_error(q.sigma2_1[i])); c2[i] = make_float4(x2[0], x2[1], x2[2], sind::sim3_max_error(q.sigma2_2[i]));
            im[i] = make_float4(p1[0], p1[1], p2[0], p2[1]);
        }
        w.n.h[b] = q.n; w.nIts.h[b] = q.n_its;
        for (int h = 0; h < q.n_its; h++) {                                                            // the sample (:166-177) and ComputeSim3
            float P1[9], P2[9];
            for (int k = 0; k < 3; k++) { const float4 a1 = c1[q.triple[3 * h + k]], a2 = c2[q.triple[3 * h + k]]; P1[k] = a1.x; P1[3 + k] = a1.y; P1[6 + k] = a1.z; P2[k] = a2.x; P2[3 + k] = a2.y; P2[6 + k] = a2.z; }
            sind::Sim3Hyp& s = w.solved[(size_t)b * its + h];
            sind::sim3_horn(P1, P2, fix_scale != 0, s);
            sind::Sim3Pose& d = w.hyp.h[(size_t)b * its + h]; cpy(d.T12, s.T12, sizeof(d.T12)); cpy(d.T21, s.T21, sizeof(d.T21));
        }
    }
    hipStream_t s = m->stream; const size_t nh = (size_t)B * its;
    SIND_TRY(w.n.up(B, s)); SIND_TRY(w.nIts.up(B, s)); SIND_TRY(w.corr.up((size_t)B * 3 * cs, s)); SIND_TRY(w.hyp.up(nh, s));
    SIND_TRY(sind::launch_sim3_check(p, sind::Sim3Arrays{w.n.d.p, w.nIts.d.p, w.corr.d.p, w.hyp.d.p, w.count.d.p, w.bits.d.p}, B, s));
    SIND_TRY(w.count.down(nh, s)); SIND_TRY(w.bits.down(nh * p.words, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        const sind_sim3_item& q = items[b]; const int nw = divup(q.n, 64);
        for (int h = 0; h < q.n_its; h++) {
            const size_t o = (size_t)b * its + h; const sind::Sim3Hyp& r = w.solved[o];
            q.count[h] = w.count.h[o]; cpy(q.inlier_bits + (size_t)h * nw, &w.bits.h[o * p.words], (size_t)nw * sizeof(uint64_t));
            q.s12[h] = r.s12; cpy(q.R12 + 9 * h, r.R12, sizeof(r.R12)); cpy(q.t12 + 3 * h, r.t12, sizeof(r.t12));
        }
    }
    return SIND_OK;
}

int sind_match_pnp_ransac(sind_match* m, const sind_pnp_item* items, int B) {
    const char* who = "sind_match_pnp_ransac: item";
    SIND_TRY(solver_prologue("sind_match_pnp_ransac", m, items, B));
    const int cs = std::min(m->last.cap, m->cur.cap);
    int its = 0, maxN = 0;
    for (int b = 0; b < B; b++) {
        const sind_pnp_item& q = items[b];
        if (q.n < 0 || q.n_its < 0 || q.best_count < 0) { sind_set_error("%s %d: negative count", who, b); return SIND_E_ARG; }
        if (q.n > cs || q.n_its > PNP_MAX_ITS) { sind_set_error("%s %d has %d correspondences / %d iterations, capacity %d / %d", who, b, q.n, q.n_its, cs, PNP_MAX_ITS); return SIND_E_CAPACITY; }
        if ((q.n && (!q.x3Dw || !q.p2d || !q.sigma2)) || (q.best_count && !q.best_bits) ||
            (q.n_its && (!q.samples || !q.count || !q.R || !q.t || !q.refine || !q.n_refines || !q.refine_hyp || !q.refine_count || !q.refine_R || !q.refine_t || (q.n && (!q.inlier_bits || !q.refine_bits))))) {
            sind_set_error("%s %d: null array", who, b); return SIND_E_ARG;
        }
        if (q.min_inliers < 1) { sind_set_error("%s %d: min_inliers %d below 1", who, b, q.min_inliers); return SIND_E_ARG; }
        for (int i = 0; i < q.n; i++) if (!(q.sigma2[i] >= 0 && std::isfinite(q.sigma2[i]))) { sind_set_error("%s %d: sigma2 %d is not a finite non-negative number", who, b, i); return SIND_E_ARG; }
        for (int h = 0; h < q.n_its; h++) {
            const int* sm = q.samples + 4 * h;
            for (int k = 0; k < 4; k++) {
                if (sm[k] < 0 || sm[k] >= q.n) { sind_set_error("%s %d: sample index %d outside [0,%d)", who, b, sm[k], q.n); return SIND_E_ARG; }
                for (int j = 0; j < k; j++) if (sm[j] == sm[k]) { sind_set_error("%s %d: sample %d repeats index %d", who, b, h, sm[k]); return SIND_E_ARG; }
            }
        }
        if (q.best_bits) {
            int pc = 0;
            for (int i = 0; i < q.n; i++) pc += (int)((q.best_bits[i >> 6] >> (i & 63)) & 1);
            if (pc != q.best_count) { sind_set_error("%s %d: best_count %d, but best_bits has %d bits set", who, b, q.best_count, pc); return SIND_E_ARG; }
        }
        its = std::max(its, q.n_its); maxN = std::max(maxN, q.n);
    }
    if (!its) return SIND_OK;                                                                          // nothing to evaluate, nothing to write
    HIP_TRY(hipSetDevice(m->device));
    sind_match::PnpSide& w = m->pnp;
    if (!w.cap) SIND_TRY(w.reserve((size_t)m->maxB, cs));
    const sind::MatchParams& c = m->prm;
    const sind::PnpParams p{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, cs, its, std::max(1, divup(maxN, 64))};
    for (int b = 0; b < B; b++) {
        const sind_pnp_item& q = items[b];
        float4* pt = &w.pts.h[(size_t)b * cs]; float2* uv = &w.uv.h[(size_t)b * cs];
        for (int i = 0; i < q.n; i++) { pt[i] = make_float4(q.x3Dw[3 * i], q.x3Dw[3 * i + 1], q.x3Dw[3 * i + 2], q.sigma2[i] * q.th2); uv[i] = make_float2(q.p2d[2 * i], q.p2d[2 * i + 1]); }
        w.n.h[b] = q.n; w.nIts.h[b] = q.n_its;
        for (int h = 0; h < q.n_its; h++) w.samples.h[(size_t)b * its + h] = make_int4(q.samples[4 * h], q.samples[4 * h + 1], q.samples[4 * h + 2], q.samples[4 * h + 3]);
        unsigned long long* bb = &w.bestBits.h[(size_t)b * p.words];
        for (int k = 0; k < p.words; k++) bb[k] = (q.best_bits && k < divup(q.n, 64)) ? q.best_bits[k] : 0ull;
    }
    hipStream_t s = m->stream; const size_t nh = (size_t)B * its;
    sind::PnpArrays a{w.n.d.p, w.nIts.d.p, w.pts.d.p, w.uv.d.p, w.samples.d.p, w.bestBits.d.p, w.pose.d.p, w.count.d.p, w.bits.d.p, w.refine.d.p, w.work.p, w.refPose.d.p, w.refCount.d.p, w.refBits.d.p};
    SIND_TRY(w.n.up(B, s)); SIND_TRY(w.nIts.up(B, s)); SIND_TRY(w.pts.up((size_t)B * cs, s)); SIND_TRY(w.uv.up((size_t)B * cs, s)); SIND_TRY(w.samples.up(nh, s)); SIND_TRY(w.bestBits.up((size_t)B * p.words, s));
    SIND_TRY(sind::launch_pnp_samples(p, a, B, s));                                                     // 1. pose(4) + check for all hypotheses
    SIND_TRY(w.count.down(nh, s)); SIND_TRY(w.bits.down(nh * p.words, s)); SIND_TRY(w.pose.down(nh, s));
    HIP_TRY(hipStreamSynchronize(s));                                                                   // 2. counts to the host
    struct Slot { int b, r; };
    std::vector<Slot> todo; std::vector<sind::PnpRefine> probs;
    for (int b = 0; b < B; b++) {
        const sind_pnp_item& q = items[b]; const int nw = divup(q.n, 64);
        if (!q.n_its) { if (q.n_refines) *q.n_refines = 0; continue; }                                 // an item without iterations in a call that has some: no refines
        for (int h = 0; h < q.n_its; h++) {
            const size_t o = (size_t)b * its + h; const sind::PnpPose& r = w.pose.h[o];
            q.count[h] = w.count.h[o]; cpy(q.inlier_bits + (size_t)h * nw, &w.bits.h[o * p.words], (size_t)nw * sizeof(uint64_t));
            cpy(q.R + 9 * h, r.R, sizeof(r.R)); cpy(q.t + 3 * h, r.t, sizeof(r.t));
        }
        const int nr = sind::pnp_refine_plan(q.count, q.n_its, q.min_inliers, q.best_count, q.best_bits != nullptr, w.refineOfHyp.data(), w.hypOfRefine.data());      // 3. the Refine list
        for (int h = 0; h < q.n_its; h++) q.refine[h] = std::max(-1, w.refineOfHyp[h]);              // -2 cannot occur: best_count > 0 comes with best_bits
        *q.n_refines = nr;
        for (int r = 0; r < nr; r++) { q.refine_hyp[r] = w.hypOfRefine[r]; todo.push_back({b, r}); probs.push_back({b, w.hypOfRefine[r]}); }
    }
    for (size_t at = 0; at < todo.size(); at += PNP_REFINE_SLOTS) {                                     // 4. pose(n) + check for the refines, a round of slots at a time
        const int k = (int)std::min<size_t>(PNP_REFINE_SLOTS, todo.size() - at);
        for (int j = 0; j < k; j++) w.refine.h[j] = probs[at + j];
        SIND_TRY(w.refine.up(k, s));
        SIND_TRY(sind::launch_pnp_refines(p, a, k, s));
        SIND_TRY(w.refCount.down(k, s)); SIND_TRY(w.refBits.down((size_t)k * p.words, s)); SIND_TRY(w.refPose.down(k, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int j = 0; j < k; j++) {                                                                  // 5. results back
            const sind_pnp_item& q = items[todo[at + j].b]; const int r = todo[at + j].r, nw = divup(q.n, 64); const sind::PnpPose& o = w.refPose.h[j];
            q.refine_count[r] = w.refCount.h[j]; cpy(q.refine_bits + (size_t)r * nw, &w.refBits.h[(size_t)j * p.words], (size_t)nw * sizeof(uint64_t));
            cpy(q.refine_R + 9 * r, o.R, sizeof(o.R)); cpy(q.refine_t + 3 * r, o.t, sizeof(o.t));
        }
    }
    return SIND_OK;
}

}  // extern "C"
