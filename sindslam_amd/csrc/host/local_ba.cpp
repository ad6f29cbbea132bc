// Host twin of sind_match_local_ba (reference src/Optimizer.cc:506-778): local_ba.hpp with the plain sequential executor, and what the two entry points share: the
// argument check, the digest of an item into the lists the phases walk (LbaPlan) and the copy of one item's results.  Compiled into libsind_hip.so (capi_match_opt.cpp
// calls the shared part) and into libsind_host.so.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>
#include "local_ba.hpp"
#include "sind_hip.h"

namespace sind {

const char* const lba_check_text[] = {"", "negative count", "null array", "ids repeat", "an obs_kf is out of range", "a key frame twice in one point's observations",
                                      "obs_start does not start at 0 or decreases", "an inv_sigma2 is not a finite non-negative number", "a pose or point is not finite",
                                      "no key frame of kind 0", "a kf_kind outside 0..2"};

static bool ids_repeat(const int64_t* id, int n) {
    std::vector<int64_t> v(id, id + n); std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) != v.end();
}

int lba_check(const ::sind_localba_item& q) {
    if (q.n_kf < 0 || q.n_mp < 0) return 1;
    if (q.n_kf && (!q.kf_id || !q.kf_kind || !q.Tcw || !q.Tcw_out)) return 2;
    if (q.n_mp && (!q.mp_id || !q.x3Dw || !q.obs_start || !q.x3Dw_out)) return 2;
    if (q.n_mp) { if (q.obs_start[0] != 0) return 6; for (int j = 0; j < q.n_mp; j++) if (q.obs_start[j + 1] < q.obs_start[j]) return 6; }
    const int nObs = q.n_mp ? q.obs_start[q.n_mp] : 0;
    if (nObs && (!q.obs_kf || !q.obs_xy || !q.u_right || !q.inv_sigma2 || !q.erase)) return 2;
    if (ids_repeat(q.kf_id, q.n_kf) || ids_repeat(q.mp_id, q.n_mp)) return 3;
    bool local = false;
    for (int k = 0; k < q.n_kf; k++) { if (q.kf_kind[k] > 2) return 10; local = local || q.kf_kind[k] == 0; }
    std::vector<int> seen((size_t)q.n_kf, -1);
    for (int j = 0; j < q.n_mp; j++) for (int e = q.obs_start[j]; e < q.obs_start[j + 1]; e++) {
        const int k = q.obs_kf[e];
        if (k < 0 || k >= q.n_kf) return 4;
        if (seen[k] == j) return 5;
        seen[k] = j;
    }
    for (int e = 0; e < nObs; e++) if (!(q.inv_sigma2[e] >= 0 && std::isfinite(q.inv_sigma2[e]))) return 7;
    for (size_t k = 0; k < (size_t)16 * q.n_kf; k++) if (!std::isfinite(q.Tcw[k])) return 8;
    for (size_t k = 0; k < (size_t)3 * q.n_mp; k++) if (!std::isfinite(q.x3Dw[k])) return 8;
    if (!local) return 9;
    return 0;
}

int lba_plan(const ::sind_localba_item& q, LbaPlan& pl) {
    const int nKf = q.n_kf, nMp = q.n_mp, nObs = nMp ? q.obs_start[nMp] : 0;
    std::vector<int> free_;                                          // the key frames of kind 0 in ascending kf_id: buildIndexMapping's pose order
    for (int k = 0; k < nKf; k++) if (q.kf_kind[k] == 0) free_.push_back(k);
    std::sort(free_.begin(), free_.end(), [&](int a, int b) { return q.kf_id[a] < q.kf_id[b]; });
    const int P = (int)free_.size();
    if (P > LBA_MAX_POSES || nKf > LBA_MAX_KF || nMp > LBA_MAX_MP || nObs > LBA_MAX_OBS) return SIND_E_CAPACITY;
    std::vector<int> kfPose((size_t)nKf, -1);
    for (int s = 0; s < P; s++) kfPose[free_[s]] = s;
    std::vector<int> ptOrder((size_t)nMp); std::iota(ptOrder.begin(), ptOrder.end(), 0);
    std::sort(ptOrder.begin(), ptOrder.end(), [&](int a, int b) { return q.mp_id[a] < q.mp_id[b]; });
    std::vector<int> ePt((size_t)nObs), ptNF((size_t)nMp, 0), ptSorted((size_t)nObs, 0), poseEdgeStart((size_t)P + 1, 0);
    for (int j = 0; j < nMp; j++) {
        int* srt = ptSorted.data() + q.obs_start[j]; int c = 0;
        for (int e = q.obs_start[j]; e < q.obs_start[j + 1]; e++) { ePt[e] = j; const int s = kfPose[q.obs_kf[e]]; if (s >= 0) { srt[c++] = e; poseEdgeStart[s + 1]++; } }
        std::sort(srt, srt + c, [&](int a, int b) { return kfPose[q.obs_kf[a]] < kfPose[q.obs_kf[b]]; });
        ptNF[j] = c;
    }
    for (int s = 0; s < P; s++) poseEdgeStart[s + 1] += poseEdgeStart[s];
    std::vector<int> poseEdge((size_t)poseEdgeStart[P]), fill(poseEdgeStart.begin(), poseEdgeStart.end() - 1);
    for (int e = 0; e < nObs; e++) { const int s = kfPose[q.obs_kf[e]]; if (s >= 0) poseEdge[fill[s]++] = e; }
    // the co-observation lists: per pair of free poses s1 <= s2, the points both see in ascending mp_id
    std::vector<size_t> cnt((size_t)LBA_MAX_POSES * LBA_MAX_POSES, 0);
    size_t total = 0;
    for (int j = 0; j < nMp; j++) { const size_t k = (size_t)ptNF[j]; total += k * (k + 1) / 2; }
    if (total > (size_t)LBA_MAX_PAIRS) return SIND_E_CAPACITY;
    auto rankOf = [&](int e) { return kfPose[q.obs_kf[e]]; };
    for (int j = 0; j < nMp; j++) { const int* srt = ptSorted.data() + q.obs_start[j]; for (int a = 0; a < ptNF[j]; a++) for (int b = a; b < ptNF[j]; b++) cnt[(size_t)rankOf(srt[a]) * LBA_MAX_POSES + rankOf(srt[b])]++; }
    std::vector<int> pairOfKey((size_t)LBA_MAX_POSES * LBA_MAX_POSES, -1), pairKey, pairStart(1, 0);
    for (size_t key = 0; key < cnt.size(); key++) if (cnt[key]) { pairOfKey[key] = (int)pairKey.size(); pairKey.push_back((int)key); pairStart.push_back(pairStart.back() + (int)cnt[key]); }
    const int nPair = (int)pairKey.size();
    std::vector<int> pairE(2 * total), at(pairStart.begin(), pairStart.end() - 1), diagPair((size_t)P, -1);
    for (int o = 0; o < nMp; o++) {
        const int j = ptOrder[o]; const int* srt = ptSorted.data() + q.obs_start[j];
        for (int a = 0; a < ptNF[j]; a++) for (int b = a; b < ptNF[j]; b++) { const int pr = pairOfKey[(size_t)rankOf(srt[a]) * LBA_MAX_POSES + rankOf(srt[b])]; const int t = at[pr]++; pairE[2 * t] = srt[a]; pairE[2 * t + 1] = srt[b]; }
    }
    for (int s = 0; s < P; s++) diagPair[s] = pairOfKey[(size_t)s * LBA_MAX_POSES + s];
    pl.nKf = nKf; pl.nMp = nMp; pl.nObs = nObs; pl.P = P; pl.nPair = nPair; pl.nPairE = (int)total;
    pl.I.clear();
    auto add = [&](const int* p, size_t n) { const size_t o = pl.I.size(); pl.I.insert(pl.I.end(), p, p + n); return o; };
    auto room = [&](size_t n) { const size_t o = pl.I.size(); pl.I.resize(o + n, 0); return o; };
    std::vector<int> kind(q.kf_kind, q.kf_kind + nKf);
    pl.oKfKind = add(kind.data(), nKf); pl.oKfPose = add(kfPose.data(), nKf); pl.oPoseKf = add(free_.data(), P); pl.oPtOrder = add(ptOrder.data(), nMp);
    if (nMp) pl.oObsStart = add(q.obs_start, (size_t)nMp + 1); else pl.oObsStart = room(1);
    pl.oEPt = add(ePt.data(), nObs); pl.oEKf = add(q.obs_kf, nObs); pl.oPoseEdgeStart = add(poseEdgeStart.data(), (size_t)P + 1); pl.oPoseEdge = add(poseEdge.data(), poseEdge.size());
    pl.oPtNF = add(ptNF.data(), nMp); pl.oPtSorted = add(ptSorted.data(), nObs); pl.oPairStart = add(pairStart.data(), (size_t)nPair + 1); pl.oPairKey = add(pairKey.data(), nPair);
    pl.oPairE = add(pairE.data(), pairE.size()); pl.oDiagPair = add(diagPair.data(), P);
    pl.oLevel = room(nObs); pl.oPoseIdx = room(P); pl.oPtAct = room(nMp); pl.oIsc = room(LBA_IS_N); pl.oErase = room(nObs);
    const size_t n = 6 * (size_t)P;
    pl.z.ints = pl.I.size(); pl.z.intsOutAt = pl.oErase; pl.z.intsOut = nObs;
    pl.z.floatsIn = 16 * (size_t)nKf + 3 * (size_t)nMp + 4 * (size_t)nObs; pl.z.floatsOut = 16 * (size_t)nKf + 3 * (size_t)nMp; pl.z.head = 8;
    pl.z.work = 8 + LBA_SC_N + 14 * (size_t)nKf + 6 * (size_t)nMp + (size_t)(LBA_C + 18) * nObs + 27 * (size_t)P + 21 * (size_t)nMp + 2 * n * n + 2 * n + 2 * (n + 3 * (size_t)nMp) + nObs;
    return SIND_OK;
}

void lba_fill(const ::sind_localba_item& q, const ItemPtrs& p) {
    const int nObs = q.n_mp ? q.obs_start[q.n_mp] : 0; float* F = p.Fin;
    if (q.n_kf) std::memcpy(F, q.Tcw, sizeof(float) * 16 * q.n_kf);
    F += 16 * (size_t)q.n_kf;
    if (q.n_mp) std::memcpy(F, q.x3Dw, sizeof(float) * 3 * q.n_mp);
    F += 3 * (size_t)q.n_mp;
    for (int e = 0; e < nObs; e++) { F[4 * e] = q.obs_xy[2 * e]; F[4 * e + 1] = q.obs_xy[2 * e + 1]; F[4 * e + 2] = q.u_right[e]; F[4 * e + 3] = q.inv_sigma2[e]; }
}

void lba_bind(const LbaPlan& pl, int doMore, const PoseOptCam& K, const ItemPtrs& p, LbaView& v) {
    int* I = p.I; const float* Fin = p.Fin; float* Fout = p.Fout;
    const size_t nKf = pl.nKf, nMp = pl.nMp, nObs = pl.nObs, P = pl.P, n = 6 * P;
    v.nKf = pl.nKf; v.nMp = pl.nMp; v.nObs = pl.nObs; v.P = pl.P; v.nPair = pl.nPair; v.doMore = doMore; v.K = K;
    v.Tcw = Fin; v.x3Dw = Fin + 16 * nKf; v.eObs = v.x3Dw + 3 * nMp;
    v.kfKind = I + pl.oKfKind; v.kfPose = I + pl.oKfPose; v.poseKf = I + pl.oPoseKf; v.ptOrder = I + pl.oPtOrder; v.obsStart = I + pl.oObsStart; v.ePt = I + pl.oEPt; v.eKf = I + pl.oEKf;
    v.poseEdgeStart = I + pl.oPoseEdgeStart; v.poseEdge = I + pl.oPoseEdge; v.ptNF = I + pl.oPtNF; v.ptSorted = I + pl.oPtSorted; v.pairStart = I + pl.oPairStart; v.pairKey = I + pl.oPairKey;
    v.pairE = I + pl.oPairE; v.diagPair = I + pl.oDiagPair;
    v.level = I + pl.oLevel; v.poseIdx = I + pl.oPoseIdx; v.ptAct = I + pl.oPtAct; v.isc = I + pl.oIsc; v.erase = I + pl.oErase;
    static_assert(sizeof(LbaDiag) <= 8 * sizeof(double) && sizeof(PoseQ) == 7 * sizeof(double), "the layout of the working state");
    double* d = p.D + 8;                                             // the room of the head in the working state
    v.diag = (LbaDiag*)p.head; v.sc = d; d += LBA_SC_N; v.est = (PoseQ*)d; d += 7 * nKf; v.bak = (PoseQ*)d; d += 7 * nKf; v.X = d; d += 3 * nMp; v.Xbak = d; d += 3 * nMp;
    v.C = d; d += LBA_C * nObs; v.BD = d; d += 18 * nObs; v.Hpp = d; d += 27 * P; v.Hll = d; d += 9 * nMp; v.Dinv = d; d += 9 * nMp; v.db = d; d += 3 * nMp;
    v.Hs = d; d += n * n; v.Lm = d; d += n * n; v.Dg = d; d += n; v.y = d; d += n; v.x = d; d += n + 3 * nMp; v.term = d; d += n + 3 * nMp; v.rho = d; d += nObs;
    v.TcwOut = Fout; v.XOut = Fout + 16 * nKf;
}

void lba_store(const ::sind_localba_item& q, const LbaPlan& pl, const ItemPtrs& p) {
    const int* erase = p.I + pl.oErase; const float* Fout = p.Fout;
    LbaDiag dg; std::memcpy(&dg, p.head, sizeof(dg));
    if (pl.nKf) std::memcpy(q.Tcw_out, Fout, sizeof(float) * 16 * pl.nKf);
    if (pl.nMp) std::memcpy(q.x3Dw_out, Fout + 16 * (size_t)pl.nKf, sizeof(float) * 3 * pl.nMp);
    for (int e = 0; e < pl.nObs; e++) q.erase[e] = (uint8_t)erase[e];
    if (q.n_stages) *q.n_stages = dg.stages;
    if (q.n_level1) *q.n_level1 = dg.nLevel1;
    if (q.stage_iters) std::memcpy(q.stage_iters, dg.iters, sizeof(dg.iters));
    if (q.stage_chi2) std::memcpy(q.stage_chi2, dg.chi2, sizeof(dg.chi2));
    if (q.stage_lambda) std::memcpy(q.stage_lambda, dg.lambda, sizeof(dg.lambda));
}

using LbaHost = HostItem<LbaPlan, LbaView>;
// plan -> workspace, Fin and the view
static void lba_host_bind(LbaHost& h, const ::sind_localba_item& q, const float* K5) {
    h.store();
    lba_fill(q, h.p);
    lba_bind(h.pl, q.do_more, {(double)K5[0], (double)K5[1], (double)K5[2], (double)K5[3], (double)K5[4]}, h.p, h.v);
}

}  // namespace sind

extern "C" {

// the same items as sind_match_local_ba, one after the other on the CPU.  -> 0, or SIND_E_ARG / SIND_E_CAPACITY with nothing written
int sindh_local_ba(const sind_localba_item* items, int B, const float* K5) {
    if (B < 0 || (B && !items) || !K5) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (sind::lba_check(items[b])) return SIND_E_ARG;
    std::vector<sind::LbaHost> h((size_t)B);
    for (int b = 0; b < B; b++) if (const int r = sind::lba_plan(items[b], h[b].pl)) return r;     // every limit is checked before anything is written; only the lists are held
    for (int b = 0; b < B; b++) {                                    // the workspace of one item at a time
        sind::lba_host_bind(h[b], items[b], K5);
        sind::SeqExec ex;
        sind::local_ba(ex, h[b].v);
        sind::lba_store(items[b], h[b].pl, h[b].p);
        h[b] = sind::LbaHost();
    }
    return SIND_OK;
}

// one edge at pose qt (q x y z w, t) and point X (the CPU test compares the Jacobians with central differences): c [LBA_C], jac [30] = Xi [3][3], Xj [3][6], error [3]
void sindh_localba_edge(const double* qt, const double* X, const float* ob4, const float* K5, int robust, double* c, double* jac) {
    sind::PoseQ P; for (int k = 0; k < 4; k++) P.q[k] = qt[k]; for (int k = 0; k < 3; k++) P.t[k] = qt[4 + k];
    sind::lba_edge(P, {(double)K5[0], (double)K5[1], (double)K5[2], (double)K5[3], (double)K5[4]}, X, ob4, robust != 0, true, true, c, jac);
}

// the first linearisation of an item and the first trial's solve (the CPU test compares x with a dense solve of the full system): C [n_obs][LBA_C] the edges'
// contributions, x [6 P + 3 n_mp] by pose rank (kind 0 in ascending kf_id) and item point, lambda [1].  -> 0, SIND_E_ARG, SIND_E_CAPACITY, or 1: the factorisation failed
int sindh_localba_linear(const sind_localba_item* item, const float* K5, double* C, double* x, double* lambda) {
    if (!item || !K5 || sind::lba_check(*item)) return SIND_E_ARG;
    sind::LbaHost h;
    if (const int r = sind::lba_plan(*item, h.pl)) return r;
    sind::lba_host_bind(h, *item, K5);
    sind::SeqExec ex; const sind::LbaView& w = h.v;
    ex.par(w.nKf, [&](int i) { sind::po_from_tcw(&w.Tcw[16 * i], w.est[i]); });
    for (int k = 0; k < 3 * w.nMp; k++) w.X[k] = (double)w.x3Dw[k];
    sind::lba_activate(ex, w); sind::lba_eval(ex, w, true, true); sind::lba_sums(ex, w, true); sind::lba_maxdiag(ex, w);
    *lambda = 1e-5 * w.sc[sind::LBA_SC_MAXD];
    sind::lba_solve(ex, w, *lambda, w.isc[sind::LBA_IS_NP]);
    std::memcpy(C, w.C, sizeof(double) * LBA_C * w.nObs); std::memcpy(x, w.x, sizeof(double) * (6 * w.P + 3 * w.nMp));
    return w.isc[sind::LBA_IS_FAIL] ? 1 : 0;
}

}  // extern "C"
