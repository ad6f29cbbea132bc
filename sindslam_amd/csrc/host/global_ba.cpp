// Host twin of sind_match_global_ba (reference src/Optimizer.cc:49-237): global_ba.hpp with the plain runner, and what the two entry points share: the argument
// check, the digest of an item into the lists the phases walk (GbaPlan: the limits first, then the per-pose edge lists, the per-point edges by pose rank, the
// co-observation lists keyed by the two ranks, first(I) and the offsets of the envelope) and the copy of one item's results.  Compiled into libsind_hip.so
// (capi_match_opt.cpp calls the shared part) and into libsind_host.so.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>
#include "global_ba.hpp"
#include "sind_hip.h"

namespace sind {

const char* const gba_check_text[] = {"", "negative count", "null array", "point ids repeat", "an obs_kf is out of range", "a key frame twice in one point's observations",
                                      "obs_start does not start at 0 or decreases", "an inv_sigma2 is not a finite non-negative number", "a pose or point is not finite",
                                      "kf_id is not strictly ascending"};

int gba_check(const ::sind_globalba_item& q) {
    if (q.n_kf < 0 || q.n_mp < 0) return 1;
    if (q.n_kf && (!q.kf_id || !q.Tcw || !q.Tcw_out)) return 2;
    if (q.n_mp && (!q.mp_id || !q.x3Dw || !q.obs_start || !q.x3Dw_out || !q.included)) return 2;
    if (q.n_mp) { if (q.obs_start[0] != 0) return 6; for (int j = 0; j < q.n_mp; j++) if (q.obs_start[j + 1] < q.obs_start[j]) return 6; }
    const int nObs = q.n_mp ? q.obs_start[q.n_mp] : 0;
    if (nObs && (!q.obs_kf || !q.obs_xy || !q.u_right || !q.inv_sigma2)) return 2;
    for (int k = 1; k < q.n_kf; k++) if (q.kf_id[k] <= q.kf_id[k - 1]) return 9;
    { std::vector<int64_t> v(q.mp_id, q.mp_id + q.n_mp); std::sort(v.begin(), v.end()); if (std::adjacent_find(v.begin(), v.end()) != v.end()) return 3; }
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
    return 0;
}

// the block rows of every block column of the envelope: I >= J with first(I) <= J, ascending (J itself first); cs: how many
static void gba_columns(const std::vector<int>& first, std::vector<int>& colStart, std::vector<int>& colRow, std::vector<int>& colLast, std::vector<int>& cs) {
    const int nAct = (int)first.size();
    colStart.assign((size_t)nAct + 1, 0); colLast.assign((size_t)nAct, 0);
    for (int I = 0; I < nAct; I++) for (int J = first[I]; J <= I; J++) colStart[J + 1]++;
    for (int J = 0; J < nAct; J++) colStart[J + 1] += colStart[J];
    colRow.assign((size_t)colStart[nAct], 0);
    std::vector<int> cat(colStart.begin(), colStart.end() - 1);
    for (int I = 0; I < nAct; I++) for (int J = first[I]; J <= I; J++) { colRow[cat[J]++] = I; colLast[J] = I; }
    cs.resize((size_t)nAct);
    for (int J = 0; J < nAct; J++) cs[J] = colStart[J + 1] - colStart[J];
}

int gba_plan(const ::sind_globalba_item& q, GbaPlan& pl) {
    const int nKf = q.n_kf, nMp = q.n_mp, nObs = nMp ? q.obs_start[nMp] : 0;
    if (nKf > GBA_MAX_KF || nMp > GBA_MAX_MP || nObs > GBA_MAX_OBS) return SIND_E_CAPACITY;
    std::vector<int> free_, kfPose((size_t)nKf, -1);                 // kf_id ascends: the item's order is buildIndexMapping's pose order
    for (int k = 0; k < nKf; k++) if (q.kf_id[k] != 0) { kfPose[k] = (int)free_.size(); free_.push_back(k); }
    const int P = (int)free_.size();
    // the counts the limits speak of, before any list: the co-observation entries, then first(I) and the envelope
    std::vector<int> ptNF((size_t)nMp, 0), ptAct((size_t)nMp, 0), nEdge((size_t)P, 0);
    size_t total = 0; int nActPts = 0;
    for (int j = 0; j < nMp; j++) {
        size_t k = 0;
        for (int e = q.obs_start[j]; e < q.obs_start[j + 1]; e++) { const int s = kfPose[q.obs_kf[e]]; if (s >= 0) { k++; nEdge[s]++; } }
        ptNF[j] = (int)k; total += k * (k + 1) / 2;
        ptAct[j] = q.obs_start[j + 1] > q.obs_start[j]; nActPts += ptAct[j];
    }
    if (total > (size_t)GBA_MAX_PAIRS) return SIND_E_CAPACITY;
    std::vector<int> poseIdx((size_t)P, -1);
    int nAct = 0;
    for (int s = 0; s < P; s++) if (nEdge[s]) poseIdx[s] = nAct++;
    std::vector<int> first((size_t)nAct);
    std::iota(first.begin(), first.end(), 0);
    for (int j = 0; j < nMp; j++) {
        int lo = nAct;
        for (int e = q.obs_start[j]; e < q.obs_start[j + 1]; e++) { const int s = kfPose[q.obs_kf[e]]; if (s >= 0) lo = std::min(lo, poseIdx[s]); }
        for (int e = q.obs_start[j]; e < q.obs_start[j + 1]; e++) { const int s = kfPose[q.obs_kf[e]]; if (s >= 0) first[poseIdx[s]] = std::min(first[poseIdx[s]], lo); }
    }
    std::vector<int> rowOff((size_t)nAct + 1, 0);
    size_t env = 0;
    for (int I = 0; I < nAct; I++) { env += (size_t)36 * (I - first[I] + 1); if (env > (size_t)GBA_MAX_ENV) return SIND_E_CAPACITY; rowOff[I + 1] = (int)env; }
    // the lists
    std::vector<int> ptOrder((size_t)nMp); std::iota(ptOrder.begin(), ptOrder.end(), 0);
    std::sort(ptOrder.begin(), ptOrder.end(), [&](int a, int b) { return q.mp_id[a] < q.mp_id[b]; });
    std::vector<int> ePt((size_t)nObs), ptSorted((size_t)nObs, 0), poseEdgeStart((size_t)P + 1, 0);
    auto rankOf = [&](int e) { return kfPose[q.obs_kf[e]]; };
    for (int j = 0; j < nMp; j++) {
        int* srt = ptSorted.data() + q.obs_start[j]; int c = 0;
        for (int e = q.obs_start[j]; e < q.obs_start[j + 1]; e++) { ePt[e] = j; if (rankOf(e) >= 0) srt[c++] = e; }
        std::sort(srt, srt + c, [&](int a, int b) { return rankOf(a) < rankOf(b); });
    }
    for (int s = 0; s < P; s++) poseEdgeStart[s + 1] = poseEdgeStart[s] + nEdge[s];
    std::vector<int> poseEdge((size_t)poseEdgeStart[P]), fill(poseEdgeStart.begin(), poseEdgeStart.end() - 1);
    for (int e = 0; e < nObs; e++) { const int s = rankOf(e); if (s >= 0) poseEdge[fill[s]++] = e; }
    // the co-observation lists: per pair of free poses s1 <= s2 in ascending (s1, s2), the points both see in ascending mp_id.  Generated in point order and sorted
    // stably by the pair, so the order inside a pair stays the point order
    struct Ent { int64_t key; int e1, e2; };
    std::vector<Ent> ent; ent.reserve(total);
    for (int o = 0; o < nMp; o++) {
        const int j = ptOrder[o]; const int* srt = ptSorted.data() + q.obs_start[j];
        for (int a = 0; a < ptNF[j]; a++) for (int b = a; b < ptNF[j]; b++) ent.push_back({(int64_t)rankOf(srt[a]) * P + rankOf(srt[b]), srt[a], srt[b]});
    }
    std::stable_sort(ent.begin(), ent.end(), [](const Ent& a, const Ent& b) { return a.key < b.key; });
    std::vector<int> pairStart, pairS1, pairS2, pairE(2 * total), diagPair((size_t)P, -1);
    for (size_t t = 0; t < total; t++) {
        if (t == 0 || ent[t].key != ent[t - 1].key) {
            const int s1 = (int)(ent[t].key / P), s2 = (int)(ent[t].key % P);
            if (s1 == s2) diagPair[s1] = (int)pairS1.size();
            pairStart.push_back((int)t); pairS1.push_back(s1); pairS2.push_back(s2);
        }
        pairE[2 * t] = ent[t].e1; pairE[2 * t + 1] = ent[t].e2;
    }
    pairStart.push_back((int)total);
    const int nPair = (int)pairS1.size();
    std::vector<Ent>().swap(ent);
    std::vector<int> colStart, colRow, colLast;
    gba_columns(first, colStart, colRow, colLast, pl.cs);

    pl.nKf = nKf; pl.nMp = nMp; pl.nObs = nObs; pl.P = P; pl.nAct = nAct; pl.nActPts = nActPts; pl.nPair = nPair; pl.nEnv = (int)env;
    pl.envDense = (long long)36 * nAct * (nAct + 1) / 2;
    pl.I.clear();
    auto add = [&](const std::vector<int>& v) { const size_t o = pl.I.size(); pl.I.insert(pl.I.end(), v.begin(), v.end()); return o; };
    pl.oKfPose = add(kfPose); pl.oPoseKf = add(free_); pl.oPtOrder = add(ptOrder);
    { const size_t o = pl.I.size(); if (nMp) pl.I.insert(pl.I.end(), q.obs_start, q.obs_start + nMp + 1); else pl.I.push_back(0); pl.oObsStart = o; }
    pl.oEPt = add(ePt);
    { const size_t o = pl.I.size(); if (nObs) pl.I.insert(pl.I.end(), q.obs_kf, q.obs_kf + nObs); pl.oEKf = o; }
    pl.oPoseEdgeStart = add(poseEdgeStart); pl.oPoseEdge = add(poseEdge); pl.oPtNF = add(ptNF); pl.oPtSorted = add(ptSorted);
    pl.oPairStart = add(pairStart); pl.oPairS1 = add(pairS1); pl.oPairS2 = add(pairS2); pl.oPairE = add(pairE); pl.oDiagPair = add(diagPair);
    pl.oPoseIdx = add(poseIdx); pl.oPtAct = add(ptAct);
    pl.oFirst = add(first); pl.oRowOff = add(rowOff); pl.oColStart = add(colStart); pl.oColRow = add(colRow); pl.oColLast = add(colLast);
    const size_t n = 6 * (size_t)nAct, nx = 6 * (size_t)P + 3 * (size_t)nMp;
    pl.z = ItemSizes{};
    pl.z.ints = pl.I.size();
    pl.z.floatsIn = 16 * (size_t)nKf + 3 * (size_t)nMp + 4 * (size_t)nObs; pl.z.floatsOut = 16 * (size_t)nKf + 3 * (size_t)nMp;
    pl.z.work = GBA_SC_N + 14 * (size_t)nKf + 6 * (size_t)nMp + (size_t)(LBA_C + 18) * nObs + 27 * (size_t)P + 21 * (size_t)nMp + env + 2 * n + 2 * nx + nObs;
    return SIND_OK;
}

void gba_fill(const ::sind_globalba_item& q, const ItemPtrs& p) {
    const int nObs = q.n_mp ? q.obs_start[q.n_mp] : 0; float* F = p.Fin;
    if (q.n_kf) std::memcpy(F, q.Tcw, sizeof(float) * 16 * q.n_kf);
    F += 16 * (size_t)q.n_kf;
    if (q.n_mp) std::memcpy(F, q.x3Dw, sizeof(float) * 3 * q.n_mp);
    F += 3 * (size_t)q.n_mp;
    for (int e = 0; e < nObs; e++) { F[4 * (size_t)e] = q.obs_xy[2 * (size_t)e]; F[4 * (size_t)e + 1] = q.obs_xy[2 * (size_t)e + 1]; F[4 * (size_t)e + 2] = q.u_right[e]; F[4 * (size_t)e + 3] = q.inv_sigma2[e]; }
}

void gba_bind(const GbaPlan& pl, const PoseOptCam& K, const ItemPtrs& p, GbaView& v) {
    int* I = p.I; const float* Fin = p.Fin; float* Fout = p.Fout;
    const size_t nKf = pl.nKf, nMp = pl.nMp, nObs = pl.nObs, P = pl.P, n = 6 * (size_t)pl.nAct, nx = 6 * P + 3 * nMp;
    v.nKf = pl.nKf; v.nMp = pl.nMp; v.nObs = pl.nObs; v.P = pl.P; v.nAct = pl.nAct; v.nActPts = pl.nActPts; v.nPair = pl.nPair; v.nEnv = pl.nEnv; v.K = K;
    v.delta[0] = (double)(float)sqrt(5.99); v.delta[1] = (double)(float)sqrt(7.815);        // const float thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815) (:85-86); setDelta takes a double
    v.Tcw = Fin; v.x3Dw = Fin + 16 * nKf; v.eObs = v.x3Dw + 3 * nMp;
    v.kfPose = I + pl.oKfPose; v.poseKf = I + pl.oPoseKf; v.ptOrder = I + pl.oPtOrder; v.obsStart = I + pl.oObsStart; v.ePt = I + pl.oEPt; v.eKf = I + pl.oEKf;
    v.poseEdgeStart = I + pl.oPoseEdgeStart; v.poseEdge = I + pl.oPoseEdge; v.ptNF = I + pl.oPtNF; v.ptSorted = I + pl.oPtSorted;
    v.pairStart = I + pl.oPairStart; v.pairS1 = I + pl.oPairS1; v.pairS2 = I + pl.oPairS2; v.pairE = I + pl.oPairE; v.diagPair = I + pl.oDiagPair;
    v.poseIdx = I + pl.oPoseIdx; v.ptAct = I + pl.oPtAct;
    v.first = I + pl.oFirst; v.rowOff = I + pl.oRowOff; v.colStart = I + pl.oColStart; v.colRow = I + pl.oColRow; v.colLast = I + pl.oColLast;
    static_assert(sizeof(PoseQ) == 7 * sizeof(double), "the layout of the working state");
    double* d = p.D;
    v.sc = d; d += GBA_SC_N; v.est = (PoseQ*)d; d += 7 * nKf; v.bak = (PoseQ*)d; d += 7 * nKf; v.X = d; d += 3 * nMp; v.Xbak = d; d += 3 * nMp;
    v.C = d; d += LBA_C * nObs; v.BD = d; d += 18 * nObs; v.Hpp = d; d += 27 * P; v.Hll = d; d += 9 * nMp; v.Dinv = d; d += 9 * nMp; v.db = d; d += 3 * nMp;
    v.E = d; d += (size_t)pl.nEnv; v.Dg = d; d += n; v.y = d; d += n; v.x = d; d += nx; v.term = d; d += nx; v.rho = d; d += nObs;
    v.TcwOut = Fout; v.XOut = Fout + 16 * nKf;
}

void gba_store(const ::sind_globalba_item& q, const GbaPlan& pl, const ItemPtrs& p, const GbaDiag& dg) {
    const float* Fout = p.Fout; const int* ptAct = pl.I.data() + pl.oPtAct;
    if (pl.nKf) std::memcpy(q.Tcw_out, Fout, sizeof(float) * 16 * pl.nKf);
    if (pl.nMp) std::memcpy(q.x3Dw_out, Fout + 16 * (size_t)pl.nKf, sizeof(float) * 3 * pl.nMp);
    for (int j = 0; j < pl.nMp; j++) q.included[j] = (uint8_t)ptAct[j];
    if (q.n_iters) *q.n_iters = dg.iters;
    if (q.chi2) *q.chi2 = dg.chi2;
    if (q.lambda) *q.lambda = dg.lambda;
    if (q.n_active_poses) *q.n_active_poses = dg.nActive;
    if (q.solver_fail) *q.solver_fail = dg.fails;
    if (q.env_entries) *q.env_entries = pl.nEnv;
    if (q.env_dense_entries) *q.env_dense_entries = pl.envDense;
}

using GbaHost = HostItem<GbaPlan, GbaView>;
static void gba_host_bind(GbaHost& h, const ::sind_globalba_item& q, const float* K5) {
    h.store();
    gba_fill(q, h.p);
    gba_bind(h.pl, {(double)K5[0], (double)K5[1], (double)K5[2], (double)K5[3], (double)K5[4]}, h.p, h.v);
}

}  // namespace sind

extern "C" {

// the same items as sind_match_global_ba, one after the other on the CPU.  -> 0, or SIND_E_ARG / SIND_E_CAPACITY with nothing written
int sindh_global_ba(const sind_globalba_item* items, int B, int iterations, int robust, const float* K5) {
    if (B < 0 || (B && !items) || !K5 || iterations < 0) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (sind::gba_check(items[b])) return SIND_E_ARG;
    std::vector<sind::GbaHost> h((size_t)B);
    for (int b = 0; b < B; b++) if (const int r = sind::gba_plan(items[b], h[b].pl)) return r;     // every limit is checked before anything is written
    for (int b = 0; b < B; b++) {                                    // the workspace of one item at a time
        sind::gba_host_bind(h[b], items[b], K5);
        sind::GbaSeqRun run; sind::GbaDiag dg{};
        sind::global_ba(run, h[b].v, h[b].pl.cs.data(), iterations, robust != 0, dg);
        sind::gba_store(items[b], h[b].pl, h[b].p, dg);
        h[b] = sind::GbaHost();
    }
    return SIND_OK;
}

// the check and the plan alone (the tests reach every limit through it without a workspace): -> 0, SIND_E_ARG or SIND_E_CAPACITY; sizes [4] = free key frames with
// an edge, co-observation pairs, stored entries of the envelope, doubles of the workspace (as double)
int sindh_globalba_plan(const sind_globalba_item* item, double* sizes) {
    if (!item || sind::gba_check(*item)) return SIND_E_ARG;
    sind::GbaPlan pl;
    if (const int r = sind::gba_plan(*item, pl)) return r;
    if (sizes) { sizes[0] = pl.nAct; sizes[1] = pl.nPair; sizes[2] = pl.nEnv; sizes[3] = (double)pl.z.work; }
    return SIND_OK;
}

// the first linearisation of an item and the first trial's solve (the CPU test compares x with a dense solve of the full system): C [n_obs][LBA_C] the edges'
// contributions, x [6 P + 3 n_mp] by pose rank (kf_id != 0, ascending) and item point, lambda [1].  -> 0, SIND_E_ARG, SIND_E_CAPACITY, or 1: the factorisation failed
int sindh_globalba_linear(const sind_globalba_item* item, int robust, const float* K5, double* C, double* x, double* lambda) {
    if (!item || !K5 || sind::gba_check(*item)) return SIND_E_ARG;
    sind::GbaHost h;
    if (const int r = sind::gba_plan(*item, h.pl)) return r;
    sind::gba_host_bind(h, *item, K5);
    sind::GbaSeqRun run; const sind::GbaView& w = h.v;
    run.go(w.nKf + w.nMp, sind::GbaInit{w}); run.go(6 * w.P + 3 * w.nMp, sind::GbaZeroX{w});
    sind::GbaLm<sind::GbaSeqRun> lm{run, w, h.pl.cs.data(), robust != 0};
    lm.linearize(); *lambda = 1e-5 * lm.max_diagonal();
    std::memcpy(C, w.C, sizeof(double) * LBA_C * w.nObs);            // of the linearisation: the trial below rewrites rho[0] and chi2 alone
    const bool ok = lm.solve(*lambda);
    std::memcpy(x, w.x, sizeof(double) * (6 * w.P + 3 * w.nMp));
    return ok ? 0 : 1;
}

// the factorisation and the two solves alone, on a matrix the caller gives (the CPU test: the envelope against the dense definition, and the zero pivot): nAct block
// rows, first [nAct] with first[I] <= I, H [n][n] row-major symmetric (n = 6 nAct; entries left of a row's first stored column are not read), b [n], x [n] in and out.
// -> 0, 1: a zero pivot, x untouched; SIND_E_ARG
int sindh_globalba_factor(int nAct, const int* first, const double* H, const double* b, double* x, double* D) {
    if (nAct < 0 || (nAct && (!first || !H || !b || !x || !D))) return SIND_E_ARG;
    for (int I = 0; I < nAct; I++) if (first[I] < 0 || first[I] > I) return SIND_E_ARG;
    const int n = 6 * nAct;
    std::vector<int> f(first, first + nAct), rowOff((size_t)nAct + 1, 0), colStart, colRow, colLast, cs, idx((size_t)nAct);
    for (int I = 0; I < nAct; I++) { rowOff[I + 1] = rowOff[I] + 36 * (I - f[I] + 1); idx[I] = I; }
    sind::gba_columns(f, colStart, colRow, colLast, cs);
    std::vector<double> E((size_t)rowOff[nAct] + 1, 0.0), Dg((size_t)n + 1, 0.0), y(b, b + n), sc(sind::GBA_SC_N, 0.0);
    sind::GbaView w{};
    w.P = nAct; w.nAct = nAct; w.nEnv = rowOff[nAct]; w.first = f.data(); w.rowOff = rowOff.data(); w.colStart = colStart.data(); w.colRow = colRow.data(); w.colLast = colLast.data();
    w.poseIdx = idx.data(); w.E = E.data(); w.Dg = Dg.data(); w.y = y.data(); w.x = x; w.sc = sc.data();
    for (int i = 0; i < n; i++) for (int j = sind::gba_fcol(w, i); j <= i; j++) E[sind::gba_at(w, i, j)] = H[(size_t)j * n + i];
    sind::GbaSeqRun run;
    for (int J = 0; J < nAct; J++) { run.go(36 * cs[J], sind::GbaFactorPre{w, J}); run.go(1, sind::GbaFactorDiag{w, J}); run.go(6 * (cs[J] - 1), sind::GbaFactorPost{w, J}); }
    run.tri(w);
    for (int i = 0; i < n; i++) D[i] = Dg[i];
    return sc[sind::GBA_SC_FAIL] != 0.0 ? 1 : 0;
}

}  // extern "C"
