// Host twin of sind_match_global_ba (reference src/Optimizer.cc:49-237): global_ba.hpp with the plain runner, and what the two entry points share: the argument
// check, the digest of an item (GbaPlan: the limits first, then global BA's rule for the free poses and the active sets over ba_plan.cpp's lists, first(I) and the
// offsets of the envelope) and the copy of one item's results.  Compiled into libsind_hip.so (capi_match_opt.cpp calls the shared part) and into libsind_host.so.
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
    const BaItem it = ba_item(q);
    if (const int r = ba_check_arrays(it, false, !q.included, false)) return r;
    for (int k = 1; k < q.n_kf; k++) if (q.kf_id[k] <= q.kf_id[k - 1]) return 9;
    if (ba_ids_repeat(q.mp_id, q.n_mp)) return 3;
    return ba_check_obs(it);
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
    const BaItem it = ba_item(q);
    const int nKf = it.nKf, nMp = it.nMp, nObs = it.nObs;
    if (nKf > GBA_MAX_KF || nMp > GBA_MAX_MP || nObs > GBA_MAX_OBS) return SIND_E_CAPACITY;
    std::vector<int> free_, kfPose((size_t)nKf, -1);                 // kf_id ascends: the item's order is buildIndexMapping's pose order
    for (int k = 0; k < nKf; k++) if (q.kf_id[k] != 0) { kfPose[k] = (int)free_.size(); free_.push_back(k); }
    const int P = (int)free_.size();
    // the counts the limits speak of, before any list: the co-observation entries, then first(I) and the envelope
    std::vector<int> ptNF, nEdge, ptAct((size_t)nMp, 0);
    const size_t total = ba_count(it, kfPose, P, ptNF, nEdge);
    if (total > (size_t)GBA_MAX_PAIRS) return SIND_E_CAPACITY;
    int nActPts = 0;
    for (int j = 0; j < nMp; j++) { ptAct[j] = q.obs_start[j + 1] > q.obs_start[j]; nActPts += ptAct[j]; }
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
    ba_lists(it, kfPose, free_, ptNF, nEdge, total, pl);
    std::vector<int> colStart, colRow, colLast;
    gba_columns(first, colStart, colRow, colLast, pl.cs);

    pl.nAct = nAct; pl.nActPts = nActPts; pl.nEnv = (int)env;
    pl.envDense = (long long)36 * nAct * (nAct + 1) / 2;
    pl.oPoseIdx = pl.add(poseIdx); pl.oPtAct = pl.add(ptAct);
    pl.oFirst = pl.add(first); pl.oRowOff = pl.add(rowOff); pl.oColStart = pl.add(colStart); pl.oColRow = pl.add(colRow); pl.oColLast = pl.add(colLast);
    ba_sizes(pl);
    pl.z.work += env + 12 * (size_t)nAct;                            // the envelope, Dg, y
    return SIND_OK;
}

void gba_bind(const GbaPlan& pl, const PoseOptCam& K, const ItemPtrs& p, GbaView& v) {
    int* I = p.I; const size_t n = 6 * (size_t)pl.nAct, nx = 6 * (size_t)pl.P + 3 * (size_t)pl.nMp;
    double* d = ba_bind(pl, K, p, p.D, v);
    v.nAct = pl.nAct; v.nActPts = pl.nActPts; v.nEnv = pl.nEnv;
    v.delta[0] = (double)(float)sqrt(5.99); v.delta[1] = (double)(float)sqrt(7.815);        // const float thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815) (:85-86); setDelta takes a double
    v.first = I + pl.oFirst; v.rowOff = I + pl.oRowOff; v.colStart = I + pl.oColStart; v.colRow = I + pl.oColRow; v.colLast = I + pl.oColLast;
    v.Hs = d; d += (size_t)pl.nEnv; v.Dg = d; d += n; v.y = d; d += n; v.x = d; d += nx; v.term = d; d += nx; v.rho = d; d += pl.nObs;
}

void gba_store(const ::sind_globalba_item& q, const GbaPlan& pl, const ItemPtrs& p, const GbaDiag& dg) {
    const int* ptAct = pl.I.data() + pl.oPtAct;
    ba_store(ba_item(q), pl, p);
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
    ba_fill(ba_item(q), h.p);
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
    std::vector<double> E((size_t)rowOff[nAct] + 1, 0.0), Dg((size_t)n + 1, 0.0), y(b, b + n), sc(sind::BA_SC_N, 0.0);
    sind::GbaView w{};
    w.P = nAct; w.nAct = nAct; w.nEnv = rowOff[nAct]; w.first = f.data(); w.rowOff = rowOff.data(); w.colStart = colStart.data(); w.colRow = colRow.data(); w.colLast = colLast.data();
    w.poseIdx = idx.data(); w.Hs = E.data(); w.Dg = Dg.data(); w.y = y.data(); w.x = x; w.sc = sc.data();
    for (int i = 0; i < n; i++) for (int j = sind::gba_fcol(w, i); j <= i; j++) E[sind::gba_at(w, i, j)] = H[(size_t)j * n + i];
    sind::GbaSeqRun run;
    for (int J = 0; J < nAct; J++) { run.go(36 * cs[J], sind::GbaFactorPre{w, J}); run.go(1, sind::GbaFactorDiag{w, J}); run.go(6 * (cs[J] - 1), sind::GbaFactorPost{w, J}); }
    run.tri(w);
    for (int i = 0; i < n; i++) D[i] = Dg[i];
    return sc[sind::BA_SC_FAIL] != 0.0 ? 1 : 0;
}

}  // extern "C"
