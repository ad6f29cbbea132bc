// Host twin of sind_match_local_ba (reference src/Optimizer.cc:506-778): local_ba.hpp with the plain sequential executor, and what the two entry points share: the
// argument check, the digest of an item (LbaPlan: local BA's rule for the free poses and its limits over ba_plan.cpp's lists) and the copy of one item's results.
// Compiled into libsind_hip.so (capi_match_opt.cpp calls the shared part) and into libsind_host.so.
#include <algorithm>
#include <cstring>
#include <vector>
#include "local_ba.hpp"
#include "sind_hip.h"

namespace sind {

const char* const lba_check_text[] = {"", "negative count", "null array", "ids repeat", "an obs_kf is out of range", "a key frame twice in one point's observations",
                                      "obs_start does not start at 0 or decreases", "an inv_sigma2 is not a finite non-negative number", "a pose or point is not finite",
                                      "no key frame of kind 0", "a kf_kind outside 0..2"};

int lba_check(const ::sind_localba_item& q) {
    const BaItem it = ba_item(q);
    if (const int r = ba_check_arrays(it, !q.kf_kind, false, !q.erase)) return r;
    if (ba_ids_repeat(q.kf_id, q.n_kf) || ba_ids_repeat(q.mp_id, q.n_mp)) return 3;
    bool local = false;
    for (int k = 0; k < q.n_kf; k++) { if (q.kf_kind[k] > 2) return 10; local = local || q.kf_kind[k] == 0; }
    if (const int r = ba_check_obs(it)) return r;
    if (!local) return 9;
    return 0;
}

int lba_plan(const ::sind_localba_item& q, LbaPlan& pl) {
    const BaItem it = ba_item(q);
    const int nKf = it.nKf, nMp = it.nMp, nObs = it.nObs;
    std::vector<int> free_;                                          // the key frames of kind 0 in ascending kf_id: buildIndexMapping's pose order
    for (int k = 0; k < nKf; k++) if (q.kf_kind[k] == 0) free_.push_back(k);
    std::sort(free_.begin(), free_.end(), [&](int a, int b) { return q.kf_id[a] < q.kf_id[b]; });
    const int P = (int)free_.size();
    if (P > LBA_MAX_POSES || nKf > LBA_MAX_KF || nMp > LBA_MAX_MP || nObs > LBA_MAX_OBS) return SIND_E_CAPACITY;
    std::vector<int> kfPose((size_t)nKf, -1), ptNF, nEdge;
    for (int s = 0; s < P; s++) kfPose[free_[s]] = s;
    const size_t total = ba_count(it, kfPose, P, ptNF, nEdge);
    if (total > (size_t)LBA_MAX_PAIRS) return SIND_E_CAPACITY;
    ba_lists(it, kfPose, free_, ptNF, nEdge, total, pl);
    std::vector<int> kind(q.kf_kind, q.kf_kind + nKf);
    pl.oKfKind = pl.add(kind);
    pl.oLevel = pl.room(nObs); pl.oPoseIdx = pl.room(P); pl.oPtAct = pl.room(nMp); pl.oIsc = pl.room(LBA_IS_N); pl.oErase = pl.room(nObs);
    const size_t n = 6 * (size_t)P;
    ba_sizes(pl);
    pl.z.intsOutAt = pl.oErase; pl.z.intsOut = nObs; pl.z.head = 8;
    pl.z.work += 8 + 2 * n * n + 2 * n;                              // the room of the head, Hs, Lm, Dg, y
    return SIND_OK;
}

void lba_bind(const LbaPlan& pl, int doMore, const PoseOptCam& K, const ItemPtrs& p, LbaView& v) {
    int* I = p.I; const size_t n = 6 * (size_t)pl.P, nx = n + 3 * (size_t)pl.nMp;
    static_assert(sizeof(LbaDiag) <= 8 * sizeof(double), "the layout of the working state");
    double* d = ba_bind(pl, K, p, p.D + 8, v);                       // the room of the head in the working state
    v.doMore = doMore; v.kfKind = I + pl.oKfKind; v.level = I + pl.oLevel; v.isc = I + pl.oIsc; v.erase = I + pl.oErase; v.diag = (LbaDiag*)p.head;
    v.Hs = d; d += n * n; v.Lm = d; d += n * n; v.Dg = d; d += n; v.y = d; d += n; v.x = d; d += nx; v.term = d; d += nx; v.rho = d; d += pl.nObs;
}

void lba_store(const ::sind_localba_item& q, const LbaPlan& pl, const ItemPtrs& p) {
    const int* erase = p.I + pl.oErase;
    LbaDiag dg; std::memcpy(&dg, p.head, sizeof(dg));
    ba_store(ba_item(q), pl, p);
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
    ba_fill(ba_item(q), h.p);
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
    sind::ba_edge(P, {(double)K5[0], (double)K5[1], (double)K5[2], (double)K5[3], (double)K5[4]}, X, ob4, robust != 0, true, true, c, jac);
}

// the first linearisation of an item and the first trial's solve (the CPU test compares x with a dense solve of the full system): C [n_obs][LBA_C] the edges'
// contributions, x [6 P + 3 n_mp] by pose rank (kind 0 in ascending kf_id) and item point, lambda [1].  -> 0, SIND_E_ARG, SIND_E_CAPACITY, or 1: the factorisation failed
int sindh_localba_linear(const sind_localba_item* item, const float* K5, double* C, double* x, double* lambda) {
    if (!item || !K5 || sind::lba_check(*item)) return SIND_E_ARG;
    sind::LbaHost h;
    if (const int r = sind::lba_plan(*item, h.pl)) return r;
    sind::lba_host_bind(h, *item, K5);
    sind::SeqExec ex; const sind::LbaView& w = h.v;
    ex.par(w.nKf + w.nMp, [&](int i) { sind::ba_init_elem(w, i); });
    sind::lba_activate(ex, w); sind::lba_eval(ex, w, true, true); sind::lba_sums(ex, w, true); sind::lba_maxdiag(ex, w);
    *lambda = 1e-5 * w.sc[sind::BA_SC_MAXD];
    sind::lba_solve(ex, w, *lambda, w.isc[sind::LBA_IS_NP]);
    std::memcpy(C, w.C, sizeof(double) * LBA_C * w.nObs); std::memcpy(x, w.x, sizeof(double) * (6 * w.P + 3 * w.nMp));
    return w.isc[sind::LBA_IS_FAIL] ? 1 : 0;
}

}  // extern "C"
