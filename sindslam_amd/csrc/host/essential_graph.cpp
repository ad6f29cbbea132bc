// Host twin of sind_match_essential_graph (reference src/Optimizer.cc:781-1044): essential_graph.hpp with the plain sequential executor, and what the two entry
// points share: the argument check, the digest of an item into the lists the phases walk (EssPlan) and the copy of one item's results.  Compiled into libsind_hip.so
// (capi_match_opt.cpp calls the shared part) and into libsind_host.so.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>
#include "essential_graph.hpp"
#include "sind_hip.h"

namespace sind {

const char* const ess_check_text[] = {"", "negative count", "null array", "kf_id is not strictly ascending", "fixed_kf is out of range", "an edge end is out of range",
                                      "an edge joins a key frame with itself", "an edge_kind outside 0..1", "an mp_ref is out of range",
                                      "a pose, Sim3 or point is not finite", "a scale is not positive"};

int ess_check(const ::sind_essgraph_item& q) {
    if (q.n_kf < 0 || q.n_edges < 0 || q.n_mp < 0) return 1;
    if (q.n_kf && (!q.kf_id || !q.Tcw || !q.has_corrected || !q.corrected || !q.has_noncorrected || !q.noncorrected || !q.Siw_out || !q.Tiw_out)) return 2;
    if (q.n_edges && (!q.edge_i || !q.edge_j || !q.edge_kind)) return 2;
    if (q.n_mp && (!q.x3Dw || !q.mp_ref || !q.x3Dw_out)) return 2;
    for (int k = 1; k < q.n_kf; k++) if (!(q.kf_id[k - 1] < q.kf_id[k])) return 3;
    if (q.n_kf && (q.fixed_kf < 0 || q.fixed_kf >= q.n_kf)) return 4;
    for (int e = 0; e < q.n_edges; e++) {
        if (q.edge_i[e] < 0 || q.edge_i[e] >= q.n_kf || q.edge_j[e] < 0 || q.edge_j[e] >= q.n_kf) return 5;
        if (q.edge_i[e] == q.edge_j[e]) return 6;
        if (q.edge_kind[e] > 1) return 7;
    }
    for (int j = 0; j < q.n_mp; j++) if (q.mp_ref[j] < 0 || q.mp_ref[j] >= q.n_kf) return 8;
    for (size_t k = 0; k < (size_t)16 * q.n_kf; k++) if (!std::isfinite(q.Tcw[k])) return 9;
    for (size_t k = 0; k < (size_t)3 * q.n_mp; k++) if (!std::isfinite(q.x3Dw[k])) return 9;
    for (int i = 0; i < q.n_kf; i++) for (int side = 0; side < 2; side++) {
        if (!(side ? q.has_noncorrected[i] : q.has_corrected[i])) continue;
        const double* p = (side ? q.noncorrected : q.corrected) + 8 * (size_t)i;
        for (int k = 0; k < 8; k++) if (!std::isfinite(p[k])) return 9;
        if (!(p[7] > 0.0)) return 10;
    }
    return 0;
}

int ess_plan(const ::sind_essgraph_item& q, EssPlan& pl) {
    const int nKf = q.n_kf, nE = q.n_edges, nMp = q.n_mp;
    if (nKf > ESS_MAX_KF || nE > ESS_MAX_EDGES || nMp > ESS_MAX_MP) return SIND_E_CAPACITY;
    std::vector<int> deg((size_t)nKf, 0), vIdx((size_t)nKf, -1), idxV;
    for (int e = 0; e < nE; e++) { deg[q.edge_i[e]]++; deg[q.edge_j[e]]++; }
    for (int i = 0; i < nKf; i++) if (i != q.fixed_kf && deg[i]) { vIdx[i] = (int)idxV.size(); idxV.push_back(i); }     // buildIndexMapping: ascending id
    const int nAct = (int)idxV.size();
    std::vector<int> vEdgeStart((size_t)nAct + 1, 0), first((size_t)nAct), rowOff((size_t)nAct, 0), blkLast((size_t)nAct, 0);
    for (int a = 0; a < nAct; a++) first[a] = a;
    std::map<std::pair<int, int>, std::vector<int>> pairs;           // (lo, hi) -> its edges in ascending order
    for (int e = 0; e < nE; e++) {
        const int a = vIdx[q.edge_i[e]], b = vIdx[q.edge_j[e]];
        if (a >= 0) vEdgeStart[a + 1]++;
        if (b >= 0) vEdgeStart[b + 1]++;
        if (a >= 0 && b >= 0) { const int lo = std::min(a, b), hi = std::max(a, b); first[hi] = std::min(first[hi], lo); pairs[{lo, hi}].push_back(2 * e + (a == hi ? 1 : 0)); }
    }
    for (int a = 0; a < nAct; a++) vEdgeStart[a + 1] += vEdgeStart[a];
    std::vector<int> vEdge((size_t)vEdgeStart[nAct]), fill(vEdgeStart.begin(), vEdgeStart.end() - 1);
    for (int e = 0; e < nE; e++) {
        const int a = vIdx[q.edge_i[e]], b = vIdx[q.edge_j[e]];
        if (a >= 0) vEdge[fill[a]++] = 2 * e;
        if (b >= 0) vEdge[fill[b]++] = 2 * e + 1;
    }
    size_t nEnv = 0;
    std::vector<int> lastOfFirst((size_t)nAct, -1);
    for (int a = 0; a < nAct; a++) {
        if (nEnv > (size_t)ESS_MAX_ENV) return SIND_E_CAPACITY;
        rowOff[a] = (int)nEnv; nEnv += 49 * (size_t)(a - first[a] + 1); lastOfFirst[first[a]] = a;
    }
    if (nEnv > (size_t)ESS_MAX_ENV) return SIND_E_CAPACITY;
    for (int a = 0, run = -1; a < nAct; a++) { run = std::max(run, lastOfFirst[a]); blkLast[a] = run; }
    std::vector<int> pairStart(1, 0), pairLo, pairHi, pairE;
    for (const auto& kv : pairs) { pairLo.push_back(kv.first.first); pairHi.push_back(kv.first.second); pairE.insert(pairE.end(), kv.second.begin(), kv.second.end()); pairStart.push_back((int)pairE.size()); }
    const int nPair = (int)pairLo.size();
    pl.nKf = nKf; pl.nE = nE; pl.nMp = nMp; pl.nAct = nAct; pl.nPair = nPair; pl.nEnv = nEnv;
    pl.I.clear();
    auto add = [&](const int* p, size_t n) { const size_t o = pl.I.size(); if (n) pl.I.insert(pl.I.end(), p, p + n); return o; };
    auto room = [&](size_t n) { const size_t o = pl.I.size(); pl.I.resize(o + n, 0); return o; };
    std::vector<int> hasC((size_t)nKf), hasN((size_t)nKf), kind((size_t)nE);
    for (int i = 0; i < nKf; i++) { hasC[i] = q.has_corrected[i] ? 1 : 0; hasN[i] = q.has_noncorrected[i] ? 1 : 0; }
    for (int e = 0; e < nE; e++) kind[e] = q.edge_kind[e];
    pl.oHasC = add(hasC.data(), nKf); pl.oHasN = add(hasN.data(), nKf); pl.oMpRef = add(q.mp_ref, nMp); pl.oEI = add(q.edge_i, nE); pl.oEJ = add(q.edge_j, nE); pl.oEKind = add(kind.data(), nE);
    pl.oVIdx = add(vIdx.data(), nKf); pl.oIdxV = add(idxV.data(), nAct); pl.oVEdgeStart = add(vEdgeStart.data(), (size_t)nAct + 1); pl.oVEdge = add(vEdge.data(), vEdge.size());
    pl.oPairStart = add(pairStart.data(), (size_t)nPair + 1); pl.oPairLo = add(pairLo.data(), nPair); pl.oPairHi = add(pairHi.data(), nPair); pl.oPairE = add(pairE.data(), pairE.size());
    pl.oFirst = add(first.data(), nAct); pl.oRowOff = add(rowOff.data(), nAct); pl.oBlkLast = add(blkLast.data(), nAct);
    pl.oIsc = room(ESS_IS_N);
    const size_t n = 7 * (size_t)nAct;
    pl.z.ints = pl.I.size(); pl.z.floatsIn = pl.z.floatsOut = 16 * (size_t)nKf + 3 * (size_t)nMp; pl.z.doublesIn = 16 * (size_t)nKf; pl.z.head = 8 + 8 * (size_t)nKf;
    pl.z.work = 8 + 8 * (size_t)nKf + ESS_SC_N + 4 * 8 * (size_t)nKf + 8 * (size_t)nE + 2 * 8 * SIM3OPT_TRANSFORMS * (size_t)nKf + (size_t)(ESS_NERR * 7 + 98 + ESS_C + 1) * nE +
                ESS_V * (size_t)nAct + 49 * (size_t)nPair + nEnv + 4 * n;
    return SIND_OK;
}

void ess_fill(const ::sind_essgraph_item& q, const ItemPtrs& p) {
    float* F = p.Fin; double* Din = p.Din;
    if (q.n_kf) std::memcpy(F, q.Tcw, sizeof(float) * 16 * q.n_kf);
    if (q.n_mp) std::memcpy(F + 16 * (size_t)q.n_kf, q.x3Dw, sizeof(float) * 3 * q.n_mp);
    for (int i = 0; i < q.n_kf; i++) for (int k = 0; k < 8; k++) {                         // an entry that is not there is not read by the caller's leave, nor by the phases
        Din[8 * (size_t)i + k] = q.has_corrected[i] ? q.corrected[8 * (size_t)i + k] : 0.0;
        Din[8 * (size_t)(q.n_kf + i) + k] = q.has_noncorrected[i] ? q.noncorrected[8 * (size_t)i + k] : 0.0;
    }
}

void ess_bind(const EssPlan& pl, int fixScale, const ItemPtrs& p, EssView& v) {
    int* I = p.I; const float* Fin = p.Fin; const double* Din = p.Din; float* Fout = p.Fout;
    const size_t nKf = pl.nKf, nE = pl.nE, nAct = pl.nAct, n = 7 * nAct;
    v.nKf = pl.nKf; v.nE = pl.nE; v.nMp = pl.nMp; v.nAct = pl.nAct; v.nPair = pl.nPair; v.n = (int)n; v.fixScale = fixScale ? 1 : 0;
    v.Tcw = Fin; v.x3Dw = Fin + 16 * nKf; v.corr = Din; v.ncorr = Din + 8 * nKf;
    v.hasC = I + pl.oHasC; v.hasN = I + pl.oHasN; v.mpRef = I + pl.oMpRef; v.eI = I + pl.oEI; v.eJ = I + pl.oEJ; v.eKind = I + pl.oEKind; v.vIdx = I + pl.oVIdx; v.idxV = I + pl.oIdxV;
    v.vEdgeStart = I + pl.oVEdgeStart; v.vEdge = I + pl.oVEdge; v.pairStart = I + pl.oPairStart; v.pairLo = I + pl.oPairLo; v.pairHi = I + pl.oPairHi; v.pairE = I + pl.oPairE;
    v.first = I + pl.oFirst; v.rowOff = I + pl.oRowOff; v.blkLast = I + pl.oBlkLast; v.isc = I + pl.oIsc;
    static_assert(sizeof(EssDiag) <= 8 * sizeof(double) && sizeof(Sim3Q) == 8 * sizeof(double), "the layout of the working state");
    double* d = p.D + 8 + 8 * nKf;                                   // the room of the head in the working state
    v.diag = (EssDiag*)p.head; v.SiwOut = p.head + 8; v.sc = d; d += ESS_SC_N;
    v.vScw = (Sim3Q*)d; d += 8 * nKf; v.est = (Sim3Q*)d; d += 8 * nKf; v.bak = (Sim3Q*)d; d += 8 * nKf; v.Swc = (Sim3Q*)d; d += 8 * nKf; v.meas = (Sim3Q*)d; d += 8 * nE;
    v.T = (Sim3Q*)d; d += 8 * SIM3OPT_TRANSFORMS * nKf; v.Ti = (Sim3Q*)d; d += 8 * SIM3OPT_TRANSFORMS * nKf;
    v.E = d; d += ESS_NERR * 7 * nE; v.J = d; d += 98 * nE; v.C = d; d += ESS_C * nE; v.chiE = d; d += nE;
    v.Hd = d; d += ESS_V * nAct; v.Ho = d; d += 49 * (size_t)pl.nPair; v.M = d; d += pl.nEnv; v.Dg = d; d += n; v.y = d; d += n; v.x = d; d += n; v.term = d; d += n;
    v.TiwOut = Fout; v.XOut = Fout + 16 * nKf;
}

void ess_store(const ::sind_essgraph_item& q, const EssPlan& pl, const ItemPtrs& p) {
    const float* Fout = p.Fout; const double* Dout = p.head;
    EssDiag dg; std::memcpy(&dg, Dout, sizeof(dg));
    if (pl.nKf) { std::memcpy(q.Siw_out, Dout + 8, sizeof(double) * 8 * pl.nKf); std::memcpy(q.Tiw_out, Fout, sizeof(float) * 16 * pl.nKf); }
    if (pl.nMp) std::memcpy(q.x3Dw_out, Fout + 16 * (size_t)pl.nKf, sizeof(float) * 3 * pl.nMp);
    if (q.n_iters) *q.n_iters = dg.iters;
    if (q.chi2) *q.chi2 = dg.chi2;
    if (q.lambda) *q.lambda = dg.lambda;
    if (q.n_active) *q.n_active = dg.nActive;
    if (q.solver_fail) *q.solver_fail = dg.solverFail;
}

using EssHost = HostItem<EssPlan, EssView>;
// plan -> workspace, Fin, Din and the view
static void ess_host_bind(EssHost& h, const ::sind_essgraph_item& q, int fixScale) {
    h.store();
    ess_fill(q, h.p);
    ess_bind(h.pl, fixScale, h.p, h.v);
}

}  // namespace sind

extern "C" {

// the same items as sind_match_essential_graph, one after the other on the CPU.  -> 0, or SIND_E_ARG / SIND_E_CAPACITY with nothing written
int sindh_essential_graph(const sind_essgraph_item* items, int B, int fix_scale) {
    if (B < 0 || (B && !items)) return SIND_E_ARG;
    for (int b = 0; b < B; b++) if (sind::ess_check(items[b])) return SIND_E_ARG;
    std::vector<sind::EssHost> h((size_t)B);
    for (int b = 0; b < B; b++) if (const int r = sind::ess_plan(items[b], h[b].pl)) return r;                   // every limit is checked before anything is written; only the lists are held
    for (int b = 0; b < B; b++) {                                    // the workspace of one item at a time
        sind::ess_host_bind(h[b], items[b], fix_scale);
        sind::SeqExec ex; const sind::EssView& w = h[b].v;
        sind::essential_graph(ex, w);
        for (int j = 0; j < w.nMp; j++) sind::ess_point(w, j);
        sind::ess_store(items[b], h[b].pl, h[b].p);
        h[b] = sind::EssHost();
    }
    return SIND_OK;
}

// the defined log and acos, Sim3::log and Sim3(Vector7d) for the CPU tests: S = qx qy qz qw tx ty tz s
double sindh_ess_log(double x) { return sind::s3_log_d(x); }
double sindh_ess_acos(double x) { return sind::s3_acos_d(x); }
void sindh_ess_sim3_log(const double* S, double* u7) { sind::Sim3Q q; sind::s3_load8(S, q); sind::s3_log(q, u7); }
void sindh_ess_sim3_exp(const double* u7, double* S) { sind::Sim3Q q; sind::s3_exp7(u7, q); sind::s3_store8(q, S); }

// the first linearisation of an item and the first trial's solve (the CPU test compares the envelope's x with a dense LDL^T of the same definition and with a dense
// solve): H [n][n] the full symmetric Hessian WITHOUT lambda, b [n], x [n], lambda [1], n = 7 * n_active in Hessian-index order; env [2] = n and the envelope's stored
// entries; any of H, b, x may be NULL (to ask for n first).  -> 0, SIND_E_ARG, SIND_E_CAPACITY, or 1: the factorisation failed
int sindh_essgraph_linear(const sind_essgraph_item* item, int fix_scale, double* H, double* b, double* x, double* lambda, long long* env) {
    if (!item || sind::ess_check(*item)) return SIND_E_ARG;
    sind::EssHost h;
    if (const int r = sind::ess_plan(*item, h.pl)) return r;
    sind::ess_host_bind(h, *item, fix_scale);
    sind::SeqExec ex; const sind::EssView& w = h.v; const int n = w.n;
    if (env) { env[0] = n; env[1] = (long long)h.pl.nEnv; }
    if (!H || !b || !x) return 0;
    sind::ess_init(ex, w);
    sind::EssLm<sind::SeqExec> lm{ex, w, 0};
    lm.linearize();
    const double lam = 1e-16; if (lambda) *lambda = lam;
    for (int i = 0; i < n; i++) { w.x[i] = 0.0; b[i] = w.Hd[(i / 7) * ESS_V + 28 + i % 7]; }
    for (size_t k = 0; k < (size_t)n * n; k++) H[k] = 0.0;
    for (int a = 0; a < w.nAct; a++) for (int r = 0; r < 7; r++) for (int c = r; c < 7; c++) { const double v = w.Hd[a * ESS_V + sind::ess_tri(r, c)]; H[(size_t)(7 * a + r) * n + 7 * a + c] = v; H[(size_t)(7 * a + c) * n + 7 * a + r] = v; }
    for (int p = 0; p < w.nPair; p++) for (int r = 0; r < 7; r++) for (int c = 0; c < 7; c++) {
        const double v = w.Ho[p * 49 + 7 * r + c]; const size_t i = 7 * (size_t)w.pairLo[p] + r, j = 7 * (size_t)w.pairHi[p] + c;
        H[i * n + j] = v; H[j * n + i] = v;
    }
    sind::ess_solve(ex, w, lam);
    std::memcpy(x, w.x, sizeof(double) * n);
    return w.isc[sind::ESS_IS_FAIL] ? 1 : 0;
}

}  // extern "C"
