// What the host layers of local BA (local_ba.cpp) and global BA (global_ba.cpp) share (ba_schur.hpp): the checks both report, the digest of an item into the lists the
// phases walk (the per-pose edge lists, the per-point edges by pose rank, the co-observation lists), the sizes, the fill of Fin, the view up to the reduced system and
// the copy of the two float outputs.  Compiled into libsind_hip.so and into libsind_host.so.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include "ba_schur.hpp"

namespace sind {

int ba_check_arrays(const BaItem& q, bool kfNull, bool mpNull, bool obsNull) {
    if (q.nKf < 0 || q.nMp < 0) return 1;
    if (q.nKf && (!q.kfId || !q.Tcw || !q.TcwOut || kfNull)) return 2;
    if (q.nMp && (!q.mpId || !q.x3Dw || !q.obsStart || !q.x3DwOut || mpNull)) return 2;
    if (q.nMp) { if (q.obsStart[0] != 0) return 6; for (int j = 0; j < q.nMp; j++) if (q.obsStart[j + 1] < q.obsStart[j]) return 6; }
    if (q.nObs && (!q.obsKf || !q.obsXy || !q.uRight || !q.invSigma2 || obsNull)) return 2;
    return 0;
}

bool ba_ids_repeat(const int64_t* id, int n) {
    std::vector<int64_t> v(id, id + n); std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) != v.end();
}

int ba_check_obs(const BaItem& q) {
    std::vector<int> seen((size_t)q.nKf, -1);
    for (int j = 0; j < q.nMp; j++) for (int e = q.obsStart[j]; e < q.obsStart[j + 1]; e++) {
        const int k = q.obsKf[e];
        if (k < 0 || k >= q.nKf) return 4;
        if (seen[k] == j) return 5;
        seen[k] = j;
    }
    for (int e = 0; e < q.nObs; e++) if (!(q.invSigma2[e] >= 0 && std::isfinite(q.invSigma2[e]))) return 7;
    for (size_t k = 0; k < (size_t)16 * q.nKf; k++) if (!std::isfinite(q.Tcw[k])) return 8;
    for (size_t k = 0; k < (size_t)3 * q.nMp; k++) if (!std::isfinite(q.x3Dw[k])) return 8;
    return 0;
}

size_t ba_count(const BaItem& q, const std::vector<int>& kfPose, int P, std::vector<int>& ptNF, std::vector<int>& nEdge) {
    ptNF.assign((size_t)q.nMp, 0); nEdge.assign((size_t)P, 0);
    size_t total = 0;
    for (int j = 0; j < q.nMp; j++) {
        size_t k = 0;
        for (int e = q.obsStart[j]; e < q.obsStart[j + 1]; e++) { const int s = kfPose[q.obsKf[e]]; if (s >= 0) { k++; nEdge[s]++; } }
        ptNF[j] = (int)k; total += k * (k + 1) / 2;
    }
    return total;
}

void ba_lists(const BaItem& q, const std::vector<int>& kfPose, const std::vector<int>& free_, const std::vector<int>& ptNF, const std::vector<int>& nEdge, size_t total, BaPlan& pl) {
    const int nKf = q.nKf, nMp = q.nMp, nObs = q.nObs, P = (int)free_.size();
    std::vector<int> ptOrder((size_t)nMp); std::iota(ptOrder.begin(), ptOrder.end(), 0);
    std::sort(ptOrder.begin(), ptOrder.end(), [&](int a, int b) { return q.mpId[a] < q.mpId[b]; });
    std::vector<int> ePt((size_t)nObs), ptSorted((size_t)nObs, 0), poseEdgeStart((size_t)P + 1, 0);
    auto rankOf = [&](int e) { return kfPose[q.obsKf[e]]; };
    for (int j = 0; j < nMp; j++) {
        int* srt = ptSorted.data() + q.obsStart[j]; int c = 0;
        for (int e = q.obsStart[j]; e < q.obsStart[j + 1]; e++) { ePt[e] = j; if (rankOf(e) >= 0) srt[c++] = e; }
        std::sort(srt, srt + c, [&](int a, int b) { return rankOf(a) < rankOf(b); });
    }
    for (int s = 0; s < P; s++) poseEdgeStart[s + 1] = poseEdgeStart[s] + nEdge[s];
    std::vector<int> poseEdge((size_t)poseEdgeStart[P]), fill(poseEdgeStart.begin(), poseEdgeStart.end() - 1);
    for (int e = 0; e < nObs; e++) { const int s = rankOf(e); if (s >= 0) poseEdge[fill[s]++] = e; }
    // the co-observation lists: per pair of free poses s1 <= s2 in ascending (s1, s2), the points both see in ascending mp_id
    struct Ent { int s1, s2, e1, e2; };
    std::vector<Ent> ent, tmp(total); ent.reserve(total);
    for (int o = 0; o < nMp; o++) {
        const int j = ptOrder[o]; const int* srt = ptSorted.data() + q.obsStart[j];
        for (int a = 0; a < ptNF[j]; a++) for (int b = a; b < ptNF[j]; b++) ent.push_back({rankOf(srt[a]), rankOf(srt[b]), srt[a], srt[b]});
    }
    std::vector<size_t> at((size_t)P + 1);
    for (int pass = 0; pass < 2; pass++) {                             // stable, by s2 from ent into tmp, then by s1 from tmp back into ent
        const std::vector<Ent>& from = pass ? tmp : ent; std::vector<Ent>& to = pass ? ent : tmp;
        std::fill(at.begin(), at.end(), (size_t)0);
        for (const Ent& t : from) at[(pass ? t.s1 : t.s2) + 1]++;
        for (int s = 0; s < P; s++) at[s + 1] += at[s];
        for (const Ent& t : from) to[at[pass ? t.s1 : t.s2]++] = t;
    }
    std::vector<Ent>().swap(tmp);
    std::vector<int> pairStart, pairS1, pairS2, pairE(2 * total), diagPair((size_t)P, -1);
    for (size_t t = 0; t < total; t++) {
        if (t == 0 || ent[t].s1 != ent[t - 1].s1 || ent[t].s2 != ent[t - 1].s2) {
            if (ent[t].s1 == ent[t].s2) diagPair[ent[t].s1] = (int)pairS1.size();
            pairStart.push_back((int)t); pairS1.push_back(ent[t].s1); pairS2.push_back(ent[t].s2);
        }
        pairE[2 * t] = ent[t].e1; pairE[2 * t + 1] = ent[t].e2;
    }
    pairStart.push_back((int)total);
    std::vector<Ent>().swap(ent);

    pl.nKf = nKf; pl.nMp = nMp; pl.nObs = nObs; pl.P = P; pl.nPair = (int)pairS1.size();
    pl.I.clear();
    pl.oKfPose = pl.add(kfPose); pl.oPoseKf = pl.add(free_); pl.oPtOrder = pl.add(ptOrder);
    pl.oObsStart = nMp ? pl.add(q.obsStart, (size_t)nMp + 1) : pl.room(1);
    pl.oEPt = pl.add(ePt); pl.oEKf = pl.add(q.obsKf, nObs);
    pl.oPoseEdgeStart = pl.add(poseEdgeStart); pl.oPoseEdge = pl.add(poseEdge); pl.oPtNF = pl.add(ptNF); pl.oPtSorted = pl.add(ptSorted);
    pl.oPairStart = pl.add(pairStart); pl.oPairS1 = pl.add(pairS1); pl.oPairS2 = pl.add(pairS2); pl.oPairE = pl.add(pairE); pl.oDiagPair = pl.add(diagPair);
}

void ba_sizes(BaPlan& pl) {
    const size_t nKf = pl.nKf, nMp = pl.nMp, nObs = pl.nObs, P = pl.P, nx = 6 * P + 3 * nMp;
    pl.z = ItemSizes{};
    pl.z.ints = pl.I.size();
    pl.z.floatsIn = 16 * nKf + 3 * nMp + 4 * nObs; pl.z.floatsOut = 16 * nKf + 3 * nMp;
    pl.z.work = BA_SC_N + 14 * nKf + 6 * nMp + (size_t)(LBA_C + 18) * nObs + 27 * P + 21 * nMp + 2 * nx + nObs;
}

void ba_fill(const BaItem& q, const ItemPtrs& p) {
    float* F = p.Fin;
    if (q.nKf) std::memcpy(F, q.Tcw, sizeof(float) * 16 * q.nKf);
    F += 16 * (size_t)q.nKf;
    if (q.nMp) std::memcpy(F, q.x3Dw, sizeof(float) * 3 * q.nMp);
    F += 3 * (size_t)q.nMp;
    for (size_t e = 0; e < (size_t)q.nObs; e++) { F[4 * e] = q.obsXy[2 * e]; F[4 * e + 1] = q.obsXy[2 * e + 1]; F[4 * e + 2] = q.uRight[e]; F[4 * e + 3] = q.invSigma2[e]; }
}

double* ba_bind(const BaPlan& pl, const PoseOptCam& K, const ItemPtrs& p, double* d, BaView& v) {
    int* I = p.I; const float* Fin = p.Fin; float* Fout = p.Fout;
    const size_t nKf = pl.nKf, nMp = pl.nMp, nObs = pl.nObs, P = pl.P;
    v.nKf = pl.nKf; v.nMp = pl.nMp; v.nObs = pl.nObs; v.P = pl.P; v.nPair = pl.nPair; v.K = K;
    v.Tcw = Fin; v.x3Dw = Fin + 16 * nKf; v.eObs = v.x3Dw + 3 * nMp;
    v.kfPose = I + pl.oKfPose; v.poseKf = I + pl.oPoseKf; v.ptOrder = I + pl.oPtOrder; v.obsStart = I + pl.oObsStart; v.ePt = I + pl.oEPt; v.eKf = I + pl.oEKf;
    v.poseEdgeStart = I + pl.oPoseEdgeStart; v.poseEdge = I + pl.oPoseEdge; v.ptNF = I + pl.oPtNF; v.ptSorted = I + pl.oPtSorted;
    v.pairStart = I + pl.oPairStart; v.pairS1 = I + pl.oPairS1; v.pairS2 = I + pl.oPairS2; v.pairE = I + pl.oPairE; v.diagPair = I + pl.oDiagPair;
    v.poseIdx = I + pl.oPoseIdx; v.ptAct = I + pl.oPtAct;
    static_assert(sizeof(PoseQ) == 7 * sizeof(double), "the layout of the working state");
    v.sc = d; d += BA_SC_N; v.est = (PoseQ*)d; d += 7 * nKf; v.bak = (PoseQ*)d; d += 7 * nKf; v.X = d; d += 3 * nMp; v.Xbak = d; d += 3 * nMp;
    v.C = d; d += LBA_C * nObs; v.BD = d; d += 18 * nObs; v.Hpp = d; d += 27 * P; v.Hll = d; d += 9 * nMp; v.Dinv = d; d += 9 * nMp; v.db = d; d += 3 * nMp;
    v.TcwOut = Fout; v.XOut = Fout + 16 * nKf;
    return d;
}

void ba_store(const BaItem& q, const BaPlan& pl, const ItemPtrs& p) {
    if (pl.nKf) std::memcpy(q.TcwOut, p.Fout, sizeof(float) * 16 * pl.nKf);
    if (pl.nMp) std::memcpy(q.x3DwOut, p.Fout + 16 * (size_t)pl.nKf, sizeof(float) * 3 * pl.nMp);
}

}  // namespace sind
