"""Plain Python restatement of the loop-closing front end of the reference (test infrastructure; nothing under sindslam_amd/ imports it):
  bow_vector()        the BowVector half of TemplatedVocabulary::transform(features, v, fv, levelsup) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194)
                      with BowVector::addWeight (BowVector.cpp:34-46) and BowVector::normalize (:62-84), TF_IDF weighting and L1 norm
  l1_score()          L1Scoring::score (ScoringObject.cpp:23-68)
  query()             what sind_bowdb_query defines per slot: common words, smallest common word, (float)score
  search_by_bow_kf()  ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (src/ORBmatcher.cc:522-655)
  KeyFrame, KeyFrameDatabase   a toy object graph with real per-word inverted lists and the mn*Query / mn*Words / m*Score members, carrying
                      KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:40-309) line by line
Sequential loops in the reference's order, numpy.float64 / float32 scalars where the reference rounds.  The reference itself cannot be built for the tests
(DBoW2 needs OpenCV), so the GPU tests compare against this restatement, as for every matcher call."""
import bisect

import numpy as np

from bow_ref import HISTO_LENGTH, TH_LOW, _shared_nodes, feature_vector, hamming, rot_bin, transform_one
from localmap_ref import three_maxima

f32, f64 = np.float32, np.float64


def bow_vector_of(word_ids, weights):
    """word and weight per feature, in feature order -> (words i32 ascending, values f64): the std::map after transform and normalize.  Every step is one
    explicit FP64 operation."""
    v = {}
    for word, weight in zip(word_ids, weights):                       # :1148-1162
        word, w = int(word), f64(weight)
        if w > 0:                                                     # not stopped
            if word in v: v[word] = f64(v[word] + w)                  # addWeight: vit->second += v
            else: v[word] = w
    words = sorted(v)
    norm = f64(0.0)
    for k in words: norm = f64(norm + np.fabs(v[k]))                  # :69-70
    if norm > 0.0:
        for k in words: v[k] = f64(v[k] / norm)                       # :81-82
    return np.array(words, np.int32), np.array([v[k] for k in words], np.float64)


def bow_vector(tree, desc, levelsup=4):
    """the descent of every descriptor (bow_ref.transform_one; the word does not depend on levelsup), then bow_vector_of"""
    t = [transform_one(tree, f, levelsup) for f in desc]
    return bow_vector_of([x[0] for x in t], [x[1] for x in t])


def l1_score(v1, v2):
    """v1, v2: (words, values) -> the double L1Scoring::score returns, and the words both hold"""
    w1, x1 = v1; w2, x2 = v2
    i = j = 0; score = f64(0.0); common = []
    while i < len(w1) and j < len(w2):
        if w1[i] == w2[j]:
            vi, wi = f64(x1[i]), f64(x2[j])
            score = f64(score + f64(f64(np.fabs(f64(vi - wi)) - np.fabs(vi)) - np.fabs(wi)))
            common.append(int(w1[i])); i += 1; j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j], i)                       # lower_bound
        else:
            j = bisect.bisect_left(w2, w1[i], j)
    return f64(f64(-score) / f64(2.0)), common


def query(q, slots):
    """slots: list of BowVectors or None (dead) -> common i32, first_word i32, score f32 per slot as sind_bowdb_query defines them"""
    n = len(slots)
    common = np.zeros(n, np.int32); first = np.full(n, -1, np.int32); score = np.zeros(n, np.float32)
    for s, v in enumerate(slots):
        if v is None: continue
        sc, cw = l1_score(q, v)
        common[s] = len(cw); first[s] = cw[0] if cw else -1; score[s] = f32(sc)
    return common, first, score


def search_by_bow_kf(k1, k2, nnratio, check_orientation=True, sequential=True, strict=True):
    """k1, k2: node, valid, angle, desc -> match12 [n1] (idx2 or -1), nmatches, choice [n1] (before the orientation check).  sequential=False ignores
    vbMatched2 (how much of the sequential dependence a scene exercises); strict=False replaces 'bestDist1 < TH_LOW' by '<=' (what a scene's pin of :598 is worth)."""
    nnratio = f32(nnratio)
    n1 = len(k1["node"])
    m12 = np.full(n1, -1, np.int32); matched2 = np.zeros(len(k2["node"]), bool); nm = 0; rot_hist = [[] for _ in range(HISTO_LENGTH)]
    fv1, fv2 = feature_vector(k1["node"]), feature_vector(k2["node"])
    for node in _shared_nodes(fv1, fv2):
        for idx1 in fv1[node]:
            if not k1["valid"][idx1]: continue                         # !pMP1 || isBad
            best1, best_i, best2 = 256, -1, 256
            for idx2 in fv2[node]:
                if (sequential and matched2[idx2]) or not k2["valid"][idx2]: continue
                d = hamming(k1["desc"][idx1], k2["desc"][idx2])
                if d < best1: best2, best1, best_i = best1, d, idx2
                elif d < best2: best2 = d
            if best1 < TH_LOW if strict else best1 <= TH_LOW:          # :598
                if f32(best1) < f32(nnratio * f32(best2)):
                    m12[idx1] = best_i; matched2[best_i] = True
                    if check_orientation:
                        rot_hist[rot_bin(k1["angle"][idx1], k2["angle"][best_i])].append(idx1)
                    nm += 1
    choice = m12.copy()
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for idx1 in rot_hist[b]:
                    m12[idx1] = -1; nm -= 1
    return m12, nm, choice


class KeyFrame:
    """what KeyFrameDatabase reads of a KeyFrame (and of a Frame: mnId and mBowVec).  mRelocScore starts at 0.0f: the reference leaves it uninitialised
    (src/KeyFrame.cc:35), sind_hip.h defines it.  mnLoopQuery / mnRelocQuery start at -1 so that a query id of 0 is an id like any other."""

    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = bow                                            # (words ascending, values)
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = -1, 0, f32(0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = -1, 0, f32(0)
        self.connected = set()                                        # GetConnectedKeyFrames()
        self.best_covisibles = []                                     # GetBestCovisibilityKeyFrames(10)


class KeyFrameDatabase:
    def __init__(self):
        self.mvInvertedFile = {}                                      # word -> list of KeyFrame, push_back order

    def add(self, pKF):                                               # :40-46
        for w in pKF.mBowVec[0]: self.mvInvertedFile.setdefault(int(w), []).append(pKF)

    def erase(self, pKF):                                             # :48-67
        for w in pKF.mBowVec[0]:
            lKFs = self.mvInvertedFile.get(int(w), [])
            for i, k in enumerate(lKFs):
                if k is pKF:
                    del lKFs[i]; break

    def clear(self):                                                  # :69-73
        self.mvInvertedFile = {}

    def sharing_loop(self, pKF):
        """:78-105 -> lKFsSharingWords"""
        l = []
        for w in pKF.mBowVec[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi not in pKF.connected:
                        pKFi.mnLoopQuery = pKF.mnId
                        l.append(pKFi)
                pKFi.mnLoopWords += 1
        return l

    def DetectLoopCandidates(self, pKF, minScore):                    # :76-197
        minScore = f32(minScore)
        lKFsSharingWords = self.sharing_loop(pKF)
        if not lKFsSharingWords: return []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords: maxCommonWords = k.mnLoopWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = f32(l1_score(pKF.mBowVec, pKFi.mBowVec)[0])
                pKFi.mLoopScore = si
                if si >= minScore: lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch: return []
        lAccScoreAndMatch = []; bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in pKFi.best_covisibles:
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = f32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore: pBestKF, bestScore = pKF2, pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore: bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)

    def sharing_reloc(self, F):
        """:201-223 -> lKFsSharingWords"""
        l = []
        for w in F.mBowVec[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    l.append(pKFi)
                pKFi.mnRelocWords += 1
        return l

    def DetectRelocalizationCandidates(self, F):                      # :199-309
        lKFsSharingWords = self.sharing_reloc(F)
        if not lKFsSharingWords: return []
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords: maxCommonWords = k.mnRelocWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = f32(l1_score(F.mBowVec, pKFi.mBowVec)[0])
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch: return []
        lAccScoreAndMatch = []; bestAccScore = f32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore, accScore, pBestKF = si, si, pKFi
            for pKF2 in pKFi.best_covisibles:
                if pKF2.mnRelocQuery != F.mnId: continue
                accScore = f32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore: pBestKF, bestScore = pKF2, pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore: bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)

    @staticmethod
    def _retain(lAccScoreAndMatch, bestAccScore):                     # :175-196, :289-308
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF, out = set(), []
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain and pKFi not in spAlreadyAddedKF:
                out.append(pKFi); spAlreadyAddedKF.add(pKFi)
        return out
