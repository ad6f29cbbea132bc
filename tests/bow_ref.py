"""Plain Python restatement of the reference's vocabulary-guided matching (test infrastructure; nothing under sindslam_amd/ imports it):
  transform()                 TemplatedVocabulary::transform, feature-vector half (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194, :1218-1259),
                              FORB::distance = Hamming distance
  feature_vector()            FeatureVector::addFeature (Thirdparty/DBoW2/DBoW2/FeatureVector.cpp:31-45) from per-keypoint node ids
  search_by_bow()             ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (src/ORBmatcher.cc:159-288)
  search_for_triangulation()  ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823) with CheckDistEpipolarLine (:140-157)
Sequential loops in the reference's order: std::map iteration with its lower_bound skips, the index lists in push_back order, numpy.float32 / float64 scalars
where the reference rounds.  A tree is a dict: levels, child_start, child, desc, word_id, weight (include/sind_hip.h: sind_voc_tree)."""
import bisect

import numpy as np

from localmap_ref import three_maxima, to_camera

f32, f64 = np.float32, np.float64
TH_LOW, HISTO_LENGTH = 50, 30
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def transform_one(tree, feature, levelsup):
    """-> (word_id, weight, nid); nid is None where the reference leaves it uninitialised (:1218-1259)"""
    cs, ch, nd = tree["child_start"], tree["child"], tree["desc"]
    nid_level = tree["levels"] - levelsup
    nid = 0 if nid_level <= 0 else None
    final_id, current_level = 0, 0
    while True:                                                       # do { } while(!isLeaf())
        current_level += 1
        nodes = ch[cs[final_id]:cs[final_id + 1]]
        final_id = int(nodes[0])
        best_d = hamming(feature, nd[final_id])
        for i in nodes[1:]:
            d = hamming(feature, nd[i])
            if d < best_d:
                best_d, final_id = d, int(i)
        if current_level == nid_level:
            nid = final_id
        if cs[final_id] == cs[final_id + 1]:
            break
    return int(tree["word_id"][final_id]), float(tree["weight"][final_id]), nid, final_id


def transform(tree, desc, levelsup=4):
    """-> node_id, word_id per descriptor.  node_id = -1: the word is stopped and the feature is not added (:1157-1161); where the reference's nid
    is uninitialised (the path ended above the level), the leaf's id, as sind_voc_transform defines it."""
    node = np.full(len(desc), -1, np.int32); word = np.full(len(desc), -1, np.int32)
    for i, f in enumerate(desc):
        w, weight, nid, leaf = transform_one(tree, f, levelsup)
        word[i] = w
        if weight > 0:
            node[i] = leaf if nid is None else nid
    return node, word


def feature_vector(node):
    """std::map<NodeId, vector<unsigned>>: keys ascending, indices in feature order"""
    fv = {}
    for i, n in enumerate(node):
        if n >= 0:
            fv.setdefault(int(n), []).append(i)
    return fv


def _shared_nodes(fv1, fv2):
    """the while loop over two map iterators (:180-264, :691-789): yields the keys both maps hold, ascending"""
    k1, k2 = sorted(fv1), sorted(fv2)
    i = j = 0
    while i < len(k1) and j < len(k2):
        if k1[i] == k2[j]:
            yield k1[i]
            i += 1; j += 1
        elif k1[i] < k2[j]:
            i = bisect.bisect_left(k1, k2[j])                         # lower_bound
        else:
            j = bisect.bisect_left(k2, k1[i])


def rot_bin(a1, a2):
    rot = f32(f32(a1) - f32(a2))
    if rot < 0: rot = f32(rot + f32(360.0))
    b = int(np.floor(f64(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH)))) + 0.5))     # round(): halves away from zero, the product is never negative
    return 0 if b == HISTO_LENGTH else b


def search_by_bow(kf, cur, nnratio, check_orientation=True, sequential=True):
    """kf: node, valid, angle, desc; cur: node, angle, desc -> match_of_cur [n_cur] (index of the key-frame keypoint, -1), nmatches, choice [n_kf] (the frame
    keypoint every key-frame keypoint took, before the orientation check).  sequential=False searches every key-frame keypoint against the frame as it was
    on entry, ignoring the claims of :209 (the count of choices that then differ is how much of the sequential dependence a scene exercises; match_of_cur
    and nmatches mean nothing then)."""
    nnratio = f32(nnratio)
    n_cur = len(cur["node"])
    m = np.full(n_cur, -1, np.int32); nm = 0; rot_hist = [[] for _ in range(HISTO_LENGTH)]; choice = np.full(len(kf["node"]), -1, np.int32)
    fv_kf, fv_f = feature_vector(kf["node"]), feature_vector(cur["node"])
    for node in _shared_nodes(fv_kf, fv_f):
        for ikf in fv_kf[node]:
            if not kf["valid"][ikf]: continue
            best1, best_i, best2 = 256, -1, 256
            for i_f in fv_f[node]:
                if sequential and m[i_f] >= 0: continue
                d = hamming(kf["desc"][ikf], cur["desc"][i_f])
                if d < best1: best2, best1, best_i = best1, d, i_f
                elif d < best2: best2 = d
            if best1 <= TH_LOW:
                if f32(best1) < f32(nnratio * f32(best2)):
                    m[best_i] = ikf; choice[ikf] = best_i
                    if check_orientation:
                        rot_hist[rot_bin(kf["angle"][ikf], cur["angle"][best_i])].append(best_i)
                    nm += 1
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for i_f in rot_hist[b]:
                    m[i_f] = -1; nm -= 1
    return m, nm, choice


def epipole(cam, T2, Cw1):
    """(ex, ey): C2 = R2w * Cw + t2w, invz = 1.0f / C2z (:664-670)"""
    fx, fy, cx, cy = [f32(v) for v in cam[:4]]
    C2 = to_camera(np.asarray(T2, np.float32), np.asarray(Cw1, np.float32))
    invz = f32(f32(1.0) / C2[2])
    return f32(f32(f32(fx * C2[0]) * invz) + cx), f32(f32(f32(fy * C2[1]) * invz) + cy)


def epipolar_line(xy1, F12):
    """a, b, c and den of CheckDistEpipolarLine (:143-149)"""
    x, y = f32(xy1[0]), f32(xy1[1]); F = np.asarray(F12, np.float32)
    a, b, c = [f32(f32(f32(x * F[0, j]) + f32(y * F[1, j])) + F[2, j]) for j in range(3)]
    return a, b, c, f32(f32(a * a) + f32(b * b))


def check_dist_epipolar_line(line, xy2, sigma2):
    a, b, c, den = line
    num = f32(f32(f32(a * f32(xy2[0])) + f32(b * f32(xy2[1]))) + c)
    if den == 0: return False
    with np.errstate(all="ignore"):
        dsqr = f32(f32(num * num) / den)
    return bool(f64(dsqr) < 3.84 * f64(sigma2))


def tri_candidate_ok(k1, k2, i1, i2, line, epi, sc, only_stereo):
    """the tests of the inner loop on idx2 that do not depend on the running best (:722-751), for the property tests: the distance, or None if one fails"""
    if k2["has_mp"][i2]: return None
    stereo1, stereo2 = k1["u_right"][i1] >= 0, k2["u_right"][i2] >= 0
    if only_stereo and not stereo2: return None
    d = hamming(k1["desc"][i1], k2["desc"][i2])
    if d > TH_LOW: return None
    x2, y2 = k2["un_xy"][i2]; s = sc[k2["octave"][i2]]
    if not stereo1 and not stereo2:
        dx, dy = f32(epi[0] - x2), f32(epi[1] - y2)
        if f32(f32(dx * dx) + f32(dy * dy)) < f32(f32(100) * s): return None
    if not check_dist_epipolar_line(line, (x2, y2), f32(s * s)): return None
    return d


def search_for_triangulation(cam, sc, T2, Cw1, F12, k1, k2, only_stereo=False, check_orientation=True):
    """k1: node, has_mp, un_xy, angle, u_right, desc; k2: the same and octave -> match12 [n1], nmatches, matched_pairs [(idx1, idx2)]"""
    epi = epipole(cam, T2, Cw1)
    n1 = len(k1["node"])
    m12 = np.full(n1, -1, np.int32); nm = 0; rot_hist = [[] for _ in range(HISTO_LENGTH)]
    fv1, fv2 = feature_vector(k1["node"]), feature_vector(k2["node"])
    for node in _shared_nodes(fv1, fv2):
        for i1 in fv1[node]:
            if k1["has_mp"][i1]: continue
            if only_stereo and not k1["u_right"][i1] >= 0: continue
            line = epipolar_line(k1["un_xy"][i1], F12)
            best_dist, best_i2 = TH_LOW, -1
            stereo1 = k1["u_right"][i1] >= 0
            for i2 in fv2[node]:
                if k2["has_mp"][i2]: continue                         # vbMatched2 is never set in the reference
                stereo2 = k2["u_right"][i2] >= 0
                if only_stereo and not stereo2: continue
                d = hamming(k1["desc"][i1], k2["desc"][i2])
                if d > TH_LOW or d > best_dist: continue
                x2, y2 = k2["un_xy"][i2]; s = sc[k2["octave"][i2]]
                if not stereo1 and not stereo2:
                    dx, dy = f32(epi[0] - x2), f32(epi[1] - y2)
                    if f32(f32(dx * dx) + f32(dy * dy)) < f32(f32(100) * s): continue
                if check_dist_epipolar_line(line, (x2, y2), f32(s * s)):
                    best_i2, best_dist = i2, d
            if best_i2 >= 0:
                m12[i1] = best_i2; nm += 1
                if check_orientation:
                    rot_hist[rot_bin(k1["angle"][i1], k2["angle"][best_i2])].append(i1)
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for i1 in rot_hist[b]:
                    m12[i1] = -1; nm -= 1
    pairs = [(i, int(m12[i])) for i in range(n1) if m12[i] >= 0]
    return m12, nm, pairs
