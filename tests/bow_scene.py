"""Test scenes for the vocabulary-guided searches (vocabulary transform, SearchByBoW, SearchForTriangulation), built on match_scene (ORACLE extractor / Frame
steps).  A tree is a dict as bow_ref reads it; a key frame / frame is a dict of per-keypoint arrays (see sindslam_amd/matcher.py)."""
import numpy as np

import bow_ref as W
import match_scene as S
import oracle_lib as O

f32 = np.float32


def bits(k):
    """32-byte descriptor with the first k bits set: hamming(bits(a), bits(b)) = |a - b|"""
    return np.packbits(np.arange(256) < k)


def _csr(children, n):
    start = np.zeros(n + 1, np.int32); flat = []
    for i in range(n):
        flat += children.get(i, []); start[i + 1] = len(flat)
    return start, np.array(flat, np.int32)


def tiny_tree():
    """k = 3, 3 levels, 12 nodes.  Leaves at depth 1 (node 2), 2 (5, 6, 7, 8) and 3 (9, 10, 11); nodes 7 and 8 have identical descriptors; the word of
    node 10 is stopped.  Node descriptors are bits(position), so a feature bits(f) descends by |f - position|:
        0 -> 1 (40) -> 4 (20) -> 9 (10), 10 (20, stopped), 11 (30)
                    -> 5 (40), 6 (60)
          -> 2 (120)
          -> 3 (200) -> 7 (200), 8 (200)"""
    children = {0: [1, 2, 3], 1: [4, 5, 6], 3: [7, 8], 4: [9, 10, 11]}
    pos = {1: 40, 2: 120, 3: 200, 4: 20, 5: 40, 6: 60, 7: 200, 8: 200, 9: 10, 10: 20, 11: 30}
    n = 12
    start, child = _csr(children, n)
    desc = np.zeros((n, 32), np.uint8)
    for i, p in pos.items(): desc[i] = bits(p)
    word = np.full(n, -1, np.int32); leaves = [i for i in range(n) if i not in children]
    word[leaves] = np.arange(len(leaves))                             # words in node order: 2, 5, 6, 7, 8, 9, 10, 11 -> 0 .. 7
    weight = np.where(word >= 0, 1.0, 0.0); weight[10] = 0.0
    return dict(levels=3, child_start=start, child=child, desc=desc, word_id=word, weight=weight)


# feature position -> (word, node id at levelsup 0, 1, 2, >= 3), worked out by hand from tiny_tree's drawing:
#   12: 1, 4, 9.  21: 1, 4, 10 (stopped).  45: 1, 5 (ends at depth 2).  50: 1, then 5 and 6 both at 10 -> the first.  80: 1 and 2 both at 40 -> the first, 6.
#   130: the depth-1 leaf 2.  230: 3, then 7 and 8 identical -> the first.
TINY_EXPECT = {12: (5, 9, 4, 1, 0), 21: (6, -1, -1, -1, -1), 45: (1, 5, 5, 1, 0), 50: (1, 5, 5, 1, 0), 80: (2, 6, 6, 1, 0), 130: (0, 2, 2, 2, 0), 230: (3, 7, 7, 3, 0)}


def random_vocabulary(pool, k=10, levels=3, seed=0, flips=6, stopped=0.03):
    """Full k-ary tree of the given depth in breadth-first node order; node descriptors are rows of `pool` with `flips` random bits flipped;
    a share `stopped` of the words has weight 0.  k = 10, levels = 3: 100 nodes at level 2 (levelsup = 1), 1000 words."""
    rng = np.random.default_rng(seed)
    n = sum(k ** l for l in range(levels + 1)); first_leaf = n - k ** levels
    children = {i: list(range(i * k + 1, i * k + k + 1)) for i in range(first_leaf)}
    start, child = _csr(children, n)
    desc = pool[rng.integers(0, len(pool), n)].copy()
    for i in range(n):
        for b in rng.integers(0, 256, flips): desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    word = np.full(n, -1, np.int32); word[first_leaf:] = np.arange(n - first_leaf)
    weight = np.where(word >= 0, rng.uniform(0.5, 8.0, n), 0.0); weight[first_leaf:][rng.random(n - first_leaf) < stopped] = 0.0
    return dict(levels=levels, child_start=start, child=child, desc=desc, word_id=word, weight=weight)


_frames = {}


def stream_frame(stream, t):
    """frame t of the synthetic stream through the oracle's extractor and Frame steps: per-keypoint dict + Tcw (ground truth) + cam10; cached"""
    if t not in _frames:
        bgr, depth = stream.frames(t, 1)
        cal = [stream.fx, stream.fy, stream.cx, stream.cy, 0, 0, 0, 0, 0, 40.0, 1.0 / stream.depth_factor]
        kp, desc = O.ORBextractor(1500, 1.2, 8, 15, 5).extract(O.bgr2gray(bgr[0]))
        post = O.frame_post_orb(cal, kp["x"], kp["y"], depth[0])
        cam10 = np.array([cal[0], cal[1], cal[2], cal[3], 40.0, np.float32(40.0) / np.float32(cal[0]), *post["bounds"]], np.float32)
        _frames[t] = dict(un_xy=post["keys_un"], octave=kp["octave"].copy(), angle=kp["angle"].copy(), u_right=post["u_right"], desc=desc, depth=post["depth"],
                          Tcw=S._tcw(stream, t), cam=cam10)
    return _frames[t]


_vocs = {}


def stream_vocabulary(stream):
    """about 100 nodes at level 2, drawn from the descriptors of frames 3 and 4"""
    if "v" not in _vocs:
        _vocs["v"] = random_vocabulary(np.concatenate([stream_frame(stream, 3)["desc"], stream_frame(stream, 4)["desc"]]), seed=11)
    return _vocs["v"]


LEVELSUP = 1                                                          # with the 3-level stream vocabulary: the 100 nodes of level 2

_nodes = {}


def stream_nodes(stream, t):
    if t not in _nodes:
        _nodes[t] = W.transform(stream_vocabulary(stream), stream_frame(stream, t)["desc"], LEVELSUP)[0]
    return _nodes[t]


def bow_pair(stream, t_kf, t_cur, seed=0, drop=0.15):
    """(kf, cur): frame t_kf as the key frame (a share `drop` of its keypoints without a good map point), frame t_cur as the frame"""
    rng = np.random.default_rng(3000 + seed)
    a, b = stream_frame(stream, t_kf), stream_frame(stream, t_cur)
    kf = dict(node=stream_nodes(stream, t_kf), valid=((a["depth"] > 0) & (rng.random(len(a["octave"])) > drop)).astype(np.uint8), angle=a["angle"], desc=a["desc"])
    cur = dict(node=stream_nodes(stream, t_cur), angle=b["angle"], desc=b["desc"])
    return kf, cur


def _flip_bytes(rng, d, rate):
    return d ^ ((rng.random(d.shape) < rate) * rng.integers(1, 255, d.shape)).astype(np.uint8)


# node -> (key-frame keypoints, frame keypoints) of the stress scene: 1, 63, 64, 65 and ~200 on each side independently, nodes on one side only
STRESS_SIZES = {10: (1, 64), 11: (63, 65), 12: (64, 1), 13: (65, 200), 14: (200, 63), 15: (64, 64), 16: (1, 1), 17: (65, 63), 18: (210, 190), 19: (63, 200),
                20: (30, 0), 21: (0, 30), 22: (5, 0), 40: (150, 130), 41: (0, 7), 5000: (90, 110)}
STRESS_CLAIMED_NODE = 30                                              # 3 frame keypoints, 40 key-frame keypoints that want them


def bow_stress_pair(seed, n_codes=12, rate=0.08):
    """A dozen distinct descriptor codes with a few flipped bytes (equal distances, contended keypoints, as match_scene.stress_pair), node ids assigned
    directly with the sizes of STRESS_SIZES, keypoint indices shuffled; node STRESS_CLAIMED_NODE: three far-apart frame descriptors and forty key-frame
    descriptors near one of them each, so all three get claimed and the later entries find them closed; 5 % of the keypoints with node -1."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n_codes, 32)).astype(np.uint8)
    sides = []
    far = rng.integers(0, 256, (3, 32)).astype(np.uint8)
    for side in range(2):
        node = np.concatenate([np.full(sz[side], nd) for nd, sz in STRESS_SIZES.items()])
        desc = _flip_bytes(rng, codes[rng.integers(0, n_codes, len(node))], rate)
        if side == 0:
            extra = _flip_bytes(rng, far[rng.integers(0, 3, 40)], 0.03)
        else:
            extra = far.copy()
        node = np.concatenate([node, np.full(len(extra), STRESS_CLAIMED_NODE)]); desc = np.concatenate([desc, extra])
        lost = int(0.05 * len(node))
        node = np.concatenate([node, np.full(lost, -1)]); desc = np.concatenate([desc, _flip_bytes(rng, codes[rng.integers(0, n_codes, lost)], rate)])
        order = rng.permutation(len(node))
        sides.append(dict(node=node[order].astype(np.int32), desc=desc[order], angle=(rng.choice([10.0, 100.0, 200.0, 300.0], len(node)) + rng.uniform(-8, 8, len(node))).astype(np.float32)))
    kf, cur = sides
    kf["valid"] = (rng.random(len(kf["node"])) > 0.1).astype(np.uint8)
    kf["valid"][kf["node"] == STRESS_CLAIMED_NODE] = 1
    return kf, cur


def fundamental(T1, T2, K):
    """F12 as LocalMapping::ComputeF12 builds it (src/LocalMapping.cc): K^-T [t12]x R12 K^-1, in FP64, rounded to FP32; an input to both sides"""
    T1, T2, K = [np.asarray(a, np.float64) for a in (T1, T2, K)]
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    R12 = R1 @ R2.T; t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Ki = np.linalg.inv(K)
    return (Ki.T @ tx @ R12 @ Ki).astype(np.float32)


def _centre(T):
    T = np.asarray(T, np.float64)
    return (-T[:3, :3].T @ T[:3, 3]).astype(np.float32)


def tri_stream_pair(stream, t1, t2, seed=0, mono=0.3, mapped=0.3):
    """(cam10, scale, Tcw2, Cw1, F12, kf1, kf2): frames t1 and t2 of the stream as two key frames, F12 from the ground-truth poses; a share `mono` of the
    keypoints with depth loses it (u_right = -1), a share `mapped` of the keypoints already has a map point"""
    rng = np.random.default_rng(4000 + seed)
    out = []
    for t in (t1, t2):
        f = stream_frame(stream, t); n = len(f["octave"])
        ur = f["u_right"].copy(); ur[rng.random(n) < mono] = -1
        out.append(dict(node=stream_nodes(stream, t), has_mp=(rng.random(n) < mapped).astype(np.uint8), un_xy=f["un_xy"], octave=f["octave"], angle=f["angle"], u_right=ur, desc=f["desc"]))
    a, b = stream_frame(stream, t1), stream_frame(stream, t2)
    cam = a["cam"]; K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float64)
    return cam, S._scale_factors(), b["Tcw"], _centre(a["Tcw"]), fundamental(a["Tcw"], b["Tcw"], K), out[0], out[1]


def tri_special_pair(seed=0, n=240):
    """Synthetic points seen by two cameras (camera 1 at the origin, camera 2 ahead and slightly turned, so the epipole lies in the image); exact projections,
    descriptors equal up to a few bits, eight nodes.
      - duplicates: the first 20 keypoints of camera 2 appear three times (same position, same descriptor, larger indices): the last one must win
      - epipole: keypoint 20 of both cameras is mono, carries one descriptor, and camera 2's copy sits on the epipole; keypoint 21 of camera 1 is its stereo twin
      - den == 0: keypoint 22 of camera 1 sits on camera 1's epipole (x0, y0), and F12(2,0), F12(2,1) are set to minus the FP32 sums x0 * F12(0,j) + y0 * F12(1,j)
        (a change in their last bits: the exact F12 satisfies this but for rounding), so a = b = 0 there although its partner has the same descriptor
    -> (cam10, scale, Tcw2, Cw1, F12, kf1, kf2)"""
    rng = np.random.default_rng(5000 + seed)
    fx, fy, cx, cy = 535.4, 539.2, 320.1, 247.6
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    ang = np.deg2rad(1.5); R2 = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    T1 = np.eye(4); T2 = np.eye(4); T2[:3, :3] = R2; T2[:3, 3] = (0.05, 0.02, -0.4)
    z = rng.uniform(2.0, 6.0, n); u = rng.uniform(40, 600, n); v = rng.uniform(40, 440, n)
    X = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    X2 = X @ R2.T + T2[:3, 3]
    xy1 = np.stack([u, v], 1).astype(np.float32); xy2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1).astype(np.float32)
    d1 = rng.integers(0, 256, (n, 32)).astype(np.uint8); d2 = _flip_bytes(rng, d1, 0.04)
    node = rng.integers(100, 108, n).astype(np.int32)
    sc = S._scale_factors()
    cam = np.array([fx, fy, cx, cy, 40.0, f32(40.0) / f32(fx), 0, 640, 0, 480], np.float32)
    T2f = T2.astype(np.float32); Cw1 = np.zeros(3, np.float32)
    F12 = fundamental(T1, T2, K)
    mk = lambda xy, d, nd: dict(node=nd.copy(), has_mp=(rng.random(len(nd)) < 0.1).astype(np.uint8), un_xy=xy.copy(), octave=rng.integers(0, 8, len(nd)).astype(np.int32),
                                angle=rng.uniform(0, 360, len(nd)).astype(np.float32), u_right=np.where(rng.random(len(nd)) < 0.4, -1.0, 100.0).astype(np.float32), desc=d.copy())
    k1, k2 = mk(xy1, d1, node), mk(xy2, d2, node)
    k2["angle"] = ((k1["angle"] + rng.choice([0.0, 0.0, 0.0, 90.0], n) + rng.uniform(-4, 4, n)) % 360).astype(np.float32)
    k1["has_mp"][:23] = 0; k2["has_mp"][:23] = 0
    # epipole
    k2["un_xy"][20] = W.epipole(cam, T2f, Cw1); k1["un_xy"][20] = (cx, cy); k1["u_right"][20] = -1; k2["u_right"][20] = -1
    k1["desc"][20] = k2["desc"][20]; k1["desc"][21] = k2["desc"][20]; k1["node"][21] = node[20]; k1["u_right"][21] = 100.0; k1["un_xy"][21] = (cx, cy)
    C2w = -R2.T @ T2[:3, 3]
    x0, y0 = f32(fx * C2w[0] / C2w[2] + cx), f32(fy * C2w[1] / C2w[2] + cy)
    for j in range(2): F12[2, j] = -f32(f32(x0 * F12[0, j]) + f32(y0 * F12[1, j]))
    k1["un_xy"][22] = (x0, y0); k1["desc"][22] = k2["desc"][22]
    # duplicates of camera 2's first 20 keypoints, twice
    k2 = {key: np.concatenate([val, val[:20], val[:20]]) for key, val in k2.items()}
    return cam, sc, T2f, Cw1, F12, k1, k2
