"""Small deterministic streams whose large-motion flags (the reference's second DeepFlow pass, DD:1081-1131) are known from the ORACLE alone, and the
oracle's results on them -- computed once per process and shared by test_motion_scene_cpu.py, test_large_motion_cpu.py and test_pipeline_motion_gpu.py.

A pan stream (dx, dy) is a window of w x h pixels of ONE 640 x 480 frame (SyntheticStream(seed=5).frame(3)), starting at (40, 40) and moving by (dx, dy)
pixels per frame, the depth cropped alike: a static scene under a translating camera.  The detector finds nothing dynamic there and its outputs do not depend
on the flow at all, so a pan stream pins the FLAG only; (dx, dy, "block") pastes a block with a motion of its own, and on those streams imgDyna changes with
the flow path taken (test_motion_scene_cpu.py asserts it).  ("walkers", k) is SyntheticStream(320, 240, seed=777, motion_scale=6.0) from frame k on: two
walkers in front of a moving camera.  FLAGS is what the oracle measured (frames 2 ..); test_motion_scene_cpu.py recomputes it."""
import functools

import numpy as np

import oracle_lib as O

ORB = (1000, 1.2, 8, 15, 5)              # nfeatures, scale, levels, FAST thresholds of every ORB run on these streams
X0, Y0 = 40, 40

# (width, height, what) -> flags of frames 2, 3, ... as the oracle measured them
FLAGS = {
    (192, 144, (0, 0)): [1, 1, 1, 1, 1],                  # zero flow
    (192, 144, (1, 0)): [0, 0, 0, 0, 0],
    (192, 144, (3, 1)): [0, 0, 0, 0, 0],
    (192, 144, (5, 0)): [0, 0, 0, 0, 0],
    (192, 144, (8, 0)): [1, 1, 1, 1, 0],
    (192, 144, (6, 2)): [0, 1, 0, 1, 1],                  # alternates inside one stream
    (192, 144, (12, 3)): [0, 0, 0, 0, 0],                 # the flow loses track
    (192, 144, (0, 0, "block")): [0, 0, 0, 0, 0],
    (192, 144, (1, 0, "block")): [0, 0, 0, 0, 0],
    (192, 144, (3, 1, "block")): [0, 0, 0, 0, 0],
    (192, 144, (5, 0, "block")): [0, 0, 0, 0, 0],
    (192, 144, (8, 0, "block")): [1, 0, 1, 1, 1],
    (192, 144, (6, 2, "block")): [1, 1, 1, 1, 1],
    (192, 144, (12, 3, "block")): [0, 0, 0, 0, 0],
    (320, 240, ("walkers", 0)): [1, 0, 1, 0, 1, 0],
    (320, 240, ("walkers", 1)): [0, 1, 0, 1, 0],
}


def intrinsics(w):
    from sindslam_amd.synth import TUM3
    s = w / 640.0
    return (TUM3["fx"] * s, TUM3["fy"] * s, TUM3["cx"] * s, TUM3["cy"] * s, TUM3["depth_factor"])


@functools.lru_cache(maxsize=None)
def _base():
    from sindslam_amd.synth import SyntheticStream
    bgr, depth = SyntheticStream(seed=5).frame(3)
    bgr.setflags(write=False); depth.setflags(write=False)
    return bgr, depth


# a block with a motion of its own in front of the panning background: without it a pan stream is a static scene, the detector finds nothing dynamic and its
# outputs do not depend on the flow at all (a wrong flow field would go unnoticed).  Texture from the base frame at SRC, 1.2 m in front of the camera.
BLOCK = dict(src=(420, 300), size=(44, 52), at=(96, 30), v=(-4, 3), depth=6000)


def window(w, h, x, y, i=None):
    """the window at (x, y) of the base frame; i (frame number) pastes the moving block at its position in frame i"""
    bgr, depth = _base()
    assert 0 <= x and x + w <= bgr.shape[1] and 0 <= y and y + h <= bgr.shape[0], (w, h, x, y)
    b = np.ascontiguousarray(bgr[y:y + h, x:x + w]); d = np.ascontiguousarray(depth[y:y + h, x:x + w])
    if i is not None:
        (sx, sy), (bw, bh), (ax, ay), (vx, vy) = BLOCK["src"], BLOCK["size"], BLOCK["at"], BLOCK["v"]
        px, py = ax + vx * i, ay + vy * i
        assert 0 <= px and px + bw <= w and 0 <= py and py + bh <= h, (i, px, py)
        b[py:py + bh, px:px + bw] = bgr[sy:sy + bh, sx:sx + bw]; d[py:py + bh, px:px + bw] = BLOCK["depth"]
    return b, d


@functools.lru_cache(maxsize=None)
def stream(w, h, what, count=7):
    """(bgr u8 [count, h, w, 3], depth u16 [count, h, w]), read-only"""
    if what[0] == "walkers":
        from sindslam_amd.synth import SyntheticStream
        b, d = SyntheticStream(width=w, height=h, seed=777, motion_scale=6.0).frames(what[1], count)
    else:
        dx, dy = what[:2]
        fr = [window(w, h, X0 + dx * i, Y0 + dy * i, i if what[2:] == ("block",) else None) for i in range(count)]
        b = np.stack([f[0] for f in fr]); d = np.stack([f[1] for f in fr])
    b.setflags(write=False); d.setflags(write=False)
    return b, d


def sequence(w, h, pans):
    """one sequence whose camera pans by pans[i] = (dx, dy) between frame i and frame i + 1 (the window's position accumulates); frame 0 at (40, 40).  The block
    walks its seven positions forth and back."""
    x, y = X0, Y0; fr = [window(w, h, x, y, 0)]
    for i, (dx, dy) in enumerate(pans):
        x += dx; y += dy; fr.append(window(w, h, x, y, abs((i + 1 + 6) % 12 - 6)))
    return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])


@functools.lru_cache(maxsize=None)
def oracle_run(w, h, what, last=5):
    """the oracle's in-order loop over frames 2 .. last of a stream (primed with frames 1, 0): per frame a dict of flag, endFlow, endFlow2, dyna, label, mask
    (the 15 x 15 dilation), keypoints and descriptors (O.ORBextractor(*ORB) on BGR2GRAY with the R / B quirk, as the pipeline runs it with orb_gray_rgb_order=1)"""
    bgr, depth = stream(w, h, what, max(7, last + 1))
    det = O.DynaDetect(bgr[1], bgr[0], *intrinsics(w)); orb = O.ORBextractor(*ORB); out = {}
    for f in range(2, last + 1):
        dy, lb = det.detect(bgr[f], depth[f]); e1, e2, lm = det.motion(); mk = O.dilate15(dy)
        k, dsc = orb.extract(O.bgr2gray(bgr[f], swap_rb=True), mk)
        for a in (dy, lb, mk, k, dsc):
            a.setflags(write=False)
        out[f] = dict(flag=int(lm), endFlow=e1, endFlow2=e2, dyna=dy, label=lb, mask=mk, keypoints=k, descriptors=dsc)
    return out


@functools.lru_cache(maxsize=None)
def oracle_flags(w, h, what, last):
    """flags only (the state-free front half of the oracle): frames 2 .. last"""
    bgr, _ = stream(w, h, what, max(7, last + 1)); K = intrinsics(w); out = []
    for f in range(2, last + 1):
        det = O.DynaDetect(bgr[f - 1], bgr[f - 2], *K); det.flow_only(bgr[f]); out.append(int(det.motion()[2]))
    return out


def path_flows(w, h, what, f):
    """frame f of a stream: (full-frame flow as the oracle computes it, the same along the FIRST path only -- flow(n, n - 2) refined against frame n - 2,
    whatever the large-motion test says --, the oracle's flag).  On an unflagged frame the two are the same bits."""
    b, _ = stream(w, h, what, max(7, f + 1))
    fw, fh = int(np.float32(0.6) * w), int(np.float32(0.6) * h)
    det = O.DynaDetect(b[f - 1], b[f - 2], *intrinsics(w)); full = det.flow_only(b[f])[0]
    g = [O.resize_u8(O.bgr2gray(b[k]), fw, fh) for k in (f, f - 2)]
    fl = -O.deepflow(g[0], g[1]); ru, rv = O.varref(g[0], g[1], fl[..., 0], fl[..., 1])
    first = O.resize_f32(np.stack([ru, rv], axis=2), w, h) * np.float32(np.float32(1.0) / np.float32(0.6))
    return full, first.astype(np.float32), int(det.motion()[2])


# ---- the configurations test_pipeline_motion_gpu.py runs: name -> (width, height, S, T, flow_slices, streams in pipeline order)
BL = "block"
CONFIGS = {
    "one_slice":        (192, 144, 4, 2, 1, [(1, 0, BL), (6, 2, BL), (3, 1, BL), (0, 0)]),          # flags 0 0 1 1 0 0 1 1 in both steps
    "slices_clean":     (192, 144, 4, 2, 2, [(1, 0, BL), (3, 1, BL), (6, 2, BL), (0, 0)]),          # slice 0 has no flagged pair, slice 1 only flagged ones
    "slices_mixed":     (192, 144, 4, 2, 2, [(5, 0, BL), (6, 2, BL), (6, 2), (8, 0, BL)]),          # 0 0 1 1 | 0 1 1 0, then 0 0 1 1 | 0 1 1 1
    "three_slices":     (192, 144, 3, 2, 3, [(6, 2, BL), (1, 0, BL), (8, 0, BL)]),                  # Bs = 2; the last slice holds one flagged pair of two (first step)
    "walkers":          (320, 240, 2, 2, 1, [("walkers", 0), ("walkers", 1)]),                      # moving content: 1 0 0 1 in both steps
    "one_one":          (192, 144, 1, 1, 1, [(8, 0, BL)]),                                          # B = 1 on the gathered path: flagged, then not
}
RAGGED = "one_slice"                     # a second step with set_active_frames([2, 1, 0, 2])
BATCH_SWITCHES = "slices_mixed"          # flow-mask and RAG batching on and off
STEPS = 2


def config_flags(name, flags_of=None):
    """[step][k = s * T + t] flags of a configuration from FLAGS (or from flags_of(w, h, what) -> list for frames 2 ..)"""
    w, h, S, T, _, streams = CONFIGS[name]
    get = flags_of or (lambda w_, h_, what: FLAGS[(w_, h_, what)])
    return [[get(w, h, streams[s])[step * T + t] for s in range(S) for t in range(T)] for step in range(STEPS)]


# ---- one sequence for the in-order driver: calm, fast, static, eight frames each (frame 0 + 24)
SEQ_SIZE = (192, 144)
SEQ_PANS = [(1, 0)] * 8 + [(8, 0)] * 8 + [(0, 0)] * 8
SEQ_STEP = 8                             # frames per step of process_sequence_exact: chunks 1..8, 9..16, 17..24


def seq_intr():
    from sindslam_amd.synth import TUM3
    K = intrinsics(SEQ_SIZE[0])
    return dict(TUM3, fx=K[0], fy=K[1], cx=K[2], cy=K[3])


@functools.lru_cache(maxsize=None)
def seq_frames():
    b, d = sequence(*SEQ_SIZE, SEQ_PANS); b.setflags(write=False); d.setflags(write=False); return b, d


@functools.lru_cache(maxsize=None)
def seq_flags(threads=8):
    """the oracle's flag of frames 1 .. (frame 0 primes twice, as the reference loop does); entry 0 is None"""
    from concurrent.futures import ThreadPoolExecutor
    bgr, _ = seq_frames(); K = intrinsics(SEQ_SIZE[0]); O.lib()

    def one(f):
        det = O.DynaDetect(bgr[f - 1], bgr[max(f - 2, 0)], *K); det.flow_only(bgr[f]); return int(det.motion()[2])
    with ThreadPoolExecutor(threads) as ex:
        return [None] + list(ex.map(one, range(1, len(bgr))))
