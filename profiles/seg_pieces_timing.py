"""Times SegAndMerge's piece extraction on the GPU (set_device_pieces) against the host function, through the single-stream detector (one tail, capacity 1).

    python profiles/seg_pieces_timing.py [frames]          # prints one JSON line per size and a summary

Per size (640 x 480, 1280 x 720): the same synthetic frames run through two detectors, switch off and on, in alternating blocks (off, on, off, on, ...) so that a
drift of the machine hits both; the first block of each is warm-up (it also creates the device stage's workspaces) and is dropped.  Reported per block: mean
milliseconds per frame of the whole call, of the depth half and of the SegAndMerge stage (sind_dyna_timing), then the median over the blocks and their spread.
The outputs of the two detectors are compared frame by frame; the counters must show every frame on the device."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sindslam_amd.dyna import DynaDetect          # noqa: E402
from sindslam_amd.synth import SyntheticStream, TUM3          # noqa: E402


def run(w, h, frames, blocks=5):
    s = SyntheticStream(w, h)
    bgr, depth = s.frames(0, frames + 2)
    K = (s.fx, s.fy, s.cx, s.cy, TUM3["depth_factor"])
    det = {False: DynaDetect(bgr[1], bgr[0], *K), True: DynaDetect(bgr[1], bgr[0], *K)}
    det[True].set_device_pieces(True)
    rows = {False: [], True: []}; outs = {}
    try:
        for blk in range(blocks + 1):
            for on in (False, True):
                d = det[on]; d.timing(True); t0 = time.perf_counter(); o = []
                for t in range(2, frames + 2):
                    o.append(d.DetectDynaArea(bgr[t], depth[t], t))
                wall = (time.perf_counter() - t0) * 1e3 / frames; tm = d.timing(True)
                if blk:
                    rows[on].append((wall, tm["depth_half"], tm["tail_stages"]["seg_and_merge"]))
                outs[on] = o
        same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(outs[False], outs[True]))
        counters = det[True].device_pieces()
    finally:
        for d in det.values():
            d.close()
    res = dict(size=[w, h], frames_per_block=frames, blocks=blocks, outputs_equal=bool(same), device_pieces=counters)
    for on in (False, True):
        a = np.array(rows[on]); tag = "device" if on else "host"
        for i, key in enumerate(("call_ms", "depth_half_ms", "seg_and_merge_ms")):
            res["%s_%s" % (tag, key)] = dict(median=round(float(np.median(a[:, i])), 3), min=round(float(a[:, i].min()), 3), max=round(float(a[:, i].max()), 3))
    return res


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    for w, h in ((640, 480), (1280, 720)):
        print(json.dumps(run(w, h, n)), flush=True)
