"""A pipeline step with SegAndMerge's piece extraction on the GPU (set_device_pieces) against the same step with the switch off.

    python profiles/seg_pieces_pipeline_ab.py [streams] [frames_per_step] [blocks]

Two pipelines of the same shape (640 x 480, synthetic stream, every stream the same frames), one with the switch on; they take turns step by step (off, on, off, on, ...)
so that a drift of the machine hits both.  The first two steps of each are warm-up (workspaces, the device stage's included) and are dropped.  Per timed step: wall
milliseconds, frame pairs per second, and the host CPU time of the whole process per frame (time.process_time).  Printed: median [min .. max] over the steps, one JSON line."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sindslam_amd.pipeline import Pipeline          # noqa: E402
from sindslam_amd.synth import SyntheticStream, TUM3          # noqa: E402


def main(S=32, T=4, blocks=6):
    w, h = 640, 480
    st = SyntheticStream(w, h); K = (st.fx, st.fy, st.cx, st.cy, TUM3["depth_factor"])
    steps = blocks + 2
    bgr, depth = st.frames(0, 2 + T * steps)
    pipes = {}
    for on in (False, True):
        p = Pipeline(S, T, w, h, *K, 1500, 1.2, 8, TUM3["ini_th"], TUM3["min_th"]); p.set_device_pieces(on)
        for s in range(S):
            p.prime(s, bgr[1], bgr[0])
        pipes[on] = p
    rows = {False: [], True: []}; same = True
    try:
        for k in range(steps):
            lo = 2 + T * k; b = np.ascontiguousarray(np.stack([bgr[lo:lo + T]] * S)); d = np.ascontiguousarray(np.stack([depth[lo:lo + T]] * S)); outs = {}
            for on in (False, True):
                c0 = time.process_time(); t0 = time.perf_counter()
                pipes[on].process(b, d)
                wall = time.perf_counter() - t0; cpu = time.process_time() - c0
                outs[on] = (pipes[on].dyna.copy(), pipes[on].label.copy())
                if k >= 2:
                    rows[on].append((wall * 1e3, S * T / wall, cpu * 1e3 / (S * T)))
            same = same and all(np.array_equal(x, y) for x, y in zip(outs[False], outs[True]))
        res = dict(shape=[S, T, w, h], timed_steps=blocks, outputs_equal=bool(same), device_pieces=pipes[True].device_pieces())
        for on in (False, True):
            a = np.array(rows[on])
            for i, key in enumerate(("step_ms", "pairs_per_s", "host_cpu_ms_per_frame")):
                res["%s_%s" % ("on" if on else "off", key)] = dict(median=round(float(np.median(a[:, i])), 3), min=round(float(a[:, i].min()), 3), max=round(float(a[:, i].max()), 3))
        print(json.dumps(res), flush=True)
    finally:
        for p in pipes.values():
            p.close()


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
