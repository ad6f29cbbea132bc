"""A pipeline step with SegAndMerge's piece extraction batched per round on the GPU (set_pieces_batch) against the same step with the switch off.

    python profiles/seg_pieces_batch_ab.py [streams] [frames_per_step] [blocks] [width] [height] [sides]

Two pipelines of the same shape (synthetic stream, every stream the same frames), one with the switch on; they take turns step by step (off, on, off, on, ...) so that
a drift of the machine hits both.  Both run whole (non-split) rounds -- bit 4 of flow_opts_off -- the schedule of a step with more streams than pool workers and the only
one the batched piece stage is part of: two pipelines of 128 streams do not fit side by side, 32 streams alone would take split rounds, where the switch does nothing.
The first two steps of each are warm-up (workspaces, the piece batch's 2 GB included) and are dropped.  Per timed step: wall milliseconds, frame pairs per second, and
the host CPU time of the whole process per frame (time.process_time).  Printed: median [min .. max] over the steps, the schedule, pieces_batch() and whether the outputs
of the two sides were equal, one JSON line.  sides = "on" or "off": that side alone (for a kernel trace of one side)."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sindslam_amd.pipeline import Pipeline          # noqa: E402
from sindslam_amd.synth import SyntheticStream, TUM3          # noqa: E402


def main(S=32, T=4, blocks=6, w=640, h=480, sides="both"):
    st = SyntheticStream(w, h); K = (st.fx, st.fy, st.cx, st.cy, TUM3["depth_factor"])
    steps = blocks + 2
    bgr, depth = st.frames(0, 2 + T * steps)
    order = [v for v in (False, True) if sides in ("both", "on" if v else "off")]
    pipes = {}
    for on in order:
        p = Pipeline(S, T, w, h, *K, 1500, 1.2, 8, TUM3["ini_th"], TUM3["min_th"], flow_opts_off=16); p.set_pieces_batch(on)
        for s in range(S):
            p.prime(s, bgr[1], bgr[0])
        pipes[on] = p
    rows = {v: [] for v in order}; same = True; sched = {}
    try:
        for k in range(steps):
            lo = 2 + T * k; b = np.ascontiguousarray(np.stack([bgr[lo:lo + T]] * S)); d = np.ascontiguousarray(np.stack([depth[lo:lo + T]] * S)); outs = {}
            for on in order:
                c0 = time.process_time(); t0 = time.perf_counter()
                pipes[on].process(b, d)
                wall = time.perf_counter() - t0; cpu = time.process_time() - c0
                outs[on] = (pipes[on].dyna.copy(), pipes[on].label.copy(), pipes[on].mask.copy()); sched[on] = pipes[on].last_schedule()
                if k >= 2:
                    rows[on].append((wall * 1e3, S * T / wall, cpu * 1e3 / (S * T)))
            if len(order) == 2:
                same = same and all(np.array_equal(x, y) for x, y in zip(outs[False], outs[True]))
        res = dict(shape=[S, T, w, h], timed_steps=blocks, schedule=[sched[v] for v in order], outputs_equal=bool(same) if len(order) == 2 else None,
                   pieces_batch=pipes[True].pieces_batch() if True in pipes else None, rag_batch=[pipes[v].rag_batch() for v in order])
        for on in order:
            a = np.array(rows[on])
            for i, key in enumerate(("step_ms", "pairs_per_s", "host_cpu_ms_per_frame")):
                res["%s_%s" % ("on" if on else "off", key)] = dict(median=round(float(np.median(a[:, i])), 3), min=round(float(a[:, i].min()), 3), max=round(float(a[:, i].max()), 3))
        print(json.dumps(res), flush=True)
    finally:
        for p in pipes.values():
            p.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(*[int(v) for v in a[:5]], *a[5:6])
