"""In-process A/B of the batched RAG stage of SegAndMerge (sind_pipe_set_rag_batch) on ONE pipeline handle: the headline's own loop (bench.py's default:
tum3, 128 streams x 4 frames, submit_dev / flush, 20 timed steps after 5 warm-up steps) with the switch off / on / off / on.  Same handle, same inputs, same
box: what differs between the legs is the switch.  Prints one JSON line per leg (pairs/s, ms per step, frames batched / fallen back, a checksum of the last step's
outputs) and, with --out FILE, appends them there.  --chunk sets the frames per set of launches (0: a whole k-means group).

    python3 profiles/rag_batch_ab.py [--config tum3] [--steps 20] [--warmup 5] [--chunk 32] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tum3"); ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=0); ap.add_argument("--frames-per-step", type=int, default=4); ap.add_argument("--out", default=None); ap.add_argument("--chunk", type=int, default=None)
    args = ap.parse_args()
    import bench as B
    import sindslam_amd.synth as SY
    cfg = B.CONFIGS[args.config]; S = args.streams or cfg["streams"]; T = args.frames_per_step; K, Wm = args.steps, args.warmup
    intr0 = getattr(SY, cfg["intr"]); sc = cfg["width"] / 640.0
    intr = dict(intr0, fx=intr0["fx"] * sc, fy=intr0["fy"] * sc, cx=intr0["cx"] * sc, cy=intr0["cy"] * sc)
    ndata = min(K + Wm, 12)
    base_b, base_d = B.base_frames(cfg, T * ndata + 2, 12345, nseeds=3)          # before torch / HIP exist: the generator forks workers
    prime_b, _ = B.stream_variants(base_b[:, :2], base_d[:, :2], S)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    pipe = B.make_pipeline(cfg, intr, S, T, 0)
    dev_b, dev_d = B.device_step_inputs(base_b, base_d, S, T, ndata, "cuda")
    torch.cuda.synchronize()
    lines = []
    for leg, on in enumerate((False, True, False, True)):
        for s in range(S):                                                       # every leg starts from the same state and the same gray history
            pipe.prime(s, prime_b[s, 1], prime_b[s, 0])
        pipe.set_rag_batch(on)
        if args.chunk is not None:
            pipe.set_rag_batch_chunk(args.chunk)
        for i in range(Wm):
            pipe.process_dev(dev_b[i % ndata].data_ptr(), dev_d[i % ndata].data_ptr())
        torch.cuda.synchronize()
        _, warm_frames, _ = pipe.rag_batch()
        t0 = time.perf_counter(); flow = tails = wait = 0.0
        for i in range(Wm, Wm + K):
            pipe.submit_dev(dev_b[i % ndata].data_ptr(), dev_d[i % ndata].data_ptr())
            st = pipe.stats(); flow += st["flow_ms"]; tails += st["tails_ms"]; wait += st["tail_wait_ms"]
        pipe.flush(); torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        _, frames, fallback = pipe.rag_batch()
        line = dict(leg=leg, rag_batch=on, chunk=args.chunk, config=args.config, streams=S, frames_per_step=T, steps=K, warmup=Wm, value=round(S * T * K / dt, 1), unit="pairs/s",
                    ms_per_step=round(dt / K * 1e3, 2), dense_flow_ms=round(flow / K, 2), tails_ms=round(tails / K, 2), tail_wait_ms=round(wait / K, 2),
                    frames_batched=frames, frames_batched_timed=frames - warm_frames, frames_fallback=fallback,
                    checksum=int(pipe.dyna.sum()) + int(pipe.label.sum()) + int(pipe.mask.sum()) + int(pipe.nkp.sum()))
        print(json.dumps(line), flush=True); lines.append(line)
    pipe.close()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
