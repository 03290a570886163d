#!/usr/bin/env python3
"""A viewer paced BELOW the GPU's speed on the benchmark's scene and view: enqueue-only forward frames with a pause between
calls, so that successive frames chain on the host but nothing overlaps on the GPU.  Prints one JSON line: the
median GPU time of a frame (HIP events around each call on the context's stream), how many frames chained and how many took
the bounded renderer grid, and the same for an unpaced burst.  Run once as is and once under LCGS_PIPELINE=0."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402
import luisacomputegaussiansplatting_amd as L  # noqa: E402


def run(r, cam, img, frames, pause):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(frames)]
    before = r.pipeline_counts()
    for a, b in ev:
        a.record()
        r.forward(cam, img, sync=False)
        b.record()
        if pause:
            time.sleep(pause)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev[4:])
    after = r.pipeline_counts()
    return {"median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4),
            **{k: after[k] - before[k] for k in after}}


def main():
    W, H = 1920, 1080
    side = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(side)
    r = L.Renderer(L.Context(0, side.cuda_stream))
    r.upload_scene(L.synth_scene(1, 2001, bench.P_BICYCLE))
    cam = L.get_lookat_cam(*bench.view_pose(0), width=W, height=H)
    img = torch.zeros(3, H, W, device="cuda:0")
    for _ in range(3):
        r.forward(cam, img, sync=True)
    out = {"LCGS_PIPELINE": os.environ.get("LCGS_PIPELINE", "1"), "frames": 60,
           "paced_3ms": run(r, cam, img, 60, 0.003), "burst": run(r, cam, img, 60, 0.0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
