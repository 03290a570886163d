"""`-m gpu`: a plain bench.py run -- the headline line alone, --steps timed frames, and the frame the timed path rendered
(--dump-outputs) equal to the oracle's frame of the same scene and view."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_image(lcgs, oracle, tmp_path):
    W, H, P, steps = 320, 240, 100000, 3
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--splats", str(P), "--res", f"{W}x{H}", "--steps",
                          str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [x for x in res.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "forward fps @1080p, mip360_bicycle" and out["unit"] == "frames/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["n_gpus"] == 1 and out["steps"] == steps and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] - 1e3) <= 1e-2 * 1e3  # one GPU: frames/s = 1000 / ms per frame
    assert out["config"]["splats"] == P and out["config"]["resolution"] == f"{W}x{H}"
    # the legs of --full stay out of a plain run
    assert not {"roofline", "frame_roofline", "per_frame_events", "stages_ms", "moving_camera", "camera_batch", "stage_path",
                "fwd_bwd", "train_step", "file_order", "cpu_baseline", "parity"} & set(out)
    assert sorted(os.listdir(tmp_path / "out")) == ["image.npy"]
    img = np.load(tmp_path / "out" / "image.npy")
    assert img.shape == (3, H, W) and img.dtype == np.float32
    scene = lcgs.synth_scene(1, 2001, P)
    ref = oracle.render(scene, oracle.lookat(*bench.view_pose(0), width=W, height=H))
    assert ref["num_rendered"] == out["config"]["tile_pairs_reference"] > 0
    assert np.array_equal(img, ref["img"]), f"{int((img != ref['img']).any(axis=0).sum())} pixels differ from the oracle"
