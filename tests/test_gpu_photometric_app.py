"""`-m gpu`: lcgs-app --fit with --loss photometric (one view, --cameras through lcgs_fit_views, --fused-adam), and the two
options' argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

APP = os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "lcgs-app")
BASE = ["--synth", "0:20000:1001", "--res=320x240", "--world", "blender", "--pose", "lego"]


def _cameras(tmp_path):
    cams = str(tmp_path / "cams.txt")
    with open(cams, "w") as f:
        for p in ([-3, -0.5, 2.3], [2.5, 1.5, 1.0], [0.2, -3.0, 0.4]):
            f.write(" ".join(str(x) for x in p + [0, 0, 0.5] + [0, 0, 1]) + "\n")
    return cams


@pytest.mark.parametrize("mode", ["one_view", "cameras", "fused_adam"])
def test_lcgs_app_fit_with_the_photometric_loss(lcgs, tmp_path, mode):
    if not os.path.exists(APP):
        lcgs.build_library()
    extra = {"one_view": [], "cameras": ["--cameras", _cameras(tmp_path)], "fused_adam": ["--fused-adam"]}[mode]
    res = subprocess.run([APP] + BASE + ["--out", str(tmp_path), "--fit", "30", "--loss", "photometric"] + extra,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    losses = [float(x) for x in re.findall(r"step \d+ loss (\S+)", res.stdout)]
    assert len(losses) == 30 and all(np.isfinite(losses)), res.stdout
    print(f"[lcgs-app --loss photometric, {mode}] loss {losses[0]:.6f} -> {losses[-1]:.6f} "
          f"(ratio {losses[-1] / losses[0]:.3f})")
    assert losses[-1] < losses[0] and min(losses[-5:]) < min(losses[:5]), losses
    if mode == "cameras":
        assert "30 steps of 3 view(s)" in res.stdout


def test_lcgs_app_lambda_dssim_changes_the_loss(lcgs, tmp_path):
    first = []
    for lam in ("0", "1"):
        res = subprocess.run([APP] + BASE + ["--out", str(tmp_path), "--fit", "1", "--loss", "photometric", "--lambda-dssim", lam],
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        first.append(float(re.findall(r"step 1 loss (\S+)", res.stdout)[0]))
    assert first[0] > 0 and first[1] > 0 and first[0] != first[1]  # mean|x - y| against 1 - SSIM


@pytest.mark.parametrize("bad", [["--loss", "bogus"], ["--lambda-dssim", "2"], ["--lambda-dssim", "x"]])
def test_lcgs_app_refuses_bad_loss_options(lcgs, tmp_path, bad):
    res = subprocess.run([APP] + BASE + ["--out", str(tmp_path), "--fit", "2"] + bad, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode != 0
    assert "lcgs-app:" in res.stderr and ("loss" in res.stderr.lower() or "lambda" in res.stderr.lower()), res.stderr
