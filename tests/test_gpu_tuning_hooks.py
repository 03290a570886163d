"""`-m gpu`: the opt-in tuning hook LCGS_GRAPH=1 (the fused frame captured once and replayed as a hipGraph, per-call
parameters read from device memory) stays correct.  It is not the default (measured: no gain, the short kernels are
GPU-latency-bound, not host-bound) but must still produce the reference frame, so the fused-frame parity suite runs once
more under it."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# (the two ingest tests: a scene the context RE-ORDERED under the graph hook -- its equal-depth scratch must exist before
#  the capture starts; round 3's advisor finding)
FILES = ["tests/test_gpu_fused.py", "tests/test_gpu_backward.py",
         "tests/test_gpu_ingest.py::test_upload_keeps_the_scene_in_spatial_order_by_default_too",
         "tests/test_gpu_ingest.py::test_equal_depths_blend_in_file_order_after_the_spatial_reorder"]


# persistent: bounded grids of tile workgroups pulling from a counter (what camera batches / lcgs_fit_views use while several
# frames are in flight), forced for EVERY frame and for the render-backward.  Same frames, bit for bit.
@pytest.mark.parametrize("hook", [{"LCGS_GRAPH": "1"}, {"LCGS_RENDER_WGS_PER_CU": "3", "LCGS_BWD_WGS_PER_CU": "2"}],
                         ids=["hipgraph", "persistent"])
def test_parity_suites_under_tuning_hook(hook):
    env = dict(os.environ, **hook)
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + FILES,
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


# The stage path's A/B hooks of round 5: the splatter's scalars by copy + synchronisation instead of the posted mailbox, the
# one-slab-per-wave SH kernel instead of the streaming one.  Both routes must produce the reference's buffers entry for entry.
@pytest.mark.parametrize("hook", [{"LCGS_STAGE_MAILBOX": "0"}, {"LCGS_STAGE_SH_STREAM": "0"}], ids=["sync-readback", "sh-one-slab"])
def test_stage_suite_under_stage_hooks(hook):
    env = dict(os.environ, **hook)
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          "tests/test_gpu_stages.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


# The render-backward's other instantiation: no kept strip bits (the launcher's form for a caller without them), the strip tests
# repeated in the kernel, every reachable entry walked.  Same gradients within the suite's tolerances.
def test_backward_suite_without_kept_masks():
    env = dict(os.environ, LCGS_BWD_USE_MASKS="0")
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          "tests/test_gpu_backward.py", "tests/test_gpu_random_sweep.py"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=1200)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


# Per-block pair lists (frames without backward state; by default only from ~3 M pairs up, which no small test scene reaches)
# forced on: the fused-frame, ingest and random-sweep suites -- every frame against the oracle bit for bit, camera batches, LOD,
# half-precision coefficients, overflow handling -- and forced off.
@pytest.mark.parametrize("mode", [{"LCGS_COARSE_LISTS": "1"}, {"LCGS_COARSE_LISTS": "0"}],
                         ids=["block-lists", "tile-lists"])
def test_parity_suites_under_forced_list_granularity(mode):
    env = dict(os.environ, **mode)
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          "tests/test_gpu_fused.py", "tests/test_gpu_ingest.py", "tests/test_gpu_random_sweep.py",
                          "tests/test_gpu_lod.py", "tests/test_gpu_sh_degrees.py", "tests/test_gpu_backward.py",
                          "tests/test_gpu_train.py", "tests/test_gpu_owner.py"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=1800)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


def test_workload_sweep_tool_runs_and_its_oracle_points_are_bit_identical(lcgs, tmp_path):
    """`bench.py --sweep` (tools/workload_sweep.py) on scenes cut to a twentieth: every point is measured, the fitted model and
    the findings are written, the two oracle points are bit-identical, and the default list granularity never loses more than
    a few per cent to a forced one (the rule of abi_frame.cpp came out of this sweep at full size)."""
    import json
    import subprocess
    import sys

    from conftest import ROOT

    out = str(tmp_path / "sweep.json")
    env = dict(os.environ, LCGS_SWEEP_QUICK="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sweep", "--sweep-out", out], env=env,
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    d = json.load(open(out))
    assert len(d["points"]) == 30 and d["quick"]
    assert all(c["bit_identical"] and c["num_rendered_equal"] for c in d["oracle_checks"]) and len(d["oracle_checks"]) == 2
    assert not d["findings"]["pair_workspace_grew_inside_a_timed_loop"]
    assert all(p["forward_fps"]["default"] > 0 and p["fwd_bwd_msplats"] > 0 and p["examined"] > 0 for p in d["points"])
