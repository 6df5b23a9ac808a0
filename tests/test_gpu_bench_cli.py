"""bench.py's command line: a plain run prints the headline line only (the rest is behind
--full), --steps sets the timed steps, and --dump-outputs writes the last step's result slots,
here compared with the same C5Shard run in this process (a 48-frame sequence)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ygzfe
from ygzfe import dist as D
from ygzfe.sequence import C5Shard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 48
FULL_ONLY = ("roofline", "cpu_baseline", "latency", "c4_batched", "tracking_searches", "dropin_call_sites",
             "next_rows", "sequence_check")


def test_plain_run_headline_and_dumped_outputs(gpu, tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--frames", str(FRAMES), "--dump-outputs", str(out)], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(FRAMES / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]

    arrays = {n: np.load(out / (n + ".npy")) for n in ("header", "sample_frames", "keypoints", "descriptors")}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in arrays)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20

    # the same job in this process: bench.py's default schedule (pipe, 4 chunks)
    sh = C5Shard(FRAMES, 0, 1, torch.device("cuda", 0), chunks=4, schedule="pipe")
    sh.step()
    torch.cuda.synchronize()
    sh.check()
    slots = sh.root_slots().cpu().numpy()
    cap = sh.cap
    assert np.array_equal(arrays["sample_frames"], np.arange(FRAMES))  # every frame fits the sample
    assert arrays["keypoints"].shape == (FRAMES, cap, 7) and arrays["descriptors"].shape == (FRAMES, cap, 32)
    for f in range(FRAMES):
        u = D.unpack_slot(slots[f], cap, ygzfe.KP_DTYPE)
        h = arrays["header"][f]
        assert (h[0], h[1], h[10], h[11]) == (u["n"], u["n_visible"], f, float(u["has_align"]))
        assert np.array_equal(h[2:6].astype(np.float32), u["q"]) and np.array_equal(h[6:9].astype(np.float32), u["t"])
        assert np.float32(h[9]) == np.float32(u["chi2"])
        n = u["n"]
        kp = arrays["keypoints"][f]
        for c, name in enumerate(ygzfe.KP_DTYPE.names):
            assert np.array_equal(kp[:n, c], u["kps"][name].astype(np.float32)), (f, name)
        assert not kp[n:].any()
        assert np.array_equal(arrays["descriptors"][f, :n], u["desc"].astype(np.float32))
