"""GPU test of the schedule of python -m segmif_amd.train beyond its first round: the other command tests stop at --rounds 1, so
none of them reaches the hand-over of checkpoints between rounds (the fusion phase's initial weights until round 2, the best
checkpoint afterwards; the segmentation phase's best checkpoint or the state the previous one left)."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_command_line_over_three_rounds(tmp_path):
    """Three rounds of one iteration each, at the smallest shapes of the other command tests, with the weights averaged: every
    phase is announced once and in order, `best` is the running maximum of the initial and the printed mIoUs, the LAST-state
    note appears exactly when nothing improved on the initial mIoU, and both checkpoints are left with finite weights."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "8", "--synthetic-size", "96", "128", "--backbone", "mit_b1",
           "--crop-size", "64", "--samples-per-gpu", "4", "--rounds", "3", "--fusion-iters", "1", "--seg-iters", "1", "--log-iters", "1",
           "--ema-decay", "0.9", "--out", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    initial = [float(ln.split()[-1]) for ln in lines if ln.startswith("[train] initial mIoU ")]
    assert len(initial) == 1, r.stdout[-4000:]
    phases = [ln for ln in lines if re.fullmatch(r"\[train\] round \d+: (fusion|segmentation)", ln)]
    assert phases == [f"[train] round {R}: {ph}" for R in (1, 2, 3) for ph in ("fusion", "segmentation")]
    scored = [re.fullmatch(r"\[train\] round (\d+) segmentation iter 1: mIoU (\S+) \(best (\S+)\)", ln) for ln in lines]
    scored = [(int(m[1]), float(m[2]), float(m[3])) for m in scored if m]
    assert [R for R, _, _ in scored] == [1, 2, 3]
    running = initial[0]
    for _, miou, best in scored:
        assert best >= running  # never decreases
        running = max(running, miou)
        assert best == running
    assert lines[-1].startswith("[train] wrote ")
    last_state = [ln for ln in lines if "LAST state" in ln]
    assert len(last_state) == (0 if any(miou > initial[0] for _, miou, _ in scored) else 1)
    assert sorted(os.listdir(tmp_path)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    for f in os.listdir(tmp_path):
        sd = torch.load(tmp_path / f, map_location="cpu")
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
