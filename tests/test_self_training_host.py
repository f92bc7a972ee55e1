"""Host tests of the self-training pieces: the float64 restatement of tests/_self_training_ref.py pinned on cases worked out by
hand, cross_mix_table, the command's flag rules, PairFolder(labelled=False), and the new symbols in the binding table and header."""
import math
import os

import numpy as np
import pytest
import torch

import _self_training_ref as ref


def test_resize_and_pseudo_label_on_a_hand_case():
    """2 x 2 -> 4 x 4, align_corners = False: source coordinates max(0, 0.5 (i + 0.5) - 0.5) = 0, 0.25, 0.75, 1 (clamped to the last
    pixel), so the per-axis weights are (1, 0), (.75, .25), (.25, .75), (0, 1).  Channel 0 is [[0, 4], [8, 12]], channel 1 is 2."""
    x = np.zeros((1, 2, 2, 2))
    x[0, :, :, 0] = [[0, 4], [8, 12]]
    x[0, :, :, 1] = 2.0
    a = np.array([[1, 0], [.75, .25], [.25, .75], [0, 1]])
    want0 = a @ x[0, :, :, 0] @ a.T
    assert np.allclose(want0[0], [0, 1, 3, 4]) and want0[1, 1] == 3.0 and want0[3, 3] == 12.0
    v = ref.resize(x, 4, 4)
    assert np.allclose(v[0, :, :, 0], want0, atol=1e-15) and np.allclose(v[0, :, :, 1], 2.0, atol=1e-15)
    r = ref.pseudo_label(x, 4, 4, tau=0.9)
    assert r["argmax"][0, 0].tolist() == [1, 1, 0, 0]  # 0 < 2, 1 < 2, 3 > 2, 4 > 2
    assert math.isclose(r["p_max"][0, 0, 0], 1 / (1 + math.exp(-2.0)), rel_tol=1e-15)      # logits (0, 2)
    assert math.isclose(r["p_max"][0, 3, 3], 1 / (1 + math.exp(-10.0)), rel_tol=1e-15)     # logits (12, 2)
    assert math.isclose(r["gap"][0, 0, 1], 1.0, rel_tol=1e-15)
    assert not r["confident"][0, 0, 0] and r["confident"][0, 3, 3]
    assert r["count"].tolist() == [int((r["p_max"] > 0.9).sum())]
    ign = ref.pseudo_label(x, 4, 4, tau=0.9, below="ignore", ignore_index=250)
    assert ign["label"][0, 0, 0] == 250 and ign["label"][0, 3, 3] == 0
    # a tie goes to the lowest index; the comparison with tau is strict
    tie = ref.pseudo_label(np.zeros((1, 2, 2, 3)), 4, 4, tau=1 / 3)
    assert (tie["argmax"] == 0).all() and tie["count"].tolist() == [0]
    assert ref.pseudo_label(np.zeros((1, 2, 2, 3)), 4, 4, tau=0.0)["count"].tolist() == [16]


def test_weighted_objective_on_a_hand_case():
    """rows (0, 0) y = 0, (0, ln 3) y = 1, one ignored row; u = (2, 0.5, 5): l = (ln 2, ln 4/3, 0).  The denominator is the valid
    count (mean) or the rows (mean_all) - never a sum of u."""
    x = torch.tensor([[0.0, 0.0], [0.0, math.log(3.0)], [1.0, -1.0]], dtype=torch.float64)
    y = torch.tensor([0, 1, 255])
    u = torch.tensor([2.0, 0.5, 5.0])
    s = 2 * math.log(2.0) + 0.5 * math.log(4.0 / 3.0)
    assert math.isclose(float(ref.weighted_objective(x, y, pixel_weight=u)), s / 2, rel_tol=1e-14)
    assert math.isclose(float(ref.weighted_objective(x, y, pixel_weight=u, reduction="mean_all")), s / 3, rel_tol=1e-14)
    # sample weights: rows_per_sample = 1 here; both weights multiply
    both = ref.weighted_objective(x, y, pixel_weight=u, sample_weight=torch.tensor([0.5, 2.0, 1.0]), reduction="mean_all")
    assert math.isclose(float(both), (math.log(2.0) + math.log(4.0 / 3.0)) / 3, rel_tol=1e-14)
    # a uniform weight scales the value: it does not cancel
    plain = ref.weighted_objective(x, y)
    assert math.isclose(float(ref.weighted_objective(x, y, sample_weight=torch.full((3,), 0.25))), 0.25 * float(plain), rel_tol=1e-14)
    # class weights enter the mean's denominator, u does not
    w = torch.tensor([3.0, 0.5], dtype=torch.float64)
    got = ref.weighted_objective(x, y, pixel_weight=u, weight=w)
    assert math.isclose(float(got), (2 * 3.0 * math.log(2.0) + 0.5 * 0.5 * math.log(4.0 / 3.0)) / 3.5, rel_tol=1e-14)
    with pytest.raises(ValueError):
        ref.weighted_objective(x, y, pixel_weight=u, reduction="ohem")


def test_cross_mix_table():
    from segmif_amd.data import ClassMix
    from segmif_amd.selftrain import cross_mix_table
    for B in (1, 2, 5):
        t = cross_mix_table(B, ClassMix(prob=1.0, seed=2))
        assert t.shape == (2 * B, 11) and t.dtype == np.int32
        assert t[:B, 0].tolist() == list(range(B)) and t[B:, 0].tolist() == list(range(B))  # every unlabelled sample takes labelled i
        assert (t[:, 1] == -1).all() and (np.sort(t[:, 2:], axis=1) == np.arange(9)).all()
    # the policy's probability, keys and stream: the rows are what policy.draw gives from the same seed
    twin = ClassMix(prob=0.5, seed=9).draw(4)
    t = cross_mix_table(4, ClassMix(prob=0.5, seed=9))
    mixed = twin[:, 0] != np.arange(4)
    assert t[4:, 0].tolist() == [i if m else 4 + i for i, m in enumerate(mixed)]
    assert np.array_equal(t[4:, 1:], twin[:, 1:])
    from segmif_amd import ops
    ops.check_mix_table(t, 8, 9)  # a table ops.class_mix accepts
    with pytest.raises(ValueError):
        cross_mix_table(2, ClassMix(classes="wanted"))


@pytest.mark.parametrize("argv", [
    ["--st-threshold", "0.9"], ["--st-below", "ignore"], ["--st-weight", "0.5"], ["--st-mix"], ["--st-mix-prob", "0.5"],
    ["--st-mix-min-pixels", "3"], ["--unlabelled-split", "extra"],
    ["--self-training"],                                                # no --ema-decay
    ["--self-training", "--ema-decay", "0.99", "--ema-nets", "fusion"],  # the segmentation net is not averaged
    ["--self-training", "--ema-decay", "0.99", "--st-mix-prob", "0.5"],  # --st-mix-prob without --st-mix
    ["--self-training", "--ema-decay", "0.99", "--st-threshold", "1.5"],
])
def test_flag_errors(argv, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--synthetic", "4"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--self-training" in err or "--st-" in err or "--ema-decay" in err


def test_pair_folder_without_labels(tmp_path):
    from segmif_amd.data import PairFolder
    rng = np.random.RandomState(0)
    for sub, shape in (("Infrared", (6, 8)), ("Visible", (6, 8, 3)), ("Mask2", (6, 8))):
        os.makedirs(tmp_path / sub)
        for name in ("a", "b"):
            np.save(tmp_path / sub / f"{name}.npy", rng.randint(0, 255, shape).astype(np.uint8))
    (tmp_path / "extra.txt").write_text("a\nb\n")
    assert not (tmp_path / "Label").exists()
    folder = PairFolder(str(tmp_path), str(tmp_path), "extra", labelled=False)
    name, ir, vis, mask, label = folder[1]
    assert name == "b" and label.shape == ir.shape == (6, 8) and label.dtype == np.uint8 and (label == 255).all()
    with pytest.raises(FileNotFoundError):
        PairFolder(str(tmp_path), str(tmp_path), "extra")[0]  # labelled, the default: Label/ is read


def test_new_symbols_are_bound_and_declared():
    from segmif_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "segmif_hip.h")).read()
    for name, nargs in (("segmif_pseudo_label_f32", 15), ("segmif_seg_objective_weighted_f32", 13),
                        ("segmif_seg_objective_weighted_bwd_f32", 16)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert f"int {name}(" in header
