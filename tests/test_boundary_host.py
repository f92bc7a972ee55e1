"""Host-side checks of the contour scores (no GPU): the numpy restatement of the rule (tests/_boundary_ref.py) against cases
worked by hand below and against scipy's binary erosion, boundary_scores and boundary_widths of utils/metrics.py, and the
command line's new flags."""
import os
import re

import numpy as np
import pytest

import _boundary_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frame(square_at):
    """7 x 9, class 0, one 3 x 3 square of class 1 whose top-left corner is `square_at`"""
    m = np.zeros((7, 9), dtype=np.int64)
    y, x = square_at
    m[y:y + 3, x:x + 3] = 1
    return m


def test_restatement_on_a_square_predicted_exactly():
    """d = 1.  Class 1: the band is the square without its centre, 8.  Class 0 has 63 - 9 = 54 pixels; a pixel's window is
    uniform iff it lies inside the frame (centres in rows 1..5, columns 1..7: 35) and misses the square (centres in rows 1..5,
    columns 2..6 touch it: 25), so 10 are uniform and 44 are in the band.  Contours: the square's 8 outer pixels, and the 5 x 5
    ring around it, 25 - 9 = 16; the frame's border is no contour.  The prediction equals the ground truth, so everything
    matches at theta = 0 and at theta = 1 alike, and the band's confusion matrix is diagonal."""
    g = frame((2, 3))
    for theta in (0, 1):
        cls, tri = ref.frame_tables(g.astype(np.int32), g, 2, 1, theta)
        assert cls.tolist() == [[44, 44, 44, 16, 16, 16, 16, 0], [8, 8, 8, 8, 8, 8, 8, 0]]
        assert tri.tolist() == [[44, 0], [0, 8]]


def test_restatement_on_a_square_predicted_one_pixel_to_the_right():
    """Ground truth: rows 2..4, columns 3..5 (centre (3, 4)); prediction: columns 4..6 (centre (3, 5)); d = 1.
    Each map alone is the case above: bands 44 and 8, contours 16 and 8.
    band_inter, class 1: the squares share columns 4, 5 (6 pixels), less the two centres: 4.
    band_inter, class 0: 63 - 12 = 51 pixels are 0 in both maps; uniform in g: columns 1, 7 of rows 1..5, uniform in p: columns
      1, 2 of rows 1..5; the union, columns 1, 2, 7, is 15 pixels, all of them 0 in both maps: 51 - 15 = 36.
    trimap, row 0 (44 band pixels of g = 0): p = 1 on column 6 of rows 2..4, which is in g's band: 3, so 41 and 3.
    trimap, row 1 (the square less (3, 4)): p = 0 on column 3: 3; p = 1 on columns 4, 5 less the centre: 5.
    theta = 0, class 1: the two 8-pixel rings meet in columns 4, 5 less both centres: 4, in both directions.
    theta = 0, class 0: the rings rows 1..5 x columns 2..6 and rows 1..5 x columns 3..7, less both squares: rows 1 and 5,
      columns 3..6: 8, in both directions.
    theta = 1: every contour pixel of either map has one of its class in the other map next to it: all 16 and all 8."""
    g, p = frame((2, 3)), frame((2, 4)).astype(np.int32)
    cls, tri = ref.frame_tables(p, g, 2, 1, 0)
    assert cls.tolist() == [[44, 44, 36, 16, 16, 8, 8, 0], [8, 8, 4, 8, 8, 4, 4, 0]]
    assert tri.tolist() == [[41, 3], [3, 5]]
    cls, tri = ref.frame_tables(p, g, 2, 1, 1)
    assert cls.tolist() == [[44, 44, 36, 16, 16, 16, 16, 0], [8, 8, 4, 8, 8, 8, 8, 0]]
    assert tri.tolist() == [[41, 3], [3, 5]]


def test_restatement_on_a_frame_of_one_class():
    """no contour anywhere; the band is the border ring of width d: 63 - 3 x 5 = 48 at d = 2; a window larger than the frame
    puts every pixel into the band"""
    g = np.zeros((7, 9), dtype=np.int64)
    cls, tri = ref.frame_tables(g.astype(np.int32), g, 3, 2, 1)
    assert cls.tolist() == [[48, 48, 48, 0, 0, 0, 0, 0], [0] * 8, [0] * 8]
    assert tri.tolist() == [[48, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert ref.frame_tables(g.astype(np.int32), g, 3, 4, 0)[0][0, 0] == 63


def test_restatement_ignores_and_blanks():
    """label values outside 0..K-1 (255, -1, 256, 2^40 + 3) are IGN whatever their low bits; the prediction is blanked there
    and where it is itself outside 0..K-1; IGN is never counted but is a different value to its neighbours"""
    label = np.array([[0, 0, 255, -1], [0, 0, 256, 2 ** 40 + 3], [0, 0, 0, 0]], dtype=np.int64)
    pred = np.array([[0, 4, 1, 1], [-1, 0, 2, 3], [0, 0, 0, 0]], dtype=np.int32)
    g, p = ref.maps(pred, label, 4)
    assert g.tolist() == [[0, 0, -1, -1], [0, 0, -1, -1], [0, 0, 0, 0]]
    assert p.tolist() == [[0, -1, -1, -1], [-1, 0, -1, -1], [0, 0, 0, 0]]
    assert ref.contour(g).tolist() == [[False, True, False, False], [False, True, False, False], [False, True, True, True]]
    other = pred.copy()
    other[:2, 2:] = 7  # (arbitrary predictions on ignored pixels change nothing)
    a, b = ref.frame_tables(pred, label, 4, 1, 1), ref.frame_tables(other, label, 4, 1, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("H,W,d", [(37, 53, 3), (20, 31, 1), (9, 12, 8), (40, 40, 5)])
def test_band_is_mask_minus_its_erosion(H, W, d):
    """band_d(m) & {m = c} == mask_c & ~binary_erosion(mask_c, ones((3, 3)), iterations=d, border_value=0): the
    mask_to_boundary of the Boundary IoU toolkit"""
    ndi = pytest.importorskip("scipy.ndimage")
    K = 5
    _, label = ref.synthetic(1, H, W, K, d, seed=H + d, ignore=False)
    m = label[0]
    b = ref.band(m, d)
    for c in range(K):
        mask = m == c
        want = mask & ~ndi.binary_erosion(mask, structure=np.ones((3, 3)), iterations=d, border_value=0)
        assert np.array_equal(b & mask, want), c


def test_row_then_column_pass_equals_the_window():
    """the separable form the kernel uses (a row pass to h, the same test on h down the columns), written out naively here,
    against the brute-force window"""
    MIXED, OUT = -3, ref.OUTSIDE
    for (H, W, d, seed) in ((23, 31, 2, 0), (9, 12, 8, 1), (30, 17, 4, 2)):
        pred, label = ref.synthetic(1, H, W, 4, d, seed=seed)
        m = ref.maps(pred[0], label[0], 4)[0]
        pad = np.full((H + 2 * d, W + 2 * d), OUT, dtype=np.int64)
        pad[d:d + H, d:d + W] = m
        h = np.array([[pad[y, x] if (pad[y, x - d:x + d + 1] == pad[y, x]).all() else MIXED for x in range(d, d + W)]
                      for y in range(H + 2 * d)])
        uniform = np.array([[h[y + d, x] != MIXED and (h[y:y + 2 * d + 1, x] == h[y + d, x]).all() for x in range(W)] for y in range(H)])
        assert np.array_equal((m != ref.IGN) & ~uniform, ref.band(m, d))


def test_boundary_scores_on_hand_made_tables():
    from segmif_amd.utils.metrics import BOUNDARY_COLUMNS, BOUNDARY_SCORE_NAMES, boundary_scores, compute_results
    assert BOUNDARY_COLUMNS == ref.COLUMNS
    #        g_band p_band inter g_cont p_cont g_match p_match
    cls = np.array([[10, 6, 4, 8, 4, 4, 3, 0],     # BIoU 4 / 12, P = 3/4, R = 1/2 -> bf = 2 (3/8) / (5/4) = 0.6
                    [0, 0, 0, 0, 0, 0, 0, 0],      # an absent class: NaN everywhere
                    [5, 0, 0, 5, 0, 0, 0, 0],      # never predicted: BIoU 0, P NaN -> bf NaN
                    [3, 3, 0, 2, 2, 0, 0, 0]],     # P = R = 0 -> bf 0
                   dtype=np.int64)
    tri = np.array([[8, 2, 0, 0], [0, 0, 0, 0], [5, 0, 0, 0], [1, 0, 0, 2]], dtype=np.int64)
    s = boundary_scores(cls, tri)
    assert tuple(s) == BOUNDARY_SCORE_NAMES
    nan = float("nan")
    for k, want in (("boundary_iou", [4 / 12, nan, 0.0, 0.0]), ("bf_precision", [0.75, nan, nan, 0.0]),
                    ("bf_recall", [0.5, nan, 0.0, 0.0]), ("bf", [2 * 0.75 * 0.5 / 1.25, nan, nan, 0.0])):
        assert s[k].dtype == np.float64
        np.testing.assert_array_equal(s[k], np.array(want), err_msg=k)
    assert s["mBIoU"] == (4 / 12) / 4 and s["mBF"] == (2 * 0.75 * 0.5 / 1.25) / 4
    iou = compute_results(tri)[2]
    np.testing.assert_array_equal(s["trimap_iou"], iou)
    np.testing.assert_array_equal(iou, np.array([8 / 16, 0.0, 0.0, 2 / 3]))
    assert s["trimap_mIoU"] == float(np.mean([0.5, 0.0, 0.0, 2 / 3]))
    import torch
    t = boundary_scores(torch.from_numpy(cls), torch.from_numpy(tri))  # tensors are taken too
    assert all(np.array_equal(np.asarray(t[k]), np.asarray(s[k]), equal_nan=True) for k in s)


def test_boundary_widths():
    from segmif_amd.utils.metrics import boundary_widths
    assert boundary_widths(480, 640) == (16, 6)
    assert boundary_widths(512, 512) == (14, 5)
    assert boundary_widths(48, 64) == (2, 1)
    assert boundary_widths(9, 12) == (1, 0)       # 0.3 and 0.11: d is at least 1, theta may be 0
    assert boundary_widths(480, 640, ratio=0.01, bf_ratio=0.02) == (8, 16)
    assert boundary_widths(2160, 3840) == (88, 33)  # wider than the kernel takes: boundary_stats refuses these, see the GPU tests


def test_tile_constant_is_the_header_s():
    from segmif_amd.utils.metrics import BOUNDARY_TILE
    text = open(os.path.join(ROOT, "include", "segmif_hip.h")).read()
    assert int(re.search(r"#define SEGMIF_BOUNDARY_TILE (\d+)", text).group(1)) == BOUNDARY_TILE == 64


BASE = ["--ir", "a", "--vis", "b", "--mask", "c", "--out", "o"]


def test_parse_args_boundary_flags(capsys):
    from segmif_amd.evaluate import boundary_settings, parse_args
    args, tta = parse_args(BASE + ["--label", "l", "--boundary-scores"])
    assert tta is None and args.boundary_scores and boundary_settings(args) == {}
    args, _ = parse_args(BASE + ["--label", "l", "--boundary-scores", "--boundary-width", "5", "--bf-tolerance", "0"])
    assert boundary_settings(args) == {"d": 5, "theta": 0}
    args, tta = parse_args(BASE + ["--label", "l", "--boundary-scores", "--boundary-ratio", "0.01", "--bf-ratio", "0.02", "--flip"])
    assert boundary_settings(args) == {"ratio": 0.01, "bf_ratio": 0.02} and tta is not None
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--boundary-scores"])
    assert "--label" in capsys.readouterr().err
    for flag, v in (("--boundary-width", "5"), ("--bf-tolerance", "2"), ("--boundary-ratio", "0.01"), ("--bf-ratio", "0.01")):
        with pytest.raises(SystemExit):
            parse_args(BASE + ["--label", "l", flag, v])
        assert flag in capsys.readouterr().err


def test_parse_args_without_the_flag_is_what_it_was():
    from segmif_amd.evaluate import boundary_settings, parse_args
    args, tta = parse_args(BASE)
    assert tta is None and boundary_settings(args) is None and not args.boundary_scores
    assert (args.ir, args.vis, args.mask, args.out, args.label, args.backbone, args.batch, args.json, args.structural_scores) == \
        ("a", "b", "c", "o", None, "mit_b3", 1, None, False)
    args, tta = parse_args(BASE + ["--label", "l", "--batch", "2", "--structural-scores", "--ms-scales", "0.5", "1.0", "--flip"])
    assert boundary_settings(args) is None and args.label == "l" and args.batch == 2 and args.structural_scores
    assert tta is not None and tuple(tta.scales) == (0.5, 1.0)


def test_evaluator_refuses_unknown_boundary_settings():
    from segmif_amd.evaluate import Evaluator
    with pytest.raises(ValueError, match="boundary="):
        Evaluator(None, None, boundary={"width": 3})
