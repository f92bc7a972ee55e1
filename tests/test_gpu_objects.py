"""GPU tests of the object-level statistics (csrc/objects.hip): the roots and the int64 tables of utils/objects.object_stats against
the min-propagation restatement (tests/_objects_ref.py), always as EQUALITY OF INTEGERS - no tolerance appears anywhere; the
labeller alone, size edges, batching, repeatability, out=, chunking, the refusals in Python; the Evaluator's and the command line's
opt-in paths.

The kernel unites inside 64 x 64 tiles in LDS, then across tile borders on the global array, then counts.  Every case of
_objects_ref.CASES is there because a part of that can fail on it: frames smaller than a tile, exactly one tile, two tiles plus one
pixel each way, a width-1 serpentine (the longest chain a find can meet; at 130 x 130 it crosses tile borders dozens of times, so
border unions race on one component), diagonals joined only through tile corners, a checkerboard (every pixel its own component
under 4-connectivity, two components touching every border under 8), a constant frame (the wave-combined atomics), blocky maps at
K = 1, 9, 32, labels 255, -1, 256, 2^40 + 3, predictions out of range, an all-ignored frame, an ignored stripe through a blob.
Each runs under both connectivities."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _boundary_ref as bref
import _objects_ref as ref
import detweights as dw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ob():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd.utils import objects
    return objects


def dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)


def host(t):
    return t.cpu().numpy()


def check(table, c, what):
    """roots, tables and status against the restatement's, by equality"""
    assert table.obj.dtype == torch.int64 and table.mass.dtype == torch.int64 and table.status.dtype == torch.int32
    assert host(table.status).tolist() == [0, 0], what
    if table.root_g is not None:
        assert table.root_g.dtype == torch.int32 and table.root_p.dtype == torch.int32
        assert np.array_equal(host(table.root_g), c["root_g"]), (what, "root_g")
        assert np.array_equal(host(table.root_p), c["root_p"]), (what, "root_p")
    assert tuple(table.obj.shape) == c["obj"].shape and tuple(table.mass.shape) == c["mass"].shape, what
    assert np.array_equal(host(table.obj), c["obj"]), (what, "obj")
    assert np.array_equal(host(table.mass), c["mass"]), (what, "mass")


@pytest.mark.parametrize("conn", [8, 4])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_roots_and_tables_equal_the_restatement(ob, name, conn):
    c = ref.case(name, conn)
    t = ob.object_stats(*dev(c["pred"], c["label"]), n_class=c["K"], connectivity=conn, return_roots=True)
    check(t, c, (name, conn))


def test_connected_components_alone_on_int32_and_int64(ob):
    c = ref.case("blocky_K9", 8)
    want = c["root_g"]
    counts = np.array([len(np.unique(r[r >= 0])) for r in want])
    for dtype in (torch.int64, torch.int32):
        m = torch.from_numpy(np.array(c["label"])).to(dtype).cuda()
        root, count = ob.connected_components(m, 9)
        assert root.dtype == torch.int32 and count.dtype == torch.int64
        assert np.array_equal(host(root), want) and np.array_equal(host(count), counts)
    c4 = ref.case("odd_labels", 4)  # the int64 path keeps 2^40 + 3 outside every component
    root, count = ob.connected_components(dev(c4["label"])[0], 9, connectivity=4)
    assert np.array_equal(host(root), c4["root_g"]) and int(count[0]) == c4["obj"][0, 0].sum()
    with pytest.raises(RuntimeError, match="int32 or torch.int64"):
        ob.connected_components(dev(c4["label"])[0].float(), 9)


@pytest.mark.parametrize("edges", [(), (1,), (3, 50, 4000)])
def test_size_edges(ob, edges):
    c = ref.case("65x129", 8, edges)
    t = ob.object_stats(*dev(c["pred"], c["label"]), n_class=c["K"], size_edges=edges, return_roots=True)
    check(t, c, edges)
    assert t.obj.shape[3] == len(edges) + 1
    if edges == (3, 50, 4000):
        assert (c["obj"][0, 0].sum(axis=(0, 2))[1:] > 0).all()  # three of the four buckets hold objects of the ground truth


def test_an_object_whose_area_equals_an_edge(ob):
    label = np.zeros((1, 20, 30), dtype=np.int64)
    label[0, 2:8, 3:9] = 1    # 36 pixels = the edge: the upper bucket
    label[0, 12:17, 3:10] = 1  # 35 pixels: the lower one
    pred = label.astype(np.int32)
    t = ob.object_stats(*dev(pred, label), n_class=2, size_edges=(36,))
    want = ref.object_stats(pred, label, 2, 8, (36,))
    assert np.array_equal(host(t.obj), want[2]) and np.array_equal(host(t.mass), want[3])
    assert host(t.obj)[0, 0, 1, :, 10].tolist() == [1, 1] and host(t.mass)[0, 0, 1, :, 0].tolist() == [35, 36]


def test_two_runs_give_equal_bits_and_a_frame_alone_equals_its_share_of_a_batch(ob):
    a, b = ref.case("65x129", 8), ref.case("serpentine_130", 8)
    c = ref.case("blocky_K9", 8)  # two frames of 65 x 129
    pred = np.concatenate([a["pred"], c["pred"]])
    label = np.concatenate([a["label"], c["label"]])
    p, l = dev(pred, label)
    first = ob.object_stats(p, l, return_roots=True)
    again = ob.object_stats(p, l, return_roots=True)
    for k in ("obj", "mass", "root_g", "root_p"):
        assert host(getattr(first, k)).tobytes() == host(getattr(again, k)).tobytes(), k
    assert host(first.status).tolist() == [0, 0]
    for i in range(3):
        alone = ob.object_stats(p[i:i + 1], l[i:i + 1], return_roots=True)
        for k in ("obj", "mass", "root_g", "root_p"):
            assert np.array_equal(host(getattr(alone, k))[0], host(getattr(first, k))[i]), (i, k)
    assert np.array_equal(host(first.obj)[0], a["obj"][0]) and np.array_equal(host(first.obj)[1:], c["obj"])
    s = ob.object_stats(*dev(b["pred"], b["label"]), n_class=2)  # racing border unions: twice, equal bits
    s2 = ob.object_stats(*dev(b["pred"], b["label"]), n_class=2)
    assert host(s.obj).tobytes() == host(s2.obj).tobytes() and host(s.mass).tobytes() == host(s2.mass).tobytes()


def test_out_accumulates_and_chunking_changes_nothing(ob):
    c = ref.case("blocky_K9", 8)
    p, l = dev(c["pred"], c["label"])
    fresh = ob.object_stats(p, l)
    total = ob.ObjectTable.zeros("cuda")
    assert ob.object_stats(p, l, out=total) is total
    ob.object_stats(p, l, out=total)
    assert tuple(total.obj.shape) == (2, 9, 3, 11) and tuple(total.mass.shape) == (2, 9, 3, 2)
    assert np.array_equal(host(total.obj), 2 * c["obj"].sum(axis=0)) and np.array_equal(host(total.mass), 2 * c["mass"].sum(axis=0))
    assert np.array_equal(host(total.obj), 2 * host(fresh.obj).sum(axis=0)) and host(total.status).tolist() == [0, 0]
    with pytest.raises(ValueError, match="same n_class, connectivity and size_edges"):
        ob.object_stats(p, l, connectivity=4, out=total)
    with pytest.raises(ValueError, match="same n_class, connectivity and size_edges"):
        ob.object_stats(p, l, size_edges=(5,), out=total)
    with pytest.raises(ValueError, match="same n_class, connectivity and size_edges"):
        ob.object_stats(p, l, out=fresh)  # per-frame tables are no sums
    one = 65 * 129 * 26 + 8  # room for one frame per chunk
    chunked = ob.object_stats(p, l, return_roots=True, max_workspace_bytes=one)
    tiny = ob.object_stats(p, l, return_roots=True, max_workspace_bytes=1)  # (never below one frame)
    check(chunked, c, "one frame per chunk")
    check(tiny, c, "one frame per chunk, limit below a frame")
    assert host(chunked.obj).tobytes() == host(fresh.obj).tobytes() and host(chunked.mass).tobytes() == host(fresh.mass).tobytes()
    s = ob.object_scores(total)
    want = ref.scores(2 * c["obj"].sum(axis=0))
    for k, w in zip(("obj_recall", "obj_precision", "obj_f1"), want):
        assert np.array_equal(s[k], w, equal_nan=True), k


def test_python_refusals(ob):
    c = ref.case("7x5", 8)
    p, l = dev(c["pred"], c["label"])
    with pytest.raises(RuntimeError, match="contiguous"):
        ob.object_stats(p.transpose(1, 2), l.transpose(1, 2).contiguous())
    with pytest.raises(RuntimeError, match="int32"):
        ob.object_stats(p.long(), l)
    with pytest.raises(RuntimeError, match="int64"):
        ob.object_stats(p, l.int())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ob.object_stats(p.cpu(), l.cpu())
    with pytest.raises(RuntimeError, match="pred is"):
        ob.object_stats(p[:, :-1].contiguous(), l)
    with pytest.raises(ValueError, match="connectivity"):
        ob.object_stats(p, l, connectivity=6)
    with pytest.raises(ValueError, match="n_class"):
        ob.object_stats(p, l, n_class=33)
    with pytest.raises(ValueError, match="size_edges"):
        ob.object_stats(p, l, size_edges=(4, 4))
    with pytest.raises(ValueError, match=">= 1"):
        ob.object_stats(p[:0], l[:0])


# ---- through the Evaluator and the command line -------------------------------------------------------------------------------

EH, EW = 48, 64
PLAIN_KEYS = {"EN", "SD", "SF", "AG", "MI", "SCD", "CC", "PSNR", "mean", "precision", "recall", "iou", "mIoU"}
EDGES = (20, 200)


@pytest.fixture(scope="module")
def nets(ob):
    import segmif_amd.core as core
    seg, fus = core.Network3("mit_b1", 9, pretrained=None), core.Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0), dw.load_det_weights(fus, seed=0)
    return seg.cuda().eval(), fus.cuda().eval()


def frames(seed, B):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:EH, 0:EW]
    ir = np.stack([np.uint8(127 + 100 * np.sin(yy / (3.0 + b) + seed) * np.cos(xx / 5.0)) for b in range(B)])
    vis = np.stack([np.stack([np.uint8(rng.integers(0, 40) + 2 * xx + yy), np.uint8(3 * yy + b), np.uint8(255 - 2 * xx)], axis=-1) for b in range(B)])
    mask = np.uint8((ir.astype(np.int32) + vis[..., 0]) // 2)
    _, label = bref.synthetic(B, EH, EW, 9, 2, seed)
    return ir, vis, mask, label


@pytest.mark.parametrize("mode", ["eager", "graph", "tta"])
def test_evaluator_accumulates_the_table(ob, nets, mode):
    """three batches: the summed table equals object_stats' (and the restatement's) on the labels the evaluator returned; without
    objects= the result has the keys and values it always had"""
    from segmif_amd.evaluate import Evaluator
    from segmif_amd.tta import TTA
    kw = {"eager": {}, "graph": {"graph": True}, "tta": {"tta": TTA((1.0,), True, 8)}}[mode]
    settings = dict(connectivity=4, size_edges=EDGES, coverage=0.3)
    ev, plain = Evaluator(*nets, objects=settings, **kw), Evaluator(*nets, **kw)
    obj, mass = np.zeros((2, 9, 3, 11), dtype=np.int64), np.zeros((2, 9, 3, 2), dtype=np.int64)
    direct = ob.ObjectTable.zeros("cuda", 9, 4, EDGES)
    for i in range(3):
        ir, vis, mask, label = frames(40 + i, 2)
        args = dev(ir, vis, mask, label)
        _, labels = ev.update(*args)
        plain.update(*args)
        ob.object_stats(labels.contiguous(), args[3], 9, 4, EDGES, out=direct)
        want = ref.object_stats(host(labels), label, 9, 4, EDGES)
        obj += want[2].sum(axis=0)
        mass += want[3].sum(axis=0)
    assert obj[0].sum() > 0 and obj[1].sum() > 0
    assert np.array_equal(host(ev._objects.obj), obj) and np.array_equal(host(ev._objects.mass), mass)
    assert np.array_equal(host(direct.obj), obj) and np.array_equal(host(direct.mass), mass)
    res, res0 = ev.results(), plain.results()
    want = ob.object_scores(ob.ObjectTable(obj, mass, np.zeros(2, dtype=np.int32), 9, 4, EDGES), 0.3)
    for k in ob.OBJECT_SCORE_NAMES:
        assert np.array_equal(np.asarray(res[k]), np.asarray(want[k]), equal_nan=True), (k, res[k], want[k])
    assert set(res0) == PLAIN_KEYS and set(res) == PLAIN_KEYS | set(ob.OBJECT_SCORE_NAMES)
    for k in PLAIN_KEYS - {"mean"}:
        assert np.array_equal(np.asarray(res0[k]), np.asarray(res[k]), equal_nan=True), k
    assert res0["mean"] == res["mean"]
    doc, doc0 = ev.document(["x"] * 6, []), plain.document(["x"] * 6, [])
    assert doc["objects"] == {"connectivity": 4, "size_edges": [20, 200], "coverage": 0.3} and "objects" not in doc0
    json.dumps(doc)


def test_evaluate_command_line(ob, tmp_path):
    """two runs in fresh child processes on three 48 x 64 .npy frames: with --object-scores the JSON carries the scores and the
    settings and the summary line names the three means; without it the JSON's key set is what it always was"""
    for sub in ("ir", "vis", "mask", "label"):
        os.makedirs(tmp_path / sub)
    ir, vis, mask, label = frames(60, 3)
    for i in range(3):
        for sub, a in (("ir", ir), ("vis", vis), ("mask", mask), ("label", label)):
            np.save(tmp_path / sub / f"{i:03d}.npy", a[i])
    docs = {}
    for flag in (True, False):
        path = tmp_path / f"res{int(flag)}.json"
        cmd = [sys.executable, "-m", "segmif_amd.evaluate", "--ir", str(tmp_path / "ir"), "--vis", str(tmp_path / "vis"),
               "--mask", str(tmp_path / "mask"), "--label", str(tmp_path / "label"), "--out", str(tmp_path / "out"), "--backbone", "mit_b1",
               "--batch", "2", "--json", str(path)]
        cmd += ["--object-scores", "--object-size-edges", "20", "200", "--object-coverage", "0.3"] if flag else []
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        docs[flag] = json.load(open(path))
        summary = [l for l in r.stdout.splitlines() if l.startswith("[evaluate] EN ")]
        assert len(summary) == 1 and "  mIoU " in summary[0]
        assert all((f"  {k} " in summary[0]) == flag for k in ("objR", "objP", "objF1"))
    new = set(ob.OBJECT_SCORE_NAMES) | {"objects"}
    assert set(docs[False]) == PLAIN_KEYS | {"names", "seeded_weights"}  # the default command line's keys are what they were
    assert new <= set(docs[True]) and set(docs[True]) - new == set(docs[False])
    assert docs[True]["objects"] == {"connectivity": 8, "size_edges": [20, 200], "coverage": 0.3}
    assert len(docs[True]["obj_recall"]) == 9 and np.asarray(docs[True]["n_gt_objects"]).shape == (9, 3)
    assert 0.0 <= docs[True]["mObjF1"] <= 1.0 and np.asarray(docs[True]["n_gt_objects"]).sum() > 0
    assert docs[True]["mIoU"] == docs[False]["mIoU"] and docs[True]["mean"] == docs[False]["mean"]
