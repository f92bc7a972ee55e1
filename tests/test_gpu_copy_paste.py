"""GPU tests of instance copy-paste: csrc/copy_paste.hip (segmif_object_boxes_i32, segmif_object_pack_u8, segmif_copy_paste_f32) through
ops.object_boxes / object_pack / copy_paste against the numpy restatement of the rule (tests/_copy_paste_ref.py), data.ObjectBank and
the pasting iterator against the restatement applied to a twin iterator without it, and the training command line with the new flags.
Integers and float BITS only: every comparison is equality."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _copy_paste_ref as ref
import _objects_ref as objects_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 0xffffffff
GUARD = 8  # rows behind a record list's capacity that must stay as they were


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import data
    return data


def _bits(t):
    t = t if isinstance(t, np.ndarray) else t.cpu().numpy()
    return t.view(np.int32) if t.dtype == np.float32 else t


def _images(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape + (3,), dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8))


def _u8_label(label, K):
    label = np.asarray(label)
    return np.where((label >= 0) & (label < K), label, 255).astype(np.uint8)


def device_boxes(label, K, conn, class_mask=ALL, min_area=1, max_box=1 << 40, capacity=None, chunks=None, frame0=0):
    """-> (count, the written records SORTED by (frame, root), the rows behind the capacity, the device roots): connected_components
    and ops.object_boxes over `label` (n, H, W) uint8, in one call or in the given chunks of frames"""
    from segmif_amd import ops
    from segmif_amd.utils.objects import connected_components
    lab = torch.from_numpy(label).cuda()
    root = connected_components(lab.to(torch.int32), K, conn)[0]
    n = len(label)
    capacity = n * label.shape[1] * label.shape[2] if capacity is None else capacity
    records = torch.full((capacity + GUARD, 8), -7, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = None
    for f0, f1 in (chunks or [(0, n)]):
        work = ops.object_boxes(root[f0:f1], lab[f0:f1], K, class_mask, min_area, max_box, records[:capacity], counter, frame0=frame0 + f0, workspace=work)
    count, rec = int(counter.item()), records.cpu().numpy()
    written = rec[:min(count, capacity)]
    return count, written[np.lexsort((written[:, 1], written[:, 0]))], rec[min(count, capacity):], root


def device_pack(rec, root, ir, vis, mask, frame0=0):
    from segmif_amd import ops
    off = ref.offsets_of(rec)
    patches = torch.full((int(off[-1]) + GUARD, 8), 0xAB, dtype=torch.uint8, device="cuda")
    ops.object_pack(torch.from_numpy(rec).cuda(), torch.from_numpy(off).cuda(), patches[:int(off[-1])], root, *(torch.from_numpy(a).cuda() for a in (ir, vis, mask)),
                    frame0=frame0)
    got = patches.cpu().numpy()
    assert (got[int(off[-1]):] == 0xAB).all()  # nothing behind the store was written
    return off, got[:int(off[-1])]


# ---- boxes and pack ---------------------------------------------------------------------------------------------------------------------

def combs():
    """two interlocking combs of one class under 4-connectivity: each box holds pixels of the other"""
    label = np.zeros((1, 9, 12), dtype=np.int64)
    label[0, 0, :11] = 3
    label[0, 0:6, 0:11:4] = 3
    label[0, 8, 1:] = 3
    label[0, 3:9, 2:12:4] = 3
    return dict(label=label, K=9)


BANK_CASES = [("1x1", 8), ("1x9", 8), ("9x1", 4), ("7x5", 8), ("64x64", 8), ("65x129", 8), ("65x129", 4), ("serpentine_130", 8), ("checkerboard_66", 4),
              ("combs", 4), ("constant_130", 8), ("all_ign", 8), ("blocky_K1", 8), ("blocky_K9", 4), ("blocky_K32", 8), ("odd_labels", 8)]


def bank_case(name, conn):
    c = combs() if name == "combs" else objects_ref.case(name, conn)
    label = _u8_label(c["label"], c["K"])
    root = ref.roots_of(label, c["K"], conn) if name == "combs" else c["root_g"]
    return label, c["K"], root


@pytest.mark.parametrize("name,conn", BANK_CASES, ids=[f"{n}-{c}" for n, c in BANK_CASES])
def test_boxes_and_pack_equal_the_restatement(data, name, conn):
    label, K, root = bank_case(name, conn)
    want = ref.boxes(root, label, K, ALL, 1, 1 << 40)
    count, got, behind, root_d = device_boxes(label, K, conn)
    assert np.array_equal(root_d.cpu().numpy(), root)
    assert count == len(want) and np.array_equal(got, want) and (behind == -7).all()
    expected_objects = {"1x1": 1, "checkerboard_66": 66 * 66, "constant_130": 1, "all_ign": 0}.get(name)
    if name == "serpentine_130":  # one component whose box is the frame, and the background's 65 strips
        snake = want[want[:, 2] == 1]
        assert len(snake) == 1 and snake[0, 4:].tolist() == [0, 0, 130, 130] and count == 66
    elif name == "combs":
        teeth = want[want[:, 2] == 3]
        assert len(teeth) == 2 and teeth[0, 4:].tolist() == [0, 0, 11, 6] and teeth[1, 4:].tolist() == [1, 3, 11, 6]
    elif expected_objects is not None:
        assert count == expected_objects
    if name == "checkerboard_66":
        assert (want[:, 3] == 1).all() and (want[:, 6:] == 1).all()
    if not count:
        return
    ir, vis, mask = _images(label.shape, 7)
    off, patches = device_pack(want, root_d, ir, vis, mask)
    expected = ref.pack(want, off, root, ir, vis, mask)
    assert np.array_equal(patches, expected)
    assert int(expected[:, 5].sum()) == int(want[:, 3].sum())  # alpha counts every object's area
    # two builds give equal bits
    count2, got2, _, root_d2 = device_boxes(label, K, conn)
    assert count2 == count and np.array_equal(got2, got) and np.array_equal(device_pack(got2, root_d2, ir, vis, mask)[1], patches)


def test_the_class_mask_drops_a_present_class_and_K_bounds_the_classes(data):
    label, K, root = bank_case("blocky_K9", 8)
    full = ref.boxes(root, label, K, ALL, 1, 1 << 40)
    present = sorted(set(full[:, 2].tolist()))
    assert len(present) >= 3
    for mask in (ALL & ~(1 << present[1]), 1 << present[0], 0):
        want = ref.boxes(root, label, K, mask, 1, 1 << 40)
        count, got, _, _ = device_boxes(label, K, 8, class_mask=mask)
        assert count == len(want) and np.array_equal(got, want)
        assert len(want) < len(full) and (mask == 0) == (len(want) == 0)
    assert present[1] not in ref.boxes(root, label, K, ALL & ~(1 << present[1]), 1, 1 << 40)[:, 2]


def test_min_area_and_max_box_at_an_objects_own_figures_and_one_past(data):
    label, K, root = bank_case("65x129", 8)
    full = ref.boxes(root, label, K, ALL, 1, 1 << 40)
    areas, boxes = np.unique(full[:, 3]), np.unique(full[:, 6] * full[:, 7])
    a, bx = int(areas[len(areas) // 2]), int(boxes[len(boxes) // 2])
    for kw in (dict(min_area=a), dict(min_area=a + 1), dict(max_box=bx), dict(max_box=bx - 1), dict(min_area=a, max_box=bx)):
        want = ref.boxes(root, label, K, ALL, kw.get("min_area", 1), kw.get("max_box", 1 << 40))
        count, got, _, _ = device_boxes(label, K, 8, **kw)
        assert count == len(want) and np.array_equal(got, want), kw
    at = lambda **kw: len(ref.boxes(root, label, K, ALL, kw.get("min_area", 1), kw.get("max_box", 1 << 40)))
    assert at(min_area=a) > at(min_area=a + 1) and at(max_box=bx) > at(max_box=bx - 1)  # the object itself is the difference


def test_two_chunks_with_frame0_equal_one_call(data):
    label, K, root = bank_case("blocky_K9", 8)
    assert len(label) == 2
    want = ref.boxes(root, label, K, ALL, 4, 400, frame0=5)
    one = device_boxes(label, K, 8, min_area=4, max_box=400, frame0=5)
    two = device_boxes(label, K, 8, min_area=4, max_box=400, frame0=5, chunks=[(0, 1), (1, 2)])
    assert one[0] == two[0] == len(want) and np.array_equal(one[1], want) and np.array_equal(two[1], want)
    assert set(want[:, 0].tolist()) == {5, 6}
    # and the pack of each chunk alone fills its objects' part of the store
    ir, vis, mask = _images(label.shape, 9)
    off = ref.offsets_of(want)
    expected = ref.pack(np.concatenate([want[:, :1] - 5, want[:, 1:]], axis=1), off, root, ir, vis, mask)
    from segmif_amd import ops
    patches = torch.zeros((int(off[-1]), 8), dtype=torch.uint8, device="cuda")
    rec_d, off_d = torch.from_numpy(want).cuda(), torch.from_numpy(off).cuda()
    for f in (0, 1):
        m0, m1 = (int(v) for v in np.searchsorted(want[:, 0], [5 + f, 6 + f]))
        ops.object_pack(rec_d[m0:m1], off_d[m0:m1 + 1], patches, one[3][f:f + 1], *(torch.from_numpy(a[f:f + 1]).cuda() for a in (ir, vis, mask)), frame0=5 + f)
    assert np.array_equal(patches.cpu().numpy(), expected)
    # a pack call skips the objects of other frames than its own
    untouched = torch.full((int(off[-1]), 8), 0x5A, dtype=torch.uint8, device="cuda")
    ops.object_pack(rec_d, off_d, untouched, one[3][:1], *(torch.from_numpy(a[:1]).cuda() for a in (ir, vis, mask)), frame0=5)
    got, first = untouched.cpu().numpy(), int(off[np.searchsorted(want[:, 0], 6)])
    assert np.array_equal(got[:first], expected[:first]) and (got[first:] == 0x5A).all()


def test_a_capacity_below_the_count(data):
    label, K, root = bank_case("checkerboard_66", 4)
    want = ref.boxes(root, label, K, ALL, 1, 1 << 40)
    count, got, behind, _ = device_boxes(label, K, 4, capacity=1000)
    assert count == 66 * 66 == len(want)                   # the counter holds the full count
    assert len(got) == 1000 and (behind == -7).all()       # nothing at or past the capacity was written
    expected = {tuple(r) for r in want.tolist()}
    rows = [tuple(r) for r in got.tolist()]
    assert len(set(rows)) == 1000 and set(rows) <= expected  # distinct members of the expected set
    again = device_boxes(label, K, 4, capacity=count)
    assert again[0] == count and np.array_equal(again[1], want)
    none = device_boxes(label, K, 4, capacity=0)
    assert none[0] == count and len(none[1]) == 0 and (none[2] == -7).all()


# ---- paste --------------------------------------------------------------------------------------------------------------------------------

def _paste_frames():
    """two 40 x 72 frames: a blob with a hole, a ONE-PIXEL object, a bar 38 rows tall, a wide thin bar, two touching classes, and a
    seeded blocky frame"""
    label = np.zeros((2, 40, 72), dtype=np.uint8)
    a = label[0]
    a[2:8, 3:12] = 1
    a[4, 6:9] = 0
    a[10, 20] = 2
    a[1:39, 30:33] = 3
    a[12:14, 36:70] = 4
    a[20:30, 40:50] = 5
    a[22:27, 50:58] = 6
    a[33:38, 3:8] = 1
    label[1] = objects_ref.blocky(1, 40, 72, 9, 33)[1][0]
    return label


@pytest.fixture(scope="module")
def bank(data):
    """a bank made by the RESTATEMENT (the paste tests do not depend on the device's boxes and pack) and uploaded"""
    label = _paste_frames()
    root = ref.roots_of(label, 9)
    rec = ref.boxes(root, label, 9, 0x1fe, 1, 1 << 40)
    off = ref.offsets_of(rec)
    ir, vis, mask = _images(label.shape, 11)
    patches = ref.pack(rec, off, root, ir, vis, mask)
    b = types.SimpleNamespace(rec=rec, off=off, pat=patches, records=torch.from_numpy(rec).cuda(), offsets=torch.from_numpy(off).cuda(),
                              patches=torch.from_numpy(patches).cuda())
    find = lambda cls, area=None: next(i for i, r in enumerate(rec) if r[0] == 0 and r[2] == cls and (area is None or r[3] == area))
    b.blob, b.dot, b.tall, b.wide, b.sq = find(1, 51), find(2), find(3), find(4), find(5)
    assert rec[b.dot, 3:].tolist() == [1, 20, 10, 1, 1] and rec[b.tall, 6:].tolist() == [3, 38] and rec[b.wide, 6:].tolist() == [34, 2]
    return b


def receiver(B, h, w, seed):
    """(ir3, vis3, mask3) as random bit patterns with -0.0, NaNs with payloads and an infinity planted, labels with 255, -1, 256 and
    2^40 + 3 planted"""
    rng = np.random.default_rng(seed)
    planes = [rng.integers(0, 2 ** 32, (B, 3, h, w), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    for p in planes:
        flat = p.reshape(B, -1)
        flat[:, 0], flat[:, 5], flat[:, 10], flat[:, 15] = 0x80000000, 0x7FC12345, 0xFFA00001, 0x7F800000
    label = rng.integers(0, 9, (B, h, w)).astype(np.int64)
    flat = label.reshape(B, -1)
    flat[:, 1], flat[:, 6], flat[:, 11], flat[:, 14] = ref.ODD_LABELS
    return [p.view(np.float32) for p in planes] + [label]


def check(bank, table, B, h, w, seed=0, tally=None, device_table=False):
    """ops.copy_paste on a seeded receiver against the restatement; -> (the device's outputs as arrays, the restatement's)"""
    from segmif_amd import ops
    table = np.asarray(table, dtype=np.int64).reshape(B, -1, 8)
    host = receiver(B, h, w, seed)
    dev = [torch.from_numpy(a).cuda() for a in host]
    before = [t.clone() for t in dev]
    tally_d = None if tally is None else torch.from_numpy(tally.copy()).cuda()
    arg = torch.from_numpy(table.astype(np.int32)).cuda() if device_table else table
    out = ops.copy_paste(*dev, bank, arg, 9, tally_d)
    assert len(out) == 5 and all(o.data_ptr() != t.data_ptr() for o, t in zip(out, dev))
    assert all(torch.equal(_t.view(torch.int32) if _t.is_floating_point() else _t, _b.view(torch.int32) if _b.is_floating_point() else _b)
               for _t, _b in zip(dev, before))  # the inputs are untouched
    want = ref.paste(*host, bank.rec, bank.off, bank.pat, table, 9, tally)
    got = [o.cpu().numpy() for o in out] + [None if tally is None else tally_d.cpu().numpy()]
    for g, e, what in zip(got[:4], want[:4], ("ir3", "vis3", "mask3", "label")):
        assert g.dtype == e.dtype and np.array_equal(_bits(g), _bits(e)), what
    assert got[4].dtype == np.int64 and np.array_equal(got[4], want[4])
    if tally is not None:
        assert np.array_equal(got[5], want[5])
    return got, want, host


EMPTY = (-1, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("B,h,w", [(1, 4, 4), (3, 4, 8), (1, 36, 68), (2, 12, 1028)])
def test_no_slot_and_empty_slots_only_are_a_bit_for_bit_copy(data, bank, B, h, w):
    for table in (np.zeros((B, 0, 8)), [[EMPTY] * 3] * B, [[(len(bank.rec), 0, 0, 4, 4, 65536, 65536, 0), (bank.blob, 0, 0, 0, 4, 65536, 65536, 0)]] * B):
        got, want, host = check(bank, table, B, h, w, seed=1, tally=np.arange(18, dtype=np.int64).reshape(9, 2))
        for g, e in zip(got[:4], host):
            assert np.array_equal(_bits(g), _bits(e))
        assert not got[4].any() and np.array_equal(got[5], np.arange(18).reshape(9, 2))
    odd = got[3].reshape(B, -1)[:, [1, 6, 11, 14]]
    assert (odd == np.asarray(ref.ODD_LABELS)).all()
    planted = _bits(got[0]).reshape(B, -1)[:, [0, 5, 10, 15]].view(np.uint32)
    assert (planted == np.asarray([0x80000000, 0x7FC12345, 0xFFA00001, 0x7F800000], dtype=np.uint32)).all()


def test_a_one_pixel_object_at_every_x_mod_4(data, bank):
    for h, w in ((4, 4), (8, 12), (36, 68)):
        table = [[(bank.dot, x, min(x, h - 1), 1, 1, 65536, 65536, x & 1) for x in range(4)] + [(bank.dot, w - 1 - x, h - 1 - (x & 1), 1, 1, 65536, 65536, 0) for x in range(4)]]
        got, want, host = check(bank, table, 1, h, w, seed=2, tally=np.zeros((9, 2), dtype=np.int64))
        assert got[4].tolist() == [len({(s[1], s[2]) for s in table[0]})] and got[5][2, 0] == 8
        changed = _bits(got[0])[0, 0] != _bits(host[0])[0, 0]
        assert changed.sum() <= got[4][0] and (got[3][0][changed] == 2).all()


SLOT_CASES = {
    # objects that straddle group boundaries, left, right, top and bottom edges, and one wholly outside
    "straddle": lambda b, h, w: [ref.slot(b.blob, 2, 1, 9, 6), ref.slot(b.blob, w - 3, 4, 9, 6), ref.slot(b.blob, -4, h - 2, 9, 6), ref.slot(b.wide, 3, -1, 34, 2)],
    "negative": lambda b, h, w: [ref.slot(b.blob, -5, -3, 9, 6), ref.slot(b.sq, -9, -9, 10, 10), ref.slot(b.sq, w - 1, h - 1, 10, 10)],
    "outside": lambda b, h, w: [ref.slot(b.blob, w, 0, 9, 6), ref.slot(b.blob, 0, h, 9, 6), ref.slot(b.blob, -9, 0, 9, 6), ref.slot(b.blob, 0, -6, 9, 6),
                                ref.slot(b.blob, -2 ** 31, 2 ** 31 - 1, 9, 6)],
    "flip": lambda b, h, w: [ref.slot(b.blob, 1, 1, 9, 6, flip=1), ref.slot(b.wide, -7, h - 3, 34, 2, flip=1), ref.slot(b.blob, w - 12, 9, 9, 6, flip=3)],
    "scales": lambda b, h, w: [ref.slot(b.blob, 0, 0, 9, 6, 0.5), ref.slot(b.blob, 9, 2, 9, 6, 1.0), ref.slot(b.blob, 20, 3, 9, 6, 2.0, flip=1),
                               ref.slot(b.blob, 41, 15, 9, 6, 1.37), ref.slot(b.sq, 3, 18, 10, 10, 1.37), ref.slot(b.dot, 30, 20, 1, 1, 2.0)],
    "tall": lambda b, h, w: [ref.slot(b.tall, 5, -1, 3, 38), ref.slot(b.tall, 13, 0, 3, 38, 2.0), ref.slot(b.tall, w - 2, -20, 3, 38, 1.37, flip=1)],
    "overlap": lambda b, h, w: [ref.slot(b.sq, 2, 2, 10, 10, 2.0), ref.slot(b.blob, 6, 5, 9, 6, 2.0), ref.slot(b.wide, 0, 9, 34, 2)],
}


@pytest.mark.parametrize("name", sorted(SLOT_CASES))
@pytest.mark.parametrize("h,w", [(4, 4), (20, 24), (36, 68)])
def test_slots_equal_the_restatement(data, bank, name, h, w):
    slots = SLOT_CASES[name](bank, h, w)
    got, want, host = check(bank, [slots], 1, h, w, seed=3, tally=np.zeros((9, 2), dtype=np.int64))
    if name == "outside":
        assert got[4].tolist() == [0] and all(np.array_equal(_bits(g), _bits(e)) for g, e in zip(got[:4], host))
        assert got[5][1].tolist() == [5, 0]  # drawn, not visible
    elif (h, w) == (36, 68):
        assert got[4][0] > 0
    if name == "overlap" and (h, w) == (36, 68):
        # the last slot wins wherever ITS alpha is set, and only there: every slot alone, then layered by hand
        alone = [check(bank, [[s]], 1, h, w, seed=3)[0] for s in slots]
        layered = [np.array(a, copy=True) for a in host]
        for one in alone:
            took = np.zeros((h, w), dtype=bool)
            for g, e in zip(one[:4], host):
                diff = _bits(g)[0] != _bits(e)[0]
                took |= diff if diff.ndim == 2 else diff.any(axis=0)
            for k in range(3):
                layered[k][0][:, took] = one[k][0][:, took]
            layered[3][0][took] = one[3][0][took]
        # (a pasted value can equal the receiver's by chance in one tensor, not in all four at once with random bits underneath)
        for g, e in zip(got[:4], layered):
            assert np.array_equal(_bits(g), _bits(e))


def test_eight_slots_and_batches(data, bank):
    rng = np.random.default_rng(5)
    M = len(bank.rec)

    def random_table(B, P, h, w):
        t = np.zeros((B, P, 8), dtype=np.int64)
        for b in range(B):
            for s in range(P):
                obj = int(rng.integers(0, M))
                t[b, s] = ref.slot(obj, int(rng.integers(-20, w + 5)), int(rng.integers(-20, h + 5)), int(bank.rec[obj, 6]), int(bank.rec[obj, 7]),
                                   float(np.exp(rng.uniform(np.log(0.4), np.log(2.5)))), int(rng.integers(0, 2)))
        return t
    for B, P, h, w in ((1, 8, 36, 68), (3, 8, 36, 68), (3, 5, 20, 24), (2, 8, 4, 4)):
        table = random_table(B, P, h, w)
        tally = np.arange(18, dtype=np.int64).reshape(9, 2)
        got, want, host = check(bank, table, B, h, w, seed=6, tally=tally)
        assert got[5][:, 0].sum() == tally[:, 0].sum() + B * P and got[5][:, 1].sum() == tally[:, 1].sum() + got[4].sum()
        if B == 3:  # a sample alone equals its share of the batch
            from segmif_amd import ops
            dev = [torch.from_numpy(a[1:2].copy()).cuda() for a in host]
            alone = ops.copy_paste(*dev, bank, table[1:2], 9)
            for a, g in zip(alone, got[:5]):
                assert np.array_equal(_bits(a), _bits(g[1:2]))
        # two runs give equal bits; and a table that already lives on the device
        again = check(bank, table, B, h, w, seed=6, tally=tally, device_table=True)[0]
        assert all(np.array_equal(_bits(a), _bits(g)) for a, g in zip(again, got))


BAD = [("obj", "M"), ("obj", -2), ("obj", 2 ** 30), ("ow", 0), ("ow", 4097), ("oh", 0), ("oh", 4097), ("ow", -5), ("sx", 0), ("sx", 2 ** 24 + 1),
       ("sy", 0), ("sy", 2 ** 24 + 1), ("sx", -65536), ("obj", -2 ** 31), ("ow", 2 ** 31 - 1), ("sy", 2 ** 31 - 1)]


@pytest.mark.parametrize("field,value", BAD, ids=[f"{f}={v}" for f, v in BAD])
def test_a_slot_outside_the_domain_is_an_empty_slot(data, bank, field, value):
    good = ref.slot(bank.blob, 3, 2, 9, 6, 2.0)
    bad = list(ref.slot(bank.sq, 1, 1, 10, 10, 1.37))
    bad[("obj", "dx", "dy", "ow", "oh", "sx", "sy", "flip").index(field)] = len(bank.rec) if value == "M" else value
    zero = np.zeros((9, 2), dtype=np.int64)
    for device_table in (False, True):
        got, want, _ = check(bank, [[good, tuple(bad)], [tuple(bad), EMPTY]], 2, 20, 24, seed=8, tally=zero, device_table=device_table)
        only, _, host = check(bank, [[good, EMPTY], [EMPTY, EMPTY]], 2, 20, 24, seed=8, tally=zero)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, only))
        assert got[4][1] == 0 and got[5][:, 0].sum() == 1
    assert ref.slot_is_empty(bad, bank.rec, bank.off, len(bank.pat)) and not ref.slot_is_empty(good, bank.rec, bank.off, len(bank.pat))


def test_two_calls_into_one_tally_and_the_wrappers_checks(data, bank):
    from segmif_amd import ops
    t1, t2 = [[ref.slot(bank.blob, 2, 1, 9, 6), ref.slot(bank.sq, 8, 8, 10, 10)]], [[ref.slot(bank.tall, 0, 0, 3, 38), EMPTY]]
    first = check(bank, t1, 1, 20, 24, seed=9, tally=np.zeros((9, 2), dtype=np.int64))[0][5]
    second = check(bank, t2, 1, 20, 24, seed=9, tally=first)[0][5]
    assert second[:, 0].tolist() == [0, 1, 0, 1, 0, 1, 0, 0, 0] and second[1, 1] == 51 and second[3, 1] == 60 and second[5, 1] == 100
    host = receiver(1, 8, 8, 0)
    dev = [torch.from_numpy(a).cuda() for a in host]
    none = np.zeros((1, 0, 8), dtype=np.int32)
    with pytest.raises(ValueError):
        ops.copy_paste(*dev, bank, np.zeros((1, 9, 8), dtype=np.int32))       # P > 8, a host table
    with pytest.raises(RuntimeError):
        ops.copy_paste(*dev, bank, torch.zeros((1, 9, 8), dtype=torch.int32, device="cuda"))  # and one on the device
    with pytest.raises(RuntimeError):
        ops.copy_paste(*(t[..., :6].contiguous() for t in dev), bank, none)    # w % 4
    with pytest.raises(RuntimeError):
        ops.copy_paste(dev[0].double(), *dev[1:], bank, none)
    with pytest.raises(RuntimeError):
        ops.copy_paste(dev[0].cpu(), *dev[1:], bank, none)
    with pytest.raises(RuntimeError):
        ops.copy_paste(*dev[:3], dev[3].int(), bank, none)
    with pytest.raises(RuntimeError):
        ops.copy_paste(*dev, bank, none, tally=torch.zeros((8, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.copy_paste(*dev, types.SimpleNamespace(records=bank.records, offsets=bank.offsets[:-1].contiguous(), patches=bank.patches), none)
    with pytest.raises(ValueError):
        ops.copy_paste(*dev, bank, none, n_class=0)


# ---- the bank and the iterator ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frames(data):
    src = data.synthetic_pairs(10, 96, 128, seed=27)
    return src, data.DeviceDataset.from_arrays(**src)


@pytest.fixture(scope="module")
def frames_ref(frames):
    """the restatement's bank of the synthetic frames, classes 1..8, min_area 16, max_box H * W // 4"""
    src, _ = frames
    root = ref.roots_of(src["label"], 9)
    rec = ref.boxes(root, src["label"], 9, 0x1fe, 16, 96 * 128 // 4)
    off = ref.offsets_of(rec)
    return root, rec, off, ref.pack(rec, off, root, src["ir"], src["vis"], src["mask"])


def test_object_bank_equals_the_restatement(data, frames, frames_ref):
    src, ds = frames
    root, rec, off, patches = frames_ref
    bank = data.ObjectBank.build(ds, min_area=16)
    assert len(bank) == len(rec) > 10 and bank.n_class == 9 and bank.shape == (96, 128)
    assert np.array_equal(bank.records_host, rec) and np.array_equal(bank.offsets_host, off)
    assert np.array_equal(bank.records.cpu().numpy(), rec) and np.array_equal(bank.offsets.cpu().numpy(), off)
    assert np.array_equal(bank.patches.cpu().numpy(), patches)
    assert sorted(bank.by_class) == sorted(set(rec[:, 2].tolist())) and 0 not in bank.by_class
    assert all(np.array_equal(bank.by_class[c], np.flatnonzero(rec[:, 2] == c)) for c in bank.by_class)
    rows = bank.table()
    assert len(rows) == 1 + len(bank.by_class) and f"of {len(rec)} objects" in rows[0]
    assert [int(r.split()[1]) for r in rows[1:]] == [len(bank.by_class[c]) for c in sorted(bank.by_class)]
    # chunks of one frame, a second build, and a subset of frames that is not one run
    tiny = data.ObjectBank.build(ds, min_area=16, max_workspace_bytes=1)
    assert np.array_equal(tiny.records_host, rec) and np.array_equal(tiny.patches.cpu().numpy(), patches)
    some = data.ObjectBank.build(ds, min_area=16, frames=[7, 0, 1, 4])
    keep = np.isin(rec[:, 0], [0, 1, 4, 7])
    assert np.array_equal(some.records_host, rec[keep])
    assert np.array_equal(some.patches.cpu().numpy(), ref.pack(rec[keep], ref.offsets_of(rec[keep]), root, src["ir"], src["vis"], src["mask"]))
    # classes, the thinning of a class, the two refusals
    c = sorted(bank.by_class)[0]
    two = data.ObjectBank.build(ds, min_area=16, classes=[0, c])  # class 0 is banked when it is asked for
    assert np.array_equal(two.records_host, ref.boxes(root, src["label"], 9, 1 | (1 << c), 16, 96 * 128 // 4)) and c in two.by_class
    thin = data.ObjectBank.build(ds, min_area=16, max_per_class=2)
    for c, idx in bank.by_class.items():
        step = -(-len(idx) // 2)
        assert np.array_equal(thin.records_host[thin.by_class[c]], rec[idx[::step]]) and len(thin.by_class[c]) <= 2
    with pytest.raises(ValueError, match="max_bytes 64.*min_area.*max_box.*max_per_class"):
        data.ObjectBank.build(ds, min_area=16, max_bytes=64)
    with pytest.raises(ValueError, match="nothing to paste"):
        data.ObjectBank.build(ds, min_area=96 * 128)
    for bad in (dict(n_class=33), dict(classes=[9]), dict(classes=[]), dict(frames=[10]), dict(min_area=0), dict(max_per_class=0)):
        with pytest.raises(ValueError, match="ObjectBank"):
            data.ObjectBank.build(ds, **bad)


def _check_iterators(pasting, twin, rec, off, patches, steps=2):
    total = np.zeros((9, 2), dtype=np.int64)
    pasted_any = 0
    for _ in range(steps):
        names, ir3, vis3, mask3, label = next(pasting)
        t_names, t_ir3, t_vis3, t_mask3, t_label = next(twin)
        assert names == t_names
        plain = [{k: v for k, v in p.items() if k != "paste"} for p in pasting.last_params]
        assert repr(plain) == repr(twin.last_params)  # the crops (and the mix) underneath are the ones the same seed gives without pasting
        table = np.asarray([p["paste"] for p in pasting.last_params], dtype=np.int64)
        assert table.shape == (len(names), 3, 8) and (table[:, 0, 0] >= 0).all()  # prob = 1
        want = ref.paste(*(t.cpu().numpy() for t in (t_ir3, t_vis3, t_mask3, t_label)), rec, off, patches, table, 9, total)
        for t, e in zip((ir3, vis3, mask3, label), want[:4]):
            assert np.array_equal(_bits(t), _bits(e))
        total = want[5]
        pasted_any += int(want[4].sum())
        assert np.array_equal(pasting.paste_tally(), total)
    assert pasted_any > 0


def test_pasting_iterator_equals_the_restatement_on_its_twin(data, frames, frames_ref):
    src, ds = frames
    _, rec, off, patches = frames_ref
    bank = data.ObjectBank.build(ds, min_area=16)
    _check_iterators(data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3, paste=data.CopyPaste(bank, prob=1.0, seed=3)),
                     data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3), rec, off, patches)
    # with mix= as well: the paste comes after the mix
    _check_iterators(data.AugmentedBatches(ds, batch=4, crop_size=64, seed=4, mix=data.ClassMix(prob=1.0, seed=4), paste=data.CopyPaste(bank, prob=1.0, seed=9)),
                     data.AugmentedBatches(ds, batch=4, crop_size=64, seed=4, mix=data.ClassMix(prob=1.0, seed=4)), rec, off, patches)
    stats = ds.label_stats()
    sampler = lambda: data.RareClassSampler(stats, range(10), min_pixels=200, fraction=0.75, seed=5)
    _check_iterators(data.AugmentedBatches(ds, batch=2, crop_size=64, seed=3, sampler=sampler(), paste=data.CopyPaste(bank, prob=1.0, stats=stats, seed=1)),
                     data.AugmentedBatches(ds, batch=2, crop_size=64, seed=3, sampler=sampler()), rec, off, patches, steps=1)
    for kw in (dict(aug=False, paste=data.CopyPaste(bank)), dict(paste=data.CopyPaste(bank, rank=1))):
        with pytest.raises(ValueError, match="paste"):
            data.AugmentedBatches(ds, batch=4, crop_size=64, **kw)
    with pytest.raises(RuntimeError):
        data.AugmentedBatches(ds, batch=4, crop_size=64).paste_tally()


def test_train_command_line_with_copy_paste(data, tmp_path):
    """python -m segmif_amd.train in a fresh child process: two iterations per phase on synthetic frames, pasting in both phases"""
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "16", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2",
           "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", str(tmp_path),
           "--copy-paste", "--copy-paste-prob", "1.0", "--copy-paste-min-area", "16", "--copy-paste-phases", "both", "--copy-paste-temperature", "0.5"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    announced = [ln for ln in lines if ln.startswith("[train] --copy-paste (")]
    assert len(announced) == 1 and "NOT the reference's loader" in announced[0] and "phases seg, fusion)" in announced[0]
    assert len([ln for ln in lines if ln.startswith("[train] --copy-paste: the object bank of the ")]) == 2  # once per phase's set
    assert any(" objects, " in ln and "bytes on the device" in ln for ln in lines)
    for phase in ("fusion", "segmentation"):
        logged = [ln for ln in lines if f"{phase} iter 2/2" in ln]
        assert len(logged) == 1 and " paste obj/px " in logged[0]
        pairs = [f.split(":")[1].split("/") for f in logged[0].split(" paste obj/px ")[1].split()]
        assert sum(int(n) for n, _ in pairs) >= 4 and all(int(n) >= 1 and int(px) >= 0 for n, px in pairs)  # 2 iterations of batch 2, prob 1
        assert 0 < sum(int(px) for _, px in pairs) <= 4 * 64 * 64
    assert sorted(os.listdir(tmp_path)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    for f in os.listdir(tmp_path):
        sd = torch.load(tmp_path / f, map_location="cpu")
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
