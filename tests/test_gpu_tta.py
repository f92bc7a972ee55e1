"""GPU tests of multi-scale + flip inference: the vote kernel and the one-pass view resize against tests/_tta_ref.py (float64),
Network3.predict_labels_tta through a cheap stand-in network and through mit_b0, PairForward / Evaluator with tta=.

Bounds.  Probabilities: E = 4 x the error of torch's own float32 evaluation of the same formulas against float64 on the same
inputs, computed here (the factor 4: the kernel's interpolation weights and expf may round differently from aten's).  Labels:
equal wherever the float64 top-2 margin exceeds 1e-4 (about 50 x that error class), and at most 0.5 % of the pixels may be
excluded by it."""
import json

import pytest
import torch
import torch.nn.functional as F

import _tta_ref as ref
import detweights as dw

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
MAX_EXCLUDED = 0.005
TOL = 2e-5  # test_gpu_kernels.py's gate for segmif_bilinear_nhwc_f32 (the same arithmetic): max error / max magnitude


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import ops as _ops
    return _ops


# ---- 1. the vote kernel -----------------------------------------------------------------------------------------------------

B, OH, OW = 2, 37, 53  # odd, not a multiple of the block
VIEWS = [(10, 14, 0), (10, 14, 1), (19, 27, 1), (5, 7, 0), (37, 53, 0), (56, 80, 1)]  # up-, same- and down-sampling
PITCHED = 2  # this view is a rows view with ldx = 16 (C = 9) / 32 (C = 19) > C


def make_views(C):
    g = torch.Generator().manual_seed(100 + C)
    return [3.0 * torch.randn(B, ih, iw, C, generator=g, dtype=torch.float64) for ih, iw, _ in VIEWS]


def on_device(views64, C):
    out = []
    for i, v in enumerate(views64):
        if i == PITCHED:
            wide = torch.full(v.shape[:3] + (16 if C <= 16 else 32,), float("nan"), device="cuda")
            wide[..., :C] = v.float().cuda()
            out.append(wide[..., :C])
        else:
            out.append(v.float().cuda())
    return out


@pytest.fixture(scope="module", params=[9, 19], ids=["C9", "C19"])
def case(request):
    C = request.param
    views64 = make_views(C)
    flips = [f for _, _, f in VIEWS]
    views32 = [v.float() for v in views64]
    want = ref.vote([v.double() for v in views32], flips, OH, OW)  # float64 on exactly the float32 inputs the kernel reads
    torch32 = ref.vote(views32, flips, OH, OW)
    return C, views32, flips, want, float((torch32.double() - want).abs().max()), torch32


def test_vote_against_float64(ops, case):
    C, views32, flips, want, e32, torch32 = case
    dev = on_device([v.double() for v in views32], C)
    assert dev[PITCHED].stride(2) > C
    labels, probs = ops.tta_vote(dev, flips, OH, OW, want_probs=True)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (B, OH, OW) and tuple(probs.shape) == (B, OH, OW, C)
    err = float((probs.double().cpu() - want).abs().max())
    margin = ref.top2_margin(want)
    stable = margin > MARGIN
    excluded = 1.0 - float(stable.float().mean())
    mism = int((labels.cpu().long()[stable] != want.argmax(3)[stable]).sum())
    mism32 = int((torch32.argmax(3)[stable] != want.argmax(3)[stable]).sum())
    print(f"tta_vote C={C}: max |probs - float64| {err:.3e}; torch float32 yardstick {e32:.3e} (bound {4 * e32:.3e}); "
          f"excluded at margin {MARGIN:g}: {100 * excluded:.3f} %; label mismatches {mism} (torch float32: {mism32})")
    assert err <= 4 * e32
    assert excluded <= MAX_EXCLUDED
    assert mism == 0
    assert float((probs.sum(3) - 1).abs().max()) < 1e-5


def test_vote_labels_do_not_depend_on_probs_or_on_the_batch(ops, case):
    C, views32, flips, _, _, _ = case
    dev = on_device([v.double() for v in views32], C)
    with_probs = ops.tta_vote(dev, flips, OH, OW, want_probs=True)[0]
    alone = ops.tta_vote(dev, flips, OH, OW)
    assert torch.equal(alone, with_probs)
    one = ops.tta_vote([v[1:2] for v in dev], flips, OH, OW)
    assert tuple(one.shape) == (1, OH, OW) and torch.equal(one[0], alone[1])
    assert torch.equal(ops.tta_vote(dev, flips, OH, OW), alone)  # bitwise reproducible


def test_vote_of_one_plain_view_is_bilinear_argmax(ops, case):
    """softmax is monotone, so a single unmirrored view votes for the resize's own argmax wherever that is decided."""
    C, views32, _, _, _, _ = case
    x = views32[0].cuda()
    up = F.interpolate(views32[0].double().permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False)
    top = up.topk(2, dim=1).values
    stable = (top[:, 0] - top[:, 1]) > 1e-3
    got, plain = ops.tta_vote([x], [False], OH, OW).cpu(), ops.bilinear_argmax(x, OH, OW).cpu()
    assert stable.float().mean() > 0.99 and torch.equal(got[stable], plain[stable])


def test_vote_rejects(ops):
    x = torch.zeros(1, 4, 4, 9, device="cuda")
    with pytest.raises(RuntimeError):
        ops.tta_vote([], [], 8, 8)
    with pytest.raises(RuntimeError):
        ops.tta_vote([x] * 17, [False] * 17, 8, 8)
    with pytest.raises(RuntimeError):
        ops.tta_vote([x, x], [False], 8, 8)
    with pytest.raises(RuntimeError):
        ops.tta_vote([x, torch.zeros(1, 4, 4, 8, device="cuda")], [False, False], 8, 8)
    with pytest.raises(RuntimeError):
        ops.tta_vote([torch.zeros(1, 4, 4, 33, device="cuda")], [False], 8, 8)
    with pytest.raises(RuntimeError):
        ops.tta_vote([x.cpu()], [False], 8, 8)


# ---- 2. the one-pass view resize --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flip", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("oh,ow", [(48, 72), (96, 144), (45, 67)])
def test_resize_flip_nchw(ops, oh, ow, flip):
    g = torch.Generator().manual_seed(7)
    x = torch.rand(2, 3, 64, 96, generator=g).cuda()
    want = ref.resize_flip(x.double(), oh, ow, flip)
    got = ops.resize_flip_nchw(x, oh, ow, flip)
    assert tuple(got.shape) == (2, 3, oh, ow) and got.is_contiguous()
    assert float((got.double() - want).abs().max() / want.abs().max()) < TOL


# ---- 3. the composition, through a stand-in network -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stand_in():
    g = torch.Generator().manual_seed(11)
    weight = 20.0 * torch.randn(9, 3, generator=g, dtype=torch.float64)
    field = torch.rand(2, 3, 8, 12, generator=g, dtype=torch.float64)
    fused = F.interpolate(field, size=(64, 96), mode="bicubic", align_corners=False) + 0.1 * torch.rand(2, 3, 64, 96, generator=g, dtype=torch.float64)
    return weight, fused.clamp(0, 1).float()


@pytest.fixture(scope="module")
def b0(ops):
    import segmif_amd.core as core
    seg = core.Network3("mit_b0", 9, pretrained=None)
    dw.load_det_weights(seg, seed=0)
    return seg.cuda().eval()


def test_predict_labels_tta_through_a_stand_in(ops, b0, stand_in):
    from segmif_amd.tta import TTA
    weight, fused = stand_in
    tta = TTA((0.75, 1.0, 1.5), True)
    plan = tta.plan(64, 96)
    assert plan == [(48, 72, False), (48, 72, True), (64, 96, False), (64, 96, True), (96, 144, False), (96, 144, True)]
    want = ref.chain(fused.double(), plan, ref.stand_in_segment(weight), 64, 96)
    segment = ref.stand_in_segment(weight.float())
    with torch.no_grad():
        labels = b0.predict_labels_tta(fused.cuda(), tta=tta, segment=segment)
        labels2, probs = b0.predict_labels_tta(fused.cuda(), tta=tta, segment=segment, return_probs=True)
        single = ops.bilinear_argmax(segment(fused.cuda()), 64, 96)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (2, 64, 96) and torch.equal(labels, labels2)
    stable = ref.top2_margin(want) > MARGIN
    excluded = 1.0 - float(stable.float().mean())
    mism = int((labels.cpu().long()[stable] != want.argmax(3)[stable]).sum())
    moved = float((labels != single).float().mean())
    print(f"stand-in chain: excluded at margin {MARGIN:g}: {100 * excluded:.3f} %; label mismatches {mism} of {labels.numel()}; "
          f"classes {want.argmax(3).unique().numel()}; voted != single view on {100 * moved:.2f} % of pixels; "
          f"max |probs - float64| {float((probs.double().cpu() - want).abs().max()):.3e}")
    assert excluded <= MAX_EXCLUDED
    assert mism == 0
    assert moved > 0  # (an implementation that ignored the views would return the single view's labels)


def test_predict_labels_tta_raises_under_grad(b0, stand_in):
    with pytest.raises(RuntimeError):
        b0.predict_labels_tta(stand_in[1].cuda())


# ---- 4. the real network ----------------------------------------------------------------------------------------------------

def test_predict_labels_tta_on_mit_b0(b0):
    from segmif_amd.tta import TTA
    fused = dw.det_input("tta_fused", (2, 3, 64, 96)).cuda()
    with torch.no_grad():
        plain = b0.predict_labels(fused)
        assert torch.equal(b0.predict_labels_tta(fused, tta=TTA((1.0,), False)), plain)
        voted = b0.predict_labels_tta(fused, tta=TTA((0.75, 1.0, 1.5), True))
        sized = b0.predict_labels_tta(fused, (32, 48), TTA((1.0,), True))
    assert voted.dtype == torch.int32 and tuple(voted.shape) == (2, 64, 96)
    assert int(voted.min()) >= 0 and int(voted.max()) < 9
    assert tuple(sized.shape) == (2, 32, 48)


@pytest.fixture(scope="module")
def pair_nets(ops):
    """(mit_b1: the fusion network takes 64 / 128-channel segmentation features, which mit_b0 does not have)"""
    import segmif_amd.core as core
    seg, fus = core.Network3("mit_b1", 9, pretrained=None), core.Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0), dw.load_det_weights(fus, seed=0)
    return seg.cuda().eval(), fus.cuda().eval()


def test_pair_forward_and_evaluator_with_tta(pair_nets):
    from segmif_amd.evaluate import Evaluator
    from segmif_amd.pipeline import PairForward
    from segmif_amd.tta import TTA
    tta = TTA((0.75, 1.0, 1.5), True)
    ir = dw.det_input("tta_ir", (2, 1, 64, 96)).cuda()
    vis = dw.det_input("tta_vis", (2, 3, 64, 96)).cuda()
    mask3 = dw.det_input("tta_mask", (2, 1, 64, 96)).repeat(1, 3, 1, 1).cuda()
    fused0, labels0 = PairForward(*pair_nets)(ir, vis, mask3)
    pf = PairForward(*pair_nets, tta=tta)
    fused1, labels1 = pf(ir, vis, mask3)
    assert torch.equal(fused1, fused0)
    assert labels1.dtype == torch.int32 and labels1.shape == labels0.shape and int(labels1.min()) >= 0 and int(labels1.max()) < 9
    with torch.no_grad():
        assert torch.equal(labels1, pair_nets[0].predict_labels_tta(fused0, vis.shape[2:], tta))
    with pytest.raises(NotImplementedError):
        pf.capture(ir, vis, mask3)

    q = lambda t: (255 * t).to(torch.uint8)
    ir_u8, vis_u8, mask_u8 = q(ir[:, 0]).contiguous(), q(vis.permute(0, 2, 3, 1)).contiguous(), q(mask3[:, 0]).contiguous()
    label = dw.det_labels("tta_gt", (2, 64, 96), 9).cuda()
    docs = {}
    for name, t in (("tta", tta), ("plain", None)):
        ev = Evaluator(*pair_nets, tta=t)
        fused_u8, labels = ev.update(ir_u8, vis_u8, mask_u8, label=label)
        assert 0.0 <= ev.results()["mIoU"] <= 1.0
        docs[name] = (json.loads(json.dumps(ev.document(["a", "b"], []))), fused_u8)
    assert "tta" not in docs["plain"][0]
    assert docs["tta"][0]["tta"] == {"scales": [0.75, 1.0, 1.5], "flip": True, "size_divisor": 8,
                                     "views": [[h, w, f] for h, w in ((48, 72), (64, 96), (96, 144)) for f in (False, True)]}
    assert set(docs["tta"][0]) - {"tta"} == set(docs["plain"][0])
    assert torch.equal(docs["tta"][1], docs["plain"][1])  # the fused image does not depend on how the labels are voted
    with pytest.raises(NotImplementedError):
        Evaluator(*pair_nets, graph=True, tta=tta)
