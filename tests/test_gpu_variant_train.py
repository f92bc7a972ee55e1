"""GPU tests of the ablation variants' training path (segmif_amd/core/variants.py in train mode with gradients wanted):
  * the linear-attention fold backward at every head geometry (segmif_linattn_fold_bwd_f32) and the SiLU backward
    (segmif_pointwise2_bwd_f32) against float64 torch autograd;
  * every trainable variant class - forward, parameter and input gradients - against float64 CPU autograd through the oracle's
    restatements (pinned to the real reference's forward records by tests/test_oracle_golden.py);
  * the contract: train mode under torch.no_grad() is the inference path bit for bit, eval mode with gradients wanted raises;
  * FusionTrainer driving three variant nets.
Observed figures are recorded through tests/_observed.py."""
import numpy as np
import pytest
import torch

import detweights as dw
import segmif_oracle as so
from _observed import observed

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4   # the bar of test_gpu_backward.py::test_fusion_network_gradients_match_oracle_autograd for _ac's training path
GRAD_TOL = 1e-3
# the cross-attention kv weights and the channel_proj halves feeding them pass through a saturated context softmax (the bar
# test_gpu_round3.py sets for those gradients)
CTX_GRAD_TOL = 5e-3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import ops as o
    return o


def rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu()) if torch.is_tensor(a) else a).double()
    b = torch.as_tensor(np.asarray(b.detach().cpu()) if torch.is_tensor(b) else b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _flat(res):
    if torch.is_tensor(res):
        return [res]
    return [t for r in res for t in _flat(r)]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. fold backward at every head geometry
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("heads,d", [(8, 2), (8, 4), (4, 8), (2, 8), (8, 8)])
def test_linattn_fold_bwd_generic_vs_fp64_autograd(ops, heads, d, halves):
    B, Nout = 2, 40
    C = heads * d
    K = C * halves
    scale = float(np.float32(d ** -0.5))  # (the C ABI takes the scale as a float, as the forward fold does)
    wend = rnd(Nout, K, seed=1)
    dweff = rnd(B, Nout, K, seed=2)
    worst_k = worst_w = 0.0
    for q in range(halves):
        ktv = rnd(B, heads, d, d, seed=10 + q, lo=-12.0, hi=12.0).double()  # saturating logits, as the context softmaxes see
        k = ktv.clone().requires_grad_(True)
        w = wend.double().requires_grad_(True)
        ctx = torch.softmax(k * scale, dim=-2)  # [b][h][i][j]
        wq = w[:, q * C:(q + 1) * C].reshape(Nout, heads, d)  # [n][h][j]
        weff_q = torch.einsum("bhij,nhj->bnhi", ctx, wq).reshape(B, Nout, C)
        (weff_q * dweff[:, :, q * C:(q + 1) * C].double()).sum().backward()
        dk = torch.empty((B, heads, d, d), device="cuda", dtype=torch.float64)
        part = torch.full((B, Nout, K), float("nan"), device="cuda")
        ops.linattn_fold_bwd(ktv.cuda(), wend.cuda(), dweff.cuda(), dk, part, q * C, q * C, scale, heads)
        torch.cuda.synchronize()
        ek = rel(dk, k.grad)
        ew = rel(part.sum(0)[:, q * C:(q + 1) * C], w.grad[:, q * C:(q + 1) * C])
        worst_k, worst_w = max(worst_k, ek), max(worst_w, ew)
        assert ek < 1e-10, (heads, d, q, ek)
        assert ew < 1e-6, (heads, d, q, ew)
        # only this fold's columns of dwend_part are written
        other = torch.cat([part[:, :, :q * C], part[:, :, (q + 1) * C:]], dim=-1)
        assert bool(torch.isnan(other).all())
    observed(f"fold_bwd_generic_dktv[{heads}x{d},{halves}]", worst_k)
    observed(f"fold_bwd_generic_dwend[{heads}x{d},{halves}]", worst_w)


def test_linattn_fold_bwd_generic_rejects_bad_geometry(ops):
    from segmif_amd import _lib
    t = torch.zeros(4096, device="cuda", dtype=torch.float64)
    f = torch.zeros(4096, device="cuda")
    lib = _lib.load()
    s = ops._stream()
    for heads, d in ((16, 8), (8, 9), (3, 2)):  # C > 64, d > 8, C % 16 != 0
        assert lib.segmif_linattn_fold_bwd_f32(t.data_ptr(), f.data_ptr(), 64, 0, f.data_ptr(), 64, 0, 1.0, t.data_ptr(),
                                               f.data_ptr(), 64, 1, 8, heads, d, s) != 0
    # a pitch too narrow for the fold's columns
    assert lib.segmif_linattn_fold_bwd_f32(t.data_ptr(), f.data_ptr(), 32, 16, f.data_ptr(), 64, 0, 1.0, t.data_ptr(),
                                           f.data_ptr(), 64, 1, 8, 8, 4, s) != 0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. SiLU backward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_pointwise2_bwd_vs_fp64(ops, mode):
    rows, C = 1001, 32  # odd row count
    abuf = rnd(rows, 48, seed=3, lo=-30.0, hi=30.0)  # |z| up to 30: saturated sigmoid
    bbuf = rnd(rows, 40, seed=4, lo=-30.0, hi=30.0)
    abuf[::7, 8:8 + C:5] = 0.0  # exact zeros
    bbuf[::5, 4:4 + C:3] = 0.0
    abuf[3, 8:12] = torch.tensor([88.0, -88.0, 1e-30, -1e-30])
    dybuf = rnd(rows, 36, seed=5)
    ad, bd, dyd = abuf.cuda(), bbuf.cuda(), dybuf.cuda()
    a, b, dy = ad[:, 8:8 + C], bd[:, 4:4 + C], dyd[:, :C]  # pitched views (ld > C)
    dabuf = torch.full((rows, 44), float("nan"), device="cuda")
    dbbuf = torch.full((rows, 52), float("nan"), device="cuda")
    da, db = ops.pointwise2_bwd(dy, a, b if mode == 1 else None, mode, da=dabuf[:, 4:4 + C], db=dbbuf[:, 16:16 + C] if mode == 1 else None)
    torch.cuda.synchronize()
    assert da.data_ptr() == dabuf[:, 4:].data_ptr()
    za = abuf[:, 8:8 + C].double().requires_grad_(True)
    zb = bbuf[:, 4:4 + C].double().requires_grad_(True)
    silu = lambda z: z * torch.sigmoid(z)
    y = silu(za) + silu(zb) if mode == 1 else silu(za)
    (y * dybuf[:, :C].double()).sum().backward()
    ea = rel(da, za.grad)
    assert ea < 1e-6, ea
    worst = ea
    if mode == 1:
        eb = rel(db, zb.grad)
        assert eb < 1e-6, eb
        worst = max(worst, eb)
        assert bool(torch.isnan(dbbuf[:, :16]).all()) and bool(torch.isnan(dbbuf[:, 16 + C:]).all())
    assert bool(torch.isfinite(da).all())
    assert bool(torch.isnan(dabuf[:, :4]).all()) and bool(torch.isnan(dabuf[:, 4 + C:]).all())  # nothing outside the views
    observed(f"pointwise2_bwd_vs_fp64[mode{mode}]", worst)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. every trainable class against float64 autograd through the oracle
# ------------------------------------------------------------------------------------------------------------------------------
NETS4 = ["Fusion_Network3", "Fusion_Network3_Con", "Fusion_Network3_Add", "Fusion_Network3_Average", "Fusion_Network3_S",
         "Fusion_Network3_M", "Fusion_Network3_obtainattention"]
NETS2 = ["Fusion_Network_rmseg", "Fusion_Network_rmseg_att"]
FFMS = {"FeatureFusionModule_SoAM": "z", "FeatureFusionModule_MoAM": "v", "FeatureFusionModule_ShowAttention": "zv"}
PATHS = {"CrossPath_M": "v", "CrossPath_S": "z", "CrossPath_showAttention": "zv"}
ALL = NETS4 + NETS2 + list(FFMS) + list(PATHS) + ["AttentionModule"]
# ill-conditioning probe: relative noise of one float32 rounding on every weight and input, a fixed set of draws
PROBE_EPS, PROBE_DRAWS = 1e-7, 8


def _variant_inputs():
    """The inputs tests/golden/variants.npz was recorded on (tests/test_gpu_round6.py::_variant_inputs)."""
    spec = {"ir": ("r6v_ir", (2, 1, 24, 40), 0.0), "vis": ("r6v_vis", (2, 3, 24, 40), 0.0), "out1": ("r6v_out1", (2, 64, 24, 40), -1.0),
            "out2": ("r6v_out2", (2, 128, 24, 40), -1.0), "x1": ("r6v_x1", (2, 32, 24, 40), -1.0), "x2": ("r6v_x2", (2, 32, 24, 40), -1.0),
            "x3": ("r6v_x3", (2, 32, 24, 40), -1.0)}
    return {k: dw.det_input(n, shp, lo=lo, hi=1.0) for k, (n, shp, lo) in spec.items()}


def _build(name):
    from segmif_amd.core import model_fusion as mf
    cls = getattr(mf, name)
    net = cls(32) if name in FFMS or name in PATHS else cls()
    sd = dw.load_det_weights(net, seed=0)
    return net.cuda(), sd


def _args(name, inp):
    """The forward's arguments for class `name` from a dict of NCHW inputs."""
    tok = lambda t: t.flatten(2).transpose(1, 2)
    if name in NETS4:
        return [inp["ir"], inp["vis"], inp["out1"], inp["out2"]]
    if name in NETS2:
        return [inp["ir"], inp["vis"]]
    if name in FFMS:
        return [inp["x1"], inp["x2"], inp["x3"]]
    if name in PATHS:
        return [tok(inp["x1"]), tok(inp["x2"]), tok(inp["x3"])]
    return [inp["x1"]]


def _oracle(name, sd, args):
    if name in NETS4 + NETS2:
        return so.fusion_variant(sd, name, *args)
    if name in FFMS:
        o1, o2 = so.ffm_variant({"ffm." + k: v for k, v in sd.items()}, "ffm", *args, FFMS[name])
        # (the reference hands back torch.tensor copies of its inputs: no gradient through them)
        return (o1, o2, [args[0].detach(), args[1].detach()]) if name.endswith("ShowAttention") else (o1, o2)
    if name in PATHS:
        return so.cross_path_variant({"cross." + k: v for k, v in sd.items()}, "cross", *args, PATHS[name],
                                     want_maps=name.endswith("Attention"))
    return so.attention_module({"att." + k: v for k, v in sd.items()}, "att", *args)


def _grad_tol(pname):
    return CTX_GRAD_TOL if (".kv" in pname or "channel_proj" in pname) else GRAD_TOL


def _oracle_grads(name, sd, inp, dtype):
    """(parameter gradients, input gradients, outputs) of the oracle evaluated in `dtype` under the fixed cotangents."""
    sdt = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    src = {k: v.to(dtype).requires_grad_(True) for k, v in inp.items()}
    ref = _flat(_oracle(name, sdt, _args(name, src)))
    cot = [rnd(*r.shape, seed=100 + i) for i, r in enumerate(ref)]
    sum(((r * g.to(dtype)).sum() for r, g in zip(ref, cot) if r.requires_grad)).backward()
    return {k: v.grad for k, v in sdt.items()}, {k: v.grad for k, v in src.items()}, ref, cot


def _fp64_spread(name, sd, inp, g64, gin64):
    """How far the float64 truth itself moves when every weight and input is perturbed by one float32 rounding (relative noise
    PROBE_EPS, PROBE_DRAWS fixed draws): key -> max relative change.  A tensor whose truth moves by ~1e-3 there is not determined
    to 1e-3 by any float32-class evaluation: a ReLU pre-activation or a saturated softmax logit sits within rounding of its
    switch point, and which side an implementation lands on is decided by rounding."""
    spread = {}
    for seed in range(PROBE_DRAWS):
        gen = torch.Generator().manual_seed(1000 + seed)
        noisy = lambda d: {k: v.double() * (1 + PROBE_EPS * (2 * torch.rand(v.shape, generator=gen, dtype=torch.float64) - 1))
                           for k, v in d.items()}
        g, gin, _, _ = _oracle_grads(name, noisy(sd), noisy(inp), torch.float64)
        for k, v in g64.items():
            if v is not None:
                spread[k] = max(spread.get(k, 0.0), rel(g[k], v))
        for k, v in gin64.items():
            if v is not None:
                spread["input:" + k] = max(spread.get("input:" + k, 0.0), rel(gin[k], v))
    return spread


@pytest.mark.parametrize("name", ALL)
def test_variant_training_gradients_vs_fp64_oracle(ops, name):
    """Train mode, gradients wanted: forward, every parameter gradient and every input gradient against float64 CPU autograd
    through the oracle, with a fixed random cotangent on every output (extras included); ffm2.* stays without gradient.
    A gradient may exceed its bar only where the float64 truth is ill-conditioned at these inputs (_fp64_spread): then it may
    differ from the truth by at most twice what one float32 rounding of the inputs and weights moves the truth itself."""
    net, sd = _build(name)
    net.train()
    inp = _variant_inputs()
    g64, gin64, ref, cot = _oracle_grads(name, sd, inp, torch.float64)
    srcd = {k: v.cuda().requires_grad_(True) for k, v in inp.items()}
    res = _flat(net(*_args(name, srcd)))
    assert len(res) == len(ref)
    fwd = 0.0
    for i, (a, b) in enumerate(zip(res, ref)):
        assert tuple(a.shape) == tuple(b.shape), (name, i)
        fwd = max(fwd, rel(a, b))
    observed(f"variant_train_fwd[{name}]", fwd)
    assert fwd < FWD_TOL, (name, fwd)
    sum((a * g.cuda()).sum() for a, g in zip(res, cot) if a.requires_grad).backward()
    torch.cuda.synchronize()
    spread = None
    errs, n = {}, 0
    for pname, p in net.named_parameters():
        if pname.startswith("ffm2."):
            assert p.grad is None, pname
            continue
        assert g64[pname] is not None and p.grad is not None, pname
        errs[pname] = (rel(p.grad, g64[pname]), _grad_tol(pname))
        n += 1
    assert n > 0
    for k, t in srcd.items():
        if gin64[k] is None:
            assert t.grad is None or float(t.grad.abs().max()) == 0.0, (name, k)
            continue
        errs["input:" + k] = (rel(t.grad, gin64[k]), GRAD_TOL)
    bad, conditioned = [], {}
    for key, (e, tol) in errs.items():
        if e < tol:
            continue
        if spread is None:
            spread = _fp64_spread(name, sd, inp, g64, gin64)
        if e <= 2 * spread[key]:
            conditioned[key] = (e, spread[key])
        else:
            bad.append((key, e, spread[key]))
    params = [e for k, (e, t) in errs.items() if not k.startswith("input:") and t < CTX_GRAD_TOL]
    ctxs = [e for k, (e, t) in errs.items() if t == CTX_GRAD_TOL]
    observed(f"variant_train_param_grad[{name}]", max(params))
    observed(f"variant_train_ctx_grad[{name}]", max(ctxs, default=0.0))
    observed(f"variant_train_input_grad[{name}]", max((e for k, (e, t) in errs.items() if k.startswith("input:")), default=0.0))
    if conditioned:
        observed(f"variant_train_conditioned[{name}]", {k: list(v) for k, v in conditioned.items()})
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the contract
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_variant_train_mode_contract(ops, name):
    """Train mode under torch.no_grad() = the eval inference result bit for bit; eval mode with gradients wanted raises
    NotImplementedError that names .train()."""
    net, _ = _build(name)
    args = [t.cuda() for t in _args(name, _variant_inputs())]
    net.train()
    with torch.no_grad():
        a = _flat(net(*args))
    net.eval()
    with torch.no_grad():
        b = _flat(net(*args))
    torch.cuda.synchronize()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y), name
    with pytest.raises(NotImplementedError, match=r"\.train\(\)"):
        net(*args)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. FusionTrainer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Fusion_Network3", "Fusion_Network3_Average", "Fusion_Network_rmseg"])
def test_fusion_trainer_trains_variant(ops, name, monkeypatch):
    """FusionTrainer (iter_ = 2) with a variant fusion net in train mode: three steps give finite losses, every fusion-net
    parameter but ffm2.* a finite gradient and a new value, the segmentation net no weight gradient; the rmseg net never runs the
    encoder."""
    from segmif_amd.core import Network3
    from segmif_amd.train import FusionTrainer
    seg = Network3("mit_b1", 9, pretrained=None)
    dw.load_det_weights(seg, seed=0)
    seg = seg.cuda().eval()
    fus, _ = _build(name)
    assert fus.training
    if name == "Fusion_Network_rmseg":
        def no_encoder(*a, **k):
            raise AssertionError("the rmseg net takes no segmentation features: the encoder must not run")
        monkeypatch.setattr(seg.denoise_net.encoder, "forward_fusion", no_encoder)
    before = {n: p.detach().clone() for n, p in fus.named_parameters()}
    opt = torch.optim.AdamW(fus.parameters(), lr=1e-4, weight_decay=0.0)
    tr = FusionTrainer(seg, fus, opt, torch.nn.CrossEntropyLoss(ignore_index=255), iter_=2)
    B, H, W = 2, 32, 48
    for st in range(3):
        ir3 = dw.det_input(f"vtr_ir{st}", (B, 1, H, W)).repeat(1, 3, 1, 1).cuda()
        vis3 = dw.det_input(f"vtr_vis{st}", (B, 3, H, W)).cuda()
        mask3 = dw.det_input(f"vtr_mask{st}", (B, 1, H, W)).repeat(1, 3, 1, 1).cuda()
        labels = dw.det_labels(f"vtr_y{st}", (B, H, W), 9).cuda()
        loss = tr.step(ir3, vis3, mask3, labels)
        assert bool(torch.isfinite(loss)), (name, st)
        assert all(np.isfinite(v) for v in tr.history[st])
    n = 0
    for pn, p in fus.named_parameters():
        if pn.startswith("ffm2."):
            assert p.grad is None and torch.equal(p.detach(), before[pn]), pn
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), pn
        assert not torch.equal(p.detach(), before[pn]), pn
        n += 1
    assert n > 20
    assert all(p.grad is None for p in seg.parameters())
