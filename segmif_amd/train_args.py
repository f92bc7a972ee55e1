"""The command line of python -m segmif_amd.train as data, host only: its names, build_parser (flags and help), check_args (what the flags
cannot mean together: the tables _BELONGS and _RANGES, then the rules that read several flags) and resolve_defaults (_DEFAULTS).
segmif_amd.train imports all of it; a new family of flags is one block in the parser and one row in each table."""
import argparse
import math
import os

SEG_CKPT, FUSION_CKPT = "model-fusion_add_final2.pth", "modelfusion-final2.pth"  # train.py:237-238, :403-407
SEG_LOSSES = ("ce", "ohem", "focal", "normal", "weighted")
SEG_REGIONS = ("lovasz", "dice")
DISTILL_KINDS = ("channel", "pixel")
DISTILL_TEMPERATURES = {"channel": 4.0, "pixel": 1.0}  # losses.DISTILL_TEMPERATURES, restated: this module imports no torch
DISTILL_BACKBONES = ("mit_b1", "mit_b2", "mit_b3", "mit_b4", "mit_b5")


def fusion_loss_names():
    """the objectives of core/loss.py that --fusion-loss / make_fusion_loss build"""
    from .core import loss
    return sorted(n for n in loss.__all__ if n.startswith(("Fusionloss", "Total_fusion_loss", "new_loss_sobel")))


def build_parser():
    """the command line of python -m segmif_amd.train, declaratively: flags and help, no checks"""
    ours = " (this project's choice: the reference reads it from a configs/*.yaml it does not ship)"
    ap = argparse.ArgumentParser(prog="python -m segmif_amd.train", description="The reference's training schedule (train.py:424-434) "
                                 "on device-made batches: per round a fusion phase (FusionTrainer) then a segmentation phase "
                                 "(seg_train_step).  Constants of the reference's code are fixed: 3e-4 / round as the fusion optimizer's "
                                 "default rate, 6000 / 4000 fusion and 10000 segmentation iterations, loss weights 0.4 / round and 0.8, "
                                 "7 rounds; --rounds / --fusion-iters / --seg-iters shorten a run.")
    ap.add_argument("--root", help="data set root: Infrared/ Visible/ Mask2/ Label/ (voc_fusion3.py:25-28)")
    ap.add_argument("--name-lists", help="folder of SPLIT.txt name lists")
    ap.add_argument("--split", default="train")
    ap.add_argument("--val-split", default="val", help="split whose mIoU decides which segmentation checkpoint is kept")
    ap.add_argument("--synthetic", type=int, metavar="N", help="train on N seeded synthetic frames instead of a data set")
    ap.add_argument("--synthetic-size", type=int, nargs=2, default=(480, 640), metavar=("H", "W"))
    ap.add_argument("--out", default="checkpoint", help=f"folder of {SEG_CKPT} and {FUSION_CKPT}")
    ap.add_argument("--backbone", default="mit_b3", help="mit_b1 .. mit_b5; mit_b0's 32/64-channel features do not fit "
                    "the fusion net's conv3 / conv4, in the reference either" + ours)
    ap.add_argument("--pretrained", action="store_true", help="load the backbone's ImageNet weights from pretrained/BACKBONE.pth as the "
                    "reference does (model_fusion.py:49); without it: random initialisation")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--fusion-iters", type=int, help="fusion iterations per round (default 6000 in round 1, then 4000)")
    ap.add_argument("--seg-iters", type=int, help="segmentation iterations per round (default 10000)")
    ap.add_argument("--samples-per-gpu", type=int, default=8, help="the loaders' batch is HALF of it (train.py:138, :290)" + ours)
    ap.add_argument("--crop-size", type=int, default=512, help="crop" + ours)
    ap.add_argument("--rescale-range", type=float, nargs=2, default=(0.5, 2.0), help="random scaling" + ours)
    ap.add_argument("--lr", type=float, default=8e-5, help="learning rate of both phases, / round in the fusion phase" + ours)
    ap.add_argument("--weight-decay", type=float, default=0.01, help=ours.strip(" ()"))
    ap.add_argument("--betas", type=float, nargs=2, default=(0.9, 0.999), help=ours.strip(" ()"))
    ap.add_argument("--warmup-iter", type=int, default=3000, help="segmentation warm-up" + ours)
    ap.add_argument("--warmup-ratio", type=float, default=1e-6, help=ours.strip(" ()"))
    ap.add_argument("--power", type=float, default=1.0, help="polynomial decay" + ours)
    ap.add_argument("--max-iters", type=int, default=160000, help="horizon of both schedules" + ours)
    ap.add_argument("--fusion-loss", metavar="NAME", help="train the fusion net on this objective of core/loss.py instead of the "
                    "reference's schedule (Fusionloss3 in round 1, then Fusionloss_grad3 as the intensity term), which is the default. "
                    "Any objective other than that schedule is this project's choice: the reference's train.py instantiates no other")
    ap.add_argument("--seg-loss", choices=SEG_LOSSES, default="ce", help="objective of the SEGMENTATION phase (the segmentation term "
                    "inside the fusion phase keeps plain CE).  ce, the default, is the reference's nn.CrossEntropyLoss(ignore_index=255); "
                    "ohem / focal / normal are core/loss.py's OhemCELoss / SoftmaxFocalLoss / NormalLoss, weighted is CE with "
                    "--seg-class-weights: none of those is the reference's objective, its train.py instantiates CE only")
    ap.add_argument("--ohem-thresh", type=float, default=0.7, help="--seg-loss ohem: probability threshold (losses above -log of it are hard)")
    ap.add_argument("--ohem-n-min", type=int, help="--seg-loss ohem: least number of pixels averaged; default batch * crop^2 // 16" + ours)
    ap.add_argument("--focal-gamma", type=float, default=2.0, help="--seg-loss focal: exponent of (1 - p)")
    ap.add_argument("--label-smoothing", type=float, default=0.0, help="--seg-loss ce / weighted: label smoothing in [0, 1); above 0 it is "
                    "not the reference's objective")
    ap.add_argument("--seg-class-weights", type=float, nargs="+", metavar="W", help="--seg-loss weighted: one weight >= 0 per class (9)")
    ap.add_argument("--seg-class-weights-from", choices=("inverse", "median", "enet"), help="--seg-loss weighted: compute "
                    "the class weights from the training split's labels, counted on the device, instead of typing them: inverse "
                    "(1 / frequency, mean 1 over the present classes), median (median-frequency balancing, Eigen and Fergus 2015) or "
                    "enet (1 / ln(1.02 + frequency), Paszke et al. 2016).  A class without a pixel gets "
                    "weight 0.  Excludes --seg-class-weights")
    ap.add_argument("--rare-class-sampling", action="store_true", help="draw the training frames by rare-class sampling (Hoyer et al. "
                    "2022, DAFormer) instead of walking the split front to back: a class c with probability proportional to "
                    "exp((1 - frequency_c) / T), a frame that holds it, and a crop that shows it.  Off by default.  This project's "
                    "addition, NOT the reference's loader")
    ap.add_argument("--rcs-temperature", type=float, metavar="T", help="with --rare-class-sampling: T > 0 (default 0.01, DAFormer's)")
    ap.add_argument("--rcs-min-pixels", type=int, metavar="N", help="with --rare-class-sampling: a frame is a candidate of a class when "
                    "it holds more than N pixels of it (default 3000, DAFormer's)")
    ap.add_argument("--rcs-min-crop-ratio", type=float, metavar="R", help="with --rare-class-sampling: a crop is accepted when it holds "
                    "more than N * R pixels of the class, scaled by the frame's resize (default 0.5, DAFormer's)")
    ap.add_argument("--rcs-fraction", type=float, metavar="F", help="with --rare-class-sampling: the share of samples drawn that way, in "
                    "(0, 1]; the others walk the split in order (default 1.0)" + ours)
    ap.add_argument("--rcs-phases", choices=("seg", "fusion", "both"), help="with --rare-class-sampling: the phases whose loader "
                    "samples (default seg)")
    ap.add_argument("--class-mix", action="store_true", help="ClassMix (Olsson et al. 2021; the mixing step of DAFormer): with "
                    "probability P a sample of a batch receives, from another sample of the same batch, the pixels of half of the "
                    "classes present in that sample's crop, in every image and in the label, on the device.  Off by default.  This "
                    "project's addition, NOT the reference's loader")
    ap.add_argument("--class-mix-prob", type=float, metavar="P", help="with --class-mix: the probability that a sample is mixed, in "
                    "(0, 1] (default 0.5, this project's choice: DAFormer mixes every sample)")
    ap.add_argument("--class-mix-min-pixels", type=int, metavar="N", help="with --class-mix: a class is present in a donor crop when "
                    "the crop holds more than N pixels of it (default 0)")
    ap.add_argument("--class-mix-classes", choices=("half", "wanted"), help="with --class-mix: paste half of the donor's present "
                    "classes (default), or the one class --rare-class-sampling drew the donor for")
    ap.add_argument("--class-mix-phases", choices=("seg", "fusion", "both"), help="with --class-mix: the phases whose batches are "
                    "mixed (default seg)")
    ap.add_argument("--copy-paste", action="store_true", help="instance copy-paste (Ghiasi et al. 2021, Simple Copy-Paste): the "
                    "connected components of the training split's labels are banked on the device once, and with probability P a "
                    "sample receives up to N of them, scaled (nearest neighbour), mirrored and placed at random, in every image and in "
                    "the label.  Off by default.  This project's addition, NOT the reference's loader; every default below is this "
                    "project's choice")
    ap.add_argument("--copy-paste-prob", type=float, metavar="P", help="with --copy-paste: the probability that a sample is pasted into, "
                    "in (0, 1] (default 0.5, this project's choice)")
    ap.add_argument("--copy-paste-max-objects", type=int, metavar="N", help="with --copy-paste: a sample receives 1..N objects, N in 1..8 "
                    "(default 3, this project's choice)")
    ap.add_argument("--copy-paste-classes", type=int, nargs="+", metavar="C", help="with --copy-paste: the classes that are banked "
                    "(default 1..8: class 0 is the background)")
    ap.add_argument("--copy-paste-min-area", type=int, metavar="A", help="with --copy-paste: an object is banked when it holds at least A "
                    "pixels (default 64, this project's choice)")
    ap.add_argument("--copy-paste-scale", type=float, nargs=2, metavar=("LO", "HI"), help="with --copy-paste: an object is scaled by a "
                    "log-uniform factor in [LO, HI], 0 < LO <= HI (default 0.5 2.0, this project's choice)")
    ap.add_argument("--copy-paste-temperature", type=float, metavar="T", help="with --copy-paste: draw an object's class with probability "
                    "proportional to exp((1 - frequency_c) / T) from the training split's class frequencies, T > 0, as "
                    "--rare-class-sampling does (default: uniform over the banked classes)")
    ap.add_argument("--copy-paste-phases", choices=("seg", "fusion", "both"), help="with --copy-paste: the phases whose batches are "
                    "pasted into (default seg); the unlabelled loader of --self-training never is")
    ap.add_argument("--seg-region", choices=SEG_REGIONS, help="add a region objective to whatever --seg-loss builds, for the "
                    "SEGMENTATION phase only: lovasz is Lovasz-Softmax (the convex surrogate of the Jaccard index, the batch as one set), "
                    "dice the soft Dice loss.  This project's addition, NOT the reference's objective: its train.py trains on CE alone")
    ap.add_argument("--seg-region-weight", type=float, metavar="W", help="--seg-region: the region term's weight, > 0 (default 1.0)")
    ap.add_argument("--seg-region-classes", choices=("present", "all"), help="--seg-region: average over the classes present in the "
                    "batch (default) or over all of them")
    ap.add_argument("--dice-smooth", type=float, metavar="S", help="--seg-region dice: the smoothing term, >= 0 (default 1.0)")
    ap.add_argument("--clip-grad-norm", type=float, metavar="X", help="clip the global gradient norm of every step of both phases to "
                    "X > 0 (torch.nn.utils.clip_grad_norm_'s rule, on the device); off by default.  This project's addition: the "
                    "reference's train.py does not clip")
    ap.add_argument("--skip-nonfinite", action="store_true", help="do not apply a step whose gradients hold an inf or a NaN (decided on "
                    "the device, no host synchronisation); off by default.  This project's addition")
    ap.add_argument("--max-consecutive-skips", type=int, default=50, metavar="N", help="with --skip-nonfinite: stop when more than N "
                    "steps in a row were skipped (checked at log lines)")
    ap.add_argument("--ema-decay", type=float, metavar="D", help="keep an exponential moving average of the weights, decay D inside "
                    "(0, 1), updated on the device in every applied optimizer step; validation, checkpoint selection and the written "
                    "checkpoints then use the AVERAGED weights.  Off by default.  This project's addition: the reference's train.py "
                    "averages nothing")
    ap.add_argument("--ema-warmup", action="store_true", help="with --ema-decay: the decay of update t is min(D, (1 + t) / (10 + t))")
    ap.add_argument("--ema-nets", choices=("seg", "fusion", "both"), help="with --ema-decay: the nets that are averaged (default seg)")
    ap.add_argument("--self-training", action="store_true", help="DAFormer-style self-training in the SEGMENTATION phase (Hoyer et al. "
                    "2022): the weight average of --ema-decay is the teacher, its predictions on the frames of --unlabelled-split become "
                    "pseudo-labels on the device, and the step adds a cross entropy on them, weighted by the share of confident pixels, "
                    "to the labelled loss.  Needs --ema-decay with the segmentation net averaged.  Off by default.  This project's "
                    "addition, NOT the reference's training; nothing here says what it does to mIoU")
    ap.add_argument("--unlabelled-split", metavar="NAME", help="with --self-training: the split of --name-lists whose frames carry no "
                    "Label/ image (Infrared/, Visible/ and Mask2/ only).  With --synthetic a seeded stand-in set is made instead")
    ap.add_argument("--st-threshold", type=float, metavar="TAU", help="with --self-training: a pixel is confident when the teacher's "
                    "softmax maximum is above TAU, in [0, 1] (default 0.968, DAFormer's)")
    ap.add_argument("--st-below", choices=("keep", "ignore"), help="with --self-training: keep the pseudo-label of a pixel that is not "
                    "confident (default; DAFormer: the per-image weight carries the confidence) or set it to the ignore value")
    ap.add_argument("--st-weight", type=float, metavar="W", help="with --self-training: weight of the unlabelled term, > 0 (default 1.0)")
    ap.add_argument("--st-temperature", type=float, metavar="T", help="with --self-training: the teacher's logits are divided by T, "
                    "finite and > 0, before the confidence test (default 1.0: nothing is added; python -m segmif_amd.evaluate --calibration "
                    "reports the temperature of lowest NLL)")
    ap.add_argument("--st-mix", action="store_true", help="with --self-training: paste half of the classes of labelled sample i into "
                    "unlabelled sample i (DAFormer's cross-set ClassMix, on csrc/class_mix.hip); pasted pixels get weight 1")
    ap.add_argument("--st-mix-prob", type=float, metavar="P", help="with --st-mix: the probability that a sample is mixed, in (0, 1] "
                    "(default 1.0, DAFormer's)")
    ap.add_argument("--st-mix-min-pixels", type=int, metavar="N", help="with --st-mix: a class is present in a labelled crop when the "
                    "crop holds more than N pixels of it (default 0)")
    ap.add_argument("--st-strong", action="store_true", help="with --self-training: the student's unlabelled input (after --st-mix) goes "
                    "through a colour jitter (brightness, contrast, saturation, hue, in this order) and a Gaussian blur on the device "
                    "(csrc/strong_augment.hip; DAFormer's strong augmentation with its constants, this project's formulas); labels and "
                    "weights are unchanged and the teacher sees the clean frames")
    ap.add_argument("--st-jitter-prob", type=float, metavar="P", help="with --st-strong: the probability that a sample is jittered, in "
                    "[0, 1] (default 0.8, DAFormer's)")
    ap.add_argument("--st-jitter-strength", type=float, metavar="S", help="with --st-strong: the brightness, contrast and saturation "
                    "factors are uniform over [1 - S, 1 + S], S in [0, 1] (default 0.2, DAFormer's)")
    ap.add_argument("--st-jitter-hue", type=float, metavar="H", help="with --st-strong: the hue shift is uniform over [-H, H], H in "
                    "[0, 0.5] (default 0.2, DAFormer's)")
    ap.add_argument("--st-blur-prob", type=float, metavar="P", help="with --st-strong: the probability that a sample is blurred, in "
                    "[0, 1] (default 0.5, DAFormer's)")
    ap.add_argument("--st-blur-sigma", type=float, nargs=2, metavar=("LO", "HI"), help="with --st-strong: the blur's sigma is uniform "
                    "over [LO, HI], 0 < LO <= HI <= 2 (default 0.15 1.15, DAFormer's)")
    ap.add_argument("--distill-from", metavar="CKPT", help="knowledge distillation in the SEGMENTATION phase: a frozen teacher, the "
                    f"Network3 state dict CKPT (a file as {SEG_CKPT}, loaded strictly) on --distill-backbone, sees every labelled batch "
                    "the student sees, and the step adds --distill-weight times a distillation term between the two nets' "
                    "quarter-resolution logits to the labelled loss (segmif_amd.distill, csrc/distill_objective.hip).  Off by default.  "
                    "Excludes --self-training (not built).  This project's addition, NOT the reference's training; nothing here says "
                    "what it does to mIoU")
    ap.add_argument("--distill-backbone", metavar="NAME", help="with --distill-from, required: the teacher's backbone, mit_b1 .. mit_b5")
    ap.add_argument("--distill-kind", choices=DISTILL_KINDS, help="with --distill-from: channel (default; channel-wise distillation, "
                    "Shu et al. 2021: a softmax over the positions of every class map) or pixel (per-pixel KD, Hinton et al. 2015: a "
                    "softmax over the classes of every pixel)")
    ap.add_argument("--distill-temperature", type=float, metavar="T", help="with --distill-from: the temperature, > 0 (default 4.0 for "
                    "channel, 1.0 for pixel; this project's choice)")
    ap.add_argument("--distill-weight", type=float, metavar="W", help="with --distill-from: weight of the distillation term, > 0 "
                    "(default 3.0; this project's choice)")
    ap.add_argument("--log-iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    return ap


N_CLASS = 9
PHASES = {"seg": ("seg",), "fusion": ("fusion",), "both": ("seg", "fusion")}  # what a --*-phases flag holds -> the phases
# check_args' tables, in the order in which their faults are reported.  A switch and the flags that mean nothing without it:
_BELONGS = (
    ("--rare-class-sampling", ("--rcs-temperature", "--rcs-min-pixels", "--rcs-min-crop-ratio", "--rcs-fraction", "--rcs-phases")),
    ("--class-mix", ("--class-mix-prob", "--class-mix-min-pixels", "--class-mix-classes", "--class-mix-phases")),
    ("--copy-paste", ("--copy-paste-prob", "--copy-paste-max-objects", "--copy-paste-classes", "--copy-paste-min-area", "--copy-paste-scale",
                      "--copy-paste-temperature", "--copy-paste-phases")),
    ("--seg-region", ("--seg-region-weight", "--seg-region-classes", "--dice-smooth")),
    ("--self-training", ("--unlabelled-split", "--st-threshold", "--st-below", "--st-weight", "--st-mix", "--st-mix-prob", "--st-mix-min-pixels",
                         "--st-strong", "--st-temperature")),
    ("--st-mix", ("--st-mix-prob", "--st-mix-min-pixels")),
    ("--st-strong", ("--st-jitter-prob", "--st-jitter-strength", "--st-jitter-hue", "--st-blur-prob", "--st-blur-sigma")),
    ("--distill-from", ("--distill-backbone", "--distill-kind", "--distill-temperature", "--distill-weight")),
)
# A flag, what a given value of it must satisfy, and the refusal after "FLAG VALUE: ":
_RANGES = (
    ("--rcs-temperature", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
    ("--rcs-min-pixels", lambda v: v >= 0, "must be >= 0"),
    ("--rcs-min-crop-ratio", lambda v: v >= 0 and math.isfinite(v), "must be a finite number >= 0"),
    ("--rcs-fraction", lambda v: 0.0 < v <= 1.0, "must lie in (0, 1]"),
    ("--class-mix-prob", lambda v: 0.0 < v <= 1.0, "must lie in (0, 1]"),
    ("--class-mix-min-pixels", lambda v: v >= 0, "must be >= 0"),
    ("--copy-paste-prob", lambda v: 0.0 < v <= 1.0, "must lie in (0, 1]"),
    ("--copy-paste-max-objects", lambda v: 1 <= v <= 8, "must lie in 1..8"),
    ("--copy-paste-classes", lambda v: all(0 <= c < N_CLASS for c in v), f"names classes in 0..{N_CLASS - 1}"),
    ("--copy-paste-min-area", lambda v: v >= 1, "must be >= 1"),
    ("--copy-paste-scale", lambda v: 0.0 < v[0] <= v[1] and math.isfinite(v[1]), "needs 0 < LO <= HI"),
    ("--copy-paste-temperature", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
    ("--label-smoothing", lambda v: 0.0 <= v < 1.0, "must lie in [0, 1)"),
    ("--seg-region-weight", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
    ("--dice-smooth", lambda v: v >= 0 and math.isfinite(v), "must be a finite number >= 0"),
    ("--clip-grad-norm", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
    ("--max-consecutive-skips", lambda v: v >= 1, "must be >= 1"),
    ("--ema-decay", lambda v: 0.0 < v < 1.0, "must lie inside (0, 1)"),
    ("--st-threshold", lambda v: 0.0 <= v <= 1.0, "must lie in [0, 1]"),
    ("--st-weight", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
    ("--st-temperature", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
    ("--st-mix-prob", lambda v: 0.0 < v <= 1.0, "must lie in (0, 1]"),
    ("--st-mix-min-pixels", lambda v: v >= 0, "must be >= 0"),
    ("--st-jitter-prob", lambda v: 0.0 <= v <= 1.0, "must lie in [0, 1]"),
    ("--st-jitter-strength", lambda v: 0.0 <= v <= 1.0, "must lie in [0, 1]"),
    ("--st-jitter-hue", lambda v: 0.0 <= v <= 0.5, "must lie in [0, 0.5]"),
    ("--st-blur-prob", lambda v: 0.0 <= v <= 1.0, "must lie in [0, 1]"),
    ("--st-blur-sigma", lambda v: 0.0 < v[0] <= v[1] <= 2.0, "needs 0 < LO <= HI <= 2"),
    ("--distill-temperature", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
    ("--distill-weight", lambda v: v > 0 and math.isfinite(v), "must be a finite number > 0"),
)
# What a flag stands for that defaults to None so that _BELONGS can tell whether it was given (--ohem-n-min: resolve_defaults):
_DEFAULTS = {
    "--rcs-temperature": 0.01, "--rcs-min-pixels": 3000, "--rcs-min-crop-ratio": 0.5, "--rcs-fraction": 1.0, "--rcs-phases": "seg",
    "--class-mix-prob": 0.5, "--class-mix-classes": "half", "--class-mix-min-pixels": 0, "--class-mix-phases": "seg",
    "--copy-paste-prob": 0.5, "--copy-paste-max-objects": 3, "--copy-paste-min-area": 64, "--copy-paste-scale": (0.5, 2.0),
    "--copy-paste-phases": "seg",  # (--copy-paste-classes and --copy-paste-temperature stay None: all classes, a uniform draw)
    "--seg-region-weight": 1.0, "--seg-region-classes": "present", "--dice-smooth": 1.0, "--ema-nets": "seg",
    "--st-threshold": 0.968, "--st-below": "keep", "--st-weight": 1.0, "--st-temperature": 1.0, "--st-mix-prob": 1.0, "--st-mix-min-pixels": 0,
    "--st-jitter-prob": 0.8, "--st-jitter-strength": 0.2, "--st-jitter-hue": 0.2, "--st-blur-prob": 0.5, "--st-blur-sigma": (0.15, 1.15),
    "--distill-kind": "channel", "--distill-weight": 3.0,  # (--distill-temperature follows the kind: resolve_defaults)
}


def _given(args, flag):
    """what the command line gave `flag`; None when it did not (the None defaults, an unset store_true)"""
    value = getattr(args, flag[2:].replace("-", "_"))
    return None if value is False else value


def check_args(args, fail):
    """Refuse, through fail(message), what the flags cannot mean together; needs no device and reads the flags as parsed.  The rows
    the two tables cannot word as the messages are worded (weighted, dice, EMA, OHEM, focal) and the cross-flag rules are code."""
    for flag in ("--seg-class-weights", "--seg-class-weights-from"):
        if _given(args, flag) is not None and args.seg_loss != "weighted":
            fail(f"{flag} belongs to --seg-loss weighted, not {args.seg_loss}")
    for switch, flags in _BELONGS:
        for flag in flags:
            if _given(args, flag) is not None and _given(args, switch) is None:
                fail(f"{flag} belongs to {switch}, which is not given")
    if args.dice_smooth is not None and args.seg_region != "dice":
        fail(f"--dice-smooth belongs to --seg-region dice, not {args.seg_region}")
    if args.ema_decay is None and (args.ema_warmup or args.ema_nets is not None):
        fail("--ema-warmup / --ema-nets belong to --ema-decay, which is not given")
    for flag, ok, text in _RANGES:
        if _given(args, flag) is not None and not ok(_given(args, flag)):
            fail(f"{flag} {_given(args, flag)}: {text}")
    if args.seg_loss == "ohem" and not 0.0 < args.ohem_thresh <= 1.0:
        fail(f"--ohem-thresh {args.ohem_thresh}: a probability in (0, 1]")
    if args.seg_loss == "focal" and not args.focal_gamma > 0:
        fail(f"--focal-gamma {args.focal_gamma}: must be > 0")
    if args.seg_class_weights_from is not None and args.seg_class_weights is not None:
        fail("--seg-class-weights-from computes the weights that --seg-class-weights types: give one of the two")
    if args.seg_loss == "weighted" and args.seg_class_weights_from is None and (
            args.seg_class_weights is None or len(args.seg_class_weights) != N_CLASS or min(args.seg_class_weights) < 0):
        fail(f"--seg-loss weighted needs --seg-class-weights with {N_CLASS} values >= 0, or --seg-class-weights-from inverse | median | enet")
    if args.class_mix and args.class_mix_classes == "wanted":
        sampled = PHASES[args.rcs_phases or "seg"] if args.rare_class_sampling else ()
        missing = [ph for ph in PHASES[args.class_mix_phases or "seg"] if ph not in sampled]
        if missing:
            fail(f"--class-mix-classes wanted pastes the class --rare-class-sampling drew the donor for: the {', '.join(missing)} "
                 "phase has no rare-class sampling (--rare-class-sampling, --rcs-phases)")
    if args.class_mix and args.samples_per_gpu < 4:
        fail(f"--class-mix with --samples-per-gpu {args.samples_per_gpu}: the loaders' batch is half of it and mixing needs two samples, "
             "give at least 4")
    if args.label_smoothing and args.seg_loss not in ("ce", "weighted"):
        fail(f"--label-smoothing belongs to --seg-loss ce / weighted, not {args.seg_loss}")
    if args.self_training and (args.ema_decay is None or args.ema_nets == "fusion"):
        fail("--self-training takes the weight average as its teacher: give --ema-decay with the segmentation net averaged "
             "(--ema-nets seg, the default, or both)")
    if args.self_training and args.synthetic is None and args.unlabelled_split is None:
        fail("--self-training needs --unlabelled-split NAME (or --synthetic N, which makes a stand-in set)")
    if args.self_training and args.synthetic is not None and args.unlabelled_split is not None:
        fail("--unlabelled-split names a split of --name-lists; --synthetic makes its own unlabelled stand-in set")
    if args.distill_from is not None:
        if args.distill_backbone is None:
            fail("--distill-from needs --distill-backbone NAME: a state dict does not say which backbone it belongs to")
        if args.distill_backbone == "mit_b0" or args.distill_backbone not in DISTILL_BACKBONES:
            fail(f"--distill-backbone {args.distill_backbone}: one of {', '.join(DISTILL_BACKBONES)}")
        if args.self_training:
            fail("--distill-from with --self-training: distillation on the unlabelled split, or beside self-training, is not built")
        if not os.path.isfile(args.distill_from):
            fail(f"--distill-from {args.distill_from}: no such file")
    seg_pixels = max(1, args.samples_per_gpu // 2) * args.crop_size ** 2
    if args.seg_loss == "ohem" and args.ohem_n_min is not None and not 1 <= args.ohem_n_min <= seg_pixels:
        fail(f"--ohem-n-min {args.ohem_n_min}: outside 1..{seg_pixels}, the pixels of a segmentation batch")
    if (args.synthetic is None) == (args.root is None):
        fail("give either --root DIR --name-lists DIR or --synthetic N")
    if args.fusion_loss is not None and args.fusion_loss not in fusion_loss_names():
        fail(f"--fusion-loss {args.fusion_loss}: one of {', '.join(fusion_loss_names())}")
    if args.backbone == "mit_b0":
        fail("--backbone mit_b0: Fusion_Network3_ac takes 64/128-channel segmentation features, mit_b0 gives 32/64")
    if args.root is not None and not args.name_lists:
        fail("--root needs --name-lists")


def resolve_defaults(args):
    """give every flag that is still None its value, in place: nothing after this asks whether a flag was given"""
    for flag, value in _DEFAULTS.items():
        if _given(args, flag) is None:
            setattr(args, flag[2:].replace("-", "_"), value)
    if args.distill_from is not None and args.distill_temperature is None:
        args.distill_temperature = DISTILL_TEMPERATURES[args.distill_kind]
    if args.ohem_n_min is None:
        args.ohem_n_min = max(1, max(1, args.samples_per_gpu // 2) * args.crop_size ** 2 // 16)
