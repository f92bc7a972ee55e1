"""Host-side check of segmif_amd.train.make_plan (no device is touched): for the argument lists of the GPU command tests -
test_gpu_augment, test_gpu_class_balance, test_gpu_class_mix (both `classes`) and test_gpu_self_training (both `mix`) - the plan's
keyword dicts, phase tuples and iteration counts are the values written out here, and its announcements start the way those tests
look for them in the log."""
import pytest

SHAPES = ["--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2", "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128",
          "--samples-per-gpu", "4", "--out", "somewhere"]
BALANCE = ["--rare-class-sampling", "--rcs-min-pixels", "16", "--seg-loss", "weighted", "--seg-class-weights-from", "median"]
MIX = BALANCE + ["--class-mix", "--class-mix-prob", "1.0"]
SELF = ["--ema-decay", "0.9", "--self-training", "--st-threshold", "0.12"]

SCHED = dict(weight_decay=0.01, betas=(0.9, 0.999), max_iter=160000, warmup_ratio=1e-6, power=1.0)
OFF = dict(batch=2, guarded=False, ema_seg=False, ema_fus=False, fusion_opt_kw=dict(lr=8e-5, **SCHED),
           seg_opt_kw=dict(lr=8e-5, warmup_iter=3000, **SCHED), loader_kw=dict(batch=2, crop_size=64, rescale_range=(0.5, 2.0), fliplr=True),
           rcs_kw=None, rcs_phases=(), mix_kw=None, mix_phases=(), st_kw=None, st_mix_kw=None, fusion_iters=[2], seg_iters=[2])
RCS = dict(rcs_kw=dict(temperature=0.01, min_pixels=16, min_crop_ratio=0.5, fraction=1.0), rcs_phases=("seg",))
EMA = dict(ema_seg=True, seg_opt_kw=dict(lr=8e-5, warmup_iter=3000, **SCHED, ema_decay=0.9, ema_warmup=False))

SLOT, PROBE = "<class table, computed weights>", "<candidates and probabilities>"  # where the lines that read the labels go
CASES = {  # name: (arguments, the plan without `say`, per announcement in order what it holds; one that begins with [train]: how it begins)
    "augment": (["--synthetic", "16"] + SHAPES, OFF,
                [["[train] --synthetic 16: training on SYNTHETIC frames"], ["[train] no --pretrained"], SLOT]),
    "class_balance": (["--synthetic", "16"] + SHAPES + BALANCE, {**OFF, **RCS},
                      [["SYNTHETIC"], [], SLOT, ["[train] --seg-loss weighted: NOT the reference's"],
                       ["[train] --rare-class-sampling (", "min_pixels 16", "phases seg)", "NOT the reference's loader"], PROBE]),
    "class_mix-half": (["--synthetic", "16"] + SHAPES + MIX,
                       {**OFF, **RCS, "mix_kw": dict(prob=1.0, classes="half", min_pixels=0, n_class=9), "mix_phases": ("seg",)},
                       [[], [], SLOT, ["[train] --seg-loss"], ["[train] --rare-class-sampling ("], PROBE,
                        ["[train] --class-mix (", "classes half", "phases seg)", "NOT the reference's loader"]]),
    "class_mix-wanted": (["--synthetic", "16"] + SHAPES + MIX + ["--class-mix-classes", "wanted"],
                         {**OFF, **RCS, "mix_kw": dict(prob=1.0, classes="wanted", min_pixels=0, n_class=9), "mix_phases": ("seg",)},
                         [[], [], SLOT, ["[train] --seg-loss"], ["[train] --rare-class-sampling ("], PROBE,
                          ["[train] --class-mix (", "classes wanted", "NOT the reference's loader"]]),
    "self_training": (["--synthetic", "8"] + SHAPES + SELF, {**OFF, **EMA, "st_kw": dict(tau=0.12, below="keep", unsup_weight=1.0)},
                      [["[train] --synthetic 8:"], [], SLOT, ["[train] --ema-decay 0.9 --ema-nets seg:"],
                       ["[train] --self-training (tau 0.12, below keep, unsup_weight 1.0; {unlabelled} unlabelled frames)",
                        "NOT the reference's training", "mIoU"]]),
    "self_training-mix": (["--synthetic", "8"] + SHAPES + SELF + ["--st-mix", "--st-below", "ignore"],
                          {**OFF, **EMA, "st_kw": dict(tau=0.12, below="ignore", unsup_weight=1.0),
                           "st_mix_kw": dict(prob=1.0, classes="half", min_pixels=0, n_class=9)},
                          [[], [], SLOT, ["[train] --ema-decay"],
                           ["[train] --self-training (tau 0.12, below ignore, unsup_weight 1.0; {unlabelled} unlabelled frames; "
                            "--st-mix prob 1.0, classes half, min_pixels 0, n_class 9)", "NOT the reference's training", "mIoU"]]),
}


def plan_of(argv):
    from segmif_amd import train
    ap = train.build_parser()
    args = ap.parse_args(argv)
    train.check_args(args, ap.error)
    train.resolve_defaults(args)
    return train.make_plan(args)


@pytest.mark.parametrize("case", list(CASES))
def test_plan_of_the_gpu_command_tests(case):
    argv, want, say = CASES[case]
    plan = plan_of(argv)
    got = {k: v for k, v in vars(plan).items() if k != "say"}
    assert got == want
    assert len(plan.say) == len(say), plan.say
    for line, needles in zip(plan.say, say):
        if isinstance(needles, str):
            assert line == needles  # a slot
            continue
        assert line.startswith("[train] ") and "\n" not in line
        for needle in needles:
            assert line.startswith(needle) if needle.startswith("[train]") else needle in line, line
    assert any("--st-mix" in line for line in plan.say) == (case == "self_training-mix")


def test_plan_of_every_switch_and_the_default_schedule():
    """the guard and the average reach the optimizers they belong to, the phases follow --*-phases, and without --fusion-iters /
    --seg-iters the rounds have the reference's iteration counts"""
    plan = plan_of(["--synthetic", "8", "--rounds", "3", "--clip-grad-norm", "1", "--skip-nonfinite", "--ema-decay", "0.9", "--ema-nets", "both",
                    "--ema-warmup", "--rare-class-sampling", "--rcs-phases", "both", "--class-mix", "--class-mix-phases", "fusion"])
    guard, ema = dict(max_grad_norm=1.0, skip_nonfinite=True), dict(ema_decay=0.9, ema_warmup=True)
    assert plan.fusion_opt_kw == dict(lr=8e-5, **SCHED, **guard, **ema)
    assert plan.seg_opt_kw == dict(lr=8e-5, warmup_iter=3000, **SCHED, **guard, **ema)
    assert (plan.guarded, plan.ema_seg, plan.ema_fus, plan.batch) == (True, True, True, 4)
    assert plan.rcs_phases == ("seg", "fusion") and plan.mix_phases == ("fusion",)
    assert plan.rcs_kw == dict(temperature=0.01, min_pixels=3000, min_crop_ratio=0.5, fraction=1.0)
    assert plan.mix_kw == dict(prob=0.5, classes="half", min_pixels=0, n_class=9)
    assert plan.fusion_iters == [6000, 4000, 4000] and plan.seg_iters == [10000, 10000, 10000]
    begins = ["[train] --synthetic 8:", "[train] no --pretrained", SLOT,
              "[train] --clip-grad-norm 1.0 --skip-nonfinite: this project's additions, NOT the reference's",
              "[train] --ema-decay 0.9 --ema-warmup --ema-nets both: this project's addition, NOT the reference's",
              "[train] --rare-class-sampling (", PROBE, "[train] --class-mix ("]
    assert len(plan.say) == len(begins) and all(line.startswith(b) for line, b in zip(plan.say, begins)), plan.say
