"""The run-time switches of the arithmetic paths: one table, read from the environment once at import, changed in-process with
set() / modes().  Imports neither torch nor the library.

The state is PROCESS-GLOBAL on purpose, not thread-local: autograd.py asks train_conv_f16() inside backward(), which runs on
the autograd engine's own threads - an override local to the caller's thread would not reach it.  (The C-side switches -
SEGMIF_WGRAD3X3, SEGMIF_GEMM_EPI, ... - are read once per process inside the library and are not in this table.)
"""
import contextlib
import os
from typing import NamedTuple


class Mode(NamedTuple):
    name: str       # key of get() / set() / modes()
    env: str        # environment variable read at import ("" counts as unset)
    values: object  # tuple of the legal strings, or a parser (str | number -> value, ValueError) for a numeric switch
    default: object
    doc: str


def _positive_float(v):
    """a positive float"""
    v = float(v)
    if not v > 0.0:
        raise ValueError(v)
    return v


_F16_BF16 = ("f16x3", "bf16x6")
_ARITH = _F16_BF16 + ("fp32",)
TABLE = (
    Mode("conv3x3", "SEGMIF_CONV3X3", ("planes", "planes16", "bf16x6", "fp32"), "planes16",
         "'bf16x6': 3x3 stride-1 convs with Cin % 16 == 0 on the bf16 matrix pipe with 3-way split operands (fp32-class accuracy, "
         "2.7x the fp32 MFMA rate); 'planes': the same, and the fusion net's DRDBs and closing convs in inference keep their "
         "activations pre-split in a planes buffer (csrc/conv3x3_planes.hip); 'planes16': as 'planes' with half-precision pairs "
         "and three products per MAC (f16x3, the same error class at half the matrix work; guarded by Planes16Guard: a forward "
         "whose planes leave the half's exponent range is repeated in 'planes'); 'fp32': exact-fp32 MFMA everywhere.  Training "
         "always uses the bf16x6 / fp32 kernels."),
    Mode("crosspath", "SEGMIF_CROSSPATH", ("gram", "gemm"), "gram",
         "'gram': CrossPath in inference on the Gram-matrix kernels of csrc/crosspath.hip; 'gemm': round 1's channel_proj GEMMs + "
         "fused kv reductions + two-source end_proj GEMM."),
    Mode("crosspath_arith", "SEGMIF_CROSSPATH_ARITH", _F16_BF16, "f16x3",
         "(r6) arithmetic of crosspath_tail's own contractions where it can be f16x3 (lazy segmentation feature, planes-only "
         "output, guarded scope); 'bf16x6' is the A/B side.  Round 4 had built the same for the kernel that still read x_3 from "
         "HBM and measured nothing (HBM-bound then); the lazy tail is bound by its vector + matrix work (DESIGN section 4)."),
    Mode("train_conv", "SEGMIF_TRAIN_CONV", _F16_BF16, "f16x3",
         "Arithmetic of the TRAINING path's 3x3 convs (forward + input gradients of the DRDBs): 'f16x3' (r4) = half pairs x three "
         "products with the input scaled into the half's range from device-side range slots; 'bf16x6' = round 3's bf16 triples."),
    Mode("linear", "SEGMIF_LINEAR", _ARITH, "f16x3",
         "'f16x3': tall nn.Linear problems on the split-operand GEMM, with half pairs and three products per MAC inside a guarded "
         "scope (run_guarded) and bf16 triples / six products outside one; 'bf16x6': always bf16 triples; 'fp32': the exact-fp32 "
         "MFMA tiles.  Weight caches are keyed on the mode."),
    Mode("pairs", "SEGMIF_GEMM_PAIRS", ("on", "off"), "on",
         "(r5) 'on': activations pre-split by their producer, both GEMM operands by LDS-DMA (csrc/gemm_pairs.hip); 'off': round "
         "4's gemm_split<f16x3> everywhere (A/B switch)."),
    Mode("mixffn", "SEGMIF_MIXFFN", ("fused", "chain"), "fused",
         "'fused': the one-kernel Mix-FFN (csrc/mixffn.hip) where it exists; 'chain': round 3's LayerNorm -> GEMM -> dwconv+GELU "
         "-> GEMM everywhere (A/B switch)."),
    Mode("attention", "SEGMIF_ATTENTION", _ARITH, "f16x3",
         "'f16x3': csrc/attention_split.hip on half pairs with three f16 MFMA products per MAC inside a guarded scope "
         "(run_guarded), on bf16 triples / six products outside one; 'bf16x6': always bf16 triples (head_dim 64, fp32-class either "
         "way); 'fp32': csrc/attention.hip (fp32 MFMA) everywhere.  head_dim 32 always runs the fp32 kernel."),
    Mode("lazy_seg", "SEGMIF_LAZY_SEG", ("1", "0"), "1",
         "'1': Fusion_Network3_ac.forward_from_features hands CrossPath the LOW-resolution segmentation feature and the kernels "
         "resize it as they read; '0': the feature is resized to H x W first (A/B switch)."),
    Mode("sr_conv", "SEGMIF_SR_CONV", ("patch", "igemm"), "patch",
         "'patch': tall spatial-reduction / patch-embed convs on the split-operand GEMM in patch mode; 'igemm': the round-3 path "
         "(fp32 implicit-GEMM tiles; A/B switch)."),
    Mode("guard_per_image", "SEGMIF_GUARD_PER_IMAGE", ("1", "0"), "1",
         "'1': a Planes16Guard keeps one range slot per image and repeats only the images that tripped; '0': one slot per "
         "launch, whole-batch repeats (round 3; A/B switch)."),
    Mode("guard_cond_bound", "SEGMIF_GUARD_COND_BOUND", _positive_float, 2e-4,
         "Planes16Guard.COND_BOUND (its comment is the record of how the number was set): the estimated relative error on the "
         "fused image above which a pair is repeated with exact convs.  The class attribute copies it ONCE, when guard.py is "
         "imported: in a running process change Planes16Guard.COND_BOUND itself - set() here does not reach the guard."),
    Mode("drdb_res", "SEGMIF_DRDB_RES", ("planes", "fp32"), "planes",
         "'planes' (r4): on f16x3 planes a DRDB takes its residual from its own input chunks; 'fp32': round 3's fp32 residual "
         "tensors (A/B switch; bf16 planes always do)."),
    Mode("conv1", "SEGMIF_CONV1", ("stencil", "igemm"), "stencil",
         "'stencil' (r6): conv1_ir / conv1_vis of the fusion net as a store-bound stencil kernel; 'igemm': the K = 9 "
         "implicit-GEMM tiles (A/B switch)."),
    Mode("attn_bwd", "SEGMIF_ATTN_BWD", ("fused", "materialize"), "fused",
         "'fused' (r5): head_dim-64 attention backward on the flash-style kernels of csrc/attention_bwd.hip; 'materialize': round "
         "4's batched GEMMs + row softmax over materialised (B, heads, N, Nk) scores."),
)
_BY_NAME = {m.name: m for m in TABLE}


def _legal(m):
    """How messages and documents name what `m` accepts: the tuple of strings, or the parser's description."""
    return m.values if isinstance(m.values, tuple) else m.values.__doc__


def _checked(m, value):
    if isinstance(m.values, tuple):
        if value not in m.values:
            raise ValueError(f"{m.name} must be one of {m.values}, got {value!r}")
        return value
    try:
        return m.values(value)
    except (TypeError, ValueError):
        raise ValueError(f"{m.name} must be {_legal(m)}, got {value!r}") from None


def _from_env(m):
    raw = os.environ.get(m.env, "")
    try:
        return _checked(m, raw) if raw else m.default
    except ValueError:
        raise RuntimeError(f"{m.env} must be {'one of ' if isinstance(m.values, tuple) else ''}{_legal(m)}, got {raw!r}") from None


_state = {m.name: _from_env(m) for m in TABLE}


def get(name):
    return _state[name]


def set(name, value):
    """-> the previous value.  ValueError (naming the legal values) for a value the switch does not have.  Every switch is read
    where it acts, except guard_cond_bound (see its entry): that one is changed on Planes16Guard.COND_BOUND."""
    prev, _state[name] = _state[name], _checked(_BY_NAME[name], value)
    return prev


@contextlib.contextmanager
def modes(**overrides):
    """with modes(conv3x3="fp32", crosspath="gemm"): ... - set several switches, restore them in reverse order on the way out."""
    done = []
    try:
        for name, value in overrides.items():
            done.append((name, set(name, value)))
        yield
    finally:
        for name, prev in reversed(done):
            set(name, prev)
