"""Multi-scale + horizontal-flip inference settings (the protocol SegFormer's mIoU tables are quoted under): the views of a
frame and the sizes their network inputs are resized to.  Pure host code; the views are combined by ops.tta_vote
(Network3.predict_labels_tta)."""
from dataclasses import dataclass
from typing import Tuple

MAX_VIEWS = 16  # (segmif_tta_vote_f32's view table)


def _round_up(n, d):
    return (n + d - 1) // d * d


def tta_plan(H, W, scales, flip, size_divisor=8):
    """-> [(h, w, flipped), ...]: for each scale s, in the given order, the plain view and then, with flip, the mirrored one;
    h = int(H * s + 0.5) rounded up to a multiple of size_divisor, w likewise.

    The default divisor is 8 because every size the stored records of the HIP forward cover (64 x 96, 72 x 104, 256 x 256,
    480 x 640, 1024) is a multiple of 8; nothing in this tree tests the forward at widths that are not multiples of 4, and
    multi-scale inference does not widen that: a smaller divisor is the caller's responsibility.

    ValueError for an empty scale list, a scale <= 0, size_divisor < 1 or more than 16 views."""
    scales = tuple(scales)
    if not scales:
        raise ValueError("tta_plan: no scales")
    if size_divisor < 1 or int(size_divisor) != size_divisor:
        raise ValueError(f"tta_plan: size_divisor must be a positive integer, got {size_divisor}")
    if H < 1 or W < 1:
        raise ValueError(f"tta_plan: frame size {H} x {W}")
    size_divisor = int(size_divisor)
    plan = []
    for s in scales:
        if not s > 0:
            raise ValueError(f"tta_plan: scale {s} is not positive")
        h, w = _round_up(max(int(H * s + 0.5), 1), size_divisor), _round_up(max(int(W * s + 0.5), 1), size_divisor)
        plan.append((h, w, False))
        if flip:
            plan.append((h, w, True))
    if len(plan) > MAX_VIEWS:
        raise ValueError(f"tta_plan: {len(plan)} views, the vote kernel takes at most {MAX_VIEWS}")
    return plan


@dataclass(frozen=True)
class TTA:
    """Settings of multi-scale + flip inference; the defaults are the SegFormer protocol (12 views)."""
    scales: Tuple[float, ...] = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
    flip: bool = True
    size_divisor: int = 8

    def __post_init__(self):
        object.__setattr__(self, "scales", tuple(float(s) for s in self.scales))

    def plan(self, H, W):
        return tta_plan(H, W, self.scales, self.flip, self.size_divisor)

    def describe(self, H, W):
        """The "tta" entry of evaluate's JSON for H x W frames."""
        return {"scales": list(self.scales), "flip": bool(self.flip), "size_divisor": int(self.size_divisor),
                "views": [[h, w, bool(f)] for h, w, f in self.plan(H, W)]}
