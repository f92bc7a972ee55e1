"""The f16x3 range and conditioning guard: Planes16Guard (per-image range slots + the CrossPath conditioning words), the
per-thread guarded scope (run_guarded / finish_guarded / install_guard / run_unguarded) and its statistics.  Imports modes, never
ops: the layering is modes <- guard <- ops.
"""
import threading
import warnings

import torch

from . import modes


class Planes16Guard:
    """Range bookkeeping of the f16x3 path, PER IMAGE: every producer launch of half pairs folds max |x| of what it wrote
    into its own row of slots, one slot per batch element (a device-side atomic max; a launch whose batch is not the
    guard's reports to column 0 and stands for every image).  tripped() reads the rows back (one host sync) and says which
    images left [2^-13, 65504) somewhere - the range in which a half pair carries an fp32 value to within one bit.  All-zero
    tensors pass; inf and NaN read as overflow (the slots hold integer maxima of bit patterns: a NaN cannot be dropped).
    One hole, by construction: the maxima are taken over the HIGH halves' patterns, so a tensor whose every |x| is
    below 2^-25 (the half's smallest subnormal, rounded) reads 0 like an all-zero tensor and passes; its values are then carried
    by the low halves alone down to 2^-36 and as zeros below - an ABSOLUTE error of at most 2^-25 |w| per product, i.e. far
    below fp32's own resolution of anything it is added to, but not the "one bit of fp32" the in-range contract states."""
    SLOTS = 4096  # (r5: 1024 -> 4096 rows - a pairs LayerNorm takes LN_SUB rows; 1 MB at 64 images, read back once per forward)
    LO, HI = 2.0 ** -13, 65504.0
    # (r5) conditioning bound.  crosspath_fold reports, per image and per INTERACTION (the fusion net runs its FeatureFusionModule
    # twice, in series), kappa = how far a CrossPath context softmax moves per unit RELATIVE perturbation of its Gram matrix
    # (csrc/crosspath.hip).  What the f16x3 convs leave on the features entering an interaction is ~COND_EPS relative; the first
    # interaction turns it into COND_EPS kappa_1, which the second amplifies again: the estimate of what reaches the fused image is
    #     est = COND_EPS (kappa_1 + kappa_2 + kappa_1 kappa_2),
    # and an image with est > COND_BOUND is repeated with the 3x3 convs in exact fp32 (verdict()).  One large kappa alone is
    # harmless (1e-7 x 2 000 = 2e-4); the inputs on which f16x3 really lost accuracy - over-exposed image-like pairs, 4.6e-3 against
    # the exact-fp32 path's 1.6e-3 - have BOTH in the hundreds (tools/cond_probe.py: 300 x 366).  The estimate is an upper-ish one
    # (the probe pattern is not the real error pattern): over 30 calibration pairs at 64 x 96 (profiles/r05_cond_calibration.txt)
    # every pair whose f16x3 error exceeded 3 x the exact-fp32-conv result's AND 1e-4 sits at est >= 3.5e-3 (the one that breaks
    # the 1e-3 tolerance at 8.4e-3), while 4 of the 8 pairs above 2e-3 lose nothing and are repeated needlessly (correct, slower);
    # below the bound the largest f16x3 error is 1.2e-4 and equals the exact-fp32 path's.  At 480 x 640 (r05_cond_fullsize.txt:
    # mit_b1 / mit_b3, inputs x1 and x4) the contexts are decided - est <= 1.8e-4, f16x3 and exact-fp32 convs agree to 7e-6 on
    # every pair - and nothing is repeated.  The bench line reports the repeat rate (f16x3_cond_repeat_rate).
    # (r6) The bound came down from 2e-3 to 2e-4 after a false-negative search at FULL size (tools/cond_search.py,
    # profiles/r06_cond_search.txt: 224 pairs at 480 x 640 - the bench's generator and image-like inputs at exposures x1 .. x8, hash
    # weights and per-layer log-uniform weight scales, every pair against the same pair on exact-fp32 MFMA kernels and, where the two
    # differ by more than 1e-4, against a float64 evaluation of the CPU restatement).  Among the pairs the 2e-3 bound let through, ONE was outside the
    # tolerance: U[0,1) inputs x 8, kappa = (0, 3 970), estimate 3.97e-4, f16x3 1.53e-3 from the truth where exact fp32 sits at
    # 6.5e-6.  Over all passed pairs the distance d between the f16x3 and the exact-fp32 result is <= 3.9 x the estimate; at
    # 2e-4 the largest d among passed pairs is 1.1e-4 (that pair: 1.1e-4 from the truth) and no pair breaks max(1e-3, 1.5 e32).
    # Price: 12 of the 187 passed pairs of that (adversarial) search and 15 of the 512 pairs of the bench's eight ranks are
    # repeated (rank 0, the one-GPU headline: none, its largest estimate is 7e-7); a repeat costs ~12 ms + 6.6 ms per pair.
    COND_EPS = 1.0e-7
    COND_BOUND = modes.get("guard_cond_bound")  # (SEGMIF_GUARD_COND_BOUND)

    def __init__(self, device, images=1):
        if modes.get("guard_per_image") == "0":  # A/B switch: one slot per launch, whole-batch repeats (round 3)
            images = 1
        self.images = max(1, int(images))
        # rows 0 .. SLOTS-1: range slots; rows SLOTS, SLOTS + 1: the conditioning words of the first / every later interaction
        # (one per image; crosspath_fold raises them)
        self.amax = torch.zeros((self.SLOTS + 2, self.images), device=device, dtype=torch.int32)
        self.used = 0
        self.shared = 0  # launches past SLOTS rows: they share the last row (overflow check exact, vanishing-tensor check pooled)
        self.whole = set()  # rows written by a launch that did not index by image
        self.interaction = 0  # FeatureFusionModule calls seen by this scope (next_interaction())

    def slot(self, images=None):
        """-> (device address of the next launch's row of range slots, amax_images for the kernel).  images: the batch the
        launch will index its slots by; anything but the guard's own count makes it a whole-batch row.  Past SLOTS launches
        the last row is shared: the overflow check stays exact (a maximum of maxima), only the vanishing-tensor check of those
        launches is pooled."""
        if self.used < self.SLOTS:
            self.used += 1
        else:
            self.shared += 1  # (r6, ADVICE r5: counted and reported - range_stats()["slot_rows_shared"])
            _note_shared_row()
        row = self.used - 1
        per_image = images is not None and images == self.images and self.images > 1
        if not per_image and self.images > 1:
            self.whole.add(row)
        return self.amax.data_ptr() + 4 * self.images * row, (self.images if per_image else 1)

    def slot_rows(self, images, n):
        """-> (address of n CONSECUTIVE rows of range slots, amax_images, rows actually granted): for a launch that spreads its
        reports (n a power of two).  Near the end of the table a single row is granted."""
        if self.used + n > self.SLOTS:
            ptr, nimg = self.slot(images)
            return ptr, nimg, 1
        ptr, nimg = self.slot(images)
        first = self.used - 1
        for _ in range(n - 1):
            self.slot(images)
        assert self.used - 1 == first + n - 1
        return ptr, nimg, n

    def next_interaction(self):
        """Called by FeatureFusionModule at the start of each forward inside the scope: the folds that follow report to the
        conditioning row of that interaction (first / later)."""
        self.interaction += 1

    def cond_slot(self, images):
        """-> device address of the conditioning words for a launch over `images` images (segmif_crosspath_fold_f32's `cond`):
        the row of the running interaction when the launch indexes the guard's batch, else None (a module run on its own with
        a batch the scope does not know gets no conditioning check)."""
        if images == self.images:
            return self.amax.data_ptr() + 4 * self.images * (self.SLOTS + (1 if self.interaction > 1 else 0))
        return None

    def reset(self):
        """Forget every launch (a recorded hipGraph re-fills the same rows on each replay)."""
        self.used = 0
        self.shared = 0
        self.interaction = 0
        self.whole.clear()
        self.amax.zero_()

    def _read(self):
        """ONE device read-back: (range maxima of the used rows, conditioning words) as float32."""
        host = torch.cat((self.amax[:self.used], self.amax[self.SLOTS:self.SLOTS + 2])).cpu().view(torch.float32)
        return host[:self.used], host[self.used:self.used + 2]

    def maxima(self):
        return self._read()[0]

    def kappa(self):
        """-> float tensor (2, images): the largest softmax conditioning figure each image's CrossPath contexts reported in the
        first interaction (row 0) and in the later one(s) (row 1)."""
        return self._read()[1]

    def cond_estimate(self, k=None):
        """-> float tensor (images,): COND_EPS (k1 + k2 + k1 k2), the estimated relative error the f16x3 convs' rounding leaves on
        the fused image after both interactions (NaN kappa: NaN)."""
        k = self.kappa() if k is None else k
        return self.COND_EPS * (k[0] + k[1] + k[0] * k[1])

    def verdict(self):
        """-> (tripped, saturated): bool tensors (images,).  tripped: some tensor of that image left the half's range (or held
        inf / NaN) - repeat on bf16x6.  saturated: in range, but the CrossPath context softmaxes are ill-conditioned enough that
        the f16x3 convs' operand rounding is estimated (cond_estimate) to reach COND_BOUND on the fused image, or their logits
        are NaN - repeat with the 3x3 convs in exact fp32.  One read-back for both."""
        m, k = self._read()
        bad = ~((m == 0) | ((m >= self.LO) & (m < self.HI)))  # NaN fails every comparison: bad
        out = bad.any(0) if bad.shape[0] else torch.zeros(self.images, dtype=torch.bool)
        for row in self.whole:
            if row < bad.shape[0] and bool(bad[row, 0]):
                out[:] = True
        sat = ~(self.cond_estimate(k) <= self.COND_BOUND)  # NaN: saturated
        return out, sat & ~out

    def tripped(self):
        """-> bool tensor (images,): True where some tensor of that image left the half's range (or held inf / NaN)."""
        return self.verdict()[0]

    def saturated(self):
        return self.verdict()[1]

    def ok(self):
        t, s = self.verdict()
        return not bool(t.any() or s.any())


class _Scope(threading.local):
    """Per-thread state of the guarded scopes: two threads running forwards in one process must not share a guard."""
    guard = None     # the Planes16Guard of the running guarded scope (run_guarded), or None
    suppress = 0     # > 0 while a scope is being repeated on the bf16x6 kernels: nested scopes must not open a guard


_scope = _Scope()
_stats_lock = threading.Lock()
_stats = {"scopes": 0, "fallbacks": 0, "images": 0, "images_repeated": 0, "images_repeated_fp32conv": 0, "streak": 0,
          "warned": False, "slot_rows_shared": 0}


def _note_shared_row():
    with _stats_lock:
        _stats["slot_rows_shared"] += 1


def _count(images, repeated, exact=0):
    """repeated: images computed again on bf16x6 (range); exact: images computed again with the 3x3 convs in fp32 (conditioning)."""
    with _stats_lock:
        _stats["scopes"] += 1
        _stats["images"] += images
        _stats["images_repeated"] += repeated
        _stats["images_repeated_fp32conv"] += exact
        if repeated:
            _stats["fallbacks"] += 1
            _stats["streak"] += 1
            if _stats["streak"] >= 8 and not _stats["warned"]:
                _stats["warned"] = True
                warnings.warn("segmif_amd: the f16x3 range guard has tripped in 8 guarded forwards in a row - those images "
                              "run twice (f16x3, then bf16x6).  Activations outside [2^-13, 65504): consider "
                              "SEGMIF_CONV3X3=planes SEGMIF_LINEAR=bf16x6 for this model / data.", RuntimeWarning)
        else:
            _stats["streak"] = 0


def active_guard():
    return _scope.guard


def range_fallbacks():
    """Guarded scopes in which at least one image was repeated on the bf16x6 kernels."""
    return _stats["fallbacks"]


def range_stats():
    """-> dict: guarded scopes, scopes with a repeat, images seen, images repeated (f16x3_trip_rate = repeated / seen)."""
    with _stats_lock:
        d = {k: _stats[k] for k in ("scopes", "fallbacks", "images", "images_repeated", "images_repeated_fp32conv", "slot_rows_shared")}
    d["trip_rate"] = d["images_repeated"] / d["images"] if d["images"] else 0.0
    d["cond_repeat_rate"] = d["images_repeated_fp32conv"] / d["images"] if d["images"] else 0.0
    return d


def f16x3_enabled():
    return modes.get("conv3x3") == "planes16" or modes.get("linear") == "f16x3" or modes.get("attention") == "f16x3"


def run_guarded(fn, device, enabled=None, images=1, redo=None):
    """Run fn() with the f16x3 kernels available (enabled=None: if a mode asks for them): inside, active_guard() hands every
    producer of half pairs its row of range slots, one slot per image.  One read-back at the end.  If images left the
    half's exponent range: with redo given, `redo(out, idx)` recomputes just those batch elements (idx: LongTensor) on the
    bf16x6 kernels and returns the patched result; without it (or when every image tripped) fn() runs again as a whole,
    without a guard.  Nested calls join the outer scope (which does the checking); fn must be repeatable."""
    if enabled is None:
        enabled = f16x3_enabled()
    if _scope.guard is not None or _scope.suppress or not enabled:
        return fn()
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        # (r6) a hipGraph capture cannot hold the scope's host read-back: a standalone call recorded by the CALLER's
        # graph runs on the bf16x6 kernels (no range to guard, capturable); PairForward.capture installs a guard of its own
        # and checks it after each replay instead
        _scope.suppress += 1
        try:
            return fn()
        finally:
            _scope.suppress -= 1
    _scope.guard = guard = Planes16Guard(device, images)
    try:
        out = fn()
        bad, sat = guard.verdict()
    finally:
        _scope.guard = None
    return finish_guarded(out, bad, sat, fn, device, redo)


def finish_guarded(out, bad, sat, fn, device, redo=None):
    """The repeat half of a guarded scope, given its verdict (Planes16Guard.verdict()): images in `bad` left the half's range
    and are computed again on the bf16x6 kernels; images in `sat` (r5) stayed in range but reported an ill-conditioned CrossPath
    softmax and are computed again with the 3x3 convs in exact fp32 and (r6) CrossPath in GEMM form (below).  With
    `redo(out, idx)` only those images run again, else fn() as a whole."""
    nbad, nsat, n = int(bad.sum()), int(sat.sum()), int(bad.numel())
    _count(n, nbad, nsat)
    if nbad == 0 and nsat == 0:
        return out
    # What a conditioning repeat switches to: the 3x3 convs in exact fp32 (round 5: the over-exposed image-like pair,
    # tools/stats_bisect.py) AND, (r6), CrossPath in its GEMM form.  tools/r6_fn_bisect.py on the pair the full-size search found
    # (U[0,1) x 8, kappa 3 970): with the Gram form the result is 1.5e-3 .. 1.6e-3 from the all-exact-fp32 one WHATEVER the convs /
    # Linears / attention run on (fp32 included), with the GEMM form 2.4e-5 (bf16x6 or fp32 convs alike).  K^T V = Wk G Wv^T takes
    # the Gram matrix's rounding (fp32 sums inside a 1024-pixel run) times the cancellation of Wk y and Wv y; the GEMM form sums
    # k v^T directly (fp32 over 32 rows, fp64 across) - slower (three 128-wide tensors per call), only for the flagged pairs.
    _scope.suppress += 1
    try:
        if redo is None or nbad == n or nsat == n:
            del out
            if nsat:  # (a whole-batch repeat serves both kinds: exact convs + GEMM-form CrossPath, everything else on bf16x6)
                with modes.modes(conv3x3="fp32", crosspath="gemm"):
                    return fn()
            return fn()
        if nbad:
            out = redo(out, bad.nonzero().flatten().to(device))
        if nsat:
            with modes.modes(conv3x3="fp32", crosspath="gemm"):
                out = redo(out, sat.nonzero().flatten().to(device))
        return out
    finally:
        _scope.suppress -= 1


def install_guard(guard):
    """Low-level: make `guard` (or None) the active one WITHOUT run_guarded's read-back, returning the previous one - for a
    caller that does the read-back itself later (pipeline.PairForward records a hipGraph this way and checks after replay)."""
    prev, _scope.guard = _scope.guard, guard
    return prev


def run_unguarded(fn, images=1, repeated=None):
    """fn() on the bf16x6 kernels, counted as a range fallback of `repeated` of `images` images (for a caller that does its
    own guard handling, and for measurements of the bf16x6 path)."""
    _count(images, images if repeated is None else repeated)
    _scope.suppress += 1
    try:
        return fn()
    finally:
        _scope.suppress -= 1
