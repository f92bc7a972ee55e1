"""The rejection contract of the C ABI (every header under include/) as a table: for every entry point one VALID baseline argument
set and a list of single-argument mutations of it, each of which the entry point must refuse with SEGMIF_EINVAL (-22) before it
launches or calls into the HIP runtime.  tests/_abi_contract_child.py sends the mutations (never a baseline) in a process that
sees no GPU; tests/test_abi_contract_host.py reads its records.

Pointers are fake, non-null, 4096-byte aligned addresses: a rejected call never dereferences one, and an accepted one ends as a
HIP error code because the child has no device.  The one host pointer an entry point reads before it validates
(segmif_gauss_blur11_f32's taps) is a real array.

An argument carries a tag that says what it is; the tag generates the generic mutations:
    P16 / P8 / P    required pointer (16-byte / 8-byte / no alignment rule):  NULL, and the address + 4 where a rule applies
    O16 / O8 / O    optional pointer, given in the baseline:                  the address + 4 where a rule applies
    Z               optional pointer, NULL in the baseline:                   -
    N(v)            a count:                                                  0 and -1
    LD(v, w)        a pitch in floats over rows of width w:                   w - 4;  with vec=True also v + 2 (no multiple of 4)
    V(v)            any other value:                                          -
    A(vals, fill)   an array field of a descriptor, its count another field:  -   (`fill` holds a legal value for every slot and
                    `vals` go in front of it, so a row that mutates the count changes nothing else)
A descriptor entry (`struct`) also gets the row "desc=NULL": the first parameter itself.
`rows` adds the mutations that are particular to the entry point, each with the header sentence or the code line behind it.  A
row's argument may be a tuple of names with a tuple of values: a rule about two arguments together (H * W >= 2^31)."""
import ctypes
import functools

from segmif_amd import _lib as L

EINVAL = -22
ACT_END = 4  # one past SEGMIF_ACT_GELU


def P16(): return {"kind": "ptr", "align": 16, "req": True}
def P8(): return {"kind": "ptr", "align": 8, "req": True}
def P(): return {"kind": "ptr", "align": 0, "req": True}
def O16(): return {"kind": "ptr", "align": 16, "req": False}
def O8(): return {"kind": "ptr", "align": 8, "req": False}
def O(): return {"kind": "ptr", "align": 0, "req": False}
def Z(): return {"kind": "null"}
def N(v): return {"kind": "count", "v": v}
def LD(v, w, vec=False): return {"kind": "pitch", "v": v, "w": w, "vec": vec}
def V(v): return {"kind": "val", "v": v}
def HOST(vals): return {"kind": "host", "v": list(vals)}
def A(vals, fill): return {"kind": "array", "v": tuple(vals), "fill": tuple(fill)}


GENERIC = {
    "null": "a required pointer is NULL (header: 'Returns 0 on success, a hipError_t / negative SEGMIF_E* code otherwise')",
    "align": "header, Conventions: 'pointers must be 16-byte aligned where a vector path applies' (8 bytes for fp64 / int64 words)",
    "count0": "a count of 0 describes no problem", "count-1": "a negative count",
    "narrow": "a pitch below the row width makes rows overlap", "pitch4": "the vector path needs pitches that are multiples of 4 floats",
}


class Entry:
    """One baseline of one entry point.  args: [(name, tag)] in call order; with `struct`, the fields of the descriptor the first
    parameter points to, and `tail` the parameters after it."""

    def __init__(self, name, args, rows=(), struct=None, tail=(), variant=""):
        self.name, self.args, self.struct, self.tail, self.variant = name, list(args), struct, list(tail), variant
        self.extra = [tuple(r) for r in rows]
        names = [a for a, _ in self.args + self.tail] + (["desc"] if struct is not None else [])
        assert len(names) == len(set(names)), (name, names)
        for arg, _, _ in self.extra:
            assert all(a in names for a in (arg if isinstance(arg, tuple) else (arg,))), (name, arg)

    @property
    def key(self):
        return self.name + ("#" + self.variant if self.variant else "")

    def baseline(self):
        """{name: value}; pointers get distinct fake addresses by position; "desc" stands for the descriptor itself (None = NULL)"""
        out = {} if self.struct is None else {"desc": "given"}
        for i, (a, t) in enumerate(self.args + self.tail):
            k = t["kind"]
            out[a] = (0x10000000 + 0x100000 * (i + 1)) if k == "ptr" else None if k == "null" else t["v"]
        return out

    def mutations(self):
        """[(label, arg, value, reason)]"""
        base, out = self.baseline(), []
        if self.struct is not None:
            out.append(("desc=NULL", "desc", None, GENERIC["null"]))
        for a, t in self.args + self.tail:
            k = t["kind"]
            if k == "ptr":
                if t["req"]:
                    out.append((f"{a}=NULL", a, None, GENERIC["null"]))
                if t["align"]:
                    out.append((f"{a}+4", a, base[a] + 4, GENERIC["align"]))
            elif k == "count":
                out.append((f"{a}=0", a, 0, GENERIC["count0"]))
                out.append((f"{a}=-1", a, -1, GENERIC["count-1"]))
            elif k == "pitch":
                out.append((f"{a}={t['w'] - 4}", a, t["w"] - 4, GENERIC["narrow"]))
                if t["vec"]:
                    out.append((f"{a}={t['v'] + 2}", a, t["v"] + 2, GENERIC["pitch4"]))
        for a, v, why in self.extra:
            shown = "NULL" if v is None else (hex(v) if isinstance(v, int) and v > 1 << 20 else v)
            out.append((f"{','.join(a) if isinstance(a, tuple) else a}={shown}", a, v, why))
        labels = [m[0] for m in out]
        assert len(labels) == len(set(labels)), (self.key, labels)
        return out

    def call(self, lib, values, keep):
        """the entry point on `values` ({name: value}); `keep` holds host arrays alive"""
        fn = getattr(lib, self.name)
        flat = self.args if self.struct is None else self.tail
        types = fn.argtypes if self.struct is None else fn.argtypes[1:]
        assert len(types) == len(flat), (self.key, len(types), len(flat))

        def conv(tag, v, ctype):
            if tag["kind"] == "host" and v is not None:
                arr = (ctypes.c_float * len(v))(*v)
                keep.append(arr)
                return arr
            if isinstance(v, int) and (ctype is ctypes.c_char_p or hasattr(ctype, "contents")):  # a typed pointer parameter
                return ctypes.cast(ctypes.c_void_p(v), ctype)
            return v
        tail = [conv(t, values[a], c) for (a, t), c in zip(flat, types)]
        if self.struct is None:
            return fn(*tail)
        if values["desc"] is None:
            return fn(None, *tail)
        d = self.struct()
        keep.append(d)
        assert [a for a, _ in self.args] == [f[0] for f in self.struct._fields_], self.key
        for a, t in self.args:
            if t["kind"] == "array":  # (a tuple cannot be assigned to a ctypes array field)
                for i, x in enumerate(tuple(values[a]) + t["fill"][len(values[a]):]):
                    getattr(d, a)[i] = x
            else:
                setattr(d, a, values[a] if values[a] is not None else (None if t["kind"] in ("ptr", "null") else 0))
        return fn(ctypes.byref(d), *tail)


S = ("stream", Z())
E = []


def add(*a, **k):
    E.append(Entry(*a, **k))


# ---------------------------------------------------------------------------------------------------------------- igemm.hip
def _igemm(**over):
    f = dict(in_=P(), in2=Z(), wt=P16(), bias=O(), res=Z(), prelu=Z(), out=P(), M=N(64), N=N(64), K=N(64), lda=LD(64, 64), lda2=V(0),
             K1=V(0), ldo=LD(64, 64), ldr=V(0), H=V(8), W=V(8), Cin=V(64), KH=V(1), KW=V(1), stride=V(1), pad=V(0), dil=V(1), OH=V(8),
             OW=V(8), act=V(0), nz=V(0), in_zstride=V(0), in2_zstride=V(0), wt_zstride=V(0), out_zstride=V(0), res_zstride=V(0),
             tile=V(-1), nz2=V(0), ldw=V(0), in_zstride2=V(0), wt_zstride2=V(0), out_zstride2=V(0), res_zstride2=V(0),
             workspace=Z(), workspace_floats=V(0), ln_gamma=Z(), ln_beta=Z(), ln_eps=V(1e-5), planes_out=Z(), planes_chunks=V(0),
             planes_chunk0=V(0), planes_f16=V(0), planes_amax=Z(), planes_amax_images=V(0), relu_mask=Z(), ld_mask=V(0),
             split_f16=V(0), split_in_amax=Z(), split_in_amax_n=V(0), split_out_amax=Z(), split_out_amax_n=V(0),
             wgrad_dy_amax=Z(), wgrad_dy_amax_n=V(0), mask_zstride=V(0))
    f.update(over)
    order = [n for n, _ in L.SegmifIgemm._fields_]
    return [(n, f[n]) for n in order]


_CONV3 = dict(K=N(288), lda=LD(32, 32), Cin=V(32), KH=V(3), KW=V(3), pad=V(1), N=N(32), ldo=LD(32, 32))
PR = 0x7f000000  # an aligned address for a pointer a row switches on

add("segmif_igemm_f32", _igemm(), struct=L.SegmifIgemm, tail=[S], variant="dense", rows=[
    ("act", 2, "header: 'prelu: device scalar slope, used when act == SEGMIF_ACT_PRELU' - PReLU without a slope"),
    ("act", ACT_END, "header: 'activation codes for fused epilogues' end at SEGMIF_ACT_GELU = 3"),
    ("ldw", 66, "igemm.hip: 'if (k.ldw % 4) return SEGMIF_EINVAL' (16-byte weight loads)"),
    ("res", PR, "igemm.hip: 'if (d->res && d->ldr <= 0)' - a residual needs its pitch"),
    ("tile", 15, "header: 'tile: -1 = auto; otherwise index into the tile table' (segmif_igemm_num_tiles() = 15 entries)"),
    ("tile", 14, "header: tile 14's 'geometry limits are those of the halo tiles (3x3, stride 1, ...), anything else returns SEGMIF_EINVAL'"),
    ("tile", 9, "the halo tiles 9 / 10 take 3x3 stride-1 convolutions only"),
    ("split_f16", 1, "igemm.hip: '(d->split_f16 || d->split_out_amax) && !(halo && tile == kSplitTile)': split 3x3 kernel only"),
    ("split_out_amax", PR, "igemm.hip: split_out_amax is the split 3x3 tile's"),
    ("relu_mask", PR, "igemm.hip: 'if (k.mask && k.ldm < d->N)' - mask pitch below N (ld_mask = 0)"),
    ("ln_gamma", PR, "igemm.hip: 'k.ln_gamma && (!k.ln_beta ...' - a fused LayerNorm needs both parameters"),
    ("planes_out", PR, "header: the planes copy needs 'a convolution (not a plain 1x1 / Linear problem)'"),
])
add("segmif_igemm_f32", _igemm(res=O(), ldr=LD(64, 64)), struct=L.SegmifIgemm, tail=[S], variant="dense_res", rows=[
    ("ldr", 0, "igemm.hip: 'if (d->res && d->ldr <= 0)'"),
])
add("segmif_igemm_f32", _igemm(in_=P16(), in2=O16(), K1=V(32), lda=LD(32, 32, True), lda2=LD(32, 32, True)), struct=L.SegmifIgemm, tail=[S],
    variant="dense2", rows=[
    ("K1", 16, "igemm.hip, two sources: 'd->K1 % 32 != 0'"),
    ("K", 72, "igemm.hip, two sources: '(d->K - d->K1) % 16 != 0'"),
    ("KH", 3, "header: 'dense, two sources ... when in2 != NULL' - in2 with a convolution"),
    ("stride", 2, "in2 with a (strided 1x1) convolution"),
])
add("segmif_igemm_f32", _igemm(out=P16(), res=O16(), ldr=LD(64, 64, True), ldo=LD(64, 64, True), ln_gamma=O(), ln_beta=P()),
    struct=L.SegmifIgemm, tail=[S], variant="fused_ln", rows=[
    ("N", 68, "header: 'optional fused LayerNorm over the output row (N must be 64, act NONE)'"),
    ("act", 1, "header: 'optional fused LayerNorm over the output row (N must be 64, act NONE)'"),
    ("relu_mask", PR, "header, relu_mask: 'no fused LayerNorm / planes copy / second batch level'"),
    ("tile", 0, "igemm.hip: 'the fused LayerNorm needs a wave tile spanning all 64 columns' (tile 7 or 8)"),
    ("planes_out", PR, "header, planes copy: needs nz <= 1 and no fused LayerNorm (igemm.hip: '... || k.ln_gamma || ...')"),
    ("out_zstride", 2, "igemm.hip: 'the fused LayerNorm epilogue only exists in its 16-byte form'"),
])
add("segmif_igemm_f32", _igemm(relu_mask=O16(), ld_mask=LD(64, 64, True), out=P16(), ldo=LD(64, 64, True)), struct=L.SegmifIgemm, tail=[S],
    variant="masked", rows=[
    ("nz2", 2, "header, relu_mask: 'no ... second batch level'"),
    ("mask_zstride", 2, "header, relu_mask: served by the 16-byte epilogue (mask_zstride a multiple of 4)"),
    ("N", 62, "header, relu_mask: 'N, ldo, ld_mask multiples of 4'"),
])
add("segmif_igemm_f32", _igemm(M=N(128), K=N(16), Cin=V(16), lda=LD(16, 16), H=V(16), W=V(16), stride=V(2), N=N(16), ldo=LD(16, 16, True),
                               out=O16(), planes_out=O16(), planes_chunks=V(4), planes_f16=V(1), planes_amax=O(),
                               planes_amax_images=V(2)),
    struct=L.SegmifIgemm, tail=[S], variant="planes", rows=[
    ("nz", 2, "header, planes copy: 'Needs the 16-byte epilogue ..., nz <= 1'"),
    ("stride", 1, "header, planes copy: 'a convolution (not a plain 1x1 / Linear problem)'"),
    ("N", 24, "header, planes copy: 'conv output (B, OH, OW, N) with N % 16 == 0'"),
    ("planes_chunk0", -1, "header: chunks [planes_chunk0, planes_chunk0 + N/16) of a planes buffer of planes_chunks"),
    ("planes_chunk0", 4, "header: chunks [planes_chunk0, planes_chunk0 + N/16) of a planes buffer of planes_chunks"),
    ("planes_chunks", 0, "header: chunks [planes_chunk0, planes_chunk0 + N/16) of a planes buffer of planes_chunks"),
    ("planes_amax_images", 3, "header: 'planes_amax_images == B: one range slot per batch element ... or <= 1'"),
    ("M", 100, "igemm.hip, planes copy: 'd->M % ((long long)d->OH * d->OW)' - whole images"),
])
add("segmif_igemm_f32", _igemm(M=N(128), K=N(16), Cin=V(16), lda=LD(16, 16), H=V(16), W=V(16), stride=V(2), N=N(16), ldo=LD(16, 16, True),
                               out=O16(), planes_out=O16(), planes_chunks=V(4)),
    struct=L.SegmifIgemm, tail=[S], variant="planes_bf16", rows=[
    ("OH", 0, "header: 'geometry of segmif_planes_dims(OH, OW)', which refuses an empty image"),
    ("OW", -1, "header: 'geometry of segmif_planes_dims(OH, OW)', which refuses an empty image"),
])
add("segmif_igemm_f32", _igemm(in_=P16(), tile=V(14), **_CONV3), struct=L.SegmifIgemm, tail=[S], variant="tile14", rows=[
    ("stride", 2, "header: tile 14 'geometry limits are those of the halo tiles (3x3, stride 1, dilation 1|2, pad = dilation, N <= 256)'"),
    ("dil", 3, "header: tile 14: dilation 1|2"), ("pad", 0, "header: tile 14: pad = dilation"), ("N", 260, "header: tile 14: N <= 256"),
    ("Cin", 24, "header, segmif_conv3x3_split_pack: 'Cin % 16 == 0'"),
    ("nz", 2, "igemm.hip: the halo tiles take nz == 1"), ("in2", PR, "in2 with a convolution"),
    ("split_f16", 1, "header: the f16x3 form needs split_in_amax, 'split_in_amax_n (1..64) device words'"),
])
add("segmif_igemm_f32", _igemm(in_=P16(), tile=V(14), split_f16=V(1), split_in_amax=P(), split_in_amax_n=V(4), split_out_amax=O(),
                               split_out_amax_n=V(4), **_CONV3), struct=L.SegmifIgemm, tail=[S], variant="tile14_f16", rows=[
    ("split_in_amax_n", 0, "header: 'split_in_amax_n (1..64) device words'"), ("split_in_amax_n", 65, "header: 'split_in_amax_n (1..64)'"),
    ("split_out_amax_n", 3, "header: split_out_amax_n 'a power of two <= 64'"), ("split_out_amax_n", 128, "header: 'a power of two <= 64'"),
])
add("segmif_pack_conv_weight", [("src", P()), ("dst", P()), ("N", N(8)), ("Cin", N(8)), ("KH", N(3)), ("KW", N(3)), S])

# ------------------------------------------------------------------------------------------ gemm_split.hip / gemm_pairs.hip
_GS = [("a", P16()), ("w", P16()), ("bias", O16()), ("res", O16()), ("prelu", Z()), ("out", P16()), ("M", N(64)), ("N", N(64)),
       ("K", N(64)), ("lda", LD(64, 64, True)), ("ldo", LD(64, 64, True)), ("ldr", LD(64, 64, True)), ("act", V(0)), ("patch_k", V(0)),
       ("patch_st", V(0)), ("patch_pad", V(0)), ("patch_H", V(0)), ("patch_W", V(0))]
_GS_ROWS = [("K", 48, "header: 'K % 32 == 0'"), ("N", 62, "gemm_split.hip: 'float4 epilogue' - N % 4"),
            ("act", 2, "PReLU without a slope"), ("act", ACT_END, "header: activation codes end at SEGMIF_ACT_GELU = 3"),
            ("ldr", 0, "gemm_split.hip: 'd->res && (d->ldr <= 0 ...'")]
_GS_PATCH = [("a", P16()), ("w", P16()), ("bias", Z()), ("res", Z()), ("prelu", Z()), ("out", P16()), ("M", N(32)), ("N", N(64)),
             ("K", V(288)), ("lda", V(32)), ("ldo", LD(64, 64, True)), ("ldr", V(0)), ("act", V(0)), ("patch_k", V(3)),
             ("patch_st", V(2)), ("patch_pad", V(1)), ("patch_H", V(8)), ("patch_W", V(8))]
_GS_PATCH_ROWS = [("patch_st", 0, "header, patch mode: a stride of at least 1"), ("patch_pad", -1, "a negative padding"),
                  ("patch_pad", 3, "gemm_split.hip: 'pad >= kk'"), ("patch_H", 0, "gemm_split.hip: 'd->patch_H + 2 * pad < kk'"),
                  ("patch_W", 0, "gemm_split.hip: 'd->patch_W + 2 * pad < kk'"), ("K", 256, "header: 'K = k * k * C'"),
                  ("lda", 48, "header: 'lda = C, C % 32 == 0'"), ("M", 33, "header: 'M = B * OH * OW'")]
add("segmif_gemm_split_f32", _GS, struct=L.SegmifGemmSplit, tail=[S], rows=_GS_ROWS)
add("segmif_gemm_split_f32", _GS_PATCH, struct=L.SegmifGemmSplit, tail=[S], variant="patch", rows=_GS_PATCH_ROWS)
_A16 = [("amax", O()), ("amax_images", V(2)), S]
add("segmif_gemm_split16_f32", _GS, struct=L.SegmifGemmSplit, tail=_A16, rows=_GS_ROWS + [
    ("amax_images", 0, "header: 'the M rows are amax_images whole images'"), ("amax_images", 3, "header: 'amax_images whole images of M / amax_images rows'")])
add("segmif_gemm_split16_f32", _GS_PATCH, struct=L.SegmifGemmSplit, tail=_A16, variant="patch", rows=_GS_PATCH_ROWS)
for nm in ("segmif_gemm_split_pack", "segmif_gemm_split16_pack"):
    add(nm, [("w", P()), ("N", N(64)), ("K", N(64)), ("ldw", LD(64, 64)), ("out", P()), S], rows=[("K", 48, "header: 'K % 32 == 0' (weight_bytes = 0)")])
add("segmif_gemm_pairs_pack", [("w", P()), ("N", N(64)), ("K", N(64)), ("ldw", LD(64, 64)), ("out", P16()), S],
    rows=[("K", 40, "gemm_pairs.hip: K a multiple of the 16-wide K step (weight_bytes = 0)")])
_GP = [("a", P16()), ("w", P16()), ("bias", O16()), ("res", O16()), ("prelu", Z()), ("out", P16()), ("M", N(64)), ("lda_bytes", V(256)),
       ("N", N(64)), ("K", N(64)), ("ldo", LD(64, 64, True)), ("ldr", LD(64, 64, True)), ("act", V(0)), ("patch_k", V(0)), ("patch_st", V(0)),
       ("patch_pad", V(0)), ("patch_H", V(0)), ("patch_W", V(0)), ("patch_C", V(0)), ("tile_rows", V(0))]
add("segmif_gemm_pairs_f32", _GP, struct=L.SegmifGemmPairs, tail=[S], rows=[
    ("K", 72, "header: a row of K values is K / 16 groups - K % 16"), ("N", 62, "gemm_pairs.hip: N % 4 (16-byte epilogue)"),
    ("lda_bytes", 240, "header: 'lda_bytes: row pitch of A in bytes (>= 4 K, a multiple of 16)'"),
    ("lda_bytes", 264, "header: 'lda_bytes: ... a multiple of 16'"), ("act", 2, "PReLU without a slope"),
    ("act", ACT_END, "header: activation codes end at SEGMIF_ACT_GELU = 3"), ("ldr", 0, "gemm_pairs.hip: 'd->res && (d->ldr <= 0 ...'"),
    ("tile_rows", 64, "header: 'tile_rows: 0 = chosen by size, 128 | 256 forces one'"),
    ("tile_rows", 129, "header: 'tile_rows: 0 = chosen by size, 128 | 256 forces one'"),
    ("tile_rows", -1, "header: 'tile_rows: 0 = chosen by size, 128 | 256 forces one'")])
add("segmif_gemm_pairs_f32", [("a", P16()), ("w", P16()), ("bias", Z()), ("res", Z()), ("prelu", Z()), ("out", P16()), ("M", N(32)),
                              ("lda_bytes", V(0)), ("N", N(64)), ("K", V(144)), ("ldo", LD(64, 64, True)), ("ldr", V(0)), ("act", V(0)),
                              ("patch_k", V(3)), ("patch_st", V(2)), ("patch_pad", V(1)), ("patch_H", V(8)), ("patch_W", V(8)),
                              ("patch_C", V(16)), ("tile_rows", V(128))], struct=L.SegmifGemmPairs, tail=[S], variant="patch", rows=[
    ("patch_st", 0, "a stride of at least 1"), ("patch_pad", -1, "a negative padding"), ("patch_pad", 3, "gemm_pairs.hip: 'pad >= kk'"),
    ("patch_H", 0, "'d->patch_H + 2 * pad < kk'"), ("patch_W", 0, "'d->patch_W + 2 * pad < kk'"), ("K", 128, "header: 'K = k k C'"),
    ("patch_C", 24, "header: 'patch_C % 16 == 0'"), ("patch_C", 0, "header: 'patch_C % 16 == 0', C > 0"), ("M", 33, "M = B * OH * OW")])
add("segmif_pairs_from_f32", [("x", P16()), ("ldx", LD(64, 64, True)), ("y", P16()), ("ldy_bytes", V(256)), ("rows", N(8)), ("C", N(64)),
                              ("amax", O()), ("amax_images", V(2)), S], rows=[
    ("C", 40, "header: 'C % 16 == 0'"), ("ldy_bytes", 240, "pairs rows of 4 C bytes: a pitch below them"), ("ldy_bytes", 264, "pairs pitch a multiple of 16 bytes"),
    ("amax_images", 0, "header: 'amax_images whole images'"), ("amax_images", 3, "header: 'amax_images whole images of rows / amax_images rows each'")])
add("segmif_pairs_to_f32", [("x", P16()), ("ldx_bytes", V(256)), ("y", P16()), ("ldy", LD(64, 64, True)), ("rows", N(8)), ("C", N(64)), S],
    rows=[("C", 40, "header: 'C % 16 == 0'"), ("ldx_bytes", 240, "a pitch below the pairs row"), ("ldx_bytes", 264, "pairs pitch a multiple of 16 bytes")])

# ------------------------------------------------------------------------------------------------------ conv3x3_planes.hip
add("segmif_planes_dims", [("H", N(8)), ("W", N(32)), ("Hp", P()), ("Wp", P())])
for nm in ("segmif_planes_zero_border", "segmif_planes16_zero_border"):
    add(nm, [("planes", P()), ("B", N(1)), ("H", N(8)), ("W", N(32)), ("chunks", N(4)), S])
_PF = [("x", P16()), ("ldx", LD(64, 32, True)), ("planes", P()), ("B", N(2)), ("H", N(8)), ("W", N(32)), ("chunks", V(4)), ("chunk0", V(1)),
       ("nconv", N(2))]
_PF_ROWS = [("chunk0", -1, "header: chunks [chunk0, chunk0 + nconv) of the buffer"), ("chunk0", 3, "header: chunks [chunk0, chunk0 + nconv) of the buffer"),
            ("chunks", 2, "header: chunks [chunk0, chunk0 + nconv) of the buffer")]
add("segmif_planes_from_f32", _PF + [S], rows=_PF_ROWS)
add("segmif_planes16_from_f32", _PF + [("amax", O()), ("amax_images", V(2)), S],
    rows=_PF_ROWS + [("amax_images", 3, "header: 'amax[b] ... when amax_images == B, amax[0] when amax_images == 1'"), ("amax_images", 0, "amax_images is B or 1")])
for nm in ("segmif_planes_pack_weight", "segmif_planes16_pack_weight"):
    add(nm, [("packed", P()), ("N", N(32)), ("Cin", N(64)), ("taps", V(9)), ("ldw", LD(576, 576)), ("out", P()), S], rows=[
        ("N", 48, "header: 'N % 32 == 0'"), ("Cin", 24, "header: 'Cin % 16 == 0'"), ("taps", 3, "header: 'taps = 9 for a 3x3 conv, 1 for a 1x1 conv'")])
_CP = [("planes_in", P()), ("planes_out", O()), ("wt", P()), ("bias", O16()), ("prelu", Z()), ("out", O16()), ("ldo", LD(32, 32, True)), ("B", N(2)),
       ("H", N(8)), ("W", N(32)), ("cin", N(64)), ("dil", V(1)), ("in_chunks", V(6)), ("out_chunks", V(6)), ("out_chunk0", V(4)), ("act", V(1)),
       ("w1", Z()), ("bias1", Z()), ("res", Z()), ("out1", Z()), ("ldr", V(0)), ("ldo1", V(0)), ("act1", V(0)), ("res_from_planes", V(0))]
_CP_ROWS = [("cin", 24, "header: the first `cin` channels of 16-channel chunks"), ("dil", 3, "header: 'dilation 1 | 2'"), ("dil", 0, "header: 'dilation 1 | 2'"),
            ("act", 2, "PReLU without a slope"), ("act", 3, "header: 'bias + act (NONE | RELU | PRELU)'"), ("act", ACT_END, "one past the enum"),
            ("in_chunks", 3, "conv3x3_planes.hip: 'k.nchunks > k.in_total'"), ("out_chunk0", -1, "header: 'two more planes chunks (planes_out / out_chunk0)'"),
            ("out_chunk0", 5, "the two output chunks must fit out_chunks")]
_CPF = [(n, {"w1": O(), "bias1": O16(), "res": O16(), "out1": P16(), "ldr": LD(64, 64, True), "ldo1": LD(64, 64, True), "act1": V(1)}.get(n, t))
        for n, t in _CP]
_CPF_ROWS = [("act1", 2, "conv3x3_planes.hip, fused tail: act1 NONE | RELU"), ("act1", ACT_END, "one past the enum")]
add("segmif_conv3x3_planes_bf16x6", _CP, struct=L.SegmifConvPlanes, tail=[S], rows=_CP_ROWS)
add("segmif_conv3x3_planes_bf16x6", _CPF, struct=L.SegmifConvPlanes, tail=[S], variant="fused_tail", rows=_CPF_ROWS)
add("segmif_conv3x3_planes_f16x3", _CP, struct=L.SegmifConvPlanes, tail=_A16, rows=_CP_ROWS + [
    ("amax_images", 3, "header: 'amax[b] for batch element b when amax_images == B, amax[0] when amax_images == 1'"), ("amax_images", 0, "amax_images is B or 1")])
add("segmif_conv3x3_planes_f16x3", _CPF, struct=L.SegmifConvPlanes, tail=_A16, variant="fused_tail", rows=_CPF_ROWS)
add("segmif_conv3x3_planes_bf16x6", [(n, {"planes_out": P(), "out": Z(), "ldo": V(0), "in_chunks": V(8), "out_chunks": V(8), "out_chunk0": V(2)}.get(n, t)) for n, t in _CP], struct=L.SegmifConvPlanes, tail=[S],
    variant="planes_only", rows=[("planes_out", 0x10000000 + 0x100000, "conv3x3_planes.hip: 'would overwrite its own input' (planes_out == planes_in, out_chunk0 < cin / 16)")])
add("segmif_conv3x3_c1_f16x3", [("x", P()), ("w", P()), ("bias", O()), ("prelu", Z()), ("act", V(1)), ("planes", O16()), ("chunks", V(6)), ("chunk0", V(2)),
                                ("out", O16()), ("ldo", LD(64, 64, True)), ("B", N(2)), ("H", N(8)), ("W", N(32)), ("amax", O()), ("amax_images", V(2)), S], rows=[
    ("act", 2, "PReLU without a slope"), ("act", 3, "conv3x3_planes.hip: 'act > SEGMIF_ACT_PRELU'"), ("act", -1, "below the enum"),
    ("chunk0", -1, "header: 'receiving chunks [chunk0, chunk0 + 4)'"), ("chunk0", 3, "header: 'receiving chunks [chunk0, chunk0 + 4)' of `chunks`"),
    ("amax_images", 3, "header: 'amax_images = B words, one per image, or 1'")])
add("segmif_conv3x3_c1_f16x3", [("x", P()), ("w", P()), ("bias", Z()), ("prelu", Z()), ("act", V(0)), ("planes", Z()), ("chunks", V(0)), ("chunk0", V(0)),
                                ("out", P16()), ("ldo", LD(64, 64, True)), ("B", N(1)), ("H", N(1)), ("W", N(1)), ("amax", Z()), ("amax_images", V(0)), S],
    variant="rows_only")  # out = NULL here: 'Outputs, at least one'

# -------------------------------------------------------------------------------------------------------------- rowops.hip
add("segmif_layernorm_f32", [("x", P16()), ("gamma", P16()), ("beta", P16()), ("y", P16()), ("rows", N(4)), ("C", N(64)), ("ldx", LD(64, 64, True)),
                             ("ldy", LD(64, 64, True)), ("eps", V(1e-5)), S],
    rows=[("C", 66, "header: 'C % 4 == 0, C <= 1024'"), ("C", 1028, "header: 'C % 4 == 0, C <= 1024'")])
add("segmif_layernorm_pairs_f32", [("x", P16()), ("gamma", P16()), ("beta", P16()), ("y", P16()), ("rows", N(4)), ("C", N(64)), ("ldx", LD(64, 64, True)),
                                   ("ldy", LD(64, 64, True)), ("eps", V(1e-5)), ("amax", O()), ("amax_images", V(2)), ("amax_sub", V(2)), ("amax_pitch", V(2)), S],
    rows=[("C", 72, "header: 'C % 16 == 0'"), ("C", 1040, "C <= 1024"), ("amax_images", 0, "header: 'rows / amax_images rows per image'"),
          ("amax_images", 3, "header: 'rows / amax_images rows per image'"), ("amax_sub", 3, "header: 'amax_sub (a power of two)'"),
          ("amax_sub", 0, "header: 'amax_sub (a power of two)'"), ("amax_pitch", 1, "header: 'amax_pitch words apart (>= amax_images'")])
add("segmif_add_layernorm_f32", [("x", P16()), ("branch", P16()), ("scale", O()), ("rows_per_image", V(2)), ("gamma", P16()), ("beta", P16()), ("sum", P16()),
                                 ("y", P16()), ("rows", N(4)), ("C", N(64)), ("ldx", LD(64, 64, True)), ("ldb", LD(64, 64, True)), ("lds", LD(64, 64, True)),
                                 ("ldy", LD(64, 64, True)), ("eps", V(1e-5)), S],
    rows=[("C", 66, "header, LayerNorm: 'C % 4 == 0, C <= 1024'"), ("C", 1028, "C <= 1024"), ("rows_per_image", 0, "header: scale[row / rows_per_image]"),
          ("rows_per_image", 3, "rowops.hip: 'rows % rows_per_image' - whole images")])
for nm in ("segmif_dwconv3x3_gelu_f32", "segmif_dwconv3x3_bias_f32"):
    add(nm, [("x", P16()), ("w9", P16()), ("bias", P16()), ("y", P16()), ("B", N(1)), ("H", N(4)), ("W", N(4)), ("C", N(8)), S],
        rows=[("C", 6, "header: 'C % 4 == 0'")])
add("segmif_dwconv3x3_gelu_pairs_f32", [("x", P16()), ("w9", P16()), ("bias", P16()), ("y", P16()), ("B", N(2)), ("H", N(4)), ("W", N(4)), ("C", N(16)),
                                        ("amax", O()), ("amax_images", V(2)), S],
    rows=[("C", 24, "header: 'C % 16 == 0'"), ("amax_images", 3, "rowops.hip: amax_images is 1 or B"), ("amax_images", 0, "amax_images is 1 or B")])
add("segmif_conv3x3_c32to1_f32", [("x", P16()), ("ldx", LD(32, 32, True)), ("wt", P16()), ("bias", O()), ("prelu", Z()), ("act", V(1)), ("y", P()), ("B", N(1)),
                                  ("H", N(4)), ("W", N(4)), S],
    rows=[("act", 2, "PReLU without a slope"), ("act", 3, "header: 'act (NONE | RELU | PRELU)'"), ("act", ACT_END, "one past the enum")])
add("segmif_bilinear_nhwc_f32", [("x", P()), ("y", P()), ("B", N(1)), ("IH", N(2)), ("IW", N(2)), ("OH", N(4)), ("OW", N(4)), ("C", N(8)), ("ldx", LD(8, 8)),
                                 ("ldo", LD(8, 8)), S],
    rows=[("OH", 65536, "rowops.hip: 'OH > 65535 || B > 65535' (grid limits)"), ("B", 65536, "rowops.hip: 'OH > 65535 || B > 65535' (grid limits)")])
add("segmif_bilinear_argmax_i32", [("x", P()), ("labels", P()), ("B", N(1)), ("IH", N(2)), ("IW", N(2)), ("OH", N(4)), ("OW", N(4)), ("C", N(9)), ("ldx", LD(13, 9)), S],
    rows=[("OH", 65536, "the grid's y / z limits, as segmif_bilinear_nhwc_f32 checks them"), ("B", 65536, "the grid's y / z limits, as segmif_bilinear_nhwc_f32 checks them")])
add("segmif_upsum_act_nhwc_f32", [("base", O16()), ("ldb", LD(8, 8, True)), ("x0", O16()), ("ih0", V(2)), ("iw0", V(2)), ("x1", Z()), ("ih1", V(0)), ("iw1", V(0)),
                                  ("x2", Z()), ("ih2", V(0)), ("iw2", V(0)), ("bias", O16()), ("out", P16()), ("ldo", LD(8, 8, True)), ("B", N(1)), ("OH", N(4)),
                                  ("OW", N(4)), ("C", N(8)), ("act", V(1)), S],
    rows=[("C", 6, "header: 'C % 4 == 0'"), ("act", 2, "header: 'act NONE or RELU'"), ("act", ACT_END, "one past the enum"), ("ih0", 0, "a given source needs its size"),
          ("iw0", -1, "a given source needs its size"), ("OH", 65536, "grid limit"), ("B", 65536, "grid limit")])
add("segmif_nchw_to_nhwc_f32", [("x", P()), ("y", P()), ("B", N(1)), ("C", N(8)), ("HW", N(16)), ("ldo", LD(12, 8)), S])
add("segmif_nhwc_to_nchw_f32", [("x", P()), ("y", P()), ("B", N(1)), ("C", N(8)), ("HW", N(16)), ("ldx", LD(12, 8)), S])
add("segmif_seg_normalize_f32", [("x", P()), ("y", P()), ("B", N(1)), ("H", N(4)), ("W", N(4)), S])
add("segmif_pointwise2_f32", [("a", P16()), ("lda", LD(8, 8, True)), ("b", P16()), ("ldb", LD(8, 8, True)), ("y", P16()), ("ldy", LD(8, 8, True)), ("rows", N(4)),
                              ("C", N(8)), ("mode", V(1)), S],
    rows=[("C", 6, "header: 'C % 4 == 0'"), ("mode", 3, "header: modes 0, 1, 2"), ("mode", -1, "header: modes 0, 1, 2")])
add("segmif_pointwise2_bwd_f32", [("dy", P16()), ("ldy", LD(8, 8, True)), ("a", P16()), ("lda", LD(8, 8, True)), ("b", P16()), ("ldb", LD(8, 8, True)), ("da", P16()),
                                  ("ldda", LD(8, 8, True)), ("db", P16()), ("lddb", LD(8, 8, True)), ("rows", N(4)), ("C", N(8)), ("mode", V(1)), S],
    rows=[("C", 6, "header: 'C % 4 == 0'"), ("mode", 0, "header: 'Mode 0 (a + b) has no kernel'"), ("mode", 3, "header: 'Backward of modes 1 and 2'")])
add("segmif_fuse_ycrcb_f32", [("vis", P()), ("yf", P()), ("out", P()), ("B", N(1)), ("HW", N(16)), S])
add("segmif_color3_f32", [("in_", P()), ("ysrc", Z()), ("out", P()), ("B", N(1)), ("HW", N(16)), ("mode", V(0)), ("nout", V(3)), S],
    rows=[("mode", 4, "header: modes 0 .. 3"), ("mode", -1, "header: modes 0 .. 3"), ("nout", 1, "header: 'nout = 1' with mode 3 only"), ("nout", 2, "nout is 3 (or 1 with mode 3)"),
          ("ysrc", PR, "header: 'mode 1 ... ysrc != NULL supplies channel 0' - ysrc with another mode")])
add("segmif_argmax_nhwc_i32", [("x", P()), ("labels", P()), ("rows", N(4)), ("C", N(9)), ("ldx", LD(13, 9)), S])
add("segmif_gauss_blur11_f32", [("x", P()), ("y", P()), ("planes", N(1)), ("H", N(4)), ("W", N(4)), ("taps11", HOST([1.0 / 11] * 11)), S],
    rows=[("taps11", None, GENERIC["null"])])

# ----------------------------------------------------------------------------------------------------------- attention*.hip
_AT = [("B", N(1)), ("heads", N(2)), ("N", N(8)), ("Nk", N(4)), ("hd", V(64)), ("ldq", LD(128, 128, True)), ("ldkv", LD(256, 256, True)),
       ("ldo", LD(128, 128, True)), ("scale", V(0.125))]
_AT_WHY = "header: q '(B, N, ldq) with head h at columns [h*hd, (h+1)*hd)'; k = kv, v = kv + C of a (B, Nk, ldkv) tensor"
add("segmif_sr_attention_f32", [("q", P16()), ("k", P16()), ("v", P16()), ("out", P16())] + _AT + [S],
    rows=[("hd", 48, "header: 'hd in {32, 64}'"), ("hd", 0, "header: 'hd in {32, 64}'"), ("hd", 128, "header: 'hd in {32, 64}'")])
_ATS = [("q", P16()), ("k", P8()), ("v", P8()), ("out", P16()), ("workspace", P16())]
_AT8 = [(n, LD(256, 256) if n == "ldkv" else t) for n, t in _AT]  # the pack kernel reads K / V in 8-byte pairs: ldkv even, k / v 8-byte aligned
_ATS_ROWS = [("hd", 32, "header: 'hd == 64 only'"), ("hd", 65, "header: 'hd == 64 only'"), ("ldkv", 257, "attention_split.hip: '(ldkv & 1)' - 8-byte loads of K / V")]
_ATS_AM = [("amax_images", 3, "header: 'amax[image] (amax_images == B) or amax[0] (1)'"), ("amax_images", 0, "amax_images is B or 1")]
add("segmif_sr_attention_split_f32", _ATS + _AT8 + [S], rows=_ATS_ROWS)
add("segmif_sr_attention_split16_f32", _ATS + [(n, N(2) if n == "B" else t) for n, t in _AT8] + [("amax", O()), ("amax_images", V(2)), S], rows=_ATS_ROWS + _ATS_AM)
add("segmif_sr_attention_split16_pairs_f32", _ATS + [(n, N(2) if n == "B" else t) for n, t in _AT8] + [("amax", O()), ("out_amax", O()), ("amax_images", V(2)), S],
    rows=_ATS_ROWS + _ATS_AM)
add("segmif_sr_attention_bwd_f32", [("q", P16()), ("k", P16()), ("v", P16()), ("out", P16()), ("dout", P16()), ("dq", P16()), ("dkv", P16()), ("workspace", P16()),
                                    ("B", N(1)), ("heads", N(2)), ("N", N(8)), ("Nk", N(4)), ("hd", V(64)), ("ldkv", LD(256, 256, True)), ("scale", V(0.125)), S],
    rows=[("hd", 32, "header: rows of heads * 64"), ("hd", 65, "header: rows of heads * 64")])

# ---------------------------------------------------------------------------------------------------------------- linattn.hip
add("segmif_linattn_partial_f32", [("kv", P16()), ("partial", P8()), ("B", N(1)), ("N", N(40)), ("heads", N(8)), ("d", N(8)), ("ldkv", LD(128, 128, True)), S],
    rows=[("d", 9, "header: 'd <= 8'"), ("heads", 9, "header: 'C = heads*d <= 64'")])
add("segmif_linattn_partial_f32", [("kv", P()), ("partial", P8()), ("B", N(1)), ("N", N(40)), ("heads", N(8)), ("d", N(4)), ("ldkv", LD(64, 64)), S], variant="generic",
    rows=[("kv", 0x10100002, "linattn.hip: the scalar-load kernel reads floats - a pointer that is not 4-byte aligned"), ("d", 9, "header: 'd <= 8'")])
add("segmif_linattn_kvpartial_f32", [("y", P16()), ("wkv", P16()), ("partial", P8()), ("B", N(1)), ("N", N(40)), ("heads", V(8)), ("d", V(8)), ("ldy", LD(64, 64, True)), S],
    rows=[("heads", 4, "linattn.hip: 'heads != 8 || d != 8' (the (128, 64) kv weight)"), ("d", 4, "linattn.hip: 'heads != 8 || d != 8'")])
add("segmif_linattn_fold_f32", [("partial", P8()), ("wend", P()), ("weff", P()), ("B", N(1)), ("nblk", N(1)), ("heads", N(8)), ("d", N(8)), ("Nout", N(64)),
                                ("ldw", V(128)), ("wofs", V(64)), ("ldweff", V(128)), ("kofs", V(64)), ("scale", V(0.125)), S],
    rows=[("d", 9, "header: 'd <= 8'"), ("heads", 9, "header: 'C = heads*d <= 64'"), ("ldw", 124, "Wend[n][wofs + h*d + j]: a pitch below wofs + C"),
          ("ldweff", 124, "Weff[b][n][kofs + h*d + i]: a pitch below kofs + C"), ("wofs", -1, "a negative column offset"), ("kofs", -1, "a negative column offset")])
add("segmif_linattn_fold_bwd_f32", [("ktv", P8()), ("wend", P()), ("ldw", V(128)), ("wofs", V(64)), ("dweff", P()), ("ldweff", V(128)), ("kofs", V(64)), ("scale", V(0.125)),
                                    ("dktv", P8()), ("dwend_part", P()), ("ldp", V(128)), ("B", N(1)), ("Nout", N(64)), ("heads", N(8)), ("d", N(8)), S],
    rows=[("d", 9, "header: 'd <= 8'"), ("d", 7, "header: 'C % 16 == 0'"), ("heads", 9, "header: 'C = heads * d <= 64'"), ("ldw", 124, "header: 'a pitch narrower than wofs + C'"),
          ("ldweff", 124, "header: 'a pitch narrower than ... kofs + C'"), ("ldp", 124, "header: dwend_part[b][n][wofs + c], pitch ldp"), ("wofs", -1, "a negative offset"),
          ("kofs", -1, "a negative offset")])

# -------------------------------------------------------------------------------------------------------------- crosspath.hip
add("segmif_crosspath_gram_f32", [("x", P16()), ("ldx", LD(64, 64, True)), ("w", P16()), ("bias", O()), ("partial", P8()), ("B", N(1)), ("N", N(40)), S])
add("segmif_crosspath_gram_lazy_f32", [("s_low", P()), ("lds", LD(64, 64)), ("ih", N(1)), ("iw", N(1)), ("H", N(1)), ("W", N(4)), ("partial", P8()), ("B", N(1)), S],
    rows=[("W", 6, "header: 'Needs W % 4 == 0'"), ("iw", 2, "header: 'an enlargement by three or more (3 iw <= W), else SEGMIF_EINVAL'"),
          ("s_low", 0x10100002, "crosspath.hip: '(uintptr_t)s_low & 3'")])
add("segmif_crosspath_gram_sum_f64", [("partial", P8()), ("nblk", N(3)), ("total", P8()), ("B", N(1)), S])
add("segmif_crosspath_fold_f32", [("partial", P8()), ("nblk", N(1)), ("wkv", P()), ("wend", P()), ("weff", P()), ("B", N(1)), ("Nout", N(64)), ("ldw", V(128)),
                                  ("wofs", V(64)), ("ldweff", V(128)), ("kofs", V(64)), ("scale", V(0.125)), ("cond", O()), S],
    rows=[("ldw", 124, "folded 'exactly like segmif_linattn_fold_f32': a pitch below wofs + 64"), ("ldweff", 124, "a pitch below kofs + 64"),
          ("wofs", -1, "a negative column offset"), ("kofs", -1, "a negative column offset")])
_CT = [("x3", P16()), ("xi", P16()), ("w3", P16()), ("b3", O()), ("wi", P16()), ("bi", O()), ("weff", P16()), ("bend", O()), ("ln_gamma", P()), ("ln_beta", P()),
       ("ln_eps", V(1e-5)), ("out", O16()), ("ld3", LD(64, 64, True)), ("ldi", LD(64, 64, True)), ("ldo", LD(64, 64, True)), ("B", N(2)), ("N", N(32)),
       ("planes_out", O()), ("H", V(4)), ("W", V(8)), ("planes_chunks", V(4)), ("planes_f16", V(1)), ("planes_amax", O()), ("planes_amax_images", V(2)),
       ("x3_ih", V(0)), ("x3_iw", V(0)), ("arith_f16", V(0)), ("arith_amax", Z()), ("arith_amax_images", V(0))]
add("segmif_crosspath_tail_f32", _CT, struct=L.SegmifCrossTail, tail=[S], rows=[
    ("H", 5, "header: 'planes ... H * W == N'"), ("H", 0, "header: 'H * W == N'"), ("planes_chunks", 3, "header: 'emits out as planes chunks 0..3'"),
    ("planes_amax_images", 3, "header: 'planes_amax_images == B: planes_amax[image]; <= 1: planes_amax[0]'"),
    ("arith_f16", 1, "header: arith_f16 is 'for the lazy (x3_ih > 0), planes-only (out == NULL), f16x3-planes launch'"),
    ("x3_iw", 2, "header: 'x3_ih > 0: x_3 is NOT a full-resolution tensor' - x3_iw without x3_ih")])
add("segmif_crosspath_tail_f32", [(n, {"w3": Z(), "b3": Z(), "out": Z(), "planes_out": P(), "x3_ih": V(1), "x3_iw": V(1), "arith_f16": V(1), "arith_amax": P(),
                                       "arith_amax_images": V(2)}.get(n, t)) for n, t in _CT], struct=L.SegmifCrossTail, tail=[S], variant="lazy_f16", rows=[
    ("x3_ih", 0, "header: a lazy source needs both x3_ih and x3_iw (and w3 otherwise)"), ("x3_iw", 0, "header: a lazy source needs both x3_ih and x3_iw"),
    ("planes_f16", 0, "header: arith_f16 needs the 'f16x3-planes launch'"), ("out", PR, "header: arith_f16 needs the 'planes-only (out == NULL)' launch"),
    ("arith_amax_images", 3, "header: 'arith_amax_images == B: one per image; <= 1: arith_amax[0]'"), ("W", 7, "header: 'H, W must be set (H * W == N)'")])

# ---------------------------------------------------------------------------------------------------------------- mixffn.hip
add("segmif_mixffn_pack", [("w1", P()), ("b1", P()), ("dw9", P()), ("dwb", P()), ("w2", P()), ("C", V(64)), ("out", P16()), S],
    rows=[("C", 32, "mixffn.hip: C is 64 or 128"), ("C", 0, "C is 64 or 128"), ("C", 192, "C is 64 or 128")])
add("segmif_mixffn_f16x3", [("x", P16()), ("out", P16()), ("wimg", P16()), ("ln_gamma", P()), ("ln_beta", P()), ("ln_eps", V(1e-5)), ("b2", P()), ("B", N(2)), ("H", N(4)),
                            ("W", N(4)), ("C", V(64)), ("amax_a", O()), ("amax_g", O()), ("amax_images", V(2))], struct=L.SegmifMixFfn, tail=[S],
    rows=[("C", 32, "mixffn.hip: C is 64 or 128"), ("C", 0, "C is 64 or 128"), ("C", 96, "C is 64 or 128"), ("amax_images", 3, "mixffn.hip: amax_images is 1 or B"),
          ("out", 0x10000000 + 0x100000, "mixffn.hip: 'd->x == d->out' - the kernel reads neighbours of what it writes")])

# ------------------------------------------------------------------------------------------------------------------ wgrad.hip
_WG_TAIL = [("dy", P()), ("ldy", LD(64, 64)), ("dy_zstride", V(0)), ("dw", P()), ("dw_sn", V(64)), ("dw_sk", V(1)), ("dbias", O()), ("dw_workspace", P()), ("accumulate", V(0)), S]
add("segmif_wgrad_f32", _igemm(in_=P16(), wt=Z(), out=Z(), bias=Z(), lda=LD(64, 64, True), ldo=V(0)), struct=L.SegmifIgemm, tail=_WG_TAIL, variant="dense", rows=[
    ("nz2", 2, "wgrad.hip: 'two batch levels: segmif_wgrad_batched2_f32'"), ("in2", PR, "header: desc describes the forward problem; two sources have no weight-gradient kernel"),
    ("K", 62, "wgrad.hip, dense: 'd->K % 4'"), ("in_zstride", 2, "wgrad.hip, dense: 'd->in_zstride % 4'")])
add("segmif_wgrad_f32", _igemm(in_=P(), wt=Z(), out=Z(), bias=Z(), split_f16=V(1), split_in_amax=P(), split_in_amax_n=V(2), wgrad_dy_amax=P(), wgrad_dy_amax_n=V(2),
                               **dict(_CONV3, ldo=V(0))), struct=L.SegmifIgemm,
    tail=[("dy", P()), ("ldy", LD(32, 32)), ("dy_zstride", V(0)), ("dw", P()), ("dw_sn", V(288)), ("dw_sk", V(1)), ("dbias", O()), ("dw_workspace", P()),
          ("accumulate", V(0)), S], variant="conv3x3_f16", rows=[
    ("split_in_amax_n", 0, "header: split_in_amax_n (1..64)"), ("split_in_amax_n", 65, "header: split_in_amax_n (1..64)"),
    ("wgrad_dy_amax_n", 0, "wgrad.hip: 'd->wgrad_dy_amax_n < 1 || d->wgrad_dy_amax_n > 64'"), ("wgrad_dy_amax_n", 65, "wgrad.hip: 'd->wgrad_dy_amax_n > 64'")])
add("segmif_wgrad_batched2_f32", _igemm(in_=P16(), wt=Z(), out=Z(), bias=Z(), lda=LD(64, 64, True), ldo=V(0), nz=V(2), nz2=V(2)), struct=L.SegmifIgemm,
    tail=[("dy", P()), ("ldy", LD(64, 64)), ("dy_zstride", V(0)), ("dy_zstride2", V(0)), ("dw", P()), ("dw_sn", V(64)), ("dw_sk", V(1)), ("dw_workspace", P()),
          ("accumulate", V(0)), S], rows=[
    ("nz", 0, "wgrad.hip: 'd->nz < 1 || d->nz2 < 1'"), ("nz2", 0, "wgrad.hip: 'd->nz < 1 || d->nz2 < 1'"), ("KH", 3, "header: 'for a dense problem batched over TWO levels'"),
    ("stride", 2, "header: 'for a dense problem batched over TWO levels'"), ("in_zstride2", 2, "wgrad.hip, dense: 'k.in_zs2 % 4'")])
add("segmif_colsum_f32", [("x", P()), ("out", P()), ("workspace", P8()), ("rows", N(4)), ("N", N(9)), ("ldx", LD(13, 9)), ("accumulate", V(0)), S])
add("segmif_act_bwd_f32", [("dy", P()), ("ref", P()), ("dx", P()), ("rows", N(4)), ("C", N(8)), ("ldy", LD(8, 8)), ("ldr", LD(8, 8)), ("ldx", LD(8, 8)), ("act", V(1)),
                           ("slope", Z()), S], rows=[("act", 2, "PReLU without a slope"), ("act", ACT_END, "one past the enum"), ("act", -1, "below the enum")])
add("segmif_act_bwd2_f32", [("dy", P()), ("ref", P()), ("ref2", P()), ("dx", P()), ("rows", N(4)), ("C", N(8)), ("ldy", LD(8, 8)), ("ldr", LD(8, 8)), ("ldr2", LD(8, 8)),
                            ("ldx", LD(8, 8)), ("act", V(1)), ("slope", Z()), S], rows=[("act", 2, "PReLU without a slope"), ("act", ACT_END, "one past the enum")])

# ---------------------------------------------------------------------------------------------------------------- backward.hip
add("segmif_col2im_f32", [("cols", P()), ("dx", P()), ("B", N(1)), ("H", N(8)), ("W", N(8)), ("C", N(8)), ("k", N(3)), ("stride", N(2)), ("pad", V(1)), ("OH", N(4)),
                          ("OW", N(4)), S], rows=[("pad", -1, "a negative padding")])
add("segmif_layernorm_bwd_f32", [("x", P16()), ("dy", P16()), ("gamma", P16()), ("dx", P16()), ("partial", P()), ("rows", N(4)), ("C", N(64)), ("ldx", LD(64, 64, True)),
                                 ("ldy", LD(64, 64, True)), ("lddx", LD(64, 64, True)), ("eps", V(1e-5)), S], rows=[("C", 66, "C % 4 == 0"), ("C", 1028, "C <= 1024")])
add("segmif_layernorm_bwd_add_f32", [("x", P16()), ("dy", P16()), ("gamma", P16()), ("dres", O16()), ("lddres", LD(64, 64, True)), ("scale", O()), ("rows_per_image", V(2)),
                                     ("dx", P16()), ("dbranch", O16()), ("lddbr", LD(64, 64, True)), ("partial", P()), ("rows", N(4)), ("C", N(64)),
                                     ("ldx", LD(64, 64, True)), ("ldy", LD(64, 64, True)), ("lddx", LD(64, 64, True)), ("eps", V(1e-5)), S],
    rows=[("C", 66, "C % 4 == 0"), ("rows_per_image", 0, "scale[row / rows_per_image]"), ("rows_per_image", 3, "whole images"),
          ("scale", None, "backward.hip: 'dbranch && (!scale ...' - the branch gradient is the scaled one")])
add("segmif_dwconv3x3_gelu_bwd_f32", [("h", P()), ("w9", P()), ("bias", P()), ("dy", P()), ("dz", P()), ("partial", P()), ("B", N(1)), ("H", N(4)), ("W", N(4)), ("C", N(128)), S],
    rows=[("C", 64, "backward.hip: 'C % 128'")])
add("segmif_dwconv3x3_bias_bwd_f32", [("h", P()), ("w9", P()), ("dy", P()), ("partial", P()), ("B", N(1)), ("H", N(4)), ("W", N(4)), ("C", N(128)), S],
    rows=[("C", 64, "backward.hip: 'C % 128'")])
add("segmif_dwconv3x3_plain_f32", [("x", P16()), ("w9", P16()), ("y", P16()), ("B", N(1)), ("H", N(4)), ("W", N(4)), ("C", N(8)), S], rows=[("C", 6, "C % 4 == 0")])
add("segmif_bilinear_nhwc_bwd_f32", [("dy", P()), ("dx", P()), ("B", N(1)), ("IH", N(2)), ("IW", N(2)), ("OH", N(4)), ("OW", N(4)), ("C", N(9)), ("lddy", LD(13, 9)),
                                     ("lddx", LD(13, 9)), S])
add("segmif_row_softmax_f32", [("s", P()), ("rows", N(4)), ("L", N(9)), ("ld", LD(13, 9)), ("scale", V(1.0)), S], rows=[("ld", 1028, "backward.hip: 'ld > 1024'")])
add("segmif_row_softmax_bwd_f32", [("p", P()), ("dp", P()), ("rows", N(4)), ("L", N(9)), ("ld", LD(13, 9)), ("scale", V(1.0)), S], rows=[("ld", 1028, "backward.hip: 'ld > 1024'")])
add("segmif_softmax_ce_f32", [("logits", P()), ("labels", P()), ("dlogits", O()), ("partial", P()), ("rows", N(4)), ("C", N(9)), ("ld", LD(13, 9)), ("ldd", LD(13, 9)),
                              ("ignore_index", V(255)), S], rows=[("C", 33, "backward.hip: 'C > 32'")])
add("segmif_conv_dgrad_strided_dil_f32", [("dy", P()), ("wd", P()), ("dx", P()), ("B", N(1)), ("H", N(8)), ("W", N(8)), ("Cin", N(8)), ("N", N(8)), ("KH", N(3)), ("KW", N(3)),
                                          ("stride", N(2)), ("pad", V(1)), ("dil", N(1)), ("OH", N(4)), ("OW", N(4)), ("lddy", LD(12, 8)), ("lddx", LD(12, 8)), S],
    rows=[("pad", -1, "a negative padding")])
add("segmif_adamw_f32", [("table", P()), ("chunk_entry", P()), ("chunk_off", P()), ("nchunks", N(2)), ("chunk_elems", N(1024)), ("beta1", V(0.9)), ("beta2", V(0.999)),
                         ("eps", V(1e-8)), ("bc1", V(0.1)), ("bc2s", V(0.03)), S],
    rows=[("bc1", 0.0, "backward.hip: '!(bc1 > 0.f)' - a bias correction of 0 divides by zero"), ("bc2s", 0.0, "backward.hip: '!(bc2s > 0.f)'"),
          ("bc1", float("nan"), "backward.hip: '!(bc1 > 0.f)' refuses NaN")])
add("segmif_bn_colstats_f32", [("x", P()), ("dz", P()), ("mu", P()), ("rstd", P()), ("partial", P()), ("out", P()), ("rows", N(4)), ("C", N(8)), ("mode", V(1)), S])
add("segmif_bn_apply_f32", [("x", P()), ("scale", P()), ("shift", P()), ("y", P()), ("rows", N(4)), ("C", N(8)), ("relu", V(1)), S], rows=[("C", 6, "backward.hip: 'C & 3'")])
add("segmif_bn_bwd_apply_f32", [("x", P()), ("dz", P()), ("mu", P()), ("rstd", P()), ("scale", P()), ("a", P()), ("b", P()), ("dx", P()), ("rows", N(4)), ("C", N(8)), S],
    rows=[("C", 6, "backward.hip: 'C & 3'")])

# ------------------------------------------------------------------------------------------------------------------ losses.hip
add("segmif_ssim_prep_f32", [("gen", P()), ("mask", P()), ("stack5", P()), ("n", N(16)), S])
add("segmif_ssim_map_f32", [("blurred5", P()), ("gen", P()), ("mask", P()), ("der3", O()), ("partial", P()), ("sums2", P()), ("n", N(16)), S])
add("segmif_ssim_grad_f32", [("blurred_der3", P()), ("gen", P()), ("mask", P()), ("grad", P()), ("n", N(16)), ("upstream", P()), ("coef_ssim", V(1.0)), ("coef_mse", V(1.0)), S])
add("segmif_sobel_l1_f32", [("gen", P()), ("mask", P()), ("pxy2", O()), ("partial", P()), ("sums2", P()), ("planes", N(1)), ("H", N(4)), ("W", N(4)), S])
add("segmif_sobel_l1_bwd_f32", [("pxy2", P()), ("gen", P()), ("mask", P()), ("grad", P()), ("planes", N(1)), ("H", N(4)), ("W", N(4)), ("upstream", P()), S])
add("segmif_laploss2_f32", [("gen", P()), ("ir", P()), ("vis", P()), ("sign3", O()), ("partial", P()), ("sums2", P()), ("planes", N(1)), ("H", N(4)), ("W", N(4)), S])
add("segmif_laploss2_bwd_f32", [("sign3", P()), ("grad", P()), ("planes", N(1)), ("H", N(4)), ("W", N(4)), ("upstream", P()), S])
add("segmif_prelu_f32", [("z", P()), ("slope", P()), ("y", P()), ("n", N(16)), S])
add("segmif_prelu_bwd_f32", [("dy", P()), ("z", P()), ("slope", P()), ("dz", P()), ("partial", P()), ("dslope", P()), ("n", N(16)), S])
add("segmif_prelu_bwd_rows_f32", [("dy", P()), ("lddy", LD(8, 8)), ("z", P()), ("slope", P()), ("dz", P()), ("partial", P()), ("dslope", P()), ("rows", N(4)), ("C", N(8)), S])

# ------------------------------------------- entry points outside the core files that no other test WITHOUT a GPU sends a rejected call
add("segmif_device_name", [("buf", P()), ("len", N(64))])
add("segmif_conv3x3_split_pack", [("packed", P()), ("N", N(32)), ("Cin", N(64)), ("ldw", LD(576, 576)), ("out", P()), S], rows=[("Cin", 24, "header: 'Cin % 16 == 0'")])
add("segmif_confusion_i32", [("pred", P()), ("label", P()), ("conf", P()), ("n", V(16)), ("K", N(9)), S], rows=[("n", -1, "a negative count"), ("K", 33, "header: 'K <= 32'")])
add("segmif_quantize_u8", [("x", P()), ("out", P()), ("minmax", P()), ("B", N(1)), ("C", N(3)), ("HW", N(16)), S])
add("segmif_dequantize_u8", [("in_", P()), ("out", P()), ("B", N(1)), ("C", N(3)), ("HW", N(16)), S])
add("segmif_boundary_stats_i32", [("pred", P()), ("label", P8()), ("B", N(1)), ("H", N(8)), ("W", N(8)), ("K", N(9)), ("d", N(2)), ("theta", V(1)), ("cls", P8()),
                                  ("trimap", P8()), S], rows=[("K", 33, "header: 'K in 1..32 classes'"), ("d", 33, "header: 'd in 1..32'"), ("theta", -1, "header: 'theta in 0..31'"),
                                                              ("theta", 32, "header: 'theta in 0..31'")])
add("segmif_augment_pick_u8", [("label", P()), ("N", N(2)), ("h", N(16)), ("w", N(16)), ("rec", P()), ("tab", P()), ("tab_words", N(64)), ("B", N(2)), ("crop_h", N(8)),
                               ("crop_w", N(8)), S])
add("segmif_augment_apply_u8", [("ir", P()), ("vis", P()), ("mask", P()), ("label", P()), ("N", N(2)), ("h", N(16)), ("w", N(16)), ("rec", P()), ("tab", P()),
                                ("tab_words", N(64)), ("B", N(2)), ("crop_h", N(8)), ("crop_w", N(8)), ("ir3", P16()), ("vis3", P16()), ("mask3", P16()),
                                ("label_out", P16()), S], rows=[("crop_w", 6, "header: 'crop_w % 4 == 0'")])
_SO = [("gamma", V(0.0)), ("label_smoothing", V(0.0)), ("ohem_t", V(0.7)), ("reduction", V(0)), ("ignore_index", V(255)), ("reserved", V(0)), ("ohem_n_min", V(0))]
_SO_ROWS = [("gamma", -1.0, "header: the focal exponent is >= 0 and finite"), ("gamma", float("inf"), "header: the focal exponent is finite"),
            ("label_smoothing", 1.0, "header: label smoothing in [0, 1)"), ("reduction", 3, "one past SEGMIF_SEG_OHEM"), ("reduction", -1, "below the enum"),
            ("C", 33, "seg_objective.hip: 'C > 32'"), ("rows_per_sample", 0, "sample_weight[row / rows_per_sample]"), ("rows_per_sample", 3, "whole samples")]
add("segmif_seg_objective_weighted_f32", _SO, struct=L.SegmifSegObjective, rows=_SO_ROWS,
    tail=[("logits", P()), ("labels", P()), ("class_weight", O()), ("pixel_weight", O()), ("sample_weight", O()), ("rows_per_sample", V(2)), ("workspace", P()), ("record4", P()),
          ("rows", N(4)), ("C", N(9)), ("ld", LD(13, 9)), S])
add("segmif_seg_objective_weighted_bwd_f32", _SO, struct=L.SegmifSegObjective, rows=_SO_ROWS,
    tail=[("logits", P()), ("labels", P()), ("class_weight", O()), ("pixel_weight", O()), ("sample_weight", O()), ("rows_per_sample", V(2)), ("workspace", O()), ("record4", P()),
          ("upstream", P()), ("dlogits", P()), ("rows", N(4)), ("C", N(9)), ("ld", LD(13, 9)), ("ldd", LD(13, 9)), S])
add("segmif_pseudo_label_f32", [("x", P()), ("labels", P()), ("conf", Z()), ("count", P()), ("B", N(1)), ("IH", N(2)), ("IW", N(2)), ("OH", N(4)), ("OW", N(4)), ("C", N(9)),
                                ("ldx", LD(13, 9)), ("tau", V(0.5)), ("below_ignore", V(0)), ("ignore_index", V(255)), S],
    rows=[("C", 33, "pseudo_label.hip: 'C > 32'"), ("tau", 1.5, "pseudo_label.hip: tau in [0, 1]"), ("tau", -0.25, "pseudo_label.hip: tau in [0, 1]"),
          ("tau", float("nan"), "pseudo_label.hip: 'NaN fails both comparisons'"), ("B", 65536, "grid dimensions"), ("OH", 65536, "grid dimensions")])
add("segmif_comm_unique_id", [("id", P()), ("bytes", V(128))], rows=[("bytes", 64, "comm.hip: 'bytes < sizeof(ncclUniqueId)'")])
add("segmif_comm_init", [("comm", P()), ("world", N(2)), ("rank", V(0)), ("id", P()), ("bytes", V(128))],
    rows=[("rank", -1, "comm.hip: 'rank < 0 || rank >= world'"), ("rank", 2, "comm.hip: 'rank >= world'"), ("bytes", 64, "comm.hip: 'bytes < sizeof(ncclUniqueId)'")])
add("segmif_comm_world", [("comm", P()), ("world", P()), ("rank", P())])
add("segmif_comm_allreduce_f32", [("comm", P()), ("send", P()), ("recv", P()), ("count", N(16)), ("average", V(0)), S])
add("segmif_comm_destroy", [("comm", P())])

# ------------------------------------------------------------------------------ distill_objective.hip (include/segmif_distill.h)
_DS = [("temperature", V(2.0)), ("mode", V(1)), ("reserved", A((), (0, 0)))]
_DS_T = "segmif_distill.h: 'T not finite or <= 0'"
_DS_ROWS = [("temperature", 0.0, _DS_T), ("temperature", -1.0, _DS_T), ("temperature", float("inf"), _DS_T), ("temperature", float("nan"), _DS_T),
            ("mode", 2, "segmif_distill.h: 'an unknown mode'"), ("mode", -1, "segmif_distill.h: 'an unknown mode'"),
            ("C", 33, "segmif_distill.h: 'C outside 1..32'"), ("lds", 8, "segmif_distill.h: 'lds, ldt (backward: ldd) below C'"),
            ("ldt", 8, "segmif_distill.h: 'lds, ldt (backward: ldd) below C'"), ("rows", -512, "segmif_distill.h: 'rows < 1'"),
            ("rows_per_sample", -256, "segmif_distill.h: 'rows_per_sample < 1'"), ("rows_per_sample", 255, "segmif_distill.h: 'rows % rows_per_sample != 0'"),
            ("rows", 65536 * 256, "segmif_distill.h: 'in channel mode B = rows / rows_per_sample > 65535 (the grid's second dimension)'")]
_DS_DIMS = [("rows", N(512)), ("rows_per_sample", N(256)), ("C", N(9)), ("lds", LD(9, 9)), ("ldt", LD(9, 9))]
add("segmif_distill_objective_f32", _DS, struct=L.SegmifDistill, rows=_DS_ROWS,
    tail=[("student", P()), ("teacher", P()), ("workspace", P()), ("record4", P())] + _DS_DIMS + [S])
add("segmif_distill_objective_bwd_f32", _DS, struct=L.SegmifDistill, rows=_DS_ROWS + [("ldd", 8, "segmif_distill.h: 'lds, ldt (backward: ldd) below C'")],
    tail=[("student", P()), ("teacher", P()), ("workspace", P()), ("record4", P()), ("upstream", P()), ("dstudent", P())] + _DS_DIMS + [("ldd", LD(9, 9)), S])

# ------------------------------------------------------------------------------- calibration_stats.hip (include/segmif_calib.h)
_CB_T, _CB_E = "segmif_calib.h: 'a temperature that is not finite or <= 0'", "segmif_calib.h: 'edges that are not strictly ascending or not inside the open interval (0, 1) (NaN included)'"
_CB_K, _CB_G = "segmif_calib.h: 'a threshold outside [0, 1] (NaN included)'", "segmif_calib.h: 'B or OH above SEGMIF_CALIB_MAX_GRID (the grid's dimensions)'"
_CB_X = "segmif_calib.h: 'B, IH, IW, OH or OW below 1'"
add("segmif_calibration_stats_f32", struct=L.SegmifCalib, args=[
    ("n_temperatures", N(2)), ("n_edges", V(3)), ("n_thresholds", V(2)), ("reserved0", V(0)),
    ("temperatures", A((1.0, 2.0), [1.0 + i for i in range(16)])), ("edges", A((0.25, 0.5, 0.75), [(i + 1) / 64.0 for i in range(32)])),
    ("thresholds", A((0.9, 0.968), [0.5] * 8)), ("reserved", A((), [0] * 4))],
    tail=[("x", P()), ("label", P()), ("counts", P()), ("above", P()), ("totals", P()), ("sums", P()), ("workspace", P()), ("conf", O()), ("pred", O()),
          ("B", N(2)), ("IH", N(3)), ("IW", N(5)), ("OH", N(11)), ("OW", N(19)), ("C", N(9)), ("ldx", LD(9, 9)), S], rows=[
    ("C", 33, "segmif_calib.h: 'C outside 1..32'"), ("ldx", 8, "segmif_calib.h: 'ldx < C'"),
    ("n_temperatures", 17, "segmif_calib.h: 'NT outside 1..16'"), ("n_edges", -1, "segmif_calib.h: 'NE outside 0..31'"),
    ("n_edges", 32, "segmif_calib.h: 'NE outside 0..31'"), ("n_thresholds", -1, "segmif_calib.h: 'NK outside 0..8'"),
    ("n_thresholds", 9, "segmif_calib.h: 'NK outside 0..8'"),
    ("temperatures", (1.0, 0.0), _CB_T), ("temperatures", (-1.0, 2.0), _CB_T), ("temperatures", (float("inf"), 2.0), _CB_T),
    ("temperatures", (1.0, float("nan")), _CB_T),
    ("edges", (0.25, 0.25, 0.75), _CB_E), ("edges", (0.5, 0.25, 0.75), _CB_E), ("edges", (0.0, 0.5, 0.75), _CB_E), ("edges", (0.25, 0.5, 1.0), _CB_E),
    ("edges", (-0.5, 0.5, 0.75), _CB_E), ("edges", (0.25, float("nan"), 0.75), _CB_E),
    ("thresholds", (0.9, 1.5), _CB_K), ("thresholds", (-0.1, 0.968), _CB_K), ("thresholds", (float("nan"), 0.968), _CB_K),
    ("B", -2, _CB_X), ("OW", -19, _CB_X), ("B", 65536, _CB_G), ("OH", 65536, _CB_G)])  # above = NULL: 'a NULL above with NK > 0' (NK = 2)

# --------------------------------------------------------------------------------------- objects.hip (include/segmif_objects.h)
_OB_C, _OB_E = "segmif_objects.h: 'connectivity other than 4 or 8'", "segmif_objects.h: 'edges not strictly ascending or below 1'"
_HW = [(65536, 32768), (46341, 46341), (2, 2 ** 30)]  # H * W >= 2^31
add("segmif_object_stats_i32", struct=L.SegmifObjects, args=[
    ("connectivity", V(8)), ("n_edges", V(2)), ("edges", A((1024, 9216), [10 ** (5 + i) for i in range(4)])), ("reserved", A((), [0] * 4))],
    tail=[("pred", P()), ("label", P()), ("obj", P()), ("mass", P()), ("status", P()), ("workspace", P()), ("root_g", O()), ("root_p", O()),
          ("B", N(2)), ("H", N(37)), ("W", N(53)), ("K", N(9)), S], rows=[
    ("K", 33, "segmif_objects.h: 'K outside 1..32'"), ("connectivity", 0, _OB_C), ("connectivity", 6, _OB_C), ("connectivity", -8, _OB_C),
    ("connectivity", 16, _OB_C), ("n_edges", -1, "segmif_objects.h: 'n_edges outside 0..3'"), ("n_edges", 4, "segmif_objects.h: 'n_edges outside 0..3'"),
    ("edges", (1024, 1024), _OB_E), ("edges", (9216, 1024), _OB_E), ("edges", (0, 9216), _OB_E), ("edges", (-5, 9216), _OB_E),
    ("B", -2, "segmif_objects.h: 'B, H or W below 1'"), ("H", -37, "segmif_objects.h: 'B, H or W below 1'"), ("W", -53, "segmif_objects.h: 'B, H or W below 1'"),
    ("B", 32768, "segmif_objects.h: 'B above SEGMIF_OBJECTS_MAX_FRAMES: the grid's z holds 2 B'")]
    + [(("H", "W"), hw, "segmif_objects.h: 'H * W >= 2^31'") for hw in _HW])

# ------------------------------------------------------------------------------------- copy_paste.hip (include/segmif_paste.h)
_PA_N, _PA_HW = "segmif_paste.h, boxes: 'n above SEGMIF_PASTE_MAX_FRAMES' (pack: 'n, H, W as above')", "segmif_paste.h, boxes: 'H * W >= 2^31' (pack: 'n, H, W as above')"
add("segmif_object_boxes_i32", [("root", P()), ("label", P()), ("n", N(2)), ("H", N(37)), ("W", N(53)), ("K", N(9)), ("class_mask", V(0x1fe)), ("min_area", V(64)),
                                ("max_box", V(500)), ("frame0", V(0)), ("records", P16()), ("capacity", V(16)), ("counter", P()), ("workspace", P()), S], rows=[
    ("K", 33, "segmif_paste.h, boxes: 'K outside 1..32'"), ("min_area", 0, "segmif_paste.h, boxes: 'min_area or max_box below 1'"),
    ("min_area", -3, "segmif_paste.h, boxes: 'min_area or max_box below 1'"), ("max_box", 0, "segmif_paste.h, boxes: 'min_area or max_box below 1'"),
    ("capacity", -1, "segmif_paste.h, boxes: 'capacity or frame0 below 0'"), ("frame0", -1, "segmif_paste.h, boxes: 'capacity or frame0 below 0'"),
    ("frame0", 2 ** 31 - 2, "segmif_paste.h, boxes: 'frame0 + n > 2^31 - 1'"), ("n", -2, "segmif_paste.h, boxes: 'n, H or W below 1'"), ("n", 32768, _PA_N),
    ("W", -53, "segmif_paste.h, boxes: 'n, H or W below 1'")] + [(("H", "W"), hw, _PA_HW) for hw in _HW[:2]])  # records = NULL: 'NULL records with capacity > 0'
add("segmif_object_pack_u8", [("records", P()), ("offsets", P8()), ("M", N(3)), ("store_pixels", V(100)), ("root", P()), ("ir", P()), ("vis", P()), ("mask", P()),
                              ("frame0", V(0)), ("n", N(2)), ("H", N(37)), ("W", N(53)), ("patches", P8()), S], rows=[
    ("store_pixels", -1, "segmif_paste.h, pack: 'store_pixels below 0'"), ("frame0", -1, "segmif_paste.h, pack: 'frame0 below 0'"), ("n", 32768, _PA_N),
    (("H", "W"), _HW[0], _PA_HW)])
_P16 = "segmif_paste.h, paste: 'one of the eight tensors not 16-byte aligned'"
add("segmif_copy_paste_f32", [("ir3", P16()), ("vis3", P16()), ("mask3", P16()), ("label", P16()), ("B", N(2)), ("h", N(8)), ("w", N(12)), ("records", P()), ("offsets", P8()),
                              ("patches", P8()), ("M", N(3)), ("store_pixels", N(100)), ("table", P()), ("P", V(3)), ("n_class", N(9)), ("ir3_out", P16()),
                              ("vis3_out", P16()), ("mask3_out", P16()), ("label_out", P16()), ("pasted", P8()), ("tally", O8()), S], rows=[
    ("P", 9, "segmif_paste.h, paste: 'P outside 0..8'"), ("P", -1, "segmif_paste.h, paste: 'P outside 0..8'"), ("w", 10, "segmif_paste.h, paste: 'w % 4'"),
    ("w", 13, "segmif_paste.h, paste: 'w % 4'"), ("B", 65536, "segmif_paste.h, paste: 'B outside 1..65535'"),
    ("n_class", 256, "segmif_paste.h, paste: 'n_class outside 1..255'"),
    ("label_out", 0x10000000 + 0x100000 * 19 + 8, _P16 + " (label_out + 8)")])  # table = NULL: 'NULL table with P > 0' (P = 3)

ENTRIES = E

_SIZE = "size query / no pointers"
EXEMPT = {
    "segmif_abi_version": _SIZE, "segmif_igemm_num_tiles": _SIZE, "segmif_igemm_tile_name": _SIZE, "segmif_conv3x3_split_weight_bytes": _SIZE,
    "segmif_conv3x3_split16_weight_bytes": _SIZE, "segmif_gemm_split_weight_bytes": _SIZE, "segmif_gemm_split16_weight_bytes": _SIZE,
    "segmif_planes_bytes": _SIZE, "segmif_planes_weight_bytes": _SIZE, "segmif_planes16_bytes": _SIZE, "segmif_planes16_weight_bytes": _SIZE,
    "segmif_gemm_pairs_weight_bytes": _SIZE, "segmif_sr_attention_bwd_chunks": _SIZE, "segmif_sr_attention_bwd_workspace_floats": _SIZE,
    "segmif_crosspath_gram_blocks": _SIZE, "segmif_mixffn_weight_bytes": _SIZE, "segmif_wgrad_workspace_size": _SIZE, "segmif_colsum_blocks": _SIZE,
    "segmif_prelu_bwd_blocks": _SIZE, "segmif_sr_attention_split_workspace": _SIZE, "segmif_linattn_num_blocks": _SIZE, "segmif_layernorm_bwd_blocks": _SIZE,
    "segmif_dwconv_bwd_partial_rows": _SIZE, "segmif_softmax_ce_blocks": _SIZE, "segmif_loss_blocks": _SIZE, "segmif_adamw_entry_bytes": _SIZE,
    "segmif_augment_record_bytes": _SIZE, "segmif_fusion_stats_workspace_bytes": _SIZE, "segmif_structural_stats_workspace_bytes": _SIZE,
    "segmif_fusion_objective_blocks": _SIZE, "segmif_seg_objective_workspace_bytes": _SIZE, "segmif_region_objective_workspace_bytes": _SIZE,
    "segmif_grad_guard_record_bytes": _SIZE, "segmif_grad_entry_stat_bytes": _SIZE, "segmif_grad_param_count_bytes": _SIZE,
    "segmif_grad_norm_workspace_bytes": _SIZE, "segmif_strong_augment_blocks": _SIZE, "segmif_distill_workspace_bytes": _SIZE,
    "segmif_calibration_workspace_bytes": _SIZE, "segmif_object_workspace_bytes": _SIZE, "segmif_object_boxes_workspace_bytes": _SIZE,
    "segmif_igemm_workspace_floats": "size query / no pointers of its own: it resolves the descriptor with segmif_igemm_f32's checks and returns 0 for a refused one",
    "segmif_comm_available": "size query / no pointers (an optional version word); -38 without RCCL",
    "segmif_conv3x3_split16_pack": "rejections covered by tests/test_abi_and_host.py::test_round4_training_entry_points_size_rules_and_rejections_without_a_gpu",
    "segmif_amax_f32": "rejections covered by tests/test_abi_and_host.py::test_round4_training_entry_points_size_rules_and_rejections_without_a_gpu",
    "segmif_fusion_stats_u8": "rejections covered by tests/test_fusion_metrics_host.py", "segmif_palette_u8": "rejections covered by tests/test_fusion_metrics_host.py",
    "segmif_structural_stats_u8": "rejections covered by tests/test_structural_scores_host.py",
    "segmif_augment_pick_class_u8": "rejections covered by tests/test_class_balance_host.py", "segmif_label_stats_u8": "rejections covered by tests/test_class_balance_host.py",
    "segmif_label_stats_i64": "rejections covered by tests/test_class_balance_host.py",
    "segmif_class_mix_select": "rejections covered by tests/test_class_mix_host.py", "segmif_class_mix_apply_f32": "rejections covered by tests/test_class_mix_host.py",
    "segmif_fusion_objective_f32": "rejections covered by tests/test_fusion_objectives_host.py",
    "segmif_fusion_objective_bwd_f32": "rejections covered by tests/test_fusion_objectives_host.py",
    "segmif_seg_objective_f32": "rejections covered by tests/test_seg_objectives_host.py", "segmif_seg_objective_bwd_f32": "rejections covered by tests/test_seg_objectives_host.py",
    "segmif_region_objective_f32": "rejections covered by tests/test_region_objectives_host.py",
    "segmif_region_objective_bwd_f32": "rejections covered by tests/test_region_objectives_host.py",
    "segmif_grad_norm_f32": "rejections covered by tests/test_grad_guard_host.py", "segmif_adamw_guarded_f32": "rejections covered by tests/test_grad_guard_host.py",
    "segmif_grad_scale_f32": "rejections covered by tests/test_grad_guard_host.py", "segmif_weight_ema_f32": "rejections covered by tests/test_weight_ema_host.py",
    "segmif_strong_augment_f32": "rejections covered by tests/test_strong_augment_host.py",
    "segmif_tta_vote_f32": "rejections covered by tests/test_tta_host.py", "segmif_resize_flip_nchw_f32": "rejections covered by tests/test_tta_host.py",
}


def find(name, arg, value):
    """the index of the row that sends `value` for `arg` to the entry point `name`: how the host test of a header holds the table to
    the cases its header lists.  A misaligned pointer stands for its misalignment, the fake base addresses being the table's own."""
    for i, e, _, a, v, _ in all_rows():
        if e.name == name and a == arg:
            tag = dict(e.args + e.tail).get(a, {}) if isinstance(a, str) else {}
            if tag.get("kind") == "ptr" and isinstance(v, int) and isinstance(value, int):
                same = v % 16 == value % 16
            else:
                same = repr(v) == repr(value)  # (repr: NaN inside a tuple, 0 and 0.0 apart)
            if same:
                return i
    raise KeyError(f"tests/_abi_contract_table.py has no row {name}: {arg} = {value!r}")


@functools.lru_cache(maxsize=None)
def all_rows():
    """[(index, entry, label, arg, value, reason)] in a fixed order: what the child sends and the tests are parametrized over"""
    out = []
    for e in ENTRIES:
        for label, arg, value, reason in e.mutations():
            out.append((len(out), e, label, arg, value, reason))
    return out
