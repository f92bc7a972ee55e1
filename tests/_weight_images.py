"""The cases of tests/golden/weight_images.npz, shared by the recorder (tools/make_golden_weight_images.py) and the test
(tests/test_gpu_weight_images.py): both build the same fp32 weights on the host, call the same C entry points and reduce the image
to the CRC32 of its 1 KiB blocks.

A weight is exact by construction and independent of any RNG version: element (n, k) is +-m 2^-24 2^(n % 7 - 3) with the 24-bit
mantissa m in [2^23, 2^24) and the sign taken from a 64-bit integer hash of (n, k).  Five rows are overridden:
    row 0  all zero                                   (scale 1)
    row 1  every magnitude in [2^-105, 2^-104) < 1e-30  (the "vanishing" branch of the row scale)
    row 2  magnitudes in [1/2, 1) and one element exactly 1.0: the maximum sits on an exponent boundary
    row 3  one +inf                                   (the non-finite branch)
    row 4  magnitudes in [2^20, 2^21)
No NaN goes in.  The source's row pitch is K + PITCH_EXTRA and the columns past K hold 2^100, which a packer must never read.
The destination is weight_bytes + GUARD bytes of 0xA5: bytes a packer does not write stay 0xA5 in the record as well, so the set
of written bytes is pinned along with their values.
"""
import zlib

import numpy as np

BLOCK, GUARD, FILL, PITCH_EXTRA = 1024, 64, 0xA5, 8

# (case name, entry-point stem, dimensions): the smallest shapes at which every index of the layout takes two values and padding exists
CASES = (
    ("conv3x3_split_n24_c32", "conv3x3_split", (24, 32)),      # 32-wide tile, 8 padded rows, two chunks
    ("conv3x3_split_n72_c16", "conv3x3_split", (72, 16)),      # 64-wide tiles, two of them, 56 padded rows
    ("conv3x3_split16_n24_c32", "conv3x3_split16", (24, 32)),
    ("conv3x3_split16_n72_c16", "conv3x3_split16", (72, 16)),
    ("planes_n32_c32_t9", "planes", (32, 32, 9)),
    ("planes_n64_c16_t1", "planes", (64, 16, 1)),              # both values of the half swap (n >> 4) & 1
    ("planes16_n32_c32_t9", "planes16", (32, 32, 9)),
    ("planes16_n64_c16_t1", "planes16", (64, 16, 1)),
    ("gemm_split_n132_k64", "gemm_split", (132, 64)),          # two column tiles, two K steps, 124 padded rows
    ("gemm_split16_n132_k64", "gemm_split16", (132, 64)),
    ("gemm_pairs_n132_k32", "gemm_pairs", (132, 32)),          # two column tiles, two K steps, all four swizzle phases
    ("mixffn_c64", "mixffn", (64,)),                           # the only two instantiations
    ("mixffn_c128", "mixffn", (128,)),
)


def _hash(n, k, salt):
    """splitmix64's finaliser over a linear mix of (n, k, salt); uint64 arithmetic wraps"""
    x = n.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + k.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(salt)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def weight(N, K, ldw=None, salt=0):
    """(N, ldw) float32, ldw >= K; see the module docstring"""
    ldw = K if ldw is None else ldw
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    h = _hash(n, k, salt)
    mant = ((h >> np.uint64(40)) | np.uint64(1 << 23)).astype(np.int64)           # 24 bits, the top one set
    mant = np.where((h >> np.uint64(39)) & np.uint64(1), -mant, mant)
    expo = n % 7 - 3
    if N > 4:
        expo[1], expo[2], expo[4] = -104, 0, 21
    w = np.full((N, ldw), np.float32(2.0 ** 100), dtype=np.float32)
    w[:, :K] = np.ldexp(mant.astype(np.float32), expo - 24)                        # exact: a 24-bit integer times a power of two
    if N > 4:
        w[0, :K] = 0.0
        w[2, K // 2] = 1.0
        w[3, 1] = np.inf
    assert not np.isnan(w).any()
    return w


def crc_blocks(image):
    """uint32 CRC32 of every 1 KiB block of a uint8 array (the last block may be short)"""
    raw = image.tobytes()
    return np.array([zlib.crc32(raw[o:o + BLOCK]) for o in range(0, len(raw), BLOCK)], dtype=np.uint32)


def pack_image(lib, stem, dims):
    """Runs one case on the current device -> (image bytes, guard bytes) as uint8 arrays."""
    import torch
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nbytes = int(getattr(lib, f"segmif_{stem}_weight_bytes")(*dims))
    assert nbytes > 0, (stem, dims)
    out = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert out.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    if stem == "mixffn":
        (C,) = dims
        w1, w2 = up(weight(4 * C, C, salt=1)), up(weight(C, 4 * C, salt=2))
        b1, dwb = up(weight(1, 4 * C, salt=3)[0]), up(weight(1, 4 * C, salt=4)[0])
        dw9 = up(weight(9, 4 * C, salt=5))
        code = lib.segmif_mixffn_pack(w1.data_ptr(), b1.data_ptr(), dw9.data_ptr(), dwb.data_ptr(), w2.data_ptr(), C, out.data_ptr(),
                                      stream)
    elif stem in ("planes", "planes16"):
        N, cin, taps = dims
        w = up(weight(N, taps * cin, taps * cin + PITCH_EXTRA))
        code = getattr(lib, f"segmif_{stem}_pack_weight")(w.data_ptr(), N, cin, taps, w.shape[1], out.data_ptr(), stream)
    else:
        N, kdim = dims
        K = 9 * kdim if stem.startswith("conv3x3") else kdim
        w = up(weight(N, K, K + PITCH_EXTRA))
        code = getattr(lib, f"segmif_{stem}_pack")(w.data_ptr(), N, kdim, w.shape[1], out.data_ptr(), stream)
    assert code == 0, f"{stem}{dims}: the pack entry point returned {code}"
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    return host[:nbytes], host[nbytes:]
