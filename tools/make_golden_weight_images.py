"""Records tests/golden/weight_images.npz: the CRC32 of every 1 KiB block of each weight image that the split-operand kernels read
(conv3x3_split / split16, planes / planes16, gemm_split / split16, gemm_pairs, mixffn), as the library's *_pack entry points write
them on the MI355X.  Generator only; the cases, the weights and the reduction live in tests/_weight_images.py and are what
tests/test_gpu_weight_images.py repeats.  It goes through the C entry points alone, so it runs unchanged on any commit with ABI 4.

Record with the library of the commit BEFORE a change to the packers, never with the code under test.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "weight_images.npz"))
    args = ap.parse_args()
    import _weight_images as wi
    from segmif_amd import _lib
    lib = _lib.load()
    rec = {}
    for name, stem, dims in wi.CASES:
        image, guard = wi.pack_image(lib, stem, dims)
        assert (guard == wi.FILL).all(), f"{name}: the packer wrote past its image"
        rec[name] = wi.crc_blocks(image)
        untouched = int((image == wi.FILL).sum())
        print(f"{name}: {image.size} bytes, {rec[name].size} blocks, {untouched} bytes equal to the fill")
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
