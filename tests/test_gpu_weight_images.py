"""The weight images of the split-operand kernels, byte for byte.  Every *_pack entry point of the library writes an image that a main
kernel streams: the tiles of a bf16x6 triple or an f16x3 scaled triple or pair plus the row scales.  tests/golden/weight_images.npz
holds the CRC32 of every 1 KiB block of each image as recorded on the MI355X (tools/make_golden_weight_images.py) before the
packers were folded into csrc/weight_pack.h; every block of every image must match, the 64 guard bytes behind the image must be
untouched, and since the destination is pre-filled with 0xA5 in the record and here, so must every byte inside the image that a
packer does not write.  The weights (tests/_weight_images.py) carry an all-zero row, a vanishing row, a row whose maximum is exactly
1.0, a row with +inf and a row near 2^20, behind a row pitch larger than K whose spare columns must not be read."""
import os

import numpy as np
import pytest
import torch

import _weight_images as wi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "weight_images.npz")))


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(name for name, _, _ in wi.CASES)


@pytest.mark.parametrize("name,stem,dims", wi.CASES, ids=[c[0] for c in wi.CASES])
def test_weight_image_matches_record(lib, golden, name, stem, dims):
    image, guard = wi.pack_image(lib, stem, dims)
    assert guard.size == wi.GUARD and (guard == wi.FILL).all(), f"{name}: bytes behind the image were written"
    crc, want = wi.crc_blocks(image), golden[name]
    assert crc.shape == want.shape, f"{name}: {image.size} bytes make {crc.size} blocks, the record has {want.size}"
    diff = np.flatnonzero(crc != want)
    assert diff.size == 0, f"{name}: {diff.size} of {crc.size} blocks differ, the first is block {int(diff[0])} (bytes from {int(diff[0]) * wi.BLOCK})"
