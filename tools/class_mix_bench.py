#!/usr/bin/env python
"""What ClassMix costs on the device: the three launches of ops.class_mix, the apply kernel of csrc/class_mix.hip alone with its
bytes and bandwidth, the same composition from torch operators, and ops.augment_apply for the same batch.

    python tools/class_mix_bench.py [--batches 4 8] [--iters 20000] [--out profiles/class_mix_bench.txt]

  mix      hipEvent time of ops.class_mix (label_stats, select, apply; it allocates its six outputs) on one augmented batch of
           synthetic crops, crop 512, every sample mixed (prob = 1)
  apply    segmif_class_mix_apply_f32 alone into preallocated outputs; its bytes are counted from the mask (per group of 4
           pixels: the donor's labels, one or two loads per plane, the receiver's labels unless the whole group is pasted, and
           the stores) and divided by the time; the timed calls reuse the same buffers, which fit the Infinity Cache, so the
           rate is a cache-warm one
  torch    the same mix from torch operators on the device (a gather of the selection words, then torch.where per tensor), after
           its result was compared bit for bit with the kernel's
  augment  ops.augment_apply for the same records

The apply kernel's registers come from the compiler's resource usage (a compile of csrc/class_mix.hip; no device needed).
The crops are synthetic: the numbers say what the pass costs, nothing about what mixing does to a data set.
"""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, CROP, N_CLASS, RESIDENT = 480, 640, 512, 9, 32


def timed(fn, n, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def torch_mix(ir3, vis3, mask3, label, donor, sel):
    """the rule from torch operators: -> (ir3', vis3', mask3', label', M)"""
    B = label.shape[0]
    don = label.index_select(0, donor)
    idx = don.clamp(0, 255)
    words = sel.gather(1, (idx >> 5).view(B, -1)).view_as(idx)
    M = (don >= 0) & (don < N_CLASS) & (((words >> (idx & 31).int()) & 1) != 0) & (donor != torch.arange(B, device=donor.device))[:, None, None]
    out = [torch.where(M[:, None], t.index_select(0, donor), t) for t in (ir3, vis3, mask3)]
    return out + [torch.where(M, don, label), M]


def apply_registers():
    """VGPRs / SGPRs / scratch / occupancy of class_mix_apply_kernel from -Rpass-analysis=kernel-resource-usage"""
    from segmif_amd import build
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "class_mix.hip"),
                                            "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return "registers: NOT recorded (the compile failed)"
    block = r.stderr.split("class_mix_apply_kernel", 1)[-1]
    field = lambda name: (re.search(name + r": (\d+)", block) or [None, "?"])[1]
    scratch, occ, lds = field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"), field(r"LDS Size \[bytes/block\]")
    return (f"registers: class_mix_apply_kernel {field('VGPRs')} VGPRs, {field('TotalSGPRs')} SGPRs, scratch {scratch} bytes/lane, "
            f"occupancy {occ} waves/SIMD, LDS {lds} bytes (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--iters", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_mix_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("class_mix_bench measures on the MI355X: no device, no numbers")
    from segmif_amd import _lib, data, ops
    lines = [f"# tools/class_mix_bench.py: synthetic crops of {RESIDENT} resident {H} x {W} frames, crop {CROP}, {N_CLASS} classes, prob 1, "
             f"{torch.cuda.get_device_name(0)}; device events, {a.iters} calls a figure, warm", "#"]
    ds = data.DeviceDataset.from_arrays(**data.synthetic_pairs(RESIDENT, H, W, seed=0))
    lib, stream = _lib.load(), lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B in a.batches:
        it = data.AugmentedBatches(ds, batch=B, crop_size=CROP, seed=1)
        params = it.draw(B)
        rec, tab = data.pack_records(list(range(B)), params, H, W)
        rec_d, tab_d = torch.from_numpy(rec).cuda(), torch.from_numpy(tab).cuda()
        ops.augment_pick(ds.label, rec_d, tab_d, CROP, CROP)
        ir3, vis3, mask3, label = ops.augment_apply(ds.ir, ds.vis, ds.mask, ds.label, rec_d, tab_d, CROP, CROP)
        table_h = data.ClassMix(prob=1.0, n_class=N_CLASS, seed=B).draw(B)
        table = torch.from_numpy(table_h).cuda()
        donor = table[:, 0].long()
        got = ops.class_mix(ir3, vis3, mask3, label, table, N_CLASS)
        sel, pasted = got[4], got[5]
        ref = torch_mix(ir3, vis3, mask3, label, donor, sel)
        for x, y in zip(got[:4], ref[:4]):
            same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.is_floating_point() else torch.equal(x, y)
            if not same:
                raise RuntimeError("ops.class_mix and the torch composition disagree")
        M = ref[4]
        if not torch.equal(M.view(B, -1).sum(1), pasted):
            raise RuntimeError("pasted is not the mask's popcount")
        per_group = M.view(B, -1, 4).sum(-1)
        groups, full, none = per_group.numel(), int((per_group == 4).sum()), int((per_group == 0).sum())
        split = groups - full - none
        nbytes = groups * (32 + 9 * 16 + 9 * 16 + 32) + split * 9 * 16 + (groups - full) * 32
        out = [torch.empty_like(t) for t in (ir3, vis3, mask3, label)]
        apply_only = lambda: lib.segmif_class_mix_apply_f32(ir3.data_ptr(), vis3.data_ptr(), mask3.data_ptr(), label.data_ptr(), table.data_ptr(),
                                                            sel.data_ptr(), B, CROP, CROP, N_CLASS, *(t.data_ptr() for t in out), stream())
        ms_mix = timed(lambda: ops.class_mix(ir3, vis3, mask3, label, table, N_CLASS), a.iters)
        ms_apply = timed(apply_only, a.iters)
        ms_torch = timed(lambda: torch_mix(ir3, vis3, mask3, label, donor, sel), max(20, a.iters // 10))
        ms_aug = timed(lambda: ops.augment_apply(ds.ir, ds.vis, ds.mask, ds.label, rec_d, tab_d, CROP, CROP), a.iters)
        px = B * CROP * CROP
        lines.append(f"B = {B}: {int(pasted.sum())} of {px} pixels pasted ({float(pasted.sum()) / px:.3f}); groups of 4: {none} kept, {full} pasted, "
                     f"{split} split")
        lines.append(f"  mix:     ops.class_mix, three launches and six allocations         {ms_mix:8.4f} ms")
        lines.append(f"  apply:   segmif_class_mix_apply_f32 alone, {nbytes / 1e6:6.1f} MB ({nbytes / px:.1f} B/pixel)  {ms_apply:8.4f} ms   {nbytes / 1e6 / ms_apply:7.1f} GB/s")
        lines.append(f"  torch:   gather of the selection + torch.where per tensor (equal bits)  {ms_torch:8.4f} ms")
        lines.append(f"  augment: ops.augment_apply for the same records                    {ms_aug:8.4f} ms")
    lines.append("note: a batch and its copy (92 MB at B = 4, 184 MB at B = 8) fit the 256 MB Infinity Cache and every call of a figure reads and "
                 "writes the same buffers, so the GB/s are cache-warm rates of the bytes the kernel moves, not HBM bandwidth")
    lines.append(apply_registers())
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
