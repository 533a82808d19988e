#!/usr/bin/env python3
"""Developer tool: CU occupancy timeline of kernel 2g (field_cosetp_k) on the headline shard.
Build:  python openlifu-python_amd/build.py -DOLX_EXP_CUTRACE --out lib/libolx_CUTRACE.so ; on the GPU box:
  OLX_LIB_PATH=openlifu-python_amd/lib/libolx_CUTRACE.so python tools/cutrace_cosetp.py [fp8]
Per block and wave the kernel records HW_ID, XCC_ID and the shader cycle at entry, at its last store issued and acknowledged; this
script groups the blocks of the LAST launch by CU and reports how many blocks are resident over time and how long a freed slot idles."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "openlifu-python_amd"))
import bench  # noqa: E402
import openlifu_amd as ol  # noqa: E402
from openlifu_amd import _native as nat, dist as od  # noqa: E402
from openlifu_amd.engine import grid_from_coords  # noqa: E402

fp8 = "fp8" in sys.argv[1:]
arr, setup, target, pattern = bench.synthetic_workload(256, 0.25)
sweep = np.array([f.get_position(units="m") for f in pattern.get_targets(target)])
shard = od.plan_foci_orbits(sweep, 8, centre_xy=(0.0, 0.0))[0]
eng = ol.get_engine(0); ctx = eng.ctx; eng.bind(arr)
ctx.bf_solve(sweep[shard], 1500.0)
origin, spacing, n = grid_from_coords(setup.get_coords())
ctx.field_plan(origin, spacing, n, 400e3, 1500.0, 1000.0, 1e5, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | (0 if fp8 else nat.FIELD_FP16_CORRECTION))
for _ in range(20):
    ctx.field_launch()
ctx.sync()
print(ctx.field_variant())
lib = nat.load()
buf = np.zeros((16384, 8, 5), dtype=np.uint64)
lib.olx_exp_read_cutrace_cosetp.argtypes = [ctypes.c_void_p]
assert lib.olx_exp_read_cutrace_cosetp(buf.ctypes.data) == 0
used = buf[:, 0, 2] > 0
b = buf[used].astype(np.int64)
nb = b.shape[0]
hw, xcc = b[:, 0, 0], b[:, 0, 1] & 0xF
cu = (hw >> 8) & 0xF; sh = (hw >> 12) & 1; se = (hw >> 13) & 0x7
key = ((xcc * 8 + se) * 2 + sh) * 16 + cu
t_in = b[:, :, 2].min(axis=1); t_issue = b[:, :, 3].max(axis=1); t_ack = b[:, :, 4].max(axis=1)
t_in_last = b[:, :, 2].max(axis=1)
print(f"{nb} blocks on {len(np.unique(key))} CUs; per block (cycles, median / p10 / p90):")
def q(x): return f"{np.median(x):9.0f} {np.percentile(x, 10):9.0f} {np.percentile(x, 90):9.0f}"
print("  first wave in -> last wave in        ", q(t_in_last - t_in))
print("  first wave in -> last store issued   ", q(t_issue - t_in))
print("  last store issued -> acknowledged    ", q(t_ack - t_issue))
print("  per-wave issue -> ack                ", q((b[:, :, 4] - b[:, :, 3]).ravel()))
print("  spread of the waves' ack times       ", q(b[:, :, 4].max(axis=1) - b[:, :, 4].min(axis=1)))
# per CU: two slots; a block starts when a slot frees -> gap = start of k-th block - k-2-th smallest end so far
gaps, spans, busy = [], [], []
for k in np.unique(key):
    m = key == k
    s0 = np.sort(t_in[m]); e0 = np.sort(t_ack[m])
    order = np.argsort(t_in[m]); st = t_in[m][order]; en = t_ack[m][order]
    span = en.max() - st.min(); spans.append(span)
    busy.append((en - st).sum() / (2.0 * span))
    # slot model: each new block (from the third on) takes the slot freed by the earliest-ending resident block
    import heapq
    h = []
    for a, e in zip(st, en):
        if len(h) == 2:
            free = heapq.heappop(h); gaps.append(a - free)
        heapq.heappush(h, e)
gaps = np.array(gaps)
print(f"per CU: span {np.median(spans):.0f} cycles, blocks {nb / len(np.unique(key)):.1f}, slot occupancy (2 slots) {np.median(busy):.3f}")
print("  slot freed (last ack of the leaving block) -> next block's first wave in:", q(gaps), f" mean {gaps.mean():.0f}")
print(f"  span over the CUs (first wave in -> last ack; the launch ends with the slowest CU): median {np.median(spans):.0f}, p90 {np.percentile(spans, 90):.0f}, max {np.max(spans):.0f} cycles"
      f" = {np.max(spans) / np.median(spans):.4f} of the median")
# the tail: how long a CU's last block runs alone (the other slot already empty for good)
alone = []
for k in np.unique(key):
    m = key == k
    e = np.sort(t_ack[m])
    alone.append(e[-1] - e[-2])
print(f"  a CU's last block outlives its second-last by (cycles, median / p10 / p90): {q(np.array(alone))}; size of the last block started per CU (tiles of wave 0):",
      np.bincount([int(((b[np.where(key == k)[0][np.argmax(t_in[key == k])], 0, 1]) >> 8) & 0xFF) for k in np.unique(key)], minlength=6).tolist())
print(f"  sum of gaps per slot {gaps.sum() / (2 * len(np.unique(key))):.0f} cycles = {gaps.sum() / (2 * len(np.unique(key))) / np.median(spans):.3f} of the span")
# ---- where the waves of a block sit: HW_ID's SIMD field per (block, wave), and the tiles each SIMD of a CU carries over the launch
simd = (b[:, :, 0] >> 4) & 3
ntile = (b[:, :, 1] >> 8) & 0xFF
print("wave -> SIMD (HW_ID bits 5:4):")
print("  SIMD of wave 0 over the blocks:", np.bincount(simd[:, 0], minlength=4).tolist())
rel = (simd - simd[:, :1]) & 3
pats, cnts = np.unique(rel, axis=0, return_counts=True)
for pat, cnt in sorted(zip(pats.tolist(), cnts.tolist()), key=lambda t: -t[1])[:6]:
    print(f"  SIMD of waves 0 .. 7 relative to wave 0's: {pat} on {cnt} blocks")
print("  blocks per SIMD count of a block (4 = two waves on each):", np.bincount([len(set(r)) for r in simd.tolist()], minlength=5).tolist())
per = np.zeros((len(np.unique(key)), 4))
for ci, k in enumerate(np.unique(key)):
    m = key == k
    per[ci] = np.bincount(simd[m].ravel(), weights=ntile[m].ravel().astype(float), minlength=4)
tot = per.sum(axis=0)
print("  tiles per SIMD over the launch (all CUs):", tot.astype(int).tolist(), " vs mean:", np.round(tot / tot.mean() - 1, 4).tolist())
srt = np.sort(per, axis=1)[:, ::-1]
print("  per CU, SIMDs sorted by load: mean tiles", np.round(srt.mean(axis=0), 1).tolist(), " busiest / mean of the CU:", f"{(srt[:, 0] / per.mean(axis=1)).mean():.4f}",
      f"(p10 {np.percentile(srt[:, 0] / per.mean(axis=1), 10):.4f}, p90 {np.percentile(srt[:, 0] / per.mean(axis=1), 90):.4f})")
five = (ntile == 5)
if five.any():
    print("  SIMD of the five-tile waves:", np.bincount(simd[five], minlength=4).tolist())
# the two blocks resident on a CU at a time: for each block the block of the same CU that started last before it -- do their most loaded SIMDs coincide?
heavy = np.array([np.bincount(simd[i], weights=ntile[i].astype(float), minlength=4).argmax() for i in range(nb)])
uneven = np.array([np.ptp(np.bincount(simd[i], weights=ntile[i].astype(float), minlength=4)) > 0 for i in range(nb)])
same = tot_pairs = 0
for k in np.unique(key):
    m = np.where((key == k) & uneven)[0]
    o = m[np.argsort(t_in[m])]
    same += int((heavy[o[1:]] == heavy[o[:-1]]).sum()); tot_pairs += len(o) - 1
print(f"  blocks that follow each other on a CU (uneven ones): most loaded SIMD the same in {same} of {tot_pairs} pairs ({same / max(tot_pairs, 1):.3f}; 0.25 = by chance)")
if "--dump" in sys.argv[1:]:
    k = np.unique(key)[3]
    m = np.where(key == k)[0]
    order = m[np.argsort(t_in[m])]
    t0 = t_in[order[0]]
    print("one CU: block id, first wave in, last wave in, first/last store-issue over waves, first/last ack over waves, npos-ish (lifetime)")
    for bi in order:
        w = b[bi]
        print(f"  {np.where(used)[0][bi]:6d} in {w[:,2].min()-t0:8d} ..{w[:,2].max()-t0:8d}  issue {w[:,3].min()-t0:8d} ..{w[:,3].max()-t0:8d}  ack {w[:,4].min()-t0:8d} ..{w[:,4].max()-t0:8d}   simd/wave-slots {sorted(set(((w[:,0]>>4)&3).tolist()))}")
