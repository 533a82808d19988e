#!/usr/bin/env python3
"""Static instruction counts of the K-step region of one kernel-2g instantiation in a hipcc -S --cuda-device-only listing.
   tools/isa_kstep.py file.s KERNEL_SUBSTRING [--list]
The region is everything from the first to the last matrix instruction of the kernel (only the K-steps issue any).  A tile-step (one tile
in one (sl, kb) group) is eight ds_read_b64 (four in the fp16 / DIR body) and its matrix instructions; whatever other vector instruction stands in the region takes an
issue slot from the matrix instructions of the other waves of the SIMD: DESIGN.md section 5.5.  --list prints the region's non-matrix
vector instructions one by one.  "per tile-step": the region cut behind the last matrix instruction of every tile-step, non-matrix vector instructions of each
piece in listing order -- guards, address arithmetic and whatever the compiler laid out between two tile-steps (the late steering request of the fp8 shape sits
on the path of a padding super-block: one piece with ~30).  Sibling of tools/isa_count.py (per basic block, whole kernel)."""
import re, sys
src, key = sys.argv[1], sys.argv[2]
lines = open(src).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\S*:', l) and key in l)
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith('s_endpgm'))
ins = [(i, l.strip()) for i, l in enumerate(lines[start + 1:end + 1]) if l.strip() and l.strip()[0] not in ';.' and not re.match(r'^\S+:', l)]
mf = [k for k, (_, s) in enumerate(ins) if s.startswith('v_mfma')]
region = [s for _, s in ins[mf[0]:mf[-1] + 1]]
keys = ('v_mov_b32', 'v_add_lshl_u32', 'v_add_u32', 'v_cndmask_b32', 'v_cmp_', 'ds_read_b64', 'v_mfma')
c = {k: sum(1 for s in region if s.startswith(k)) for k in keys}
other = [s for s in region if s.startswith('v_') and not s.startswith('v_mfma')]
c['other vector (all non-matrix v_*)'] = len(other)
c['s_cbranch'] = sum(1 for s in region if s.startswith('s_cbranch'))
per, n = [], 0
for k, s_ in enumerate(region):
    is_m = s_.startswith('v_mfma')
    if k and region[k - 1].startswith('v_mfma') and not is_m:      # a matrix run ends: a new tile-step begins here if fragment reads come before the next matrix instruction
        nxt = next((r for r in region[k:] if r.startswith(('v_mfma', 'ds_read_b64'))), '')
        if nxt.startswith('ds_read_b64'): per.append(n); n = 0
    if s_.startswith('v_') and not is_m: n += 1
per.append(n)
print(lines[start].split(':')[0])
print('K-step region: %d instructions' % len(region))
for k, v in c.items(): print('  %-36s %d' % (k, v))
print('  per tile-step (non-matrix vector)   ', ' '.join(map(str, per)))
if '--list' in sys.argv:
    for s in other: print('   ', s)
